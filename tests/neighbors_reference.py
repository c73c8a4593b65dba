"""Host restatements for the neighbour queries (cu2rec_model_similar / cu2rec_model_top_users): the top-k selection in
cu2rec_model_topk's key order over given float32 scores, and float64 cosine / dot scores of factor rows."""
import numpy as np


def radix_code(scores):
    """rocPRIM's radix code of float32 scores (descending sort's order; +0.0 and -0.0 one code) as uint32."""
    b = np.ascontiguousarray(scores, np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return b ^ np.where(b & 0x80000000, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


NEG_INF_CODE = 0x007FFFFF  # radix code of -inf: a score at or below it is never listed


def select(scores, allowed, k):
    """The k best allowed entries of one row of float32 scores -> (ids, scores), topk's order: descending radix code, equal
    codes by ascending id, -inf never listed, -1 / NaN padding."""
    scores = np.asarray(scores, np.float32)
    code = radix_code(scores).astype(np.int64)
    ids = np.nonzero(np.asarray(allowed, bool) & (code > NEG_INF_CODE))[0]
    order = ids[np.lexsort((ids, -code[ids]))][:k]
    out_i = np.full(k, -1, np.int32)
    out_s = np.full(k, np.nan, np.float32)
    out_i[:len(order)] = order
    out_s[:len(order)] = scores[order]
    return out_i, out_s


def excluded_sets(csr, rows):
    """row -> set of excluded ids of a HostCSR (rows past its last row: empty)"""
    out = [set() for _ in range(rows)]
    for r in range(min(csr.rows, rows)):
        out[r].update(csr.indices[csr.indptr[r]:csr.indptr[r + 1]].tolist())
    return out


def cosine64(X, rows=None):
    """float64 cosine of rows `rows` (default all) of X against every row; zero rows have cosine 0 with everything."""
    X = np.asarray(X, np.float64)
    norm = np.sqrt((X * X).sum(axis=1))
    inv = np.divide(1.0, norm, out=np.zeros_like(norm), where=norm > 0)
    rows = np.arange(len(X)) if rows is None else np.asarray(rows)
    return (X[rows] @ X.T) * inv[rows][:, None] * inv[None, :]
