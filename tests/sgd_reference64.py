"""TEST INFRASTRUCTURE: the sequential SGD update (mf_sequential.cu:102-143) restated in float64 with numpy, separate from the C
oracle, driven by the product's sample stream (cu2rec_sampler_index).

Every update reads the old p / q on the right-hand side, then moves the two biases:
    err = r - (((global_bias + ub) + ib) + p . q)
    p  <- p  + lr (err q - P_reg p)          q  <- q  + lr (err p_old - Q_reg q)
    ub <- ub + lr (err - user_bias_reg ub)   ib <- ib + lr (err - item_bias_reg ib)
The hyper-parameters are the float32 values the kernels and the oracle see, widened to float64.

Beside the float64 trajectory the walk carries a running bound B (one per parameter) on how far a float32 evaluation of the same
updates -- the oracle's, any kernel's, with the dot product summed in any order and no fused multiply-add -- can be from it.  Only
float32 rounding enters it (unit roundoff u = 2^-24, gamma_n = n u / (1 - n u)); its propagation uses magnitudes widened by the bound
itself, so it is an upper bound and not a first-order estimate:
  * err:    |d err| <= B_ub + B_ib + sum_k (|q_k| + B_qk) B_pk + (|p_k| + B_pk) B_qk
                       + gamma_(f+4) (|r| + |global_bias| + |ub| + |ib| + sum_k |p_k q_k|)     (f products, f - 1 + 4 additions)
  * p_k:    B' = |1 - lr P_reg| B_pk + lr |err| B_qk + lr |q_k| |d err| + gamma_4 (|p_k| + lr (|err q_k| + P_reg |p_k|))
  * q_k:    the same with p and q exchanged and Q_reg;
  * biases: B' = |1 - lr reg| B + lr |d err| + gamma_4 (|b| + lr (|err| + reg |b|))
(with |err|, |p_k|, |q_k|, |b| each widened by its own bound).  The float64 arithmetic of the walk itself is ~1e-16 relative and
is not counted."""
import numpy as np

from cu2rec_amd import api

U32 = 2.0 ** -24


def gamma(n):
    return n * U32 / (1.0 - n * U32)


class State64:
    """float64 P, Q, user_bias, item_bias and their bounds (all zero: the start is the float32 state itself, exactly)."""

    def __init__(self, P, Q, ub, ib):
        self.P, self.Q = np.array(P, np.float64), np.array(Q, np.float64)
        self.ub, self.ib = np.array(ub, np.float64), np.array(ib, np.float64)
        self.BP, self.BQ = np.zeros_like(self.P), np.zeros_like(self.Q)
        self.Bub, self.Bib = np.zeros_like(self.ub), np.zeros_like(self.ib)

    def arrays(self):
        return self.P, self.Q, self.ub, self.ib

    def bounds(self):
        return self.BP, self.BQ, self.Bub, self.Bib


def sgd64(csr, st, global_bias, hyper, seed, iter0, n_iters, update_items=True, bound=True):
    """n_iters sequential iterations from iter0, in place on the State64 `st`; csr has indptr / indices / data / rows.  bound=False:
    the trajectory only (on long chains the worst-case bound grows geometrically and says nothing)."""
    lr, p_reg, q_reg, ub_reg, ib_reg = (float(np.float32(h)) for h in hyper)
    gb = float(np.float32(global_bias))
    f = st.P.shape[1]
    g_err, g4 = gamma(f + 4), gamma(4)
    indptr, indices, data = csr.indptr, csr.indices, csr.data
    for it in range(iter0, iter0 + n_iters):
        for x in range(csr.rows):
            lo, hi = int(indptr[x]), int(indptr[x + 1])
            if lo == hi:
                continue
            k = api.sampler_index(seed, x, it, lo, hi)
            y, r = int(indices[k]), float(data[k])
            p, q, ub, ib = st.P[x].copy(), st.Q[y].copy(), st.ub[x], st.ib[y]
            bp, bq, bub, bib = st.BP[x].copy(), st.BQ[y].copy(), st.Bub[x], st.Bib[y]
            pq = p * q
            err = r - (((gb + ub) + ib) + float(pq.sum()))
            ap, aq = np.abs(p) + bp, np.abs(q) + bq
            d_err = (bub + bib + float((aq * bp + ap * bq).sum())
                     + g_err * (abs(r) + abs(gb) + abs(ub) + abs(ib) + float(np.abs(pq).sum())))
            ae = abs(err) + d_err
            st.P[x] = p + lr * (err * q - p_reg * p)
            st.ub[x] = ub + lr * (err - ub_reg * ub)
            if update_items:
                st.Q[y] = q + lr * (err * p - q_reg * q)
                st.ib[y] = ib + lr * (err - ib_reg * ib)
            if not bound:
                continue
            st.BP[x] = abs(1.0 - lr * p_reg) * bp + lr * ae * bq + lr * aq * d_err + g4 * (ap + lr * (ae * aq + p_reg * ap))
            st.Bub[x] = abs(1.0 - lr * ub_reg) * bub + lr * d_err + g4 * (abs(ub) + bub + lr * (ae + ub_reg * (abs(ub) + bub)))
            if update_items:
                st.BQ[y] = abs(1.0 - lr * q_reg) * bq + lr * ae * bp + lr * ap * d_err + g4 * (aq + lr * (ae * ap + q_reg * aq))
                st.Bib[y] = abs(1.0 - lr * ib_reg) * bib + lr * d_err + g4 * (abs(ib) + bib + lr * (ae + ib_reg * (abs(ib) + bib)))
    return st


def excess(arrays32, st):
    """max over all parameters of |float32 value - float64 value| / bound (<= 1: inside the bound), and the largest distance."""
    worst, dist = 0.0, 0.0
    for a, w, b in zip(arrays32, st.arrays(), st.bounds()):
        d = np.abs(np.asarray(a, np.float64) - w)
        dist = max(dist, float(d.max()))
        worst = max(worst, float((d / np.maximum(b, 1e-300)).max()))
    return worst, dist


def distance(arrays32, st):
    """max |float32 value - float64 value| over all parameters."""
    return max(float(np.abs(np.asarray(a, np.float64) - w).max()) for a, w in zip(arrays32, st.arrays()))
