"""Times ItemKNN (cu2rec_knn_*) on the synthetic ML-20M shape: create, neighbors and recommend.

    python tools/knn_probe.py [--shapes ml-20m] [--weighting cosine] [--neighbours 20] [--k 10] [--users 4096] [--reps 3] [--out FILE]

Times are wall clock around the synchronous call, best of --reps after one warm-up call (the warm-up builds the row-sorted and
the item-major view, which the CSR keeps; every timed create repeats the weights, the product and the id-sorted copy).  Beside the
times, the work counts of the build: sum over users of n_u^2 accumulations (every stored pair of a row, both orders and the diagonal,
across all slices) and the bytes its wavefronts gather (8 bytes per accumulation: the partner row's id and weight), and the same for
the recommend call over the lists.  No time is a pass condition: there is no earlier ItemKNN here to compare with."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cu2rec_amd as cu  # noqa: E402
from cu2rec_amd import synth  # noqa: E402


def best(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml-20m")
    ap.add_argument("--weighting", default="cosine")
    ap.add_argument("--neighbours", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--users", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    s = cu.lib().cu2rec_knn_slice_items()
    for name in args.shapes.split(","):
        tr, _ = synth.make_named(name)
        d = cu.DeviceCSR(tr)
        n_u = np.diff(tr.indptr).astype(np.float64)
        m_i = np.bincount(tr.indices, minlength=tr.cols).astype(np.float64)
        slices = -(-tr.cols // s)
        say("%s: %d users, %d items, %d entries; weighting %s, N = %d, slices of %d items: %d per query" %
            (name, tr.rows, tr.cols, tr.nnz, args.weighting, args.neighbours, s, slices))
        say("  longest row %d entries, longest column %d users (one wavefront per (item, slice) walks its column in order: the tail)" %
            (int(n_u.max()), int(m_i.max())))
        knn = cu.ItemKNN(d, args.weighting, args.neighbours)  # warm-up
        knn.close()
        made = []

        def create():
            if made:
                made.pop().close()
            made.append(cu.ItemKNN(d, args.weighting, args.neighbours))

        t_create = best(create, args.reps)
        knn = made[0]
        acc = float((n_u * n_u).sum())
        say("  create                 %10.2f ms   %.4g accumulations (sum_u n_u^2), %.4g bytes gathered, %.4g binary searches" %
            (1e3 * t_create, acc, 8 * acc, 2.0 * tr.nnz * slices))
        t_weights = best(lambda: d.knn_weights(args.weighting), args.reps)
        say("  weights alone          %10.2f ms   (with the download of %d floats)" % (1e3 * t_weights, tr.nnz))
        t_all = best(lambda: knn.neighbors(), args.reps)
        say("  neighbors, every item  %10.2f ms   (a gather of %d x %d lists and their download)" % (1e3 * t_all, tr.cols, args.neighbours))
        users = np.arange(min(args.users, tr.rows), dtype=np.int32)
        ids, _ = knn.neighbors()
        listed = (ids >= 0).sum(axis=1).astype(np.float64)
        rec_acc = float(sum(listed[tr.indices[tr.indptr[u]:tr.indptr[u + 1]]].sum() for u in users))
        knn.recommend(d, d, args.k, users)  # warm-up
        t_rec = best(lambda: knn.recommend(d, d, args.k, users), args.reps)
        say("  recommend, %5d rows  %10.2f ms   k = %d, history = exclusion = the training rows; %.4g accumulations, %.4g bytes gathered" %
            (len(users), 1e3 * t_rec, args.k, rec_acc, 8 * rec_acc))
        t_rank = best(lambda: knn.rank_metrics(d, d, args.k, exclude=d), 1)
        say("  rank_metrics, all rows %10.2f ms   (one call, %d rows)" % (1e3 * t_rank, tr.rows))
        knn.close()
        d.close()
    say("NOT MEASURED: kernel times (no trace was taken: these are call times), the long columns' share of create, cache hit rates,")
    say("the once-per-CSR segmented sort and item-major view (inside the warm-up), other weightings, N, k or shapes.")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
