"""Times the logistic-matrix-factorization half-steps (cu2rec_model_lmf) and objective on the synthetic ML-20M shape and prints each
time next to the all-pairs pass's flop count.

    python tools/lmf_probe.py [--shapes ml-20m] [--factors 100] [--reps 3] [--alpha 1]

For every shape: the user half-step, the item half-step, a whole sweep and the objective, after one warm-up sweep (it builds the
item-major view and the accumulators).  Times are wall clock around the synchronous call (a half-step returns after a
device-to-host read of its unchanged-row count), best of --reps.  The all-pairs pass of a half-step is 4 U I f flop (2 U I f for the
scores, 2 U I f for sigma(S) Y) whichever side moves; the objective's is the scores alone.  The yardstick is the fused top-k
selection's measured 30 TFLOP/s on the same walk, not the 155 TF/s fp32 MFMA peak."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cu2rec_amd as cu  # noqa: E402
from cu2rec_amd import synth  # noqa: E402

TOPK_TFLOPS = 30.0
HYPER = (0.05, 0.6, 0.6, 0.0, 0.0)


def best(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml-20m")
    ap.add_argument("--factors", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--alpha", type=float, default=1.0)
    args = ap.parse_args()
    f = args.factors
    for name in args.shapes.split(","):
        tr, _ = synth.make_named(name)
        d = cu.DeviceCSR(tr)
        m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        dense = 4.0 * tr.rows * tr.cols * f
        print("%s: %d users, %d items, %d entries, f = %d; all-pairs pass %.2e flop per half-step" % (name, tr.rows, tr.cols, tr.nnz, f, dense),
              flush=True)
        assert m.lmf(d, HYPER, args.alpha, "both") == 0  # warm-up: the item-major view, the accumulators, the kernels' first launches
        rows = [("users", dense, best(lambda: m.lmf(d, HYPER, args.alpha, "users"), args.reps)),
                ("items", dense, best(lambda: m.lmf(d, HYPER, args.alpha, "items"), args.reps)),
                ("sweep (users + items)", 2 * dense, best(lambda: m.lmf(d, HYPER, args.alpha, "both"), args.reps)),
                ("objective", dense / 2, best(lambda: m.lmf_objective(d, HYPER, args.alpha), args.reps))]
        for label, flop, t in rows:
            tf = flop / t / 1e12
            print("  %-24s %9.2f ms   %6.2f TFLOP/s on the all-pairs pass (%.2f of top-k's %.0f)" % (label, 1e3 * t, tf, tf / TOPK_TFLOPS,
                                                                                                  TOPK_TFLOPS), flush=True)
        m.close()
        d.close()


if __name__ == "__main__":
    main()
