"""Times the pieces of a BPR sweep (cu2rec_model_bpr) on the synthetic ML-20M shape.

    python tools/bpr_probe.py [--shapes ml-20m] [--factors 100] [--reps 3]

For every shape, after one warm-up sweep (it builds the CSR's row-sorted and item-major views and the accumulators): the gradient calls
with the sweep's negatives and regrouping already cached on the CSR, the same calls on a fresh sweep -- the differences are the
negatives pass and the regrouping sort -- then the two half-steps, a whole sweep and the objective.  Times are wall clock around the
synchronous C call (the gradient calls with NULL outputs: nothing is copied to the host; a half-step returns after a device-to-host
read of its unchanged-row count), best of --reps.  Beside each time, the rows the pass gathers (two item rows per triple on the
user side and for the coefficients, two user rows per triple on the item side) as bytes per second."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cu2rec_amd as cu  # noqa: E402
from cu2rec_amd import api, synth  # noqa: E402
from cu2rec_amd._lib import lib  # noqa: E402

HYPER = (0.05, 0.01, 0.01, 0.0, 0.01)
SEED = 42


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml-20m")
    ap.add_argument("--factors", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    f = args.factors
    for name in args.shapes.split(","):
        tr, _ = synth.make_named(name)
        d = cu.DeviceCSR(tr)
        m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        h = cu.Hyper(*HYPER)
        row_bytes = 4.0 * f
        print("%s: %d users, %d items, %d entries, f = %d" % (name, tr.rows, tr.cols, tr.nnz, f), flush=True)
        assert m.bpr(d, HYPER, SEED, 0, "both") == 0  # warm-up
        sweep = [0]

        def gradient(side, fresh):
            if fresh:
                sweep[0] += 1
            t0 = time.perf_counter()
            api.check(lib().cu2rec_model_bpr_gradient(m._h, d._h, C.byref(h), SEED, sweep[0], side, None, None))
            return time.perf_counter() - t0

        def step(side, fresh):
            if fresh:
                sweep[0] += 1
            t0 = time.perf_counter()
            m.bpr(d, HYPER, SEED, sweep[0], side)
            return time.perf_counter() - t0

        def items_gradient_after_users():  # a fresh sweep whose negatives the users' call has cached: the regrouping is still to do
            gradient(0, True)
            return gradient(1, False)

        def items_step_after_users():
            step("users", True)
            return step("items", False)

        def both():
            return step("users", True) + step("items", False)

        def objective():
            t0 = time.perf_counter()
            m.bpr_objective(d, HYPER, SEED, sweep[0])
            return time.perf_counter() - t0

        best = lambda fn: min(fn() for _ in range(args.reps))
        users_fresh = best(lambda: gradient(0, True))
        users_cached = best(lambda: gradient(0, False))
        items_fresh = best(items_gradient_after_users)
        items_cached = best(lambda: gradient(1, False))
        gathered = 2.0 * tr.nnz * row_bytes
        rows = [("users gradient, cached", users_cached, gathered),
                ("negatives pass", users_fresh - users_cached, 0.0),
                ("items gradient, cached", items_cached, 2 * gathered),  # the coefficients' pass, then the items'
                ("regrouping sort", items_fresh - items_cached, 0.0),
                ("users half-step", best(lambda: step("users", True)), gathered),
                ("items half-step", best(items_step_after_users), 2 * gathered),
                ("sweep (users + items)", best(both), 3 * gathered),
                ("objective", best(objective), gathered)]
        for label, t, nbytes in rows:
            rate = "   %7.1f GB/s of gathered rows" % (nbytes / t / 1e9) if nbytes else ""
            print("  %-26s %9.2f ms%s" % (label, 1e3 * t, rate), flush=True)
        neg = d.bpr_negatives(SEED, sweep[0])
        print("  entries without a triple in the last sweep: %d of %d" % (int((neg < 0).sum()), tr.nnz), flush=True)
        m.close()
        d.close()


if __name__ == "__main__":
    main()
