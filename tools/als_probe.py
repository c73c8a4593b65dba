"""Times the alternating-least-squares half-steps (cu2rec_model_als) on the synthetic ML-20M and Netflix shapes and prints each time
next to its Gram roofline.

    python tools/als_probe.py [--shapes ml-20m,netflix] [--factors 100] [--reps 3] [--cg-steps N] [--implicit [--alpha 40]]

For every shape: the item half-step's first call on a fresh cu2rec_csr (it builds the item-major view), the item half-step again
(view cached), the user half-step, and a whole sweep (users then items).  Times are wall clock around the synchronous call (the
call returns after a device-to-host read of its unsolved count), best of --reps.  Roofline: the Gram of a half-step is
2 nnz (f + 2)^2 flop when formed whole; its lower triangle half that; at 155 TF/s (fp32 MFMA peak of the MI355X) -- the partner-row
gather (nnz x 4 (f + 1) bytes) and the per-row Cholesky (about rows x (f + 1)^3 / 3 flop) come on top.

--implicit: after the explicit rows, the implicit-feedback half-steps and sweep (cu2rec_model_als_implicit) in the same process, on
the same cu2rec_csr and a model of their own, with the ratio implicit / explicit of the sweeps.  An implicit half-step does the
same per-entry work, solves EVERY row (rows without entries are written as zeros) and forms the partner side's global Gram first
(rows x f^2 multiply-adds over both half-steps of a sweep: users + items rows).

--cg-steps N (with --implicit): after the implicit rows, the same half-steps and sweep by N conjugate-gradient steps per row
(cu2rec_model_als_implicit_cg) on a model of their own, each with its ratio to the implicit Cholesky time above it.  Per row of n
entries CG does (N + 1) x (f^2 + 2 n f) multiply-adds -- one operator application for the starting residual, one per step --
against n f^2 / 2 for the Gram's lower triangle plus f^3 / 3 for Cholesky.

--cg-steps N without --implicit: after the explicit rows, the explicit half-steps and sweep by N conjugate-gradient steps per row
(cu2rec_model_als_cg) on a model of their own, each with its ratio to the explicit Cholesky time above it, and the rows of each side
that CG takes (1 .. 1,024 ratings) against those solved exactly.  Per row of n ratings explicit CG does (N + 1) x 2 n (f + 1)
multiply-adds against n F^2 / 2 + (f + 1)^3 / 3, F = f + 2 rounded up to 32 (the Gram's MFMA tiles)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import cu2rec_amd as cu  # noqa: E402
from cu2rec_amd import synth  # noqa: E402

PEAK = 155e12
HYPER = (0.01, 0.05, 0.05, 0.02, 0.02)


def best(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml-20m,netflix")
    ap.add_argument("--factors", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--implicit", action="store_true")
    ap.add_argument("--alpha", type=float, default=40.0)
    ap.add_argument("--cg-steps", type=int, default=0)
    args = ap.parse_args()
    f = args.factors
    for name in args.shapes.split(","):
        tr, _ = synth.make_named(name)
        d = cu.DeviceCSR(tr)
        m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
        gram = 2.0 * tr.nnz * (f + 2) ** 2
        roof_full, roof_lower = gram / PEAK * 1e3, gram / 2 / PEAK * 1e3
        gather_gb = tr.nnz * 4.0 * (f + 1) / 1e9
        users = int((np.diff(tr.indptr) > 0).sum())
        items = int((np.bincount(tr.indices, minlength=tr.cols) > 0).sum())
        print("%s: %d users, %d items, %d ratings, f = %d; Gram %.2e flop per half-step -> roofline %.2f ms whole, %.2f ms lower "
              "triangle; gather %.1f GB; Cholesky ~%.1e flop (users), ~%.1e (items)"
              % (name, tr.rows, tr.cols, tr.nnz, f, gram, roof_full, roof_lower, gather_gb, users * (f + 1) ** 3 / 3.0,
                 items * (f + 1) ** 3 / 3.0), flush=True)
        t0 = time.perf_counter()
        assert m.als(d, HYPER, "items") == 0  # first item half-step: builds the item-major view
        first = time.perf_counter() - t0
        rows = [("items, first call (builds the view)", first)]
        rows.append(("items", best(lambda: m.als(d, HYPER, "items"), args.reps)))
        rows.append(("users", best(lambda: m.als(d, HYPER, "users"), args.reps)))
        rows.append(("sweep (users + items)", best(lambda: m.als(d, HYPER, "both"), args.reps)))
        for label, t in rows:
            roof = 2 * roof_lower if label.startswith("sweep") else roof_lower
            print("  %-38s %9.2f ms   (lower-triangle Gram roofline %.2f ms: %.1fx)" % (label, 1e3 * t, roof, 1e3 * t / roof),
                  flush=True)
        m.close()
        if args.cg_steps > 0 and not args.implicit:
            exact = [t for _, t in rows[1:]]  # items, users, sweep
            kw = dict(solver="cg", cg_steps=args.cg_steps)
            m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
            assert m.als(d, HYPER, "both", **kw) == 0  # warm: the kernels' first launches
            rows = [("CG-%d items" % args.cg_steps, best(lambda: m.als(d, HYPER, "items", **kw), args.reps)),
                    ("CG-%d users" % args.cg_steps, best(lambda: m.als(d, HYPER, "users", **kw), args.reps)),
                    ("CG-%d sweep (users + items)" % args.cg_steps, best(lambda: m.als(d, HYPER, "both", **kw), args.reps))]
            for (label, t), t_exact in zip(rows, exact):
                print("  %-38s %9.2f ms   (%.2f x the Cholesky time)" % (label, 1e3 * t, t / t_exact), flush=True)
            n_users, n_items = np.diff(tr.indptr), np.bincount(tr.indices, minlength=tr.cols)
            for side, n in (("users", n_users), ("items", n_items)):
                short = n[(n > 0) & (n <= cu.api.ALS_CHUNK)].astype(np.float64)
                long_n = n[n > cu.api.ALS_CHUNK].astype(np.float64)
                cg = (args.cg_steps + 1) * 2.0 * short.sum() * (f + 1)
                F = -(-(f + 2) // 32) * 32  # the Gram's staged columns: f + 2 rounded up to whole 32-column MFMA tiles
                chol = short.sum() * F ** 2 / 2.0 + len(short) * (f + 1) ** 3 / 3.0
                print("  rows of 1 .. %d ratings, %s: %d with %d ratings (%d longer ones with %d ratings solved exactly); CG %.2e "
                      "multiply-adds, Gram + Cholesky %.2e" % (cu.api.ALS_CHUNK, side, len(short), int(short.sum()), len(long_n),
                                                               int(long_n.sum()), cg, chol), flush=True)
            m.close()
        if args.implicit:
            explicit_sweep = rows[-1][1]
            m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
            assert m.ials(d, HYPER, args.alpha, "both") == 0  # warm: both sides' plans exist already
            rows = [("implicit items", best(lambda: m.ials(d, HYPER, args.alpha, "items"), args.reps)),
                    ("implicit users", best(lambda: m.ials(d, HYPER, args.alpha, "users"), args.reps)),
                    ("implicit sweep (users + items)", best(lambda: m.ials(d, HYPER, args.alpha, "both"), args.reps))]
            for label, t in rows:
                print("  %-38s %9.2f ms" % (label, 1e3 * t), flush=True)
            print("  implicit / explicit sweep: %.2f   (global Grams: (%d + %d) rows x f^2 = %.2e multiply-adds per sweep)"
                  % (rows[-1][1] / explicit_sweep, tr.rows, tr.cols, (tr.rows + tr.cols) * float(f) ** 2), flush=True)
            m.close()
            if args.cg_steps > 0:
                exact = [t for _, t in rows]
                kw = dict(solver="cg", cg_steps=args.cg_steps)
                m = cu.Model(tr.rows, tr.cols, f, tr.global_bias)
                assert m.ials(d, HYPER, args.alpha, "both", **kw) == 0
                rows = [("implicit CG-%d items" % args.cg_steps, best(lambda: m.ials(d, HYPER, args.alpha, "items", **kw), args.reps)),
                        ("implicit CG-%d users" % args.cg_steps, best(lambda: m.ials(d, HYPER, args.alpha, "users", **kw), args.reps)),
                        ("implicit CG-%d sweep (users + items)" % args.cg_steps,
                         best(lambda: m.ials(d, HYPER, args.alpha, "both", **kw), args.reps))]
                for (label, t), t_exact in zip(rows, exact):
                    print("  %-38s %9.2f ms   (%.2f x the implicit Cholesky time)" % (label, 1e3 * t, t / t_exact), flush=True)
                n_users, n_items = np.diff(tr.indptr), np.bincount(tr.indices, minlength=tr.cols)
                for side, n in (("users", n_users), ("items", n_items)):
                    short = n[(n > 0) & (n <= cu.api.ALS_CHUNK)].astype(np.float64)
                    cg = (args.cg_steps + 1) * (len(short) * float(f) ** 2 + 2.0 * short.sum() * f)
                    chol = short.sum() * f ** 2 / 2.0 + len(short) * f ** 3 / 3.0
                    print("  rows of 1 .. %d entries, %s: %d (%d longer ones solved exactly); CG %.2e multiply-adds, Gram + Cholesky %.2e"
                          % (cu.api.ALS_CHUNK, side, len(short), int((n > cu.api.ALS_CHUNK).sum()), cg, chol), flush=True)
                m.close()
        d.close()


if __name__ == "__main__":
    main()
