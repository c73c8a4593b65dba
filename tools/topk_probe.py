"""Times cu2rec_model_topk against cu2rec_model_recommend at the ML-20M shape (GPU tool; run as one process under its own time limit).

    timeout -k 10 900 python tools/topk_probe.py [--out result.json]

138,493 users x 26,744 items, f = 100, k = 10, excluding a synthetic training set with ML-20M's 20,000,263 ratings.  Both calls
are timed end to end through the C ABI (each returns after its last device-to-host copy: the device is synchronised), after one
warm-up call each; the median of the repeats is reported with the outputs' equality (items and the raw bits of the scores) and
the fused path's achieved TFLOP/s (2 U I f / time) against the 157 TFLOP/s f32 MFMA peak of an MI355X.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cu2rec_amd as cu  # noqa: E402
from cu2rec_amd import synth  # noqa: E402

PEAK_F32_MFMA = 157e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=138_493)
    ap.add_argument("--items", type=int, default=26_744)
    ap.add_argument("--nnz", type=int, default=20_000_263)
    ap.add_argument("--f", type=int, default=100)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--recommend-repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    if cu.device_count() < 1:
        raise SystemExit("topk_probe needs a GPU")

    t0 = time.perf_counter()
    tr, _ = synth.make_ratings(args.users, args.items, args.nnz, min_degree=20, seed=20240917, test_fraction=0.0)
    gen_s = time.perf_counter() - t0
    rng = np.random.RandomState(1)
    U, I, f, k = tr.rows, tr.cols, args.f, args.k
    P, Q = (rng.randn(U, f) * 0.1).astype(np.float32), (rng.randn(I, f) * 0.1).astype(np.float32)
    ub, ib = (rng.randn(U) * 0.1).astype(np.float32), (rng.randn(I) * 0.1).astype(np.float32)
    model = cu.Model(U, I, f, tr.global_bias, P, Q, ub, ib)
    ex = cu.DeviceCSR(tr)

    def timed(fn, n):
        out, times = fn(), []  # warm-up
        for _ in range(n):
            t = time.perf_counter()
            out = fn()
            times.append(time.perf_counter() - t)
        return out, times

    topk, t_topk = timed(lambda: model.topk(ex, k), args.repeats)
    rec, t_rec = timed(lambda: model.recommend(ex, k), args.recommend_repeats)
    same_items = bool(np.array_equal(topk[0], rec[0]))
    same_scores = bool(np.array_equal(topk[1].view(np.uint32), rec[1].view(np.uint32)))
    med_topk, med_rec = float(np.median(t_topk)), float(np.median(t_rec))
    flops = 2.0 * U * I * f
    res = {"shape": {"users": U, "items": I, "nnz_excluded": int(tr.nnz), "f": f, "k": k}, "generate_s": gen_s,
           "topk_s": t_topk, "recommend_s": t_rec, "topk_median_s": med_topk, "recommend_median_s": med_rec,
           "speedup": med_rec / med_topk, "equal_items": same_items, "equal_score_bits": same_scores,
           "topk_tflops": flops / med_topk / 1e12, "topk_share_of_f32_mfma_peak": flops / med_topk / PEAK_F32_MFMA}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0 if same_items and same_scores else 1


if __name__ == "__main__":
    sys.exit(main())
