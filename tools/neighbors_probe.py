"""Times the neighbour queries at the ML-20M shape against cu2rec_model_topk in the same process (GPU tool; one process under its
own time limit).

    timeout -k 10 900 python tools/neighbors_probe.py [--out result.json]

138,493 users x 26,744 items, f = 100, k = 10, random factors; a synthetic training set with ML-20M's 20,000,263 ratings is the
exclusion (user-major for topk, its transpose for top_users).  Three calls, each timed end to end through the C ABI (each returns
after its last device-to-host copy) after one warm-up call, median of the repeats:
    similar(every item, cosine)            2 I^2 f FLOP
    top_users(every item, exclude = R^T)   2 U I f FLOP
    topk(every user, exclude = R)          2 U I f FLOP, the yardstick
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
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    if cu.device_count() < 1:
        raise SystemExit("neighbors_probe needs a GPU")

    t0 = time.perf_counter()
    tr, _ = synth.make_ratings(args.users, args.items, args.nnz, min_degree=20, seed=20240917, test_fraction=0.0)
    tr_t = tr.transpose()
    gen_s = time.perf_counter() - t0
    rng = np.random.RandomState(1)
    U, I, f, k = tr.rows, tr.cols, args.f, args.k
    P, Q = (rng.randn(U, f) * 0.1).astype(np.float32), (rng.randn(I, f) * 0.1).astype(np.float32)
    ub, ib = (rng.randn(U) * 0.1).astype(np.float32), (rng.randn(I) * 0.1).astype(np.float32)
    model = cu.Model(U, I, f, tr.global_bias, P, Q, ub, ib)
    ex, ex_t = cu.DeviceCSR(tr), cu.DeviceCSR(tr_t)

    def timed(fn, n):
        out, times = fn(), []  # warm-up
        for _ in range(n):
            t = time.perf_counter()
            out = fn()
            times.append(time.perf_counter() - t)
        return out, times

    calls = {
        "similar_items_cosine": (lambda: model.similar(None, k, side="items", metric="cosine"), 2.0 * I * I * f),
        "top_users": (lambda: model.top_users(ex_t, k), 2.0 * U * I * f),
        "topk": (lambda: model.topk(ex, k), 2.0 * U * I * f),
    }
    res = {"shape": {"users": U, "items": I, "nnz_excluded": int(tr.nnz), "f": f, "k": k}, "generate_s": gen_s}
    outs = {}
    for name, (fn, flops) in calls.items():
        outs[name], times = timed(fn, args.repeats)
        med = float(np.median(times))
        res[name] = {"s": times, "median_s": med, "tflops": flops / med / 1e12, "share_of_f32_mfma_peak": flops / med / PEAK_F32_MFMA}
    res["top_users_over_topk"] = res["top_users"]["median_s"] / res["topk"]["median_s"]
    # sanity: at this shape every query has far more than k candidates, so every list is full
    res["lists_full"] = bool(all((o[0] >= 0).all() for o in outs.values()))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0 if res["lists_full"] else 1


if __name__ == "__main__":
    sys.exit(main())
