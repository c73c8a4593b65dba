"""Times EASE (cu2rec_ease_*) on the synthetic ML-20M shape: create as a whole and stage by stage, and recommend for every row.

    python tools/ease_probe.py [--shapes ml-20m] [--l2 500] [--k 10] [--reps 2] [--no-stages] [--out FILE]

Call times are wall clock around the synchronous call, best of --reps after one warm-up call (the warm-up builds the row-sorted and
the item-major view, which the CSR keeps).  The stages of create are kernel times: a child process builds one model under
`rocprofv3 --kernel-trace`, and the kernels' durations are summed per stage by name (ease_gram; ease_potrf / ease_trsm / ease_syrk;
ease_trtri / ease_copy_panel / ease_trtri_panel; ease_lauum / ease_mirror; ease_diag / ease_weights; the two small copies that a
later stage launches again count where they are named).  No time is a pass condition: there is no earlier EASE here to compare with."""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cu2rec_amd as cu  # noqa: E402
from cu2rec_amd import synth  # noqa: E402

STAGES = (("1 Gram", ("ease_gram",)), ("2 Cholesky", ("ease_potrf", "ease_trsm", "ease_syrk")),
          ("3 inverse of L", ("ease_trtri", "ease_copy_panel", "ease_trtri_panel")), ("4 P = W^T W, mirror", ("ease_lauum", "ease_mirror")),
          ("5 weights", ("ease_diag", "ease_weights")))


def best(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out)


def stage_times(shape, l2):
    """One create in a child under a kernel trace -> [(stage, kernels, summed ms, {kernel: ms})], or a word on why not."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--shapes", shape, "--l2", str(l2)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        except (OSError, subprocess.TimeoutExpired) as err:
            return "the traced child did not run: %s" % err
        traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if res.returncode != 0 or not traces:
            return "the traced child failed (%d): %s" % (res.returncode, res.stderr[-300:])
        with open(traces[0]) as fh:
            rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(fh)]
    out = []
    named = [(m.group(1), a, b) for m, a, b in ((re.search(r"\b(ease_\w+)_kernel\b", n), a, b) for n, a, b in rows) if m]
    for stage, names in STAGES:
        mine = [(n, a, b) for n, a, b in named if n in names]
        per = {}
        for n, a, b in mine:
            per[n] = per.get(n, 0.0) + (b - a) / 1e6
        out.append((stage, len(mine), sum(per.values()), per))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml-20m")
    ap.add_argument("--l2", type=float, default=500.0)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-stages", action="store_true")
    ap.add_argument("--child", action="store_true", help="build one model and leave (what the kernel trace wraps)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        tr, _ = synth.make_named(args.shapes)
        cu.EASE(cu.DeviceCSR(tr), args.l2).close()
        return
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    nb, s = cu.lib().cu2rec_ease_block_items(), cu.lib().cu2rec_knn_slice_items()
    for name in args.shapes.split(","):
        tr, _ = synth.make_named(name)
        d = cu.DeviceCSR(tr)
        ld = -(-tr.cols // nb) * nb
        n_u = np.diff(tr.indptr).astype(np.float64)
        say("%s: %d users, %d items, %d entries; l2 = %g, blocks of %d items: order %d, %d block columns, the matrix %.2f GB" %
            (name, tr.rows, tr.cols, tr.nnz, args.l2, nb, ld, ld // nb, 4.0 * ld * ld / 1e9))
        cu.EASE(d, args.l2).close()  # warm-up
        made = []

        def create():
            if made:
                made.pop().close()
            made.append(cu.EASE(d, args.l2))

        t_create = best(create, args.reps)
        ease = made[0]
        say("  create                  %10.2f ms   about %.3g flop in the dense stages (I^3 / 3 each for the Cholesky factor, the triangular"
            % (1e3 * t_create, 1.0 * ld ** 3))
        say("                                         inverse and W^T W), %.3g accumulations in the Gram matrix" % float((n_u * n_u).sum()))
        if not args.no_stages:
            stages = stage_times(name, args.l2)
            if isinstance(stages, str):
                say("  stages: NOT MEASURED (%s)" % stages)
            else:
                for stage, count, total, per in stages:
                    say("    %-22s %10.2f ms in %5d kernels   %s" % (stage, total, count, ", ".join("%s %.2f" % (k, v) for k, v in sorted(per.items()))))
                say("    (kernel times of one traced create, summed by kernel name; the launches are serial on one stream)")
        slices = -(-tr.cols // s)
        t_rec = best(lambda: ease.recommend(d, d, args.k), args.reps)
        say("  recommend, %6d rows  %10.2f ms   k = %d, history = exclusion = the training rows; %d slices per row, %.4g bytes of B rows read" %
            (tr.rows, 1e3 * t_rec, args.k, slices, 4.0 * tr.nnz * tr.cols))
        t_rank = best(lambda: ease.rank_metrics(d, d, args.k, exclude=d), 1)
        say("  rank_metrics, all rows  %10.2f ms   (one call)" % (1e3 * t_rank))
        t_nb = best(lambda: ease.neighbors(None, args.k), 1)
        say("  neighbors, every item   %10.2f ms   k = %d" % (1e3 * t_nb, args.k))
        ease.close()
        d.close()
    say("NOT MEASURED: cache hit rates, what bounds each stage (no counters were read), the once-per-CSR segmented sort and item-major")
    say("view (inside the warm-up), other l2, k, block orders or shapes.")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
