"""Times SLIM (cu2rec_slim_create) on the synthetic ML-20M shape: a build of 1, 2, .. --sweeps sweeps (tol = 0), the time of each sweep
split by kernel, the share of update tiles each sweep skips, and the nonzero fraction of W after each.

    python tools/slim_probe.py [--shapes ml-20m] [--l1 5] [--l2 500] [--sweeps 3] [--no-kernels] [--out FILE]

Build times are wall clock around the synchronous call after one warm-up build of one sweep (which builds the row-sorted and the
item-major view, which the CSR keeps); the time of sweep s is the build of s sweeps minus the build of s - 1 (the first also holds the
Gram matrix, the copy and the allocations).  Kernel times: a child process builds the --sweeps model under `rocprofv3 --kernel-trace`;
a sweep is one slim_sweep and one slim_update launch per block of coordinates, so the launches of each kernel, in their order, split
into sweeps by count.  The skipped tiles are counted from the models themselves: builds are bit-identical, so the weights a sweep
changed are where the model of s sweeps differs from the model of s - 1, and a 64 x 64 tile of that difference with no nonzero is a
tile of Delta whose flag was clear -- every one of the block's update workgroups in that column of tiles returned at once.
No time is a pass condition: there is no earlier SLIM here to compare with.  The yardstick quoted is EASE's build on the same shape."""
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

EASE_CREATE_MS = 1287.0  # profiles/ease_probe_ml20m.txt: cu2rec_ease_create on the same shape


def kernel_times(shape, l1, l2, sweeps, blocks):
    """One build in a child under a kernel trace -> [{kernel: ms} per sweep], or a word on why not."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--shapes", shape, "--l1", str(l1), "--l2", str(l2), "--sweeps", str(sweeps)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        except (OSError, subprocess.TimeoutExpired) as err:
            return "the traced child did not run: %s" % err
        traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if res.returncode != 0 or not traces:
            return "the traced child failed (%d): %s" % (res.returncode, res.stderr[-300:])
        with open(traces[0]) as fh:
            rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], int(r["End_Timestamp"])) for r in csv.DictReader(fh))
    out = [dict() for _ in range(sweeps)]
    seen = {}
    for start, name, end in rows:
        m = re.search(r"\b(slim_sweep|slim_update)_kernel\b", name)
        if not m:
            continue
        n = seen.get(m.group(1), 0)
        seen[m.group(1)] = n + 1
        if n // blocks < sweeps:
            out[n // blocks][m.group(1)] = out[n // blocks].get(m.group(1), 0.0) + (end - start) / 1e6
    if any(seen.get(k, 0) != sweeps * blocks for k in ("slim_sweep", "slim_update")):
        return "the trace holds %s launches, not %d of each kernel" % (seen, sweeps * blocks)
    return out


def changed_tiles(before, after, cols, nb):
    """(blocks, tiles) bool: the nb x nb tiles in which the two models' weights differ (before None: all zeros)."""
    T = -(-cols // nb)
    out = np.zeros((T, T), bool)
    pad = T * nb - cols
    for kb in range(T):
        ids = np.arange(kb * nb, min((kb + 1) * nb, cols), dtype=np.int32)
        d = after.weights(ids)
        if before is not None:
            d = d != before.weights(ids)
        out[kb] = np.pad(d != 0, ((0, 0), (0, pad))).reshape(len(ids), T, nb).any(axis=(0, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml-20m")
    ap.add_argument("--l1", type=float, default=5.0)
    ap.add_argument("--l2", type=float, default=500.0)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help="build one model and leave (what the kernel trace wraps)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        tr, _ = synth.make_named(args.shapes)
        cu.SLIM(cu.DeviceCSR(tr), args.l1, args.l2, True, args.sweeps, 0.0).close()
        return
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    nb = cu.lib().cu2rec_ease_block_items()
    for name in args.shapes.split(","):
        tr, _ = synth.make_named(name)
        d = cu.DeviceCSR(tr)
        T = -(-tr.cols // nb)
        ld = T * nb
        say("%s: %d users, %d items, %d entries; l1 = %g, l2 = %g, non-negative, tol = 0; blocks of %d coordinates: order %d, %d blocks,"
            % (name, tr.rows, tr.cols, tr.nnz, args.l1, args.l2, nb, ld, T))
        say("  three matrices of %.2f GB while building; a dense sweep is %.3g flop in %d x %d x %d tile products" % (4.0 * ld * ld / 1e9, 2.0 * ld ** 3, T, T, T))
        cu.SLIM(d, args.l1, args.l2, True, 1, 0.0).close()  # warm-up
        models, walls = [], []
        for s in range(1, args.sweeps + 1):
            t0 = time.perf_counter()
            models.append(cu.SLIM(d, args.l1, args.l2, True, s, 0.0))
            walls.append(1e3 * (time.perf_counter() - t0))
        kernels = None if args.no_kernels else kernel_times(name, args.l1, args.l2, args.sweeps, T)
        say("  sweeps   build ms   this sweep ms   slim_sweep ms  slim_update ms   update tiles skipped   largest |delta|   nonzero fraction of W")
        for s in range(1, args.sweeps + 1):
            changed = changed_tiles(models[s - 2] if s > 1 else None, models[s - 1], tr.cols, nb)
            rep = models[s - 1].report
            ker = ("%14.2f %15.2f" % (kernels[s - 1].get("slim_sweep", 0.0), kernels[s - 1].get("slim_update", 0.0))
                   if isinstance(kernels, list) else "%14s %15s" % ("-", "-"))
            say("  %6d %10.2f %15.2f %s %22.4f %17.3g %23.5f" %
                (s, walls[s - 1], walls[s - 1] - (walls[s - 2] if s > 1 else 0.0), ker, 1.0 - changed.mean(), rep["last_delta"],
                 rep["nonzeros"] / float(tr.cols) ** 2))
            if s > 1:
                models[s - 2].close()
        if isinstance(kernels, str):
            say("  kernel times: NOT MEASURED (%s)" % kernels)
        else:
            say("  (kernel times of one traced build of %d sweeps, summed per sweep; the launches are serial on one stream.  The first" % args.sweeps)
            say("  sweep's wall time also holds the Gram matrix, the copy of A and the three allocations.)")
        say("  yardstick: cu2rec_ease_create on this shape took %.0f ms (profiles/ease_probe_ml20m.txt)" % EASE_CREATE_MS)
        models[-1].close()
        d.close()
    say("NOT MEASURED: sweeps past the last one above or a run to a tol stop, cache hit rates and what bounds either kernel (no counters")
    say("were read), the once-per-CSR segmented sort and item-major view (inside the warm-up), other l1, l2, block orders or shapes,")
    say("signed weights, and real data: the synthetic shape's values and co-occurrences are not MovieLens's.")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
