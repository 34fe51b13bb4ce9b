"""The neighbour census at config-5 size ("Neighbour census").

Writes an N-row frame -- float32 mass, velocity, energy and position (uniform in a triclinic box) -- to /dev/shm from the
device, selects the rows of one cell of the 2x2x2 decomposition (about N / 8 entries), sorts that list by cell for the grid
`pgsd.hoomd.neighbour_grid_for` gives for a range ``r`` of about 40 neighbours per entry, and times, served from the
staged rows on a warm page cache:
  * neighbours_device over the sorted list (check, offsets, compaction, pair and final kernels, the summary's copy),
  * yardstick (c): the parent's cell_moments_device over the same ordered list and grid -- what ordering, offsets and a
    gathered pass cost without a pair loop,
  * the ordering itself, order_rows_by_cell_device, which the hoomd-level call pays once before the pass.
``candidates`` is the number of (i, j) pairs the pair kernel visits, computed from the per-cell counts of the ordered list
(the cell fields' counts), so that candidate pairs per second can be set against tools/labs/pair_ceiling.hip.
With ``--host`` also yardstick (b), what the answer costs without the feature: a host read of the position chunk and
pgsd.hoomd.particle_neighbours over a SUB-list -- the rows of a slab of the same cell, about ``--model-entries`` of them
--, once; the GPU's result over the same sub-list must equal it exactly, and the figure is scaled to the whole list by the
candidates (said as such in the record).
``staged_ms`` is the median of ``--repeats`` calls with minimum and maximum.  One JSON line per call.  The kernels' own
times come from a separate run under ``rocprofv3 --kernel-trace --stats -- python tools/neighbours_bench.py
--kernels-only``, which issues every call once.

    python tools/neighbours_bench.py [--n 80000000] [--r 0.197] [--repeats 5] [--kernels-only] [--host] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pgsd-sph_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402
from cell_moments_bench import BOX, NAMES, timed, write  # noqa: E402


def candidates_of(count, grid):
    """The (i, j) pairs the pair kernel visits for per-cell counts ``count`` (x fastest): per cell its count times the
    counts of the deduplicated adjacent cells, minus the self pairs."""
    c = np.asarray(count, dtype=np.float64).reshape(grid[2], grid[1], grid[0])
    around = np.zeros_like(c)
    offsets = [hoomd._axis_offsets(g) for g in grid]
    for oz in offsets[2]:
        for oy in offsets[1]:
            for ox in offsets[0]:
                around += np.roll(c, shift=(-oz, -oy, -ox), axis=(0, 1, 2))
    return int((c * around).sum() - c.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--r", type=float, default=0.197, help="the range: about 40 neighbours per entry at the default size")
    ap.add_argument("--bins", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="issue every call once (for rocprofv3)")
    ap.add_argument("--host", action="store_true", help="also time the host read and the numpy model over a sub-list, once")
    ap.add_argument("--model-entries", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = "/dev/shm/pgsd_neighbours_bench_%d.gsd" % os.getpid()
    lines = []

    def say(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        return rec

    def record(rec, fn):
        rec["value"] = fn()
        if not a.kernels_only:
            staged = [timed(fn)[0] for _ in range(a.repeats)]
            rec.update(staged_ms=round(float(np.median(staged)), 3), staged_min_ms=round(min(staged), 3),
                       staged_max_ms=round(max(staged), 3))
        return say(rec)

    try:
        write(path, a.n)
        chunks = [(0, name) for name in NAMES]
        grid = hoomd.neighbour_grid_for(BOX, a.r)
        n_cells = grid[0] * grid[1] * grid[2]
        with fl.open(path, "r") as f:
            # warm: reader threads, pinned ring, kernels; the row list of one cell; all four chunks staged, which they stay
            # until the wait at the end
            selected, count = f.select_domain_device(0, NAMES[3], BOX, hoomd.domain_grid(2, 2, 2)[0])
            rows = selected.clone()
            f.frame_moments_device([None] + chunks, rows=rows, n=count)
            t_order, cell = timed(lambda: f.order_rows_by_cell_device(0, NAMES[3], BOX, grid, rows, n=count))
            fields = f.cell_moments_device(chunks, rows, cell, count, n_cells)
            base = {"N": a.n, "rows": count, "r": a.r, "grid": list(grid), "n_cells": n_cells, "bins": a.bins,
                    "candidates": candidates_of(fields.count, grid), "largest_cell": int(fields.count.max())}
            say(dict(base, kind="order_rows_by_cell", staged_ms=round(t_order, 3)))
            record(dict(base, kind="cell_moments_same_list"),
                   lambda: float(f.cell_moments_device(chunks, rows, cell, count, n_cells).kinetic.sum()))
            got = f.neighbours_device(0, NAMES[3], BOX, a.r, grid, rows, cell, n=count, bins=a.bins)
            base.update(pairs=got.pairs, mean_count=round(got.mean_count, 3), count_max=got.count_max, isolated=got.isolated,
                        closest_distance=got.closest_distance)
            mine = record(dict(base, kind="neighbours"),
                          lambda: int(f.neighbours_device(0, NAMES[3], BOX, a.r, grid, rows, cell, n=count, bins=a.bins).pairs))
            if not a.kernels_only:
                mine["candidates_per_s_of_the_call"] = float("%.4g" % (base["candidates"] / (mine["staged_ms"] * 1e-3)))
                say({"kind": "rate", "candidates_per_s_of_the_call": mine["candidates_per_s_of_the_call"]})
            if a.host:
                # a slab of the same cell with about --model-entries rows: the real density, a list the model finishes
                width = 0.5 * min(1.0, a.model_entries / max(count, 1))
                slab = hoomd.Domain((0.0, 0.0, 0.0), (width, 0.5, 0.5))
                sub, m = f.select_domain_device(0, NAMES[3], BOX, slab)
                sub = sub.clone()
                sub_cell = f.order_rows_by_cell_device(0, NAMES[3], BOX, grid, sub, n=m)
                sub_fields = f.cell_moments_device(chunks, sub, sub_cell, m, n_cells)
                sub_candidates = candidates_of(sub_fields.count, grid)
                t_gpu, small = timed(lambda: f.neighbours_device(0, NAMES[3], BOX, a.r, grid, sub, sub_cell, n=m, bins=a.bins,
                                                                 return_rows=True))
                t_read, position = timed(lambda: f.read_chunk(0, NAMES[3]))
                h_rows = sub[:m].cpu().numpy()
                t_model, want = timed(lambda: hoomd.particle_neighbours(position, BOX, a.r, rows=h_rows, cells=grid, bins=a.bins))
                equal = bool(np.array_equal(want.summary, small.summary)
                             and np.float64(want.closest2).view(np.uint64) == np.float64(small.closest2).view(np.uint64)
                             and np.array_equal(small.count[:m].cpu().numpy().view(np.uint32), want.count)
                             and np.array_equal(small.nearest[:m].cpu().numpy().view(np.uint32), want.nearest)
                             and np.array_equal(small.nearest2[:m].cpu().numpy().view(np.uint64), want.nearest2.view(np.uint64)))
                say(dict(base, kind="host_read_and_model", sub_rows=m, sub_candidates=sub_candidates,
                         read_ms=round(t_read, 1), model_ms=round(t_model, 1), gpu_ms_same_sub_list=round(t_gpu, 3),
                         model_ms_scaled_to_the_list=round(t_model * base["candidates"] / max(sub_candidates, 1), 1),
                         scaled_by="candidates of the list over candidates of the sub-list", equals_the_gpu=equal))
                del position
            f.wait_read()
    finally:
        if os.path.exists(path):
            os.unlink(path)
    if a.out:
        with open(a.out, "w") as out:
            for r in lines:
                out.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
