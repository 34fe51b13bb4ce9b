"""The SPH samples at config-5 size ("SPH samples").

Writes the frame of tools/neighbours_bench.py -- N rows, float32 mass, velocity, energy and position (uniform in a
triclinic box) -- to /dev/shm from the device, selects the rows of one cell of the 2x2x2 decomposition (about N / 8
entries), sorts that list by cell for the grid `pgsd.hoomd.neighbour_grid_for` gives for the support ``2h`` (the same
list, the same grid and the same ``h`` as tools/sph_forces_bench.py), lays a `pgsd.hoomd.sample_grid` over the same
cell of the decomposition with about as many points as the list has entries, and times, served from the staged rows on a
warm page cache and with the points in GPU memory:
  * sph_samples_device at those points for both kernels, with the velocity and one scalar as values (C = 4; the frame
    stores no density: its float32 energy column stands in for the density chunk) and with no value (C = 0),
  * once, with ``--shuffled``, the same call with the points in a seeded random order: what unordered points cost,
  * the yardstick: sph_sums_device with the volume sum over the same ordered list and grid, the call whose pair loop this
    one resembles most.
``candidates`` is the number of (centre, j) pairs a pair kernel visits, from the per-cell counts of the ordered list and,
for the samples, of the points; every record carries the candidates per second of its call.
With ``--host`` also the numpy model over the 20 000 points of a small sub-box and a sub-list that covers their reach, once;
the GPU's result over the same points and sub-list must equal it bit for bit: the tool exits 1 if it does not.
``staged_ms`` is the median of ``--repeats`` calls with minimum and maximum.  One JSON line per call.  The kernels' own
times come from a separate run under ``rocprofv3 --kernel-trace --stats -- python tools/sph_samples_bench.py
--kernels-only``, which issues every call once.

    python tools/sph_samples_bench.py [--n 80000000] [--h 0.0985] [--repeats 5] [--kernels-only] [--host] [--shuffled]
                                      [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pgsd-sph_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402,F401

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402
from cell_moments_bench import BOX, NAMES, timed, write  # noqa: E402
from neighbours_bench import candidates_of  # noqa: E402
from sph_sums_bench import bits_equal  # noqa: E402

MASS, VELOCITY, DENSITY, POSITION = NAMES       # (the energy column stands in for the density chunk)
VALUES = {4: [(0, VELOCITY), (0, MASS)], 0: []}


def sample_candidates(entries, points, grid):
    """The (point, j) pairs the point kernel visits: per cell its points times the entries of the deduplicated adjacent
    cells (x fastest)."""
    c = np.asarray(entries, dtype=np.float64).reshape(grid[2], grid[1], grid[0])
    p = np.asarray(points, dtype=np.float64).reshape(grid[2], grid[1], grid[0])
    around = np.zeros_like(c)
    offsets = [hoomd._axis_offsets(g) for g in grid]
    for oz in offsets[2]:
        for oy in offsets[1]:
            for ox in offsets[0]:
                around += np.roll(c, shift=(-oz, -oy, -ox), axis=(0, 1, 2))
    return int((p * around).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--h", type=float, default=0.0985, help="the smoothing length: 2h = 0.197, the census' range")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="issue every call once (for rocprofv3)")
    ap.add_argument("--host", action="store_true", help="also run the numpy model over a sub-box of the points, once")
    ap.add_argument("--shuffled", action="store_true", help="also time the points in a seeded random order, C = 4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = "/dev/shm/pgsd_sph_samples_bench_%d.gsd" % os.getpid()
    lines = []
    support = float(np.float64(2.0) * np.float64(a.h))

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
            rec["candidates_per_s_of_the_call"] = float("%.4g" % (rec["candidates"] / (rec["staged_ms"] * 1e-3)))
        return say(rec)

    try:
        write(path, a.n)
        chunks = [(0, name) for name in NAMES]
        grid = hoomd.neighbour_grid_for(BOX, support)
        n_cells = grid[0] * grid[1] * grid[2]
        with fl.open(path, "r") as f:
            device = torch.device("cuda", f.pipeline_device())
            # warm: reader threads, pinned ring, kernels; the row list of one cell; all four chunks staged, which they stay
            # until the wait at the end
            selected, count = f.select_domain_device(0, POSITION, BOX, hoomd.domain_grid(2, 2, 2)[0])
            rows = selected.clone()
            f.frame_moments_device([None] + chunks, rows=rows, n=count)
            t_order, cell = timed(lambda: f.order_rows_by_cell_device(0, POSITION, BOX, grid, rows, n=count))
            fields = f.cell_moments_device(chunks, rows, cell, count, n_cells)
            side = max(1, int(round(count ** (1.0 / 3.0))))
            host_points = hoomd.sample_grid(BOX, (side, side, side), lo=(0.0, 0.0, 0.0), hi=(0.5, 0.5, 0.5))
            K = len(host_points)
            per_cell = np.bincount(hoomd.cell_ids(host_points, BOX, grid), minlength=n_cells + 1)[:n_cells]
            points = torch.from_numpy(host_points).to(device)
            base = {"N": a.n, "rows": count, "h": a.h, "support": support, "grid": list(grid), "n_cells": n_cells,
                    "largest_cell": int(fields.count.max())}
            list_candidates = candidates_of(fields.count, grid) + count          # (the SPH kernels visit each entry itself too)
            point_candidates = sample_candidates(fields.count, per_cell, grid)
            say(dict(base, kind="order_rows_by_cell", staged_ms=round(t_order, 3)))
            for kernel in hoomd.SPH_KERNELS:
                record(dict(base, kind="sph_sums", kernel=kernel, volume=True, candidates=list_candidates),
                       lambda: f.sph_sums_device(0, POSITION, BOX, a.h, grid, rows, cell, n=count, mass=(0, MASS),
                                                 density=(0, DENSITY), kernel=kernel).density_max)

            def sample(kernel, C, at=points, which=rows, ids=cell, m=count, **kw):
                return f.sph_samples_device(0, POSITION, BOX, a.h, grid, which, ids, at, n=m, values=VALUES[C], mass=(0, MASS),
                                            density=(0, DENSITY), kernel=kernel, **kw)

            for kernel in hoomd.SPH_KERNELS:
                for C in (4, 0):
                    got = sample(kernel, C)
                    record(dict(base, kind="sph_samples", kernel=kernel, C=C, points=K, sample_grid=[side] * 3,
                                candidates=point_candidates, empty=got.empty, outside=got.outside, nowhere=got.nowhere,
                                not_finite=got.not_finite, count_max=got.count_max),
                           lambda kernel=kernel, C=C: sample(kernel, C).shepard_max)
            if a.shuffled:
                order = torch.randperm(K, generator=torch.Generator().manual_seed(2)).to(device)
                mixed = points[order].contiguous()
                record(dict(base, kind="sph_samples_shuffled_points", kernel="wendland_c2", C=4, points=K,
                            candidates=point_candidates), lambda: sample("wendland_c2", 4, at=mixed).shepard_max)
                del mixed, order
            if a.host:
                # the points of a sub-box and the entries of a slab that covers their reach: a call the model finishes
                few = hoomd.sample_grid(BOX, (32, 25, 25), lo=(0.1, 0.1, 0.1), hi=(0.12, 0.115, 0.115))
                slab = hoomd.Domain((0.09, 0.09, 0.09), (0.13, 0.125, 0.125))
                sub, m = f.select_domain_device(0, POSITION, BOX, slab)
                sub = sub.clone()
                sub_cell = f.order_rows_by_cell_device(0, POSITION, BOX, grid, sub, n=m)
                t_read, arrays = timed(lambda: [f.read_chunk(0, name) for name in (POSITION, VELOCITY, MASS, DENSITY)])
                h_rows = sub[:m].cpu().numpy()
                for kernel in hoomd.SPH_KERNELS:
                    t_gpu, small = timed(lambda: sample(kernel, 4, few, sub, sub_cell, m, normalise=True))
                    t_model, want = timed(lambda: hoomd.sph_samples(few, arrays[0], BOX, a.h, values=[arrays[1], arrays[2]],
                                                                    mass=arrays[2], density=arrays[3], rows=h_rows, cells=grid,
                                                                    kernel=kernel, normalise=True))
                    equal = bool(np.array_equal(want.summary[:7], small.summary[:7])
                                 and bits_equal(want.summary[7:].view(np.float64), small.summary[7:].view(np.float64))
                                 and np.array_equal(small.count.cpu().numpy(), want.count)
                                 and bits_equal(small.density.cpu().numpy(), want.density)
                                 and bits_equal(small.shepard.cpu().numpy(), want.shepard)
                                 and bits_equal(small.values.cpu().numpy().ravel(), want.values.ravel()))
                    say(dict(base, kind="host_read_and_model", kernel=kernel, sub_rows=m, sub_points=len(few),
                             read_ms=round(t_read, 1), model_ms=round(t_model, 1), gpu_ms_same_points=round(t_gpu, 3),
                             count_max=want.count_max, empty=want.empty, equals_the_gpu=equal))
                del arrays
            f.wait_read()
    finally:
        if os.path.exists(path):
            os.unlink(path)
    if a.out:
        with open(a.out, "w") as out:
            for r in lines:
                out.write(json.dumps(r) + "\n")
    # (the model must equal the GPU: a record that says otherwise fails the run)
    return 0 if all(r.get("equals_the_gpu", True) for r in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
