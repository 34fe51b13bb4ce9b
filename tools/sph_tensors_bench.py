"""The SPH gradient tensors at config-5 size ("SPH gradient tensors").

Writes the frame of tools/neighbours_bench.py -- N rows, float32 mass, velocity, energy and position (uniform in a
triclinic box) -- to /dev/shm from the device, selects the rows of one cell of the 2x2x2 decomposition (about N / 8
entries), sorts that list by cell for the grid `pgsd.hoomd.neighbour_grid_for` gives for the support ``2h`` (the same
list, the same grid, the same candidates as tools/sph_gradients_bench.py), and times, served from the staged rows on a
warm page cache:
  * sph_tensors_device over the sorted list for both kernels (the frame stores no density: its float32 energy column
    stands in for the density chunk, which costs the same staging and the same arithmetic),
  * the yardstick: sph_gradients_device with the volume sums over the same ordered list and grid, the call whose pair
    loop this one widens from eight accumulators to fifteen.
``candidates`` is the number of (i, j) pairs the census' pair kernel visits, from the per-cell counts of the ordered list;
the SPH pair kernels visit these and each entry itself.
With ``--host`` also what the answer costs without the feature: a host read of the four chunks and
pgsd.hoomd.sph_gradient_tensors over a SUB-list -- the rows of a slab of the same cell, about ``--model-entries`` of them
--, once; the GPU's result over the same sub-list must equal it bit for bit, and the figure is scaled to the whole list by
the candidates (said as such in the record).
``staged_ms`` is the median of ``--repeats`` calls with minimum and maximum.  One JSON line per call.  The kernels' own
times come from a separate run under ``rocprofv3 --kernel-trace --stats -- python tools/sph_tensors_bench.py
--kernels-only``, which issues every call once.

    python tools/sph_tensors_bench.py [--n 80000000] [--h 0.0985] [--det-min 0.25] [--repeats 5] [--kernels-only] [--host]
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
ARRAYS = ('correction', 'determinant', 'velocity_gradient', 'shear_rate')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--h", type=float, default=0.0985, help="the smoothing length: 2h = 0.197, the census' range")
    ap.add_argument("--det-min", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="issue every call once (for rocprofv3)")
    ap.add_argument("--host", action="store_true", help="also time the host read and the numpy model over a sub-list, once")
    ap.add_argument("--model-entries", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = "/dev/shm/pgsd_sph_tensors_bench_%d.gsd" % os.getpid()
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
            # warm: reader threads, pinned ring, kernels; the row list of one cell; all four chunks staged, which they stay
            # until the wait at the end
            selected, count = f.select_domain_device(0, POSITION, BOX, hoomd.domain_grid(2, 2, 2)[0])
            rows = selected.clone()
            f.frame_moments_device([None] + chunks, rows=rows, n=count)
            t_order, cell = timed(lambda: f.order_rows_by_cell_device(0, POSITION, BOX, grid, rows, n=count))
            fields = f.cell_moments_device(chunks, rows, cell, count, n_cells)
            base = {"N": a.n, "rows": count, "h": a.h, "support": support, "grid": list(grid), "n_cells": n_cells,
                    "candidates": candidates_of(fields.count, grid), "largest_cell": int(fields.count.max())}
            say(dict(base, kind="order_rows_by_cell", staged_ms=round(t_order, 3)))
            for kernel in hoomd.SPH_KERNELS:
                record(dict(base, kind="sph_gradients", kernel=kernel, volume=True),
                       lambda: f.sph_gradients_device(0, POSITION, BOX, a.h, grid, rows, cell, n=count, velocity=(0, VELOCITY),
                                                      mass=(0, MASS), density=(0, DENSITY), kernel=kernel).density_rate_max)
            for kernel in hoomd.SPH_KERNELS:
                def call(kernel=kernel, **kw):
                    return f.sph_tensors_device(0, POSITION, BOX, a.h, grid, rows, cell, n=count, velocity=(0, VELOCITY),
                                                mass=(0, MASS), density=(0, DENSITY), kernel=kernel, det_min=a.det_min, **kw)
                got = call()
                record(dict(base, kind="sph_tensors", kernel=kernel, det_min=a.det_min, uncorrected=got.uncorrected,
                            determinant_min=got.determinant_min, determinant_max=got.determinant_max, trace_min=got.trace_min,
                            trace_max=got.trace_max, shear=got.shear, not_finite=got.not_finite),
                       lambda: call().shear)
            if a.host:
                # a slab of the same cell with about --model-entries rows: a list the model finishes
                width = 0.5 * min(1.0, a.model_entries / max(count, 1))
                slab = hoomd.Domain((0.0, 0.0, 0.0), (width, 0.5, 0.5))
                sub, m = f.select_domain_device(0, POSITION, BOX, slab)
                sub = sub.clone()
                sub_cell = f.order_rows_by_cell_device(0, POSITION, BOX, grid, sub, n=m)
                sub_candidates = candidates_of(f.cell_moments_device(chunks, sub, sub_cell, m, n_cells).count, grid)
                t_read, arrays = timed(lambda: [f.read_chunk(0, name) for name in (POSITION, VELOCITY, MASS, DENSITY)])
                h_rows = sub[:m].cpu().numpy()
                for kernel in hoomd.SPH_KERNELS:
                    t_gpu, small = timed(lambda: f.sph_tensors_device(0, POSITION, BOX, a.h, grid, sub, sub_cell, n=m,
                                                                      velocity=(0, VELOCITY), mass=(0, MASS),
                                                                      density=(0, DENSITY), kernel=kernel, det_min=a.det_min,
                                                                      return_rows=True))
                    t_model, want = timed(lambda: hoomd.sph_gradient_tensors(arrays[0], arrays[1], BOX, a.h, mass=arrays[2],
                                                                             density=arrays[3], rows=h_rows, cells=grid,
                                                                             kernel=kernel, det_min=a.det_min))
                    equal = bool(np.array_equal(want.summary[:8], small.summary[:8]) and want.summary[13] == small.summary[13]
                                 and bits_equal(want.summary[8:13].view(np.float64), small.summary[8:13].view(np.float64))
                                 and all(bits_equal(getattr(small, name)[:m].cpu().numpy().ravel(), getattr(want, name).ravel())
                                         for name in ARRAYS))
                    say(dict(base, kind="host_read_and_model", kernel=kernel, sub_rows=m, sub_candidates=sub_candidates,
                             read_ms=round(t_read, 1), model_ms=round(t_model, 1), gpu_ms_same_sub_list=round(t_gpu, 3),
                             model_ms_scaled_to_the_list=round(t_model * base["candidates"] / max(sub_candidates, 1), 1),
                             scaled_by="candidates of the list over candidates of the sub-list", equals_the_gpu=equal))
                del arrays
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
