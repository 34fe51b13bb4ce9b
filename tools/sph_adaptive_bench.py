"""The SPH sums with a per-particle smoothing length at config-5 size ("SPH sums with a per-particle
smoothing length").

Writes the frame of tools/sph_sums_bench.py -- N rows, float32 mass, velocity, energy and position (uniform in a
triclinic box) -- with one more column, a seeded float32 ``slength`` uniform in ``[h / ratio, h]`` (``--h-ratio 1``: every
row holds ``h``), to /dev/shm from the device, selects the rows of one cell of the 2x2x2 decomposition (about N / 8
entries) and times, served from the staged rows on a warm page cache:
  * smoothing_range_device over the list (the call that finds ``h_max``) and the ordering for the grid of ``2 h_max``,
  * the yardstick: sph_sums_device over the sorted list with the volume sum, at ``h`` (the uniform pass),
  * sph_adaptive_sums_device over the same list and grid for both modes and both kernels, with the volume sum (the
    float32 energy column stands in for the density chunk).
``candidates`` is the number of (i, j) pairs a pair kernel visits on this grid, from the per-cell counts of the ordered
list; ``pairs`` is the number that pass the per-pair support test.  With ``--h-ratio 1`` gather mode does the work of the
uniform pass plus F and one accumulator, and the two must agree bit for bit (``equals_the_uniform_pass``).
``staged_ms`` is the median of ``--repeats`` calls with minimum and maximum.  One JSON line per call.  The kernels' own
times come from a separate run under ``rocprofv3 --kernel-trace --stats -- python tools/sph_adaptive_bench.py
--kernels-only``, which issues every call once.

    python tools/sph_adaptive_bench.py [--n 80000000] [--h 0.0985] [--h-ratio 2] [--repeats 5] [--kernels-only] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pgsd-sph_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402
from cell_moments_bench import BOX, NAMES, timed  # noqa: E402
from neighbours_bench import candidates_of  # noqa: E402
from sph_sums_bench import bits_equal  # noqa: E402

MASS, DENSITY, POSITION = NAMES[0], NAMES[2], NAMES[3]      # (the energy column stands in for the density chunk)
SLENGTH = "particles/slength"


def write(path, N, h, ratio):
    """cell_moments_bench.write's frame (the same generator, so the same rows) and the slength column."""
    g = torch.Generator(device="cuda").manual_seed(1)
    s = torch.rand((N, 3), generator=g, device="cuda", dtype=torch.float32) - 0.5
    Lx, Ly, Lz, xy, xz, yz = BOX
    pos = torch.empty((N, 3), dtype=torch.float32, device="cuda")
    pos[:, 2] = s[:, 2] * Lz
    pos[:, 1] = s[:, 1] * Ly + yz * pos[:, 2]
    pos[:, 0] = s[:, 0] * Lx + xy * pos[:, 1] + xz * pos[:, 2]
    del s
    vel = torch.randn((N, 3), generator=g, device="cuda", dtype=torch.float32)
    mass = 0.5 + torch.rand((N,), generator=g, device="cuda", dtype=torch.float32)
    energy = 1.0 + 0.1 * torch.randn((N,), generator=g, device="cuda", dtype=torch.float32)
    lo = h / ratio
    slength = (lo + (h - lo) * torch.rand((N,), generator=g, device="cuda", dtype=torch.float32)).clamp(max=h)
    with fl.open(path, "w", application="sph_adaptive_bench", schema="hoomd", schema_version=[1, 4]) as f:
        f.write_chunk("configuration/step", np.array([0], dtype=np.uint64), write_all=False)
        f.write_chunk("configuration/box", np.array(BOX, dtype=np.float32), write_all=False)
        f.write_chunk("particles/N", np.array([N], dtype=np.uint32), write_all=False)
        f.write_chunks([(NAMES[0], fl.DeviceField.from_tensor(mass)), (NAMES[1], fl.DeviceField.from_tensor(vel)),
                        (NAMES[2], fl.DeviceField.from_tensor(energy)), (NAMES[3], fl.DeviceField.from_tensor(pos)),
                        (SLENGTH, fl.DeviceField.from_tensor(slength))], offset=np.array([N]))
        f.end_frame()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--h", type=float, default=0.0985, help="the largest smoothing length: 2h = 0.197, the census' range")
    ap.add_argument("--h-ratio", type=float, default=2.0, help="the largest smoothing length over the smallest (1: uniform)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="issue every call once (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not a.h_ratio >= 1.0:
        ap.error("--h-ratio is at least 1")
    path = "/dev/shm/pgsd_sph_adaptive_bench_%d.gsd" % os.getpid()
    lines = []
    h = float(np.float32(a.h))

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
        write(path, a.n, h, a.h_ratio)
        chunks = [(0, name) for name in NAMES]
        with fl.open(path, "r") as f:
            # warm: reader threads, pinned ring, kernels; the row list of one cell; the chunks staged, which they stay until
            # the wait at the end
            selected, count = f.select_domain_device(0, POSITION, BOX, hoomd.domain_grid(2, 2, 2)[0])
            rows = selected.clone()
            f.frame_moments_device([None] + chunks, rows=rows, n=count)
            f.smoothing_range_device((0, SLENGTH), a.n, rows, n=count)
            t_range, found = timed(lambda: f.smoothing_range_device((0, SLENGTH), a.n, rows, n=count))
            h_max = found[3]
            support = float(np.float64(2.0) * np.float64(h_max))
            grid = hoomd.neighbour_grid_for(BOX, support)
            n_cells = grid[0] * grid[1] * grid[2]
            t_order, cell = timed(lambda: f.order_rows_by_cell_device(0, POSITION, BOX, grid, rows, n=count))
            fields = f.cell_moments_device(chunks, rows, cell, count, n_cells)
            base = {"N": a.n, "rows": count, "h": h, "h_ratio": a.h_ratio, "h_min": found[2], "h_max": h_max, "grid": list(grid),
                    "n_cells": n_cells, "candidates": candidates_of(fields.count, grid), "largest_cell": int(fields.count.max())}
            say(dict(base, kind="smoothing_range", staged_ms=round(t_range, 3), bad=found[1]))
            say(dict(base, kind="order_rows_by_cell", staged_ms=round(t_order, 3)))

            def uniform(**kw):
                return f.sph_sums_device(0, POSITION, BOX, h_max, grid, rows, cell, n=count, mass=(0, MASS), density=(0, DENSITY),
                                         kernel='wendland_c2', **kw)
            record(dict(base, kind="sph_sums", kernel='wendland_c2', volume=True), lambda: uniform().density_max)
            for mode in hoomd.SPH_MODES:
                for kernel in hoomd.SPH_KERNELS:
                    def call(kernel=kernel, mode=mode, **kw):
                        return f.sph_adaptive_sums_device(0, POSITION, BOX, h_max, grid, rows, cell, n=count, slength=(0, SLENGTH),
                                                          mass=(0, MASS), density=(0, DENSITY), kernel=kernel, mode=mode, **kw)
                    got = call()
                    rec = dict(base, kind="sph_adaptive_sums", mode=mode, kernel=kernel, volume=True, pairs=got.pairs,
                               count_min=got.count_min, count_max=got.count_max, density_min=got.density_min,
                               density_max=got.density_max, omega_min=got.omega_min, omega_max=got.omega_max)
                    if a.h_ratio == 1.0 and mode == 'gather' and kernel == 'wendland_c2':
                        one, two = uniform(return_rows=True), call(return_rows=True)
                        rec["equals_the_uniform_pass"] = bool(
                            bits_equal(one.density[:count].cpu().numpy(), two.density[:count].cpu().numpy())
                            and bits_equal(one.shepard[:count].cpu().numpy(), two.shepard[:count].cpu().numpy()))
                        del one, two
                    record(rec, lambda: call().density_max)
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
