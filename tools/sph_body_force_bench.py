"""The SPH body forces at config-5 size ("SPH body forces").

Writes the frame of tools/neighbours_bench.py -- N rows, float32 mass, velocity, energy and position (uniform in a
triclinic box) -- to /dev/shm from the device, selects the rows of one cell of the 2x2x2 decomposition (about N / 8
entries: the accelerations' list) and splits it into a slab (the body: a fifth of the cell's width) and the rest (the
fluid), sorts both lists by cell for the grid `pgsd.hoomd.neighbour_grid_for` gives for the support ``2h`` (the
accelerations' frame and grid: tools/sph_forces_bench.py), and times, served from the staged rows on a warm page cache:
  * sph_body_force_device with the slab as the targets and the rest as the sources, for both kernels, with and without
    the viscous term (the frame stores neither density nor pressure: its float32 energy column stands in for the density
    chunk and its mass column for the pressure chunk, which costs the same arithmetic),
  * the same call with the whole list on both sides -- the accelerations' candidates and each entry itself --, beside
  * the yardstick: sph_accelerations_device over the whole list, the call whose pair loop this one shares.
``candidates`` is the number of (b, f) pairs the pair kernel visits, from the per-cell counts of the two ordered lists.
With ``--host`` also what the answer costs without the feature: a host read of the five chunks and
pgsd.hoomd.sph_body_force over a thin slab of targets, about ``--model-entries`` of them, against the rest, once; the GPU's
result over the same lists must equal it bit for bit.
``staged_ms`` is the median of ``--repeats`` calls with minimum and maximum.  One JSON line per call.  The kernels' own
times -- the pair kernel's, the reduction's, everything around them -- come from a separate run under ``rocprofv3
--kernel-trace --stats -- python tools/sph_body_force_bench.py --kernels-only``, which issues every call once.

    python tools/sph_body_force_bench.py [--n 80000000] [--h 0.0985] [--repeats 5] [--kernels-only] [--host] [--out FILE.jsonl]
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
from sph_sums_bench import bits_equal  # noqa: E402

MASS, VELOCITY, DENSITY, POSITION = NAMES       # (the energy column stands in for the density chunk)
PRESSURE = MASS                                 # (and the mass column for the pressure chunk)
VISCOSITY, ABOUT = 0.001, (5.0, 5.0, 5.0)


def candidates_between(count_t, count_s, grid):
    """The (b, f) pairs the pair kernel visits: per cell the targets' count times the sources' counts of the
    deduplicated adjacent cells (x fastest)."""
    t = np.asarray(count_t, dtype=np.float64).reshape(grid[2], grid[1], grid[0])
    s = np.asarray(count_s, dtype=np.float64).reshape(grid[2], grid[1], grid[0])
    around = np.zeros_like(s)
    offsets = [hoomd._axis_offsets(g) for g in grid]
    for oz in offsets[2]:
        for oy in offsets[1]:
            for ox in offsets[0]:
                around += np.roll(s, shift=(-oz, -oy, -ox), axis=(0, 1, 2))
    return int((t * around).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--h", type=float, default=0.0985, help="the smoothing length: 2h = 0.197, the census' range")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="issue every call once (for rocprofv3)")
    ap.add_argument("--host", action="store_true", help="also time the host read and the numpy model over a thin body, once")
    ap.add_argument("--model-entries", type=int, default=50_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = "/dev/shm/pgsd_sph_body_force_bench_%d.gsd" % os.getpid()
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
            def ordered(domains):
                """The rows of the domains as one list in cell order: (rows, cell, entries, per-cell counts, ms)."""
                parts = []
                for d in domains:
                    selected, m = f.select_domain_device(0, POSITION, BOX, d)
                    parts.append(selected[:m].clone())
                rows = parts[0] if len(parts) == 1 else torch.cat(parts)
                m = int(rows.shape[0])
                t, cell = timed(lambda: f.order_rows_by_cell_device(0, POSITION, BOX, grid, rows, n=m))
                return rows, cell, m, f.cell_moments_device(chunks, rows, cell, m, n_cells).count, t

            # warm: reader threads, pinned ring, kernels; all four chunks staged, which they stay until the wait at the end
            whole = ordered([hoomd.domain_grid(2, 2, 2)[0]])
            f.frame_moments_device([None] + chunks, rows=whole[0], n=whole[2])
            body = ordered([hoomd.Domain((0.2, 0.0, 0.0), (0.3, 0.5, 0.5))])
            fluid = ordered([hoomd.Domain((0.0, 0.0, 0.0), (0.2, 0.5, 0.5)), hoomd.Domain((0.3, 0.0, 0.0), (0.5, 0.5, 0.5))])
            base = {"N": a.n, "h": a.h, "support": support, "grid": list(grid), "n_cells": n_cells}
            say(dict(base, kind="order_rows_by_cell", rows=whole[2], staged_ms=round(whole[4], 3)))
            say(dict(base, kind="order_rows_by_cell", rows=body[2], staged_ms=round(body[4], 3), what="the body"))
            say(dict(base, kind="order_rows_by_cell", rows=fluid[2], staged_ms=round(fluid[4], 3), what="the fluid"))

            def accelerations(kernel, viscous):
                return f.sph_accelerations_device(0, POSITION, BOX, a.h, grid, whole[0], whole[1], n=whole[2],
                                                  velocity=(0, VELOCITY), mass=(0, MASS), density=(0, DENSITY),
                                                  pressure=(0, PRESSURE), viscosity=VISCOSITY if viscous else None, kernel=kernel)

            def forces(kernel, viscous, t, s, **kw):
                return f.sph_body_force_device(0, POSITION, BOX, a.h, grid, t[0], t[1], s[0], s[1], n_body=t[2], n_fluid=s[2],
                                               velocity=(0, VELOCITY), mass=(0, MASS), density=(0, DENSITY),
                                               pressure=(0, PRESSURE), viscosity=VISCOSITY if viscous else None, about=ABOUT,
                                               kernel=kernel, **kw)

            self_pairs = candidates_between(whole[3], whole[3], grid)
            for kernel in hoomd.SPH_KERNELS:
                record(dict(base, kind="sph_accelerations", kernel=kernel, viscous=True, rows=whole[2], candidates=self_pairs),
                       lambda kernel=kernel: accelerations(kernel, True).total2)
            for what, t, s in (("slab_and_rest", body, fluid), ("whole_list_both_sides", whole, whole)):
                pairs = candidates_between(t[3], s[3], grid)
                for kernel in hoomd.SPH_KERNELS:
                    for viscous in (True, False):
                        got = forces(kernel, viscous, t, s)
                        record(dict(base, kind="sph_body_force", lists=what, kernel=kernel, viscous=viscous, targets=t[2],
                                    sources=s[2], candidates=pairs, wetted=got.wetted, pairs=got.pairs, bad=got.bad,
                                    force=list(got.force), torque=list(got.torque)),
                               lambda kernel=kernel, viscous=viscous, t=t, s=s: forces(kernel, viscous, t, s).force[0])
            if a.host:
                # a thin slab of targets with about --model-entries rows against the fluid: lists the model finishes
                width = 0.1 * min(1.0, a.model_entries / max(body[2], 1))
                thin = ordered([hoomd.Domain((0.2, 0.0, 0.0), (0.2 + width, 0.5, 0.5))])
                t_read, arrays = timed(lambda: [f.read_chunk(0, name) for name in (POSITION, VELOCITY, MASS, DENSITY, PRESSURE)])
                b_rows, f_rows = thin[0][:thin[2]].cpu().numpy(), fluid[0][:fluid[2]].cpu().numpy()
                for kernel in hoomd.SPH_KERNELS:
                    t_gpu, small = timed(lambda: forces(kernel, True, thin, fluid, return_rows=True))
                    t_model, want = timed(lambda: hoomd.sph_body_force(arrays[0], arrays[1], BOX, a.h, b_rows, f_rows,
                                                                       mass=arrays[2], density=arrays[3], pressure=arrays[4],
                                                                       viscosity=VISCOSITY, about=ABOUT, cells=grid,
                                                                       kernel=kernel))
                    m = thin[2]
                    equal = bool(np.array_equal(want.summary[:9], small.summary[:9])
                                 and bits_equal(want.summary[9:].view(np.float64), small.summary[9:].view(np.float64))
                                 and np.array_equal(small.contacts[:m].cpu().numpy(), want.contacts)
                                 and bits_equal(small.pressure_acc[:m].cpu().numpy().ravel(), want.pressure_acc.ravel())
                                 and bits_equal(small.viscous_acc[:m].cpu().numpy().ravel(), want.viscous_acc.ravel()))
                    say(dict(base, kind="host_read_and_model", kernel=kernel, targets=m, sources=fluid[2],
                             candidates=candidates_between(thin[3], fluid[3], grid), read_ms=round(t_read, 1),
                             model_ms=round(t_model, 1), gpu_ms_same_lists=round(t_gpu, 3), equals_the_gpu=equal))
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
