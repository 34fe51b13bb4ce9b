"""Cell fields against the conservation sums over the same gathered rows, at config-5 size ("Cell
fields").

Writes an N-row frame -- float32 mass, velocity, energy and position (uniform in a triclinic box) -- to /dev/shm from the
device, selects the rows of one cell of the 2x2x2 decomposition, and per grid sorts a copy of that row list by cell and
times, served from the staged rows on a warm page cache:
  * cell_moments_device over the sorted list (check, offsets, piece and long kernels, the copy of the result table),
  * yardstick 1: frame_moments_device with one group over the same sorted list -- the same bytes through the same index,
  * the ordering itself, order_rows_by_cell_device, which the hoomd-level call pays once before the sums.
With ``--host`` also yardstick 2, what the answer costs without the feature: a host read of the four chunks and
pgsd.hoomd.cell_moments over the same list, once.
``staged_ms`` is the median of ``--repeats`` calls with minimum and maximum; ``ratio`` divides the cell fields' median by
yardstick 1's.  One JSON line per call.  The kernels' own times come from a separate run under ``rocprofv3
--kernel-trace --stats -- python tools/cell_moments_bench.py --kernels-only``, which issues every call once per grid.

    python tools/cell_moments_bench.py [--n 80000000] [--repeats 5] [--kernels-only] [--host] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pgsd-sph_amd"))

import torch  # noqa: E402

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402

BOX = [40.0, 40.0, 40.0, 0.25, 0.125, -0.0625]
NAMES = ["particles/mass", "particles/velocity", "particles/energy", "particles/position"]
GRIDS = [(8, 8, 8), (64, 64, 64), (128, 128, 64)]


def write(path, N):
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
    with fl.open(path, "w", application="cell_moments_bench", schema="hoomd", schema_version=[1, 4]) as f:
        f.write_chunk("configuration/step", np.array([0], dtype=np.uint64), write_all=False)
        f.write_chunk("configuration/box", np.array(BOX, dtype=np.float32), write_all=False)
        f.write_chunk("particles/N", np.array([N], dtype=np.uint32), write_all=False)
        f.write_chunks([(NAMES[0], fl.DeviceField.from_tensor(mass)), (NAMES[1], fl.DeviceField.from_tensor(vel)),
                        (NAMES[2], fl.DeviceField.from_tensor(energy)), (NAMES[3], fl.DeviceField.from_tensor(pos))],
                       offset=np.array([N]))
        f.end_frame()
    torch.cuda.synchronize()


def timed(fn):
    t0 = time.perf_counter()
    value = fn()
    return (time.perf_counter() - t0) * 1e3, value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="issue every call once per grid (for rocprofv3)")
    ap.add_argument("--host", action="store_true", help="also time the host read and the numpy model, once, at 64^3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = "/dev/shm/pgsd_cell_moments_bench_%d.gsd" % os.getpid()
    lines = []

    def record(rec, fn):
        rec["value"] = fn()
        if not a.kernels_only:
            staged = [timed(fn)[0] for _ in range(a.repeats)]
            rec.update(staged_ms=round(float(np.median(staged)), 3), staged_min_ms=round(min(staged), 3),
                       staged_max_ms=round(max(staged), 3))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        return rec

    try:
        write(path, a.n)
        chunks = [(0, name) for name in NAMES]
        with fl.open(path, "r") as f:
            # warm: reader threads, pinned ring, kernels; the row list of one cell; all four chunks staged, which they
            # stay until the wait at the end
            selected, count = f.select_domain_device(0, NAMES[3], BOX, hoomd.domain_grid(2, 2, 2)[0])
            selected = selected.clone()
            f.frame_moments_device([None] + chunks, rows=selected, n=count)
            for grid in GRIDS:
                n_cells = grid[0] * grid[1] * grid[2]
                rows = selected.clone()
                t_order, cell = timed(lambda: f.order_rows_by_cell_device(0, NAMES[3], BOX, grid, rows, n=count))
                base = {"N": a.n, "rows": count, "grid": list(grid), "n_cells": n_cells, "bytes": 32 * count}
                got = f.cell_moments_device(chunks, rows, cell, count, n_cells)
                base["occupied"] = int((got.count > 0).sum())
                base["largest_cell"] = int(got.count.max())
                lines.append(dict(base, kind="order_rows_by_cell", staged_ms=round(t_order, 3)))
                print(json.dumps(lines[-1]), flush=True)
                yard = record(dict(base, kind="moments_sorted_rows_1"),
                              lambda: float(f.frame_moments_device([None] + chunks, rows=rows, n=count).kinetic[0]))
                mine = record(dict(base, kind="cell_moments"),
                              lambda: float(f.cell_moments_device(chunks, rows, cell, count, n_cells).kinetic.sum()))
                if not a.kernels_only:
                    mine["ratio"] = round(mine["staged_ms"] / yard["staged_ms"], 2)
                    print(json.dumps({"kind": "ratio", "grid": list(grid), "ratio": mine["ratio"]}), flush=True)
                if a.host and grid == (64, 64, 64):
                    t0 = time.perf_counter()
                    host = [f.read_chunk(0, name) for name in NAMES]
                    t_read = (time.perf_counter() - t0) * 1e3
                    h_rows, h_cell = rows[:count].cpu().numpy(), cell[:count].cpu().numpy()
                    t_model, want = timed(lambda: hoomd.cell_moments(host[0], host[1], host[2], host[3], cell=h_cell,
                                                                     n_cells=n_cells, rows=h_rows))
                    equal = bool(np.array_equal(want.sums.view(np.uint64), got.sums.view(np.uint64))
                                 and np.array_equal(want.count, got.count) and np.array_equal(want.bad, got.bad))
                    lines.append(dict(base, kind="host_read_and_model", read_ms=round(t_read, 1), model_ms=round(t_model, 1),
                                      equals_the_gpu=equal))
                    print(json.dumps(lines[-1]), flush=True)
                    del host
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
