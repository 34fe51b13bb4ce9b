"""Conservation sums against the statistics passes over the same bytes, at config-5 size (DESIGN.md section 8,
"Conservation sums").

Writes an N-row frame -- float32 typeid (four types in long runs, as real files hold them), mass, velocity, energy and
position (uniform in a triclinic box) -- to /dev/shm from the device, stages the five chunks once and then times, served
from the staged rows on a warm page cache:
  * frame_moments_device over all rows with one group and no typeid (32 bytes per row) and with four types (36 bytes),
  * the same through the row list of one cell of the 2x2x2 grid (the gathered pass),
  * the yardstick, what the same bytes cost before: chunk_stats_device over each of the five chunks (velocity and position
    with the norm column), whose sum ``stats_sum`` is reported as a record of its own, and select_domain_device of the
    cell, the single pass over the position chunk that the statistics were measured against.
``staged_ms`` is the median of ``--repeats`` calls -- the kernels, their launches, the copy of the result and one stream
wait --, with minimum and maximum; ``gbytes_per_s`` divides the chunk bytes the call reads by it.  One JSON line per
call.  The kernels' own times come from a separate run under ``rocprofv3 --kernel-trace --stats -- python
tools/frame_moments_bench.py --kernels-only``, which stages once and issues every call once.

    python tools/frame_moments_bench.py [--n 80000000] [--repeats 5] [--kernels-only] [--out profiles/r13_frame_moments_bench.jsonl]
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
NAMES = ["particles/typeid", "particles/mass", "particles/velocity", "particles/energy", "particles/position"]
ROW_BYTES = [4, 4, 12, 4, 12]


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
    # four runs; the ids travel as the bits of a float32 array, as HOOMD keeps them in position.w
    tid = (torch.arange(N, device="cuda", dtype=torch.int64) * 4 // max(N, 1)).to(torch.int32).view(torch.float32)
    with fl.open(path, "w", application="frame_moments_bench", schema="hoomd", schema_version=[1, 4]) as f:
        f.write_chunk("configuration/step", np.array([0], dtype=np.uint64), write_all=False)
        f.write_chunk("configuration/box", np.array(BOX, dtype=np.float32), write_all=False)
        f.write_chunk("particles/N", np.array([N], dtype=np.uint32), write_all=False)
        f.write_chunks([(NAMES[0], fl.DeviceField.from_tensor(tid, out_dtype=np.uint32, bitcast=True)),
                        (NAMES[1], fl.DeviceField.from_tensor(mass)), (NAMES[2], fl.DeviceField.from_tensor(vel)),
                        (NAMES[3], fl.DeviceField.from_tensor(energy)), (NAMES[4], fl.DeviceField.from_tensor(pos))],
                       offset=np.array([N]))
        f.end_frame()
    torch.cuda.synchronize()


def calls(f, rows, count, N):
    """(kind, entries, chunk bytes read, call)"""
    cell = hoomd.domain_grid(2, 2, 2)[0]
    chunks = [(0, name) for name in NAMES]
    untyped = [None] + chunks[1:]
    out = [
        ("moments_dense_1", N, 32 * N, lambda: float(f.frame_moments_device(untyped).kinetic[0])),
        ("moments_dense_4", N, 36 * N, lambda: float(f.frame_moments_device(chunks, n_types=4).kinetic[0])),
        ("moments_cell_rows_1", count, 32 * count, lambda: float(f.frame_moments_device(untyped, rows=rows, n=count).kinetic[0])),
        ("moments_cell_rows_4", count, 36 * count,
         lambda: float(f.frame_moments_device(chunks, n_types=4, rows=rows, n=count).kinetic[0])),
    ]
    for name, row_bytes in zip(NAMES, ROW_BYTES):
        out.append(("stats_" + name.split('/')[1], N, row_bytes * N,
                    lambda name=name, norm2=row_bytes == 12: float(f.chunk_stats_device(0, name, norm2=norm2).sum[0])))
    out.append(("select_domain", N, 12 * N, lambda: int(f.select_domain_device(0, NAMES[4], BOX, cell)[1])))
    return out


def timed(fn):
    t0 = time.perf_counter()
    value = fn()
    return (time.perf_counter() - t0) * 1e3, value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="stage once, issue every call once (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = "/dev/shm/pgsd_frame_moments_bench_%d.gsd" % os.getpid()
    lines = []
    try:
        write(path, a.n)
        with fl.open(path, "r") as f:
            # warm: reader threads, pinned ring, kernels; the row list of one cell (a copy: the next selection writes a
            # list of its own); and all five chunks staged, which they stay until the wait at the end
            rows, count = f.select_domain_device(0, NAMES[4], BOX, hoomd.domain_grid(2, 2, 2)[0])
            rows = rows.clone()
            t0 = time.perf_counter()
            f.frame_moments_device([(0, name) for name in NAMES], n_types=4)
            staging_ms = (time.perf_counter() - t0) * 1e3
            stats_sum = 0.0
            for kind, entries, nbytes, fn in calls(f, rows, count, a.n):
                rec = {"kind": kind, "N": a.n, "rows": entries, "bytes": nbytes}
                if a.kernels_only:
                    rec["value"] = fn()
                else:
                    rec["value"] = fn()
                    staged = [timed(fn)[0] for _ in range(a.repeats)]
                    ms = float(np.median(staged))
                    rec.update(staged_ms=round(ms, 3), staged_min_ms=round(min(staged), 3),
                               staged_max_ms=round(max(staged), 3), gbytes_per_s=round(nbytes / ms / 1e6, 1))
                    if kind.startswith("stats_"):
                        stats_sum += ms
                lines.append(rec)
                print(json.dumps(rec), flush=True)
            if not a.kernels_only:
                rec = {"kind": "stats_sum", "N": a.n, "rows": a.n, "bytes": 36 * a.n, "staged_ms": round(stats_sum, 3),
                       "gbytes_per_s": round(36 * a.n / stats_sum / 1e6, 1), "first_moments_call_with_staging_ms": round(staging_ms, 3)}
                lines.append(rec)
                print(json.dumps(rec), flush=True)
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
