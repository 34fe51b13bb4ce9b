"""Frame statistics against a domain selection, at config-5 size ("Frame statistics").

Writes an N-row frame -- the float32 position chunk (uniform in a triclinic box) and a one-column float32 density
chunk -- to /dev/shm from the device, then times on a warm page cache:
  * chunk_stats_device over the whole position chunk, with and without the norm column (the dense pass, N x 12 bytes),
  * chunk_stats_device over the whole density chunk (the dense pass over one column),
  * chunk_stats_device of the position chunk through the row list of one cell of the 2x2x2 grid (the gathered pass),
  * select_domain_device of that cell: the yardstick, whose count pass makes the same single pass over the position chunk.
Every call is timed twice: ``first_ms`` with the staging of the chunk (pread, host-to-device), and ``staged_ms``, the
median of ``--repeats`` calls served from the rows the first left staged -- the kernels, their launches, the copy of the
result and one stream wait --, with their minimum and maximum.  One JSON line per call.  The kernels' own times come
from a separate run under ``rocprofv3 --kernel-trace --stats -- python tools/frame_stats_bench.py --kernels-only``,
which stages once and issues every call once.

    python tools/frame_stats_bench.py [--n 80000000] [--repeats 5] [--kernels-only] [--out profiles/r12_frame_stats_bench.jsonl]
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
POSITION, DENSITY = "particles/position", "particles/density"


def write(path, N):
    g = torch.Generator(device="cuda").manual_seed(1)
    s = torch.rand((N, 3), generator=g, device="cuda", dtype=torch.float32) - 0.5
    Lx, Ly, Lz, xy, xz, yz = BOX
    pos = torch.empty((N, 3), dtype=torch.float32, device="cuda")
    pos[:, 2] = s[:, 2] * Lz
    pos[:, 1] = s[:, 1] * Ly + yz * pos[:, 2]
    pos[:, 0] = s[:, 0] * Lx + xy * pos[:, 1] + xz * pos[:, 2]
    del s
    rho = 1000.0 + 50.0 * torch.randn((N,), generator=g, device="cuda", dtype=torch.float32)
    with fl.open(path, "w", application="frame_stats_bench", schema="hoomd", schema_version=[1, 4]) as f:
        f.write_chunk("configuration/step", np.array([0], dtype=np.uint64), write_all=False)
        f.write_chunk("configuration/box", np.array(BOX, dtype=np.float32), write_all=False)
        f.write_chunk("particles/N", np.array([N], dtype=np.uint32), write_all=False)
        f.write_chunks([(POSITION, fl.DeviceField.from_tensor(pos)), (DENSITY, fl.DeviceField.from_tensor(rho))],
                       offset=np.array([N]))
        f.end_frame()
    torch.cuda.synchronize()


def calls(f, rows, count):
    cell = hoomd.domain_grid(2, 2, 2)[0]
    return [
        ("stats_position_norm2", lambda: float(f.chunk_stats_device(0, POSITION, norm2=True).max[3])),
        ("stats_position", lambda: float(f.chunk_stats_device(0, POSITION).sum[0])),
        ("stats_density", lambda: float(f.chunk_stats_device(0, DENSITY).sum[0])),
        ("stats_position_cell_rows", lambda: float(f.chunk_stats_device(0, POSITION, rows=rows, n=count, norm2=True).sum[0])),
        ("select_domain", lambda: int(f.select_domain_device(0, POSITION, BOX, cell)[1])),
    ]


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
    path = "/dev/shm/pgsd_frame_stats_bench_%d.gsd" % os.getpid()
    lines = []
    try:
        write(path, a.n)
        with fl.open(path, "r") as f:
            # warm: reader threads, pinned ring, kernels; and the row list of one cell (a copy: the next selection
            # writes a list of its own)
            rows, count = f.select_domain_device(0, POSITION, BOX, hoomd.domain_grid(2, 2, 2)[0])
            rows = rows.clone()
            f.chunk_stats_device(0, DENSITY)
            f.wait_read()
            for kind, fn in calls(f, rows, count):
                rec = {"kind": kind, "N": a.n, "rows": count if kind.endswith("_rows") else a.n}
                if a.kernels_only:
                    rec["value"] = fn()
                else:
                    first, rec["value"] = timed(fn)
                    staged = [timed(fn)[0] for _ in range(a.repeats)]
                    rec.update(first_ms=round(first, 3), staged_ms=round(float(np.median(staged)), 3),
                               staged_min_ms=round(min(staged), 3), staged_max_ms=round(max(staged), 3))
                    f.wait_read()                                           # gives up the staged rows
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
