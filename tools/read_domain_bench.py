"""Domain-decomposed restart against a row slab, at config-5 size ("Domain reads").

Writes an N-row frame (position, typeid, velocity, mass, image; positions uniform in a triclinic box) to /dev/shm
from the device, then times, each on a warm page cache:
  * read_frame_device(0, domain=d, scalar4=True) for every domain d of a 2x2x2 grid (rank 0 .. 7), and
  * read_frame_device(0, part=(r * N/8, N/8), scalar4=True) for the same ranks -- the slab read of config 5.
With ``--ghost WIDTH`` the selections alone are timed as well, for every domain: select_halo_device (the cell plus a
ghost layer of that width) beside select_domain_device of the same cell, each with the staging of the position chunk.
One JSON line per read.  The kernels' own times come from a separate run under
``rocprofv3 --kernel-trace --stats -- python tools/read_domain_bench.py --n ... --repeats 1``.

    python tools/read_domain_bench.py [--n 80000000] [--repeats 2] [--ghost WIDTH] [--out profiles/r06_read_domain.jsonl]
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


def write(path, N):
    g = torch.Generator(device="cuda").manual_seed(1)
    s = torch.rand((N, 3), generator=g, device="cuda", dtype=torch.float32) - 0.5
    Lx, Ly, Lz, xy, xz, yz = BOX
    pos4 = torch.empty((N, 4), dtype=torch.float32, device="cuda")
    pos4[:, 2] = s[:, 2] * Lz
    pos4[:, 1] = s[:, 1] * Ly + yz * pos4[:, 2]
    pos4[:, 0] = s[:, 0] * Lx + xy * pos4[:, 1] + xz * pos4[:, 2]
    pos4[:, 3] = torch.randint(0, 4, (N,), generator=g, device="cuda", dtype=torch.int32).view(torch.float32)
    del s
    vel4 = torch.randn((N, 4), generator=g, device="cuda")
    image = torch.randint(-2, 3, (N, 3), generator=g, device="cuda", dtype=torch.int32)
    with fl.open(path, "w", application="read_domain_bench", schema="hoomd", schema_version=[1, 4]) as f:
        f.write_chunk("configuration/step", np.array([0], dtype=np.uint64), write_all=False)
        f.write_chunk("configuration/box", np.array(BOX, dtype=np.float32), write_all=False)
        f.write_chunk("particles/N", np.array([N], dtype=np.uint32), write_all=False)
        f.write_chunks([("particles/position", fl.DeviceField.from_tensor(pos4, columns=(0, 3))),
                        ("particles/typeid", fl.DeviceField.from_tensor(pos4, columns=(3, 4), out_dtype=np.uint32,
                                                                        bitcast=True)),
                        ("particles/velocity", fl.DeviceField.from_tensor(vel4, columns=(0, 3))),
                        ("particles/mass", fl.DeviceField.from_tensor(vel4, columns=(3, 4))),
                        ("particles/image", fl.DeviceField.from_tensor(image))], offset=np.array([N]))
        f.end_frame()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--ghost", type=float, default=None, help="also time the halo selection with this layer width")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = "/dev/shm/pgsd_read_domain_bench_%d.gsd" % os.getpid()
    lines = []
    try:
        write(path, a.n)
        grid = hoomd.domain_grid(2, 2, 2)
        slab = a.n // 8
        with hoomd.open(path, "r") as t:
            t.read_frame_device(0, part=(0, slab), scalar4=True)       # warm: reader threads, pinned ring, arenas
            for rep in range(a.repeats):
                for rank, d in enumerate(grid):
                    for kind in ("domain", "slab"):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        if kind == "domain":
                            fr = t.read_frame_device(0, domain=d, scalar4=True)
                        else:
                            fr = t.read_frame_device(0, part=(rank * slab, slab), scalar4=True)
                        torch.cuda.synchronize()
                        ms = (time.perf_counter() - t0) * 1e3
                        rec = {"kind": kind, "rank": rank, "repeat": rep, "N": a.n, "rows": int(fr.particles.N),
                               "ms": round(ms, 2)}
                        lines.append(rec)
                        print(json.dumps(rec), flush=True)
                        del fr
            for rep in range(a.repeats if a.ghost is not None else 0):
                for rank, d in enumerate(grid):
                    for kind in ("select_halo", "select_domain"):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        if kind == "select_halo":
                            got = t.file.select_halo_device(0, "particles/position", BOX, d, a.ghost)
                            rows, ghosts = got[1] + got[2], got[2]
                        else:
                            rows, ghosts = t.file.select_domain_device(0, "particles/position", BOX, d)[1], 0
                        ms = (time.perf_counter() - t0) * 1e3
                        t.file.wait_read()                              # gives up the staged position rows
                        rec = {"kind": kind, "rank": rank, "repeat": rep, "N": a.n, "rows": int(rows),
                               "ghosts": int(ghosts), "ms": round(ms, 2)}
                        lines.append(rec)
                        print(json.dumps(rec), flush=True)
        for kind in ("domain", "slab") + (("select_halo", "select_domain") if a.ghost is not None else ()):
            ms = [r["ms"] for r in lines if r["kind"] == kind and r["repeat"] == a.repeats - 1]
            summary = {"kind": kind + "_summary", "N": a.n, "median_ms": float(np.median(ms)), "min_ms": min(ms),
                       "max_ms": max(ms)}
            lines.append(summary)
            print(json.dumps(summary), flush=True)
    finally:
        if os.path.exists(path):
            os.unlink(path)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
