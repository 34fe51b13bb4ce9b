"""Cell-ordered domain reads against plain ones, at config-5 size ("Cell order").

Writes an N-row frame (position, typeid, velocity, mass, image; positions uniform in a triclinic box, rows in random
order like a tag-ordered file after many steps) to /dev/shm from the device, then times on a warm page cache, for one
cell of a 2x2x2 grid (an eighth of the rows) and the cell grids 64^3 and 1024^3:
  * ``order``: order_rows_by_cell_device over the selection's row list, served from the position rows the selection left
    staged -- key kernel, sort passes, apply kernel, one stream wait; every repeat sorts a fresh copy of the list;
  * ``read``: the whole read_frame_device(0, domain=d, scalar4=True, cell_order=c), beside the same read with
    cell_order=None from the same run.
Each figure is the median of ``--repeats`` calls, with their minimum and maximum: the spread.  ``--baseline`` times only
the read without cell_order and uses nothing this feature added, so the same file of this tool measures the parent
commit's tree.  One JSON line per figure.  The kernels' own times come from a separate run under
``rocprofv3 --kernel-trace --stats -- python tools/cell_order_bench.py --kernels-only``, which selects once and orders
once per grid.

    python tools/cell_order_bench.py [--n 80000000] [--repeats 5] [--baseline | --kernels-only] [--out FILE.jsonl]
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
GRIDS = [(64, 64, 64), (1024, 1024, 1024)]


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
    with fl.open(path, "w", application="cell_order_bench", schema="hoomd", schema_version=[1, 4]) as f:
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


def spread(kind, N, rows, ms, **more):
    rec = {"kind": kind, "N": N, "rows": int(rows), "median_ms": round(float(np.median(ms)), 3),
           "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "repeats": len(ms)}
    rec.update(more)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline", action="store_true", help="only the read without cell_order (runs on the parent commit)")
    ap.add_argument("--kernels-only", action="store_true", help="select once, order once per grid (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = "/dev/shm/pgsd_cell_order_bench_%d.gsd" % os.getpid()
    name = "particles/position"
    lines = []
    try:
        write(path, a.n)
        d = hoomd.domain_grid(2, 2, 2)[0]
        with hoomd.open(path, "r") as t:
            f = t.file
            t.read_frame_device(0, part=(0, a.n // 8), scalar4=True)       # warm: reader threads, pinned ring, arenas
            if a.kernels_only:
                rows, count = f.select_domain_device(0, name, BOX, d)
                for cells in GRIDS:
                    cell = f.order_rows_by_cell_device(0, name, BOX, cells, rows.clone())
                    rec = {"kind": "order", "cells": list(cells), "N": a.n, "rows": count, "last_cell": int(cell[-1])}
                    lines.append(rec)
                    print(json.dumps(rec), flush=True)
                f.wait_read()
            else:
                if not a.baseline:
                    rows, count = f.select_domain_device(0, name, BOX, d)
                    for cells in GRIDS:
                        f.order_rows_by_cell_device(0, name, BOX, cells, rows.clone())     # warm: scratch space, kernels
                        ms = []
                        for _ in range(a.repeats):
                            work = rows.clone()
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            f.order_rows_by_cell_device(0, name, BOX, cells, work)
                            ms.append((time.perf_counter() - t0) * 1e3)
                        lines.append(spread("order", a.n, count, ms, cells=list(cells)))
                    f.wait_read()                                               # gives up the staged position rows
                    del rows, work
                for cells in [None] + ([] if a.baseline else GRIDS):
                    kw = {} if cells is None else {"cell_order": cells}
                    t.read_frame_device(0, domain=d, scalar4=True, **kw)        # warm
                    ms = []
                    for _ in range(a.repeats):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fr = t.read_frame_device(0, domain=d, scalar4=True, **kw)
                        torch.cuda.synchronize()
                        ms.append((time.perf_counter() - t0) * 1e3)
                        count = int(fr.particles.N)
                        del fr
                    lines.append(spread("read", a.n, count, ms, cells=None if cells is None else list(cells)))
    finally:
        if os.path.exists(path):
            os.unlink(path)
    if a.out:
        with open(a.out, "w") as out:
            for r in lines:
                out.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
