"""Components at config-5 size ("Components").

The frame, the selection (one cell of the 2x2x2 decomposition, about N / 8 entries), the ordering and the grid are those of
tools/neighbour_list_bench.py.  Timed, served from the staged rows on a warm page cache:
  * pgsd_components_device over the sorted list (check, offsets, open, link, flatten, roots, scan, number and component
    kernels, the summary's copy), into outputs allocated once,
  * the yardstick: neighbours_device, the census, over the same list in the same process -- the same traversal over all
    the pairs with no union-find, so that components / census says what the atomics on the parent array cost over one
    bare traversal (the link kernel visits every candidate and unites half the pairs).
``staged_ms`` is the median of ``--repeats`` calls with minimum and maximum.  One JSON line per call, then the ratio and
the components found.  The kernels' own times come from a separate run under ``rocprofv3 --kernel-trace --stats -- python
tools/components_bench.py --kernels-only``, which issues every call once.

    python tools/components_bench.py [--n 80000000] [--r 0.197] [--repeats 5] [--kernels-only] [--out FILE.jsonl]
"""
import argparse
import ctypes
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
from pgsd import _lib  # noqa: E402
from cell_moments_bench import BOX, NAMES, timed, write  # noqa: E402
from neighbours_bench import candidates_of  # noqa: E402


def entry_point():
    D, U = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    fn = _lib.lib.pgsd_components_device
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.POINTER(_lib.Handle), ctypes.POINTER(_lib.IndexEntry), D, ctypes.c_double, ctypes.c_uint32, U,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--r", type=float, default=0.197, help="the range: about 40 neighbours per entry at the default size")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="issue every call once (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = "/dev/shm/pgsd_components_bench_%d.gsd" % os.getpid()
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
        fn = entry_point()
        with fl.open(path, "r") as f:
            # warm: reader threads, pinned ring, kernels; the row list of one cell; the position chunk staged, which it
            # stays until the wait at the end
            selected, count = f.select_domain_device(0, NAMES[3], BOX, hoomd.domain_grid(2, 2, 2)[0])
            rows = selected.clone()
            cell = f.order_rows_by_cell_device(0, NAMES[3], BOX, grid, rows, n=count)
            fields = f.cell_moments_device(chunks, rows, cell, count, n_cells)
            base = {"N": a.n, "rows": count, "r": a.r, "grid": list(grid), "n_cells": n_cells,
                    "candidates": candidates_of(fields.count, grid)}
            census = record(dict(base, kind="neighbours"),
                            lambda: int(f.neighbours_device(0, NAMES[3], BOX, a.r, grid, rows, cell, n=count).pairs))
            h = f._h()
            entry = _lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(h, 0, NAMES[3].encode()).contents)
            device = f.pipeline_device()
            label = fl.DeviceBuffer((max(count, 1),), np.uint32, device)
            component = fl.DeviceBuffer((max(count, 1),), np.uint32, device)
            sizes = fl.DeviceBuffer((max(count, 1),), np.uint32, device)
            summary = (ctypes.c_uint64 * 6)()
            args = (h, ctypes.byref(entry), (ctypes.c_double * 6)(*hoomd.box_vectors(np.asarray(BOX, np.float32))), a.r, 3,
                    (ctypes.c_uint32 * 3)(*grid), ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(cell.data_ptr()), count, 0,
                    ctypes.c_void_p(label.ptr), ctypes.c_void_p(component.ptr), ctypes.c_void_p(sizes.ptr), summary)

            def call():
                rc = fn(*args)
                assert rc == 0, _lib.last_error()
                return int(summary[2])

            got = record(dict(base, kind="components"), call)
            found = dict(nowhere=int(summary[1]), components=int(summary[2]), singletons=int(summary[3]),
                         largest=int(summary[4]), largest_label=int(summary[5]), pairs_of_the_census=census["value"])
            if a.kernels_only:
                say(dict(base, kind="found", **found))
            else:
                say(dict(base, kind="ratio", components_ms=got["staged_ms"], census_ms=census["staged_ms"],
                         components_over_census=round(got["staged_ms"] / census["staged_ms"], 3),
                         entries_per_s=float("%.4g" % (count / (got["staged_ms"] * 1e-3))), **found))
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
