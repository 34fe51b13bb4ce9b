"""Neighbour lists at config-5 size ("Neighbour lists").

The frame, the selection (one cell of the 2x2x2 decomposition, about N / 8 entries), the ordering and the grid are those of
tools/neighbours_bench.py.  Timed, served from the staged rows on a warm page cache:
  * pgsd_neighbour_offsets_device over the sorted list (check, offsets, compaction, count, scan and offsets kernels, the
    summary's copy),
  * pgsd_neighbour_list_device into segments allocated once for the pairs the first call reported (check, offsets,
    compaction, the fill kernel, the copy of the mismatch word and of offsets[n]),
  * the yardstick: neighbours_device, the census, over the same list -- the same traversal with no list output, so that
    (offsets + fill) / census says what the variable-length output costs over two bare traversals.
``staged_ms`` is the median of ``--repeats`` calls with minimum and maximum; the fill's record adds the pairs written per
second and the bytes per second its stores move (4 bytes per pair, 12 with ``--distances``).  One JSON line per call.  The
kernels' own times come from a separate run under ``rocprofv3 --kernel-trace --stats -- python
tools/neighbour_list_bench.py --kernels-only``, which issues every call once.

    python tools/neighbour_list_bench.py [--n 80000000] [--r 0.197] [--repeats 5] [--half] [--distances] [--kernels-only]
                                         [--out FILE.jsonl]
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


def entry_points():
    D, U = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    head = [ctypes.POINTER(_lib.Handle), ctypes.POINTER(_lib.IndexEntry), D, ctypes.c_double, ctypes.c_uint32, U,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]
    offsets_fn, fill_fn = _lib.lib.pgsd_neighbour_offsets_device, _lib.lib.pgsd_neighbour_list_device
    offsets_fn.restype = fill_fn.restype = ctypes.c_int32
    offsets_fn.argtypes = head + [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    fill_fn.argtypes = head + [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return offsets_fn, fill_fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--r", type=float, default=0.197, help="the range: about 40 neighbours per entry at the default size")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--half", action="store_true", help="the half list: j > i by list position")
    ap.add_argument("--distances", action="store_true", help="also store the squared distance of every pair")
    ap.add_argument("--kernels-only", action="store_true", help="issue every call once (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = "/dev/shm/pgsd_neighbour_list_bench_%d.gsd" % os.getpid()
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
        offsets_fn, fill_fn = entry_points()
        with fl.open(path, "r") as f:
            # warm: reader threads, pinned ring, kernels; the row list of one cell; the position chunk staged, which it
            # stays until the wait at the end
            selected, count = f.select_domain_device(0, NAMES[3], BOX, hoomd.domain_grid(2, 2, 2)[0])
            rows = selected.clone()
            cell = f.order_rows_by_cell_device(0, NAMES[3], BOX, grid, rows, n=count)
            fields = f.cell_moments_device(chunks, rows, cell, count, n_cells)
            base = {"N": a.n, "rows": count, "r": a.r, "grid": list(grid), "n_cells": n_cells, "half": a.half,
                    "distances": a.distances, "candidates": candidates_of(fields.count, grid)}
            census = record(dict(base, kind="neighbours"),
                            lambda: int(f.neighbours_device(0, NAMES[3], BOX, a.r, grid, rows, cell, n=count).pairs))
            h = f._h()
            entry = _lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(h, 0, NAMES[3].encode()).contents)
            head = (h, ctypes.byref(entry), (ctypes.c_double * 6)(*hoomd.box_vectors(np.asarray(BOX, np.float32))), a.r, 3,
                    (ctypes.c_uint32 * 3)(*grid), ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(cell.data_ptr()), count,
                    1 if a.half else 0)
            device = f.pipeline_device()
            offsets = fl.DeviceBuffer((count + 1,), np.uint64, device)
            summary = (ctypes.c_uint64 * 4)()

            def call_offsets():
                rc = offsets_fn(*(head + (ctypes.c_void_p(offsets.ptr), summary)))
                assert rc == 0, _lib.last_error()
                return int(summary[2])

            first = record(dict(base, kind="neighbour_offsets"), call_offsets)
            pairs = first["value"]
            base.update(pairs=pairs, longest=int(summary[3]), nowhere=int(summary[1]),
                        list_bytes=hoomd.neighbour_list_bytes(count, pairs, a.distances))
            neighbours = fl.DeviceBuffer((max(pairs, 1),), np.uint32, device)
            distance2 = fl.DeviceBuffer((max(pairs, 1),), np.float64, device) if a.distances else None

            def call_fill():
                rc = fill_fn(*(head + (ctypes.c_void_p(offsets.ptr), pairs, ctypes.c_void_p(neighbours.ptr),
                                       ctypes.c_void_p(distance2.ptr) if a.distances else None)))
                assert rc == 0, _lib.last_error()
                return pairs

            second = record(dict(base, kind="neighbour_list"), call_fill)
            if not a.kernels_only:
                both = first["staged_ms"] + second["staged_ms"]
                per_pair = 12 if a.distances else 4
                say(dict(base, kind="ratio", offsets_ms=first["staged_ms"], fill_ms=second["staged_ms"],
                         census_ms=census["staged_ms"], list_over_census=round(both / census["staged_ms"], 3),
                         pairs_per_s_of_the_fill=float("%.4g" % (pairs / (second["staged_ms"] * 1e-3))),
                         pairs_per_s_of_both_calls=float("%.4g" % (pairs / (both * 1e-3))),
                         store_bytes_per_pair=per_pair,
                         store_bytes_per_s_of_the_fill=float("%.4g" % (per_pair * pairs / (second["staged_ms"] * 1e-3)))))
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
