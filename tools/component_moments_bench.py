"""Component fields at config-5 size ("Component fields").

The frame, the selection (one cell of the 2x2x2 decomposition, about N / 8 entries) and the ordering are those of
tools/components_bench.py.  Two ranges over the same list:
  (a) ``--r`` (0.197): the frame is one component -- the long path, about n / 1024 piece sums added by one lane;
  (b) ``--r-dust`` (0.0576: a mean neighbour count near 1 at the default density): the list shatters into mostly singletons
      and pairs -- a wave walks up to 1024 piece starts per slab.
Per range, served from the staged rows on a warm page cache, into outputs allocated once:
  * pgsd_component_moments_device over the labels and ids of a components call (check, sort, offsets, verify, piece, long,
    flags and pick kernels, the summary's copy),
  * yardstick 1: pgsd_components_device on the same list,
  * yardstick 2: cell_moments_device over the same list sorted by its grid -- the same four chunks gathered through the
    same kind of segmented sum, with no sort and no displacement,
  * the combined call, HOOMDTrajectory.frame_component_moments_device with the same domain: selection, ordering, components,
    moments and the closing wait_read, every chunk staged anew.
``staged_ms`` is the median of ``--repeats`` calls with minimum and maximum.  One JSON line per call, then the ratios, the
components found and the histogram of their sizes.  The kernels' own times come from a separate run under ``rocprofv3
--kernel-trace --stats -- python tools/component_moments_bench.py --kernels-only``, which issues every call once.

    python tools/component_moments_bench.py [--n 80000000] [--r 0.197] [--r-dust 0.0576] [--repeats 5] [--kernels-only]
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
from components_bench import entry_point as components_entry_point  # noqa: E402


def entry_point():
    D, E = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_lib.IndexEntry)
    fn = _lib.lib.pgsd_component_moments_device
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.POINTER(_lib.Handle), E, E, E, E, D, D, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    return fn


def size_histogram(sizes):
    """Components of 1, 2, 3, 4, 5-8, 9-64, 65-1024 and more than 1024 entries."""
    edges = [1, 2, 3, 4, 5, 9, 65, 1025]
    names = ["1", "2", "3", "4", "5-8", "9-64", "65-1024", ">1024"]
    at = np.searchsorted(edges, sizes, side="right") - 1
    return dict(zip(names, np.bincount(at, minlength=len(names)).tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--r", type=float, default=0.197, help="(a): one component at the default size")
    ap.add_argument("--r-dust", type=float, default=0.0576, help="(b): a mean neighbour count near 1 at the default size")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="issue every call once (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = "/dev/shm/pgsd_component_moments_bench_%d.gsd" % os.getpid()
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
        domain = hoomd.domain_grid(2, 2, 2)[0]
        fn, fn_components = entry_point(), components_entry_point()
        vectors = (ctypes.c_double * 6)(*hoomd.box_vectors(np.asarray(BOX, np.float32)))
        defaults = (ctypes.c_double * 8)(1, 0, 0, 0, 0, 0, 0, 0)
        with fl.open(path, "r") as f:
            h = f._h()
            entries = [_lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(h, 0, name.encode()).contents) for name in NAMES]
            device = f.pipeline_device()
            selected, count = f.select_domain_device(0, NAMES[3], BOX, domain)
            selected = selected.clone()
            room = max(count, 1)
            label, component, sizes = [fl.DeviceBuffer((room,), np.uint32, device) for _ in range(3)]
            out = [fl.DeviceBuffer((room, w), dt, device) for w, dt in ((9, np.float64), (6, np.float64), (3, np.float64), (2, np.uint32))]
            found, summary = (ctypes.c_uint64 * 6)(), (ctypes.c_uint64 * 6)()
            for case, r in (("one_component", a.r), ("dust", a.r_dust)):
                grid = hoomd.neighbour_grid_for(BOX, r)
                n_cells = grid[0] * grid[1] * grid[2]
                rows = selected.clone()
                cell = f.order_rows_by_cell_device(0, NAMES[3], BOX, grid, rows, n=count)
                base = {"N": a.n, "rows": count, "case": case, "r": r, "grid": list(grid), "n_cells": n_cells}
                args_c = (h, ctypes.byref(entries[3]), vectors, r, 3, (ctypes.c_uint32 * 3)(*grid), ctypes.c_void_p(rows.data_ptr()),
                          ctypes.c_void_p(cell.data_ptr()), count, 0, ctypes.c_void_p(label.ptr), ctypes.c_void_p(component.ptr),
                          ctypes.c_void_p(sizes.ptr), found)

                def call_components():
                    rc = fn_components(*args_c)
                    assert rc == 0, _lib.last_error()
                    return int(found[2])

                yard_c = record(dict(base, kind="components"), call_components)
                components = int(found[2])
                yard_m = record(dict(base, kind="cell_moments"),
                                lambda: float(f.cell_moments_device(chunks, rows, cell, count, n_cells).mass.sum()))
                args_m = (h, ctypes.byref(entries[0]), ctypes.byref(entries[1]), ctypes.byref(entries[2]), ctypes.byref(entries[3]),
                          defaults, vectors, 3, ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(label.ptr),
                          ctypes.c_void_p(component.ptr), count, components, 0, *[ctypes.c_void_p(o.ptr) for o in out], summary)

                def call_moments():
                    rc = fn(*args_m)
                    assert rc == 0, _lib.last_error()
                    return [int(v) for v in summary]

                mine = record(dict(base, kind="component_moments", components=components), call_moments)
                host_sizes = sizes.view(shape=(components,)).to_host()
                say(dict(base, kind="found", components=components, singletons=int(found[3]), largest=int(found[4]),
                         bad=int(summary[2]), wide=int(summary[3]), heaviest=int(summary[4]), widest=int(summary[5]),
                         mean_size=round(count / max(components, 1), 3), sizes=size_histogram(host_sizes)))
                if not a.kernels_only:
                    say(dict(base, kind="ratio", component_moments_ms=mine["staged_ms"], components_ms=yard_c["staged_ms"],
                             cell_moments_ms=yard_m["staged_ms"],
                             over_components=round(mine["staged_ms"] / yard_c["staged_ms"], 3),
                             over_cell_moments=round(mine["staged_ms"] / yard_m["staged_ms"], 3),
                             entries_per_s=float("%.4g" % (count / (mine["staged_ms"] * 1e-3)))))
            f.wait_read()
        # the combined call: selection, ordering, components, moments and the closing wait_read, every chunk staged anew
        with hoomd.open(path, "r") as t:
            for case, r in (("one_component", a.r), ("dust", a.r_dust)):
                record({"N": a.n, "case": case, "r": r, "kind": "frame_component_moments_device"},
                       lambda: int(t.frame_component_moments_device(0, r, domain=domain).components))
    finally:
        if os.path.exists(path):
            os.unlink(path)
    if a.out:
        with open(a.out, "w") as out:
            for r in lines:
                out.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
