"""The domain census against a domain selection, at config-5 size ("Domain census").

Writes an N-row position chunk (uniform in a triclinic box, or -- ``clustered`` -- every particle in one eighth of it)
to /dev/shm from the device, then times on a warm page cache, per distribution:
  * axis_histograms_device at 1024 and 4096 bins,
  * domain_counts_device for 2x2x2 and 8x8x8 cells,
  * select_domain_device of one cell of the 2x2x2 grid (its count pass makes the same single pass over the chunk).
Every call is timed twice: ``first_ms`` with the staging of the position chunk (pread, host-to-device), and
``staged_ms``, the median of ``--repeats`` calls served from the rows the first left staged -- the kernels, their
launches, the copy of the result and one stream wait.  One JSON line per call.  The kernels' own times come from a
separate run under ``rocprofv3 --kernel-trace --stats -- python tools/domain_census_bench.py --kernels-only``, which
stages once per distribution and issues every call once.

    python tools/domain_census_bench.py [--n 80000000] [--repeats 5] [--kernels-only] [--out profiles/r10_domain_census_bench.jsonl]
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


def write(path, N, clustered):
    g = torch.Generator(device="cuda").manual_seed(1)
    s = torch.rand((N, 3), generator=g, device="cuda", dtype=torch.float32)
    s = s * 0.5 - 0.5 if clustered else s - 0.5      # fractions [0, 1/2) of every axis: one cell of the 2x2x2 grid
    Lx, Ly, Lz, xy, xz, yz = BOX
    pos = torch.empty((N, 3), dtype=torch.float32, device="cuda")
    pos[:, 2] = s[:, 2] * Lz
    pos[:, 1] = s[:, 1] * Ly + yz * pos[:, 2]
    pos[:, 0] = s[:, 0] * Lx + xy * pos[:, 1] + xz * pos[:, 2]
    del s
    with fl.open(path, "w", application="domain_census_bench", schema="hoomd", schema_version=[1, 4]) as f:
        f.write_chunk("configuration/step", np.array([0], dtype=np.uint64), write_all=False)
        f.write_chunk("configuration/box", np.array(BOX, dtype=np.float32), write_all=False)
        f.write_chunk("particles/N", np.array([N], dtype=np.uint32), write_all=False)
        f.write_chunks([("particles/position", fl.DeviceField.from_tensor(pos))], offset=np.array([N]))
        f.end_frame()
    torch.cuda.synchronize()


def calls(f):
    name = "particles/position"
    inner2 = [[0.5]] * 3
    inner8 = [[k / 8 for k in range(1, 8)]] * 3
    cell = hoomd.domain_grid(2, 2, 2)[0]
    return [
        ("hist_1024", lambda: int(f.domain_histogram_device(0, name, BOX, 1024)[0].sum())),
        ("hist_4096", lambda: int(f.domain_histogram_device(0, name, BOX, 4096)[0].sum())),
        ("counts_2x2x2", lambda: int(f.domain_counts_device(0, name, BOX, (2, 2, 2), inner2)[0].max())),
        ("counts_8x8x8", lambda: int(f.domain_counts_device(0, name, BOX, (8, 8, 8), inner8)[0].max())),
        ("select_domain", lambda: int(f.select_domain_device(0, name, BOX, cell)[1])),
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
    path = "/dev/shm/pgsd_domain_census_bench_%d.gsd" % os.getpid()
    lines = []
    try:
        for dist in ("uniform", "clustered"):
            write(path, a.n, dist == "clustered")
            with fl.open(path, "r") as f:
                f.domain_histogram_device(0, "particles/position", BOX, 64)  # warm: reader threads, pinned ring, kernels
                f.wait_read()
                if a.kernels_only:
                    for kind, fn in calls(f):
                        rec = {"kind": kind, "dist": dist, "N": a.n, "value": fn()}
                        lines.append(rec)
                        print(json.dumps(rec), flush=True)
                    f.wait_read()
                    continue
                for kind, fn in calls(f):
                    first, value = timed(fn)
                    staged = [timed(fn)[0] for _ in range(a.repeats)]
                    f.wait_read()                                           # gives up the staged position rows
                    rec = {"kind": kind, "dist": dist, "N": a.n, "value": value, "first_ms": round(first, 3),
                           "staged_ms": round(float(np.median(staged)), 3), "staged_min_ms": round(min(staged), 3)}
                    lines.append(rec)
                    print(json.dumps(rec), flush=True)
            os.unlink(path)
    finally:
        if os.path.exists(path):
            os.unlink(path)
    if a.out:
        with open(a.out, "w") as out:
            for r in lines:
                out.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
