#!/usr/bin/env python3
"""One small-N point per family of GPU passes over staged chunks: where the launchers' host side dominates.

Writes a 4096-row frame (position, typeid, mass, velocity, energy) to /dev/shm through the host path, then times -- on the
host clock, around the synchronising call, chunks staged by the warm-up calls -- pgsd_select_rows, the domain, halo and
group selections, an axis histogram, a cell count, a cell ordering, chunk statistics, conservation sums and a row plan:
20 warm-up calls, then the median, 10th and 90th percentile of ``--repeats`` calls.  One JSON line per call.  ``--root``
names the tree whose built package is measured (default: this one), ``--label`` goes into the records: a second checkout
of another commit, built, is measured by the same file of this tool.

    python tools/small_n_bench.py [--root TREE] [--label NAME] [--n 4096] [--repeats 400]
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--repeats", type=int, default=400)
args = ap.parse_args()
root, label = args.root, args.label
sys.path.insert(0, os.path.join(root, "pgsd-sph_amd"))
import numpy as np
import pgsd.fl as fl
import pgsd.hoomd as hoomd
from pgsd import _lib
assert os.path.dirname(_lib.LIB_PATH).startswith(os.path.abspath(root)), _lib.LIB_PATH
N, REPS = args.n, args.repeats
TRI = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
rng = np.random.default_rng(5)
path = "/dev/shm/pgsd_small_n_%d.gsd" % os.getpid()
A = {'pos': rng.uniform(-3, 3, size=(N, 3)).astype(np.float32), 'tid': (np.arange(N) % 4).astype(np.uint32).reshape(N, 1),
     'm': rng.uniform(0.5, 2, size=(N, 1)).astype(np.float32), 'v': rng.standard_normal((N, 3)).astype(np.float32),
     'e': rng.standard_normal((N, 1)).astype(np.float32)}
with fl.open(path, 'w', application="bench", schema="none", schema_version=[1, 0]) as f:
    for k, a in A.items():
        f.write_chunk(k, a)
    f.end_frame()
cell = hoomd.domain_grid(2, 2, 2)[3]
inner = [b[1:-1] for b in hoomd.grid_bounds(4, 4, 4)]
def timed(name, call):
    for _ in range(20):
        call()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); call(); ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e6
    print(json.dumps({"tool": "small_n", "lib": label, "call": name, "N": N, "median_us": round(float(np.median(ts)), 1),
                      "p10_us": round(float(np.percentile(ts, 10)), 1), "p90_us": round(float(np.percentile(ts, 90)), 1)}), flush=True)
with fl.open(path, 'r') as f:
    dev = f.pipeline_device()
    flags = fl._device_from_host((rng.random(N) < 0.5).astype(np.uint8), dev)
    rows = fl._device_from_host(rng.integers(0, N, size=N).astype(np.int32), dev)
    timed("select_rows", lambda: fl.select_rows(flags))
    timed("select_domain", lambda: f.select_domain_device(0, 'pos', TRI, cell))
    timed("select_halo", lambda: f.select_halo_device(0, 'pos', TRI, cell, 0.3))
    timed("select_where", lambda: f.select_where_device([(0, 'tid', 0, [0, 2])]))
    timed("histogram_1024", lambda: f.domain_histogram_device(0, 'pos', TRI, 1024))
    timed("counts_4x4x4", lambda: f.domain_counts_device(0, 'pos', TRI, (4, 4, 4), inner))
    timed("order_64^3", lambda: f.order_rows_by_cell_device(0, 'pos', TRI, (64, 64, 64), rows))
    timed("chunk_stats", lambda: f.chunk_stats_device(0, 'v', norm2=True))
    timed("frame_moments", lambda: f.frame_moments_device([(0, k) for k in ('tid', 'm', 'v', 'e', 'pos')], n_types=4))
    vectors = hoomd.box_vectors(TRI)
    timed("frame_displacements", lambda: f.frame_displacements_device([(0, 'pos'), None, (0, 'pos'), None, (0, 'tid')], vectors,
                                                                     vectors, n_types=4))
    timed("plan_rows", lambda: f.plan_rows(rows, N))
    f.wait_read()
os.unlink(path)
