"""Particle tracks against whole-chunk indexed reads, at config-5 size ("Tracks").

Writes an N-row frame (position, velocity) to /dev/shm from the device, then times, each on a warm page cache and five
times (min / median / max):
  * tracks:  read_tracks_device(rows, fields=(position, velocity)) per frame for K = 10^3, 10^5, 10^7 uniformly random
             rows and 10^7 rows in one contiguous range, with the file bytes read, the touched blocks T and the plan time;
  * whole:   the same rows through read_chunk_device(rows=tensor) -- the route that stages whole chunks.  With
             ``--pkg DIR`` the package is imported from DIR (a build of another commit: the parent's numbers);
  * sweep_r: the sparse route at R = 256 ... 16384 rows per block for K = 10^3 and 10^5;
  * sweep_f: sparse against whole at touched fractions 0.01 ... 1.0 (contiguous clusters of rows) at the current R.
One JSON line per measurement.  The kernels' own times come from a separate run under
``rocprofv3 --kernel-trace --stats -- python tools/read_tracks_bench.py --what tracks --repeats 1``.

    python tools/read_tracks_bench.py [--n 80000000] [--what tracks,whole,sweep_r,sweep_f] [--out FILE] [--pkg DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--what", default="tracks,whole,sweep_r,sweep_f")
    ap.add_argument("--out", default=None)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "pgsd-sph_amd"))
    ap.add_argument("--label", default="this")
    return ap.parse_args()


A = _args()
sys.path.insert(0, A.pkg)

import torch  # noqa: E402

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402
from pgsd import _lib  # noqa: E402

FIELDS = ("position", "velocity")
LINES = []


def emit(rec):
    rec = dict(label=A.label, N=A.n, **rec)
    LINES.append(rec)
    print(json.dumps(rec), flush=True)


def write(path, N):
    g = torch.Generator(device="cuda").manual_seed(1)
    pos = torch.rand((N, 3), generator=g, device="cuda", dtype=torch.float32)
    vel = torch.randn((N, 3), generator=g, device="cuda")
    with fl.open(path, "w", application="read_tracks_bench", schema="hoomd", schema_version=[1, 4]) as f:
        f.write_chunk("configuration/step", np.array([0], dtype=np.uint64), write_all=False)
        f.write_chunk("particles/N", np.array([N], dtype=np.uint32), write_all=False)
        f.write_chunks([("particles/position", fl.DeviceField.from_tensor(pos)),
                        ("particles/velocity", fl.DeviceField.from_tensor(vel))], offset=np.array([N]))
        f.end_frame()
    torch.cuda.synchronize()


def row_sets(N):
    rng = np.random.default_rng(3)
    sets = {}
    for K in (10**3, 10**5, 10**7):
        if K <= N:
            sets["random_%d" % K] = rng.integers(0, N, size=K)
    K = min(10**7, N)
    sets["contiguous_%d" % K] = np.arange(N // 3, N // 3 + K) % N
    return sets


def clusters(N, fraction, n_clusters=16, step=64):
    """Every `step`-th row of n_clusters contiguous ranges that cover `fraction` of the rows."""
    width = max(int(N * fraction / n_clusters), 1)
    starts = (np.arange(n_clusters) * (N // n_clusters)).astype(np.int64)
    return np.concatenate([np.arange(s, min(s + width, N), step) for s in starts])


def dev_rows(r):
    return torch.from_numpy(np.asarray(r, dtype=np.int64).astype(np.int32)).cuda()


def timed(fn, repeats):
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(ms), 3), "median_ms": round(float(np.median(ms)), 3), "max_ms": round(max(ms), 3),
            "repeats": repeats}


def read_pair(f, rows, outs):
    for name, out in zip(FIELDS, outs):
        f.read_chunk_device(0, "particles/" + name, out=out, rows=rows, wait=False)
    f.wait_read()


def stats(f):
    return f.device_read_stats(reset=True)["pread_bytes"] if hasattr(f, "device_read_stats") else None


def main():
    what = A.what.split(",")
    path = "/dev/shm/pgsd_read_tracks_bench_%d.gsd" % os.getpid()
    N = A.n
    try:
        write(path, N)
        with hoomd.open(path, "r") as t:
            f = t.file
            f.read_chunk_device(0, "particles/position", N=min(N, 1 << 20))     # warm: reader threads, ring, arenas
            for name, r in row_sets(N).items():
                d = dev_rows(r)
                outs = [torch.empty((len(r), 3), dtype=torch.float32, device="cuda") for _ in FIELDS]
                if "whole" in what:
                    read_pair(f, d, outs)
                    stats(f)
                    rec = timed(lambda: read_pair(f, d, outs), A.repeats)
                    b = stats(f)
                    emit(dict(kind="whole", rows=name, K=len(r), pread_bytes=None if b is None else b // A.repeats, **rec))
                if "tracks" in what:
                    t.read_tracks_device(d, frames=[0], fields=FIELDS)
                    plan_ms = timed(lambda: f.plan_rows(d, N), A.repeats)
                    plan = f.plan_rows(d, N)
                    stats(f)
                    frames = [0, 0, 0, 0]
                    rec = timed(lambda: t.read_tracks_device(d, frames=frames, fields=FIELDS), A.repeats)
                    b = stats(f)
                    for k in ("min_ms", "median_ms", "max_ms"):
                        rec[k] = round(rec[k] / len(frames), 3)
                    emit(dict(kind="tracks", rows=name, K=len(r), per="frame", R=plan.block_rows, T=plan.touched_blocks,
                              runs=plan.runs, sparse=bool(plan.sparse), plan_median_ms=plan_ms["median_ms"],
                              pread_bytes=b // (A.repeats * len(frames)), **rec))
                del outs
            if "sweep_r" in what:
                for K in (10**3, 10**5):
                    r = np.random.default_rng(3).integers(0, N, size=K)
                    d = dev_rows(r)
                    outs = [torch.empty((K, 3), dtype=torch.float32, device="cuda") for _ in FIELDS]
                    for R in (256, 1024, 4096, 16384):
                        os.environ["PGSD_PLAN_BLOCK_ROWS"] = str(R)
                        _lib.lib.pgsd_reload_tuning()
                        plan = f.plan_rows(d, N, threshold=1.0)
                        read_pair(f, plan, outs)
                        stats(f)
                        rec = timed(lambda: read_pair(f, plan, outs), A.repeats)
                        emit(dict(kind="sweep_r", K=K, R=R, T=plan.touched_blocks, runs=plan.runs,
                                  pread_bytes=stats(f) // A.repeats, **rec))
                    os.environ.pop("PGSD_PLAN_BLOCK_ROWS")
                    _lib.lib.pgsd_reload_tuning()
            if "sweep_f" in what:
                for fraction in (0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0):
                    r = clusters(N, fraction)
                    d = dev_rows(r)
                    outs = [torch.empty((len(r), 3), dtype=torch.float32, device="cuda") for _ in FIELDS]
                    for route, thr in (("sparse", 1.0), ("whole", -1.0)):
                        plan = f.plan_rows(d, N, threshold=thr)
                        read_pair(f, plan, outs)
                        stats(f)
                        rec = timed(lambda: read_pair(f, plan, outs), A.repeats)
                        emit(dict(kind="sweep_f", fraction=fraction, route=route, K=len(r), R=plan.block_rows,
                                  T=plan.touched_blocks, touched_fraction=round(plan.touched_fraction, 4),
                                  pread_bytes=stats(f) // A.repeats, **rec))
    finally:
        if os.path.exists(path):
            os.unlink(path)
    if A.out:
        with open(A.out, "a") as fo:
            for r in LINES:
                fo.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
