"""Frame displacements against two yardsticks from the same run, at config-5 size ("Frame
displacements").

Writes a two-frame, N-row file to /dev/shm from the device -- float32 positions (uniform in a triclinic box; frame 1 moved
by a small normal step), int32 images, typeid in four long runs, and the mass, velocity and energy the yardstick needs --,
stages every chunk once and then times, served from the staged rows on a warm page cache:
  * frame_displacements_device over all rows: one group and four types, with images (48 and 52 bytes per row), without
    (24 and 28) and with the minimum image (28: three float64 divisions per row),
  * the same with images through the row list of one cell of the 2x2x2 grid (the gathered pass),
  * the yardsticks: frame_moments_device with one group over mass, velocity, energy and position (32 bytes per row:
    moments_tile_kernel, the memory-bound pass next door) and domain_counts_device of the 2x2x2 grid (12 bytes and three
    float64 divisions per row: domain_count_kernel).
``staged_ms`` is the median of ``--repeats`` calls -- the kernels, their launches, the copy of the result and one stream
wait --, with minimum and maximum; ``gbytes_per_s`` divides the chunk bytes the call reads by it.  One JSON line per
call.  The kernels' own times come from a separate run under ``rocprofv3 --kernel-trace --stats -- python
tools/frame_displacements_bench.py --kernels-only``, which stages once and issues every call once.

    python tools/frame_displacements_bench.py [--n 80000000] [--repeats 5] [--kernels-only] [--out FILE.jsonl]
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
POS, IMG, TID = "particles/position", "particles/image", "particles/typeid"
MOMENTS = [None, (0, "particles/mass"), (0, "particles/velocity"), (0, "particles/energy"), (0, POS)]


def write(path, N):
    g = torch.Generator(device="cuda").manual_seed(1)
    s = torch.rand((N, 3), generator=g, device="cuda", dtype=torch.float32) - 0.5
    Lx, Ly, Lz, xy, xz, yz = BOX
    pos = torch.empty((N, 3), dtype=torch.float32, device="cuda")
    pos[:, 2] = s[:, 2] * Lz
    pos[:, 1] = s[:, 1] * Ly + yz * pos[:, 2]
    pos[:, 0] = s[:, 0] * Lx + xy * pos[:, 1] + xz * pos[:, 2]
    del s
    image = torch.randint(-2, 3, (N, 3), generator=g, device="cuda", dtype=torch.int32)
    vel = torch.randn((N, 3), generator=g, device="cuda", dtype=torch.float32)
    mass = 0.5 + torch.rand((N,), generator=g, device="cuda", dtype=torch.float32)
    energy = 1.0 + 0.1 * torch.randn((N,), generator=g, device="cuda", dtype=torch.float32)
    # four runs; the ids travel as the bits of a float32 array, as HOOMD keeps them in position.w
    tid = (torch.arange(N, device="cuda", dtype=torch.int64) * 4 // max(N, 1)).to(torch.int32).view(torch.float32)
    with fl.open(path, "w", application="frame_displacements_bench", schema="hoomd", schema_version=[1, 4]) as f:
        f.write_chunk("configuration/step", np.array([0], dtype=np.uint64), write_all=False)
        f.write_chunk("configuration/box", np.array(BOX, dtype=np.float32), write_all=False)
        f.write_chunk("particles/N", np.array([N], dtype=np.uint32), write_all=False)
        f.write_chunks([(TID, fl.DeviceField.from_tensor(tid, out_dtype=np.uint32, bitcast=True)),
                        ("particles/mass", fl.DeviceField.from_tensor(mass)),
                        ("particles/velocity", fl.DeviceField.from_tensor(vel)),
                        ("particles/energy", fl.DeviceField.from_tensor(energy)),
                        (POS, fl.DeviceField.from_tensor(pos)), (IMG, fl.DeviceField.from_tensor(image))],
                       offset=np.array([N]))
        f.end_frame()
        torch.cuda.synchronize()
        del vel, mass, energy, tid
        pos += 0.05 * torch.randn((N, 3), generator=g, device="cuda", dtype=torch.float32)
        image += torch.randint(-1, 2, (N, 3), generator=g, device="cuda", dtype=torch.int32)
        f.write_chunk("configuration/step", np.array([1], dtype=np.uint64), write_all=False)
        f.write_chunks([(POS, fl.DeviceField.from_tensor(pos)), (IMG, fl.DeviceField.from_tensor(image))],
                       offset=np.array([N]))
        f.end_frame()
    torch.cuda.synchronize()


def calls(f, rows, count, N):
    """(kind, entries, chunk bytes read, call)"""
    v = hoomd.box_vectors(BOX)
    with_images = [(0, POS), (0, IMG), (1, POS), (1, IMG)]
    without = [(0, POS), None, (1, POS), None]

    def disp(chunks, typed, **kw):
        spec = chunks + [(0, TID) if typed else None]
        return lambda: float(f.frame_displacements_device(spec, v, v, n_types=4 if typed else 1, **kw).square[0])

    listed = dict(rows=rows, n=count)
    return [
        ("displacements_dense_1", N, 48 * N, disp(with_images, False)),
        ("displacements_dense_4", N, 52 * N, disp(with_images, True)),
        ("displacements_dense_1_no_images", N, 24 * N, disp(without, False)),
        ("displacements_dense_4_no_images", N, 28 * N, disp(without, True)),
        ("displacements_dense_4_minimum_image", N, 28 * N, disp(without, True, minimum_image=True)),
        ("displacements_cell_rows_1", count, 48 * count, disp(with_images, False, **listed)),
        ("displacements_cell_rows_4", count, 52 * count, disp(with_images, True, **listed)),
        ("moments_dense_1", N, 32 * N, lambda: float(f.frame_moments_device(MOMENTS).kinetic[0])),
        ("domain_counts", N, 12 * N, lambda: int(f.domain_counts_device(0, POS, BOX, (2, 2, 2), [[0.5], [0.5], [0.5]])[0][0])),
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
    path = "/dev/shm/pgsd_frame_displacements_bench_%d.gsd" % os.getpid()
    lines = []
    try:
        write(path, a.n)
        with fl.open(path, "r") as f:
            # warm: reader threads, pinned ring, kernels; the row list of one cell of frame 1 (a copy: the next
            # selection writes a list of its own); and every chunk staged, which they stay until the wait at the end
            rows, count = f.select_domain_device(1, POS, BOX, hoomd.domain_grid(2, 2, 2)[0])
            rows = rows.clone()
            t0 = time.perf_counter()
            f.frame_displacements_device([(0, POS), (0, IMG), (1, POS), (1, IMG), (0, TID)], hoomd.box_vectors(BOX),
                                         hoomd.box_vectors(BOX), n_types=4)
            staging_ms = (time.perf_counter() - t0) * 1e3
            f.frame_moments_device(MOMENTS)
            for kind, entries, nbytes, fn in calls(f, rows, count, a.n):
                rec = {"kind": kind, "N": a.n, "rows": entries, "bytes": nbytes}
                rec["value"] = fn()
                if not a.kernels_only:
                    staged = [timed(fn)[0] for _ in range(a.repeats)]
                    ms = float(np.median(staged))
                    rec.update(staged_ms=round(ms, 3), staged_min_ms=round(min(staged), 3),
                               staged_max_ms=round(max(staged), 3), gbytes_per_s=round(nbytes / ms / 1e6, 1))
                lines.append(rec)
                print(json.dumps(rec), flush=True)
            if not a.kernels_only:
                # what a loop over frames pays per frame: the origin's chunks come from the page cache again
                rec = {"kind": "first_call_with_staging", "N": a.n, "rows": a.n, "bytes": 52 * a.n,
                       "staged_ms": round(staging_ms, 3), "gbytes_per_s": round(40 * a.n / staging_ms / 1e6, 1),
                       "note": "40 bytes per row were read and copied (frame 1's position was staged by the selection)"}
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
