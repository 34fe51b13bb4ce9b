"""Group reads against reading everything and masking, at config-5 size ("Group reads").

Writes an N-row frame (position, typeid, velocity, mass, density, image; positions uniform in a triclinic box, four
types of equal share) to /dev/shm from the device, then times, each on a warm page cache, three groups:
  * typeid      where={'typeid': [0, 1]}                            (half of the rows)
  * density     where={'typeid': [0, 1], 'density': (0.0, None)}    (a quarter)
  * domain      where={'typeid': [0, 1]}, domain = a cell of a 2x2x2 grid  (a sixteenth)
and for each
  * select      select_where_device alone (staging of the terms' chunks + the three kernels), and beside it
                select_domain_device of the same cell;
  * where       read_frame_device(0, where=..., [domain=...,] scalar4=True), and
  * mask        read_frame_device(0, part=(0, N), scalar4=True), the predicate in torch on the GPU, every array indexed
                by the mask -- what a caller does without where=.
One JSON line per measurement.  The kernels' own times come from a separate run under
``rocprofv3 --kernel-trace --stats -- python tools/read_where_bench.py --n ... --repeats 1 --select-only``.

    python tools/read_where_bench.py [--n 80000000] [--repeats 3] [--out profiles/r08_read_where_bench.jsonl]
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
ARRAYS = ('position', 'typeid', 'velocity', 'mass', 'density', 'image')


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
    density = torch.randn((N,), generator=g, device="cuda")
    image = torch.randint(-2, 3, (N, 3), generator=g, device="cuda", dtype=torch.int32)
    with fl.open(path, "w", application="read_where_bench", schema="hoomd", schema_version=[1, 4]) as f:
        f.write_chunk("configuration/step", np.array([0], dtype=np.uint64), write_all=False)
        f.write_chunk("configuration/box", np.array(BOX, dtype=np.float32), write_all=False)
        f.write_chunk("particles/N", np.array([N], dtype=np.uint32), write_all=False)
        f.write_chunks([("particles/position", fl.DeviceField.from_tensor(pos4, columns=(0, 3))),
                        ("particles/typeid", fl.DeviceField.from_tensor(pos4, columns=(3, 4), out_dtype=np.uint32,
                                                                        bitcast=True)),
                        ("particles/velocity", fl.DeviceField.from_tensor(vel4, columns=(0, 3))),
                        ("particles/mass", fl.DeviceField.from_tensor(vel4, columns=(3, 4))),
                        ("particles/density", fl.DeviceField.from_tensor(density)),
                        ("particles/image", fl.DeviceField.from_tensor(image))], offset=np.array([N]))
        f.end_frame()
    torch.cuda.synchronize()


def masked(t, N, where, domain):
    """The baseline: the whole frame into HBM, the predicate in torch, every array indexed by the mask."""
    fr = t.read_frame_device(0, part=(0, N), scalar4=True)
    p = fr.particles
    keep = (p.typeid == 0) | (p.typeid == 1)
    if 'density' in where:
        keep &= p.density >= 0.0
    if domain is not None:
        Lx, Ly, Lz, xy, xz, yz = (float(v) for v in np.asarray(BOX, np.float32))
        x, y, z = (p.position[:, a].double() for a in range(3))
        s = [((x + Lx / 2) - ((xz - yz * xy) * z + xy * y)) / Lx, ((y + Ly / 2) - yz * z) / Ly, (z + Lz / 2) / Lz]
        for a in range(3):
            f = s[a] - torch.floor(s[a])
            f[f >= 1.0] = 0.0
            keep &= (domain.lo[a] <= f) & (f < domain.hi[a])
        del x, y, z, s, f
    out = dict((name, getattr(p, name)[keep]) for name in ARRAYS + ('pos4', 'vel4'))
    return int(keep.sum()), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--select-only", action="store_true", help="the selections alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = "/dev/shm/pgsd_read_where_bench_%d.gsd" % os.getpid()
    cell = hoomd.domain_grid(2, 2, 2)[5]
    groups = [("typeid", {'typeid': [0, 1]}, None),
              ("density", {'typeid': [0, 1], 'density': (0.0, None)}, None),
              ("domain", {'typeid': [0, 1]}, cell)]
    lines = []

    def timed(kind, group, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = fn()
        torch.cuda.synchronize()
        rec = {"kind": kind, "group": group, "N": a.n, "rows": rows, "ms": round((time.perf_counter() - t0) * 1e3, 2)}
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    try:
        write(path, a.n)
        with hoomd.open(path, "r") as t:
            f = t.file
            t.read_frame_device(0, part=(0, a.n // 8), scalar4=True)       # warm: reader threads, pinned ring, arenas
            for rep in range(a.repeats):
                for group, where, domain in groups:
                    terms = [(0, 'particles/' + name, 0, value) for name, value in where.items()]
                    dom = None if domain is None else (0, 'particles/position', domain)

                    def select():
                        n = f.select_where_device(terms, domain=dom, box=BOX)[1]
                        f.wait_read()
                        return n

                    timed("select", group, select)
                    if domain is not None:
                        def select_domain():
                            n = f.select_domain_device(0, 'particles/position', BOX, domain)[1]
                            f.wait_read()
                            return n

                        timed("select_domain_alone", group, select_domain)
                    if a.select_only:
                        continue
                    timed("where", group,
                          lambda: int(t.read_frame_device(0, where=where, domain=domain, scalar4=True).particles.N))
                    timed("mask", group, lambda: masked(t, a.n, where, domain)[0])
        for kind in sorted(set(r["kind"] for r in lines)):
            for group, _, _ in groups:
                ms = [r["ms"] for r in lines if r["kind"] == kind and r["group"] == group][1:] or \
                     [r["ms"] for r in lines if r["kind"] == kind and r["group"] == group]
                if ms:
                    summary = {"kind": kind + "_summary", "group": group, "N": a.n, "median_ms": float(np.median(ms)),
                               "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}
                    lines.append(summary)
                    print(json.dumps(summary), flush=True)
    finally:
        if os.path.exists(path):
            os.unlink(path)
    if a.out:
        with open(a.out, "w") as out:
            for r in lines:
                out.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
