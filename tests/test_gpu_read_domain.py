"""Domain-decomposed restart: read_frame_device(domain=...) selects a rank's particles on the GPU from the frame's
effective position and box and gathers every per-particle array through that row list (pgsd_select_domain_device,
pgsd_read_rows_device).  The selection must equal pgsd.hoomd.domain_rows -- the numpy model -- exactly, and every array
the host reader's frame indexed by those rows, byte for byte.  Files are written through the host path."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)      # triclinic; every value a short binary fraction
GRIDS = {
    "1x1x1": hoomd.domain_grid(1, 1, 1),
    "2x2x2": hoomd.domain_grid(2, 2, 2),
    "3x1x2": hoomd.domain_grid(3, 1, 2, x_split=[0.25, 0.5], z_split=[0.375]),
}
SIZES = [1, 1000, 70_001, 3_000_001]
PLANES = (0.0, 0.25, 0.375, 0.5, 0.75)     # every split plane of GRIDS (and the box faces)


def _on_planes(rng, n):
    """Positions whose fractional coordinates are exactly split-plane values: all float32 and float64 operations of the
    predicate are exact on them, so each sits exactly on a plane (or a box face)."""
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in BOX)
    s = rng.choice(PLANES, size=(n, 3)) + rng.integers(-1, 2, size=(n, 3))     # and periodic images of them
    z = (s[:, 2] - 0.5) * Lz
    y = (s[:, 1] - 0.5) * Ly + yz * z
    x = (s[:, 0] - 0.5) * Lx + xz * z + xy * y
    p = np.stack([x, y, z], axis=1)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32)


def _frame(rng, N, pos=None, typeid=None):
    fr = hoomd.Frame()
    fr.configuration.step = 10
    fr.configuration.box = BOX
    fr.particles.N = N
    fr.particles.types = ['A', 'B', 'C']
    if pos is None:
        pos = rng.uniform(-3.0, 3.0, size=(N, 3)).astype(np.float32)
        k = min(N, 4096)
        pos[:k] = _on_planes(rng, k)
    fr.particles.position = pos
    fr.particles.typeid = rng.integers(0, 3, size=N).astype(np.uint32) if typeid is None else typeid
    fr.particles.velocity = rng.standard_normal((N, 3)).astype(np.float32)
    fr.particles.mass = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
    fr.particles.image = rng.integers(-3, 4, size=(N, 3)).astype(np.int32)
    fr.particles.density = rng.standard_normal(N).astype(np.float32)
    fr.particles.orientation = rng.standard_normal((N, 4)).astype(np.float32)
    return fr


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Per N: frame 0; frame 1 elides position and typeid (equal to frame 0's); frame 2 elides typeid only."""
    d = "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp("dom"))
    out = {}
    for N in SIZES:
        rng = np.random.default_rng(N)
        path = os.path.join(d, "pgsd_domain_%d_%d.gsd" % (os.getpid(), N))
        f0 = _frame(rng, N)
        with hoomd.open(path, 'w') as t:
            t.append(f0)
            t.append(_frame(rng, N, pos=f0.particles.position, typeid=f0.particles.typeid))
            t.append(_frame(rng, N, typeid=f0.particles.typeid))
        with fl.open(path, 'r') as f:
            assert not f.chunk_exists(1, 'particles/position') and not f.chunk_exists(1, 'particles/typeid')
            assert f.chunk_exists(2, 'particles/position') and not f.chunk_exists(2, 'particles/typeid')
        out[N] = path
    yield out
    for p in out.values():
        os.unlink(p)


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _same(dev, host):
    a, b = np.ascontiguousarray(_host(dev)), np.ascontiguousarray(host)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_domain(t, host, idx, d, N):
    s = t.read_frame_device(idx, domain=d, scalar4=True)
    rows = hoomd.domain_rows(host.particles.position, host.configuration.box, d)
    tag = _host(s.tag)
    assert tag.dtype == np.int32 and np.array_equal(tag, rows)
    assert s.particles.N == len(rows) and s.particles.N_global == N
    for name in ('position', 'typeid', 'velocity', 'mass', 'image', 'density', 'orientation', 'body', 'slength',
                 'auxiliary1'):
        assert _same(getattr(s.particles, name), getattr(host.particles, name)[rows]), name
    pos4 = np.concatenate([host.particles.position[rows], host.particles.typeid[rows].view(np.float32)[:, None]], 1)
    vel4 = np.concatenate([host.particles.velocity[rows], host.particles.mass[rows][:, None]], 1)
    assert _same(s.particles.pos4, pos4) and _same(s.particles.vel4, vel4)
    return rows


@pytest.mark.parametrize("N", SIZES)
def test_domains_of_every_grid_match_the_model_and_the_host_frame(files, N):
    with hoomd.open(files[N], 'r') as t:
        for idx in range(3) if N < 3_000_000 else (0, 1):
            host = t[idx]
            for name, grid in GRIDS.items():
                got = [_check_domain(t, host, idx, d, N) for d in grid]
                assert np.array_equal(np.sort(np.concatenate(got)), np.arange(N)), (idx, name)


def test_empty_domains_give_zero_row_arrays(files):
    with hoomd.open(files[1], 'r') as t:
        host = t[0]
        empty = [d for d in GRIDS["2x2x2"] if len(hoomd.domain_rows(host.particles.position, BOX, d)) == 0]
        assert len(empty) == 7
        for d in empty:
            s = t.read_frame_device(0, domain=d, scalar4=True)
            assert s.particles.N == 0 and s.particles.N_global == 1 and s.tag.numel() == 0
            assert tuple(s.particles.position.shape) == (0, 3) and tuple(s.particles.pos4.shape) == (0, 4)
            assert tuple(s.particles.mass.shape) == (0,)


def test_domain_and_part_are_exclusive_and_bad_domains_raise(files):
    with hoomd.open(files[1000], 'r') as t:
        with pytest.raises(ValueError):
            t.read_frame_device(0, part=(0, 10), domain=GRIDS["1x1x1"][0])
        with pytest.raises(ValueError):
            t.read_frame_device(0, domain=((0, 0, 0), (1, 1, 1.5)))
        with pytest.raises(ValueError):
            t.file.select_domain_device(0, 'particles/position', [0, 1, 1, 0, 0, 0], GRIDS["1x1x1"][0])
        with pytest.raises(ValueError):
            t.file.select_domain_device(0, 'particles/mass', BOX, GRIDS["1x1x1"][0])      # not N x 3


def test_slab_reads_are_unchanged_after_domain_reads(files):
    with hoomd.open(files[70_001], 'r') as t:
        host = t[1]
        t.read_frame_device(1, domain=GRIDS["2x2x2"][3])
        s = t.read_frame_device(1, part=(1000, 5000), scalar4=True)
        assert s.particles.N == 5000 and not hasattr(s, 'tag')
        assert _same(s.particles.position, host.particles.position[1000:6000])
        assert _same(s.particles.typeid, host.particles.typeid[1000:6000])
        t.read_frame_device(1, domain=GRIDS["2x2x2"][4])
        again = t.read_frame_device(1, part=(1000, 5000))
        assert _same(again.particles.position, host.particles.position[1000:6000])


@pytest.mark.parametrize("N", [1000, 70_001, 3_000_001])
def test_read_chunk_device_rows_equals_fancy_indexing(files, N):
    g = torch.Generator(device="cuda").manual_seed(N)
    flags = (torch.rand(N, generator=g, device="cuda") < 0.3).to(torch.uint8)
    rows, n = fl.select_rows(flags)
    r = rows.cpu().numpy()
    with hoomd.open(files[N], 'r') as t:
        host = t[0]
        f = t.file
        assert _same(f.read_chunk_device(0, 'particles/image', rows=rows), host.particles.image[r])
        assert _same(f.read_chunk_device(0, 'particles/orientation', rows=rows), host.particles.orientation[r])
        dens = torch.empty((n,), dtype=torch.float64, device="cuda")
        f.read_chunk_device(0, 'particles/density', out=dens, rows=rows)
        assert _same(dens, host.particles.density[r].astype(np.float64))
        # a Scalar4 destination: xyz + typeid bits in one wait, whole rows; and xyz alone with a fill
        pos4 = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        f.read_chunk_device(0, 'particles/position', out=pos4, columns=(0, 3), rows=rows, wait=False)
        f.read_chunk_device(0, 'particles/typeid', out=pos4, columns=(3, 4), bitcast=True, rows=rows, wait=False)
        f.wait_read()
        want = np.concatenate([host.particles.position[r], host.particles.typeid[r].view(np.float32)[:, None]], 1)
        assert _same(pos4, want)
        vel4 = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        f.read_chunk_device(0, 'particles/velocity', out=vel4, columns=(0, 3), rows=rows, fill=1.0)
        want = np.concatenate([host.particles.velocity[r], np.ones((n, 1), np.float32)], 1)
        assert _same(vel4, want)
        # a prefix of the list, into a float64 Scalar4 (conversion on the row-per-lane path)
        pos4d = torch.empty((n // 2, 4), dtype=torch.float64, device="cuda")
        f.read_chunk_device(0, 'particles/position', out=pos4d, columns=(0, 3), rows=rows, N=n // 2, fill=0.0)
        want = np.concatenate([host.particles.position[r[:n // 2]], np.zeros((n // 2, 1))], 1).astype(np.float64)
        assert _same(pos4d, want)
        with pytest.raises(ValueError):
            f.read_chunk_device(0, 'particles/mass', rows=rows, offset=1)


def test_selection_reuses_the_staged_position_rows(files):
    """An indexed read of the position chunk right after its selection: served from the rows the selection staged."""
    N = 3_000_001
    with hoomd.open(files[N], 'r') as t:
        host = t[0]
        f = t.file
        d = GRIDS["3x1x2"][4]
        rows, n = f.select_domain_device(0, 'particles/position', BOX, d)
        out = f.read_chunk_device(0, 'particles/position', rows=rows)
        r = hoomd.domain_rows(host.particles.position, BOX, d)
        assert n == len(r) and np.array_equal(rows.cpu().numpy(), r)
        assert _same(out, host.particles.position[r])


CHILD = r'''
import os, pickle, sys
sys.modules["torch"] = None                    # `import torch` raises ImportError from here on
root, path, out_path = sys.argv[1:4]
sys.path[:0] = [os.path.join(root, "pgsd-sph_amd"), os.path.join(root, "tests")]
import numpy as np
import pgsd.fl as fl
import pgsd.hoomd as hoomd
from pgsd import _lib
assert _lib._torch is None
grid = hoomd.domain_grid(3, 1, 2, x_split=[0.25, 0.5], z_split=[0.375])
res = []
with hoomd.open(path, 'r') as t:
    for idx in (0, 1):
        for d in grid:
            s = t.read_frame_device(idx, domain=d, scalar4=True)
            assert isinstance(s.tag, fl.DeviceBuffer)
            res.append((idx, d.lo, d.hi, s.tag.to_host(), s.particles.position.to_host(), s.particles.pos4.to_host(),
                        s.particles.image.to_host()))
pickle.dump(res, open(out_path, "wb"))
'''


def test_domain_read_without_torch(files, tmp_path):
    N = 70_001
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, files[N], str(out)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))
    with hoomd.open(files[N], 'r') as t:
        hosts = {0: t[0], 1: t[1]}
    union = {0: [], 1: []}
    for idx, lo, hi, tag, pos, pos4, image in res:
        h = hosts[idx]
        rows = hoomd.domain_rows(h.particles.position, h.configuration.box, hoomd.Domain(lo, hi))
        assert tag.dtype == np.int32 and np.array_equal(tag, rows)
        assert pos.tobytes() == h.particles.position[rows].tobytes()
        assert image.tobytes() == h.particles.image[rows].tobytes()
        assert pos4[:, 3].view(np.uint32).tobytes() == h.particles.typeid[rows].tobytes()
        union[idx].append(tag)
    for idx in (0, 1):
        assert np.array_equal(np.sort(np.concatenate(union[idx])), np.arange(N))
