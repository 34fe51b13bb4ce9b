"""Domain reads with a ghost layer: read_frame_device(domain=..., ghost=...) selects a cell's own particles and the
halo its neighbours reach on the GPU (pgsd_select_halo_device) and gathers every per-particle array through the
concatenated row list.  Rows, counts and shifts must equal pgsd.hoomd.halo_rows -- the numpy model -- exactly, planes
included, and every array the host reader's frame indexed by those rows, byte for byte.  Files are written through the
host path."""
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
GRIDS = {
    "1x1x1": hoomd.domain_grid(1, 1, 1),
    "2x2x2": hoomd.domain_grid(2, 2, 2),
    "3x1x2": hoomd.domain_grid(3, 1, 2),
    "unequal": hoomd.domain_grid(3, 1, 2, x_split=[0.25, 0.5], z_split=[0.375]),
}
# one lane, one partial block, exactly one selection block, one row past it, 17 blocks and a ragged one, many blocks
SIZES = [1, 1000, 4096, 4097, 70_001, 3_000_001]
# kind -> (box, ghost width).  ortho: every particle on the 1/64 lattice of fractions, the layer 1/16 of the box: all
# bounds are lattice points, every operation is exact, particles sit exactly on lo - g, lo, hi, hi + g, 0 and the
# wrapped bounds.  tri: random particles; the width keeps 2 g <= 1 - (hi - lo) for every cell above (gz = 0.125)
KINDS = {
    "ortho": (np.array([16.0, 16.0, 16.0, 0.0, 0.0, 0.0], np.float32), 1.0),
    "tri": (np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32), 0.25),
}
FIELDS = ('position', 'typeid', 'velocity', 'mass', 'image', 'density', 'energy', 'body', 'slength', 'auxiliary1')


def _positions(rng, kind, N):
    if kind == "tri":
        return rng.uniform(-3.0, 3.0, size=(N, 3)).astype(np.float32)
    k = rng.integers(0, 64, size=(N, 3))
    k[:64] = np.arange(64)[:min(N, 64), None]               # every lattice value on every axis
    p = (k / 64.0 + rng.integers(-1, 2, size=(N, 3)) - 0.5) * 16.0     # ... in the box or a periodic image
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32)


def _frame(rng, kind, N, pos, typeid=None):
    fr = hoomd.Frame()
    fr.configuration.step = 10
    fr.configuration.box = KINDS[kind][0]
    fr.particles.N = N
    fr.particles.types = ['A', 'B', 'C']
    fr.particles.position = pos
    fr.particles.typeid = rng.integers(0, 3, size=N).astype(np.uint32) if typeid is None else typeid
    fr.particles.velocity = rng.standard_normal((N, 3)).astype(np.float32)
    fr.particles.mass = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
    # the same positions as a float64 chunk: the lattice points as they are, the random ones moved off every float32
    fr.log['pos64'] = pos.astype(np.float64) * (1.0 if kind == "ortho" else 1.0 + 2.0 ** -40)
    return fr


class _Case:
    """One file and what the tests share about it: the host reader's frames and the model's answers, computed once."""

    def __init__(self, path, kind, N):
        self.path, self.kind, self.N = path, kind, N
        self.box, self.width = KINDS[kind]
        self._hosts, self._models = {}, {}

    def host(self, t, idx):
        if idx not in self._hosts:
            self._hosts[idx] = t[idx]
        return self._hosts[idx]

    def model(self, t, chunk, grid, cell):
        """halo_rows of frame 0's 'position' or 'pos64' for one cell."""
        key = (chunk, grid, cell)
        if key not in self._models:
            h = self.host(t, 0)
            pos = h.particles.position if chunk == 'position' else h.log['pos64']
            self._models[key] = hoomd.halo_rows(pos, self.box, GRIDS[grid][cell], self.width)
        return self._models[key]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """Per kind and N: frame 0; frame 1 elides position and typeid (equal to frame 0's)."""
    d = "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp("halo"))
    out = {}
    for kind in KINDS:
        for N in SIZES:
            rng = np.random.default_rng(N)
            path = os.path.join(d, "pgsd_halo_%d_%s_%d.gsd" % (os.getpid(), kind, N))
            f0 = _frame(rng, kind, N, _positions(rng, kind, N))
            with hoomd.open(path, 'w') as t:
                t.append(f0)
                if N == 70_001:
                    t.append(_frame(rng, kind, N, f0.particles.position, typeid=f0.particles.typeid))
            out[kind, N] = _Case(path, kind, N)
    with fl.open(out["tri", 70_001].path, 'r') as f:
        assert not f.chunk_exists(1, 'particles/position') and f.chunk_exists(1, 'particles/velocity')
    yield out
    for c in out.values():
        os.unlink(c.path)


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _same(dev, host):
    a, b = np.ascontiguousarray(_host(dev)), np.ascontiguousarray(host)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_frame(s, host, model, N):
    """A ghost read against the host frame's rows at concatenate(owned, ghost)."""
    owned, ghosts, shift = model
    rows = np.concatenate([owned, ghosts])
    tag = _host(s.tag)
    assert tag.dtype == np.int32 and np.array_equal(tag, rows)
    assert s.n_owned == len(owned) and s.particles.N == len(rows) and s.particles.N_global == N
    assert _same(s.ghost_shift, shift)
    for name in FIELDS:
        assert _same(getattr(s.particles, name), getattr(host.particles, name)[rows]), name
    pos4 = np.concatenate([host.particles.position[rows], host.particles.typeid[rows].view(np.float32)[:, None]], 1)
    vel4 = np.concatenate([host.particles.velocity[rows], host.particles.mass[rows][:, None]], 1)
    assert _same(s.particles.pos4, pos4) and _same(s.particles.vel4, vel4)


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("chunk", ['position', 'pos64'])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("N", SIZES)
def test_selection_equals_the_model(cases, N, kind, chunk, grid):
    c = cases[kind, N]
    name = 'particles/position' if chunk == 'position' else 'log/pos64'
    seen = 0
    with hoomd.open(c.path, 'r') as t:
        for cell, d in enumerate(GRIDS[grid]):
            owned, ghosts, shift = c.model(t, chunk, grid, cell)
            rows, n_owned, n_ghost, got = t.file.select_halo_device(0, name, c.box, d, c.width)
            t.file.wait_read()
            assert (n_owned, n_ghost) == (len(owned), len(ghosts))
            r = _host(rows)
            assert r.dtype == np.int32 and np.array_equal(r, np.concatenate([owned, ghosts]))
            assert _same(got, shift)
            seen += n_ghost
    assert grid == "1x1x1" or N < 1000 or seen > 0


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("N", SIZES)
def test_ghost_reads_of_every_cell_match_the_host_frame(cases, N, kind, grid):
    c = cases[kind, N]
    with hoomd.open(c.path, 'r') as t:
        host = c.host(t, 0)
        for cell, d in enumerate(GRIDS[grid]):
            s = t.read_frame_device(0, domain=d, ghost=c.width, scalar4=True)
            _check_frame(s, host, c.model(t, 'position', grid, cell), N)
            assert s.domain == d


def test_fractions_in_place_of_a_width(cases):
    c = cases["tri", 4097]
    g = hoomd.ghost_fractions(c.box, c.width)
    with hoomd.open(c.path, 'r') as t:
        s = t.read_frame_device(0, domain=GRIDS["2x2x2"][5], ghost=g, scalar4=True)
        _check_frame(s, c.host(t, 0), c.model(t, 'position', "2x2x2", 5), 4097)


def test_an_empty_ghost_set_gives_zero_row_arrays(cases):
    c = cases["tri", 1000]
    with hoomd.open(c.path, 'r') as t:
        host = c.host(t, 0)
        for d, ghost in ((GRIDS["2x2x2"][2], 0.0), (GRIDS["1x1x1"][0], c.width)):
            s = t.read_frame_device(0, domain=d, ghost=ghost)
            rows = hoomd.domain_rows(host.particles.position, c.box, d)
            assert s.n_owned == s.particles.N == len(rows) > 0 and np.array_equal(_host(s.tag), rows)
            assert tuple(s.ghost_shift.shape) == (0, 3) and _host(s.ghost_shift).dtype == np.int32
    # a single particle, at a corner of the box: the cells in the middle of x neither own nor reach it
    c = cases["ortho", 1]
    with hoomd.open(c.path, 'r') as t:
        models = [c.model(t, 'position', "unequal", cell) for cell in range(6)]
        empty = [cell for cell in range(6) if len(models[cell][0]) + len(models[cell][1]) == 0]
        assert empty == [1, 4]
        for cell in empty:
            s = t.read_frame_device(0, domain=GRIDS["unequal"][cell], ghost=c.width, scalar4=True)
            assert s.particles.N == s.n_owned == 0 and s.particles.N_global == 1 and s.tag.numel() == 0
            assert tuple(s.particles.position.shape) == (0, 3) and tuple(s.particles.pos4.shape) == (0, 4)
            assert tuple(s.ghost_shift.shape) == (0, 3)


def test_a_cell_with_ghosts_but_no_particle_of_its_own(tmp_path):
    """Particles in the lower half of x only: the upper cell owns none and reaches those next to its two faces."""
    box, width = KINDS["ortho"]
    rng = np.random.default_rng(2)
    N = 5000
    k = rng.integers(0, 64, size=(N, 3))
    k[:, 0] %= 32
    pos = ((k / 64.0 - 0.5) * 16.0).astype(np.float32)
    path = str(tmp_path / "lower.gsd")
    with hoomd.open(path, 'w') as t:
        t.append(_frame(rng, "ortho", N, pos))
    upper = hoomd.domain_grid(2, 1, 1)[1]
    owned, ghosts, shift = hoomd.halo_rows(pos, box, upper, width)
    assert len(owned) == 0 and len(ghosts) > 0 and set(shift[:, 0].tolist()) == {0, 1}
    with hoomd.open(path, 'r') as t:
        s = t.read_frame_device(0, domain=upper, ghost=width, scalar4=True)
        _check_frame(s, t[0], (owned, ghosts, shift), N)
        assert s.n_owned == 0 and s.particles.N == len(ghosts)


def test_an_elided_position_is_selected_from_frame_0(cases):
    for kind in sorted(KINDS):
        c = cases[kind, 70_001]
        with hoomd.open(c.path, 'r') as t:
            host = t[1]
            assert np.array_equal(host.particles.position, c.host(t, 0).particles.position)
            for cell, d in enumerate(GRIDS["unequal"]):
                s = t.read_frame_device(1, domain=d, ghost=c.width, scalar4=True)
                _check_frame(s, host, c.model(t, 'position', "unequal", cell), 70_001)


def test_the_staged_position_rows_serve_the_gather(cases):
    """The selection followed by the read costs the position chunk's bytes once."""
    c = cases["tri", 70_001]
    N = c.N
    d = GRIDS["unequal"][4]
    with hoomd.open(c.path, 'r') as t:
        f = t.file
        host = c.host(t, 0)
        owned, ghosts, shift = c.model(t, 'position', "unequal", 4)
        want = np.concatenate([owned, ghosts])
        f.device_read_stats(reset=True)
        rows, n_owned, n_ghost, _ = f.select_halo_device(0, 'particles/position', c.box, d, c.width)
        assert f.device_read_stats()["pread_bytes"] == N * 12
        out = f.read_chunk_device(0, 'particles/position', rows=rows)
        assert f.device_read_stats()["pread_bytes"] == N * 12
        assert _same(out, host.particles.position[want])
        # the whole ghost read: position and typeid (for pos4 too), velocity and mass (for vel4 too), each chunk once
        # at the most (the chunks behind the position go through a row plan, which may read fewer blocks)
        f.device_read_stats(reset=True)
        s = t.read_frame_device(0, domain=d, ghost=c.width)
        _check_frame_arrays = [n for n in FIELDS if f.chunk_exists(0, 'particles/' + n)]
        assert sorted(_check_frame_arrays) == ['mass', 'position', 'typeid', 'velocity']
        assert N * 12 <= f.device_read_stats()["pread_bytes"] <= N * (12 + 4 + 12 + 4)
        assert _same(s.particles.position, host.particles.position[want])


def test_domain_and_slab_reads_are_unchanged_after_ghost_reads(cases):
    c = cases["tri", 70_001]
    d = GRIDS["2x2x2"][3]

    def reads(t):
        a = t.read_frame_device(1, domain=d, scalar4=True)
        b = t.read_frame_device(1, part=(1000, 5000), scalar4=True)
        return a, b

    with hoomd.open(c.path, 'r') as t:
        fresh = reads(t)
    with hoomd.open(c.path, 'r') as t:
        host = t[1]
        t.read_frame_device(1, domain=d, ghost=c.width, scalar4=True)
        t.read_frame_device(0, domain=GRIDS["unequal"][1], ghost=c.width)
        after = reads(t)
    rows = hoomd.domain_rows(host.particles.position, c.box, d)
    for (a, b), label in ((fresh, "fresh"), (after, "after")):
        assert np.array_equal(_host(a.tag), rows) and not hasattr(a, 'n_owned') and not hasattr(a, 'ghost_shift')
        assert not hasattr(b, 'tag') and not hasattr(b, 'n_owned') and b.particles.N == 5000
    for name in FIELDS + ('pos4', 'vel4'):
        for x, y in zip(fresh, after):
            assert _same(getattr(x.particles, name), _host(getattr(y.particles, name))), name
    assert _same(after[0].particles.velocity, host.particles.velocity[rows])
    assert _same(after[1].particles.position, host.particles.position[1000:6000])


def test_bad_arguments_raise(cases):
    c = cases["tri", 1000]
    with hoomd.open(c.path, 'r') as t:
        cell = GRIDS["2x2x2"][0]
        with pytest.raises(ValueError):
            t.read_frame_device(0, domain=cell, ghost=-1.0)
        with pytest.raises(ValueError):
            t.read_frame_device(0, domain=cell, ghost=float('nan'))
        with pytest.raises(ValueError, match="twice"):
            t.read_frame_device(0, domain=cell, ghost=(0.3, 0.0, 0.0))
        with pytest.raises(ValueError):
            t.read_frame_device(0, ghost=c.width)
        with pytest.raises(ValueError):
            t.read_frame_device(0, domain=cell, where={'typeid': [0]}, ghost=c.width)
        with pytest.raises(ValueError):
            t.file.select_halo_device(0, 'particles/mass', c.box, cell, c.width)         # not N x 3
        with pytest.raises(ValueError):
            t.file.select_halo_device(0, 'particles/position', [0, 1, 1, 0, 0, 0], cell, (0.1, 0.1, 0.1))


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
            s = t.read_frame_device(idx, domain=d, ghost=0.25, scalar4=True)
            assert isinstance(s.tag, fl.DeviceBuffer) and isinstance(s.ghost_shift, fl.DeviceBuffer)
            res.append((idx, s.n_owned, s.tag.to_host(), s.ghost_shift.to_host(), s.particles.position.to_host(),
                        s.particles.pos4.to_host(), s.particles.velocity.to_host()))
pickle.dump(res, open(out_path, "wb"))
'''


def test_ghost_read_without_torch(cases, tmp_path):
    c = cases["tri", 70_001]
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, c.path, str(out)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))
    assert len(res) == 12
    with hoomd.open(c.path, 'r') as t:
        hosts = {0: c.host(t, 0), 1: t[1]}
        for i, (idx, n_owned, tag, shift, pos, pos4, vel) in enumerate(res):
            owned, ghosts, want_shift = c.model(t, 'position', "unequal", i % 6)
            rows = np.concatenate([owned, ghosts])
            h = hosts[idx]
            assert n_owned == len(owned) and tag.dtype == np.int32 and np.array_equal(tag, rows)
            assert shift.dtype == np.int32 and shift.shape == want_shift.shape and np.array_equal(shift, want_shift)
            assert pos.tobytes() == h.particles.position[rows].tobytes()
            assert vel.tobytes() == h.particles.velocity[rows].tobytes()
            assert pos4[:, 3].view(np.uint32).tobytes() == h.particles.typeid[rows].tobytes()
