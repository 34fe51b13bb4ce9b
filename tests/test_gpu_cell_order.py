"""Cell-ordered restart reads on the GPU: pgsd_order_rows_by_cell_device sorts a row list by the grid cell of its rows'
positions (key kernel, stable radix sort of (key, entry) pairs, apply kernel), behind
pgsd.fl.PGSDFile.order_rows_by_cell_device and read_frame_device(cell_order=...).  Every result must equal the numpy
models pgsd.hoomd.cell_ids / cell_order exactly -- they are integers and gathered bytes, no tolerance applies.  Files
are written through the host path.

The sort takes 8 bits of the key per pass, and only as many passes as the largest key of a call has bits.  The grids
below make every pass count occur: one cell (one key value, or two with the ghost run: pure stability), 64 cells (one
pass), 256 cells (two passes: the "nowhere" id 256 of a NaN row, and every ghost key, lies past the first digit), 65 536
cells (three) and 2^30 cells (four)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 70_001
ORTHO = np.array([16.0, 16.0, 16.0, 0.0, 0.0, 0.0], np.float32)
TRI = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
FLAT = np.array([4.0, 4.0, 1.0, 0.5, 0.0, 0.0], np.float32)
# lattice: the 1/64 lattice of fractions (exact arithmetic, rows on cell corners).  tri: random rows in a triclinic box.
# nan: the same with NaN and infinite rows.  cluster: every row the same point -- one key, every lane of every wave
# asks for the same counter.
KINDS = {"lattice": ORTHO, "tri": TRI, "nan": TRI, "cluster": TRI}
GRIDS = [(1, 1, 1), (4, 4, 4), (16, 16, 1), (64, 64, 16), (1024, 1024, 1024)]
# nothing, one entry, around one wave step, around one tile of 4096, many tiles with a ragged end
SIZES = [0, 1, 63, 64, 65, 4096, 4097, N]
FIELDS = ('position', 'typeid', 'velocity', 'mass', 'image', 'density', 'energy', 'body', 'slength', 'auxiliary1')


def _positions(rng, kind, n):
    if kind == "cluster":
        return np.broadcast_to(np.array([0.75, -1.25, 0.375], np.float32), (n, 3)).copy()
    if kind in ("tri", "nan"):
        pos = rng.uniform(-3.0, 3.0, size=(n, 3)).astype(np.float32)
        if kind == "nan":
            pos[::7] = np.nan
            pos[1::11, 2] = np.inf
            pos[2::13, 0] = -np.inf
            pos[3::17, 1] = np.nan
        return pos
    k = rng.integers(0, 64, size=(n, 3))
    k[:64] = np.arange(64)[:min(n, 64), None]
    p = (k / 64.0 + rng.integers(-1, 2, size=(n, 3)) - 0.5) * 16.0
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32)


def _frame(rng, box, pos, step=0, typeid=None, dimensions=3, pos64=True):
    n = len(pos)
    fr = hoomd.Frame()
    fr.configuration.step = step
    fr.configuration.box = box
    fr.configuration.dimensions = dimensions
    fr.particles.N = n
    fr.particles.types = ['A', 'B', 'C']
    fr.particles.position = pos
    fr.particles.typeid = rng.integers(0, 3, size=n).astype(np.uint32) if typeid is None else typeid
    fr.particles.velocity = rng.standard_normal((n, 3)).astype(np.float32)
    fr.particles.mass = rng.uniform(0.5, 2.0, size=n).astype(np.float32)
    if pos64:
        fr.log['pos64'] = pos.astype(np.float64) * (1.0 if box is ORTHO else 1.0 + 2.0 ** -40)
    return fr


def _dir(tmp_path_factory, name):
    return "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp(name))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """Per kind one file of N rows: frame 0 (float32 position chunk, float64 log chunk of the same rows), and for "tri"
    a frame 1 that elides position and typeid.  Value: path and the host reader's frames."""
    d = _dir(tmp_path_factory, "cell_order")
    out = {}
    for kind, box in KINDS.items():
        rng = np.random.default_rng(len(kind))
        path = os.path.join(d, "pgsd_cell_order_%d_%s.gsd" % (os.getpid(), kind))
        f0 = _frame(rng, box, _positions(rng, kind, N))
        with hoomd.open(path, 'w') as t:
            t.append(f0)
            if kind == "tri":
                t.append(_frame(rng, box, f0.particles.position, step=5, typeid=f0.particles.typeid, pos64=False))
        with hoomd.open(path, 'r') as t:
            out[kind] = (path, [t[i] for i in range(len(t))])
    with fl.open(out["tri"][0], 'r') as f:
        assert not f.chunk_exists(1, 'particles/position') and f.chunk_exists(1, 'particles/velocity')
    yield out
    for path, _ in out.values():
        os.unlink(path)


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _same(dev, host):
    a, b = np.ascontiguousarray(_host(dev)), np.ascontiguousarray(host)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _lists(f, name, box, n):
    """The two row lists of n entries a case sorts: the head of a selection's (ascending), and seeded random rows with
    repeats (host copies)."""
    rows, count = f.select_domain_device(0, name, box, hoomd.domain_grid(1, 1, 1)[0])
    selected = _host(rows)[:n].astype(np.int32)
    rng = np.random.default_rng(1000 + n)
    return {"selected": selected, "random": rng.integers(0, N, size=n).astype(np.int32)}


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(str(v) for v in g))
@pytest.mark.parametrize("chunk", ['position', 'pos64'])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_ordering_equals_the_model(cases, kind, chunk, grid):
    path, frames = cases[kind]
    box = KINDS[kind]
    pos = frames[0].particles.position if chunk == 'position' else frames[0].log['pos64']
    name = 'particles/position' if chunk == 'position' else 'log/pos64'
    ids = hoomd.cell_ids(pos, box, grid)
    n_cells = grid[0] * grid[1] * grid[2]
    with fl.open(path, 'r') as f:
        device = f.pipeline_device()
        for size in SIZES:
            for which, rows in sorted(_lists(f, name, box, size).items()):
                n = len(rows)           # (the selection leaves out the "nan" file's NaN rows: its whole list is shorter)
                assert n == size or (kind == "nan" and which == "selected" and size == N and n > N // 2)
                for n_owned in (n, n // 3):
                    what = (n, which, n_owned)
                    want_rows, want_cell, perm = hoomd.cell_order(pos, box, rows, grid, n_owned=n_owned)
                    assert np.array_equal(want_cell, ids[want_rows])
                    shift = np.random.default_rng(n).integers(-1, 2, size=(n - n_owned, 3)).astype(np.int32)
                    d_rows = fl._device_from_host(rows, device)
                    d_shift = fl._device_from_host(shift, device)
                    cell = f.order_rows_by_cell_device(0, name, box, grid, d_rows, n_owned=n_owned, shift=d_shift)
                    got_rows, got_cell = _host(d_rows), _host(cell)
                    assert got_cell.dtype == np.int32 and got_cell.shape == (n,), what
                    assert np.array_equal(got_rows, want_rows), (what, np.flatnonzero(got_rows != want_rows)[:8])
                    assert np.array_equal(got_cell, want_cell), (what, np.flatnonzero(got_cell != want_cell)[:8])
                    assert np.array_equal(_host(d_shift).reshape(-1, 3), shift[perm[n_owned:] - n_owned]), what
        f.wait_read()
    if kind == "nan":
        assert (ids == n_cells).sum() > 1000                 # the "nowhere" id is among the keys
    if kind == "cluster":
        assert len(set(ids.tolist())) == 1
    if kind in ("tri", "lattice") and n_cells > 1:
        assert len(set(ids.tolist())) > min(n_cells, N) // 4


def test_an_ordering_after_a_selection_reads_no_file_byte(cases):
    path, frames = cases["tri"]
    pos = frames[0].particles.position
    d = hoomd.domain_grid(2, 2, 2)[3]
    with fl.open(path, 'r') as f:
        f.device_read_stats(reset=True)
        rows, count = f.select_domain_device(0, 'particles/position', TRI, d)
        assert f.device_read_stats()["pread_bytes"] == N * 12
        cell = f.order_rows_by_cell_device(0, 'particles/position', TRI, (8, 8, 8), rows)
        assert f.device_read_stats()["pread_bytes"] == N * 12
        want_rows, want_cell, _ = hoomd.cell_order(pos, TRI, hoomd.domain_rows(pos, TRI, d), (8, 8, 8))
        assert np.array_equal(_host(rows), want_rows) and np.array_equal(_host(cell), want_cell) and count == len(want_rows)
        # ... and neither does the position gather through the ordered rows
        out = f.read_chunk_device(0, 'particles/position', rows=rows)
        assert f.device_read_stats()["pread_bytes"] == N * 12
        assert _same(out, pos[want_rows])
        # after the wait the chunk is released: an ordering on its own stages it, once
        rows = fl._device_from_host(np.arange(100, dtype=np.int32)[::-1].copy(), f.pipeline_device())
        f.order_rows_by_cell_device(0, 'particles/position', TRI, (2, 2, 2), rows)
        f.order_rows_by_cell_device(0, 'particles/position', TRI, (3, 3, 3), rows)
        assert f.device_read_stats()["pread_bytes"] == 2 * N * 12
        f.wait_read()


def test_every_refusal_has_its_message_and_writes_nothing(cases):
    path, frames = cases["tri"]
    pos = frames[0].particles.position
    name = 'particles/position'
    with fl.open(path, 'r') as f:
        device = f.pipeline_device()
        host_rows = np.random.default_rng(5).integers(0, N, size=5000).astype(np.int32)
        host_shift = np.random.default_rng(6).integers(-1, 2, size=(3000, 3)).astype(np.int32)
        rows = fl._device_from_host(host_rows, device)
        shift = fl._device_from_host(host_shift, device)
        for cells in ((0, 1, 1), (1, 1025, 1), (4, 4, 0)):
            with pytest.raises(ValueError, match="1 to 1024 cells"):
                f.order_rows_by_cell_device(0, name, TRI, cells, rows)
        with pytest.raises(ValueError, match="three counts"):
            f.order_rows_by_cell_device(0, name, TRI, (4, 4), rows)
        with pytest.raises(ValueError, match="one z cell"):
            f.order_rows_by_cell_device(0, name, TRI, (4, 4, 2), rows, dimensions=2)
        with pytest.raises(ValueError, match="n_owned"):
            f.order_rows_by_cell_device(0, name, TRI, (4, 4, 4), rows, n=100, n_owned=101)
        with pytest.raises(ValueError, match="2\\^32"):
            f.order_rows_by_cell_device(0, name, TRI, (4, 4, 4), rows, n=1 << 32)
        with pytest.raises(ValueError, match="fewer entries"):
            f.order_rows_by_cell_device(0, name, TRI, (4, 4, 4), rows, n=5001)
        with pytest.raises(ValueError, match="3 x"):
            f.order_rows_by_cell_device(0, name, TRI, (4, 4, 4), rows, n_owned=1000, shift=shift)
        # the selection's refusals
        with pytest.raises(ValueError, match="N x 3"):
            f.order_rows_by_cell_device(0, 'particles/mass', TRI, (4, 4, 4), rows)
        with pytest.raises(ValueError, match="box lengths"):
            f.order_rows_by_cell_device(0, name, [0, 1, 1, 0, 0, 0], (4, 4, 4), rows)
        with pytest.raises(ValueError):
            f.order_rows_by_cell_device(0, name, TRI, (4, 4, 1), rows, dimensions=4)
        with pytest.raises(KeyError):
            f.order_rows_by_cell_device(0, 'particles/nothing', TRI, (4, 4, 4), rows)
        assert np.array_equal(_host(rows), host_rows) and np.array_equal(_host(shift), host_shift)
        # an entry outside the chunk: found by the key pass, before anything of the caller's is written -- in the first
        # tile, in the last, in the owned and in the ghost run
        for at in (0, 1999, 2000, 4999):
            bad = host_rows.copy()
            bad[at] = N if at != 1999 else -1
            d_bad = fl._device_from_host(bad, device)
            with pytest.raises(ValueError, match="outside the position chunk"):
                f.order_rows_by_cell_device(0, name, TRI, (64, 64, 16), d_bad, n_owned=2000, shift=shift)
            assert np.array_equal(_host(d_bad), bad) and np.array_equal(_host(shift), host_shift)
        # n == 0 succeeds and touches nothing; the handle works as before
        cell = f.order_rows_by_cell_device(0, name, TRI, (4, 4, 4), rows, n=0)
        assert _host(cell).shape == (0,) and np.array_equal(_host(rows), host_rows)
        cell = f.order_rows_by_cell_device(0, name, TRI, (64, 64, 16), rows, n_owned=2000, shift=shift)
        want_rows, want_cell, perm = hoomd.cell_order(pos, TRI, host_rows, (64, 64, 16), n_owned=2000)
        assert np.array_equal(_host(rows), want_rows) and np.array_equal(_host(cell), want_cell)
        assert np.array_equal(_host(shift), host_shift[perm[2000:] - 2000])
        # a prefix: the entries behind n stay
        rows = fl._device_from_host(host_rows, device)
        f.order_rows_by_cell_device(0, name, TRI, (4, 4, 4), rows, n=777)
        got = _host(rows)
        assert np.array_equal(got[:777], hoomd.cell_order(pos, TRI, host_rows[:777], (4, 4, 4))[0])
        assert np.array_equal(got[777:], host_rows[777:])
        f.wait_read()


# ---------------------------------------------------------------------------------------------------- pgsd.hoomd
GRID = hoomd.domain_grid(2, 2, 2)
CELLS = (16, 16, 16)        # 4096 cells: two passes, three with the ghost run's segment bit


def _check_frame(s, host, rows, cell, n_global, n_owned=None, shift=None, cells=CELLS):
    """A cell-ordered read against the host frame's rows at the model's sorted row list."""
    tag = _host(s.tag)
    assert tag.dtype == np.int32 and np.array_equal(tag, rows)
    got_cell = _host(s.cell)
    assert got_cell.dtype == np.int32 and np.array_equal(got_cell, cell)
    assert s.cell_grid == tuple(cells)
    assert s.particles.N == len(rows) and s.particles.N_global == n_global
    if n_owned is not None:
        assert s.n_owned == n_owned and _same(s.ghost_shift, shift)
    for name in FIELDS:
        assert _same(getattr(s.particles, name), getattr(host.particles, name)[rows]), name
    pos4 = np.concatenate([host.particles.position[rows], host.particles.typeid[rows].view(np.float32)[:, None]], 1)
    vel4 = np.concatenate([host.particles.velocity[rows], host.particles.mass[rows][:, None]], 1)
    assert _same(s.particles.pos4, pos4) and _same(s.particles.vel4, vel4)


@pytest.mark.parametrize("kind", ["lattice", "tri"])
def test_a_cell_ordered_domain_read_matches_the_host_frame(cases, kind):
    path, frames = cases[kind]
    box, host = KINDS[kind], frames[0]
    pos = host.particles.position
    with hoomd.open(path, 'r') as t:
        for r in (0, 5):
            want = hoomd.cell_order(pos, box, hoomd.domain_rows(pos, box, GRID[r]), CELLS)
            assert len(want[0]) > 5000 and len(set(want[1].tolist())) > 100
            s = t.read_frame_device(0, domain=GRID[r], cell_order=CELLS, scalar4=True)
            _check_frame(s, host, want[0], want[1], N)
            assert s.domain == GRID[r] and (np.diff(_host(s.cell)) >= 0).all()


@pytest.mark.parametrize("kind", ["lattice", "tri"])
def test_a_cell_ordered_ghost_read_matches_the_host_frame(cases, kind):
    path, frames = cases[kind]
    box, host = KINDS[kind], frames[0]
    width = 1.0 if kind == "lattice" else 0.25
    pos = host.particles.position
    with hoomd.open(path, 'r') as t:
        owned, ghosts, shift = hoomd.halo_rows(pos, box, GRID[3], width)
        n = len(owned)
        assert len(ghosts) > 1000 and shift.any()
        rows, cell, perm = hoomd.cell_order(pos, box, np.concatenate([owned, ghosts]), CELLS, n_owned=n)
        s = t.read_frame_device(0, domain=GRID[3], ghost=width, cell_order=CELLS, scalar4=True)
        _check_frame(s, host, rows, cell, N, n_owned=n, shift=shift[perm[n:] - n])
        got = _host(s.cell)
        assert (np.diff(got[:n]) >= 0).all() and (np.diff(got[n:]) >= 0).all() and got[n] < got[n - 1]


def test_a_cell_ordered_group_read_matches_the_host_frame(cases):
    path, frames = cases["tri"]
    host = frames[0]
    pos = host.particles.position
    where = {'type': ['A', 'C'], ('velocity', 2): (None, 0.5)}
    arrays = {'typeid': host.particles.typeid, 'velocity': host.particles.velocity}
    group = hoomd.where_rows(arrays, where, host.particles.types)
    with hoomd.open(path, 'r') as t:
        # a group inside a cell
        inside = np.intersect1d(group, hoomd.domain_rows(pos, TRI, GRID[6]))
        want = hoomd.cell_order(pos, TRI, inside, CELLS)
        assert len(inside) > 1000
        s = t.read_frame_device(0, where=where, domain=GRID[6], cell_order=CELLS, scalar4=True)
        _check_frame(s, host, want[0], want[1], N)
        # a group alone: the ordering stages the position chunk itself
        want = hoomd.cell_order(pos, TRI, group, (4, 4, 4))
        s = t.read_frame_device(0, where=where, cell_order=(4, 4, 4), scalar4=True)
        _check_frame(s, host, want[0], want[1], N, cells=(4, 4, 4))
        # a group nobody is in
        s = t.read_frame_device(0, where={'mass': (100.0, None)}, cell_order=CELLS)
        assert s.particles.N == 0 and _host(s.cell).shape == (0,) and _host(s.tag).shape == (0,)


def test_an_elided_position_is_ordered_from_frame_0(cases):
    path, frames = cases["tri"]
    pos = frames[0].particles.position
    host = frames[1]
    assert np.array_equal(host.particles.position, pos)
    want = hoomd.cell_order(pos, TRI, hoomd.domain_rows(pos, TRI, GRID[2]), CELLS)
    with hoomd.open(path, 'r') as t:
        s = t.read_frame_device(1, domain=GRID[2], cell_order=CELLS, scalar4=True)
        _check_frame(s, host, want[0], want[1], N)
        assert s.configuration.step == 5


def test_a_position_stored_nowhere_keeps_the_order(tmp_path_factory):
    d = _dir(tmp_path_factory, "cell_order_default")
    path = os.path.join(d, "pgsd_cell_order_%d_default.gsd" % os.getpid())
    rng = np.random.default_rng(3)
    fr = hoomd.Frame()
    fr.configuration.box = TRI
    fr.particles.N = 5000
    fr.particles.mass = rng.uniform(0.5, 2.0, size=5000).astype(np.float32)
    try:
        with hoomd.open(path, 'w') as t:
            t.append(fr)
        with hoomd.open(path, 'r') as t:
            assert not t.file.chunk_exists(0, 'particles/position')
            one = int(hoomd.cell_ids(np.zeros((1, 3), np.float32), TRI, CELLS)[0])
            # the origin lies in cell 7 of the 2 x 2 x 2 grid
            s = t.read_frame_device(0, domain=GRID[7], cell_order=CELLS)
            assert s.particles.N == 5000 and np.array_equal(_host(s.tag), np.arange(5000))
            assert _host(s.cell).dtype == np.int32 and _host(s.cell).tolist() == [one] * 5000 and s.cell_grid == CELLS
            assert _same(s.particles.mass, fr.particles.mass)
            s = t.read_frame_device(0, domain=GRID[0], cell_order=CELLS)
            assert s.particles.N == 0 and _host(s.cell).shape == (0,)
            s = t.read_frame_device(0, where={'mass': (1.0, None)}, cell_order=CELLS)
            keep = np.flatnonzero(fr.particles.mass >= 1.0)
            assert np.array_equal(_host(s.tag), keep) and _host(s.cell).tolist() == [one] * len(keep)
    finally:
        if os.path.exists(path):
            os.unlink(path)


def test_a_two_dimensional_frame(tmp_path_factory):
    d = _dir(tmp_path_factory, "cell_order_flat")
    path = os.path.join(d, "pgsd_cell_order_%d_flat.gsd" % os.getpid())
    rng = np.random.default_rng(4)
    pos = _positions(rng, "tri", 9000)
    pos[:, 2] = 0.0
    try:
        with hoomd.open(path, 'w') as t:
            t.append(_frame(rng, FLAT, pos, dimensions=2, pos64=False))
        with hoomd.open(path, 'r') as t:
            host = t[0]
            assert int(host.configuration.dimensions) == 2
            cell2 = hoomd.domain_grid(2, 2, 1)[1]
            want = hoomd.cell_order(pos, FLAT, hoomd.domain_rows(pos, FLAT, cell2, 2), (32, 32, 1), dimensions=2)
            s = t.read_frame_device(0, domain=cell2, cell_order=(32, 32, 1), scalar4=True)
            _check_frame(s, host, want[0], want[1], 9000, cells=(32, 32, 1))
            with pytest.raises(ValueError, match="cz == 1"):
                t.read_frame_device(0, domain=cell2, cell_order=(4, 4, 2))
    finally:
        if os.path.exists(path):
            os.unlink(path)


def test_reads_without_cell_order_are_what_they_were(cases):
    """cell_order=None changes nothing: ascending rows, no cell attributes -- before and after ordered reads."""
    path, frames = cases["tri"]
    host = frames[0]
    pos = host.particles.position
    want = hoomd.domain_rows(pos, TRI, GRID[3])
    owned, ghosts, shift = hoomd.halo_rows(pos, TRI, GRID[3], 0.25)
    with hoomd.open(path, 'r') as t:
        for again in range(2):
            s = t.read_frame_device(0, domain=GRID[3], scalar4=True)
            assert np.array_equal(_host(s.tag), want) and not hasattr(s, 'cell') and not hasattr(s, 'cell_grid')
            for name in FIELDS:
                assert _same(getattr(s.particles, name), getattr(host.particles, name)[want]), name
            s = t.read_frame_device(0, domain=GRID[3], ghost=0.25)
            assert np.array_equal(_host(s.tag), np.concatenate([owned, ghosts])) and _same(s.ghost_shift, shift)
            assert s.n_owned == len(owned) and not hasattr(s, 'cell')
            s = t.read_frame_device(0, where={'type': ['B']})
            assert np.array_equal(_host(s.tag), np.flatnonzero(host.particles.typeid == 1)) and not hasattr(s, 'cell')
            t.read_frame_device(0, domain=GRID[3], ghost=0.25, cell_order=CELLS)
        with pytest.raises(ValueError, match="cell_order needs domain or where"):
            t.read_frame_device(0, cell_order=CELLS)
        with pytest.raises(ValueError, match="cell_order needs domain or where"):
            t.read_frame_device(0, part=(0, 10), cell_order=CELLS)


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
res = {}
d = hoomd.domain_grid(2, 2, 2)[3]
with hoomd.open(path, 'r') as t:
    s = t.read_frame_device(1, domain=d, ghost=0.25, cell_order=(16, 16, 16), scalar4=True)
    assert isinstance(s.cell, fl.DeviceBuffer) and isinstance(s.tag, fl.DeviceBuffer)
    res["ghost"] = dict(tag=s.tag.to_host(), cell=s.cell.to_host(), n_owned=s.n_owned, shift=s.ghost_shift.to_host(),
                        velocity=s.particles.velocity.to_host(), pos4=s.particles.pos4.to_host())
    f = t.file
    rows = fl._device_from_host(np.arange(70001, dtype=np.int32)[::-1].copy(), f.pipeline_device())
    cell = f.order_rows_by_cell_device(0, 'log/pos64', t[0].configuration.box, (1024, 1024, 1024), rows)
    res["fl"] = dict(rows=rows.to_host(), cell=cell.to_host())
    f.wait_read()
pickle.dump(res, open(out_path, "wb"))
'''


def test_cell_order_without_torch(cases, tmp_path):
    path, frames = cases["tri"]
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, path, str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))
    pos, host = frames[0].particles.position, frames[1]
    owned, ghosts, shift = hoomd.halo_rows(pos, TRI, GRID[3], 0.25)
    n = len(owned)
    rows, cell, perm = hoomd.cell_order(pos, TRI, np.concatenate([owned, ghosts]), (16, 16, 16), n_owned=n)
    got = res["ghost"]
    assert np.array_equal(got["tag"], rows) and np.array_equal(got["cell"], cell) and got["n_owned"] == n
    assert np.array_equal(got["shift"], shift[perm[n:] - n])
    assert got["velocity"].tobytes() == host.particles.velocity[rows].tobytes()
    assert got["pos4"][:, :3].tobytes() == np.ascontiguousarray(pos[rows]).tobytes()
    back = np.arange(N, dtype=np.int32)[::-1]
    want = hoomd.cell_order(frames[0].log['pos64'], TRI, back, (1024, 1024, 1024))
    assert np.array_equal(res["fl"]["rows"], want[0]) and np.array_equal(res["fl"]["cell"], want[1])
