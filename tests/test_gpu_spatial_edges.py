"""The spatial GPU kernels where random three-dimensional frames do not reach: two-dimensional frames whose z is junk,
non-finite rows through the selections, and tiles that keep almost nothing or everything.

Every spatial kernel derives a row's wrapped fraction through domain_skew() / domain_wrap() (pgsd_select.hpp): the
domain, ghost-layer and group selections, the axis histograms and cell counts, the cell keys.  Each must equal its numpy
model in pgsd.hoomd exactly -- integer row lists, counts and shifts, no tolerance applies.  Three parts:

A  ``dimensions == 2``: z has no say.  z is finite junk (a quarter of the rows at 0, all others with a z fraction of
   their own), the box is flat (Lz == 0: z's own fraction is NaN or infinite for every row), flat with Lz > 0, or tilted
   (z enters the x and y fractions and is not compared itself), and the cells carry a z interval that is not [0, 1).
   Against the models, and -- model-free -- against the same rows with z = 0 where z enters nothing.
B  NaN and infinite coordinates, -0.0 and the largest float32 through the three selections: such rows belong nowhere.
C  The compaction epilogue (a head of 0 to 3 single stores, 16-byte stores, a tail): the truth is constructed from three
   lattice points, tiles keep 0, 1, 2, 3, 4, 5, 7, 4093 ... 4096 rows at every start residue modulo 4, and a frame of
   more than 256 tiles sends the one-block scan through a second trip with a carry.

Files are written through the host path, once per module."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402

TILE = 4096                  # rows per workgroup of the selections: row = base + k * 256 + lane, k < 16
SIZES = [1, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5]
FIELDS = ('position', 'typeid', 'velocity', 'mass', 'image', 'density', 'energy', 'body', 'slength', 'auxiliary1')


def _dir(tmp_path_factory, name):
    return "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp(name))


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _same(dev, host):
    a, b = np.ascontiguousarray(_host(dev)), np.ascontiguousarray(host)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _typeid(n):
    i = np.arange(n)
    return ((i * 7 + i // 5 + 1) % 4).astype(np.uint32)         # row 0 is 1: no array equals its default and is elided


def _write(path, box, pos, scale=1.0, typeid=None, rng=None):
    """One frame: ``pos`` as particles/position (float32) and, times ``scale``, as the float64 chunk log/pos64; with
    ``rng`` a velocity and a mass too.  Returns the two arrays as written."""
    fr = hoomd.Frame()
    fr.configuration.step = 3
    fr.configuration.box = box
    fr.particles.N = len(pos)
    fr.particles.types = ['A', 'B', 'C', 'D']
    fr.particles.position = pos
    fr.particles.typeid = typeid
    if rng is not None:
        fr.particles.velocity = rng.standard_normal((len(pos), 3)).astype(np.float32)
        fr.particles.mass = rng.uniform(0.5, 2.0, size=len(pos)).astype(np.float32)
    fr.log['pos64'] = pos.astype(np.float64) * scale
    with hoomd.open(path, 'w') as t:
        t.append(fr)
    return {'position': pos, 'pos64': fr.log['pos64']}


def _chunk(chunk):
    return 'particles/position' if chunk == 'position' else 'log/pos64'


OFF_GRID = 1.0 + 2.0 ** -40          # moves a float32 value to a float64 no float32 holds

# ---------------------------------------------------------------------------------------------------- A: two dimensions
FLAT0 = np.array([4.0, 4.0, 0.0, 0.5, 0.0, 0.0], np.float32)
FLAT1 = np.array([4.0, 4.0, 2.0, 0.5, 0.0, 0.0], np.float32)
TILT = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
BOXES = {"flat0": FLAT0, "flat1": FLAT1, "tilt": TILT}
Z_LO, Z_HI = 0.25, 0.5               # the z interval every cell carries: the 2-D model ignores it
SPLIT = dict(x_split=[0.25, 0.5])
CELLS2 = [hoomd.Domain((d.lo[0], d.lo[1], Z_LO), (d.hi[0], d.hi[1], Z_HI)) for d in hoomd.domain_grid(3, 2, 1, **SPLIT)]
INNER2 = [b[1:-1] for b in hoomd.grid_bounds(3, 2, 1, **SPLIT)]
WIDTH = 0.25
SET = [1, 2]


def _flat_positions(rng, n):
    """Random x and y; z is 0 in every fourth row and elsewhere k / 2^19 - 1 + 2 m with no k twice and m in {-1, 0, 1}:
    finite junk in [-3, 3) whose fraction of a box with Lz == 2 no two of these rows share.  Row 0 lies just above the
    plane y fraction 0.5 (z == 0, so in every box here): some cell has it in its ghost layer at every n."""
    pos = rng.uniform(-3.0, 3.0, size=(n, 3))
    k = rng.choice(2 ** 20 - 1, size=n, replace=False)
    k += k >= 2 ** 19                                           # (k == 2^19 is the fraction of z == 0)
    z = (k / 2.0 ** 20 - 0.5) * 2.0 + 2.0 * rng.integers(-1, 2, size=n)
    z[::4] = 0.0
    pos[:, 2] = z
    pos[0, 1] = 0.04
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
    return pos.astype(np.float32)


class _Flat:
    def __init__(self, n, path, rows, path0, rows0):
        self.N, self.path, self.rows, self.path0, self.rows0 = n, path, rows, path0, rows0
        self.typeid = _typeid(n)


@pytest.fixture(scope="module")
def flat(tmp_path_factory):
    """Per N two files of one frame: the junk z, and the same rows with z = 0."""
    d = _dir(tmp_path_factory, "spatial_flat")
    out = {}
    for n in SIZES:
        rng = np.random.default_rng(n)
        pos = _flat_positions(rng, n)
        pos0 = pos.copy()
        pos0[:, 2] = 0.0
        path, path0 = (os.path.join(d, "pgsd_edges_%d_flat%s_%d.gsd" % (os.getpid(), v, n)) for v in ("", "0"))
        c = out[n] = _Flat(n, path, _write(path, TILT, pos, OFF_GRID, _typeid(n)),
                           path0, _write(path0, TILT, pos0, OFF_GRID, _typeid(n)))
        for chunk in ('position', 'pos64'):
            p = c.rows[chunk]
            # by the 3-D model: at least a quarter of the rows lie outside the cells' z interval, ...
            slab = hoomd.Domain((0.0, 0.0, Z_LO), (1.0, 1.0, Z_HI))
            for box in (FLAT1, TILT):
                assert 4 * (n - len(hoomd.domain_rows(p, box, slab, 3))) >= n
            # ... no two rows off z == 0 agree in z's fraction, a quarter of the rows has z == 0, ...
            fz = hoomd._wrapped_fractions(p, FLAT1, 3)[2]
            off = p[:, 2] != 0
            assert len(np.unique(fz[off])) == off.sum() and 4 * (n - off.sum()) >= n and not (fz[off] == 0.5).any()
            # ... and in the flat box z's own fraction is NaN or infinite for every row
            with np.errstate(invalid='ignore', divide='ignore'):
                assert not np.isfinite((p[:, 2].astype(np.float64) + 0.0) / np.float64(FLAT0[2])).any()
            assert np.array_equal(c.rows0[chunk][:, :2], p[:, :2]) and not c.rows0[chunk][:, 2].any()
    yield out
    for c in out.values():
        os.unlink(c.path)
        os.unlink(c.path0)


def _ignores_z(key):
    return key != "tilt"              # xz == yz == 0: z enters no fraction that takes part


@pytest.mark.parametrize("chunk", ['position', 'pos64'])
@pytest.mark.parametrize("N", SIZES)
def test_2d_domain_selection_ignores_z(flat, N, chunk):
    c, name = flat[N], _chunk(chunk)
    with fl.open(c.path, 'r') as f, fl.open(c.path0, 'r') as f0:
        for key, box in BOXES.items():
            seen = []
            for cell in CELLS2:
                rows, count = f.select_domain_device(0, name, box, cell, dimensions=2)
                want = hoomd.domain_rows(c.rows[chunk], box, cell, dimensions=2)
                got = _host(rows)
                assert count == len(want) and got.dtype == np.int32 and np.array_equal(got, want), (key, cell)
                if _ignores_z(key):
                    rows0, count0 = f0.select_domain_device(0, name, box, cell, dimensions=2)
                    assert count0 == count and np.array_equal(_host(rows0), got), (key, cell)
                seen.append(got)
            assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(N)), key     # the cells partition the rows
        f.wait_read()
        f0.wait_read()


@pytest.mark.parametrize("chunk", ['position', 'pos64'])
@pytest.mark.parametrize("N", SIZES)
def test_2d_ghost_layer_ignores_z(flat, N, chunk):
    c, name = flat[N], _chunk(chunk)
    with fl.open(c.path, 'r') as f, fl.open(c.path0, 'r') as f0:
        for key, box in BOXES.items():
            ghosts_seen = 0
            for cell in CELLS2:
                owned, ghosts, shift = hoomd.halo_rows(c.rows[chunk], box, cell, WIDTH, dimensions=2)
                rows, n_owned, n_ghost, got_shift = f.select_halo_device(0, name, box, cell, WIDTH, dimensions=2)
                got = _host(rows)
                assert (n_owned, n_ghost) == (len(owned), len(ghosts)), (key, cell)
                assert got.dtype == np.int32 and np.array_equal(got, np.concatenate([owned, ghosts])), (key, cell)
                assert _same(got_shift, shift) and not _host(got_shift)[:, 2].any(), (key, cell)
                if _ignores_z(key):
                    rows0, n_owned0, n_ghost0, shift0 = f0.select_halo_device(0, name, box, cell, WIDTH, dimensions=2)
                    assert (n_owned0, n_ghost0) == (n_owned, n_ghost) and np.array_equal(_host(rows0), got)
                    assert _same(shift0, _host(got_shift))
                ghosts_seen += n_ghost
            assert ghosts_seen > 0, key
        f.wait_read()
        f0.wait_read()


@pytest.mark.parametrize("chunk", ['position', 'pos64'])
@pytest.mark.parametrize("N", SIZES)
def test_2d_group_selection_in_a_domain_ignores_z(flat, N, chunk):
    c, name = flat[N], _chunk(chunk)
    group = hoomd.where_rows({'typeid': c.typeid}, {'typeid': SET})
    term = [(0, 'particles/typeid', 0, SET)]
    with fl.open(c.path, 'r') as f, fl.open(c.path0, 'r') as f0:
        for key, box in BOXES.items():
            total = 0
            for cell in CELLS2:
                want = np.intersect1d(group, hoomd.domain_rows(c.rows[chunk], box, cell, dimensions=2))
                rows, count = f.select_where_device(term, domain=(0, name, cell), box=box, dimensions=2)
                got = _host(rows)
                assert count == len(want) and got.dtype == np.int32 and np.array_equal(got, want), (key, cell)
                if _ignores_z(key):
                    rows0, count0 = f0.select_where_device(term, domain=(0, name, cell), box=box, dimensions=2)
                    assert count0 == count and np.array_equal(_host(rows0), got), (key, cell)
                total += count
            assert total == len(group) > 0, key
        f.wait_read()
        f0.wait_read()


@pytest.mark.parametrize("chunk", ['position', 'pos64'])
@pytest.mark.parametrize("N", SIZES)
def test_2d_census_ignores_z(flat, N, chunk):
    c, name = flat[N], _chunk(chunk)
    with fl.open(c.path, 'r') as f, fl.open(c.path0, 'r') as f0:
        for key, box in BOXES.items():
            hist = f.domain_histogram_device(0, name, box, 64, dimensions=2)
            assert np.array_equal(hist, hoomd.axis_histograms(c.rows[chunk], box, 64, dimensions=2)), key
            assert not hist[2].any() and hist[0].sum() == N and hist[1].sum() == N, key
            counts, nowhere = f.domain_counts_device(0, name, box, (3, 2, 1), INNER2, dimensions=2)
            want, want_nowhere = hoomd.domain_counts(c.rows[chunk], box, 3, 2, 1, dimensions=2, **SPLIT)
            assert np.array_equal(counts, want) and nowhere == want_nowhere == 0 and counts.sum() == N, key
            if _ignores_z(key):
                assert np.array_equal(f0.domain_histogram_device(0, name, box, 64, dimensions=2), hist), key
                counts0, nowhere0 = f0.domain_counts_device(0, name, box, (3, 2, 1), INNER2, dimensions=2)
                assert np.array_equal(counts0, counts) and nowhere0 == 0, key
        f.wait_read()
        f0.wait_read()


@pytest.mark.parametrize("chunk", ['position', 'pos64'])
@pytest.mark.parametrize("N", SIZES)
def test_2d_cell_order_ignores_z(flat, N, chunk):
    c, name = flat[N], _chunk(chunk)
    cells = (8, 8, 1)
    lists = {"ascending": np.arange(N, dtype=np.int32),
             "random": np.random.default_rng(N + 1).integers(0, N, size=N).astype(np.int32)}
    with fl.open(c.path, 'r') as f, fl.open(c.path0, 'r') as f0:
        for key, box in BOXES.items():
            for which, rows in sorted(lists.items()):
                want_rows, want_cell, _ = hoomd.cell_order(c.rows[chunk], box, rows, cells, dimensions=2)
                d_rows = fl._device_from_host(rows, f.pipeline_device())
                cell = f.order_rows_by_cell_device(0, name, box, cells, d_rows, dimensions=2)
                got_rows, got_cell = _host(d_rows), _host(cell)
                assert np.array_equal(got_rows, want_rows) and np.array_equal(got_cell, want_cell), (key, which)
                assert got_cell.dtype == np.int32 and (got_cell != 64).all(), (key, which)      # nobody is "nowhere"
                if _ignores_z(key):
                    d_rows0 = fl._device_from_host(rows, f0.pipeline_device())
                    cell0 = f0.order_rows_by_cell_device(0, name, box, cells, d_rows0, dimensions=2)
                    assert np.array_equal(_host(d_rows0), got_rows) and np.array_equal(_host(cell0), got_cell), (key, which)
        f.wait_read()
        f0.wait_read()


def test_a_flat_frame_with_junk_z_read_end_to_end(tmp_path_factory):
    """configuration.box with Lz == 0 makes the frame two-dimensional by itself; domain, ghost and cell-ordered reads
    take ``dimensions`` from the file and must not let z / 0 near a verdict."""
    n = SIZES[-1]
    rng = np.random.default_rng(2)
    path = os.path.join(_dir(tmp_path_factory, "spatial_e2e"), "pgsd_edges_%d_e2e.gsd" % os.getpid())
    cell = CELLS2[1]
    try:
        _write(path, FLAT0, _flat_positions(rng, n), typeid=_typeid(n), rng=rng)
        with hoomd.open(path, 'r') as t:
            host = t[0]
            assert int(host.configuration.dimensions) == 2 and host.configuration.box[2] == 0
            pos = host.particles.position
            assert np.count_nonzero(pos[:, 2]) >= n // 2
            owned, ghosts, shift = hoomd.halo_rows(pos, FLAT0, cell, WIDTH, dimensions=2)
            assert len(owned) > 0 and len(ghosts) > 0
            s = t.read_frame_device(0, domain=cell, ghost=WIDTH, scalar4=True)
            _check_frame(s, host, np.concatenate([owned, ghosts]), n)
            assert s.n_owned == len(owned) and _same(s.ghost_shift, shift) and s.domain == cell
            assert int(s.configuration.dimensions) == 2
            rows, ids, _ = hoomd.cell_order(pos, FLAT0, hoomd.domain_rows(pos, FLAT0, cell, 2), (8, 8, 1), dimensions=2)
            assert np.array_equal(rows[np.argsort(rows, kind='stable')], owned) and len(set(ids.tolist())) > 4
            s = t.read_frame_device(0, domain=cell, cell_order=(8, 8, 1), scalar4=True)
            _check_frame(s, host, rows, n)
            got_cell = _host(s.cell)
            assert got_cell.dtype == np.int32 and np.array_equal(got_cell, ids) and s.cell_grid == (8, 8, 1)
    finally:
        if os.path.exists(path):
            os.unlink(path)


def _check_frame(s, host, rows, n_global):
    """A domain read against the host frame's rows at the model's row list."""
    tag = _host(s.tag)
    assert tag.dtype == np.int32 and np.array_equal(tag, rows)
    assert s.particles.N == len(rows) and s.particles.N_global == n_global
    for name in FIELDS:
        assert _same(getattr(s.particles, name), getattr(host.particles, name)[rows]), name
    pos4 = np.concatenate([host.particles.position[rows], host.particles.typeid[rows].view(np.float32)[:, None]], 1)
    vel4 = np.concatenate([host.particles.velocity[rows], host.particles.mass[rows][:, None]], 1)
    assert _same(s.particles.pos4, pos4) and _same(s.particles.vel4, vel4)


# ---------------------------------------------------------------------------------------------------- B: non-finite rows
UNEQUAL = dict(x_split=[0.25, 0.5], z_split=[0.375])
GRIDS3 = {"2x2x2": ((2, 2, 2), {}), "3x1x2": ((3, 1, 2), UNEQUAL)}


@pytest.fixture(scope="module")
def nonfinite(tmp_path_factory):
    """9000 rows of the triclinic box: whole-row NaN, +inf in z, -inf in x, NaN in y at co-prime strides, one row of
    -0.0 and one of the largest float32.  Value: path, the rows of both chunks, the type ids, who is somewhere."""
    n = 9000
    rng = np.random.default_rng(77)
    pos = rng.uniform(-3.0, 3.0, size=(n, 3)).astype(np.float32)
    pos[::7] = np.nan
    pos[1::11, 2] = np.inf              # z enters every fraction of the triclinic box
    pos[2::13, 0] = -np.inf             # x enters only its own
    pos[3::17, 1] = np.nan              # y enters x and y
    pos[5] = -0.0
    pos[6] = np.finfo(np.float32).max
    assert np.signbit(pos[5]).all() and np.isfinite(pos[5:7]).all()
    path = os.path.join(_dir(tmp_path_factory, "spatial_nan"), "pgsd_edges_%d_nan.gsd" % os.getpid())
    rows = _write(path, TILT, pos, OFF_GRID, _typeid(n))
    somewhere = {}
    for chunk, p in rows.items():
        assert np.isfinite(p[5:7]).all() and np.signbit(p[5]).all()
        somewhere[chunk] = hoomd.cell_ids(p, TILT, (1, 1, 1)) == 0
        for shape, split in GRIDS3.values():
            counts, nowhere = hoomd.domain_counts(p, TILT, *shape, **split)
            assert nowhere == n - somewhere[chunk].sum() > 1000 and counts.sum() == somewhere[chunk].sum() > 1000
        assert somewhere[chunk][5] and somewhere[chunk][6]
    yield path, rows, _typeid(n), somewhere
    os.unlink(path)


@pytest.mark.parametrize("grid", sorted(GRIDS3))
@pytest.mark.parametrize("chunk", ['position', 'pos64'])
def test_non_finite_rows_belong_to_no_cell_and_no_ghost_layer(nonfinite, chunk, grid):
    path, rows, typeid, somewhere = nonfinite
    pos, name = rows[chunk], _chunk(chunk)
    shape, split = GRIDS3[grid]
    group = hoomd.where_rows({'typeid': typeid}, {'typeid': [0, 2]})
    all_owned, ghosts_seen = [], 0
    with fl.open(path, 'r') as f:
        for cell in hoomd.domain_grid(*shape, **split):
            owned, ghosts, shift = hoomd.halo_rows(pos, TILT, cell, WIDTH)
            assert np.array_equal(owned, hoomd.domain_rows(pos, TILT, cell))
            sel, count = f.select_domain_device(0, name, TILT, cell)
            got = _host(sel)
            assert count == len(owned) and got.dtype == np.int32 and np.array_equal(got, owned), cell
            all_owned.append(got)
            sel, n_owned, n_ghost, got_shift = f.select_halo_device(0, name, TILT, cell, WIDTH)
            got = _host(sel)
            assert (n_owned, n_ghost) == (len(owned), len(ghosts)), cell
            assert np.array_equal(got, np.concatenate([owned, ghosts])) and _same(got_shift, shift), cell
            assert somewhere[chunk][got[n_owned:]].all(), cell              # no nowhere-row in a ghost list
            sel, count = f.select_where_device([(0, 'particles/typeid', 0, [0, 2])], domain=(0, name, cell), box=TILT)
            want = np.intersect1d(group, owned)
            assert count == len(want) and np.array_equal(_host(sel), want), cell
            ghosts_seen += n_ghost
        f.wait_read()
    # the cells own exactly the rows the census does not count as nowhere, each once
    assert np.array_equal(np.sort(np.concatenate(all_owned)), np.flatnonzero(somewhere[chunk]))
    assert ghosts_seen > 1000


# ---------------------------------------------------------------------------------------------------- C: constructed tiles
BOXC = np.array([16.0, 16.0, 16.0, 0.0, 0.0, 0.0], np.float32)
CELL0 = hoomd.domain_grid(2, 1, 1)[0]            # x fraction in [0, 0.5); with a layer of 1/16: bands [15/16, 1) and [0.5, 9/16)
WIDTHC = 1.0                                     # 1/16 of the box on every axis
OUT, IN, GHOST = 0, 1, 2
# x fractions 0.75, 0.25 and 0.5 -- the last one ON the cell's upper plane, the first point of its "above" band (shift 0)
POINTS = np.array([[4.0, 2.0, -6.0], [-4.0, 2.0, -6.0], [0.0, 2.0, -6.0]], np.float32)
COUNTS = [0, 1, 2, 3, 4, 5, 7, 4093, 4094, 4095, 4096]
# where a sparse tile keeps its few rows, (k, lane) of row base + k * 256 + lane: waves 0 and 3 and k = 0 and 15 first
SLOTS = [k * 256 + t for k, t in [(0, 5), (15, 250), (0, 200), (15, 3), (7, 100), (3, 64), (12, 191), (0, 255), (15, 0),
                                  (8, 63), (1, 192), (14, 128)]]
RAGGED = 37
RAGGED_SLOTS = [0, 36, 5, 17, 1, 30, 9, 22]
# per variant the owned and the ghost count of eight full tiles, then of the ragged one; the total owned count of
# variant v is v modulo 4, so its ghost run starts at that residue
VARIANTS = [
    ([4096, 0, 4096, 1, 2, 3, 4, 4094, 0], [0, 4096, 0, 7, 4094, 4093, 7, 2, 4]),
    ([5, 4096, 7, 4093, 4095, 0, 3, 1, 1], [7, 0, 5, 3, 1, 4094, 4, 4095, 0]),
    ([2, 4096, 4094, 0, 1, 4093, 7, 4, 1], [4094, 0, 2, 3, 4095, 1, 5, 7, 7]),
    ([3, 4096, 0, 4096, 5, 2, 4095, 1, 5], [4093, 0, 4096, 0, 3, 4094, 1, 4095, 3]),
]


def _tile_classes(n_in, n_ghost, size, slots):
    """The classes of one tile: the most frequent class fills it, the others sit on ``slots``."""
    want = {IN: n_in, GHOST: n_ghost, OUT: size - n_in - n_ghost}
    assert min(want.values()) >= 0
    fill = max(want, key=lambda c: want[c])
    cls = np.full(size, fill, np.uint32)
    at = 0
    for c in (IN, GHOST, OUT):
        if c != fill:
            cls[slots[at:at + want[c]]] = c
            at += want[c]
    assert at <= len(slots) and [int((cls == c).sum()) for c in (IN, GHOST, OUT)] == [want[IN], want[GHOST], want[OUT]]
    return cls


def _variant_classes(v):
    owned, ghost = VARIANTS[v]
    return np.concatenate([_tile_classes(o, g, RAGGED if i == len(owned) - 1 else TILE,
                                         RAGGED_SLOTS if i == len(owned) - 1 else SLOTS)
                           for i, (o, g) in enumerate(zip(owned, ghost))])


def _starts(counts, first=0):
    """(start offset, count) of every tile's run in the output list."""
    at, out = first, []
    for c in counts:
        out.append((at, c))
        at += c
    return out


def _check_the_variants_cover_the_epilogue():
    assert len(set(SLOTS)) == len(SLOTS) and max(SLOTS) < TILE and max(RAGGED_SLOTS) < RAGGED
    assert {s % 256 // 64 for s in SLOTS[:4]} == {0, 3} and {s // 256 for s in SLOTS[:4]} == {0, 15}
    runs = {"owned": [], "ghost": []}
    for v, (owned, ghost) in enumerate(VARIANTS):
        assert 7 <= len(owned) <= 9 and len(ghost) == len(owned)
        assert sum(owned) % 4 == v                                              # the ghost run starts misaligned
        runs["owned"] += _starts(owned)
        runs["ghost"] += _starts(ghost, sum(owned))
    for which, r in runs.items():
        assert {c for _, c in r} >= set(COUNTS), which                          # every count of the list
        for count in (1, 4093):             # every start residue is reached, by sparse and by (nearly) full tiles
            assert {at % 4 for at, c in r if c >= count} == {0, 1, 2, 3}, which
        assert any(0 < c < (4 - at % 4) % 4 for at, c in r), which              # a tile that keeps fewer rows than its head
        assert any(at % 4 and c > 8 and (at + c) % 4 for at, c in r), which     # head, 16-byte stores and a tail in one tile
    assert {at % 4 for at, c in runs["owned"] if c == TILE} == {0, 1, 2, 3}
    assert any(o[i:i + 3] == [TILE, 0, TILE] for o, _ in VARIANTS for i in range(len(o) - 2))   # empty between two full


_check_the_variants_cover_the_epilogue()


class _Built:
    def __init__(self, path, cls):
        self.path, self.cls, self.N = path, cls, len(cls)
        self.owned, self.ghosts = np.flatnonzero(cls == IN), np.flatnonzero(cls == GHOST)
        self.shift = np.zeros((len(self.ghosts), 3), np.int32)


def _build(path, cls, typeid=True):
    """The file of a class array, and the construction checked against the models on both chunks."""
    rows = _write(path, BOXC, POINTS[cls], 1.0, cls.astype(np.uint32) if typeid else None)
    c = _Built(path, cls)
    for p in rows.values():
        assert np.array_equal(hoomd.domain_rows(p, BOXC, CELL0), c.owned)
        owned, ghosts, shift = hoomd.halo_rows(p, BOXC, CELL0, WIDTHC)
        assert np.array_equal(owned, c.owned) and np.array_equal(ghosts, c.ghosts) and np.array_equal(shift, c.shift)
    return c


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = _dir(tmp_path_factory, "spatial_tiles")
    out = []
    for v in range(len(VARIANTS)):
        c = _build(os.path.join(d, "pgsd_edges_%d_tiles%d.gsd" % (os.getpid(), v)), _variant_classes(v))
        assert c.N == 8 * TILE + RAGGED and len(c.owned) % 4 == v and len(c.ghosts) > 0
        out.append(c)
    yield out
    for c in out:
        os.unlink(c.path)


@pytest.mark.parametrize("chunk", ['position', 'pos64'])
@pytest.mark.parametrize("v", range(len(VARIANTS)))
def test_constructed_tiles_through_the_domain_and_ghost_selections(built, v, chunk):
    c, name = built[v], _chunk(chunk)
    with fl.open(c.path, 'r') as f:
        rows, count = f.select_domain_device(0, name, BOXC, CELL0)
        got = _host(rows)
        assert count == len(c.owned) and got.dtype == np.int32 and np.array_equal(got, c.owned)
        rows, n_owned, n_ghost, shift = f.select_halo_device(0, name, BOXC, CELL0, WIDTHC)
        got = _host(rows)
        assert (n_owned, n_ghost) == (len(c.owned), len(c.ghosts))
        assert np.array_equal(got[:n_owned], c.owned) and np.array_equal(got[n_owned:], c.ghosts)
        assert _same(shift, c.shift)
        f.wait_read()


@pytest.mark.parametrize("v", range(len(VARIANTS)))
def test_constructed_tiles_through_the_group_selection(built, v):
    c = built[v]
    both = np.flatnonzero(c.cls != OUT)
    with fl.open(c.path, 'r') as f:
        for members, want in (([IN], c.owned), ([GHOST], c.ghosts), ([IN, GHOST], both)):
            rows, count = f.select_where_device([(0, 'particles/typeid', 0, members)])
            assert count == len(want) and np.array_equal(_host(rows), want), members
        for name in ('particles/position', 'log/pos64'):
            rows, count = f.select_where_device([(0, 'particles/typeid', 0, [IN, GHOST])], domain=(0, name, CELL0), box=BOXC)
            assert count == len(c.owned) and np.array_equal(_host(rows), c.owned), name
        f.wait_read()


@pytest.mark.parametrize("v", range(len(VARIANTS)))
def test_constructed_tiles_through_the_flag_compaction(built, v):
    """The same keep-masks as uint8 flags, the flag pointer on and 1, 2, 3 bytes off a 16-byte boundary."""
    c = built[v]
    values = (1 + np.arange(c.N) % 255).astype(np.uint8)
    for keep, want in ((c.cls == IN, c.owned), (c.cls == GHOST, c.ghosts), (c.cls != OUT, np.flatnonzero(c.cls != OUT))):
        flags = torch.from_numpy(np.where(keep, values, 0).astype(np.uint8))
        for off in range(4):
            buf = torch.zeros((c.N + 16,), dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            buf[off:off + c.N].copy_(flags)
            index, count = fl.select_rows(buf[off:off + c.N])
            got = _host(index)
            assert count == len(want) and got.dtype == np.int32 and np.array_equal(got, want), off


def test_more_than_256_tiles_take_the_scan_through_a_second_trip(tmp_path_factory):
    """256 * 4096 + 1 rows are 257 tiles: the one-block scan of the tile counts takes a second trip, with the carry of
    the first.  Tiles keep 0, 4096 and 1 rows in turn; the ghosts likewise."""
    n = 256 * TILE + 1
    parts = []
    for t in range(256):
        if t % 3 == 1:
            parts.append(_tile_classes(TILE, 0, TILE, SLOTS))
        elif t % 3 == 2:
            parts.append(_tile_classes(1, 1, TILE, SLOTS[t % 12:] + SLOTS[:t % 12]))
        else:
            parts.append(_tile_classes(0, TILE if t % 6 == 0 else 1, TILE, SLOTS[t % 12:] + SLOTS[:t % 12]))
    parts.append(np.full(1, IN, np.uint32))                     # the tile of the second trip owns its one row
    cls = np.concatenate(parts)
    assert len(cls) == n and (n + TILE - 1) // TILE == 257
    path = os.path.join(_dir(tmp_path_factory, "spatial_trip"), "pgsd_edges_%d_trip.gsd" % os.getpid())
    try:
        c = _build(path, cls, typeid=False)
        assert c.owned[-1] == n - 1 and len(c.owned) > 85 * TILE and len(c.ghosts) > 42 * TILE
        with fl.open(path, 'r') as f:
            for name in ('particles/position', 'log/pos64'):
                rows, count = f.select_domain_device(0, name, BOXC, CELL0)
                assert count == len(c.owned) and np.array_equal(_host(rows), c.owned), name
                rows, n_owned, n_ghost, shift = f.select_halo_device(0, name, BOXC, CELL0, WIDTHC)
                got = _host(rows)
                assert (n_owned, n_ghost) == (len(c.owned), len(c.ghosts)), name
                assert np.array_equal(got[:n_owned], c.owned) and np.array_equal(got[n_owned:], c.ghosts), name
                assert _same(shift, c.shift), name
            f.wait_read()
    finally:
        if os.path.exists(path):
            os.unlink(path)
