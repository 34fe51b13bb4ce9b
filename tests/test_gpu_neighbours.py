"""The neighbour census on the GPU: pgsd_neighbours_device behind pgsd.fl's neighbours_device and pgsd.hoomd's
frame_neighbours_device.  Every result must equal the numpy model pgsd.hoomd.particle_neighbours / frame_neighbours exactly
-- every counter and index with numpy.array_equal, nearest2 and closest2 bit for bit (tests/test_neighbours_model.py
checks the model itself against a double loop and against a search over all pairs).  The cases at the pgsd.fl level read
constructed position chunks, once as float32 and once as float64, and order the list on the GPU first, as a caller does."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402
from pgsd import _lib  # noqa: E402
from neighbours_cases import FLAT, MUTATIONS, NONE, ORTHO, TRICLINIC, random_rows  # noqa: E402

CUBE = [8, 8, 8, 0, 0, 0]
WIDE = [64, 64, 64, 0, 0, 0]
N = 20_011
TYPES = ['fluid', 'wall', 'inlet']
DTYPES = {'f32': np.float32, 'f64': np.float64}


def _through(box, f):
    """Fractions in [0, 1) (or slightly outside) -> real coordinates of the box, float64."""
    Lx, Ly, Lz, xy, xz, yz = [float(np.float32(b)) for b in box]
    g = np.asarray(f, np.float64) - 0.5
    z = g[:, 2] * Lz
    y = g[:, 1] * Ly + yz * z
    return np.stack([g[:, 0] * Lx + xy * (g[:, 1] * Ly) + xz * z, y, z], axis=1)


def _faces():
    """Rows on cell faces of the (7, 5, 4) grid, at fraction 0 and just below 1, slightly outside the box, and a partner a
    short way off each of them: pairs across every periodic face and across the corners of the tilted box."""
    fx = [0.0, 1 / 7, 2 / 7, 0.5, 0.9999999, -0.005, 1.004]
    fy = [0.0, 0.2, 0.5, 0.9999999, 1.003]
    fz = [0.0, 0.25, 0.9999999, -0.004]
    f = np.array([(a, b, c) for a in fx for b in fy for c in fz])
    base = _through(TRICLINIC, f)
    rng = np.random.default_rng(21)
    return np.concatenate([base, base + rng.uniform(-0.6, 0.6, size=base.shape)])


def _half_box():
    """Rows at -L/2 and at the largest float32 below +L/2 on every axis of the orthorhombic box, and neighbours of them."""
    lo = -np.array(ORTHO[:3], np.float64) / 2
    hi = np.nextafter((np.array(ORTHO[:3]) / 2).astype(np.float32), np.float32(0)).astype(np.float64)
    rows = [lo, hi, [lo[0], 0, 0], [hi[0], 0, 0], [0, lo[1], 0], [0, hi[1], 0], [0, 0, lo[2]], [0, 0, hi[2]],
            [lo[0], hi[1], lo[2]], [hi[0], lo[1], hi[2]], [lo[0] + 0.3, 0.1, 0], [0.2, hi[1] - 0.4, 0.1], [0, 0.3, lo[2] + 0.5]]
    return np.concatenate([np.array(rows, np.float64), random_rows(5, 51, ORTHO, np.float64)])


def _on_edges():
    """Pairs exactly on bin edges for r = 1 and bins 1, 7 and 1024: distances k * (1 / 7) and k / 1024 from well-separated
    rows, and 0 (a row stored twice)."""
    w = np.float64(1.0) / np.float64(7)
    rows = [[0, 0, 0]] + [[k * w, 0, 0] for k in range(1, 7)]
    rows += [[0, 3, 0]] + [[0, 3 + k / 1024, 0] for k in (1, 2, 512, 1023)]
    rows += [[3, 0, 3], [3, 0, 3], [-3, -3, -3], [-3 + 1.0, -3, -3]]           # distance 0, and distance r itself
    return np.concatenate([np.array(rows, np.float64), random_rows(6, 200, CUBE, np.float64)])


def _clump():
    """700 entries inside one cell of the (3, 3, 3) grid -- longer than a workgroup -- with empty cells beside it, and a few
    rows elsewhere."""
    rng = np.random.default_rng(8)
    return np.concatenate([rng.uniform(-0.5, 0.5, size=(700, 3)), [[3.5, 3.5, 3.5], [3.6, 3.5, 3.5], [-3.9, 0, 0]]])


def _sparse():
    """3 000 rows in 64^3 cells: mostly empty cells; 750 of the rows have a partner inside the range."""
    a = random_rows(9, 2250, WIDE, np.float64)
    return np.concatenate([a, a[:750] + np.random.default_rng(10).uniform(-0.5, 0.5, size=(750, 3))])


def _with_lost_rows(p, every=97):
    p = p.copy()
    p[5::every, 0] = np.nan
    p[11::every, 1] = np.inf
    return p


# name -> (positions as float64, keyword arguments of particle_neighbours besides position)
CASES = {
    'one_cell_65': (random_rows(1, 65, CUBE, np.float64), dict(box=CUBE, r=2.0, cells=(1, 1, 1))),
    'two_cells_64': (random_rows(2, 64, CUBE, np.float64), dict(box=CUBE, r=2.0, cells=(2, 2, 2))),
    'flat_63': (random_rows(3, 63, FLAT, np.float64, 2), dict(box=FLAT, r=1.3, cells=(2, 3, 1), dimensions=2)),
    'flat_z_ignored': (random_rows(3, 300, FLAT, np.float64, 3), dict(box=FLAT, r=0.6, dimensions=2)),
    'three_cells_4097': (_with_lost_rows(random_rows(4, 4097, CUBE, np.float64)), dict(box=CUBE, r=2.0, cells=(3, 3, 3))),
    'triclinic_754': (_with_lost_rows(random_rows(5, 3000, TRICLINIC, np.float64)), dict(box=TRICLINIC, r=1.3, cells=(7, 5, 4))),
    'sparse_64cubed': (_sparse(), dict(box=WIDE, r=1.0, cells=(64, 64, 64))),
    'about_20000': (_with_lost_rows(random_rows(6, N, TRICLINIC, np.float64), 997), dict(box=TRICLINIC, r=0.61)),
    'clump_700': (_clump(), dict(box=CUBE, r=2.0, cells=(3, 3, 3))),
    'all_nowhere': (np.full((100, 3), np.nan), dict(box=CUBE, r=1.0)),
    'faces': (_faces(), dict(box=TRICLINIC, r=1.3, cells=(7, 5, 4))),
    'half_box': (_half_box(), dict(box=ORTHO, r=1.3)),
    'on_edges': (_on_edges(), dict(box=CUBE, r=1.0)),
    'boundary': (np.array([[0, 0, 0], [0.5, 0, 0]], np.float64), dict(box=CUBE, r=0.5)),
    # x axes of 4 and 5 cells, the smallest at which the first and last cell of a row take two x-runs and the inner
    # ones one (and one of 1 beside them); test_a_case_equals_the_model walks these with a pair histogram as well
    'x_runs_444': (random_rows(40, 400, CUBE, np.float64), dict(box=CUBE, r=2.0, cells=(4, 4, 4))),
    'x_runs_511': (random_rows(41, 300, CUBE, np.float64), dict(box=CUBE, r=1.6, cells=(5, 1, 1))),
    'x_runs_flat_421': (random_rows(42, 300, FLAT, np.float64, 2), dict(box=FLAT, r=1.3, cells=(4, 2, 1), dimensions=2)),
    'x_runs_triclinic_154': (random_rows(43, 300, TRICLINIC, np.float64), dict(box=TRICLINIC, r=1.3, cells=(1, 5, 4))),
}
for _k, (_name, (_switch, _case)) in enumerate(sorted(MUTATIONS.items())):
    _kw = dict(_case)
    CASES['mutation_%02d' % _k] = (np.asarray(_kw.pop('position'), np.float64), _kw)
MUTATION_CASE = dict((name, 'mutation_%02d' % k) for k, name in enumerate(sorted(MUTATIONS)))


def chunk(name, key):
    return 'log/%s_%s' % (name, key)


def _dir(tmp_path_factory, name):
    return "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp(name))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """One file of one frame: 20 011 particles with types, a density and random positions in the triclinic box (the
    pgsd.hoomd level), and every case's positions as a float32 and a float64 log chunk.  The host's arrays beside it."""
    path = os.path.join(_dir(tmp_path_factory, "neighbours"), "pgsd_neighbours_%d.gsd" % os.getpid())
    rng = np.random.default_rng(N)
    fr = hoomd.Frame()
    fr.configuration.box = TRICLINIC
    fr.particles.N = N
    fr.particles.types = TYPES
    fr.particles.position = _with_lost_rows(random_rows(7, N, TRICLINIC, np.float32), 997)
    fr.particles.typeid = rng.integers(0, len(TYPES), size=N).astype(np.uint32)
    fr.particles.density = (1000.0 + 50.0 * rng.standard_normal(N)).astype(np.float32)
    fr.particles.mass = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
    arrays = {}
    for name, (p, _) in CASES.items():
        for key, dt in DTYPES.items():
            arrays[chunk(name, key)] = fr.log['%s_%s' % (name, key)] = np.ascontiguousarray(p.astype(dt))
    with hoomd.open(path, 'w') as t:
        t.append(fr)
    yield path, arrays
    os.unlink(path)


def to_device(f, a):
    return fl._device_from_host(np.ascontiguousarray(a, dtype=np.int32), f.pipeline_device())


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr() if hasattr(x, 'data_ptr') else x.ptr)


def equal(got, want, what):
    """The kernel's Neighbours (per-entry arrays in GPU memory) against the model's."""
    assert np.array_equal(got.summary, want.summary), (what, got, want)
    assert np.float64(got.closest2).view(np.uint64) == np.float64(want.closest2).view(np.uint64), what
    assert got.grid == want.grid and got.bins == want.bins and got.closest_rows == want.closest_rows, what
    if got.count is not None:
        assert np.array_equal(_host(got.rows), want.rows) and np.array_equal(_host(got.cell), want.cell), what
        assert np.array_equal(_host(got.count).view(np.uint32), want.count), what
        assert np.array_equal(_host(got.nearest).view(np.uint32), want.nearest), what
        assert np.array_equal(_host(got.nearest2).view(np.uint64), want.nearest2.view(np.uint64)), what
    return True


def census(f, name, host, rows=None, bins=0, return_rows=True, **kw):
    """Order the list on the GPU, run the pass; the model beside it."""
    box, r, dims = kw['box'], kw['r'], kw.get('dimensions', 3)
    want = hoomd.particle_neighbours(host, rows=rows, bins=bins, **kw)
    every = np.arange(len(host)) if rows is None else np.asarray(rows)
    d_rows = to_device(f, every)
    d_cell = f.order_rows_by_cell_device(0, name, box, want.grid, d_rows, n=len(every), dimensions=dims)
    got = f.neighbours_device(0, name, box, r, want.grid, d_rows, d_cell, n=len(every), dimensions=dims, bins=bins,
                              return_rows=return_rows)
    return got, want


# ---------------------------------------------------------------- constructed cases
@pytest.mark.parametrize("key", sorted(DTYPES))
@pytest.mark.parametrize("name", [c for c in sorted(CASES) if not c.startswith('mutation')])
def test_a_case_equals_the_model(data, name, key):
    path, arrays = data
    host, kw = arrays[chunk(name, key)], CASES[name][1]
    with fl.open(path, 'r') as f:
        got, want = census(f, chunk(name, key), host, **kw)
        assert equal(got, want, (name, key))
        if name.startswith('x_runs'):       # the HIST instances over the same runs; no entry is without a neighbour
            binned, model = census(f, chunk(name, key), host, bins=3, **kw)
            assert equal(binned, model, (name, key, 3)) and int(binned.pair_hist.sum()) == binned.pairs == got.pairs
            assert got.nowhere == 0 and got.count_min >= 1
        f.wait_read()
    assert want.n == len(host) and int(want.count_hist.sum()) + want.nowhere == want.n
    if name == 'all_nowhere':
        assert got.nowhere == 100 and got.pairs == 0 and got.closest == NONE and got.closest2 == np.inf
    if name == 'clump_700':
        assert got.count_max == 699 and got.count_hist[256] == 700      # every pair of the clump lies inside r
    if name == 'sparse_64cubed':
        assert got.grid == (64, 64, 64) and got.isolated > 100 and got.pairs > 1000
    if name == 'about_20000':
        assert 30 < got.mean_count < 50 and got.nowhere > 0
    if name in ('faces', 'half_box'):
        assert got.pairs > 0
    if name == 'flat_z_ignored':
        assert got.dimensions == 2 and got.pairs > 0


@pytest.mark.parametrize("key", sorted(DTYPES))
def test_lists_of_0_1_63_64_65_entries_repeats_and_any_order(data, key):
    """n in {0, 1, 63, 64, 65}; a list in descending order with rows listed twice (distance 0 between two entries)."""
    path, arrays = data
    name = chunk('three_cells_4097', key)
    host, kw = arrays[name], CASES['three_cells_4097'][1]
    with fl.open(path, 'r') as f:
        for n in (0, 1, 63, 64, 65):
            got, want = census(f, name, host, rows=np.arange(100, 100 + n), bins=3, **kw)
            assert equal(got, want, (key, n)) and got.n == n
        rows = np.concatenate([np.arange(400, 0, -1), [7, 7, 400, 12]])
        got, want = census(f, name, host, rows=rows, **kw)
        assert equal(got, want, key) and got.closest2 == 0.0 and got.n == 404
        assert _host(got.nearest2).min() == 0.0
        f.wait_read()


def test_the_strict_boundary(data):
    """Rows (0, 0, 0) and (0.5, 0, 0): with r = 0.5 the pair is not counted, with the next double above it is."""
    path, arrays = data
    for key in sorted(DTYPES):
        name = chunk('boundary', key)
        with fl.open(path, 'r') as f:
            got, want = census(f, name, arrays[name], box=CUBE, r=0.5)
            assert equal(got, want, key) and got.pairs == 0 and got.isolated == 2
            got, want = census(f, name, arrays[name], box=CUBE, r=float(np.nextafter(0.5, 1)))
            assert equal(got, want, key) and got.pairs == 2 and got.closest2 == 0.25 and got.closest_rows == (0, 1)
            f.wait_read()


@pytest.mark.parametrize("bins", [1, 7, 1024])
@pytest.mark.parametrize("key", sorted(DTYPES))
def test_the_pair_histogram_with_pairs_on_edges(data, key, bins):
    path, arrays = data
    name = chunk('on_edges', key)
    host = arrays[name]
    with fl.open(path, 'r') as f:
        got, want = census(f, name, host, bins=bins, box=CUBE, r=1.0)
        assert equal(got, want, (key, bins)) and int(got.pair_hist.sum()) == got.pairs > 0
        f.wait_read()
    edges2 = hoomd.neighbour_edges2(1.0, bins)
    if key == 'f64' and bins == 7:      # row k at distance k * (1 / 7) from row 0: exactly on edge k, hence in bin k
        d2 = hoomd.pair_distance2(host[0], host[1:7], hoomd.box_vectors(CUBE))
        assert (d2 == edges2[1:7]).all()
    if bins == 1024:                    # k / 1024 is exact in both element types
        d2 = hoomd.pair_distance2(host[7], host[8:12], hoomd.box_vectors(CUBE))
        assert (d2 == edges2[[1, 2, 512, 1023]]).all()


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_the_kernel_on_every_mutation_case(data, mutation):
    """The case on which the mutated loop differs from the model (tests/test_neighbours_model.py): the kernel equals the
    model there, so it does not hold the mutation."""
    path, arrays = data
    name = MUTATION_CASE[mutation]
    kw = CASES[name][1]
    key = 'f64' if MUTATIONS[mutation][1]['position'].dtype == np.float64 else 'f32'
    with fl.open(path, 'r') as f:
        got, want = census(f, chunk(name, key), arrays[chunk(name, key)], **kw)
        assert equal(got, want, mutation)
        f.wait_read()


# ---------------------------------------------------------------- staging, the per-entry outputs
def test_a_second_call_is_served_from_the_staged_chunk_and_return_rows(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    host, kw = arrays[name], CASES['triclinic_754'][1]
    with fl.open(path, 'r') as f:
        f.device_read_stats(reset=True)
        got, want = census(f, name, host, bins=7, **kw)                         # the ordering stages the chunk
        assert f.device_read_stats()["pread_bytes"] == len(host) * 12 and equal(got, want, "first")
        got, _ = census(f, name, host, bins=7, return_rows=False, **kw)
        assert f.device_read_stats()["pread_bytes"] == len(host) * 12 and equal(got, want, "second")
        assert got.rows is None and got.cell is None and got.count is None and got.nearest2 is None and got.nearest is None
        f.wait_read()
        f.device_read_stats(reset=True)
        got, _ = census(f, name, host, **kw)
        assert f.device_read_stats()["pread_bytes"] == len(host) * 12           # released by wait_read: read again
        assert _host(got.count).dtype == np.int32 and _host(got.nearest2).dtype == np.float64
        f.wait_read()


# ---------------------------------------------------------------- refusals
def test_what_the_python_layers_refuse(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    with fl.open(path, 'r') as f:
        rows = to_device(f, np.arange(100))
        cell = f.order_rows_by_cell_device(0, name, TRICLINIC, (7, 5, 4), rows, n=100)

        def call(name=name, box=TRICLINIC, r=1.3, cells=(7, 5, 4), rows=rows, cell=cell, **kw):
            return f.neighbours_device(0, name, box, r, cells, rows, cell, **kw)

        for kw, message in ((dict(r=0.0), "finite and positive"), (dict(r=float('nan')), "finite and positive"),
                            (dict(r=float('inf')), "finite and positive"), (dict(cells=(8, 5, 4)), "narrower"),
                            (dict(cells=(7, 5)), "three counts"), (dict(cells=(0, 5, 4)), "1 to 1024"),
                            (dict(r=3.01, cells=(1, 1, 1)), "count twice"), (dict(bins=1025), "1024 bins"),
                            (dict(dimensions=2), "one z cell"), (dict(dimensions=4, cells=(1, 1, 1)), "dimensions is 2 or 3"),
                            (dict(n=101), "fewer entries than n"), (dict(name='particles/typeid'), "float32 or float64"),
                            (dict(name='particles/mass'), "3 columns"), (dict(box=[1, 2, 3]), "6 values"),
                            (dict(box=WIDE, r=0.05, cells=(1024, 1024, 2)), "2\\^20 cells")):
            with pytest.raises(ValueError, match=message):
                call(**kw)
        with pytest.raises(KeyError):
            call(name='log/nothing')
        f.wait_read()


def test_every_refusal_has_its_message_and_leaves_the_outputs_untouched(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    host = arrays[name]
    n, bins = 500, 4
    want = hoomd.particle_neighbours(host, TRICLINIC, 1.3, rows=np.arange(n), cells=(7, 5, 4), bins=bins)
    fn = _lib.lib.pgsd_neighbours_device
    fn.restype = ctypes.c_int32
    D, U = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    fn.argtypes = [ctypes.POINTER(_lib.Handle), ctypes.POINTER(_lib.IndexEntry), D, ctypes.c_double, ctypes.c_uint32, U,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, D, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), D]
    with fl.open(path, 'r') as f:
        h = f._h()

        def entry_of(chunk_name):
            return _lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(h, 0, chunk_name.encode()).contents)

        d_rows, d_cell = to_device(f, want.rows), to_device(f, want.cell)
        descending, outside_cell, outside_row = want.cell.copy(), want.cell.copy(), want.rows.copy()
        descending[300] = 0
        outside_cell[n - 1] = 141
        outside_row[7] = len(host)
        d_desc, d_outc, d_outr = to_device(f, descending), to_device(f, outside_cell), to_device(f, outside_row)
        words = 8 + 257 + bins
        summary = (ctypes.c_uint64 * words)(*([77] * words))
        closest2 = ctypes.c_double(77.0)
        out_count, out_nearest = to_device(f, np.full(n, 77)), to_device(f, np.full(n, 77))
        out_nearest2 = fl._device_from_host(np.full(n, 77.0), f.pipeline_device())
        good = dict(entry=entry_of(name), vectors=hoomd.box_vectors(np.asarray(TRICLINIC, np.float32)), r=1.3, dims=3,
                    cells=(7, 5, 4), rows=d_rows, cell=d_cell, n=n, bins=bins, edges2=hoomd.neighbour_edges2(1.3, bins))

        def raw(**changes):
            a = dict(good, **changes)
            return fn(h, ctypes.byref(a['entry']), (ctypes.c_double * 6)(*a['vectors']), a['r'], a['dims'],
                      (ctypes.c_uint32 * 3)(*a['cells']), _ptr(a['rows']), _ptr(a['cell']), a['n'], a['bins'],
                      (ctypes.c_double * len(a['edges2']))(*a['edges2']), _ptr(out_count), _ptr(out_nearest2), _ptr(out_nearest),
                      summary, ctypes.byref(closest2))

        huge = entry_of(name)
        huge.N = 2 ** 32
        flat_vectors = hoomd.box_vectors(np.asarray(FLAT, np.float32))
        wide_vectors = hoomd.box_vectors(np.asarray([2000, 2000, 2000, 0, 0, 0], np.float32))
        down = good['edges2'].copy()
        down[2] = down[1] / 2
        gap = good['edges2'].copy()
        gap[3] = np.nan
        for changes, message in (
                (dict(entry=entry_of('particles/typeid')), "float32 or float64"), (dict(entry=entry_of('particles/mass')), "3 columns"),
                (dict(entry=huge), "2^32 rows"), (dict(n=2 ** 32), "2^32 entries"), (dict(dims=4), "dimensions is 2 or 3"),
                (dict(r=0.0), "finite and positive"), (dict(r=-1.0), "finite and positive"),
                (dict(r=float('inf')), "finite and positive"), (dict(r=float('nan')), "finite and positive"),
                (dict(vectors=[10, 0, 6, 0, 0, 0]), "box lengths"), (dict(cells=(0, 5, 4)), "1 to 1024 cells"),
                (dict(cells=(1025, 5, 4)), "1 to 1024 cells"), (dict(cells=(8, 5, 4)), "narrower than the range"),
                (dict(cells=(7, 6, 4)), "narrower than the range"), (dict(cells=(7, 5, 5)), "narrower than the range"),
                (dict(dims=2, vectors=flat_vectors, cells=(2, 3, 2)), "one z cell"),
                (dict(r=3.01, cells=(1, 1, 1)), "count twice"), (dict(vectors=wide_vectors, r=1.0, cells=(1024, 1024, 2)), "2^20 cells"),
                (dict(bins=1025, edges2=np.zeros(1026)), "1024 bins"), (dict(edges2=down), "descend"), (dict(edges2=gap), "descend"),
                (dict(cell=d_desc), "descends or lies outside"), (dict(cell=d_outc), "descends or lies outside"),
                (dict(rows=d_outr), "outside the position chunk"), (dict(cells=(7, 5, 3)), "descends or lies outside")):
            assert raw(**changes) == _lib.ERROR_INVALID_ARGUMENT and message in _lib.last_error(), (message, _lib.last_error())
            assert list(summary) == [77] * words and closest2.value == 77.0, message
            assert _host(out_count).tolist() == [77] * n and _host(out_nearest).tolist() == [77] * n, message
            assert _host(out_nearest2).tolist() == [77.0] * n, message
        # the same call as it is: correct, and n == 0 is the summary of no entry
        assert raw() == 0
        assert np.array_equal(np.array(list(summary), np.uint64), want.summary)
        assert np.float64(closest2.value).view(np.uint64) == np.float64(want.closest2).view(np.uint64)
        assert np.array_equal(_host(out_count).view(np.uint32), want.count)
        assert np.array_equal(_host(out_nearest).view(np.uint32), want.nearest)
        assert np.array_equal(_host(out_nearest2).view(np.uint64), want.nearest2.view(np.uint64))
        assert raw(n=0) == 0
        assert list(summary) == [0] * 5 + [NONE] * 3 + [0] * (257 + bins) and closest2.value == np.inf
        f.wait_read()


# ---------------------------------------------------------------- through pgsd.hoomd
WHERE = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
CELL = hoomd.domain_grid(2, 2, 1)[1]
SELECTIONS = {"all": {}, "where": {'where': WHERE}, "domain": {'domain': CELL}, "both": {'where': WHERE, 'domain': CELL}}


@pytest.mark.parametrize("selection", sorted(SELECTIONS))
def test_frame_neighbours_device_equals_the_host_model(data, selection):
    path, _ = data
    kwargs = SELECTIONS[selection]
    with hoomd.open(path, 'r') as t:
        for options in (dict(r=0.61), dict(r=1.3, bins=16, cells=(5, 5, 3))):
            want = t.frame_neighbours(0, **options, **kwargs)
            t.file.device_read_stats(reset=True)
            got = t.frame_neighbours_device(0, return_rows=True, **options, **kwargs)
            pread = t.file.device_read_stats()["pread_bytes"]
            assert equal(got, want, (selection, options))
            # the position is read once -- by the selection, the ordering or the pass --, and the selection's typeid and density
            assert pread == N * (12 + (8 if 'where' in kwargs else 0)), (selection, options)
        summary_only = t.frame_neighbours_device(0, r=0.61, **kwargs)
        assert summary_only.count is None and np.array_equal(summary_only.summary, t.frame_neighbours(0, r=0.61, **kwargs).summary)
        if selection == "all":
            assert got.n == N and got.nowhere > 0
        else:
            assert 0 < got.n < N
        with pytest.raises(ValueError, match="narrower"):
            t.frame_neighbours_device(0, 1.3, cells=(8, 5, 4), **kwargs)
        with pytest.raises(ValueError, match="count twice"):
            t.frame_neighbours_device(0, 3.5, **kwargs)
        with pytest.raises(ValueError, match="bins"):
            t.frame_neighbours_device(0, 1.3, bins=1025, **kwargs)
        with pytest.raises(IndexError):
            t.frame_neighbours_device(1, 1.3)
