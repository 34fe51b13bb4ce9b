"""The SPH samples on the GPU: pgsd_sph_samples_device behind pgsd.fl's sph_samples_device and pgsd.hoomd's
frame_samples_device.  Every per-point array and every summary word must equal the numpy model pgsd.hoomd.sph_samples /
frame_samples exactly, the floats bit for bit (tests/test_sph_sample_model.py holds the model against a plain double loop;
a NaN equals a NaN, whose sign and payload IEEE 754 leaves to the processor).  The cases at the pgsd.fl level read
constructed chunks, once with float32 and once with float64 positions and columns, with both kernels, normalised and not,
and order the list on the GPU first, as a caller does.  A model result is computed once and shared."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402
from pgsd import _lib  # noqa: E402
from neighbours_cases import FLAT, TRICLINIC, random_rows  # noqa: E402
from sph_cases import KERNELS, NONE, WIDE, bits_equal  # noqa: E402
from sph_gradient_cases import velocities  # noqa: E402
from sph_force_cases import pressures  # noqa: E402
from sph_sample_cases import CASES as SHARED_CASES, MUTATIONS, WIDTHS, _small, special_points, value_arrays, words_equal  # noqa: E402

N = 20_011
N1 = 5_003
TYPES = ['fluid', 'wall', 'inlet']
DTYPES = {'f32': np.float32, 'f64': np.float64}
CASES = dict(SHARED_CASES)          # (and behind them the mutation cases and one case per number of columns, as chunks)
MUTATION_CASE = {}
for _k, (_name, (_switch, _case)) in enumerate(sorted(MUTATIONS.items())):
    MUTATION_CASE[_name] = 'mutation_%02d' % _k
    CASES['mutation_%02d' % _k] = dict(_case)
for _C in sorted(WIDTHS):
    CASES['columns_%d' % _C] = dict(_small(50 + _C), values=value_arrays(50 + _C, 60, _C))
_MODEL = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chunk(name, key):
    return 'log/%s_%s' % (name, key)


def _dir(tmp_path_factory, name):
    return "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp(name))


def _lost(p, every=997):
    p = p.copy()
    p[5::every, 0] = np.nan
    p[11::every, 1] = np.inf
    return p


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """One file of two frames.  Frame 0: 20 011 particles with types, velocities, masses, densities, pressures, a uniform
    slength of 0.305 and random positions in the triclinic box (the pgsd.hoomd level; auxiliary1 is stored nowhere), and
    every case's positions as a float32 and a float64 log chunk with its mass, density and value columns in both element
    types.  Frame 1: 5 003 other particles with a slength that is not uniform and nothing else stored (a frame at rest).
    The host's arrays beside it."""
    path = os.path.join(_dir(tmp_path_factory, "sphs"), "pgsd_sph_samples_%d.gsd" % os.getpid())
    rng = np.random.default_rng(N)
    fr = hoomd.Frame()
    fr.configuration.box = TRICLINIC
    fr.particles.N = N
    fr.particles.types = TYPES
    fr.particles.position = _lost(random_rows(7, N, TRICLINIC, np.float32))
    fr.particles.velocity = velocities(7, N).astype(np.float32)
    fr.particles.typeid = rng.integers(0, len(TYPES), size=N).astype(np.uint32)
    fr.particles.density = (1000.0 + 50.0 * rng.standard_normal(N)).astype(np.float32)
    fr.particles.mass = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
    fr.particles.pressure = pressures(7, N).astype(np.float32)
    fr.particles.slength = np.full(N, 0.305, np.float32)
    arrays = {}
    for name, case in CASES.items():
        for key, dt in DTYPES.items():
            columns = [('', case['position']), ('_mass', case.get('mass')), ('_density', case.get('density'))]
            columns += [('_value%d' % k, v) for k, v in enumerate(case['values'])]
            for suffix, values in columns:
                if values is not None:
                    arrays[chunk(name + suffix, key)] = fr.log['%s%s_%s' % (name, suffix, key)] = \
                        np.ascontiguousarray(np.asarray(values).astype(dt))
    with hoomd.open(path, 'w') as t:
        t.append(fr)
        other = hoomd.Frame()
        other.configuration.box = TRICLINIC
        other.particles.N = N1
        other.particles.types = TYPES
        other.particles.position = _lost(random_rows(8, N1, TRICLINIC, np.float32))
        other.particles.slength = np.where(np.arange(N1) == 4321, 0.31, 0.305).astype(np.float32)
        t.append(other)
    yield path, arrays
    os.unlink(path)


def to_device(f, a, dtype=np.int32):
    return fl._device_from_host(np.ascontiguousarray(a, dtype=dtype), f.pipeline_device())


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr() if hasattr(x, 'data_ptr') else x.ptr)


def equal(got, want, what):
    """The kernel's KernelSamples (per-point arrays in GPU memory) against the model's."""
    assert words_equal(got.summary, want.summary), (what, got, want, got.summary, want.summary)
    assert got.grid == want.grid and got.kernel == want.kernel and got.h == want.h and got.sigma == want.sigma, what
    assert got.dimensions == want.dimensions and got.normalise == want.normalise and got.columns == want.columns, what
    for name in ('points', 'nowhere', 'outside', 'empty', 'not_finite', 'count_max', 'count_max_at'):
        assert getattr(got, name) == getattr(want, name), (what, name)
    count = _host(got.count)
    assert count.dtype == np.uint32 and np.array_equal(count, want.count), what
    for name in ('density', 'shepard', 'values'):
        mine, theirs = _host(getattr(got, name)), getattr(want, name)
        assert mine.shape == theirs.shape and mine.dtype == np.float64, (what, name, mine.shape, theirs.shape)
        assert bits_equal(mine.ravel(), theirs.ravel()), (what, name)
    for k, width in enumerate(want.columns):
        assert bits_equal(_host_field(got, k).ravel(), want.field(k).ravel()), (what, k)
    return True


def _host_field(got, k):
    v = got.field(k)
    if hasattr(v, 'cpu'):
        return v.cpu().numpy()
    first = sum(got.columns[:k])
    assert isinstance(v, fl.DeviceBuffer) and v.shape == (got.points, got.columns[k])
    return _host(got.values)[:, first:first + got.columns[k]]


def model(arrays, name, key, columns, kernel, normalise, points, rows, absent, kw):
    """The model over the arrays the chunks hold, computed once per argument set."""
    tag = (name, key, columns, kernel, normalise, points.tobytes(), None if rows is None else tuple(int(r) for r in rows), absent)
    if tag not in _MODEL:
        mass, density = (None if c in absent else arrays.get(chunk(name + '_' + c, columns)) for c in ('mass', 'density'))
        values = [arrays[chunk(name + '_value%d' % k, columns)] for k in range(len(CASES[name]['values']))]
        _MODEL[tag] = hoomd.sph_samples(points, arrays[chunk(name, key)], values=values, mass=mass, density=density, rows=rows,
                                        kernel=kernel, normalise=normalise, **kw)
    return _MODEL[tag]


def samples(f, arrays, name, key, kernel, normalise=False, points=None, rows=None, columns=None, absent=(), device_points=False):
    """Order the list on the GPU, run the pass; the model over the arrays the chunks hold beside it.  ``columns``: the
    element type key of the mass, density and value chunks (the positions' by default); ``absent``: of 'mass' and
    'density' those that are not handed over although stored."""
    case = CASES[name]
    kw = dict((k, v) for k, v in case.items() if k not in ('points', 'position', 'values', 'mass', 'density', 'normalise', 'kernel'))
    columns = key if columns is None else columns
    points = np.asarray(case['points'] if points is None else points, np.float64).reshape(-1, 3)
    host = arrays[chunk(name, key)]
    stored = [(0, chunk(name + '_' + c, columns)) if chunk(name + '_' + c, columns) in arrays and c not in absent else None
              for c in ('mass', 'density')]
    values = [(0, chunk(name + '_value%d' % k, columns)) for k in range(len(case['values']))]
    box, h, dims = kw['box'], kw['h'], kw.get('dimensions', 3)
    want = model(arrays, name, key, columns, kernel, normalise, points, rows, tuple(absent), kw)
    every = np.arange(len(host)) if rows is None else np.asarray(rows)
    d_rows = to_device(f, every)
    if len(every):
        d_cell = f.order_rows_by_cell_device(0, chunk(name, key), box, want.grid, d_rows, n=len(every), dimensions=dims)
    else:
        d_cell = to_device(f, np.zeros(1))
    given = to_device(f, points if len(points) else np.zeros((1, 3)), np.float64) if device_points else points
    if device_points and len(points) == 0:
        given = given[:0] if hasattr(given, 'cpu') else given.view(shape=(0, 3))
    got = f.sph_samples_device(0, chunk(name, key), box, h, want.grid, d_rows, d_cell, given, n=len(every), values=values,
                               mass=stored[0], density=stored[1], dimensions=dims, kernel=kernel, normalise=normalise)
    return got, want


# ---------------------------------------------------------------- constructed cases
@pytest.mark.parametrize("normalise", (False, True))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("key", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(SHARED_CASES))
def test_a_case_equals_the_model(data, name, key, kernel, normalise):
    path, arrays = data
    with fl.open(path, 'r') as f:
        got, want = samples(f, arrays, name, key, kernel, normalise)
        assert equal(got, want, (name, key, kernel, normalise))
        f.wait_read()
    K = len(CASES[name]['points'])
    assert got.points == K
    if name != 'lone':
        # the special points: two nowhere (+0.0 whatever normalise says), two outside the box
        assert got.nowhere >= 2 and got.outside >= 2
        for a in (_host(got.density)[-4:-2], _host(got.shepard)[-4:-2], _host(got.values)[-4:-2]):
            assert not a.any() and not np.signbit(a).any()
    if name == 'all_nowhere':
        assert got.empty == K - got.nowhere and got.count_max == 0 and not _host(got.count).any()
    if name == 'lone':
        assert _host(got.count).tolist() == [0, 1, 1, 0] and np.isnan(_host(got.values)[0, 0]) == normalise
    if name in ('one_cell_65', 'mass_only', 'no_density'):
        assert got.shepard_max == np.inf and got.not_finite > 0
    if name == 'clump_700':
        assert got.count_max > 600                  # a sum longer than a workgroup
    if name == 'sparse_64cubed':
        assert got.grid == (64, 64, 64) and got.empty > 0
    if name == 'flat':
        assert got.dimensions == 2
    if name == 'no_values':
        assert _host(got.values).shape == (K, 0)


@pytest.mark.parametrize("C", sorted(WIDTHS))
def test_every_number_of_columns(data, C):
    """C in {0, 1, 2, 3, 4, 5, 8}: padding on both sides of every instantiated width."""
    path, arrays = data
    with fl.open(path, 'r') as f:
        for key in sorted(DTYPES):
            for kernel in KERNELS:
                for normalise in (False, True):
                    got, want = samples(f, arrays, 'columns_%d' % C, key, kernel, normalise)
                    assert equal(got, want, (C, key, kernel, normalise)) and got.columns == WIDTHS[C]
        f.wait_read()


@pytest.mark.parametrize("columns", sorted(DTYPES))
@pytest.mark.parametrize("key", sorted(DTYPES))
def test_column_chunks_of_either_element_type_and_each_chunk_absent(data, key, columns):
    """float32 and float64 mass, density and value chunks beside positions of either type; a row with density 0 and one with
    a NaN density; the mass and the density chunk not handed over, each alone."""
    path, arrays = data
    with fl.open(path, 'r') as f:
        for kernel in KERNELS:
            for absent in ((), ('mass',), ('density',)):
                got, want = samples(f, arrays, 'mass_density', key, kernel, True, columns=columns, absent=absent)
                assert equal(got, want, (key, columns, kernel, absent)) and got.not_finite > 0
        f.wait_read()


@pytest.mark.parametrize("key", sorted(DTYPES))
def test_0_1_63_64_65_and_4097_points_and_lists_of_0_1_and_65_entries(data, key):
    path, arrays = data
    points = CASES['triclinic_754']['points']
    with fl.open(path, 'r') as f:
        for K in (0, 1, 63, 64, 65, 4097):
            for device_points in (False, True):
                got, want = samples(f, arrays, 'triclinic_754', key, 'wendland_c2', K == 65, points=np.resize(points, (K, 3)),
                                    device_points=device_points)
                assert equal(got, want, (key, K, device_points)) and got.points == K
        assert got.count_max > 0 and got.nowhere > 0
        for n in (0, 1, 65):
            for normalise in (False, True):
                got, want = samples(f, arrays, 'triclinic_754', key, 'cubic_spline', normalise, rows=np.arange(100, 100 + n))
                assert equal(got, want, (key, n, normalise)) and got.points == len(points)
            assert (got.empty == got.points - got.nowhere) == (n == 0)
        # a list in descending order with rows listed twice
        rows = np.concatenate([np.arange(400, 0, -1), [7, 7, 400, 12]])
        got, want = samples(f, arrays, 'triclinic_754', key, 'wendland_c2', rows=rows)
        assert equal(got, want, (key, 'repeats'))
        f.wait_read()


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_the_kernel_on_every_mutation_case(data, mutation):
    """The case on which the mutated loop differs from the model (tests/test_sph_sample_model.py): the kernel equals the
    model there, so it does not hold the mutation."""
    path, arrays = data
    name = MUTATION_CASE[mutation]
    with fl.open(path, 'r') as f:
        for kernel in KERNELS:
            for key in sorted(DTYPES):
                got, want = samples(f, arrays, name, key, kernel, bool(CASES[name].get('normalise', False)))
                assert equal(got, want, (mutation, kernel, key))
        f.wait_read()


def test_at_the_entries_positions_the_samples_are_the_sums_on_the_gpu(data):
    """points = position[rows] as float64: density and shepard are sph_sums_device's of the same list, bit for bit, and
    both ran on the GPU."""
    path, arrays = data
    for name in ('triclinic_754', 'flat', 'three_cells'):
        case = CASES[name]
        box, h, dims = case['box'], case['h'], case.get('dimensions', 3)
        host = arrays[chunk(name, 'f32')]
        stored = [(0, chunk(name + '_' + c, 'f32')) for c in ('mass', 'density')]
        with fl.open(path, 'r') as f:
            grid = hoomd.neighbour_grid_for(box, 2.0 * h, dims) if 'cells' not in case else case['cells']
            d_rows = to_device(f, np.arange(len(host)))
            d_cell = f.order_rows_by_cell_device(0, chunk(name, 'f32'), box, grid, d_rows, dimensions=dims)
            for kernel in KERNELS:
                sums = f.sph_sums_device(0, chunk(name, 'f32'), box, h, grid, d_rows, d_cell, mass=stored[0], density=stored[1],
                                         dimensions=dims, kernel=kernel, return_rows=True)
                points = host[_host(d_rows)].astype(np.float64)
                got = f.sph_samples_device(0, chunk(name, 'f32'), box, h, grid, d_rows, d_cell, points, mass=stored[0],
                                           density=stored[1], dimensions=dims, kernel=kernel)
                assert bits_equal(_host(got.density), _host(sums.density)) and bits_equal(_host(got.shepard), _host(sums.shepard))
                assert got.nowhere == sums.nowhere and got.empty == 0 and _host(got.values).shape == (len(host), 0)
            f.wait_read()


# ---------------------------------------------------------------- staging
def test_a_second_call_is_served_from_the_staged_rows(data):
    path, arrays = data
    name = 'triclinic_754'
    n = len(arrays[chunk(name, 'f32')])
    once = n * (12 + 4 + 4 + 12 + 4)                        # position by the ordering, then mass, density and two values
    with fl.open(path, 'r') as f:
        f.device_read_stats(reset=True)
        got, want = samples(f, arrays, name, 'f32', 'wendland_c2')
        assert f.device_read_stats()["pread_bytes"] == once and equal(got, want, "first")
        got, want = samples(f, arrays, name, 'f32', 'cubic_spline', True)
        assert f.device_read_stats()["pread_bytes"] == once and equal(got, want, "second")
        f.wait_read()
        f.device_read_stats(reset=True)
        got, want = samples(f, arrays, name, 'f32', 'wendland_c2')
        assert f.device_read_stats()["pread_bytes"] == once and equal(got, want, "third")   # released by wait_read: read again
        f.wait_read()


# ---------------------------------------------------------------- refusals
def test_what_the_python_layers_refuse(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    with fl.open(path, 'r') as f:
        rows = to_device(f, np.arange(100))
        cell = f.order_rows_by_cell_device(0, name, TRICLINIC, (7, 5, 4), rows, n=100)
        points = np.zeros((5, 3))

        def call(name=name, box=TRICLINIC, h=0.625, cells=(7, 5, 4), rows=rows, cell=cell, points=points, **kw):
            return f.sph_samples_device(0, name, box, h, cells, rows, cell, points, **kw)

        mass = (0, chunk('triclinic_754_mass', 'f32'))
        for kw, message in ((dict(h=0.0), "finite and positive"), (dict(h=float('nan')), "finite and positive"),
                            (dict(cells=(8, 5, 4)), "narrower"), (dict(cells=(7, 5)), "three counts"),
                            (dict(h=1.51, cells=(1, 1, 1)), "count twice"), (dict(kernel='gaussian'), "kernel is one of"),
                            (dict(dimensions=2), "one z cell"), (dict(dimensions=4, cells=(1, 1, 1)), "dimensions is 2 or 3"),
                            (dict(n=101), "fewer entries than n"), (dict(name='particles/typeid'), "float32 or float64"),
                            (dict(name='particles/mass'), "3 columns"), (dict(box=[1, 2, 3]), "6 values"),
                            (dict(mass=(0, 'particles/typeid')), "mass chunk holds float32 or float64"),
                            (dict(density=(0, 'particles/position')), "density chunk has 1 column"),
                            (dict(mass=(0, 'particles/mass')), "differ in their number of rows"),
                            (dict(values=[(0, 'particles/typeid')]), "value chunk 0 holds float32 or float64"),
                            (dict(values=[mass, ((0, name), 2, 0.0)]), "value chunk 1 has 2 columns"),
                            (dict(values=[(0, 'particles/velocity')]), "value chunk 0 and the position chunk differ"),
                            (dict(values=[mass] * 5), "at most 4 chunks"), (dict(defaults=[1.0]), "a mass and a density"),
                            (dict(points=np.zeros((5, 2))), "points holds K x 3"),
                            (dict(box=WIDE, h=0.025, cells=(1024, 1024, 2)), "2\\^20 cells")):
            with pytest.raises(ValueError, match=message):
                call(**kw)
        with pytest.raises(KeyError):
            call(values=[(0, 'log/nothing')])
        f.wait_read()


def test_every_refusal_has_its_message_and_leaves_the_outputs_untouched(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    host = arrays[name]
    mass, density, v0, v1 = (arrays[chunk('triclinic_754_' + c, 'f32')] for c in ('mass', 'density', 'value0', 'value1'))
    n, points = 500, CASES['triclinic_754']['points'][:200]
    K = len(points)
    asked = dict(mass=mass, density=density, rows=np.arange(n), cells=(7, 5, 4))
    want = hoomd.sph_samples(points, host, TRICLINIC, 0.625, values=[v0, v1], **asked)
    rows_sorted, cell_sorted, _ = hoomd.cell_order(host, TRICLINIC, np.arange(n), (7, 5, 4))
    fn = _lib.lib.pgsd_sph_samples_device
    fn.restype = ctypes.c_int32
    D, U, E = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_lib.IndexEntry)
    fn.argtypes = [ctypes.POINTER(_lib.Handle), E, E, E, ctypes.POINTER(E), U, D, D, ctypes.POINTER(ctypes.c_float), D,
                   ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, U, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                   ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    with fl.open(path, 'r') as f:
        h = f._h()

        def entry_of(chunk_name):
            return _lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(h, 0, chunk_name.encode()).contents)

        d_rows, d_cell, d_points = to_device(f, rows_sorted), to_device(f, cell_sorted), to_device(f, points, np.float64)
        descending, outside_cell, outside_row = cell_sorted.copy(), cell_sorted.copy(), rows_sorted.copy()
        descending[300] = 0
        outside_cell[n - 1] = 141
        outside_row[7] = len(host)
        d_desc, d_outc, d_outr = to_device(f, descending), to_device(f, outside_cell), to_device(f, outside_row)
        summary = (ctypes.c_uint64 * 11)(*([77] * 11))
        outs = [fl._device_from_host(np.full(K, 77, np.uint32), f.pipeline_device())]
        outs += [fl._device_from_host(np.full(size, 77.0), f.pipeline_device()) for size in (K, K, 4 * K)]
        good = dict(entry=entry_of(name), mass=entry_of(chunk('triclinic_754_mass', 'f32')),
                    density=entry_of(chunk('triclinic_754_density', 'f32')),
                    values=[entry_of(chunk('triclinic_754_value0', 'f32')), entry_of(chunk('triclinic_754_value1', 'f32')), None, None],
                    columns=[3, 1, 0, 0], value_defaults=[0.0] * 4, defaults=[1.0, 0.0], box=TRICLINIC,
                    vectors=hoomd.box_vectors(np.asarray(TRICLINIC, np.float32)), h=0.625, kernel=0, dims=3, cells=(7, 5, 4),
                    rows=d_rows, cell=d_cell, n=n, points=d_points, K=K, normalise=0)

        def raw(**changes):
            a = dict(good, **changes)
            optional = [None if a[c] is None else ctypes.byref(a[c]) for c in ('mass', 'density')]
            values = (E * 4)(*[None if v is None else ctypes.pointer(v) for v in a['values']])
            return fn(h, ctypes.byref(a['entry']), optional[0], optional[1], values, (ctypes.c_uint32 * 4)(*a['columns']),
                      (ctypes.c_double * 4)(*a['value_defaults']), (ctypes.c_double * 2)(*a['defaults']),
                      (ctypes.c_float * 6)(*a['box']), (ctypes.c_double * 6)(*a['vectors']), a['h'], a['kernel'], a['dims'],
                      (ctypes.c_uint32 * 3)(*a['cells']), _ptr(a['rows']), _ptr(a['cell']), a['n'],
                      None if a['points'] is None else _ptr(a['points']), a['K'], a['normalise'], _ptr(outs[0]), _ptr(outs[1]),
                      _ptr(outs[2]), _ptr(outs[3]), summary)

        def untouched():
            return all(_host(o).tolist() == [77] * len(_host(o)) for o in outs)

        huge = entry_of(name)
        huge.N = 2 ** 32
        flat_vectors = hoomd.box_vectors(np.asarray(FLAT, np.float32))
        wide = [2000, 2000, 2000, 0, 0, 0]
        inf, nan = float('inf'), float('nan')
        v0_e, v1_e, mass_e = good['values'][0], good['values'][1], good['mass']
        for changes, message in (
                (dict(entry=entry_of('particles/typeid')), "float32 or float64"), (dict(entry=entry_of('particles/mass')), "3 columns"),
                (dict(entry=huge), "2^32 rows"), (dict(n=2 ** 32), "2^32 entries"), (dict(dims=4), "dimensions is 2 or 3"),
                (dict(h=0.0), "finite and positive"), (dict(h=inf), "finite and positive"), (dict(h=nan), "finite and positive"),
                (dict(kernel=2), "the kernel is 0"), (dict(mass=entry_of('particles/typeid')), "the mass chunk holds float32 or float64"),
                (dict(density=entry_of(name)), "the density chunk has 1 column"),
                (dict(mass=entry_of('particles/mass')), "the mass chunk and the position chunk differ"),
                (dict(K=2 ** 32), "fewer than 2^32 points"), (dict(points=None), "points is NULL with K > 0"),
                (dict(columns=[3, 5, 0, 0]), "a value chunk has 1 to 4 columns"),
                (dict(values=[v0_e, v0_e, v0_e, None], columns=[3, 3, 3, 0]), "at most 8 columns together"),
                (dict(values=[v0_e, None, v1_e, None], columns=[3, 0, 1, 0]), "a used value slot follows an unused one"),
                (dict(values=[entry_of('particles/typeid'), v1_e, None, None], columns=[1, 1, 0, 0]),
                 "value chunk 0 holds float32 or float64"),
                (dict(values=[v0_e, v0_e, None, None]), "value chunk 1 has 1 column"),
                (dict(values=[v0_e, mass_e, None, None], columns=[3, 2, 0, 0]), "value chunk 1 has 2 columns"),
                (dict(values=[entry_of('particles/velocity'), v1_e, None, None]), "value chunk 0 and the position chunk differ"),
                (dict(values=[v0_e, None, None, None], value_defaults=[0.0, nan, 0.0, 0.0]),
                 "value chunk 1 is stored nowhere and its default is no number"),
                (dict(box=[10, 0, 6, 0.3, -0.2, 0.4]), "box lengths"), (dict(box=[10, 8, 6, 0.3, -0.2, 0.5]), "the box and the vectors disagree"),
                (dict(box=[10, 8, 6.5, 0.3, -0.2, 0.4]), "the box and the vectors disagree"),
                (dict(vectors=[10, 0, 6, 0, 0, 0]), "box lengths"), (dict(cells=(0, 5, 4)), "1 to 1024 cells"),
                (dict(cells=(8, 5, 4)), "narrower than the support"), (dict(cells=(7, 5, 5)), "narrower than the support"),
                (dict(dims=2, box=FLAT, vectors=flat_vectors, cells=(2, 3, 2)), "one z cell"),
                (dict(h=1.51, cells=(1, 1, 1)), "count twice"),
                (dict(box=wide, vectors=hoomd.box_vectors(np.asarray(wide, np.float32)), h=0.5, cells=(1024, 1024, 2)), "2^20 cells"),
                (dict(cell=d_desc), "descends or lies outside"), (dict(cell=d_outc), "descends or lies outside"),
                (dict(rows=d_outr), "outside the chunks"), (dict(cells=(7, 5, 3)), "descends or lies outside")):
            assert raw(**changes) == _lib.ERROR_INVALID_ARGUMENT and message in _lib.last_error(), (message, _lib.last_error())
            assert "pgsd_sph_samples_device" in _lib.last_error()
            assert list(summary) == [77] * 11, message
            assert untouched(), message

        def landed(model):
            return (words_equal(np.array(list(summary), np.uint64), model.summary) and np.array_equal(_host(outs[0]), model.count)
                    and bits_equal(_host(outs[1]), model.density) and bits_equal(_host(outs[2]), model.shepard)
                    and bits_equal(_host(outs[3])[:model.values.size], model.values.ravel()))

        # the call after them, as it is: correct
        assert raw() == 0 and landed(want)
        # without the pressure chunk its default stands for every element; normalised
        assert raw(values=[v0_e, None, None, None], value_defaults=[0.0, 2.5e4, 0.0, 0.0], normalise=1) == 0
        assert landed(hoomd.sph_samples(points, host, TRICLINIC, 0.625, values=[v0, np.full(len(host), 2.5e4)], normalise=True, **asked))
        # without the mass and density chunks their defaults do
        assert raw(mass=None, density=None, defaults=[2.0, 4.0]) == 0
        assert landed(hoomd.sph_samples(points, host, TRICLINIC, 0.625, values=[v0, v1], rows=np.arange(n), cells=(7, 5, 4),
                                        mass=np.full(len(host), 2.0), density=np.full(len(host), 4.0)))
        # no point: the summary of no point, nothing launched, the arrays as they were
        before = [_host(o).copy() for o in outs]
        assert raw(K=0, points=None) == 0
        assert list(summary) == [0] * 6 + [NONE] + list(np.array([inf, -inf, inf, -inf]).view(np.uint64))
        assert all(np.array_equal(_host(o).view(np.uint8), b.view(np.uint8)) for o, b in zip(outs, before))
        # no entry: every point that has a cell is empty
        assert raw(n=0) == 0
        assert landed(hoomd.sph_samples(points, host, TRICLINIC, 0.625, values=[v0, v1], rows=np.arange(0), cells=(7, 5, 4)))
        f.wait_read()


# ---------------------------------------------------------------- through pgsd.hoomd
WHERE = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
CELL = hoomd.domain_grid(2, 2, 1)[1]
SELECTIONS = {"all": {}, "where": {'where': WHERE}, "domain": {'domain': CELL}, "both": {'where': WHERE, 'domain': CELL}}
GRID = hoomd.sample_grid(TRICLINIC, (24, 24, 24))


@pytest.mark.parametrize("selection", sorted(SELECTIONS))
def test_frame_samples_device_equals_the_host_model(data, selection):
    """about_20000: the triclinic box at 2h = 0.61 (h=None from the uniform slength 0.305) sampled on a 24^3 sample_grid,
    with where, domain, an elided field (auxiliary1 is stored nowhere) and normalise."""
    path, _ = data
    kwargs = SELECTIONS[selection]
    with hoomd.open(path, 'r') as t:
        for options in (dict(fields=('velocity', 'pressure', 'auxiliary1')),
                        dict(fields=('pressure',), h=0.3125, kernel='cubic_spline', cells=(12, 10, 8), normalise=True)):
            want = t.frame_samples(0, GRID, **options, **kwargs)
            got = t.frame_samples_device(0, GRID, **options, **kwargs)
            assert equal(got, want, (selection, options))
        assert want.h == 0.3125 and want.points == 24 ** 3 and want.outside == 0 and want.nowhere == 0 and want.count_max > 0
        first = t.frame_samples_device(0, GRID[:100], fields=('velocity', 'auxiliary1'), **kwargs)
        assert first.h == float(np.float32(0.305)) and not _host(first.values)[:, 3:].any() and _host(first.values)[:, :3].any()
        assert _host(t.frame_samples_device(0, GRID, fields=('pressure',), **kwargs).values).reshape(24, 24, 24).shape == (24,) * 3
        with pytest.raises(ValueError, match="narrower"):
            t.frame_samples_device(0, GRID[:10], h=0.65, cells=(8, 5, 4), **kwargs)
        with pytest.raises(ValueError, match="count twice"):
            t.frame_samples_device(0, GRID[:10], h=1.75, **kwargs)
        with pytest.raises(ValueError, match="kernel is one of"):
            t.frame_samples_device(0, GRID[:10], h=0.3, kernel='gaussian', **kwargs)
        with pytest.raises(ValueError, match="cannot be sampled"):
            t.frame_samples_device(0, GRID[:10], fields=('typeid',), **kwargs)
        with pytest.raises(IndexError):
            t.frame_samples_device(2, GRID[:10], h=0.3)


def test_h_none_and_a_frame_at_rest_on_the_device(data):
    """Frame 1 stores a slength that is not uniform, and neither velocity, mass nor density: the velocity samples as zeros
    and the defaults 1.0 and 0.0 stand for mass and density, so every V is infinite, in the model and on the GPU alike."""
    path, _ = data
    points = np.concatenate([GRID[::29], special_points(TRICLINIC)])
    with hoomd.open(path, 'r') as t:
        with pytest.raises(ValueError, match="slength ranges from 0.30"):
            t.frame_samples_device(1, points)
        with pytest.raises(ValueError, match="slength ranges from 0.30"):
            t.frame_samples(1, points)
        want = t.frame_samples(1, points, h=0.305, where={'type': ['fluid']})
        got = t.frame_samples_device(1, points, h=0.305, where={'type': ['fluid']})
        assert equal(got, want, "defaults") and got.columns == (3,) and got.nowhere == 2 and got.outside == 2
        assert got.shepard_max == np.inf and got.not_finite > 0


# ---------------------------------------------------------------- without a tensor library
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
points = hoomd.sample_grid([10, 8, 6, 0.3, -0.2, 0.4], (6, 5, 4))
with hoomd.open(path, 'r') as t:
    got = t.frame_samples_device(0, points, fields=('velocity', 'pressure'), where={'type': ['wall']}, normalise=True)
    assert isinstance(got.values, fl.DeviceBuffer) and got.values.shape == (120, 4) and got.count.shape == (120,)
    assert isinstance(got.field(1), fl.DeviceBuffer) and got.field(1).shape == (120, 1) and got.field(0).shape == (120, 3)
    res = dict((name, getattr(got, name).to_host()) for name in ('count', 'density', 'shepard', 'values'))
    res['summary'] = got.summary
    res['grid'] = got.as_grid(1, (6, 5, 4))
pickle.dump(res, open(out_path, "wb"))
'''


def test_the_results_stay_in_device_memory_without_torch(data, tmp_path):
    """Without a tensor library the four arrays are DeviceBuffers."""
    path, _ = data
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, path, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))
    with hoomd.open(path, 'r') as t:
        want = t.frame_samples(0, hoomd.sample_grid(TRICLINIC, (6, 5, 4)), fields=('velocity', 'pressure'), where={'type': ['wall']},
                               normalise=True)
    assert words_equal(res['summary'], want.summary) and np.array_equal(res['count'], want.count) and want.count_max > 0
    for name in ('density', 'shepard', 'values'):
        assert res[name].shape == getattr(want, name).shape and bits_equal(res[name].ravel(), getattr(want, name).ravel()), name
    assert res['grid'].shape == (4, 5, 6, 1) and bits_equal(res['grid'].ravel(), want.field(1).ravel())
