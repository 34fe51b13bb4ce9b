"""The SPH sums with a per-particle smoothing length on the GPU: pgsd_sph_adaptive_sums_device and
pgsd_sph_smoothing_range_device behind pgsd.fl's sph_adaptive_sums_device and smoothing_range_device and pgsd.hoomd's
frame_adaptive_sums_device.  Every per-entry array and every summary word must equal the numpy model
pgsd.hoomd.sph_adaptive_sums / frame_adaptive_sums exactly, the floats bit for bit (tests/test_sph_adaptive_model.py holds
the model against a plain double loop; a NaN equals a NaN).  The cases at the pgsd.fl level read constructed chunks, once
with float32 and once with float64 positions, in both modes with both kernels; the range is reduced and the list ordered
on the GPU first, as a caller does."""
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
from sph_cases import CASES as SUM_CASES, KERNELS, NONE, WIDE, bits_equal  # noqa: E402
from sph_adaptive_cases import (MODES, MUTATIONS, derivative_error, jittered, lattice, seeded_h, words_equal)  # noqa: E402
from test_sph_adaptive_model import DERIVATIVE_BOUND, LATTICE_DENSITY, LATTICE_OMEGA  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20_011
N1 = 5_003
TYPES = ['fluid', 'wall', 'inlet']
DTYPES = {'f32': np.float32, 'f64': np.float64}
BAD = (0.0, -0.5, np.nan, np.inf)
BAD_ROWS = [3, 77, 300]
STEP = 1e-4

# name -> (positions as float64, {column name: values}, keyword arguments of sph_adaptive_sums besides those)
CASES = {}
for _name, (_p, _mass, _density, _kw) in SUM_CASES.items():
    _kw = dict(_kw)
    _h = _kw.pop('h')
    _columns = {'slength': seeded_h(_name, len(_p), _h)}
    if _mass is not None:
        _columns['mass'] = _mass
    if _density is not None:
        _columns['density'] = _density
    CASES[_name] = (_p, _columns, _kw)
UNIFORM_H = dict((name, case[3]['h']) for name, case in SUM_CASES.items())
for _k, _bad in enumerate(BAD):
    _s = CASES['mass_density'][1]['slength'].copy()
    _s[BAD_ROWS] = _bad
    CASES['mass_density'][1]['bad%d' % _k] = _s
for _k, (_name, (_switch, _case)) in enumerate(sorted(MUTATIONS.items())):
    _kw = dict(_case)
    _columns = dict((c, np.asarray(_kw.pop(c), np.float64)) for c in ('slength', 'mass', 'density') if c in _kw)
    CASES['mutation_%02d' % _k] = (np.asarray(_kw.pop('position'), np.float64), _columns, _kw)
MUTATION_CASE = dict((name, 'mutation_%02d' % k) for k, name in enumerate(sorted(MUTATIONS)))
for _dims in (3, 2):
    _p, _box, _h, _interior = lattice(_dims)
    CASES['lattice_%d' % _dims] = (_p, {'slength': _h}, dict(box=_box, dimensions=_dims))
_p, _box, _h, _mass = jittered()
CASES['jittered'] = (_p, {'slength': _h, 'up': _h * (1.0 + STEP), 'down': _h * (1.0 - STEP), 'mass': _mass}, dict(box=_box))
SHARED = [c for c in sorted(CASES) if c in SUM_CASES]


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
    """One file of two frames.  Frame 0: 20 011 particles with types, masses, densities, a slength in [0.2, 0.305] that
    differs from row to row (four rows hold an inf, a NaN, a 0 and a negative one) and random positions in the triclinic
    box (the pgsd.hoomd level), and every case's positions and columns as float32 and float64 log chunks.  Frame 1: 5 003
    other particles with nothing but a position stored.  The host's arrays beside it."""
    path = os.path.join(_dir(tmp_path_factory, "spha"), "pgsd_spha_%d.gsd" % os.getpid())
    rng = np.random.default_rng(N)
    fr = hoomd.Frame()
    fr.configuration.box = TRICLINIC
    fr.particles.N = N
    fr.particles.types = TYPES
    fr.particles.position = _lost(random_rows(7, N, TRICLINIC, np.float32))
    fr.particles.typeid = rng.integers(0, len(TYPES), size=N).astype(np.uint32)
    fr.particles.density = (1000.0 + 50.0 * rng.standard_normal(N)).astype(np.float32)
    fr.particles.mass = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
    s = rng.uniform(0.2, 0.305, size=N).astype(np.float32)
    s[[10, 2000, 4000, 19000]] = [np.inf, np.nan, 0.0, -0.25]
    fr.particles.slength = s
    arrays = {}
    for name, (p, columns, _) in CASES.items():
        for key, dt in DTYPES.items():
            arrays[chunk(name, key)] = fr.log['%s_%s' % (name, key)] = np.ascontiguousarray(p.astype(dt))
            for column, values in columns.items():
                arrays[chunk(name + '_' + column, key)] = fr.log['%s_%s_%s' % (name, column, key)] = \
                    np.ascontiguousarray(np.asarray(values).astype(dt))
    with hoomd.open(path, 'w') as t:
        t.append(fr)
        other = hoomd.Frame()
        other.configuration.box = TRICLINIC
        other.particles.N = N1
        other.particles.types = TYPES
        other.particles.position = _lost(random_rows(8, N1, TRICLINIC, np.float32))
        t.append(other)
    yield path, arrays
    os.unlink(path)


def to_device(f, a):
    return fl._device_from_host(np.ascontiguousarray(a, dtype=np.int32), f.pipeline_device())


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr() if hasattr(x, 'data_ptr') else x.ptr)


ATTRIBUTES = ('n', 'nowhere', 'bad_h', 'not_finite', 'surface', 'deviation_at', 'deviation_row', 'count_min', 'count_max',
              'count_min_at', 'pairs')


def equal(got, want, what):
    """The kernel's AdaptiveSums (per-entry arrays in GPU memory) against the model's."""
    assert words_equal(got.summary, want.summary), (what, got, want, got.summary, want.summary)
    assert got.grid == want.grid and got.kernel == want.kernel and got.mode == want.mode and got.volume == want.volume, what
    assert got.h_max == want.h_max or want.n == 0, (what, got.h_max, want.h_max)
    for name in ATTRIBUTES:
        assert getattr(got, name) == getattr(want, name), (what, name)
    if got.number is not None:
        assert np.array_equal(_host(got.rows), want.rows) and np.array_equal(_host(got.cell), want.cell), what
        assert _host(got.count).dtype == np.uint32 and np.array_equal(_host(got.count), want.count), (what, 'count')
        for name in ('number', 'density', 'shepard', 'omega'):
            mine, theirs = getattr(got, name), getattr(want, name)
            assert (mine is None) == (theirs is None), (what, name)
            if theirs is not None:
                assert bits_equal(_host(mine), theirs), (what, name)
    return True


def sums(f, arrays, name, key, kernel, mode, rows=None, return_rows=True, columns=None, slength='slength', **kw):
    """Reduce the range and order the list on the GPU, run the pass; the model over the arrays the chunks hold beside
    it.  ``columns``: the element type key of the slength, mass and density chunks (the positions' by default);
    ``slength``: the name of the column that holds the smoothing lengths."""
    columns = key if columns is None else columns
    host = arrays[chunk(name, key)]
    s = arrays[chunk(name + '_' + slength, columns)]
    mass, density = arrays.get(chunk(name + '_mass', columns)), arrays.get(chunk(name + '_density', columns))
    box, dims = kw['box'], kw.get('dimensions', 3)
    want = hoomd.sph_adaptive_sums(host, box, s, mass=mass, density=density, rows=rows, kernel=kernel, mode=mode,
                                   cells=kw.get('cells'), dimensions=dims, surface_below=kw.get('surface_below'))
    every = np.arange(len(host)) if rows is None else np.asarray(rows)
    d_rows = to_device(f, every)
    found = f.smoothing_range_device((0, chunk(name + '_' + slength, columns)), len(host), d_rows, n=len(every))
    assert found[:2] == hoomd.smoothing_range(s, every)[:2] and bits_equal(found[2:], hoomd.smoothing_range(s, every)[2:])
    h_max = found[3] if len(every) else 1.0                 # (a list of no entry: any valid bound)
    d_cell = f.order_rows_by_cell_device(0, chunk(name, key), box, want.grid, d_rows, n=len(every), dimensions=dims)
    got = f.sph_adaptive_sums_device(0, chunk(name, key), box, h_max, want.grid, d_rows, d_cell, n=len(every),
                                     slength=(0, chunk(name + '_' + slength, columns)),
                                     mass=None if mass is None else (0, chunk(name + '_mass', columns)),
                                     density=None if density is None else (0, chunk(name + '_density', columns)),
                                     dimensions=dims, kernel=kernel, mode=mode, surface_below=kw.get('surface_below'),
                                     return_rows=return_rows)
    return got, want


# ---------------------------------------------------------------- constructed cases
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("key", sorted(DTYPES))
@pytest.mark.parametrize("name", SHARED)
def test_a_case_equals_the_model(data, name, key, kernel, mode):
    path, arrays = data
    kw = CASES[name][2]
    with fl.open(path, 'r') as f:
        got, want = sums(f, arrays, name, key, kernel, mode, **kw)
        assert equal(got, want, (name, key, kernel, mode))
        f.wait_read()
    assert want.n == len(arrays[chunk(name, key)]) and got.slength is None
    if name == 'all_nowhere':
        assert got.nowhere == 100 and got.density_min == np.inf and got.count_min is None and got.pairs == 0
        for a in (got.count, got.number, got.density, got.shepard):
            assert not _host(a).any() and not np.signbit(_host(a).astype(np.float64)).any()
    if name == 'three_cells':
        assert got.nowhere > 0 and got.n == 4097
    if name == 'sparse_64cubed':
        assert got.grid == (64, 64, 64) and got.count_min == 1
    if name == 'flat':
        assert got.dimensions == 2
    if name == 'clump_700':
        assert got.count_max > 256                              # a sum longer than a workgroup
    assert (got.omega is None) == (mode == 'mean')


@pytest.mark.parametrize("columns", sorted(DTYPES))
@pytest.mark.parametrize("key", sorted(DTYPES))
def test_slength_mass_and_density_chunks_of_either_element_type(data, key, columns):
    path, arrays = data
    with fl.open(path, 'r') as f:
        for kernel, mode in zip(KERNELS, MODES):
            got, want = sums(f, arrays, 'mass_density', key, kernel, mode, columns=columns, **CASES['mass_density'][2])
            assert equal(got, want, (key, columns, kernel)) and got.volume and got.surface is not None
        f.wait_read()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", SHARED)
def test_with_one_h_it_is_the_existing_uniform_pass_on_the_gpu(data, name, kernel):
    """No slength chunk: the default H stands for every row, and gather mode equals the EXISTING sph_sums_device of the
    same list, both on the GPU, bit for bit in number, density, shepard, the bounds and the deviation."""
    path, arrays = data
    kw, H, key = CASES[name][2], UNIFORM_H[name], 'f32'
    host = arrays[chunk(name, key)]
    mass, density = arrays.get(chunk(name + '_mass', key)), arrays.get(chunk(name + '_density', key))
    dims, n = kw.get('dimensions', 3), len(host)
    chunks = dict(mass=None if mass is None else (0, chunk(name + '_mass', key)),
                  density=None if density is None else (0, chunk(name + '_density', key)))
    with fl.open(path, 'r') as f:
        grid = hoomd.sph_kernel_sums(host, kw['box'], H, cells=kw.get('cells'), dimensions=dims).grid
        d_rows = to_device(f, np.arange(n))
        assert f.smoothing_range_device(None, n, d_rows, default=H) == (n, 0, H, H)
        d_cell = f.order_rows_by_cell_device(0, chunk(name, key), kw['box'], grid, d_rows, n=n, dimensions=dims)
        uniform = f.sph_sums_device(0, chunk(name, key), kw['box'], H, grid, d_rows, d_cell, n=n, dimensions=dims, kernel=kernel,
                                    surface_below=kw.get('surface_below'), return_rows=True, **chunks)
        got = f.sph_adaptive_sums_device(0, chunk(name, key), kw['box'], H, grid, d_rows, d_cell, n=n, slength=None,
                                         defaults=[1.0, float('nan'), H], dimensions=dims, kernel=kernel,
                                         surface_below=kw.get('surface_below'), return_rows=True, **chunks)
        for a in ('number', 'density', 'shepard'):
            x, y = getattr(got, a), getattr(uniform, a)
            assert (x is None) == (y is None) and (x is None or bits_equal(_host(x), _host(y))), a
        for a in ('n', 'nowhere', 'not_finite', 'surface', 'deviation_at', 'deviation_row'):
            assert getattr(got, a) == getattr(uniform, a), a
        for a in ('number_min', 'number_max', 'density_min', 'density_max', 'shepard_min', 'shepard_max', 'deviation'):
            x, y = getattr(got, a), getattr(uniform, a)
            assert (x is None) == (y is None) and (x is None or bits_equal(x, y)), a
        assert got.bad_h == 0 and (got.n == got.nowhere or got.slength_min == got.slength_max == H)
        f.wait_read()


@pytest.mark.parametrize("key", sorted(DTYPES))
def test_lists_of_0_1_63_64_65_entries_repeats_and_any_order(data, key):
    path, arrays = data
    kw = CASES['three_cells'][2]
    with fl.open(path, 'r') as f:
        for n in (0, 1, 63, 64, 65):
            for mode in MODES:
                got, want = sums(f, arrays, 'three_cells', key, 'wendland_c2', mode, rows=np.arange(100, 100 + n), **kw)
                assert equal(got, want, (key, n, mode)) and got.n == n
        assert got.count_min >= 1
        got, want = sums(f, arrays, 'three_cells', key, 'cubic_spline', 'gather', rows=np.arange(0), **kw)
        assert got.n == 0 and got.density_min == np.inf and got.count_min is None and got.pairs == 0
        rows = np.concatenate([np.arange(400, 0, -1), [7, 7, 400, 12]])
        for kernel, mode in zip(KERNELS, MODES):
            got, want = sums(f, arrays, 'three_cells', key, kernel, mode, rows=rows, **kw)
            assert equal(got, want, (key, kernel)) and got.n == 404
        f.wait_read()


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_the_kernel_on_every_mutation_case(data, mutation):
    """The case on which the mutated loop differs from the model (tests/test_sph_adaptive_model.py): the kernel equals the
    model there, so it does not hold the mutation."""
    path, arrays = data
    name = MUTATION_CASE[mutation]
    kw = dict(CASES[name][2])
    kernels = [kw.pop('kernel')] if 'kernel' in kw else KERNELS
    mode = kw.pop('mode')
    key = 'f64' if MUTATIONS[mutation][1]['position'].dtype == np.float64 else 'f32'
    with fl.open(path, 'r') as f:
        for kernel in kernels:
            got, want = sums(f, arrays, name, key, kernel, mode, **kw)
            assert equal(got, want, (mutation, kernel))
        f.wait_read()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bad", range(len(BAD)))
def test_an_invalid_h_on_the_gpu(data, bad, mode):
    path, arrays = data
    with fl.open(path, 'r') as f:
        for key in sorted(DTYPES):
            got, want = sums(f, arrays, 'mass_density', key, 'wendland_c2', mode, slength='bad%d' % bad, **CASES['mass_density'][2])
            assert equal(got, want, (bad, mode, key)) and got.bad_h == 3 and got.nowhere == 0
            at = np.isin(_host(got.rows), BAD_ROWS)
            for a in (got.count, got.number, got.density, got.shepard):
                assert not _host(a)[at].any() and not np.signbit(_host(a)[at].astype(np.float64)).any()
        f.wait_read()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dimensions", (3, 2))
def test_a_lattice_has_density_one_and_omega_one_on_the_gpu(data, dimensions, kernel):
    path, arrays = data
    name = 'lattice_%d' % dimensions
    interior = lattice(dimensions)[3]
    with fl.open(path, 'r') as f:
        got, want = sums(f, arrays, name, 'f64', kernel, 'gather', **CASES[name][2])
        assert equal(got, want, (name, kernel))
        inside = interior[_host(got.rows)]
        assert inside.sum() == 4 ** dimensions
        assert np.abs(_host(got.density)[inside] - 1.0).max() <= LATTICE_DENSITY
        assert np.abs(_host(got.omega)[inside] - 1.0).max() <= LATTICE_OMEGA
        f.wait_read()


@pytest.mark.parametrize("kernel", KERNELS)
def test_omega_is_the_derivative_of_the_density_in_h_on_the_gpu(data, kernel):
    path, arrays = data
    p, box, h, mass = jittered()
    values = {}
    with fl.open(path, 'r') as f:
        for column in ('slength', 'up', 'down'):
            got, want = sums(f, arrays, 'jittered', 'f64', kernel, 'gather', slength=column, **CASES['jittered'][2])
            assert equal(got, want, (column, kernel))
            rows = _host(got.rows)
            density, omega = np.empty(len(p)), np.empty(len(p))
            density[rows], omega[rows] = _host(got.density), _host(got.omega)
            values[column] = (density, omega)
        f.wait_read()
    columns = {tuple(h * (1.0 + STEP)): 'up', tuple(h * (1.0 - STEP)): 'down'}
    error = derivative_error(p, box, h, mass, lambda s: values[columns[tuple(s)]][0], values['slength'][1], values['slength'][0],
                             step=STEP)
    print("omega against the central difference on the GPU, %s: worst relative error %.3g" % (kernel, error))
    assert error <= DERIVATIVE_BOUND


def test_the_range_of_a_column_with_an_inf_a_nan_and_a_zero(data):
    path, arrays = data
    with hoomd.open(path, 'r') as t:
        s = t[0].particles.slength
    with fl.open(path, 'r') as f:
        for rows in (None, np.arange(0, N, 3), np.array([10, 2000, 4000, 19000]), np.array([5, 5, 4000, 7]), np.arange(0)):
            d_rows = None if rows is None else to_device(f, rows)
            got = f.smoothing_range_device((0, 'particles/slength'), N, d_rows, n=None if rows is None else len(rows))
            want = hoomd.smoothing_range(s, rows)
            assert got[:2] == want[:2] and bits_equal(got[2:], want[2:]), (rows, got, want)
        assert hoomd.smoothing_range(s)[1] == 4
        # no chunk: the default in every row, nothing read; an invalid default is bad in every row
        assert f.smoothing_range_device(None, N, to_device(f, np.arange(50)), default=0.5) == (50, 0, 0.5, 0.5)
        assert f.smoothing_range_device(None, N, default=0.0) == (N, N, np.inf, -np.inf)
        for kw, message in ((dict(rows=to_device(f, [N])), "outside the chunk"),
                            (dict(slength=(0, 'particles/typeid')), "float32 or float64"),
                            (dict(slength=(0, 'particles/position')), "1 column"), (dict(N=N + 1), "holds N rows")):
            with pytest.raises(ValueError, match=message):
                f.smoothing_range_device(**dict(dict(slength=(0, 'particles/slength'), N=N), **kw))
        f.wait_read()


# ---------------------------------------------------------------- staging
def test_a_second_call_is_served_from_the_staged_rows_and_return_rows(data):
    path, arrays = data
    name, kw = 'triclinic_754', CASES['triclinic_754'][2]
    n = len(arrays[chunk(name, 'f32')])
    with fl.open(path, 'r') as f:
        f.device_read_stats(reset=True)
        got, want = sums(f, arrays, name, 'f32', 'wendland_c2', 'gather', **kw)   # slength by the range, position by the order
        assert f.device_read_stats()["pread_bytes"] == n * (4 + 12 + 4 + 4) and equal(got, want, "first")
        got, _ = sums(f, arrays, name, 'f32', 'wendland_c2', 'gather', return_rows=False, **kw)
        assert f.device_read_stats()["pread_bytes"] == n * (4 + 12 + 4 + 4) and equal(got, want, "second")
        assert got.rows is None and got.cell is None and got.count is None and got.number is None and got.omega is None
        f.wait_read()
        f.device_read_stats(reset=True)
        got, _ = sums(f, arrays, name, 'f32', 'cubic_spline', 'mean', **kw)
        assert f.device_read_stats()["pread_bytes"] == n * (4 + 12 + 4 + 4)      # released by wait_read: read again
        assert _host(got.number).dtype == np.float64 and got.omega is None
        f.wait_read()


# ---------------------------------------------------------------- refusals
def test_what_the_python_layers_refuse(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    with fl.open(path, 'r') as f:
        rows = to_device(f, np.arange(100))
        cell = f.order_rows_by_cell_device(0, name, TRICLINIC, (7, 5, 4), rows, n=100)

        def call(name=name, box=TRICLINIC, h_max=0.625, cells=(7, 5, 4), rows=rows, cell=cell, **kw):
            kw.setdefault('slength', (0, chunk('triclinic_754_slength', 'f32')))
            return f.sph_adaptive_sums_device(0, name, box, h_max, cells, rows, cell, **kw)

        for kw, message in ((dict(h_max=0.0), "h_max.*finite and positive"), (dict(h_max=float('nan')), "finite and positive"),
                            (dict(h_max=float('inf')), "finite and positive"), (dict(cells=(8, 5, 4)), "narrower"),
                            (dict(cells=(7, 5)), "three counts"), (dict(h_max=1.51, cells=(1, 1, 1)), "count twice"),
                            (dict(kernel='gaussian'), "kernel is one of"), (dict(mode='scatter'), "mode is one of"),
                            (dict(dimensions=2), "one z cell"), (dict(n=101), "fewer entries than n"),
                            (dict(name='particles/mass'), "3 columns"),
                            (dict(slength=(0, 'particles/typeid')), "slength chunk holds float32 or float64"),
                            (dict(slength=(0, 'particles/position')), "slength chunk has 1 column"),
                            (dict(slength=(0, 'particles/slength')), "slength chunk and the position chunk differ"),
                            (dict(mass=(0, 'particles/mass')), "differ in their number of rows"),
                            (dict(defaults=[1.0, 0.0]), "a mass, a density and a smoothing length"),
                            (dict(h_max=0.3), "exceeds h_max")):
            with pytest.raises(ValueError, match=message):
                call(**kw)
        with pytest.raises(KeyError):
            call(slength=(0, 'log/nothing'))
        f.wait_read()


def test_every_refusal_has_its_message_and_leaves_the_outputs_untouched(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    host, s = arrays[name], arrays[chunk('triclinic_754_slength', 'f32')]
    mass, density = arrays[chunk('triclinic_754_mass', 'f32')], arrays[chunk('triclinic_754_density', 'f32')]
    n = 500
    want = hoomd.sph_adaptive_sums(host, TRICLINIC, s, mass=mass, density=density, rows=np.arange(n), cells=(7, 5, 4),
                                   surface_below=0.004)
    fn = _lib.lib.pgsd_sph_adaptive_sums_device
    fn.restype = ctypes.c_int32
    D, U, E = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_lib.IndexEntry)
    fn.argtypes = [ctypes.POINTER(_lib.Handle), E, E, E, E, D, D, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32,
                   ctypes.c_uint32, U, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
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
        summary = (ctypes.c_uint64 * 22)(*([77] * 22))
        counts = fl._device_from_host(np.full(n, 77, np.uint32), f.pipeline_device())
        outs = [fl._device_from_host(np.full(n, 77.0), f.pipeline_device()) for _ in range(4)]
        good = dict(entry=entry_of(name), mass=entry_of(chunk('triclinic_754_mass', 'f32')),
                    density=entry_of(chunk('triclinic_754_density', 'f32')), slength=entry_of(chunk('triclinic_754_slength', 'f32')),
                    defaults=[1.0, float('nan'), 1.0], vectors=hoomd.box_vectors(np.asarray(TRICLINIC, np.float32)),
                    h_max=want.h_max, kernel=0, mode=0, dims=3, cells=(7, 5, 4), rows=d_rows, cell=d_cell, n=n, surface=0.004)

        def raw(**changes):
            a = dict(good, **changes)
            return fn(h, ctypes.byref(a['entry']), None if a['mass'] is None else ctypes.byref(a['mass']),
                      None if a['density'] is None else ctypes.byref(a['density']),
                      None if a['slength'] is None else ctypes.byref(a['slength']), (ctypes.c_double * 3)(*a['defaults']),
                      (ctypes.c_double * 6)(*a['vectors']), a['h_max'], a['kernel'], a['mode'], a['dims'],
                      (ctypes.c_uint32 * 3)(*a['cells']), _ptr(a['rows']), _ptr(a['cell']), a['n'], a['surface'], _ptr(counts),
                      _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), summary)

        def untouched(message):
            assert list(summary) == [77] * 22, message
            assert _host(counts).tolist() == [77] * n, message
            for out in outs:
                assert _host(out).tolist() == [77.0] * n, message

        huge = entry_of(name)
        huge.N = 2 ** 32
        flat_vectors = hoomd.box_vectors(np.asarray(FLAT, np.float32))
        wide_vectors = hoomd.box_vectors(np.asarray([2000, 2000, 2000, 0, 0, 0], np.float32))
        for changes, message in (
                (dict(entry=entry_of('particles/typeid')), "float32 or float64"), (dict(entry=entry_of('particles/mass')), "3 columns"),
                (dict(entry=huge), "2^32 rows"), (dict(n=2 ** 32), "2^32 entries"), (dict(dims=4), "dimensions is 2 or 3"),
                (dict(h_max=0.0), "h_max"), (dict(h_max=-1.0), "h_max"), (dict(h_max=float('inf')), "h_max"),
                (dict(h_max=float('nan')), "h_max"), (dict(kernel=2), "the kernel is 0"), (dict(mode=2), "the mode is 0 (gather) or 1 (mean)"),
                (dict(mass=entry_of('particles/typeid')), "the mass chunk holds float32 or float64"),
                (dict(density=entry_of(name)), "the density chunk has 1 column"),
                (dict(mass=entry_of('particles/mass')), "the mass chunk and the position chunk differ"),
                (dict(slength=entry_of('particles/typeid')), "the slength chunk holds float32 or float64"),
                (dict(slength=entry_of(name)), "the slength chunk has 1 column"),
                (dict(slength=entry_of('particles/slength')), "the slength chunk and the position chunk differ"),
                (dict(vectors=[10, 0, 6, 0, 0, 0]), "box lengths"), (dict(cells=(0, 5, 4)), "1 to 1024 cells"),
                (dict(cells=(1025, 5, 4)), "1 to 1024 cells"), (dict(cells=(8, 5, 4)), "narrower than the support"),
                (dict(cells=(7, 6, 4)), "narrower than the support"), (dict(cells=(7, 5, 5)), "narrower than the support"),
                (dict(dims=2, vectors=flat_vectors, cells=(2, 3, 2)), "one z cell"),
                (dict(h_max=1.51, cells=(1, 1, 1)), "count twice"),
                (dict(vectors=wide_vectors, h_max=0.5, cells=(1024, 1024, 2)), "2^20 cells"),
                (dict(cell=d_desc), "descends or lies outside"), (dict(cell=d_outc), "descends or lies outside"),
                (dict(rows=d_outr), "outside the chunks"), (dict(cells=(7, 5, 3)), "descends or lies outside"),
                # a declared bound below a listed h: found on the device (the grid of 0.3 would be legal for the box)
                (dict(h_max=float(np.nextafter(np.float64(want.h_max), 0))), "a listed smoothing length exceeds h_max"),
                (dict(h_max=0.3), "a listed smoothing length exceeds h_max")):
            assert raw(**changes) == _lib.ERROR_INVALID_ARGUMENT and message in _lib.last_error(), (message, _lib.last_error())
            untouched(message)
        # the call after a refusal, as it is: correct; a larger declared bound gives the same result
        for h_max in (want.h_max, 0.625):
            assert raw(h_max=h_max) == 0
            assert words_equal(np.array(list(summary), np.uint64), want.summary)
            assert np.array_equal(_host(counts), want.count) and bits_equal(_host(outs[0]), want.number)
            assert bits_equal(_host(outs[1]), want.density) and bits_equal(_host(outs[2]), want.shepard)
            assert bits_equal(_host(outs[3]), want.omega)
        # mean mode leaves out_omega as it is; without a volume the shepard array stays; n == 0 is the summary of no entry
        assert raw(mode=1, density=None) == 0
        mean = hoomd.sph_adaptive_sums(host, TRICLINIC, s, mass=mass, rows=np.arange(n), cells=(7, 5, 4), mode='mean')
        assert words_equal(np.array(list(summary), np.uint64), mean.summary) and bits_equal(_host(outs[1]), mean.density)
        assert bits_equal(_host(outs[2]), want.shepard) and bits_equal(_host(outs[3]), want.omega)
        assert raw(n=0) == 0
        inf = np.array([np.inf, -np.inf] * 5 + [0.0]).view(np.uint64).tolist()
        assert list(summary) == [0] * 5 + [NONE] * 2 + [0, 0, NONE] + inf + [0]
        f.wait_read()


# ---------------------------------------------------------------- through pgsd.hoomd
WHERE = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
CELL = hoomd.domain_grid(2, 2, 1)[1]
SELECTIONS = {"all": {}, "where": {'where': WHERE}, "domain": {'domain': CELL}, "both": {'where': WHERE, 'domain': CELL}}


@pytest.mark.parametrize("selection", sorted(SELECTIONS))
def test_frame_adaptive_sums_device_equals_the_host_model(data, selection):
    """The frame as stored: a slength that differs from row to row -- the frame `frame_kernel_sums_device` refuses --, with
    where, domain, surface_below and return_rows."""
    path, _ = data
    kwargs = SELECTIONS[selection]
    with hoomd.open(path, 'r') as t:
        with pytest.raises(ValueError, match="a per-particle smoothing length is not supported; pass h"):
            t.frame_kernel_sums_device(0, **kwargs)
        for options in (dict(surface_below=0.03), dict(mode='mean', kernel='cubic_spline', cells=(12, 10, 8))):
            want = t.frame_adaptive_sums(0, **options, **kwargs)
            got = t.frame_adaptive_sums_device(0, return_rows=True, **options, **kwargs)
            assert equal(got, want, (selection, options))
        summary_only = t.frame_adaptive_sums_device(0, surface_below=0.03, **kwargs)
        assert summary_only.number is None and summary_only.count is None
        assert words_equal(summary_only.summary, t.frame_adaptive_sums(0, surface_below=0.03, **kwargs).summary)
        assert summary_only.surface is not None and summary_only.deviation is not None and summary_only.omega_min is not None
        if selection == "all":
            assert got.n == N and got.nowhere > 0 and got.bad_h == 4
        else:
            assert 0 < got.n < N
        with pytest.raises(ValueError, match="narrower"):
            t.frame_adaptive_sums_device(0, cells=(17, 12, 9), **kwargs)
        with pytest.raises(ValueError, match="kernel is one of"):
            t.frame_adaptive_sums_device(0, kernel='gaussian', **kwargs)
        with pytest.raises(ValueError, match="mode is one of"):
            t.frame_adaptive_sums_device(0, mode='scatter', **kwargs)
        with pytest.raises(IndexError):
            t.frame_adaptive_sums_device(2)


def test_a_frame_without_a_slength_and_a_selection_of_nothing(data):
    """Frame 1 stores a position and nothing else: the schema's slength 1.0, mass 1.0 and density 0.0 stand for every row,
    in the model and on the GPU alike.  A selection that keeps no row is answered without a launch."""
    path, _ = data
    with hoomd.open(path, 'r') as t:
        want = t.frame_adaptive_sums(1)
        got = t.frame_adaptive_sums_device(1, return_rows=True)
        assert equal(got, want, "defaults") and got.h_max == 1.0 and got.volume and got.shepard_min == np.inf and got.n == N1
        nothing = {'density': (5000.0, 6000.0)}
        want = t.frame_adaptive_sums(0, where=nothing)
        got = t.frame_adaptive_sums_device(0, where=nothing, return_rows=True)
        assert want.n == 0 and words_equal(got.summary, want.summary) and got.grid == want.grid and got.pairs == 0


# ---------------------------------------------------------------- without a tensor library
CHILD = r'''
import os, pickle, sys
sys.modules["torch"] = None                    # `import torch` raises ImportError from here on
root, path, out_path = sys.argv[1:4]
sys.path[:0] = [os.path.join(root, "pgsd-sph_amd"), os.path.join(root, "tests")]
import pgsd.fl as fl
import pgsd.hoomd as hoomd
from pgsd import _lib
assert _lib._torch is None
with hoomd.open(path, 'r') as t:
    got = t.frame_adaptive_sums_device(0, where={'type': ['wall', 'fluid']}, return_rows=True)
    names = ('rows', 'cell', 'count', 'number', 'density', 'shepard', 'omega')
    for name in names:
        assert isinstance(getattr(got, name), fl.DeviceBuffer) and getattr(got, name).shape == (got.n,), name
    res = dict((name, getattr(got, name).to_host()) for name in names)
    res['summary'] = got.summary
pickle.dump(res, open(out_path, "wb"))
'''


def test_the_rows_stay_in_device_memory_without_torch(data, tmp_path):
    """return_rows without a tensor library, in a fresh child process: the five arrays are DeviceBuffers of n entries."""
    path, _ = data
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, path, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))
    with hoomd.open(path, 'r') as t:
        want = t.frame_adaptive_sums(0, where={'type': ['wall', 'fluid']})
    assert words_equal(res['summary'], want.summary) and 0 < want.n < N
    assert np.array_equal(res['rows'], want.rows) and np.array_equal(res['cell'], want.cell)
    assert res['count'].dtype == np.uint32 and np.array_equal(res['count'], want.count)
    for name in ('number', 'density', 'shepard', 'omega'):
        assert bits_equal(res[name], getattr(want, name)), name
