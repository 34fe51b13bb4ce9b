"""The SPH accelerations on the GPU: pgsd_sph_accelerations_device behind pgsd.fl's sph_accelerations_device and
pgsd.hoomd's frame_accelerations_device.  Every per-entry array and every summary word must equal the numpy model
pgsd.hoomd.sph_accelerations / frame_accelerations exactly, the floats bit for bit (tests/test_sph_force_model.py holds
the model against a plain double loop; a NaN equals a NaN, whose sign and payload IEEE 754 leaves to the processor).  The
cases at the pgsd.fl level read constructed chunks, once with float32 and once with float64 positions, with both kernels,
with and without the viscous term, and order the list on the GPU first, as a caller does.  A model result is computed
once and shared."""
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
from sph_force_cases import CASES as SHARED_CASES, MUTATIONS, TERMS, pressures, velocities, words_equal  # noqa: E402

N = 20_011
N1 = 5_003
TYPES = ['fluid', 'wall', 'inlet']
DTYPES = {'f32': np.float32, 'f64': np.float64}
COLUMNS = ('velocity', 'mass', 'density', 'pressure')
CASES = dict(SHARED_CASES)         # (and behind them the mutation cases, as chunks of the same file)
MUTATION_TERMS = {}
for _k, (_name, (_switch, _case)) in enumerate(sorted(MUTATIONS.items())):
    _kw = dict(_case)
    MUTATION_TERMS['mutation_%02d' % _k] = dict(viscosity=_kw.pop('viscosity', None), gravity=_kw.pop('gravity', None))
    CASES['mutation_%02d' % _k] = (np.asarray(_kw.pop('position'), np.float64), np.asarray(_kw.pop('velocity'), np.float64),
                                   _kw.pop('mass', None), _kw.pop('density', None), _kw.pop('pressure', None), _kw)
MUTATION_CASE = dict((name, 'mutation_%02d' % k) for k, name in enumerate(sorted(MUTATIONS)))
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
    slength of 0.305 and random positions in the triclinic box (the pgsd.hoomd level), and every case's positions as a
    float32 and a float64 log chunk with its velocity, mass, density and pressure columns in both element types.  Frame 1:
    5 003 other particles with a slength that is not uniform and nothing else stored (another N: frame 0's chunks do not
    stand in).  The host's arrays beside it."""
    path = os.path.join(_dir(tmp_path_factory, "sphf"), "pgsd_sph_forces_%d.gsd" % os.getpid())
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
    for name, (p, w, mass, density, pressure, _) in CASES.items():
        for key, dt in DTYPES.items():
            arrays[chunk(name, key)] = fr.log['%s_%s' % (name, key)] = np.ascontiguousarray(p.astype(dt))
            for column, values in zip(COLUMNS, (w, mass, density, pressure)):
                if values is not None:
                    arrays[chunk(name + '_' + column, key)] = fr.log['%s_%s_%s' % (name, column, key)] = \
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


def to_device(f, a):
    return fl._device_from_host(np.ascontiguousarray(a, dtype=np.int32), f.pipeline_device())


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr() if hasattr(x, 'data_ptr') else x.ptr)


def equal(got, want, what):
    """The kernel's KernelAccelerations (per-entry arrays in GPU memory) against the model's."""
    assert words_equal(got.summary, want.summary), (what, got, want, got.summary, want.summary)
    assert got.grid == want.grid and got.kernel == want.kernel and got.h == want.h and got.G == want.G, what
    assert got.dimensions == want.dimensions and got.viscosity == want.viscosity and got.gravity == want.gravity, what
    for name in ('n', 'nowhere', 'not_finite', 'total_at', 'total_row', 'pressure_at', 'pressure_row', 'viscous_at', 'viscous_row'):
        assert getattr(got, name) == getattr(want, name), (what, name)
    assert got.force_time_step() == want.force_time_step(), what
    if got.total is not None:
        assert np.array_equal(_host(got.rows), want.rows) and np.array_equal(_host(got.cell), want.cell), what
        for name in ('pressure_acc', 'viscous_acc', 'total'):
            mine, theirs = getattr(got, name), getattr(want, name)
            assert (mine is None) == (theirs is None), (what, name)
            if theirs is not None:
                mine = _host(mine)
                assert mine.shape == theirs.shape and mine.dtype == np.float64, (what, name)
                assert bits_equal(mine.ravel(), theirs.ravel()), (what, name)
    return True


def model(arrays, name, key, kernel, rows, columns, terms, kw):
    """The model over the arrays the chunks hold, computed once per argument set."""
    tag = (name, key, kernel, None if rows is None else tuple(int(r) for r in rows), columns, tuple(sorted(terms.items())))
    if tag not in _MODEL:
        w, mass, density, pressure = (arrays.get(chunk(name + '_' + c, columns)) for c in COLUMNS)
        _MODEL[tag] = hoomd.sph_accelerations(arrays[chunk(name, key)], w, mass=mass, density=density, pressure=pressure,
                                              rows=rows, kernel=kernel, **terms, **kw)
    return _MODEL[tag]


def accelerations(f, arrays, name, key, kernel, terms, rows=None, return_rows=True, columns=None, **kw):
    """Order the list on the GPU, run the pass; the model over the arrays the chunks hold beside it.  ``columns``: the
    element type key of the velocity, mass, density and pressure chunks (the positions' by default); ``terms``: the
    viscosity and the gravity."""
    columns = key if columns is None else columns
    host = arrays[chunk(name, key)]
    stored = [(0, chunk(name + '_' + c, columns)) if chunk(name + '_' + c, columns) in arrays else None for c in COLUMNS]
    box, h, dims = kw['box'], kw['h'], kw.get('dimensions', 3)
    want = model(arrays, name, key, kernel, rows, columns, terms, kw)
    every = np.arange(len(host)) if rows is None else np.asarray(rows)
    d_rows = to_device(f, every)
    d_cell = f.order_rows_by_cell_device(0, chunk(name, key), box, want.grid, d_rows, n=len(every), dimensions=dims)
    got = f.sph_accelerations_device(0, chunk(name, key), box, h, want.grid, d_rows, d_cell, n=len(every), velocity=stored[0],
                                     mass=stored[1], density=stored[2], pressure=stored[3], dimensions=dims, kernel=kernel,
                                     return_rows=return_rows, **terms)
    return got, want


# ---------------------------------------------------------------- constructed cases
@pytest.mark.parametrize("terms", sorted(TERMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("key", sorted(DTYPES))
@pytest.mark.parametrize("name", [c for c in sorted(CASES) if not c.startswith('mutation')])
def test_a_case_equals_the_model(data, name, key, kernel, terms):
    path, arrays = data
    kw = CASES[name][5]
    viscous = terms == 'viscous'
    with fl.open(path, 'r') as f:
        got, want = accelerations(f, arrays, name, key, kernel, TERMS[terms], **kw)
        assert equal(got, want, (name, key, kernel, terms))
        f.wait_read()
    assert want.n == len(arrays[chunk(name, key)]) and (got.viscous_acc is None) == (not viscous)
    if name == 'all_nowhere':
        assert got.nowhere == 100 and got.total2 is None and got.pressure_at is None and got.force_time_step() is None
        for a in (got.pressure_acc, got.viscous_acc, got.total):        # +0.0, the gravity notwithstanding
            assert a is None or (not _host(a).any() and not np.signbit(_host(a)).any())
    if name in ('one_cell_65', 'mass_only', 'no_density'):
        # the density is the default 0.0: every A is infinite and every own term inf * 0
        assert got.not_finite == got.n - got.nowhere and got.total2 is None and np.isnan(_host(got.pressure_acc)).all()
    if name == 'no_pressure':
        assert not _host(got.pressure_acc).any() and got.pressure2 == 0.0
    if name == 'no_velocity' and viscous:
        assert not _host(got.viscous_acc).any() and got.viscous2 == 0.0 and _host(got.pressure_acc).any()
    if name == 'no_mass':
        assert got.not_finite == 0 and got.pressure2 > 0
    if name == 'clump_700':
        assert got.pressure2 > 0 and (not viscous or got.viscous2 > 0)      # sums of some hundred terms, longer than a workgroup
    if name == 'sparse_64cubed':
        assert got.grid == (64, 64, 64) and got.total2 > 0
    if name == 'flat':
        assert got.dimensions == 2 and not _host(got.pressure_acc)[:, 2].any() and (not viscous or _host(got.viscous_acc)[:, 2].any())
    if name == 'three_cells':
        lost = _host(got.cell) == 27
        assert got.nowhere == lost.sum() > 0 and not _host(got.total)[lost].any()
        assert not np.signbit(_host(got.total)[lost]).any() and not np.signbit(_host(got.pressure_acc)[lost]).any()
    if name == 'boundary':
        # 2h itself is not counted: row 1's infinite A would make row 0's sums NaN
        at = dict(zip(_host(got.rows).tolist(), range(got.n)))
        assert np.isfinite(_host(got.total)[at[0]]).all() and np.isnan(_host(got.total)[at[1]]).all()
    if name == 'mass_density':
        assert 0 < got.not_finite < got.n and np.isnan(_host(got.total)).any() and got.total2 > 0


@pytest.mark.parametrize("columns", sorted(DTYPES))
@pytest.mark.parametrize("key", sorted(DTYPES))
def test_column_chunks_of_either_element_type(data, key, columns):
    """float32 and float64 velocity, mass, density and pressure chunks beside positions of either type; a row with density
    0, one with a NaN density and one with an infinite pressure."""
    path, arrays = data
    with fl.open(path, 'r') as f:
        for kernel in KERNELS:
            for terms in sorted(TERMS):
                got, want = accelerations(f, arrays, 'mass_density', key, kernel, TERMS[terms], columns=columns,
                                          **CASES['mass_density'][5])
                assert equal(got, want, (key, columns, kernel, terms)) and got.not_finite > 0
        f.wait_read()


@pytest.mark.parametrize("key", sorted(DTYPES))
def test_lists_of_0_1_63_64_65_entries_repeats_and_any_order(data, key):
    """n in {0, 1, 63, 64, 65}; a list in descending order with rows listed twice (two entries at distance 0)."""
    path, arrays = data
    kw = CASES['three_cells'][5]
    with fl.open(path, 'r') as f:
        for n in (0, 1, 63, 64, 65):
            for terms in sorted(TERMS):
                got, want = accelerations(f, arrays, 'three_cells', key, 'wendland_c2', TERMS[terms], rows=np.arange(100, 100 + n), **kw)
                assert equal(got, want, (key, n, terms)) and got.n == n
        got, want = accelerations(f, arrays, 'three_cells', key, 'cubic_spline', TERMS['viscous'], rows=np.arange(0), **kw)
        assert equal(got, want, (key, 'nothing')) and got.n == 0 and got.total2 is None and got.viscous_at is None
        rows = np.concatenate([np.arange(400, 0, -1), [7, 7, 400, 12]])
        for kernel in KERNELS:
            got, want = accelerations(f, arrays, 'three_cells', key, kernel, TERMS['viscous'], rows=rows, **kw)
            assert equal(got, want, (key, kernel)) and got.n == 404
        f.wait_read()


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_the_kernel_on_every_mutation_case(data, mutation):
    """The case on which the mutated loop differs from the model (tests/test_sph_force_model.py): the kernel equals the
    model there, so it does not hold the mutation."""
    path, arrays = data
    name = MUTATION_CASE[mutation]
    kw = dict(CASES[name][5])
    kernels = [kw.pop('kernel')] if 'kernel' in kw else KERNELS
    case = MUTATIONS[mutation][1]
    key = 'f64' if case['position'].dtype == np.float64 else 'f32'
    columns = 'f64' if case['velocity'].dtype == np.float64 else 'f32'
    with fl.open(path, 'r') as f:
        for kernel in kernels:
            got, want = accelerations(f, arrays, name, key, kernel, MUTATION_TERMS[name], columns=columns, **kw)
            assert equal(got, want, (mutation, kernel))
        f.wait_read()


# ---------------------------------------------------------------- staging, the per-entry outputs
def test_a_second_call_is_served_from_the_staged_rows_and_return_rows(data):
    path, arrays = data
    name, kw = 'triclinic_754', CASES['triclinic_754'][5]
    n = len(arrays[chunk(name, 'f32')])
    once = n * (12 + 12 + 4 + 4 + 4)                        # position by the ordering, then four columns
    with fl.open(path, 'r') as f:
        f.device_read_stats(reset=True)
        got, want = accelerations(f, arrays, name, 'f32', 'wendland_c2', TERMS['viscous'], **kw)
        assert f.device_read_stats()["pread_bytes"] == once and equal(got, want, "first")
        got, _ = accelerations(f, arrays, name, 'f32', 'wendland_c2', TERMS['viscous'], return_rows=False, **kw)
        assert f.device_read_stats()["pread_bytes"] == once and equal(got, want, "second")
        assert got.rows is None and got.cell is None and got.pressure_acc is None and got.viscous_acc is None
        assert got.total is None and got.total2 == want.total2
        f.wait_read()
        f.device_read_stats(reset=True)
        got, _ = accelerations(f, arrays, name, 'f32', 'cubic_spline', TERMS['plain'], **kw)
        assert f.device_read_stats()["pread_bytes"] == once                    # released by wait_read: read again
        assert _host(got.total).dtype == np.float64 and _host(got.pressure_acc).shape == (n, 3) and got.viscous_acc is None
        f.wait_read()


# ---------------------------------------------------------------- refusals
def test_what_the_python_layers_refuse(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    with fl.open(path, 'r') as f:
        rows = to_device(f, np.arange(100))
        cell = f.order_rows_by_cell_device(0, name, TRICLINIC, (7, 5, 4), rows, n=100)

        def call(name=name, box=TRICLINIC, h=0.625, cells=(7, 5, 4), rows=rows, cell=cell, **kw):
            return f.sph_accelerations_device(0, name, box, h, cells, rows, cell, **kw)

        for kw, message in ((dict(h=0.0), "finite and positive"), (dict(h=float('nan')), "finite and positive"),
                            (dict(h=float('inf')), "finite and positive"), (dict(cells=(8, 5, 4)), "narrower"),
                            (dict(cells=(7, 5)), "three counts"), (dict(cells=(0, 5, 4)), "1 to 1024"),
                            (dict(h=1.51, cells=(1, 1, 1)), "count twice"), (dict(kernel='gaussian'), "kernel is one of"),
                            (dict(dimensions=2), "one z cell"), (dict(dimensions=4, cells=(1, 1, 1)), "dimensions is 2 or 3"),
                            (dict(n=101), "fewer entries than n"), (dict(name='particles/typeid'), "float32 or float64"),
                            (dict(name='particles/mass'), "3 columns"), (dict(box=[1, 2, 3]), "6 values"),
                            (dict(mass=(0, 'particles/typeid')), "mass chunk holds float32 or float64"),
                            (dict(density=(0, 'particles/position')), "density chunk has 1 column"),
                            (dict(mass=(0, 'particles/mass')), "differ in their number of rows"),
                            (dict(velocity=(0, 'particles/typeid')), "velocity chunk holds float32 or float64"),
                            (dict(velocity=(0, 'particles/mass')), "velocity chunk has 3 columns"),
                            (dict(velocity=(0, 'particles/velocity')), "velocity chunk and the position chunk differ"),
                            (dict(pressure=(0, 'particles/typeid')), "pressure chunk holds float32 or float64"),
                            (dict(pressure=(0, 'particles/velocity')), "pressure chunk has 1 column"),
                            (dict(pressure=(0, 'particles/pressure')), "pressure chunk and the position chunk differ"),
                            (dict(defaults=[1.0, 0.0]), "a mass, a density and a pressure"),
                            (dict(viscosity=-1.0), "viscosity is a finite number"), (dict(gravity=(0, 0)), "three finite numbers"),
                            (dict(box=WIDE, h=0.025, cells=(1024, 1024, 2)), "2\\^20 cells")):
            with pytest.raises(ValueError, match=message):
                call(**kw)
        with pytest.raises(KeyError):
            call(name='log/nothing')
        with pytest.raises(KeyError):
            call(pressure=(0, 'log/nothing'))
        f.wait_read()


def test_every_refusal_has_its_message_and_leaves_the_outputs_untouched(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    host = arrays[name]
    w, mass, density, pressure = (arrays[chunk('triclinic_754_' + c, 'f32')] for c in COLUMNS)
    n = 500
    asked = dict(mass=mass, density=density, pressure=pressure, rows=np.arange(n), cells=(7, 5, 4))
    gravity = (0.25, -9.81, 0.5)
    want = hoomd.sph_accelerations(host, w, TRICLINIC, 0.625, viscosity=0.7, gravity=gravity, **asked)
    fn = _lib.lib.pgsd_sph_accelerations_device
    fn.restype = ctypes.c_int32
    D, U, E = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_lib.IndexEntry)
    fn.argtypes = [ctypes.POINTER(_lib.Handle), E, E, E, E, E, D, D, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, U,
                   ctypes.c_double, D, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
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
        summary = (ctypes.c_uint64 * 12)(*([77] * 12))
        outs = [fl._device_from_host(np.full(3 * n, 77.0), f.pipeline_device()) for _ in range(3)]
        good = dict(entry=entry_of(name), velocity=entry_of(chunk('triclinic_754_velocity', 'f32')),
                    mass=entry_of(chunk('triclinic_754_mass', 'f32')), density=entry_of(chunk('triclinic_754_density', 'f32')),
                    pressure=entry_of(chunk('triclinic_754_pressure', 'f32')), defaults=[1.0, 0.0, 0.0],
                    vectors=hoomd.box_vectors(np.asarray(TRICLINIC, np.float32)), h=0.625, kernel=0, dims=3, cells=(7, 5, 4),
                    viscosity=0.7, gravity=gravity, rows=d_rows, cell=d_cell, n=n)

        def raw(**changes):
            a = dict(good, **changes)
            optional = [None if a[c] is None else ctypes.byref(a[c]) for c in COLUMNS]
            return fn(h, ctypes.byref(a['entry']), optional[0], optional[1], optional[2], optional[3],
                      (ctypes.c_double * 3)(*a['defaults']), (ctypes.c_double * 6)(*a['vectors']), a['h'], a['kernel'], a['dims'],
                      (ctypes.c_uint32 * 3)(*a['cells']), a['viscosity'], (ctypes.c_double * 3)(*a['gravity']), _ptr(a['rows']),
                      _ptr(a['cell']), a['n'], _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), summary)

        def untouched(which=range(3)):
            return all(_host(outs[k]).tolist() == [77.0] * (3 * n) for k in which)

        huge = entry_of(name)
        huge.N = 2 ** 32
        flat_vectors = hoomd.box_vectors(np.asarray(FLAT, np.float32))
        wide_vectors = hoomd.box_vectors(np.asarray([2000, 2000, 2000, 0, 0, 0], np.float32))
        inf, nan = float('inf'), float('nan')
        for changes, message in (
                (dict(entry=entry_of('particles/typeid')), "float32 or float64"), (dict(entry=entry_of('particles/mass')), "3 columns"),
                (dict(entry=huge), "2^32 rows"), (dict(n=2 ** 32), "2^32 entries"), (dict(dims=4), "dimensions is 2 or 3"),
                (dict(h=0.0), "finite and positive"), (dict(h=-1.0), "finite and positive"),
                (dict(h=inf), "finite and positive"), (dict(h=nan), "finite and positive"),
                (dict(kernel=2), "the kernel is 0"), (dict(mass=entry_of('particles/typeid')), "the mass chunk holds float32 or float64"),
                (dict(density=entry_of(name)), "the density chunk has 1 column"),
                (dict(mass=entry_of('particles/mass')), "the mass chunk and the position chunk differ"),
                (dict(density=entry_of('particles/density')), "the density chunk and the position chunk differ"),
                (dict(velocity=entry_of('particles/typeid')), "the velocity chunk holds float32 or float64"),
                (dict(velocity=entry_of(chunk('triclinic_754_mass', 'f32'))), "the velocity chunk has 3 columns"),
                (dict(velocity=entry_of('particles/velocity')), "the velocity chunk and the position chunk differ"),
                (dict(pressure=entry_of('particles/typeid')), "the pressure chunk holds float32 or float64"),
                (dict(pressure=entry_of(name)), "the pressure chunk has 1 column"),
                (dict(pressure=entry_of('particles/pressure')), "the pressure chunk and the position chunk differ"),
                (dict(viscosity=nan), "the viscosity must be finite"), (dict(viscosity=inf), "the viscosity must be finite"),
                (dict(viscosity=-inf), "the viscosity must be finite"),
                (dict(gravity=(0.0, nan, 0.0)), "the gravity must hold three finite components"),
                (dict(gravity=(inf, 0.0, 0.0)), "the gravity must hold three finite components"),
                (dict(gravity=(0.0, 0.0, -inf)), "the gravity must hold three finite components"),
                (dict(vectors=[10, 0, 6, 0, 0, 0]), "box lengths"), (dict(cells=(0, 5, 4)), "1 to 1024 cells"),
                (dict(cells=(1025, 5, 4)), "1 to 1024 cells"), (dict(cells=(8, 5, 4)), "narrower than the support"),
                (dict(cells=(7, 6, 4)), "narrower than the support"), (dict(cells=(7, 5, 5)), "narrower than the support"),
                (dict(dims=2, vectors=flat_vectors, cells=(2, 3, 2)), "one z cell"),
                (dict(h=1.51, cells=(1, 1, 1)), "count twice"), (dict(vectors=wide_vectors, h=0.5, cells=(1024, 1024, 2)), "2^20 cells"),
                (dict(cell=d_desc), "descends or lies outside"), (dict(cell=d_outc), "descends or lies outside"),
                (dict(rows=d_outr), "outside the chunks"), (dict(cells=(7, 5, 3)), "descends or lies outside")):
            assert raw(**changes) == _lib.ERROR_INVALID_ARGUMENT and message in _lib.last_error(), (message, _lib.last_error())
            assert "pgsd_sph_accelerations_device" in _lib.last_error()
            assert list(summary) == [77] * 12, message
            assert untouched(), message
        # the call after them, as it is: correct
        assert raw() == 0
        assert words_equal(np.array(list(summary), np.uint64), want.summary)
        assert bits_equal(_host(outs[0]), want.pressure_acc.ravel()) and bits_equal(_host(outs[1]), want.viscous_acc.ravel())
        assert bits_equal(_host(outs[2]), want.total.ravel())
        # without a pressure chunk the default stands for every row
        assert raw(pressure=None, defaults=[1.0, 0.0, 2.5e4]) == 0
        flat = hoomd.sph_accelerations(host, w, TRICLINIC, 0.625, viscosity=0.7, gravity=gravity,
                                       **dict(asked, pressure=np.full(len(host), 2.5e4)))
        assert words_equal(np.array(list(summary), np.uint64), flat.summary) and bits_equal(_host(outs[2]), flat.total.ravel())
        assert bits_equal(_host(outs[1]), want.viscous_acc.ravel())
        # a negative viscosity: no viscous term, and the second array stays as it was; n == 0 is the summary of no entry
        outs[1] = fl._device_from_host(np.full(3 * n, 77.0), f.pipeline_device())
        assert raw(viscosity=-1.0) == 0
        none = hoomd.sph_accelerations(host, w, TRICLINIC, 0.625, gravity=gravity, **asked)
        assert words_equal(np.array(list(summary), np.uint64), none.summary) and untouched((1,))
        assert bits_equal(_host(outs[0]), want.pressure_acc.ravel()) and bits_equal(_host(outs[2]), none.total.ravel())
        assert raw(n=0) == 0
        assert list(summary) == [0] * 3 + [NONE] * 6 + [0] * 3
        f.wait_read()


# ---------------------------------------------------------------- through pgsd.hoomd
WHERE = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
CELL = hoomd.domain_grid(2, 2, 1)[1]
SELECTIONS = {"all": {}, "where": {'where': WHERE}, "domain": {'domain': CELL}, "both": {'where': WHERE, 'domain': CELL}}


@pytest.mark.parametrize("selection", sorted(SELECTIONS))
def test_frame_accelerations_device_equals_the_host_model(data, selection):
    """about_20000: the triclinic box at 2h = 0.61 (h=None from the uniform slength 0.305), with where, domain,
    return_rows, a viscosity and a gravity."""
    path, _ = data
    kwargs = SELECTIONS[selection]
    with hoomd.open(path, 'r') as t:
        for options in (dict(viscosity=0.7, gravity=(0.25, -9.81, 0.5)), dict(h=0.3125, kernel='cubic_spline', cells=(12, 10, 8))):
            want = t.frame_accelerations(0, **options, **kwargs)
            got = t.frame_accelerations_device(0, return_rows=True, **options, **kwargs)
            assert equal(got, want, (selection, options))
            if 'h' not in options:
                assert want.h == float(np.float32(0.305)) and want.viscous2 > 0
                summary_only = t.frame_accelerations_device(0, **options, **kwargs)
                assert summary_only.total is None and summary_only.pressure_acc is None
                assert words_equal(summary_only.summary, want.summary) and summary_only.total2 is not None
        assert want.h == 0.3125 and want.viscous_acc is None
        if selection == "all":
            assert got.n == N and got.nowhere > 0
        else:
            assert 0 < got.n < N
        with pytest.raises(ValueError, match="narrower"):
            t.frame_accelerations_device(0, 0.65, cells=(8, 5, 4), **kwargs)
        with pytest.raises(ValueError, match="count twice"):
            t.frame_accelerations_device(0, 1.75, **kwargs)
        with pytest.raises(ValueError, match="kernel is one of"):
            t.frame_accelerations_device(0, 0.3, kernel='gaussian', **kwargs)
        with pytest.raises(ValueError, match="viscosity is a finite number"):
            t.frame_accelerations_device(0, 0.3, viscosity=float('nan'), **kwargs)
        with pytest.raises(ValueError, match="gravity holds three finite numbers"):
            t.frame_accelerations_device(0, 0.3, gravity=(0, 0, float('inf')), **kwargs)
        with pytest.raises(IndexError):
            t.frame_accelerations_device(2, 0.3)


def test_h_none_and_the_defaults_on_the_device(data):
    """Frame 1 stores a slength that is not uniform, and neither typeid, velocity, mass, density nor pressure: every row is
    of type 0, every velocity is the zero vector and the defaults 1.0, 0.0 and 0.0 stand for mass, density and pressure,
    so every A is 0/0, in the model and on the GPU alike."""
    path, _ = data
    with hoomd.open(path, 'r') as t:
        with pytest.raises(ValueError, match="slength ranges from 0.30"):
            t.frame_accelerations_device(1)
        with pytest.raises(ValueError, match="slength ranges from 0.30"):
            t.frame_accelerations(1)
        want = t.frame_accelerations(1, 0.305, viscosity=0.5, where={'type': ['fluid']})
        got = t.frame_accelerations_device(1, 0.305, viscosity=0.5, where={'type': ['fluid']}, return_rows=True)
        assert equal(got, want, "defaults") and got.n == N1 and got.not_finite == got.n - got.nowhere and got.total2 is None


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
    got = t.frame_accelerations_device(0, viscosity=0.7, gravity=(0, 0, -9.81), where={'type': ['wall']}, return_rows=True)
    assert isinstance(got.total, fl.DeviceBuffer) and got.total.shape == (got.n, 3) and got.viscous_acc.shape == (got.n, 3)
    res = dict((name, getattr(got, name).to_host()) for name in ('rows', 'cell', 'pressure_acc', 'viscous_acc', 'total'))
    res['summary'] = got.summary
pickle.dump(res, open(out_path, "wb"))
'''


def test_the_rows_stay_in_device_memory_without_torch(data, tmp_path):
    """return_rows without a tensor library: the three arrays are DeviceBuffers, n x 3."""
    path, _ = data
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, path, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))
    with hoomd.open(path, 'r') as t:
        want = t.frame_accelerations(0, viscosity=0.7, gravity=(0, 0, -9.81), where={'type': ['wall']})
    assert words_equal(res['summary'], want.summary) and 0 < want.n < N
    assert np.array_equal(res['rows'], want.rows) and np.array_equal(res['cell'], want.cell)
    for name in ('pressure_acc', 'viscous_acc', 'total'):
        assert res[name].shape == getattr(want, name).shape and bits_equal(res[name].ravel(), getattr(want, name).ravel()), name
