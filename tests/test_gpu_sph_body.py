"""The SPH body forces on the GPU: pgsd_sph_body_force_device behind pgsd.fl's sph_body_force_device and pgsd.hoomd's
frame_body_force_device.  Every per-target array and every summary word must equal the numpy model
pgsd.hoomd.sph_body_force / frame_body_force exactly, the floats bit for bit (tests/test_sph_body_model.py holds the model
against a plain double loop; a NaN equals a NaN, whose sign and payload IEEE 754 leaves to the processor).  The cases at the
pgsd.fl level read constructed chunks, once with float32 and once with float64 positions, with both kernels, with and
without the viscous term, and order both lists on the GPU first, as a caller does.  A model result is computed once and
shared."""
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
from sph_cases import CUBE, KERNELS, NONE, WIDE, _columns, bits_equal  # noqa: E402
from sph_body_cases import CASES as SHARED_CASES, MUTATIONS, TERMS, pressures, velocities, words_equal  # noqa: E402

N = 20_011
N1 = 5_003
TYPES = ['fluid', 'wall', 'inlet']
DTYPES = {'f32': np.float32, 'f64': np.float64}
COLUMNS = ('velocity', 'mass', 'density', 'pressure')
# name -> (positions, velocities, mass, density, pressure, body rows, fluid rows, keyword arguments)
CASES = dict(SHARED_CASES)         # (and behind them the mutation cases, as chunks of the same file)
MUTATION_TERMS = {}
for _k, (_name, (_switch, _case)) in enumerate(sorted(MUTATIONS.items())):
    _kw = dict(_case)
    MUTATION_TERMS['mutation_%02d' % _k] = dict(viscosity=_kw.pop('viscosity', None), about=_kw.pop('about', None))
    CASES['mutation_%02d' % _k] = (np.asarray(_kw.pop('position'), np.float64), np.asarray(_kw.pop('velocity'), np.float64),
                                   _kw.pop('mass', None), _kw.pop('density', None), _kw.pop('pressure', None),
                                   np.asarray(_kw.pop('body_rows')), np.asarray(_kw.pop('fluid_rows')), _kw)
MUTATION_CASE = dict((name, 'mutation_%02d' % k) for k, name in enumerate(sorted(MUTATIONS)))
# half of the rows nowhere: the targets, or with the lists exchanged the sources
_HALF = random_rows(17, 200, CUBE, np.float64)
_HALF[:100] = np.nan
CASES['half_nowhere'] = (_HALF, velocities(17, 200)) + _columns(17, 200) + (pressures(17, 200), np.arange(100), np.arange(100, 200),
                                                                             dict(box=CUBE, h=0.75))
# 256 * 4096 + 1 targets, so that lane 0 of the final walk takes a second tile; the 40 sources sit in the grid's last
# cell, where 300 of the targets are -- the last target in cell order among them --, so the model stays cheap
BIG = 256 * 4096 + 1


def _big():
    rng = np.random.default_rng(99)
    targets = random_rows(98, BIG, WIDE, np.float32)
    targets[-300:] = rng.uniform(31.05, 31.95, size=(300, 3)).astype(np.float32)
    sources = rng.uniform(31.05, 31.95, size=(40, 3)).astype(np.float32)
    p = np.concatenate([targets, sources])
    n = len(p)
    mass, density = _columns(98, n)
    return (p, velocities(98, n).astype(np.float32), mass.astype(np.float32), density.astype(np.float32),
            pressures(98, n).astype(np.float32), np.arange(BIG), np.arange(BIG, n), dict(box=WIDE, h=0.5, cells=(64, 64, 64)))


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
    slength of 0.305 and random positions in the triclinic box (the pgsd.hoomd level), every case's positions as a float32
    and a float64 log chunk with its velocity, mass, density and pressure columns in both element types, and the large
    case in float32 alone.  Frame 1: 5 003 other particles with a slength that is not uniform and nothing else stored.
    The host's arrays beside it."""
    path = os.path.join(_dir(tmp_path_factory, "sphb"), "pgsd_sph_body_%d.gsd" % os.getpid())
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
    CASES['big'] = _big()
    for name, (p, w, mass, density, pressure, _, _, _) in CASES.items():
        for key, dt in DTYPES.items():
            if name == 'big' and key == 'f64':
                continue
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
    """The kernel's KernelBodyForce (per-target arrays in GPU memory) against the model's."""
    assert words_equal(got.summary, want.summary), (what, got, want, got.summary, want.summary)
    assert got.grid == want.grid and got.kernel == want.kernel and got.h == want.h and got.G == want.G, what
    assert got.dimensions == want.dimensions and got.viscosity == want.viscosity and got.about == want.about, what
    for name in ('n', 'nowhere', 'n_sources', 'sources_nowhere', 'wetted', 'pairs', 'bad', 'largest_at', 'largest_row'):
        assert getattr(got, name) == getattr(want, name), (what, name)
    if got.contacts is not None:
        assert np.array_equal(_host(got.rows), want.rows) and np.array_equal(_host(got.cell), want.cell), what
        mine = _host(got.contacts)
        assert mine.dtype == np.uint32 and np.array_equal(mine, want.contacts), what
        for name in ('pressure_acc', 'viscous_acc'):
            mine, theirs = getattr(got, name), getattr(want, name)
            assert (mine is None) == (theirs is None), (what, name)
            if theirs is not None:
                mine = _host(mine)
                assert mine.shape == theirs.shape and mine.dtype == np.float64, (what, name)
                assert bits_equal(mine.ravel(), theirs.ravel()), (what, name)
    return True


def model(arrays, name, key, kernel, body, fluid, columns, terms, kw):
    """The model over the arrays the chunks hold, computed once per argument set."""
    tag = (name, key, kernel, body.tobytes(), fluid.tobytes(), columns, tuple(sorted(terms.items())))
    if tag not in _MODEL:
        w, mass, density, pressure = (arrays.get(chunk(name + '_' + c, columns)) for c in COLUMNS)
        _MODEL[tag] = hoomd.sph_body_force(arrays[chunk(name, key)], w, body_rows=body, fluid_rows=fluid, mass=mass,
                                           density=density, pressure=pressure, kernel=kernel, **terms, **kw)
    return _MODEL[tag]


def body_force(f, arrays, name, key, kernel, terms, body=None, fluid=None, return_rows=True, columns=None, **kw):
    """Order both lists on the GPU, run the pass; the model over the arrays the chunks hold beside it.  ``columns``: the
    element type key of the velocity, mass, density and pressure chunks (the positions' by default); ``terms``: the
    viscosity and the point the torque is taken about; ``body``, ``fluid``: the case's lists by default."""
    columns = key if columns is None else columns
    body = np.asarray(CASES[name][5] if body is None else body, dtype=np.int64)
    fluid = np.asarray(CASES[name][6] if fluid is None else fluid, dtype=np.int64)
    stored = [(0, chunk(name + '_' + c, columns)) if chunk(name + '_' + c, columns) in arrays else None for c in COLUMNS]
    box, h, dims = kw['box'], kw['h'], kw.get('dimensions', 3)
    want = model(arrays, name, key, kernel, body, fluid, columns, terms, kw)
    lists = []
    for rows in (body, fluid):
        d_rows = to_device(f, rows)
        d_cell = f.order_rows_by_cell_device(0, chunk(name, key), box, want.grid, d_rows, n=len(rows), dimensions=dims)
        lists += [d_rows, d_cell]
    got = f.sph_body_force_device(0, chunk(name, key), box, h, want.grid, lists[0], lists[1], lists[2], lists[3],
                                  n_body=len(body), n_fluid=len(fluid), velocity=stored[0], mass=stored[1], density=stored[2],
                                  pressure=stored[3], dimensions=dims, kernel=kernel, return_rows=return_rows, **terms)
    return got, want


# ---------------------------------------------------------------- constructed cases
@pytest.mark.parametrize("terms", sorted(TERMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("key", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(SHARED_CASES))
def test_a_case_equals_the_model(data, name, key, kernel, terms):
    path, arrays = data
    kw = CASES[name][7]
    viscous = terms == 'viscous'
    with fl.open(path, 'r') as f:
        got, want = body_force(f, arrays, name, key, kernel, TERMS[terms], **kw)
        assert equal(got, want, (name, key, kernel, terms))
        f.wait_read()
    assert want.n == len(CASES[name][5]) and want.n_sources == len(CASES[name][6]) and (got.viscous_acc is None) == (not viscous)
    if name == 'all_nowhere':
        assert got.nowhere == got.n and got.sources_nowhere == got.n_sources and got.largest2 is None and got.pairs == 0
        for a in (got.pressure_acc, got.viscous_acc):
            assert a is None or (not _host(a).any() and not np.signbit(_host(a)).any())
        assert got.force == (0.0, 0.0, 0.0) and got.torque == (0.0, 0.0, 0.0)
    if name in ('one_cell_65', 'mass_only', 'no_density'):
        assert got.bad >= got.wetted > 0 and got.force_pressure == (0.0, 0.0, 0.0)
    if name == 'no_pressure':
        assert not _host(got.pressure_acc).any() and got.largest2 == 0.0
    if name == 'clump_700':
        assert got.pairs > 50_000 and any(got.force)                # runs of some hundred sources, longer than a workgroup
    if name == 'sparse_64cubed':
        assert got.grid == (64, 64, 64) and 0 < got.wetted < got.n
    if name == 'flat':
        assert got.dimensions == 2 and got.force_pressure[2] == 0.0 and got.torque_pressure[2] != 0.0
    if name == 'three_cells':
        lost = _host(got.cell) == 27
        assert got.nowhere == lost.sum() > 0 and got.sources_nowhere > 0 and not _host(got.contacts)[lost].any()
        assert not np.signbit(_host(got.pressure_acc)[lost]).any()
    if name == 'mass_density':
        assert 0 < got.bad < got.n and np.isnan(_host(got.pressure_acc)).any() and np.isfinite(got.force).all()


@pytest.mark.parametrize("columns", sorted(DTYPES))
@pytest.mark.parametrize("key", sorted(DTYPES))
def test_column_chunks_of_either_element_type(data, key, columns):
    """float32 and float64 velocity, mass, density and pressure chunks beside positions of either type; a row with density
    0, one with a NaN density and one with an infinite pressure."""
    path, arrays = data
    with fl.open(path, 'r') as f:
        for kernel in KERNELS:
            for terms in sorted(TERMS):
                got, want = body_force(f, arrays, 'mass_density', key, kernel, TERMS[terms], columns=columns,
                                       **CASES['mass_density'][7])
                assert equal(got, want, (key, columns, kernel, terms)) and got.bad > 0
        f.wait_read()


@pytest.mark.parametrize("key", sorted(DTYPES))
def test_targets_or_sources_that_are_all_nowhere(data, key):
    path, arrays = data
    _, _, _, _, _, body, fluid, kw = CASES['half_nowhere']
    with fl.open(path, 'r') as f:
        for terms in sorted(TERMS):
            got, want = body_force(f, arrays, 'half_nowhere', key, 'wendland_c2', TERMS[terms], **kw)
            assert equal(got, want, (key, terms, 'targets')) and got.nowhere == got.n == 100 and got.sources_nowhere == 0
            assert got.pairs == 0 and got.largest2 is None and not _host(got.pressure_acc).any()
            got, want = body_force(f, arrays, 'half_nowhere', key, 'cubic_spline', TERMS[terms], body=fluid, fluid=body, **kw)
            assert equal(got, want, (key, terms, 'sources')) and got.nowhere == 0 and got.sources_nowhere == 100
            assert got.pairs == 0 and got.wetted == 0 and got.largest2 == 0.0 and got.force == (0.0, 0.0, 0.0)
        f.wait_read()


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097))
def test_bodies_of_every_size_around_a_wave_a_workgroup_and_a_tile(data, n):
    """n_body around 64, 256 and 4096 over the 4 097 rows of three_cells; the sources are 600 of the same rows, so the
    lists overlap."""
    path, arrays = data
    kw = CASES['three_cells'][7]
    with fl.open(path, 'r') as f:
        for key, kernel, terms in (('f32', 'wendland_c2', 'viscous'), ('f64', 'cubic_spline', 'plain')):
            got, want = body_force(f, arrays, 'three_cells', key, kernel, TERMS[terms], body=np.arange(n), fluid=np.arange(3000, 3600),
                                   **kw)
            assert equal(got, want, (key, n, terms)) and got.n == n and got.n_sources == 600
        if n == 0:
            assert got.largest2 is None and got.sources_nowhere == 0 and not got.summary[9:].any()
        else:
            assert got.wetted > 0 or n == 1
        f.wait_read()


@pytest.mark.parametrize("key", sorted(DTYPES))
def test_no_source_one_source_repeats_and_any_order(data, key):
    path, arrays = data
    kw = CASES['three_cells'][7]
    with fl.open(path, 'r') as f:
        for terms in sorted(TERMS):
            got, want = body_force(f, arrays, 'three_cells', key, 'wendland_c2', TERMS[terms], body=np.arange(500), fluid=np.arange(0),
                                   **kw)
            assert equal(got, want, (key, terms, 'dry')) and got.n_sources == 0 and got.pairs == 0 and got.wetted == 0
            assert not got.summary[10:].any() and not _host(got.pressure_acc).any()
            got, want = body_force(f, arrays, 'three_cells', key, 'cubic_spline', TERMS[terms], body=np.arange(500),
                                   fluid=np.array([700]), **kw)
            assert equal(got, want, (key, terms, 'one source')) and got.n_sources == 1 and got.pairs == got.wetted > 0
        body = np.concatenate([np.arange(400, 0, -1), [7, 7, 400, 12]])
        fluid = np.concatenate([np.arange(350, 1200), [7, 500, 500]])
        for kernel in KERNELS:
            got, want = body_force(f, arrays, 'three_cells', key, kernel, TERMS['viscous'], body=body, fluid=fluid, **kw)
            assert equal(got, want, (key, kernel)) and got.n == 404 and got.n_sources == 853
        f.wait_read()


@pytest.mark.parametrize("key", sorted(DTYPES))
def test_lists_that_overlap_wholly_give_the_accelerations(data, key):
    """Both lists are every row: the pass is the accelerations' pair loop, and pressure_acc and viscous_acc are
    sph_accelerations_device's of the same list, bit for bit."""
    path, arrays = data
    name = 'triclinic_754'
    kw = CASES[name][7]
    every = np.arange(len(arrays[chunk(name, key)]))
    stored = [(0, chunk(name + '_' + c, key)) for c in COLUMNS]
    with fl.open(path, 'r') as f:
        for kernel in KERNELS:
            got, want = body_force(f, arrays, name, key, kernel, TERMS['viscous'], body=every, fluid=every, **kw)
            assert equal(got, want, (key, kernel)) and got.n == got.n_sources == len(every)
            d_rows = to_device(f, every)
            d_cell = f.order_rows_by_cell_device(0, chunk(name, key), kw['box'], want.grid, d_rows, n=len(every))
            acc = f.sph_accelerations_device(0, chunk(name, key), kw['box'], kw['h'], want.grid, d_rows, d_cell, n=len(every),
                                             velocity=stored[0], mass=stored[1], density=stored[2], pressure=stored[3],
                                             kernel=kernel, viscosity=TERMS['viscous']['viscosity'], return_rows=True)
            assert np.array_equal(_host(acc.rows), _host(got.rows))
            assert bits_equal(_host(acc.pressure_acc).ravel(), _host(got.pressure_acc).ravel())
            assert bits_equal(_host(acc.viscous_acc).ravel(), _host(got.viscous_acc).ravel())
        f.wait_read()


def test_the_second_round_of_the_tile_walk(data):
    """256 * 4096 + 1 targets: 257 tiles, so lane 0 of the final kernel adds tile 0 and then tile 256, which holds the
    last target alone -- one with contacts."""
    path, arrays = data
    kw = CASES['big'][7]
    with fl.open(path, 'r') as f:
        for kernel, terms in (('wendland_c2', 'viscous'), ('cubic_spline', 'plain')):
            got, want = body_force(f, arrays, 'big', 'f32', kernel, TERMS[terms], **kw)
            assert equal(got, want, ('big', kernel, terms)) and got.n == BIG and got.n_sources == 40
            assert want.contacts[-1] > 0 and want.pressure_acc[-1].any() and 300 <= got.wetted < 2000 and any(got.torque)
        f.wait_read()


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_the_kernel_on_every_mutation_case(data, mutation):
    """The case on which the mutated loop differs from the model (tests/test_sph_body_model.py): the kernel equals the model
    there, so it does not hold the mutation."""
    path, arrays = data
    name = MUTATION_CASE[mutation]
    kw = dict(CASES[name][7])
    kernels = [kw.pop('kernel')] if 'kernel' in kw else KERNELS
    case = MUTATIONS[mutation][1]
    key = 'f64' if case['position'].dtype == np.float64 else 'f32'
    columns = 'f64' if case['velocity'].dtype == np.float64 else 'f32'
    with fl.open(path, 'r') as f:
        for kernel in kernels:
            got, want = body_force(f, arrays, name, key, kernel, MUTATION_TERMS[name], columns=columns, **kw)
            assert equal(got, want, (mutation, kernel))
        f.wait_read()


# ---------------------------------------------------------------- staging, the per-target outputs
def test_a_second_call_is_served_from_the_staged_rows_and_return_rows(data):
    path, arrays = data
    name, kw = 'triclinic_754', CASES['triclinic_754'][7]
    n = len(arrays[chunk(name, 'f32')])
    once = n * (12 + 12 + 4 + 4 + 4)                        # position by the ordering, then four columns: both lists read them
    with fl.open(path, 'r') as f:
        f.device_read_stats(reset=True)
        got, want = body_force(f, arrays, name, 'f32', 'wendland_c2', TERMS['viscous'], **kw)
        assert f.device_read_stats()["pread_bytes"] == once and equal(got, want, "first")
        got, _ = body_force(f, arrays, name, 'f32', 'wendland_c2', TERMS['viscous'], return_rows=False, **kw)
        assert f.device_read_stats()["pread_bytes"] == once and equal(got, want, "second")
        assert got.rows is None and got.cell is None and got.contacts is None and got.pressure_acc is None
        assert got.viscous_acc is None and got.force == want.force and got.torque == want.torque
        f.wait_read()
        f.device_read_stats(reset=True)
        got, _ = body_force(f, arrays, name, 'f32', 'cubic_spline', TERMS['plain'], **kw)
        assert f.device_read_stats()["pread_bytes"] == once                    # released by wait_read: read again
        assert _host(got.contacts).shape == (got.n,) and _host(got.pressure_acc).shape == (got.n, 3) and got.viscous_acc is None
        f.wait_read()


# ---------------------------------------------------------------- refusals
def test_every_refusal_has_its_message_and_leaves_the_outputs_untouched(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    host = arrays[name]
    w, mass, density, pressure = (arrays[chunk('triclinic_754_' + c, 'f32')] for c in COLUMNS)
    n, n_s = 300, 500
    asked = dict(mass=mass, density=density, pressure=pressure, body_rows=np.arange(n), fluid_rows=np.arange(n, n + n_s),
                 cells=(7, 5, 4))
    about = (0.5, -1.25, 2.0)
    want = hoomd.sph_body_force(host, w, TRICLINIC, 0.625, viscosity=0.7, about=about, **asked)
    fluid_rows, fluid_cell, _ = hoomd.cell_order(host, TRICLINIC, np.arange(n, n + n_s), (7, 5, 4))
    fn = _lib.lib.pgsd_sph_body_force_device
    fn.restype = ctypes.c_int32
    D, U, E = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_lib.IndexEntry)
    fn.argtypes = [ctypes.POINTER(_lib.Handle), E, E, E, E, E, D, D, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, U,
                   ctypes.c_double, D, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    with fl.open(path, 'r') as f:
        h = f._h()

        def entry_of(chunk_name):
            return _lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(h, 0, chunk_name.encode()).contents)

        d_rows, d_cell = to_device(f, want.rows), to_device(f, want.cell)
        s_rows, s_cell = to_device(f, fluid_rows), to_device(f, fluid_cell)
        descending, outside_cell, outside_row = want.cell.copy(), want.cell.copy(), want.rows.copy()
        descending[200] = 0
        outside_cell[n - 1] = 141
        outside_row[7] = len(host)
        d_desc, d_outc, d_outr = to_device(f, descending), to_device(f, outside_cell), to_device(f, outside_row)
        descending, outside_cell, outside_row = fluid_cell.copy(), fluid_cell.copy(), fluid_rows.copy()
        descending[300] = 0
        outside_cell[n_s - 1] = 141
        outside_row[7] = len(host)
        s_desc, s_outc, s_outr = to_device(f, descending), to_device(f, outside_cell), to_device(f, outside_row)
        summary = (ctypes.c_uint64 * 22)(*([77] * 22))
        contacts = fl._device_from_host(np.full(n, 77, np.uint32), f.pipeline_device())
        outs = [fl._device_from_host(np.full(3 * n, 77.0), f.pipeline_device()) for _ in range(2)]
        good = dict(entry=entry_of(name), velocity=entry_of(chunk('triclinic_754_velocity', 'f32')),
                    mass=entry_of(chunk('triclinic_754_mass', 'f32')), density=entry_of(chunk('triclinic_754_density', 'f32')),
                    pressure=entry_of(chunk('triclinic_754_pressure', 'f32')), defaults=[1.0, 0.0, 0.0],
                    vectors=hoomd.box_vectors(np.asarray(TRICLINIC, np.float32)), h=0.625, kernel=0, dims=3, cells=(7, 5, 4),
                    viscosity=0.7, about=about, rows=d_rows, cell=d_cell, n=n, rows2=s_rows, cell2=s_cell, n2=n_s)

        def raw(**changes):
            a = dict(good, **changes)
            optional = [None if a[c] is None else ctypes.byref(a[c]) for c in COLUMNS]
            return fn(h, ctypes.byref(a['entry']), optional[0], optional[1], optional[2], optional[3],
                      (ctypes.c_double * 3)(*a['defaults']), (ctypes.c_double * 6)(*a['vectors']), a['h'], a['kernel'], a['dims'],
                      (ctypes.c_uint32 * 3)(*a['cells']), a['viscosity'], (ctypes.c_double * 3)(*a['about']), _ptr(a['rows']),
                      _ptr(a['cell']), a['n'], _ptr(a['rows2']), _ptr(a['cell2']), a['n2'], _ptr(contacts), _ptr(outs[0]),
                      _ptr(outs[1]), summary)

        def untouched(which=range(2)):
            return (all(_host(outs[k]).tolist() == [77.0] * (3 * n) for k in which)
                    and _host(contacts).tolist() == [77] * n)

        huge = entry_of(name)
        huge.N = 2 ** 32
        flat_vectors = hoomd.box_vectors(np.asarray(FLAT, np.float32))
        wide_vectors = hoomd.box_vectors(np.asarray([2000, 2000, 2000, 0, 0, 0], np.float32))
        inf, nan = float('inf'), float('nan')
        for changes, message in (
                (dict(entry=entry_of('particles/typeid')), "float32 or float64"), (dict(entry=entry_of('particles/mass')), "3 columns"),
                (dict(entry=huge), "2^32 rows"), (dict(n=2 ** 32), "2^32 entries"), (dict(n2=2 ** 32), "2^32 entries"),
                (dict(dims=4), "dimensions is 2 or 3"),
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
                (dict(about=(0.0, nan, 0.0)), "about must hold three finite components"),
                (dict(about=(inf, 0.0, 0.0)), "about must hold three finite components"),
                (dict(about=(0.0, 0.0, -inf)), "about must hold three finite components"),
                (dict(vectors=[10, 0, 6, 0, 0, 0]), "box lengths"), (dict(cells=(0, 5, 4)), "1 to 1024 cells"),
                (dict(cells=(1025, 5, 4)), "1 to 1024 cells"), (dict(cells=(8, 5, 4)), "narrower than the support"),
                (dict(cells=(7, 6, 4)), "narrower than the support"), (dict(cells=(7, 5, 5)), "narrower than the support"),
                (dict(dims=2, vectors=flat_vectors, cells=(2, 3, 2)), "one z cell"),
                (dict(h=1.51, cells=(1, 1, 1)), "count twice"), (dict(vectors=wide_vectors, h=0.5, cells=(1024, 1024, 2)), "2^20 cells"),
                (dict(cell=d_desc), "descends or lies outside"), (dict(cell=d_outc), "descends or lies outside"),
                (dict(rows=d_outr), "outside the chunks"), (dict(cell2=s_desc), "descends or lies outside"),
                (dict(cell2=s_outc), "descends or lies outside"), (dict(rows2=s_outr), "outside the chunks"),
                (dict(cells=(7, 5, 3)), "descends or lies outside")):
            assert raw(**changes) == _lib.ERROR_INVALID_ARGUMENT and message in _lib.last_error(), (message, _lib.last_error())
            assert "pgsd_sph_body_force_device" in _lib.last_error()
            assert list(summary) == [77] * 22, message
            assert untouched(), message
        # the call after them, as it is: correct
        assert raw() == 0
        assert words_equal(np.array(list(summary), np.uint64), want.summary)
        assert np.array_equal(_host(contacts), want.contacts)
        assert bits_equal(_host(outs[0]), want.pressure_acc.ravel()) and bits_equal(_host(outs[1]), want.viscous_acc.ravel())
        # without a pressure chunk the default stands for every row
        assert raw(pressure=None, defaults=[1.0, 0.0, 2.5e4]) == 0
        flat = hoomd.sph_body_force(host, w, TRICLINIC, 0.625, viscosity=0.7, about=about,
                                    **dict(asked, pressure=np.full(len(host), 2.5e4)))
        assert words_equal(np.array(list(summary), np.uint64), flat.summary) and bits_equal(_host(outs[0]), flat.pressure_acc.ravel())
        # a negative viscosity: no viscous term, and the second array stays as it was
        outs[1] = fl._device_from_host(np.full(3 * n, 77.0), f.pipeline_device())
        assert raw(viscosity=-1.0) == 0
        none = hoomd.sph_body_force(host, w, TRICLINIC, 0.625, about=about, **asked)
        assert words_equal(np.array(list(summary), np.uint64), none.summary)
        assert _host(outs[1]).tolist() == [77.0] * (3 * n) and bits_equal(_host(outs[0]), want.pressure_acc.ravel())
        # no target: the summary of nothing, nothing launched; no source: every target dry
        assert raw(n=0) == 0
        assert list(summary) == [0, 0, n_s, 0, 0, 0, 0, NONE, NONE] + [0] * 13
        assert raw(n2=0) == 0
        dry = hoomd.sph_body_force(host, w, TRICLINIC, 0.625, viscosity=0.7, about=about, **dict(asked, fluid_rows=np.arange(0)))
        assert words_equal(np.array(list(summary), np.uint64), dry.summary) and not _host(contacts).any()
        f.wait_read()


def test_what_the_python_layer_refuses_on_the_device(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    with fl.open(path, 'r') as f:
        rows = to_device(f, np.arange(100))
        cell = f.order_rows_by_cell_device(0, name, TRICLINIC, (7, 5, 4), rows, n=100)

        def call(name=name, box=TRICLINIC, h=0.625, cells=(7, 5, 4), **kw):
            return f.sph_body_force_device(0, name, box, h, cells, rows, cell, rows, cell, **kw)

        for kw, message in ((dict(h=0.0), "finite and positive"), (dict(cells=(8, 5, 4)), "narrower"),
                            (dict(kernel='gaussian'), "kernel is one of"), (dict(n_body=101), "fewer entries than n"),
                            (dict(n_fluid=101), "fewer entries than n"), (dict(name='particles/typeid'), "float32 or float64"),
                            (dict(mass=(0, 'particles/mass')), "differ in their number of rows"),
                            (dict(defaults=[1.0, 0.0]), "a mass, a density and a pressure"),
                            (dict(viscosity=-1.0), "viscosity is a finite number"), (dict(about=(0, 0)), "about holds three finite numbers")):
            with pytest.raises(ValueError, match=message):
                call(**kw)
        f.wait_read()


# ---------------------------------------------------------------- through pgsd.hoomd
BODY = {'type': ['wall'], 'density': (950.0, 1060.0)}
FLUID = {'type': ['fluid', 'inlet']}
CELL = hoomd.domain_grid(2, 2, 1)[1]
SELECTIONS = {"types": {}, "domain": {'domain': CELL}}


@pytest.mark.parametrize("selection", sorted(SELECTIONS))
def test_frame_body_force_device_equals_the_host_model(data, selection):
    """about_20000: the triclinic box at 2h = 0.61 (h=None from the uniform slength 0.305), with type selections, a domain,
    return_rows, a viscosity and a point for the torque."""
    path, _ = data
    kwargs = SELECTIONS[selection]
    with hoomd.open(path, 'r') as t:
        for options in (dict(viscosity=0.7, about=(1.0, -2.0, 0.5)), dict(h=0.3125, kernel='cubic_spline', cells=(12, 10, 8))):
            want = t.frame_body_force(0, BODY, FLUID, **options, **kwargs)
            got = t.frame_body_force_device(0, BODY, FLUID, return_rows=True, **options, **kwargs)
            assert equal(got, want, (selection, options))
            if 'h' not in options:
                assert want.h == float(np.float32(0.305)) and any(want.force_viscous) and any(want.torque)
                summary_only = t.frame_body_force_device(0, BODY, FLUID, **options, **kwargs)
                assert summary_only.contacts is None and summary_only.pressure_acc is None
                assert words_equal(summary_only.summary, want.summary) and summary_only.force == want.force
        assert want.h == 0.3125 and want.viscous_acc is None and 0 < got.n < got.n_sources < N and got.wetted > 0
        with pytest.raises(ValueError, match="narrower"):
            t.frame_body_force_device(0, BODY, FLUID, 0.65, cells=(8, 5, 4), **kwargs)
        with pytest.raises(ValueError, match="count twice"):
            t.frame_body_force_device(0, BODY, FLUID, 1.75, **kwargs)
        with pytest.raises(ValueError, match="kernel is one of"):
            t.frame_body_force_device(0, BODY, FLUID, 0.3, kernel='gaussian', **kwargs)
        with pytest.raises(ValueError, match="viscosity is a finite number"):
            t.frame_body_force_device(0, BODY, FLUID, 0.3, viscosity=float('nan'), **kwargs)
        with pytest.raises(ValueError, match="about holds three finite numbers"):
            t.frame_body_force_device(0, BODY, FLUID, 0.3, about=(0, 0, float('inf')), **kwargs)
        with pytest.raises(ValueError, match="both are required"):
            t.frame_body_force_device(0, BODY, None, 0.3, **kwargs)
        with pytest.raises(IndexError):
            t.frame_body_force_device(2, BODY, FLUID, 0.3)


def test_h_none_and_the_defaults_on_the_device(data):
    """Frame 1 stores a slength that is not uniform, and neither typeid, velocity, mass, density nor pressure: every row is
    of type 0, so the wall is empty -- the summary of nothing --, and with the fluid on both sides every A is 0/0, in the
    model and on the GPU alike."""
    path, _ = data
    with hoomd.open(path, 'r') as t:
        with pytest.raises(ValueError, match="slength ranges from 0.30"):
            t.frame_body_force_device(1, BODY, FLUID)
        want = t.frame_body_force(1, {'type': ['wall']}, FLUID, 0.305)
        got = t.frame_body_force_device(1, {'type': ['wall']}, FLUID, 0.305, return_rows=True)
        assert equal(got, want, "no wall") and got.n == 0 and got.n_sources == N1 and got.largest2 is None
        want = t.frame_body_force(1, FLUID, FLUID, 0.305, viscosity=0.5)
        got = t.frame_body_force_device(1, FLUID, FLUID, 0.305, viscosity=0.5, return_rows=True)
        assert equal(got, want, "defaults") and got.n == N1 and got.bad == got.n - got.nowhere and got.force == (0.0, 0.0, 0.0)


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
    got = t.frame_body_force_device(0, {'type': ['wall']}, {'type': ['fluid']}, viscosity=0.7, about=(0, 0, 1), return_rows=True)
    assert isinstance(got.contacts, fl.DeviceBuffer) and got.contacts.shape == (got.n,)
    assert isinstance(got.pressure_acc, fl.DeviceBuffer) and got.pressure_acc.shape == (got.n, 3) and got.viscous_acc.shape == (got.n, 3)
    res = dict((name, getattr(got, name).to_host()) for name in ('rows', 'cell', 'contacts', 'pressure_acc', 'viscous_acc'))
    res['summary'] = got.summary
pickle.dump(res, open(out_path, "wb"))
'''


def test_the_rows_stay_in_device_memory_without_torch(data, tmp_path):
    """return_rows without a tensor library: the three arrays are DeviceBuffers."""
    path, _ = data
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, path, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))
    with hoomd.open(path, 'r') as t:
        want = t.frame_body_force(0, {'type': ['wall']}, {'type': ['fluid']}, viscosity=0.7, about=(0, 0, 1))
    assert words_equal(res['summary'], want.summary) and 0 < want.n < N
    assert np.array_equal(res['rows'], want.rows) and np.array_equal(res['cell'], want.cell)
    assert np.array_equal(res['contacts'], want.contacts)
    for name in ('pressure_acc', 'viscous_acc'):
        assert res[name].shape == getattr(want, name).shape and bits_equal(res[name].ravel(), getattr(want, name).ravel()), name
