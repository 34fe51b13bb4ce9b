"""The SPH kernel sums on the GPU: pgsd_sph_sums_device behind pgsd.fl's sph_sums_device and pgsd.hoomd's
frame_kernel_sums_device.  Every per-entry array and every summary word must equal the numpy model
pgsd.hoomd.sph_kernel_sums / frame_kernel_sums exactly, the floats bit for bit (tests/test_sph_model.py holds the model
against a plain double loop; a NaN equals a NaN, whose sign and payload IEEE 754 leaves to the processor).  The cases at
the pgsd.fl level read constructed chunks, once with float32 and once with float64 positions, with both kernels, and order
the list on the GPU first, as a caller does."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402
from pgsd import _lib  # noqa: E402
from neighbours_cases import FLAT, TRICLINIC, random_rows  # noqa: E402
from sph_cases import CASES as SHARED_CASES, KERNELS, MUTATIONS, NONE, WIDE, bits_equal, words_equal  # noqa: E402

N = 20_011
N1 = 5_003
TYPES = ['fluid', 'wall', 'inlet']
DTYPES = {'f32': np.float32, 'f64': np.float64}
CASES = dict(SHARED_CASES)         # (and behind them the mutation cases, as chunks of the same file)
for _k, (_name, (_switch, _case)) in enumerate(sorted(MUTATIONS.items())):
    _kw = dict(_case)
    CASES['mutation_%02d' % _k] = (np.asarray(_kw.pop('position'), np.float64), _kw.pop('mass', None), _kw.pop('density', None), _kw)
MUTATION_CASE = dict((name, 'mutation_%02d' % k) for k, name in enumerate(sorted(MUTATIONS)))


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
    """One file of two frames.  Frame 0: 20 011 particles with types, masses, densities, a uniform slength of 0.305 and
    random positions in the triclinic box (the pgsd.hoomd level), and every case's positions as a float32 and a float64
    log chunk with its mass and density columns in both element types.  Frame 1: 5 003 other particles with a slength that
    is not uniform and nothing else stored (another N: frame 0's chunks do not stand in).  The host's arrays beside it."""
    path = os.path.join(_dir(tmp_path_factory, "sph"), "pgsd_sph_%d.gsd" % os.getpid())
    rng = np.random.default_rng(N)
    fr = hoomd.Frame()
    fr.configuration.box = TRICLINIC
    fr.particles.N = N
    fr.particles.types = TYPES
    fr.particles.position = _lost(random_rows(7, N, TRICLINIC, np.float32))
    fr.particles.typeid = rng.integers(0, len(TYPES), size=N).astype(np.uint32)
    fr.particles.density = (1000.0 + 50.0 * rng.standard_normal(N)).astype(np.float32)
    fr.particles.mass = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
    fr.particles.slength = np.full(N, 0.305, np.float32)
    arrays = {}
    for name, (p, mass, density, _) in CASES.items():
        for key, dt in DTYPES.items():
            arrays[chunk(name, key)] = fr.log['%s_%s' % (name, key)] = np.ascontiguousarray(p.astype(dt))
            for column, values in (('mass', mass), ('density', density)):
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
    """The kernel's KernelSums (per-entry arrays in GPU memory) against the model's."""
    assert words_equal(got.summary, want.summary), (what, got, want, got.summary, want.summary)
    assert got.grid == want.grid and got.kernel == want.kernel and got.volume == want.volume and got.h == want.h, what
    for name in ('n', 'nowhere', 'not_finite', 'surface', 'deviation_at', 'deviation_row'):
        assert getattr(got, name) == getattr(want, name), (what, name)
    if got.number is not None:
        assert np.array_equal(_host(got.rows), want.rows) and np.array_equal(_host(got.cell), want.cell), what
        assert bits_equal(_host(got.number), want.number), (what, 'number')
        assert bits_equal(_host(got.density), want.density), (what, 'density')
        assert (got.shepard is None) == (want.shepard is None), what
        if want.shepard is not None:
            assert bits_equal(_host(got.shepard), want.shepard), (what, 'shepard')
    return True


def sums(f, arrays, name, key, kernel, rows=None, return_rows=True, columns=None, **kw):
    """Order the list on the GPU, run the pass; the model over the arrays the chunks hold beside it.  ``columns``: the
    element type key of the mass and density chunks (the positions' by default)."""
    columns = key if columns is None else columns
    host = arrays[chunk(name, key)]
    mass, density = arrays.get(chunk(name + '_mass', columns)), arrays.get(chunk(name + '_density', columns))
    box, h, dims = kw['box'], kw['h'], kw.get('dimensions', 3)
    want = hoomd.sph_kernel_sums(host, mass=mass, density=density, rows=rows, kernel=kernel, **kw)
    every = np.arange(len(host)) if rows is None else np.asarray(rows)
    d_rows = to_device(f, every)
    d_cell = f.order_rows_by_cell_device(0, chunk(name, key), box, want.grid, d_rows, n=len(every), dimensions=dims)
    got = f.sph_sums_device(0, chunk(name, key), box, h, want.grid, d_rows, d_cell, n=len(every),
                            mass=None if mass is None else (0, chunk(name + '_mass', columns)),
                            density=None if density is None else (0, chunk(name + '_density', columns)),
                            dimensions=dims, kernel=kernel, surface_below=kw.get('surface_below'), return_rows=return_rows)
    return got, want


# ---------------------------------------------------------------- constructed cases
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("key", sorted(DTYPES))
@pytest.mark.parametrize("name", [c for c in sorted(CASES) if not c.startswith('mutation')])
def test_a_case_equals_the_model(data, name, key, kernel):
    path, arrays = data
    kw = CASES[name][3]
    with fl.open(path, 'r') as f:
        got, want = sums(f, arrays, name, key, kernel, **kw)
        assert equal(got, want, (name, key, kernel))
        f.wait_read()
    assert want.n == len(arrays[chunk(name, key)])
    if name == 'all_nowhere':
        assert got.nowhere == 100 and got.density_min == np.inf and got.deviation is None
        assert not _host(got.number).any() and not np.signbit(_host(got.number)).any()
    if name == 'one_cell_65':
        assert got.shepard is None and got.shepard_min is None and got.deviation is None and got.surface is None
    if name == 'clump_700':
        assert got.number_max > 100 * got.sigma                     # a sum of some hundred terms, longer than a workgroup
    if name == 'sparse_64cubed':
        assert got.grid == (64, 64, 64) and got.number_min == got.sigma      # an entry alone: its own w = 1
    if name == 'flat':
        assert got.dimensions == 2 and got.sigma == hoomd.sph_sigma(kernel, 0.375, 2)
    if name == 'three_cells':
        assert got.nowhere > 0
    if name == 'boundary':
        number = dict(zip(_host(got.rows).tolist(), _host(got.number).tolist()))
        assert number[0] == got.sigma and number[2] == number[3] == 2.0 * got.sigma   # 2h itself not counted; w = 1 at 0
        assert got.shepard_max == np.inf and got.not_finite == 0
        if kernel == 'cubic_spline':
            assert number[4] == 1.25 * got.sigma                     # q == 1 exactly
            assert (number[6] != number[4] and number[8] != number[4]) == (key == 'f64')     # an ulp either side
    if name == 'mass_density':
        assert got.surface > 0 and np.isnan(_host(got.shepard)).any() and np.isinf(_host(got.shepard)).any()


@pytest.mark.parametrize("columns", sorted(DTYPES))
@pytest.mark.parametrize("key", sorted(DTYPES))
def test_mass_and_density_chunks_of_either_element_type(data, key, columns):
    """float32 and float64 mass and density chunks beside positions of either type; a row with density 0 and one with a
    NaN density."""
    path, arrays = data
    with fl.open(path, 'r') as f:
        for kernel in KERNELS:
            got, want = sums(f, arrays, 'mass_density', key, kernel, columns=columns, **CASES['mass_density'][3])
            assert equal(got, want, (key, columns, kernel)) and got.volume
        f.wait_read()


@pytest.mark.parametrize("key", sorted(DTYPES))
def test_lists_of_0_1_63_64_65_entries_repeats_and_any_order(data, key):
    """n in {0, 1, 63, 64, 65}; a list in descending order with rows listed twice (two entries at distance 0)."""
    path, arrays = data
    kw = CASES['three_cells'][3]
    with fl.open(path, 'r') as f:
        for n in (0, 1, 63, 64, 65):
            got, want = sums(f, arrays, 'three_cells', key, 'wendland_c2', rows=np.arange(100, 100 + n), **kw)
            assert equal(got, want, (key, n)) and got.n == n
        assert got.number_min >= got.sigma
        got, want = sums(f, arrays, 'three_cells', key, 'cubic_spline', rows=np.arange(0), **kw)
        assert equal(got, want, (key, 'nothing')) and got.n == 0 and got.density_min == np.inf and got.deviation is None
        rows = np.concatenate([np.arange(400, 0, -1), [7, 7, 400, 12]])
        for kernel in KERNELS:
            got, want = sums(f, arrays, 'three_cells', key, kernel, rows=rows, **kw)
            assert equal(got, want, (key, kernel)) and got.n == 404
        f.wait_read()


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_the_kernel_on_every_mutation_case(data, mutation):
    """The case on which the mutated loop differs from the model (tests/test_sph_model.py): the kernel equals the model
    there, so it does not hold the mutation."""
    path, arrays = data
    name = MUTATION_CASE[mutation]
    kw = dict(CASES[name][3])
    kernels = [kw.pop('kernel')] if 'kernel' in kw else KERNELS
    key = 'f64' if MUTATIONS[mutation][1]['position'].dtype == np.float64 else 'f32'
    with fl.open(path, 'r') as f:
        for kernel in kernels:
            got, want = sums(f, arrays, name, key, kernel, **kw)
            assert equal(got, want, (mutation, kernel))
        f.wait_read()


# ---------------------------------------------------------------- staging, the per-entry outputs
def test_a_second_call_is_served_from_the_staged_rows_and_return_rows(data):
    path, arrays = data
    name, kw = 'triclinic_754', CASES['triclinic_754'][3]
    n = len(arrays[chunk(name, 'f32')])
    with fl.open(path, 'r') as f:
        f.device_read_stats(reset=True)
        got, want = sums(f, arrays, name, 'f32', 'wendland_c2', **kw)       # position by the ordering, then two columns
        assert f.device_read_stats()["pread_bytes"] == n * (12 + 4 + 4) and equal(got, want, "first")
        got, _ = sums(f, arrays, name, 'f32', 'wendland_c2', return_rows=False, **kw)
        assert f.device_read_stats()["pread_bytes"] == n * (12 + 4 + 4) and equal(got, want, "second")
        assert got.rows is None and got.cell is None and got.number is None and got.density is None and got.shepard is None
        f.wait_read()
        f.device_read_stats(reset=True)
        got, _ = sums(f, arrays, name, 'f32', 'cubic_spline', **kw)
        assert f.device_read_stats()["pread_bytes"] == n * (12 + 4 + 4)     # released by wait_read: read again
        assert _host(got.number).dtype == np.float64 and _host(got.shepard).dtype == np.float64
        f.wait_read()


def test_one_chunk_given_as_mass_and_as_density(data):
    """One stored chunk named twice in one call -- as the mass and as the density --: the staging takes the file range
    once and both slots share its address.  'flat' is the smallest case whose list spans two workgroups."""
    path, arrays = data
    name, kw = chunk('flat', 'f32'), CASES['flat'][3]
    column = chunk('flat_mass', 'f32')
    host, m = arrays[name], arrays[column]
    n = len(host)
    assert n > 256
    want = hoomd.sph_kernel_sums(host, mass=m, density=m, kernel='wendland_c2', **kw)
    with fl.open(path, 'r') as f:
        d_rows = to_device(f, np.arange(n))
        d_cell = f.order_rows_by_cell_device(0, name, kw['box'], want.grid, d_rows, n=n, dimensions=2)
        f.device_read_stats(reset=True)
        got = f.sph_sums_device(0, name, kw['box'], kw['h'], want.grid, d_rows, d_cell, n=n, mass=(0, column),
                                density=(0, column), dimensions=2, kernel='wendland_c2', return_rows=True)
        assert f.device_read_stats()["pread_bytes"] == n * 4           # the column once; the position by the ordering
        assert equal(got, want, "mass is density") and got.volume
        f.wait_read()


# ---------------------------------------------------------------- refusals
def test_what_the_python_layers_refuse(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    with fl.open(path, 'r') as f:
        rows = to_device(f, np.arange(100))
        cell = f.order_rows_by_cell_device(0, name, TRICLINIC, (7, 5, 4), rows, n=100)

        def call(name=name, box=TRICLINIC, h=0.625, cells=(7, 5, 4), rows=rows, cell=cell, **kw):
            return f.sph_sums_device(0, name, box, h, cells, rows, cell, **kw)

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
                            (dict(defaults=[1.0]), "a mass and a density"),
                            (dict(box=WIDE, h=0.025, cells=(1024, 1024, 2)), "2\\^20 cells")):
            with pytest.raises(ValueError, match=message):
                call(**kw)
        with pytest.raises(KeyError):
            call(name='log/nothing')
        with pytest.raises(KeyError):
            call(density=(0, 'log/nothing'))
        f.wait_read()


def test_every_refusal_has_its_message_and_leaves_the_outputs_untouched(data):
    path, arrays = data
    name = chunk('triclinic_754', 'f32')
    host = arrays[name]
    mass, density = arrays[chunk('triclinic_754_mass', 'f32')], arrays[chunk('triclinic_754_density', 'f32')]
    n = 500
    want = hoomd.sph_kernel_sums(host, TRICLINIC, 0.625, mass=mass, density=density, rows=np.arange(n), cells=(7, 5, 4),
                                 surface_below=0.004)
    fn = _lib.lib.pgsd_sph_sums_device
    fn.restype = ctypes.c_int32
    D, U, E = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_lib.IndexEntry)
    fn.argtypes = [ctypes.POINTER(_lib.Handle), E, E, E, D, D, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, U,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p,
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
        summary = (ctypes.c_uint64 * 13)(*([77] * 13))
        outs = [fl._device_from_host(np.full(n, 77.0), f.pipeline_device()) for _ in range(3)]
        good = dict(entry=entry_of(name), mass=entry_of(chunk('triclinic_754_mass', 'f32')),
                    density=entry_of(chunk('triclinic_754_density', 'f32')), defaults=[1.0, float('nan')],
                    vectors=hoomd.box_vectors(np.asarray(TRICLINIC, np.float32)), h=0.625, kernel=0, dims=3, cells=(7, 5, 4),
                    rows=d_rows, cell=d_cell, n=n, surface=0.004)

        def raw(**changes):
            a = dict(good, **changes)
            return fn(h, ctypes.byref(a['entry']), None if a['mass'] is None else ctypes.byref(a['mass']),
                      None if a['density'] is None else ctypes.byref(a['density']), (ctypes.c_double * 2)(*a['defaults']),
                      (ctypes.c_double * 6)(*a['vectors']), a['h'], a['kernel'], a['dims'], (ctypes.c_uint32 * 3)(*a['cells']),
                      _ptr(a['rows']), _ptr(a['cell']), a['n'], a['surface'], _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                      summary)

        huge = entry_of(name)
        huge.N = 2 ** 32
        flat_vectors = hoomd.box_vectors(np.asarray(FLAT, np.float32))
        wide_vectors = hoomd.box_vectors(np.asarray([2000, 2000, 2000, 0, 0, 0], np.float32))
        for changes, message in (
                (dict(entry=entry_of('particles/typeid')), "float32 or float64"), (dict(entry=entry_of('particles/mass')), "3 columns"),
                (dict(entry=huge), "2^32 rows"), (dict(n=2 ** 32), "2^32 entries"), (dict(dims=4), "dimensions is 2 or 3"),
                (dict(h=0.0), "finite and positive"), (dict(h=-1.0), "finite and positive"),
                (dict(h=float('inf')), "finite and positive"), (dict(h=float('nan')), "finite and positive"),
                (dict(kernel=2), "the kernel is 0"), (dict(mass=entry_of('particles/typeid')), "the mass chunk holds float32 or float64"),
                (dict(density=entry_of(name)), "the density chunk has 1 column"),
                (dict(mass=entry_of('particles/mass')), "the mass chunk and the position chunk differ"),
                (dict(density=entry_of('particles/density')), "the density chunk and the position chunk differ"),
                (dict(vectors=[10, 0, 6, 0, 0, 0]), "box lengths"), (dict(cells=(0, 5, 4)), "1 to 1024 cells"),
                (dict(cells=(1025, 5, 4)), "1 to 1024 cells"), (dict(cells=(8, 5, 4)), "narrower than the support"),
                (dict(cells=(7, 6, 4)), "narrower than the support"), (dict(cells=(7, 5, 5)), "narrower than the support"),
                (dict(dims=2, vectors=flat_vectors, cells=(2, 3, 2)), "one z cell"),
                (dict(h=1.51, cells=(1, 1, 1)), "count twice"), (dict(vectors=wide_vectors, h=0.5, cells=(1024, 1024, 2)), "2^20 cells"),
                (dict(cell=d_desc), "descends or lies outside"), (dict(cell=d_outc), "descends or lies outside"),
                (dict(rows=d_outr), "outside the chunks"), (dict(cells=(7, 5, 3)), "descends or lies outside")):
            assert raw(**changes) == _lib.ERROR_INVALID_ARGUMENT and message in _lib.last_error(), (message, _lib.last_error())
            assert list(summary) == [77] * 13, message
            for out in outs:
                assert _host(out).tolist() == [77.0] * n, message
        # the same call as it is: correct; without a volume the third array stays; n == 0 is the summary of no entry
        assert raw() == 0
        assert words_equal(np.array(list(summary), np.uint64), want.summary)
        assert bits_equal(_host(outs[0]), want.number) and bits_equal(_host(outs[1]), want.density)
        assert bits_equal(_host(outs[2]), want.shepard)
        assert raw(density=None) == 0
        none = hoomd.sph_kernel_sums(host, TRICLINIC, 0.625, mass=mass, rows=np.arange(n), cells=(7, 5, 4))
        assert words_equal(np.array(list(summary), np.uint64), none.summary) and bits_equal(_host(outs[2]), want.shepard)
        assert raw(n=0) == 0
        inf = np.array([np.inf, -np.inf] * 3 + [0.0]).view(np.uint64).tolist()
        assert list(summary) == [0] * 4 + [NONE] * 2 + inf
        f.wait_read()


# ---------------------------------------------------------------- through pgsd.hoomd
WHERE = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
CELL = hoomd.domain_grid(2, 2, 1)[1]
SELECTIONS = {"all": {}, "where": {'where': WHERE}, "domain": {'domain': CELL}, "both": {'where': WHERE, 'domain': CELL}}


@pytest.mark.parametrize("selection", sorted(SELECTIONS))
def test_frame_kernel_sums_device_equals_the_host_model(data, selection):
    """about_20000: the triclinic box at 2h = 0.61 (h=None from the uniform slength 0.305), with where, domain,
    surface_below and return_rows."""
    path, _ = data
    kwargs = SELECTIONS[selection]
    with hoomd.open(path, 'r') as t:
        for options in (dict(surface_below=0.03), dict(h=0.3125, kernel='cubic_spline', cells=(12, 10, 8))):
            want = t.frame_kernel_sums(0, **options, **kwargs)
            got = t.frame_kernel_sums_device(0, return_rows=True, **options, **kwargs)
            assert equal(got, want, (selection, options))
        assert want.h == 0.3125 and t.frame_kernel_sums(0).h == float(np.float32(0.305))
        summary_only = t.frame_kernel_sums_device(0, surface_below=0.03, **kwargs)
        assert summary_only.number is None and words_equal(summary_only.summary,
                                                           t.frame_kernel_sums(0, surface_below=0.03, **kwargs).summary)
        assert summary_only.surface is not None and summary_only.deviation is not None
        if selection == "all":
            assert got.n == N and got.nowhere > 0
        else:
            assert 0 < got.n < N
        with pytest.raises(ValueError, match="narrower"):
            t.frame_kernel_sums_device(0, 0.65, cells=(8, 5, 4), **kwargs)
        with pytest.raises(ValueError, match="count twice"):
            t.frame_kernel_sums_device(0, 1.75, **kwargs)
        with pytest.raises(ValueError, match="kernel is one of"):
            t.frame_kernel_sums_device(0, 0.3, kernel='gaussian', **kwargs)
        with pytest.raises(IndexError):
            t.frame_kernel_sums_device(2, 0.3)


def test_h_none_on_the_device(data):
    """Frame 1 stores a slength that is not uniform, and neither typeid, mass nor density: every row is of type 0 and the
    defaults 1.0 and 0.0 stand for mass and density, so every volume is infinite, in the model and on the GPU alike."""
    path, _ = data
    with hoomd.open(path, 'r') as t:
        with pytest.raises(ValueError, match="slength ranges from 0.30"):
            t.frame_kernel_sums_device(1)
        with pytest.raises(ValueError, match="slength ranges from 0.30"):
            t.frame_kernel_sums(1)
        want = t.frame_kernel_sums(1, 0.305, where={'type': ['fluid']})
        got = t.frame_kernel_sums_device(1, 0.305, where={'type': ['fluid']}, return_rows=True)
        assert equal(got, want, "defaults") and got.volume and got.shepard_min == np.inf and got.n == N1
