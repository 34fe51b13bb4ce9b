"""Conservation sums on the GPU: pgsd_frame_moments_device behind pgsd.fl's frame_moments_device and pgsd.hoomd's
frame_moments_device.  Every result must equal the numpy model pgsd.hoomd.particle_moments / frame_moments exactly --
the counters with numpy.array_equal, the nine sums per type bit for bit: the order of the sums is part of the definition
(tests/test_moments_model.py checks the model itself).  Files are written through the host path; the float64 inputs and
the other type layouts are per-particle log chunks."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one lane, around one wave, around one tile, a ragged many-tile case, and 257 tiles: a lane of the final kernel adds a
# second tile
SIZES = [1, 63, 64, 65, 4095, 4096, 4097, 70_001, 1_048_577]
LIST_LENGTHS = [0, 1, 63, 64, 65, 4096, 4097, 70_001]
TRI = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
NAMES = ('count', 'bad', 'mass', 'momentum', 'kinetic', 'internal', 'first_moment')
DENORMAL = np.float32(2.0 ** -140)
INPUTS = ('mass', 'velocity', 'energy', 'position')
# the chunks of the five inputs per element type; the type layouts
CHUNKS = {'f32': ['particles/typeid', 'particles/mass', 'particles/velocity', 'particles/energy', 'particles/position'],
          'f64': ['particles/typeid', 'log/m64', 'log/v64', 'log/e64', 'log/x64']}
# a default row whose values float32 holds exactly and that is nothing like the schema's
ROW = [0.375, 3.0, -7.0, 1.5 * 2.0 ** 30, -2.5, 1.5, 2.5, -0.3125]


def wide(rng, n, dtype=np.float32):
    """Normal values scaled over 15 decades: an input whose sum depends on the order (tests/test_moments_model.py)."""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 12, n)).astype(dtype)


def _dir(tmp_path_factory, name):
    return "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp(name))


def floats(rng, N, dtype):
    """mass, velocity, energy, position with NaN, infinities, an infinite velocity on a zero mass, -0.0 and a float32
    denormal in the first wave, in lane 255 (steps 0, 1 and 15) and in the last, partial tile; float64: a velocity
    whose square overflows while the momentum does not."""
    a = dict(mass=np.abs(wide(rng, N, dtype)) + dtype(0.5), velocity=wide(rng, 3 * N, dtype).reshape(N, 3),
             energy=wide(rng, N, dtype), position=rng.uniform(-3.0, 3.0, size=(N, 3)).astype(dtype))
    if N >= 63:
        big = 1e200 if dtype is np.float64 else np.inf
        spots = [(1, 'mass', np.nan), (2, 'velocity', np.inf), (2, 'mass', 0.0), (3, 'velocity', big), (4, 'mass', -0.0),
                 (5, 'mass', DENORMAL), (6, 'energy', -np.inf), (255, 'velocity', np.nan), (511, 'energy', np.inf),
                 (4095, 'mass', np.inf), (4095 + 256, 'position', np.nan), (N - 1, 'position', np.nan),
                 (N - 2, 'velocity', -np.inf), (N - 3, 'mass', np.nan), (N - 4, 'mass', -0.0), (N - 5, 'energy', np.nan)]
        for row, name, value in spots:
            if 0 <= row < N:
                if a[name].ndim == 2:
                    a[name][row, row % 3] = value
                else:
                    a[name][row] = value
    return a


def run_layout(N):
    """Contiguous runs whose edges fall at entries 63 / 64 / 65 and 4095 / 4096 / 4097, then long runs."""
    t = np.zeros(N, np.uint32)
    for k, edge in enumerate([63, 64, 65, 4095, 4096, 4097, 20_000, 45_000]):
        t[edge:] = (k + 1) % 4
    return t


def sparse_layout(N):
    """Type 1 lives in tile 3 only (and there in one wave's lanes), type 2 on every second entry of tile 2 and on one
    entry of every second tile, type 3 nowhere."""
    t = np.zeros(N, np.uint32)
    t[8192::8192] = 2
    t[2 * 4096:3 * 4096:2] = 2
    t[3 * 4096 + 64:3 * 4096 + 128] = 1
    return t


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Per N one file of one frame: the five particle chunks (float32, typeid (k + 1) % 5), the float inputs again as float64
    log chunks, and type layouts as log chunks; the host's arrays beside it.  Computed once and left unchanged."""
    d = _dir(tmp_path_factory, "moments")
    out = {}
    for N in SIZES:
        rng = np.random.default_rng(N)
        path = os.path.join(d, "pgsd_moments_%d_%d.gsd" % (os.getpid(), N))
        fr = hoomd.Frame()
        fr.configuration.box = TRI
        fr.particles.N = N
        fr.particles.types = ['a', 'b', 'c', 'd', 'e']
        arrays = {}
        a32, a64 = floats(rng, N, np.float32), floats(rng, N, np.float64)
        arrays['particles/typeid'] = fr.particles.typeid = ((np.arange(N) + 1) % 5).astype(np.uint32)   # (never all default)
        for name in INPUTS:
            setattr(fr.particles, name, a32[name])
            arrays['particles/' + name] = a32[name]
        for short, name in (('m64', 'mass'), ('v64', 'velocity'), ('e64', 'energy'), ('x64', 'position')):
            arrays['log/' + short] = fr.log[short] = a64[name]
        signed = (np.arange(N) % 5).astype(np.int32)
        signed[::7] = -1 - signed[::7]            # negative ids: of no type
        signed[N // 2] = -2 ** 31
        arrays['log/tid_i32'] = fr.log['tid_i32'] = signed
        if N == 70_001:
            arrays['log/tid_runs'] = fr.log['tid_runs'] = run_layout(N)
            arrays['log/tid_sparse'] = fr.log['tid_sparse'] = sparse_layout(N)
        with hoomd.open(path, 'w') as t:
            t.append(fr)
        out[N] = (path, arrays)
    yield out
    for path, _ in out.values():
        os.unlink(path)


def same(got, want, what=None):
    """Integers equal, sums bit for bit."""
    assert got.other == want.other, (what, got.other, want.other)
    for name in NAMES:
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, name, g.tolist(), w.tolist())
        else:
            assert np.array_equal(g, w), (what, name, g.tolist(), w.tolist())
    return True


def spec(names):
    return [None if name is None else (0, name) for name in names]


def model(arrays, names, defaults=None, **kwargs):
    """particle_moments for the chunk names (None: the default row) of a device call."""
    d = [1, 0, 0, 0, 0, 0, 0, 0] if defaults is None else defaults
    rows = dict(mass=d[0], velocity=d[1:4], energy=d[4], position=d[5:8])
    given = dict((k, rows[k] if name is None else arrays[name]) for k, name in zip(INPUTS, names[1:]))
    tid = None if names[0] is None else arrays[names[0]]
    return hoomd.particle_moments(typeid=tid, **given, **kwargs)


def to_device(f, rows):
    return fl._device_from_host(np.ascontiguousarray(rows, dtype=np.int32), f.pipeline_device())


# ---------------------------------------------------------------- the dense route
def groups_of(N, key):
    """(type0, n_types) per case: every group size and both type0 at the small sizes, two groups at the largest."""
    if N == 1_048_577:
        return [(0, 4), (3, 2)]
    return [(0, 1), (0, 2), (0, 4), (3, 1), (3, 2), (3, 4), (1, 3)]


@pytest.mark.parametrize("key", ['f32', 'f64'])
@pytest.mark.parametrize("N", SIZES)
def test_the_dense_route_equals_the_model(files, N, key):
    path, arrays = files[N]
    names = CHUNKS[key]
    with fl.open(path, 'r') as f:
        for type0, n_types in groups_of(N, key):
            got = f.frame_moments_device(spec(names), type0=type0, n_types=n_types)
            assert same(got, model(arrays, names, type0=type0, n_types=n_types), (type0, n_types))
            assert int(got.count.sum()) + got.other == N
        if N != 1_048_577:
            none = [None] + names[1:]
            assert same(f.frame_moments_device(spec(none)), model(arrays, none), 'no typeid')
        f.wait_read()


def test_the_special_rows_are_where_the_cases_need_them(files):
    """What the dense cases rely on: values that are not finite in the first wave, in lane 255 and in the last tile, an
    infinite velocity on a zero mass, a kinetic term that overflows alone, and sums that depend on the order."""
    _, arrays = files[70_001]
    m, v = arrays['particles/mass'], arrays['particles/velocity']
    assert np.isnan(m[1]) and m[2] == 0 and np.isinf(v[2, 2]) and np.signbit(m[4]) and m[5] == DENORMAL
    assert np.isnan(v[255, 0]) and np.isinf(arrays['particles/energy'][511]) and np.isinf(m[4095])
    assert np.isnan(arrays['particles/position'][70_000]).any() and np.isinf(v[69_999]).any()
    v64 = arrays['log/v64']
    assert v64[3, 0] == 1e200 and np.isfinite(arrays['log/m64'][3] * 1e200)
    want = model(arrays, CHUNKS['f32'], n_types=4)
    assert want.bad.sum() >= 8 and want.bad[3] >= 1            # (row 2: NaN momentum on a mass that is summed)
    differs = 0
    for t in range(4):
        for a in range(3):
            with np.errstate(invalid='ignore'):
                q = m.astype(np.float64) * v[:, a].astype(np.float64)
            seq = np.where(np.isfinite(q) & (arrays['particles/typeid'] == t), q, 0.0)
            assert want.momentum[t, a] == hoomd._ordered_sum(seq)
            differs += want.momentum[t, a] != np.sum(seq)
    assert differs >= 6


# ---------------------------------------------------------------- the gathered route
@pytest.fixture(scope="module")
def lists(files):
    """Row lists over the 70 001-row chunks: random with repeats, of every length."""
    rng = np.random.default_rng(99)
    return dict((n, rng.integers(0, 70_001, size=n).astype(np.int32)) for n in LIST_LENGTHS + [1_048_577])


@pytest.mark.parametrize("key", ['f32', 'f64'])
@pytest.mark.parametrize("n", LIST_LENGTHS)
def test_a_random_list_with_repeats_equals_the_model(files, lists, n, key):
    path, arrays = files[70_001]
    names, rows = CHUNKS[key], lists[n]
    with fl.open(path, 'r') as f:
        dev = to_device(f, rows)
        for type0, n_types in ((0, 4), (3, 2), (2, 1)):
            got = f.frame_moments_device(spec(names), type0=type0, n_types=n_types, rows=dev)
            assert same(got, model(arrays, names, type0=type0, n_types=n_types, rows=rows), (type0, n_types))
        none = [None] + names[1:]
        assert same(f.frame_moments_device(spec(none), rows=dev), model(arrays, none, rows=rows), 'no typeid')
        f.wait_read()


def test_a_list_of_many_tiles_with_repeats(files, lists):
    path, arrays = files[70_001]
    rows = lists[1_048_577]
    with fl.open(path, 'r') as f:
        dev = to_device(f, rows)
        got = f.frame_moments_device(spec(CHUNKS['f64']), type0=1, n_types=4, rows=dev)
        assert same(got, model(arrays, CHUNKS['f64'], type0=1, n_types=4, rows=rows))
        f.wait_read()


def test_the_list_of_a_selection(files):
    """An ascending list as a selection returns it, whole and -- through ``n`` -- its first entries."""
    path, arrays = files[70_001]
    with np.errstate(invalid='ignore'):
        want_rows = np.flatnonzero(arrays['particles/energy'] >= 0.0).astype(np.int32)
    assert 4097 < len(want_rows) < 70_001
    with fl.open(path, 'r') as f:
        rows, count = f.select_where_device([(0, 'particles/energy', 0, (0.0, None))])
        assert count == len(want_rows)
        for key in ('f32', 'f64'):
            got = f.frame_moments_device(spec(CHUNKS[key]), n_types=4, rows=rows, n=count)
            assert same(got, model(arrays, CHUNKS[key], n_types=4, rows=want_rows), key)
            for n in (0, 1, 64, 4097):
                got = f.frame_moments_device(spec(CHUNKS[key]), type0=1, n_types=2, rows=rows, n=n)
                assert same(got, model(arrays, CHUNKS[key], type0=1, n_types=2, rows=want_rows[:n]), (key, n))
        f.wait_read()


# ---------------------------------------------------------------- type layouts
@pytest.mark.parametrize("layout", ['log/tid_runs', 'log/tid_sparse', 'log/tid_i32'])
def test_type_layouts(files, lists, layout):
    """Runs with edges around a wave and a tile; a type absent from whole tiles and one absent from the chunk (a wave
    that holds none of a type skips its adds); int32 ids, the negative ones of no type."""
    path, arrays = files[70_001]
    names = [layout] + CHUNKS['f32'][1:]
    with fl.open(path, 'r') as f:
        dev = to_device(f, lists[4097])
        for type0, n_types in ((0, 4), (0, 2), (1, 1), (3, 1), (2, 4)):
            got = f.frame_moments_device(spec(names), type0=type0, n_types=n_types)
            want = model(arrays, names, type0=type0, n_types=n_types)
            assert same(got, want, (type0, n_types))
            got = f.frame_moments_device(spec(names), type0=type0, n_types=n_types, rows=dev)
            assert same(got, model(arrays, names, type0=type0, n_types=n_types, rows=lists[4097]), (type0, n_types, 'list'))
        full = f.frame_moments_device(spec(names), n_types=4)
        f.wait_read()
    if layout == 'log/tid_sparse':
        assert full.count.tolist() == np.bincount(arrays[layout], minlength=4).tolist() and full.other == 0
        assert full.count[1] == 64 and full.count[2] == 2048 + 7 and full.count[3] == 0
        assert full.sums[3].view(np.uint64).tolist() == [0] * 9           # +0.0 for a type with no entry
    elif layout == 'log/tid_i32':
        assert full.other > 70_001 // 7 and (arrays[layout] < 0).sum() == 70_001 // 7 + 1


# ---------------------------------------------------------------- chunk presence
@pytest.mark.parametrize("key", ['f32', 'f64'])
def test_every_chunk_may_be_stored_nowhere(files, lists, key):
    path, arrays = files[4097]
    rows = lists[4097] % 4097
    with fl.open(path, 'r') as f:
        dev = to_device(f, rows)
        for absent in ([1], [2], [3], [4], [0], [1, 2, 3, 4], [0, 2, 4], [0, 1, 2, 3, 4]):
            names = [None if i in absent else name for i, name in enumerate(CHUNKS[key])]
            n_types = 1 if 0 in absent else 4
            kw = dict(N=4097) if len(absent) == 5 else {}
            for defaults in (ROW, None):
                got = f.frame_moments_device(spec(names), defaults, n_types=n_types, rows=dev)
                assert same(got, model(arrays, names, defaults, n_types=n_types, rows=rows, **kw), (absent, 'list'))
                got = f.frame_moments_device(spec(names), defaults, n_types=n_types, n=4097 if len(absent) == 5 else None)
                assert same(got, model(arrays, names, defaults, n_types=n_types, **kw), absent)
        f.wait_read()
    assert got.mass.tolist() == [4097.0] and not got.momentum.any()       # (the schema's defaults, no chunk at all)


# ---------------------------------------------------------------- refusals
def test_an_entry_outside_the_chunks_is_refused(files):
    path, arrays = files[4097]
    names = CHUNKS['f32']
    with fl.open(path, 'r') as f:
        for bad_at, bad in ((0, 4097), (4096, 2 ** 31 - 1), (5000, -1)):
            rows = np.arange(5001, dtype=np.int32) % 4097
            rows[bad_at] = bad
            with pytest.raises(ValueError, match="an entry of the row list lies outside the chunks"):
                f.frame_moments_device(spec(names), n_types=4, rows=to_device(f, rows))
            # the call after it on the same handle is correct
            rows[bad_at] = 7
            got = f.frame_moments_device(spec(names), n_types=4, rows=to_device(f, rows))
            assert same(got, model(arrays, names, n_types=4, rows=rows), bad)
            assert same(f.frame_moments_device(spec(names), n_types=2), model(arrays, names, n_types=2), bad)
        f.wait_read()


def test_every_refusal_has_its_message_and_leaves_the_handle_usable(files, tmp_path):
    path, arrays = files[4097]
    other = str(tmp_path / "other.gsd")
    with fl.open(other, 'w', application="test", schema="none", schema_version=[1, 0]) as f:
        for name, a in (('tid', np.zeros((9, 1), np.uint32)), ('tid_f', np.zeros((9, 1), np.float32)),
                        ('tid_u64', np.zeros((9, 1), np.uint64)), ('tid_2', np.zeros((9, 2), np.uint32)),
                        ('m', np.ones((9, 1), np.float32)), ('m64', np.ones((9, 1), np.float64)),
                        ('m_i', np.ones((9, 1), np.int32)), ('m_8', np.ones((8, 1), np.float32)),
                        ('v', np.ones((9, 3), np.float32)), ('v64', np.ones((9, 3), np.float64)),
                        ('v_4', np.ones((9, 4), np.float32)), ('x_1', np.ones((9, 1), np.float32))):
            f.write_chunk(name, a)
        f.end_frame()
    with fl.open(other, 'r') as f:
        def call(names, **kw):
            return f.frame_moments_device(spec(names), **kw)
        for names, message in ((['tid_f', 'm', 'v', None, None], "typeid chunk holds uint32 or int32"),
                               (['tid_u64', 'm', 'v', None, None], "typeid chunk holds uint32 or int32"),
                               (['tid_2', 'm', 'v', None, None], "typeid chunk has 1 column"),
                               (['tid', 'm_i', 'v', None, None], "mass chunk holds float32 or float64"),
                               (['tid', 'm', 'tid', None, None], "velocity chunk holds float32 or float64"),
                               (['tid', 'm64', 'v', None, None], "not mixed"),
                               (['tid', 'm', 'v', 'm64', None], "not mixed"),
                               (['tid', 'm', 'v64', None, 'v'], "not mixed"),
                               (['tid', 'v', 'v', None, None], "mass chunk has 1 column"),
                               (['tid', 'm', 'v_4', None, None], "velocity chunk has 3 columns"),
                               (['tid', 'm', 'm', None, None], "velocity chunk has 3 columns"),
                               (['tid', 'm', 'v', 'v', None], "energy chunk has 1 column"),
                               (['tid', 'm', 'v', None, 'x_1'], "position chunk has 3 columns"),
                               (['tid', 'm_8', 'v', None, None], "differ in their number of rows"),
                               (['tid', None, 'v', 'm_8', None], "differ in their number of rows")):
            with pytest.raises(ValueError, match=message):
                call(names)
        for n_types in (0, 5, 2 ** 32 - 1):
            with pytest.raises(ValueError, match="1 to 4 types"):
                call(['tid', 'm', 'v', None, None], n_types=n_types)
        with pytest.raises(ValueError, match="n_types must be 1"):
            call([None, 'm', 'v', None, None], n_types=2)
        with pytest.raises(KeyError):
            call(['tid', 'nothing', 'v', None, None])
        with pytest.raises(ValueError, match="typeid, mass, velocity, energy, position"):
            call(['tid', 'm', 'v', None])
        with pytest.raises(ValueError, match="defaults holds"):
            call(['tid', 'm', 'v', None, None], defaults=[1.0, 2.0])
        with pytest.raises(ValueError, match="n goes with rows"):
            call(['tid', 'm', 'v', None, None], n=5)
        with pytest.raises(ValueError, match="n says how many"):
            call([None] * 5)
        rows = to_device(f, np.arange(9))
        with pytest.raises(ValueError, match="fewer entries than n"):
            call(['tid', 'm', 'v', None, None], rows=rows, n=10)
        with pytest.raises(ValueError, match="32-bit"):
            call(['tid', 'm', 'v', None, None], rows=fl._device_from_host(np.arange(4, dtype=np.int64), f.pipeline_device()))
        assert call(['tid', 'm', 'v', None, None]).kinetic.tolist() == [13.5]          # the handle works as before
        assert call([None] * 5, n=0).count.tolist() == [0]
        f.wait_read()
    with fl.open(path, 'r') as f:
        # what no file holds, through the entry point itself: 2^32 rows, 2^32 entries; the outputs stay untouched
        fn = _lib.lib.pgsd_frame_moments_device
        fn.restype = ctypes.c_int32
        E = ctypes.POINTER(_lib.IndexEntry)
        fn.argtypes = [ctypes.POINTER(_lib.Handle), E, E, E, E, E, ctypes.POINTER(ctypes.c_double), ctypes.c_uint32,
                       ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                       ctypes.POINTER(ctypes.c_double)]
        h = f._h()
        entries = [_lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(h, 0, name.encode()).contents)
                   for name in CHUNKS['f32']]
        defaults = (ctypes.c_double * 8)(1, 0, 0, 0, 0, 0, 0, 0)
        counts, sums = (ctypes.c_uint64 * 9)(*([77] * 9)), (ctypes.c_double * 36)(*([77.0] * 36))
        rows = to_device(f, np.array([0, 1, 4097, 2]))
        dev = ctypes.c_void_p(rows.data_ptr() if hasattr(rows, 'data_ptr') else rows.ptr)

        def raw(entries, n_types=4, rows=None, n=0):
            return fn(h, *[ctypes.byref(e) if e is not None else None for e in entries], defaults, 0, n_types, rows, n,
                      counts, sums)

        huge = [_lib.IndexEntry.from_buffer_copy(e) for e in entries]
        for e in huge:
            e.N = 2 ** 32
        for args, message in ((dict(entries=huge), "2^32 rows"), (dict(entries=entries, rows=dev, n=2 ** 32), "2^32 entries"),
                              (dict(entries=[None] * 5, n_types=1, n=2 ** 32), "2^32 entries"),
                              (dict(entries=entries, rows=dev, n=4), "outside the chunks"),
                              (dict(entries=entries, n_types=5), "1 to 4 types")):
            assert raw(**args) == _lib.ERROR_INVALID_ARGUMENT and message in _lib.last_error(), (message, _lib.last_error())
            assert list(counts) == [77] * 9 and list(sums) == [77.0] * 36        # written on success only
        # the same call as it is: correct
        assert raw(entries) == 0
        want = model(arrays, CHUNKS['f32'], n_types=4)
        assert [counts[2 * t] for t in range(4)] == want.count.tolist() and counts[8] == want.other
        assert [counts[2 * t + 1] for t in range(4)] == want.bad.tolist()
        assert np.array_equal(np.array(list(sums)).reshape(4, 9).view(np.uint64), want.sums.view(np.uint64))
        f.wait_read()


# ---------------------------------------------------------------- staging
def test_staged_chunks_are_not_read_again(files):
    N = 70_001
    path, arrays = files[N]
    names = CHUNKS['f32']
    with hoomd.open(path, 'r') as t:
        f = t.file
        # two calls read every chunk once
        f.device_read_stats(reset=True)
        f.frame_moments_device(spec(names), n_types=4)
        assert f.device_read_stats()["pread_bytes"] == N * 36
        got = f.frame_moments_device(spec(names), type0=4, n_types=1)
        assert f.device_read_stats()["pread_bytes"] == N * 36
        assert same(got, model(arrays, names, type0=4, n_types=1))
        f.wait_read()
        # after a selection over typeid and energy inside a domain, and statistics of the velocity: only the mass is read
        f.device_read_stats(reset=True)
        cell = hoomd.domain_grid(2, 1, 1)[0]
        rows, count = f.select_where_device([(0, 'particles/typeid', 0, [0, 2]), (0, 'particles/energy', 0, (None, 5.0))],
                                            domain=(0, 'particles/position', cell), box=TRI)
        f.chunk_stats_device(0, 'particles/velocity', norm2=True)
        before = f.device_read_stats()["pread_bytes"]
        assert before == N * 32
        got = f.frame_moments_device(spec(names), n_types=4, rows=rows, n=count)
        assert f.device_read_stats()["pread_bytes"] == before + N * 4
        where = hoomd.where_rows({'typeid': arrays['particles/typeid'], 'energy': arrays['particles/energy']},
                                 {'typeid': [0, 2], 'energy': (None, 5.0)})
        want_rows = np.intersect1d(where, hoomd.domain_rows(arrays['particles/position'], TRI, cell))
        assert count == len(want_rows) and same(got, model(arrays, names, n_types=4, rows=want_rows))
        f.wait_read()
        # after the wait the chunks are released: the next call reads them again
        f.frame_moments_device(spec(names), n_types=4)
        assert f.device_read_stats()["pread_bytes"] == before + N * 4 + N * 36
        f.wait_read()


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def test_statistics_and_domain_reads_are_unchanged_around_a_moments_call(files):
    path, arrays = files[70_001]
    d = hoomd.domain_grid(2, 2, 2)[3]
    want_rows = hoomd.domain_rows(arrays['particles/position'], TRI, d)
    with hoomd.open(path, 'r') as t:
        stats_before = t.frame_stats_device(0, ['velocity', 'mass', 'typeid'], domain=d)
        before = t.read_frame_device(0, domain=d)
        t.frame_moments_device(0, domain=d)
        t.file.frame_moments_device(spec(CHUNKS['f64']), n_types=1)
        t.file.wait_read()
        stats_after = t.frame_stats_device(0, ['velocity', 'mass', 'typeid'], domain=d)
        after = t.read_frame_device(0, domain=d)
        want = t.frame_stats(0, ['velocity', 'mass', 'typeid'], domain=d)
    for s in (before, after):
        assert np.array_equal(_host(s.tag), want_rows) and s.particles.N == len(want_rows)
        assert _host(s.particles.velocity).tobytes() == arrays['particles/velocity'][want_rows].tobytes()
    for name in want:
        for q in hoomd.FieldStats.__slots__:
            for st in (stats_before, stats_after):
                assert np.array_equal(getattr(st[name], q), getattr(want[name], q)), (name, q)


# ---------------------------------------------------------------- through pgsd.hoomd
TYPES6 = ['fluid', 'wall', 'inlet', 'outlet', 'gate', 'probe']


def _frame(rng, n, step, types, dimensions=3):
    fr = hoomd.Frame()
    fr.configuration.step = step
    fr.configuration.box = TRI if dimensions == 3 else np.array([4.0, 4.0, 1.0, 0.5, 0.0, 0.0], np.float32)
    fr.configuration.dimensions = dimensions
    fr.particles.N = n
    fr.particles.types = types
    fr.particles.position = rng.uniform(-3.0, 3.0, size=(n, 3)).astype(np.float32)
    if dimensions == 2:
        fr.particles.position[:, 2] = 0.0
    fr.particles.velocity = wide(rng, 3 * n).reshape(n, 3)
    fr.particles.mass = rng.uniform(0.5, 2.0, size=n).astype(np.float32)
    fr.particles.density = (1000.0 + 50.0 * rng.standard_normal(n)).astype(np.float32)
    fr.particles.typeid = rng.integers(0, len(types), size=n).astype(np.uint32)
    return fr


@pytest.fixture(scope="module")
def trajectories(tmp_path_factory):
    """traj: two frames of 70 001 particles of three types -- the second elides position, typeid and mass, which equal
    frame 0's; energy is stored nowhere.  six: one frame of six types with energy.  flat: a 2-D frame.  empty: a frame
    of no particle.  bare: particles with nothing but a velocity (no typeid, no mass, no position)."""
    d = _dir(tmp_path_factory, "moments_traj")
    rng = np.random.default_rng(12)
    n = 70_001
    paths = dict((k, os.path.join(d, "pgsd_moments_%d_%s.gsd" % (os.getpid(), k)))
                 for k in ("traj", "six", "flat", "empty", "bare"))
    f0 = _frame(rng, n, 0, TYPES6[:3])
    f0.particles.velocity[[3, 255, n - 1]] = [[np.nan, 1, 1], [np.inf, 0, 0], [1, -np.inf, np.nan]]
    f1 = _frame(rng, n, 10, TYPES6[:3])
    f1.particles.position, f1.particles.typeid, f1.particles.mass = (f0.particles.position, f0.particles.typeid,
                                                                      f0.particles.mass)
    with hoomd.open(paths["traj"], 'w') as t:
        t.append(f0)
        t.append(f1)
    six = _frame(rng, 20_011, 0, TYPES6)
    six.particles.energy = wide(rng, 20_011)
    with hoomd.open(paths["six"], 'w') as t:
        t.append(six)
    with hoomd.open(paths["flat"], 'w') as t:
        t.append(_frame(rng, 9001, 0, TYPES6[:3], dimensions=2))
    none = hoomd.Frame()
    none.configuration.box = TRI
    none.particles.types = TYPES6[:3]
    with hoomd.open(paths["empty"], 'w') as t:
        t.append(none)
    bare = hoomd.Frame()
    bare.configuration.box = TRI
    bare.particles.N = 5003
    bare.particles.types = TYPES6[:2]
    bare.particles.velocity = wide(rng, 3 * 5003).reshape(5003, 3)
    with hoomd.open(paths["bare"], 'w') as t:
        t.append(bare)
    yield paths
    for path in paths.values():
        os.unlink(path)


WHERE = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
CELL = hoomd.domain_grid(2, 2, 1)[1]
SELECTIONS = {"all": {}, "where": {'where': WHERE}, "domain": {'domain': CELL}, "both": {'where': WHERE, 'domain': CELL}}


@pytest.mark.parametrize("which", ["traj0", "traj1", "six", "flat"])
@pytest.mark.parametrize("selection", sorted(SELECTIONS))
def test_frame_moments_device_equals_the_host_model(trajectories, selection, which):
    path, idx = (trajectories["traj"], int(which[4:])) if which.startswith("traj") else (trajectories[which], 0)
    kwargs = SELECTIONS[selection]
    with hoomd.open(path, 'r') as t:
        if which == "traj1":      # frame 1 elides what equals frame 0's; the energy is stored nowhere
            assert not t.file.chunk_exists(1, 'particles/position') and not t.file.chunk_exists(1, 'particles/mass')
            assert t.file.chunk_exists(1, 'particles/velocity') and not t.file.chunk_exists(0, 'particles/energy')
        for options in (dict(), dict(by_type=False), dict(centre=False)):
            want = t.frame_moments(idx, **options, **kwargs)
            t.file.device_read_stats(reset=True)
            got = t.frame_moments_device(idx, **options, **kwargs)
            pread = t.file.device_read_stats()["pread_bytes"]
            assert same(got, want, (which, selection, options))
            n = t.file.read_chunk(0, 'particles/N')[0]
            if which.startswith("traj"):
                # every chunk that takes part is read exactly once, whatever the number of passes
                used = 4 + 12 + (4 if options.get('by_type', True) or 'where' in kwargs else 0)
                used += 12 if options.get('centre', True) or 'domain' in kwargs else 0
                assert pread == n * (used + (4 if 'where' in kwargs else 0)), (selection, options)
        full = t.frame_moments_device(idx, **kwargs)
    T = 6 if which == "six" else 3
    assert full.count.shape == (T,) and full.momentum.shape == (T, 3) and full.other == 0
    assert (int(full.count.sum()) == n) if selection == "all" else (0 < int(full.count.sum()) < n)
    if 'where' in kwargs:
        assert full.count[1] == 0 and full.sums[1].view(np.uint64).tolist() == [0] * 9
    if which == "traj0" and selection == "all":
        assert full.bad.sum() == 3 and not full.internal.any()


def test_a_negative_index_and_an_index_outside(trajectories):
    with hoomd.open(trajectories["traj"], 'r') as t:
        assert same(t.frame_moments_device(-1), t.frame_moments(1))
        with pytest.raises(IndexError):
            t.frame_moments_device(2)


def test_frames_without_particles_and_without_chunks(trajectories):
    with hoomd.open(trajectories["empty"], 'r') as t:
        for kwargs in SELECTIONS.values():
            got = t.frame_moments_device(0, **kwargs)
            assert same(got, t.frame_moments(0, **kwargs))
            assert got.count.tolist() == [0, 0, 0] and not got.sums.any() and np.isnan(got.centre_of_mass).all()
    with hoomd.open(trajectories["bare"], 'r') as t:
        for kwargs in ({}, {'domain': CELL}, {'where': {'type': ['fluid']}}, {'where': {'type': ['wall']}}):
            for options in (dict(), dict(by_type=False)):
                t.file.device_read_stats(reset=True)
                got = t.frame_moments_device(0, **options, **kwargs)
                assert t.file.device_read_stats()["pread_bytes"] in (0, 5003 * 12)
                assert same(got, t.frame_moments(0, **options, **kwargs), (kwargs, options))
        assert t.frame_moments_device(0).count.tolist() == [5003, 0]


# ---------------------------------------------------------------- without a tensor library
CHILD = r'''
import os, pickle, sys
sys.modules["torch"] = None                    # `import torch` raises ImportError from here on
root, path, traj, out_path = sys.argv[1:5]
sys.path[:0] = [os.path.join(root, "pgsd-sph_amd"), os.path.join(root, "tests")]
import numpy as np
import pgsd.fl as fl
import pgsd.hoomd as hoomd
from pgsd import _lib
assert _lib._torch is None
F32 = [(0, 'particles/' + n) for n in ('typeid', 'mass', 'velocity', 'energy', 'position')]
F64 = [(0, 'particles/typeid')] + [(0, 'log/' + n) for n in ('m64', 'v64', 'e64', 'x64')]
res = {}
with fl.open(path, 'r') as f:
    res["dense"] = f.frame_moments_device(F32, n_types=4)
    rows = fl._device_from_host(np.arange(70000, -1, -7, dtype=np.int32), f.pipeline_device())
    res["listed"] = f.frame_moments_device(F64, type0=3, n_types=2, rows=rows)
    sel, count = f.select_where_device([(0, 'particles/typeid', 0, [1, 4])])
    res["selected"] = f.frame_moments_device([None] + F32[1:], [1, 0, 0, 0, 0, 0, 0, 0], rows=sel, n=count)
    f.wait_read()
with hoomd.open(traj, 'r') as t:
    res["frame"] = t.frame_moments_device(1, where={'type': ['wall']}, domain=hoomd.domain_grid(2, 1, 1)[0])
res = dict((k, dict((q, getattr(v, q)) for q in hoomd.Moments.__slots__)) for k, v in res.items())
pickle.dump(res, open(out_path, "wb"))
'''


def test_moments_without_torch(files, trajectories, tmp_path):
    path, arrays = files[70_001]
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, path, trajectories["traj"], str(out)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))

    def check(got, want, what):
        assert same(hoomd.Moments(**got), want, what)

    check(res["dense"], model(arrays, CHUNKS['f32'], n_types=4), "dense")
    check(res["listed"], model(arrays, CHUNKS['f64'], type0=3, n_types=2, rows=np.arange(70000, -1, -7)), "listed")
    sel = np.flatnonzero(np.isin(arrays['particles/typeid'], [1, 4]))
    check(res["selected"], model(arrays, [None] + CHUNKS['f32'][1:], rows=sel), "selected")
    with hoomd.open(trajectories["traj"], 'r') as t:
        check(res["frame"], t.frame_moments(1, where={'type': ['wall']}, domain=hoomd.domain_grid(2, 1, 1)[0]), "frame")
