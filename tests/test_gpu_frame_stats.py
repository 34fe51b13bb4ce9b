"""Frame statistics on the GPU: pgsd_chunk_stats_device behind pgsd.fl's chunk_stats_device and pgsd.hoomd's
frame_stats_device.  Every result must equal the numpy model pgsd.hoomd.column_stats / frame_stats exactly -- the six
arrays with numpy.array_equal, the sums bit for bit: the order of the sum is part of the definition.  Files are written
through the host path; chunks of other element types and widths are per-particle log chunks."""
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
# one lane, around one wave, around one tile, a ragged many-tile case, and more than 256 tiles: the final kernel's lanes
# add a second tile
SIZES = [1, 63, 64, 65, 4095, 4096, 4097, 70_001, 1_048_577]
LIST_LENGTHS = [0, 1, 63, 64, 65, 4096, 4097, 70_001]
DTYPES = {'f32': np.float32, 'f64': np.float64, 'i32': np.int32, 'u32': np.uint32}
WIDTHS = [1, 3, 4]
TRI = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
QUANTITIES = hoomd.FieldStats.__slots__
DENORMAL = np.float32(2.0 ** -140)
SPECIAL = [np.nan, np.inf, -np.inf, -0.0, DENORMAL]


def wide(rng, n, dtype=np.float32):
    """Normal values scaled over 15 decades: an input whose sum depends on the order (tests/test_stats_model.py)."""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 12, n)).astype(dtype)


def chunk_values(rng, N, M, key):
    dtype = DTYPES[key]
    if key == 'i32':
        a = rng.integers(-2 ** 31, 2 ** 31, size=(N, M), dtype=np.int64).astype(np.int32)
    elif key == 'u32':
        a = rng.integers(0, 2 ** 32, size=(N, M), dtype=np.int64).astype(np.uint32)
    else:
        a = wide(rng, N * M, dtype).reshape(N, M)
        # NaN, +-infinity, -0.0 and a float32 denormal in the first wave, in the last lane of a tile (lane 255 of steps
        # 0 .. 3 and 15) and in the last, partial tile
        spots = [1, 2, 3, 4, 5] + [255, 511, 767, 1023, 4095] + [N - 1, N - 2, N - 3, N - 4, N - 5]
        for i, row in enumerate(spots):
            if N >= 63 and 0 <= row < N:
                a[row, i % M] = SPECIAL[i % 5]
    if key == 'i32' and N > 2:
        a[0, 0], a[N - 1, M - 1] = -2 ** 31, 2 ** 31 - 1
    if key == 'u32' and N > 2:
        a[1, 0] = 2 ** 32 - 1
    return a[:, 0].copy() if M == 1 else a


def _dir(tmp_path_factory, name):
    return "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp(name))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Per N one file of one frame whose log holds a per-particle chunk for every element type and width; the host's
    arrays beside it.  Computed once and left unchanged."""
    d = _dir(tmp_path_factory, "stats")
    out = {}
    for N in SIZES:
        rng = np.random.default_rng(N)
        path = os.path.join(d, "pgsd_stats_%d_%d.gsd" % (os.getpid(), N))
        fr = hoomd.Frame()
        fr.configuration.box = TRI
        fr.particles.N = N
        fr.particles.position = rng.uniform(-3.0, 3.0, size=(N, 3)).astype(np.float32)
        arrays = {}
        for key in DTYPES:
            for M in WIDTHS:
                arrays['%s_%d' % (key, M)] = fr.log['%s_%d' % (key, M)] = chunk_values(rng, N, M, key)
        arrays['position'] = fr.particles.position
        with hoomd.open(path, 'w') as t:
            t.append(fr)
        out[N] = (path, arrays)
    yield out
    for path, _ in out.values():
        os.unlink(path)


def same(got, want, what):
    for q in QUANTITIES:
        g, w = getattr(got, q), getattr(want, q)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, q)
        assert np.array_equal(g, w), (what, q, g.tolist(), w.tolist())
    with np.errstate(invalid='ignore'):
        assert np.array_equal(got.mean, want.mean, equal_nan=True), what
    return True


def norm2_variants(key, M):
    return (False, True) if key in ('f32', 'f64') and M == 3 else (False,)


def to_device(f, rows):
    return fl._device_from_host(np.ascontiguousarray(rows, dtype=np.int32), f.pipeline_device())


# ---------------------------------------------------------------- the dense route
@pytest.mark.parametrize("key", sorted(DTYPES))
@pytest.mark.parametrize("N", SIZES)
def test_the_dense_route_equals_the_model(files, N, key):
    path, arrays = files[N]
    with fl.open(path, 'r') as f:
        for M in WIDTHS:
            name = '%s_%d' % (key, M)
            for norm2 in norm2_variants(key, M):
                got = f.chunk_stats_device(0, 'log/' + name, norm2=norm2)
                assert same(got, hoomd.column_stats(arrays[name], norm2=norm2), (name, norm2))
                assert got.count.tolist() == [N] * (M + norm2)
            f.wait_read()


def test_the_special_rows_are_where_the_cases_need_them(files):
    """What the dense cases rely on: non-finite rows, a negative zero and a denormal in the first wave, in lane 255 and
    in the last tile, and a sum that depends on the order."""
    _, arrays = files[70_001]
    a = arrays['f32_1']
    for rows in ([1, 2, 3, 4, 5], [255, 511, 767, 1023, 4095], [70_000, 69_999, 69_998, 69_997, 69_996]):
        v = a[rows]
        assert np.isnan(v[0]) and v[1] == np.inf and v[2] == -np.inf and v[3] == 0 and np.signbit(v[3]) and v[4] == DENORMAL
    st = hoomd.column_stats(a)
    assert st.nan[0] == 3 and st.inf[0] == 6
    finite = np.where(np.isfinite(a), a, 0).astype(np.float64)
    others = {float(np.sum(finite)), float(np.cumsum(finite)[-1]), float(hoomd.column_stats(finite[::-1].copy()).sum[0])}
    assert float(st.sum[0]) != float(np.sum(finite)) and len(others | {float(st.sum[0])}) >= 3


# ---------------------------------------------------------------- the gathered route
@pytest.fixture(scope="module")
def lists(files):
    """Row lists over the 70 001-row chunks: random with repeats, of every length."""
    rng = np.random.default_rng(99)
    return dict((n, rng.integers(0, 70_001, size=n).astype(np.int32)) for n in LIST_LENGTHS + [1_048_577])


@pytest.mark.parametrize("key", sorted(DTYPES))
@pytest.mark.parametrize("n", LIST_LENGTHS)
def test_a_random_list_with_repeats_equals_the_model(files, lists, n, key):
    path, arrays = files[70_001]
    rows = lists[n]
    with fl.open(path, 'r') as f:
        dev = to_device(f, rows)
        for M in WIDTHS:
            name = '%s_%d' % (key, M)
            for norm2 in norm2_variants(key, M):
                got = f.chunk_stats_device(0, 'log/' + name, rows=dev, norm2=norm2)
                assert same(got, hoomd.column_stats(arrays[name], rows, norm2=norm2), (name, norm2))
            f.wait_read()


def test_a_list_of_many_tiles_with_repeats(files, lists):
    path, arrays = files[70_001]
    rows = lists[1_048_577]
    with fl.open(path, 'r') as f:
        dev = to_device(f, rows)
        for name, norm2 in (('f32_3', True), ('f64_4', False), ('i32_1', False), ('u32_3', False)):
            got = f.chunk_stats_device(0, 'log/' + name, rows=dev, norm2=norm2)
            assert same(got, hoomd.column_stats(arrays[name], rows, norm2=norm2), name)
            f.wait_read()


def test_the_list_of_a_selection(files):
    """An ascending list as a selection returns it, whole and -- through ``n`` -- its first entries."""
    path, arrays = files[70_001]
    lo, hi = -50.0, 2000.0
    with np.errstate(invalid='ignore'):
        want_rows = np.flatnonzero((arrays['f32_1'] >= lo) & (arrays['f32_1'] < hi)).astype(np.int32)
    assert 4097 < len(want_rows) < 70_001
    with fl.open(path, 'r') as f:
        rows, count = f.select_where_device([(0, 'log/f32_1', 0, (lo, hi))])
        assert count == len(want_rows)
        for name, norm2 in (('f32_1', False), ('f32_3', True), ('f64_3', True), ('i32_4', False), ('u32_1', False)):
            got = f.chunk_stats_device(0, 'log/' + name, rows=rows, n=count, norm2=norm2)
            assert same(got, hoomd.column_stats(arrays[name], want_rows, norm2=norm2), name)
            for n in (0, 1, 64, 4097):
                got = f.chunk_stats_device(0, 'log/' + name, rows=rows, n=n, norm2=norm2)
                assert same(got, hoomd.column_stats(arrays[name], want_rows[:n], norm2=norm2), (name, n))
        # the selected values lie in the range
        st = f.chunk_stats_device(0, 'log/f32_1', rows=rows, n=count)
        assert lo <= st.min[0] and st.max[0] < hi and st.nan[0] == st.inf[0] == 0
        f.wait_read()


def test_an_entry_outside_the_chunk_is_refused(files, lists):
    path, arrays = files[4097]
    with fl.open(path, 'r') as f:
        for bad_at, bad in ((0, 4097), (4096, 2 ** 31 - 1), (5000, -1)):
            rows = np.arange(5001, dtype=np.int32) % 4097
            rows[bad_at] = bad
            with pytest.raises(ValueError, match="an entry of the row list lies outside the chunk"):
                f.chunk_stats_device(0, 'log/f32_3', rows=to_device(f, rows), norm2=True)
            # the call after it on the same handle is correct
            rows[bad_at] = 7
            got = f.chunk_stats_device(0, 'log/f32_3', rows=to_device(f, rows), norm2=True)
            assert same(got, hoomd.column_stats(arrays['f32_3'], rows, norm2=True), bad)
            assert same(f.chunk_stats_device(0, 'log/f32_3'), hoomd.column_stats(arrays['f32_3']), bad)
        f.wait_read()


# ---------------------------------------------------------------- staging
def test_a_staged_chunk_is_not_read_again(files):
    N = 70_001
    path, arrays = files[N]
    with hoomd.open(path, 'r') as t:
        f = t.file
        # after a selection over the chunk
        f.device_read_stats(reset=True)
        rows, count = f.select_where_device([(0, 'log/f32_1', 0, (0.0, None))])
        assert f.device_read_stats()["pread_bytes"] == N * 4
        got = f.chunk_stats_device(0, 'log/f32_1', rows=rows, n=count)
        assert f.device_read_stats()["pread_bytes"] == N * 4
        with np.errstate(invalid='ignore'):
            assert same(got, hoomd.column_stats(arrays['f32_1'], np.flatnonzero(arrays['f32_1'] >= 0.0)), 'selection')
        f.wait_read()
        # after a census of the position chunk; two statistics calls of one chunk read it once
        f.device_read_stats(reset=True)
        f.domain_histogram_device(0, 'particles/position', TRI, 64)
        assert f.device_read_stats()["pread_bytes"] == N * 12
        first = f.chunk_stats_device(0, 'particles/position', norm2=True)
        again = f.chunk_stats_device(0, 'particles/position')
        assert f.device_read_stats()["pread_bytes"] == N * 12
        assert same(first, hoomd.column_stats(arrays['position'], norm2=True), 'position')
        assert np.array_equal(first.sum[:3], again.sum)
        f.chunk_stats_device(0, 'log/f64_4')
        f.chunk_stats_device(0, 'log/f64_4')
        assert f.device_read_stats()["pread_bytes"] == N * 12 + N * 32
        f.wait_read()
        # after the wait the chunk is released: the next call reads it again
        f.chunk_stats_device(0, 'log/f64_4')
        assert f.device_read_stats()["pread_bytes"] == N * 12 + 2 * N * 32
        f.wait_read()


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def test_domain_reads_are_unchanged_after_statistics(files):
    path, arrays = files[70_001]
    d = hoomd.domain_grid(2, 2, 2)[3]
    want = hoomd.domain_rows(arrays['position'], TRI, d)
    with hoomd.open(path, 'r') as t:
        before = t.read_frame_device(0, domain=d)
        t.file.chunk_stats_device(0, 'particles/position', norm2=True)
        t.file.wait_read()
        t.frame_stats_device(0, ['position'], domain=d)
        after = t.read_frame_device(0, domain=d)
    for s in (before, after):
        assert np.array_equal(_host(s.tag), want) and s.particles.N == len(want)
        assert _host(s.particles.position).tobytes() == arrays['position'][want].tobytes()


# ---------------------------------------------------------------- through pgsd.hoomd
def _frame(rng, n, step):
    fr = hoomd.Frame()
    fr.configuration.step = step
    fr.configuration.box = TRI
    fr.particles.N = n
    fr.particles.types = ['fluid', 'wall', 'inlet']
    fr.particles.position = rng.uniform(-3.0, 3.0, size=(n, 3)).astype(np.float32)
    fr.particles.velocity = wide(rng, 3 * n).reshape(n, 3)
    fr.particles.density = (1000.0 + 50.0 * rng.standard_normal(n)).astype(np.float32)
    fr.particles.typeid = rng.integers(0, 3, size=n).astype(np.uint32)
    fr.particles.image = rng.integers(-2, 3, size=(n, 3)).astype(np.int32)
    return fr


@pytest.fixture(scope="module")
def trajectory(tmp_path_factory):
    """Two frames of 70 001 particles -- the second elides position, typeid and image, which equal frame 0's -- and a
    file whose one frame has no particle."""
    d = _dir(tmp_path_factory, "stats_traj")
    rng = np.random.default_rng(12)
    n = 70_001
    f0 = _frame(rng, n, 0)
    f0.particles.velocity[[3, 255, n - 1]] = [[np.nan, 1, 1], [np.inf, 0, 0], [1, -np.inf, np.nan]]
    f1 = _frame(rng, n, 10)
    f1.particles.position, f1.particles.typeid, f1.particles.image = (f0.particles.position, f0.particles.typeid,
                                                                       f0.particles.image)
    path, empty = (os.path.join(d, "pgsd_stats_%d_%s.gsd" % (os.getpid(), k)) for k in ("traj", "empty"))
    with hoomd.open(path, 'w') as t:
        t.append(f0)
        t.append(f1)
    none = hoomd.Frame()
    none.configuration.box = TRI
    none.particles.types = ['fluid', 'wall', 'inlet']
    with hoomd.open(empty, 'w') as t:
        t.append(none)
    yield path, empty
    os.unlink(path)
    os.unlink(empty)


FIELDS = ['position', 'velocity', 'density', 'pressure', 'typeid', 'image', 'mass']
WHERE = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
CELL = hoomd.domain_grid(2, 2, 1)[1]
SELECTIONS = {"all": {}, "where": {'where': WHERE}, "domain": {'domain': CELL}, "both": {'where': WHERE, 'domain': CELL}}


@pytest.mark.parametrize("idx", [0, 1])
@pytest.mark.parametrize("selection", sorted(SELECTIONS))
def test_frame_stats_device_equals_the_host_model(trajectory, selection, idx):
    path, _ = trajectory
    kwargs = SELECTIONS[selection]
    with hoomd.open(path, 'r') as t:
        if idx == 1:      # frame 1 elides what equals frame 0's: those statistics are frame 0's rows'
            assert not t.file.chunk_exists(1, 'particles/position') and t.file.chunk_exists(1, 'particles/velocity')
        assert not t.file.chunk_exists(idx, 'particles/pressure') and not t.file.chunk_exists(0, 'particles/pressure')
        want = t.frame_stats(idx, FIELDS, **kwargs)
        t.file.device_read_stats(reset=True)
        got = t.frame_stats_device(idx, FIELDS, **kwargs)
        pread = t.file.device_read_stats()["pread_bytes"]
    assert list(got) == list(want) == FIELDS
    for name in FIELDS:
        assert same(got[name], want[name], (selection, idx, name))
    count = int(want['density'].count[0])
    assert (count == 70_001) if selection == "all" else (0 < count < 70_001)
    # pressure and mass are stored nowhere: the default row, `count` times, and no file byte
    assert want['pressure'].max.tolist() == [0.0] and want['mass'].sum.tolist() == [float(count)]
    # every chunk is read exactly once: a selection's chunks serve their own statistics
    assert pread == 70_001 * (12 + 12 + 4 + 4 + 12)
    if selection == "all" and idx == 0:
        assert got['velocity'].nan.tolist() == [1, 0, 1, 2] and got['velocity'].inf.tolist() == [1, 1, 0, 1]


def test_the_default_fields_and_a_negative_index(trajectory):
    path, _ = trajectory
    with hoomd.open(path, 'r') as t:
        got, want = t.frame_stats_device(-1), t.frame_stats(-1)
        assert list(got) == ['position', 'velocity', 'density', 'pressure', 'energy']
        for name in got:
            assert same(got[name], want[name], name)
        assert got['velocity'].max[3] == np.max(np.sum(t[1].particles.velocity.astype(np.float64) ** 2, axis=1))
        with pytest.raises(IndexError):
            t.frame_stats_device(2)
        with pytest.raises(ValueError, match="not a per-particle attribute"):
            t.frame_stats_device(0, ['speed'])


def test_a_frame_without_particles(trajectory):
    _, empty = trajectory
    with hoomd.open(empty, 'r') as t:
        for kwargs in SELECTIONS.values():
            got, want = t.frame_stats_device(0, FIELDS, **kwargs), t.frame_stats(0, FIELDS, **kwargs)
            for name in FIELDS:
                assert same(got[name], want[name], name)
                assert not got[name].count.any() and np.isnan(got[name].mean).all()
                assert (got[name].min == np.inf).all() and (got[name].max == -np.inf).all() and not got[name].sum.any()


# ---------------------------------------------------------------- refusals
def test_every_refusal_has_its_message_and_leaves_the_handle_usable(files, tmp_path):
    path, arrays = files[4097]
    other = str(tmp_path / "other.gsd")
    with fl.open(other, 'w', application="test", schema="none", schema_version=[1, 0]) as f:
        for name, a in (('u8', np.zeros((9, 1), np.uint8)), ('i16', np.zeros((9, 3), np.int16)),
                        ('u64', np.zeros((9, 1), np.uint64)), ('i64', np.zeros((9, 1), np.int64)),
                        ('f32_5', np.zeros((9, 5), np.float32)), ('f64_7', np.zeros((9, 7), np.float64))):
            f.write_chunk(name, a)
        f.end_frame()
    with fl.open(other, 'r') as f:
        for name in ('u8', 'i16', 'u64', 'i64'):
            with pytest.raises(ValueError, match="float32, float64, int32 or uint32"):
                f.chunk_stats_device(0, name)
        for name in ('f32_5', 'f64_7'):
            with pytest.raises(ValueError, match="1 to 4 columns"):
                f.chunk_stats_device(0, name)
        with pytest.raises(KeyError):
            f.chunk_stats_device(0, 'nothing')
    with fl.open(path, 'r') as f:
        for name in ('i32_3', 'u32_3', 'f32_1', 'f32_4', 'f64_4', 'f64_1'):
            with pytest.raises(ValueError, match="norm2 needs a float chunk of three columns"):
                f.chunk_stats_device(0, 'log/' + name, norm2=True)
        rows = to_device(f, np.arange(10))
        with pytest.raises(ValueError, match="fewer entries than n"):
            f.chunk_stats_device(0, 'log/f32_1', rows=rows, n=11)
        with pytest.raises(ValueError, match="n goes with rows"):
            f.chunk_stats_device(0, 'log/f32_1', n=5)
        with pytest.raises(ValueError, match="32-bit"):
            f.chunk_stats_device(0, 'log/f32_1', rows=fl._device_from_host(np.arange(4, dtype=np.int64), f.pipeline_device()))
        # what no file holds, through the entry point itself: a chunk without columns, 2^32 rows, 2^32 entries
        fn = _lib.lib.pgsd_chunk_stats_device
        fn.restype = ctypes.c_int32
        fn.argtypes = [ctypes.POINTER(_lib.Handle), ctypes.POINTER(_lib.IndexEntry), ctypes.c_void_p, ctypes.c_uint64,
                       ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]
        h = f._h()
        entry = _lib.lib.pgsd_find_chunk(h, 0, b'log/f32_3').contents
        counts, values = (ctypes.c_uint64 * 15)(*([77] * 15)), (ctypes.c_double * 15)(*([77.0] * 15))
        dev = ctypes.c_void_p(rows.data_ptr() if hasattr(rows, 'data_ptr') else rows.ptr)
        for change, n, message in ((dict(M=0), 0, "1 to 4 columns"), (dict(N=2 ** 32), 0, "2^32 rows"),
                                   (dict(), 2 ** 32, "fewer than 2^32 entries"), (dict(type=4), 0, "float32, float64")):
            e = _lib.IndexEntry.from_buffer_copy(entry)
            for k, v in change.items():
                setattr(e, k, v)
            rc = fn(h, ctypes.byref(e), dev if n else None, n, 0, counts, values)
            assert rc == _lib.ERROR_INVALID_ARGUMENT and message in _lib.last_error(), (change, n, _lib.last_error())
            assert list(counts) == [77] * 15 and list(values) == [77.0] * 15        # written on success only
        # the same call as it is: correct, and the handle works as before
        e = _lib.IndexEntry.from_buffer_copy(entry)
        assert fn(h, ctypes.byref(e), None, 0, 1, counts, values) == 0
        want = hoomd.column_stats(arrays['f32_3'], norm2=True)
        assert [counts[3 * c + 1] for c in range(4)] == want.nan.tolist()
        assert [values[3 * c + 2] for c in range(4)] == want.sum.tolist()
        assert same(f.chunk_stats_device(0, 'log/u32_4'), hoomd.column_stats(arrays['u32_4']), 'after')
        f.wait_read()


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
res = {}
with fl.open(path, 'r') as f:
    res["dense"] = f.chunk_stats_device(0, 'log/f32_3', norm2=True)
    rows = fl._device_from_host(np.arange(70000, -1, -7, dtype=np.int32), f.pipeline_device())
    res["listed"] = f.chunk_stats_device(0, 'log/f64_4', rows=rows)
    sel, count = f.select_where_device([(0, 'log/i32_1', 0, (0, None))])
    res["selected"] = f.chunk_stats_device(0, 'log/i32_1', rows=sel, n=count)
    f.wait_read()
with hoomd.open(traj, 'r') as t:
    res["frame"] = t.frame_stats_device(1, ['velocity', 'density', 'mass'], where={'type': ['wall']},
                                        domain=hoomd.domain_grid(2, 1, 1)[0])
res = dict((k, dict((q, getattr(v, q)) for q in hoomd.FieldStats.__slots__) if k != "frame" else
               dict((n, dict((q, getattr(s, q)) for q in hoomd.FieldStats.__slots__)) for n, s in v.items()))
           for k, v in res.items())
pickle.dump(res, open(out_path, "wb"))
'''


def test_statistics_without_torch(files, trajectory, tmp_path):
    path, arrays = files[70_001]
    traj, _ = trajectory
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, path, traj, str(out)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))

    def check(got, want, what):
        for q in QUANTITIES:
            assert np.array_equal(got[q], getattr(want, q)), (what, q)

    check(res["dense"], hoomd.column_stats(arrays['f32_3'], norm2=True), "dense")
    check(res["listed"], hoomd.column_stats(arrays['f64_4'], np.arange(70000, -1, -7)), "listed")
    check(res["selected"], hoomd.column_stats(arrays['i32_1'], np.flatnonzero(arrays['i32_1'] >= 0)), "selected")
    with hoomd.open(traj, 'r') as t:
        want = t.frame_stats(1, ['velocity', 'density', 'mass'], where={'type': ['wall']},
                             domain=hoomd.domain_grid(2, 1, 1)[0])
    for name in want:
        check(res["frame"][name], want[name], name)
