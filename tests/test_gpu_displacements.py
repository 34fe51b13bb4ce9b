"""Frame displacements on the GPU: pgsd_frame_displacements_device behind pgsd.fl's frame_displacements_device and
pgsd.hoomd's frame_displacements_device.  Every result must equal the numpy model pgsd.hoomd.particle_displacements /
frame_displacements exactly -- the counters and the largest entry with numpy.array_equal, the four sums and the largest
value per type bit for bit: the order of the sums is part of the definition (tests/test_displacement_model.py checks the
model itself).  Files are written through the host path; frame b's rows, the float64 inputs and the other type layouts
are per-particle log chunks."""
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
TRI_B = np.array([5.0, 3.0, 2.5, -0.25, 0.125, 0.375], np.float32)
VA, VB = hoomd.box_vectors(TRI), hoomd.box_vectors(TRI_B)
NAMES = ('count', 'bad', 'largest_entry', 'drift', 'square', 'largest')
# position a, image a, position b, image b, typeid per element type
CHUNKS = {'f32': ['particles/position', 'particles/image', 'log/pb', 'log/ib', 'particles/typeid'],
          'f64': ['log/pa64', 'particles/image', 'log/pb64', 'log/ib', 'particles/typeid']}


def wide(rng, shape, dtype=np.float32):
    """Normal values scaled over many decades: an input whose sum depends on the order."""
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 9, shape)).astype(dtype)


def _dir(tmp_path_factory, name):
    return "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp(name))


def positions(rng, N, dtype):
    """Both positions, with NaN, infinities, -0.0 and (float64) a move whose square overflows in the first wave, in lane
    255 (steps 0, 1 and 15) and in the last, partial tile."""
    pa = rng.uniform(-2.0, 2.0, (N, 3)).astype(dtype)
    pb = (pa + wide(rng, (N, 3), dtype)).astype(dtype)
    if N >= 63:
        big = 1e200 if dtype is np.float64 else np.inf
        for row, which, value in ((1, pb, np.nan), (2, pb, np.inf), (3, pb, big), (4, pa, -0.0), (6, pa, -np.inf),
                                  (255, pb, np.nan), (511, pa, np.inf), (4095, pb, np.inf), (4095 + 256, pa, np.nan),
                                  (N - 1, pb, np.nan), (N - 2, pa, -np.inf), (N - 3, pb, big), (N - 4, pb, -0.0)):
            if 0 <= row < N:
                which[row, row % 3] = value
        pb[4] = pa[4]
    return pa, pb


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


# ties for the maximum: the entries that hold the largest move, per chunk (the smallest must win)
TIES = {'log/tie_lane': [5 + 256, 5 + 512, 9 + 256], 'log/tie_lanes': [5, 9, 40], 'log/tie_waves': [200, 70, 255],
        'log/tie_tiles': [4096 * 7 + 1, 4096 * 2 + 5, 4096 * 2 + 300]}
TIE_FAR = [1_048_576, 4000, 4096 * 200]       # tiles 256, 0 and 200: lane 0 of the final walk holds tiles 0 and 256


def tie_chunk(N, entries):
    p = np.zeros((N, 3), np.float32)
    p[::3, 1] = 0.5
    p[entries, 0] = 7.0
    p[entries, 1] = 0.0
    return p


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Per N one file of one frame: position and image of frame a as particle chunks, those of frame b as log chunks,
    typeid (k + 1) % 5, both positions again as float64, type layouts and the tie chunks; the host's arrays beside it.
    Computed once and left unchanged."""
    d = _dir(tmp_path_factory, "displacements")
    out = {}
    for N in SIZES:
        rng = np.random.default_rng(N)
        path = os.path.join(d, "pgsd_displacements_%d_%d.gsd" % (os.getpid(), N))
        fr = hoomd.Frame()
        fr.configuration.box = TRI
        fr.particles.N = N
        fr.particles.types = ['a', 'b', 'c', 'd', 'e']
        arrays = {}
        pa, pb = positions(rng, N, np.float32)
        pa64, pb64 = positions(rng, N, np.float64)
        ia = rng.integers(-3, 4, (N, 3)).astype(np.int32)
        ia[::11] = 0
        ia[N // 2] = [1000, -1000, 1000]
        ib = (ia + rng.integers(-1, 2, (N, 3))).astype(np.int32)
        arrays['particles/typeid'] = fr.particles.typeid = ((np.arange(N) + 1) % 5).astype(np.uint32)
        arrays['particles/position'] = fr.particles.position = pa
        arrays['particles/image'] = fr.particles.image = ia
        for name, a in (('pb', pb), ('ib', ib), ('pa64', pa64), ('pb64', pb64)):
            arrays['log/' + name] = fr.log[name] = a
        signed = (np.arange(N) % 5).astype(np.int32)
        signed[::7] = -1 - signed[::7]            # negative ids: of no type
        signed[N // 2] = -2 ** 31
        arrays['log/tid_i32'] = fr.log['tid_i32'] = signed
        if N == 70_001:
            arrays['log/tid_runs'] = fr.log['tid_runs'] = run_layout(N)
            arrays['log/tid_sparse'] = fr.log['tid_sparse'] = sparse_layout(N)
            for name, entries in TIES.items():
                arrays[name] = fr.log[name[4:]] = tie_chunk(N, entries)
        if N == 1_048_577:
            arrays['log/tie_far'] = fr.log['tie_far'] = tie_chunk(N, TIE_FAR)
        if N >= 70_001:
            arrays['log/zero'] = fr.log['zero'] = np.zeros((N, 3), np.float32)
        with hoomd.open(path, 'w') as t:
            t.append(fr)
        out[N] = (path, arrays)
    yield out
    for path, _ in out.values():
        os.unlink(path)


def same(got, want, what=None):
    """Integers equal, values bit for bit."""
    assert got.other == want.other, (what, got.other, want.other)
    for name in NAMES:
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, name, g.tolist(), w.tolist())
        else:
            assert np.array_equal(g, w), (what, name, g.tolist(), w.tolist())
    return True


def same_rows(got, want):
    """Per-entry displacements: a NaN where the model has one, every other value bit for bit, the sign of a zero included.
    (Which NaN an invalid operation returns -- its sign and payload -- belongs to the processor, not to IEEE 754: the host
    returns the negative quiet NaN for inf - inf, the GPU the positive one.)"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))
    return True


def spec(names):
    return [None if name is None else (0, name) for name in names]


def model(arrays, names, va=VA, vb=VB, **kwargs):
    """particle_displacements for the chunk names (None: stored nowhere) of a device call."""
    pa, ia, pb, ib, tid = [None if name is None else arrays[name] for name in names]
    return hoomd.particle_displacements(pa, pb, ia, ib, va, vb, typeid=tid, **kwargs)


def vectors(arrays, names, va=VA, vb=VB, **kwargs):
    pa, ia, pb, ib, _ = [None if name is None else arrays[name] for name in names]
    return hoomd.displacement_vectors(pa, pb, ia, ib, va, vb, **kwargs)


def to_device(f, rows):
    return fl._device_from_host(np.ascontiguousarray(rows, dtype=np.int32), f.pipeline_device())


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


# ---------------------------------------------------------------- the dense route
def groups_of(N):
    """(type0, n_types) per case: every group size and type0 0 to 3 at the small sizes, two groups at the largest."""
    if N == 1_048_577:
        return [(0, 4), (3, 2)]
    return [(0, 1), (0, 2), (0, 4), (1, 3), (2, 2), (3, 1), (3, 4), (1, 4)]


@pytest.mark.parametrize("key", ['f32', 'f64'])
@pytest.mark.parametrize("N", SIZES)
def test_the_dense_route_equals_the_model(files, N, key):
    path, arrays = files[N]
    names = CHUNKS[key]
    with fl.open(path, 'r') as f:
        for type0, n_types in groups_of(N):
            got = f.frame_displacements_device(spec(names), VA, VB, type0=type0, n_types=n_types)
            assert same(got, model(arrays, names, type0=type0, n_types=n_types), (type0, n_types))
            assert int(got.count.sum()) + got.other == N
        if N != 1_048_577:
            none = names[:4] + [None]
            assert same(f.frame_displacements_device(spec(none), VA, VB), model(arrays, none), 'no typeid')
        f.wait_read()


def test_the_special_rows_are_where_the_cases_need_them(files):
    """What the dense cases rely on: values that are not finite in the first wave, in lane 255 and in the last tile, a
    square that overflows alone, -0.0, and sums that depend on the order."""
    _, arrays = files[70_001]
    pa, pb = arrays['particles/position'], arrays['log/pb']
    assert np.isnan(pb[1, 1]) and np.isinf(pb[2, 2]) and np.isnan(pb[255, 0]) and np.isinf(pb[4095, 0])
    assert np.isnan(pb[70_000]).any() and np.isinf(pa[69_999]).any() and np.isinf(pa[511]).any()
    assert arrays['log/pb64'][3, 0] == 1e200 and arrays['log/pb64'][69_998, 69_998 % 3] == 1e200
    want = model(arrays, CHUNKS['f64'], n_types=4)
    assert want.bad.sum() >= 8 and np.isinf(want.largest).any()
    d = vectors(arrays, CHUNKS['f32'])
    tid = arrays['particles/typeid']
    want = model(arrays, CHUNKS['f32'], n_types=4)
    differs = 0
    for t in range(4):
        for a in range(3):
            seq = np.where(np.isfinite(d[:, a]) & (tid == t), d[:, a], 0.0)
            assert want.drift[t, a] == hoomd._ordered_sum(seq)
            differs += want.drift[t, a] != np.sum(seq)
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
            got = f.frame_displacements_device(spec(names), VA, VB, type0=type0, n_types=n_types, rows=dev)
            assert same(got, model(arrays, names, type0=type0, n_types=n_types, rows=rows), (type0, n_types))
        none = names[:4] + [None]
        assert same(f.frame_displacements_device(spec(none), VA, VB, rows=dev), model(arrays, none, rows=rows), 'no typeid')
        f.wait_read()


def test_a_list_of_many_tiles_with_repeats(files, lists):
    path, arrays = files[70_001]
    rows = lists[1_048_577]
    with fl.open(path, 'r') as f:
        dev = to_device(f, rows)
        got = f.frame_displacements_device(spec(CHUNKS['f64']), VA, VB, type0=1, n_types=4, rows=dev)
        assert same(got, model(arrays, CHUNKS['f64'], type0=1, n_types=4, rows=rows))
        f.wait_read()


def test_the_list_of_a_selection(files):
    """An ascending list as a selection returns it, whole and -- through ``n`` -- its first entries."""
    path, arrays = files[70_001]
    want_rows = np.flatnonzero(np.isin(arrays['particles/typeid'], [1, 4])).astype(np.int32)
    with fl.open(path, 'r') as f:
        rows, count = f.select_where_device([(0, 'particles/typeid', 0, [1, 4])])
        assert count == len(want_rows) and 4097 < count < 70_001
        for key in ('f32', 'f64'):
            got = f.frame_displacements_device(spec(CHUNKS[key]), VA, VB, n_types=4, rows=rows, n=count)
            assert same(got, model(arrays, CHUNKS[key], n_types=4, rows=want_rows), key)
            for n in (0, 1, 64, 4097):
                got = f.frame_displacements_device(spec(CHUNKS[key]), VA, VB, type0=1, n_types=2, rows=rows, n=n)
                assert same(got, model(arrays, CHUNKS[key], type0=1, n_types=2, rows=want_rows[:n]), (key, n))
        f.wait_read()


# ---------------------------------------------------------------- type layouts
@pytest.mark.parametrize("layout", ['log/tid_runs', 'log/tid_sparse', 'log/tid_i32'])
def test_type_layouts(files, lists, layout):
    """Runs with edges around a wave and a tile; a type absent from whole tiles and one absent from the chunk (a wave
    that holds none of a type skips it); int32 ids, the negative ones of no type."""
    path, arrays = files[70_001]
    names = CHUNKS['f32'][:4] + [layout]
    with fl.open(path, 'r') as f:
        dev = to_device(f, lists[4097])
        for type0, n_types in ((0, 4), (0, 2), (1, 1), (3, 1), (2, 4), (1, 3)):
            got = f.frame_displacements_device(spec(names), VA, VB, type0=type0, n_types=n_types)
            assert same(got, model(arrays, names, type0=type0, n_types=n_types), (type0, n_types))
            got = f.frame_displacements_device(spec(names), VA, VB, type0=type0, n_types=n_types, rows=dev)
            assert same(got, model(arrays, names, type0=type0, n_types=n_types, rows=lists[4097]), (type0, n_types, 'list'))
        full = f.frame_displacements_device(spec(names), VA, VB, n_types=4)
        f.wait_read()
    if layout == 'log/tid_sparse':
        assert full.count.tolist() == np.bincount(arrays[layout], minlength=4).tolist() and full.other == 0
        assert full.count[1] == 64 and full.count[3] == 0 and full.largest_entry[3] == -1 and full.largest[3] == -np.inf
        assert full.sums[3, :4].view(np.uint64).tolist() == [0] * 4           # +0.0 for a type with no entry
        assert 3 * 4096 + 64 <= full.largest_entry[1] < 3 * 4096 + 128
    elif layout == 'log/tid_i32':
        assert full.other > 70_001 // 7 and (arrays[layout] < 0).sum() == 70_001 // 7 + 1


# ---------------------------------------------------------------- images, the minimum image, boxes
@pytest.mark.parametrize("key", ['f32', 'f64'])
def test_each_image_may_be_stored_nowhere(files, lists, key):
    path, arrays = files[4097]
    rows = lists[4097] % 4097
    with fl.open(path, 'r') as f:
        dev = to_device(f, rows)
        for absent in ([1], [3], [1, 3], [1, 3, 4], [4]):
            names = [None if i in absent else name for i, name in enumerate(CHUNKS[key])]
            n_types = 1 if 4 in absent else 4
            got = f.frame_displacements_device(spec(names), VA, VB, n_types=n_types)
            assert same(got, model(arrays, names, n_types=n_types), absent)
            got = f.frame_displacements_device(spec(names), VB, VA, n_types=n_types, rows=dev)       # (the boxes swapped)
            assert same(got, model(arrays, names, VB, VA, n_types=n_types, rows=rows), (absent, 'list'))
        f.wait_read()


@pytest.mark.parametrize("key", ['f32', 'f64'])
def test_the_minimum_image(files, lists, key):
    """Three and two dimensions, a triclinic box, exact halves of the box (rint to even), a list."""
    path, arrays = files[70_001]
    names = [CHUNKS[key][0], None, CHUNKS[key][2], None, 'particles/typeid']
    cube = hoomd.box_vectors([4, 4, 4, 0, 0, 0])
    inf_box = hoomd.box_vectors([np.inf, 4, 4, 0, 0, 0])
    with fl.open(path, 'r') as f:
        dev = to_device(f, lists[4097])
        for vb, dims in ((VB, 3), (VB, 2), (VA, 3), (cube, 3), (cube, 2)):
            got = f.frame_displacements_device(spec(names), VA, vb, minimum_image=True, dimensions=dims, n_types=4)
            assert same(got, model(arrays, names, VA, vb, minimum_image=True, dimensions=dims, n_types=4), dims)
            got = f.frame_displacements_device(spec(names), VA, vb, minimum_image=True, dimensions=dims, type0=2,
                                               n_types=2, rows=dev)
            assert same(got, model(arrays, names, VA, vb, minimum_image=True, dimensions=dims, type0=2, n_types=2,
                                   rows=lists[4097]), (dims, 'list'))
        # an infinite box length without images: no product is formed, no NaN appears
        got = f.frame_displacements_device(spec(names), inf_box, inf_box, n_types=4)
        assert same(got, model(arrays, names, inf_box, inf_box, n_types=4)) and same(got, model(arrays, names, n_types=4))
        # halves: zero against the tie chunk scaled so that d / L is 0.5, 1.5 and -0.5
        halves = ['log/zero', None, 'log/tie_lanes', None, None]
        half = hoomd.box_vectors([14, 1, 1, 0, 0, 0])             # 7 / 14 = 0.5 -> 0; 0.5 / 1 = 0.5 -> 0
        got = f.frame_displacements_device(spec(halves), half, half, minimum_image=True)
        assert same(got, model(arrays, halves, half, half, minimum_image=True))
        assert got.largest.tolist() == [49.0] and got.largest_entry.tolist() == [5]
        f.wait_read()


# ---------------------------------------------------------------- ties for the maximum
@pytest.mark.parametrize("name", sorted(TIES))
def test_ties_for_the_maximum(files, name):
    """The same largest move in one lane, in two lanes of a wave, in two waves and in two tiles: the smallest entry."""
    path, arrays = files[70_001]
    names = ['log/zero', None, name, None, None]
    first = min(TIES[name])
    with fl.open(path, 'r') as f:
        got = f.frame_displacements_device(spec(names), VA, VB)
        assert same(got, model(arrays, names)) and got.largest_entry.tolist() == [first] and got.largest.tolist() == [49.0]
        typed = names[:4] + ['particles/typeid']
        got = f.frame_displacements_device(spec(typed), VA, VB, n_types=4)
        assert same(got, model(arrays, typed, n_types=4))
        # through a list that reverses the rows: the earlier POSITION wins, which is the largest row
        rows = np.arange(70_000, -1, -1, dtype=np.int32)
        got = f.frame_displacements_device(spec(names), VA, VB, rows=to_device(f, rows))
        assert same(got, model(arrays, names, rows=rows)) and got.largest_entry.tolist() == [70_000 - max(TIES[name])]
        f.wait_read()


def test_a_tie_across_tiles_t_and_t_plus_256(files):
    path, arrays = files[1_048_577]
    names = ['log/zero', None, 'log/tie_far', None, None]
    with fl.open(path, 'r') as f:
        got = f.frame_displacements_device(spec(names), VA, VB)
        assert same(got, model(arrays, names)) and got.largest_entry.tolist() == [4000]
        rows = np.arange(1_048_576, -1, -1, dtype=np.int32)
        got = f.frame_displacements_device(spec(names), VA, VB, rows=to_device(f, rows))
        assert same(got, model(arrays, names, rows=rows)) and got.largest_entry.tolist() == [0]
        f.wait_read()


# ---------------------------------------------------------------- one stored chunk in both frames
def test_the_same_chunk_in_both_frames_is_staged_once(files):
    N = 70_001
    path, arrays = files[N]
    with fl.open(path, 'r') as f:
        f.device_read_stats(reset=True)
        names = ['particles/position', 'particles/image', 'particles/position', 'particles/image', 'particles/typeid']
        got = f.frame_displacements_device(spec(names), VA, VA, n_types=4)
        assert f.device_read_stats()["pread_bytes"] == N * (12 + 12 + 4)
        want = model(arrays, names, VA, VA, n_types=4)
        assert same(got, want)
        # a - a is zero wherever a is finite
        assert not got.drift.any() and not got.square.any() and got.largest.tolist() == [0.0] * 4
        assert got.bad.sum() == 4 and got.largest_entry.tolist() == [4, 0, 1, 2]
        f.wait_read()
        f.device_read_stats(reset=True)
        same_pos = ['particles/position', None, 'particles/position', None, None]
        got = f.frame_displacements_device(spec(same_pos), VA, VB, minimum_image=True)
        assert f.device_read_stats()["pread_bytes"] == N * 12 and same(got, model(arrays, same_pos, minimum_image=True))
        f.wait_read()


# ---------------------------------------------------------------- the per-entry output
@pytest.mark.parametrize("key", ['f32', 'f64'])
def test_out_rows_equal_the_model_and_nothing_past_n_is_touched(files, lists, key):
    path, arrays = files[70_001]
    names = CHUNKS[key]
    with fl.open(path, 'r') as f:
        dev = f.pipeline_device()
        for rows, kw in ((None, {}), (lists[4097], {}), (lists[70_001], {}), (lists[65], {}),
                         (None, dict(minimum_image=True)), (lists[4096], dict(minimum_image=True, dimensions=2))):
            use = names if not kw else [names[0], None, names[2], None, names[4]]
            n = 70_001 if rows is None else len(rows)
            out = fl._device_from_host(np.full((n + 5, 3), 77.0), dev)
            got = f.frame_displacements_device(spec(use), VA, VB, n_types=4, out=out,
                                               rows=None if rows is None else to_device(f, rows), **kw)
            assert same(got, model(arrays, use, n_types=4, rows=rows, **kw))
            host = _host(out)
            want = vectors(arrays, use, rows=rows, **kw)
            assert same_rows(host[:n], want), (n, kw)
            assert (host[n:] == 77.0).all()
        with pytest.raises(ValueError, match="out holds fewer"):
            f.frame_displacements_device(spec(names), VA, VB, out=fl._device_from_host(np.zeros((70_000, 3)), dev))
        f.wait_read()


# ---------------------------------------------------------------- refusals
def test_an_entry_outside_the_chunks_is_refused(files):
    path, arrays = files[4097]
    names = CHUNKS['f32']
    with fl.open(path, 'r') as f:
        for bad_at, bad in ((0, 4097), (4096, 2 ** 31 - 1), (5000, -1)):
            rows = np.arange(5001, dtype=np.int32) % 4097
            rows[bad_at] = bad
            out = fl._device_from_host(np.full((5001 + 2, 3), 77.0), f.pipeline_device())
            with pytest.raises(ValueError, match="an entry of the row list lies outside the chunks"):
                f.frame_displacements_device(spec(names), VA, VB, n_types=4, rows=to_device(f, rows), out=out)
            host = _host(out)
            assert (host[bad_at] == 77.0).all() and (host[5001:] == 77.0).all()        # nothing stored for the entry
            # the call after it on the same handle is correct
            rows[bad_at] = 7
            got = f.frame_displacements_device(spec(names), VA, VB, n_types=4, rows=to_device(f, rows))
            assert same(got, model(arrays, names, n_types=4, rows=rows), bad)
            assert same(f.frame_displacements_device(spec(names), VA, VB, n_types=2), model(arrays, names, n_types=2), bad)
        f.wait_read()


def test_every_refusal_has_its_message_and_leaves_the_handle_usable(files, tmp_path):
    path, arrays = files[4097]
    other = str(tmp_path / "other.gsd")
    with fl.open(other, 'w', application="test", schema="none", schema_version=[1, 0]) as f:
        for name, a in (('tid', np.zeros((9, 1), np.uint32)), ('tid_f', np.zeros((9, 1), np.float32)),
                        ('tid_u64', np.zeros((9, 1), np.uint64)), ('tid_2', np.zeros((9, 2), np.uint32)),
                        ('p', np.ones((9, 3), np.float32)), ('q', 3 * np.ones((9, 3), np.float32)),
                        ('p64', np.ones((9, 3), np.float64)), ('p_i', np.ones((9, 3), np.int32)),
                        ('p_8', np.ones((8, 3), np.float32)), ('p_4', np.ones((9, 4), np.float32)),
                        ('im', np.zeros((9, 3), np.int32)), ('im_u', np.zeros((9, 3), np.uint32)),
                        ('im_2', np.zeros((9, 2), np.int32)), ('im_8', np.zeros((8, 3), np.int32))):
            f.write_chunk(name, a)
        f.end_frame()
    with fl.open(other, 'r') as f:
        def call(names, va=VA, vb=VB, **kw):
            return f.frame_displacements_device(spec(names), va, vb, **kw)
        for names, message in ((['p_i', None, 'p', None, None], "position chunk holds float32 or float64"),
                               (['p', None, 'tid', None, None], "position chunk holds float32 or float64"),
                               (['p', None, 'p64', None, None], "not mixed"),
                               (['p64', None, 'p', None, None], "not mixed"),
                               (['p', 'im_u', 'p', None, None], "image chunk holds int32"),
                               (['p', None, 'p', 'p', None], "image chunk holds int32"),
                               (['p', None, 'p', None, 'tid_f'], "typeid chunk holds uint32 or int32"),
                               (['p', None, 'p', None, 'tid_u64'], "typeid chunk holds uint32 or int32"),
                               (['p', None, 'p', None, 'tid_2'], "typeid chunk has 1 column"),
                               (['p_4', None, 'p', None, None], "position chunk has 3 columns"),
                               (['p', 'im_2', 'p', None, None], "image chunk has 3 columns"),
                               (['p', None, 'p_8', None, None], "differ in their number of rows"),
                               (['p', None, 'p', 'im_8', None], "differ in their number of rows")):
            with pytest.raises(ValueError, match=message):
                call(names)
        for n_types in (0, 5, 2 ** 32 - 1):
            with pytest.raises(ValueError, match="1 to 4 types"):
                call(['p', None, 'p', None, 'tid'], n_types=n_types)
        with pytest.raises(ValueError, match="n_types must be 1"):
            call(['p', None, 'p', None, None], n_types=2)
        for images in (['im', None], [None, 'im']):
            with pytest.raises(ValueError, match="minimum image is taken without image chunks"):
                call(['p', images[0], 'p', images[1], None], minimum_image=True)
        for dims in (0, 1, 4):
            with pytest.raises(ValueError, match="dimensions is 2 or 3"):
                call(['p', None, 'p', None, None], dimensions=dims)
        with pytest.raises(KeyError):
            call(['p', None, 'nothing', None, None])
        with pytest.raises(ValueError, match="position a, image a, position b, image b, typeid"):
            call(['p', None, 'p', None])
        with pytest.raises(ValueError, match="both positions"):
            call([None, None, 'p', None, None])
        with pytest.raises(ValueError, match="six values"):
            call(['p', None, 'p', None, None], va=VA[:5])
        with pytest.raises(ValueError, match="n goes with rows"):
            call(['p', None, 'p', None, None], n=5)
        rows = to_device(f, np.arange(9))
        with pytest.raises(ValueError, match="fewer entries than n"):
            call(['p', None, 'p', None, None], rows=rows, n=10)
        with pytest.raises(ValueError, match="32-bit"):
            call(['p', None, 'p', None, None], rows=fl._device_from_host(np.arange(4, dtype=np.int64), f.pipeline_device()))
        got = call(['p', 'im', 'q', 'im', 'tid'])                                # the handle works as before
        assert got.square.tolist() == [9 * 12.0] and got.drift.tolist() == [[18.0] * 3] and got.largest_entry.tolist() == [0]
        nothing = call(['p', None, 'q', None, None], rows=rows, n=0)
        assert nothing.count.tolist() == [0] and nothing.largest.tolist() == [-np.inf]
        assert nothing.largest_entry.tolist() == [-1] and nothing.sums[0, :4].view(np.uint64).tolist() == [0] * 4
        f.wait_read()
    with fl.open(path, 'r') as f:
        # what no file holds, through the entry point itself: 2^32 rows, 2^32 entries; the outputs stay untouched
        fn = _lib.lib.pgsd_frame_displacements_device
        fn.restype = ctypes.c_int32
        E, D = ctypes.POINTER(_lib.IndexEntry), ctypes.POINTER(ctypes.c_double)
        fn.argtypes = [ctypes.POINTER(_lib.Handle), E, E, E, E, E, D, D, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                       ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), D]
        h = f._h()
        entries = [_lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(h, 0, name.encode()).contents)
                   for name in CHUNKS['f32']]
        va, vb = (ctypes.c_double * 6)(*VA), (ctypes.c_double * 6)(*VB)
        counts, values = (ctypes.c_uint64 * 13)(*([77] * 13)), (ctypes.c_double * 20)(*([77.0] * 20))
        rows = to_device(f, np.array([0, 1, 4097, 2]))
        dev = ctypes.c_void_p(rows.data_ptr() if hasattr(rows, 'data_ptr') else rows.ptr)

        def raw(entries, n_types=4, rows=None, n=0, flags=0, dims=3):
            return fn(h, *[ctypes.byref(e) if e is not None else None for e in entries], va, vb, flags, dims, 0, n_types,
                      rows, n, None, counts, values)

        huge = [_lib.IndexEntry.from_buffer_copy(e) for e in entries]
        for e in huge:
            e.N = 2 ** 32
        no_images = [entries[0], None, entries[2], None, entries[4]]
        for args, message in ((dict(entries=huge), "2^32 rows"), (dict(entries=entries, rows=dev, n=2 ** 32), "2^32 entries"),
                              (dict(entries=entries, rows=dev, n=4), "outside the chunks"),
                              (dict(entries=entries, n_types=5), "1 to 4 types"),
                              (dict(entries=entries, flags=1), "without image chunks"),
                              (dict(entries=no_images, flags=2), "minimum-image bit"),
                              (dict(entries=no_images, dims=1), "dimensions is 2 or 3"),
                              (dict(entries=no_images[:4] + [None]), "n_types must be 1")):
            assert raw(**args) == _lib.ERROR_INVALID_ARGUMENT and message in _lib.last_error(), (message, _lib.last_error())
            assert list(counts) == [77] * 13 and list(values) == [77.0] * 20        # written on success only
        # the same call as it is: correct
        assert raw(entries) == 0
        want = model(arrays, CHUNKS['f32'], n_types=4)
        assert [counts[3 * t] for t in range(4)] == want.count.tolist() and counts[12] == want.other
        assert [counts[3 * t + 1] for t in range(4)] == want.bad.tolist()
        assert [counts[3 * t + 2] for t in range(4)] == want.largest_entry.tolist()
        assert np.array_equal(np.array(list(values)).reshape(4, 5).view(np.uint64), want.sums.view(np.uint64))
        # a type without an entry: UINT64_MAX
        assert raw(entries[:4] + [None], n_types=1, rows=dev, n=0) == 0
        assert counts[0] == 0 and counts[2] == 2 ** 64 - 1 and values[4] == -np.inf
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
        f.frame_displacements_device(spec(names), VA, VB, n_types=4)
        assert f.device_read_stats()["pread_bytes"] == N * 52
        got = f.frame_displacements_device(spec(names), VA, VB, type0=4, n_types=1)
        assert f.device_read_stats()["pread_bytes"] == N * 52
        assert same(got, model(arrays, names, type0=4, n_types=1))
        f.wait_read()
        # after a selection over typeid inside a domain of log/pb's... the position, and statistics of both images:
        # nothing is left to read but frame b's position
        f.device_read_stats(reset=True)
        cell = hoomd.domain_grid(2, 1, 1)[0]
        rows, count = f.select_where_device([(0, 'particles/typeid', 0, [0, 2])], domain=(0, 'particles/position', cell),
                                            box=TRI)
        f.chunk_stats_device(0, 'particles/image')
        f.chunk_stats_device(0, 'log/ib')
        f.chunk_stats_device(0, 'log/pb', norm2=True)
        before = f.device_read_stats()["pread_bytes"]
        assert before == N * 52
        got = f.frame_displacements_device(spec(names), VA, VB, n_types=4, rows=rows, n=count)
        assert f.device_read_stats()["pread_bytes"] == before
        where = hoomd.where_rows({'typeid': arrays['particles/typeid']}, {'typeid': [0, 2]})
        want_rows = np.intersect1d(where, hoomd.domain_rows(arrays['particles/position'], TRI, cell))
        assert count == len(want_rows) and same(got, model(arrays, names, n_types=4, rows=want_rows))
        f.wait_read()
        # after the wait the chunks are released: the next call reads them again
        f.frame_displacements_device(spec(names), VA, VB, n_types=4)
        assert f.device_read_stats()["pread_bytes"] == before + N * 52
        f.wait_read()


# ---------------------------------------------------------------- through pgsd.hoomd
TYPES6 = ['fluid', 'wall', 'inlet', 'outlet', 'gate', 'probe']


def _frame(rng, n, step, types, box=TRI, dimensions=3, images=True, like=None):
    fr = hoomd.Frame()
    fr.configuration.step = step
    fr.configuration.box = box
    fr.configuration.dimensions = dimensions
    fr.particles.N = n
    fr.particles.types = types
    fr.particles.position = rng.uniform(-1.9, 1.9, size=(n, 3)).astype(np.float32)
    if dimensions == 2:
        fr.particles.position[:, 2] = 0.0
    if images:
        fr.particles.image = rng.integers(-2, 3, size=(n, 3)).astype(np.int32)
        if dimensions == 2:
            fr.particles.image[:, 2] = 0
    fr.particles.density = (1000.0 + 50.0 * rng.standard_normal(n)).astype(np.float32)
    fr.particles.typeid = rng.integers(0, len(types), size=n).astype(np.uint32) if like is None else like.particles.typeid
    return fr


@pytest.fixture(scope="module")
def trajectories(tmp_path_factory):
    """traj: three frames of 70 001 particles of three types, frame 1 in another box; frame 2 elides position, image and
    typeid, which equal frame 0's.  six: two frames of six types.  flat: two 2-D frames without images.  empty: two
    frames of no particle.  other_n: two frames of different N."""
    d = _dir(tmp_path_factory, "displacements_traj")
    rng = np.random.default_rng(12)
    n = 70_001
    paths = dict((k, os.path.join(d, "pgsd_displacements_%d_%s.gsd" % (os.getpid(), k)))
                 for k in ("traj", "six", "flat", "empty", "other_n"))
    f0 = _frame(rng, n, 0, TYPES6[:3])
    f1 = _frame(rng, n, 10, TYPES6[:3], box=TRI_B, like=f0)
    f1.particles.position[[3, 255, n - 1]] = [[np.nan, 1, 1], [np.inf, 0, 0], [1, -np.inf, np.nan]]
    f2 = _frame(rng, n, 20, TYPES6[:3], like=f0)
    f2.particles.position, f2.particles.image = f0.particles.position, f0.particles.image
    with hoomd.open(paths["traj"], 'w') as t:
        for fr in (f0, f1, f2):
            t.append(fr)
    s0 = _frame(rng, 20_011, 0, TYPES6)
    with hoomd.open(paths["six"], 'w') as t:
        t.append(s0)
        t.append(_frame(rng, 20_011, 1, TYPES6, like=s0))
    flat_box = np.array([4.0, 4.0, 1.0, 0.5, 0.0, 0.0], np.float32)
    with hoomd.open(paths["flat"], 'w') as t:
        a = _frame(rng, 9001, 0, TYPES6[:3], box=flat_box, dimensions=2, images=False)
        t.append(a)
        b = _frame(rng, 9001, 1, TYPES6[:3], box=flat_box, dimensions=2, images=False, like=a)
        b.particles.position[:, 2] = rng.uniform(-9, 9, 9001).astype(np.float32)      # (z is not folded in 2-D)
        t.append(b)
    with hoomd.open(paths["empty"], 'w') as t:
        for step in (0, 1):
            none = hoomd.Frame()
            none.configuration.step = step
            none.configuration.box = TRI
            none.particles.types = TYPES6[:3]
            t.append(none)
    with hoomd.open(paths["other_n"], 'w') as t:
        t.append(_frame(rng, 100, 0, TYPES6[:3]))
        t.append(_frame(rng, 101, 1, TYPES6[:3]))
    yield paths
    for path in paths.values():
        os.unlink(path)


WHERE = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
CELL = hoomd.domain_grid(2, 2, 1)[1]
SELECTIONS = {"all": {}, "where": {'where': WHERE}, "domain": {'domain': CELL}, "both": {'where': WHERE, 'domain': CELL}}


@pytest.mark.parametrize("which", ["traj1", "traj2", "six", "flat"])
@pytest.mark.parametrize("selection", sorted(SELECTIONS))
def test_frame_displacements_device_equals_the_host_model(trajectories, selection, which):
    path, idx = (trajectories["traj"], int(which[4:])) if which.startswith("traj") else (trajectories[which], 1)
    kwargs = SELECTIONS[selection]
    with hoomd.open(path, 'r') as t:
        if which == "traj2":      # frame 2 elides what equals frame 0's
            assert not t.file.chunk_exists(2, 'particles/position') and not t.file.chunk_exists(2, 'particles/image')
        variants = [dict(), dict(by_type=False), dict(images=False)]
        variants += [dict(images=False, minimum_image=True)] if which != "six" else []
        for options in variants:
            want = t.frame_displacements(idx, **options, **kwargs)
            t.file.device_read_stats(reset=True)
            got = t.frame_displacements_device(idx, **options, **kwargs)
            pread = t.file.device_read_stats()["pread_bytes"]
            assert same(got, want, (which, selection, options))
            n = t.file.read_chunk(0, 'particles/N')[0]
            if which.startswith("traj"):
                # every chunk that takes part is read exactly once, whatever the number of passes
                frames = 1 if which == "traj2" else 2
                used = 12 * frames + (12 * frames if options.get('images', True) else 0)
                used += 4 if options.get('by_type', True) or 'where' in kwargs else 0
                assert pread == n * (used + (4 if 'where' in kwargs else 0)), (selection, options)
        full = t.frame_displacements_device(idx, **kwargs)
        if which == "traj1" and selection == "domain":
            got, rows = t.frame_displacements_device(idx, return_rows=True, **kwargs)
            want, host_rows = t.frame_displacements(idx, return_rows=True, **kwargs)
            assert same(got, want) and same(got, full)
            assert same_rows(_host(rows), host_rows) and len(host_rows) == got.count.sum()
        if which == "traj1" and selection == "all":
            assert same(t.frame_displacements_device(2, origin=1), t.frame_displacements(2, origin=1))
            assert same(t.frame_displacements_device(-1, origin=-2), t.frame_displacements(2, 1))
    T = 6 if which == "six" else 3
    assert full.count.shape == (T,) and full.drift.shape == (T, 3) and full.other == 0
    assert (int(full.count.sum()) == n) if selection == "all" else (0 < int(full.count.sum()) < n)
    if 'where' in kwargs:
        assert full.count[1] == 0 and full.largest_entry[1] == -1 and full.largest[1] == -np.inf
    if which == "traj2":
        assert not full.square.any() and not full.drift.any() and full.bad.sum() == 0
    if which == "traj1" and selection == "all":
        assert full.bad.sum() == 3


def test_frames_of_no_particle_of_different_n_and_outside(trajectories):
    with hoomd.open(trajectories["empty"], 'r') as t:
        for kwargs in SELECTIONS.values():
            got = t.frame_displacements_device(1, **kwargs)
            assert same(got, t.frame_displacements(1, **kwargs))
            assert got.count.tolist() == [0, 0, 0] and got.largest_entry.tolist() == [-1] * 3 and np.isnan(got.msd).all()
        got, rows = t.frame_displacements_device(1, return_rows=True)
        assert _host(rows).shape == (0, 3)
    with hoomd.open(trajectories["other_n"], 'r') as t:
        t.file.device_read_stats(reset=True)
        with pytest.raises(ValueError, match="differ in their number of particles"):
            t.frame_displacements_device(1)
        assert t.file.device_read_stats()["pread_bytes"] == 0           # before anything is read
        with pytest.raises(ValueError, match="differ in their number of particles"):
            t.frame_displacements(1)
    with hoomd.open(trajectories["traj"], 'r') as t:
        with pytest.raises(IndexError):
            t.frame_displacements_device(3)
        with pytest.raises(IndexError):
            t.frame_displacements_device(1, origin=3)
        with pytest.raises(ValueError, match="without image flags"):
            t.frame_displacements_device(1, minimum_image=True)
        assert same(t.frame_displacements_device(1), t.frame_displacements(1))       # the wait was made on the error path


def test_moments_statistics_and_domain_reads_are_unchanged_around_a_displacement_call(trajectories):
    d = hoomd.domain_grid(2, 2, 2)[3]
    fields = ['position', 'density', 'typeid']
    with hoomd.open(trajectories["traj"], 'r') as t:
        want_rows = hoomd.domain_rows(t[1].particles.position, TRI_B, d)
        stats_before, moments_before = t.frame_stats_device(1, fields, domain=d), t.frame_moments_device(1, domain=d)
        before = t.read_frame_device(1, domain=d)
        t.frame_displacements_device(1, domain=d)
        t.frame_displacements_device(2, origin=1, images=False, by_type=False)
        stats_after, moments_after = t.frame_stats_device(1, fields, domain=d), t.frame_moments_device(1, domain=d)
        after = t.read_frame_device(1, domain=d)
        want, want_moments = t.frame_stats(1, fields, domain=d), t.frame_moments(1, domain=d)
        density = t[1].particles.density
    for s in (before, after):
        assert np.array_equal(_host(s.tag), want_rows) and s.particles.N == len(want_rows)
        assert _host(s.particles.density).tobytes() == density[want_rows].tobytes()
    for name in want:
        for q in hoomd.FieldStats.__slots__:
            for st in (stats_before, stats_after):
                assert np.array_equal(getattr(st[name], q), getattr(want[name], q), equal_nan=True), (name, q)
    for m in (moments_before, moments_after):
        assert m.count.tolist() == want_moments.count.tolist()
        assert np.array_equal(m.sums.view(np.uint64), want_moments.sums.view(np.uint64))


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
TRI = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
VA = hoomd.box_vectors(TRI)
F32 = [(0, n) for n in ('particles/position', 'particles/image', 'log/pb', 'log/ib', 'particles/typeid')]
F64 = [(0, n) for n in ('log/pa64', 'particles/image', 'log/pb64', 'log/ib', 'particles/typeid')]
res = {}
with fl.open(path, 'r') as f:
    res["dense"] = f.frame_displacements_device(F32, VA, VA, n_types=4)
    rows = fl._device_from_host(np.arange(70000, -1, -7, dtype=np.int32), f.pipeline_device())
    out = fl.DeviceBuffer((10001, 3), np.float64, f.pipeline_device())
    res["listed"] = f.frame_displacements_device(F64, VA, VA, type0=3, n_types=2, rows=rows, out=out)
    rows_out = out.to_host()
    sel, count = f.select_where_device([(0, 'particles/typeid', 0, [1, 4])])
    res["selected"] = f.frame_displacements_device([F32[0], None, F32[2], None, None], VA, VA, minimum_image=True,
                                                   rows=sel, n=count)
    f.wait_read()
with hoomd.open(traj, 'r') as t:
    res["frame"], d = t.frame_displacements_device(1, where={'type': ['wall']}, domain=hoomd.domain_grid(2, 1, 1)[0],
                                                   return_rows=True)
    frame_rows = d.to_host()
res = dict((k, dict((q, getattr(v, q)) for q in hoomd.Displacements.__slots__)) for k, v in res.items())
res["rows_out"], res["frame_rows"] = rows_out, frame_rows
pickle.dump(res, open(out_path, "wb"))
'''


def test_displacements_without_torch(files, trajectories, tmp_path):
    path, arrays = files[70_001]
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, path, trajectories["traj"], str(out)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))

    def check(got, want, what):
        assert same(hoomd.Displacements(**got), want, what)

    listed = np.arange(70000, -1, -7)
    check(res["dense"], model(arrays, CHUNKS['f32'], VA, VA, n_types=4), "dense")
    check(res["listed"], model(arrays, CHUNKS['f64'], VA, VA, type0=3, n_types=2, rows=listed), "listed")
    assert same_rows(res["rows_out"], vectors(arrays, CHUNKS['f64'], VA, VA, rows=listed))
    sel = np.flatnonzero(np.isin(arrays['particles/typeid'], [1, 4]))
    names = ['particles/position', None, 'log/pb', None, None]
    check(res["selected"], model(arrays, names, VA, VA, minimum_image=True, rows=sel), "selected")
    with hoomd.open(trajectories["traj"], 'r') as t:
        want, rows = t.frame_displacements(1, where={'type': ['wall']}, domain=hoomd.domain_grid(2, 1, 1)[0], return_rows=True)
    check(res["frame"], want, "frame")
    assert same_rows(res["frame_rows"], rows)
