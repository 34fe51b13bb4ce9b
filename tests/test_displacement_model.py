"""The definition of the frame displacements: pgsd.hoomd.particle_displacements / frame_displacements (numpy, host only)
against a plain Python loop that spells out the tile, the lane, the step, both trees and the pair rule of the maximum --
the order in which the GPU kernels add and compare.  The loop takes a `mutation`: one deliberate mistake, which stands
for a kernel with the same mistake; every mutation must change a result of the case DESIGN.md names for it."""
import math
import os

import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

TRI = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
TRI_B = np.array([5.0, 3.0, 2.5, -0.25, 0.125, 0.375], np.float32)
SIZES = [0, 1, 63, 64, 65, 256, 4095, 4097, 70_001]
INF = math.inf


def same(got, want, what=None):
    """Integers equal, values bit for bit."""
    assert got.other == want.other, (what, got.other, want.other)
    for name in ('count', 'bad', 'largest_entry', 'drift', 'square', 'largest'):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, name, g.tolist(), w.tolist())
        else:
            assert np.array_equal(g, w), (what, name, g.tolist(), w.tolist())
    return True


def differs(got, want):
    try:
        same(got, want)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------- the loop
def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return float(np.float64(a) / np.float64(b))


def _rint(x, away=False):
    if not math.isfinite(x):
        return x
    if away:
        return math.copysign(math.floor(abs(x) + 0.5), x)
    return math.copysign(float(round(x)), x)


def _wave_tree(p):
    p = list(p)
    h = 32
    while h >= 1:
        for i in range(h):
            p[i] = p[i] + p[i + h]
        h //= 2
    return p[0]


def _block_tree(p):
    w = [_wave_tree(p[64 * i:64 * i + 64]) for i in range(4)]
    return (w[0] + w[1]) + (w[2] + w[3])


def _pair(a, b, tie=True):
    """larger value, then smaller entry; `tie` False: the tie rule dropped (the first operand keeps a tie)"""
    if b[0] > a[0] or (b[0] == a[0] and tie and b[1] < a[1]):
        return b
    return a


NO_ENTRY = 2 ** 32 - 1


def loop(pa, pb, ia=None, ib=None, va=None, vb=None, minimum_image=False, dimensions=3, typeid=None, type0=0, n_types=1,
         rows=None, mutation=None):
    """particle_displacements entry by entry in the kernels' order."""
    N = len(pa)
    entries = list(range(N)) if rows is None else [int(r) for r in rows]
    n = len(entries)
    tiles = (n + 4095) // 4096
    if mutation == 'vectors':
        vb = va
    va = None if va is None else [float(c) for c in va]
    vb = None if vb is None else [float(c) for c in vb]
    acc = [[[[0.0] * 4 for _ in range(256)] for _ in range(tiles)] for _ in range(n_types)]
    best = [[[(-INF, NO_ENTRY)] * 256 for _ in range(tiles)] for _ in range(n_types)]
    count, bad, other = [0] * n_types, [0] * n_types, 0
    out = np.zeros((n, 3))

    def unwrap(x, im, v):
        x = [float(c) for c in x]
        if im is None:
            return x
        i = [float(c) for c in im]
        if mutation == 'tilt':
            return [x[0] + (i[0] * v[0] + (i[1] * v[3] + i[2] * v[4])), x[1] + (i[1] * v[1] + i[2] * v[5]), x[2] + i[2] * v[2]]
        return [x[0] + ((i[0] * v[0] + i[1] * v[3]) + i[2] * v[4]), x[1] + (i[1] * v[1] + i[2] * v[5]), x[2] + i[2] * v[2]]

    def fold_z(d):
        m = _rint(_div(d[2], vb[2]), mutation == 'round')
        d[2] = d[2] - m * vb[2]
        d[1] = d[1] - m * vb[5]
        d[0] = d[0] - m * vb[4]

    def fold_y(d):
        m = _rint(_div(d[1], vb[1]), mutation == 'round')
        d[1] = d[1] - m * vb[1]
        d[0] = d[0] - m * vb[3]

    def fold_x(d):
        m = _rint(_div(d[0], vb[0]), mutation == 'round')
        d[0] = d[0] - m * vb[0]

    for k, row in enumerate(entries):       # (ascending k: every lane sees its steps in order)
        tile, lane = k // 4096, k % 256
        ua = unwrap(pa[row], None if ia is None else ia[row], va)
        ub = unwrap(pb[row], None if ib is None else ib[row], vb)
        d = [ub[a] - ua[a] for a in range(3)]
        if minimum_image:
            if mutation == 'fold order':
                fold_x(d)
                fold_y(d)
                if dimensions == 3:
                    fold_z(d)
            else:
                if dimensions == 3:
                    fold_z(d)
                fold_y(d)
                fold_x(d)
        if mutation == 'square':
            s = d[0] * d[0] + (d[1] * d[1] + d[2] * d[2])
        else:
            s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        out[k] = d
        t = 0 if typeid is None else int(typeid[row]) - type0
        if mutation == 'type mask' and typeid is not None:
            t -= 1
        if not 0 <= t < n_types:
            other += 1
            continue
        values = d + [s]
        fin = [math.isfinite(v) for v in values]
        if mutation == 'square sum':
            fin[3] = not math.isnan(s)
        count[t] += 1
        bad[t] += not all(math.isfinite(v) for v in values)
        for q in range(4):
            acc[t][tile][lane][q] = acc[t][tile][lane][q] + (values[q] if fin[q] else 0.0)
        held = best[t][tile][lane]
        if s > held[0] or (mutation == 'lane max' and s >= held[0]):
            best[t][tile][lane] = (s, k)
    sums = np.zeros((n_types, 5))
    entry = np.zeros(n_types, np.int64)
    for t in range(n_types):
        for q in range(4):
            tile_sums = [_block_tree([acc[t][tile][lane][q] for lane in range(256)]) for tile in range(tiles)]
            lanes = [0.0] * 256
            for tile, v in enumerate(tile_sums):    # lane t adds tiles t, t + 256, ...
                lanes[tile % 256] = lanes[tile % 256] + v
            sums[t, q] = _block_tree(lanes)
        top = (-INF, NO_ENTRY)
        # lanes in a butterfly-like scrambled order, tiles descending: the rule does not care
        for tile in reversed(range(tiles)):
            in_tile = (-INF, NO_ENTRY)
            for lane in [(37 * i + 11) % 256 for i in range(256)]:
                in_tile = _pair(in_tile, best[t][tile][lane])
            top = _pair(top, in_tile, tie=mutation != 'tile tie')
        sums[t, 4] = top[0]
        entry[t] = -1 if top[1] == NO_ENTRY else top[1]
    return hoomd.Displacements.from_sums(count, bad, entry, other, sums), out


def wide(rng, shape, dtype):
    """Normal values scaled over many decades: an input whose sum depends on the order."""
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 9, shape)).astype(dtype)


def inputs(n, dtype, seed=0):
    rng = np.random.default_rng(seed + n)
    pa = rng.uniform(-2.0, 2.0, (n, 3)).astype(dtype)
    pb = (pa + wide(rng, (n, 3), dtype)).astype(dtype)
    ia = rng.integers(-3, 4, (n, 3)).astype(np.int32)
    ib = (ia + rng.integers(-1, 2, (n, 3))).astype(np.int32)
    tid = rng.integers(0, 5, n).astype(np.uint32)
    return pa, pb, ia, ib, tid


VA, VB = hoomd.box_vectors(TRI), hoomd.box_vectors(TRI_B)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", SIZES[:-1])
def test_the_model_equals_the_loop(n, dtype):
    pa, pb, ia, ib, tid = inputs(n, dtype)
    rng = np.random.default_rng(n)
    rows = rng.integers(0, max(n, 1), size=n + 3) if n else np.zeros(0, np.int64)       # unsorted, with repeats
    for kw in (dict(ia=ia, ib=ib, typeid=tid, n_types=4), dict(ia=ia, ib=ib), dict(typeid=tid, type0=1, n_types=3),
               dict(), dict(ia=ia, typeid=tid, type0=3, n_types=2, rows=rows), dict(ib=ib, rows=rows),
               dict(minimum_image=True, typeid=tid, n_types=2), dict(minimum_image=True, dimensions=2, rows=rows)):
        want, d = loop(pa, pb, va=VA, vb=VB, **kw)
        args = dict(image_a=kw.get('ia'), image_b=kw.get('ib'), vectors_a=VA, vectors_b=VB,
                    minimum_image=kw.get('minimum_image', False), dimensions=kw.get('dimensions', 3), rows=kw.get('rows'))
        got = hoomd.particle_displacements(pa, pb, typeid=kw.get('typeid'), type0=kw.get('type0', 0),
                                           n_types=kw.get('n_types', 1), **args)
        assert same(got, want, (n, sorted(kw)))
        assert np.array_equal(hoomd.displacement_vectors(pa, pb, **args).view(np.uint64), d.view(np.uint64))


@pytest.fixture(scope="module")
def many():
    return inputs(70_001, np.float32)


def test_the_model_equals_the_loop_over_many_tiles(many):
    pa, pb, ia, ib, tid = many
    want, _ = loop(pa, pb, ia, ib, VA, VB, typeid=tid, n_types=4)
    got = hoomd.particle_displacements(pa, pb, ia, ib, VA, VB, typeid=tid, n_types=4)
    assert same(got, want)
    # the order shows: a plain numpy sum of the same values differs
    d = hoomd.displacement_vectors(pa, pb, ia, ib, VA, VB)
    assert sum(got.drift[t, a] != np.sum(np.where(tid == t, d[:, a], 0.0)) for t in range(4) for a in range(3)) >= 6


def test_the_tile_walk_over_more_than_256_tiles():
    """257 tiles: lane 0 of the final walk adds a second tile."""
    n = 256 * 4096 + 1
    rng = np.random.default_rng(5)
    pa = np.zeros((n, 3), np.float32)
    pb = wide(rng, (n, 3), np.float32)
    got = hoomd.particle_displacements(pa, pb)
    d = pb.astype(np.float64)
    lanes = d.copy()
    lanes.resize((257 * 4096, 3))
    per_tile = [hoomd._ordered_sum(lanes[t * 4096:(t + 1) * 4096, 0]) for t in range(257)]
    walk = [0.0] * 256
    for t, v in enumerate(per_tile):
        walk[t % 256] = walk[t % 256] + v
    assert got.drift[0, 0] == _block_tree(walk)
    assert got.largest_entry[0] == int(np.argmax((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))


# ---------------------------------------------------------------- by hand
def test_box_vectors():
    v = hoomd.box_vectors(TRI)
    assert v.dtype == np.float64 and v.tolist() == [4.0, 4.0, 2.0, 2.0, 0.5, -0.25]
    third = np.float32(1.0) / np.float32(3.0)
    v = hoomd.box_vectors(np.array([3.0, third, third, third, third, third], np.float32))
    t = float(third)
    assert v.tolist() == [3.0, t, t, t * t, t * t, t * t]        # float64 first, then ONE float64 product
    assert np.isinf(hoomd.box_vectors([np.inf, 1, 1, 0, 0, 0])[0])
    with pytest.raises(ValueError):
        hoomd.box_vectors([1, 2, 3])


def one(pa, pb, **kw):
    return hoomd.particle_displacements(np.array(pa, np.float64).reshape(-1, 3), np.array(pb, np.float64).reshape(-1, 3), **kw)


def test_a_triclinic_box_and_different_boxes():
    ia, ib = np.array([[1, -1, 2]], np.int32), np.array([[0, 1, -1]], np.int32)
    got = one([0.5, 0.25, -0.5], [1.0, 1.0, 1.0], image_a=ia, image_b=ib, vectors_a=VA, vectors_b=VB)
    ua = [0.5 + ((1 * 4.0 + -1 * 2.0) + 2 * 0.5), 0.25 + (-1 * 4.0 + 2 * -0.25), -0.5 + 2 * 2.0]
    b = [float(c) for c in VB]
    ub = [1.0 + ((0 * b[0] + 1 * b[3]) + -1 * b[4]), 1.0 + (1 * b[1] + -1 * b[5]), 1.0 + -1 * b[2]]
    d = [ub[a] - ua[a] for a in range(3)]
    assert got.drift.tolist() == [d] and got.square.tolist() == [(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]]
    assert got.largest.tolist() == got.square.tolist() and got.largest_entry.tolist() == [0]
    assert b[3] == -0.25 * 3.0 and ua == [3.5, -4.25, 3.5]


@pytest.mark.parametrize("step", [1, -1, 1000, -1000])
def test_image_differences(step):
    ia = np.zeros((2, 3), np.int32)
    ib = np.array([[step, 0, 0], [0, step, step]], np.int32)
    x = [[0.5, 0.5, 0.5], [-1.0, 1.0, 0.25]]
    got = one(x, x, image_a=ia, image_b=ib, vectors_a=VA, vectors_b=VA)
    d1 = [(0.0 + step * 2.0) + step * 0.5, step * 4.0 + step * -0.25, step * 2.0]
    assert got.drift[0].tolist() == [step * 4.0 + d1[0], d1[1], d1[2]]
    assert got.largest_entry.tolist() == [1]


def test_special_values():
    pa = np.zeros((6, 3))
    pb = np.array([[1, 2, 2], [np.nan, 1, 1], [np.inf, 0, 0], [-0.0, -0.0, -0.0], [3, 0, 0], [1e200, 0, 0]])
    got = hoomd.particle_displacements(pa, pb)
    # each sum skips only its own non-finite entries; row 5: d is finite, its square is not
    assert got.count.tolist() == [6] and got.bad.tolist() == [3]
    assert got.drift.tolist() == [[1 + 3 + 1e200, 2 + 1, 2 + 1]] and got.square.tolist() == [9.0 + 0.0 + 9.0]
    assert got.largest.tolist() == [np.inf] and got.largest_entry.tolist() == [2]        # infinities take part, NaN not
    assert got.msd.tolist() == [18.0 / 3] and got.largest_distance.tolist() == [np.inf]
    zero = hoomd.particle_displacements(pa[3:4], pb[3:4])
    assert zero.drift.view(np.uint64).tolist() == [[0, 0, 0]] and zero.largest.tolist() == [0.0]    # +0.0: never -0.0
    assert np.signbit(hoomd.displacement_vectors(pa[3:4], pb[3:4])).all()


def test_ties_for_the_maximum():
    pa = np.zeros((5, 3))
    pb = np.array([[1, 0, 0], [0, 3, 0], [0, 0, -3], [3, 0, 0], [0, 2, 0]], float)
    assert hoomd.particle_displacements(pa, pb).largest_entry.tolist() == [1]
    got = hoomd.particle_displacements(pa, pb, rows=[4, 3, 0, 2, 1, 3])
    assert got.largest_entry.tolist() == [1] and got.largest.tolist() == [9.0]        # a position in the list: the earlier
    tid = np.array([0, 1, 0, 1, 0], np.uint32)
    got = hoomd.particle_displacements(pa, pb, typeid=tid, n_types=2)
    assert got.largest_entry.tolist() == [2, 1]
    assert got.total().largest_entry.tolist() == [1] and got.total().largest.tolist() == [9.0]


def test_no_entry_all_nan_and_ids_outside():
    pa = np.zeros((4, 3), np.float32)
    pb = np.array([[np.nan, 0, 0], [1, 0, 0], [0, np.nan, 0], [2, 0, 0]], np.float32)
    tid = np.array([0, 1, 0, 7], np.uint32)
    got = hoomd.particle_displacements(pa, pb, typeid=tid, n_types=3)
    assert got.count.tolist() == [2, 1, 0] and got.bad.tolist() == [2, 0, 0] and got.other == 1
    assert got.largest.tolist() == [-np.inf, 1.0, -np.inf] and got.largest_entry.tolist() == [-1, 1, -1]
    assert got.square.view(np.uint64).tolist() == [0, np.float64(1.0).view(np.uint64), 0]
    assert np.isnan(got.msd[[0, 2]]).all() and got.msd[1] == 1.0 and np.isnan(got.mean_drift[0]).all()
    assert got.largest_distance[1] == 1.0 and np.isnan(got.largest_distance[0])       # sqrt(-inf)
    signed = np.array([-1, 1, -2 ** 31, 0], np.int32)
    got = hoomd.particle_displacements(pa, pb, typeid=signed, type0=0, n_types=2)
    assert got.count.tolist() == [1, 1] and got.other == 2
    got = hoomd.particle_displacements(pa, pb, typeid=tid, type0=1, n_types=1)
    assert got.count.tolist() == [1] and got.other == 3
    empty = hoomd.particle_displacements(pa[:0], pb[:0])
    assert empty.count.tolist() == [0] and empty.largest.tolist() == [-np.inf] and empty.largest_entry.tolist() == [-1]
    assert empty.drift.view(np.uint64).tolist() == [[0, 0, 0]]


def test_minimum_image():
    cube = hoomd.box_vectors([4, 4, 4, 0, 0, 0])
    # exactly half a box: rint rounds to even, so 2.0 / 4 = 0.5 -> 0 (stays +2) and 6.0 / 4 = 1.5 -> 2 (becomes -2)
    got = hoomd.displacement_vectors(np.zeros((4, 3)), np.array([[2.0, 0, 0], [6.0, 0, 0], [-2.0, 0, 0], [0, 0, 10.0]]),
                                     vectors_b=cube, minimum_image=True)
    assert got.tolist() == [[2.0, 0, 0], [-2.0, 0, 0], [-2.0, 0, 0], [0, 0, 2.0]]
    # two dimensions: z is not folded
    flat = hoomd.displacement_vectors(np.zeros((1, 3)), np.array([[5.0, -5.0, 10.0]]), vectors_b=cube, minimum_image=True,
                                      dimensions=2)
    assert flat.tolist() == [[1.0, -1.0, 10.0]]
    # tilt: folding z by one box vector moves y by yz*Lz and x by xz*Lz; then y moves x by xy*Ly
    v = [float(c) for c in VA]
    d = hoomd.displacement_vectors(np.zeros((1, 3)), np.array([[0.25, 3.0, 1.5]]), vectors_b=VA, minimum_image=True)
    z = 1.5 - 1.0 * v[2]
    y = 3.0 - 1.0 * v[5]
    x = 0.25 - 1.0 * v[4]
    ny = float(np.rint(y / v[1]))
    y, x = y - ny * v[1], x - ny * v[3]
    nx = float(np.rint(x / v[0]))
    assert ny == 1.0 and d.tolist() == [[x - nx * v[0], y, z]]
    with pytest.raises(ValueError, match="without image flags"):
        hoomd.particle_displacements(np.zeros((1, 3)), np.zeros((1, 3)), image_b=np.zeros((1, 3), np.int32), vectors_b=cube,
                                     minimum_image=True)


def test_an_infinite_box_without_images_creates_no_nan():
    box = hoomd.box_vectors([np.inf, 4, 4, 0, 0, 0])
    pa, pb = np.zeros((2, 3), np.float32), np.array([[1, 2, 2], [0, 0, 1]], np.float32)
    got = hoomd.particle_displacements(pa, pb, vectors_a=box, vectors_b=box)
    assert got.bad.tolist() == [0] and got.square.tolist() == [10.0]
    zero = np.zeros((2, 3), np.int32)
    with_images = hoomd.particle_displacements(pa, pb, image_a=zero, image_b=zero, vectors_a=box, vectors_b=box)
    assert with_images.bad.tolist() == [2]         # 0 * inf: the products ARE formed with an image array


# ---------------------------------------------------------------- groups of types, frames
def test_six_types_in_two_groups_and_the_total():
    pa, pb, ia, ib, _ = inputs(9001, np.float32, seed=3)
    tid = np.random.default_rng(1).integers(0, 6, 9001).astype(np.uint32)
    kw = dict(image_a=ia, image_b=ib, vectors_a=VA, vectors_b=VB, typeid=tid)
    parts = [hoomd.particle_displacements(pa, pb, type0=0, n_types=4, **kw),
             hoomd.particle_displacements(pa, pb, type0=4, n_types=2, **kw)]
    assert parts[0].other == int((tid >= 4).sum())
    six = hoomd.Displacements.concatenate(parts, 9001)
    assert six.count.tolist() == np.bincount(tid, minlength=6).tolist() and six.other == 0
    assert six.drift.shape == (6, 3) and six.largest_entry.dtype == np.int64
    total = six.total()
    acc = six.sums[0, :4].copy()
    for t in range(1, 6):
        acc = acc + six.sums[t, :4]
    assert total.sums[0, :4].tolist() == acc.tolist() and total.count.tolist() == [9001]
    one_group = hoomd.particle_displacements(pa, pb, **dict(kw, typeid=None))
    assert total.largest.tolist() == one_group.largest.tolist()
    assert total.largest_entry.tolist() == one_group.largest_entry.tolist()
    frames = ({'position': pa, 'image': ia}, {'position': pb, 'image': ib, 'typeid': tid})
    got = hoomd.frame_displacements(*frames, types=list('abcdef'), box=(TRI, TRI_B))
    assert same(got, six)
    assert same(hoomd.frame_displacements(*frames, by_type=False, box=(TRI, TRI_B)), one_group)
    none = hoomd.frame_displacements(*frames, images=False, by_type=False)
    assert same(none, hoomd.particle_displacements(pa, pb))
    assert not hasattr(got, '__dict__') and "Displacements(" in repr(got) and isinstance(got.other, int)


def test_frame_displacements_over_a_selection():
    pa, pb, ia, ib, _ = inputs(5003, np.float32, seed=8)
    pb = np.clip(pb, -1.9, 1.9)
    tid = np.random.default_rng(2).integers(0, 3, 5003).astype(np.uint32)
    a, b = {'position': pa, 'image': ia}, {'position': pb, 'image': ib, 'typeid': tid}
    types = ['fluid', 'wall', 'inlet']
    cell = hoomd.domain_grid(2, 1, 1)[0]
    where = {'type': ['fluid', 'inlet']}
    rows_w = hoomd.where_rows(b, where, types)
    rows_d = hoomd.domain_rows(pb, TRI, cell)                   # (the selection looks at frame b)
    assert 0 < len(rows_d) < 5003 and not np.array_equal(rows_d, hoomd.domain_rows(pa, TRI, cell))
    kw = dict(image_a=ia, image_b=ib, vectors_a=VA, vectors_b=VA, typeid=tid, n_types=3)
    for sel, rows in ((dict(where=where), rows_w), (dict(domain=cell), rows_d),
                      (dict(where=where, domain=cell), np.intersect1d(rows_w, rows_d))):
        got = hoomd.frame_displacements(a, b, types=types, box=TRI, **sel)
        assert same(got, hoomd.particle_displacements(pa, pb, rows=rows, **kw), sorted(sel))
    fa, fb = hoomd.Frame(), hoomd.Frame()
    for fr, p, im, box in ((fa, pa, ia, TRI), (fb, pb, ib, TRI_B)):
        fr.configuration.box = box
        fr.particles.N, fr.particles.types, fr.particles.position, fr.particles.image = 5003, types, p, im
    fb.particles.typeid = tid
    got = hoomd.frame_displacements(fa, fb, where=where)
    assert same(got, hoomd.particle_displacements(pa, pb, rows=rows_w, **dict(kw, vectors_b=VB)))


def test_every_value_error():
    p, q = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float64)
    im, tid = np.zeros((4, 3), np.int32), np.zeros(4, np.uint32)
    f = hoomd.particle_displacements
    for args, kw, message in (((p.astype(np.int32), p), {}, "float32 or float64 positions"),
                              ((p, q), {}, "not float32 and float64 mixed"),
                              ((p[:, :2], p), {}, "N x 3"),
                              ((p, p[:3]), {}, "differ in their number of rows"),
                              ((p, p), dict(image_a=im.astype(np.int64), vectors_a=VA), "int32"),
                              ((p, p), dict(image_b=im[:3], vectors_b=VA), "differ in their number of rows"),
                              ((p, p), dict(image_b=im[:, :2], vectors_b=VA), "N x 3"),
                              ((p, p), dict(image_a=im), "box vectors"),
                              ((p, p), dict(minimum_image=True), "box vectors"),
                              ((p, p), dict(image_a=im, vectors_a=VA[:5]), "six values"),
                              ((p, p), dict(image_a=im, vectors_a=VA, vectors_b=VA, minimum_image=True), "without image flags"),
                              ((p, p), dict(dimensions=4), "dimensions is 2 or 3"),
                              ((p, p), dict(n_types=0), "1 to 4 types"), ((p, p), dict(typeid=tid, n_types=5), "1 to 4 types"),
                              ((p, p), dict(n_types=2), "n_types must be 1"),
                              ((p, p), dict(typeid=tid.astype(np.float32)), "uint32 or int32"),
                              ((p, p), dict(typeid=tid[:3]), "differ in their number of rows"),
                              ((p, p), dict(typeid=tid, type0=-1), "type0"),
                              ((p, p), dict(rows=[0, 4]), "outside the array"), ((p, p), dict(rows=[0.5]), "integer")):
        with pytest.raises(ValueError, match=message):
            f(*args, **kw)
    with pytest.raises(ValueError, match="number of particles"):
        hoomd.frame_displacements({'position': p}, {'position': p[:3]}, by_type=False)
    with pytest.raises(ValueError, match="by_type needs"):
        hoomd.frame_displacements({'position': p}, {'position': p})
    with pytest.raises(ValueError, match="a domain needs box"):
        hoomd.frame_displacements({'position': p}, {'position': p}, by_type=False, domain=hoomd.domain_grid(2, 1, 1)[0])
    with pytest.raises(ValueError, match="no 'position'"):
        hoomd.frame_displacements({'image': im}, {'position': p}, by_type=False)


# ---------------------------------------------------------------- mutations
def _case(name):
    """The inputs of the case DESIGN.md names for a mutation."""
    rng = np.random.default_rng(17)
    n = 300
    pa = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    pb = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    ia = rng.integers(-1000, 1001, (n, 3)).astype(np.int32)
    ib = rng.integers(-1000, 1001, (n, 3)).astype(np.int32)
    tid = rng.integers(0, 4, n).astype(np.uint32)
    third = hoomd.box_vectors(np.array([3.3, 4.7, 2.9, 0.37, 0.23, -0.19], np.float32))
    if name == 'square':
        return (wide(rng, (n, 3), np.float32), wide(rng, (n, 3), np.float32)), dict(typeid=tid, n_types=4)
    if name == 'square sum':
        pa64, pb64 = pa.astype(np.float64), pb.astype(np.float64)
        pb64[7] = [1e200, 1, 1]              # d is finite, s is infinite
        return (pa64, pb64), dict(typeid=tid, n_types=4)
    if name == 'tilt':
        return (pa, pb), dict(ia=ia, ib=ib, va=third, vb=third)
    if name == 'vectors':
        return (pa, pb), dict(ia=ia, ib=ib, va=VA, vb=VB)
    if name in ('lane max', 'tile tie'):
        # ties in one lane (entries 5 and 5 + 256), in two lanes, in two waves and in two tiles
        n = 2 * 4096
        pa, pb = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        for k in (5, 5 + 256, 70, 200, 4096 + 5) if name == 'lane max' else (70, 200, 4096 + 5):
            pb[k, 0] = 7.0
        return (pa, pb), dict()
    if name in ('fold order', 'round'):
        pb = rng.uniform(-9, 9, (n, 3)).astype(np.float32)
        pa[:] = 0
        pb[0] = [2.0, 6.0, 1.0]              # d / L is exactly 0.5 and 1.5: half away from zero goes wrong
        return (pa, pb), dict(vb=VA, minimum_image=True)
    if name == 'type mask':
        return (pa, pb), dict(typeid=tid, type0=1, n_types=2)
    raise KeyError(name)


MUTATIONS = ['square', 'tilt', 'vectors', 'lane max', 'tile tie', 'fold order', 'round', 'type mask', 'square sum']


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_every_mutation_is_caught(mutation):
    """The loop with one mistake differs from the model on the case named for it, and the loop without it does not."""
    (pa, pb), kw = _case(mutation)
    model_kw = dict(image_a=kw.get('ia'), image_b=kw.get('ib'), vectors_a=kw.get('va'), vectors_b=kw.get('vb'),
                    minimum_image=kw.get('minimum_image', False), typeid=kw.get('typeid'), type0=kw.get('type0', 0),
                    n_types=kw.get('n_types', 1))
    want = hoomd.particle_displacements(pa, pb, **model_kw)
    assert same(loop(pa, pb, **kw)[0], want, mutation)
    assert differs(loop(pa, pb, mutation=mutation, **kw)[0], want), mutation


# ---------------------------------------------------------------- the command line
def test_the_command_line_prints_the_displacements(tmp_path, capsys):
    path = str(tmp_path / "small.gsd")
    with hoomd.open(path, 'w') as t:
        for step, shift, image in ((0, 0.0, 0), (5, 1.0, 0), (9, -1.0, 1)):
            fr = hoomd.Frame()
            fr.configuration.step = step
            fr.configuration.box = [8, 8, 8, 0, 0, 0]
            fr.particles.N = 4
            fr.particles.types = ['fluid', 'wall']
            fr.particles.typeid = np.array([0, 0, 1, 0], np.uint32)
            fr.particles.position = np.array([[1, 1, 1], [-2, 0, 2], [0.5, 0.5, 0.5], [2, -2, 0]], np.float32)
            fr.particles.position[[0, 1, 3], 0] += shift
            fr.particles.position[3, 1] += 2 * shift
            fr.particles.image = np.array([[0, 0, 0], [image, 0, 0], [0, 0, 0], [0, 0, 0]], np.int32)
            t.append(fr)
    assert pgsd_main(['info', path, '--displacement', '--frame', '1']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "displacements of frame 1 against frame 0:" in lines
    assert "fluid count 3 bad 0 mean drift (1.0, 0.6666666666666666, 0.0) msd 2.3333333333333335 largest distance " \
           "2.23606797749979 row 3" in lines
    assert "wall count 1 bad 0 mean drift (0.0, 0.0, 0.0) msd 0.0 largest distance 0.0 row 2" in lines
    assert "total count 4 bad 0 mean drift (0.75, 0.5, 0.0) msd 1.75 largest distance 2.23606797749979 row 3" in lines
    assert pgsd_main(['info', path, '--displacement', '--all-frames', '--types', 'fluid']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "displacements per frame against frame 0 (types fluid):" in lines
    assert "frame 0 step 0 count 3 bad 0 mean drift (0.0, 0.0, 0.0) msd 0.0 largest distance 0.0 row 0" in lines
    # frame 2: particle 1 moved by -1 and crossed into the next image: +8 - 1 = 7; position 1 of the fluid's row list
    assert "frame 2 step 9 count 3 bad 0 mean drift (1.6666666666666667, -0.6666666666666666, 0.0) msd 18.333333333333332 " \
           "largest distance 7.0 row 1" in lines
    assert pgsd_main(['info', path, '--displacement', '--minimum-image', '--origin', '1']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "displacements of frame 2 against frame 1 (minimum image):" in lines
    assert "fluid count 3 bad 0 mean drift (-2.0, -1.3333333333333333, 0.0) msd 9.333333333333334 largest distance " \
           "4.47213595499958 row 3" in lines
    assert os.path.exists(path)
