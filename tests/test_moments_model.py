"""Conservation sums, the host model: pgsd.hoomd.particle_moments / frame_moments / Moments and `info --moments`.  The
model is the definition the GPU reduction must equal bit for bit (tests/test_gpu_moments.py), so it is itself checked
against a plain Python loop that states tile, lane, step and both trees explicitly."""
import math
import os

import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
TRI = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
NAMES = ('count', 'bad', 'mass', 'momentum', 'kinetic', 'internal', 'first_moment')


def wide(rng, n, dtype=np.float32):
    """Normal values scaled over 15 decades: an input whose sum depends on the order."""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 12, n)).astype(dtype)


def inputs(rng, n, dtype):
    return dict(mass=np.abs(wide(rng, n, dtype)) + dtype(0.5), velocity=wide(rng, 3 * n, dtype).reshape(n, 3),
                energy=wide(rng, n, dtype), position=rng.uniform(-3, 3, (n, 3)).astype(dtype),
                typeid=(np.arange(n) % 5).astype(np.uint32))


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


# ---------------------------------------------------------------- the definition as a loop
def tree(p):
    """The block tree over 256 lane sums."""
    w = []
    for wave in range(4):
        q = list(p[64 * wave:64 * wave + 64])
        for h in (32, 16, 8, 4, 2, 1):
            for i in range(h):
                q[i] = q[i] + q[i + h]
        w.append(q[0])
    return (w[0] + w[1]) + (w[2] + w[3])


def loop_sum(seq):
    """Entry k: tile k // 4096, lane k % 256, step (k % 4096) // 256; lanes add in step order, the tree per tile; lane t
    of the last step adds tiles t, t + 256, ... in that order, and the tree again."""
    n = len(seq)
    tile_sums = []
    for tile in range((n + 4095) // 4096):
        lanes = [0.0] * 256
        for step in range(16):
            for lane in range(256):
                k = tile * 4096 + step * 256 + lane
                if k < n:
                    lanes[lane] = lanes[lane] + seq[k]
        tile_sums.append(tree(lanes))
    lanes = [0.0] * 256
    for lane in range(256):
        for t in range(lane, len(tile_sums), 256):
            lanes[lane] = lanes[lane] + tile_sums[t]
    return tree(lanes)


def loop_moments(mass, velocity, energy, position, typeid=None, type0=0, n_types=1, rows=None):
    """particle_moments over materialised arrays, entry by entry in Python floats (IEEE doubles, no fused multiply-add)."""
    order = range(len(mass)) if rows is None else [int(r) for r in rows]
    seq = [[[] for _ in range(9)] for _ in range(n_types)]
    count, bad, other = [0] * n_types, [0] * n_types, 0
    for r in order:
        m, e = float(mass[r]), float(energy[r])
        vx, vy, vz = (float(c) for c in velocity[r])
        x = [float(c) for c in position[r]]
        val = [m, m * vx, m * vy, m * vz, (0.5 * m) * ((vx * vx + vy * vy) + vz * vz), m * e, m * x[0], m * x[1], m * x[2]]
        t = 0 if typeid is None else int(typeid[r]) - type0
        if not 0 <= t < n_types:
            other += 1
            t = None
        else:
            count[t] += 1
            bad[t] += 0 if all(math.isfinite(q) for q in val) else 1
        for u in range(n_types):
            for q in range(9):
                seq[u][q].append(val[q] if u == t and math.isfinite(val[q]) else 0.0)
    sums = [[loop_sum(seq[u][q]) for q in range(9)] for u in range(n_types)]
    return hoomd.Moments.from_sums(count, bad, other, np.array(sums, dtype=np.float64).reshape(n_types, 9))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", LENGTHS)
def test_the_model_equals_the_loop(n, dtype):
    a = inputs(np.random.default_rng(n + 1), n, dtype)
    floats = dict((k, a[k]) for k in ('mass', 'velocity', 'energy', 'position'))
    assert same(hoomd.particle_moments(**floats), loop_moments(**floats), 'no typeid')
    assert same(hoomd.particle_moments(typeid=a['typeid'], type0=1, n_types=2, **floats),
                loop_moments(typeid=a['typeid'], type0=1, n_types=2, **floats), 'two types')
    if n:
        rows = np.random.default_rng(7).integers(0, n, size=n + 3)        # unsorted, with repeats
        assert same(hoomd.particle_moments(typeid=a['typeid'].astype(np.int32), n_types=4, rows=rows, **floats),
                    loop_moments(typeid=a['typeid'], n_types=4, rows=rows, **floats), 'list')


@pytest.fixture(scope="module")
def many():
    """70 001 entries scaled over many decades."""
    return inputs(np.random.default_rng(70_001), 70_001, np.float32)


def test_the_model_equals_the_loop_over_many_tiles(many):
    floats = dict((k, many[k]) for k in ('mass', 'velocity', 'energy', 'position'))
    rows = np.random.default_rng(8).integers(0, 70_001, size=70_001)
    assert same(hoomd.particle_moments(typeid=many['typeid'], type0=3, n_types=2, rows=rows, **floats),
                loop_moments(typeid=many['typeid'], type0=3, n_types=2, rows=rows, **floats), 'list')
    f64 = dict((k, v.astype(np.float64) * 1.000000001) for k, v in floats.items())
    assert same(hoomd.particle_moments(**f64), loop_moments(**f64), 'float64')


def test_the_tile_walk_over_more_than_256_tiles():
    """257 tiles: lane 0 of the last step adds tile 0, then tile 256.  One quantity against the loop is enough for the
    walk (the loop over all nine at this length would take a minute)."""
    n = 256 * 4096 + 1
    mass = np.abs(wide(np.random.default_rng(257), n)) + np.float32(0.5)
    got = hoomd.particle_moments(mass, None)
    want = loop_sum([float(m) for m in mass])
    assert got.mass[0] == want and got.count.tolist() == [n]
    assert got.mass[0] != float(np.sum(mass.astype(np.float64)))


def test_the_input_tells_summation_orders_apart(many):
    """The ordered sum of the per-type momentum differs from numpy's pairwise sum and from a running sum."""
    got = hoomd.particle_moments(many['mass'], many['velocity'], typeid=many['typeid'], n_types=4)
    m, v = many['mass'].astype(np.float64), many['velocity'].astype(np.float64)
    differs = 0
    for t in range(4):
        seq = np.where(many['typeid'] == t, m * v[:, 0], 0.0)
        assert got.momentum[t, 0] == hoomd._ordered_sum(seq)
        differs += got.momentum[t, 0] != np.sum(seq)
        assert len({float(got.momentum[t, 0]), float(np.sum(seq)), float(np.cumsum(seq)[-1])}) >= 2
    assert differs >= 1
    seq = m * v[:, 0]
    assert hoomd.particle_moments(many['mass'], many['velocity']).momentum[0, 0] != np.sum(seq)


# ---------------------------------------------------------------- special values
def test_special_values_by_hand():
    mass = np.array([np.nan, 0.0, 2.0, -0.0, 1.0], np.float32)
    velocity = np.array([[1, 2, 3], [np.inf, 0, 0], [1, -2, 0.5], [1, 1, 1], [-0.0, 0, 0]], np.float32)
    got = hoomd.particle_moments(mass, velocity, energy=np.float32(2.0), position=(1.0, 0.0, -1.0))
    # entry 0: every value NaN; entry 1: m * inf = NaN, kinetic NaN, but the mass 0 and m * e, m * x are summed
    assert got.count.tolist() == [5] and got.bad.tolist() == [2] and got.other == 0
    assert got.mass.tolist() == [3.0] and got.momentum.tolist() == [[2.0, -4.0, 1.0]]
    assert got.kinetic.tolist() == [1.0 * (1 + 4 + 0.25)] and got.internal.tolist() == [6.0]
    assert got.first_moment.tolist() == [[3.0, 0.0, -3.0]]
    assert not np.signbit(got.first_moment[0, 1])
    assert same(got, loop_moments(mass, velocity, np.full(5, 2.0), np.tile([1.0, 0.0, -1.0], (5, 1))))
    # only negative zeros: the sums start at +0.0 and stay there
    z = hoomd.particle_moments(np.full(3, -0.0, np.float32), np.zeros((3, 3), np.float32))
    assert z.mass.view(np.uint64).tolist() == [0] and z.momentum.view(np.uint64).tolist() == [[0, 0, 0]]


def test_a_float32_denormal_and_a_kinetic_overflow():
    d = np.float32(2.0 ** -140)
    got = hoomd.particle_moments(np.array([d, d], np.float32), np.array([[d, 1, 0], [0, 0, 2]], np.float32))
    assert got.mass[0] == 2.0 ** -139 and got.momentum[0].tolist() == [2.0 ** -280, 2.0 ** -140, 2.0 ** -139]
    assert got.bad[0] == 0
    # float64: |v|^2 overflows, m * v does not -- the entry is bad, its momentum and mass are summed, its kinetic is not
    big = hoomd.particle_moments(np.array([2.0, 1.0]), np.array([[1e200, 0, 0], [3.0, 4.0, 0]]))
    assert big.bad.tolist() == [1] and big.mass.tolist() == [3.0] and big.momentum[0].tolist() == [2e200 + 3.0, 4.0, 0.0]
    assert big.kinetic.tolist() == [12.5]


def test_a_type_without_entries_and_ids_outside_the_range():
    rng = np.random.default_rng(3)
    a = inputs(rng, 300, np.float32)
    tid = np.array([0, 2, 7, -1, -2 ** 31] * 60, np.int32)
    got = hoomd.particle_moments(a['mass'], a['velocity'], a['energy'], a['position'], typeid=tid, n_types=3)
    assert got.count.tolist() == [60, 0, 60] and got.other == 180
    assert got.sums[1].view(np.uint64).tolist() == [0] * 9            # +0.0, not -0.0
    assert np.isnan(got.centre_of_mass[1]).all() and np.isnan(got.mean_velocity[1]).all()
    assert np.array_equal(got.centre_of_mass[0], got.first_moment[0] / got.mass[0])
    assert np.array_equal(got.mean_velocity[2], got.momentum[2] / got.mass[2])
    # the same ids as uint32: 2^32 - 1 and 2^31 are ids like any other
    big = hoomd.particle_moments(a['mass'], a['velocity'], typeid=tid.view(np.uint32), type0=2 ** 32 - 1, n_types=1)
    assert big.count.tolist() == [60] and big.other == 240
    assert hoomd.particle_moments(a['mass'], a['velocity'], typeid=tid, type0=2 ** 32 - 1).count.tolist() == [0]
    assert same(got, loop_moments(a['mass'], a['velocity'], a['energy'], a['position'], tid, 0, 3))


def test_default_rows_and_none_equal_materialised_arrays():
    rng = np.random.default_rng(4)
    n = 5000
    a = inputs(rng, n, np.float32)
    ones, zeros, zeros3 = np.ones(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    want = hoomd.particle_moments(ones, a['velocity'], zeros, zeros3, typeid=a['typeid'], n_types=4)
    assert same(hoomd.particle_moments(None, a['velocity'], typeid=a['typeid'], n_types=4), want)
    assert same(hoomd.particle_moments(1.0, a['velocity'], 0.0, (0, 0, 0), typeid=a['typeid'], n_types=4), want)
    row = dict(mass=0.1, velocity=(0.1, -7.0, 1e10), energy=3.3, position=[1.5, 2.5, -0.3])
    full = dict((k, np.broadcast_to(np.asarray(v, np.float32), (n,) + np.shape(v)).copy()) for k, v in row.items())
    for name in row:
        mixed = dict(full)
        mixed[name] = row[name]          # converted to the arrays' float32, like the array's elements
        assert same(hoomd.particle_moments(typeid=a['typeid'], type0=1, n_types=2, **mixed),
                    hoomd.particle_moments(typeid=a['typeid'], type0=1, n_types=2, **full), name)
    # no array at all: N says how many, float64 rows
    rows = rng.integers(0, n, 777)
    full64 = dict((k, np.broadcast_to(np.asarray(v, np.float64), (n,) + np.shape(v)).copy()) for k, v in row.items())
    assert same(hoomd.particle_moments(N=n, **row), hoomd.particle_moments(**full64))
    assert same(hoomd.particle_moments(N=n, rows=rows, **row), hoomd.particle_moments(rows=rows, **full64))
    assert hoomd.particle_moments(None, None, N=12).mass.tolist() == [12.0]


def test_six_types_in_two_groups_and_the_total():
    rng = np.random.default_rng(5)
    n = 9000
    a = inputs(rng, n, np.float32)
    a['typeid'] = rng.integers(0, 7, n).astype(np.uint32)          # type 6 is none of the six
    types = ['a', 'b', 'c', 'd', 'e', 'f']
    got = hoomd.frame_moments(a, types=types)
    want = loop_moments_all(a, 6)
    assert same(got, want)
    assert got.count.shape == (6,) and got.other == int((a['typeid'] == 6).sum()) > 0
    total = got.total()
    assert total.count.tolist() == [int(got.count.sum())] and total.other == got.other
    acc = got.sums[0]
    for t in range(1, 6):
        acc = acc + got.sums[t]
    assert np.array_equal(total.sums[0].view(np.uint64), acc.view(np.uint64))
    one = hoomd.frame_moments(a, by_type=False)
    assert one.count.tolist() == [n] and one.other == 0 and one.total().mass[0] == one.mass[0]


def loop_moments_all(a, T):
    """One loop over all T types (the definition has no limit of four; a call has)."""
    parts = [loop_moments(a['mass'], a['velocity'], a['energy'], a['position'], a['typeid'], t, 1) for t in range(T)]
    return hoomd.Moments.concatenate(parts, len(a['mass']))


def test_frame_moments_over_a_selection_and_without_centre():
    rng = np.random.default_rng(6)
    n = 6000
    a = inputs(rng, n, np.float32)
    a['density'] = (1000 + 50 * rng.standard_normal(n)).astype(np.float32)
    types = ['fluid', 'wall', 'inlet', 'x', 'y']
    where = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
    cell = hoomd.domain_grid(2, 2, 1)[1]
    w = hoomd.where_rows(a, where, types)
    d = hoomd.domain_rows(a['position'], TRI, cell)
    floats = dict((k, a[k]) for k in ('mass', 'velocity', 'energy', 'position'))
    for kwargs, rows in ((dict(where=where), w), (dict(domain=cell, box=TRI), d),
                         (dict(where=where, domain=cell, box=TRI), np.intersect1d(w, d))):
        assert 0 < len(rows) < n
        got = hoomd.frame_moments(a, types=types, **kwargs)
        parts = [hoomd.particle_moments(typeid=a['typeid'], type0=t0, n_types=k, rows=rows, **floats)
                 for t0, k in ((0, 4), (4, 1))]
        assert same(got, hoomd.Moments.concatenate(parts, len(rows)), sorted(kwargs))
        assert got.other == 0 and int(got.count.sum()) == len(rows)
        assert same(hoomd.frame_moments(a, by_type=False, types=types, **kwargs),
                    hoomd.particle_moments(rows=rows, **floats))
    flat = hoomd.frame_moments(a, types=types, centre=False)
    assert not flat.first_moment.any() and np.array_equal(flat.momentum, hoomd.frame_moments(a, types=types).momentum)
    # a Frame: its own types, box and dimensions; missing attributes are the schema's defaults
    fr = hoomd.Frame()
    fr.configuration.box = TRI
    fr.particles.N = n
    fr.particles.types = types
    fr.particles.typeid, fr.particles.velocity, fr.particles.position = a['typeid'], a['velocity'], a['position']
    got = hoomd.frame_moments(fr, domain=cell)
    assert same(got, hoomd.frame_moments(dict(typeid=a['typeid'], velocity=a['velocity'], position=a['position']),
                                         types=types, domain=cell, box=TRI))
    assert got.mass.tolist() == got.count.astype(np.float64).tolist() and not got.internal.any()


def test_every_value_error():
    m, v = np.ones(8, np.float32), np.zeros((8, 3), np.float32)
    tid = np.zeros(8, np.uint32)
    bad = [
        (dict(mass=m.astype(np.float16), velocity=v), "float32 or float64"),
        (dict(mass=m.astype(np.int32), velocity=v), "float32 or float64"),
        (dict(mass=m.astype(np.float64), velocity=v), "one float type"),
        (dict(mass=m, velocity=v, energy=np.ones(8)), "one float type"),
        (dict(mass=m, velocity=np.zeros((8, 2), np.float32)), "N x 3"),
        (dict(mass=m, velocity=np.zeros((8, 3, 1), np.float32)), "N x 3 array or three values"),
        (dict(mass=m, velocity=(0.0, 1.0)), "N x 3 array or three values"),
        (dict(mass=m.reshape(8, 1), velocity=v), "N values or one value"),
        (dict(mass=m, velocity=v, energy=np.ones(7, np.float32)), "differ in their number of rows"),
        (dict(mass=m, velocity=v, position=np.zeros((9, 3), np.float32)), "differ in their number of rows"),
        (dict(mass=m, velocity=v, typeid=np.zeros(9, np.uint32)), "differ in their number of rows"),
        (dict(mass=m, velocity=v, N=9), "differ in their number of rows"),
        (dict(mass=m, velocity=v, typeid=tid, n_types=0), "1 to 4 types"),
        (dict(mass=m, velocity=v, typeid=tid, n_types=5), "1 to 4 types"),
        (dict(mass=m, velocity=v, n_types=2), "n_types must be 1"),
        (dict(mass=m, velocity=v, typeid=tid.astype(np.float32)), "uint32 or int32"),
        (dict(mass=m, velocity=v, typeid=tid.astype(np.int64)), "uint32 or int32"),
        (dict(mass=m, velocity=v, typeid=tid.reshape(8, 1)), "N values"),
        (dict(mass=m, velocity=v, typeid=tid, type0=-1), "type0"),
        (dict(mass=None, velocity=None), "N says how many"),
        (dict(mass=m, velocity=v, rows=[0, 8]), "outside the array"),
        (dict(mass=m, velocity=v, rows=[-1]), "outside the array"),
        (dict(mass=m, velocity=v, rows=[0.5]), "integer row indices"),
    ]
    for kwargs, message in bad:
        with pytest.raises(ValueError, match=message):
            hoomd.particle_moments(**kwargs)
    with pytest.raises(ValueError, match="by_type needs"):
        hoomd.frame_moments(dict(mass=m, velocity=v))
    with pytest.raises(ValueError, match="a domain needs box"):
        hoomd.frame_moments(dict(mass=m, velocity=v), by_type=False, domain=hoomd.domain_grid(2, 1, 1)[0])


def test_moments_has_slots_like_field_stats():
    got = hoomd.particle_moments(None, None, N=3)
    assert not hasattr(got, '__dict__') and 'count' in hoomd.Moments.__slots__
    assert got.count.dtype == np.int64 and got.bad.dtype == np.int64 and isinstance(got.other, int)
    assert got.momentum.shape == (1, 3) and got.first_moment.shape == (1, 3) and "Moments(" in repr(got)


# ---------------------------------------------------------------- the command line
def test_the_command_line_prints_the_conservation_table(tmp_path, capsys):
    path = str(tmp_path / "small.gsd")
    with hoomd.open(path, 'w') as t:
        for step, scale in ((0, 1.0), (5, 2.0)):
            fr = hoomd.Frame()
            fr.configuration.step = step
            fr.configuration.box = [8, 8, 8, 0, 0, 0]
            fr.particles.N = 4
            fr.particles.types = ['fluid', 'wall']
            fr.particles.typeid = np.array([0, 0, 1, 0], np.uint32)
            fr.particles.mass = np.array([2, 1, 4, 1], np.float32)
            fr.particles.velocity = np.array([[1, 0, 0], [0, 2, 0], [0, 0, 0], [0, 0, -2]], np.float32) * scale
            fr.particles.energy = np.array([0.5, 1, 0.25, 2], np.float32)
            fr.particles.position = np.array([[1, 1, 1], [-2, 0, 2], [0.5, 0.5, 0.5], [2, -2, 0]], np.float32)
            t.append(fr)
    assert pgsd_main(['info', path, '--moments', '--frame', '0']) == 0
    out = capsys.readouterr().out
    assert "conservation sums of frame 0:" in out
    lines = [' '.join(l.split()) for l in out.splitlines()]
    assert ("fluid count 3 bad 0 mass 4.0 momentum (2.0, 2.0, -2.0) kinetic 5.0 internal 4.0 "
            "centre of mass (0.5, 0.0, 1.0)") in lines
    assert ("wall count 1 bad 0 mass 4.0 momentum (0.0, 0.0, 0.0) kinetic 0.0 internal 1.0 "
            "centre of mass (0.5, 0.5, 0.5)") in lines
    assert ("total count 4 bad 0 mass 8.0 momentum (2.0, 2.0, -2.0) kinetic 5.0 internal 5.0 "
            "centre of mass (0.5, 0.25, 0.75)") in lines
    assert pgsd_main(['info', path, '--moments', '--types', 'wall']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "conservation sums of frame 1 (types wall):" in lines
    assert ("fluid count 0 bad 0 mass 0.0 momentum (0.0, 0.0, 0.0) kinetic 0.0 internal 0.0 "
            "centre of mass (nan, nan, nan)") in lines
    assert pgsd_main(['info', path, '--moments', '--all-frames']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "frame 0 step 0 count 4 bad 0 mass 8.0 momentum (2.0, 2.0, -2.0) kinetic 5.0 internal 5.0" in lines
    assert "frame 1 step 5 count 4 bad 0 mass 8.0 momentum (4.0, 4.0, -4.0) kinetic 20.0 internal 5.0" in lines
    assert os.path.exists(path)
