"""The definition of the frame statistics (pgsd.hoomd.column_stats / frame_stats / FieldStats) on the host: the vectorised
model against a plain-loop restatement with an explicit tile, lane, step and tree, the special values by hand, norm2,
frame_stats over selections, every ValueError, and `python -m pgsd info --stats`.  The GPU reduction is compared with
this model in tests/test_gpu_frame_stats.py; everything here is exact: no tolerance anywhere."""
import math

import numpy as np
import pytest

import pgsd.hoomd as hoomd

LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 70_001]
DTYPES = [np.float32, np.float64, np.int32, np.uint32]
INF = float('inf')


def wide(rng, n, dtype=np.float32):
    """The generator of the issue: normal values scaled over 15 decades, so that the order of a sum shows."""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 12, n)).astype(dtype)


def values_of(rng, n, M, dtype):
    if np.dtype(dtype).kind == 'f':
        a = wide(rng, n * M, dtype).reshape(n, M)
    elif dtype is np.int32:
        a = rng.integers(-2 ** 31, 2 ** 31, size=(n, M), dtype=np.int64).astype(np.int32)
    else:
        a = rng.integers(0, 2 ** 32, size=(n, M), dtype=np.int64).astype(np.uint32)
    return a[:, 0].copy() if M == 1 else a


# ---------------------------------------------------------------- the restatement: one entry at a time
def loop_block_tree(p):
    assert len(p) == 256
    waves = []
    for w in range(4):
        q = list(p[64 * w:64 * w + 64])
        for h in (32, 16, 8, 4, 2, 1):
            for i in range(h):
                q[i] = q[i] + q[i + h]
        waves.append(q[0])
    return (waves[0] + waves[1]) + (waves[2] + waves[3])


def loop_sum(v):
    """v: Python floats, an entry that does not count already +0.0."""
    n = len(v)
    tile_sums = []
    for tile in range((n + 4095) // 4096):
        lanes = []
        for lane in range(256):
            s = 0.0
            for step in range(16):
                k = tile * 4096 + step * 256 + lane
                s = s + (v[k] if k < n else 0.0)
            lanes.append(s)
        tile_sums.append(loop_block_tree(lanes))
    lanes = []
    for t in range(256):
        s = 0.0
        for tile in range(t, len(tile_sums), 256):
            s = s + tile_sums[tile]
        lanes.append(s)
    return loop_block_tree(lanes)


def loop_stats(values, rows=None, norm2=False):
    """(count, nan, inf, min, max, sum) as lists of one entry per column."""
    a = np.asarray(values)
    a = a.reshape(len(a), a.shape[1] if a.ndim == 2 else 1)
    order = range(len(a)) if rows is None else [int(r) for r in rows]
    table = [[float(x) for x in a[r]] for r in order]       # float(): the exact conversion to float64
    if norm2:
        for row in table:
            row.append((row[0] * row[0] + row[1] * row[1]) + row[2] * row[2])
    C = a.shape[1] + (1 if norm2 else 0)
    out = [[], [], [], [], [], []]
    for c in range(C):
        n_nan = n_inf = 0
        lo, hi, finite = INF, -INF, []
        for row in table:
            x = row[c]
            if x != x:
                n_nan += 1
                finite.append(0.0)
                continue
            if x in (INF, -INF):
                n_inf += 1
            lo, hi = (x if x < lo else lo), (x if x > hi else hi)
            finite.append(0.0 if x in (INF, -INF) else x)
        for k, x in enumerate((len(table), n_nan, n_inf, lo, hi, loop_sum(finite))):
            out[k].append(x)
    return out


def same(stats, want):
    got = [stats.count, stats.nan, stats.inf, stats.min, stats.max, stats.sum]
    for g, w, name in zip(got, want, ('count', 'nan', 'inf', 'min', 'max', 'sum')):
        assert g.dtype == (np.int64 if name in ('count', 'nan', 'inf') else np.float64), name
        assert np.array_equal(g, np.array(w, dtype=g.dtype)), (name, g.tolist(), w)
    return True


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("M", [1, 3, 4])
def test_the_model_equals_the_plain_loop(dtype, M):
    for n in LENGTHS:
        rng = np.random.default_rng(1000 * M + n)
        a = values_of(rng, n, M, dtype)
        assert same(hoomd.column_stats(a), loop_stats(a)), n
        if n:
            rows = rng.integers(0, n, size=n + 3)           # unsorted, with repeats
            rows[1] = rows[0]
            assert same(hoomd.column_stats(a, rows), loop_stats(a, rows)), n
        assert same(hoomd.column_stats(a, []), loop_stats(a, [])), n


def test_the_input_can_tell_orders_apart():
    """The model's sum differs from numpy's pairwise sum of the same float64 values: an input whose sum does not depend
    on the order would let any reduction pass."""
    for n in (4096, 70_001):
        x = wide(np.random.default_rng(7), n)
        assert hoomd.column_stats(x).sum[0] != np.sum(x.astype(np.float64)), n
        assert hoomd.column_stats(x).sum[0] == loop_sum([float(v) for v in x]), n


def test_special_values_by_hand():
    denormal = np.float32(2.0 ** -140)
    x = np.array([1.5, np.nan, np.inf, -np.inf, -0.0, denormal, -2.5], np.float32)
    st = hoomd.column_stats(x)
    assert st.count.tolist() == [7] and st.nan.tolist() == [1] and st.inf.tolist() == [2]
    assert st.min.tolist() == [-INF] and st.max.tolist() == [INF]
    assert st.sum[0] == -1.0 and st.mean[0] == -0.25        # (2^-140 is far below the last bit of -1.0)
    d = hoomd.column_stats(np.array([denormal, -denormal, denormal, denormal], np.float32))
    assert d.min[0] == -2.0 ** -140 and d.max[0] == 2.0 ** -140 and d.sum[0] == 2.0 ** -139      # not flushed to zero
    # zeros of either sign: compared with ==, and a sum of them is +0.0
    z = hoomd.column_stats(np.array([-0.0, -0.0], np.float64))
    assert z.min[0] == 0.0 and z.max[0] == 0.0 and z.sum[0] == 0.0 and not math.copysign(1.0, z.sum[0]) < 0
    i = hoomd.column_stats(np.array([[-2 ** 31, 0], [2 ** 31 - 1, 7]], np.int32))
    assert i.min.tolist() == [-2.0 ** 31, 0.0] and i.max.tolist() == [2.0 ** 31 - 1, 7.0]
    assert i.sum.tolist() == [-1.0, 7.0] and i.nan.tolist() == i.inf.tolist() == [0, 0]
    u = hoomd.column_stats(np.array([2 ** 32 - 1, 2 ** 32 - 1, 1], np.uint32))
    assert u.max[0] == 2.0 ** 32 - 1 and u.min[0] == 1.0 and u.sum[0] == 2.0 ** 33 - 1 and u.mean[0] == (2.0 ** 33 - 1) / 3


def test_a_column_without_a_number():
    st = hoomd.column_stats(np.full((5, 3), np.nan, np.float32), norm2=True)
    assert st.count.tolist() == [5] * 4 and st.nan.tolist() == [5] * 4 and st.inf.tolist() == [0] * 4
    assert st.min.tolist() == [INF] * 4 and st.max.tolist() == [-INF] * 4 and st.sum.tolist() == [0.0] * 4
    assert np.isnan(st.mean).all()
    empty = hoomd.column_stats(np.zeros((0, 3), np.float64))
    assert empty.count.tolist() == [0] * 3 and empty.min.tolist() == [INF] * 3 and empty.max.tolist() == [-INF] * 3
    assert empty.sum.tolist() == [0.0] * 3 and np.isnan(empty.mean).all()
    only_inf = hoomd.column_stats(np.array([np.inf, -np.inf], np.float32))
    assert only_inf.inf.tolist() == [2] and only_inf.sum.tolist() == [0.0] and np.isnan(only_inf.mean[0])
    assert only_inf.min.tolist() == [-INF] and only_inf.max.tolist() == [INF]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_norm2_against_a_row_loop(dtype):
    rng = np.random.default_rng(3)
    for n in (1, 65, 4097):
        v = values_of(rng, n, 3, dtype)
        if n > 10:
            v[2, 1] = np.nan
            v[5] = [np.inf, 1.0, np.nan]
            v[7, 0] = -np.inf
            v[9] = [-0.0, 0.0, -0.0]
        rows = rng.integers(0, n, size=2 * n)
        assert same(hoomd.column_stats(v, norm2=True), loop_stats(v, norm2=True))
        assert same(hoomd.column_stats(v, rows, norm2=True), loop_stats(v, rows, norm2=True))
    # a float64 row whose square overflows counts as infinite; the association is (x*x + y*y) + z*z
    big = hoomd.column_stats(np.array([[1e200, 0.0, 0.0], [3.0, 4.0, 12.0]], np.float64), norm2=True)
    assert big.inf.tolist() == [0, 0, 0, 1] and big.max[3] == INF and big.min[3] == 169.0 and big.sum[3] == 169.0
    x, y, z = 1.0 + 2.0 ** -30, 2.0 ** -27, 1.0 - 2.0 ** -31
    one = hoomd.column_stats(np.array([[x, y, z]], np.float64), norm2=True)
    assert one.max[3] == (x * x + y * y) + z * z


def test_norm2_refusals():
    for bad in (np.zeros((4, 3), np.int32), np.zeros((4, 3), np.uint32), np.zeros((4, 4), np.float32),
                np.zeros((4, 2), np.float64), np.zeros(4, np.float32)):
        with pytest.raises(ValueError, match="norm2"):
            hoomd.column_stats(bad, norm2=True)


def test_every_value_error():
    ok = np.zeros((6, 3), np.float32)
    for bad in (ok.astype(np.float16), ok.astype(np.int64), ok.astype(np.uint8), ok.astype(np.int16), ok > 0):
        with pytest.raises(ValueError, match="float32, float64, int32 or uint32"):
            hoomd.column_stats(bad)
    with pytest.raises(ValueError, match="1 to 4 columns"):
        hoomd.column_stats(np.zeros((6, 5), np.float32))
    with pytest.raises(ValueError, match="1 to 4 columns"):
        hoomd.column_stats(np.zeros((6, 0), np.float32))
    with pytest.raises(ValueError, match="N or N x M"):
        hoomd.column_stats(np.zeros((6, 2, 2), np.float32))
    with pytest.raises(ValueError, match="N or N x M"):
        hoomd.column_stats(np.float32(1.0))
    for rows in ([6], [-1], [0, 2 ** 32]):
        with pytest.raises(ValueError, match="outside"):
            hoomd.column_stats(ok, rows)
    with pytest.raises(ValueError, match="integer"):
        hoomd.column_stats(ok, [0.5])
    arrays = {'position': ok, 'density': np.zeros(6, np.float32)}
    with pytest.raises(ValueError, match="not a per-particle attribute"):
        hoomd.frame_stats(arrays, ['speed'])
    with pytest.raises(ValueError, match="holds no 'velocity'"):
        hoomd.frame_stats(arrays, ['velocity'])
    with pytest.raises(ValueError, match="box"):
        hoomd.frame_stats(arrays, ['density'], domain=hoomd.domain_grid(2, 1, 1)[0])
    with pytest.raises(ValueError, match="position"):
        hoomd.frame_stats({'density': arrays['density']}, ['density'], domain=hoomd.domain_grid(2, 1, 1)[0],
                          box=[4, 4, 4, 0, 0, 0])
    with pytest.raises(ValueError, match="unknown particle type"):
        hoomd.frame_stats(arrays, ['density'], where={'type': ['steam']}, types=['fluid'])
    with pytest.raises(ValueError, match="holds floats"):
        hoomd.frame_stats(arrays, ['density'], where={'density': [1]})


def _frame(rng, n):
    fr = hoomd.Frame()
    fr.configuration.box = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
    fr.particles.N = n
    fr.particles.types = ['fluid', 'wall', 'inlet']
    fr.particles.position = rng.uniform(-3.0, 3.0, size=(n, 3)).astype(np.float32)
    fr.particles.velocity = wide(rng, 3 * n).reshape(n, 3)
    fr.particles.density = (1000.0 + 50.0 * rng.standard_normal(n)).astype(np.float32)
    fr.particles.typeid = rng.integers(0, 3, size=n).astype(np.uint32)
    fr.particles.image = rng.integers(-2, 3, size=(n, 3)).astype(np.int32)
    return fr


def test_frame_stats_is_column_stats_over_the_selection():
    rng = np.random.default_rng(5)
    n = 9000
    fr = _frame(rng, n)
    fr.particles.velocity[17] = np.nan
    p = fr.particles
    arrays = hoomd._particle_arrays(p)
    fields = ['position', 'velocity', 'density', 'typeid', 'image']
    where = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
    cell = hoomd.domain_grid(2, 2, 1)[1]
    w_rows = hoomd.where_rows(arrays, where, p.types)
    d_rows = hoomd.domain_rows(p.position, fr.configuration.box, cell)
    both = np.array(sorted(set(w_rows.tolist()) & set(d_rows.tolist())), dtype=np.int64)
    assert 0 < len(both) < min(len(w_rows), len(d_rows))
    for kwargs, rows in (({}, None), ({'where': where}, w_rows), ({'domain': cell}, d_rows),
                         ({'where': where, 'domain': cell}, both)):
        got = hoomd.frame_stats(fr, fields, **kwargs)
        assert list(got) == fields
        for name in fields:
            a = getattr(p, name)
            want = hoomd.column_stats(a, rows, norm2=name in ('position', 'velocity'))
            for q in hoomd.FieldStats.__slots__:
                assert np.array_equal(getattr(got[name], q), getattr(want, q)), (name, q)
            assert len(got[name].count) == {'position': 4, 'velocity': 4, 'density': 1, 'typeid': 1, 'image': 3}[name]
        # the same through a dict of arrays
        again = hoomd.frame_stats(arrays, ['velocity'], types=p.types, box=fr.configuration.box, **kwargs)
        assert np.array_equal(again['velocity'].sum, got['velocity'].sum)
    assert hoomd.frame_stats(fr, ['velocity'])['velocity'].nan.tolist() == [1, 1, 1, 1]
    # the default fields, and one name as a string
    assert list(hoomd.frame_stats({'density': p.density}, 'density')) == ['density']


def test_the_trajectory_method_reads_the_frame(tmp_path):
    rng = np.random.default_rng(6)
    fr = _frame(rng, 300)
    path = str(tmp_path / "t.gsd")
    with hoomd.open(path, 'w') as t:
        t.append(fr)
    with hoomd.open(path, 'r') as t:
        got = t.frame_stats(0, ['velocity', 'mass'], where={'type': ['wall']})
        want = hoomd.frame_stats(t[0], ['velocity', 'mass'], where={'type': ['wall']})
    rows = np.flatnonzero(fr.particles.typeid == 1)
    assert np.array_equal(got['velocity'].sum, hoomd.column_stats(fr.particles.velocity, rows, norm2=True).sum)
    assert np.array_equal(got['velocity'].sum, want['velocity'].sum)
    assert got['mass'].min.tolist() == got['mass'].max.tolist() == [1.0] and got['mass'].sum.tolist() == [float(len(rows))]


# ---------------------------------------------------------------- the command line
def test_info_stats_prints_literal_numbers(tmp_path, capsys):
    from pgsd.__main__ import main
    path = str(tmp_path / "cli.gsd")
    with hoomd.open(path, 'w') as t:
        for step in range(3):
            fr = hoomd.Frame()
            fr.configuration.step = 10 * step
            fr.particles.N = 4
            fr.particles.types = ['fluid', 'wall']
            fr.particles.typeid = np.array([0, 1, 0, 1], np.uint32)
            fr.particles.position = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, -3]], np.float32)
            fr.particles.velocity = np.array([[3, 4, 0], [0, 0, 0], [1, 2, 2], [6, 8, 0]], np.float32) * (step + 1)
            fr.particles.density = np.array([1000.0, 1002.0, 998.0, 1004.0], np.float32)
            if step == 2:
                fr.particles.density[0] = np.nan
                fr.particles.velocity[2, 1] = np.inf
            t.append(fr)
    assert main(['info', path, '--stats', '--frame', '0', '--fields', 'velocity,density']) == 0
    out = capsys.readouterr().out
    assert "statistics of frame 0:" in out
    assert "  velocity     0  count 4  nan 0  inf 0  min 0.0  max 6.0  mean 2.5" in out
    assert "  velocity     1  count 4  nan 0  inf 0  min 0.0  max 8.0  mean 3.5" in out
    assert "  velocity     2  count 4  nan 0  inf 0  min 0.0  max 2.0  mean 0.5" in out
    assert "  velocity     max norm 10.0" in out
    assert "  density      0  count 4  nan 0  inf 0  min 998.0  max 1004.0  mean 1001.0" in out
    assert "position" not in out.split("statistics of frame 0:")[1]
    # the particles of one type; the last frame by default, whose NaN and infinity are counted and left out of the mean
    assert main(['info', path, '--stats', '--types', 'fluid']) == 0
    out = capsys.readouterr().out
    assert "statistics of frame 2 (types fluid):" in out
    assert "  density      0  count 2  nan 1  inf 0  min 998.0  max 998.0  mean 998.0" in out
    assert "  velocity     1  count 2  nan 0  inf 1  min 12.0  max inf  mean 12.0" in out
    assert "  velocity     max norm inf" in out
    assert "  position     max norm 2.0" in out
    assert "  pressure     0  count 2  nan 0  inf 0  min 0.0  max 0.0  mean 0.0" in out
    # the blow-up scan
    assert main(['info', path, '--stats', '--all-frames', '--fields', 'velocity,density']) == 0
    lines = [l.split() for l in capsys.readouterr().out.splitlines() if l.startswith("  frame ")]
    assert [(l[1], l[3], l[5], l[8]) for l in lines] == [('0', '0', '0', '10.0'), ('1', '10', '0', '20.0'),
                                                          ('2', '20', '2', 'inf')]
    assert main(['info', path, '--stats', '--all-frames', '--types', 'wall', '--fields', 'density']) == 0
    lines = [l.split() for l in capsys.readouterr().out.splitlines() if l.startswith("  frame ")]
    assert [(l[5], l[8]) for l in lines] == [('0', '10.0'), ('0', '20.0'), ('0', '30.0')]
    assert main(['info', path, '--stats', '--types', 'steam']) == 1
    assert "unknown particle type" in capsys.readouterr().err
    assert main(['info', path, '--stats', '--fields', 'speed']) == 1
