"""pgsd.hoomd.where_rows -- the numpy model that DEFINES a group predicate (read_frame_device(where=...),
select_where_device) -- against a row-by-row Python loop that restates the specification, and pgsd2vtu(where=...)
against subsetting a frame by hand.  No GPU."""
import math
import os

import numpy as np
import pytest

import pgsd.hoomd as hoomd
import pgsd.vtu as vtu

N = 777
SPECIAL = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 0.5]


def _arrays(seed=0):
    rng = np.random.default_rng(seed)
    a = {
        'typeid': rng.integers(0, 70, size=N).astype(np.uint32),         # some ids beyond the 64-bit mask
        'body': rng.integers(-3, 66, size=N).astype(np.int32),
        'image': rng.integers(-2, 3, size=(N, 3)).astype(np.int32),
        'density': rng.standard_normal(N).astype(np.float32),
        'mass': rng.uniform(0.5, 2.0, size=N).astype(np.float32),
        'velocity': rng.standard_normal((N, 3)).astype(np.float32),
        'position': rng.uniform(-3, 3, size=(N, 3)).astype(np.float32),
    }
    for name in ('density', 'velocity'):                                 # NaN, +-inf, +-0.0 and bounds hit exactly
        flat = a[name].reshape(-1)
        at = rng.choice(flat.size, size=200, replace=False)
        flat[at] = rng.choice(SPECIAL, size=200).astype(np.float32)
    a['typeid'][:3] = [0, 63, 64]
    a['body'][:4] = [-1, 0, 63, 64]
    return a


def _brute(arrays, terms):
    """terms: (name, column, 'range', lo, hi) or (name, column, 'set', members) -- the specification, row by row."""
    n = len(next(iter(arrays.values())))
    rows = []
    for i in range(n):
        ok = True
        for t in terms:
            x = arrays[t[0]].reshape(n, -1)[i, t[1]]
            if t[2] == 'set':
                ok = ok and 0 <= int(x) < 64 and int(x) in t[3]
            else:
                v = float(x)
                ok = ok and not math.isnan(v) and (t[3] is None or t[3] <= v) and (t[4] is None or v < t[4])
        if ok:
            rows.append(i)
    return np.array(rows, dtype=np.int32)


def _check(arrays, where, terms, types=None):
    got = hoomd.where_rows(arrays, where, types)
    want = _brute(arrays, terms)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    return got


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ranges_match_the_row_loop(seed):
    a = _arrays(seed)
    for lo, hi in [(0.0, 1.0), (-0.0, 0.5), (None, 0.0), (0.0, None), (None, None), (-np.inf, np.inf), (-1.0, 1.0),
                   (1.0, -1.0), (0.5, 0.5), (np.inf, None), (None, -np.inf)]:
        r = _check(a, {'density': (lo, hi)}, [('density', 0, 'range', lo, hi)])
        assert not np.isnan(a['density'][r]).any()
    _check(a, {'body': (-2, 3)}, [('body', 0, 'range', -2.0, 3.0)])
    _check(a, {'typeid': (10, None)}, [('typeid', 0, 'range', 10.0, None)])
    _check(a, {'mass': (1.0, 1.5)}, [('mass', 0, 'range', 1.0, 1.5)])


def test_half_open_edges_and_zeros():
    a = {'density': np.array([1.0, 2.0, np.nextafter(np.float32(2.0), np.float32(0)), -0.0, 0.0, np.nan, np.inf, -np.inf],
                             dtype=np.float32)}
    assert hoomd.where_rows(a, {'density': (1.0, 2.0)}).tolist() == [0, 2]          # lo kept, hi not
    assert hoomd.where_rows(a, {'density': (0.0, 1.0)}).tolist() == [3, 4]          # -0.0 >= 0.0
    assert hoomd.where_rows(a, {'density': (None, -0.0)}).tolist() == [7]           # neither zero is < -0.0
    assert hoomd.where_rows(a, {'density': (None, None)}).tolist() == [0, 1, 2, 3, 4, 6, 7]     # NaN is never kept
    assert hoomd.where_rows(a, {'density': (None, np.inf)}).tolist() == [0, 1, 2, 3, 4, 7]      # inf < inf is false
    assert hoomd.where_rows(a, {'density': (2.0, 1.0)}).tolist() == []
    assert hoomd.where_rows(a, {'density': (1.0, 1.0)}).tolist() == []
    assert hoomd.where_rows(a, {'density': (np.nan, None)}).tolist() == []


def test_sets_match_the_row_loop():
    a = _arrays(3)
    _check(a, {'typeid': [0, 63]}, [('typeid', 0, 'set', {0, 63})])
    assert {0, 1} <= set(hoomd.where_rows(a, {'typeid': [0, 63]}).tolist())
    assert 2 not in hoomd.where_rows(a, {'typeid': list(range(64))})                # id 64 matches no set
    r = _check(a, {'body': {0, 1, 63}}, [('body', 0, 'set', {0, 1, 63})])
    assert (a['body'][r] >= 0).all() and 1 in r and 2 in r
    r = _check(a, {'body': list(range(64))}, [('body', 0, 'set', set(range(64)))])
    assert 0 not in r and (a['body'][r] >= 0).all()                                 # body == -1 matches no set
    _check(a, {('image', 2): [0, 1, 2]}, [('image', 2, 'set', {0, 1, 2})])
    _check(a, {'typeid': []}, [('typeid', 0, 'set', set())])


def test_column_keys_type_sugar_empty_dict_and_four_terms():
    a = _arrays(4)
    _check(a, {('velocity', 2): (0.0, None)}, [('velocity', 2, 'range', 0.0, None)])
    _check(a, {('position', 1): (-1.0, 1.0)}, [('position', 1, 'range', -1.0, 1.0)])
    _check(a, {('density', 0): (0.0, None)}, [('density', 0, 'range', 0.0, None)])
    types = ['fluid', 'wall', 'inlet']
    r = _check(a, {'type': ['fluid', 'inlet']}, [('typeid', 0, 'set', {0, 2})], types)
    assert np.array_equal(r, hoomd.where_rows(a, {'typeid': [0, 2]}))
    assert np.array_equal(hoomd.where_rows(a, {}), np.arange(N))
    assert hoomd.where_rows(a, {}).dtype == np.int32
    where = {'typeid': list(range(0, 40)), 'density': (-1.0, 1.0), ('velocity', 2): (None, 0.5), 'body': (-2, 30)}
    r = _check(a, where, [('typeid', 0, 'set', set(range(40))), ('density', 0, 'range', -1.0, 1.0),
                          ('velocity', 2, 'range', None, 0.5), ('body', 0, 'range', -2.0, 30.0)])
    assert 0 < len(r) < N
    assert (np.diff(r) > 0).all()


@pytest.mark.parametrize("where, types", [
    ({'colour': (0, 1)}, None),                              # unknown attribute
    ({('velocity', 3): (0, 1)}, None),                       # column >= M
    ({('density', 1): (0, 1)}, None),
    ({'density': [0, 1]}, None),                             # a set on a float attribute
    ({('position', 0): {1}}, None),
    ({'typeid': [64]}, None),                                # members outside [0, 64)
    ({'body': [-1]}, None),
    ({'type': ['steam']}, ['fluid', 'wall']),                # unknown type name
    ({'type': ['fluid']}, None),
    ({'typeid': (0, 1), 'body': (0, 1), 'mass': (0, 1), 'density': (0, 1), 'energy': (0, 1)}, None),    # 5 terms
    ({'density': 1.0}, None),                                # neither a range nor a set
    ({'density': (0, 1, 2)}, None),
])
def test_value_errors(where, types):
    a = _arrays(5)
    a['energy'] = a['density']
    with pytest.raises(ValueError):
        hoomd.where_rows(a, where, types)


def test_pgsd2vtu_where_equals_subsetting_by_hand(tmp_path):
    rng = np.random.default_rng(7)
    n = 300
    path = str(tmp_path / "group.gsd")
    frames = []
    with hoomd.open(path, 'w') as t:
        for step in (0, 5):
            fr = hoomd.Frame()
            fr.configuration.step = step
            fr.particles.N = n
            fr.particles.types = ['fluid', 'wall', 'inlet']
            fr.particles.position = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
            fr.particles.typeid = rng.integers(0, 3, size=n).astype(np.uint32)
            fr.particles.density = rng.standard_normal(n).astype(np.float32)
            fr.particles.velocity = rng.standard_normal((n, 3)).astype(np.float32)
            t.append(fr)
            frames.append(fr)
    where = {'type': ['fluid', 'inlet'], 'density': (0.0, None)}
    files = vtu.pgsd2vtu(path, str(tmp_path / "out"), where=where)
    assert len(files) == 2
    for name, fr in zip(files, frames):
        p = fr.particles
        keep = np.flatnonzero(((p.typeid == 0) | (p.typeid == 2)) & (p.density >= 0.0))
        assert 0 < len(keep) < n
        got = vtu.read_vtu_arrays(name)
        assert np.array_equal(got['points'], p.position[keep])
        assert np.array_equal(got['typeid'], p.typeid[keep])
        assert np.array_equal(got['density'], p.density[keep])
        assert np.array_equal(got['velocity'], p.velocity[keep])
        assert np.array_equal(got['mass'], np.ones(len(keep), np.float32))      # a defaulted array is subset too
    # without where: unchanged, every particle
    full = vtu.pgsd2vtu(path, str(tmp_path / "full"))
    assert len(vtu.read_vtu_arrays(full[0])['points']) == n


def test_command_line_types_option(tmp_path, capsys):
    from pgsd.__main__ import main
    n = 50
    path = str(tmp_path / "cli.gsd")
    fr = hoomd.Frame()
    fr.particles.N = n
    fr.particles.types = ['fluid', 'wall']
    fr.particles.position = np.zeros((n, 3), np.float32)
    fr.particles.typeid = (np.arange(n) % 2).astype(np.uint32)
    with hoomd.open(path, 'w') as t:
        t.append(fr)
    assert main(['vtu', path, '-o', str(tmp_path / "cli"), '--types', 'wall']) == 0
    name = capsys.readouterr().out.split()[0]
    assert os.path.exists(name)
    assert np.array_equal(vtu.read_vtu_arrays(name)['typeid'], np.ones(n // 2, np.uint32))
    assert main(['vtu', path, '-o', str(tmp_path / "cli"), '--types', 'steam']) == 1
