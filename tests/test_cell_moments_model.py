"""Cell fields, the host model: pgsd.hoomd.cell_offsets / cell_moments / frame_cell_moments / CellMoments and
`info --cells`.  The model is the definition the GPU reduction must equal bit for bit (tests/test_gpu_cell_moments.py),
so it is itself checked against a plain Python loop that states piece, lane, step and tree explicitly.  The loop also
takes the mutations of the definition that the cases must tell apart; the layouts and the loop are shared with the GPU
module."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

CELL_LENGTHS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 70_001]
TRI = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
NAMES = ('count', 'bad', 'mass', 'momentum', 'kinetic', 'internal', 'first_moment')
INPUTS = ('mass', 'velocity', 'energy', 'position')
SCHEMA_ROW = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
# a default row whose values float32 holds exactly and that is nothing like the schema's
ROW = [0.375, 3.0, -7.0, 1.5 * 2.0 ** 30, -2.5, 1.5, 2.5, -0.3125]
DENORMAL = np.float32(2.0 ** -140)


def wide(rng, n, dtype=np.float32):
    """Normal values scaled over 15 decades: an input whose sum depends on the order (tests/test_gpu_moments.py)."""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 12, n)).astype(dtype)


def inputs(rng, n, dtype):
    return dict(mass=np.abs(wide(rng, n, dtype)) + dtype(0.5), velocity=wide(rng, 3 * n, dtype).reshape(n, 3),
                energy=wide(rng, n, dtype), position=rng.uniform(-3, 3, (n, 3)).astype(dtype))


# rows 1 .. 8 of an input made by special_rows: a NaN mass, an infinite velocity on a zero mass, -0.0, a denormal, a
# kinetic term that overflows alone (float64: 1e200 squared; float32 values are exact in float64, so there an infinite
# velocity stands in), an infinite energy, a NaN position, an infinite mass
SPECIAL = (1, 2, 3, 4, 5, 6, 7, 8)


def special_rows(a, dtype):
    big = 1e200 if dtype is np.float64 else np.inf
    a['mass'][1] = np.nan
    a['mass'][2], a['velocity'][2, 2] = 0.0, np.inf
    a['mass'][3] = -0.0
    a['mass'][4] = DENORMAL
    a['velocity'][5, 0] = big
    a['energy'][6] = -np.inf
    a['position'][7, 1] = np.nan
    a['mass'][8] = np.inf
    return a


def cells_of(lengths, nowhere=0):
    """The sorted id list of cells with these lengths, then `nowhere` entries of the id len(lengths)."""
    ids = np.repeat(np.arange(len(lengths) + 1), list(lengths) + [nowhere])
    return ids.astype(np.int64)


def same(got, want, what=None):
    """Integers equal, sums bit for bit."""
    assert got.nowhere == want.nowhere, (what, got.nowhere, want.nowhere)
    for name in NAMES:
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.dtype == np.float64:
            bad = np.flatnonzero((g.view(np.uint64) != w.view(np.uint64)).reshape(len(g), -1).any(axis=1))
            assert bad.size == 0, (what, name, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())
        else:
            assert np.array_equal(g, w), (what, name)
    return True


# ---------------------------------------------------------------- the definition as a loop
def nine(arrays, rows, defaults=None, dtype=np.float64):
    """The nine float64 values per list entry, stated again: numpy's elementwise float64 products, no fused
    multiply-add.  arrays[name] None: the default row, converted to the arrays' element type first."""
    d = np.asarray(SCHEMA_ROW if defaults is None else defaults).astype(dtype).astype(np.float64)
    n = len(rows)

    def col(name, c, at):
        if arrays.get(name) is None:
            return np.full(n, d[at + c])
        a = np.asarray(arrays[name])
        return (a if a.ndim == 1 else a[:, c])[rows].astype(np.float64)

    m, e = col('mass', 0, 0), col('energy', 0, 4)
    v = [col('velocity', c, 1) for c in range(3)]
    x = [col('position', c, 5) for c in range(3)]
    with np.errstate(all='ignore'):
        return ([m] + [m * v[c] for c in range(3)] + [(0.5 * m) * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), m * e]
                + [m * x[c] for c in range(3)])


def piece_sum(p, piece=1024, walk='strided'):
    """One piece: 64 lanes, each adds its entries in step order to +0.0; then the wave tree."""
    steps = piece // 64
    lanes = []
    for lane in range(64):
        acc = 0.0
        for step in range(steps):
            i = lane + 64 * step if walk == 'strided' else lane * steps + step
            acc = acc + (p[i] if i < len(p) else 0.0)
        lanes.append(acc)
    for h in (32, 16, 8, 4, 2, 1):
        for i in range(h):
            lanes[i] = lanes[i] + lanes[i + h]
    return lanes[0]


def loop_cells(values, cell, n_cells, quantities=range(9), piece=1024, walk='strided', origin='cell', long='sequence',
               skip=True, bound='lower'):
    """Per cell and quantity the sum as the definition words it, entry by entry; the keyword arguments are the
    mutations.  Returns (count, bad, nowhere, sums) with sums[c][q] for q in `quantities`."""
    n = len(cell)
    order = sorted(range(n), key=lambda k: int(cell[k]))          # (stable: list order inside a cell)
    members = [[] for _ in range(n_cells + 2)]
    first = [0] * (n_cells + 2)
    for at, k in enumerate(order):
        if not members[int(cell[k])]:
            first[int(cell[k])] = at
        members[int(cell[k])].append(k)
    fin = [np.isfinite(v) for v in values]
    count, bad, sums = [], [], []
    for c in range(n_cells):
        ks = members[c if bound == 'lower' else c + 1]              # (an upper bound hands cell c the next cell's run)
        start = first[c if bound == 'lower' else c + 1]
        count.append(len(ks))
        bad.append(sum(1 for k in ks if not all(f[k] for f in fin)))
        row = []
        for q in quantities:
            seq = [float(values[q][k]) if (fin[q][k] or not skip) else 0.0 for k in ks]
            if origin == 'cell':
                cuts = list(range(0, len(seq), piece))
            else:                                                   # pieces counted from the slab's start
                cuts = sorted(set([0] + [s - start for s in range(start - start % piece + piece, start + len(seq), piece)]))
            parts = [piece_sum(seq[a:b], piece, walk) for a, b in zip(cuts, cuts[1:] + [len(seq)])] if seq else []
            if long == 'sequence':
                total = 0.0
                for p in parts:
                    total = total + p
            else:
                while len(parts) > 1:
                    parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
                total = 0.0 + parts[0] if parts else 0.0
            row.append(total)
        sums.append(row)
    return count, bad, len(members[n_cells]), sums


MUTATIONS = {'piece length 4096': dict(piece=4096), 'lane walk contiguous': dict(walk='contiguous'),
             'pieces from the slab': dict(origin='slab'), 'long cell by a tree': dict(long='tree'),
             'non-finite not skipped': dict(skip=False), 'default ignored': dict(defaults=None),
             'upper bound': dict(bound='upper')}


def mutation_differs(name, arrays, rows, cell, n_cells, defaults, dtype, quantity):
    """Does the mutated loop give another bit pattern than the model for one of `quantity` in some cell of this case?"""
    kw = dict(MUTATIONS[name])
    values = nine(arrays, rows, kw.pop('defaults', defaults), dtype)
    _, _, _, sums = loop_cells(values, cell, n_cells, quantities=quantity, **kw)
    want = hoomd.cell_moments(*[arrays.get(k) if arrays.get(k) is not None else dict(zip(INPUTS, split(defaults)))[k]
                                for k in INPUTS], cell=cell, n_cells=n_cells, rows=rows, N=len_of(arrays))
    return any(np.float64(sums[c][i]).view(np.uint64) != want.sums[c, q].view(np.uint64) for c in range(n_cells)
               for i, q in enumerate(quantity))


def split(defaults):
    d = SCHEMA_ROW if defaults is None else defaults
    return d[0], d[1:4], d[4], d[5:8]


def len_of(arrays):
    return next(len(a) for a in arrays.values() if a is not None)


def check_against_the_loop(arrays, rows, cell, n_cells, defaults, dtype, what):
    given = dict(zip(INPUTS, split(defaults)))
    got = hoomd.cell_moments(*[arrays[k] if arrays.get(k) is not None else given[k] for k in INPUTS], cell=cell,
                             n_cells=n_cells, rows=rows, N=len_of(arrays))
    every = np.arange(len_of(arrays)) if rows is None else np.asarray(rows)
    count, bad, nowhere, sums = loop_cells(nine(arrays, every, defaults, dtype), cell, n_cells)
    assert got.count.tolist() == count and got.bad.tolist() == bad and got.nowhere == nowhere, what
    assert np.array_equal(got.sums.view(np.uint64), np.array(sums, dtype=np.float64).reshape(n_cells, 9).view(np.uint64)), what
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_model_equals_the_loop_at_every_cell_length(dtype):
    """Cells of 0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049 and 70 001 entries, interleaved in the list; the
    sequential sum tells the orders apart."""
    rng = np.random.default_rng(5)
    sorted_ids = cells_of(CELL_LENGTHS, nowhere=77)
    n = len(sorted_ids)
    cell = sorted_ids[rng.permutation(n)]                          # any order: the model sorts stably
    a = special_rows(inputs(rng, n, dtype), dtype)
    got = check_against_the_loop(a, None, cell, len(CELL_LENGTHS), None, dtype, dtype.__name__)
    assert got.count.tolist() == CELL_LENGTHS and got.nowhere == 77 and got.bad.sum() >= 5
    assert got.sums[0].view(np.uint64).tolist() == [0] * 9         # +0.0 for a cell without entries
    q = nine(a, np.arange(n), None, dtype)[1]
    seq = np.bincount(cell, weights=np.where(np.isfinite(q), q, 0.0), minlength=len(CELL_LENGTHS) + 1)[:-1]
    assert (seq != got.momentum[:, 0]).sum() >= 1


def test_an_unsorted_cell_array_with_repeats_in_rows():
    rng = np.random.default_rng(6)
    a = special_rows(inputs(rng, 500, np.float32), np.float32)
    rows = rng.integers(0, 500, size=3000)
    rows[:9] = np.arange(9)
    cell = rng.integers(0, 8, size=3000)                           # 7 cells and nowhere
    got = check_against_the_loop(a, rows, cell, 7, None, np.float32, 'repeats')
    assert got.nowhere == (cell == 7).sum() and int(got.count.sum()) + got.nowhere == 3000
    # the same entries listed in cell order give the same sums: the order is the cell's own
    perm = np.argsort(cell, kind='stable')
    again = hoomd.cell_moments(a['mass'], a['velocity'], a['energy'], a['position'], cell=cell[perm], n_cells=7, rows=rows[perm])
    assert same(again, got)


def test_nowhere_one_cell_and_more_cells_than_entries():
    rng = np.random.default_rng(7)
    a = inputs(rng, 65, np.float64)
    args = [a[k] for k in INPUTS]
    got = hoomd.cell_moments(*args, cell=np.full(65, 4), n_cells=4)
    assert got.nowhere == 65 and got.count.tolist() == [0] * 4 and not got.sums.view(np.uint64).any()
    check_against_the_loop(a, None, np.zeros(65, np.int64), 1, None, np.float64, 'one cell')
    cell = rng.permutation(5000)[:65]
    got = check_against_the_loop(a, None, cell, 5000, None, np.float64, 'sparse')
    assert got.count.sum() == 65 and got.count.max() == 1
    assert np.array_equal(got.mass[cell].view(np.uint64), a['mass'].view(np.uint64))
    big = hoomd.cell_moments(*args, cell=cell * 200, n_cells=2 ** 20)
    assert big.count.shape == (2 ** 20,) and np.array_equal(big.mass[cell * 200], a['mass'])


def test_special_values_by_hand():
    nan, inf = np.nan, np.inf
    mass = np.array([nan, 0.0, -0.0, 2.0 ** -1060, 2.0, 3.0])
    vel = np.array([[1, 1, 1], [inf, 0, 0], [1, 2, 3], [1, 0, 0], [1e200, 0, 0], [1, 2, 2]], np.float64)
    got = hoomd.cell_moments(mass, vel, np.array([1.0, 1, 1, 1, 1, 2]), None, cell=[0, 0, 1, 1, 2, 2], n_cells=3)
    assert got.count.tolist() == [2, 2, 2] and got.bad.tolist() == [2, 0, 1] and got.nowhere == 0
    # cell 0: the NaN mass poisons every value of its entry; 0 * inf is NaN but the zero mass itself is summed
    assert got.mass[0] == 0.0 and not np.signbit(got.mass[0]) and got.momentum[0].tolist() == [0.0, 0.0, 0.0]
    # cell 1: -0.0 and a denormal: -0.0 + denormal, sums never -0.0
    assert got.mass[1] == 2.0 ** -1060 and got.momentum[1].tolist() == [2.0 ** -1060, 0.0, 0.0]
    assert not np.signbit(got.momentum[1]).any() and got.kinetic[1] == 0.5 * 2.0 ** -1060
    # cell 2: the kinetic term of entry 4 overflows alone; its momentum is summed
    assert got.kinetic[2] == 13.5 and got.momentum[2].tolist() == [2e200 + 3.0, 6.0, 6.0] and got.mass[2] == 5.0
    assert got.internal.tolist() == [0.0, 2.0 ** -1060, 8.0]


def test_default_rows_and_none():
    rng = np.random.default_rng(8)
    for dtype in (np.float32, np.float64):
        a = inputs(rng, 300, dtype)
        cell = rng.integers(0, 4, size=300)
        for absent in ([0], [1], [2], [3], [0, 1, 2, 3]):
            part = dict((k, None if i in absent else a[k]) for i, k in enumerate(INPUTS))
            if len(absent) == 4:
                got = hoomd.cell_moments(*split(ROW), cell=cell, n_cells=3, N=300)
                count, bad, nowhere, sums = loop_cells(nine(part, np.arange(300), ROW, np.float64), cell, 3)
                assert got.count.tolist() == count and np.array_equal(got.sums, np.array(sums))
            else:
                check_against_the_loop(part, None, cell, 3, ROW, dtype, absent)
                check_against_the_loop(part, None, cell, 3, None, dtype, absent)
    got = hoomd.cell_moments(None, None, cell=[0, 1, 1], n_cells=2, N=3)
    assert got.mass.tolist() == [1.0, 2.0] and not got.momentum.any() and got.bad.tolist() == [0, 0]


def test_cell_offsets_against_a_loop_and_its_refusals():
    rng = np.random.default_rng(9)
    for n_cells, n in ((1, 0), (1, 5), (7, 0), (7, 100), (5000, 300)):
        cell = np.sort(rng.integers(0, n_cells + 1, size=n))
        offs = hoomd.cell_offsets(cell, n_cells)
        assert offs.dtype == np.int64 and offs.shape == (n_cells + 2,) and offs[-1] == n
        want = [sum(1 for v in cell if v < c) for c in range(n_cells + 2)] if n_cells < 100 else \
            np.concatenate(([0], np.cumsum(np.bincount(cell, minlength=n_cells + 1)))).tolist()
        assert offs.tolist() == want
    for cell, n_cells, message in (([0, 2, 1], 3, "descend"), ([0, 4], 3, "outside"), ([-1, 0], 3, "outside"),
                                   ([0.5], 3, "integer"), ([0], 0, "1 to 2\\^20"), ([0], 2 ** 20 + 1, "1 to 2\\^20")):
        with pytest.raises(ValueError, match=message):
            hoomd.cell_offsets(cell, n_cells)
    assert hoomd.cell_offsets([0, 3, 3], 3).tolist() == [0, 1, 1, 1, 3]          # (3 is nowhere)


def test_what_cell_moments_refuses():
    m, v = np.ones(4, np.float32), np.ones((4, 3), np.float32)
    for kwargs, message in ((dict(cell=[0, 0, 0], n_cells=2), "one id per list entry"),
                            (dict(cell=[0, 0, 0, 3], n_cells=2), "outside"),
                            (dict(cell=[0, 0, 0, 0], n_cells=0), "1 to 2\\^20"),
                            (dict(cell=None, n_cells=2), "one cell id per entry"),
                            (dict(cell=[0, 1], n_cells=2, rows=[0, 9]), "outside the array"),
                            (dict(cell=[0.0, 1.0, 1.0, 1.0], n_cells=2), "integer")):
        with pytest.raises(ValueError, match=message):
            hoomd.cell_moments(m, v, **kwargs)
    with pytest.raises(ValueError, match="not float32 and float64 mixed"):
        hoomd.cell_moments(m, v.astype(np.float64), cell=[0] * 4, n_cells=1)


def test_cell_moments_has_slots_and_its_properties():
    got = hoomd.cell_moments(np.array([2.0, 0.0, 4.0]), np.array([[1.0, 0, 0], [0, 0, 0], [0, 2, 0]]), None,
                             np.array([[1.0, 1, 1], [0, 0, 0], [2, 2, 2]]), cell=[0, 1, 5], n_cells=6)
    assert not hasattr(got, '__dict__') and "CellMoments(" in repr(got)
    assert got.count.dtype == np.int64 and got.bad.dtype == np.int64 and isinstance(got.nowhere, int)
    assert got.mean_velocity[0].tolist() == [1.0, 0, 0] and got.centre_of_mass[5].tolist() == [2.0, 2, 2]
    assert np.isnan(got.mean_velocity[1]).all() and np.isnan(got.centre_of_mass[2]).all()
    with pytest.raises(ValueError, match="cell volume"):
        got.density
    with pytest.raises(ValueError, match="grid"):
        got.as_grid('mass')
    got.grid, got.cell_volume = (3, 2, 1), 0.5
    assert got.density.tolist() == [4.0, 0, 0, 0, 0, 8.0] and got.as_grid('mass').shape == (1, 2, 3)
    assert got.as_grid('momentum').shape == (1, 2, 3, 3) and got.as_grid('mass')[0, 1, 2] == 4.0


# ---------------------------------------------------------------- frames
def _arrays(rng, n, dimensions=3):
    a = inputs(rng, n, np.float32)
    if dimensions == 2:
        a['position'][:, 2] = 0.0
    a['typeid'] = rng.integers(0, 3, size=n).astype(np.uint32)
    a['density'] = (1000.0 + 50.0 * rng.standard_normal(n)).astype(np.float32)
    a['position'][5, 0] = np.nan                                   # nowhere
    return a


def test_frame_cell_moments_over_selections():
    rng = np.random.default_rng(10)
    a = _arrays(rng, 3001)
    types = ['fluid', 'wall', 'inlet']
    where = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
    domain = hoomd.domain_grid(2, 1, 1)[0]
    w_rows = hoomd.where_rows(a, where, types)
    d_rows = hoomd.domain_rows(a['position'], TRI, domain)
    for kwargs, rows in ((dict(), np.arange(3001)), (dict(where=where), w_rows), (dict(domain=domain), d_rows),
                         (dict(where=where, domain=domain), np.intersect1d(w_rows, d_rows))):
        got = hoomd.frame_cell_moments(a, (4, 3, 2), types=types, box=TRI, **kwargs)
        cell = hoomd.cell_ids(a['position'][rows], TRI, (4, 3, 2))
        want = hoomd.cell_moments(a['mass'], a['velocity'], a['energy'], a['position'], cell=cell, n_cells=24, rows=rows)
        assert same(got, want, kwargs) and got.grid == (4, 3, 2) and int(got.count.sum()) + got.nowhere == len(rows)
        assert got.cell_volume == 4.0 * 4.0 * 2.0 / 24
    assert hoomd.frame_cell_moments(a, (4, 3, 2), box=TRI).nowhere == 1
    off = hoomd.frame_cell_moments(a, (4, 3, 2), box=TRI, centre=False)
    assert not off.first_moment.any() and np.array_equal(off.mass, hoomd.frame_cell_moments(a, (4, 3, 2), box=TRI).mass)
    for cells, message in (((1024, 1024, 2), "at most 2\\^20"), ((0, 1, 1), "each 1 to"), ((2, 2), "three counts")):
        with pytest.raises(ValueError, match=message):
            hoomd.frame_cell_moments(a, cells, box=TRI)
    with pytest.raises(ValueError, match="needs the box"):
        hoomd.frame_cell_moments(a, (2, 2, 2))
    # no position: every row in the origin's cell
    bare = dict(velocity=a['velocity'], mass=a['mass'])
    got = hoomd.frame_cell_moments(bare, (2, 2, 2), box=TRI)
    origin = int(hoomd.cell_ids(np.zeros((1, 3), np.float32), TRI, (2, 2, 2))[0])
    assert got.count[origin] == 3001 and got.count.sum() == 3001


def test_frame_cell_moments_in_two_dimensions_and_of_a_frame():
    rng = np.random.default_rng(11)
    box = np.array([4.0, 4.0, 1.0, 0.5, 0.0, 0.0], np.float32)
    fr = hoomd.Frame()
    fr.configuration.box, fr.configuration.dimensions = box, 2
    a = _arrays(rng, 901, 2)
    fr.particles.N, fr.particles.types = 901, ['fluid', 'wall', 'inlet']
    for name in ('position', 'velocity', 'mass', 'energy', 'typeid'):
        setattr(fr.particles, name, a[name])
    got = hoomd.frame_cell_moments(fr, (5, 4, 1), where={'type': ['wall']})
    rows = np.flatnonzero(a['typeid'] == 1)
    cell = hoomd.cell_ids(a['position'][rows], box, (5, 4, 1), 2)
    assert same(got, hoomd.cell_moments(a['mass'], a['velocity'], a['energy'], a['position'], cell=cell, n_cells=20, rows=rows))
    assert got.cell_volume == 16.0 / 20 and got.as_grid('count').shape == (1, 4, 5)
    with pytest.raises(ValueError, match="cz == 1"):
        hoomd.frame_cell_moments(fr, (5, 4, 2))


def test_density_in_a_triclinic_box():
    """Equal cells in fractional coordinates are equal in volume: a uniform lattice in fractions has the same density
    in every cell, Lx * Ly * Lz / n_cells being the cell's volume whatever the tilt."""
    g = (np.arange(8) + 0.5) / 8 - 0.5
    f = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    Lx, Ly, Lz, xy, xz, yz = [float(v) for v in TRI]
    pos = np.stack([f[:, 0] * Lx + f[:, 1] * xy * Ly + f[:, 2] * xz * Lz, f[:, 1] * Ly + f[:, 2] * yz * Lz, f[:, 2] * Lz], axis=1)
    got = hoomd.frame_cell_moments(dict(position=pos, mass=np.full(512, 0.25)), (2, 2, 2), box=TRI)
    assert got.count.tolist() == [64] * 8 and got.cell_volume == 4.0
    assert got.density.tolist() == [64 * 0.25 / 4.0] * 8


# ---------------------------------------------------------------- mutations
# (cell lengths, quantities) of a small case per mutation that the model must tell from the mutated loop
MUTATION_CASES = {'piece length 4096': ([1500, 3], range(9)), 'lane walk contiguous': ([300, 3], range(9)),
                  'pieces from the slab': ([500, 1500], range(9)), 'long cell by a tree': ([3300, 2], range(9)),
                  'non-finite not skipped': ([70, 3], [0]), 'default ignored': ([70, 3], [0]), 'upper bound': ([70, 3], [0])}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_each_mutation_is_told_apart(name):
    rng = np.random.default_rng(12)
    lengths, quantity = MUTATION_CASES[name]
    cell = cells_of(lengths)
    a = special_rows(inputs(rng, len(cell), np.float64), np.float64)
    if name == 'default ignored':
        a['mass'] = None
    assert mutation_differs(name, a, np.arange(len(cell)), cell, len(lengths), ROW, np.float64, quantity)
    # ... and the loop without the mutation agrees, so the difference is the mutation's
    MUTATIONS['none'] = {}
    try:
        assert not mutation_differs('none', a, np.arange(len(cell)), cell, len(lengths), ROW, np.float64, quantity)
    finally:
        del MUTATIONS['none']


# ---------------------------------------------------------------- the command line
def test_the_command_line_prints_the_cell_summary(tmp_path, capsys):
    path = str(tmp_path / "small.gsd")
    with hoomd.open(path, 'w') as t:
        fr = hoomd.Frame()
        fr.configuration.box = [8, 8, 8, 0, 0, 0]
        fr.particles.N = 5
        fr.particles.types = ['fluid', 'wall']
        fr.particles.typeid = np.array([0, 0, 1, 0, 0], np.uint32)
        fr.particles.mass = np.array([2, 1, 4, 1, 1], np.float32)
        fr.particles.velocity = np.array([[0, 0, 0], [0, 2, 0], [0, 0, 0], [0, 0, -2], [1, 1, 1]], np.float32)
        fr.particles.position = np.array([[1, 1, 1], [2, 3, 2], [-1, -1, -1], [-2, -2, 2], [np.nan, 0, 0]], np.float32)
        t.append(fr)
    assert pgsd_main(['info', path, '--cells', '2,2,2']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "cell fields of frame 0 over 2 x 2 x 2 cells:" in lines
    assert "occupied cells: 3 of 8" in lines and "count: smallest 1 largest 2" in lines
    assert "largest density: 0.0625 in cell (0, 0, 0)" in lines         # 4 / 64
    assert "largest speed: 2.0 in cell (0, 0, 1)" in lines
    assert "nowhere: 1" in lines
    assert pgsd_main(['info', path, '--cells', '2,2,2', '--types', 'fluid', '--frame', '0']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "cell fields of frame 0 over 2 x 2 x 2 cells (types fluid):" in lines
    assert "occupied cells: 2 of 8" in lines and "largest density: 0.046875 in cell (1, 1, 1)" in lines
    assert pgsd_main(['info', path, '--cells', '2,2']) == 1
    assert "--cells takes CX,CY,CZ" in capsys.readouterr().err
