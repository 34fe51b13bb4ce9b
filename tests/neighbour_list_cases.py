"""What the neighbour list tests share: a plain double loop in Python floats that builds the CSR pair list of
`pgsd.hoomd.neighbour_list` -- the cells in the defined order, inside a cell ascending -- with switches that each stand for
one kernel mistake, and the mutation table with the smallest case on which each mutation differs.
`test_neighbour_list_model.py` holds the model against these; `test_gpu_neighbour_list.py` runs the kernels on the same
cases.  The fold of one pair and the offsets of one axis are `neighbours_cases`'."""
import numpy as np

import pgsd.hoomd as hoomd
from neighbours_cases import FLAT, MUTATIONS as CENSUS_MUTATIONS, axis_offsets, fold

CUBE = [8, 8, 8, 0, 0, 0]


def cell_sequence(at, grid, dedupe=True, oz_outermost=True, x_defined_order=True):
    """The candidate cells of an entry in cell ``at``, in the order they are visited."""
    ox_, oy_, oz_ = [axis_offsets(c, dedupe) for c in grid]
    seq = []
    if oz_outermost:
        for oz in oz_:
            for oy in oy_:
                xs = [(at[0] + ox) % grid[0] for ox in ox_]
                if not x_defined_order:
                    xs = sorted(xs)                 # the row's cells as they lie in memory
                seq += [(wx, (at[1] + oy) % grid[1], (at[2] + oz) % grid[2]) for wx in xs]
    else:
        for ox in ox_:
            for oy in oy_:
                for oz in oz_:
                    seq.append(((at[0] + ox) % grid[0], (at[1] + oy) % grid[1], (at[2] + oz) % grid[2]))
    return seq


def loop_neighbour_list(position, box, r, rows=None, cells=None, dimensions=3, half=False, distances=False, strict=True,
                        dedupe=True, skip_self=True, z_in_2d=False, nowhere_is_cell0=False, oz_outermost=True,
                        ascending=True, x_defined_order=True, half_strict=True, half_by_position=True, exclusive=True):
    """The pair list by a double loop over list entries in plain Python floats: ``(summary, rows, cell, offsets,
    neighbours, distance2)`` in the layout of `pgsd.hoomd.NeighbourList`.  Every keyword from ``strict`` on is a mutation."""
    p = np.asarray(position).reshape(-1, 3)
    grid = hoomd.neighbour_grid_for(box, r, dimensions) if cells is None else tuple(int(c) for c in cells)
    every = np.arange(len(p)) if rows is None else np.asarray(rows)
    rows_sorted, cell_sorted, _ = hoomd.cell_order(p, box, every, grid, dimensions)
    n, n_cells = len(rows_sorted), grid[0] * grid[1] * grid[2]
    v = [float(x) for x in hoomd.box_vectors(np.asarray(box, np.float32))]
    r2 = float(np.float64(r) * np.float64(r))
    x = [[float(np.float64(c)) for c in p[k]] for k in rows_sorted]
    ids = [int(c) for c in cell_sorted]
    nowhere = sum(1 for c in ids if c >= n_cells)
    if nowhere_is_cell0:
        ids = [0 if c == n_cells else c for c in ids]
        nowhere = 0
    members = {}
    for k, c in enumerate(ids):
        members.setdefault(c, []).append(k)
    segments = []
    for i in range(n):
        seg = []
        if ids[i] < n_cells:
            at = (ids[i] % grid[0], (ids[i] // grid[0]) % grid[1], ids[i] // (grid[0] * grid[1]))
            for w in cell_sequence(at, grid, dedupe, oz_outermost, x_defined_order):
                inside = members.get(w[0] + grid[0] * (w[1] + grid[1] * w[2]), [])
                for j in (inside if ascending else inside[::-1]):
                    if j == i and skip_self:
                        continue
                    if half:
                        a, b = (j, i) if half_by_position else (int(rows_sorted[j]), int(rows_sorted[i]))
                        if not (a > b or (not half_strict and a == b)):
                            continue
                    d2 = fold([x[j][c] - x[i][c] for c in range(3)], v, dimensions, z_in_2d)
                    if d2 < r2 or (not strict and d2 == r2):
                        seg.append((j, d2))
        segments.append(seg)
    counts = [len(s) for s in segments]
    offsets = [0] * (n + 1)
    for k in range(n):
        offsets[k + 1] = offsets[k] + counts[k]
    if not exclusive:
        offsets = offsets[1:] + [offsets[n]]
    summary = np.array([n, nowhere, sum(counts), max(counts) if n else 0], dtype=np.uint64)
    neighbours = np.array([j for s in segments for j, _ in s], dtype=np.uint32)
    distance2 = np.array([d for s in segments for _, d in s], dtype=np.float64) if distances else None
    return summary, np.asarray(rows_sorted), np.asarray(cell_sorted), np.array(offsets, dtype=np.uint64), neighbours, distance2


def same(got, want):
    """Is a `NeighbourList` with numpy arrays (the model's, or the kernels' copied to the host) the loop's result, bit for
    bit?"""
    summary, rows, cell, offsets, neighbours, distance2 = want
    if (got.distance2 is None) != (distance2 is None):
        return False
    return (np.array_equal(got.summary, summary) and np.array_equal(np.asarray(got.rows), rows)
            and np.array_equal(np.asarray(got.cell), cell)
            and np.asarray(got.offsets).dtype == np.uint64 and np.array_equal(got.offsets, offsets)
            and np.asarray(got.neighbours).dtype == np.uint32 and np.array_equal(got.neighbours, neighbours)
            and (distance2 is None or np.array_equal(np.asarray(got.distance2, dtype=np.float64).view(np.uint64),
                                                     distance2.view(np.uint64))))


def _census_case(name):
    return dict(CENSUS_MUTATIONS[name][1])


# name -> (the loop's switch, the case: keyword arguments of neighbour_list).  Each case is the smallest on which the
# mutated loop differs from the definition; the unmutated loop agrees with it on every one of them.
MUTATIONS = {
    # the entry in the middle cell of (3, 3, 3) has one neighbour at (ox, oz) = (+1, -1) and one at (-1, +1)
    'ox outermost instead of oz': (
        dict(oz_outermost=False),
        dict(position=np.array([[0, 0, 0], [1.4, 0, -1.4], [-1.4, 0, 1.4]], np.float32), box=CUBE, r=2.0, cells=(3, 3, 3))),
    'descending inside a cell': (
        dict(ascending=False),
        dict(position=np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]], np.float32), box=CUBE, r=1.0, cells=(1, 1, 1))),
    # the entry in cell ix == 0 of cx == 3 has one neighbour in cell cx - 1 (across the face) and one in cell 1
    'the x-runs of a wrapping row in memory order': (
        dict(x_defined_order=False),
        dict(position=np.array([[-2.7, 0, 0], [3.9, 0, 0], [-1.2, 0, 0]], np.float32), box=CUBE, r=2.0, cells=(3, 1, 1))),
    'the self pair listed': (dict(skip_self=False), dict(position=np.array([[1, 2, 3]], np.float32), box=CUBE, r=1.0)),
    'half as j >= i': (dict(half_strict=False, skip_self=False),
                       dict(position=np.array([[1, 2, 3]], np.float32), box=CUBE, r=1.0, half=True)),
    'half decided by row instead of list position': (
        dict(half_by_position=False),
        dict(position=np.array([[1, 2, 3]], np.float32), box=CUBE, r=1.0, rows=np.array([0, 0]), half=True)),
    '<= for <': (dict(strict=False), _census_case('<= for <')),
    'inclusive instead of exclusive offsets': (
        dict(exclusive=False), dict(position=np.array([[0, 0, 0], [0.5, 0, 0]], np.float32), box=CUBE, r=1.0)),
    'a nowhere entry given cell 0\'s segment': (dict(nowhere_is_cell0=True), _census_case('a nowhere entry in cell 0')),
    'three offsets at two cells': (dict(dedupe=False), _census_case('three offsets at two cells')),
    'z used with dimensions == 2': (dict(z_in_2d=True), _census_case('z used in two dimensions')),
}
assert FLAT == MUTATIONS['z used with dimensions == 2'][1]['box']
