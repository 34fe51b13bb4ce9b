"""What the components tests share: a plain-Python labelling of `pgsd.hoomd.neighbour_components` -- a double loop over the
pairs of list entries in adjacent cells in Python floats, then a breadth-first search over the edges it found -- with
switches that each stand for one kernel mistake, and the mutation table with the smallest case on which each mutation
differs.  `test_components_model.py` holds the model against these; `test_gpu_components.py` runs the kernels on the same
cases.  The fold of one pair and the offsets of one axis are `neighbours_cases`', the cell order is `pgsd.hoomd.cell_order`
as in the other case files; none of the model's labelling is used."""
import itertools
from collections import deque

import numpy as np

import pgsd.hoomd as hoomd
from neighbours_cases import FLAT, MUTATIONS as CENSUS_MUTATIONS, TRICLINIC, axis_offsets, fold

CUBE = [8, 8, 8, 0, 0, 0]


def loop_components(position, box, r, rows=None, cells=None, dimensions=3, strict=True, wrap=True, z_in_2d=False,
                    nowhere_joins_cell0=False, join_repeats=True, label_by_position=True, number_by_smallest=True,
                    tie_smallest=True, forward=True):
    """The components by a double loop and a breadth-first search: ``(summary, rows, cell, label, component, sizes)`` in the
    layout of `pgsd.hoomd.Components`.  Every keyword from ``strict`` on is a mutation."""
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
    members = {}
    for k, c in enumerate(ids):
        members.setdefault(c, []).append(k)
    offsets = list(itertools.product(*[axis_offsets(c) for c in grid]))
    linked = [set() for _ in range(n)]
    for i in range(n):
        if ids[i] >= n_cells:
            if nowhere_joins_cell0:
                for j in members.get(0, ()):
                    linked[i].add(j)
                    linked[j].add(i)
            continue
        at = (ids[i] % grid[0], (ids[i] // grid[0]) % grid[1], ids[i] // (grid[0] * grid[1]))
        for o in offsets:
            w = [at[a] + o[a] for a in range(3)]
            if not wrap and any(not 0 <= w[a] < grid[a] for a in range(3)):
                continue
            w = [w[a] % grid[a] for a in range(3)]
            for j in members.get(w[0] + grid[0] * (w[1] + grid[1] * w[2]), ()):
                if j <= i:                          # the edge i -- j belongs to the smaller list position
                    continue
                if not join_repeats and rows_sorted[i] == rows_sorted[j]:
                    continue
                if forward:
                    d2 = fold([x[j][c] - x[i][c] for c in range(3)], v, dimensions, z_in_2d)
                else:
                    d2 = fold([x[i][c] - x[j][c] for c in range(3)], v, dimensions, z_in_2d)
                if d2 < r2 or (not strict and d2 == r2):
                    linked[i].add(j)
                    linked[j].add(i)
    pieces, seen = [], [False] * n
    for start in range(n):                          # ascending: a piece is found from its smallest member
        if seen[start]:
            continue
        seen[start] = True
        piece, queue = [], deque([start])
        while queue:
            k = queue.popleft()
            piece.append(k)
            for j in sorted(linked[k]):
                if not seen[j]:
                    seen[j] = True
                    queue.append(j)
        pieces.append(sorted(piece))
    if not number_by_smallest:
        pieces.sort(key=lambda piece: piece[-1])
    label, component = [0] * n, [0] * n
    for c, piece in enumerate(pieces):
        name = piece[0] if label_by_position else min(piece, key=lambda k: (int(rows_sorted[k]), k))
        for k in piece:
            label[k], component[k] = name, c
    sizes = [len(piece) for piece in pieces]
    summary = [n, nowhere, len(pieces), sum(1 for s in sizes if s == 1), 0, 0]
    if n:
        summary[4] = max(sizes)
        tied = [label[piece[0]] for piece in pieces if len(piece) == summary[4]]
        summary[5] = min(tied) if tie_smallest else max(tied)
    return (np.array(summary, dtype=np.uint64), np.asarray(rows_sorted), np.asarray(cell_sorted),
            np.array(label, dtype=np.uint32), np.array(component, dtype=np.uint32), np.array(sizes, dtype=np.uint32))


def same(got, want):
    """Is a `Components` with numpy arrays (the model's, or the kernels' copied to the host) the loop's result?"""
    summary, rows, cell, label, component, sizes = want
    return (np.array_equal(got.summary, summary) and np.array_equal(np.asarray(got.rows), rows)
            and np.array_equal(np.asarray(got.cell), cell)
            and np.asarray(got.label).dtype == np.uint32 and np.array_equal(got.label, label)
            and np.asarray(got.component).dtype == np.uint32 and np.array_equal(got.component, component)
            and np.asarray(got.sizes).dtype == np.uint32 and np.array_equal(got.sizes, sizes))


def _census_case(name):
    case = dict(CENSUS_MUTATIONS[name][1])
    case.pop('bins', None)
    return case


# name -> (the loop's switch, the case: keyword arguments of neighbour_components).  Each case is the smallest on which the
# mutated loop differs from the definition; the unmutated loop agrees with it on every one of them.
MUTATIONS = {
    # row 1 lies in the cell before row 0's: the list is [1, 0], the two are joined, and the smallest row sits at position 1
    'the label is the smallest row instead of the smallest position': (
        dict(label_by_position=False),
        dict(position=np.array([[0.3, 0, 0], [-0.3, 0, 0]], np.float32), box=CUBE, r=1.0)),
    '<= for <': (dict(strict=False), _census_case('<= for <')),
    'a nowhere entry joined to cell 0': (dict(nowhere_joins_cell0=True), _census_case('a nowhere entry in cell 0')),
    'a repeated row not joined to itself': (
        dict(join_repeats=False), dict(position=np.array([[1, 2, 3]], np.float32), box=CUBE, r=1.0, rows=np.array([0, 0]))),
    # one cell: the list is the rows; the pieces {0, 3} and {1, 2}: the smallest members order them 0, 1, the largest 1, 0
    'the dense ids in the order of the largest member': (
        dict(number_by_smallest=False),
        dict(position=np.array([[0, 0, 0], [3, 0, 0], [3.5, 0, 0], [0.5, 0, 0]], np.float32), box=CUBE, r=1.0,
             cells=(1, 1, 1))),
    # two pieces of two entries each
    'largest_label the largest label among ties': (
        dict(tie_smallest=False),
        dict(position=np.array([[0, 0, 0], [0.5, 0, 0], [3, 0, 0], [3.5, 0, 0]], np.float32), box=CUBE, r=1.0,
             cells=(1, 1, 1))),
    'z used with dimensions == 2': (dict(z_in_2d=True), _census_case('z used in two dimensions')),
    # two entries at x = -3.9 and x = +3.9 of the 8-cube: 0.2 apart through the face
    'an edge across the periodic face missed': (dict(wrap=False), _census_case('no periodic wrap of the neighbour cell')),
}
assert FLAT == MUTATIONS['z used with dimensions == 2'][1]['box']

# The mutation "the edges taken from j -> i instead of i -> j" (``forward=False``) has NO case on which it differs, and so
# no row above.  i -> j and j -> i fold exact negatives; the fold is asymmetric only where a component of the difference
# is exactly half the box length L of its axis (`>=` shifts, `<` does not).  After the fold that component is -L/2 either
# way, so d2 >= (L/2)^2 in both directions (a sum of non-negative terms is no smaller than any of them, in floating point
# too), while every range the grid accepts is at most half the nearest plane distance, which is at most L/2: r*r <=
# (L/2)^2 and the strict test fails in both directions.  The two directions can differ in d2, never in the edge.  The
# cases below sit on such ties -- on each of the three axes of the tilted box, at the largest range it takes -- and
# `test_components_model.py` checks that the reversed loop agrees on them and on random frames.
TIES = {
    'x': dict(position=np.array([[-2.5, 0, 0], [2.5, 0, 0], [2.25, 0.5, 0]], np.float64), box=TRICLINIC, r=2.9),
    'y': dict(position=np.array([[0, -2, 0], [0, 2, 0], [0.5, 1.75, 0]], np.float64), box=TRICLINIC, r=2.9),
    'z': dict(position=np.array([[0, 0, -1.5], [0, 0, 1.5], [0, 0.5, 1.45]], np.float64), box=TRICLINIC, r=2.9),
}
