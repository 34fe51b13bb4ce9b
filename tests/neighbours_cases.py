"""What the neighbour census tests share: a plain double loop over ordered pairs with the adjacency rule of
`pgsd.hoomd.particle_neighbours` -- with switches that each stand for a kernel mistake --, a search over all pairs without
cells, and the mutation table with the case on which each mutation differs.  `test_neighbours_model.py` holds the model
against these; `test_gpu_neighbours.py` runs the kernel on the same cases."""
import itertools
import math

import numpy as np

import pgsd.hoomd as hoomd

NONE = 0xFFFFFFFF
ORTHO = [10, 8, 6, 0, 0, 0]
TRICLINIC = [10, 8, 6, 0.3, -0.2, 0.4]
FLAT = [9, 7, 1, 0.25, 0, 0]                # dimensions == 2


def fold(d, v, dimensions, z_in_2d=False, y_tilt=True, z_first=True):
    """HOOMD's single-shift minimum image of the difference d (three Python floats), z then y then x."""
    dx, dy, dz = d
    if dimensions == 2 and not z_in_2d:
        dz = 0.0

    def shift_z(dx, dy, dz):
        if dimensions == 3 or z_in_2d:
            if dz >= v[2] / 2:
                return dx - v[4], dy - v[5], dz - v[2]
            if dz < -(v[2] / 2):
                return dx + v[4], dy + v[5], dz + v[2]
        return dx, dy, dz

    def shift_y(dx, dy, dz):
        if dy >= v[1] / 2:
            return (dx - v[3] if y_tilt else dx), dy - v[1], dz
        if dy < -(v[1] / 2):
            return (dx + v[3] if y_tilt else dx), dy + v[1], dz
        return dx, dy, dz

    for step in ((shift_z, shift_y) if z_first else (shift_y, shift_z)):
        dx, dy, dz = step(dx, dy, dz)
    if dx >= v[0] / 2:
        dx -= v[0]
    elif dx < -(v[0] / 2):
        dx += v[0]
    return (dx * dx + dy * dy) + dz * dz


def axis_offsets(c, dedupe=True):
    if c == 1:
        return (0,)
    if c == 2 and dedupe:
        return (0, 1)
    return (-1, 0, 1)


def loop_neighbours(position, box, r, rows=None, cells=None, dimensions=3, bins=0, strict=True, wrap=True, dedupe=True,
                    skip_self=True, z_in_2d=False, y_tilt=True, z_first=True, tie_small=True, right_closed=False,
                    last_edge_r2=True, nowhere_is_cell0=False):
    """The census by a double loop over ordered pairs of list entries in plain Python floats: ``(summary, closest2, count,
    nearest2, nearest)`` in the layout of `pgsd.hoomd.Neighbours`.  Every keyword from ``strict`` on is a mutation."""
    p = np.asarray(position).reshape(-1, 3)
    grid = hoomd.neighbour_grid_for(box, r, dimensions) if cells is None else tuple(int(c) for c in cells)
    every = np.arange(len(p)) if rows is None else np.asarray(rows)
    rows_sorted, cell_sorted, _ = hoomd.cell_order(p, box, every, grid, dimensions)
    n, n_cells = len(rows_sorted), grid[0] * grid[1] * grid[2]
    v = [float(x) for x in hoomd.box_vectors(np.asarray(box, np.float32))]
    r2 = float(np.float64(r) * np.float64(r))
    x = [[float(np.float64(c)) for c in p[k]] for k in rows_sorted]
    ids = [int(c) for c in cell_sorted]
    if nowhere_is_cell0:
        ids = [0 if c == n_cells else c for c in ids]
    width = float(np.float64(r) / np.float64(bins)) if bins else 0.0
    edges = [(k * width) ** 2 for k in range(bins + 1)]
    if bins and last_edge_r2:
        edges[bins] = r2
    members = {}
    for k, c in enumerate(ids):
        members.setdefault(c, []).append(k)
    count, nearest2, nearest, pair_hist = [0] * n, [math.inf] * n, [NONE] * n, [0] * bins
    offsets = list(itertools.product(*[axis_offsets(c, dedupe) for c in grid]))
    for i in range(n):
        if ids[i] >= n_cells:
            continue
        at = (ids[i] % grid[0], (ids[i] // grid[0]) % grid[1], ids[i] // (grid[0] * grid[1]))
        for o in offsets:
            w = [at[a] + o[a] for a in range(3)]
            if not wrap and any(not 0 <= w[a] < grid[a] for a in range(3)):
                continue
            w = [w[a] % grid[a] for a in range(3)]
            for j in members.get(w[0] + grid[0] * (w[1] + grid[1] * w[2]), ()):
                if j == i and skip_self:
                    continue
                d2 = fold([x[j][a] - x[i][a] for a in range(3)], v, dimensions, z_in_2d, y_tilt, z_first)
                if not (d2 < r2 or (not strict and d2 == r2)):
                    continue
                count[i] += 1
                if d2 < nearest2[i] or (d2 == nearest2[i] and (j < nearest[i] if tie_small else j > nearest[i])):
                    nearest2[i], nearest[i] = d2, j
                if bins:
                    if right_closed:
                        b = sum(1 for e in edges if e < d2) - 1
                    else:
                        b = sum(1 for e in edges if e <= d2) - 1
                    if 0 <= b < bins:
                        pair_hist[b] += 1
    with_cell = [k for k in range(n) if ids[k] < n_cells]
    summary = [n, n - len(with_cell), sum(count), 0, 0, NONE, NONE, NONE] + [0] * 257 + pair_hist
    closest2 = math.inf
    if with_cell:
        summary[3], summary[4] = min(count[k] for k in with_cell), max(count[k] for k in with_cell)
        for k in with_cell:
            summary[8 + min(count[k], 256)] += 1
        for k in range(n):
            if nearest[k] != NONE and nearest2[k] < closest2:
                closest2 = nearest2[k]
                summary[5], summary[6], summary[7] = k, int(rows_sorted[k]), int(rows_sorted[nearest[k]])
    return (np.array(summary, dtype=np.uint64), closest2, np.array(count, dtype=np.uint32),
            np.array(nearest2, dtype=np.float64), np.array(nearest, dtype=np.uint32))


def same(got, want):
    """Is the model's (or the kernel's, copied to the host) `Neighbours` the loop's result, bit for bit?"""
    summary, closest2, count, nearest2, nearest = want
    return (np.array_equal(got.summary, summary)
            and np.float64(got.closest2).view(np.uint64) == np.float64(closest2).view(np.uint64)
            and np.array_equal(np.asarray(got.count).view(np.uint32), count)
            and np.array_equal(np.asarray(got.nearest2, dtype=np.float64).view(np.uint64), nearest2.view(np.uint64))
            and np.array_equal(np.asarray(got.nearest).view(np.uint32), nearest))


def brute_force(position, box, r, dimensions=3):
    """Counts and nearest d2 per ROW over all ordered pairs, without cells: numpy over the N x N differences with the fold
    written out once more."""
    p = np.asarray(position).astype(np.float64).reshape(-1, 3)
    v = hoomd.box_vectors(np.asarray(box, np.float32))
    d = p[None, :, :] - p[:, None, :]               # d[i, j] = x_j - x_i
    dx, dy, dz = d[..., 0].copy(), d[..., 1].copy(), d[..., 2].copy()
    if dimensions == 3:
        s = np.where(dz >= v[2] / 2, -1.0, np.where(dz < -(v[2] / 2), 1.0, 0.0))
        dx, dy, dz = dx + s * v[4], dy + s * v[5], dz + s * v[2]
    else:
        dz[:] = 0.0
    s = np.where(dy >= v[1] / 2, -1.0, np.where(dy < -(v[1] / 2), 1.0, 0.0))
    dx, dy = dx + s * v[3], dy + s * v[1]
    s = np.where(dx >= v[0] / 2, -1.0, np.where(dx < -(v[0] / 2), 1.0, 0.0))
    dx = dx + s * v[0]
    d2 = (dx * dx + dy * dy) + dz * dz
    np.fill_diagonal(d2, np.inf)
    near = d2 < np.float64(r) * np.float64(r)
    return near.sum(axis=1).astype(np.uint32), np.where(near, d2, np.inf).min(axis=1, initial=np.inf)


def random_rows(seed, n, box, dtype=np.float32, dimensions=3):
    """n uniformly random rows inside the box (fractions in [0, 1) mapped through the box matrix)."""
    rng = np.random.default_rng(seed)
    f = rng.random((n, 3)) - 0.5
    Lx, Ly, Lz, xy, xz, yz = [float(b) for b in box]
    z = f[:, 2] * Lz if dimensions == 3 else np.zeros(n)
    y = f[:, 1] * Ly + yz * z
    x = f[:, 0] * Lx + xy * (f[:, 1] * Ly) + xz * z
    return np.stack([x, y, z], axis=1).astype(dtype)


def _short_last_edge():
    """(r, bins) at which bins * (r / bins) rounds below r, so that the last edge formed that way is below r * r."""
    for r in (1.3, 0.7, 1.1, 2.9, 0.6):
        for bins in range(2, 64):
            if bins * (np.float64(r) / np.float64(bins)) < np.float64(r):
                return r, bins
    raise AssertionError("no such pair")


_R_SHORT, _BINS_SHORT = _short_last_edge()

# name -> (the loop's switch, the case: keyword arguments of particle_neighbours).  Each case is the smallest on which the
# mutated loop differs from the definition; the unmutated loop agrees with it on every one of them.
MUTATIONS = {
    '<= for <': (dict(strict=False),
                 dict(position=np.array([[0, 0, 0], [0.5, 0, 0]], np.float32), box=[8, 8, 8, 0, 0, 0], r=0.5)),
    'no periodic wrap of the neighbour cell': (
        dict(wrap=False), dict(position=np.array([[-3.9, 0, 0], [3.9, 0.1, 0]], np.float32), box=[8, 8, 8, 0, 0, 0], r=0.5)),
    'three offsets at two cells': (
        dict(dedupe=False),
        dict(position=np.array([[-0.5, 0, 0], [0.5, 0, 0]], np.float32), box=[8, 8, 8, 0, 0, 0], r=2.0, cells=(2, 2, 2))),
    'the self pair counted': (dict(skip_self=False),
                              dict(position=np.array([[1, 2, 3]], np.float32), box=[8, 8, 8, 0, 0, 0], r=1.0)),
    'z used in two dimensions': (
        dict(z_in_2d=True), dict(position=np.array([[0, 0, 0], [0.1, 0, 5]], np.float32), box=FLAT, r=0.5, dimensions=2)),
    'the y shift without its x tilt': (
        dict(y_tilt=False), dict(position=np.array([[1.2, 3.9, 0], [-1.2, -3.9, 0]], np.float32), box=TRICLINIC, r=0.6)),
    'the z shift after the y shift': (
        dict(z_first=False),
        dict(position=np.array([[0, -1.5, -2.9], [0, 1.55, 2.9]], np.float32), box=[10, 4, 6, 0, 0, 0.5], r=0.6)),
    'the tie towards the larger position': (
        dict(tie_small=False),
        dict(position=np.array([[0, 0, 0], [0.25, 0, 0], [-0.25, 0, 0]], np.float32), box=[8, 8, 8, 0, 0, 0], r=0.5,
             cells=(1, 1, 1))),
    'the bin edge closed on the right': (
        dict(right_closed=True),
        dict(position=np.array([[0, 0, 0], [0.5, 0, 0]], np.float32), box=[8, 8, 8, 0, 0, 0], r=1.0, bins=2)),
    'the last edge from the bin width': (
        dict(last_edge_r2=False),
        dict(position=np.array([[0, 0, 0], [_BINS_SHORT * (np.float64(_R_SHORT) / _BINS_SHORT), 0, 0]], np.float64),
             box=[8, 8, 8, 0, 0, 0], r=_R_SHORT, bins=_BINS_SHORT)),
    'a nowhere entry in cell 0': (
        dict(nowhere_is_cell0=True),
        dict(position=np.array([[-3.9, -3.9, -3.9], [np.nan, 0, 0], [1, 1, 1]], np.float32), box=[8, 8, 8, 0, 0, 0], r=1.0)),
}
