"""What the SPH body-force tests share: a plain double loop of the definition of `pgsd.hoomd.sph_body_force` in Python floats
-- with switches that each stand for a kernel mistake --, the mutation table with the smallest case on which each mutation
differs, and the constructed cases: the geometry and the columns of `sph_force_cases.CASES`, split into a body and a fluid
by a seeded mask.  `test_sph_body_model.py` holds the model against the loop; `test_gpu_sph_body.py` runs the kernel on the
same cases."""
import math

import numpy as np

import pgsd.hoomd as hoomd
from neighbours_cases import FLAT, random_rows
from sph_cases import CASES as SUM_CASES, CUBE, KERNELS, NONE, _columns, bits_equal  # noqa: F401
from sph_force_cases import CASES as FORCE_CASES, _div, pressures
from sph_gradient_cases import LOOP_ENTRIES, displacement, factor, velocities  # noqa: F401

# the two ways every case is asked: the pressure term alone about the origin, and everything about a point off it
TERMS = {'plain': dict(viscosity=None, about=None), 'viscous': dict(viscosity=0.7, about=(0.5, -1.25, 2.0))}
TILE, LANES = 4096, 256


def _tree(lane):
    """The block tree over 256 lane sums: the halvings 32 .. 1 inside each run of 64, then (w0 + w1) + (w2 + w3)."""
    w = []
    for s in range(0, LANES, 64):
        p = list(lane[s:s + 64])
        for h in (32, 16, 8, 4, 2, 1):
            p = [p[i] + p[i + h] for i in range(h)]
        w.append(p[0])
    return (w[0] + w[1]) + (w[2] + w[3])


def ordered_sum(values, sequential=False):
    """The sum of Python floats in the defined order: tiles of 4096, lane k % 256 adds its 16 steps in order, the tree;
    over the tiles lane t adds tiles t, t + 256, ..., then the tree again.  ``sequential``: a mutation, one running sum."""
    if sequential:
        total = 0.0
        for v in values:
            total = total + v
        return total
    sums = []
    for t in range(0, len(values), TILE):
        tile = values[t:t + TILE]
        lane = [0.0] * LANES
        for k, v in enumerate(tile):        # (ascending k: lane k % 256 takes its steps in order)
            lane[k % LANES] = lane[k % LANES] + v
        sums.append(_tree(lane))
    lane = [0.0] * LANES
    for t, v in enumerate(sums):
        lane[t % LANES] = lane[t % LANES] + v
    return _tree(lane)


class _List(object):
    """One of the two lists in cell order, in Python floats."""

    def __init__(self, p, rows, box, grid, dimensions, raw_w, mass, density, pressure):
        self.rows, cell, _ = hoomd.cell_order(p, box, np.asarray(rows, dtype=np.int64), grid, dimensions)
        self.n, self.n_cells = len(self.rows), grid[0] * grid[1] * grid[2]
        self.ids = [int(c) for c in cell]
        self.offs = [sum(1 for c in self.ids if c < k) for k in range(self.n_cells + 2)] if self.n_cells <= 64 else None
        self.members = {}
        for k, c in enumerate(self.ids):
            self.members.setdefault(c, []).append(k)

        def column(values, default):
            return [default if values is None else float(np.float64(np.asarray(values).reshape(-1)[k])) for k in self.rows]

        self.x = [[float(np.float64(c)) for c in p[k]] for k in self.rows]
        self.w = [[float(np.float64(c)) for c in raw_w[k]] for k in self.rows]
        self.m, self.rho, pr = column(mass, 1.0), column(density, 0.0), column(pressure, 0.0)
        self.A = [_div(a, b * b) for a, b in zip(pr, self.rho)]
        self.V = [_div(a, b) for a, b in zip(self.m, self.rho)]


def loop_body_force(position, velocity, box, h, body_rows, fluid_rows, mass=None, density=None, pressure=None, viscosity=None,
                    about=None, cells=None, dimensions=3, kernel='wendland_c2', extras=None, own_offsets=False,
                    cell_from_sources=False, ab_from_sources=False, rho_from_sources=False, mf_for_mb=False, g_first=False,
                    raw_arm=False, reversed_arm=False, f_cross_r=False, sequential=False, bad_enter=False, lost_sources=False,
                    strict=True, skip_shared=False, descending_j=False, ascending_cells=False, nowhere_computed=False):
    """The body force by a double loop over (target, source) pairs in plain Python floats: ``(words, contacts,
    pressure_acc, viscous_acc)`` in the layout of `pgsd.hoomd.KernelBodyForce` (``viscous_acc`` None without a viscosity).
    Every keyword from ``own_offsets`` on is a mutation.  ``extras``: a dict that receives ``budget``, per part (pressure,
    viscous) and axis the sum over all pairs of the absolute force term, ``terms``, the pairs, and ``longest``, the most
    contacts of one target."""
    p = np.asarray(position).reshape(-1, 3)
    support = float(np.float64(2.0) * np.float64(h))
    grid = hoomd.neighbour_grid_for(box, support, dimensions) if cells is None else tuple(int(c) for c in cells)
    v = [float(x) for x in hoomd.box_vectors(np.asarray(box, np.float32))]
    r2, inv_h, hh = support * support, 1.0 / float(h), float(h)
    pi = math.pi
    if dimensions == 3:
        sigma = 21.0 / (16.0 * pi * (hh * hh * hh)) if kernel == 'wendland_c2' else 1.0 / (pi * (hh * hh * hh))
    else:
        sigma = 7.0 / (4.0 * pi * (hh * hh)) if kernel == 'wendland_c2' else 10.0 / (7.0 * pi * (hh * hh))
    G = -((sigma * inv_h) * inv_h)
    eta2 = (0.01 * hh) * hh
    Gv = None if viscosity is None else G * (2.0 * float(viscosity))
    c0 = [0.0, 0.0, 0.0] if about is None else [float(c) for c in about]
    raw_w = np.zeros((len(p), 3)) if velocity is None else np.asarray(velocity).reshape(-1, 3)
    T = _List(p, body_rows, box, grid, dimensions, raw_w, mass, density, pressure)
    S = _List(p, fluid_rows, box, grid, dimensions, raw_w, mass, density, pressure)
    n, n_cells = T.n, T.n_cells
    members = dict((c, list(ks)) for c, ks in S.members.items() if c < n_cells)
    if lost_sources:
        # (a source without a cell put where its x and y alone put it)
        for k, c in enumerate(S.ids):
            if c >= n_cells:
                flat = np.array([[S.x[k][0], S.x[k][1], 0.0]])
                c2 = int(hoomd.cell_ids(flat, box, grid, dimensions)[0])
                if c2 < n_cells:
                    members.setdefault(c2, []).append(k)
        for c in members:
            members[c].sort()
    contacts = [0] * n
    pressure_acc = [[0.0] * 3 for _ in range(n)]
    viscous_acc = None if Gv is None else [[0.0] * 3 for _ in range(n)]
    offsets = [hoomd._axis_offsets(c) for c in grid]
    budget, n_terms = [[0.0] * 3, [0.0] * 3], 0
    has, fp_first = [False] * n, {}
    for b in range(n):
        cell = T.ids[b]
        if cell_from_sources:
            cell = S.ids[b] if b < S.n else n_cells
        if cell >= n_cells:
            if nowhere_computed:
                # (the zero accumulators put through the closing arithmetic instead of +0.0 written)
                pressure_acc[b] = [-(G * 0.0)] * 3
                if Gv is not None:
                    viscous_acc[b] = [_div(Gv * 0.0, T.rho[b])] * 3
            continue
        has[b] = True
        Ab, vb, rho_b = T.A[b], T.w[b], T.rho[b]
        if ab_from_sources and b < S.n:
            Ab, vb = S.A[b], S.w[b]
        if rho_from_sources and b < S.n:
            rho_b = S.rho[b]
        at = (cell % grid[0], (cell // grid[0]) % grid[1], cell // (grid[0] * grid[1]))
        a_p, a_v = [0.0] * 3, [0.0] * 3
        for oz in offsets[2]:
            for oy in offsets[1]:
                xcells = [(at[0] + ox) % grid[0] for ox in offsets[0]]
                if ascending_cells:
                    xcells = sorted(xcells)
                for wx in xcells:
                    wy, wz = (at[1] + oy) % grid[1], (at[2] + oz) % grid[2]
                    c = wx + grid[0] * (wy + grid[1] * wz)
                    if own_offsets:
                        inside = [j for j in range(T.offs[c], T.offs[c + 1]) if j < S.n]
                    else:
                        inside = members.get(c, ())
                    for j in (reversed(inside) if descending_j else inside):
                        if skip_shared and S.rows[j] == T.rows[b]:
                            continue
                        d = displacement(T.x[b], S.x[j], v, dimensions)
                        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                        if not (d2 < r2 or (not strict and d2 == r2)):
                            continue
                        contacts[b] += 1
                        q = math.sqrt(d2) * inv_h
                        F = factor(q, kernel)
                        Ssum = Ab + S.A[j]
                        n_terms += 1
                        for k in range(3):
                            term = S.m[j] * (Ssum * (F * d[k]))
                            a_p[k] = a_p[k] + term
                            if term == term:
                                budget[0][k] += abs((T.m[b] * G) * term)
                        if Gv is None:
                            continue
                        K = _div(F * d2, d2 + eta2)
                        for k in range(3):
                            term = S.V[j] * (K * (S.w[j][k] - vb[k]))
                            a_v[k] = a_v[k] + term
                            if term == term:
                                budget[1][k] += abs(_div((T.m[b] * Gv) * term, rho_b))
        for k in range(3):
            pressure_acc[b][k] = -(G * a_p[k])
            if Gv is not None:
                viscous_acc[b][k] = _div(Gv * a_v[k], rho_b)
        if g_first:
            fp_first[b] = [-((T.m[b] * G) * a_p[k]) for k in range(3)]
    if extras is not None:
        extras['budget'], extras['terms'], extras['longest'] = budget, n_terms, max(contacts + [0])
    # the force and torque terms per target
    C = 6 if Gv is None else 12
    table = [[0.0] * n for _ in range(C)]
    words = np.zeros(22, dtype=np.uint64)
    f = words[9:22].view(np.float64)
    words[0], words[1] = n, sum(1 for c in T.ids if c >= n_cells)
    words[2], words[3] = S.n, (sum(1 for c in S.ids if c >= n_cells) if n else 0)
    words[7] = words[8] = NONE
    best = -1.0
    for b in range(n):
        if not has[b]:
            continue
        mb = S.m[b] if (mf_for_mb and b < S.n) else T.m[b]
        fp = fp_first[b] if g_first else [mb * pressure_acc[b][k] for k in range(3)]
        if raw_arm:
            r = displacement(c0, T.x[b], v, dimensions, minimum_image=False)
        elif reversed_arm:
            r = displacement(T.x[b], c0, v, dimensions)
        else:
            r = displacement(c0, T.x[b], v, dimensions)

        def cross(r, g):
            if f_cross_r:
                r, g = g, r
            return [r[1] * g[2] - r[2] * g[1], r[2] * g[0] - r[0] * g[2], r[0] * g[1] - r[1] * g[0]]

        terms = list(fp) + cross(r, fp)
        if Gv is not None:
            fv = [mb * viscous_acc[b][k] for k in range(3)]
            terms = list(fp) + fv + cross(r, fp) + cross(r, fv)
        bad = not all(math.isfinite(t) for t in terms)
        if contacts[b] >= 1:
            words[4] += 1
        if bad:
            words[6] += 1
        if bad and not bad_enter:
            continue
        for k in range(C):
            table[k][b] = terms[k]
        if bad:
            continue
        norm2 = (fp[0] * fp[0] + fp[1] * fp[1]) + fp[2] * fp[2]
        if norm2 == norm2 and norm2 > best:
            best = f[0] = norm2
            words[7], words[8] = b, int(T.rows[b])
    words[5] = sum(contacts)
    for k in range(C):
        slot = k if Gv is not None else (k if k < 3 else k + 3)
        f[1 + slot] = ordered_sum(table[k], sequential)
    as_array = lambda a: None if a is None else np.array(a, dtype=np.float64).reshape(n, 3)  # noqa: E731
    return words, np.array(contacts, dtype=np.uint32), as_array(pressure_acc), as_array(viscous_acc)


def words_equal(a, b):
    """Two summaries: the nine integer words exactly, the thirteen float words as `bits_equal`."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return np.array_equal(a[:9], b[:9]) and bits_equal(a[9:].view(np.float64), b[9:].view(np.float64))


def same(got, want):
    """Is the model's (or the kernel's, copied to the host) `KernelBodyForce` the loop's result, bit for bit?"""
    words, contacts, pressure_acc, viscous_acc = want
    if not words_equal(got.summary, words):
        return False
    if not np.array_equal(np.asarray(got.contacts, dtype=np.uint32).reshape(-1), contacts):
        return False
    for mine, theirs in ((got.pressure_acc, pressure_acc), (got.viscous_acc, viscous_acc)):
        if (mine is None) != (theirs is None):
            return False
        if mine is not None and not (np.shape(mine) == theirs.shape and bits_equal(np.ravel(mine), np.ravel(theirs))):
            return False
    return True


def split(seed, n, share=0.4):
    """``(body_rows, fluid_rows)``: the rows of ``n`` split by a seeded mask."""
    mask = np.random.default_rng(5000 + seed).random(n) < share
    return np.flatnonzero(mask), np.flatnonzero(~mask)


def _case(k, name):
    p, w, mass, density, pressure, kw = FORCE_CASES[name]
    body, fluid = split(k, len(p))
    return p, w, mass, density, pressure, body, fluid, kw


# name -> (positions, velocities, mass or None, density or None, pressure or None, body rows, fluid rows, keyword arguments
# of sph_body_force).  The cases of `sph_force_cases` (the sums' geometry, the chunks absent one at a time), each split by
# a seeded mask.
CASES = dict((name, _case(k, name)) for k, name in enumerate(sorted(FORCE_CASES)))


def case_arguments(name):
    """The keyword arguments of `sph_body_force` (and of the loop) for a case, without the terms."""
    p, w, mass, density, pressure, body, fluid, kw = CASES[name]
    return dict(dict(position=p, velocity=w, mass=mass, density=density, pressure=pressure, body_rows=body, fluid_rows=fluid),
                **kw)


def _cloud(seed, n=60, dtype=np.float64):
    return random_rows(seed, n, CUBE, dtype)


def _fluid(seed, n=60):
    rng = np.random.default_rng(2000 + seed)
    return dict(mass=rng.uniform(0.5, 2.0, size=n), density=1000.0 + 50.0 * rng.standard_normal(n), pressure=pressures(seed, n))


def _small(seed, n=60, cells=(2, 2, 2), n_body=20, **more):
    """A cloud of ``n`` rows of which the first ``n_body`` in a seeded shuffle are the body: fewer targets than sources."""
    order = np.random.default_rng(6000 + seed).permutation(n)
    return dict(dict(position=_cloud(seed, n), velocity=velocities(seed, n), box=CUBE, h=1.0, cells=cells, viscosity=0.7,
                     about=(0.5, -1.25, 2.0), body_rows=np.sort(order[:n_body]), fluid_rows=np.sort(order[n_body:]),
                     **_fluid(seed, n)), **more)


def _across_the_wrap():
    """A body in the x columns 0 and 3 of a (4, 4, 4) grid -- it lies across the periodic wrap -- with `about` inside column
    0: the arm of the targets in column 3 needs the minimum image."""
    p = SUM_CASES['four_cells_wrap'][0][:160]
    body = np.flatnonzero(np.arange(160) % 3 == 0)
    return dict(position=p, velocity=velocities(65, 160), box=CUBE, h=1.0, cells=(4, 4, 4), viscosity=0.7, about=(-3.5, 0.0, 0.0),
                body_rows=body, fluid_rows=np.setdiff1d(np.arange(160), body), **_fluid(65, 160))


def _many_targets():
    """257 targets -- the second wave of the tree and one entry more than the lanes -- over a cloud of 300."""
    return _small(74, 300, cells=(2, 2, 2), n_body=257)


def _one_bad():
    """One target of density 0: its A is infinite, its terms are not finite."""
    case = _small(75)
    density = case['density'].copy()
    density[case['body_rows'][3]] = 0.0
    return dict(case, density=density)


def _flat_lost():
    """2-D: z enters the x and y fractions -- 0 * NaN is a NaN --, so a source with a NaN z is nowhere, but the 2-D distance
    never looks at z: such a source lies inside the support of the targets beside it."""
    p = np.concatenate([random_rows(93, 30, FLAT, np.float64, 2), [[-4.3, -3.4, np.nan]] * 6,
                        [[-4.25, -3.35, 0.0], [-4.2, -3.3, 0.0]]])
    n = len(p)
    body = np.array([36, 37, 0, 1, 2, 3])
    return dict(position=p, velocity=velocities(93, n), box=FLAT, h=0.3, dimensions=2, viscosity=0.7, about=(1.0, 0.5, 0.0),
                body_rows=np.sort(body), fluid_rows=np.setdiff1d(np.arange(n), body), **_fluid(93, n))


# (at exactly 2h F is -0.0 and so is e: only S = inf shows the pair, as inf * 0; the source, row 1, has density 0)
_PAIR_AT_2H = dict(position=np.array([[0, 0, 0], [0.5, 0, 0]], np.float32), velocity=np.array([[0, 0, 0], [1, 2, 3]], np.float32),
                   box=CUBE, h=0.25, density=np.array([1, 0], np.float32), pressure=np.array([1, 1], np.float32),
                   body_rows=np.array([0]), fluid_rows=np.array([1]))
# (a row of density 0 in both lists: its A is infinite and its self term inf * 0, a NaN -- the target is bad)
_SHARED = dict(position=np.array([[1, 2, 3], [1.25, 2, 3]], np.float32), velocity=np.array([[1, 0, 0], [0, 1, 0]], np.float32),
               box=CUBE, h=0.5, density=np.array([0, 1], np.float32), pressure=np.array([1, 1], np.float32),
               body_rows=np.array([0]), fluid_rows=np.array([0, 1]))


def _nowhere_target():
    """A target nowhere beside ordinary ones, with a viscosity: Gv is negative, so (Gv * 0.0) / rho_b is -0.0."""
    case = _small(76)
    p = case['position'].copy()
    p[case['body_rows'][5], 1] = np.nan
    return dict(case, position=p)


# name -> (the loop's switch, the case: keyword arguments of sph_body_force).  Each case is a small one on which the
# mutated loop differs from the definition; the unmutated loop agrees with the model on every one of them.
MUTATIONS = {
    "the candidates looked up in the targets' own offsets": (dict(own_offsets=True), _small(61)),
    "the target's cell read from the sources' cell array": (dict(cell_from_sources=True), _small(62)),
    "A_b and v_b read from the sources' compaction": (dict(ab_from_sources=True), _small(63)),
    "rho_b read from the sources' compaction": (dict(rho_from_sources=True), _small(64)),
    'm_f used for m_b in fp': (dict(mf_for_mb=True), _small(66)),
    'fp formed as (m_b * G) * a_p': (dict(g_first=True), _small(67, 200, n_body=70)),
    'the arm without the minimum image': (dict(raw_arm=True), _across_the_wrap()),
    'the arm taken as about - x_b': (dict(reversed_arm=True), _small(68)),
    'the torque formed as f x r': (dict(f_cross_r=True), _small(69)),
    'the sum run sequentially over the list': (dict(sequential=True), _many_targets()),
    'bad targets entering the sums': (dict(bad_enter=True), _one_bad()),
    'a nowhere source contributing': (dict(lost_sources=True), _flat_lost()),
    '<= for <': (dict(strict=False), _PAIR_AT_2H),
    'a row present in both lists skipped': (dict(skip_shared=True), _SHARED),
    'j descending inside a cell': (dict(descending_j=True), _small(70, 60, cells=(1, 1, 1))),
    'cells in ascending wrapped index': (dict(ascending_cells=True), _small(71, 160, cells=(3, 3, 3), n_body=40)),
    'a target nowhere given the closing arithmetic of zero sums': (dict(nowhere_computed=True), _nowhere_target()),
}
