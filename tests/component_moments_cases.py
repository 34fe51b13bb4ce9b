"""What the component fields tests share: a plain double-loop restatement of `pgsd.hoomd.component_moments` -- the entries
of each component in list order, then Python loops over pieces, lanes and the tree, everything in Python floats -- with
switches that each stand for one kernel mistake, and the mutation table with the smallest case on which each mutation
differs.  `test_component_moments_model.py` holds the model against these; `test_gpu_component_moments.py` runs the kernels
on the same cases.  A case is a frame and a linking length: the labels and ids come from `pgsd.hoomd.neighbour_components`,
whose own restatement is `components_cases`'; nothing of the model's sums, displacements or extents is used here."""
import math

import numpy as np

import pgsd.hoomd as hoomd
from neighbours_cases import FLAT, TRICLINIC
from components_cases import CUBE

PIECE, LANES = 1024, 64


def frame_values(n_rows, seed, dtype=np.float64, spread=12):
    """mass, velocity and energy for n_rows rows whose magnitudes range over 2^-spread .. 2^spread (half that for the
    velocity, a third for the energy).  As float64 they have full mantissas and a sum's rounding depends on its order;
    ``spread=0`` makes every addition round (in a wide-ranged sum the few large values decide the result)."""
    rng = np.random.default_rng(seed)
    mass = rng.uniform(0.5, 2.0, size=n_rows) * 2.0 ** rng.integers(-spread, spread + 1, size=n_rows)
    velocity = rng.standard_normal((n_rows, 3)) * 2.0 ** rng.integers(-(spread // 2), spread // 2 + 1, size=(n_rows, 1))
    energy = rng.uniform(-1.0, 3.0, size=n_rows) * 2.0 ** rng.integers(-(spread // 3), spread // 3 + 1, size=n_rows)
    return mass.astype(dtype), velocity.astype(dtype), energy.astype(dtype)


def displacement(x_root, x_k, v, dimensions, to_root=False, raw=False, y_tilt=True, z_in_2d=False):
    """root -> entry under HOOMD's single-shift minimum image, z then y then x, in Python floats."""
    if raw:
        return list(x_k)
    a, b = (x_k, x_root) if to_root else (x_root, x_k)
    dx, dy, dz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    if dimensions == 3 or z_in_2d:
        if dz >= v[2] / 2:
            dx, dy, dz = dx - v[4], dy - v[5], dz - v[2]
        elif dz < -(v[2] / 2):
            dx, dy, dz = dx + v[4], dy + v[5], dz + v[2]
    else:
        dz = 0.0
    if dy >= v[1] / 2:
        dx, dy = (dx - v[3] if y_tilt else dx), dy - v[1]
    elif dy < -(v[1] / 2):
        dx, dy = (dx + v[3] if y_tilt else dx), dy + v[1]
    if dx >= v[0] / 2:
        dx -= v[0]
    elif dx < -(v[0] / 2):
        dx += v[0]
    return [dx, dy, dz]


def _mul(a, b):
    """a * b as the processor forms it (inf * 0 is a NaN, not an exception; an overflow is inf)."""
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        return float(np.float64(a) * np.float64(b))


def ordered_sum(values, first_position=0, poison=False):
    """The cell fields' sum of a segment's values (Python floats, in the segment's order): pieces of 1024 counted from
    the segment's first entry (``first_position``: from the slab the entry lies in instead -- a mutation), 64 striding
    lanes, the wave tree, the pieces added in ascending order to +0.0; a value that is not finite counts as +0.0."""
    pieces = {}
    for i, value in enumerate(values):
        at = first_position + i
        pieces.setdefault(at // PIECE, []).append((at % PIECE, value))
    total = 0.0
    for number in sorted(pieces):
        lanes = [0.0] * LANES
        for within, value in pieces[number]:            # (ascending: lane l adds l, l + 64, ... in that order)
            if not poison and not math.isfinite(value):
                value = 0.0
            lanes[within % LANES] = lanes[within % LANES] + value
        h = LANES // 2
        while h >= 1:
            for i in range(h):
                lanes[i] = lanes[i] + lanes[i + h]
            h //= 2
        total = total + lanes[0]
    return total


def loop_component_moments(mass, velocity, energy, position, box, label, component, rows=None, dimensions=3, to_root=False,
                           raw=False, y_tilt=True, z_in_2d=False, pieces_from_slab=False, row_order=False, poison=False,
                           bad_per_value=False, extent_from_inf=False, extent_takes_all=False, wide_strict=False,
                           kinetic_other=False, tie_smallest=True):
    """`pgsd.hoomd.component_moments` by loops: ``dict(summary, sums, lo, hi, origin, bad, wide)``.  mass, velocity and
    energy are arrays or ``None`` (the schema defaults 1, 0, 0).  Every keyword from ``to_root`` on is a mutation."""
    p = np.asarray(position).reshape(-1, 3)
    every = np.arange(len(p)) if rows is None else np.asarray(rows)
    n = len(every)
    v = [float(x) for x in hoomd.box_vectors(np.asarray(box, np.float32))]
    x = [[float(np.float64(c)) for c in p[k]] for k in every]
    m = [1.0 if mass is None else float(np.float64(np.asarray(mass)[k])) for k in every]
    e = [0.0 if energy is None else float(np.float64(np.asarray(energy)[k])) for k in every]
    w = [[0.0] * 3 if velocity is None else [float(np.float64(c)) for c in np.asarray(velocity)[k]] for k in every]
    components = int(max(component)) + 1 if n else 0
    sums, lo, hi, origin, bad, wide = [], [], [], [], [], []
    first_position = 0
    for c in range(components):
        entries = [k for k in range(n) if int(component[k]) == c]               # list order
        if row_order:
            entries.sort(key=lambda k: (int(every[k]), k))
        root = int(label[entries[0]])
        values = [[] for _ in range(9)]
        low, high = ([math.inf] * 3, [-math.inf] * 3) if extent_from_inf else ([0.0] * 3, [0.0] * 3)
        n_bad = 0
        for k in entries:
            d = [0.0, 0.0, 0.0] if k == root and not raw else displacement(x[root], x[k], v, dimensions, to_root, raw, y_tilt,
                                                                            z_in_2d)
            if kinetic_other:       # (0.5 * (m * v2) would be no mutation: a product with 0.5 is exact)
                speed2 = _mul(w[k][0], w[k][0]) + (_mul(w[k][1], w[k][1]) + _mul(w[k][2], w[k][2]))
            else:
                speed2 = (_mul(w[k][0], w[k][0]) + _mul(w[k][1], w[k][1])) + _mul(w[k][2], w[k][2])
            nine = ([m[k]] + [_mul(m[k], w[k][a]) for a in range(3)] + [_mul(_mul(0.5, m[k]), speed2), _mul(m[k], e[k])]
                    + [_mul(m[k], d[a]) for a in range(3)])
            not_finite = sum(1 for q in nine if not math.isfinite(q))
            n_bad += not_finite if bad_per_value else (1 if not_finite else 0)
            for q in range(9):
                values[q].append(nine[q])
            if k != root:
                for a in range(3):
                    if math.isfinite(d[a]) or extent_takes_all:
                        if d[a] < low[a]:
                            low[a] = d[a]
                        if d[a] > high[a]:
                            high[a] = d[a]
        sums.append([ordered_sum(values[q], first_position if pieces_from_slab else 0, poison) for q in range(9)])
        first_position += len(entries)
        lo.append(low)
        hi.append(high)
        origin.append(x[root])
        bad.append(n_bad)
        is_wide = 0
        for a in range(dimensions):
            span = high[a] - low[a]
            if span > v[a] / 2 or (not wide_strict and span == v[a] / 2):
                is_wide = 1
        wide.append(is_wide)
    summary = [n, components, sum(bad), sum(wide), 0, 0]
    if components:
        def key(value):
            return -math.inf if math.isnan(value) else value
        masses = [key(s[0]) for s in sums]
        spans = [key(max(hi[c][a] - lo[c][a] for a in range(3))) for c in range(components)]
        for at, values in ((4, masses), (5, spans)):
            tied = [c for c in range(components) if values[c] == max(values)]
            summary[at] = min(tied) if tie_smallest else max(tied)
    shaped = lambda a, width: np.array(a, dtype=np.float64).reshape(components, width)  # noqa: E731
    return dict(summary=np.array(summary, dtype=np.uint64), sums=shaped(sums, 9), lo=shaped(lo, 3), hi=shaped(hi, 3),
                origin=shaped(origin, 3), bad=np.array(bad, dtype=np.uint32), wide=np.array(wide, dtype=np.uint32))


def bits(a):
    """The bytes of a float64 array: +0.0 and -0.0 differ, a NaN equals itself."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()


def differences(got, want):
    """The names at which a `ComponentMoments` over numpy arrays (the model's, or the kernels' copied to the host) differs
    from the loop's result; empty: the same, bit for bit."""
    sums = np.concatenate([got.mass[:, None], got.momentum, got.kinetic[:, None], got.internal[:, None], got.first_moment],
                          axis=1) if got.components else np.zeros((0, 9))
    out = []
    if not np.array_equal(got.summary, want['summary']):
        out.append('summary')
    for name, a, b in (('sums', sums, want['sums']), ('lo', got.lo, want['lo']), ('hi', got.hi, want['hi']),
                       ('origin', got.origin, want['origin'])):
        if np.asarray(a).shape != b.shape or bits(a) != bits(b):
            out.append(name)
    for name in ('bad', 'wide'):
        a = np.asarray(getattr(got, name))
        if a.dtype != np.uint32 or not np.array_equal(a, want[name]):
            out.append(name)
    return out


def labelled(case):
    """The `Components` of a case's frame, from the model."""
    return hoomd.neighbour_components(case['position'], case['box'], case['r'], rows=case.get('rows'), cells=case.get('cells'),
                                      dimensions=case.get('dimensions', 3))


def loop_of(case, comps=None, **mutation):
    comps = labelled(case) if comps is None else comps
    return loop_component_moments(case.get('mass'), case.get('velocity'), case.get('energy'), case['position'], case['box'],
                                  comps.label, comps.component, rows=comps.rows, dimensions=case.get('dimensions', 3),
                                  **mutation)


def model_of(case, comps=None):
    comps = labelled(case) if comps is None else comps
    return hoomd.component_moments(case.get('mass'), case.get('velocity'), case.get('energy'), case['position'], case['box'],
                                   comps.label, comps.component, rows=comps.rows, dimensions=case.get('dimensions', 3))


def _frame(position, seed=1, dtype=np.float32, spread=12, **kw):
    p = np.asarray(position, dtype=dtype).reshape(-1, 3)
    mass, velocity, energy = frame_values(len(p), seed, dtype, spread)
    return dict(dict(position=p, mass=mass, velocity=velocity, energy=energy), **kw)


def _chain(k, x0=-30.0, y=0.0):
    return np.stack([x0 + 0.0125 * np.arange(k), np.full(k, y), np.zeros(k)], axis=1)


WIDE_BOX = [64, 64, 64, 0, 0, 0]
_PAIR = dict(box=CUBE, r=1.0, cells=(1, 1, 1))
# one singleton in the first cell of the x axis, then a chain of 1024 in the following cells: one piece counted from the
# chain's first entry, two (1023 + 1, other lanes) counted from the slab
_OFFSET_CHAIN = np.concatenate([[[-31.5, 0, 0]], _chain(1024)])
# a row order that is not the list order inside ONE component: one cell, three entries of a chain listed as rows [2, 0, 1].
# Lane l holds the l-th of them and the tree adds (lane 0 + lane 2) + lane 1: the list order gives (m2 + m1) + m0 = 2^-52 + 1,
# the row order (m0 + m2) + m1 = 1, each 2^-53 lost to the tie at 1
_REVERSED = dict(_frame(_chain(3, x0=0.0), dtype=np.float64, box=WIDE_BOX, r=0.013, cells=(1, 1, 1)),
                 mass=np.array([1.0, 2.0 ** -53, 2.0 ** -53]), rows=np.array([2, 0, 1]))


def _one_entry_whose_speed_depends_on_the_association():
    """One entry with (vx*vx + vy*vy) + vz*vz != vx*vx + (vy*vy + vz*vz): the first of a seeded sequence."""
    rng = np.random.default_rng(11)
    while True:
        v = rng.uniform(1.0, 2.0, size=3)
        if (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2] != v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]):
            return dict(_frame([[1, 2, 3]], dtype=np.float64, box=CUBE, r=1.0), mass=np.array([2.0]), velocity=v.reshape(1, 3))


# name -> (the loop's switch, the case).  Each case is the smallest on which the mutated loop differs from the definition;
# the unmutated loop agrees with the model on every one of them.
MUTATIONS = {
    'the displacement from the entry to the root': (
        dict(to_root=True), _frame([[0, 0, 0], [0.5, 0, 0]], **_PAIR)),
    'the raw position instead of the displacement': (
        dict(raw=True), _frame([[1, 2, 3], [1.5, 2, 3]], **_PAIR)),
    # the pair of the census' case: y folds, and the x tilt xy * Ly = 2.4 must go with it
    'the y shift without its x tilt': (
        dict(y_tilt=False), _frame([[1.2, 3.9, 0], [-1.2, -3.9, 0]], box=TRICLINIC, r=0.6)),
    # two entries of one flat piece whose z differ: d_z is 0 in two dimensions
    'z used with dimensions == 2': (
        dict(z_in_2d=True), _frame([[0, 0, 0], [0.1, 0, 0.25]], box=FLAT, r=0.5, dimensions=2)),
    'pieces counted from the slab': (
        dict(pieces_from_slab=True), _frame(_OFFSET_CHAIN, seed=3, dtype=np.float64, box=WIDE_BOX, r=0.013, cells=(64, 1, 1))),
    'a component in row order instead of list order': (dict(row_order=True), _REVERSED),
    'a value that is not finite poisons its sum': (
        dict(poison=True), dict(_frame([[0, 0, 0], [0.5, 0, 0]], **_PAIR), mass=np.array([1.0, np.inf], np.float32))),
    # an infinite mass makes several of the entry's nine values not finite: one bad entry
    'bad counted per value': (
        dict(bad_per_value=True), dict(_frame([[0, 0, 0], [0.5, 0, 0]], **_PAIR), mass=np.array([1.0, np.inf], np.float32))),
    'the extent started at +-inf': (dict(extent_from_inf=True), _frame([[1, 2, 3]], box=CUBE, r=1.0)),
    # root 1, members at d = -2 and d = -4 (exactly -L/2 is not shifted): the span is exactly L/2
    'wide tested with >': (
        dict(wide_strict=True), _frame([[1, 0, 0], [-1, 0, 0], [-3, 0, 0]], box=CUBE, r=2.5, cells=(1, 1, 1))),
    'the kinetic energy associated as vx2 + (vy2 + vz2)': (
        dict(kinetic_other=True), _one_entry_whose_speed_depends_on_the_association()),
    # two singletons of one mass and no extent
    'heaviest and widest the largest id among ties': (
        dict(tie_smallest=False), dict(_frame([[0, 0, 0], [3, 0, 0]], **_PAIR), mass=np.array([2.0, 2.0], np.float32))),
}

# The mutation "the extent takes a d that is not finite" (``extent_takes_all=True``) has NO case on which it differs, and so
# no row above.  A NaN is taken by neither strict comparison, so only d_a = +-inf could differ.  d is a difference of two
# stored coordinates and a few box shifts: it is infinite only if exactly one of the two coordinates is infinite (two
# infinite ones of one sign give inf - inf, a NaN; the shifts are finite).  An entry with an infinite coordinate has a NaN
# wrapped fraction, so it has no cell, no edge, and is a component of its own: it is its own root and no d is formed.  So
# inside any labelling that `neighbour_components` produces no d is ever infinite.  The switch stays for labellings made by
# hand (`component_moments` accepts any consistent one): `test_component_moments_model.py` builds one and checks the model
# against both loops there.
NO_CASE = {'the extent takes a d that is not finite': dict(extent_takes_all=True)}


def mismatches(got, want):
    """The attributes at which two `ComponentMoments` over numpy arrays differ (floats bit for bit); empty: the same."""
    out = [] if np.array_equal(got.summary, want.summary) else ['summary']
    for name in ('mass', 'momentum', 'kinetic', 'internal', 'first_moment', 'origin', 'lo', 'hi'):
        a, b = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        if a.dtype != np.float64 or a.shape != b.shape or bits(a) != bits(b):
            out.append(name)
    for name in ('bad', 'wide'):
        a, b = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        if a.dtype != np.uint32 or a.shape != b.shape or not np.array_equal(a, b):
            out.append(name)
    return out
