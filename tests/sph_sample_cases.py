"""What the SPH sampling tests share: a plain double loop of the definition of `pgsd.hoomd.sph_samples` in Python floats --
with switches that each stand for a kernel mistake --, the mutation table with the smallest case on which each mutation
differs, and the constructed cases: the geometry of `sph_cases.CASES` with the seeded velocity columns of
`sph_gradient_cases` and the seeded pressure columns of `sph_force_cases` as values, sampled at the particles' own
positions, on a `sample_grid` lattice, at seeded random points and at special points.  `test_sph_sample_model.py` holds
the model against the loop; `test_gpu_sph_samples.py` runs the kernel on the same cases."""
import math

import numpy as np

import pgsd.hoomd as hoomd
from neighbours_cases import FLAT, TRICLINIC, random_rows  # noqa: F401
from sph_cases import CASES as SUM_CASES, CUBE, KERNELS, NONE, WIDE, _columns, bits_equal, weight  # noqa: F401
from sph_gradient_cases import displacement, velocities
from sph_force_cases import pressures

# the widths of the value arrays that make C columns: padding on both sides of every instantiated width (0, 1, 4, 8)
WIDTHS = {0: (), 1: (1,), 2: (2,), 3: (3,), 4: (3, 1), 5: (4, 1), 8: (3, 1, 2, 2)}


def _div(a, b):
    """a / b as IEEE gives it (Python raises on a zero divisor)."""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        return float(np.float64(a) / np.float64(b))


def _mul(a, b):
    """a * b as IEEE gives it (inf * 0 is a NaN, no exception)."""
    with np.errstate(invalid='ignore', over='ignore'):
        return float(np.float64(a) * np.float64(b))


def fractions(x, box):
    """The three fractions of `pgsd.hoomd.domain_rows` before the wrap, in Python floats (box rounded to float32)."""
    Lx, Ly, Lz, xy, xz, yz = [float(np.float32(b)) for b in box]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        x0, x1, x2 = (np.float64(c) for c in x)
        return [float(((x0 + Lx / 2) - ((xz - yz * xy) * x2 + xy * x1)) / Lx), float(((x1 + Ly / 2) - yz * x2) / Ly),
                float((x2 + Lz / 2) / Lz)]


def wrapped(s):
    if not math.isfinite(s):
        return math.nan
    f = s - math.floor(s)
    return 0.0 if f >= 1.0 else f


def loop_samples(points, position, box, h, values=(), mass=None, density=None, rows=None, cells=None, dimensions=3,
                 kernel='wendland_c2', normalise=False, extras=None, reversed_d=False, lost_entries=False, point_f32=False,
                 vf_first=False, sigma_inside=False, normalise_scaled=False, v_f32=False, strict=True, descending_j=False,
                 ascending_cells=False, no_image=False, count_candidates=False, nowhere_nan=False, outside_wrapped=False):
    """The samples by a double loop over points and list entries in plain Python floats: ``(words, count, density,
    shepard, values)`` in the layout of `pgsd.hoomd.KernelSamples`.  Every keyword from ``reversed_d`` on is a mutation.
    ``extras``: a dict that receives per point ``weight`` = sum vw and per column ``budget`` = sum |vw f|."""
    p = np.asarray(position).reshape(-1, 3)
    support = float(np.float64(2.0) * np.float64(h))
    grid = hoomd.neighbour_grid_for(box, support, dimensions) if cells is None else tuple(int(c) for c in cells)
    every = np.arange(len(p)) if rows is None else np.asarray(rows)
    rows_sorted, cell_sorted, _ = hoomd.cell_order(p, box, every, grid, dimensions)
    n, n_cells = len(rows_sorted), grid[0] * grid[1] * grid[2]
    v = [float(x) for x in hoomd.box_vectors(np.asarray(box, np.float32))]
    r2, inv_h, hh = support * support, 1.0 / float(h), float(h)
    pi = math.pi
    if dimensions == 3:
        sigma = 21.0 / (16.0 * pi * (hh * hh * hh)) if kernel == 'wendland_c2' else 1.0 / (pi * (hh * hh * hh))
    else:
        sigma = 7.0 / (4.0 * pi * (hh * hh)) if kernel == 'wendland_c2' else 10.0 / (7.0 * pi * (hh * hh))

    def column(given, default):
        return [default if given is None else float(np.float64(np.asarray(given).reshape(-1)[k])) for k in rows_sorted]

    x = [[float(np.float64(c)) for c in p[k]] for k in rows_sorted]
    m, rho = column(mass, 1.0), column(density, 0.0)
    if v_f32:
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            V = [float(np.float32(a) / np.float32(b)) for a, b in zip(m, rho)]
    else:
        V = [_div(a, b) for a, b in zip(m, rho)]
    table = [np.asarray(a).reshape(len(p), -1) for a in values]
    f = [[float(np.float64(c)) for a in table for c in a[k]] for k in rows_sorted]
    C = sum(a.shape[1] for a in table)
    ids = [int(c) for c in cell_sorted]
    members = {}
    for k, c in enumerate(ids):
        if c < n_cells:
            members.setdefault(c, []).append(k)
        elif lost_entries:
            # (an entry without a cell put where the integer conversion of its fractions would put it: NaN as 0)
            s = [wrapped(t) for t in fractions(x[k], box)]
            at = [0 if t != t else min(int(t * grid[a]), grid[a] - 1) for a, t in enumerate(s)]
            members.setdefault(at[0] + grid[0] * (at[1] + grid[1] * (at[2] if dimensions == 3 else 0)), []).append(k)
    for c in members:
        members[c].sort()
    xp = np.asarray(points).reshape(-1, 3)
    xp = xp.astype(np.float32).astype(np.float64) if point_f32 else xp.astype(np.float64)
    K = len(xp)
    count, rho_sum, shepard = [0] * K, [0.0] * K, [0.0] * K
    out = [[0.0] * C for _ in range(K)]
    has, outside = [False] * K, [False] * K
    offsets = [hoomd._axis_offsets(c) for c in grid]
    axes = 2 if dimensions == 2 else 3
    weights, budgets = [0.0] * K, [[0.0] * C for _ in range(K)]
    for i in range(K):
        xi = [float(c) for c in xp[i]]
        s = fractions(xi, box)[:axes]
        fr = [wrapped(t) for t in s]
        if any(t != t for t in fr):
            if nowhere_nan and normalise:
                out[i] = [math.nan] * C
            continue
        has[i] = True
        outside[i] = any(t < 0.0 or t >= 1.0 for t in (fr if outside_wrapped else s))
        at = [min(int(t * grid[a]), grid[a] - 1) for a, t in enumerate(fr)] + [0] * (3 - axes)
        a_m, a_v, a_f = 0.0, 0.0, [0.0] * C
        for oz in offsets[2]:
            for oy in offsets[1]:
                xcells = [(at[0] + ox) % grid[0] for ox in offsets[0]]
                if ascending_cells:
                    xcells = sorted(xcells)
                for wx in xcells:
                    wy, wz = (at[1] + oy) % grid[1], (at[2] + oz) % grid[2]
                    inside = members.get(wx + grid[0] * (wy + grid[1] * wz), ())
                    for j in (reversed(inside) if descending_j else inside):
                        if count_candidates:
                            count[i] += 1
                        d = displacement(x[j], xi, v, dimensions, not no_image) if reversed_d \
                            else displacement(xi, x[j], v, dimensions, not no_image)
                        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                        if not (d2 < r2 or (not strict and d2 == r2)):
                            continue
                        if not count_candidates:
                            count[i] += 1
                        w = weight(math.sqrt(d2) * inv_h, kernel)
                        if sigma_inside:
                            w = sigma * w
                        a_m = a_m + _mul(m[j], w)
                        vw = _mul(V[j], w)
                        a_v = a_v + vw
                        weights[i] += abs(vw) if vw == vw else 0.0
                        for c in range(C):
                            term = _mul(_mul(V[j], f[j][c]), w) if vf_first else _mul(vw, f[j][c])
                            with np.errstate(invalid='ignore', over='ignore'):
                                a_f[c] = float(np.float64(a_f[c]) + np.float64(term))
                            budgets[i][c] += abs(term) if term == term else 0.0
        scale = 1.0 if sigma_inside else sigma
        rho_sum[i], shepard[i] = _mul(scale, a_m), _mul(scale, a_v)
        for c in range(C):
            if not normalise:
                out[i][c] = _mul(scale, a_f[c])
            elif normalise_scaled:
                out[i][c] = _div(_mul(scale, a_f[c]), _mul(scale, a_v))
            else:
                out[i][c] = _div(a_f[c], a_v)
    if extras is not None:
        extras['weight'], extras['budget'] = weights, budgets
    words = np.zeros(11, dtype=np.uint64)
    fw = words[7:11].view(np.float64)
    fw[0::2], fw[1::2] = math.inf, -math.inf
    with_cell = [i for i in range(K) if has[i]]
    words[0], words[1], words[6] = K, K - len(with_cell), NONE
    words[2] = sum(1 for i in with_cell if outside[i])
    words[3] = sum(1 for i in with_cell if count[i] == 0)
    words[4] = sum(1 for i in with_cell if not all(math.isfinite(c) for c in [rho_sum[i], shepard[i]] + out[i]))
    best = -1
    for i in with_cell:
        if count[i] > best:
            best = count[i]
            words[5], words[6] = count[i], i
        for s, value in enumerate((shepard[i], rho_sum[i])):
            if value < fw[2 * s]:
                fw[2 * s] = value
            if value > fw[2 * s + 1]:
                fw[2 * s + 1] = value
    return (words, np.array(count, dtype=np.uint32), np.array(rho_sum, dtype=np.float64), np.array(shepard, dtype=np.float64),
            np.array(out, dtype=np.float64).reshape(K, C))


def words_equal(a, b):
    """Two summaries: the seven integer words exactly, the four float words as `bits_equal`."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return np.array_equal(a[:7], b[:7]) and bits_equal(a[7:].view(np.float64), b[7:].view(np.float64))


def same(got, want):
    """Is the model's (or the kernel's, copied to the host) `KernelSamples` the loop's result, bit for bit?"""
    words, count, rho_sum, shepard, out = want
    return (words_equal(got.summary, words) and np.array_equal(np.asarray(got.count), count)
            and np.asarray(got.count).dtype == np.uint32 and bits_equal(got.density, rho_sum) and bits_equal(got.shepard, shepard)
            and np.shape(got.values) == out.shape and bits_equal(np.ravel(got.values), out.ravel()))


def value_arrays(seed, n, C, dtype=np.float64):
    """The value arrays of `WIDTHS` ``[C]``: the velocity (where a width is 3), pressures and seeded columns."""
    rng = np.random.default_rng(4000 + seed)
    out = []
    for k, width in enumerate(WIDTHS[C]):
        a = velocities(seed + k, n) if width == 3 else (pressures(seed + k, n).reshape(n, 1) if width == 1
                                                        else rng.standard_normal((n, width)))
        out.append(np.ascontiguousarray(a.astype(dtype)))
    return out


def special_points(box, dimensions=3):
    """A NaN coordinate, an infinite one, a point outside the box by a quarter and one by two box lengths."""
    Lx, Ly = float(box[0]), float(box[1])
    return np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.75 * Lx, 0.1, 0.0], [0.2, -2.0 * Ly - 0.3, 0.0]], np.float64)


def points_of(seed, position, box, dimensions=3, own=150, shape=(5, 4, 3), rnd=100):
    """The point set of a case: some of the particles' own positions, a `sample_grid` lattice, seeded random points and
    the special points, float64."""
    p = np.asarray(position, np.float64).reshape(-1, 3)
    shape = shape if dimensions == 3 else (shape[0], shape[1], 1)
    return np.concatenate([p[::max(1, len(p) // own)], hoomd.sample_grid(box, shape, dimensions),
                           random_rows(500 + seed, rnd, box, np.float64, dimensions), special_points(box, dimensions)])


def _case(k, name):
    p, mass, density, kw = SUM_CASES[name]
    kw = dict((key, value) for key, value in kw.items() if key != 'surface_below')
    return dict(points=points_of(k, p, kw['box'], kw.get('dimensions', 3)), position=p, values=value_arrays(k, len(p), 4),
                mass=mass, density=density, **kw)


# name -> keyword arguments of sph_samples.  A density that is stored nowhere is the schema's 0.0: every V of one_cell_65
# and mass_only is infinite.
CASES = dict((name, _case(k, name)) for k, name in enumerate(sorted(SUM_CASES)))
# (each chunk absent alone, and no value, over one geometry)
_P = SUM_CASES['mass_only'][0]
_BASE = dict(points=points_of(20, _P, CUBE), position=_P, values=value_arrays(20, 200, 4), mass=_columns(20, 200)[0],
             density=_columns(20, 200)[1], box=CUBE, h=0.75)
CASES['no_mass'] = dict(_BASE, mass=None)
CASES['no_density'] = dict(_BASE, density=None)
CASES['no_values'] = dict(_BASE, values=())
# (a lone particle: a point exactly 2h from it, one coinciding with it, one inside and one out of reach)
CASES['lone'] = dict(points=np.array([[1.5, 2, 3], [1, 2, 3], [1.25, 2, 3], [-3, -3, -3]], np.float64),
                     position=np.array([[1, 2, 3]], np.float64), values=[np.array([[2.0]])], mass=np.array([1.5]),
                     density=np.array([3.0]), box=CUBE, h=0.25)
# the points of a case the double loop takes (all of them up to this many; a strided subset beyond)
LOOP_POINTS = 200


def _cloud(seed, n=60):
    return random_rows(seed, n, CUBE, np.float64)


def _small(seed, n=60, cells=(2, 2, 2), K=40, **more):
    mass, density = _columns(seed, n)
    return dict(dict(points=random_rows(700 + seed, K, CUBE, np.float64), position=_cloud(seed, n), values=value_arrays(seed, n, 4),
                     mass=mass, density=density, box=CUBE, h=1.0, cells=cells), **more)


_LONE = dict(CASES['lone'])
# six entries at (-4.3, -3.4, NaN) of the flat box among 30 ordinary ones, two points beside them and ten elsewhere
_FLAT_LOST = dict(points=np.concatenate([[[-4.25, -3.35, 0.0], [-4.2, -3.3, 0.0]], random_rows(793, 10, FLAT, np.float64, 2)]),
                  position=np.concatenate([random_rows(93, 30, FLAT, np.float64, 2), [[-4.3, -3.4, np.nan]] * 6]),
                  values=value_arrays(93, 36, 4), mass=_columns(93, 36)[0], density=_columns(93, 36)[1], box=FLAT, h=0.3,
                  dimensions=2)
# name -> (the loop's switch, the case: keyword arguments of sph_samples).  Each case is a small one on which the mutated
# loop differs from the definition; the unmutated loop agrees with the model on every one of them.
MUTATIONS = {
    'the point rounded to float32 before its cell or its displacement': (dict(point_f32=True), _small(81)),
    '(V_j * f) * w': (dict(vf_first=True), _small(82)),
    'sigma inside the sum': (dict(sigma_inside=True), _small(83)),
    'normalised as (sigma*a_f) / (sigma*a_v)': (dict(normalise_scaled=True), _small(84, normalise=True)),
    'V_j formed in float32': (dict(v_f32=True), _small(85)),
    # (the first point lies exactly 2h from the lone particle: w is 0 there, the count is what shows)
    '<= for <': (dict(strict=False), _LONE),
    'descending j in a cell': (dict(descending_j=True), _small(86, 40, cells=(1, 1, 1))),
    'cells in ascending wrapped index': (dict(ascending_cells=True), _small(87, 120, cells=(3, 3, 3))),
    # (entries in the x columns 0 and 3 of four and points among them: every sum crosses the periodic wrap)
    'no minimum image': (dict(no_image=True), dict(points=SUM_CASES['four_cells_wrap'][0][:60] + 0.05,
                                                   position=SUM_CASES['four_cells_wrap'][0][:160], values=value_arrays(88, 160, 4),
                                                   mass=_columns(88, 160)[0], density=_columns(88, 160)[1], box=CUBE, h=1.0,
                                                   cells=(4, 4, 4))),
    'count of candidates visited instead of contributing': (dict(count_candidates=True), _small(89)),
    'a nowhere point given 0/0 under normalise': (dict(nowhere_nan=True), dict(_small(90, K=5), normalise=True,
                                                                              points=special_points(CUBE))),
    'outside judged on the wrapped fraction': (dict(outside_wrapped=True), dict(_small(91, K=5), points=special_points(CUBE))),
    # (2-D: z enters the x and y fractions -- 0 * NaN is a NaN --, so an entry with a NaN z is nowhere, but the 2-D
    # displacement never reads z: its d2 is finite, and only its missing cell keeps it out of the sums of the points beside it)
    'list entries that are nowhere contributing': (dict(lost_entries=True), _FLAT_LOST),
}
# A mutation no input can show.  d taken as x_p - x_j: only d2 is used, and the fold of -d is the negative of the fold of d
# except where a component sits exactly on half a box length, which is far outside the support.
EQUIVALENT = {
    'd taken as x_p - x_j': (dict(reversed_d=True), _small(92)),
}
