"""What the tests of the SPH sums with a per-particle smoothing length share: a plain double loop of the definition of
`pgsd.hoomd.sph_adaptive_sums` in Python floats -- with switches that each stand for a kernel mistake --, the mutation
table with the case on which each mutation differs, the seeded ``h`` columns of the shared SPH cases and the constructed
clouds of the physics checks.  `test_sph_adaptive_model.py` holds the model against the loop; `test_gpu_sph_adaptive.py`
runs the kernel on the same cases."""
import math

import numpy as np

import pgsd.hoomd as hoomd
from neighbours_cases import fold, random_rows
from sph_cases import CASES as SUM_CASES, CUBE, NONE, bits_equal, fma

MODES = hoomd.SPH_MODES
FLAT8 = [8, 8, 1, 0, 0, 0]


def valid(h):
    return h > 0.0 and h < math.inf


def sigma_of(kernel, hh, dimensions):
    pi = math.pi
    if dimensions == 3:
        return 21.0 / (16.0 * pi * (hh * hh * hh)) if kernel == 'wendland_c2' else 1.0 / (pi * (hh * hh * hh))
    return 7.0 / (4.0 * pi * (hh * hh)) if kernel == 'wendland_c2' else 10.0 / (7.0 * pi * (hh * hh))


def weight(q, kernel, fused=False):
    if kernel == 'wendland_c2':
        t = fma(-0.5, q, 1.0) if fused else 1.0 - 0.5 * q
        t2 = t * t
        return (t2 * t2) * (fma(2.0, q, 1.0) if fused else 2.0 * q + 1.0)
    q2 = q * q
    if q < 1.0:
        return (1.0 - 1.5 * q2) + 0.75 * (q2 * q)
    u = 2.0 - q
    return 0.25 * ((u * u) * u)


def factor(q, kernel, fused=False):
    if kernel == 'wendland_c2':
        t = fma(-0.5, q, 1.0) if fused else 1.0 - 0.5 * q
        return -5.0 * ((t * t) * t)
    if q < 1.0:
        return 2.25 * q - 3.0
    u = 2.0 - q
    return float(np.float64(-0.75 * (u * u)) / np.float64(q))


def loop_adaptive(position, box, slength, mass=None, density=None, rows=None, cells=None, dimensions=3, kernel='wendland_c2',
                  mode='gather', surface_below=None, strict=True, support_from_hj=False, q_from_hj=False, sigma_inside=False,
                  p_outside=False, hij_geometric=False, s2_from_hij=False, q_times_f=False, d_always_3=False,
                  bad_h_source=False, skip_self=False, descending_j=False, f32_accumulator=False, fused=False,
                  fused_weight=False):
    """The sums by a double loop over ordered pairs of list entries in plain Python floats: ``(words, count, number,
    density, shepard, omega)`` in the layout of `pgsd.hoomd.AdaptiveSums` (``shepard`` None without a density, ``omega``
    None in mean mode).  Every keyword from ``strict`` on is a mutation."""
    p = np.asarray(position).reshape(-1, 3)
    s = np.asarray(slength).reshape(-1).astype(np.float64)
    every = np.arange(len(p)) if rows is None else np.asarray(rows)
    listed = [float(s[k]) for k in every]
    h_max = max([hh for hh in listed if valid(hh)], default=-math.inf)
    gather = mode == 'gather'
    if len(every):
        support = float(np.float64(2.0) * np.float64(h_max))
        grid = hoomd.neighbour_grid_for(box, support, dimensions) if cells is None else tuple(int(c) for c in cells)
    else:
        grid = (1, 1, 1) if cells is None else tuple(int(c) for c in cells)
    rows_sorted, cell_sorted, _ = hoomd.cell_order(p, box, every, grid, dimensions)
    n, n_cells = len(rows_sorted), grid[0] * grid[1] * grid[2]
    v = [float(x) for x in hoomd.box_vectors(np.asarray(box, np.float32))]
    x = [[float(np.float64(c)) for c in p[k]] for k in rows_sorted]
    h = [float(s[k]) for k in rows_sorted]
    m = [1.0 if mass is None else float(np.float64(np.asarray(mass).reshape(-1)[k])) for k in rows_sorted]
    rho = None if density is None else [float(np.float64(np.asarray(density).reshape(-1)[k])) for k in rows_sorted]
    vol = None
    if rho is not None:
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            vol = [float(np.float64(a) / np.float64(b)) for a, b in zip(m, rho)]
    ids = [int(c) for c in cell_sorted]
    members = {}
    for k, c in enumerate(ids):
        members.setdefault(c, []).append(k)
    acc = (lambda a: float(np.float32(a))) if f32_accumulator else (lambda a: a)
    D = 3.0 if dimensions == 3 or d_always_3 else 2.0
    C = sigma_of(kernel, 1.0, dimensions)
    count, number, rho_sum = [0] * n, [0.0] * n, [0.0] * n
    shepard = None if vol is None else [0.0] * n
    omega = [0.0] * n if gather else None
    offsets = [hoomd._axis_offsets(c) for c in grid]
    live = [ids[k] < n_cells and valid(h[k]) for k in range(n)]
    f64 = np.float64
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for i in range(n):
            if not live[i]:
                continue
            at = (ids[i] % grid[0], (ids[i] // grid[0]) % grid[1], ids[i] // (grid[0] * grid[1]))
            a_n = a_m = a_v = a_o = 0.0
            for oz in offsets[2]:
                for oy in offsets[1]:
                    for ox in offsets[0]:
                        wx, wy, wz = (at[0] + ox) % grid[0], (at[1] + oy) % grid[1], (at[2] + oz) % grid[2]
                        inside = members.get(wx + grid[0] * (wy + grid[1] * wz), ())
                        for j in (reversed(inside) if descending_j else inside):
                            if j == i and skip_self:
                                continue
                            if not valid(h[j]) and not (bad_h_source and gather):
                                continue
                            d2 = fold([x[j][a] - x[i][a] for a in range(3)], v, dimensions)
                            if gather:
                                hs, hq = (h[j] if support_from_hj else h[i]), (h[j] if q_from_hj else h[i])
                                si = 2.0 * hs
                                r2 = si * si
                                ih = float(f64(1.0) / f64(hq))
                            else:
                                sij = h[i] + h[j]
                                hij = math.sqrt(h[i] * h[j]) if hij_geometric else 0.5 * sij
                                r2 = (4.0 * hij) * hij if s2_from_hij else sij * sij
                                ih = float(f64(1.0) / f64(hij))
                            if not (d2 < r2 or (not strict and d2 == r2)):
                                continue
                            q = math.sqrt(d2) * ih
                            w = weight(q, kernel, fused or fused_weight)
                            if gather:
                                F = factor(q, kernel, fused or fused_weight)
                                if q_times_f:
                                    term = D * w + q * F
                                elif fused:
                                    term = fma(q * q, F, D * w)
                                else:
                                    term = D * w + (q * q) * F
                                a_o = acc(a_o + float(f64(m[j]) * f64(term)))
                                if sigma_inside:
                                    w = sigma_of(kernel, h[i], dimensions) * w
                            elif not p_outside:
                                w = w * ((ih * ih) * ih if dimensions == 3 else ih * ih)
                            a_n = acc(a_n + w)
                            a_m = acc(a_m + float(f64(m[j]) * f64(w)))
                            if vol is not None:
                                a_v = acc(a_v + float(f64(vol[j]) * f64(w)))
                            count[i] += 1
            if gather:
                scale = 1.0 if sigma_inside else sigma_of(kernel, h[i], dimensions)
            else:
                scale = C
                if p_outside:
                    ii = float(f64(1.0) / f64(h[i]))
                    scale = C * ((ii * ii) * ii if dimensions == 3 else ii * ii)
            number[i], rho_sum[i] = float(f64(scale) * f64(a_n)), float(f64(scale) * f64(a_m))
            if vol is not None:
                shepard[i] = float(f64(scale) * f64(a_v))
            if gather:
                omega[i] = float(f64(1.0) - f64(a_o) / (f64(D) * f64(a_m)))
    with_cell = [k for k in range(n) if ids[k] < n_cells]
    alive = [k for k in range(n) if live[k]]
    words = np.zeros(22, dtype=np.uint64)
    f = words[10:21].view(np.float64)
    words[0], words[1], words[2] = n, n - len(with_cell), len(with_cell) - len(alive)
    words[5] = words[6] = words[9] = NONE
    f[0:10:2], f[1:10:2] = math.inf, -math.inf
    for s_, values in enumerate((h, number, rho_sum, shepard, omega)):
        if values is None:
            continue
        for k in alive:
            if values[k] < f[2 * s_]:
                f[2 * s_] = values[k]
            if values[k] > f[2 * s_ + 1]:
                f[2 * s_ + 1] = values[k]
    words[3] = sum(1 for k in alive if not math.isfinite(rho_sum[k]))
    for k in alive:
        if int(words[9]) == NONE or count[k] < int(words[7]):
            words[7], words[9] = count[k], k
        words[8] = max(int(words[8]), count[k])
    words[21] = sum(count)
    if vol is not None:
        if surface_below is not None:
            words[4] = sum(1 for k in alive if shepard[k] < surface_below)
        best = -1.0
        for k in alive:
            dev = float(f64(rho_sum[k]) - f64(rho[k]))
            if dev == dev and abs(dev) > best:
                best, f[10] = abs(dev), dev
                words[5], words[6] = k, int(rows_sorted[k])
    return (words, np.array(count, dtype=np.uint32), np.array(number), np.array(rho_sum),
            None if shepard is None else np.array(shepard), None if omega is None else np.array(omega))


def words_equal(a, b):
    """Two summaries: the integer words exactly, the eleven float words as `bits_equal`."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return (np.array_equal(a[:10], b[:10]) and a[21] == b[21]
            and bits_equal(a[10:21].view(np.float64), b[10:21].view(np.float64)))


def same(got, want):
    """Is the model's (or the kernel's, copied to the host) `AdaptiveSums` the loop's result, bit for bit?"""
    words, count, number, rho_sum, shepard, omega = want
    if not (words_equal(got.summary, words) and np.array_equal(got.count, count) and bits_equal(got.number, number)
            and bits_equal(got.density, rho_sum)):
        return False
    for mine, theirs in ((got.shepard, shepard), (got.omega, omega)):
        if (mine is None) != (theirs is None) or (theirs is not None and not bits_equal(mine, theirs)):
            return False
    return True


def seeded_h(name, n, h, lo=0.6, hi=1.0, dtype=np.float64):
    """The case's per-row smoothing lengths: seeded, in ``[lo, hi]`` times the case's ``h`` (the case's own grid stays
    legal: no listed ``h`` exceeds the one it was made for), rounded to ``dtype``."""
    rng = np.random.default_rng(sum(name.encode()) + 1000)
    return (rng.uniform(lo, hi, size=n) * h).astype(dtype)


def adaptive_case(name):
    """``(position, mass, density, keyword arguments without h, h)`` of a shared SPH case."""
    p, mass, density, kw = SUM_CASES[name]
    kw = dict(kw)
    h = kw.pop('h')
    return p, mass, density, kw, h


def _cloud(seed, n=60, box=CUBE, dims=3):
    p = random_rows(seed, n, box, np.float64, dims)
    return p


def _h(seed, n, lo, hi):
    return np.random.default_rng(seed).uniform(lo, hi, size=n)


def _columns(seed, n):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, size=n), 1000.0 + 50.0 * rng.standard_normal(n)


def _bad_source():
    """Row 1 has h = 0 and sits inside the support of row 0."""
    return dict(position=np.array([[0, 0, 0], [0.3, 0, 0], [0, 0.4, 0]], np.float64), box=CUBE,
                slength=np.array([0.5, 0.0, 0.5]), mode='gather')


# name -> (the loop's switch, the case: keyword arguments of sph_adaptive_sums).  Each case is a small one on which the
# mutated loop differs from the definition; the unmutated loop agrees with the model on every one of them.
MUTATIONS = {
    '<= for < (gather)': (dict(strict=False), dict(position=np.array([[0, 0, 0], [0.5, 0, 0]], np.float32), box=CUBE,
                                                   slength=np.array([0.25, 0.25], np.float32),
                                                   density=np.array([1, 0], np.float32), mode='gather')),
    '<= for < (mean)': (dict(strict=False), dict(position=np.array([[0, 0, 0], [0.5, 0, 0]], np.float32), box=CUBE,
                                                 slength=np.array([0.375, 0.125], np.float32),
                                                 density=np.array([1, 0], np.float32), mode='mean')),
    'the support from h_j in gather mode': (dict(support_from_hj=True),
                                            dict(position=_cloud(41), box=CUBE, slength=_h(41, 60, 0.5, 1.0), cells=(2, 2, 2),
                                                 mode='gather')),
    'q from h_j': (dict(q_from_hj=True), dict(position=_cloud(42), box=CUBE, slength=_h(42, 60, 0.5, 1.0), cells=(2, 2, 2),
                                              mode='gather')),
    'sigma multiplied inside the sum (gather)': (dict(sigma_inside=True),
                                                 dict(position=_cloud(43), box=CUBE, slength=_h(43, 60, 0.6, 1.0), cells=(2, 2, 2),
                                                      mode='gather')),
    'p outside the sum (mean)': (dict(p_outside=True), dict(position=_cloud(44), box=CUBE, slength=_h(44, 60, 0.5, 1.0),
                                                            cells=(2, 2, 2), mode='mean')),
    'hij as sqrt(h_i h_j)': (dict(hij_geometric=True), dict(position=_cloud(45), box=CUBE, slength=_h(45, 60, 0.5, 1.0),
                                                            cells=(2, 2, 2), mode='mean')),
    'q*F for (q*q)*F': (dict(q_times_f=True), dict(position=_cloud(46), box=CUBE, slength=_h(46, 60, 0.6, 1.0), cells=(2, 2, 2),
                                                   mode='gather')),
    'D fixed at 3 in 2-D': (dict(d_always_3=True), dict(position=_cloud(47, 80, FLAT8, 2), box=FLAT8, slength=_h(47, 80, 0.4, 0.6),
                                                        dimensions=2, mode='gather')),
    'a bad-h entry kept as a source': (dict(bad_h_source=True), _bad_source()),
    'self excluded': (dict(skip_self=True), dict(position=np.array([[1, 2, 3]], np.float32), box=CUBE,
                                                 slength=np.array([0.5], np.float32), mode='gather')),
    'j descending inside a cell': (dict(descending_j=True), dict(position=_cloud(48, 40), box=CUBE, slength=_h(48, 40, 0.6, 1.0),
                                                                 cells=(1, 1, 1), mode='mean')),
    'a float32 accumulator': (dict(f32_accumulator=True), dict(position=_cloud(49), box=CUBE, slength=_h(49, 60, 0.6, 1.0),
                                                               cells=(2, 2, 2), mode='gather')),
    'the Wendland polynomial and the omega term with fused multiply-adds': (
        dict(fused=True), dict(position=np.random.default_rng(50).uniform(-0.6, 0.6, size=(120, 3)), box=CUBE,
                               slength=_h(50, 120, 0.6, 1.0), cells=(2, 2, 2), kernel='wendland_c2', mode='gather',
                               mass=_columns(50, 120)[0])),
}
# Mutations no input can show.  `s*s` as `(4.0*hij)*hij`: hij = 0.5*s and 4.0*hij = 2*s are exact (powers of two), so
# (2s)*(0.5s) and s*s are the same real product and round to the same double for every s that neither overflows nor
# underflows.  The Wendland weight and factor with fused multiply-adds alone: 0.5*q and 2*q are exact, so fma(-0.5, q, 1)
# and fma(2, q, 1) round once to the same double as the plain forms (tests/sph_cases.py says the same of the uniform
# pass); the contraction that does show is the omega term's D*w + (q*q)*F (`MUTATIONS`).
EQUIVALENT = {
    's*s as 4*hij*hij': (dict(s2_from_hij=True), dict(position=_cloud(51, 200), box=CUBE, slength=_h(51, 200, 0.5, 1.0),
                                                      cells=(2, 2, 2), mode='mean')),
    'the Wendland weight and factor alone with fused multiply-adds': (
        dict(fused_weight=True), dict(position=_cloud(52, 120), box=CUBE, slength=_h(52, 120, 0.6, 1.0), cells=(2, 2, 2),
                                      kernel='wendland_c2', mode='gather')),
}


# ---------------------------------------------------------------- the constructed clouds of the physics checks
def lattice(dimensions, side=12):
    """A ``side``^D lattice of spacing 1 in the middle of a box of twice that side (its faces are open: nothing wraps
    inside a support), unit masses, ``h`` seeded in [1.0, 1.6]:
    ``(position, box, slength, interior)``; ``interior``: the rows at least 4 from every face."""
    axis = np.arange(side) - side / 2 + 0.5
    if dimensions == 3:
        p = np.array([(a, b, c) for c in axis for b in axis for a in axis], np.float64)
        box = [2 * side, 2 * side, 2 * side, 0, 0, 0]
    else:
        p = np.array([(a, b, 0.0) for b in axis for a in axis], np.float64)
        box = [2 * side, 2 * side, 1, 0, 0, 0]
    h = np.random.default_rng(60 + dimensions).uniform(1.0, 1.6, size=len(p))
    edge = (side - 1) / 2 - 4
    interior = np.all(np.abs(p[:, :dimensions]) <= edge, axis=1)
    return p, box, h, interior


def jittered(seed=70, side=8):
    """A seeded jittered ``side``^3 cloud (+-0.3) in a periodic box, ``h`` in [1.2, 1.5], masses in [0.5, 2):
    ``(position, box, slength, mass)``."""
    axis = np.arange(side) - side / 2 + 0.5
    rng = np.random.default_rng(seed)
    p = np.array([(a, b, c) for c in axis for b in axis for a in axis], np.float64) + rng.uniform(-0.3, 0.3, size=(side ** 3, 3))
    return p, [side, side, side, 0, 0, 0], rng.uniform(1.2, 1.5, size=side ** 3), rng.uniform(0.5, 2.0, size=side ** 3)


def derivative_error(p, box, h, mass, density_of, omega, density, step=1e-4):
    """The worst relative difference between ``-(sigma_i/h_i) a_o``, recovered as ``(omega - 1) * D * density / h_i``, and
    the central difference of the gather density in ``h_i`` at relative step ``step``; ``density_of(slength)`` gives the
    per-row density (in row order) for a column.  Every row's own ``h`` is varied at once: gather mode does not look at
    ``h_j``."""
    up, down = density_of(h * (1.0 + step)), density_of(h * (1.0 - step))
    numeric = (up - down) / (h * (1.0 + step) - h * (1.0 - step))
    analytic = (omega - 1.0) * 3.0 * density / h
    return float(np.max(np.abs(analytic - numeric) / np.abs(numeric)))
