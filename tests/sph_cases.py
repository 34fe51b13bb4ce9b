"""What the SPH kernel-sum tests share: a plain double loop of the definition of `pgsd.hoomd.sph_kernel_sums` in Python
floats -- with switches that each stand for a kernel mistake --, the mutation table with the case on which each mutation
differs, and the constructed cases.  `test_sph_model.py` holds the model against the loop; `test_gpu_sph_sums.py` runs the
kernel on the same cases."""
import math
from fractions import Fraction

import numpy as np

import pgsd.hoomd as hoomd
from neighbours_cases import FLAT, TRICLINIC, fold, random_rows

NONE = 0xFFFFFFFF
CUBE = [8, 8, 8, 0, 0, 0]
WIDE = [64, 64, 64, 0, 0, 0]
KERNELS = hoomd.SPH_KERNELS


def fma(a, b, c):
    """a * b + c with one rounding, exactly (float() of a Fraction rounds to nearest, ties to even)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def weight(q, kernel, fused=False, branch_le=False):
    if kernel == 'wendland_c2':
        t = fma(-0.5, q, 1.0) if fused else 1.0 - 0.5 * q
        t2 = t * t
        return (t2 * t2) * (fma(2.0, q, 1.0) if fused else 2.0 * q + 1.0)
    q2 = q * q
    if q < 1.0 or (branch_le and q == 1.0):
        if fused:
            return fma(0.75, q2 * q, fma(-1.5, q2, 1.0))
        return (1.0 - 1.5 * q2) + 0.75 * (q2 * q)
    u = 2.0 - q
    return 0.25 * ((u * u) * u)


def loop_sums(position, box, h, mass=None, density=None, rows=None, cells=None, dimensions=3, kernel='wendland_c2',
              surface_below=None, ascending_cells=False, descending_j=False, skip_self=False, strict=True, sigma_inside=False,
              f32_accumulator=False, fused=False, q_divide=False, branch_le=False, v_f32=False):
    """The sums by a double loop over ordered pairs of list entries in plain Python floats: ``(words, number, density,
    shepard)`` in the layout of `pgsd.hoomd.KernelSums` (``shepard`` None without a density).  Every keyword from
    ``ascending_cells`` on is a mutation."""
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
    x = [[float(np.float64(c)) for c in p[k]] for k in rows_sorted]
    m = [1.0 if mass is None else float(np.float64(np.asarray(mass).reshape(-1)[k])) for k in rows_sorted]
    rho = None if density is None else [float(np.float64(np.asarray(density).reshape(-1)[k])) for k in rows_sorted]
    vol = None
    if rho is not None:
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            if v_f32:
                vol = [float(np.float32(a) / np.float32(b)) for a, b in zip(m, rho)]
            else:
                vol = [float(np.float64(a) / np.float64(b)) for a, b in zip(m, rho)]
    ids = [int(c) for c in cell_sorted]
    members = {}
    for k, c in enumerate(ids):
        members.setdefault(c, []).append(k)
    acc = (lambda a: float(np.float32(a))) if f32_accumulator else (lambda a: a)
    number, rho_sum, shepard = [0.0] * n, [0.0] * n, None if vol is None else [0.0] * n
    offsets = [hoomd._axis_offsets(c) for c in grid]
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(n):
            if ids[i] >= n_cells:
                continue
            at = (ids[i] % grid[0], (ids[i] // grid[0]) % grid[1], ids[i] // (grid[0] * grid[1]))
            a_n = a_m = a_v = 0.0
            for oz in offsets[2]:
                for oy in offsets[1]:
                    xcells = [(at[0] + ox) % grid[0] for ox in offsets[0]]
                    if ascending_cells:
                        xcells = sorted(xcells)
                    for wx in xcells:
                        wy, wz = (at[1] + oy) % grid[1], (at[2] + oz) % grid[2]
                        inside = members.get(wx + grid[0] * (wy + grid[1] * wz), ())
                        for j in (reversed(inside) if descending_j else inside):
                            if j == i and skip_self:
                                continue
                            d2 = fold([x[j][a] - x[i][a] for a in range(3)], v, dimensions)
                            if not (d2 < r2 or (not strict and d2 == r2)):
                                continue
                            rr = math.sqrt(d2)
                            q = rr / hh if q_divide else rr * inv_h
                            w = weight(q, kernel, fused, branch_le)
                            if sigma_inside:
                                w = sigma * w
                            # numpy scalars: inf * 0 and inf - inf are NaN, not an exception
                            a_n = acc(a_n + w)
                            a_m = acc(a_m + float(np.float64(m[j]) * np.float64(w)))
                            if vol is not None:
                                a_v = acc(a_v + float(np.float64(vol[j]) * np.float64(w)))
            scale = 1.0 if sigma_inside else sigma
            number[i], rho_sum[i] = scale * a_n, scale * a_m
            if vol is not None:
                shepard[i] = float(np.float64(scale) * np.float64(a_v))
    with_cell = [k for k in range(n) if ids[k] < n_cells]
    words = np.zeros(13, dtype=np.uint64)
    f = words[6:13].view(np.float64)
    words[0], words[1], words[4], words[5] = n, n - len(with_cell), NONE, NONE
    f[0:6:2], f[1:6:2] = math.inf, -math.inf
    for s, values in enumerate((number, rho_sum, shepard)):
        if values is None:
            continue
        for k in with_cell:
            if values[k] < f[2 * s]:
                f[2 * s] = values[k]
            if values[k] > f[2 * s + 1]:
                f[2 * s + 1] = values[k]
    words[2] = sum(1 for k in with_cell if not math.isfinite(rho_sum[k]))
    if vol is not None:
        if surface_below is not None:
            words[3] = sum(1 for k in with_cell if shepard[k] < surface_below)
        best = -1.0
        for k in with_cell:
            dev = float(np.float64(rho_sum[k]) - np.float64(rho[k]))
            if dev == dev and abs(dev) > best:
                best, f[6] = abs(dev), dev
                words[4], words[5] = k, int(rows_sorted[k])
    return (words, np.array(number, dtype=np.float64), np.array(rho_sum, dtype=np.float64),
            None if shepard is None else np.array(shepard, dtype=np.float64))


def bits_equal(a, b):
    """Two float64 arrays bit for bit; a NaN equals a NaN (IEEE 754 leaves its sign and payload to the processor)."""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    nan = a != a
    return a.shape == b.shape and np.array_equal(nan, b != b) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def words_equal(a, b):
    """Two summaries: the six integer words exactly, the seven float words as `bits_equal`."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return np.array_equal(a[:6], b[:6]) and bits_equal(a[6:].view(np.float64), b[6:].view(np.float64))


def same(got, want):
    """Is the model's (or the kernel's, copied to the host) `KernelSums` the loop's result, bit for bit?"""
    words, number, rho_sum, shepard = want
    return (words_equal(got.summary, words) and bits_equal(got.number, number) and bits_equal(got.density, rho_sum)
            and ((got.shepard is None) == (shepard is None)) and (shepard is None or bits_equal(got.shepard, shepard)))


def _through(box, f):
    """Fractions in [0, 1) (or slightly outside) -> real coordinates of the box, float64."""
    Lx, Ly, Lz, xy, xz, yz = [float(np.float32(b)) for b in box]
    g = np.asarray(f, np.float64) - 0.5
    z = g[:, 2] * Lz
    y = g[:, 1] * Ly + yz * z
    return np.stack([g[:, 0] * Lx + xy * (g[:, 1] * Ly) + xz * z, y, z], axis=1)


def _faces():
    """Rows on cell faces of the (7, 5, 4) grid, at fraction 0 and just below 1 and slightly outside the box, a partner a
    short way off each of them, and a random filling."""
    fx = [0.0, 1 / 7, 2 / 7, 0.5, 0.9999999, -0.005, 1.004]
    fy = [0.0, 0.2, 0.5, 0.9999999, 1.003]
    fz = [0.0, 0.25, 0.9999999, -0.004]
    base = _through(TRICLINIC, np.array([(a, b, c) for a in fx for b in fy for c in fz]))
    rng = np.random.default_rng(21)
    return np.concatenate([base, base + rng.uniform(-0.6, 0.6, size=base.shape), random_rows(5, 600, TRICLINIC, np.float64)])


def _with_lost_rows(p, every=97):
    p = p.copy()
    p[5::every, 0] = np.nan
    p[11::every, 1] = np.inf
    return p


def _wrap_columns():
    """Entries in the x columns ix = 0 and ix = 3 of a (4, 4, 4) grid only: every sum crosses the periodic wrap."""
    p = random_rows(12, 400, CUBE, np.float64)
    p[:, 0] = np.where(p[:, 0] < 0, -4.0 + (p[:, 0] + 4.0) * 0.5, 2.0 + p[:, 0] * 0.5)
    return p


def _clump():
    """700 entries inside one cell of the (3, 3, 3) grid -- a sum longer than a workgroup -- and a few rows elsewhere."""
    rng = np.random.default_rng(8)
    return np.concatenate([rng.uniform(-0.5, 0.5, size=(700, 3)), [[3.5, 3.5, 3.5], [3.6, 3.5, 3.5], [-3.9, 0, 0]]])


def _sparse():
    """3 000 rows in 64^3 cells: mostly empty cells; 750 of the rows have a partner inside the support."""
    a = random_rows(9, 2250, WIDE, np.float64)
    return np.concatenate([a, a[:750] + np.random.default_rng(10).uniform(-0.5, 0.5, size=(750, 3))])


def _boundary():
    """h = 0.25, all exact in float32: a pair at exactly 2h = 0.5 (rows 0, 1; row 1 has density 0, so that counting it
    shows as a NaN), a row stored twice (2, 3: distance 0, w = 1), a pair at exactly q = 1 (4, 5) and pairs one float64 ulp
    either side of it (6, 7 and 8, 9; float32 chunks round them onto q = 1)."""
    below, above = np.nextafter(0.25, 0), np.nextafter(0.25, 1)
    return np.array([[0, 0, 0], [0.5, 0, 0], [2, 2, 2], [2, 2, 2], [-2, 0, 0], [-2, 0.25, 0], [0, -2, 0], [0, -2, below],
                     [0, 2, 0], [above, 2, 0]], np.float64)


def _columns(seed, n, zero=None, nan=None):
    """A mass and a density column: masses in [0.5, 2), densities around 1000; one density 0 and one NaN on demand."""
    rng = np.random.default_rng(seed)
    mass, density = rng.uniform(0.5, 2.0, size=n), 1000.0 + 50.0 * rng.standard_normal(n)
    if zero is not None:
        density[zero] = 0.0
    if nan is not None:
        density[nan] = np.nan
    return mass, density


# name -> (positions as float64, mass or None, density or None, keyword arguments of sph_kernel_sums besides those).
# The smallest shapes at which the kernel can go wrong; h is exact in float32.
CASES = {
    'one_cell_65': (random_rows(1, 65, CUBE, np.float64), None, None, dict(box=CUBE, h=1.0, cells=(1, 1, 1))),
    'two_cells_64': (random_rows(2, 64, CUBE, np.float64),) + _columns(2, 64) + (dict(box=CUBE, h=1.0, cells=(2, 2, 2)),),
    'three_cells': (_with_lost_rows(random_rows(4, 4097, CUBE, np.float64)),) + _columns(4, 4097)
    + (dict(box=CUBE, h=1.0, cells=(3, 3, 3)),),
    'four_cells_wrap': (_wrap_columns(),) + _columns(12, 400) + (dict(box=CUBE, h=1.0, cells=(4, 4, 4)),),
    'triclinic_754': (_faces(),) + _columns(5, len(_faces())) + (dict(box=TRICLINIC, h=0.625, cells=(7, 5, 4)),),
    'flat': (random_rows(3, 300, FLAT, np.float64, 3),) + _columns(3, 300) + (dict(box=FLAT, h=0.375, dimensions=2),),
    'clump_700': (_clump(),) + _columns(8, 703) + (dict(box=CUBE, h=1.0, cells=(3, 3, 3)),),
    'sparse_64cubed': (_sparse(),) + _columns(9, 3000) + (dict(box=WIDE, h=0.5, cells=(64, 64, 64)),),
    'boundary': (_boundary(), np.ones(10), np.array([1, 0, 1, 1, 1, 1, 1, 1, 1, 1], np.float64), dict(box=CUBE, h=0.25)),
    'mass_density': (random_rows(13, 500, CUBE, np.float64),) + _columns(13, 500, zero=17, nan=123)
    + (dict(box=CUBE, h=0.75, surface_below=0.5),),
    'mass_only': (random_rows(14, 200, CUBE, np.float64), _columns(14, 200)[0], None, dict(box=CUBE, h=0.75)),
    'density_only': (random_rows(15, 200, CUBE, np.float64), None, _columns(15, 200)[1], dict(box=CUBE, h=0.75)),
    'all_nowhere': (np.full((100, 3), np.nan),) + _columns(16, 100) + (dict(box=CUBE, h=0.5),),
}
# the entries of a case the double loop takes (all of them up to this many; a strided sub-list beyond)
LOOP_ENTRIES = 800


def _cloud(seed, n=60, dtype=np.float64):
    return random_rows(seed, n, CUBE, dtype)


# name -> (the loop's switch, the case: keyword arguments of sph_kernel_sums).  Each case is a small one on which the
# mutated loop differs from the definition; the unmutated loop agrees with the model on every one of them.
MUTATIONS = {
    'cells in ascending wrapped index': (dict(ascending_cells=True),
                                         dict(position=_cloud(31, 120), box=CUBE, h=1.0, cells=(3, 3, 3))),
    'j descending inside a cell': (dict(descending_j=True), dict(position=_cloud(32, 40), box=CUBE, h=1.0, cells=(1, 1, 1))),
    'self excluded': (dict(skip_self=True), dict(position=np.array([[1, 2, 3]], np.float32), box=CUBE, h=0.5)),
    '<= for <': (dict(strict=False),
                 dict(position=np.array([[0, 0, 0], [0.5, 0, 0]], np.float32), box=CUBE, h=0.25,
                      density=np.array([1, 0], np.float32))),
    'sigma multiplied inside the sum': (dict(sigma_inside=True), dict(position=_cloud(33), box=CUBE, h=1.0, cells=(2, 2, 2))),
    'a float32 accumulator': (dict(f32_accumulator=True), dict(position=_cloud(34), box=CUBE, h=1.0, cells=(2, 2, 2))),
    "the spline's inner polynomial with fused multiply-adds": (
        # (a dense cloud: many pairs below q = 1, where one ulp of w survives the addition to the sum now and then)
        dict(fused=True), dict(position=np.random.default_rng(35).uniform(-0.6, 0.6, size=(120, 3)), box=CUBE, h=1.0,
                               cells=(2, 2, 2), kernel='cubic_spline')),
    'q = rr / h': (dict(q_divide=True), dict(position=_cloud(36), box=CUBE, h=0.7, cells=(2, 2, 2))),
    'V_j formed in float32': (dict(v_f32=True),
                              dict(position=_cloud(37), box=CUBE, h=1.0, cells=(2, 2, 2), mass=_columns(37, 60)[0],
                                   density=_columns(37, 60)[1])),
}
# Mutations no input can show.  At q == 1 both branches of the cubic spline give 0.25 exactly ((1 - 1.5) + 0.75 and
# 0.25 * 1), so `q <= 1` for `q < 1` changes no result; the case puts pairs at q == 1 and an ulp either side of it.  The
# Wendland kernel's fused forms fma(-0.5, q, 1) and fma(2, q, 1) round once where the plain forms round twice, but 0.5 * q
# and 2 * q are exact (a power of two), so both give the same double for every q in [0, 2]: its contraction is harmless,
# the spline's (`MUTATIONS`) is not.
EQUIVALENT = {
    'the Wendland kernel with fused multiply-adds': (dict(fused=True),
                                                     dict(position=_cloud(35), box=CUBE, h=1.0, cells=(2, 2, 2))),
    "the spline's branch taken at q <= 1": (dict(branch_le=True),
                                            dict(position=_boundary(), box=CUBE, h=0.25, kernel='cubic_spline')),
}
