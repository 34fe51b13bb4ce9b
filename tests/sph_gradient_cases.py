"""What the SPH kernel-gradient tests share: a plain double loop of the definition of `pgsd.hoomd.sph_kernel_gradients` in
Python floats -- with switches that each stand for a kernel mistake --, the mutation table with the case on which each
mutation differs, and the constructed cases: the geometry of `sph_cases.CASES` with seeded velocity columns.
`test_sph_gradient_model.py` holds the model against the loop; `test_gpu_sph_gradients.py` runs the kernel on the same
cases."""
import math

import numpy as np

import pgsd.hoomd as hoomd
from sph_cases import CASES as SUM_CASES, CUBE, KERNELS, NONE, bits_equal, fma  # noqa: F401

LOOP_ENTRIES = 800


def displacement(xi, xj, v, dimensions, minimum_image=True):
    """x_j - x_i under HOOMD's single-shift minimum image, z then y then x, in Python floats."""
    dx, dy, dz = xj[0] - xi[0], xj[1] - xi[1], (xj[2] - xi[2] if dimensions == 3 else 0.0)
    if not minimum_image:
        return dx, dy, dz
    if dimensions == 3:
        if dz >= v[2] / 2:
            dx, dy, dz = dx - v[4], dy - v[5], dz - v[2]
        elif dz < -(v[2] / 2):
            dx, dy, dz = dx + v[4], dy + v[5], dz + v[2]
    if dy >= v[1] / 2:
        dx, dy = dx - v[3], dy - v[1]
    elif dy < -(v[1] / 2):
        dx, dy = dx + v[3], dy + v[1]
    if dx >= v[0] / 2:
        dx -= v[0]
    elif dx < -(v[0] / 2):
        dx += v[0]
    return dx, dy, dz


def factor(q, kernel, reciprocal=False, fused=False):
    if kernel == 'wendland_c2':
        t = fma(-0.5, q, 1.0) if fused else 1.0 - 0.5 * q
        return -5.0 * ((t * t) * t)
    if q < 1.0:
        return 2.25 * q - 3.0
    u = 2.0 - q
    return (-0.75 * (u * u)) * (1.0 / q) if reciprocal else (-0.75 * (u * u)) / q


def loop_gradients(position, velocity, box, h, mass=None, density=None, rows=None, cells=None, dimensions=3,
                   kernel='wendland_c2', reversed_d=False, raw_e=False, g_inside=False, fused_dot=False, dot_right=False,
                   u_cross_e=False, ve_dot_u=False, u_f32=False, reciprocal=False, fused_factor=False, strict=True, skip_self=False,
                   descending_j=False, ascending_cells=False):
    """The gradients by a double loop over ordered pairs of list entries in plain Python floats: ``(words, density_rate,
    divergence, curl, normal)`` in the layout of `pgsd.hoomd.KernelGradients` (the last three None without a density).
    Every keyword from ``reversed_d`` on is a mutation."""
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
    G = -((sigma * inv_h) * inv_h)
    x = [[float(np.float64(c)) for c in p[k]] for k in rows_sorted]
    raw_w = np.zeros((len(p), 3)) if velocity is None else np.asarray(velocity).reshape(-1, 3)
    w = [[float(np.float64(c)) for c in raw_w[k]] for k in rows_sorted]
    m = [1.0 if mass is None else float(np.float64(np.asarray(mass).reshape(-1)[k])) for k in rows_sorted]
    vol = None
    if density is not None:
        rho = [float(np.float64(np.asarray(density).reshape(-1)[k])) for k in rows_sorted]
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            vol = [float(np.float64(a) / np.float64(b)) for a, b in zip(m, rho)]
    ids = [int(c) for c in cell_sorted]
    members = {}
    for k, c in enumerate(ids):
        members.setdefault(c, []).append(k)
    rate = [0.0] * n
    divergence, curl, normal = (None, None, None) if vol is None else ([0.0] * n, [[0.0] * 3 for _ in range(n)],
                                                                       [[0.0] * 3 for _ in range(n)])
    offsets = [hoomd._axis_offsets(c) for c in grid]
    scale = G if g_inside else 1.0
    for i in range(n):
        if ids[i] >= n_cells:
            continue
        at = (ids[i] % grid[0], (ids[i] // grid[0]) % grid[1], ids[i] // (grid[0] * grid[1]))
        a_r = a_d = 0.0
        a_w, a_c = [0.0] * 3, [0.0] * 3
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
                        d = displacement(x[j], x[i], v, dimensions) if reversed_d else displacement(x[i], x[j], v, dimensions)
                        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                        if not (d2 < r2 or (not strict and d2 == r2)):
                            continue
                        if raw_e:
                            d = displacement(x[i], x[j], v, dimensions, minimum_image=False)
                        q = math.sqrt(d2) * inv_h
                        F = factor(q, kernel, reciprocal, fused_factor) * scale
                        e = [F * d[0], F * d[1], F * d[2]]
                        if u_f32:
                            u = [float(np.float32(raw_w[rows_sorted[j]][k]) - np.float32(raw_w[rows_sorted[i]][k])) for k in range(3)]
                        else:
                            u = [w[j][k] - w[i][k] for k in range(3)]
                        if fused_dot:
                            dot = fma(u[2], e[2], fma(u[1], e[1], u[0] * e[0]))
                        elif dot_right:
                            dot = u[0] * e[0] + (u[1] * e[1] + u[2] * e[2])
                        else:
                            dot = (u[0] * e[0] + u[1] * e[1]) + u[2] * e[2]
                        a_r = a_r + m[j] * dot
                        if vol is None:
                            continue
                        V = vol[j]
                        c = [e[1] * u[2] - e[2] * u[1], e[2] * u[0] - e[0] * u[2], e[0] * u[1] - e[1] * u[0]]
                        if u_cross_e:
                            c = [u[1] * e[2] - u[2] * e[1], u[2] * e[0] - u[0] * e[2], u[0] * e[1] - u[1] * e[0]]
                        if ve_dot_u:
                            a_d = a_d + (((V * e[0]) * u[0] + (V * e[1]) * u[1]) + (V * e[2]) * u[2])
                        else:
                            a_d = a_d + V * dot
                        for k in range(3):
                            a_w[k] = a_w[k] + V * c[k]
                            a_c[k] = a_c[k] + V * e[k]
        last = 1.0 if g_inside else G
        rate[i] = -(last * a_r)
        if vol is not None:
            divergence[i] = last * a_d
            curl[i] = [last * a for a in a_w]
            normal[i] = [last * a for a in a_c]
    with_cell = [k for k in range(n) if ids[k] < n_cells]
    words = np.zeros(13, dtype=np.uint64)
    f = words[7:13].view(np.float64)
    words[0], words[1], words[3:7] = n, n - len(with_cell), NONE
    f[0:4:2], f[1:4:2] = math.inf, -math.inf
    for s, values in enumerate((divergence, rate)):
        if values is None:
            continue
        for k in with_cell:
            if values[k] < f[2 * s]:
                f[2 * s] = values[k]
            if values[k] > f[2 * s + 1]:
                f[2 * s + 1] = values[k]
    words[2] = sum(1 for k in with_cell if not math.isfinite(rate[k]))
    for s, values in enumerate((curl, normal)):
        if values is None:
            continue
        best = -1.0
        for k in with_cell:
            c = values[k]
            norm2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
            if norm2 == norm2 and norm2 > best:
                best = f[4 + s] = norm2
                words[3 + 2 * s], words[4 + 2 * s] = k, int(rows_sorted[k])
    as_array = lambda a, shape: None if a is None else np.array(a, dtype=np.float64).reshape(shape)  # noqa: E731
    return (words, as_array(rate, (n,)), as_array(divergence, (n,)), as_array(curl, (n, 3)), as_array(normal, (n, 3)))


def words_equal(a, b):
    """Two summaries: the seven integer words exactly, the six float words as `bits_equal`."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return np.array_equal(a[:7], b[:7]) and bits_equal(a[7:].view(np.float64), b[7:].view(np.float64))


def same(got, want):
    """Is the model's (or the kernel's, copied to the host) `KernelGradients` the loop's result, bit for bit?"""
    words, rate, divergence, curl, normal = want
    if not (words_equal(got.summary, words) and bits_equal(got.density_rate, rate)):
        return False
    for mine, theirs in ((got.divergence, divergence), (got.curl, curl), (got.normal, normal)):
        if (mine is None) != (theirs is None):
            return False
        if mine is not None and not (np.shape(mine) == theirs.shape and bits_equal(np.ravel(mine), np.ravel(theirs))):
            return False
    return True


def velocities(seed, n, special=None):
    """A seeded float64 velocity column around a shear flow; ``special``: row -> vector."""
    rng = np.random.default_rng(1000 + seed)
    w = rng.standard_normal((n, 3)) * np.array([1.0, 0.5, 0.25]) + np.array([0.3, -0.2, 0.1])
    for row, value in (special or {}).items():
        w[row] = value
    return w


def _case(k, name):
    p, mass, density, kw = SUM_CASES[name]
    kw = dict((key, value) for key, value in kw.items() if key != 'surface_below')
    # mass_density: beside its density 0 (row 17) and NaN density (row 123) one infinite velocity component
    special = {200: [np.inf, 0.5, -0.5]} if name == 'mass_density' else None
    return p, velocities(k, len(p), special), mass, density, kw


# name -> (positions, velocities as float64, mass or None, density or None, keyword arguments of sph_kernel_gradients)
CASES = dict((name, _case(k, name)) for k, name in enumerate(sorted(SUM_CASES)))
# (a velocity that is stored nowhere: the zero vector)
CASES['no_velocity'] = CASES['mass_only'][:1] + (None,) + CASES['density_only'][2:]


def _cloud(seed, n=60, dtype=np.float64):
    from neighbours_cases import random_rows
    return random_rows(seed, n, CUBE, dtype)


def _flow(seed, n=60, dtype=np.float64):
    return velocities(seed, n).astype(dtype)


def _fluid(seed, n=60):
    rng = np.random.default_rng(2000 + seed)
    return dict(mass=rng.uniform(0.5, 2.0, size=n), density=1000.0 + 50.0 * rng.standard_normal(n))


def _small(seed, n=60, cells=(2, 2, 2), **more):
    return dict(dict(position=_cloud(seed, n), velocity=_flow(seed, n), box=CUBE, h=1.0, cells=cells, **_fluid(seed, n)), **more)


# name -> (the loop's switch, the case: keyword arguments of sph_kernel_gradients).  Each case is a small one on which the
# mutated loop differs from the definition; the unmutated loop agrees with the model on every one of them.
MUTATIONS = {
    'd taken as x_i - x_j': (dict(reversed_d=True), _small(41)),
    'e from the raw difference without the minimum image': (
        # (entries in the x columns 0 and 3 of four: every sum crosses the periodic wrap)
        dict(raw_e=True), dict(position=SUM_CASES['four_cells_wrap'][0][:160], velocity=_flow(42, 160), box=CUBE, h=1.0,
                               cells=(4, 4, 4), **_fluid(42, 160))),
    'G multiplied inside the sum': (dict(g_inside=True), _small(43)),
    'a fused dot': (dict(fused_dot=True), _small(44)),
    'dot associated as u0*e0 + (u1*e1 + u2*e2)': (dict(dot_right=True), _small(45)),
    'u x e instead of e x u': (dict(u_cross_e=True), _small(46)),
    '(V_j*e) . u instead of V_j * (e . u)': (dict(ve_dot_u=True), _small(47)),
    'the velocity difference taken in float32 before conversion': (
        dict(u_f32=True), dict(_small(48), velocity=_flow(48, 60, np.float32))),
    "the spline's outer F as (-0.75*(u*u)) * (1/q)": (dict(reciprocal=True), _small(49, kernel='cubic_spline')),
    # (only inf * 0 shows it, as in the sums: at exactly 2h F is -0.0, so the term is a zero unless V_j is infinite)
    '<= for <': (dict(strict=False),
                 dict(position=np.array([[0, 0, 0], [0.5, 0, 0]], np.float32), velocity=np.array([[0, 0, 0], [1, 2, 3]], np.float32),
                      box=CUBE, h=0.25, density=np.array([1, 0], np.float32))),
    # (one row with an infinite velocity: its own term is (inf - inf) * 0, a NaN)
    'self excluded': (dict(skip_self=True), dict(position=np.array([[1, 2, 3]], np.float32),
                                                 velocity=np.array([[np.inf, 0, 0]], np.float32), box=CUBE, h=0.5)),
    'j descending inside a cell': (dict(descending_j=True), _small(50, 40, cells=(1, 1, 1))),
    'cells in ascending wrapped index': (dict(ascending_cells=True), _small(51, 120, cells=(3, 3, 3))),
}
# Mutations no input can show.  The Wendland factor with fused multiply-adds: t = fma(-0.5, q, 1.0) rounds once where 1.0 -
# 0.5*q rounds twice, but 0.5*q is exact (a power of two), so both give the same double for every q; the products (t*t)*t
# and -5.0 * (...) have no addition to fuse with.  The contraction that does matter is the dot's (`MUTATIONS`).
EQUIVALENT = {
    'the Wendland factor with a fused multiply-add': (dict(fused_factor=True), _small(52)),
}
