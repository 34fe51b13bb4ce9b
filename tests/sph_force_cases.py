"""What the SPH acceleration tests share: a plain double loop of the definition of `pgsd.hoomd.sph_accelerations` in Python
floats -- with switches that each stand for a kernel mistake --, the mutation table with the smallest case on which each
mutation differs, and the constructed cases: the geometry of `sph_cases.CASES` with the seeded velocity columns of
`sph_gradient_cases` and seeded pressure columns.  `test_sph_force_model.py` holds the model against the loop;
`test_gpu_sph_forces.py` runs the kernel on the same cases."""
import math

import numpy as np

import pgsd.hoomd as hoomd
from sph_cases import CASES as SUM_CASES, CUBE, KERNELS, NONE, _columns, bits_equal  # noqa: F401
from sph_gradient_cases import LOOP_ENTRIES, displacement, factor, velocities  # noqa: F401

# the two ways every case is asked: the pressure term alone without gravity, and everything
TERMS = {'plain': dict(viscosity=None, gravity=None), 'viscous': dict(viscosity=0.7, gravity=(0.25, -9.81, 0.5))}


def _div(a, b):
    """a / b as IEEE gives it (Python raises on a zero divisor)."""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        return float(np.float64(a) / np.float64(b))


def loop_accelerations(position, velocity, box, h, mass=None, density=None, pressure=None, viscosity=None, gravity=None,
                       rows=None, cells=None, dimensions=3, kernel='wendland_c2', extras=None, pair_division=False,
                       divided_twice=False, ms_first=False, g_inside=False, reversed_d=False, raw_e=False, k_right=False,
                       no_eta=False, rho_inside=False, u_f32=False, strict=True, skip_self=False, descending_j=False,
                       ascending_cells=False, gravity_first=False):
    """The accelerations by a double loop over ordered pairs of list entries in plain Python floats: ``(words,
    pressure_acc, viscous_acc, total)`` in the layout of `pgsd.hoomd.KernelAccelerations` (``viscous_acc`` None without a
    viscosity).  Every keyword from ``pair_division`` on is a mutation.  ``extras``: a dict that receives ``budget``, per
    axis the sum over all pairs of ``|m_i m_j G S e_k|``, and ``longest``, the longest candidate run of one entry."""
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
    eta2 = (0.01 * hh) * hh
    Gv = None if viscosity is None else G * (2.0 * float(viscosity))
    g = [0.0, 0.0, 0.0] if gravity is None else [float(c) for c in gravity]

    def column(values, default):
        return [default if values is None else float(np.float64(np.asarray(values).reshape(-1)[k])) for k in rows_sorted]

    x = [[float(np.float64(c)) for c in p[k]] for k in rows_sorted]
    raw_w = np.zeros((len(p), 3)) if velocity is None else np.asarray(velocity).reshape(-1, 3)
    w = [[float(np.float64(c)) for c in raw_w[k]] for k in rows_sorted]
    m, rho, pr = column(mass, 1.0), column(density, 0.0), column(pressure, 0.0)
    if divided_twice:
        A = [_div(_div(a, b), b) for a, b in zip(pr, rho)]
    else:
        A = [_div(a, b * b) for a, b in zip(pr, rho)]
    V = [_div(a, b) for a, b in zip(m, rho)]
    ids = [int(c) for c in cell_sorted]
    members = {}
    for k, c in enumerate(ids):
        members.setdefault(c, []).append(k)
    pressure_acc, total = [[0.0] * 3 for _ in range(n)], [[0.0] * 3 for _ in range(n)]
    viscous_acc = None if Gv is None else [[0.0] * 3 for _ in range(n)]
    offsets = [hoomd._axis_offsets(c) for c in grid]
    scale = G if g_inside else 1.0
    budget, longest = [0.0] * 3, 0
    for i in range(n):
        if ids[i] >= n_cells:
            continue
        at = (ids[i] % grid[0], (ids[i] // grid[0]) % grid[1], ids[i] // (grid[0] * grid[1]))
        a_p, a_v, run = [0.0] * 3, [0.0] * 3, 0
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
                        run += 1
                        if raw_e:
                            d = displacement(x[i], x[j], v, dimensions, minimum_image=False)
                        q = math.sqrt(d2) * inv_h
                        F = factor(q, kernel)
                        e = [(F * scale) * d[0], (F * scale) * d[1], (F * scale) * d[2]]
                        if pair_division:
                            S = _div(pr[i], rho[i] * rho[i]) + _div(pr[j], rho[j] * rho[j])
                        else:
                            S = A[i] + A[j]
                        for k in range(3):
                            term = (m[j] * S) * e[k] if ms_first else m[j] * (S * e[k])
                            a_p[k] = a_p[k] + term
                            if extras is not None and term == term:
                                budget[k] += abs((m[i] * G) * term)
                        if Gv is None:
                            continue
                        if no_eta:
                            K = _div(F * d2, d2)
                        elif k_right:
                            K = F * _div(d2, d2 + eta2)
                        else:
                            K = _div(F * d2, d2 + eta2)
                        if u_f32:
                            u = [float(np.float32(raw_w[rows_sorted[j]][k]) - np.float32(raw_w[rows_sorted[i]][k])) for k in range(3)]
                        else:
                            u = [w[j][k] - w[i][k] for k in range(3)]
                        for k in range(3):
                            term = V[j] * (K * u[k])
                            a_v[k] = a_v[k] + (_div(term, rho[i]) if rho_inside else term)
        longest = max(longest, run)
        last = 1.0 if g_inside else G
        for k in range(3):
            pressure_acc[i][k] = -(last * a_p[k])
            if Gv is None:
                total[i][k] = pressure_acc[i][k] + g[k]
                continue
            viscous_acc[i][k] = Gv * a_v[k] if rho_inside else _div(Gv * a_v[k], rho[i])
            if gravity_first:
                total[i][k] = (pressure_acc[i][k] + g[k]) + viscous_acc[i][k]
            else:
                total[i][k] = (pressure_acc[i][k] + viscous_acc[i][k]) + g[k]
    if extras is not None:
        extras['budget'], extras['longest'] = budget, longest
    with_cell = [k for k in range(n) if ids[k] < n_cells]
    words = np.zeros(12, dtype=np.uint64)
    f = words[9:12].view(np.float64)
    words[0], words[1], words[3:9] = n, n - len(with_cell), NONE
    words[2] = sum(1 for k in with_cell if not all(math.isfinite(c) for c in total[k]))
    for s, values in enumerate((total, pressure_acc, viscous_acc)):
        if values is None:
            continue
        best = -1.0
        for k in with_cell:
            c = values[k]
            norm2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
            if norm2 == norm2 and norm2 > best:
                best = f[s] = norm2
                words[3 + 2 * s], words[4 + 2 * s] = k, int(rows_sorted[k])
    as_array = lambda a: None if a is None else np.array(a, dtype=np.float64).reshape(n, 3)  # noqa: E731
    return words, as_array(pressure_acc), as_array(viscous_acc), as_array(total)


def words_equal(a, b):
    """Two summaries: the nine integer words exactly, the three float words as `bits_equal`."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return np.array_equal(a[:9], b[:9]) and bits_equal(a[9:].view(np.float64), b[9:].view(np.float64))


def same(got, want):
    """Is the model's (or the kernel's, copied to the host) `KernelAccelerations` the loop's result, bit for bit?"""
    words, pressure_acc, viscous_acc, total = want
    if not words_equal(got.summary, words):
        return False
    for mine, theirs in ((got.pressure_acc, pressure_acc), (got.viscous_acc, viscous_acc), (got.total, total)):
        if (mine is None) != (theirs is None):
            return False
        if mine is not None and not (np.shape(mine) == theirs.shape and bits_equal(np.ravel(mine), np.ravel(theirs))):
            return False
    return True


def pressures(seed, n, special=None):
    """A seeded float64 pressure column around 1e5; ``special``: row -> value."""
    p = 1.0e5 + 1.0e4 * np.random.default_rng(3000 + seed).standard_normal(n)
    for row, value in (special or {}).items():
        p[row] = value
    return p


def _case(k, name):
    p, mass, density, kw = SUM_CASES[name]
    kw = dict((key, value) for key, value in kw.items() if key != 'surface_below')
    # mass_density: beside its density 0 (row 17) and NaN density (row 123) one infinite pressure
    special = {300: np.inf} if name == 'mass_density' else None
    return p, velocities(k, len(p)), mass, density, pressures(k, len(p), special), kw


# name -> (positions, velocities, mass or None, density or None, pressure or None, keyword arguments of sph_accelerations).
# A density that is stored nowhere is the schema's 0.0: every A and V of one_cell_65 and mass_only is infinite or NaN.
CASES = dict((name, _case(k, name)) for k, name in enumerate(sorted(SUM_CASES)))
# (each chunk absent alone, over one geometry)
_BASE = (SUM_CASES['mass_only'][0], velocities(20, 200)) + _columns(20, 200) + (pressures(20, 200), dict(box=CUBE, h=0.75))
CASES['no_velocity'] = _BASE[:1] + (None,) + _BASE[2:]
CASES['no_mass'] = _BASE[:2] + (None,) + _BASE[3:]
CASES['no_density'] = _BASE[:3] + (None,) + _BASE[4:]
CASES['no_pressure'] = _BASE[:4] + (None,) + _BASE[5:]


def _cloud(seed, n=60, dtype=np.float64):
    from neighbours_cases import random_rows
    return random_rows(seed, n, CUBE, dtype)


def _fluid(seed, n=60):
    rng = np.random.default_rng(2000 + seed)
    return dict(mass=rng.uniform(0.5, 2.0, size=n), density=1000.0 + 50.0 * rng.standard_normal(n), pressure=pressures(seed, n))


def _small(seed, n=60, cells=(2, 2, 2), **more):
    return dict(dict(position=_cloud(seed, n), velocity=velocities(seed, n), box=CUBE, h=1.0, cells=cells,
                     viscosity=0.7, gravity=(0.25, -9.81, 0.5), **_fluid(seed, n)), **more)


_PAIR_AT_2H = dict(position=np.array([[0, 0, 0], [0.5, 0, 0]], np.float32), velocity=np.array([[0, 0, 0], [1, 2, 3]], np.float32),
                   box=CUBE, h=0.25, density=np.array([1, 0], np.float32), pressure=np.array([1, 1], np.float32))
_ALONE = dict(position=np.array([[1, 2, 3]], np.float32), velocity=np.array([[1, 0, 0]], np.float32), box=CUBE, h=0.5,
              density=np.array([0], np.float32), pressure=np.array([1], np.float32))
# name -> (the loop's switch, the case: keyword arguments of sph_accelerations).  Each case is a small one on which the
# mutated loop differs from the definition; the unmutated loop agrees with the model on every one of them.
MUTATIONS = {
    'A formed as (p / rho) / rho': (dict(divided_twice=True), _small(61)),
    '(m_j * S) * e_k': (dict(ms_first=True), _small(62)),
    'G multiplied inside the sum': (dict(g_inside=True), _small(63)),
    'd taken as x_i - x_j': (dict(reversed_d=True), _small(64)),
    'e from the raw difference without the minimum image': (
        # (entries in the x columns 0 and 3 of four: every sum crosses the periodic wrap)
        dict(raw_e=True), dict(position=SUM_CASES['four_cells_wrap'][0][:160], velocity=velocities(65, 160), box=CUBE, h=1.0,
                               cells=(4, 4, 4), **_fluid(65, 160))),
    'K = F * (d2 / (d2 + eta2))': (dict(k_right=True), _small(66)),
    # (the self pair: (F * 0) / 0 is a NaN, (F * 0) / eta2 a zero)
    'eta2 omitted': (dict(no_eta=True), _small(67, 5, cells=(1, 1, 1))),
    'the division by rho_i inside the sum': (dict(rho_inside=True), _small(68)),
    'the velocity difference taken in float32 before conversion': (
        dict(u_f32=True), dict(_small(69), velocity=velocities(69, 60).astype(np.float32))),
    # (at exactly 2h F is -0.0 and so is e: only S = inf shows the pair, as inf * 0; row 1 has density 0)
    '<= for <': (dict(strict=False), _PAIR_AT_2H),
    # (one row with density 0: A_i is infinite and its own term inf * 0, a NaN)
    'self excluded': (dict(skip_self=True), _ALONE),
    'j descending inside a cell': (dict(descending_j=True), _small(70, 40, cells=(1, 1, 1))),
    'cells in ascending wrapped index': (dict(ascending_cells=True), _small(71, 120, cells=(3, 3, 3))),
    'gravity added before the viscous term': (dict(gravity_first=True), _small(72)),
}
# Mutations no input can show.  S formed per pair as p_i / (rho_i*rho_i) + p_j / (rho_j*rho_j): the division of the same
# two doubles rounds to the same double whenever it is done, so dividing once per entry (the stored A) or once per pair
# gives the same S for every input -- it costs two divisions per candidate and changes no bit.  What does change bits is
# another formula for A (`MUTATIONS`: divided twice).
EQUIVALENT = {
    'S with per-pair divisions instead of the stored A': (dict(pair_division=True), _small(73)),
}
