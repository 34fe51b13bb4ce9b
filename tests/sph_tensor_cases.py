"""What the SPH gradient-tensor tests share: a plain double loop of the definition of `pgsd.hoomd.sph_gradient_tensors` in
Python floats -- with switches that each stand for a kernel mistake --, the mutation table with the case on which each
mutation differs, the singular cases and the constructed cases: those of `sph_gradient_cases.CASES` with a `det_min`.
`test_sph_tensor_model.py` holds the model against the loop; `test_gpu_sph_tensors.py` runs the kernel on the same
cases."""
import math

import numpy as np

import pgsd.hoomd as hoomd
from sph_cases import CUBE, KERNELS, NONE, bits_equal, fma  # noqa: F401
from sph_gradient_cases import CASES as GRADIENT_CASES, LOOP_ENTRIES, displacement, factor, velocities  # noqa: F401

UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def loop_tensors(position, velocity, box, h, mass=None, density=None, rows=None, cells=None, dimensions=3,
                 kernel='wendland_c2', det_min=0.25, b_transposed=False, g_transposed=False, l_times_r=False, g_inside=False,
                 fused_det=False, det_right=False, c01_sign=False, det_min_ge=False, identity_computed=False,
                 flat_through_3d=False, raw_shear=False, skip_self=False, descending_j=False, u_f32=False):
    """The tensors by a double loop over ordered pairs of list entries in plain Python floats: ``(words, correction,
    determinant, velocity_gradient, shear_rate)`` in the layout of `pgsd.hoomd.KernelTensors`.  Every keyword from
    ``b_transposed`` on is a mutation."""
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
    rho = [0.0 if density is None else float(np.float64(np.asarray(density).reshape(-1)[k])) for k in rows_sorted]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        vol = [float(np.float64(a) / np.float64(b)) for a, b in zip(m, rho)]
    ids = [int(c) for c in cell_sorted]
    members = {}
    for k, c in enumerate(ids):
        members.setdefault(c, []).append(k)
    offsets = [hoomd._axis_offsets(c) for c in grid]
    scale = G if g_inside else 1.0
    three = dimensions == 3 or flat_through_3d
    correction, determinant = [[0.0] * 6 for _ in range(n)], [0.0] * n
    gradient, trace, shear, good = [[0.0] * 9 for _ in range(n)], [0.0] * n, [0.0] * n, [False] * n
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i in range(n):
            if ids[i] >= n_cells:
                continue
            at = (ids[i] % grid[0], (ids[i] // grid[0]) % grid[1], ids[i] // (grid[0] * grid[1]))
            b, g = [np.float64(0.0)] * 6, [np.float64(0.0)] * 9
            for oz in offsets[2]:
                for oy in offsets[1]:
                    for ox in offsets[0]:
                        wx, wy, wz = (at[0] + ox) % grid[0], (at[1] + oy) % grid[1], (at[2] + oz) % grid[2]
                        inside = members.get(wx + grid[0] * (wy + grid[1] * wz), ())
                        for j in (reversed(inside) if descending_j else inside):
                            if j == i and skip_self:
                                continue
                            d = displacement(x[i], x[j], v, dimensions)
                            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                            if not d2 < r2:
                                continue
                            q = math.sqrt(d2) * inv_h
                            F = np.float64(factor(q, kernel) * scale)
                            d = [np.float64(c) for c in d]
                            e = [F * d[0], F * d[1], F * d[2]]
                            if u_f32:
                                u = [np.float64(np.float32(raw_w[rows_sorted[j]][k]) - np.float32(raw_w[rows_sorted[i]][k]))
                                     for k in range(3)]
                            else:
                                u = [np.float64(w[j][k]) - np.float64(w[i][k]) for k in range(3)]
                            V = np.float64(vol[j])
                            for k, (r, c) in enumerate(UPPER):
                                b[k] = b[k] + V * ((e[r] * d[c]) if b_transposed else (d[r] * e[c]))
                            for r in range(3):
                                for c in range(3):
                                    g[3 * r + c] = g[3 * r + c] + V * ((u[c] * e[r]) if g_transposed else (u[r] * e[c]))
            last = np.float64(1.0 if g_inside else G)
            B00, B01, B02, B11, B12, B22 = (last * a for a in b)
            R = [last * a for a in g]
            zero = np.float64(0.0)
            if three:
                c00 = B11 * B22 - B12 * B12
                c01 = (B01 * B22 - B02 * B12) if c01_sign else (B02 * B12 - B01 * B22)
                c02 = B01 * B12 - B02 * B11
                c11 = B00 * B22 - B02 * B02
                c12 = B01 * B02 - B00 * B12
                c22 = B00 * B11 - B01 * B01
                if fused_det:
                    det = np.float64(fma(float(B02), float(c02), fma(float(B01), float(c01), float(B00 * c00))))
                elif det_right:
                    det = B00 * c00 + (B01 * c01 + B02 * c02)
                else:
                    det = (B00 * c00 + B01 * c01) + B02 * c02
            else:
                det = B00 * B11 - B01 * B01
                c00, c01, c11 = B11, (B01 if c01_sign else -B01), B00
                c02 = c12 = c22 = zero
            ok = bool((det >= det_min if det_min_ge else det > det_min) and det < math.inf)
            one = np.float64(1.0)
            if ok:
                L = [c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det]
                if not three:
                    L[2] = L[4] = L[5] = zero
            else:
                L = [one, zero, zero, one, zero, one if three else zero]
            Lm = ((L[0], L[1], L[2]), (L[1], L[3], L[4]), (L[2], L[4], L[5]))
            if ok or identity_computed:
                D = []
                for r in range(3):
                    for c in range(3):
                        if l_times_r:
                            D.append((Lm[r][0] * R[c] + Lm[r][1] * R[3 + c]) + Lm[r][2] * R[6 + c])
                        elif three:
                            D.append((R[3 * r] * Lm[0][c] + R[3 * r + 1] * Lm[1][c]) + R[3 * r + 2] * Lm[2][c])
                        elif c < 2:
                            D.append(R[3 * r] * Lm[0][c] + R[3 * r + 1] * Lm[1][c])
                        else:
                            D.append(zero)
            else:
                D = list(R)
            tr = (D[0] + D[4]) + D[8]
            if raw_shear:
                s01, s02, s12 = D[1], D[2], D[5]
            else:
                s01, s02, s12 = 0.5 * (D[1] + D[3]), 0.5 * (D[2] + D[6]), 0.5 * (D[5] + D[7])
            ss = ((D[0] * D[0] + D[4] * D[4]) + D[8] * D[8]) + 2.0 * ((s01 * s01 + s02 * s02) + s12 * s12)
            correction[i], determinant[i], gradient[i] = [float(a) for a in L], float(det), [float(a) for a in D]
            trace[i], shear[i], good[i] = float(tr), float(np.sqrt(2.0 * ss)), ok
    with_cell = [k for k in range(n) if ids[k] < n_cells]
    words = np.zeros(14, dtype=np.uint64)
    f = words[8:13].view(np.float64)
    words[0], words[1], words[4:8] = n, n - len(with_cell), NONE
    f[0:4:2], f[1:4:2] = math.inf, -math.inf
    below = lambda a, b: a < b or (a == b and math.copysign(1.0, a) < math.copysign(1.0, b))  # noqa: E731  (-0.0 < +0.0)
    for s, values in enumerate((determinant, trace)):
        for k in with_cell:
            if below(values[k], f[2 * s]):
                f[2 * s] = values[k]
            if below(f[2 * s + 1], values[k]):
                f[2 * s + 1] = values[k]
    words[2] = sum(1 for k in with_cell if not math.isfinite(shear[k]))
    words[3] = sum(1 for k in with_cell if not good[k])
    smallest, largest = math.inf, -math.inf
    for k in with_cell:
        if determinant[k] < smallest:
            smallest = determinant[k]
            words[4], words[5] = k, int(rows_sorted[k])
        if shear[k] > largest:
            largest = f[4] = shear[k]
            words[6], words[7] = k, int(rows_sorted[k])
    return (words, np.array(correction, dtype=np.float64).reshape(n, 6), np.array(determinant, dtype=np.float64),
            np.array(gradient, dtype=np.float64).reshape(n, 9), np.array(shear, dtype=np.float64))


def words_equal(a, b):
    """Two summaries: the eight integer words and the last one exactly, the five float words as `bits_equal`."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return (a.shape == b.shape == (14,) and np.array_equal(a[:8], b[:8]) and a[13] == b[13] == 0
            and bits_equal(a[8:13].view(np.float64), b[8:13].view(np.float64)))


def same(got, want):
    """Is the model's (or the kernel's, copied to the host) `KernelTensors` the loop's result, bit for bit?"""
    words, correction, determinant, gradient, shear = want
    if not words_equal(got.summary, words):
        return False
    for mine, theirs in ((got.correction, correction), (got.determinant, determinant), (got.velocity_gradient, gradient),
                         (got.shear_rate, shear)):
        if not (np.shape(mine) == theirs.shape and bits_equal(np.ravel(mine), np.ravel(theirs))):
            return False
    return True


# name -> (positions, velocities as float64 or None, mass or None, density or None, keyword arguments of
# sph_gradient_tensors).  The gradient tests' cases; their densities lie around 1000, so every determinant is tiny:
# det_min = 0 corrects the entries whose determinant is positive and leaves the others uncorrected, both ways in one case
CASES = dict((name, case[:4] + (dict(case[4], det_min=0.0),)) for name, case in GRADIENT_CASES.items())


def fluid(seed, n=120, dimensions=3, dtype=np.float64):
    """A cloud whose volumes fill the box -- the determinants lie around 1 --: ``n`` seeded rows of the cube (2-D: of its
    z = 0 plane), seeded velocities, masses in [0.5, 2) and densities that make the mean volume the box's share."""
    from neighbours_cases import random_rows
    rng = np.random.default_rng(3000 + seed)
    p = random_rows(seed, n, CUBE, np.float64, dimensions)
    mass = rng.uniform(0.5, 2.0, size=n)
    share = (512.0 if dimensions == 3 else 64.0) / n
    density = mass / (share * rng.uniform(0.8, 1.2, size=n))
    return dict(position=p.astype(dtype), velocity=velocities(seed, n).astype(dtype), box=CUBE, h=1.25, cells=(3, 3, 3 if
                dimensions == 3 else 1), mass=mass, density=density, dimensions=dimensions, det_min=1e-3)


def _det_min_cases():
    """`det_min` set to the model's own determinant of one corrected entry leaves that entry uncorrected; `nextafter`
    below it corrects it."""
    case = dict(fluid(68), kernel='wendland_c2')
    got = hoomd.sph_gradient_tensors(**case)
    at = int(np.argmax(got.determinant))
    det = float(got.determinant[at])
    assert det > 1e-3
    return at, dict(case, det_min=det), dict(case, det_min=float(np.nextafter(det, 0.0)))


DET_AT, DET_MIN_AT, DET_MIN_BELOW = _det_min_cases()

# Two rows on the x axis, 0.5 apart, one of them moving at 1e300 along x, volumes of 1e10: g00 overflows, so R00 is
# infinite while R01 is a zero; the two are collinear, so the determinant is 0 and the entry stays uncorrected.  Written,
# D01 is that zero; computed as R00*L01 + ..., it is inf * 0.
INFINITE_R = dict(position=np.array([[1, 2, 3], [1.5, 2, 3]], np.float64), velocity=np.array([[0, 0, 0], [1e300, 0, 0]], np.float64),
                  box=CUBE, h=0.5, mass=np.full(2, 1e10), density=np.ones(2))
# (one row with an infinite velocity: its own term is (inf - inf) * 0, a NaN, and so is every R_0b)
ISOLATED_INFINITE = dict(position=np.array([[1, 2, 3]], np.float32), velocity=np.array([[np.inf, 0, 0]], np.float32), box=CUBE,
                         h=0.5, density=np.ones(1, np.float32))

# name -> (the loop's switch, the case: keyword arguments of sph_gradient_tensors).  Each case is a small one on which the
# mutated loop differs from the definition; the unmutated loop agrees with the model on every one of them.
MUTATIONS = {
    '01 b from e_a*d_b': (dict(b_transposed=True), fluid(61)),
    '02 g transposed (u_b*e_a)': (dict(g_transposed=True), fluid(62)),
    '03 L.R instead of R.L': (dict(l_times_r=True), fluid(63)),
    '04 G multiplied inside the sum': (dict(g_inside=True), fluid(64)),
    '05 a fused det': (dict(fused_det=True), fluid(65)),
    '06 det associated as B00*c00 + (B01*c01 + B02*c02)': (dict(det_right=True), fluid(66)),
    '07 a cofactor with the wrong sign (c01)': (dict(c01_sign=True), fluid(67)),
    '08 >= for > at det_min': (dict(det_min_ge=True), DET_MIN_AT),
    '09 the identity fall-back computed instead of written': (dict(identity_computed=True), INFINITE_R),
    '10 2-D run through the 3-D inverse': (dict(flat_through_3d=True), fluid(70, dimensions=2)),
    '11 shear_rate from the unsymmetrised off-diagonals': (dict(raw_shear=True), fluid(71)),
    '12 self excluded': (dict(skip_self=True), ISOLATED_INFINITE),
    '13 j descending inside a cell': (dict(descending_j=True), dict(fluid(73), cells=(1, 1, 1))),
    '14 the velocity difference taken in float32': (dict(u_f32=True), dict(fluid(74), velocity=velocities(74, 120).astype(np.float32))),
}

# The singular inputs: every entry stays uncorrected, with the identity and D == R bit for bit.
SINGULAR = {
    'an isolated entry': dict(position=np.array([[1, 2, 3], [-3, -3, -3]], np.float64), velocity=np.array([[1, 2, 3], [0, 1, 0]],
                              np.float64), box=CUBE, h=0.5, density=np.ones(2), det_min=0.0),
    # (every d_z is 0, exactly: det is +-0.0 whatever det_min)
    'a coplanar sheet in 3-D': dict(dict(fluid(81, dimensions=2), dimensions=3, cells=(3, 3, 3)), det_min=0.0),
    # (every d_y is 0)
    'a collinear row in 2-D': dict(position=np.stack([np.linspace(-3.5, 3.5, 40), np.full(40, 0.5), np.zeros(40)], axis=1),
                                   velocity=velocities(82, 40), box=CUBE, h=1.0, mass=np.ones(40), density=np.full(40, 5.0),
                                   dimensions=2, cells=(4, 4, 1), det_min=0.0),
}


# ---------------------------------------------------------------- the physical checks' inputs
def jittered_cloud(dimensions=3):
    """The exactness cloud: an 8^3 lattice of spacing 1 (2-D: 12^2), each coordinate jittered by a seeded uniform +-0.3, in
    a box of edge 24, h = 1.5, masses in [0.5, 2), densities in [0.8, 1.2): ``(position, mass, density, box)``."""
    rng = np.random.default_rng(512)
    if dimensions == 3:
        g = np.arange(8) - 3.5
        p = np.array([(x, y, z) for z in g for y in g for x in g], np.float64)
        p = p + rng.uniform(-0.3, 0.3, size=p.shape)
    else:
        g = np.arange(12) - 5.5
        p = np.array([(x, y, 0.0) for y in g for x in g], np.float64)
        p[:, :2] = p[:, :2] + rng.uniform(-0.3, 0.3, size=(len(p), 2))
    return p, rng.uniform(0.5, 2.0, size=len(p)), rng.uniform(0.8, 1.2, size=len(p)), [24, 24, 24 if dimensions == 3 else 1, 0, 0, 0]


def seeded_matrix():
    return np.random.default_rng(33).uniform(-1.0, 1.0, size=(3, 3))
