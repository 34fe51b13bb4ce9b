"""The numpy model of the SPH kernel gradients (pgsd.hoomd.sph_kernel_gradients / frame_kernel_gradients), the definition
the GPU pass equals exactly (tests/test_gpu_sph_gradients.py): it equals a plain double loop bit for bit -- so its
numpy.add.at is the sequential sum --, every mutation of the loop differs from it on the case that names it, a linear
velocity field on a lattice gives back its divergence and curl, the colour gradient points into the fluid, and the command
line prints it.  No GPU."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

from neighbours_cases import FLAT, ORTHO, TRICLINIC, random_rows
from sph_cases import CASES as SUM_CASES, CUBE, KERNELS, NONE, bits_equal
from sph_gradient_cases import CASES, EQUIVALENT, LOOP_ENTRIES, MUTATIONS, loop_gradients, same, velocities


# ---------------------------------------------------------------- the model is the loop
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_equals_the_double_loop_bit_for_bit(name, kernel):
    p, w, mass, density, kw = CASES[name]
    n = len(p)
    # (the loop is quadratic in a crowded cell: beyond LOOP_ENTRIES entries it takes a strided sub-list of the case)
    rows = None if n <= LOOP_ENTRIES else np.arange(0, n, -(-n // LOOP_ENTRIES))
    for dtype in (np.float64, np.float32):
        args = dict(kw, position=p.astype(dtype), velocity=None if w is None else w.astype(dtype), mass=mass, density=density,
                    rows=rows, kernel=kernel)
        got = hoomd.sph_kernel_gradients(**args)
        assert same(got, loop_gradients(**args)), (name, kernel, dtype)
    assert got.n == (n if rows is None else len(rows)) and got.G == hoomd.sph_gradient_scale(kernel, kw['h'], kw.get('dimensions', 3))
    assert (got.divergence is None) == (density is None) and got.volume == (density is not None)
    if density is not None:
        assert got.curl.shape == (got.n, 3) and got.normal.shape == (got.n, 3)
    if name == 'all_nowhere':
        assert got.nowhere == got.n and got.density_rate_min == np.inf and got.density_rate_max == -np.inf
        assert got.curl2 is None and got.normal_at is None
        for a in (got.density_rate, got.divergence, got.curl, got.normal):
            assert not a.any() and not np.signbit(a).any()
    if name == 'three_cells':
        lost = got.cell == 27
        assert lost.any() and not got.curl[lost].any() and not np.signbit(got.divergence[lost]).any()
    if name == 'no_velocity':
        # every u is zero: no rate, no divergence, no curl; the colour gradient needs no velocity
        assert not got.density_rate.any() and not got.divergence.any() and not got.curl.any() and got.normal.any()
    if name == 'flat':
        assert not got.normal[:, 2].any() and got.curl[:, 0].any()      # d_z is 0; a non-zero v_z still enters the curl
    if name == 'mass_density':
        assert got.not_finite > 0 and np.isnan(got.divergence).any()


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_list_in_any_order_with_repeats(kernel):
    p, w, mass, density, kw = CASES['three_cells']
    rows = np.concatenate([np.arange(300, 0, -1), [7, 7, 300, 12]])
    got = hoomd.sph_kernel_gradients(p, w, mass=mass, density=density, rows=rows, kernel=kernel, **kw)
    assert same(got, loop_gradients(p, w, mass=mass, density=density, rows=rows, kernel=kernel, **kw)) and got.n == 304


def test_pair_displacement_is_pair_distance2s_arithmetic():
    for box, dims in ((TRICLINIC, 3), (FLAT, 2)):
        a, b = random_rows(1, 500, box, np.float32, 3), random_rows(2, 500, box, np.float32, 3)
        vectors = hoomd.box_vectors(np.asarray(box, np.float32))
        dx, dy, dz = hoomd.pair_displacement(a, b, vectors, dims)
        assert dx.dtype == np.float64 and bits_equal((dx * dx + dy * dy) + dz * dz, hoomd.pair_distance2(a, b, vectors, dims))
        assert (dims == 3) == bool(dz.any())
        back = hoomd.pair_displacement(b, a, vectors, dims)
        assert np.allclose(back[0], -dx) and np.allclose(back[1], -dy)
    with pytest.raises(ValueError, match="dimensions must be 2 or 3"):
        hoomd.pair_displacement(a, b, vectors, 4)


def test_the_factor_is_the_derivative_of_the_weight():
    """F(q) = (1/q) dw/dq against a central difference of sph_weight, and its values by hand."""
    q = np.linspace(0.05, 1.95, 39)
    for kernel in KERNELS:
        slope = (hoomd.sph_weight(q + 1e-6, kernel) - hoomd.sph_weight(q - 1e-6, kernel)) / 2e-6
        assert np.allclose(hoomd.sph_gradient_factor(q, kernel) * q, slope, atol=1e-8)
        assert hoomd.sph_gradient_factor(2.0, kernel) == 0.0
    assert hoomd.sph_gradient_factor(0.0, 'wendland_c2') == -5.0 and hoomd.sph_gradient_factor(0.0, 'cubic_spline') == -3.0
    assert hoomd.sph_gradient_factor(1.0, 'cubic_spline') == -0.75 == 2.25 * 1.0 - 3.0      # both branches agree at q == 1
    assert hoomd.sph_gradient_scale('wendland_c2', 2.0) == -((hoomd.sph_sigma('wendland_c2', 2.0) * 0.5) * 0.5)


# ---------------------------------------------------------------- the mutations
@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_every_mutation_differs_on_its_case(mutation):
    switch, case = MUTATIONS[mutation]
    case = dict(case)
    kernels = [case.pop('kernel')] if 'kernel' in case else KERNELS
    for kernel in kernels:
        got = hoomd.sph_kernel_gradients(kernel=kernel, **case)
        assert same(got, loop_gradients(kernel=kernel, **case)), mutation
        assert not same(got, loop_gradients(kernel=kernel, **dict(case, **switch))), (mutation, kernel)


def test_the_mutation_no_input_can_show():
    """The Wendland factor's t = 1.0 - 0.5*q fused: 0.5*q is exact, so one rounding or two give the same double."""
    for mutation, (switch, case) in EQUIVALENT.items():
        got = hoomd.sph_kernel_gradients(**case)
        assert same(got, loop_gradients(**case)) and same(got, loop_gradients(**dict(case, **switch))), mutation


# ---------------------------------------------------------------- the physics
A = np.array([[0.30, -0.20, 0.10], [0.50, -0.10, 0.25], [-0.40, 0.15, 0.20]])
# sum_j V_j d_a (grad W)_b on the unit lattice at h = 1.5, computed on the CPU: the kernels' own lattice error
LATTICE = {('wendland_c2', 3): 1.0006, ('cubic_spline', 3): 1.0101, ('wendland_c2', 2): 0.9974, ('cubic_spline', 2): 1.0067}
BOUND = 0.02


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_linear_velocity_field_on_a_lattice(kernel):
    """A 12^3 lattice of spacing 1 inside a cubic box of edge 24 (no pair wraps), h = 1.5, mass and density 1, v = A x:
    for the entries at least 3 from every face the divergence is trace(A), the curl the axial vector of A - A^T and the
    density rate -trace(A), each within 2 % (the kernels' own lattice error is at most 1.01 %)."""
    g = np.arange(12) - 5.5
    p = np.array([(x, y, z) for z in g for y in g for x in g], np.float64)
    got = hoomd.sph_kernel_gradients(p, p @ A.T, [24, 24, 24, 0, 0, 0], 1.5, density=np.ones(len(p)), kernel=kernel)
    inner = np.all(np.abs(p[got.rows]) <= 2.5, axis=1)               # 3 or more from every face of the lattice
    assert inner.sum() == 6 ** 3 and got.n == 12 ** 3 and got.nowhere == 0 and got.not_finite == 0
    trace = np.trace(A)
    axial = np.array([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]])
    assert max(abs(v - 1) for v in LATTICE.values()) < BOUND
    assert np.all(np.abs(got.divergence[inner] - trace) <= BOUND * abs(trace))
    assert np.all(np.abs(got.density_rate[inner] + trace) <= BOUND * abs(trace))
    assert np.all(np.abs(got.curl[inner] - axial) <= BOUND * np.abs(axial))
    # (and the measured factor is the recorded one: a wrong constant fails, the lattice error does not)
    assert abs(got.divergence[inner].mean() / trace - LATTICE[kernel, 3]) < 2e-4
    # inside, the neighbourhood is symmetric: the colour gradient vanishes against its size at the faces
    assert np.abs(got.normal[inner]).max() < 1e-12 < 0.1 < got.normal2 ** 0.5


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_normal_points_inward_on_the_faces_of_a_flat_lattice(kernel):
    """The 12^2 lattice in a box of edge 24, 2-D: on the lattice's faces the colour gradient points into the lattice, and
    a linear field's divergence and z vorticity come back inside."""
    g = np.arange(12) - 5.5
    p = np.array([(x, y, 0.25) for y in g for x in g], np.float64)
    got = hoomd.sph_kernel_gradients(p, p @ A.T, [24, 24, 1, 0, 0, 0], 1.5, density=np.ones(len(p)), dimensions=2, kernel=kernel)
    x = p[got.rows]
    for axis in (0, 1):
        for side in (-1, 1):
            face = x[:, axis] == side * 5.5
            assert face.sum() == 12 and np.all(got.normal[face, axis] * side < 0)        # inward: against the face's side
    assert not got.normal[:, 2].any()
    inner = np.all(np.abs(x[:, :2]) <= 2.5, axis=1)
    trace2 = A[0, 0] + A[1, 1]
    assert np.all(np.abs(got.divergence[inner] - trace2) <= BOUND * abs(trace2))
    assert np.all(np.abs(got.curl[inner, 2] - (A[1, 0] - A[0, 1])) <= BOUND * abs(A[1, 0] - A[0, 1]))
    assert abs(got.divergence[inner].mean() / trace2 - LATTICE[kernel, 2]) < 2e-4
    assert np.abs(x[got.normal_at, :2]).max() == 5.5                                   # the largest normal lies on a face


# ---------------------------------------------------------------- the summary
def test_the_summary_rules():
    """A NaN never replaces a bound and never is a largest norm; the smaller position wins a tie; no density: no volume
    words."""
    p, w, mass, density, kw = CASES['mass_density']
    got = hoomd.sph_kernel_gradients(p, w, mass=mass, density=density, **kw)
    has = got.cell < np.prod(got.grid)
    rate, div = got.density_rate[has], got.divergence[has]
    assert np.isnan(rate).any() and got.not_finite == int((~np.isfinite(rate)).sum())
    assert got.density_rate_min == np.nanmin(rate) and got.density_rate_max == np.nanmax(rate)
    assert got.divergence_min == np.nanmin(div) and got.divergence_max == np.nanmax(div)
    for name, values in (('curl', got.curl), ('normal', got.normal)):
        v = values[has]
        norm2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        assert np.isnan(norm2).any()
        at = getattr(got, name + '_at')
        assert getattr(got, name + '2') == np.nanmax(norm2) == norm2[at] and getattr(got, name + '_row') == got.rows[at]
        assert at == int(np.flatnonzero(norm2 == np.nanmax(norm2))[0])
    # a tie: two pairs that are translates of one another give the same curl and normal: the smaller list position
    x = np.array([[-3, 0, 0], [-2.5, 0, 0], [3, 0, 0], [3.5, 0, 0]], np.float32)
    v = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0], [0, 1, 0]], np.float32)
    two = hoomd.sph_kernel_gradients(x, v, CUBE, 0.5, density=np.ones(4, np.float32))
    assert two.curl_at == 0 and two.normal_at == 0 and two.curl2 > 0 and bits_equal(two.curl[0], two.curl[2])
    assert two.curl_row == two.rows[0] and two.divergence_min == two.divergence_max == 0.0
    # without a density: the density rate alone
    none = hoomd.sph_kernel_gradients(p, w, mass=mass, **kw)
    assert none.divergence is None and none.curl is None and none.normal is None and not none.volume
    assert none.divergence_min is None and none.curl2 is None and none.curl_at is None and none.normal_row is None
    assert bits_equal(none.density_rate, got.density_rate) and none.density_rate_max == got.density_rate_max
    s = none.summary
    assert [int(v) for v in s[3:7]] == [NONE] * 4 and s[7:9].view(np.float64).tolist() == [np.inf, -np.inf]
    assert s[11:13].view(np.float64).tolist() == [0.0, 0.0]
    # nothing
    nothing = hoomd.sph_kernel_gradients(p, w, mass=mass, density=density, rows=np.arange(0), **kw)
    s = nothing.summary
    assert nothing.n == 0 and [int(v) for v in s[:7]] == [0, 0, 0] + [NONE] * 4 and nothing.curl2 is None
    assert s[7:].view(np.float64).tolist() == [np.inf, -np.inf, np.inf, -np.inf, 0.0, 0.0] and nothing.curl.shape == (0, 3)


# ---------------------------------------------------------------- frames, h=None, the command line
def small_frame(slength=None, density=True, velocity=True):
    fr = hoomd.Frame()
    fr.configuration.box = [8, 8, 8, 0, 0, 0]
    fr.particles.N = 6
    fr.particles.types = ['fluid', 'wall']
    fr.particles.typeid = np.array([0, 0, 1, 0, 0, 0], np.uint32)
    fr.particles.position = np.array([[1, 1, 1], [1.5, 1, 1], [1, 1.25, 1], [-3.9, 0, 0], [3.9, 0, 0], [np.nan, 0, 0]], np.float32)
    fr.particles.mass = np.array([1, 2, 1, 1, 1, 1], np.float32)
    if velocity:
        fr.particles.velocity = np.array([[0, 0, 0], [0, 1, 0], [-1, 0, 0.5], [1, 0, 0], [-1, 0, 0], [9, 9, 9]], np.float32)
    if density:
        fr.particles.density = np.array([1, 1, 1, 0.5, 0.5, 1], np.float32)
    if slength is not None:
        fr.particles.slength = np.asarray(slength, np.float32)
    return fr


def test_h_none_takes_a_uniform_slength_and_refuses_another():
    fr = small_frame(slength=[0.5] * 6)
    got = hoomd.frame_kernel_gradients(fr)
    want = hoomd.sph_kernel_gradients(fr.particles.position, fr.particles.velocity, fr.configuration.box, 0.5,
                                      mass=fr.particles.mass, density=fr.particles.density)
    assert got.h == 0.5 and np.array_equal(got.summary, want.summary) and bits_equal(got.curl.ravel(), want.curl.ravel())
    assert got.divergence_max > 0 and got.density_rate_min < 0 < got.curl2            # rows 3 and 4 part across the wrap
    assert hoomd.frame_kernel_gradients(small_frame()).h == 1.0                       # stored nowhere: the schema default
    assert hoomd.frame_kernel_gradients(small_frame(slength=[0.5] * 6), h=0.75).h == 0.75
    with pytest.raises(ValueError, match="slength ranges from 0.5 to 0.75"):
        hoomd.frame_kernel_gradients(small_frame(slength=[0.5, 0.5, 0.75, 0.5, 0.5, 0.5]))
    # the selection is the list: both i and j come from it
    fluid = hoomd.frame_kernel_gradients(fr, where={'type': ['fluid']})
    assert fluid.n == 5 and fluid.curl2 != got.curl2
    # a velocity that is stored nowhere is the zero vector
    still = hoomd.frame_kernel_gradients(small_frame(slength=[0.5] * 6, velocity=False))
    assert not still.density_rate.any() and not still.curl.any() and bits_equal(still.normal.ravel(), got.normal.ravel())
    arrays = dict(position=fr.particles.position, velocity=fr.particles.velocity, mass=fr.particles.mass)
    assert hoomd.frame_kernel_gradients(arrays, h=0.5, box=fr.configuration.box).divergence is None


def test_what_sph_kernel_gradients_refuses():
    p = random_rows(1, 10, ORTHO)
    w = velocities(1, 10).astype(np.float32)
    for h in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match="finite and positive"):
            hoomd.sph_kernel_gradients(p, w, ORTHO, h)
        with pytest.raises(ValueError, match="finite and positive"):
            hoomd.sph_gradient_scale('wendland_c2', h)
    with pytest.raises(ValueError, match="kernel is one of"):
        hoomd.sph_kernel_gradients(p, w, ORTHO, 0.5, kernel='gaussian')
    with pytest.raises(ValueError, match="kernel is one of"):
        hoomd.sph_gradient_factor(0.5, 'gaussian')
    with pytest.raises(ValueError, match="narrower"):
        hoomd.sph_kernel_gradients(p, w, ORTHO, 0.65, cells=(8, 6, 4))
    with pytest.raises(ValueError, match="narrower"):
        hoomd.sph_kernel_gradients(p, w, TRICLINIC, 0.65, cells=hoomd.cell_grid_for(ORTHO, 1.3))  # the tilt narrows x
    with pytest.raises(ValueError, match="2\\^20"):
        hoomd.sph_kernel_gradients(p, w, [1000, 800, 600, 0, 0, 0], 0.5, cells=(1000, 800, 600))
    with pytest.raises(ValueError, match="count twice"):
        hoomd.sph_kernel_gradients(p, w, ORTHO, 1.6)                                   # 2h = 3.2 > Lz / 2
    with pytest.raises(ValueError, match="cz == 1"):
        hoomd.sph_kernel_gradients(p, w, FLAT, 0.3, cells=(2, 2, 2), dimensions=2)
    with pytest.raises(ValueError, match="float32 or float64"):
        hoomd.sph_kernel_gradients(p.astype(np.int32), w, ORTHO, 0.5)
    with pytest.raises(ValueError, match="mass holds one float32 or float64 value per row"):
        hoomd.sph_kernel_gradients(p, w, ORTHO, 0.5, mass=np.ones(9))
    with pytest.raises(ValueError, match="density holds one float32 or float64 value per row"):
        hoomd.sph_kernel_gradients(p, w, ORTHO, 0.5, density=np.ones(10, np.int32))
    with pytest.raises(ValueError, match="velocity holds three float32 or float64 values per row"):
        hoomd.sph_kernel_gradients(p, w[:9], ORTHO, 0.5)
    with pytest.raises(ValueError, match="velocity holds three float32 or float64 values per row"):
        hoomd.sph_kernel_gradients(p, w.astype(np.int32), ORTHO, 0.5)
    with pytest.raises(ValueError, match="needs the box"):
        hoomd.frame_kernel_gradients(dict(position=p), h=0.5)
    assert set(SUM_CASES) < set(CASES)


def test_the_command_line_prints_the_gradients(tmp_path, capsys):
    path = str(tmp_path / "small.gsd")
    with hoomd.open(path, 'w') as t:
        t.append(small_frame(slength=[0.5] * 6))
    with hoomd.open(path, 'r') as t:
        want = hoomd.frame_kernel_gradients(t[0])
        spline = t.frame_kernel_gradients(0, 0.75, kernel='cubic_spline', where={'type': ['fluid']})
    assert pgsd_main(['info', path, '--sph-gradients']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "SPH gradients of frame 0 with h = 0.5 (wendland_c2) over 8 x 8 x 8 cells:" in lines
    assert "entries: 6 nowhere: 1" in lines
    assert "divergence: smallest %r largest %r" % (want.divergence_min, want.divergence_max) in lines
    assert "density rate: smallest %r largest %r not finite: 0" % (want.density_rate_min, want.density_rate_max) in lines
    assert "vorticity: largest %r at row %d" % (want.curl2 ** 0.5, want.curl_row) in lines
    assert "normal: largest %r at row %d" % (want.normal2 ** 0.5, want.normal_row) in lines
    assert not any(l.startswith("SPH sums") for l in lines)
    assert pgsd_main(['info', path, '--sph-gradients', '0.75', '--kernel', 'cubic_spline', '--types', 'fluid']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "SPH gradients of frame 0 with h = 0.75 (cubic_spline) over 5 x 5 x 5 cells (types fluid):" in lines
    assert "entries: 5 nowhere: 1" in lines
    assert "density rate: smallest %r largest %r not finite: 0" % (spline.density_rate_min, spline.density_rate_max) in lines
    assert pgsd_main(['info', path, '--sph-gradients', '2.5']) == 1
    assert "count twice" in capsys.readouterr().err
