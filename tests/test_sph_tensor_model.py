"""The numpy model of the SPH gradient tensors (pgsd.hoomd.sph_gradient_tensors / frame_gradient_tensors), the definition
the GPU pass equals exactly (tests/test_gpu_sph_tensors.py): it equals a plain double loop bit for bit -- so its
numpy.add.at is the sequential sum --, every mutation of the loop differs from it on the case that names it, the corrected
gradient of a linear velocity field is exact on a disordered cloud, the correction matrix is the reciprocal of the
lattice factors the gradients record, singular neighbourhoods stay uncorrected, and the command line prints it.  No GPU."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

from neighbours_cases import FLAT, ORTHO, TRICLINIC, random_rows
from sph_cases import CUBE, KERNELS, NONE, bits_equal
from sph_tensor_cases import (CASES, DET_AT, DET_MIN_AT, DET_MIN_BELOW, INFINITE_R, ISOLATED_INFINITE, LOOP_ENTRIES, MUTATIONS,
                              SINGULAR, fluid, jittered_cloud, loop_tensors, same, seeded_matrix, velocities)
from test_sph_gradient_model import LATTICE, small_frame


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
        got = hoomd.sph_gradient_tensors(**args)
        assert same(got, loop_tensors(**args)), (name, kernel, dtype)
    dims = kw.get('dimensions', 3)
    assert got.n == (n if rows is None else len(rows)) and got.G == hoomd.sph_gradient_scale(kernel, kw['h'], dims)
    assert got.correction.shape == (got.n, 6) and got.velocity_gradient.shape == (got.n, 9) and got.det_min == 0.0
    assert got.determinant.shape == got.shear_rate.shape == (got.n,)
    if name == 'all_nowhere':
        assert got.nowhere == got.n and got.determinant_min == np.inf and got.trace_max == -np.inf and got.uncorrected == 0
        assert got.det_at is None and got.shear is None and got.shear_row is None
        for a in (got.correction, got.determinant, got.velocity_gradient, got.shear_rate):
            assert not a.any() and not np.signbit(a).any()
    if name == 'three_cells':
        lost = got.cell == 27
        assert lost.any() and not got.correction[lost].any() and not np.signbit(got.velocity_gradient[lost]).any()
        assert got.uncorrected == 0                                     # every neighbourhood is full: all corrected
    if name == 'no_velocity':
        assert not got.velocity_gradient.any() and not got.shear_rate.any() and got.determinant.any()
    if name == 'flat':
        # d_z is 0: the z column of D and the z entries of L are +0.0 where corrected; a non-zero v_z still has a gradient
        fixed = got.determinant > 0
        assert fixed.any() and not got.correction[fixed][:, [2, 4, 5]].any() and not got.velocity_gradient[fixed][:, [2, 5, 8]].any()
        assert got.velocity_gradient[fixed][:, 6].any()
    if name == 'mass_density':
        assert got.not_finite > 0 and np.isnan(got.determinant).any()
        assert 0 < got.uncorrected < got.n - got.nowhere                # sparse: both ways of the epilogue in one case
    if name in ('mass_only', 'one_cell_65'):
        assert np.isnan(got.determinant[got.cell < np.prod(got.grid)]).all()   # a density stored nowhere is the schema's 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_list_in_any_order_with_repeats(kernel):
    case = fluid(5, 320)
    rows = np.concatenate([np.arange(300, 0, -1), [7, 7, 300, 12]])
    got = hoomd.sph_gradient_tensors(rows=rows, kernel=kernel, **case)
    assert same(got, loop_tensors(rows=rows, kernel=kernel, **case)) and got.n == 304 and got.uncorrected < 304


# ---------------------------------------------------------------- the mutations
@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_every_mutation_differs_on_its_case(mutation):
    switch, case = MUTATIONS[mutation]
    case = dict(case)
    kernels = [case.pop('kernel')] if 'kernel' in case else KERNELS
    for kernel in kernels:
        got = hoomd.sph_gradient_tensors(kernel=kernel, **case)
        assert same(got, loop_tensors(kernel=kernel, **case)), mutation
        assert not same(got, loop_tensors(kernel=kernel, **dict(case, **switch))), (mutation, kernel)


def test_the_det_min_boundary_is_strict():
    at, below = hoomd.sph_gradient_tensors(**DET_MIN_AT), hoomd.sph_gradient_tensors(**DET_MIN_BELOW)
    assert at.determinant[DET_AT] == at.det_min and below.det_min < at.det_min
    assert at.uncorrected == below.uncorrected + 1
    assert at.correction[DET_AT].tolist() == [1, 0, 0, 1, 0, 1] and below.correction[DET_AT].tolist() != [1, 0, 0, 1, 0, 1]
    assert same(below, loop_tensors(**DET_MIN_BELOW))


def test_the_fall_back_is_written_not_computed():
    got = hoomd.sph_gradient_tensors(**INFINITE_R)
    D = got.velocity_gradient
    assert got.uncorrected == 2 and np.isinf(D[:, 0]).all() and not np.isnan(D).any() and not D[:, 1:].any()
    alone = hoomd.sph_gradient_tensors(**ISOLATED_INFINITE)
    assert alone.uncorrected == 1 and np.isnan(alone.velocity_gradient[0, :3]).all() and alone.not_finite == 1
    assert alone.shear is None and alone.shear_at is None and alone.det_at == 0 and alone.determinant_min == 0.0


# ---------------------------------------------------------------- the physics
@pytest.mark.parametrize("dimensions", (3, 2))
def test_the_corrected_gradient_of_a_linear_field_is_exact(dimensions):
    """The jittered cloud, v = A x with a seeded A, Wendland: for EVERY entry that is ok at det_min = 1e-3 the corrected
    tensor is A within 1e-9 max|A| (a brute-force float64 check gave 2.3e-15, corners with det = 0.009 included; the bound
    leaves six orders for the inverse's conditioning, an error of a constant, sign or index is of order 1), while the
    uncorrected R misses A by more than 1e-3 max|A| somewhere: the correction acts."""
    p, mass, density, box = jittered_cloud(dimensions)
    A = seeded_matrix()
    if dimensions == 2:
        A[:, 2] = 0.0                                                   # (no derivative along z exists in 2-D)
    size = np.abs(A).max()
    got = hoomd.sph_gradient_tensors(p, p @ A.T, box, 1.5, mass=mass, density=density, dimensions=dimensions, det_min=1e-3)
    ok = (got.determinant > 1e-3) & (got.determinant < np.inf)
    assert got.n == (512 if dimensions == 3 else 144) and got.nowhere == 0 and ok.sum() == got.n - got.uncorrected
    assert ok.sum() > got.n // 2                                        # (the interior, at the least)
    error = np.abs(got.velocity_gradient[ok] - A.ravel()).max()
    print("max|D - A| = %.3g of max|A| = %.3g over %d entries" % (error, size, ok.sum()))
    assert error <= 1e-9 * size
    raw = hoomd.sph_gradient_tensors(p, p @ A.T, box, 1.5, mass=mass, density=density, dimensions=dimensions, det_min=np.inf)
    assert raw.uncorrected == raw.n and np.abs(raw.velocity_gradient - A.ravel()).max() > 1e-3 * size
    # (det_min decides what is corrected, never what the determinant is)
    assert bits_equal(raw.determinant, got.determinant)


@pytest.mark.parametrize("dimensions", (3, 2))
@pytest.mark.parametrize("kernel", KERNELS)
def test_the_correction_on_a_lattice_is_the_reciprocal_of_the_recorded_factor(kernel, dimensions):
    """The 12^3 (12^2) lattice of the gradient tests, h = 1.5, unit mass and density: for the entries at least 3 from every
    face sum_j V_j d_a (grad W)_b is f times the identity, so correction xx is 1/f within 2e-4 and the determinant f^dim
    within dim * 2e-4, with the f the gradients' lattice check records."""
    g = np.arange(12) - 5.5
    if dimensions == 3:
        p = np.array([(x, y, z) for z in g for y in g for x in g], np.float64)
    else:
        p = np.array([(x, y, 0.25) for y in g for x in g], np.float64)
    box = [24, 24, 24 if dimensions == 3 else 1, 0, 0, 0]
    got = hoomd.sph_gradient_tensors(p, None, box, 1.5, mass=np.ones(len(p)), density=np.ones(len(p)), dimensions=dimensions,
                                     kernel=kernel)
    inner = np.all(np.abs(p[got.rows][:, :dimensions]) <= 2.5, axis=1)
    f = LATTICE[kernel, dimensions]
    assert inner.sum() == 6 ** dimensions and f in (1.0006, 1.0101, 0.9974, 1.0067)
    assert np.all(np.abs(got.correction[inner, 0] - 1 / f) <= 2e-4)
    assert np.all(np.abs(got.determinant[inner] - f ** dimensions) <= dimensions * 2e-4)
    assert np.abs(got.correction[inner][:, [1, 2, 4]]).max() < 1e-12     # the lattice is symmetric: no off-diagonal


def test_simple_shear_and_rigid_rotation():
    """On the jittered cloud: v = (gamma y, 0, 0) has the shear rate |gamma| within 1e-9 |gamma|; v = omega x r has none
    within 1e-9 |omega|, while D01 - D10 is -2 omega_z within the same bound."""
    p, mass, density, box = jittered_cloud(3)
    gamma = -0.7
    v = np.zeros_like(p)
    v[:, 0] = gamma * p[:, 1]
    got = hoomd.sph_gradient_tensors(p, v, box, 1.5, mass=mass, density=density, det_min=1e-3)
    ok = got.determinant > 1e-3
    assert ok.sum() >= 504 and np.all(np.abs(got.shear_rate[ok] - abs(gamma)) <= 1e-9 * abs(gamma))
    omega = np.array([0.3, -0.5, 0.8])
    got = hoomd.sph_gradient_tensors(p, np.cross(omega, p), box, 1.5, mass=mass, density=density, det_min=1e-3)
    size = np.linalg.norm(omega)
    D = got.velocity_gradient[ok]
    assert np.all(got.shear_rate[ok] <= 1e-9 * size) and np.all(np.abs((D[:, 1] - D[:, 3]) + 2 * omega[2]) <= 1e-9 * size)


@pytest.mark.parametrize("name", sorted(SINGULAR))
def test_singular_neighbourhoods_stay_uncorrected(name):
    case = SINGULAR[name]
    flat = case.get('dimensions', 3) == 2
    for kernel in KERNELS:
        got = hoomd.sph_gradient_tensors(kernel=kernel, **case)
        assert same(got, loop_tensors(kernel=kernel, **case))
        assert got.uncorrected == got.n > 0 and got.nowhere == 0 and not (got.determinant != 0).any()
        assert np.array_equal(got.correction, np.tile([1, 0, 0, 1, 0, 0 if flat else 1], (got.n, 1)))
        # D == R: the uncorrected gradient, as a run that corrects nothing forms it
        raw = hoomd.sph_gradient_tensors(kernel=kernel, **dict(case, det_min=np.inf))
        assert bits_equal(got.velocity_gradient.ravel(), raw.velocity_gradient.ravel())
    if name != 'an isolated entry':
        assert got.velocity_gradient.any()


# ---------------------------------------------------------------- the summary
def test_the_summary_rules():
    """A NaN never replaces a bound, is no smallest determinant and no largest shear rate; the smaller position wins a
    tie; nothing: the gradients' rule."""
    p, w, mass, density, kw = CASES['mass_density']
    got = hoomd.sph_gradient_tensors(p, w, mass=mass, density=density, **kw)
    has = got.cell < np.prod(got.grid)
    det, shear, D = got.determinant[has], got.shear_rate[has], got.velocity_gradient[has]
    with np.errstate(invalid='ignore'):
        trace = (D[:, 0] + D[:, 4]) + D[:, 8]
    assert np.isnan(det).any() and np.isnan(shear).any() and got.not_finite == int((~np.isfinite(shear)).sum())
    assert got.determinant_min == np.nanmin(det) and got.determinant_max == np.nanmax(det)
    assert got.trace_min == np.nanmin(trace) and got.trace_max == np.nanmax(trace)
    assert got.uncorrected == int((~((det > 0) & (det < np.inf))).sum())
    assert got.det_at == int(np.flatnonzero(det == np.nanmin(det))[0]) and got.det_row == got.rows[got.det_at]
    finite = np.where(np.isnan(shear), -1.0, shear)
    assert got.shear == finite.max() and got.shear_at == int(np.argmax(finite)) and got.shear_row == got.rows[got.shear_at]
    # a tie: two pairs that are translates of one another give the same determinant and shear rate: the smaller position
    x = np.array([[-3, 0, 0], [-2.5, 0, 0], [3, 0, 0], [3.5, 0, 0]], np.float32)
    v = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0], [0, 1, 0]], np.float32)
    two = hoomd.sph_gradient_tensors(x, v, CUBE, 0.5, density=np.ones(4, np.float32))
    assert two.det_at == 0 and two.shear_at == 0 and two.shear > 0 and bits_equal(two.shear_rate[0], two.shear_rate[2])
    assert two.det_row == two.rows[0] and two.uncorrected == 4 and two.determinant_min == two.determinant_max == 0.0
    # nothing
    nothing = hoomd.sph_gradient_tensors(p, w, mass=mass, density=density, rows=np.arange(0), **kw)
    s = nothing.summary
    assert nothing.n == 0 and [int(v) for v in s[:8]] == [0, 0, 0, 0] + [NONE] * 4 and nothing.shear is None and s[13] == 0
    assert s[8:13].view(np.float64).tolist() == [np.inf, -np.inf, np.inf, -np.inf, 0.0]
    assert nothing.correction.shape == (0, 6) and nothing.velocity_gradient.shape == (0, 9)
    with pytest.raises(ValueError, match="14 words"):
        hoomd.KernelTensors(1.0, 'wendland_c2', (1, 1, 1), 3, np.zeros(13, np.uint64))


# ---------------------------------------------------------------- frames, h=None, the command line
def test_h_none_takes_a_uniform_slength_and_refuses_another():
    fr = small_frame(slength=[0.5] * 6)
    got = hoomd.frame_gradient_tensors(fr, det_min=0.0)
    want = hoomd.sph_gradient_tensors(fr.particles.position, fr.particles.velocity, fr.configuration.box, 0.5,
                                      mass=fr.particles.mass, density=fr.particles.density, det_min=0.0)
    assert got.h == 0.5 and np.array_equal(got.summary, want.summary)
    assert bits_equal(got.velocity_gradient.ravel(), want.velocity_gradient.ravel()) and got.shear > 0
    assert hoomd.frame_gradient_tensors(small_frame()).h == 1.0                       # stored nowhere: the schema default
    assert hoomd.frame_gradient_tensors(small_frame(slength=[0.5] * 6), h=0.75).h == 0.75
    with pytest.raises(ValueError, match="slength ranges from 0.5 to 0.75"):
        hoomd.frame_gradient_tensors(small_frame(slength=[0.5, 0.5, 0.75, 0.5, 0.5, 0.5]))
    # the selection is the list: both i and j come from it
    fluid_only = hoomd.frame_gradient_tensors(fr, where={'type': ['fluid']}, det_min=0.0)
    assert fluid_only.n == 5 and not bits_equal(fluid_only.velocity_gradient[fluid_only.rows == 0],
                                                 got.velocity_gradient[got.rows == 0])
    # a velocity that is stored nowhere is the zero vector; a density stored nowhere is the schema's 0.0
    still = hoomd.frame_gradient_tensors(small_frame(slength=[0.5] * 6, velocity=False), det_min=0.0)
    assert not still.velocity_gradient.any() and bits_equal(still.determinant, got.determinant)
    arrays = dict(position=fr.particles.position, velocity=fr.particles.velocity, mass=fr.particles.mass)
    none = hoomd.frame_gradient_tensors(arrays, h=0.5, box=fr.configuration.box)
    assert np.isnan(none.determinant[:5]).all() and none.uncorrected == 5


def test_what_sph_gradient_tensors_refuses():
    p = random_rows(1, 10, ORTHO)
    w = velocities(1, 10).astype(np.float32)
    for h in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match="finite and positive"):
            hoomd.sph_gradient_tensors(p, w, ORTHO, h)
    for det_min in (-1e-300, float('nan'), -np.inf):
        with pytest.raises(ValueError, match="det_min is a number, at least 0"):
            hoomd.sph_gradient_tensors(p, w, ORTHO, 0.5, det_min=det_min)
    with pytest.raises(ValueError, match="kernel is one of"):
        hoomd.sph_gradient_tensors(p, w, ORTHO, 0.5, kernel='gaussian')
    with pytest.raises(ValueError, match="narrower"):
        hoomd.sph_gradient_tensors(p, w, ORTHO, 0.65, cells=(8, 6, 4))
    with pytest.raises(ValueError, match="narrower"):
        hoomd.sph_gradient_tensors(p, w, TRICLINIC, 0.65, cells=hoomd.cell_grid_for(ORTHO, 1.3))  # the tilt narrows x
    with pytest.raises(ValueError, match="2\\^20"):
        hoomd.sph_gradient_tensors(p, w, [1000, 800, 600, 0, 0, 0], 0.5, cells=(1000, 800, 600))
    with pytest.raises(ValueError, match="count twice"):
        hoomd.sph_gradient_tensors(p, w, ORTHO, 1.6)                                   # 2h = 3.2 > Lz / 2
    with pytest.raises(ValueError, match="cz == 1"):
        hoomd.sph_gradient_tensors(p, w, FLAT, 0.3, cells=(2, 2, 2), dimensions=2)
    with pytest.raises(ValueError, match="float32 or float64"):
        hoomd.sph_gradient_tensors(p.astype(np.int32), w, ORTHO, 0.5)
    with pytest.raises(ValueError, match="mass holds one float32 or float64 value per row"):
        hoomd.sph_gradient_tensors(p, w, ORTHO, 0.5, mass=np.ones(9))
    with pytest.raises(ValueError, match="density holds one float32 or float64 value per row"):
        hoomd.sph_gradient_tensors(p, w, ORTHO, 0.5, density=np.ones(10, np.int32))
    with pytest.raises(ValueError, match="velocity holds three float32 or float64 values per row"):
        hoomd.sph_gradient_tensors(p, w[:9], ORTHO, 0.5)
    with pytest.raises(ValueError, match="velocity holds three float32 or float64 values per row"):
        hoomd.sph_gradient_tensors(p, w.astype(np.int32), ORTHO, 0.5)
    with pytest.raises(ValueError, match="needs the box"):
        hoomd.frame_gradient_tensors(dict(position=p), h=0.5)


def test_the_command_line_prints_the_tensors(tmp_path, capsys):
    path = str(tmp_path / "small.gsd")
    with hoomd.open(path, 'w') as t:
        t.append(small_frame(slength=[0.5] * 6))
    with hoomd.open(path, 'r') as t:
        want = hoomd.frame_gradient_tensors(t[0])
        loose = t.frame_gradient_tensors(0, 0.75, kernel='cubic_spline', det_min=0.0, where={'type': ['fluid']})
    assert pgsd_main(['info', path, '--sph-tensors']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "SPH gradient tensors of frame 0 with h = 0.5 (wendland_c2), det_min = 0.25, over 8 x 8 x 8 cells:" in lines
    assert "entries: 6 nowhere: 1 uncorrected: %d" % want.uncorrected in lines and want.uncorrected == 5
    assert "determinant: smallest %r largest %r" % (want.determinant_min, want.determinant_max) in lines
    assert "trace: smallest %r largest %r" % (want.trace_min, want.trace_max) in lines
    assert "shear rate: largest %r at row %d not finite: 0" % (want.shear, want.shear_row) in lines
    assert not any(l.startswith("SPH gradients") for l in lines)
    assert pgsd_main(['info', path, '--sph-tensors', '0.75', '--det-min', '0', '--kernel', 'cubic_spline', '--types', 'fluid']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "SPH gradient tensors of frame 0 with h = 0.75 (cubic_spline), det_min = 0.0, over 5 x 5 x 5 cells (types fluid):" in lines
    assert "entries: 5 nowhere: 1 uncorrected: %d" % loose.uncorrected in lines
    assert "shear rate: largest %r at row %d not finite: 0" % (loose.shear, loose.shear_row) in lines
    assert pgsd_main(['info', path, '--sph-tensors', '2.5']) == 1
    assert "count twice" in capsys.readouterr().err
    assert pgsd_main(['info', path, '--sph-tensors', '--det-min', '-1']) == 1
    assert "det_min" in capsys.readouterr().err
