"""The numpy model of the SPH accelerations (pgsd.hoomd.sph_accelerations / frame_accelerations), the definition the GPU
pass equals exactly (tests/test_gpu_sph_forces.py): it equals a plain double loop bit for bit -- so its numpy.add.at is the
sequential sum --, every mutation of the loop differs from it on the case that names it, a linear pressure field on a
lattice balances gravity, a parabolic velocity profile gives back its Laplacian, the pressure force conserves momentum to
rounding, and the command line prints it.  No GPU."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

from neighbours_cases import FLAT, ORTHO, TRICLINIC, random_rows
from sph_cases import CASES as SUM_CASES, CUBE, KERNELS, NONE, bits_equal
from sph_force_cases import (CASES, EQUIVALENT, LOOP_ENTRIES, MUTATIONS, TERMS, _small, loop_accelerations, pressures, same,
                             velocities)


# ---------------------------------------------------------------- the model is the loop
@pytest.mark.parametrize("terms", sorted(TERMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_equals_the_double_loop_bit_for_bit(name, kernel, terms):
    p, w, mass, density, pressure, kw = CASES[name]
    n = len(p)
    # (the loop is quadratic in a crowded cell: beyond LOOP_ENTRIES entries it takes a strided sub-list of the case)
    rows = None if n <= LOOP_ENTRIES else np.arange(0, n, -(-n // LOOP_ENTRIES))
    for dtype in (np.float64, np.float32):
        args = dict(kw, position=p.astype(dtype), velocity=None if w is None else w.astype(dtype), mass=mass, density=density,
                    pressure=pressure, rows=rows, kernel=kernel, **TERMS[terms])
        got = hoomd.sph_accelerations(**args)
        assert same(got, loop_accelerations(**args)), (name, kernel, dtype)
    assert got.n == (n if rows is None else len(rows)) and got.G == hoomd.sph_gradient_scale(kernel, kw['h'], kw.get('dimensions', 3))
    assert got.pressure_acc.shape == (got.n, 3) and got.total.shape == (got.n, 3)
    assert (got.viscous_acc is None) == (terms == 'plain') and (got.viscous2 is None) >= (terms == 'plain')
    assert got.viscosity == TERMS[terms]['viscosity'] and got.gravity == tuple(TERMS[terms]['gravity'] or (0.0, 0.0, 0.0))
    if name == 'all_nowhere':
        assert got.nowhere == got.n and got.total2 is None and got.pressure_at is None and got.force_time_step() is None
        for a in (got.pressure_acc, got.viscous_acc, got.total):        # +0.0, the gravity notwithstanding
            assert a is None or (not a.any() and not np.signbit(a).any())
    if name == 'three_cells':
        lost = got.cell == 27
        assert lost.any() and not got.total[lost].any() and not np.signbit(got.pressure_acc[lost]).any()
    if name in ('one_cell_65', 'mass_only', 'no_density'):
        # the density is the schema's 0.0: every A is infinite and every own term inf * 0
        assert got.not_finite == got.n - got.nowhere and got.total2 is None and np.isnan(got.pressure_acc).all()
    if name == 'no_pressure':
        assert not got.pressure_acc.any() and got.pressure2 == 0.0
    if name == 'no_velocity' and terms == 'viscous':
        assert not got.viscous_acc.any() and got.viscous2 == 0.0 and got.pressure_acc.any()
    if name == 'flat':
        assert not got.pressure_acc[:, 2].any() and (terms == 'plain' or got.viscous_acc[:, 2].any())
    if name == 'mass_density':
        assert 0 < got.not_finite < got.n and np.isnan(got.total).any() and got.total2 > 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_list_in_any_order_with_repeats(kernel):
    p, w, mass, density, pressure, kw = CASES['three_cells']
    rows = np.concatenate([np.arange(300, 0, -1), [7, 7, 300, 12]])
    args = dict(kw, position=p, velocity=w, mass=mass, density=density, pressure=pressure, rows=rows, kernel=kernel,
                **TERMS['viscous'])
    got = hoomd.sph_accelerations(**args)
    assert same(got, loop_accelerations(**args)) and got.n == 304


def test_the_sums_and_the_gradients_keep_their_bits():
    """`_sph_list` serves a fourth column: what the sums and the gradients read of it has not moved."""
    p, w, mass, density, pressure, kw = CASES['triclinic_754']
    from sph_cases import loop_sums, same as same_sums
    from sph_gradient_cases import loop_gradients, same as same_gradients
    rows = np.arange(0, len(p), 2)
    assert same_sums(hoomd.sph_kernel_sums(p, mass=mass, density=density, rows=rows, **kw),
                     loop_sums(p, mass=mass, density=density, rows=rows, **kw))
    assert same_gradients(hoomd.sph_kernel_gradients(p, w, mass=mass, density=density, rows=rows, **kw),
                          loop_gradients(p, w, mass=mass, density=density, rows=rows, **kw))


# ---------------------------------------------------------------- the mutations
@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_every_mutation_differs_on_its_case(mutation):
    switch, case = MUTATIONS[mutation]
    case = dict(case)
    kernels = [case.pop('kernel')] if 'kernel' in case else KERNELS
    for kernel in kernels:
        got = hoomd.sph_accelerations(kernel=kernel, **case)
        assert same(got, loop_accelerations(kernel=kernel, **case)), mutation
        assert not same(got, loop_accelerations(kernel=kernel, **dict(case, **switch))), (mutation, kernel)


def test_the_mutation_no_input_can_show():
    """S divided per pair: p / (rho*rho) of the same two doubles is the same double whenever it is formed."""
    for mutation, (switch, case) in EQUIVALENT.items():
        for kernel in KERNELS:
            got = hoomd.sph_accelerations(kernel=kernel, **case)
            assert same(got, loop_accelerations(kernel=kernel, **case)), mutation
            assert same(got, loop_accelerations(kernel=kernel, **dict(case, **switch))), mutation


# ---------------------------------------------------------------- the physics
# sum_j V_j d_a (grad W)_a on the unit lattice at h = 1.5 (the gradients' lattice constants) ...
LATTICE = {('wendland_c2', 3): 1.0006, ('cubic_spline', 3): 1.0101, ('wendland_c2', 2): 0.9974, ('cubic_spline', 2): 1.0067}
# ... and the lattice factor of the Laplacian 2 sum_j V_j F d2 / (d2 + eta2), measured from the model on a parabolic profile
LAPLACIAN = {('wendland_c2', 3): 0.990600, ('cubic_spline', 3): 1.000985, ('wendland_c2', 2): 0.984879,
             ('cubic_spline', 2): 0.995207}
BOUND = 0.02


def lattice(dimensions):
    """The 12^3 lattice (12^2 in 2-D) of spacing 1 in a box of edge 24 (no pair wraps): (positions, box, the axis of the
    gradient, keyword arguments)."""
    g = np.arange(12) - 5.5
    if dimensions == 3:
        return np.array([(x, y, z) for z in g for y in g for x in g], np.float64), [24, 24, 24, 0, 0, 0], 2
    return np.array([(x, y, 0.25) for y in g for x in g], np.float64), [24, 24, 1, 0, 0, 0], 1


def inner_of(got, p, dimensions):
    inner = np.all(np.abs(p[got.rows][:, :dimensions]) <= 2.5, axis=1)      # 3 or more from every face of the lattice
    assert inner.sum() == 6 ** dimensions and got.n == 12 ** dimensions and got.nowhere == 0 and got.not_finite == 0
    return inner


@pytest.mark.parametrize("dimensions", (3, 2))
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_hydrostatic_column_is_in_equilibrium(kernel, dimensions):
    """Unit mass and density, p = 20 - z (20 - y in 2-D), gravity -1 on that axis: for the entries at least 3 from every
    face |total| is below 2 % of g, and the pressure acceleration along the axis is the kernel's lattice constant."""
    p, box, axis = lattice(dimensions)
    gravity = [0.0, 0.0, 0.0]
    gravity[axis] = -1.0
    ones = np.ones(len(p))
    got = hoomd.sph_accelerations(p, None, box, 1.5, mass=ones, density=ones, pressure=20.0 - p[:, axis], gravity=gravity,
                                  dimensions=dimensions, kernel=kernel)
    inner = inner_of(got, p, dimensions)
    norm = np.sqrt((got.total[inner] ** 2).sum(axis=1))
    print("hydrostatic", kernel, dimensions, "largest |total| inside:", norm.max(), "pressure_acc along the axis:",
          got.pressure_acc[inner, axis].min(), got.pressure_acc[inner, axis].max(), "across:",
          np.abs(np.delete(got.pressure_acc[inner], axis, axis=1)).max())
    assert np.all(norm < BOUND * 1.0)
    assert np.all(np.abs(got.pressure_acc[inner, axis] - LATTICE[kernel, dimensions]) < 2e-4)
    assert np.abs(np.delete(got.pressure_acc[inner], axis, axis=1)).max() < 1e-12
    assert got.viscous_acc is None and got.viscous2 is None
    # the largest acceleration lies on a face of the lattice, and it sets the time step
    assert np.abs(p[got.total_row][:dimensions]).max() == 5.5 and got.total_at == int(np.flatnonzero(got.rows == got.total_row)[0])
    assert got.force_time_step() == 0.25 * np.sqrt(1.5 / np.sqrt(got.total2)) and got.force_time_step(0.5) == 2 * got.force_time_step()


@pytest.mark.parametrize("dimensions", (3, 2))
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_parabolic_profile_gives_back_its_laplacian(kernel, dimensions):
    """The same lattices, v_x = 0.5 z^2 (0.5 y^2 in 2-D), mu = 1, constant pressure: the inner entries' viscous_acc_x is
    within 2 % of mu lap(v_x) / rho = 1, and their mean is the operator's own lattice factor."""
    p, box, axis = lattice(dimensions)
    v = np.zeros_like(p)
    v[:, 0] = 0.5 * p[:, axis] ** 2
    ones = np.ones(len(p))
    got = hoomd.sph_accelerations(p, v, box, 1.5, mass=ones, density=ones, pressure=ones, viscosity=1.0, dimensions=dimensions,
                                  kernel=kernel)
    inner = inner_of(got, p, dimensions)
    ax = got.viscous_acc[inner, 0]
    print("viscous", kernel, dimensions, "viscous_acc_x inside: smallest %r largest %r mean %r" % (ax.min(), ax.max(), ax.mean()))
    assert max(abs(c - 1) for c in LAPLACIAN.values()) < BOUND
    assert np.all(np.abs(ax - 1.0) <= BOUND)
    assert abs(ax.mean() - LAPLACIAN[kernel, dimensions]) < 2e-4
    assert not got.viscous_acc[:, 1:].any()                             # v has an x component alone
    assert bits_equal(got.total, (got.pressure_acc + got.viscous_acc) + 0.0)


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_pressure_force_conserves_momentum_to_rounding(kernel):
    """A periodic cloud, no entry nowhere, neither gravity nor viscosity: the pair terms m_i m_j G S e cancel exactly in
    exact arithmetic, so |sum_i m_i pressure_acc_i[k]| stays below the bound of recursive summation, (c + n + 4) u times
    the sum of the terms' sizes: c additions in the longest candidate run, n in the sum over the entries, and four
    roundings in a term (S * e, m_j *, G *, m_i *); u = 2^-53."""
    case = dict(_small(81, 200), viscosity=None, gravity=None)
    extras = {}
    want = loop_accelerations(kernel=kernel, extras=extras, **case)
    got = hoomd.sph_accelerations(kernel=kernel, **case)
    assert same(got, want) and got.nowhere == 0 and got.not_finite == 0
    m = case['mass'][got.rows]
    n, c = got.n, extras['longest']
    assert n == 200 and 1 < c < n
    for k in range(3):
        momentum = 0.0
        for i in range(n):
            momentum = momentum + m[i] * got.pressure_acc[i, k]
        bound = (c + n + 4) * 2.0 ** -53 * extras['budget'][k]
        print("momentum", kernel, k, "sum:", momentum, "bound:", bound, "largest m*a:", np.abs(m * got.pressure_acc[:, k]).max())
        assert abs(momentum) <= bound
        # (and the bound has teeth: it lies a million times below one entry's own m * a, so a lost pair term would show)
        assert bound < 1e-6 * np.abs(m * got.pressure_acc[:, k]).max()


# ---------------------------------------------------------------- the summary
def test_the_summary_rules():
    """A NaN never is a largest norm; the smaller position wins a tie; not_finite counts entries, not components; no
    viscosity: no viscous words."""
    p, w, mass, density, pressure, kw = CASES['mass_density']
    got = hoomd.sph_accelerations(p, w, mass=mass, density=density, pressure=pressure, **kw, **TERMS['viscous'])
    has = got.cell < np.prod(got.grid)
    bad = ~np.isfinite(got.total[has]).all(axis=1)
    assert got.not_finite == int(bad.sum()) > 0 and got.summary[2] == got.not_finite
    for name, values in (('total', got.total), ('pressure', got.pressure_acc), ('viscous', got.viscous_acc)):
        v = values[has]
        norm2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        assert np.isnan(norm2).any()
        at = getattr(got, name + '_at')
        assert getattr(got, name + '2') == np.nanmax(norm2) == norm2[at] and getattr(got, name + '_row') == got.rows[at]
        assert at == int(np.flatnonzero(norm2 == np.nanmax(norm2))[0])
    # a tie: two pairs that are translates of one another give the same accelerations: the smaller list position
    x = np.array([[-3, 0, 0], [-2.5, 0, 0], [3, 0, 0], [3.5, 0, 0]], np.float32)
    v = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0], [0, 1, 0]], np.float32)
    ones = np.ones(4, np.float32)
    two = hoomd.sph_accelerations(x, v, CUBE, 0.5, density=ones, pressure=ones, viscosity=0.5)
    assert two.total_at == 0 and two.pressure_at == 0 and two.viscous_at == 0 and two.total2 > 0 and two.viscous2 > 0
    assert bits_equal(two.total[0], two.total[2]) and two.total_row == two.rows[0] and two.not_finite == 0
    # without a viscosity: no viscous term, and gravity=None still adds +0.0 (a -0.0 becomes +0.0)
    none = hoomd.sph_accelerations(x, v, CUBE, 0.5, density=ones, pressure=ones)
    assert none.viscous_acc is None and none.viscous2 is None and none.viscous_at is None and none.viscous_row is None
    assert bits_equal(none.pressure_acc, two.pressure_acc) and bits_equal(none.total, none.pressure_acc + 0.0)
    s = none.summary
    assert [int(c) for c in s[7:9]] == [NONE] * 2 and s[11:].view(np.float64).tolist() == [0.0] and none.gravity == (0.0, 0.0, 0.0)
    # nothing
    nothing = hoomd.sph_accelerations(p, w, mass=mass, density=density, pressure=pressure, rows=np.arange(0), **kw)
    s = nothing.summary
    assert nothing.n == 0 and [int(c) for c in s[:9]] == [0, 0, 0] + [NONE] * 6 and nothing.total2 is None
    assert s[9:].view(np.float64).tolist() == [0.0, 0.0, 0.0] and nothing.total.shape == (0, 3)
    assert nothing.force_time_step() is None
    with pytest.raises(ValueError, match="12 words"):
        hoomd.KernelAccelerations(0.5, 'wendland_c2', (1, 1, 1), 3, np.zeros(13, np.uint64))


# ---------------------------------------------------------------- frames, h=None, the command line
def small_frame(slength=None, density=True, pressure=True):
    fr = hoomd.Frame()
    fr.configuration.box = [8, 8, 8, 0, 0, 0]
    fr.particles.N = 6
    fr.particles.types = ['fluid', 'wall']
    fr.particles.typeid = np.array([0, 0, 1, 0, 0, 0], np.uint32)
    fr.particles.position = np.array([[1, 1, 1], [1.5, 1, 1], [1, 1.25, 1], [-3.9, 0, 0], [3.9, 0, 0], [np.nan, 0, 0]], np.float32)
    fr.particles.mass = np.array([1, 2, 1, 1, 1, 1], np.float32)
    fr.particles.velocity = np.array([[0, 0, 0], [0, 1, 0], [-1, 0, 0.5], [1, 0, 0], [-1, 0, 0], [9, 9, 9]], np.float32)
    if density:
        fr.particles.density = np.array([1, 1, 1, 0.5, 0.5, 1], np.float32)
    if pressure:
        fr.particles.pressure = np.array([1, 2, 3, 1, 1.5, 1], np.float32)
    if slength is not None:
        fr.particles.slength = np.asarray(slength, np.float32)
    return fr


def test_h_none_takes_a_uniform_slength_and_refuses_another():
    fr = small_frame(slength=[0.5] * 6)
    got = hoomd.frame_accelerations(fr, viscosity=0.25, gravity=(0, 0, -1))
    want = hoomd.sph_accelerations(fr.particles.position, fr.particles.velocity, fr.configuration.box, 0.5, mass=fr.particles.mass,
                                   density=fr.particles.density, pressure=fr.particles.pressure, viscosity=0.25, gravity=(0, 0, -1))
    assert got.h == 0.5 and np.array_equal(got.summary, want.summary) and bits_equal(got.total.ravel(), want.total.ravel())
    assert got.n == 6 and got.nowhere == 1 and got.total2 > 1 and got.viscous2 > 0 and got.not_finite == 0
    assert hoomd.frame_accelerations(small_frame()).h == 1.0                             # stored nowhere: the schema default
    assert hoomd.frame_accelerations(small_frame(slength=[0.5] * 6), h=0.75).h == 0.75
    with pytest.raises(ValueError, match="slength ranges from 0.5 to 0.75"):
        hoomd.frame_accelerations(small_frame(slength=[0.5, 0.5, 0.75, 0.5, 0.5, 0.5]))
    # the selection is the list: both i and j come from it
    fluid = hoomd.frame_accelerations(fr, where={'type': ['fluid']})
    mine, theirs = fluid.pressure_acc[list(fluid.rows).index(0)], got.pressure_acc[list(got.rows).index(0)]
    assert fluid.n == 5 and mine.any() and not bits_equal(mine, theirs)                  # row 0 has lost the wall row 2
    # a pressure that is stored nowhere is 0.0: no pressure acceleration; a density stored nowhere is 0.0: nothing is finite
    still = hoomd.frame_accelerations(small_frame(slength=[0.5] * 6, pressure=False), gravity=(0, 0, -1))
    assert not still.pressure_acc.any() and still.total2 == 1.0 and still.force_time_step() == 0.25 * np.sqrt(0.5)
    void = hoomd.frame_accelerations(small_frame(slength=[0.5] * 6, density=False))
    assert void.not_finite == 5 and void.total2 is None
    arrays = dict(position=fr.particles.position, density=fr.particles.density, pressure=fr.particles.pressure)
    assert hoomd.frame_accelerations(arrays, h=0.5, box=fr.configuration.box).viscous_acc is None


def test_what_sph_accelerations_refuses():
    p = random_rows(1, 10, ORTHO)
    w = velocities(1, 10).astype(np.float32)
    for h in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match="finite and positive"):
            hoomd.sph_accelerations(p, w, ORTHO, h)
    with pytest.raises(ValueError, match="kernel is one of"):
        hoomd.sph_accelerations(p, w, ORTHO, 0.5, kernel='gaussian')
    with pytest.raises(ValueError, match="narrower"):
        hoomd.sph_accelerations(p, w, ORTHO, 0.65, cells=(8, 6, 4))
    with pytest.raises(ValueError, match="narrower"):
        hoomd.sph_accelerations(p, w, TRICLINIC, 0.65, cells=hoomd.cell_grid_for(ORTHO, 1.3))   # the tilt narrows x
    with pytest.raises(ValueError, match="2\\^20"):
        hoomd.sph_accelerations(p, w, [1000, 800, 600, 0, 0, 0], 0.5, cells=(1000, 800, 600))
    with pytest.raises(ValueError, match="count twice"):
        hoomd.sph_accelerations(p, w, ORTHO, 1.6)                                       # 2h = 3.2 > Lz / 2
    with pytest.raises(ValueError, match="cz == 1"):
        hoomd.sph_accelerations(p, w, FLAT, 0.3, cells=(2, 2, 2), dimensions=2)
    with pytest.raises(ValueError, match="float32 or float64"):
        hoomd.sph_accelerations(p.astype(np.int32), w, ORTHO, 0.5)
    with pytest.raises(ValueError, match="mass holds one float32 or float64 value per row"):
        hoomd.sph_accelerations(p, w, ORTHO, 0.5, mass=np.ones(9))
    with pytest.raises(ValueError, match="density holds one float32 or float64 value per row"):
        hoomd.sph_accelerations(p, w, ORTHO, 0.5, density=np.ones(10, np.int32))
    with pytest.raises(ValueError, match="pressure holds one float32 or float64 value per row"):
        hoomd.sph_accelerations(p, w, ORTHO, 0.5, pressure=np.ones(11))
    with pytest.raises(ValueError, match="pressure holds one float32 or float64 value per row"):
        hoomd.sph_accelerations(p, w, ORTHO, 0.5, pressure=np.ones(10, np.int64))
    with pytest.raises(ValueError, match="velocity holds three float32 or float64 values per row"):
        hoomd.sph_accelerations(p, w[:9], ORTHO, 0.5)
    for mu in (-0.5, float('inf'), float('nan')):
        with pytest.raises(ValueError, match="viscosity is a finite number, at least 0, or None"):
            hoomd.sph_accelerations(p, w, ORTHO, 0.5, viscosity=mu)
    for g in ((0, 0), (0, 0, float('nan')), (float('inf'), 0, 0), (0, 0, 0, 0)):
        with pytest.raises(ValueError, match="gravity holds three finite numbers"):
            hoomd.sph_accelerations(p, w, ORTHO, 0.5, gravity=g)
    with pytest.raises(ValueError, match="needs the box"):
        hoomd.frame_accelerations(dict(position=p), h=0.5)
    assert set(SUM_CASES) < set(CASES) and pressures(1, 10).shape == (10,)


def test_the_command_line_prints_the_accelerations(tmp_path, capsys):
    path = str(tmp_path / "small.gsd")
    with hoomd.open(path, 'w') as t:
        t.append(small_frame(slength=[0.5] * 6))
    with hoomd.open(path, 'r') as t:
        want = hoomd.frame_accelerations(t[0])
        spline = t.frame_accelerations(0, 0.75, kernel='cubic_spline', viscosity=0.25, gravity=(0, -1, 0.5), where={'type': ['fluid']})
    assert pgsd_main(['info', path, '--sph-forces']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "SPH accelerations of frame 0 with h = 0.5 (wendland_c2) over 8 x 8 x 8 cells:" in lines
    assert "entries: 6 nowhere: 1" in lines
    assert "viscosity: none gravity: 0.0 0.0 0.0" in lines
    assert "total: largest %r at row %d" % (want.total2 ** 0.5, want.total_row) in lines
    assert "pressure: largest %r at row %d" % (want.pressure2 ** 0.5, want.pressure_row) in lines
    assert not any(l.startswith("viscous:") for l in lines) and "not finite: 0" in lines
    assert "time step: %r (0.25 * sqrt(h / largest total))" % want.force_time_step() in lines
    assert not any(l.startswith("SPH gradients") for l in lines)
    assert pgsd_main(['info', path, '--sph-forces', '0.75', '--kernel', 'cubic_spline', '--types', 'fluid', '--viscosity', '0.25',
                      '--gravity', '0,-1,0.5']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "SPH accelerations of frame 0 with h = 0.75 (cubic_spline) over 5 x 5 x 5 cells (types fluid):" in lines
    assert "entries: 5 nowhere: 1" in lines and "viscosity: 0.25 gravity: 0.0 -1.0 0.5" in lines
    assert "total: largest %r at row %d" % (spline.total2 ** 0.5, spline.total_row) in lines
    assert "viscous: largest %r at row %d" % (spline.viscous2 ** 0.5, spline.viscous_row) in lines
    assert "time step: %r (0.25 * sqrt(h / largest total))" % spline.force_time_step() in lines
    assert pgsd_main(['info', path, '--sph-forces', '2.5']) == 1
    assert "count twice" in capsys.readouterr().err
    assert pgsd_main(['info', path, '--sph-forces', '--gravity', '0,1']) == 1
    assert "gravity holds three finite numbers" in capsys.readouterr().err
    assert pgsd_main(['info', path, '--sph-forces', '--viscosity', '-1']) == 1
    assert "viscosity is a finite number" in capsys.readouterr().err
