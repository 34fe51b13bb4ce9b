"""The numpy model of the SPH body forces (pgsd.hoomd.sph_body_force / frame_body_force), the definition the GPU pass
equals exactly (tests/test_gpu_sph_body.py): it equals a plain double loop bit for bit -- so its numpy.add.at is the
sequential sum and its `_ordered_sum` the tile tree --, every mutation of the loop differs from it on the case that names it,
the fluid's force on the body is minus the body's on the fluid, a block in a hydrostatic column is lifted by the weight it
displaces, a couple gives arm times force, and the command line prints it.  No GPU."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

from neighbours_cases import FLAT, ORTHO, TRICLINIC, random_rows
from sph_cases import CUBE, KERNELS, NONE, bits_equal
from sph_body_cases import (CASES, LOOP_ENTRIES, MUTATIONS, TERMS, _small, case_arguments, loop_body_force, ordered_sum, same,
                            velocities)
from test_sph_force_model import LATTICE, lattice, small_frame

U = 2.0 ** -53


# ---------------------------------------------------------------- the model is the loop
@pytest.mark.parametrize("terms", sorted(TERMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_equals_the_double_loop_bit_for_bit(name, kernel, terms):
    kw = case_arguments(name)
    body = kw['body_rows']
    # (the loop is quadratic in a crowded cell: beyond LOOP_ENTRIES targets it takes a strided sub-list of the body)
    if len(body) > LOOP_ENTRIES:
        body = body[::-(-len(body) // LOOP_ENTRIES)]
    for dtype in (np.float64, np.float32):
        args = dict(kw, position=kw['position'].astype(dtype), velocity=None if kw['velocity'] is None else kw['velocity'].astype(dtype),
                    body_rows=body, kernel=kernel, **TERMS[terms])
        got = hoomd.sph_body_force(**args)
        assert same(got, loop_body_force(**args)), (name, kernel, dtype)
    assert got.n == len(body) and got.n_sources == len(kw['fluid_rows'])
    assert got.G == hoomd.sph_gradient_scale(kernel, kw['h'], kw.get('dimensions', 3))
    assert got.pressure_acc.shape == (got.n, 3) and got.contacts.shape == (got.n,) and got.contacts.dtype == np.uint32
    assert (got.viscous_acc is None) == (terms == 'plain')
    assert got.viscosity == TERMS[terms]['viscosity'] and got.about == tuple(TERMS[terms]['about'] or (0.0, 0.0, 0.0))
    assert got.pairs == int(got.contacts.sum()) and got.wetted == int(np.count_nonzero(got.contacts))
    if terms == 'plain':
        assert got.force_viscous == (0.0, 0.0, 0.0) and got.torque_viscous == (0.0, 0.0, 0.0)
        assert not np.signbit(got.summary[13:16].view(np.float64)).any() and got.force == got.force_pressure
    if name == 'all_nowhere':
        assert got.nowhere == got.n and got.sources_nowhere == got.n_sources and got.largest2 is None and got.pairs == 0
        for a in (got.pressure_acc, got.viscous_acc):
            assert a is None or (not a.any() and not np.signbit(a).any())
        assert got.force == (0.0, 0.0, 0.0) and got.torque == (0.0, 0.0, 0.0)
    if name == 'three_cells':
        lost = got.cell == 27
        assert lost.any() and not got.contacts[lost].any() and not np.signbit(got.pressure_acc[lost]).any()
        assert got.sources_nowhere > 0
    if name in ('one_cell_65', 'mass_only', 'no_density'):
        # the density is the schema's 0.0: every A is infinite -- every wetted target is bad and no sum takes a term
        assert got.bad >= got.wetted > 0 and got.force_pressure == (0.0, 0.0, 0.0) and got.largest2 in (None, 0.0)
    if name == 'no_pressure':
        assert not got.pressure_acc.any() and got.force_pressure == (0.0, 0.0, 0.0) and got.largest2 == 0.0
    if name == 'flat':
        assert got.force_pressure[2] == 0.0 and got.torque_pressure[0] == 0.0 and got.torque_pressure[1] == 0.0
        assert got.torque_pressure[2] != 0.0
    if name == 'mass_density':
        assert 0 < got.bad < got.n and np.isnan(got.pressure_acc).any() and np.isfinite(got.force).all() and got.largest2 > 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_lists_in_any_order_with_repeats_and_overlap(kernel):
    kw = case_arguments('three_cells')
    body = np.concatenate([np.arange(300, 0, -1), [7, 7, 300, 12]])
    fluid = np.concatenate([np.arange(250, 900), [7, 400, 400]])         # (rows 250 .. 300, 7 and 12: in both lists)
    args = dict(kw, body_rows=body, fluid_rows=fluid, kernel=kernel, **TERMS['viscous'])
    got = hoomd.sph_body_force(**args)
    assert same(got, loop_body_force(**args)) and got.n == 304 and got.n_sources == 653


def test_the_ordered_sum_of_the_loop_is_the_models():
    rng = np.random.default_rng(7)
    for n in (0, 1, 255, 256, 257, 4095, 4096, 4097, 9000):
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, size=n)
        assert bits_equal(hoomd._ordered_sum(v), ordered_sum([float(c) for c in v])), n


# ---------------------------------------------------------------- the mutations
@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_every_mutation_differs_on_its_case(mutation):
    switch, case = MUTATIONS[mutation]
    case = dict(case)
    kernels = [case.pop('kernel')] if 'kernel' in case else KERNELS
    for kernel in kernels:
        got = hoomd.sph_body_force(kernel=kernel, **case)
        assert same(got, loop_body_force(kernel=kernel, **case)), mutation
        assert not same(got, loop_body_force(kernel=kernel, **dict(case, **switch))), (mutation, kernel)


# ---------------------------------------------------------------- the physics
def _bound(extras, n, part, k, roundings):
    """The bound of recursive summation on one component of one part: (c + n + r) u times the sum of the terms' sizes --
    c additions in the longest candidate run, n in the sum over the targets (the tile tree adds fewer in a row) and r
    roundings in a term."""
    return (extras['longest'] + n + roundings) * U * extras['budget'][part][k]


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_force_on_the_body_is_minus_the_force_on_the_fluid(kernel):
    """A periodic cloud, no entry nowhere: the pair terms m_b m_f G S e and V_b V_f Gv K u are antisymmetric in exact
    arithmetic, so the two calls with the lists exchanged cancel per component to the two bounds of recursive summation
    and one more rounding.  A pressure term has four roundings (S * e, m_f *, G *, m_b *), a viscous one nine."""
    case = _small(81, 200, n_body=70)
    there, back = {}, {}
    want = loop_body_force(kernel=kernel, extras=there, **case)
    on_body = hoomd.sph_body_force(kernel=kernel, **case)
    exchanged = dict(case, body_rows=case['fluid_rows'], fluid_rows=case['body_rows'])
    on_fluid = hoomd.sph_body_force(kernel=kernel, **exchanged)
    assert same(on_body, want) and same(on_fluid, loop_body_force(kernel=kernel, extras=back, **exchanged))
    assert on_body.nowhere == on_fluid.nowhere == 0 and on_body.bad == on_fluid.bad == 0
    assert on_body.pairs == on_fluid.pairs > 0 and there['terms'] == back['terms']
    for part, (name, roundings) in enumerate((('force_pressure', 4), ('force_viscous', 9))):
        for k in range(3):
            a, b = getattr(on_body, name)[k], getattr(on_fluid, name)[k]
            bound = _bound(there, on_body.n, part, k, roundings) + _bound(back, on_fluid.n, part, k, roundings) + U * abs(a)
            print("reaction", kernel, name, k, "sum:", a + b, "bound:", bound, "force:", a)
            assert abs(a + b) <= bound
            # (and the bound has teeth: it lies far below the force itself, so a lost pair term would show)
            assert bound < 1e-9 * abs(a)


@pytest.mark.parametrize("dimensions", (3, 2))
@pytest.mark.parametrize("kernel", KERNELS)
def test_archimedes(kernel, dimensions):
    """The forces tests' lattice, unit mass and density, p = 20 - z (20 - y in 2-D); the body is the 4^3 block (4^2) at
    least 3 from every face, the fluid the rest.  The pressure force equals sum_b m_b pressure_acc_b of `sph_accelerations`
    over the union -- the body-body pairs cancel -- within the bounds of recursive summation; per body particle its axis
    component is the kernel's lattice constant, the weight of the displaced fluid; the other components and the torque
    about the block's centre vanish to rounding."""
    p, box, axis = lattice(dimensions)
    ones = np.ones(len(p))
    inside = np.all(np.abs(p[:, :dimensions]) <= 1.5, axis=1)
    body, fluid = np.flatnonzero(inside), np.flatnonzero(~inside)
    assert len(body) == 4 ** dimensions
    case = dict(position=p, velocity=None, box=box, h=1.5, mass=ones, density=ones, pressure=20.0 - p[:, axis],
                dimensions=dimensions, kernel=kernel, about=(0.0, 0.0, 0.25 if dimensions == 2 else 0.0))
    got = hoomd.sph_body_force(body_rows=body, fluid_rows=fluid, **case)
    from_fluid, from_body = {}, {}
    assert same(got, loop_body_force(body_rows=body, fluid_rows=fluid, extras=from_fluid, **case))
    loop_body_force(body_rows=body, fluid_rows=body, extras=from_body, **case)
    assert got.n == got.wetted == len(body) and got.nowhere == 0 and got.bad == 0 and got.n_sources == len(fluid)
    union = hoomd.sph_accelerations(p, None, box, 1.5, mass=ones, density=ones, pressure=20.0 - p[:, axis],
                                    dimensions=dimensions, kernel=kernel)
    mine = np.isin(union.rows, body)
    n = len(body)
    for k in range(3):
        total = 0.0
        for a in union.pressure_acc[mine, k]:
            total = total + 1.0 * a
        longest = from_fluid['longest'] + from_body['longest']
        bound = ((longest + n + 4) * U * (from_fluid['budget'][0][k] + from_body['budget'][0][k])
                 + _bound(from_fluid, n, 0, k, 4))
        print("archimedes", kernel, dimensions, k, "force:", got.force_pressure[k], "union:", total, "difference:",
              got.force_pressure[k] - total, "bound:", bound, "torque:", got.torque_pressure[k])
        assert abs(got.force_pressure[k] - total) <= bound
        if k == axis:
            assert abs(got.force_pressure[k] / n - LATTICE[kernel, dimensions]) < 2e-4
        else:
            # (symmetric pairs cancel: what is left is rounding, measured at 3e-14 and below -- DESIGN.md)
            assert abs(got.force_pressure[k]) <= _bound(from_fluid, n, 0, k, 4)
    # the torque about the block's centre: every arm is at most 1.5 sqrt(3) long, and the terms cancel by symmetry
    for k in range(3):
        others = [c for c in range(3) if c != k]
        assert abs(got.torque_pressure[k]) <= 3.0 * sum(_bound(from_fluid, n, 0, c, 6) for c in others)
    assert got.force_viscous == (0.0, 0.0, 0.0) and got.force == got.force_pressure
    assert abs(p[got.largest_row][axis]) == 1.5                           # the largest particle force: on a face of the block


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_couple_gives_arm_times_force(kernel):
    """Two targets at (-1, 0, 0) and (1, 0, 0), a source a quarter below the first and a quarter above the second: the
    forces are equal and opposite, all numbers exact in float32 -- the force vanishes and the torque is the arm, 2, times
    the force, about any point."""
    x = np.array([[-1, 0, 0], [1, 0, 0], [-1, -0.25, 0], [1, 0.25, 0]], np.float32)
    ones = np.ones(4, np.float32)
    got = hoomd.sph_body_force(x, None, CUBE, 0.25, [0, 1], [2, 3], density=ones, pressure=ones, kernel=kernel)
    assert got.n == got.wetted == 2 and got.pairs == 2 and got.bad == 0
    f = got.pressure_acc[list(got.rows).index(0), 1]
    assert f > 0 and bits_equal(got.pressure_acc[list(got.rows).index(1)], [0.0, -f, 0.0])
    assert got.force_pressure == (0.0, 0.0, 0.0) and got.torque_pressure == (0.0, 0.0, -(2.0 * f))
    assert got.largest2 == f * f and got.largest_at == 0
    moved = hoomd.sph_body_force(x, None, CUBE, 0.25, [0, 1], [2, 3], density=ones, pressure=ones, kernel=kernel,
                                 about=(0.5, 0.25, -0.125))
    assert moved.force_pressure == (0.0, 0.0, 0.0) and moved.torque_pressure == got.torque_pressure    # (exact numbers)
    # across the wrap: the body at x = 3.75 and -3.75 is half a unit wide, not seven and a half: the arms from -3.9375 are
    # -0.3125 (through the wrap) and 0.1875
    y = x.copy()
    y[:, 0] = [3.75, -3.75, 3.75, -3.75]
    wrapped = hoomd.sph_body_force(y, None, CUBE, 0.25, [0, 1], [2, 3], density=ones, pressure=ones, kernel=kernel,
                                   about=(-3.9375, 0, 0))
    assert wrapped.force_pressure == (0.0, 0.0, 0.0) and wrapped.torque_pressure == (0.0, 0.0, -(0.5 * f))


# ---------------------------------------------------------------- the summary
def test_the_summary_rules():
    """A NaN never is the largest force and neither is a bad target; the smaller position wins a tie; bad counts targets;
    no viscosity: six +0.0 words; nothing: the summary of nothing."""
    kw = case_arguments('mass_density')
    got = hoomd.sph_body_force(**dict(kw, **TERMS['viscous']))
    has = got.cell < np.prod(got.grid)
    m = kw['mass'][got.rows]
    fp = m[:, None] * got.pressure_acc
    fv = m[:, None] * got.viscous_acc
    finite = np.isfinite(fp).all(axis=1) & np.isfinite(fv).all(axis=1)
    assert got.bad >= int((has & ~finite).sum()) > 0 and got.summary[6] == got.bad
    norm2 = (fp[:, 0] * fp[:, 0] + fp[:, 1] * fp[:, 1]) + fp[:, 2] * fp[:, 2]
    assert finite[got.largest_at] and got.largest2 == norm2[got.largest_at] and got.largest_row == got.rows[got.largest_at]
    assert got.largest2 >= norm2[has & finite].max() * (1 - 1e-15)
    assert got.force == tuple(a + b for a, b in zip(got.force_pressure, got.force_viscous))
    assert got.torque == tuple(a + b for a, b in zip(got.torque_pressure, got.torque_viscous))
    # a tie: two pairs that are translates of one another give the same force: the smaller list position
    x = np.array([[-3, 0, 0], [-2.5, 0, 0], [3, 0, 0], [3.5, 0, 0]], np.float32)
    ones = np.ones(4, np.float32)
    two = hoomd.sph_body_force(x, None, CUBE, 0.5, [0, 2], [1, 3], density=ones, pressure=ones)
    assert two.largest_at == 0 and two.largest_row == two.rows[0] and two.largest2 > 0
    assert bits_equal(two.pressure_acc[0], two.pressure_acc[1])
    s = two.summary
    assert s[13:16].view(np.float64).tolist() == [0.0] * 3 and s[19:22].view(np.float64).tolist() == [0.0] * 3
    assert two.viscous_acc is None and two.force_viscous == (0.0, 0.0, 0.0)
    # no target: the summary of nothing (no source is looked at); no source: every target is dry
    nothing = hoomd.sph_body_force(**dict(kw, body_rows=np.arange(0)))
    s = nothing.summary
    assert [int(c) for c in s[:9]] == [0, 0, len(kw['fluid_rows']), 0, 0, 0, 0, NONE, NONE] and not s[9:].any()
    assert nothing.largest2 is None and nothing.pressure_acc.shape == (0, 3) and nothing.contacts.shape == (0,)
    dry = hoomd.sph_body_force(**dict(kw, fluid_rows=np.arange(0), **TERMS['viscous']))
    assert dry.n == len(kw['body_rows']) and dry.n_sources == 0 and dry.wetted == 0 and dry.pairs == 0
    assert not dry.summary[10:].any() and not dry.pressure_acc.any()
    # (a density of 0 or NaN is bad even when dry with a viscosity: 0/0; without one every dry target is good)
    assert hoomd.sph_body_force(**dict(kw, fluid_rows=np.arange(0))).bad == 0
    with pytest.raises(ValueError, match="22 words"):
        hoomd.KernelBodyForce(0.5, 'wendland_c2', (1, 1, 1), 3, np.zeros(12, np.uint64))


# ---------------------------------------------------------------- frames, h=None, the command line
def test_h_none_takes_a_uniform_slength_and_refuses_another():
    fr = small_frame(slength=[0.5] * 6)
    body, fluid = {'type': ['wall']}, {'type': ['fluid']}
    got = hoomd.frame_body_force(fr, body, fluid, viscosity=0.25, about=(1, 1, 1))
    want = hoomd.sph_body_force(fr.particles.position, fr.particles.velocity, fr.configuration.box, 0.5, [2], [0, 1, 3, 4, 5],
                                mass=fr.particles.mass, density=fr.particles.density, pressure=fr.particles.pressure,
                                viscosity=0.25, about=(1, 1, 1))
    assert got.h == 0.5 and np.array_equal(got.summary, want.summary) and bits_equal(got.pressure_acc.ravel(), want.pressure_acc.ravel())
    assert got.n == 1 and got.n_sources == 5 and got.sources_nowhere == 1 and got.wetted == 1 and got.pairs == 2
    assert any(got.force) and any(got.torque) and got.largest_row == 2
    assert hoomd.frame_body_force(small_frame(), body, fluid).h == 1.0               # stored nowhere: the schema default
    assert hoomd.frame_body_force(small_frame(slength=[0.5] * 6), body, fluid, h=0.75).h == 0.75
    with pytest.raises(ValueError, match="slength ranges from 0.5 to 0.75"):
        hoomd.frame_body_force(small_frame(slength=[0.5, 0.5, 0.75, 0.5, 0.5, 0.5]), body, fluid)
    # a domain cuts both selections
    cut = hoomd.frame_body_force(fr, body, fluid, domain=hoomd.Domain((0.5, 0.5, 0.5), (1, 1, 1)))
    assert cut.n == 1 and cut.n_sources == 3 and np.array_equal(cut.summary[4:7], got.summary[4:7])
    arrays = dict(position=fr.particles.position, density=fr.particles.density, pressure=fr.particles.pressure,
                  mass=fr.particles.mass, typeid=fr.particles.typeid)
    plain = hoomd.frame_body_force(arrays, body, fluid, h=0.5, box=fr.configuration.box, types=['fluid', 'wall'])
    assert plain.viscous_acc is None and bits_equal(plain.pressure_acc.ravel(), got.pressure_acc.ravel())
    for missing in ((None, fluid), (body, None)):
        with pytest.raises(ValueError, match="body and fluid are where dicts: both are required"):
            hoomd.frame_body_force(fr, *missing)


def test_what_sph_body_force_refuses():
    p = random_rows(1, 10, ORTHO)
    w = velocities(1, 10).astype(np.float32)
    b, f = [0, 1, 2], [3, 4, 5, 6]
    for h in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match="finite and positive"):
            hoomd.sph_body_force(p, w, ORTHO, h, b, f)
    with pytest.raises(ValueError, match="kernel is one of"):
        hoomd.sph_body_force(p, w, ORTHO, 0.5, b, f, kernel='gaussian')
    with pytest.raises(ValueError, match="narrower"):
        hoomd.sph_body_force(p, w, ORTHO, 0.65, b, f, cells=(8, 6, 4))
    with pytest.raises(ValueError, match="narrower"):
        hoomd.sph_body_force(p, w, TRICLINIC, 0.65, b, f, cells=hoomd.cell_grid_for(ORTHO, 1.3))
    with pytest.raises(ValueError, match="2\\^20"):
        hoomd.sph_body_force(p, w, [1000, 800, 600, 0, 0, 0], 0.5, b, f, cells=(1000, 800, 600))
    with pytest.raises(ValueError, match="count twice"):
        hoomd.sph_body_force(p, w, ORTHO, 1.6, b, f)
    with pytest.raises(ValueError, match="cz == 1"):
        hoomd.sph_body_force(p, w, FLAT, 0.3, b, f, cells=(2, 2, 2), dimensions=2)
    with pytest.raises(ValueError, match="float32 or float64"):
        hoomd.sph_body_force(p.astype(np.int32), w, ORTHO, 0.5, b, f)
    with pytest.raises(ValueError, match="mass holds one float32 or float64 value per row"):
        hoomd.sph_body_force(p, w, ORTHO, 0.5, b, f, mass=np.ones(9))
    with pytest.raises(ValueError, match="density holds one float32 or float64 value per row"):
        hoomd.sph_body_force(p, w, ORTHO, 0.5, b, f, density=np.ones(10, np.int32))
    with pytest.raises(ValueError, match="pressure holds one float32 or float64 value per row"):
        hoomd.sph_body_force(p, w, ORTHO, 0.5, b, f, pressure=np.ones(11))
    with pytest.raises(ValueError, match="velocity holds three float32 or float64 values per row"):
        hoomd.sph_body_force(p, w[:9], ORTHO, 0.5, b, f)
    for mu in (-0.5, float('inf'), float('nan')):
        with pytest.raises(ValueError, match="viscosity is a finite number, at least 0, or None"):
            hoomd.sph_body_force(p, w, ORTHO, 0.5, b, f, viscosity=mu)
    for c in ((0, 0), (0, 0, float('nan')), (float('inf'), 0, 0), (0, 0, 0, 0)):
        with pytest.raises(ValueError, match="about holds three finite numbers, or is None"):
            hoomd.sph_body_force(p, w, ORTHO, 0.5, b, f, about=c)
    for lists in ((None, f), (b, None)):
        with pytest.raises(ValueError, match="body_rows and fluid_rows are row lists: None is not accepted for either"):
            hoomd.sph_body_force(p, w, ORTHO, 0.5, *lists)
    for lists in (([0, 10], f), (b, [-1])):
        with pytest.raises(ValueError, match="an entry of the row list lies outside the position array"):
            hoomd.sph_body_force(p, w, ORTHO, 0.5, *lists)
    with pytest.raises(ValueError, match="needs the box"):
        hoomd.frame_body_force(dict(position=p), {'type': [0]}, {'type': [1]}, h=0.5)


def test_the_command_line_prints_the_body_force(tmp_path, capsys):
    path = str(tmp_path / "small.gsd")
    with hoomd.open(path, 'w') as t:
        t.append(small_frame(slength=[0.5] * 6))
    with hoomd.open(path, 'r') as t:
        want = hoomd.frame_body_force(t[0], {'type': ['wall']}, {'type': ['fluid']})
        spline = t.frame_body_force(0, {'type': ['wall']}, {'type': ['fluid']}, 0.75, kernel='cubic_spline', viscosity=0.25,
                                    about=(1, 1.25, 1))
    assert pgsd_main(['info', path, '--body-force', 'wall', '--fluid', 'fluid']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "SPH body force of frame 0 with h = 0.5 (wendland_c2) over 8 x 8 x 8 cells (body wall, fluid fluid):" in lines
    assert "targets: 1 nowhere: 0 wetted: 1 bad: 0" in lines and "sources: 5 nowhere: 1 pairs: 2" in lines
    assert "viscosity: none about: 0.0 0.0 0.0" in lines
    assert "force: %r %r %r" % want.force in lines and "torque: %r %r %r" % want.torque in lines
    assert "pressure: %r %r %r" % want.force_pressure in lines and "pressure: %r %r %r" % want.torque_pressure in lines
    assert "viscous: 0.0 0.0 0.0" in lines
    assert "largest: %r at row 2 (the pressure force on one particle)" % (want.largest2 ** 0.5) in lines
    assert not any(l.startswith("SPH accelerations") for l in lines)
    assert pgsd_main(['info', path, '--body-force', 'wall', '--fluid', 'fluid', '0.75', '--kernel', 'cubic_spline', '--viscosity',
                      '0.25', '--about', '1,1.25,1']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "SPH body force of frame 0 with h = 0.75 (cubic_spline) over 5 x 5 x 5 cells (body wall, fluid fluid):" in lines
    assert "viscosity: 0.25 about: 1.0 1.25 1.0" in lines
    assert "force: %r %r %r" % spline.force in lines and "viscous: %r %r %r" % spline.force_viscous in lines
    assert "torque: %r %r %r" % spline.torque in lines and "viscous: %r %r %r" % spline.torque_viscous in lines
    assert pgsd_main(['info', path, '--body-force', 'wall']) == 1
    assert "go together" in capsys.readouterr().err
    assert pgsd_main(['info', path, '--body-force', 'wall', '--fluid', 'fluid', '2.5']) == 1
    assert "count twice" in capsys.readouterr().err
    assert pgsd_main(['info', path, '--body-force', 'wall', '--fluid', 'fluid', '--about', '0,1']) == 1
    assert "about holds three finite numbers" in capsys.readouterr().err
    assert pgsd_main(['info', path, '--body-force', 'wall', '--fluid', 'fluid', '0.5', '0.5']) == 1
    assert "--fluid takes TYPE[,TYPE...] [H]" in capsys.readouterr().err
