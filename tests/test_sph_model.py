"""The numpy model of the SPH kernel sums (pgsd.hoomd.sph_kernel_sums / frame_kernel_sums), the definition the GPU pass
equals exactly (tests/test_gpu_sph_sums.py): it equals a plain double loop bit for bit -- so its numpy.add.at is the
sequential sum --, every mutation of the loop differs from it on the case that names it, its normalisation is the
physical one, and the command line prints it.  No GPU."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

from neighbours_cases import FLAT, ORTHO, TRICLINIC, random_rows
from sph_cases import CASES, CUBE, EQUIVALENT, KERNELS, LOOP_ENTRIES, MUTATIONS, NONE, bits_equal, loop_sums, same


def model_kw(case):
    p, mass, density, kw = case
    return dict(kw, position=p, mass=mass, density=density)


# ---------------------------------------------------------------- the model is the loop
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_equals_the_double_loop_bit_for_bit(name, kernel):
    kw = model_kw(CASES[name])
    n = len(kw['position'])
    # (the loop is quadratic in a crowded cell: beyond LOOP_ENTRIES entries it takes a strided sub-list of the case)
    rows = None if n <= LOOP_ENTRIES else np.arange(0, n, -(-n // LOOP_ENTRIES))
    for dtype in (np.float64, np.float32):
        kw['position'] = CASES[name][0].astype(dtype)
        got = hoomd.sph_kernel_sums(rows=rows, kernel=kernel, **kw)
        assert same(got, loop_sums(rows=rows, kernel=kernel, **kw)), (name, kernel, dtype)
    assert got.n == (n if rows is None else len(rows))
    if name == 'all_nowhere':
        assert got.nowhere == got.n and got.density_min == np.inf and got.density_max == -np.inf and got.deviation is None
        assert not got.number.any() and not np.signbit(got.number).any()


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_list_in_any_order_with_repeats(kernel):
    p, mass, density, kw = CASES['three_cells']
    rows = np.concatenate([np.arange(300, 0, -1), [7, 7, 300, 12]])
    got = hoomd.sph_kernel_sums(p, mass=mass, density=density, rows=rows, kernel=kernel, **kw)
    assert same(got, loop_sums(p, mass=mass, density=density, rows=rows, kernel=kernel, **kw)) and got.n == 304


def test_the_boundary_case_by_hand():
    """A pair at exactly 2h is not counted (its partner's infinite volume would show), a row stored twice counts itself
    and its twin with w = 1, and the spline gives 0.25 at q = 1 from either branch."""
    p, mass, density, kw = CASES['boundary']
    for kernel in KERNELS:
        got = hoomd.sph_kernel_sums(p, mass=mass, density=density, kernel=kernel, **kw)
        at = dict((int(r), k) for k, r in enumerate(got.rows))
        sigma = hoomd.sph_sigma(kernel, 0.25)
        assert got.number[at[0]] == sigma * 1.0 and got.shepard[at[0]] == sigma * 1.0 and got.shepard[at[1]] == np.inf
        assert got.number[at[2]] == got.number[at[3]] == sigma * 2.0
        assert got.shepard_max == np.inf and got.not_finite == 0
    assert hoomd.sph_weight(1.0, 'cubic_spline') == 0.25 and hoomd.sph_weight(0.0, 'cubic_spline') == 1.0
    assert hoomd.sph_weight(0.0, 'wendland_c2') == 1.0 and hoomd.sph_weight(2.0, 'wendland_c2') == 0.0
    assert got.number[at[4]] == sigma * 1.25
    assert got.number[at[6]] != got.number[at[4]] and got.number[at[8]] != got.number[at[4]]      # an ulp either side


# ---------------------------------------------------------------- the mutations
@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_every_mutation_differs_on_its_case(mutation):
    switch, case = MUTATIONS[mutation]
    case = dict(case)
    kernels = [case.pop('kernel')] if 'kernel' in case else KERNELS
    differs = False
    for kernel in kernels:
        got = hoomd.sph_kernel_sums(kernel=kernel, **case)
        assert same(got, loop_sums(kernel=kernel, **case)), mutation
        differs = differs or not same(got, loop_sums(kernel=kernel, **dict(case, **switch)))
    assert differs, mutation


def test_the_mutation_no_input_can_show():
    """`q <= 1` for `q < 1` in the cubic spline: both branches give 0.25 exactly at q == 1."""
    for mutation, (switch, case) in EQUIVALENT.items():
        got = hoomd.sph_kernel_sums(**case)
        assert same(got, loop_sums(**case)) and same(got, loop_sums(**dict(case, **switch))), mutation


# ---------------------------------------------------------------- the normalisation
LATTICE = {('wendland_c2', 3): 1.00314, ('wendland_c2', 2): 1.00514, ('cubic_spline', 3): 1.00179, ('cubic_spline', 2): 1.00344}
BOUND = 2 * (max(LATTICE.values()) - 1)            # twice the kernels' own lattice error: 1.03 %


@pytest.mark.parametrize("dimensions", [3, 2])
@pytest.mark.parametrize("kernel", KERNELS)
def test_sigma_on_a_periodic_lattice(kernel, dimensions):
    """A periodic cubic lattice of spacing 1 with unit masses and h = 1.5 has density 1: every entry's summation density
    lies within 1 % of it (the values of LATTICE, computed with numpy), so a wrong constant fails and the kernels' own
    lattice error does not."""
    g = np.arange(12) - 5.5
    if dimensions == 3:
        p = np.array([(x, y, z) for z in g for y in g for x in g], np.float64)
    else:
        p = np.array([(x, y, 0.25) for y in g for x in g], np.float64)
    box = [12, 12, 12 if dimensions == 3 else 1, 0, 0, 0]
    got = hoomd.sph_kernel_sums(p, box, 1.5, density=np.ones(len(p)), dimensions=dimensions, kernel=kernel, surface_below=0.9)
    assert BOUND < 0.0103 and got.n == len(p) and got.nowhere == 0 and got.not_finite == 0
    assert np.all(np.abs(got.density - 1.0) < 0.01) and np.all(np.abs(got.density - 1.0) < BOUND)
    assert abs(got.density_max - LATTICE[kernel, dimensions]) < 1e-5
    # density == 1 and mass == 1: the volume is 1, so shepard is number times it, and the deviation is density - 1
    assert np.all(np.abs(got.shepard - got.number * 1.0) < BOUND) and bits_equal(got.shepard, got.number)
    dev = got.density - 1.0
    k = int(np.argmax(np.abs(dev)))
    assert got.deviation == dev[k] and got.deviation_at == k and got.deviation_row == got.rows[k]
    assert got.surface == 0 and got.shepard_min == got.number_min and got.shepard_max == got.number_max
    assert got.sigma == hoomd.sph_sigma(kernel, 1.5, dimensions)


def test_sigma_by_hand():
    assert hoomd.sph_sigma('wendland_c2', 2.0) == 21.0 / (16.0 * np.pi * 8.0)
    assert hoomd.sph_sigma('wendland_c2', 2.0, 2) == 7.0 / (4.0 * np.pi * 4.0)
    assert hoomd.sph_sigma('cubic_spline', 2.0) == 1.0 / (np.pi * 8.0)
    assert hoomd.sph_sigma('cubic_spline', 2.0, 2) == 10.0 / (7.0 * np.pi * 4.0)


def test_the_summary_rules():
    """A NaN never replaces a bound and never wins the deviation; the smaller position wins a tie; surface is strict."""
    p, mass, density, kw = CASES['mass_density']
    got = hoomd.sph_kernel_sums(p, mass=mass, density=density, **kw)
    finite = np.isfinite(got.shepard)
    assert (~finite).any() and got.shepard_min == got.shepard[got.shepard == got.shepard].min()
    assert got.shepard_max == np.inf and got.not_finite == 0
    assert got.surface == int((got.shepard < 0.5).sum()) and 0 < got.surface < got.n
    dev = got.density - density[got.rows]
    assert np.isnan(dev).any() and got.deviation == dev[got.deviation_at] and abs(got.deviation) == np.nanmax(np.abs(dev))
    # a tie: two far rows with the same density, the same deviation: the smaller list position
    two = hoomd.sph_kernel_sums(np.array([[3, 0, 0], [-3, 0, 0]], np.float32), CUBE, 0.5, density=np.array([2, 2], np.float32))
    assert two.deviation_at == 0 and two.deviation == two.density[0] - 2.0 and two.density[0] == two.density[1]
    # without a density: no volume outputs
    none = hoomd.sph_kernel_sums(p, mass=mass, **kw)
    assert none.shepard is None and none.shepard_min is None and none.deviation is None and none.deviation_at is None
    assert none.surface is None and not none.volume and bits_equal(none.density, got.density)
    assert int(none.summary[4]) == NONE


# ---------------------------------------------------------------- frames, h=None, the command line
def small_frame(slength=None, density=True):
    fr = hoomd.Frame()
    fr.configuration.box = [8, 8, 8, 0, 0, 0]
    fr.particles.N = 6
    fr.particles.types = ['fluid', 'wall']
    fr.particles.typeid = np.array([0, 0, 1, 0, 0, 0], np.uint32)
    fr.particles.position = np.array([[1, 1, 1], [1.5, 1, 1], [1, 1.25, 1], [-3.9, 0, 0], [3.9, 0, 0], [np.nan, 0, 0]], np.float32)
    fr.particles.mass = np.array([1, 2, 1, 1, 1, 1], np.float32)
    if density:
        fr.particles.density = np.array([1, 1, 1, 0.5, 0.5, 1], np.float32)
    if slength is not None:
        fr.particles.slength = np.asarray(slength, np.float32)
    return fr


def test_h_none_takes_a_uniform_slength_and_refuses_another():
    fr = small_frame(slength=[0.5] * 6)
    got = hoomd.frame_kernel_sums(fr)
    want = hoomd.sph_kernel_sums(fr.particles.position, fr.configuration.box, 0.5, mass=fr.particles.mass,
                                 density=fr.particles.density)
    assert got.h == 0.5 and np.array_equal(got.summary, want.summary) and bits_equal(got.density, want.density)
    assert hoomd.frame_kernel_sums(small_frame()).h == 1.0                         # stored nowhere: the schema default
    assert hoomd.frame_kernel_sums(small_frame(slength=[0.5] * 6), h=0.75).h == 0.75
    with pytest.raises(ValueError, match="slength ranges from 0.5 to 0.75"):
        hoomd.frame_kernel_sums(small_frame(slength=[0.5, 0.5, 0.75, 0.5, 0.5, 0.5]))
    with pytest.raises(ValueError, match="slength ranges"):
        hoomd.frame_kernel_sums(small_frame(slength=[np.nan] * 6))
    # the selection is the list: both i and j come from it
    fluid = hoomd.frame_kernel_sums(fr, where={'type': ['fluid']})
    assert fluid.n == 5 and fluid.number_max < got.number_max
    arrays = dict(position=fr.particles.position, mass=fr.particles.mass)
    assert hoomd.frame_kernel_sums(arrays, h=0.5, box=fr.configuration.box).shepard is None


def test_what_sph_kernel_sums_refuses():
    p = random_rows(1, 10, ORTHO)
    for h in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match="finite and positive"):
            hoomd.sph_kernel_sums(p, ORTHO, h)
        with pytest.raises(ValueError, match="finite and positive"):
            hoomd.sph_sigma('wendland_c2', h)
    with pytest.raises(ValueError, match="kernel is one of"):
        hoomd.sph_kernel_sums(p, ORTHO, 0.5, kernel='gaussian')
    with pytest.raises(ValueError, match="narrower"):
        hoomd.sph_kernel_sums(p, ORTHO, 0.65, cells=(8, 6, 4))
    with pytest.raises(ValueError, match="narrower"):
        hoomd.sph_kernel_sums(p, TRICLINIC, 0.65, cells=hoomd.cell_grid_for(ORTHO, 1.3))  # the tilt narrows x
    with pytest.raises(ValueError, match="2\\^20"):
        hoomd.sph_kernel_sums(p, [1000, 800, 600, 0, 0, 0], 0.5, cells=(1000, 800, 600))
    with pytest.raises(ValueError, match="count twice"):
        hoomd.sph_kernel_sums(p, ORTHO, 1.6)                                         # 2h = 3.2 > Lz / 2
    with pytest.raises(ValueError, match="cz == 1"):
        hoomd.sph_kernel_sums(p, FLAT, 0.3, cells=(2, 2, 2), dimensions=2)
    with pytest.raises(ValueError, match="float32 or float64"):
        hoomd.sph_kernel_sums(p.astype(np.int32), ORTHO, 0.5)
    with pytest.raises(ValueError, match="mass holds one float32 or float64 value per row"):
        hoomd.sph_kernel_sums(p, ORTHO, 0.5, mass=np.ones(9))
    with pytest.raises(ValueError, match="density holds one float32 or float64 value per row"):
        hoomd.sph_kernel_sums(p, ORTHO, 0.5, density=np.ones(10, np.int32))
    with pytest.raises(ValueError, match="surface_below"):
        hoomd.sph_kernel_sums(p, ORTHO, 0.5, surface_below=float('nan'))
    with pytest.raises(ValueError, match="needs the box"):
        hoomd.frame_kernel_sums(dict(position=p), h=0.5)


def test_the_command_line_prints_the_sums(tmp_path, capsys):
    path = str(tmp_path / "small.gsd")
    with hoomd.open(path, 'w') as t:
        t.append(small_frame(slength=[0.5] * 6))
    with hoomd.open(path, 'r') as t:
        want = hoomd.frame_kernel_sums(t[0], surface_below=7.0)
        spline = t.frame_kernel_sums(0, 0.75, kernel='cubic_spline', where={'type': ['fluid']})
    assert pgsd_main(['info', path, '--sph', '--surface', '7']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "SPH sums of frame 0 with h = 0.5 (wendland_c2) over 8 x 8 x 8 cells:" in lines
    assert "entries: 6 nowhere: 1" in lines
    assert "density: smallest %r largest %r not finite: 0" % (want.density_min, want.density_max) in lines
    assert "deviation: %r from the stored density at row %d" % (want.deviation, want.deviation_row) in lines
    assert "shepard: smallest %r largest %r" % (want.shepard_min, want.shepard_max) in lines
    assert "surface: 2 entries below 7.0" in lines and want.surface == 2
    assert pgsd_main(['info', path, '--sph', '0.75', '--kernel', 'cubic_spline', '--types', 'fluid']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "SPH sums of frame 0 with h = 0.75 (cubic_spline) over 5 x 5 x 5 cells (types fluid):" in lines
    assert "entries: 5 nowhere: 1" in lines
    assert "density: smallest %r largest %r not finite: 0" % (spline.density_min, spline.density_max) in lines
    assert not any(l.startswith("surface:") for l in lines)
    assert pgsd_main(['info', path, '--sph', '2.5']) == 1
    assert "count twice" in capsys.readouterr().err
