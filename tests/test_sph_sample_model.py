"""The numpy model of the SPH samples (pgsd.hoomd.sph_samples / frame_samples / sample_grid), the definition the GPU pass
equals exactly (tests/test_gpu_sph_samples.py): it equals a plain double loop bit for bit -- so its numpy.add.at is the
sequential sum --, every mutation of the loop differs from it on the case that names it, at the particles' own positions
it is the SPH kernel sums and the neighbour census, a constant and a linear field on a lattice come back to rounding, and
the command line prints it.  No GPU."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

from neighbours_cases import FLAT, ORTHO, TRICLINIC, random_rows
from sph_cases import CASES as SUM_CASES, CUBE, KERNELS, NONE, bits_equal
from sph_sample_cases import (CASES, EQUIVALENT, LOOP_POINTS, MUTATIONS, WIDTHS, _small, loop_samples, same, special_points,
                              value_arrays, words_equal)


def _strided(points):
    """(the loop is quadratic in a crowded cell: beyond LOOP_POINTS points it takes a strided subset of the case's)"""
    K = len(points)
    return points if K <= LOOP_POINTS else np.concatenate([points[:-4:-(-K // LOOP_POINTS)], points[-4:]])   # (the special ones stay)


# ---------------------------------------------------------------- the model is the loop
@pytest.mark.parametrize("normalise", (False, True))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_equals_the_double_loop_bit_for_bit(name, kernel, normalise):
    kw = dict(CASES[name], kernel=kernel, normalise=normalise)
    kw['points'] = _strided(kw['points'])
    for dtype in (np.float64, np.float32):
        args = dict(kw, position=kw['position'].astype(dtype), values=[v.astype(dtype) for v in kw['values']],
                    points=kw['points'].astype(dtype))
        got = hoomd.sph_samples(**args)
        assert same(got, loop_samples(**args)), (name, kernel, dtype)
    K, C = len(kw['points']), sum(v.shape[1] for v in kw['values'])
    assert got.points == K and got.values.shape == (K, C) and got.count.shape == (K,) and got.normalise == normalise
    assert got.columns == tuple(v.shape[1] for v in kw['values']) and got.sigma == hoomd.sph_sigma(kernel, kw['h'], got.dimensions)
    for k, width in enumerate(got.columns):
        assert got.field(k).shape == (K, width) and np.shares_memory(got.field(k), got.values)
    if name not in ('lone',):
        # the special points: two nowhere (+0.0 whatever normalise says), two outside the box
        assert got.nowhere >= 2 and got.outside >= 2 and not got.count[-4:-2].any()
        for a in (got.density[-4:-2], got.shepard[-4:-2], got.values[-4:-2]):
            assert not a.any() and not np.signbit(a).any()
    if name == 'all_nowhere':
        assert got.empty == K - got.nowhere and got.count_max == 0 and got.count_max_at is not None and not got.count.any()
        assert np.isnan(got.values[got.count_max_at]).all() == normalise      # an empty point: 0/0 under normalise
    if name == 'lone':
        # exactly 2h away: not counted; coinciding: w = 1; the last point is out of reach
        assert got.count.tolist() == [0, 1, 1, 0] and got.empty == 2 and got.count_max_at == 1
        assert got.shepard[1] == got.sigma * 0.5 and (got.values[1, 0] == 2.0 if normalise else got.values[1, 0] == got.sigma * 1.0)
        assert np.isnan(got.values[0, 0]) == normalise and got.not_finite == (2 if normalise else 0)
    if name in ('one_cell_65', 'mass_only', 'no_density'):
        assert got.shepard_max == np.inf and got.not_finite > 0          # the density is the default 0.0: every V is infinite
    if name == 'flat':
        assert got.dimensions == 2 and got.grid[2] == 1
    if name == 'no_values':
        assert got.values.shape == (K, 0) and got.columns == ()


@pytest.mark.parametrize("C", sorted(WIDTHS))
def test_every_number_of_columns(C):
    kw = dict(_small(50 + C), values=value_arrays(50 + C, 60, C))
    for normalise in (False, True):
        got = hoomd.sph_samples(normalise=normalise, **kw)
        assert same(got, loop_samples(normalise=normalise, **kw)) and got.values.shape == (40, C) and got.columns == WIDTHS[C]
    # a one-column value may be given flat
    if C == 1:
        flat = hoomd.sph_samples(**dict(kw, values=[kw['values'][0].reshape(-1)]))
        assert bits_equal(flat.values.ravel(), hoomd.sph_samples(**kw).values.ravel())


# ---------------------------------------------------------------- mutations
@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_every_mutation_differs_on_its_case(mutation):
    switch, kw = MUTATIONS[mutation]
    got = hoomd.sph_samples(**kw)
    assert same(got, loop_samples(**kw)), mutation
    assert not same(got, loop_samples(**kw, **switch)), mutation


@pytest.mark.parametrize("mutation", sorted(EQUIVALENT))
def test_mutations_no_input_can_show(mutation):
    switch, kw = EQUIVALENT[mutation]
    for normalise in (False, True):
        got = hoomd.sph_samples(normalise=normalise, **kw)
        assert same(got, loop_samples(normalise=normalise, **kw)) and same(got, loop_samples(normalise=normalise, **kw, **switch))
    assert len(MUTATIONS) == 13 and len(EQUIVALENT) == 1


# ---------------------------------------------------------------- the sums and the census at the particles' own positions
@pytest.mark.parametrize("name", ['three_cells', 'triclinic_754', 'flat', 'mass_density', 'boundary', 'all_nowhere'])
def test_at_the_entries_positions_the_samples_are_the_kernel_sums(name):
    p, mass, density, kw = SUM_CASES[name]
    kw = dict((k, v) for k, v in kw.items() if k != 'surface_below')
    rows = np.arange(0, len(p), 4) if len(p) > 2000 else None           # (a sub-list of the largest case)
    for kernel in KERNELS:
        sums = hoomd.sph_kernel_sums(p, mass=mass, density=density, kernel=kernel, rows=rows, **kw)
        got = hoomd.sph_samples(p[sums.rows], p, mass=mass, density=density, kernel=kernel, cells=sums.grid, rows=rows,
                                **dict((k, v) for k, v in kw.items() if k != 'cells'))
        assert got.grid == sums.grid and bits_equal(got.density, sums.density) and bits_equal(got.shepard, sums.shepard)
    census = hoomd.particle_neighbours(p, kw['box'], 2.0 * kw['h'], rows=rows, cells=sums.grid, dimensions=kw.get('dimensions', 3))
    assert np.array_equal(census.rows, sums.rows)
    has = sums.cell < sums.grid[0] * sums.grid[1] * sums.grid[2]
    assert np.array_equal(got.count[has], census.count[has] + 1) and not got.count[~has].any()
    assert got.nowhere == sums.nowhere == int((~has).sum()) and got.empty == 0


# ---------------------------------------------------------------- physics
LATTICE_BOX = [24, 24, 24, 0, 0, 0]


def lattice():
    """12^3 sites, spacing 1, centred in a box of edge 24."""
    a = np.arange(12, dtype=np.float64) - 5.5
    z, y, x = np.meshgrid(a, a, a, indexing='ij')
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_constant_field_comes_back(kernel):
    """Unit mass and density, h = 1.5: at random interior points the normalised value of a constant field c is c within
    (count + 2) * 2^-53 * |c|, the bound of a recursive sum of count terms and one division."""
    p = lattice()
    points = np.random.default_rng(5).uniform(-2.5, 2.5, size=(300, 3))
    for c in (2.0, 1.7, -1234.56789):
        got = hoomd.sph_samples(points, p, LATTICE_BOX, 1.5, values=[np.full((len(p), 1), c)], mass=np.ones(len(p)),
                                density=np.ones(len(p)), kernel=kernel, normalise=True)
        assert got.count.min() > 50 and got.empty == 0 and got.not_finite == 0 and got.outside == 0
        error = np.abs(got.values[:, 0] - c)
        print("constant", kernel, c, "largest error / bound:", float((error / ((got.count + 2) * 2.0 ** -53 * abs(c))).max()))
        assert (error <= (got.count + 2) * 2.0 ** -53 * abs(c)).all()
        assert abs(got.shepard - 1.0).max() < 0.02                        # the lattice is a partition of unity to a per cent


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_linear_field_comes_back_at_sites_and_cell_centres(kernel):
    """At lattice sites and cell centres at least 3 from every face the neighbourhood is symmetric, so the normalised value
    of a + b.x is a + b.x_p within (count + 2) * 2^-53 * (sum |vw f| / sum vw), the same kind of bound with the loop's
    budget."""
    p = lattice()
    a, b = 0.75, np.array([0.5, -1.25, 2.0])
    f = (a + p @ b).reshape(-1, 1)
    sites = np.arange(6, dtype=np.float64) - 2.5
    centres = np.arange(5, dtype=np.float64) - 2.0
    points = np.concatenate([np.stack(np.meshgrid(s, s, s, indexing='ij'), axis=-1).reshape(-1, 3) for s in (sites, centres)])
    kw = dict(points=points, position=p, box=LATTICE_BOX, h=1.5, values=[f], mass=np.ones(len(p)), density=np.ones(len(p)),
              kernel=kernel, normalise=True)
    got, extras = hoomd.sph_samples(**kw), {}
    assert same(got, loop_samples(extras=extras, **kw))
    budget = np.array([c[0] for c in extras['budget']]) / np.array(extras['weight'])
    error, bound = np.abs(got.values[:, 0] - (a + points @ b)), (got.count + 2) * 2.0 ** -53 * budget
    print("linear", kernel, "largest error / bound:", float((error / bound).max()))
    assert (error <= bound).all() and got.count.min() > 50


# ---------------------------------------------------------------- the summary, the grid
def test_the_summary_rules():
    kw = dict(_small(7, K=5), points=np.concatenate([special_points(CUBE), [[0.0, 0.0, 0.0], [3.99, 3.99, 3.99]]]))
    got = hoomd.sph_samples(**kw)
    assert (got.points, got.nowhere, got.outside) == (6, 2, 2)
    assert got.empty == int((got.count[2:] == 0).sum()) and got.count_max == got.count[2:].max()
    assert got.count_max_at == 2 + int(np.argmax(got.count[2:])) and got.shepard_min == got.shepard[2:].min()
    assert got.density_max == got.density[2:].max() and got.summary.dtype == np.uint64 and got.summary.shape == (11,)
    # a NaN replaces neither bound and counts as not finite; a tie goes to the smaller index
    nan = hoomd.sph_samples(**dict(kw, points=kw['position'][:6], density=np.where(np.arange(60) == 3, np.nan, kw['density'])))
    assert nan.not_finite > 0 and np.isnan(nan.shepard[3]) and nan.shepard_max < np.inf and nan.shepard_min > 0
    twice = hoomd.sph_samples(**dict(kw, points=np.array([[0.5, 0.5, 0.5]] * 3)))
    assert twice.count_max_at == 0 and twice.count[0] == twice.count[2] == twice.count_max
    # no point, no entry
    none = hoomd.sph_samples(**dict(kw, points=np.zeros((0, 3))))
    assert [int(w) for w in none.summary[:7]] == [0, 0, 0, 0, 0, 0, NONE] and none.count_max_at is None
    assert none.summary[7:].view(np.float64).tolist() == [np.inf, -np.inf, np.inf, -np.inf] and none.values.shape == (0, 4)
    empty = hoomd.sph_samples(kw['points'], np.zeros((0, 3), np.float32), CUBE, 1.0)
    assert (empty.points, empty.nowhere, empty.empty, empty.count_max, empty.count_max_at) == (6, 2, 4, 0, 2)
    assert words_equal(empty.summary, loop_samples(kw['points'], np.zeros((0, 3), np.float32), CUBE, 1.0)[0])
    with pytest.raises(ValueError, match="11 words"):
        hoomd.KernelSamples(0.5, 'wendland_c2', (1, 1, 1), 3, np.zeros(12, np.uint64))
    with pytest.raises(ValueError, match="no array 4"):
        got.field(4)


@pytest.mark.parametrize("box,dims,shape", [(TRICLINIC, 3, (7, 5, 4)), (CUBE, 3, (1, 1, 1)), (ORTHO, 3, (3, 16, 2)),
                                            (FLAT, 2, (11, 9, 1)), (TRICLINIC, 3, (64, 3, 5))])
def test_sample_grid_round_trip(box, dims, shape):
    """The points of a lattice are the centres of the cells of the same grid, in the grid's order."""
    points = hoomd.sample_grid(box, shape, dims)
    n = shape[0] * shape[1] * shape[2]
    assert points.shape == (n, 3) and points.dtype == np.float64
    assert np.array_equal(hoomd.cell_ids(points, box, shape, dims), np.arange(n))
    if dims == 2:
        assert not points[:, 2].any()
    # a sub-box: the same points as the cells of the finer grid it is a part of
    lo, hi = (0.5, 0.0, 0.0), (1.0, 1.0, 1.0)
    half = hoomd.sample_grid(box, shape, dims, lo=lo, hi=hi)
    ids = hoomd.cell_ids(half, box, (2 * shape[0], shape[1], shape[2]), dims)
    ix = ids % (2 * shape[0])
    assert (ix >= shape[0]).all() and np.array_equal(np.unique(ids), np.sort(ids))
    got = hoomd.sph_samples(points, random_rows(3, 50, box, np.float32, dims), box, 0.3, dimensions=dims)
    assert got.as_grid('count', shape).shape == (shape[2], shape[1], shape[0]) and got.outside == 0 and got.nowhere == 0
    assert got.as_grid('count', shape)[0, 0, -1] == got.count[shape[0] - 1]
    with pytest.raises(ValueError, match="as_grid needs"):
        got.as_grid('density', (shape[0] + 1, shape[1], shape[2]))


def test_what_sample_grid_refuses():
    for shape in ((4, 4), (4, 0, 4), (4, 4, 4, 4)):
        with pytest.raises(ValueError, match="three counts"):
            hoomd.sample_grid(CUBE, shape)
    with pytest.raises(ValueError, match="nz == 1"):
        hoomd.sample_grid(FLAT, (4, 4, 2), dimensions=2)
    with pytest.raises(ValueError, match="dimensions must be 2 or 3"):
        hoomd.sample_grid(CUBE, (4, 4, 4), dimensions=4)
    with pytest.raises(ValueError, match="6 values"):
        hoomd.sample_grid([8, 8, 8], (4, 4, 4))
    with pytest.raises(ValueError, match="three finite fractions"):
        hoomd.sample_grid(CUBE, (4, 4, 4), lo=(0, 0))


# ---------------------------------------------------------------- frames, h=None, the command line
def small_frame(slength=None, velocity=True, density=True):
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
    fr.particles.pressure = np.array([1, 2, 3, 1, 1.5, 1], np.float32)
    if slength is not None:
        fr.particles.slength = np.asarray(slength, np.float32)
    return fr


POINTS = np.array([[1.1, 1.1, 1.0], [3.95, 0, 0], [0, 0, 0], [np.nan, 0, 0]], np.float64)


def test_h_none_elided_fields_and_selections():
    fr = small_frame(slength=[0.5] * 6)
    got = hoomd.frame_samples(fr, POINTS, fields=('velocity', 'pressure'))
    want = hoomd.sph_samples(POINTS, fr.particles.position, fr.configuration.box, 0.5, mass=fr.particles.mass,
                             values=[fr.particles.velocity, fr.particles.pressure], density=fr.particles.density)
    assert got.h == 0.5 and words_equal(got.summary, want.summary) and bits_equal(got.values.ravel(), want.values.ravel())
    assert got.columns == (3, 1) and got.count.tolist() == [3, 2, 0, 0] and got.nowhere == 1 and got.empty == 1
    assert hoomd.frame_samples(small_frame(), POINTS).h == 1.0                       # stored nowhere: the schema default
    assert hoomd.frame_samples(fr, POINTS, h=0.75).h == 0.75
    with pytest.raises(ValueError, match="slength ranges from 0.5 to 0.75"):
        hoomd.frame_samples(small_frame(slength=[0.5, 0.5, 0.75, 0.5, 0.5, 0.5]), POINTS)
    # a frame at rest has its velocity elided: it samples as zeros and does not raise
    rest = hoomd.frame_samples(small_frame(slength=[0.5] * 6, velocity=False), POINTS, fields=('velocity',))
    assert rest.values.shape == (4, 3) and not rest.values.any() and bits_equal(rest.shepard, got.shepard)
    blank = hoomd.frame_samples(small_frame(slength=[0.5] * 6, velocity=False), POINTS, normalise=True)
    assert np.isnan(blank.values[2]).all() and not blank.values[[0, 1, 3]].any()   # an empty point is the blank value
    # a density stored nowhere is the number 0.0
    assert hoomd.frame_samples(small_frame(slength=[0.5] * 6, density=False), POINTS).shepard_max == np.inf
    # the selection is the list the entries come from
    fluid = hoomd.frame_samples(fr, POINTS, where={'type': ['fluid']})
    assert fluid.count.tolist() == [2, 2, 0, 0]
    left = hoomd.frame_samples(fr, POINTS, domain=hoomd.domain_grid(2, 1, 1)[0])
    assert left.count.tolist() == [0, 1, 0, 0]                                      # the point reaches across the wrap
    arrays = dict(position=fr.particles.position, density=fr.particles.density)
    assert hoomd.frame_samples(arrays, POINTS, fields=(), h=0.5, box=fr.configuration.box).values.shape == (4, 0)


def test_what_sph_samples_refuses():
    p = random_rows(1, 10, ORTHO)
    x = np.zeros((3, 3))
    for h in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match="finite and positive"):
            hoomd.sph_samples(x, p, ORTHO, h)
    with pytest.raises(ValueError, match="kernel is one of"):
        hoomd.sph_samples(x, p, ORTHO, 0.5, kernel='gaussian')
    with pytest.raises(ValueError, match="narrower"):
        hoomd.sph_samples(x, p, ORTHO, 0.65, cells=(8, 6, 4))
    with pytest.raises(ValueError, match="count twice"):
        hoomd.sph_samples(x, p, ORTHO, 1.6)
    with pytest.raises(ValueError, match="cz == 1"):
        hoomd.sph_samples(x, p, FLAT, 0.3, cells=(2, 2, 2), dimensions=2)
    with pytest.raises(ValueError, match="position holds float32 or float64"):
        hoomd.sph_samples(x, p.astype(np.int32), ORTHO, 0.5)
    with pytest.raises(ValueError, match="mass holds one float32 or float64 value per row"):
        hoomd.sph_samples(x, p, ORTHO, 0.5, mass=np.ones(9))
    with pytest.raises(ValueError, match="density holds one float32 or float64 value per row"):
        hoomd.sph_samples(x, p, ORTHO, 0.5, density=np.ones(10, np.int32))
    for points in (np.zeros((3, 2)), np.zeros(6), np.zeros((3, 3), np.int64)):
        with pytest.raises(ValueError, match="points holds K x 3 float32 or float64 values"):
            hoomd.sph_samples(points, p, ORTHO, 0.5)
    with pytest.raises(ValueError, match="values holds at most 4 arrays: 5"):
        hoomd.sph_samples(x, p, ORTHO, 0.5, values=[np.ones(10)] * 5)
    for bad in (np.ones((10, 5)), np.ones((9, 2)), np.ones((10, 2), np.int32), np.ones((10, 2, 1))):
        with pytest.raises(ValueError, match="value 1 holds N x M float32 or float64 values, 1 <= M <= 4"):
            hoomd.sph_samples(x, p, ORTHO, 0.5, values=[np.ones(10), bad])
    with pytest.raises(ValueError, match="at most 8 columns together: 9"):
        hoomd.sph_samples(x, p, ORTHO, 0.5, values=[np.ones((10, 3))] * 3)
    with pytest.raises(ValueError, match="needs the box"):
        hoomd.frame_samples(dict(position=p), x, h=0.5)
    with pytest.raises(ValueError, match="is not a per-particle attribute"):
        hoomd.frame_samples(small_frame(), x, fields=('speed',))
    for name in ('typeid', 'image', 'orientation'):
        with pytest.raises(ValueError, match="cannot be sampled"):
            hoomd.frame_samples(small_frame(), x, fields=(name,))
    with pytest.raises(ValueError, match="at most 4 names"):
        hoomd.frame_samples(small_frame(), x, fields=('mass',) * 5)
    with pytest.raises(ValueError, match="at most 8 columns together: 9"):
        hoomd.frame_samples(small_frame(), x, fields=('velocity', 'auxiliary1', 'auxiliary2'))


def test_the_command_line_prints_the_samples(tmp_path, capsys):
    path = str(tmp_path / "small.gsd")
    with hoomd.open(path, 'w') as t:
        t.append(small_frame(slength=[0.5] * 6))
    with hoomd.open(path, 'r') as t:
        points = hoomd.sample_grid(t[0].configuration.box, (4, 4, 4))
        want = t.frame_samples(0, points)
        spline = t.frame_samples(0, hoomd.sample_grid(t[0].configuration.box, (8, 8, 2)), fields=('pressure', 'velocity'), h=0.75,
                                 kernel='cubic_spline', normalise=True, where={'type': ['fluid']})
    assert pgsd_main(['info', path, '--sample', '4,4,4']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "SPH samples of frame 0 with h = 0.5 (wendland_c2) on 4 x 4 x 4 points over 8 x 8 x 8 cells:" in lines
    assert "points: 64 nowhere: 0 outside: 0 empty: %d not finite: 0" % want.empty in lines
    assert "count: largest %d at point %d" % (want.count_max, want.count_max_at) in lines
    assert "density: smallest %r largest %r" % (want.density_min, want.density_max) in lines
    assert "shepard: smallest %r largest %r" % (want.shepard_min, want.shepard_max) in lines
    assert "velocity[1]: smallest %r largest %r" % (float(want.values[:, 1].min()), float(want.values[:, 1].max())) in lines
    assert not any(l.startswith("SPH sums") for l in lines)
    assert pgsd_main(['info', path, '--sample', '8,8,2', '0.75', '--kernel', 'cubic_spline', '--types', 'fluid', '--fields',
                      'pressure,velocity', '--normalise']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "SPH samples of frame 0 with h = 0.75 (cubic_spline) on 8 x 8 x 2 points over 5 x 5 x 5 cells (types fluid):" in lines
    assert "points: 128 nowhere: 0 outside: 0 empty: %d not finite: %d" % (spline.empty, spline.not_finite) in lines
    ok = spline.values[:, 0][spline.values[:, 0] == spline.values[:, 0]]
    assert "pressure[0]: smallest %r largest %r (normalised)" % (float(ok.min()), float(ok.max())) in lines
    assert any(l.startswith("velocity[2]:") for l in lines) and spline.empty == spline.not_finite > 0
    assert pgsd_main(['info', path, '--sample', '4,4,4', '2.5']) == 1
    assert "count twice" in capsys.readouterr().err
    assert pgsd_main(['info', path, '--sample', '4,4']) == 1
    assert "--sample takes NX,NY,NZ [H]" in capsys.readouterr().err
    assert pgsd_main(['info', path, '--sample', '4,4,4', '--fields', 'typeid']) == 1
    assert "cannot be sampled" in capsys.readouterr().err
    assert set(SUM_CASES) < set(CASES)
