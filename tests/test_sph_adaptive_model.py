"""The numpy model of the SPH sums with a per-particle smoothing length (pgsd.hoomd.sph_adaptive_sums /
frame_adaptive_sums), the definition the GPU pass equals exactly (tests/test_gpu_sph_adaptive.py): it equals a plain double
loop bit for bit, with every h equal it IS the uniform pass bit for bit, gather mode does not look at h_j, the count is a
brute-force count, a lattice gives density 1 and omega 1, omega is the derivative of the density in h_i, every mutation of
the loop differs from it on the case that names it, and the command line prints it.  No GPU."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

from sph_cases import CASES as SUM_CASES, CUBE, KERNELS, LOOP_ENTRIES, NONE, bits_equal
from sph_adaptive_cases import (EQUIVALENT, MODES, MUTATIONS, adaptive_case, derivative_error, jittered, lattice, loop_adaptive,
                                same, seeded_h)
from test_sph_model import small_frame

# The worst relative error of check 6 measured with the model (numpy, float64): 3.7e-5 for the Wendland kernel, 1.5e-4
# for the cubic spline ("SPH sums with a per-particle smoothing length").  It is relative to the
# derivative itself, which falls to 1e-4 of density / h where omega is close to 1, and that is what inflates it: against
# density / h the error is 3.9e-8 and 4.2e-8.  100 times the larger figure
# exceeds the cap of 1e-3, so the cap is the bound.  Dropping the q w' term misses by 4.7e3 (Wendland) and 2.9e4 (spline),
# flipping its sign by twice that.
DERIVATIVE_MEASURED = 1.5e-4
DERIVATIVE_BOUND = min(100 * DERIVATIVE_MEASURED, 1e-3)
LATTICE_DENSITY, LATTICE_OMEGA = 0.05, 0.1


# ---------------------------------------------------------------- 1. the model is the loop
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", sorted(SUM_CASES))
def test_the_model_equals_the_double_loop_bit_for_bit(name, kernel, mode):
    p, mass, density, kw, h = adaptive_case(name)
    n = len(p)
    # (the loop is quadratic in a crowded cell: beyond LOOP_ENTRIES entries it takes a strided sub-list of the case)
    rows = None if n <= LOOP_ENTRIES else np.arange(0, n, -(-n // LOOP_ENTRIES))
    for dtype in (np.float64, np.float32):
        args = dict(kw, position=p.astype(dtype), slength=seeded_h(name, n, h, dtype=dtype), mass=mass, density=density,
                    rows=rows, kernel=kernel, mode=mode)
        got = hoomd.sph_adaptive_sums(**args)
        assert same(got, loop_adaptive(**args)), (name, kernel, mode, dtype)
    assert got.n == (n if rows is None else len(rows)) and got.mode == mode and got.kernel == kernel
    assert got.count.dtype == np.uint32 and got.pairs == int(got.count.sum()) and got.bad_h == 0
    assert (got.omega is None) == (mode == 'mean') and (got.omega_min is None) == (mode == 'mean')
    assert got.slength.dtype == np.float64
    if name == 'all_nowhere':
        assert got.nowhere == got.n and got.density_min == np.inf and got.count_min is None and got.pairs == 0
        for a in (got.number, got.density, got.shepard) + (() if got.omega is None else (got.omega,)):
            assert not a.any() and not np.signbit(a).any()
    else:
        assert got.h_max == float(got.slength.max()) and got.slength_max <= got.h_max and got.count_min >= 1
    if name == 'three_cells':
        lost = got.cell == 27
        assert lost.any() and not got.count[lost].any() and not got.density[lost].any()
    if name == 'flat':
        assert got.dimensions == 2
    if name == 'one_cell_65':
        assert got.shepard is None and got.shepard_min is None and got.deviation is None and got.surface is None


@pytest.mark.parametrize("mode", MODES)
def test_a_list_in_any_order_with_repeats(mode):
    p, mass, density, kw, h = adaptive_case('three_cells')
    rows = np.concatenate([np.arange(400, 0, -1), [7, 7, 400, 12]])
    args = dict(kw, position=p, slength=seeded_h('three_cells', len(p), h), mass=mass, density=density, rows=rows, mode=mode)
    got = hoomd.sph_adaptive_sums(**args)
    assert same(got, loop_adaptive(**args)) and got.n == 404 and got.count_min >= 1
    assert got.h_max == got.slength.max() < seeded_h('three_cells', len(p), h).max()      # the maximum over the LIST


# ---------------------------------------------------------------- 2. every h equal: the uniform pass
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", sorted(SUM_CASES))
def test_with_one_h_gather_mode_is_the_uniform_pass_bit_for_bit(name, kernel):
    p, mass, density, kw = SUM_CASES[name]
    want = hoomd.sph_kernel_sums(p, mass=mass, density=density, kernel=kernel, **kw)
    kw = dict(kw)
    H = kw.pop('h')
    if name == 'all_nowhere':
        kw['cells'] = want.grid
    got = hoomd.sph_adaptive_sums(p, kw.pop('box'), np.full(len(p), H), mass=mass, density=density, kernel=kernel, **kw)
    assert got.grid == want.grid and got.h_max == want.h and np.array_equal(got.rows, want.rows)
    assert bits_equal(got.number, want.number) and bits_equal(got.density, want.density)
    assert (got.shepard is None) == (want.shepard is None) and (want.shepard is None or bits_equal(got.shepard, want.shepard))
    for a in ('n', 'nowhere', 'not_finite', 'surface', 'deviation_at', 'deviation_row'):
        assert getattr(got, a) == getattr(want, a), a
    for a in ('number_min', 'number_max', 'density_min', 'density_max', 'shepard_min', 'shepard_max', 'deviation'):
        x, y = getattr(got, a), getattr(want, a)
        assert (x is None) == (y is None) and (x is None or bits_equal(x, y)), a


# ---------------------------------------------------------------- 3. independence from h_j; the mean is symmetric
@pytest.mark.parametrize("kernel", KERNELS)
def test_gather_mode_does_not_look_at_h_j_and_the_mean_is_symmetric(kernel):
    p, mass, density, kw, h = adaptive_case('mass_density')
    n = len(p)
    s = seeded_h('mass_density', n, h, lo=0.5)
    s[0] = h                                                            # (row 0 holds h_max in both columns)
    other = s.copy()
    other[1::2] = np.random.default_rng(3).uniform(0.1 * h, h, size=len(other[1::2]))
    a = hoomd.sph_adaptive_sums(p, slength=s, mass=mass, density=density, kernel=kernel, **kw)
    b = hoomd.sph_adaptive_sums(p, slength=other, mass=mass, density=density, kernel=kernel, **kw)
    assert np.array_equal(a.rows, b.rows) and a.h_max == b.h_max == h
    kept = np.isin(a.rows, np.arange(0, n, 2))
    assert kept.sum() == n // 2 and not np.array_equal(a.count[~kept], b.count[~kept])
    for name in ('count', 'number', 'density', 'shepard', 'omega'):
        assert bits_equal(getattr(a, name)[kept], getattr(b, name)[kept]), name
    # two particles, mean mode: i <- j and j <- i carry the same w*p
    two = dict(position=np.array([[0, 0, 0], [0.7, 0.2, -0.1]]), box=CUBE, slength=np.array([0.9, 0.4]), kernel=kernel, mode='mean')
    ab = hoomd.sph_adaptive_sums(**two)
    ba = hoomd.sph_adaptive_sums(**dict(two, position=two['position'][::-1].copy(), slength=two['slength'][::-1].copy()))
    C = hoomd.sph_sigma(kernel, 1.0)
    own = [C * float(hoomd.sph_weight(0.0, kernel)) / hh ** 3 for hh in (0.9, 0.4)]
    assert ab.count.tolist() == [2, 2] and ab.pairs == 4
    pair = [ab.number[list(ab.rows).index(r)] - own[r] for r in (0, 1)]
    assert pair[0] > 0 and abs(pair[0] - pair[1]) <= 4 * np.spacing(ab.number.max())
    assert bits_equal(np.sort(ab.number), np.sort(ba.number))


# ---------------------------------------------------------------- 4. the count against brute force
@pytest.mark.parametrize("mode", MODES)
def test_the_count_is_a_brute_force_count(mode):
    rng = np.random.default_rng(300)
    p = rng.uniform(-4, 4, size=(300, 3))
    s = rng.uniform(0.5, 1.0, size=300)
    got = hoomd.sph_adaptive_sums(p, CUBE, s, mode=mode)
    x, hh = p[got.rows], s[got.rows]
    d = x[:, None, :] - x[None, :, :]
    d -= 8.0 * np.round(d / 8.0)
    r = np.sqrt((d * d).sum(axis=2))
    reach = 2.0 * hh[:, None] if mode == 'gather' else hh[:, None] + hh[None, :]
    brute = (r < reach).sum(axis=1)
    assert np.array_equal(got.count, brute) and got.pairs == int(brute.sum()) and got.slength_max / got.slength_min > 1.9
    assert got.count_min == brute.min() and got.count_max == brute.max() and got.count_min_at == int(np.argmin(brute))


# ---------------------------------------------------------------- 5. the lattice constants
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dimensions", (3, 2))
def test_a_lattice_has_density_one_and_omega_one(dimensions, kernel):
    """Spacing 1, unit masses, h seeded in [1.0, 1.6]: over the interior (at least 4 from every face) the gather density
    is within 0.05 of 1 and omega within 0.1 of 1 (measured worst: 0.038 and 0.059, Wendland, 2-D).  Without the q w' term
    omega is 0, with its sign flipped about -1."""
    p, box, h, interior = lattice(dimensions)
    got = hoomd.sph_adaptive_sums(p, box, h, dimensions=dimensions, kernel=kernel)
    inside = interior[got.rows]
    assert inside.sum() == 4 ** dimensions
    assert np.abs(got.density[inside] - 1.0).max() <= LATTICE_DENSITY
    assert np.abs(got.omega[inside] - 1.0).max() <= LATTICE_OMEGA
    assert bits_equal(got.number, got.density) and got.bad_h == 0 and got.nowhere == 0


# ---------------------------------------------------------------- 6. omega is the derivative
def density_in_row_order(p, box, mass, kernel):
    def of(slength):
        got = hoomd.sph_adaptive_sums(p, box, slength, mass=mass, kernel=kernel)
        out = np.empty(len(p))
        out[got.rows] = got.density
        return out
    return of


@pytest.mark.parametrize("kernel", KERNELS)
def test_omega_is_the_derivative_of_the_density_in_h(kernel):
    p, box, h, mass = jittered()
    got = hoomd.sph_adaptive_sums(p, box, h, mass=mass, kernel=kernel)
    omega, density = np.empty(len(p)), np.empty(len(p))
    omega[got.rows], density[got.rows] = got.omega, got.density
    error = derivative_error(p, box, h, mass, density_in_row_order(p, box, mass, kernel), omega, density)
    print("omega against the central difference, %s: worst relative error %.3g" % (kernel, error))
    assert error <= DERIVATIVE_BOUND
    # the mutants: a_m is sum m_j w, so omega = -sum m_j q w' / (D a_m): without the q w' term it is 0, with the term's
    # sign flipped it is -omega
    for mutant in (np.zeros_like(omega), -omega):
        assert derivative_error(p, box, h, mass, density_in_row_order(p, box, mass, kernel), mutant, density) > 0.3


# ---------------------------------------------------------------- 7. the mutations
@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_every_mutation_differs_on_its_case(mutation):
    switch, case = MUTATIONS[mutation]
    case = dict(case)
    kernels = [case.pop('kernel')] if 'kernel' in case else KERNELS
    for kernel in kernels:
        got = hoomd.sph_adaptive_sums(kernel=kernel, **case)
        assert same(got, loop_adaptive(kernel=kernel, **case)), mutation
        assert not same(got, loop_adaptive(kernel=kernel, **dict(case, **switch))), (mutation, kernel)


@pytest.mark.parametrize("mutation", sorted(EQUIVALENT))
def test_a_mutation_no_input_can_show_is_said_so(mutation):
    """tests/sph_adaptive_cases.py gives the reason each of these changes no result; here it changes none on its case."""
    switch, case = EQUIVALENT[mutation]
    case = dict(case)
    kernels = [case.pop('kernel')] if 'kernel' in case else KERNELS
    for kernel in kernels:
        got = hoomd.sph_adaptive_sums(kernel=kernel, **case)
        assert same(got, loop_adaptive(kernel=kernel, **dict(case, **switch))), (mutation, kernel)


# ---------------------------------------------------------------- 8. an h that is not valid
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bad", (0.0, -0.5, np.nan, np.inf))
def test_an_invalid_h_is_bad_h_contributes_to_nobody_and_is_written_as_zero(bad, mode):
    p, mass, density, kw, h = adaptive_case('mass_density')
    s = seeded_h('mass_density', len(p), h)
    s[[3, 77, 300]] = bad
    args = dict(kw, position=p, slength=s, mass=mass, density=density, mode=mode)
    got = hoomd.sph_adaptive_sums(**args)
    assert same(got, loop_adaptive(**args)) and got.bad_h == 3 and got.nowhere == 0
    at = np.isin(got.rows, [3, 77, 300])
    for a in (got.count, got.number, got.density, got.shepard) + (() if got.omega is None else (got.omega,)):
        assert not a[at].any() and not np.signbit(a[at].astype(np.float64)).any()
    # nobody's sums contain them: the same list without the three rows gives the same values for the others
    rest = np.setdiff1d(np.arange(len(p)), [3, 77, 300])
    without = hoomd.sph_adaptive_sums(**dict(args, rows=rest, cells=got.grid))
    assert without.bad_h == 0 and np.array_equal(without.rows, got.rows[~at])
    assert bits_equal(without.density, got.density[~at]) and np.array_equal(without.count, got.count[~at])
    assert got.pairs == without.pairs and got.slength_max == without.slength_max and got.count_min_at is not None


# ---------------------------------------------------------------- 9. the rest
def test_a_list_without_a_valid_h_raises_and_a_list_of_nothing_is_answered():
    p = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="no listed row has a valid smoothing length"):
        hoomd.sph_adaptive_sums(p, CUBE, np.array([0.0, np.nan, -1.0, np.inf]))
    with pytest.raises(ValueError, match="no listed row has a valid smoothing length"):
        hoomd.sph_adaptive_sums(p, CUBE, np.array([0.5, np.nan, -1.0, np.inf]), rows=[1, 2])
    for mode in MODES:
        got = hoomd.sph_adaptive_sums(p, CUBE, np.full(4, 0.5), rows=np.arange(0), mode=mode)
        assert same(got, loop_adaptive(p, CUBE, np.full(4, 0.5), rows=np.arange(0), mode=mode))
        assert got.n == 0 and got.pairs == 0 and got.h_max == -np.inf and got.count_min is None and got.density_min == np.inf
        assert got.summary.tolist()[:10] == [0, 0, 0, 0, 0, NONE, NONE, 0, 0, NONE]
        assert got.count.shape == (0,) and got.grid == (1, 1, 1)


def test_the_summary_rules():
    # a NaN never replaces a bound; the smaller position wins a tie of the count; the deviation keeps its sign
    p = np.array([[0, 0, 0], [3, 3, 3], [-3, -3, -3], [0.1, 0, 0]], np.float64)
    s = np.array([0.5, 0.5, 0.25, 0.5])
    got = hoomd.sph_adaptive_sums(p, CUBE, s, mass=np.array([1, 1, np.nan, 1.0]), density=np.array([1, 50, 1, 1.0]),
                                  surface_below=10.0)
    assert got.not_finite == 1 and np.isnan(got.density).sum() == 1 and np.isfinite([got.density_min, got.density_max]).all()
    assert got.count.tolist().count(1) == 2 and got.count_min == 1 and got.count_max == 2
    assert got.count_min_at == min(k for k in range(4) if got.count[k] == 1)
    assert got.deviation < 0 and got.deviation_row == 1 and got.rows[got.deviation_at] == 1
    assert got.surface == int((got.shepard < 10.0).sum()) > 0 and got.slength_min == 0.25 and got.slength_max == 0.5 and got.pairs == 6
    assert np.isnan(got.omega).sum() == 1 and np.isfinite([got.omega_min, got.omega_max]).all()
    with pytest.raises(ValueError, match="22 words"):
        hoomd.AdaptiveSums(1.0, 'wendland_c2', 'gather', (1, 1, 1), 3, np.zeros(13, np.uint64), False)
    assert "AdaptiveSums(h_max=0.5" in repr(got) and np.array_equal(got.summary, got.summary)


def test_what_the_model_refuses():
    p = np.random.default_rng(1).uniform(-4, 4, size=(20, 3))
    s = np.full(20, 0.5)
    for kw, message in ((dict(mode='scatter'), "the mode is one of gather, mean"), (dict(kernel='gauss'), "the kernel is one of"),
                        (dict(slength=s[:19]), "slength holds one float32 or float64 value per row"),
                        (dict(slength=np.arange(20)), "slength holds one float32 or float64 value per row"),
                        (dict(cells=(9, 8, 8)), "narrower"), (dict(slength=np.full(20, 2.5)), "count twice"),
                        (dict(surface_below=np.nan), "surface_below is a number or None"),
                        (dict(mass=np.ones(19)), "mass holds one"), (dict(rows=[20]), "outside"),
                        (dict(dimensions=2, cells=(4, 4, 4)), "dimensions == 2 takes cz == 1"), (dict(cells=(8, 8)), "three counts")):
        with pytest.raises(ValueError, match=message):
            hoomd.sph_adaptive_sums(**dict(dict(position=p, box=CUBE, slength=s), **kw))
    # the grid is checked against 2 h_max of the LIST: a wide h that is not listed does not count
    wide = s.copy()
    wide[7] = 2.5
    assert hoomd.sph_adaptive_sums(p, CUBE, wide, rows=np.setdiff1d(np.arange(20), [7]), cells=(8, 8, 8)).h_max == 0.5


def test_smoothing_range():
    s = np.array([0.5, np.inf, 0.25, np.nan, 0.0, -1.0, 0.75], np.float32)
    assert hoomd.smoothing_range(s) == (7, 4, 0.25, 0.75)
    assert hoomd.smoothing_range(s, rows=[0, 0, 2, 3]) == (4, 1, 0.25, 0.5)
    assert hoomd.smoothing_range(s, rows=[1, 3]) == (2, 2, np.inf, -np.inf)
    assert hoomd.smoothing_range(s, rows=np.arange(0)) == (0, 0, np.inf, -np.inf)
    assert hoomd.smoothing_range(np.array([np.float32(0.1)])) == (1, 0, float(np.float32(0.1)), float(np.float32(0.1)))
    with pytest.raises(ValueError, match="outside"):
        hoomd.smoothing_range(s, rows=[7])
    with pytest.raises(ValueError, match="float32 or float64"):
        hoomd.smoothing_range(np.arange(3))


SIX = [0.5, 0.5, 0.75, 0.5, 0.5, 0.5]


def test_the_frame_the_uniform_pass_refuses_is_answered_here():
    fr = small_frame(slength=SIX)
    with pytest.raises(ValueError, match="a per-particle smoothing length is not supported; pass h"):
        hoomd.frame_kernel_sums(fr)
    for mode in MODES:
        got = hoomd.frame_adaptive_sums(fr, mode=mode, surface_below=0.5)
        want = hoomd.sph_adaptive_sums(fr.particles.position, fr.configuration.box, np.asarray(SIX, np.float32),
                                       mass=fr.particles.mass, density=fr.particles.density, mode=mode, surface_below=0.5)
        assert np.array_equal(got.summary, want.summary) and bits_equal(got.density, want.density)
        assert got.n == 6 and got.nowhere == 1 and got.h_max == 0.75 and got.slength_min == 0.5 and got.volume
    assert got.count[list(got.rows).index(2)] == 3 and got.count[list(got.rows).index(3)] == 2       # 3 and 4 across the wrap
    fluid = hoomd.frame_adaptive_sums(fr, where={'type': ['fluid']})
    assert fluid.n == 5 and fluid.h_max == 0.5                          # the wide row is a wall: the maximum is the list's
    # a slength stored nowhere is the schema default in every row: the uniform pass at h = 1.0
    plain = hoomd.frame_adaptive_sums(small_frame())
    assert plain.h_max == 1.0 and bits_equal(plain.density, hoomd.frame_kernel_sums(small_frame()).density)
    # arrays in place of a frame
    arrays = dict(position=fr.particles.position, slength=fr.particles.slength, mass=fr.particles.mass)
    bare = hoomd.frame_adaptive_sums(arrays, box=fr.configuration.box)
    assert bare.shepard is None and bits_equal(bare.density, hoomd.frame_adaptive_sums(fr).density)


def test_the_command_line_prints_it(tmp_path, capsys):
    path = str(tmp_path / "six.gsd")
    with hoomd.open(path, 'w') as t:
        t.append(small_frame(slength=SIX))
    assert pgsd_main(['info', path, '--sph-adaptive', '--surface', '7']) == 0
    out = capsys.readouterr().out
    want = hoomd.frame_adaptive_sums(small_frame(slength=SIX), surface_below=7.0)
    assert "(wendland_c2, gather), h_max = 0.75, over %d x %d x %d cells" % want.grid in out
    assert "entries:      6  nowhere: 1  bad_h: 0" in out and "slength:      smallest 0.5  largest 0.75" in out
    assert "pairs: %d" % want.pairs in out and "density:      smallest %r  largest %r" % (want.density_min, want.density_max) in out
    assert "deviation:    %r at row %d" % (want.deviation, want.deviation_row) in out and "surface:      %d below 7.0" % want.surface in out
    assert "omega:        smallest %r  largest %r" % (want.omega_min, want.omega_max) in out
    assert pgsd_main(['info', path, '--sph-adaptive', '--mode', 'mean', '--kernel', 'cubic_spline', '--types', 'fluid']) == 0
    out = capsys.readouterr().out
    assert "(cubic_spline, mean), h_max = 0.5" in out and "(types fluid)" in out and "omega" not in out
    assert "entries:      5" in out
    # the uniform pass still refuses this frame on the command line
    assert pgsd_main(['info', path, '--sph']) == 1
    assert "a per-particle smoothing length is not supported" in capsys.readouterr().err
