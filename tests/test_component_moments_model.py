"""pgsd.hoomd.component_moments, the definition of the GPU component fields, against the plain loops of
component_moments_cases: on every mutation case, on random frames with wide-ranged values (so that the order of a sum is told
apart from a bincount), and each mutation of the loop on the case made for it.  Then what the definition promises a user:
its refusals, exact translation invariance of a piece across the periodic faces, `wide` for the ring and the chain of the
components tests, and the per-component masses against frame_moments.  CPU only."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
from neighbours_cases import FLAT, TRICLINIC, random_rows
from components_cases import CUBE
from component_moments_cases import (MUTATIONS, NO_CASE, WIDE_BOX, bits, differences, frame_values, labelled, loop_component_moments,
                                     loop_of, model_of)


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_the_model_equals_the_loop_and_the_mutation_differs_on_its_case(name):
    mutation, case = MUTATIONS[name]
    comps = labelled(case)
    got = model_of(case, comps)
    assert differences(got, loop_of(case, comps)) == []
    assert differences(got, loop_of(case, comps, **mutation)) != [], name
    assert got.n == comps.n and got.components == comps.components


def _random_case(seed, n, box, r, dimensions=3, dtype=np.float64, lost=False, rows=None, **kw):
    p = random_rows(seed, n, box, dtype, dimensions)
    mass, velocity, energy = frame_values(n, seed + 100, dtype)
    if lost:
        p[5::97, 0] = np.nan
        mass[3::41] = np.inf
        velocity[7::53, 1] = np.nan
        energy[11::59] = -np.inf
    return dict(dict(position=p, mass=mass, velocity=velocity, energy=energy, box=box, r=r, dimensions=dimensions, rows=rows), **kw)


RANDOM = {
    'cube': _random_case(1, 700, CUBE, 0.7),
    'cube_f32_lost': _random_case(2, 700, CUBE, 0.8, dtype=np.float32, lost=True),
    'triclinic': _random_case(3, 600, TRICLINIC, 0.7, lost=True),
    'flat': _random_case(4, 300, FLAT, 0.5, dimensions=2),
    'listed': _random_case(5, 500, TRICLINIC, 0.8, rows=np.random.default_rng(5).integers(0, 500, size=400)),
    'no_energy_no_velocity': dict(_random_case(6, 400, CUBE, 0.8), energy=None, velocity=None),
    'no_mass': dict(_random_case(7, 400, CUBE, 0.8), mass=None),
}


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_the_model_equals_the_loop_on_random_frames(name):
    case = RANDOM[name]
    comps = labelled(case)
    got = model_of(case, comps)
    assert differences(got, loop_of(case, comps)) == []
    assert 1 < got.components < got.n and comps.largest > 2
    if case.get('mass') is not None:
        m = np.asarray(case['mass'], np.float64)[comps.rows]
        plain = np.bincount(comps.component, weights=np.where(np.isfinite(m), m, 0.0), minlength=comps.components)
        assert np.allclose(plain, got.mass, rtol=1e-12)
        assert bits(plain) != bits(got.mass)    # the order matters here: a bincount of the same values gives other bits


def test_a_long_component_takes_the_piece_walk():
    """2 049 entries in one component: three pieces; and the loop's order differs from a plain sum."""
    p = np.stack([-30 + 0.0125 * np.arange(2049), np.zeros(2049), np.zeros(2049)], axis=1)
    mass, velocity, energy = frame_values(2049, 9, spread=0)
    case = dict(position=p, mass=mass, velocity=velocity, energy=energy, box=WIDE_BOX, r=0.013, cells=(64, 1, 1))
    comps = labelled(case)
    got = model_of(case, comps)
    assert comps.components == 1 and differences(got, loop_of(case, comps)) == []
    assert got.mass[0] != np.sum(mass[comps.rows]) or got.mass[0] != float(sum(float(v) for v in mass[comps.rows]))
    assert got.wide.tolist() == [0] and got.hi[0, 0] == p[-1, 0] - p[0, 0]


def test_the_extent_of_a_labelling_made_by_hand_takes_no_infinite_displacement():
    """The mutation without a case among the components' own labellings (component_moments_cases.NO_CASE): two rows joined
    by hand, the second infinitely far away."""
    p = np.array([[0, 0, 0], [np.inf, 1, -np.inf]], np.float64)
    label, component = np.array([0, 0], np.uint32), np.array([0, 0], np.uint32)
    got = hoomd.component_moments(None, None, None, p, CUBE, label, component)
    want = loop_component_moments(None, None, None, p, CUBE, label, component)
    assert differences(got, want) == []
    assert bits(got.lo) == bits(np.zeros((1, 3))) and bits(got.hi) == bits(np.array([[0.0, 1.0, 0.0]])) and got.bad.tolist() == [1]
    (switch,) = NO_CASE.values()
    mutated = differences(got, loop_component_moments(None, None, None, p, CUBE, label, component, **switch))
    assert 'lo' in mutated and 'hi' in mutated and 'sums' not in mutated         # (and with them the span: wide, widest)


def test_neither_bound_is_ever_a_negative_zero():
    # the second entry's displacement is -0.0 on every axis
    got = hoomd.component_moments(None, None, None, np.array([[0, 0, 0], [-0.0, -0.0, -0.0]]), CUBE, [0, 0], [0, 0])
    assert bits(got.lo) == bits(np.zeros((1, 3))) and bits(got.hi) == bits(np.zeros((1, 3)))
    assert bits(got.first_moment) == bits(np.zeros((1, 3)))


def test_nothing_and_one_entry():
    got = hoomd.component_moments(np.zeros(0, np.float32), np.zeros((0, 3), np.float32), None, np.zeros((0, 3), np.float32), CUBE,
                                  [], [])
    assert got.summary.tolist() == [0] * 6 and got.mass.shape == (0,) and got.origin.shape == (0, 3)
    assert got.centre_of_mass.shape == (0, 3) and got.heaviest(3).tolist() == []
    one = hoomd.component_moments([2.0], [[1.0, 2, 2]], [3.0], np.array([[1.0, 2, 3]]), CUBE, [0], [0])
    assert one.summary.tolist() == [1, 1, 0, 0, 0, 0] and one.mass.tolist() == [2.0] and one.kinetic.tolist() == [9.0]
    assert one.internal.tolist() == [6.0] and one.origin.tolist() == [[1, 2, 3]] and one.centre_of_mass.tolist() == [[1, 2, 3]]
    assert one.mean_velocity.tolist() == [[1, 2, 2]] and one.span.tolist() == [[0, 0, 0]]


def test_refusals():
    p = np.zeros((4, 3), np.float32)
    p[:, 0] = [0, 0.5, 3, 3.5]
    good = dict(label=[0, 0, 2, 2], component=[0, 0, 1, 1])
    hoomd.component_moments(None, None, None, p, CUBE, **good)
    for label, component, message in (([0, 2, 2, 2], [0, 1, 1, 1], "above its entry"),
                                      ([0, 0, 1, 2], [0, 0, 0, 1], "no root"),
                                      ([0, 0, 2, 2], [0, 0, 1, 2], "differs from its root's"),
                                      ([0, 0, 2, 2], [1, 1, 0, 0], "dense ascending"),
                                      ([0, 0, 2, 2], [0, 0, 2, 2], "dense ascending"),
                                      ([0, 0, 2], [0, 0, 1], "one entry per list entry"),
                                      ([0, 0, 2, 2], [0, 0, 1], "one entry per list entry"),
                                      ([0.0, 0, 2, 2], [0, 0, 1, 1], "integers")):
        with pytest.raises(ValueError, match=message):
            hoomd.component_moments(None, None, None, p, CUBE, label, component)
    with pytest.raises(ValueError, match="row"):
        hoomd.component_moments(None, None, None, p, CUBE, rows=[0, 1, 2, 4], **good)
    with pytest.raises(ValueError, match="position array"):
        hoomd.component_moments(np.ones(4, np.float32), None, None, None, CUBE, **good)
    with pytest.raises(ValueError, match="dimensions"):
        hoomd.component_moments(None, None, None, p, CUBE, dimensions=1, **good)
    with pytest.raises(ValueError, match="differ in their number of rows"):
        hoomd.component_moments(np.ones(3, np.float32), None, None, p, CUBE, **good)
    on_device = hoomd.ComponentMoments.from_tables(np.zeros(6, np.uint64), *[np.zeros((0, w)) for w in (9, 6, 3)],
                                                   np.zeros((0, 2), np.uint32))
    on_device.mass = object()
    for call in (lambda: on_device.centre_of_mass, lambda: on_device.mean_velocity, lambda: on_device.heaviest(1)):
        with pytest.raises(ValueError, match="GPU memory"):
            call()


def _droplet(seed=3, k=60):
    """A droplet on a dyadic lattice: coordinates, masses, velocities and energies are multiples of 2^-8 below 2^3, so every
    difference, product and sum below is exact in float64 whatever the order."""
    rng = np.random.default_rng(seed)
    cells = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing='ij'), axis=-1).reshape(-1, 3)[rng.permutation(64)[:k]]
    offsets = cells * 0.25 + rng.integers(0, 8, size=(k, 3)) / 256.0
    q = lambda a: np.round(a * 256) / 256             # noqa: E731
    return offsets, q(rng.uniform(0.5, 2, k)), q(rng.uniform(-2, 2, (k, 3))), q(rng.uniform(0, 2, k))


def _wrapped(p, box):
    """The stored form of unwrapped positions: folded into the box through the triclinic lattice, exactly (dyadic)."""
    Lx, Ly, Lz, xy, xz, yz = [float(np.float32(b)) for b in box]
    p = p.copy()
    for vec, L, axis in (((xz * Lz, yz * Lz, Lz), Lz, 2), ((xy * Ly, Ly, 0.0), Ly, 1), ((Lx, 0.0, 0.0), Lx, 0)):
        i = np.floor(p[:, axis] / L + 0.5)
        p -= i[:, None] * np.array(vec)
    return p


DYADIC_TRICLINIC = [8, 8, 8, 0.25, -0.125, 0.5]


@pytest.mark.parametrize("box", [CUBE, DYADIC_TRICLINIC], ids=['cube', 'triclinic'])
def test_translation_invariance_is_exact_across_every_face_and_a_corner(box):
    """One cell, so the list is the rows and the root is the droplet's row 0 wherever the droplet lies."""
    offsets, mass, velocity, energy = _droplet()
    results = {}
    for where, corner in (('middle', [-0.5, -0.5, -0.5]), ('x', [3.5, -0.5, -0.5]), ('y', [-0.5, 3.5, -0.5]),
                          ('z', [-0.5, -0.5, 3.5]), ('corner', [3.5, 3.5, 3.5])):
        placed = offsets + np.array(corner)
        stored = _wrapped(placed, box)
        case = dict(position=stored, mass=mass, velocity=velocity, energy=energy, box=box, r=0.6, cells=(1, 1, 1))
        comps = labelled(case)
        assert comps.components == 1 and comps.label.max() == 0, where     # (linked at r = 0.6: lattice spacing 0.25)
        got = model_of(case, comps)
        assert differences(got, loop_of(case, comps)) == []
        assert (where == 'middle') == np.array_equal(stored, placed), where    # elsewhere it does lie across a face
        results[where] = (got, stored[0], placed[0])
    ref, ref_root, ref_placed = results['middle']
    for where, (got, root, placed) in results.items():
        for name in ('mass', 'momentum', 'kinetic', 'internal', 'first_moment', 'lo', 'hi'):
            assert bits(getattr(got, name)) == bits(getattr(ref, name)), (where, name)
        assert got.wide.tolist() == [0] and bits(got.origin[0]) == bits(root)
        # Exactly: the centre relative to the root, first_moment / mass, is one value wherever the droplet lies, and the
        # origin differs by exactly the shift of the stored root -- the translation, less the lattice vector that folded
        # it (below).  centre_of_mass = origin + first_moment / mass adds the two and rounds once more, so the centres
        # themselves differ by the shift to that last rounding only: half an ulp of each of the two centres.
        relative = got.first_moment[0] / got.mass[0]
        assert bits(relative) == bits(ref.first_moment[0] / ref.mass[0]), where
        assert bits(got.origin[0] - ref.origin[0]) == bits(root - ref_root), where
        assert bits(got.centre_of_mass[0]) == bits(got.origin[0] + relative), where
        rounding = 0.5 * (np.spacing(np.abs(got.centre_of_mass[0])) + np.spacing(np.abs(ref.centre_of_mass[0])))
        assert (np.abs((got.centre_of_mass[0] - ref.centre_of_mass[0]) - (root - ref_root)) <= 2 * rounding).all(), where
        lattice = (placed - ref_placed) - (root - ref_root)
        Lx, Ly, Lz, xy, xz, yz = box
        k = lattice[2] / Lz
        j = (lattice[1] - k * yz * Lz) / Ly
        i = (lattice[0] - j * xy * Ly - k * xz * Lz) / Lx
        assert all(float(c).is_integer() for c in (i, j, k)), (where, lattice)
    # and the unwrapped centre is where the droplet's own centre is
    centre = (mass[:, None] * (offsets - offsets[0])).sum(axis=0) / mass.sum()
    assert np.allclose(ref.centre_of_mass[0] - ref_root, centre, rtol=0, atol=1e-13)


@pytest.mark.parametrize("k, ring", [(640, True), (639, False)])
def test_the_ring_and_the_chain_of_the_components_tests_are_wide(k, ring):
    p = np.stack([-4.0 + 0.0125 * np.arange(k), np.zeros(k), np.zeros(k)], axis=1)
    case = dict(position=p, box=CUBE, r=0.013, cells=(64, 1, 1))
    comps = labelled(case)
    got = model_of(case, comps)
    assert comps.components == 1 and got.wide.tolist() == [1] and got.wide_components == 1 and got.widest_id == 0
    assert differences(got, loop_of(case, comps)) == []
    assert got.span[0, 0] >= 4.0 and got.span[0, 1] == 0 and got.span[0, 2] == 0


def test_the_masses_add_up_to_frame_moments_and_the_frame_level_equals_the_parts():
    n = 900
    fr = hoomd.Frame()
    fr.configuration.box = TRICLINIC
    fr.particles.N = n
    fr.particles.types = ['a', 'b']
    fr.particles.typeid = np.random.default_rng(1).integers(0, 2, n).astype(np.uint32)
    fr.particles.position = random_rows(8, n, TRICLINIC, np.float32)
    mass, velocity, energy = frame_values(n, 8, np.float32, spread=4)
    fr.particles.mass, fr.particles.velocity, fr.particles.energy = mass, velocity, energy
    for options in (dict(), dict(where={'type': ['a']}), dict(domain=hoomd.domain_grid(2, 1, 1)[0])):
        got = hoomd.frame_component_moments(fr, 0.7, **options)
        comps = hoomd.frame_components(fr, 0.7, **options)
        total = hoomd.frame_moments(fr, by_type=False, **options)
        assert got.components_of.components == comps.components == got.components and np.array_equal(got.sizes, comps.sizes)
        assert np.array_equal(got.components_of.label, comps.label)
        assert np.isclose(got.mass.sum(), total.mass[0], rtol=1e-13) and np.allclose(got.momentum.sum(axis=0), total.momentum[0],
                                                                                       rtol=1e-10, atol=1e-9)
        assert np.isclose(got.kinetic.sum(), total.kinetic[0], rtol=1e-12) and got.n == comps.n
        want = hoomd.component_moments(mass, velocity, energy, fr.particles.position, TRICLINIC, comps.label, comps.component,
                                       rows=comps.rows)
        assert bits(want.mass) == bits(got.mass) and bits(want.first_moment) == bits(got.first_moment)
        assert got.heaviest_id == int(np.argmax(got.mass)) and got.heaviest(3)[0] == got.heaviest_id
        assert got.widest_id == int(np.argmax(got.span.max(axis=1)))
        inside = got.wide == 0
        assert inside.any() and (np.abs(got.centre_of_mass[inside] - got.origin[inside]) <= got.span[inside] + 1e-12).all()


def test_the_command_line_prints_the_heaviest_pieces(tmp_path, capsys):
    from pgsd.__main__ import main as pgsd_main
    path = str(tmp_path / "pieces.gsd")
    fr = hoomd.Frame()
    fr.configuration.box = CUBE
    fr.particles.N = 6
    # a piece of three across the x face (mass 6), a pair (mass 3), a singleton whose mass is not finite
    fr.particles.position = np.array([[3.75, 0, 0], [-3.75, 0, 0], [-3.25, 0, 0], [0, 1, 0], [0.5, 1, 0], [0, -2, 0]], np.float32)
    fr.particles.mass = np.array([2, 2, 2, 1, 2, np.inf], np.float32)
    fr.particles.velocity = np.array([[1, 0, 0], [1, 0, 0], [4, 0, 0], [0, 3, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    with hoomd.open(path, 'w') as t:
        t.append(fr)
    want = hoomd.frame_component_moments(fr, 1.0)
    assert want.components == 3 and want.bad_entries == 1 and want.wide_components == 0
    assert pgsd_main(['info', path, '--components', '1.0']) == 0
    assert "heaviest" not in capsys.readouterr().out
    assert pgsd_main(['info', path, '--components', '1.0', '--pieces']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "the 3 heaviest of 3 pieces (centre, mean velocity and span per axis):" in lines
    across = int(want.heaviest(1)[0])
    assert want.sizes[across] == 3 and want.mass[across] == 6.0 and want.span[across].tolist() == [1.0, 0, 0]
    # the piece across the face about its root, the entry at x = -3.75: d = 0, +0.5 and -0.5 (through the face)
    c = want.centre_of_mass[across]
    first = "piece %d: 3 entries, mass 6, centre (%.6g, %.6g, %.6g), velocity (2, 0, 0), span (1, 0, 0)" % (across, c[0], c[1], c[2])
    assert lines[lines.index("the 3 heaviest of 3 pieces (centre, mean velocity and span per axis):") + 1] == first
    assert c.tolist() == [-3.75, 0, 0] and want.lo[across, 0] == -0.5 and want.hi[across, 0] == 0.5
    assert "wide pieces: 0 (extent >= half a box length: centre and span are not meaningful)" in lines
    assert "bad entries: 1 (a value that is not finite; left out of the sums)" in lines
    assert pgsd_main(['info', path, '--components', '1.0', '--pieces', '1']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "the 1 heaviest of 3 pieces (centre, mean velocity and span per axis):" in lines
    assert sum(1 for l in lines if l.startswith("piece ")) == 1
