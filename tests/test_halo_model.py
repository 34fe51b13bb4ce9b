"""The numpy model of a domain read with a ghost layer (pgsd.hoomd.ghost_fractions / halo_bands / halo_rows): the
definition the GPU selection of read_frame_device(domain=..., ghost=...) must equal exactly
(tests/test_gpu_halo.py).  CPU only."""
import itertools

import numpy as np
import pytest

import pgsd.hoomd as hoomd

GRIDS = {
    "1x1x1": hoomd.domain_grid(1, 1, 1),
    "2x2x2": hoomd.domain_grid(2, 2, 2),
    "3x1x2": hoomd.domain_grid(3, 1, 2),
    "unequal": hoomd.domain_grid(3, 1, 2, x_split=[0.25, 0.5], z_split=[0.375]),
}
ORTHO = np.array([16.0, 16.0, 16.0, 0.0, 0.0, 0.0], np.float32)     # width 1.0 is g = 1/16 on every axis, exactly
WIDTH = 1.0
G = 1.0 / 16.0


def _triclinic_box(rng):
    L = rng.uniform(2.0, 20.0, size=3)
    tilt = rng.uniform(-0.8, 0.8, size=3)
    return np.array([L[0], L[1], L[2], tilt[0], tilt[1], tilt[2]], dtype=np.float32)


def _positions(rng, box, n):
    """Points of the box and well outside it (periodic images), as float32."""
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in box)
    s = rng.uniform(-1.5, 2.5, size=(n, 3))
    z = (s[:, 2] - 0.5) * Lz
    y = (s[:, 1] - 0.5) * Ly + yz * z
    x = (s[:, 0] - 0.5) * Lx + xy * y + xz * z
    return np.stack([x, y, z], axis=1).astype(np.float32)


def grid_positions(rng, n):
    """(positions, fractions): fractions k / 64 per axis, every k on every axis, placed in the ORTHO box or one of its
    periodic images -- every operation of the model and of the brute force below is exact on them."""
    k = rng.integers(0, 64, size=(n, 3))
    k[:64] = np.arange(64)[:, None]                         # every multiple of 1/64 on every axis
    f = k / 64.0
    image = rng.integers(-1, 2, size=(n, 3))
    p = (f + image - 0.5) * 16.0
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32), f


def brute_force(f, domain, g):
    """Row by row over the 27 periodic images: a row that the cell does not own is a ghost when one image s of it lies
    in the cell grown by g on every divided axis (an undivided axis takes no image but s = 0 and asks nothing)."""
    lo, hi = domain.lo, domain.hi
    divided = [not (lo[a] == 0.0 and hi[a] == 1.0) for a in range(3)]
    owned, ghosts, shifts = [], [], []
    for i in range(len(f)):
        if all(lo[a] <= f[i, a] < hi[a] for a in range(3)):
            owned.append(i)
            continue
        found = []
        for s in itertools.product((-1, 0, 1), repeat=3):
            if any(s[a] != 0 and not divided[a] for a in range(3)):
                continue
            if all(not divided[a] or lo[a] - g <= f[i, a] + s[a] < hi[a] + g for a in range(3)):
                found.append(s)
        assert len(found) <= 1, (i, found)
        if found:
            ghosts.append(i)
            shifts.append(found[0])
    return np.array(owned, np.int64), np.array(ghosts, np.int64), np.array(shifts, np.int32).reshape(-1, 3)


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_owned_rows_are_domain_rows(grid):
    rng = np.random.default_rng(11)
    box = _triclinic_box(rng)
    pos = _positions(rng, box, 4000)
    on_grid = grid_positions(rng, 2000)[0]
    for d in GRIDS[grid]:
        assert np.array_equal(hoomd.halo_rows(pos, box, d, (0.05, 0.04, 0.03))[0], hoomd.domain_rows(pos, box, d))
        assert np.array_equal(hoomd.halo_rows(on_grid, ORTHO, d, WIDTH)[0], hoomd.domain_rows(on_grid, ORTHO, d))


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_ghosts_and_shifts_equal_the_brute_force_over_27_images(grid):
    rng = np.random.default_rng(5)
    pos, f = grid_positions(rng, 3000)
    assert hoomd.ghost_fractions(ORTHO, WIDTH) == (G, G, G)
    for d in GRIDS[grid]:
        # rows exactly on lo - g, lo, hi, hi + g, 0 and the wrapped bounds of every divided axis are in the set
        for a in range(3):
            if d.lo[a] == 0.0 and d.hi[a] == 1.0:
                continue
            planes = {(d.lo[a] - G) % 1.0, d.lo[a], d.hi[a] % 1.0, (d.hi[a] + G) % 1.0, 0.0}
            exact = {v for v in planes if v * 64 == int(v * 64)}
            assert exact and exact <= set(f[:, a]), (grid, a, planes)
        owned, ghosts, shift = hoomd.halo_rows(pos, ORTHO, d, WIDTH)
        want_owned, want_ghosts, want_shift = brute_force(f, d, G)
        assert np.array_equal(owned, want_owned)
        assert np.array_equal(ghosts, want_ghosts), (grid, d)
        assert shift.dtype == np.int32 and shift.shape == (len(ghosts), 3) and np.array_equal(shift, want_shift)
        if grid != "1x1x1":
            assert len(ghosts) > 0 and np.abs(shift).max() == 1         # every such cell touches a face of the box


@pytest.mark.parametrize("seed", range(4))
def test_invariants_on_random_positions_in_a_triclinic_box(seed):
    rng = np.random.default_rng(seed)
    box = _triclinic_box(rng)
    pos = _positions(rng, box, 5000)
    g = hoomd.ghost_fractions(box, 0.2)
    assert all(0.0 < v <= 0.25 for v in g)
    for name, grid in GRIDS.items():
        for d in grid:
            owned, ghosts, shift = hoomd.halo_rows(pos, box, d, 0.2)
            assert np.array_equal(hoomd.halo_rows(pos, box, d, g)[1], ghosts)       # a width or its three fractions
            assert len(np.intersect1d(owned, ghosts)) == 0
            assert (np.diff(owned) > 0).all() and (np.diff(ghosts) > 0).all()
            for a in range(3):
                if d.lo[a] == 0.0 and d.hi[a] == 1.0:
                    assert (shift[:, a] == 0).all()
            if name == "1x1x1":
                assert len(ghosts) == 0 and len(owned) == len(pos)
            o0, g0, s0 = hoomd.halo_rows(pos, box, d, 0.0)
            assert np.array_equal(o0, owned) and len(g0) == 0 and s0.shape == (0, 3)
            assert len(hoomd.halo_rows(pos, box, d, (0.0, 0.0, 0.0))[1]) == 0


def test_with_two_dimensions_z_has_no_say():
    rng = np.random.default_rng(3)
    box = _triclinic_box(rng)
    box[4] = box[5] = 0.0
    pos = _positions(rng, box, 3000)
    moved = pos.copy()
    moved[:, 2] = rng.uniform(-50.0, 50.0, size=len(pos)).astype(np.float32)
    assert hoomd.ghost_fractions(box, 0.2, dimensions=2)[2] == 0.0
    for d in GRIDS["2x2x2"] + GRIDS["unequal"]:
        a = hoomd.halo_rows(pos, box, d, 0.2, dimensions=2)
        b = hoomd.halo_rows(moved, box, d, 0.2, dimensions=2)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert (a[2][:, 2] == 0).all() and len(a[1]) > 0
        flat = hoomd.Domain((d.lo[0], d.lo[1], 0.0), (d.hi[0], d.hi[1], 1.0))
        c = hoomd.halo_rows(pos, box, flat, 0.2, dimensions=2)
        assert all(np.array_equal(x, y) for x, y in zip(a, c))


def test_a_particle_near_a_face_is_a_ghost_of_the_face_neighbour():
    A, B = hoomd.domain_grid(2, 1, 1)
    f = np.array([[1 / 64, 0.3, 0.7],        # owned by A, next to B's upper face through the periodic boundary
                  [31 / 64, 0.3, 0.7],       # owned by A, just below the plane between A and B
                  [63 / 64, 0.3, 0.7],       # owned by B, next to A's lower face through the periodic boundary
                  [32 / 64, 0.3, 0.7],       # owned by B, on the plane
                  [16 / 64, 0.3, 0.7]])      # owned by A, out of B's reach
    pos = ((f - 0.5) * 16.0).astype(np.float32)
    oa, ga, sa = hoomd.halo_rows(pos, ORTHO, A, WIDTH)
    ob, gb, sb = hoomd.halo_rows(pos, ORTHO, B, WIDTH)
    assert oa.tolist() == [0, 1, 4] and ob.tolist() == [2, 3]
    assert gb.tolist() == [0, 1] and sb.tolist() == [[1, 0, 0], [0, 0, 0]]
    assert ga.tolist() == [2, 3] and sa.tolist() == [[-1, 0, 0], [0, 0, 0]]
    # the shift puts the ghost next to the cell: x' = x + sx * Lx lies within the layer of the cell's face
    x = pos[:, 0].astype(np.float64) + 8.0
    assert 16.0 <= x[0] + 16.0 * sb[0, 0] < 16.0 + WIDTH and -WIDTH <= x[2] + 16.0 * sa[0, 0] < 0.0


def test_bands_of_a_cell_at_the_box_faces_and_inside():
    bands, divided = hoomd.halo_bands(hoomd.Domain((0.0, 0.25, 0.0), (0.25, 0.75, 1.0)), (G, G, G))
    assert divided.tolist() == [1, 1, 0]
    assert bands[0].tolist() == [0.0, 0.0, 1.0 - G, 1.0, 0.25, 0.25 + G, 1.0, 0.0]
    assert bands[1].tolist() == [0.25 - G, 0.25, 1.0, 0.0, 0.75, 0.75 + G, 1.0, 0.0]
    assert bands[2].tolist() == [1.0, 0.0] * 4
    top = hoomd.halo_bands(hoomd.Domain((0.75, 0.0, 0.0), (1.0, 1.0, 1.0)), (G, G, G))[0][0]
    assert top.tolist() == [0.75 - G, 0.75, 1.0, 0.0, 1.0, 1.0, 0.0, G]


def test_ghost_fractions_against_hand_values():
    assert hoomd.ghost_fractions([16, 8, 4, 0, 0, 0], 1.0) == (1 / 16, 1 / 8, 1 / 4)
    assert hoomd.ghost_fractions([16, 8, 4, 0, 0, 0], 1.0, dimensions=2) == (1 / 16, 1 / 8, 0.0)
    assert hoomd.ghost_fractions([16, 8, 0, 0, 0, 0], 0.5, dimensions=2) == (1 / 32, 1 / 16, 0.0)
    # xy = 0.5, xz = 0.5, yz = 0.75: xy*yz - xz = -0.125, 1 + 0.25 + 0.015625 = 1.125^2; 1 + 0.5625 = 1.25^2
    gx, gy, gz = hoomd.ghost_fractions([9.0, 10.0, 4.0, 0.5, 0.5, 0.75], 2.0)
    assert (gx, gy, gz) == (2.0 * 1.125 / 9.0, 2.0 * 1.25 / 10.0, 0.5)
    gx, gy, gz = hoomd.ghost_fractions([10.0, 10.0, 10.0, 1.0, 0.0, 0.0], 1.0)
    assert gx == 1.0 / (10.0 / np.sqrt(2.0)) and gy == 0.1 and gz == 0.1
    assert hoomd.ghost_fractions(ORTHO, 0.0) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("width", [-1.0, -1e-300, float('nan'), float('inf')])
def test_a_negative_or_non_finite_width_is_refused(width):
    with pytest.raises(ValueError):
        hoomd.ghost_fractions(ORTHO, width)
    pos = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError):
        hoomd.halo_rows(pos, ORTHO, GRIDS["2x2x2"][0], width)
    with pytest.raises(ValueError):
        hoomd.halo_rows(pos, ORTHO, GRIDS["2x2x2"][0], (0.01, width, 0.01))


def test_a_layer_that_would_show_a_particle_twice_is_refused():
    pos = np.zeros((4, 3), np.float32)
    cell = hoomd.domain_grid(2, 1, 1)[0]                   # 1 - (hi - lo) = 0.5 on x
    hoomd.halo_rows(pos, ORTHO, cell, (0.25, 0.9, 0.9))    # 2g == 0.5 is legal; y and z are undivided
    with pytest.raises(ValueError, match="axis x"):
        hoomd.halo_rows(pos, ORTHO, cell, (0.2500001, 0.0, 0.0))
    with pytest.raises(ValueError, match="axis z"):
        hoomd.halo_rows(pos, ORTHO, GRIDS["unequal"][0], (0.0, 0.0, 0.32))      # z cell [0, 0.375): 0.64 > 0.625
    with pytest.raises(ValueError, match="axis x"):
        hoomd.halo_rows(pos, ORTHO, cell, 4.5)             # a width of 4.5 in a box of 16: g = 0.28125


def test_ghost_goes_with_domain_only(tmp_path):
    path = str(tmp_path / "t.gsd")
    fr = hoomd.Frame()
    fr.configuration.box = ORTHO
    fr.particles.N = 4
    fr.particles.position = np.zeros((4, 3), np.float32)
    with hoomd.open(path, 'w') as t:
        t.append(fr)
    cell = GRIDS["2x2x2"][0]
    with hoomd.open(path, 'r') as t:
        with pytest.raises(ValueError, match="ghost"):
            t.read_frame_device(0, ghost=1.0)
        with pytest.raises(ValueError, match="ghost"):
            t.read_frame_device(0, part=(0, 2), ghost=1.0)
        with pytest.raises(ValueError, match="ghost"):
            t.read_frame_device(0, part=(0, 2), domain=cell, ghost=1.0)
        with pytest.raises(ValueError, match="ghost"):
            t.read_frame_device(0, where={'typeid': [0]}, ghost=1.0)
        with pytest.raises(ValueError, match="ghost"):
            t.read_frame_device(0, where={'typeid': [0]}, domain=cell, ghost=1.0)
