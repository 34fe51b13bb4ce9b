"""The numpy model of a spatial domain read (pgsd.hoomd.Domain / domain_grid / domain_rows): the definition the GPU
selection of read_frame_device(domain=...) must match bit for bit (tests/test_gpu_read_domain.py).  CPU only."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd


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


@pytest.mark.parametrize("seed", range(6))
def test_every_row_lies_in_exactly_one_domain(seed):
    rng = np.random.default_rng(seed)
    box = _triclinic_box(rng)
    pos = _positions(rng, box, 5000)
    nx, ny, nz = (int(v) for v in rng.integers(1, 5, size=3))
    splits = []
    for n in (nx, ny, nz):
        if n > 1 and rng.random() < 0.7:
            w = rng.uniform(0.2, 1.0, size=n)
            splits.append(list(w[:-1] / w.sum()))          # uneven cells
        else:
            splits.append(None)
    grid = hoomd.domain_grid(nx, ny, nz, *splits)
    assert len(grid) == nx * ny * nz
    owners = np.zeros(len(pos), dtype=np.int64)
    for d in grid:
        owners[hoomd.domain_rows(pos, box, d)] += 1
    assert (owners == 1).all()
    rows = np.concatenate([hoomd.domain_rows(pos, box, d) for d in grid])
    assert np.array_equal(np.sort(rows), np.arange(len(pos)))


def test_rows_are_ascending_and_float64_positions_are_taken_as_they_are():
    rng = np.random.default_rng(7)
    box = _triclinic_box(rng)
    pos = _positions(rng, box, 2000).astype(np.float64) + 1e-9
    d = hoomd.domain_grid(2, 2, 2)[5]
    rows = hoomd.domain_rows(pos, box, d)
    assert len(rows) > 0 and (np.diff(rows) > 0).all()


def test_split_plane_belongs_to_the_upper_cell():
    box = np.array([4.0, 4.0, 4.0, 0.0, 0.0, 0.0], np.float32)
    grid = hoomd.domain_grid(2, 1, 1)
    on_plane = np.array([[0.0, 0.3, -0.2]], np.float32)      # sx == 0.5 exactly
    assert len(hoomd.domain_rows(on_plane, box, grid[0])) == 0
    assert list(hoomd.domain_rows(on_plane, box, grid[1])) == [0]
    uneven = hoomd.domain_grid(1, 1, 2, z_split=[0.25])        # plane at sz == 0.25: z = -1.0
    assert uneven[0].hi[2] == 0.25 and uneven[1].lo[2] == 0.25
    p = np.array([[0.5, 0.5, -1.0]], np.float32)
    assert len(hoomd.domain_rows(p, box, uneven[0])) == 0
    assert list(hoomd.domain_rows(p, box, uneven[1])) == [0]


def test_box_edges_and_outside_positions_wrap():
    box = np.array([4.0, 2.0, 2.0, 0.0, 0.0, 0.0], np.float32)
    grid = hoomd.domain_grid(4, 1, 1)
    edge = np.array([[2.0, 0.0, 0.0]], np.float32)            # x = +Lx/2: sx == 1.0 -> 0.0, the first cell
    assert list(hoomd.domain_rows(edge, box, grid[0])) == [0]
    low = np.array([[-2.0, 0.0, 0.0]], np.float32)            # x = -Lx/2: sx == 0.0
    assert list(hoomd.domain_rows(low, box, grid[0])) == [0]
    outside = np.array([[2.5, 0.0, 0.0], [-2.5, 0.0, 0.0], [10.5, 0.0, 0.0]], np.float32)
    # 2.5 -> sx 1.125 -> 0.125 (cell 0); -2.5 -> -0.125 -> 0.875 (cell 3); 10.5 -> 3.125 -> 0.125 (cell 0)
    assert list(hoomd.domain_rows(outside, box, grid[0])) == [0, 2]
    assert list(hoomd.domain_rows(outside, box, grid[3])) == [1]
    # sx = (0 - xy * y) / Lx = -1.25e-31: s - floor(s) rounds to 1.0, which wraps to 0.0 (the first cell, not the last)
    tilted = np.array([4.0, 2.0, 2.0, 0.5, 0.0, 0.0], np.float32)
    tiny = np.array([[-2.0, 1e-30, 0.0]], np.float64)
    assert list(hoomd.domain_rows(tiny, tilted, grid[0])) == [0]
    assert len(hoomd.domain_rows(tiny, tilted, grid[3])) == 0


def test_two_dimensions_ignore_z():
    box = np.array([4.0, 4.0, 0.0, 0.3, 0.0, 0.0], np.float32)
    pos = np.array([[0.5, 0.5, 123.0], [0.5, 0.5, -7.0], [-1.0, -1.0, 0.0]], np.float32)
    grid = hoomd.domain_grid(2, 2, 1)
    got = [list(hoomd.domain_rows(pos, box, d, dimensions=2)) for d in grid]
    assert sorted(r for g in got for r in g) == [0, 1, 2]
    assert got[3] == [0, 1]
    with pytest.raises(ValueError):
        hoomd.domain_rows(pos, box, grid[0], dimensions=3)    # Lz == 0 in three dimensions


def test_rank_order_is_x_fastest():
    grid = hoomd.domain_grid(3, 2, 2)
    for rank, d in enumerate(grid):
        x, y, z = rank % 3, (rank // 3) % 2, rank // 6
        assert d.lo == pytest.approx((x / 3, y / 2, z / 2))
        assert d.hi == pytest.approx(((x + 1) / 3, (y + 1) / 2, (z + 1) / 2))
    assert grid[-1].hi == (1.0, 1.0, 1.0)
    split = hoomd.domain_grid(3, 1, 1, x_split=[0.5, 0.2])
    assert [d.lo[0] for d in split] == [0.0, 0.5, 0.7] and split[2].hi[0] == 1.0


@pytest.mark.parametrize("lo,hi", [((0, 0, 0), (0, 1, 1)), ((-0.1, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1.5, 1)),
                                   ((0.6, 0, 0), (0.4, 1, 1)), ((0, 0), (1, 1))])
def test_invalid_domains_raise(lo, hi):
    with pytest.raises(ValueError):
        hoomd.Domain(lo, hi)


def test_invalid_grids_and_boxes_raise():
    with pytest.raises(ValueError):
        hoomd.domain_grid(0, 1, 1)
    with pytest.raises(ValueError):
        hoomd.domain_grid(2, 1, 1, x_split=[0.5, 0.2])        # nx - 1 widths
    with pytest.raises(ValueError):
        hoomd.domain_grid(3, 1, 1, x_split=[0.6, 0.5])        # no room for the last cell
    with pytest.raises(ValueError):
        hoomd.domain_grid(2, 1, 1, x_split=[0.0])
    d = hoomd.Domain((0, 0, 0), (1, 1, 1))
    pos = np.zeros((3, 3), np.float32)
    for box in ([0, 1, 1, 0, 0, 0], [1, -1, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [np.nan, 1, 1, 0, 0, 0], [1, 1, 1]):
        with pytest.raises(ValueError):
            hoomd.domain_rows(pos, box, d)
    with pytest.raises(ValueError):
        hoomd.domain_rows(pos, [1, 1, 1, 0, 0, 0], d, dimensions=4)


def test_whole_box_domain_takes_everything_and_tuples_are_domains():
    rng = np.random.default_rng(3)
    box = _triclinic_box(rng)
    pos = _positions(rng, box, 1000)
    assert np.array_equal(hoomd.domain_rows(pos, box, ((0, 0, 0), (1, 1, 1))), np.arange(1000))
    assert len(hoomd.domain_rows(np.zeros((0, 3), np.float32), box, hoomd.domain_grid(1, 1, 1)[0])) == 0
