"""The host models of the cell-ordered restart read: pgsd.hoomd.cell_ids (a row's cell in a uniform grid over the wrapped
fractions the selections compare), cell_order (the stable sort of a row list by that id, the ghost run on its own) and
cell_grid_for (the grid for an interaction range).  They are the definitions the GPU ordering is tested against, so they
are checked here against plain row loops and hand values.  No GPU."""
import math

import numpy as np
import pytest

import pgsd.hoomd as hoomd

ORTHO = np.array([16.0, 16.0, 16.0, 0.0, 0.0, 0.0], np.float32)
TRI = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
FLAT = np.array([4.0, 4.0, 1.0, 0.5, 0.0, 0.0], np.float32)


def lattice(rng, N):
    """Points of the 1/64 lattice of fractions in the 16^3 box, periodic images included (tests/test_gpu_census.py)."""
    k = rng.integers(0, 64, size=(N, 3))
    k[:64] = np.arange(64)[:min(N, 64), None]
    p = (k / 64.0 + rng.integers(-1, 2, size=(N, 3)) - 0.5) * 16.0
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32)


def loop_ids(position, box, cells, dimensions=3):
    """cell_ids one row and one axis at a time, in Python floats (IEEE float64, one rounding per operation)."""
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in np.asarray(box, np.float32)[:6])
    out = []
    for x, y, z in np.asarray(position, dtype=np.float64).reshape(-1, 3).tolist():
        s = [((x + Lx / 2) - ((xz - yz * xy) * z + xy * y)) / Lx, ((y + Ly / 2) - yz * z) / Ly,
             ((z + Lz / 2) / Lz) if dimensions == 3 else 0.0]
        cell, stride, nowhere = 0, 1, False
        for a in range(dimensions):
            if s[a] != s[a] or math.isinf(s[a]):
                nowhere = True
                continue
            f = s[a] - math.floor(s[a])
            if f >= 1.0:
                f = 0.0
            cell += min(int(f * cells[a]), cells[a] - 1) * stride
            stride *= cells[a]
        out.append(cells[0] * cells[1] * cells[2] if nowhere else cell)
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("cells", [(64, 64, 64), (3, 1, 2), (1024, 1024, 1024)])
def test_cell_ids_of_lattice_points(cells):
    pos = lattice(np.random.default_rng(1), 3000)
    got = hoomd.cell_ids(pos, ORTHO, cells)
    assert got.dtype == np.int64 and got.shape == (3000,)
    assert np.array_equal(got, loop_ids(pos, ORTHO, cells))
    assert got.min() >= 0 and got.max() < cells[0] * cells[1] * cells[2]
    if cells == (64, 64, 64):
        # a lattice point IS a cell corner: the id is the lattice index, exactly
        f = hoomd._wrapped_fractions(pos, ORTHO, 3)
        k = [np.rint(v * 64).astype(np.int64) for v in f]
        assert np.array_equal(got, k[0] + 64 * (k[1] + 64 * k[2]))
        assert len(set(got[:64].tolist())) == 64


@pytest.mark.parametrize("cells", [(2, 2, 2), (7, 5, 3), (1024, 1024, 1024)])
def test_cell_ids_of_random_rows_in_a_triclinic_box(cells):
    pos = np.random.default_rng(2).uniform(-3.0, 3.0, size=(2000, 3)).astype(np.float32)
    assert np.array_equal(hoomd.cell_ids(pos, TRI, cells), loop_ids(pos, TRI, cells))
    p64 = pos.astype(np.float64) * (1.0 + 2.0 ** -40)
    assert np.array_equal(hoomd.cell_ids(p64, TRI, cells), loop_ids(p64, TRI, cells))


def test_cell_ids_agree_with_the_domain_grid():
    """An equal 2 x 2 x 2 grid's cell r holds exactly domain_rows(domain_grid(2, 2, 2)[r])."""
    pos = np.random.default_rng(3).uniform(-3.0, 3.0, size=(5000, 3)).astype(np.float32)
    ids = hoomd.cell_ids(pos, TRI, (2, 2, 2))
    for r, d in enumerate(hoomd.domain_grid(2, 2, 2)):
        assert np.array_equal(np.flatnonzero(ids == r), hoomd.domain_rows(pos, TRI, d))


def test_nan_and_infinite_rows_get_the_nowhere_id():
    pos = np.random.default_rng(4).uniform(-3.0, 3.0, size=(400, 3)).astype(np.float32)
    pos[::7] = np.nan
    pos[1::11, 2] = np.inf
    pos[2::13, 0] = -np.inf
    pos[3::17, 1] = np.nan
    cells = (16, 16, 1)
    got = hoomd.cell_ids(pos, TRI, cells)
    assert np.array_equal(got, loop_ids(pos, TRI, cells))
    bad = ~np.isfinite(pos).all(axis=1)
    assert (got[bad] == 256).all() and (got[~bad] < 256).all() and bad.sum() > 50


def test_two_dimensions_do_not_look_at_z():
    rng = np.random.default_rng(5)
    pos = rng.uniform(-3.0, 3.0, size=(1000, 3)).astype(np.float32)
    got = hoomd.cell_ids(pos, FLAT, (5, 4, 1), dimensions=2)
    assert np.array_equal(got, loop_ids(pos, FLAT, (5, 4, 1), dimensions=2))
    other = pos.copy()
    other[:, 2] = 7.0                               # (finite: with xz = yz = 0 it enters no fraction)
    assert np.array_equal(hoomd.cell_ids(other, FLAT, (5, 4, 1), dimensions=2), got) and got.max() < 20


def test_the_clamp_never_binds():
    """f <= 1 - 2^-53 and c <= 1024: the float64 product rounds below c, so int(f * c) is c - 1 at most."""
    f = np.nextafter(1.0, 0.0)
    assert f == 1.0 - 2.0 ** -53
    for c in range(1, 1025):
        assert int(f * c) == c - 1
        assert int((np.float64(f) * np.float64(c))) == c - 1


def test_cell_order_is_the_stable_argsort():
    rng = np.random.default_rng(6)
    pos = rng.uniform(-3.0, 3.0, size=(3000, 3)).astype(np.float32)
    rows = np.sort(rng.choice(3000, size=1200, replace=False))
    cells = (3, 2, 2)
    got_rows, got_cell, perm = hoomd.cell_order(pos, TRI, rows, cells)
    ids = hoomd.cell_ids(pos[rows], TRI, cells)
    want = np.argsort(ids, kind='stable')
    assert np.array_equal(perm, want) and np.array_equal(got_rows, rows[want]) and np.array_equal(got_cell, ids[want])
    assert (np.diff(got_cell) >= 0).all()
    for c in range(12):                             # rows of one cell stay ascending
        assert (np.diff(got_rows[got_cell == c]) > 0).all()
    # a list in any order, with repeats: equal cells keep their LIST order
    rows = rng.integers(0, 3000, size=2000)
    got_rows, got_cell, perm = hoomd.cell_order(pos, TRI, rows, cells)
    for c in range(12):
        assert (np.diff(perm[got_cell == c]) > 0).all()
    assert np.array_equal(np.sort(perm), np.arange(2000)) and np.array_equal(got_rows, rows[perm])


def test_cell_order_keeps_the_owned_and_the_ghost_run_apart():
    rng = np.random.default_rng(7)
    pos = rng.uniform(-3.0, 3.0, size=(4000, 3)).astype(np.float32)
    d = hoomd.domain_grid(2, 2, 2)[5]
    owned, ghosts, shift = hoomd.halo_rows(pos, TRI, d, 0.3)
    assert len(ghosts) > 100 and shift.any()
    rows = np.concatenate((owned, ghosts))
    cells = (4, 4, 4)
    got_rows, got_cell, perm = hoomd.cell_order(pos, TRI, rows, cells, n_owned=len(owned))
    n = len(owned)
    assert np.array_equal(np.sort(got_rows[:n]), owned) and np.array_equal(np.sort(got_rows[n:]), ghosts)
    assert (perm[:n] < n).all() and (perm[n:] >= n).all()
    assert (np.diff(got_cell[:n]) >= 0).all() and (np.diff(got_cell[n:]) >= 0).all()
    assert got_cell[n] < got_cell[n - 1]            # the ghost run starts over
    assert np.array_equal(perm[:n], np.argsort(hoomd.cell_ids(pos[owned], TRI, cells), kind='stable'))
    assert np.array_equal(perm[n:] - n, np.argsort(hoomd.cell_ids(pos[ghosts], TRI, cells), kind='stable'))
    # the shift rows follow their ghosts
    shift_sorted = shift[perm[n:] - n]
    by_row = dict(zip(ghosts.tolist(), shift.tolist()))
    assert [by_row[r] for r in got_rows[n:].tolist()] == shift_sorted.tolist()


def test_cell_order_of_an_empty_list():
    pos = np.zeros((10, 3), np.float32)
    for n_owned in (None, 0):
        rows, cell, perm = hoomd.cell_order(pos, TRI, np.zeros(0, np.int64), (2, 2, 2), n_owned=n_owned)
        assert rows.shape == cell.shape == perm.shape == (0,) and rows.dtype == cell.dtype == perm.dtype == np.int64
    rows, cell, perm = hoomd.cell_order(np.zeros((0, 3), np.float32), TRI, [], (1, 1, 1))
    assert len(rows) == 0


def test_cell_grid_for_hand_values():
    # orthorhombic 16^3: the plane distances are the lengths
    assert hoomd.cell_grid_for(ORTHO, 1.0) == (16, 16, 16)
    assert hoomd.cell_grid_for(ORTHO, 3.0) == (5, 5, 5)
    assert hoomd.cell_grid_for(ORTHO, 16.0) == (1, 1, 1)
    assert hoomd.cell_grid_for(ORTHO, 100.0) == (1, 1, 1)
    assert hoomd.cell_grid_for(ORTHO, 0.001) == (1024, 1024, 1024)
    assert hoomd.cell_grid_for(ORTHO, 0.0) == (1024, 1024, 1024)
    assert hoomd.cell_grid_for(ORTHO, 1.0, dimensions=2) == (16, 16, 1)
    # triclinic: npd_x = 4 / sqrt(1 + 0.25 + (0.5 * -0.125 - 0.25)^2) = 3.4456..., npd_y = 4 / sqrt(1 + 1/64) = 3.9691...,
    # npd_z = 2
    npd = (4.0 / math.sqrt(1.0 + 0.25 + (0.5 * -0.125 - 0.25) ** 2), 4.0 / math.sqrt(1.0 + 0.125 ** 2), 2.0)
    assert [round(v, 3) for v in npd] == [3.446, 3.969, 2.0]
    assert hoomd.cell_grid_for(TRI, 0.5) == (6, 7, 4)
    assert hoomd.cell_grid_for(TRI, 1.0) == (3, 3, 2)
    # no narrower than the width: c cells of fraction 1 / c >= g
    g = hoomd.ghost_fractions(TRI, 0.3)
    c = hoomd.cell_grid_for(TRI, 0.3)
    assert all(1.0 / c[a] >= g[a] > 1.0 / (c[a] + 1) for a in range(3))


def test_every_value_error():
    pos = np.zeros((10, 3), np.float32)
    for cells in ((0, 1, 1), (1, 1025, 1), (1, 1, -1), (2, 2), (1, 1, 1, 1)):
        with pytest.raises(ValueError, match="1 to 1024"):
            hoomd.cell_ids(pos, TRI, cells)
        with pytest.raises(ValueError, match="1 to 1024"):
            hoomd.cell_order(pos, TRI, [0, 1], cells)
    with pytest.raises(ValueError, match="cz == 1"):
        hoomd.cell_ids(pos, FLAT, (2, 2, 2), dimensions=2)
    with pytest.raises(ValueError, match="dimensions"):
        hoomd.cell_ids(pos, TRI, (2, 2, 2), dimensions=4)
    with pytest.raises(ValueError, match="box lengths"):
        hoomd.cell_ids(pos, [0, 1, 1, 0, 0, 0], (2, 2, 2))
    with pytest.raises(ValueError, match="6 values"):
        hoomd.cell_ids(pos, [1, 1, 1], (2, 2, 2))
    with pytest.raises(ValueError, match="n_owned"):
        hoomd.cell_order(pos, TRI, [0, 1, 2], (2, 2, 2), n_owned=4)
    with pytest.raises(ValueError, match="n_owned"):
        hoomd.cell_order(pos, TRI, [0, 1, 2], (2, 2, 2), n_owned=-1)
    for rows in ([0, 10], [-1, 2]):
        with pytest.raises(ValueError, match="outside"):
            hoomd.cell_order(pos, TRI, rows, (2, 2, 2))
    with pytest.raises(ValueError, match="finite"):
        hoomd.cell_grid_for(TRI, -1.0)
    with pytest.raises(ValueError, match="finite"):
        hoomd.cell_grid_for(TRI, float('inf'))
    with pytest.raises(ValueError, match="dimensions"):
        hoomd.cell_grid_for(TRI, 1.0, dimensions=1)


def test_read_frame_device_refuses_cell_order_without_a_selection(tmp_path):
    """The keyword's own checks come before anything touches a GPU."""
    path = str(tmp_path / "t.gsd")
    fr = hoomd.Frame()
    fr.particles.N = 4
    fr.particles.position = np.zeros((4, 3), np.float32)
    with hoomd.open(path, 'w') as t:
        t.append(fr)
    with hoomd.open(path, 'r') as t:
        with pytest.raises(ValueError, match="cell_order needs domain or where"):
            t.read_frame_device(0, cell_order=(2, 2, 2))
        with pytest.raises(ValueError, match="cell_order needs domain or where"):
            t.read_frame_device(0, part=(0, 2), cell_order=(2, 2, 2))
        with pytest.raises(ValueError, match="1 to 1024"):
            t.read_frame_device(0, domain=hoomd.domain_grid(1, 1, 1)[0], cell_order=(2, 2, 0))
