"""The neighbour census model (`pgsd.hoomd.particle_neighbours`, `pair_distance2`, `neighbour_grid_for`,
`frame_neighbours`) against a plain double loop with the adjacency rule, against a search over all pairs without cells,
and against each mutation of the loop that stands for a kernel mistake (`neighbours_cases.py`).  No GPU."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

from neighbours_cases import (FLAT, MUTATIONS, NONE, ORTHO, TRICLINIC, brute_force, loop_neighbours, random_rows, same)

BOXES = {'orthorhombic': (ORTHO, 3), 'triclinic': (TRICLINIC, 3), 'flat': (FLAT, 2)}


# ---------------------------------------------------------------- the arithmetic of one pair
def test_pair_distance2_by_hand():
    v = hoomd.box_vectors(np.asarray(TRICLINIC, np.float32))         # (10, 8, 6, 2.4, -1.2, 2.4) from the stored float32 box
    assert v.tolist() == [10.0, 8.0, 6.0, float(np.float32(0.3)) * 8, float(np.float32(-0.2)) * 6, float(np.float32(0.4)) * 6]
    # no shift
    assert hoomd.pair_distance2([0, 0, 0], [1, 2, 2], v) == 9.0
    # z first: d_z = 3 is the half box exactly (>=: shifted down), and the shift carries its x and y terms
    d2 = hoomd.pair_distance2(np.zeros(3), np.array([0.0, 0.0, 3.0]), v)
    dx, dy, dz = 0.0 - v[4], 0.0 - v[5], 3.0 - 6.0
    assert d2 == (dx * dx + dy * dy) + dz * dz
    # -Lz/2 is not below -(Lz/2): no shift
    assert hoomd.pair_distance2(np.zeros(3), np.array([0.0, 0.0, -3.0]), v) == 9.0
    # two dimensions: z is never looked at
    assert hoomd.pair_distance2([0, 0, 0], [0.5, 0, 77.0], hoomd.box_vectors(FLAT), dimensions=2) == 0.25
    # float32 rows are converted exactly, and the call broadcasts
    a = np.array([[0.1, 0.2, 0.3]], np.float32)
    b = np.array([[0.4, 0.1, 0.2], [4.9, 3.9, 2.9]], np.float32)
    got = hoomd.pair_distance2(a, b, hoomd.box_vectors(ORTHO))
    d = b.astype(np.float64) - a.astype(np.float64)
    assert got.shape == (2,) and got[0] == (d[0, 0] * d[0, 0] + d[0, 1] * d[0, 1]) + d[0, 2] * d[0, 2]
    with pytest.raises(ValueError):
        hoomd.pair_distance2(a, b, [1, 2, 3])
    with pytest.raises(ValueError):
        hoomd.pair_distance2(a, b, v, dimensions=4)


def test_a_position_more_than_one_image_outside_is_not_folded_fully():
    """HOOMD's range of validity: one shift per axis."""
    v = hoomd.box_vectors([8, 8, 8, 0, 0, 0])
    assert hoomd.pair_distance2([0, 0, 0], [16.5, 0, 0], v) == 8.5 * 8.5


# ---------------------------------------------------------------- the grid
def test_neighbour_grid_for_and_its_coarsening():
    assert hoomd.neighbour_grid_for(ORTHO, 1.3) == hoomd.cell_grid_for(ORTHO, 1.3) == (7, 6, 4)
    assert hoomd.neighbour_grid_for(FLAT, 0.6, 2) == hoomd.cell_grid_for(FLAT, 0.6, 2)
    big = [1000, 800, 600, 0, 0, 0]
    assert hoomd.cell_grid_for(big, 1.0) == (1000, 800, 600)
    # 1000 -> 500, 800 -> 400, 600 -> 300, 500 -> 250, 400 -> 200, 300 -> 150, 250 -> 125, 200 -> 100, 150 -> 75: 937 500 cells
    assert hoomd.neighbour_grid_for(big, 1.0) == (125, 100, 75)
    # a tie takes the lowest axis; an odd count rounds up
    cube = [303, 303, 303, 0, 0, 0]
    assert hoomd.cell_grid_for(cube, 1.0) == (303, 303, 303)
    assert hoomd.neighbour_grid_for(cube, 1.0) == (76, 76, 152)    # 303 -> 152 three times, then x and y -> 76
    for box, r in ((big, 1.0), (cube, 1.0)):
        g, widest = hoomd.neighbour_grid_for(box, r), hoomd.cell_grid_for(box, r)
        assert g[0] * g[1] * g[2] <= 2 ** 20 and all(g[a] <= widest[a] for a in range(3))


def test_what_particle_neighbours_refuses():
    p = random_rows(1, 10, ORTHO)
    for r in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match="finite and positive"):
            hoomd.particle_neighbours(p, ORTHO, r)
        with pytest.raises(ValueError, match="finite and positive"):
            hoomd.neighbour_grid_for(ORTHO, r)
    with pytest.raises(ValueError, match="narrower"):
        hoomd.particle_neighbours(p, ORTHO, 1.3, cells=(8, 6, 4))
    with pytest.raises(ValueError, match="narrower"):
        hoomd.particle_neighbours(p, TRICLINIC, 1.3, cells=hoomd.cell_grid_for(ORTHO, 1.3))    # the tilt narrows x
    with pytest.raises(ValueError, match="2\\^20"):
        hoomd.particle_neighbours(p, [1000, 800, 600, 0, 0, 0], 1.0, cells=(1000, 800, 600))
    with pytest.raises(ValueError, match="count twice"):
        hoomd.particle_neighbours(p, ORTHO, 3.01)              # above Lz / 2
    hoomd.particle_neighbours(p, ORTHO, 3.0)                   # half the nearest plane distance itself is allowed
    hoomd.particle_neighbours(p, FLAT, 3.4, dimensions=2)      # z does not take part: Lz = 1 bounds nothing
    with pytest.raises(ValueError, match="count twice"):
        hoomd.particle_neighbours(p, FLAT, 3.4)
    with pytest.raises(ValueError, match="cz == 1"):
        hoomd.particle_neighbours(p, FLAT, 0.5, cells=(3, 2, 2), dimensions=2)
    for bins in (-1, 1025):
        with pytest.raises(ValueError, match="bins"):
            hoomd.particle_neighbours(p, ORTHO, 1.0, bins=bins)
    with pytest.raises(ValueError, match="outside the position array"):
        hoomd.particle_neighbours(p, ORTHO, 1.0, rows=[0, 10])
    with pytest.raises(ValueError, match="float32 or float64"):
        hoomd.particle_neighbours(np.zeros((4, 3), np.int32), ORTHO, 1.0)


# ---------------------------------------------------------------- the model against the loop and against brute force
@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_model_equals_the_double_loop(name, dtype):
    """A list with repeats and a nowhere entry, over the automatic grid and over coarse ones (two cells and one cell on
    an axis), with a pair histogram."""
    box, dims = BOXES[name]
    p = random_rows(3, 150, box, dtype, dims)
    p[7] = np.nan
    rows = np.concatenate([np.arange(150), [5, 5, 149]])
    for r, cells in ((0.6, None), (1.3, None), (2.9, (3, 2, 2) if dims == 3 else (3, 2, 1)), (1.3, (1, 2, 1))):
        want = loop_neighbours(p, box, r, rows, cells, dims, bins=5)
        got = hoomd.particle_neighbours(p, box, r, rows=rows, cells=cells, dimensions=dims, bins=5)
        assert same(got, want), (name, r, cells)
        assert got.nowhere == 1 and got.n == 153 and got.closest2 == 0.0      # the repeated row


@pytest.mark.parametrize("name", sorted(BOXES))
def test_the_model_equals_a_search_over_all_pairs(name):
    """600 uniformly random float32 rows, r in {0.6, 1.3, 2.9}: counts and nearest d2 equal brute force exactly."""
    box, dims = BOXES[name]
    p = random_rows(11, 600, box, np.float32, dims)
    for r in (0.6, 1.3, 2.9):
        got = hoomd.particle_neighbours(p, box, r, dimensions=dims)
        count, nearest2 = brute_force(p, box, r, dims)
        assert np.array_equal(got.count, count[got.rows]), (name, r)
        assert np.array_equal(got.nearest2.view(np.uint64), nearest2[got.rows].view(np.uint64)), (name, r)
        assert got.pairs == int(count.sum()) and got.closest2 == nearest2.min()
        assert got.count_min == count.min() and got.count_max == count.max()
        assert got.isolated == int((count == 0).sum()) and got.mean_count == count.sum() / 600


def test_the_steps_of_the_model_do_not_show(monkeypatch):
    """The model expands candidates in steps of at most 2^22; a step of 50 gives the same result."""
    p = random_rows(4, 300, TRICLINIC)
    want = hoomd.particle_neighbours(p, TRICLINIC, 1.3, bins=3)
    monkeypatch.setattr(hoomd, '_NEIGHBOURS_PAIRS_PER_STEP', 50)
    got = hoomd.particle_neighbours(p, TRICLINIC, 1.3, bins=3)
    assert same(got, (want.summary, want.closest2, want.count, want.nearest2, want.nearest))


def test_nothing_one_entry_and_everything_nowhere():
    got = hoomd.particle_neighbours(np.zeros((0, 3), np.float32), ORTHO, 1.0, bins=4)
    assert got.n == 0 and got.pairs == 0 and got.closest == NONE and got.closest_rows is None and got.closest2 == np.inf
    assert got.count_hist.sum() == 0 and got.pair_hist.tolist() == [0] * 4 and np.isnan(got.mean_count)
    one = hoomd.particle_neighbours(np.ones((1, 3), np.float32), ORTHO, 1.0)
    assert one.count.tolist() == [0] and one.nearest.tolist() == [NONE] and one.isolated == 1 and one.count_min == 0
    lost = hoomd.particle_neighbours(np.full((5, 3), np.nan, np.float32), ORTHO, 1.0)
    assert lost.nowhere == 5 and lost.count.tolist() == [0] * 5 and lost.count_hist.sum() == 0 and lost.count_max == 0
    assert np.isinf(lost.nearest2).all() and (lost.nearest == NONE).all() and lost.closest_rows is None


def test_the_count_histogram_saturates_at_256():
    """A clump of 300 rows on one spot: every entry has 299 neighbours, all in bin 256."""
    p = np.tile(np.array([[1, 1, 1]], np.float32), (300, 1))
    got = hoomd.particle_neighbours(p, ORTHO, 1.0)
    assert got.count_hist[256] == 300 and got.count_hist[:256].sum() == 0 and got.count_min == got.count_max == 299
    assert got.pairs == 300 * 299 and got.closest2 == 0.0 and got.closest == 0 and got.closest_rows == (0, 1)
    assert got.nearest[:3].tolist() == [1, 0, 0]


# ---------------------------------------------------------------- the pair histogram
def test_pair_hist_edges_with_a_pair_exactly_on_an_edge():
    edges2 = hoomd.neighbour_edges2(1.0, 4)
    assert edges2.tolist() == [0.0, 0.0625, 0.25, 0.5625, 1.0]
    r = 0.7
    e = hoomd.neighbour_edges2(r, 7)
    w = np.float64(r) / np.float64(7)
    assert e[7] == np.float64(r) * np.float64(r) and all(e[k] == (k * w) ** 2 for k in range(7))
    # pairs at distance 0.25 (an edge: the bin above), 0.5 (an edge), 0.6 and 0 (the first edge)
    p = np.array([[0, 0, 0], [0.25, 0, 0], [2, 0, 0], [2, 0.5, 0], [0, 2, 0], [0, 2, 0.6], [3, 3, 2], [3, 3, 2]], np.float32)
    got = hoomd.particle_neighbours(p, ORTHO, 1.0, bins=4)
    d2 = float(np.float64(np.float32(0.6)) ** 2)
    assert got.pair_hist.tolist() == [2, 2, 2 + (2 if d2 < 0.5625 else 0), 2 if d2 >= 0.5625 else 0]
    assert got.pair_hist.sum() == got.pairs == 8
    mid, g = got.rdf(10 * 8 * 6)
    e = np.sqrt(edges2)
    shell = 4.0 / 3.0 * np.pi * (e[1:] ** 3 - e[:-1] ** 3)
    assert np.allclose(mid, 0.5 * (e[1:] + e[:-1])) and np.allclose(g, got.pair_hist / (8 * (8 / 480.0) * shell))
    flat = hoomd.particle_neighbours(p, FLAT, 1.0, dimensions=2, bins=4)
    _, g2 = flat.rdf(63.0)
    assert np.allclose(g2, flat.pair_hist / (8 * (8 / 63.0) * np.pi * (e[1:] ** 2 - e[:-1] ** 2)))
    with pytest.raises(ValueError, match="bins"):
        hoomd.particle_neighbours(p, ORTHO, 1.0).rdf(1.0)


# ---------------------------------------------------------------- the frame level
def test_frame_neighbours_over_selections():
    p = random_rows(8, 400, TRICLINIC)
    typeid = (np.arange(400) % 3).astype(np.uint32)
    arrays = dict(position=p, typeid=typeid)
    got = hoomd.frame_neighbours(arrays, 1.3, where={'type': ['b']}, types=['a', 'b', 'c'], box=TRICLINIC)
    rows = np.flatnonzero(typeid == 1)
    assert same(got, loop_neighbours(p, TRICLINIC, 1.3, rows))
    dom = hoomd.Domain((0, 0, 0), (0.5, 1, 1))
    got = hoomd.frame_neighbours(arrays, 1.3, bins=3, domain=dom, box=TRICLINIC)
    want = hoomd.particle_neighbours(p, TRICLINIC, 1.3, rows=hoomd.domain_rows(p, TRICLINIC, dom), bins=3)
    assert np.array_equal(got.summary, want.summary) and got.n == len(hoomd.domain_rows(p, TRICLINIC, dom))
    both = hoomd.frame_neighbours(arrays, 1.3, where={'type': ['b']}, types=['a', 'b', 'c'], domain=dom, box=TRICLINIC)
    assert both.n == len(np.intersect1d(rows, hoomd.domain_rows(p, TRICLINIC, dom)))
    with pytest.raises(ValueError, match="box"):
        hoomd.frame_neighbours(arrays, 1.3)
    fr = hoomd.Frame()
    fr.configuration.box = FLAT
    fr.configuration.dimensions = 2
    fr.particles.N = 400
    fr.particles.position = random_rows(9, 400, FLAT, dimensions=2)
    got = hoomd.frame_neighbours(fr, 0.6, cells=(3, 2, 1))
    assert got.dimensions == 2 and got.grid == (3, 2, 1)
    assert same(got, loop_neighbours(fr.particles.position, FLAT, 0.6, None, (3, 2, 1), 2))


def test_neighbours_has_slots_and_a_summary_that_round_trips():
    got = hoomd.particle_neighbours(random_rows(2, 50, ORTHO), ORTHO, 2.0, bins=2)
    with pytest.raises(AttributeError):
        got.other = 1
    again = hoomd.Neighbours(got.r, got.bins, got.grid, got.dimensions, got.summary, got.closest2)
    assert np.array_equal(again.summary, got.summary) and again.count is None and again.closest_rows == got.closest_rows
    assert got.closest_distance == np.sqrt(got.closest2) and "Neighbours(r=2.0" in repr(got)
    with pytest.raises(ValueError, match="words"):
        hoomd.Neighbours(1.0, 3, None, 3, got.summary, 0.0)


# ---------------------------------------------------------------- mutations
@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_every_mutation_is_caught(name):
    switch, case = MUTATIONS[name]
    got = hoomd.particle_neighbours(**case)
    assert not same(got, loop_neighbours(**case, **switch)), "the mutation does not show on its case"
    # ... and the loop without the mutation agrees, so the difference is the mutation's
    assert same(got, loop_neighbours(**case))


# ---------------------------------------------------------------- the command line
def test_the_command_line_prints_the_neighbour_summary(tmp_path, capsys):
    path = str(tmp_path / "small.gsd")
    with hoomd.open(path, 'w') as t:
        fr = hoomd.Frame()
        fr.configuration.box = [8, 8, 8, 0, 0, 0]
        fr.particles.N = 6
        fr.particles.types = ['fluid', 'wall']
        fr.particles.typeid = np.array([0, 0, 1, 0, 0, 0], np.uint32)
        fr.particles.position = np.array([[1, 1, 1], [1.5, 1, 1], [1, 1.25, 1], [-3.9, 0, 0], [3.9, 0, 0], [np.nan, 0, 0]],
                                         np.float32)
        t.append(fr)
    assert pgsd_main(['info', path, '--neighbours', '1.0', '--bins', '2']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "neighbours of frame 0 inside 1.0 over 8 x 8 x 8 cells:" in lines
    assert "entries: 6 nowhere: 1" in lines
    assert "count: mean 1.6 smallest 1 largest 2" in lines and "isolated: 0" in lines
    assert "closest pair: rows 3 and 4 at distance 0.1999998" in [l[:len("closest pair: rows 3 and 4 at distance 0.1999998")] for l in lines]
    assert "g(r):" in lines and sum(l.startswith("0.") for l in lines) == 2
    assert pgsd_main(['info', path, '--neighbours', '1.0', '--types', 'fluid']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "neighbours of frame 0 inside 1.0 over 8 x 8 x 8 cells (types fluid):" in lines
    assert "entries: 5 nowhere: 1" in lines and "isolated: 0" in lines
    assert pgsd_main(['info', path, '--neighbours', '5.0']) == 1
    assert "count twice" in capsys.readouterr().err
