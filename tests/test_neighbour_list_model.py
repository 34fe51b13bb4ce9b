"""The neighbour list model (`pgsd.hoomd.neighbour_list`, `NeighbourList`, `frame_neighbour_list`) against a plain double
loop that walks the cells in the defined order, against each mutation of the loop that stands for a kernel mistake
(`neighbour_list_cases.py`), and against the census `pgsd.hoomd.particle_neighbours` of the same list.  No GPU."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

from neighbours_cases import FLAT, NONE, ORTHO, TRICLINIC, random_rows
from neighbour_list_cases import CUBE, MUTATIONS, loop_neighbour_list, same

BOXES = {'orthorhombic': (ORTHO, 3), 'triclinic': (TRICLINIC, 3), 'flat': (FLAT, 2)}


# ---------------------------------------------------------------- mutations
@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_every_mutation_is_caught(name):
    switch, case = MUTATIONS[name]
    got = hoomd.neighbour_list(distances=True, **case)
    assert not same(got, loop_neighbour_list(distances=True, **case, **switch)), "the mutation does not show on its case"
    # ... and the loop without the mutation agrees, so the difference is the mutation's
    assert same(got, loop_neighbour_list(distances=True, **case))


def test_the_order_cases_by_hand():
    """The three cases about the order, written out: positions are list positions."""
    got = hoomd.neighbour_list(**MUTATIONS['ox outermost instead of oz'][1])
    assert got.rows.tolist() == [1, 0, 2] and got.of(1).tolist() == [0, 2]             # oz = -1 before oz = +1
    got = hoomd.neighbour_list(**MUTATIONS['the x-runs of a wrapping row in memory order'][1])
    assert got.rows.tolist() == [0, 2, 1] and got.of(0).tolist() == [2, 1]             # cell cx - 1, then cell 1
    got = hoomd.neighbour_list(**MUTATIONS['descending inside a cell'][1])
    assert [got.of(k).tolist() for k in range(3)] == [[1, 2], [0, 2], [0, 1]]


# ---------------------------------------------------------------- the model against the loop
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_model_equals_the_double_loop(name, dtype, half):
    """A few hundred rows with repeats and a nowhere entry, over the automatic grid and over coarse ones (three, two and
    one cell on an axis)."""
    box, dims = BOXES[name]
    p = random_rows(3, 300, box, dtype, dims)
    p[7] = np.nan
    rows = np.concatenate([np.arange(300), [5, 5, 299]])
    for r, cells in ((0.6, None), (1.3, None), (2.9, (3, 2, 2) if dims == 3 else (3, 2, 1)), (1.3, (1, 2, 1))):
        want = loop_neighbour_list(p, box, r, rows, cells, dims, half=half, distances=True)
        got = hoomd.neighbour_list(p, box, r, rows=rows, cells=cells, dimensions=dims, half=half, distances=True)
        assert same(got, want), (name, r, cells)
        assert got.nowhere == 1 and got.n == 303 and got.half is half and got.distance2.min() == 0.0   # the repeated row
        plain = hoomd.neighbour_list(p, box, r, rows=rows, cells=cells, dimensions=dims, half=half)
        assert plain.distance2 is None and np.array_equal(plain.neighbours, got.neighbours)


def test_the_steps_of_the_walk_do_not_show(monkeypatch):
    """The walk expands candidates in steps of at most 2^22; a step of 50 gives the same list."""
    p = random_rows(4, 300, TRICLINIC)
    want = hoomd.neighbour_list(p, TRICLINIC, 1.3, distances=True)
    monkeypatch.setattr(hoomd, '_NEIGHBOURS_PAIRS_PER_STEP', 50)
    got = hoomd.neighbour_list(p, TRICLINIC, 1.3, distances=True)
    assert same(got, (want.summary, want.rows, want.cell, want.offsets, want.neighbours, want.distance2))


# ---------------------------------------------------------------- the list against the census
@pytest.mark.parametrize("name", sorted(BOXES))
def test_counts_and_nearest_equal_the_census(name):
    box, dims = BOXES[name]
    p = random_rows(11, 400, box, np.float32, dims)
    p[3] = np.inf
    rows = np.concatenate([np.arange(400), [17, 17]])
    for r in (0.6, 1.3):
        census = hoomd.particle_neighbours(p, box, r, rows=rows, dimensions=dims)
        got = hoomd.neighbour_list(p, box, r, rows=rows, dimensions=dims, distances=True)
        assert np.array_equal(got.rows, census.rows) and np.array_equal(got.cell, census.cell) and got.grid == census.grid
        assert np.array_equal(got.counts, census.count) and got.pairs == census.pairs and got.nowhere == census.nowhere
        assert got.longest == census.count_max
        # the nearest neighbour as the census defines it: the minimum over (d2, j)
        for k in range(got.n):
            seg, d2 = got.of(k), got.distance2[int(got.offsets[k]):int(got.offsets[k + 1])]
            if len(seg) == 0:
                assert census.nearest[k] == NONE and census.nearest2[k] == np.inf
                continue
            best = min(zip(d2.tolist(), seg.tolist()))
            assert best == (float(census.nearest2[k]), int(census.nearest[k])), (name, r, k)
            first = int(np.argmin(d2))                  # the first position of the smallest distance ...
            if (d2 == d2[first]).sum() == 1:            # ... is the census's nearest unless the distance is tied
                assert int(seg[first]) == int(census.nearest[k])


def test_the_half_list_is_the_full_list_filtered():
    """Orthorhombic box, random rows (no half-box ties): every pair is in the full list twice and in the half list once."""
    p = random_rows(12, 500, ORTHO, np.float64)
    full = hoomd.neighbour_list(p, ORTHO, 1.3, distances=True)
    half = hoomd.neighbour_list(p, ORTHO, 1.3, half=True, distances=True)
    assert full.pairs == 2 * half.pairs > 0
    i = np.repeat(np.arange(full.n), full.counts.astype(np.int64))
    keep = full.neighbours > i
    assert np.array_equal(full.neighbours[keep], half.neighbours)
    assert np.array_equal(full.distance2[keep].view(np.uint64), half.distance2.view(np.uint64))
    assert np.array_equal(np.bincount(i[keep], minlength=full.n), half.counts)
    a, b = full.pair_rows(), half.pair_rows()
    assert a.shape == (full.pairs, 2) and b.shape == (half.pairs, 2)
    assert set(map(tuple, a.tolist())) == set(map(tuple, b.tolist())) | set((y, x) for x, y in b.tolist())


# ---------------------------------------------------------------- edges, the result type
def test_nothing_one_entry_and_everything_nowhere():
    for half in (False, True):
        got = hoomd.neighbour_list(np.zeros((0, 3), np.float32), CUBE, 1.0, half=half, distances=True)
        assert got.n == got.pairs == got.longest == got.nowhere == 0 and got.offsets.tolist() == [0]
        assert got.neighbours.shape == (0,) and got.neighbours.dtype == np.uint32 and got.distance2.shape == (0,)
        assert got.counts.shape == (0,) and got.pair_rows().shape == (0, 2)
        got = hoomd.neighbour_list(np.array([[1, 2, 3]], np.float32), CUBE, 1.0, half=half)
        assert got.n == 1 and got.pairs == 0 and got.offsets.tolist() == [0, 0] and got.of(0).shape == (0,)
        got = hoomd.neighbour_list(np.full((5, 3), np.nan, np.float32), CUBE, 1.0, half=half)
        assert got.n == got.nowhere == 5 and got.pairs == 0 and got.offsets.tolist() == [0] * 6
    with pytest.raises(IndexError):
        got.of(5)


def test_the_bytes_a_list_occupies():
    got = hoomd.neighbour_list(random_rows(5, 200, CUBE), CUBE, 1.5, distances=True)
    assert got.pairs > 0 and got.nbytes == got.offsets.nbytes + got.neighbours.nbytes + got.distance2.nbytes
    assert hoomd.neighbour_list_bytes(got.n, got.pairs) == got.offsets.nbytes + got.neighbours.nbytes
    assert hoomd.neighbour_list_bytes(0, 0) == 8 and hoomd.neighbour_list_bytes(10, 7, True) == 88 + 28 + 56


def test_neighbour_list_has_slots_a_summary_and_host_side_helpers_only():
    got = hoomd.neighbour_list(random_rows(5, 50, CUBE), CUBE, 1.5)
    with pytest.raises(AttributeError):
        got.anything = 1
    again = hoomd.NeighbourList(got.r, got.grid, got.dimensions, got.half, got.summary)
    assert (again.n, again.nowhere, again.pairs, again.longest) == (got.n, got.nowhere, got.pairs, got.longest)
    with pytest.raises(ValueError, match="words"):
        hoomd.NeighbourList(1.0, (1, 1, 1), 3, False, np.zeros(5, np.uint64))

    class InGpuMemory(object):          # what the device path leaves on the result: no numpy array
        __cuda_array_interface__ = {}

    again.offsets = again.neighbours = again.rows = InGpuMemory()
    for call in (lambda: again.counts, lambda: again.of(0), again.pair_rows):
        with pytest.raises(ValueError, match="GPU memory"):
            call()


# ---------------------------------------------------------------- refusals, frames, the command line
def test_what_neighbour_list_refuses():
    """The refusals of particle_neighbours, with its messages."""
    p = random_rows(1, 10, ORTHO)
    for r in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match="finite and positive"):
            hoomd.neighbour_list(p, ORTHO, r)
    with pytest.raises(ValueError, match="narrower"):
        hoomd.neighbour_list(p, ORTHO, 1.3, cells=(8, 6, 4))
    with pytest.raises(ValueError, match="narrower"):
        hoomd.neighbour_list(p, TRICLINIC, 1.3, cells=hoomd.cell_grid_for(ORTHO, 1.3))
    with pytest.raises(ValueError, match="2\\^20"):
        hoomd.neighbour_list(p, [1000, 800, 600, 0, 0, 0], 1.0, cells=(1000, 800, 600))
    with pytest.raises(ValueError, match="count twice"):
        hoomd.neighbour_list(p, ORTHO, 3.01)
    hoomd.neighbour_list(p, ORTHO, 3.0)
    hoomd.neighbour_list(p, FLAT, 3.4, dimensions=2)
    with pytest.raises(ValueError, match="count twice"):
        hoomd.neighbour_list(p, FLAT, 3.4)
    with pytest.raises(ValueError, match="cz == 1"):
        hoomd.neighbour_list(p, FLAT, 0.5, cells=(3, 2, 2), dimensions=2)
    with pytest.raises(ValueError, match="outside the position array"):
        hoomd.neighbour_list(p, ORTHO, 1.0, rows=[0, 10])
    with pytest.raises(ValueError, match="float32 or float64"):
        hoomd.neighbour_list(np.zeros((4, 3), np.int32), ORTHO, 1.0)


def _small_frame():
    fr = hoomd.Frame()
    fr.configuration.box = [8, 8, 8, 0, 0, 0]
    fr.particles.N = 6
    fr.particles.types = ['fluid', 'wall']
    fr.particles.typeid = np.array([0, 0, 1, 0, 0, 0], np.uint32)
    fr.particles.position = np.array([[1, 1, 1], [1.5, 1, 1], [1, 1.25, 1], [-3.9, 0, 0], [3.9, 0, 0], [np.nan, 0, 0]],
                                     np.float32)
    return fr


def test_frame_neighbour_list_over_selections():
    fr = _small_frame()
    p = fr.particles.position
    got = hoomd.frame_neighbour_list(fr, 1.0, distances=True)
    want = hoomd.neighbour_list(p, fr.configuration.box, 1.0, distances=True)
    assert same(got, (want.summary, want.rows, want.cell, want.offsets, want.neighbours, want.distance2))
    assert got.pairs == 8 and got.nowhere == 1 and got.longest == 2
    fluid = hoomd.frame_neighbour_list(fr, 1.0, half=True, where={'type': ['fluid']})
    want = hoomd.neighbour_list(p, fr.configuration.box, 1.0, rows=[0, 1, 3, 4, 5], half=True)
    assert same(fluid, (want.summary, want.rows, want.cell, want.offsets, want.neighbours, None)) and fluid.pairs == 2
    dom = hoomd.Domain((0.5, 0, 0), (1, 1, 1))
    inside = hoomd.frame_neighbour_list(fr, 1.0, domain=dom)
    want = hoomd.neighbour_list(p, fr.configuration.box, 1.0, rows=hoomd.domain_rows(p, fr.configuration.box, dom))
    assert same(inside, (want.summary, want.rows, want.cell, want.offsets, want.neighbours, None)) and 0 < inside.n < 6
    arrays = {'position': p}
    with pytest.raises(ValueError, match="box"):
        hoomd.frame_neighbour_list(arrays, 1.0)
    assert hoomd.frame_neighbour_list(arrays, 1.0, box=fr.configuration.box).pairs == 8
    with pytest.raises(ValueError, match="finite and positive"):
        hoomd.frame_neighbour_list(fr, 0.0)


def test_the_command_line_prints_what_a_list_would_hold(tmp_path, capsys):
    path = str(tmp_path / "small.gsd")
    with hoomd.open(path, 'w') as t:
        t.append(_small_frame())
    with hoomd.open(path, 'r') as t:
        assert t.frame_neighbour_list(0, 1.0).pairs == 8
    assert pgsd_main(['info', path, '--neighbour-list', '1.0']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "neighbour list of frame 0 inside 1.0 over 8 x 8 x 8 cells:" in lines
    assert "entries: 6 nowhere: 1" in lines and "pairs: 8 longest segment: 2" in lines
    assert "bytes: %d with distances: %d" % (8 * 7 + 4 * 8, 8 * 7 + 12 * 8) in lines
    assert pgsd_main(['info', path, '--neighbour-list', '1.0', '--half', '--types', 'fluid']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "neighbour list of frame 0 inside 1.0 over 8 x 8 x 8 cells (half) (types fluid):" in lines
    assert "entries: 5 nowhere: 1" in lines and "pairs: 2 longest segment: 1" in lines
    assert "bytes: %d with distances: %d" % (8 * 6 + 4 * 2, 8 * 6 + 12 * 2) in lines
    assert pgsd_main(['info', path, '--neighbour-list', '5.0']) == 1
    assert "count twice" in capsys.readouterr().err
