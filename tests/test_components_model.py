"""The components model (`pgsd.hoomd.neighbour_components`, `Components`, `frame_components`) against a plain-Python
labelling -- a double loop over pairs and a breadth-first search -- and against each mutation of it that stands for a kernel
mistake (`components_cases.py`), and against the neighbour list of the same arguments.  No GPU."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
from pgsd.__main__ import main as pgsd_main

from neighbours_cases import FLAT, ORTHO, TRICLINIC, random_rows
from components_cases import CUBE, MUTATIONS, TIES, loop_components, same

BOXES = {'orthorhombic': (ORTHO, 3), 'triclinic': (TRICLINIC, 3), 'flat': (FLAT, 2)}


def _invariants(got):
    """What holds of every result: the sizes sum to n, a label is its own label, the ids are dense and ascend with the
    labels, and the summary is the arrays'."""
    label, component, sizes = got.label.astype(np.int64), got.component.astype(np.int64), got.sizes.astype(np.int64)
    assert int(sizes.sum()) == got.n and len(sizes) == got.components
    assert np.array_equal(label[label], label) and (label <= np.arange(got.n)).all()
    roots = np.nonzero(label == np.arange(got.n))[0]
    assert len(roots) == got.components and np.array_equal(component[roots], np.arange(got.components))
    assert np.array_equal(component, component[label]) and np.array_equal(np.bincount(component, minlength=len(sizes)), sizes)
    assert got.singletons == int((sizes == 1).sum()) >= got.nowhere
    if got.n:
        assert got.largest == sizes.max() and got.largest_label == roots[int(np.argmax(sizes))]
    else:
        assert got.summary.tolist() == [0] * 6
    return True


# ---------------------------------------------------------------- mutations
@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_every_mutation_is_caught(name):
    switch, case = MUTATIONS[name]
    got = hoomd.neighbour_components(**case)
    assert not same(got, loop_components(**case, **switch)), "the mutation does not show on its case"
    # ... and the loop without the mutation agrees, so the difference is the mutation's
    assert same(got, loop_components(**case)) and _invariants(got)


def test_the_mutation_cases_by_hand():
    got = hoomd.neighbour_components(**MUTATIONS['the label is the smallest row instead of the smallest position'][1])
    assert got.rows.tolist() == [1, 0] and got.label.tolist() == [0, 0] and got.components == 1
    got = hoomd.neighbour_components(**MUTATIONS['the dense ids in the order of the largest member'][1])
    assert got.label.tolist() == [0, 1, 1, 0] and got.component.tolist() == [0, 1, 1, 0] and got.sizes.tolist() == [2, 2]
    got = hoomd.neighbour_components(**MUTATIONS['largest_label the largest label among ties'][1])
    assert got.label.tolist() == [0, 0, 2, 2] and (got.largest, got.largest_label) == (2, 0)
    got = hoomd.neighbour_components(**MUTATIONS['a repeated row not joined to itself'][1])
    assert got.n == 2 and got.components == 1 and got.sizes.tolist() == [2]
    got = hoomd.neighbour_components(**MUTATIONS['a nowhere entry joined to cell 0'][1])
    assert (got.nowhere, got.components, got.singletons) == (1, 3, 3) and got.label.tolist() == [0, 1, 2]
    got = hoomd.neighbour_components(**MUTATIONS['<= for <'][1])
    assert got.components == 2
    got = hoomd.neighbour_components(**MUTATIONS['an edge across the periodic face missed'][1])
    assert got.components == 1


@pytest.mark.parametrize("name", sorted(TIES))
def test_the_direction_of_an_edge_never_shows(name):
    """`components_cases.TIES`: at an exact half-box tie the two directions of a pair fold differently, and both lie
    outside every range the grid accepts, so a loop that takes its edges from j -> i equals the definition."""
    case = TIES[name]
    v = hoomd.box_vectors(np.asarray(case['box'], np.float32))
    a, b = case['position'][0], case['position'][1]
    assert abs(b - a)['xyz'.index(name)] == v['xyz'.index(name)] / 2           # the tie is exact
    got = hoomd.neighbour_components(**case)
    assert same(got, loop_components(**case)) and same(got, loop_components(forward=False, **case))
    pairs = set(map(tuple, hoomd.neighbour_list(half=False, distances=True, **case).pair_rows().tolist()))
    assert (0, 1) not in pairs and (1, 0) not in pairs                          # the tied pair is no edge, either way
    assert pairs == set((y, x) for x, y in pairs) and len(pairs) == 2 and got.components == 2
    # ... although the two directions do fold differently: that is what makes the case a tie
    x, y = np.float64(a)[None, :], np.float64(b)[None, :]
    there, back = hoomd.pair_displacement(x, y, v), hoomd.pair_displacement(y, x, v)
    assert any(float(there[c][0]) != -float(back[c][0]) for c in range(3))


# ---------------------------------------------------------------- the model against the loop
@pytest.mark.parametrize("name", sorted(BOXES))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_model_equals_the_loop_on_random_rows(name, dtype):
    """A few hundred rows with repeats and a nowhere entry, from dust to one percolating piece, over the automatic grid and
    over coarse ones."""
    box, dims = BOXES[name]
    p = random_rows(3, 300, box, dtype, dims)
    p[7] = np.nan
    rows = np.concatenate([np.arange(300), [5, 5, 299]])
    counts = []
    for r, cells in ((0.3, None), (0.6, None), (1.3, None), (2.9, (3, 2, 2) if dims == 3 else (3, 2, 1)), (1.3, (1, 2, 1))):
        want = loop_components(p, box, r, rows, cells, dims)
        got = hoomd.neighbour_components(p, box, r, rows=rows, cells=cells, dimensions=dims)
        assert same(got, want) and _invariants(got), (name, r, cells)
        assert same(got, loop_components(p, box, r, rows, cells, dims, forward=False)), (name, r, cells)
        assert got.nowhere == 1 and got.n == 303
        counts.append(got.components)
    assert counts[0] > counts[1] > counts[2] >= counts[3] and counts[3] <= 3   # dust first, one piece (and the lost row) last


# ---------------------------------------------------------------- against the neighbour list
def test_the_full_and_the_half_list_induce_the_same_labels():
    """Random rows have no half-box tie: the full list's pairs, as undirected edges, are the half list's, and the labels
    are those of either."""
    p = random_rows(12, 500, TRICLINIC, np.float64)
    for r in (0.5, 0.9):
        got = hoomd.neighbour_components(p, TRICLINIC, r)
        for half in (False, True):
            nl = hoomd.neighbour_list(p, TRICLINIC, r, half=half)
            assert np.array_equal(nl.rows, got.rows) and np.array_equal(nl.cell, got.cell) and nl.grid == got.grid
            parent = list(range(nl.n))

            def find(x):
                while parent[x] != x:
                    parent[x] = parent[parent[x]]
                    x = parent[x]
                return x

            for i in range(nl.n):
                for j in nl.of(i).tolist():
                    a, b = find(i), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
            assert [find(k) for k in range(nl.n)] == got.label.tolist(), (r, half)
        assert 1 < got.components < 500 and got.nowhere == 0


def test_members_fragments_and_the_result_type():
    p = random_rows(5, 200, CUBE)
    got = hoomd.neighbour_components(p, CUBE, 0.9)
    assert _invariants(got) and got.components > 1
    for c in range(got.components):
        m = got.members(c)
        assert len(m) == got.sizes[c] and m[0] == got.label[m[0]] and (got.label[m] == m[0]).all()
    with pytest.raises(IndexError):
        got.members(got.components)
    big = got.fragments(3)
    assert np.array_equal(big, np.nonzero(got.sizes >= 3)[0]) and len(got.fragments()) == got.components
    with pytest.raises(AttributeError):
        got.anything = 1
    again = hoomd.Components(got.r, got.grid, got.dimensions, got.summary)
    assert np.array_equal(again.summary, got.summary) and "components=%d" % got.components in repr(again)
    with pytest.raises(ValueError, match="words"):
        hoomd.Components(1.0, (1, 1, 1), 3, np.zeros(4, np.uint64))

    class InGpuMemory(object):          # what the device path leaves on the result: no numpy array
        __cuda_array_interface__ = {}

    again.component = again.sizes = InGpuMemory()
    for call in (lambda: again.members(0), again.fragments):
        with pytest.raises(ValueError, match="GPU memory"):
            call()


def test_nothing_one_entry_and_everything_nowhere():
    got = hoomd.neighbour_components(np.zeros((0, 3), np.float32), CUBE, 1.0)
    assert got.summary.tolist() == [0] * 6 and got.label.shape == got.component.shape == got.sizes.shape == (0,)
    assert got.label.dtype == got.component.dtype == got.sizes.dtype == np.uint32 and _invariants(got)
    got = hoomd.neighbour_components(np.array([[1, 2, 3]], np.float32), CUBE, 1.0)
    assert got.summary.tolist() == [1, 0, 1, 1, 1, 0] and got.sizes.tolist() == [1]
    got = hoomd.neighbour_components(np.full((5, 3), np.nan, np.float32), CUBE, 1.0)
    assert got.summary.tolist() == [5, 5, 5, 5, 1, 0] and got.label.tolist() == list(range(5)) and _invariants(got)


# ---------------------------------------------------------------- refusals, frames, the command line
def test_what_neighbour_components_refuses():
    """The refusals of neighbour_list, with its messages."""
    p = random_rows(1, 10, ORTHO)
    for r in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match="finite and positive"):
            hoomd.neighbour_components(p, ORTHO, r)
    with pytest.raises(ValueError, match="narrower"):
        hoomd.neighbour_components(p, ORTHO, 1.3, cells=(8, 6, 4))
    with pytest.raises(ValueError, match="count twice"):
        hoomd.neighbour_components(p, ORTHO, 3.01)
    with pytest.raises(ValueError, match="outside the position array"):
        hoomd.neighbour_components(p, ORTHO, 1.0, rows=[0, 10])
    with pytest.raises(ValueError, match="float32 or float64"):
        hoomd.neighbour_components(np.zeros((4, 3), np.int32), ORTHO, 1.0)


def _small_frame():
    fr = hoomd.Frame()
    fr.configuration.box = [8, 8, 8, 0, 0, 0]
    fr.particles.N = 7
    fr.particles.types = ['fluid', 'wall']
    fr.particles.typeid = np.array([0, 0, 1, 0, 0, 0, 0], np.uint32)
    fr.particles.position = np.array([[1, 1, 1], [1.5, 1, 1], [1, 1.25, 1], [-3.9, 0, 0], [3.9, 0, 0], [np.nan, 0, 0],
                                      [0, -3, 0]], np.float32)
    return fr


def test_frame_components_over_selections():
    fr = _small_frame()
    p = fr.particles.position
    got = hoomd.frame_components(fr, 1.0)
    want = hoomd.neighbour_components(p, fr.configuration.box, 1.0)
    assert same(got, (want.summary, want.rows, want.cell, want.label, want.component, want.sizes))
    assert (got.components, got.singletons, got.largest, got.nowhere) == (4, 2, 3, 1)
    assert sorted(got.rows[got.label == got.largest_label].tolist()) == [0, 1, 2]
    fluid = hoomd.frame_components(fr, 0.4, where={'type': ['fluid']})
    want = hoomd.neighbour_components(p, fr.configuration.box, 0.4, rows=[0, 1, 3, 4, 5, 6])
    assert same(fluid, (want.summary, want.rows, want.cell, want.label, want.component, want.sizes))
    assert (fluid.n, fluid.components, fluid.largest) == (6, 5, 2)      # only the pair through the face is left
    dom = hoomd.Domain((0.5, 0, 0), (1, 1, 1))
    inside = hoomd.frame_components(fr, 1.0, domain=dom)
    want = hoomd.neighbour_components(p, fr.configuration.box, 1.0, rows=hoomd.domain_rows(p, fr.configuration.box, dom))
    assert same(inside, (want.summary, want.rows, want.cell, want.label, want.component, want.sizes)) and 0 < inside.n < 7
    arrays = {'position': p}
    with pytest.raises(ValueError, match="box"):
        hoomd.frame_components(arrays, 1.0)
    assert hoomd.frame_components(arrays, 1.0, box=fr.configuration.box).components == 4
    with pytest.raises(ValueError, match="finite and positive"):
        hoomd.frame_components(fr, 0.0)


def test_the_command_line_prints_the_components(tmp_path, capsys):
    path = str(tmp_path / "small.gsd")
    with hoomd.open(path, 'w') as t:
        t.append(_small_frame())
    with hoomd.open(path, 'r') as t:
        want = t.frame_components(0, 1.0)
        assert want.components == 4
    assert pgsd_main(['info', path, '--components', '1.0']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "components of frame 0 inside 1.0 over 8 x 8 x 8 cells:" in lines
    assert "entries: 7 nowhere: 1" in lines and "components: 4 singletons: 2" in lines
    assert "largest: 3 entries, label %d, row %d" % (want.largest_label, want.rows[want.largest_label]) in lines
    assert not any(l.startswith("at least") for l in lines)
    assert pgsd_main(['info', path, '--components', '1.0', '--min-size', '2']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "at least 2: 2 components holding 5 entries (71.43 %)" in lines
    assert pgsd_main(['info', path, '--components', '0.4', '--types', 'fluid', '--min-size', '2']) == 0
    lines = [' '.join(l.split()) for l in capsys.readouterr().out.splitlines()]
    assert "components of frame 0 inside 0.4 over %d x %d x %d cells (types fluid):" % hoomd.neighbour_grid_for(
        [8, 8, 8, 0, 0, 0], 0.4) in lines
    assert "entries: 6 nowhere: 1" in lines and "components: 5 singletons: 4" in lines
    assert "at least 2: 1 components holding 2 entries (33.33 %)" in lines
    assert pgsd_main(['info', path, '--components', '5.0']) == 1
    assert "count twice" in capsys.readouterr().err
