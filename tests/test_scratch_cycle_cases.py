"""The sequences of tests/test_gpu_scratch_cycle.py, held against what they are meant to exercise before anything goes to
a GPU: every family's tiny step lies below the scratch's 64 KiB floor and its big step above it, the mid step inside the
big one, the fourth step fits or grows as `scratch_cycle_cases.FOURTH` records, and under the host models alone no big or
mid step is degenerate -- pairs, rows that are nowhere, a run longer than a workgroup, a cell and a component longer than a
slab of 1024, more than one component, a body and a fluid, a probe point with and one without a neighbour.  These are
conditions on the inputs, not measurements."""
import numpy as np
import pytest

import pgsd.hoomd as hoomd
import scratch_cycle_cases as S


@pytest.fixture(scope="module")
def A():
    return S.arrays()


def big_and_mid(family):
    return [s for s in S.SEQUENCES[family] if s['n'] in (S.BIG, S.MID)]


def test_the_file_holds_what_the_sequences_read(A):
    assert S.FINE == hoomd.neighbour_grid_for(S.BOX, S.R) and 2.0 * S.H == S.R
    for n in S.HEIGHTS:
        for key, dt in S.DTYPES.items():
            for c, width in (('x', 3), ('m', 1), ('rho', 1), ('v', 3), ('e', 1), ('p', 1), ('s', 1)):
                a = A['%s%d_%s' % (c, n, key)]
                assert a.dtype == dt and a.size == n * width, (c, n, key)
            s = A['s%d_%s' % (n, key)]
            assert (s > 0).all() and 2.0 * float(s.max()) <= S.R           # every grid is wide enough for the largest support
        body, fluid = S.body_fluid(A, n)
        assert len(body) > 0 and len(fluid) > 0 and len(body) + len(fluid) == n
    assert A['points'].shape == (S.POINTS, 3) and S.POINTS > 256
    assert sum(a.nbytes for a in A.values()) < 2 << 20


@pytest.mark.parametrize("family", S.FAMILIES)
def test_the_sizes_straddle_the_floor_as_the_sequence_says(A, family):
    tiny64, big, mid, fourth, tiny32 = S.SEQUENCES[family]
    assert [(s['n'], s['key']) for s in S.SEQUENCES[family]] == [(S.TINY, 'f64'), (S.BIG, 'f32'), (S.MID, 'f32'), (S.MID, 'f64'),
                                                                  (S.TINY, 'f32')]
    needs = [S.step_need(A, s) for s in S.SEQUENCES[family]]
    assert needs[0] < S.FLOOR < needs[1] and needs[4] < S.FLOOR, needs
    assert needs[2] <= needs[1], needs
    assert mid['grid'] != big['grid'] and S.n_cells_of(mid['grid']) <= S.n_cells_of(big['grid'])
    assert mid['opts'] != big['opts'] or family == 'components'             # (the components take no optional input)
    grown = S.capacity(needs[1])
    assert grown >= needs[1] and S.capacity(needs[0]) == S.FLOOR
    assert ('fits' if needs[3] <= grown else 'grows') == S.FOURTH[family], (needs, grown)


def test_every_step_of_the_mixed_sequence_is_a_step_of_a_family():
    assert [s['family'] for s in S.INTERLEAVED[:12]] == list(
        ('census', 'sums', 'list', 'components', 'component_fields', 'cells', 'adaptive', 'gradients', 'tensors', 'forces',
         'body', 'samples'))
    assert sorted(set(s['family'] for s in S.INTERLEAVED)) == sorted(S.FAMILIES)
    for s in S.INTERLEAVED:
        assert s in S.SEQUENCES[s['family']]
    again = dict((s['family'], s) for s in S.INTERLEAVED[12:])
    for first in S.INTERLEAVED[:4]:
        assert again[first['family']]['n'] != first['n']


@pytest.mark.parametrize("family", ['census', 'list'])
def test_the_pair_steps_have_pairs_lost_rows_and_a_run_longer_than_a_workgroup(A, family):
    for step in big_and_mid(family):
        want = S.model(A, step)
        assert want.pairs > 0 and want.nowhere > 0 and want.n == step['n']
        clump = np.isin(want.rows, np.arange(2000, 2000 + S.CLUMP))
        if family == 'census':
            assert want.count[clump].max() > 256 and want.count_max > 256
            if step['n'] == S.BIG:      # outside the clump an entry has some 20 to 40 neighbours: the models stay quick
                assert 20 <= np.median(want.count[want.cell < S.n_cells_of(step['grid'])]) <= 40
        else:
            assert want.longest > 256 and np.diff(want.offsets.astype(np.int64))[clump].max() > 256


@pytest.mark.parametrize("family", ['cells', 'component_fields'])
def test_the_slab_families_have_a_piece_longer_than_a_slab(A, family):
    for step in big_and_mid(family):
        want = S.model(A, step)
        if family == 'cells':
            assert want.count.max() > 1024 and want.nowhere > 0 and int(want.count.sum()) + want.nowhere == step['n']
        else:
            comps, fields = want
            assert comps.largest > 1024 and comps.components > 1 and comps.nowhere > 0 and fields.components == comps.components


def test_the_components_steps_have_more_than_one_component(A):
    for step in big_and_mid('components'):
        want = S.model(A, step)
        assert want.components > want.nowhere + 1 and want.largest > 1024 and want.nowhere > 0     # (a lost row is a piece)
        assert int(want.sizes.astype(np.int64).sum()) == step['n']


@pytest.mark.parametrize("family", ['sums', 'adaptive', 'gradients', 'tensors', 'forces'])
def test_the_sph_steps_sum_over_neighbours_and_lost_rows(A, family):
    for step in big_and_mid(family):
        want = S.model(A, step)
        assert want.n == step['n'] and want.nowhere > 0 and want.not_finite == 0
        census = hoomd.particle_neighbours(S.col(A, 'x', step), S.BOX, S.R, cells=step['grid'])
        assert census.pairs > 0 and census.count_max > 256              # the support is the census' range
        if family == 'adaptive':
            assert want.pairs > 0 and want.count_max > 256 and want.bad_h == 0


def test_the_body_steps_have_a_body_in_a_fluid(A):
    for step in big_and_mid('body'):
        want = S.model(A, step)
        assert want.n > 256 and want.n_sources > 256 and want.n + want.n_sources == step['n']
        assert want.pairs > 0 and 0 < want.wetted < want.n and want.nowhere > 0 and want.sources_nowhere > 0
        assert want.contacts.max() > 256


def test_the_sample_steps_have_points_with_and_without_a_neighbour(A):
    cells = hoomd.cell_ids(A['points'], S.BOX, S.FINE)
    assert cells[0] < S.n_cells_of(S.FINE) and cells[2] == S.n_cells_of(S.FINE)       # the void has a cell, the NaN has none
    for step in big_and_mid('samples'):
        want = S.model(A, step)
        assert want.points == S.POINTS and want.nowhere == 1
        assert want.count[0] == 0 and want.count[1] > 1024 and want.count[2] == 0 and (want.count[3:] > 0).sum() > 256
        assert want.columns == ((3,) if step['opts']['values'] else ())


def test_the_tiny_steps_are_not_empty(A):
    for family in S.FAMILIES:
        for step in (S.SEQUENCES[family][0], S.SEQUENCES[family][4]):
            want = S.model(A, step)
            if family == 'samples':
                assert want.points == S.POINTS
            elif family == 'cells':
                assert int(want.count.sum()) + want.nowhere == S.TINY
            elif family == 'component_fields':
                assert want[0].n == want[1].n == S.TINY
            else:
                assert want.n + getattr(want, 'n_sources', 0) == S.TINY


def test_the_comparison_tells_a_bit_and_takes_a_nan_for_a_nan():
    a = np.array([1.0, np.nan, -0.0])
    assert not S.arrays_differ(a, a.copy()) and S.arrays_differ(a, np.array([1.0, np.nan, 0.0]))
    assert not S.arrays_differ(a, np.array([1.0, -np.nan, -0.0])) and S.arrays_differ(a, np.array([1.0, 2.0, -0.0]))
    assert S.arrays_differ(a.astype(np.float32), a) and S.arrays_differ(a[:2], a) and S.arrays_differ(None, a)
    assert not S.arrays_differ(None, None)
    assert not S.arrays_differ(np.array([-1, 5], np.int32), np.array([0xFFFFFFFF, 5], np.uint32))
    assert not S.arrays_differ(np.array([1, 5], np.int32), np.array([1, 5], np.int64))
    assert S.arrays_differ(np.array([1, 6], np.int32), np.array([1, 5], np.int64))
    words = np.array([7, 0xFFFFFFFF, np.float64(np.nan).view(np.uint64)], np.uint64)
    other = words.copy()
    other[2] |= np.uint64(1) << np.uint64(63)
    assert not S.words_differ(words, other)
    other[0] = 8
    assert S.words_differ(words, other) and S.words_differ(words, words[:2])
