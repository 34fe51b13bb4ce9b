"""Cell fields on the GPU: pgsd_cell_offsets_device and pgsd_cell_moments_device behind pgsd.fl's cell_offsets_device and
cell_moments_device and pgsd.hoomd's cell_moments_device.  Every result must equal the numpy model
pgsd.hoomd.cell_offsets / cell_moments / frame_cell_moments exactly -- the counters with numpy.array_equal, the nine sums
per cell bit for bit: the order of a cell's sum is part of the definition (tests/test_cell_moments_model.py checks the
model itself against a loop).  The cases at the pgsd.fl level pass a constructed sorted cell array, so the layouts are
exact: where a cell starts in its slab of 1024 sorted entries, how many pieces it has, what follows it."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402
from pgsd import _lib  # noqa: E402
from test_cell_moments_model import (INPUTS, MUTATIONS, ROW, SPECIAL, TRI, cells_of, inputs, mutation_differs, same,  # noqa: E402
                                     special_rows, split, wide)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 70_001
CHUNKS = {'f32': ['particles/mass', 'particles/velocity', 'particles/energy', 'particles/position'],
          'f64': ['log/m64', 'log/v64', 'log/e64', 'log/x64']}
DTYPES = {'f32': np.float32, 'f64': np.float64}
# name -> (entries per cell, entries nowhere): a cell whose first entry sits at sorted position 1023, 1024, 1025; a long
# cell (2500 entries: three pieces) that starts mid-slab, followed by cells of 1, 2 and 64 entries; a long cell that ends
# exactly on a slab edge (512 + 2560 = 3 x 1024); two long cells back to back (the second has five pieces: a tree over
# them pairs otherwise than the sequence); one cell of 69 pieces; empty cells between occupied ones; nothing but nowhere;
# no entry at all; one cell
LAYOUTS = {'first_at_1023': ([1023, 70, 5], 3), 'first_at_1024': ([1024, 70, 5], 0), 'first_at_1025': ([1025, 70, 5], 3),
           'long_mid_slab': ([300, 2500, 1, 2, 64], 5), 'long_ends_on_edge': ([512, 2560, 10], 0),
           'two_long': ([100, 1500, 4500, 7], 1), 'one_70001': ([70_001], 0),
           'empty_between': ([5, 0, 0, 70, 0, 1100, 0], 2), 'all_nowhere': ([0, 0, 0, 0], 100), 'nothing': ([0, 0, 0], 0),
           'one_cell': ([65], 0)}


def _dir(tmp_path_factory, name):
    return "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp(name))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """One file of one frame of 70 001 particles: the four float inputs as float32 particle chunks and again as float64
    log chunks, the special rows of the model module in rows 1 .. 8; the host's arrays beside it.  Left unchanged."""
    path = os.path.join(_dir(tmp_path_factory, "cells"), "pgsd_cells_%d.gsd" % os.getpid())
    rng = np.random.default_rng(N)
    fr = hoomd.Frame()
    fr.configuration.box = TRI
    fr.particles.N = N
    arrays = {}
    a32, a64 = special_rows(inputs(rng, N, np.float32), np.float32), special_rows(inputs(rng, N, np.float64), np.float64)
    for name in INPUTS:
        setattr(fr.particles, name, a32[name])
        arrays['particles/' + name] = a32[name]
    for short, name in (('m64', 'mass'), ('v64', 'velocity'), ('e64', 'energy'), ('x64', 'position')):
        arrays['log/' + short] = fr.log[short] = a64[name]
    with hoomd.open(path, 'w') as t:
        t.append(fr)
    yield path, arrays
    os.unlink(path)


def layout(name):
    """(rows, sorted cell ids, n_cells) of a layout: random rows with repeats; the special rows stand in every cell's
    first lane, in its lane 63, in the last step of its first piece (entry 1023) and at its last entry (the last
    piece)."""
    if name == 'sparse':                # 3000 entries spread over 5000 cells
        lengths, nowhere = np.bincount(np.random.default_rng(3).integers(0, 5000, size=3000), minlength=5000).tolist(), 0
    elif name == 'million':             # 2^20 cells, 65 entries, the first and the last cell among them
        lengths = np.zeros(2 ** 20, np.int64)
        lengths[np.concatenate(([0, 2 ** 20 - 1], np.random.default_rng(4).permutation(2 ** 20 - 2)[:61] + 1))] = 1
        lengths[2 ** 19] += 2
        lengths, nowhere = lengths.tolist(), 0
    else:
        lengths, nowhere = LAYOUTS[name]
    cell = cells_of(lengths, nowhere)
    rng = np.random.default_rng(len(cell) + 1)
    rows = rng.integers(0, N, size=len(cell))
    first = np.concatenate(([0], np.cumsum(lengths)))
    k = 0
    for c in np.flatnonzero(lengths):
        for spot in (0, 63, 1023, lengths[c] - 1):
            if 0 <= spot < lengths[c]:
                rows[first[c] + spot] = SPECIAL[k % len(SPECIAL)]
                k += 1
    return rows.astype(np.int32), cell.astype(np.int32), len(lengths)


def spec(names):
    return [None if name is None else (0, name) for name in names]


def model(arrays, names, rows, cell, n_cells, defaults=None):
    """cell_moments for the chunk names (None: the default row) of a device call."""
    given = dict(zip(INPUTS, split(defaults)))
    args = [given[k] if name is None else arrays[name] for k, name in zip(INPUTS, names)]
    return hoomd.cell_moments(*args, cell=cell, n_cells=n_cells, rows=rows, N=N)


def to_device(f, a):
    return fl._device_from_host(np.ascontiguousarray(a, dtype=np.int32), f.pipeline_device())


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr() if hasattr(x, 'data_ptr') else x.ptr)


# ---------------------------------------------------------------- constructed layouts
@pytest.mark.parametrize("key", ['f32', 'f64'])
@pytest.mark.parametrize("name", sorted(LAYOUTS) + ['sparse', 'million'])
def test_a_constructed_layout_equals_the_model(data, name, key):
    path, arrays = data
    rows, cell, n_cells = layout(name)
    n = len(rows)
    with fl.open(path, 'r') as f:
        d_rows, d_cell = to_device(f, rows), to_device(f, cell)
        offs = _host(f.cell_offsets_device(d_cell, n, n_cells))
        assert np.array_equal(offs, hoomd.cell_offsets(cell, n_cells)) and offs.dtype == np.int32
        for absent in ([], [0], [1], [2], [3], [0, 1, 2, 3]):
            names = [None if i in absent else c for i, c in enumerate(CHUNKS[key])]
            for defaults in ((ROW, None) if absent in ([], [0, 1, 2, 3]) and n_cells < 2 ** 20 else (ROW,)):
                got = f.cell_moments_device(spec(names), d_rows, d_cell, n, n_cells, defaults)
                assert same(got, model(arrays, names, rows, cell, n_cells, defaults), (name, key, absent))
        f.wait_read()
    assert int(got.count.sum()) + got.nowhere == n
    if name == 'empty_between':
        assert got.count.tolist() == [5, 0, 0, 70, 0, 1100, 0] and got.sums[1].view(np.uint64).tolist() == [0] * 9
    if name in ('all_nowhere', 'nothing'):
        assert not got.count.any() and not got.sums.view(np.uint64).any() and got.nowhere == n


def test_the_special_rows_are_where_the_cases_need_them(data):
    """What the layout cases rely on: values that are not finite in a cell's first lane, in lane 63, in the last step
    of a piece and in the last piece, and sums that depend on the order."""
    _, arrays = data
    m = arrays['particles/mass']
    assert np.isnan(m[1]) and m[2] == 0 and np.isinf(arrays['particles/velocity'][2, 2]) and np.signbit(m[3])
    assert np.isinf(arrays['particles/energy'][6]) and np.isnan(arrays['particles/position'][7, 1]) and np.isinf(m[8])
    assert arrays['log/v64'][5, 0] == 1e200 and np.isfinite(arrays['log/m64'][5] * 1e200)
    rows, cell, n_cells = layout('long_mid_slab')
    assert set(rows[[300, 363, 1323, 2799]].tolist()) <= set(SPECIAL)
    want = model(arrays, CHUNKS['f64'], rows, cell, n_cells)
    assert want.bad[1] >= 3
    q = arrays['log/m64'][rows] * arrays['log/v64'][rows, 1]
    seq = np.bincount(cell, weights=np.where(np.isfinite(q), q, 0.0), minlength=n_cells + 1)[:n_cells]
    assert (seq != want.momentum[:, 1]).any()


MUTATION_LAYOUTS = {'piece length 4096': 'long_mid_slab', 'lane walk contiguous': 'first_at_1023',
                    'pieces from the slab': 'long_mid_slab', 'long cell by a tree': 'two_long',
                    'non-finite not skipped': 'first_at_1025', 'default ignored': 'first_at_1024',
                    'upper bound': 'empty_between'}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_the_layouts_tell_every_mutation_apart(data, mutation):
    """The GPU equals the model on these layouts; a reduction with the mutation would not: the mutated loop differs
    from the model on the layout's own rows."""
    _, arrays = data
    rows, cell, n_cells = layout(MUTATION_LAYOUTS[mutation])
    a = dict((k, arrays[c]) for k, c in zip(INPUTS, CHUNKS['f64']))
    if mutation == 'default ignored':
        a['mass'] = None
    assert mutation_differs(mutation, a, rows, cell, n_cells, ROW, np.float64, range(9))


# ---------------------------------------------------------------- refusals
def test_lists_that_must_be_refused(data):
    """Descending ids, ids outside [0, n_cells] and an entry >= N: refused, nothing more; the next call is correct."""
    path, arrays = data
    rows, cell, n_cells = layout('long_mid_slab')
    n = len(rows)
    names = CHUNKS['f32']
    with fl.open(path, 'r') as f:
        good_rows, good_cell = to_device(f, rows), to_device(f, cell)
        for what, at, value in (('cell', 1500, 0), ('cell', n - 1, 3), ('cell', 0, -1), ('cell', n - 1, n_cells + 1),
                                ('cell', 2000, 2 ** 31 - 1), ('rows', 0, N), ('rows', n - 1, -1), ('rows', 1400, 2 ** 31 - 1)):
            bad_rows, bad_cell = rows.copy(), cell.copy()
            (bad_cell if what == 'cell' else bad_rows)[at] = value
            with pytest.raises(ValueError, match="descends or lies outside"):
                f.cell_moments_device(spec(names), to_device(f, bad_rows), to_device(f, bad_cell), n, n_cells)
            if what == 'cell':
                with pytest.raises(ValueError, match="descends or lies outside"):
                    f.cell_offsets_device(to_device(f, bad_cell), n, n_cells)
            got = f.cell_moments_device(spec(names), good_rows, good_cell, n, n_cells)
            assert same(got, model(arrays, names, rows, cell, n_cells), (what, at, value))
            assert np.array_equal(_host(f.cell_offsets_device(good_cell, n, n_cells)), hoomd.cell_offsets(cell, n_cells))
        f.wait_read()


def test_every_refusal_has_its_message_and_leaves_the_outputs_untouched(data, tmp_path):
    path, arrays = data
    rows, cell, n_cells = layout('first_at_1025')
    n = len(rows)
    with fl.open(path, 'r') as f:
        d_rows, d_cell = to_device(f, rows), to_device(f, cell)

        def call(names=CHUNKS['f32'], rows=d_rows, cell=d_cell, n=n, n_cells=n_cells, **kw):
            return f.cell_moments_device(spec(names), rows, cell, n, n_cells, **kw)

        for kw, message in ((dict(n_cells=0), "1 to 2\\^20 cells"), (dict(n_cells=2 ** 20 + 1), "1 to 2\\^20 cells"),
                            (dict(names=['log/m64'] + CHUNKS['f32'][1:]), "not mixed"),
                            (dict(names=['particles/velocity'] + CHUNKS['f32'][1:]), "mass chunk has 1 column"),
                            (dict(names=CHUNKS['f32'][:3]), "mass, velocity, energy, position"),
                            (dict(defaults=[1.0]), "defaults holds"), (dict(n=n + 1), "fewer entries than n"),
                            (dict(cell=to_device(f, cell[:5])), "fewer entries than n")):
            with pytest.raises(ValueError, match=message):
                call(**kw)
        with pytest.raises(ValueError, match="1 to 2\\^20 cells"):
            f.cell_offsets_device(d_cell, n, 0)
        with pytest.raises(KeyError):
            call(names=['particles/nothing'] + CHUNKS['f32'][1:])
        assert same(call(), model(arrays, CHUNKS['f32'], rows, cell, n_cells))
        # through the entry points themselves: the outputs stay as they were
        fn = _lib.lib.pgsd_cell_moments_device
        fn.restype = ctypes.c_int32
        E = ctypes.POINTER(_lib.IndexEntry)
        fn.argtypes = [ctypes.POINTER(_lib.Handle), E, E, E, E, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p,
                       ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64),
                       ctypes.POINTER(ctypes.c_double)]
        off = _lib.lib.pgsd_cell_offsets_device
        off.restype = ctypes.c_int32
        off.argtypes = [ctypes.POINTER(_lib.Handle), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
        h = f._h()
        entries = [_lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(h, 0, name.encode()).contents)
                   for name in CHUNKS['f32']]
        defaults = (ctypes.c_double * 8)(1, 0, 0, 0, 0, 0, 0, 0)
        counts = (ctypes.c_uint64 * (2 * n_cells + 1))(*([77] * (2 * n_cells + 1)))
        sums = (ctypes.c_double * (9 * n_cells))(*([77.0] * (9 * n_cells)))
        descending = cell.copy()
        descending[1030] = 0
        outside = rows.copy()
        outside[7] = N
        d_desc, d_out = to_device(f, descending), to_device(f, outside)

        def raw(entries=entries, rows=d_rows, cell=d_cell, n=n, n_cells=n_cells):
            return fn(h, *[ctypes.byref(e) if e is not None else None for e in entries], defaults, _ptr(rows), _ptr(cell),
                      n, n_cells, counts, sums)

        huge = [_lib.IndexEntry.from_buffer_copy(e) for e in entries]
        for e in huge:
            e.N = 2 ** 32
        for args, message in ((dict(entries=huge), "2^32 rows"), (dict(n=2 ** 32), "2^32 entries"),
                              (dict(cell=d_desc), "descends or lies outside"), (dict(rows=d_out), "outside the chunks"),
                              (dict(n_cells=2), "descends or lies outside"), (dict(n_cells=0), "2^20 cells"),
                              (dict(n_cells=2 ** 20 + 1), "2^20 cells")):
            assert raw(**args) == _lib.ERROR_INVALID_ARGUMENT and message in _lib.last_error(), (message, _lib.last_error())
            assert list(counts) == [77] * (2 * n_cells + 1) and list(sums) == [77.0] * (9 * n_cells)
        out = to_device(f, np.full(n_cells + 2, 77))
        for args, message in (((_ptr(d_desc), n, n_cells), "descends or lies outside"), ((_ptr(d_cell), n, 2), "descends or lies"),
                              ((_ptr(d_cell), 2 ** 32, n_cells), "2^32 entries"), ((_ptr(d_cell), n, 0), "2^20 cells")):
            assert off(h, *args, _ptr(out)) == _lib.ERROR_INVALID_ARGUMENT and message in _lib.last_error(), _lib.last_error()
            assert _host(out).tolist() == [77] * (n_cells + 2)
        # the same calls as they are: correct
        assert off(h, _ptr(d_cell), n, n_cells, _ptr(out)) == 0
        assert _host(out).tolist() == hoomd.cell_offsets(cell, n_cells).tolist()
        assert off(h, _ptr(d_cell), 0, n_cells, _ptr(out)) == 0 and _host(out).tolist() == [0] * (n_cells + 2)
        assert raw() == 0
        want = model(arrays, CHUNKS['f32'], rows, cell, n_cells)
        assert [counts[2 * c] for c in range(n_cells)] == want.count.tolist() and counts[2 * n_cells] == want.nowhere
        assert [counts[2 * c + 1] for c in range(n_cells)] == want.bad.tolist()
        assert np.array_equal(np.array(list(sums)).reshape(n_cells, 9).view(np.uint64), want.sums.view(np.uint64))
        f.wait_read()


# ---------------------------------------------------------------- staging
def test_staged_chunks_are_not_read_again(data):
    path, arrays = data
    rows, cell, n_cells = layout('two_long')
    names = CHUNKS['f32']
    with fl.open(path, 'r') as f:
        d_rows, d_cell = to_device(f, rows), to_device(f, cell)
        # two calls read every chunk once
        f.device_read_stats(reset=True)
        f.cell_moments_device(spec(names), d_rows, d_cell, len(rows), n_cells)
        assert f.device_read_stats()["pread_bytes"] == N * 32
        got = f.cell_moments_device(spec(names), d_rows, d_cell, len(rows), n_cells)
        assert f.device_read_stats()["pread_bytes"] == N * 32 and same(got, model(arrays, names, rows, cell, n_cells))
        f.wait_read()
        # after a selection and its ordering have staged the position: no file byte for the position's field
        f.device_read_stats(reset=True)
        d = hoomd.domain_grid(2, 1, 1)[1]
        sel, count = f.select_domain_device(0, 'particles/position', TRI, d)
        ids = f.order_rows_by_cell_device(0, 'particles/position', TRI, (4, 4, 4), sel, n=count)
        before = f.device_read_stats()["pread_bytes"]
        assert before == N * 12
        got = f.cell_moments_device(spec([None, None, None, names[3]]), sel, ids, count, 64)
        assert f.device_read_stats()["pread_bytes"] == before
        inside = hoomd.domain_rows(arrays[names[3]], TRI, d)
        want_rows, want_cell, _ = hoomd.cell_order(arrays[names[3]], TRI, inside, (4, 4, 4))
        assert np.array_equal(_host(sel)[:count], want_rows) and np.array_equal(_host(ids)[:count], want_cell)
        assert same(got, model(arrays, [None, None, None, names[3]], want_rows, want_cell, 64))
        f.wait_read()


# ---------------------------------------------------------------- through pgsd.hoomd
TYPES = ['fluid', 'wall', 'inlet']


def _frame(rng, n, step, dimensions=3):
    fr = hoomd.Frame()
    fr.configuration.step = step
    fr.configuration.box = TRI if dimensions == 3 else np.array([4.0, 4.0, 1.0, 0.5, 0.0, 0.0], np.float32)
    fr.configuration.dimensions = dimensions
    fr.particles.N = n
    fr.particles.types = TYPES
    fr.particles.position = rng.uniform(-3.0, 3.0, size=(n, 3)).astype(np.float32)
    if dimensions == 2:
        fr.particles.position[:, 2] = 0.0
    fr.particles.position[11] = [np.inf, 0.0, 0.0]              # nowhere (and equal to itself: the chunk can be elided)
    fr.particles.velocity = wide(rng, 3 * n).reshape(n, 3)
    fr.particles.mass = rng.uniform(0.5, 2.0, size=n).astype(np.float32)
    fr.particles.density = (1000.0 + 50.0 * rng.standard_normal(n)).astype(np.float32)
    fr.particles.typeid = rng.integers(0, len(TYPES), size=n).astype(np.uint32)
    return fr


@pytest.fixture(scope="module")
def trajectories(tmp_path_factory):
    """traj: two frames of 70 001 particles -- the second elides position, typeid and mass, which equal frame 0's;
    energy is stored nowhere.  flat: a 2-D frame.  empty: a frame of no particle.  bare: particles with nothing but a
    velocity (no mass, no position: every row in the origin's cell)."""
    d = _dir(tmp_path_factory, "cells_traj")
    rng = np.random.default_rng(13)
    paths = dict((k, os.path.join(d, "pgsd_cells_%d_%s.gsd" % (os.getpid(), k))) for k in ("traj", "flat", "empty", "bare"))
    f0 = _frame(rng, N, 0)
    f0.particles.velocity[[3, 255, N - 1]] = [[np.nan, 1, 1], [np.inf, 0, 0], [1, -np.inf, np.nan]]
    f1 = _frame(rng, N, 10)
    f1.particles.position, f1.particles.typeid, f1.particles.mass = f0.particles.position, f0.particles.typeid, f0.particles.mass
    with hoomd.open(paths["traj"], 'w') as t:
        t.append(f0)
        t.append(f1)
    with hoomd.open(paths["flat"], 'w') as t:
        t.append(_frame(rng, 9001, 0, dimensions=2))
    none = hoomd.Frame()
    none.configuration.box = TRI
    none.particles.types = TYPES
    with hoomd.open(paths["empty"], 'w') as t:
        t.append(none)
    bare = hoomd.Frame()
    bare.configuration.box = TRI
    bare.particles.N = 5003
    bare.particles.types = TYPES[:2]
    bare.particles.velocity = wide(rng, 3 * 5003).reshape(5003, 3)
    with hoomd.open(paths["bare"], 'w') as t:
        t.append(bare)
    yield paths
    for path in paths.values():
        os.unlink(path)


WHERE = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
CELL = hoomd.domain_grid(2, 2, 1)[1]
SELECTIONS = {"all": {}, "where": {'where': WHERE}, "domain": {'domain': CELL}, "both": {'where': WHERE, 'domain': CELL}}


def same_field(got, want, what):
    assert same(got, want, what) and got.grid == want.grid and got.cell_volume == want.cell_volume
    return True


@pytest.mark.parametrize("grid", [(4, 4, 4), (3, 1, 2), (64, 64, 64)])
@pytest.mark.parametrize("selection", sorted(SELECTIONS))
def test_cell_moments_device_equals_the_host_model(trajectories, selection, grid):
    kwargs = SELECTIONS[selection]
    with hoomd.open(trajectories["traj"], 'r') as t:
        assert not t.file.chunk_exists(1, 'particles/position') and not t.file.chunk_exists(0, 'particles/energy')
        for idx, options in ((0, dict()), (1, dict()), (0, dict(centre=False))):   # frame 1: elided chunks
            want = t.cell_moments(idx, grid, **options, **kwargs)
            t.file.device_read_stats(reset=True)
            got = t.cell_moments_device(idx, grid, **options, **kwargs)
            pread = t.file.device_read_stats()["pread_bytes"]
            assert same_field(got, want, (selection, grid, idx, options))
            # every chunk that takes part is read exactly once: mass, velocity, position (the cells need it), and the
            # selection's typeid and density
            assert pread == N * (4 + 12 + 12 + (8 if 'where' in kwargs else 0)), (selection, options)
    n_cells = grid[0] * grid[1] * grid[2]
    assert got.count.shape == (n_cells,) and got.as_grid('momentum').shape == grid[::-1] + (3,)
    if selection == "all":
        assert int(got.count.sum()) + got.nowhere == N and got.nowhere == 1 and got.bad.sum() == 3
        assert not got.internal.any() and not got.first_moment.any()
    else:
        assert 0 < int(got.count.sum()) < N


def test_two_dimensions_no_particle_and_no_position(trajectories):
    with hoomd.open(trajectories["flat"], 'r') as t:
        for kwargs in SELECTIONS.values():
            assert same_field(t.cell_moments_device(0, (5, 4, 1), **kwargs), t.cell_moments(0, (5, 4, 1), **kwargs), kwargs)
        with pytest.raises(ValueError, match="cz == 1"):
            t.cell_moments_device(0, (5, 4, 2))
    with hoomd.open(trajectories["empty"], 'r') as t:
        for kwargs in SELECTIONS.values():
            got = t.cell_moments_device(0, (3, 1, 2), **kwargs)
            assert same_field(got, t.cell_moments(0, (3, 1, 2), **kwargs), kwargs)
            assert got.count.tolist() == [0] * 6 and got.nowhere == 0 and np.isnan(got.centre_of_mass).all()
    with hoomd.open(trajectories["bare"], 'r') as t:
        for kwargs in ({}, {'domain': CELL}, {'where': {'type': ['fluid']}}, {'where': {'type': ['wall']}}):
            t.file.device_read_stats(reset=True)
            got = t.cell_moments_device(0, (4, 4, 4), **kwargs)
            assert t.file.device_read_stats()["pread_bytes"] in (0, 5003 * 12)
            assert same_field(got, t.cell_moments(0, (4, 4, 4), **kwargs), kwargs)
        full = t.cell_moments_device(0, (4, 4, 4))
        origin = int(hoomd.cell_ids(np.zeros((1, 3), np.float32), TRI, (4, 4, 4))[0])
        assert full.count[origin] == 5003 and full.count.sum() == 5003 and full.mass[origin] == 5003.0
        with pytest.raises(ValueError, match="at most 2\\^20"):
            t.cell_moments_device(0, (1024, 1024, 2))
        with pytest.raises(IndexError):
            t.cell_moments_device(1, (2, 2, 2))


def test_other_passes_are_unchanged_around_a_cell_moments_call(trajectories):
    d = hoomd.domain_grid(2, 2, 2)[3]
    with hoomd.open(trajectories["traj"], 'r') as t:
        def others():
            m = t.frame_moments_device(0, domain=d)
            s = t.read_frame_device(0, domain=d, cell_order=(4, 4, 4))
            return m, _host(s.tag), _host(s.cell), _host(s.particles.velocity)
        before = others()
        t.cell_moments_device(0, (64, 64, 64))
        t.cell_moments_device(1, (3, 1, 2), domain=d)
        after = others()
        want = t.frame_moments(0, domain=d)
        host = t[0]
    for m, tag, cell, velocity in (before, after):
        for name in hoomd.Moments.__slots__:
            g, w = getattr(m, name), getattr(want, name)
            assert np.array_equal(np.asarray(g).view(np.uint64) if name != 'other' else g,
                                  np.asarray(w).view(np.uint64) if name != 'other' else w), name
        rows = hoomd.domain_rows(host.particles.position, TRI, d)
        want_rows, want_cell, _ = hoomd.cell_order(host.particles.position, TRI, rows, (4, 4, 4))
        assert np.array_equal(tag, want_rows) and np.array_equal(cell, want_cell)
        assert velocity.tobytes() == host.particles.velocity[want_rows].tobytes()


# ---------------------------------------------------------------- without a tensor library
CHILD = r'''
import os, pickle, sys
sys.modules["torch"] = None                    # `import torch` raises ImportError from here on
root, path, traj, out_path = sys.argv[1:5]
sys.path[:0] = [os.path.join(root, "pgsd-sph_amd"), os.path.join(root, "tests")]
import numpy as np
import pgsd.fl as fl
import pgsd.hoomd as hoomd
from pgsd import _lib
import test_gpu_cell_moments as T
assert _lib._torch is None
res = {}
rows, cell, n_cells = T.layout('long_mid_slab')
with fl.open(path, 'r') as f:
    d_rows, d_cell = T.to_device(f, rows), T.to_device(f, cell)
    res["offsets"] = f.cell_offsets_device(d_cell, len(cell), n_cells).to_host()
    res["f32"] = f.cell_moments_device(T.spec(T.CHUNKS['f32']), d_rows, d_cell, len(rows), n_cells)
    res["f64"] = f.cell_moments_device(T.spec([None] + T.CHUNKS['f64'][1:]), d_rows, d_cell, len(rows), n_cells, T.ROW)
    f.wait_read()
with hoomd.open(traj, 'r') as t:
    res["frame"] = t.cell_moments_device(1, (4, 4, 4), where={'type': ['wall']}, domain=hoomd.domain_grid(2, 1, 1)[0])
    res["all"] = t.cell_moments_device(0, (3, 1, 2))
res = dict((k, v if k == "offsets" else dict((q, getattr(v, q)) for q in hoomd.CellMoments.__slots__)) for k, v in res.items())
pickle.dump(res, open(out_path, "wb"))
'''


def test_cell_moments_without_torch(data, trajectories, tmp_path):
    path, arrays = data
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, path, trajectories["traj"], str(out)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))
    rows, cell, n_cells = layout('long_mid_slab')
    assert np.array_equal(res["offsets"], hoomd.cell_offsets(cell, n_cells))
    assert same(hoomd.CellMoments(**res["f32"]), model(arrays, CHUNKS['f32'], rows, cell, n_cells), "f32")
    assert same(hoomd.CellMoments(**res["f64"]), model(arrays, [None] + CHUNKS['f64'][1:], rows, cell, n_cells, ROW), "f64")
    with hoomd.open(trajectories["traj"], 'r') as t:
        want = t.cell_moments(1, (4, 4, 4), where={'type': ['wall']}, domain=hoomd.domain_grid(2, 1, 1)[0])
        assert same_field(hoomd.CellMoments(**res["frame"]), want, "frame")
        assert same_field(hoomd.CellMoments(**res["all"]), t.cell_moments(0, (3, 1, 2)), "all")
