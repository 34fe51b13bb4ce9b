"""Neighbour lists on the GPU: pgsd_neighbour_offsets_device and pgsd_neighbour_list_device behind pgsd.fl's
neighbour_list_device and pgsd.hoomd's frame_neighbour_list_device.  Every array must equal the numpy model
pgsd.hoomd.neighbour_list / frame_neighbour_list exactly -- numpy.array_equal, distance2 through its uint64 view
(tests/test_neighbour_list_model.py checks the model itself against a double loop in the defined order).  The cases at the
pgsd.fl level read constructed position chunks, once as float32 and once as float64, and order the list on the GPU first,
as a caller does; the protocol tests call the two entry points themselves, with output buffers that are larger than the
capacity they declare and hold a guard pattern."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import product  # noqa: E402
import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402
from pgsd import _lib  # noqa: E402
from neighbours_cases import FLAT, TRICLINIC, random_rows  # noqa: E402
from neighbour_list_cases import CUBE, MUTATIONS  # noqa: E402

WIDE = [64, 64, 64, 0, 0, 0]
N = 3001
TYPES = ['fluid', 'wall', 'inlet']
DTYPES = {'f32': np.float32, 'f64': np.float64}
GUARD = 0xA5A5A5A5
GUARD_WORDS = 64


def _clump():
    """700 entries inside one cell of the (3, 3, 3) grid -- segments longer than a workgroup -- with empty cells beside
    it, and a few rows elsewhere."""
    rng = np.random.default_rng(8)
    return np.concatenate([rng.uniform(-0.5, 0.5, size=(700, 3)), [[3.5, 3.5, 3.5], [3.6, 3.5, 3.5], [-3.9, 0, 0]]])


def _sparse():
    """65 537 rows in 64^3 cells -- 257 workgroups, the smallest count at which the one-workgroup scan takes a second
    round --, mostly empty cells; 16 384 of the rows have a partner inside the range."""
    a = random_rows(9, 49153, WIDE, np.float64)
    return np.concatenate([a, a[:16384] + np.random.default_rng(10).uniform(-0.5, 0.5, size=(16384, 3))])


def _with_lost_rows(p, every=97):
    p = p.copy()
    p[5::every, 0] = np.nan
    p[11::every, 1] = np.inf
    return p


# name -> (positions as float64, keyword arguments of neighbour_list besides position, half and distances)
CASES = {
    'nothing': (np.zeros((0, 3)), dict(box=CUBE, r=1.0)),
    'one_entry': (np.array([[1.0, 2, 3]]), dict(box=CUBE, r=1.0)),
    'exactly_r': (np.array([[0, 0, 0], [0.5, 0, 0]], np.float64), dict(box=CUBE, r=0.5)),
    'one_cell_65': (random_rows(1, 65, CUBE, np.float64), dict(box=CUBE, r=2.0, cells=(1, 1, 1))),
    'clump_700': (_clump(), dict(box=CUBE, r=2.0, cells=(3, 3, 3))),
    'three_cells_4097': (_with_lost_rows(random_rows(4, 4097, CUBE, np.float64)), dict(box=CUBE, r=2.0, cells=(3, 3, 3))),
    'x_runs_444': (random_rows(40, 400, CUBE, np.float64), dict(box=CUBE, r=2.0, cells=(4, 4, 4))),
    'x_runs_511': (random_rows(41, 300, CUBE, np.float64), dict(box=CUBE, r=1.6, cells=(5, 1, 1))),
    'x_runs_flat_421': (random_rows(42, 300, FLAT, np.float64, 2), dict(box=FLAT, r=1.3, cells=(4, 2, 1), dimensions=2)),
    'x_runs_triclinic_154': (random_rows(43, 300, TRICLINIC, np.float64), dict(box=TRICLINIC, r=1.3, cells=(1, 5, 4))),
    'all_nowhere': (np.full((100, 3), np.nan), dict(box=CUBE, r=1.0)),
    'sparse_64cubed': (_sparse(), dict(box=WIDE, r=1.0, cells=(64, 64, 64))),
}
ROWS = {}                                   # name -> the row list of a case that has one (default: every row)
for _k, (_name, (_switch, _case)) in enumerate(sorted(MUTATIONS.items())):
    _kw = dict(_case)
    _kw.pop('half', None)                   # every case runs full and half
    if 'rows' in _kw:
        ROWS['mutation_%02d' % _k] = _kw.pop('rows')
    CASES['mutation_%02d' % _k] = (np.asarray(_kw.pop('position'), np.float64), _kw)


def chunk(name, key):
    return 'log/%s_%s' % (name, key)


def _dir(tmp_path_factory, name):
    return "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp(name))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """One file of one frame: 3 001 particles with types, a density and random positions in the triclinic box (the
    pgsd.hoomd level), and every case's positions as a float32 and a float64 log chunk.  The host's arrays beside it."""
    path = os.path.join(_dir(tmp_path_factory, "neighbour_list"), "pgsd_neighbour_list_%d.gsd" % os.getpid())
    rng = np.random.default_rng(N)
    fr = hoomd.Frame()
    fr.configuration.box = TRICLINIC
    fr.particles.N = N
    fr.particles.types = TYPES
    fr.particles.position = _with_lost_rows(random_rows(7, N, TRICLINIC, np.float32), 997)
    fr.particles.typeid = rng.integers(0, len(TYPES), size=N).astype(np.uint32)
    fr.particles.density = (1000.0 + 50.0 * rng.standard_normal(N)).astype(np.float32)
    arrays = {}
    for name, (p, _) in CASES.items():
        for key, dt in DTYPES.items():
            a = np.ascontiguousarray(p.astype(dt))
            arrays[chunk(name, key)] = a
            if len(a):                      # (no entry: there is no chunk to store; the case reads another one)
                fr.log['%s_%s' % (name, key)] = a
    with hoomd.open(path, 'w') as t:
        t.append(fr)
    yield path, arrays
    os.unlink(path)


_MODEL = {}


def model(arrays, name, key, half):
    """The model's list of a case, with distances, computed once."""
    at = (name, key, half)
    if at not in _MODEL:
        _MODEL[at] = hoomd.neighbour_list(arrays[chunk(name, key)], rows=ROWS.get(name), half=half, distances=True,
                                          **CASES[name][1])
    return _MODEL[at]


def to_device(f, a):
    return fl._device_from_host(np.ascontiguousarray(a, dtype=np.int32), f.pipeline_device())


def device_buffer(f, a, dtype):
    """A library-owned buffer that holds the host array ``a`` as ``dtype`` (offsets, outputs with a guard pattern)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    return fl.DeviceBuffer((a.size,), dtype, f.pipeline_device(), pattern=a)


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr() if hasattr(x, 'data_ptr') else x.ptr)


def equal(got, want, what):
    """The kernels' NeighbourList (arrays in GPU memory) against the model's."""
    assert np.array_equal(got.summary, want.summary), (what, got, want)
    assert got.grid == want.grid and got.half == want.half and got.r == want.r and got.dimensions == want.dimensions, what
    assert np.array_equal(_host(got.rows), want.rows) and np.array_equal(_host(got.cell), want.cell), what
    offsets, neighbours = _host(got.offsets), _host(got.neighbours)
    assert offsets.dtype == np.uint64 and np.array_equal(offsets, want.offsets), what
    assert neighbours.dtype == np.uint32 and np.array_equal(neighbours, want.neighbours), what
    if got.distance2 is not None:
        d2 = _host(got.distance2)
        assert d2.dtype == np.float64 and np.array_equal(d2.view(np.uint64), want.distance2.view(np.uint64)), what
    for call in (lambda: got.counts, got.pair_rows):
        with pytest.raises(ValueError, match="GPU memory"):
            call()
    return True


def ordered(f, name, host, rows, want, kw):
    """The list sorted by cell on the GPU, as a caller does: (rows, cell, entries)."""
    every = np.arange(len(host)) if rows is None else np.asarray(rows)
    d_rows = to_device(f, every)
    d_cell = f.order_rows_by_cell_device(0, name, kw['box'], want.grid, d_rows, n=len(every), dimensions=kw.get('dimensions', 3))
    return d_rows, d_cell, len(every)


# ---------------------------------------------------------------- constructed cases
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("key", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_case_equals_the_model(data, name, key, half):
    path, arrays = data
    host, kw = arrays[chunk(name, key)], CASES[name][1]
    want = model(arrays, name, key, half)
    stored = chunk(name if len(host) else 'one_entry', key)         # no entry: any position chunk, none of its rows
    with fl.open(path, 'r') as f:
        d_rows, d_cell, n = ordered(f, stored, host, ROWS.get(name), want, kw)
        for distances in (True, False):
            got = f.neighbour_list_device(0, stored, kw['box'], kw['r'], want.grid, d_rows, d_cell, n=n,
                                          dimensions=kw.get('dimensions', 3), half=half, distances=distances)
            assert (got.distance2 is not None) == distances and equal(got, want, (name, key, half, distances))
        f.wait_read()
    assert want.n == len(host) if name not in ROWS else want.n == len(ROWS[name])
    if name == 'nothing':
        assert want.n == 0 and _host(got.offsets).tolist() == [0]
    if name == 'exactly_r':
        assert want.pairs == 0
    if name == 'clump_700':
        assert want.longest == 699 and want.pairs == (700 * 699 + 2) // (2 if half else 1)
    if name == 'three_cells_4097':
        assert want.nowhere > 0 and want.pairs > 4097
    if name == 'all_nowhere':
        assert want.nowhere == 100 and want.pairs == 0
    if name == 'sparse_64cubed':
        assert want.n == 65537 and want.grid == (64, 64, 64) and want.pairs > 10000 // (2 if half else 1)
    if name.startswith('x_runs'):
        assert want.nowhere == 0 and want.pairs > 0


@pytest.mark.parametrize("key", sorted(DTYPES))
def test_lists_with_repeats_in_any_order(data, key):
    """A list in descending order with rows listed twice: two entries of one row are each other's neighbour at distance 0."""
    path, arrays = data
    name = chunk('three_cells_4097', key)
    host, kw = arrays[name], CASES['three_cells_4097'][1]
    rows = np.concatenate([np.arange(400, 0, -1), [7, 7, 400, 12]])
    with fl.open(path, 'r') as f:
        for half in (False, True):
            want = hoomd.neighbour_list(host, rows=rows, half=half, distances=True, **kw)
            d_rows, d_cell, n = ordered(f, name, host, rows, want, kw)
            got = f.neighbour_list_device(0, name, kw['box'], kw['r'], want.grid, d_rows, d_cell, n=n, half=half, distances=True)
            assert equal(got, want, (key, half)) and got.n == 404 and _host(got.distance2).min() == 0.0
        f.wait_read()


# ---------------------------------------------------------------- the protocol of the two calls
D, U = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
_HEAD = [ctypes.POINTER(_lib.Handle), ctypes.POINTER(_lib.IndexEntry), D, ctypes.c_double, ctypes.c_uint32, U,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]


def _entry_points():
    offsets_fn, fill_fn = _lib.lib.pgsd_neighbour_offsets_device, _lib.lib.pgsd_neighbour_list_device
    offsets_fn.restype = fill_fn.restype = ctypes.c_int32
    offsets_fn.argtypes = _HEAD + [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    fill_fn.argtypes = _HEAD + [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return offsets_fn, fill_fn


class Protocol(object):
    """The two entry points over the first 500 rows of the triclinic particles' own position chunk; a refusal raises
    ValueError with the library's message, as the binding does."""

    def __init__(self, f, host, r=1.2, n=500):
        self.f, self.h, self.n, self.r, self.host = f, f._h(), n, r, host
        self.offsets_fn, self.fill_fn = _entry_points()
        self.full = hoomd.neighbour_list(host, TRICLINIC, r, rows=np.arange(n), cells=(7, 5, 4), distances=True)
        self.entry = _lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(self.h, 0, b'particles/position').contents)
        self.rows, self.cell = to_device(f, self.full.rows), to_device(f, self.full.cell)
        self.vectors = hoomd.box_vectors(np.asarray(TRICLINIC, np.float32))

    def _head(self, r, flags, cell=None):
        return (self.h, ctypes.byref(self.entry), (ctypes.c_double * 6)(*self.vectors), r, 3, (ctypes.c_uint32 * 3)(7, 5, 4),
                _ptr(self.rows), _ptr(self.cell if cell is None else cell), self.n, flags)

    @staticmethod
    def _checked(rc):
        if rc == _lib.ERROR_INVALID_ARGUMENT:
            raise ValueError(_lib.last_error())
        assert rc == 0, (rc, _lib.last_error())

    def offsets(self, r=None, flags=0, cell=None):
        """(offsets in GPU memory, the four summary words)"""
        out = device_buffer(self.f, np.full(self.n + 1, 77), np.uint64)
        summary = (ctypes.c_uint64 * 4)(77, 77, 77, 77)
        try:
            self._checked(self.offsets_fn(*(self._head(self.r if r is None else r, flags, cell) + (_ptr(out), summary))))
        except ValueError:
            assert list(summary) == [77] * 4 and _host(out).tolist() == [77] * (self.n + 1)    # written on success only
            raise
        return out, np.array(list(summary), np.uint64)

    def fill(self, offsets, capacity, distances=True, flags=0):
        """(neighbours, distance2) on the host, guard words behind the capacity included; ValueError: the same behind
        ``self.refused``."""
        room = capacity + GUARD_WORDS
        nb = device_buffer(self.f, np.full(room, GUARD), np.uint32)
        d2 = device_buffer(self.f, np.full(room, GUARD), np.uint64) if distances else None
        try:
            self._checked(self.fill_fn(*(self._head(self.r, flags) + (_ptr(offsets), capacity, _ptr(nb),
                                                                      _ptr(d2) if distances else None))))
        finally:
            self.refused = (_host(nb), _host(d2) if distances else None)
        return self.refused

    def guard_holds(self, capacity):
        nb, d2 = self.refused
        return (nb[capacity:] == GUARD).all() and len(nb) == capacity + GUARD_WORDS and (d2 is None or (d2[capacity:] == GUARD).all())


@pytest.fixture()
def protocol(data):
    path, _ = data
    with hoomd.open(path, 'r') as t:
        host = t[0].particles.position
    with fl.open(path, 'r') as f:
        yield Protocol(f, host)
        f.wait_read()


def test_the_offsets_call_alone_and_the_fill_at_the_exact_capacity(protocol):
    want = protocol.full
    offsets, summary = protocol.offsets()
    assert np.array_equal(_host(offsets), want.offsets) and np.array_equal(summary, want.summary) and want.pairs > 500
    nb, d2 = protocol.fill(offsets, want.pairs)
    assert np.array_equal(nb[:want.pairs], want.neighbours) and protocol.guard_holds(want.pairs)
    assert np.array_equal(d2[:want.pairs], want.distance2.view(np.uint64))
    nb, d2 = protocol.fill(offsets, want.pairs, distances=False)
    assert d2 is None and np.array_equal(nb[:want.pairs], want.neighbours) and protocol.guard_holds(want.pairs)
    # the half list: bit 0 of flags, in both calls
    half = hoomd.neighbour_list(protocol.host, TRICLINIC, protocol.r, rows=np.arange(protocol.n), cells=(7, 5, 4),
                                half=True)
    offsets, summary = protocol.offsets(flags=1)
    assert np.array_equal(_host(offsets), half.offsets) and np.array_equal(summary, half.summary)
    nb, _ = protocol.fill(offsets, half.pairs, flags=1)
    assert np.array_equal(nb[:half.pairs], half.neighbours) and protocol.guard_holds(half.pairs)


def test_a_capacity_that_is_too_small_is_refused_and_nothing_lands_behind_it(protocol):
    want = protocol.full
    offsets, _ = protocol.offsets()
    capacity = want.pairs - 1
    with pytest.raises(ValueError, match="capacity of %d entries is too small for the %d pairs" % (capacity, want.pairs)):
        protocol.fill(offsets, capacity)
    assert protocol.guard_holds(capacity)
    # every segment that ends inside the capacity was filled or left alone; none was written outside itself
    nb = protocol.refused[0]
    whole = int(want.offsets[np.nonzero(want.counts > 0)[0][-1]])       # where the last segment that holds a pair begins
    assert np.array_equal(nb[:whole], want.neighbours[:whole])
    with pytest.raises(ValueError, match="too small"):
        protocol.fill(offsets, 0, distances=False)
    assert protocol.guard_holds(0)
    # the handle is usable: the next good call equals the model
    nb, d2 = protocol.fill(offsets, want.pairs)
    assert np.array_equal(nb[:want.pairs], want.neighbours) and np.array_equal(d2[:want.pairs], want.distance2.view(np.uint64))


def test_offsets_of_another_list_are_refused_and_nothing_lands_behind_the_capacity(protocol):
    want = protocol.full
    # the offsets of a smaller range on the same rows: they ascend and fit, but every busy entry finds more than they hold
    fewer, summary = protocol.offsets(r=0.9)
    assert 0 < int(summary[2]) < want.pairs
    with pytest.raises(ValueError, match="do not belong to this list"):
        protocol.fill(fewer, want.pairs)
    assert protocol.guard_holds(want.pairs)
    # ... and those of a larger one, declared with the capacity of this list: more pairs than the capacity
    more, summary = protocol.offsets(r=1.3)
    assert int(summary[2]) > want.pairs
    with pytest.raises(ValueError, match="too small"):
        protocol.fill(more, want.pairs)
    assert protocol.guard_holds(want.pairs)
    # ... and with room for them: the segments are another list's
    with pytest.raises(ValueError, match="do not belong to this list"):
        protocol.fill(more, int(summary[2]))
    assert protocol.guard_holds(int(summary[2]))
    # offsets that descend, and offsets that do not begin at 0
    down = want.offsets.copy()
    k = int(np.nonzero(want.counts > 0)[0][1])      # the second entry that has a neighbour: its segment begins above 0
    down[k + 1] = down[k] - 1
    with pytest.raises(ValueError, match="do not belong to this list"):
        protocol.fill(device_buffer(protocol.f, down, np.uint64), want.pairs)
    assert protocol.guard_holds(want.pairs)
    with pytest.raises(ValueError, match="do not belong to this list"):
        protocol.fill(device_buffer(protocol.f, want.offsets + np.uint64(1), np.uint64), want.pairs + 1)
    assert protocol.guard_holds(want.pairs + 1)
    offsets, _ = protocol.offsets()
    nb, _ = protocol.fill(offsets, want.pairs)
    assert np.array_equal(nb[:want.pairs], want.neighbours)


def test_undefined_flag_bits_and_the_refusals_of_the_census(protocol):
    want = protocol.full
    offsets, _ = protocol.offsets()
    for flags in (2, 3, 1 << 31):
        with pytest.raises(ValueError, match="undefined bits"):
            protocol.offsets(flags=flags)
        with pytest.raises(ValueError, match="undefined bits"):
            protocol.fill(offsets, want.pairs, flags=flags)
        assert protocol.guard_holds(want.pairs) and (protocol.refused[0] == GUARD).all()
    for r, message in ((0.0, "finite and positive"), (float('nan'), "finite and positive"), (1.5, "narrower than the range"),
                       (0.5, None)):
        if message is None:
            protocol.offsets(r=r)               # (cells wider than the range are fine)
            continue
        with pytest.raises(ValueError, match=message):
            protocol.offsets(r=r)
    descending = want.cell.copy()
    descending[300] = 0
    with pytest.raises(ValueError, match="descends or lies outside"):
        protocol.offsets(cell=to_device(protocol.f, descending))
    # through the binding: ValueError, and the next good call equals the model
    f = protocol.f
    with pytest.raises(ValueError, match="narrower"):
        f.neighbour_list_device(0, 'particles/position', TRICLINIC, protocol.r, (8, 5, 4), protocol.rows, protocol.cell, n=protocol.n)
    with pytest.raises(ValueError, match="fewer entries than n"):
        f.neighbour_list_device(0, 'particles/position', TRICLINIC, protocol.r, (7, 5, 4), protocol.rows, protocol.cell, n=501)
    with pytest.raises(ValueError, match="float32 or float64"):
        f.neighbour_list_device(0, 'particles/typeid', TRICLINIC, protocol.r, (7, 5, 4), protocol.rows, protocol.cell, n=protocol.n)
    got = f.neighbour_list_device(0, 'particles/position', TRICLINIC, protocol.r, (7, 5, 4), protocol.rows, protocol.cell,
                                  n=protocol.n, distances=True)
    assert equal(got, want, "after the refusals")


# ---------------------------------------------------------------- against the units that exist
def test_the_counts_equal_the_census_on_the_same_list(protocol):
    f, want = protocol.f, protocol.full
    census = f.neighbours_device(0, 'particles/position', TRICLINIC, protocol.r, (7, 5, 4), protocol.rows, protocol.cell, n=protocol.n,
                                 return_rows=True)
    got = f.neighbour_list_device(0, 'particles/position', TRICLINIC, protocol.r, (7, 5, 4), protocol.rows, protocol.cell, n=protocol.n)
    assert np.array_equal(np.diff(_host(got.offsets)), _host(census.count).view(np.uint32))
    assert got.pairs == census.pairs and got.nowhere == census.nowhere and got.longest == census.count_max
    assert np.array_equal(want.counts, _host(census.count).view(np.uint32))


WHERE = {'type': ['fluid', 'inlet'], 'density': (990.0, 1040.0)}
CELL = hoomd.domain_grid(2, 2, 1)[1]
SELECTIONS = {"all": {}, "where": {'where': WHERE}, "domain": {'domain': CELL}, "both": {'where': WHERE, 'domain': CELL}}


@pytest.mark.parametrize("selection", sorted(SELECTIONS))
def test_frame_neighbour_list_device_equals_the_host_model(data, selection):
    path, _ = data
    kwargs = SELECTIONS[selection]
    with hoomd.open(path, 'r') as t:
        for options in (dict(r=0.61), dict(r=1.3, cells=(5, 5, 3), half=True, distances=True)):
            want = t.frame_neighbour_list(0, **options, **kwargs)
            t.file.device_read_stats(reset=True)
            got = t.frame_neighbour_list_device(0, **options, **kwargs)
            pread = t.file.device_read_stats()["pread_bytes"]
            assert equal(got, want, (selection, options))
            # the position is read once -- by the selection, the ordering or the passes --, and the selection's typeid and density
            assert pread == N * (12 + (8 if 'where' in kwargs else 0)), (selection, options)
        if selection == "all":
            assert got.n == N and got.nowhere > 0
        else:
            assert 0 < got.n < N
        with pytest.raises(ValueError, match="narrower"):
            t.frame_neighbour_list_device(0, 1.3, cells=(8, 5, 4), **kwargs)
        with pytest.raises(ValueError, match="count twice"):
            t.frame_neighbour_list_device(0, 3.5, **kwargs)
        with pytest.raises(IndexError):
            t.frame_neighbour_list_device(1, 1.3)


def test_the_list_indexes_a_frame_restarted_in_cell_order(data):
    """read_frame_device(where=W, cell_order=grid) and frame_neighbour_list_device(where=W, cells=grid): row k of the
    restarted arrays is list position k, so `neighbours` indexes them directly."""
    path, _ = data
    grid = (5, 5, 3)
    with hoomd.open(path, 'r') as t:
        stored = t[0].particles
        for kwargs in ({'where': WHERE}, {'domain': CELL}):
            snap = t.read_frame_device(0, cell_order=grid, **kwargs)
            got = t.frame_neighbour_list_device(0, 1.3, cells=grid, distances=True, **kwargs)
            rows = _host(got.rows)
            position = _host(snap.particles.position)
            assert snap.particles.N == got.n == len(rows)
            assert position.tobytes() == stored.position[rows].tobytes()
            assert np.array_equal(_host(snap.particles.typeid), stored.typeid[rows])
            # ... hence the distances of the list are those of the restarted rows
            offsets, nb = _host(got.offsets), _host(got.neighbours).astype(np.int64)
            i = np.repeat(np.arange(got.n), np.diff(offsets).astype(np.int64))
            d2 = hoomd.pair_distance2(position[i], position[nb], hoomd.box_vectors(np.asarray(TRICLINIC, np.float32)))
            assert got.pairs > 0 and np.array_equal(d2.view(np.uint64), _host(got.distance2).view(np.uint64))


CHILD = r'''
import os, sys
sys.modules["torch"] = None                    # `import torch` raises ImportError from here on
root, path = sys.argv[1:3]
sys.path[:0] = [os.path.join(root, "pgsd-sph_amd"), os.path.join(root, "tests")]
import numpy as np
import pgsd.fl as fl
import pgsd.hoomd as hoomd
from pgsd import _lib
assert _lib._torch is None
try:
    import torch
    raise SystemExit("torch imported")
except ImportError:
    pass
with hoomd.open(path, "r") as t:
    for options in (dict(), dict(half=True, distances=True, where={"type": ["fluid"]})):
        want = t.frame_neighbour_list(0, 1.3, **options)
        got = t.frame_neighbour_list_device(0, 1.3, **options)
        for name in ("rows", "cell", "offsets", "neighbours") + (("distance2",) if options else ()):
            a = getattr(got, name)
            assert isinstance(a, fl.DeviceBuffer), (name, type(a))
            assert np.array_equal(a.to_host(), getattr(want, name)), name
            if name == "distance2":
                assert a.to_host().tobytes() == want.distance2.tobytes()
        assert np.array_equal(got.summary, want.summary) and got.pairs > 0
print("TORCH_FREE_OK")
'''


def test_the_list_needs_no_tensor_library(data, tmp_path):
    path, _ = data
    script = str(tmp_path / "child.py")
    with open(script, "w") as fh:
        fh.write(CHILD)
    p = subprocess.run([sys.executable, script, product.ROOT, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "TORCH_FREE_OK" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
