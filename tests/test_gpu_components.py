"""Components on the GPU: pgsd_components_device behind pgsd.fl's components_device and pgsd.hoomd's
frame_components_device.  The three arrays and the summary must equal the numpy model pgsd.hoomd.neighbour_components /
frame_components exactly -- numpy.array_equal (tests/test_components_model.py checks the model itself against a plain
breadth-first labelling).  The cases at the pgsd.fl level read constructed position chunks, once as float32 and once as
float64, and order the list on the GPU first, as a caller does; the protocol tests call the entry point itself, with output
buffers that are 64 guard words longer than n."""
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
from components_cases import CUBE, MUTATIONS, TIES  # noqa: E402

WIDE = [64, 64, 64, 0, 0, 0]
N = 3001
TYPES = ['fluid', 'wall', 'inlet']
DTYPES = {'f32': np.float32, 'f64': np.float64}
GUARD = 0xA5A5A5A5
GUARD_WORDS = 64


def _line(k, y=0.0):
    """k entries at spacing 0.0125 along x of the 8-cube, from the face on: 640 of them close the ring."""
    return np.stack([-4.0 + 0.0125 * np.arange(k), np.full(k, y), np.zeros(k)], axis=1)


def _clump():
    """The neighbour list tests' clump: 700 entries inside one cell of the (3, 3, 3) grid -- more than a workgroup, every
    one within the range of every other -- and three rows elsewhere, two of them a pair."""
    rng = np.random.default_rng(8)
    return np.concatenate([rng.uniform(-0.5, 0.5, size=(700, 3)), [[3.5, 3.5, 3.5], [3.6, 3.5, 3.5], [-3.9, 0, 0]]])


def _sparse():
    """The neighbour list tests' sparse frame: 65 537 rows in 64^3 cells -- 257 workgroups, the smallest count at which
    the one-workgroup scan takes a second round --; 16 384 of the rows have a partner inside the range."""
    a = random_rows(9, 49153, WIDE, np.float64)
    return np.concatenate([a, a[:16384] + np.random.default_rng(10).uniform(-0.5, 0.5, size=(16384, 3))])


def _with_lost_rows(p, every=97):
    p = p.copy()
    p[5::every, 0] = np.nan
    p[11::every, 1] = np.inf
    return p


# name -> (positions as float64, keyword arguments of neighbour_components besides position)
CASES = {
    'nothing': (np.zeros((0, 3)), dict(box=CUBE, r=1.0)),
    'one_entry': (np.array([[1.0, 2, 3]]), dict(box=CUBE, r=1.0)),
    'exactly_r': (np.array([[0, 0, 0], [0.5, 0, 0]], np.float64), dict(box=CUBE, r=0.5)),
    'all_nowhere': (np.full((100, 3), np.nan), dict(box=CUBE, r=1.0)),
    'ring_640': (_line(640), dict(box=CUBE, r=0.013, cells=(64, 1, 1))),
    'chain_639': (_line(639), dict(box=CUBE, r=0.013, cells=(64, 1, 1))),
    'two_rails': (np.concatenate([_line(639), _line(639, 0.05)]), dict(box=CUBE, r=0.013, cells=(64, 1, 1))),
    'hub_700': (_clump(), dict(box=CUBE, r=2.0, cells=(3, 3, 3))),
    'percolating_4097': (_with_lost_rows(random_rows(4, 4097, CUBE, np.float64)), dict(box=CUBE, r=0.45, cells=(16, 16, 16))),
    'dust_4097': (_with_lost_rows(random_rows(4, 4097, CUBE, np.float64)), dict(box=CUBE, r=0.4, cells=(16, 16, 16))),
    'triclinic_3001': (random_rows(7, 3001, TRICLINIC, np.float64), dict(box=TRICLINIC, r=0.5)),
    'flat_600': (random_rows(42, 600, FLAT, np.float64, 2), dict(box=FLAT, r=0.4, dimensions=2)),
    'sparse_64cubed': (_sparse(), dict(box=WIDE, r=1.0, cells=(64, 64, 64))),
}
ROWS = {}                                   # name -> the row list of a case that has one (default: every row)
for _k, (_name, _case) in enumerate([(k, v[1]) for k, v in sorted(MUTATIONS.items())] + sorted(TIES.items())):
    _kw = dict(_case)
    if 'rows' in _kw:
        ROWS['mutation_%02d' % _k] = _kw.pop('rows')
    CASES['mutation_%02d' % _k] = (np.asarray(_kw.pop('position'), np.float64), _kw)

# (n, nowhere, components, singletons, largest, largest_label) of the cases whose structure is known by construction
KNOWN = {
    'nothing': (0, 0, 0, 0, 0, 0),
    'one_entry': (1, 0, 1, 1, 1, 0),
    'exactly_r': (2, 0, 2, 2, 1, 0),
    'all_nowhere': (100, 100, 100, 100, 1, 0),
    'ring_640': (640, 0, 1, 0, 640, 0),
    'chain_639': (639, 0, 1, 0, 639, 0),
    'two_rails': (1278, 0, 2, 0, 639, 0),
}


def chunk(name, key):
    return 'log/%s_%s' % (name, key)


def _dir(tmp_path_factory, name):
    return "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp(name))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """One file of one frame: 3 001 particles with types and random positions in the triclinic box (the pgsd.hoomd level),
    and every case's positions as a float32 and a float64 log chunk.  The host's arrays beside it."""
    path = os.path.join(_dir(tmp_path_factory, "components"), "pgsd_components_%d.gsd" % os.getpid())
    rng = np.random.default_rng(N)
    fr = hoomd.Frame()
    fr.configuration.box = TRICLINIC
    fr.particles.N = N
    fr.particles.types = TYPES
    fr.particles.position = _with_lost_rows(random_rows(7, N, TRICLINIC, np.float32), 997)
    fr.particles.typeid = rng.integers(0, len(TYPES), size=N).astype(np.uint32)
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


def model(arrays, name, key):
    """The model's components of a case, computed once."""
    at = (name, key)
    if at not in _MODEL:
        _MODEL[at] = hoomd.neighbour_components(arrays[chunk(name, key)], rows=ROWS.get(name), **CASES[name][1])
    return _MODEL[at]


def to_device(f, a):
    return fl._device_from_host(np.ascontiguousarray(a, dtype=np.int32), f.pipeline_device())


def device_buffer(f, a, dtype):
    """A library-owned buffer that holds the host array ``a`` as ``dtype`` (outputs with a guard pattern)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    return fl.DeviceBuffer((a.size,), dtype, f.pipeline_device(), pattern=a)


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr() if hasattr(x, 'data_ptr') else x.ptr)


def equal(got, want, what):
    """The kernels' Components (arrays in GPU memory) against the model's."""
    assert np.array_equal(got.summary, want.summary), (what, got, want)
    assert got.grid == want.grid and got.r == want.r and got.dimensions == want.dimensions, what
    assert np.array_equal(_host(got.rows), want.rows) and np.array_equal(_host(got.cell), want.cell), what
    for name in ('label', 'component', 'sizes'):
        a, b = _host(getattr(got, name)), getattr(want, name)
        assert a.dtype == np.uint32 and a.shape == b.shape and np.array_equal(a, b), (what, name)
    for call in (lambda: got.members(0), got.fragments):
        with pytest.raises(ValueError, match="GPU memory"):
            call()
    return True


def ordered(f, name, host, rows, want, kw):
    """The list sorted by cell on the GPU, as a caller does: (rows, cell, entries)."""
    every = np.arange(len(host)) if rows is None else np.asarray(rows)
    d_rows = to_device(f, every)
    d_cell = f.order_rows_by_cell_device(0, name, kw['box'], want.grid, d_rows, n=len(every), dimensions=kw.get('dimensions', 3))
    return d_rows, d_cell, len(every)


def run(f, arrays, name, key):
    host, kw = arrays[chunk(name, key)], CASES[name][1]
    want = model(arrays, name, key)
    stored = chunk(name if len(host) else 'one_entry', key)         # no entry: any position chunk, none of its rows
    d_rows, d_cell, n = ordered(f, stored, host, ROWS.get(name), want, kw)
    return f.components_device(0, stored, kw['box'], kw['r'], want.grid, d_rows, d_cell, n=n, dimensions=kw.get('dimensions', 3))


# ---------------------------------------------------------------- constructed cases
@pytest.mark.parametrize("key", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_case_equals_the_model(data, name, key):
    path, arrays = data
    want = model(arrays, name, key)
    with fl.open(path, 'r') as f:
        got = run(f, arrays, name, key)
        assert equal(got, want, (name, key))
        f.wait_read()
    s = tuple(int(v) for v in want.summary)
    assert want.n == (len(ROWS[name]) if name in ROWS else len(arrays[chunk(name, key)]))
    assert int(want.sizes.astype(np.int64).sum()) == want.n
    if name in KNOWN:
        assert s == KNOWN[name]
    if name == 'two_rails':
        assert want.sizes.tolist() == [639, 639] and len(set(want.component[:20].tolist())) == 2    # interleaved in a cell
    if name == 'hub_700':
        assert want.sizes.tolist().count(700) == 1 and sorted(want.sizes.tolist()) == [1, 2, 700] and want.largest == 700
    if name == 'percolating_4097':
        # (370 components, 195 singletons and one of 2 676 entries before the rows are lost; after them, from the model:)
        assert s == (4097, 86, 474, 290, 2418, 1)
    if name == 'dust_4097':
        # (958 components, the largest 64, before the rows are lost)
        assert s == (4097, 86, 1054, 581, 56, 113)
    if name in ('triclinic_3001', 'flat_600'):
        assert want.nowhere == 0 and 1 < want.components < want.n and want.largest > 2
    if name == 'sparse_64cubed':
        assert want.n == 65537 and want.grid == (64, 64, 64) and want.components < 65537 - 10000 and want.largest >= 2


def test_two_runs_in_one_process_are_identical(data):
    """The hooks race; the result does not: it is unique."""
    path, arrays = data
    with fl.open(path, 'r') as f:
        first = run(f, arrays, 'percolating_4097', 'f32')
        second = run(f, arrays, 'percolating_4097', 'f32')
        for name in ('label', 'component', 'sizes'):
            assert _host(getattr(first, name)).tobytes() == _host(getattr(second, name)).tobytes(), name
        assert np.array_equal(first.summary, second.summary) and first.components > 100
        f.wait_read()


# ---------------------------------------------------------------- the protocol of the call
D, U = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
_ARGS = [ctypes.POINTER(_lib.Handle), ctypes.POINTER(_lib.IndexEntry), D, ctypes.c_double, ctypes.c_uint32, U,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]


class Protocol(object):
    """The entry point over the first 500 rows of the triclinic particles' own position chunk; a refusal raises
    ValueError with the library's message, as the binding does."""

    def __init__(self, f, host, r=0.9, n=500):
        self.f, self.h, self.n, self.r, self.host = f, f._h(), n, r, host
        self.fn = _lib.lib.pgsd_components_device
        self.fn.restype, self.fn.argtypes = ctypes.c_int32, _ARGS
        self.want = hoomd.neighbour_components(host, TRICLINIC, r, rows=np.arange(n), cells=(7, 5, 4))
        self.entry = _lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(self.h, 0, b'particles/position').contents)
        self.rows, self.cell = to_device(f, self.want.rows), to_device(f, self.want.cell)
        self.vectors = hoomd.box_vectors(np.asarray(TRICLINIC, np.float32))

    def call(self, r=None, flags=0, cells=(7, 5, 4), rows=None, cell=None, n=None, component=True, sizes=True):
        """(label, component, sizes, summary) on the host, guard words included; the outputs that were not asked for are
        None.  ValueError: the summary was left alone."""
        n = self.n if n is None else n
        out = [device_buffer(self.f, np.full(n + GUARD_WORDS, GUARD), np.uint32) if asked else None
               for asked in (True, component, sizes)]
        summary = (ctypes.c_uint64 * 6)(*([77] * 6))
        rc = self.fn(self.h, ctypes.byref(self.entry), (ctypes.c_double * 6)(*self.vectors), self.r if r is None else r, 3,
                     (ctypes.c_uint32 * 3)(*cells), _ptr(self.rows if rows is None else rows),
                     _ptr(self.cell if cell is None else cell), n, flags, *[None if o is None else _ptr(o) for o in out],
                     summary)
        if rc == _lib.ERROR_INVALID_ARGUMENT:
            assert list(summary) == [77] * 6                        # written on success only
            raise ValueError(_lib.last_error())
        assert rc == 0, (rc, _lib.last_error())
        return tuple(None if o is None else _host(o) for o in out) + (np.array(list(summary), np.uint64),)


@pytest.fixture()
def protocol(data):
    path, _ = data
    with hoomd.open(path, 'r') as t:
        host = t[0].particles.position
    with fl.open(path, 'r') as f:
        yield Protocol(f, host)
        f.wait_read()


def test_no_store_lands_behind_n_and_the_optional_outputs_may_be_null(protocol):
    want, n = protocol.want, protocol.n
    assert 1 < want.components < n and want.largest > 2
    for component, sizes in ((True, True), (False, True), (True, False), (False, False)):
        label, comp, size, summary = protocol.call(component=component, sizes=sizes)
        assert np.array_equal(summary, want.summary), (component, sizes)
        assert len(label) == n + GUARD_WORDS and np.array_equal(label[:n], want.label) and (label[n:] == GUARD).all()
        assert (comp is not None) == component and (size is not None) == sizes
        if component:
            assert np.array_equal(comp[:n], want.component) and (comp[n:] == GUARD).all()
        if sizes:
            assert np.array_equal(size[:want.components], want.sizes) and (size[n:] == GUARD).all()


def test_flags_and_the_refusals_of_the_census(protocol):
    want = protocol.want
    for flags in (1, 2, 1 << 31):
        with pytest.raises(ValueError, match="undefined bits"):
            protocol.call(flags=flags)
    for r, cells, message in ((0.0, (7, 5, 4), "finite and positive"), (float('nan'), (7, 5, 4), "finite and positive"),
                              (3.5, (1, 1, 1), "an image would count twice"), (1.5, (7, 5, 4), "narrower than the range")):
        with pytest.raises(ValueError, match=message):
            protocol.call(r=r, cells=cells)
    descending = want.cell.copy()
    descending[300] = 0
    with pytest.raises(ValueError, match="descends or lies outside"):
        protocol.call(cell=to_device(protocol.f, descending))
    beyond = want.rows.copy()
    beyond[17] = N
    with pytest.raises(ValueError, match="an entry of the row list lies outside"):
        protocol.call(rows=to_device(protocol.f, beyond))
    # no entry: nothing is staged or launched, the outputs are left alone and the summary is six zeros
    protocol.f.wait_read()
    protocol.f.device_read_stats(reset=True)
    label, comp, size, summary = protocol.call(n=0)
    assert summary.tolist() == [0] * 6 and all((a == GUARD).all() and len(a) == GUARD_WORDS for a in (label, comp, size))
    assert protocol.f.device_read_stats()["pread_bytes"] == 0
    # through the binding: ValueError, and the next good call equals the model
    f = protocol.f
    with pytest.raises(ValueError, match="narrower"):
        f.components_device(0, 'particles/position', TRICLINIC, protocol.r, (12, 5, 4), protocol.rows, protocol.cell, n=protocol.n)
    with pytest.raises(ValueError, match="fewer entries than n"):
        f.components_device(0, 'particles/position', TRICLINIC, protocol.r, (7, 5, 4), protocol.rows, protocol.cell, n=501)
    with pytest.raises(ValueError, match="float32 or float64"):
        f.components_device(0, 'particles/typeid', TRICLINIC, protocol.r, (7, 5, 4), protocol.rows, protocol.cell, n=protocol.n)
    got = f.components_device(0, 'particles/position', TRICLINIC, protocol.r, (7, 5, 4), protocol.rows, protocol.cell, n=protocol.n)
    assert equal(got, want, "after the refusals")


# ---------------------------------------------------------------- the trajectory level
WHERE = {'type': ['fluid']}


def test_frame_components_device_equals_the_host_model(data):
    path, _ = data
    with hoomd.open(path, 'r') as t:
        for options in (dict(r=0.61, where=WHERE), dict(r=0.9, cells=(5, 5, 3)),
                        dict(r=0.7, where=WHERE, domain=hoomd.domain_grid(2, 2, 1)[1])):
            want = t.frame_components(0, **options)
            got = t.frame_components_device(0, **options)
            assert equal(got, want, options) and 1 < want.components < want.n
        assert got.n < N
        with pytest.raises(ValueError, match="narrower"):
            t.frame_components_device(0, 1.3, cells=(8, 5, 4))
        with pytest.raises(ValueError, match="count twice"):
            t.frame_components_device(0, 3.5)
        with pytest.raises(IndexError):
            t.frame_components_device(1, 1.3)


def test_the_labels_index_a_frame_restarted_in_cell_order(data):
    """read_frame_device(where=W, cell_order=grid) and frame_components_device(where=W, cells=grid): row k of the
    restarted arrays is list position k, so `label` gathers each component's smallest member."""
    path, _ = data
    grid = (5, 5, 3)
    with hoomd.open(path, 'r') as t:
        stored = t[0].particles
        snap = t.read_frame_device(0, cell_order=grid, where=WHERE)
        got = t.frame_components_device(0, 0.9, cells=grid, where=WHERE)
        want = t.frame_components(0, 0.9, cells=grid, where=WHERE)
        assert equal(got, want, "restart")
        position = _host(snap.particles.position)
        label, component = _host(got.label).astype(np.int64), _host(got.component).astype(np.int64)
        assert snap.particles.N == got.n == len(label) and position.tobytes() == stored.position[want.rows].tobytes()
        smallest = np.array([want.members(c)[0] for c in range(want.components)])
        assert position[label].tobytes() == stored.position[want.rows[smallest[component]]].tobytes()
        assert (stored.typeid[want.rows[label]] == TYPES.index('fluid')).all()


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
    for options in (dict(), dict(where={"type": ["fluid"]})):
        want = t.frame_components(0, 0.9, **options)
        got = t.frame_components_device(0, 0.9, **options)
        for name in ("rows", "cell", "label", "component", "sizes"):
            a = getattr(got, name)
            assert isinstance(a, fl.DeviceBuffer), (name, type(a))
            assert np.array_equal(a.to_host(), getattr(want, name)), name
        assert np.array_equal(got.summary, want.summary) and 1 < got.components < got.n
print("TORCH_FREE_OK")
'''


def test_the_components_need_no_tensor_library(data, tmp_path):
    path, _ = data
    script = str(tmp_path / "child.py")
    with open(script, "w") as fh:
        fh.write(CHILD)
    p = subprocess.run([sys.executable, script, product.ROOT, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "TORCH_FREE_OK" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
