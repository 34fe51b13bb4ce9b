"""Component fields on the GPU: pgsd_component_moments_device behind pgsd.fl's component_moments_device and pgsd.hoomd's
frame_component_moments_device.  Every table and the summary must equal the numpy model pgsd.hoomd.component_moments /
frame_component_moments exactly -- the counters with numpy.array_equal, every float bit for bit: the order of a component's
sum is part of the definition (tests/test_component_moments_model.py checks the model itself against plain loops).  The
cases at the pgsd.fl level read constructed chunks, once as float32 and once as float64, order the list and run
components_device on the GPU first, as a caller does; the protocol tests call the entry point itself, with output buffers
that are 64 guard rows longer than `components`."""
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
from components_cases import CUBE  # noqa: E402
from component_moments_cases import MUTATIONS, WIDE_BOX, frame_values, mismatches  # noqa: E402

N = 3001
TYPES = ['fluid', 'wall', 'inlet']
DTYPES = {'f32': np.float32, 'f64': np.float64}
FIELDS = ('mass', 'velocity', 'energy', 'position')
GUARD_ROWS = 64


def _chain(k, x0=-30.0, y=0.0):
    """k entries at spacing 0.0125 along x of the 64-cube: linked at r = 0.013, 25.6 long at k = 2049 (not wide)."""
    return np.stack([x0 + 0.0125 * np.arange(k), np.full(k, y), np.zeros(k)], axis=1)


def _interleaved(k):
    """Two chains of k entries in the same cells, their rows alternating: a segment's entries are not contiguous in the
    list."""
    p = np.zeros((2 * k, 3))
    p[0::2], p[1::2] = _chain(k), _chain(k, y=0.05)
    return p


def _offset_chain(before, k):
    """`before` singletons in the first cell of the x axis (0.05 apart in y), then a chain of k: its first entry lies at
    sorted position `before`."""
    dust = np.stack([np.full(before, -31.5), -30 + 0.05 * np.arange(before), np.zeros(before)], axis=1)
    return np.concatenate([dust, _chain(k, x0=-20.0)])


def _clump():
    rng = np.random.default_rng(8)
    return np.concatenate([rng.uniform(-0.5, 0.5, size=(700, 3)), [[3.5, 3.5, 3.5], [3.6, 3.5, 3.5], [-3.9, 0, 0]]])


def _with_lost_rows(p, every=97):
    p = p.copy()
    p[5::every, 0] = np.nan
    p[11::every, 1] = np.inf
    return p


def _case(position, seed, box, r, rows=None, absent=(), bad_values=False, **kw):
    p = np.asarray(position, np.float64).reshape(-1, 3)
    mass, velocity, energy = frame_values(len(p), seed)
    if bad_values:
        mass[3::41] = np.inf
        mass[4::43] = np.nan
        velocity[7::53, 1] = np.nan
        velocity[9::61, 2] = -np.inf
    case = dict(position=p, mass=mass, velocity=velocity, energy=energy, rows=rows, kw=dict(dict(box=box, r=r), **kw))
    for name in absent:
        case[name] = None
    return case


_CHAINS = dict(box=WIDE_BOX, r=0.013, cells=(64, 1, 1))
_SINGLETONS = dict(box=WIDE_BOX, r=0.001, cells=(64, 64, 64))
CASES = {
    'nothing': _case(np.zeros((0, 3)), 1, CUBE, 1.0),
    'one_entry': _case([[1.0, 2, 3]], 2, CUBE, 1.0),
    'all_nowhere': _case(np.full((100, 3), np.nan), 3, CUBE, 1.0),
    'dust_4097': _case(_with_lost_rows(random_rows(4, 4097, CUBE, np.float64)), 4, CUBE, 0.4, cells=(16, 16, 16)),
    'percolating_4097': _case(_with_lost_rows(random_rows(4, 4097, CUBE, np.float64)), 5, CUBE, 0.45, cells=(16, 16, 16)),
    'triclinic_3001': _case(random_rows(7, 3001, TRICLINIC, np.float64), 6, TRICLINIC, 0.5),
    'flat_600': _case(random_rows(42, 600, FLAT, np.float64, 2), 7, FLAT, 0.4, dimensions=2),
    'hub_700': _case(_clump(), 8, CUBE, 2.0, cells=(3, 3, 3)),
    'chain_1024': _case(_chain(1024), 9, **_CHAINS),
    'chain_1025': _case(_chain(1025), 10, **_CHAINS),
    'chain_2048': _case(_chain(2048), 11, **_CHAINS),
    'chain_2049': _case(_chain(2049), 12, **_CHAINS),
    'interleaved_1025': _case(_interleaved(1025), 13, **_CHAINS),
    'long_from_1023': _case(_offset_chain(1023, 1100), 14, **_CHAINS),
    'singletons_257': _case(random_rows(9, 257, WIDE_BOX, np.float64), 15, **_SINGLETONS),
    'singletons_65537': _case(random_rows(9, 65537, WIDE_BOX, np.float64), 16, **_SINGLETONS),
    'a_row_twice': _case(random_rows(7, 3001, TRICLINIC, np.float64), 17, TRICLINIC, 0.5,
                         rows=np.random.default_rng(17).integers(0, 3001, size=2500)),
    'no_energy_no_velocity': _case(random_rows(7, 3001, TRICLINIC, np.float64), 18, TRICLINIC, 0.5, absent=('energy', 'velocity')),
    'only_position': _case(random_rows(4, 4097, CUBE, np.float64), 19, CUBE, 0.45, cells=(16, 16, 16),
                           absent=('mass', 'energy', 'velocity')),
    'not_finite_values': _case(_with_lost_rows(random_rows(4, 4097, CUBE, np.float64)), 20, CUBE, 0.45, cells=(16, 16, 16),
                               bad_values=True),
}
for _k, (_name, (_, _m)) in enumerate(sorted(MUTATIONS.items())):
    _kw = dict((k, v) for k, v in _m.items() if k not in FIELDS + ('rows',))
    CASES['mutation_%02d' % _k] = dict(dict((k, None if _m.get(k) is None else np.asarray(_m[k], np.float64)) for k in FIELDS),
                                       rows=_m.get('rows'), kw=_kw)

# (n, components, wide components) of the cases whose structure is known by construction
KNOWN = {
    'nothing': (0, 0, 0), 'one_entry': (1, 1, 0), 'all_nowhere': (100, 100, 0), 'chain_1024': (1024, 1, 0),
    'chain_1025': (1025, 1, 0), 'chain_2048': (2048, 1, 0), 'chain_2049': (2049, 1, 0), 'interleaved_1025': (2050, 2, 0),
    'long_from_1023': (2123, 1024, 0), 'singletons_257': (257, 257, 0), 'singletons_65537': (65537, 65537, 0),
}


def chunk(name, field, key):
    return 'log/%s_%s_%s' % (name, field, key)


def _dir(tmp_path_factory, name):
    return "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp(name))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """One file of one frame: 3 001 particles with types, positions in the triclinic box, masses, velocities and energies
    (the pgsd.hoomd level), and every case's four inputs as float32 and as float64 log chunks.  The host's arrays beside
    it."""
    path = os.path.join(_dir(tmp_path_factory, "component_moments"), "pgsd_component_moments_%d.gsd" % os.getpid())
    rng = np.random.default_rng(N)
    fr = hoomd.Frame()
    fr.configuration.box = TRICLINIC
    fr.particles.N = N
    fr.particles.types = TYPES
    fr.particles.position = _with_lost_rows(random_rows(7, N, TRICLINIC, np.float32), 997)
    fr.particles.typeid = rng.integers(0, len(TYPES), size=N).astype(np.uint32)
    fr.particles.mass, fr.particles.velocity, fr.particles.energy = frame_values(N, N, np.float32, spread=6)
    arrays = {}
    for name, case in CASES.items():
        for key, dt in DTYPES.items():
            for field in FIELDS:
                if case[field] is None:
                    continue
                a = np.ascontiguousarray(case[field].astype(dt))
                arrays[chunk(name, field, key)] = a
                if len(a):                  # (no entry: there is no chunk to store; the case reads another one)
                    fr.log[chunk(name, field, key)[4:]] = a
    with hoomd.open(path, 'w') as t:
        t.append(fr)
    yield path, arrays
    os.unlink(path)


_MODEL = {}


def model(arrays, name, key):
    """(the model's components, the model's moments) of a case, computed once."""
    at = (name, key)
    if at not in _MODEL:
        case = CASES[name]
        given = [arrays.get(chunk(name, field, key)) for field in FIELDS]
        comps = hoomd.neighbour_components(given[3], rows=case['rows'], **case['kw'])
        _MODEL[at] = (comps, hoomd.component_moments(given[0], given[1], given[2], given[3], case['kw']['box'], comps.label,
                                                     comps.component, rows=comps.rows,
                                                     dimensions=case['kw'].get('dimensions', 3)))
    return _MODEL[at]


def to_device(f, a):
    return fl._device_from_host(np.ascontiguousarray(a, dtype=np.int32), f.pipeline_device())


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr() if hasattr(x, 'data_ptr') else x.ptr)


def run(f, arrays, name, key):
    """Order the list, run the components pass, then the moments -- all on the GPU."""
    case, kw = CASES[name], CASES[name]['kw']
    comps, _ = model(arrays, name, key)
    stored = name if len(case['position']) else 'one_entry'         # no entry: any chunks, none of their rows
    every = np.arange(len(case['position'])) if case['rows'] is None else np.asarray(case['rows'])
    dims = kw.get('dimensions', 3)
    d_rows = to_device(f, every)
    d_cell = f.order_rows_by_cell_device(0, chunk(stored, 'position', key), kw['box'], comps.grid, d_rows, n=len(every),
                                         dimensions=dims)
    found = f.components_device(0, chunk(stored, 'position', key), kw['box'], kw['r'], comps.grid, d_rows, d_cell, n=len(every),
                                dimensions=dims)
    chunks = [None if CASES[stored][field] is None else (0, chunk(stored, field, key)) for field in FIELDS]
    got = f.component_moments_device(chunks, kw['box'], found.rows, found.label, found.component, found.n, found.components,
                                     dimensions=dims)
    return found, got


def equal(got, want, what):
    """The kernels' ComponentMoments (tables in GPU memory) against the model's."""
    for call in (lambda: got.centre_of_mass, lambda: got.span, lambda: got.heaviest(1)):
        with pytest.raises(ValueError, match="GPU memory"):
            call()
    assert got.mass.shape == (want.components,) and got.momentum.shape == (want.components, 3), what
    host = got.to_host()
    assert mismatches(host, want) == [], (what, host, want)
    return True


# ---------------------------------------------------------------- constructed cases
@pytest.mark.parametrize("key", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_case_equals_the_model(data, name, key):
    path, arrays = data
    comps, want = model(arrays, name, key)
    with fl.open(path, 'r') as f:
        found, got = run(f, arrays, name, key)
        assert np.array_equal(found.summary, comps.summary)
        assert equal(got, want, (name, key))
        f.wait_read()
    assert want.n == comps.n and want.components == comps.components
    if name in KNOWN:
        assert (want.n, want.components, want.wide_components) == KNOWN[name]
    if name.startswith('chain_') or name == 'interleaved_1025':
        assert comps.largest == int(name.split('_')[1]) and want.bad_entries == 0
    if name == 'long_from_1023':
        assert comps.sizes.tolist() == [1] * 1023 + [1100]          # the long component's first entry: sorted position 1023
    if name == 'interleaved_1025':
        assert len(set(comps.component[:20].tolist())) == 2          # interleaved in the list
    if name == 'percolating_4097':
        assert want.wide_components >= 1 and want.widest_id == int(np.argmax(comps.sizes))
    if name == 'not_finite_values':
        assert want.bad_entries > 150 and (want.bad > 0).sum() > 10
    if name == 'a_row_twice':
        assert len(np.unique(comps.rows)) < comps.n
    if name in ('only_position', 'no_energy_no_velocity'):
        assert not want.kinetic.any() and not want.internal.any() and want.mass.any()
    if name == 'only_position':
        assert np.array_equal(want.mass, comps.sizes.astype(np.float64))


def test_two_runs_in_one_process_are_identical(data):
    path, arrays = data
    with fl.open(path, 'r') as f:
        first = run(f, arrays, 'percolating_4097', 'f32')[1].to_host()
        second = run(f, arrays, 'percolating_4097', 'f32')[1].to_host()
        assert mismatches(first, second) == [] and first.components > 100
        f.wait_read()


# ---------------------------------------------------------------- the protocol of the call
D = ctypes.POINTER(ctypes.c_double)
E = ctypes.POINTER(_lib.IndexEntry)
_ARGS = [ctypes.POINTER(_lib.Handle), E, E, E, E, D, D, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.POINTER(ctypes.c_uint64)]
GUARD_F, GUARD_U = -1234.5, 0xA5A5A5A5


class Protocol(object):
    """The entry point over the first 500 rows of the triclinic particles' own chunks; a refusal raises ValueError with the
    library's message, as the binding does."""

    def __init__(self, f, frame, r=0.9, n=500):
        self.f, self.h, self.n, self.position = f, f._h(), n, frame.particles.position
        self.fn = _lib.lib.pgsd_component_moments_device
        self.fn.restype, self.fn.argtypes = ctypes.c_int32, _ARGS
        p = frame.particles
        self.comps = hoomd.neighbour_components(p.position, TRICLINIC, r, rows=np.arange(n), cells=(7, 5, 4))
        self.want = hoomd.component_moments(p.mass, p.velocity, p.energy, p.position, TRICLINIC, self.comps.label,
                                            self.comps.component, rows=self.comps.rows)
        self.entries = [_lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(self.h, 0, ('particles/' + name).encode()).contents)
                        for name in FIELDS]
        self.lists = dict(rows=to_device(f, self.comps.rows), label=to_device(f, self.comps.label),
                          component=to_device(f, self.comps.component))
        self.vectors = hoomd.box_vectors(np.asarray(TRICLINIC, np.float32))

    def call(self, flags=0, n=None, components=None, position=True, **lists):
        """(sums, extent, origin, flags, summary) on the host, guard rows included.  ValueError: the summary and every
        output were left alone."""
        n = self.n if n is None else n
        components = self.want.components if components is None else components
        rows = components + GUARD_ROWS
        device = self.f.pipeline_device()
        out = [fl.DeviceBuffer((rows * w,), dt, device, pattern=np.full(rows * w, g, dt))
               for w, dt, g in ((9, np.float64, GUARD_F), (6, np.float64, GUARD_F), (3, np.float64, GUARD_F), (2, np.uint32, GUARD_U))]
        summary = (ctypes.c_uint64 * 6)(*([77] * 6))
        given = dict(self.lists, **lists)
        entries = [ctypes.byref(e) for e in self.entries]
        if not position:
            entries[3] = None
        rc = self.fn(self.h, *entries, (ctypes.c_double * 8)(1, 0, 0, 0, 0, 0, 0, 0), (ctypes.c_double * 6)(*self.vectors), 3,
                     _ptr(given['rows']), _ptr(given['label']), _ptr(given['component']), n, components, flags,
                     *[_ptr(o) for o in out], summary)
        host = [_host(o).reshape(rows, -1) for o in out]
        if rc == _lib.ERROR_INVALID_ARGUMENT:
            assert list(summary) == [77] * 6                        # written on success only
            assert all((a == g).all() for a, g in zip(host, (GUARD_F, GUARD_F, GUARD_F, GUARD_U)))      # nothing touched
            raise ValueError(_lib.last_error())
        assert rc == 0, (rc, _lib.last_error())
        return tuple(host) + (np.array(list(summary), np.uint64),)

    def good(self, what):
        sums, extent, origin, flags, summary = self.call()
        c = self.want.components
        got = hoomd.ComponentMoments.from_tables(summary, sums[:c], extent[:c], origin[:c], flags[:c])
        assert mismatches(got, self.want) == [], what
        for table, guard in ((sums, GUARD_F), (extent, GUARD_F), (origin, GUARD_F), (flags, GUARD_U)):
            assert len(table) == c + GUARD_ROWS and (table[c:] == guard).all(), what
        return True


@pytest.fixture()
def protocol(data):
    path, _ = data
    with hoomd.open(path, 'r') as t:
        frame = t[0]
    with fl.open(path, 'r') as f:
        yield Protocol(f, frame)
        f.wait_read()


def test_no_store_lands_behind_components(protocol):
    assert 1 < protocol.want.components < protocol.n and protocol.comps.largest > 2
    assert protocol.good("the plain call")


def test_each_refusal_leaves_the_outputs_alone_and_the_next_call_is_correct(protocol):
    comps, f, n, C = protocol.comps, protocol.f, protocol.n, protocol.want.components
    member = int(np.flatnonzero(comps.label != np.arange(n))[0])          # an entry that is no root
    later = n - 1
    assert member < later

    def changed(a, at, value):
        a = np.array(a, dtype=np.int64)
        a[at] = value
        return to_device(f, a)

    finer = hoomd.neighbour_components(protocol.position, TRICLINIC, 0.5, rows=np.arange(n), cells=(7, 5, 4))
    assert np.array_equal(finer.rows, comps.rows) and finer.components > C          # the same list, other pieces
    refusals = {
        'a label that is no root': dict(label=changed(comps.label, later, member)),
        'a label above its entry': dict(label=changed(comps.label, 0, 5)),
        'an id >= components': dict(component=changed(comps.component, member, C)),
        'an id other than its root\'s': dict(component=changed(comps.component, member, (int(comps.component[member]) + 1) % C)),
        'the labels of another run': dict(label=to_device(f, finer.label)),
        'a row >= N': dict(rows=changed(comps.rows, 17, N)),
        'the ids numbered downwards': dict(component=to_device(f, C - 1 - comps.component.astype(np.int64))),
    }
    for what, lists in refusals.items():
        with pytest.raises(ValueError, match="not a components result of this list|lies outside the chunks"):
            protocol.call(**lists)
        assert protocol.good("after " + what)
    # fewer components than the ids say, and more: an id >= components, and a component without an entry
    for components in (protocol.want.components - 1, protocol.want.components + 1):
        with pytest.raises(ValueError, match="not a components result of this list"):
            protocol.call(components=components)
    assert protocol.good("after a wrong number of components")


def test_flags_and_the_arguments(protocol):
    for flags in (1, 2, 1 << 31):
        with pytest.raises(ValueError, match="undefined bits"):
            protocol.call(flags=flags)
    with pytest.raises(ValueError, match="stored nowhere"):
        protocol.call(position=False)
    with pytest.raises(ValueError, match="1 to n components"):
        protocol.call(components=protocol.n + 1)
    with pytest.raises(ValueError, match="1 to n components"):
        protocol.call(components=0)
    # no entry: nothing is staged or launched, the outputs are left alone and the summary is six zeros
    protocol.f.wait_read()
    protocol.f.device_read_stats(reset=True)
    sums, extent, origin, flags, summary = protocol.call(n=0, components=0)
    assert summary.tolist() == [0] * 6 and (sums == GUARD_F).all() and (flags == GUARD_U).all() and len(sums) == GUARD_ROWS
    assert protocol.f.device_read_stats()["pread_bytes"] == 0
    # through the binding: ValueError, and the next good call equals the model
    f, lists = protocol.f, protocol.lists
    chunks = [(0, 'particles/' + name) for name in FIELDS]
    with pytest.raises(ValueError, match="fewer entries than n"):
        f.component_moments_device(chunks, TRICLINIC, lists['rows'], lists['label'], lists['component'], 501, protocol.want.components)
    with pytest.raises(ValueError, match="float32 or float64"):
        f.component_moments_device([(0, 'particles/typeid')] + chunks[1:], TRICLINIC, lists['rows'], lists['label'],
                                   lists['component'], 500, protocol.want.components)
    with pytest.raises(ValueError, match="stored nowhere"):
        f.component_moments_device(chunks[:3] + [None], TRICLINIC, lists['rows'], lists['label'], lists['component'], 500,
                                   protocol.want.components)
    with pytest.raises(ValueError, match="mass, velocity, energy, position"):
        f.component_moments_device(chunks[:3], TRICLINIC, lists['rows'], lists['label'], lists['component'], 500,
                                   protocol.want.components)
    got = f.component_moments_device(chunks, TRICLINIC, lists['rows'], lists['label'], lists['component'], 500,
                                     protocol.want.components)
    assert equal(got, protocol.want, "after the refusals")


# ---------------------------------------------------------------- the trajectory level
WHERE = {'type': ['fluid']}


def test_frame_component_moments_device_equals_the_host_model(data):
    path, _ = data
    with hoomd.open(path, 'r') as t:
        for options in (dict(r=0.61, where=WHERE), dict(r=0.9, cells=(5, 5, 3)),
                        dict(r=0.7, where=WHERE, domain=hoomd.domain_grid(2, 2, 1)[1])):
            want = t.frame_component_moments(0, **options)
            got = t.frame_component_moments_device(0, **options)
            assert equal(got, want, options) and 1 < want.components < want.n
            assert np.array_equal(_host(got.sizes), want.sizes) and np.array_equal(_host(got.components_of.label),
                                                                                    want.components_of.label)
            assert np.array_equal(got.components_of.summary, want.components_of.summary)
            host = got.to_host()
            assert np.array_equal(host.heaviest(3), want.heaviest(3)) and host.heaviest(1)[0] == want.heaviest_id
        assert got.n < N
        with pytest.raises(ValueError, match="narrower"):
            t.frame_component_moments_device(0, 1.3, cells=(8, 5, 4))
        with pytest.raises(IndexError):
            t.frame_component_moments_device(1, 1.3)
        # the staged chunks were released on the error paths too: the next call is correct
        assert equal(t.frame_component_moments_device(0, 0.9), t.frame_component_moments(0, 0.9), "after the errors")


CHILD = r'''
import os, sys
sys.modules["torch"] = None                    # `import torch` raises ImportError from here on
root, path = sys.argv[1:3]
sys.path[:0] = [os.path.join(root, "pgsd-sph_amd"), os.path.join(root, "tests")]
import numpy as np
import pgsd.fl as fl
import pgsd.hoomd as hoomd
from pgsd import _lib
from component_moments_cases import mismatches
assert _lib._torch is None
with hoomd.open(path, "r") as t:
    want = t.frame_component_moments(0, 0.9, where={"type": ["fluid"]})
    got = t.frame_component_moments_device(0, 0.9, where={"type": ["fluid"]})
    assert isinstance(got.mass, fl.DeviceBuffer) and isinstance(got.origin, fl.DeviceBuffer)
    assert mismatches(got.to_host(), want) == [] and 1 < got.components < got.n
print("TORCH_FREE_OK")
'''


def test_the_component_fields_need_no_tensor_library(data, tmp_path):
    path, _ = data
    script = str(tmp_path / "child.py")
    with open(script, "w") as fh:
        fh.write(CHILD)
    p = subprocess.run([sys.executable, script, product.ROOT, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "TORCH_FREE_OK" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
