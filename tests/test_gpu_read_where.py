"""Group reads: read_frame_device(where=...) selects the particles that satisfy a predicate over per-particle chunks --
a set of types, ranges of values, optionally inside a domain -- on the GPU (pgsd_select_where_device) and gathers every
per-particle array through that row list.  The selection must equal pgsd.hoomd.where_rows -- the numpy model --
exactly (intersected with pgsd.hoomd.domain_rows where a domain is given), and every array the host reader's frame
indexed by those rows, byte for byte.  Files are written through the host path, once per module."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)      # triclinic; every value a short binary fraction
GRID = hoomd.domain_grid(2, 2, 2)
PLANES = (0.0, 0.25, 0.5, 0.75)
TYPES = ['fluid', 'wall', 'inlet', 'outlet']
# a wave, the 256-row lane stride, a 4096-row workgroup, the 256-block step of the one-block scan (2^20 rows)
SIZES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 1_048_575, 1_048_577, 3_000_001]
LO, HI = -0.5, 0.75                                                  # the density range; both exact in float32
EDGE_VALUES = np.array([np.nan, 0.0, -0.0, LO, HI, np.nextafter(np.float32(LO), np.float32(-1)),
                        np.nextafter(np.float32(HI), np.float32(0)), np.inf, -np.inf], np.float32)

# name -> (where of read_frame_device / where_rows, the same as terms of select_where_device in frame 0)
TERMS = {
    'typeid_set': ({'typeid': [0, 2]}, [(0, 'particles/typeid', 0, [0, 2])]),
    'density_range': ({'density': (LO, HI)}, [(0, 'particles/density', 0, (LO, HI))]),
    'velocity_z': ({('velocity', 2): (0.0, None)}, [(0, 'particles/velocity', 2, (0.0, None))]),
    'body_range': ({'body': (-2, 3)}, [(0, 'particles/body', 0, (-2, 3))]),
}
TERMS['all_four'] = (dict(kv for w, _ in list(TERMS.values()) for kv in w.items()),
                     [t for _, ts in list(TERMS.values()) for t in ts])
# further ranges whose bounds are the zeros, and open ends: no domain
EDGE_TERMS = {
    'density_from_zero': ({'density': (0.0, HI)}, [(0, 'particles/density', 0, (0.0, HI))]),
    'density_from_negzero': ({'density': (-0.0, None)}, [(0, 'particles/density', 0, (-0.0, None))]),
    'density_below_zero': ({'density': (None, 0.0)}, [(0, 'particles/density', 0, (None, 0.0))]),
    'density_open': ({'density': (None, None)}, [(0, 'particles/density', 0, (None, None))]),
    'density_to_inf': ({'density': (LO, np.inf)}, [(0, 'particles/density', 0, (LO, np.inf))]),
    'density_reversed': ({'density': (HI, LO)}, [(0, 'particles/density', 0, (HI, LO))]),
    'everything': ({'typeid': [0, 1, 2, 3]}, [(0, 'particles/typeid', 0, [0, 1, 2, 3])]),
    'nothing': ({'typeid': [7, 63]}, [(0, 'particles/typeid', 0, [7, 63])]),
    'row_0': ({'body': [60]}, [(0, 'particles/body', 0, [60])]),
    'row_last': ({'body': [61]}, [(0, 'particles/body', 0, [61])]),
    'image_y_set': ({('image', 1): [0, 1, 2, 3]}, [(0, 'particles/image', 1, [0, 1, 2, 3])]),
}


def _on_planes(rng, n):
    """Positions whose fractional coordinates are exactly split-plane values (see test_gpu_read_domain.py)."""
    Lx, Ly, Lz, xy, xz, yz = (float(v) for v in BOX)
    s = rng.choice(PLANES, size=(n, 3)) + rng.integers(-1, 2, size=(n, 3))
    z = (s[:, 2] - 0.5) * Lz
    y = (s[:, 1] - 0.5) * Ly + yz * z
    x = (s[:, 0] - 0.5) * Lx + xz * z + xy * y
    return np.stack([x, y, z], axis=1).astype(np.float32)


def _blips(rng, flat):
    """NaN, the zeros, the infinities and values on and next to the range's bounds at seeded places; the first and the
    last element among them."""
    at = np.unique(np.concatenate([[0, flat.size - 1], rng.integers(0, flat.size, size=min(flat.size, 512))]))
    flat[at] = rng.choice(EDGE_VALUES, size=at.size)
    flat[0] = np.nan                                # (and no array of one row equals its default, which would elide it)


def _frame(rng, N, step=0):
    fr = hoomd.Frame()
    fr.configuration.step = step
    fr.configuration.box = BOX
    fr.particles.N = N
    fr.particles.types = TYPES
    i = np.arange(N)
    pos = rng.uniform(-3.0, 3.0, size=(N, 3)).astype(np.float32)
    k = min(N, 4096)
    pos[:k] = _on_planes(rng, k)
    fr.particles.position = pos
    fr.particles.typeid = ((i * 7 + i // 5 + 1) % 4).astype(np.uint32)
    fr.particles.body = ((i * 3 + i // 11) % 9 - 3).astype(np.int32)     # -3 .. 5
    fr.particles.body[0] = 60
    fr.particles.body[N - 1] = 61
    fr.particles.velocity = rng.standard_normal((N, 3)).astype(np.float32)
    _blips(rng, fr.particles.velocity.reshape(-1))
    fr.particles.density = rng.standard_normal(N).astype(np.float32)
    _blips(rng, fr.particles.density)
    fr.particles.mass = (1.0 + (i % 1024) / 1024.0).astype(np.float32)
    fr.particles.image = rng.integers(-3, 4, size=(N, 3)).astype(np.int32)
    fr.log['pos64'] = pos.astype(np.float64) * (1.0 + 2.0 ** -40)        # a float64 N x 3 chunk no float32 holds
    return fr


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Per N one frame; for N = 4097 also frame 1, which elides typeid and body (equal to frame 0's; its density, which
    holds NaNs, equals nothing), and frame 2 of 1000 particles without typeid, body and density.  No frame holds a
    pressure."""
    d = "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp("where"))
    out = {}
    for N in SIZES:
        rng = np.random.default_rng(N)
        path = os.path.join(d, "pgsd_where_%d_%d.gsd" % (os.getpid(), N))
        f0 = _frame(rng, N)
        with hoomd.open(path, 'w') as t:
            t.append(f0)
            if N == 4097:
                f1 = _frame(rng, N, step=1)
                t.append(f1)
                f2 = _frame(rng, 1000, step=2)
                f2.particles.typeid = f2.particles.body = f2.particles.density = None
                t.append(f2)
        out[N] = path
        with fl.open(path, 'r') as f:
            assert all(f.chunk_exists(0, 'particles/' + c) for c in ('typeid', 'body', 'density', 'velocity', 'image'))
    with fl.open(out[4097], 'r') as f:
        assert not f.chunk_exists(1, 'particles/typeid') and not f.chunk_exists(1, 'particles/body')
        assert f.chunk_exists(1, 'particles/velocity') and f.chunk_exists(1, 'particles/density')
        assert not f.chunk_exists(2, 'particles/body') and not f.chunk_exists(2, 'particles/density')
    yield out
    for p in out.values():
        os.unlink(p)


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _same(dev, host):
    a, b = np.ascontiguousarray(_host(dev)), np.ascontiguousarray(host)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _arrays(host):
    return dict((name, getattr(host.particles, name)) for name in hoomd._PARTICLE_FIELDS
                if getattr(host.particles, name) is not None)


def _selected(f, terms, want, domain=None, what=None):
    rows, count = f.select_where_device(terms, domain=None if domain is None else (0, 'particles/position', domain),
                                        box=BOX)
    got = _host(rows)
    assert got.dtype == np.int32 and count == len(want) and np.array_equal(got, want), what


@pytest.mark.parametrize("N", SIZES)
def test_selections_match_the_model(files, N):
    cells = GRID if N <= 4097 else [GRID[0], GRID[5]]
    with hoomd.open(files[N], 'r') as t:
        host = t[0]
        arrays = _arrays(host)
        f = t.file
        inside = [hoomd.domain_rows(host.particles.position, BOX, d) for d in cells]
        pos64 = host.log['pos64']
        cases = [(name, hoomd.where_rows(arrays, where, TYPES), terms) for name, (where, terms) in TERMS.items()]
        cases.append(('float64_column', hoomd.where_rows({'position': pos64}, {('position', 1): (-1.0, 1.5)}),
                      [(0, 'log/pos64', 1, (-1.0, 1.5))]))
        for name, want, terms in cases:
            assert want.dtype == np.int32 and (np.diff(want) > 0).all()
            _selected(f, terms, want, what=name)
            for d, rows_d in zip(cells, inside):
                _selected(f, terms, np.intersect1d(want, rows_d), domain=d, what=(name, d))
        for name, (where, terms) in EDGE_TERMS.items():
            _selected(f, terms, hoomd.where_rows(arrays, where, TYPES), what=name)
        # the domain alone is the domain selection
        _selected(f, [], inside[0], domain=cells[0], what='domain alone')
        assert len(hoomd.where_rows(arrays, EDGE_TERMS['everything'][0])) == N
        assert len(hoomd.where_rows(arrays, EDGE_TERMS['nothing'][0])) == 0
        assert hoomd.where_rows(arrays, EDGE_TERMS['row_last'][0]).tolist() == [N - 1]
        if N > 1:
            assert hoomd.where_rows(arrays, EDGE_TERMS['row_0'][0]).tolist() == [0]


def _check_group(t, host, idx, where, domain, n_global):
    s = t.read_frame_device(idx, where=where, domain=domain, scalar4=True)
    rows = hoomd.where_rows(_arrays(host), where, host.particles.types)
    if domain is not None:
        rows = np.intersect1d(rows, hoomd.domain_rows(host.particles.position, host.configuration.box, domain))
    tag = _host(s.tag)
    assert tag.dtype == np.int32 and np.array_equal(tag, rows)
    assert s.particles.N == len(rows) and s.particles.N_global == n_global and s.where == where
    for name in ('position', 'typeid', 'velocity', 'mass', 'image', 'density', 'body', 'slength', 'pressure',
                 'auxiliary1'):
        assert _same(getattr(s.particles, name), getattr(host.particles, name)[rows]), name
    pos4 = np.concatenate([host.particles.position[rows], host.particles.typeid[rows].view(np.float32)[:, None]], 1)
    vel4 = np.concatenate([host.particles.velocity[rows], host.particles.mass[rows][:, None]], 1)
    assert _same(s.particles.pos4, pos4) and _same(s.particles.vel4, vel4)
    return rows


@pytest.mark.parametrize("N", [1, 257, 4097, 1_048_577])
def test_gathered_arrays_equal_the_host_frame_rows(files, N):
    with hoomd.open(files[N], 'r') as t:
        host = t[0]
        _check_group(t, host, 0, TERMS['all_four'][0], None, N)
        _check_group(t, host, 0, {'type': ['fluid', 'inlet']}, None, N)
        got = [_check_group(t, host, 0, {'type': ['fluid', 'inlet'], ('velocity', 2): (0.0, None)}, d, N)
               for d in (GRID if N <= 4097 else GRID[:2])]
        if N <= 4097:
            want = hoomd.where_rows(_arrays(host), {'typeid': [0, 2], ('velocity', 2): (0.0, None)})
            assert np.array_equal(np.sort(np.concatenate(got)), want)


def test_empty_groups_give_zero_row_arrays(files):
    with hoomd.open(files[257], 'r') as t:
        for where in ({'typeid': [7]}, {'density': (HI, LO)}, {'density': (np.nan, None)}):
            s = t.read_frame_device(0, where=where, scalar4=True)
            assert s.particles.N == 0 and s.particles.N_global == 257 and s.tag.numel() == 0
            assert tuple(s.particles.position.shape) == (0, 3) and tuple(s.particles.pos4.shape) == (0, 4)
            assert tuple(s.particles.mass.shape) == (0,)
        s = t.read_frame_device(0, where={})
        assert s.particles.N == 257 and np.array_equal(_host(s.tag), np.arange(257))
        assert _same(s.particles.velocity, t[0].particles.velocity)


def test_effective_frame_rule(files):
    N = 4097
    with hoomd.open(files[N], 'r') as t:
        # frame 1: typeid and body are elided, their terms read frame 0's chunks; velocity and density are frame 1's own
        host = t[1]
        rows = _check_group(t, host, 1, TERMS['all_four'][0], GRID[3], N)
        assert np.array_equal(host.particles.typeid, t[0].particles.typeid)
        assert not np.array_equal(host.particles.velocity, t[0].particles.velocity)
        assert not np.array_equal(host.particles.density, t[0].particles.density, equal_nan=True)
        _check_group(t, host, 1, {'type': ['wall'], 'body': (None, 0)}, None, N)
        # no frame holds a pressure: the default row (0.0) decides, all or nothing
        assert len(_check_group(t, host, 1, {'pressure': (0.0, 1.0)}, None, N)) == N
        assert len(_check_group(t, host, 1, {'pressure': (1.0, None)}, None, N)) == 0
        assert 0 < len(rows) < N
        both = {'pressure': (0.0, 1.0), ('velocity', 0): (0.0, None)}
        assert 0 < len(_check_group(t, host, 1, both, GRID[1], N)) < N
        # frame 2 has another N: frame 0's typeid, body and density do not apply, their defaults (0, -1, 0.0) decide
        host2 = t[2]
        assert host2.particles.N == 1000
        assert len(_check_group(t, host2, 2, {'type': ['fluid']}, None, 1000)) == 1000
        assert len(_check_group(t, host2, 2, {'typeid': [1, 2]}, None, 1000)) == 0
        assert len(_check_group(t, host2, 2, {'body': list(range(64))}, None, 1000)) == 0      # -1 matches no set
        assert len(_check_group(t, host2, 2, {'body': (-1, 0)}, GRID[0], 1000)) > 0
        assert 0 < len(_check_group(t, host2, 2, {'density': (0.0, 1.0), ('velocity', 1): (None, 0.0)}, None, 1000))


def test_errors(files):
    with hoomd.open(files[4097], 'r') as t:
        with pytest.raises(ValueError):
            t.read_frame_device(0, part=(0, 10), where={'typeid': [0]})
        with pytest.raises(ValueError):
            t.read_frame_device(0, where={'density': [0]})
        with pytest.raises(ValueError):
            t.read_frame_device(0, where={'type': ['steam']})
        with pytest.raises(ValueError):
            t.read_frame_device(0, where={('velocity', 3): (0, 1)})
        with pytest.raises(ValueError):
            t.read_frame_device(0, where={'charge': (0, 1)})                # an upstream attribute the file never stored
        f = t.file
        # refusals of the library itself surface as ValueError with its message
        with pytest.raises(ValueError, match="a set needs a chunk of integers"):
            f.select_where_device([(0, 'particles/density', 0, [1])])
        with pytest.raises(ValueError, match="column 3 of a chunk of 3"):
            f.select_where_device([(0, 'particles/velocity', 3, (0.0, 1.0))])
        with pytest.raises(ValueError, match="differ in N"):
            f.select_where_device([(0, 'particles/typeid', 0, [1]), (2, 'particles/mass', 0, (0.0, None))])
        with pytest.raises(ValueError, match="differ in N"):
            f.select_where_device([(0, 'particles/typeid', 0, [1])], domain=(2, 'particles/position', GRID[0]), box=BOX)
        with pytest.raises(ValueError, match="uint32, int32, float32 or float64"):
            f.select_where_device([(1, 'configuration/step', 0, (0.0, None))])      # uint64
        with pytest.raises(ValueError, match="neither a term nor a domain"):
            f.select_where_device([])
        with pytest.raises(ValueError, match="at most 4 terms"):
            f.select_where_device([(0, 'particles/typeid', 0, [1])] * 5)
        with pytest.raises(ValueError, match="0 <= lo < hi <= 1"):
            f.select_where_device([(0, 'particles/typeid', 0, [1])],
                                  domain=(0, 'particles/position', ((0, 0, 0), (1, 1, 1.5))), box=BOX)
        # and the pipeline is as good as before
        _check_group(t, t[0], 0, TERMS['typeid_set'][0], None, 4097)


def test_selection_keeps_its_staged_chunks_for_the_gathers(files):
    """Indexed reads of the terms' chunks and of the domain's position chunk right after the selection are served from
    the rows the selection staged: no file byte is read again."""
    N = 3_000_001
    with hoomd.open(files[N], 'r') as t:
        host = t[0]
        f = t.file
        terms = TERMS['typeid_set'][1] + TERMS['density_range'][1]
        f.device_read_stats(reset=True)
        rows, n = f.select_where_device(terms, domain=(0, 'particles/position', GRID[6]), box=BOX)
        staged = f.device_read_stats()["pread_bytes"]
        assert staged == N * (4 + 4 + 12)
        pos = f.read_chunk_device(0, 'particles/position', rows=rows, wait=False)
        tid = f.read_chunk_device(0, 'particles/typeid', rows=rows, wait=False)
        rho = f.read_chunk_device(0, 'particles/density', rows=rows, wait=False)
        f.wait_read()
        assert f.device_read_stats()["pread_bytes"] == staged
        r = _host(rows)
        want = np.intersect1d(hoomd.where_rows(_arrays(host), {'typeid': [0, 2], 'density': (LO, HI)}),
                              hoomd.domain_rows(host.particles.position, BOX, GRID[6]))
        assert n == len(want) and np.array_equal(r, want)
        assert _same(pos, host.particles.position[r]) and _same(tid, host.particles.typeid[r])
        assert _same(rho, host.particles.density[r])
        # two terms on one chunk stage it once
        f.device_read_stats(reset=True)
        f.select_where_device([(0, 'particles/velocity', 0, (0.0, None)), (0, 'particles/velocity', 2, (None, 0.0))])
        assert f.device_read_stats()["pread_bytes"] == N * 12
        f.wait_read()


def test_slab_and_domain_reads_are_unchanged_after_group_reads(files):
    N = 4097
    with hoomd.open(files[N], 'r') as t:
        host = t[1]
        t.read_frame_device(1, where=TERMS['all_four'][0], domain=GRID[2])
        s = t.read_frame_device(1, part=(1000, 2000), scalar4=True)
        assert s.particles.N == 2000 and not hasattr(s, 'tag') and not hasattr(s, 'where')
        assert _same(s.particles.position, host.particles.position[1000:3000])
        assert _same(s.particles.typeid, host.particles.typeid[1000:3000])
        t.read_frame_device(1, where={'type': ['wall']})
        d = t.read_frame_device(1, domain=GRID[5], scalar4=True)
        rows = hoomd.domain_rows(host.particles.position, BOX, GRID[5])
        assert np.array_equal(_host(d.tag), rows) and not hasattr(d, 'where')
        assert _same(d.particles.velocity, host.particles.velocity[rows])
        assert _same(d.particles.pos4[:, :3].contiguous(), host.particles.position[rows])
        again = t.read_frame_device(1, part=(1000, 2000))
        assert _same(again.particles.density, host.particles.density[1000:3000])


CHILD = r'''
import os, pickle, sys
sys.modules["torch"] = None                    # `import torch` raises ImportError from here on
root, path, out_path = sys.argv[1:4]
sys.path[:0] = [os.path.join(root, "pgsd-sph_amd"), os.path.join(root, "tests")]
import numpy as np
import pgsd.fl as fl
import pgsd.hoomd as hoomd
from pgsd import _lib
assert _lib._torch is None
grid = hoomd.domain_grid(2, 2, 2)
where = {'type': ['fluid', 'inlet'], 'density': (-0.5, 0.75), ('velocity', 2): (0.0, None)}
res = []
with hoomd.open(path, 'r') as t:
    for idx in (0, 1):
        for d in (None, grid[0], grid[7]):
            s = t.read_frame_device(idx, where=where, domain=d, scalar4=True)
            assert isinstance(s.tag, fl.DeviceBuffer)
            res.append((idx, None if d is None else (d.lo, d.hi), s.tag.to_host(), s.particles.position.to_host(),
                        s.particles.pos4.to_host(), s.particles.density.to_host(), s.particles.image.to_host()))
    rows, n = t.file.select_where_device([(0, 'particles/body', 0, (-2, 3))])
    assert isinstance(rows, fl.DeviceBuffer)
    res.append(('body', n, rows.to_host()))
pickle.dump(res, open(out_path, "wb"))
'''


def test_group_read_without_torch(files, tmp_path):
    N = 4097
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, files[N], str(out)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))
    where = {'typeid': [0, 2], 'density': (LO, HI), ('velocity', 2): (0.0, None)}
    with hoomd.open(files[N], 'r') as t:
        hosts = {0: t[0], 1: t[1]}
    _, n, body_rows = res.pop()
    want = hoomd.where_rows(_arrays(hosts[0]), {'body': (-2, 3)})
    assert n == len(want) and body_rows.dtype == np.int32 and np.array_equal(body_rows, want)
    assert len(res) == 6
    for idx, cell, tag, pos, pos4, density, image in res:
        h = hosts[idx]
        rows = hoomd.where_rows(_arrays(h), where)
        if cell is not None:
            rows = np.intersect1d(rows, hoomd.domain_rows(h.particles.position, BOX, hoomd.Domain(*cell)))
        assert tag.dtype == np.int32 and np.array_equal(tag, rows) and len(rows) > 0
        assert pos.tobytes() == h.particles.position[rows].tobytes()
        assert density.tobytes() == h.particles.density[rows].tobytes()
        assert image.tobytes() == h.particles.image[rows].tobytes()
        assert pos4[:, 3].view(np.uint32).tobytes() == h.particles.typeid[rows].tobytes()
