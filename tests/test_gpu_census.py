"""The domain census on the GPU: per-axis histograms of the fractional coordinates (pgsd_domain_histogram_device) and
per-cell counts of a decomposition (pgsd_domain_counts_device), behind pgsd.fl's domain_histogram_device /
domain_counts_device and pgsd.hoomd's axis_histograms_device / domain_counts_device / balanced_grid_device.  Every
result must equal the numpy models pgsd.hoomd.axis_histograms / domain_counts / balanced_grid exactly -- they are
integer counts --, bin edges, cell planes and NaN rows included.  Files are written through the host path."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pgsd.fl as fl  # noqa: E402
import pgsd.hoomd as hoomd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNEQUAL = dict(x_split=[0.25, 0.5], z_split=[0.375])        # the unequal splits of tests/test_gpu_halo.py
GRIDS = {
    "1x1x1": ((1, 1, 1), {}),
    "2x2x2": ((2, 2, 2), {}),
    "3x1x2": ((3, 1, 2), {}),
    "unequal": ((3, 1, 2), UNEQUAL),
    "8x8x8": ((8, 8, 8), {}),
}
BINS = [2, 64, 4096]
# one lane, a partial tile, exactly one tile, one row past it, a ragged many-tile case, and more rows than the capped grid
# (2 x 256 compute units x 4096 rows = 2 097 152) takes in one trip: some workgroup goes through its tile loop twice
SIZES = [1, 1000, 4096, 4097, 70_001, 3_000_001]
ORTHO = np.array([16.0, 16.0, 16.0, 0.0, 0.0, 0.0], np.float32)
TRI = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
# lattice: every particle on the 1/64 lattice of fractions (exact arithmetic; rows on 0 and on every edge of 2 and 64
# bins and of the equal and unequal grids).  tri: random rows in the triclinic box of test_gpu_halo.py.  cluster: every
# row the same point -- one bin, one cell: every lane of every wave adds to one LDS counter.
KINDS = {"lattice": ORTHO, "tri": TRI, "cluster": TRI}


def _positions(rng, kind, N):
    if kind == "tri":
        return rng.uniform(-3.0, 3.0, size=(N, 3)).astype(np.float32)
    if kind == "cluster":
        return np.broadcast_to(np.array([0.75, -1.25, 0.375], np.float32), (N, 3)).copy()
    k = rng.integers(0, 64, size=(N, 3))
    k[:64] = np.arange(64)[:min(N, 64), None]
    p = (k / 64.0 + rng.integers(-1, 2, size=(N, 3)) - 0.5) * 16.0
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32)


def _frame(box, pos, step=0, pos64=True, dimensions=3):
    fr = hoomd.Frame()
    fr.configuration.step = step
    fr.configuration.box = box
    fr.configuration.dimensions = dimensions
    if pos is not None:
        fr.particles.N = len(pos)
        fr.particles.position = pos
    if pos64:
        # the same rows as a float64 chunk: the lattice points as they are, the others moved off every float32
        exact = box is ORTHO
        fr.log['pos64'] = pos.astype(np.float64) * (1.0 if exact else 1.0 + 2.0 ** -40)
    return fr


def _dir(tmp_path_factory, name):
    return "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path_factory.mktemp(name))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """Per kind and N one file of one frame (70 001 rows: a second frame that elides the position): path and the host's
    rows of both chunks."""
    d = _dir(tmp_path_factory, "census")
    out = {}
    for kind, box in KINDS.items():
        for N in SIZES:
            rng = np.random.default_rng(N)
            path = os.path.join(d, "pgsd_census_%d_%s_%d.gsd" % (os.getpid(), kind, N))
            f0 = _frame(box, _positions(rng, kind, N))
            with hoomd.open(path, 'w') as t:
                t.append(f0)
                if N == 70_001:
                    f1 = _frame(box, f0.particles.position, step=5, pos64=False)
                    f1.particles.velocity = rng.standard_normal((N, 3)).astype(np.float32)
                    t.append(f1)
            out[kind, N] = (path, {'position': f0.particles.position, 'pos64': f0.log['pos64']})
    yield out
    for path, _ in out.values():
        os.unlink(path)


def _host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def _inner(n, split):
    return [b[1:-1] for b in hoomd.grid_bounds(*n, **split)]


@pytest.mark.parametrize("chunk", ['position', 'pos64'])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("N", SIZES)
def test_histograms_and_counts_equal_the_models(cases, N, kind, chunk):
    path, rows = cases[kind, N]
    box, pos = KINDS[kind], rows[chunk]
    name = 'particles/position' if chunk == 'position' else 'log/pos64'
    with fl.open(path, 'r') as f:
        for bins in BINS:
            got = f.domain_histogram_device(0, name, box, bins)
            want = hoomd.axis_histograms(pos, box, bins)
            assert got.dtype == np.int64 and got.shape == (3, bins)
            assert np.array_equal(got, want), (bins, np.flatnonzero((got != want).any(axis=0))[:8])
            assert got.sum() == 3 * N
        for grid, (n, split) in sorted(GRIDS.items()):
            counts, nowhere = f.domain_counts_device(0, name, box, n, _inner(n, split))
            want, want_nowhere = hoomd.domain_counts(pos, box, *n, **split)
            assert counts.dtype == np.int64 and counts.shape == want.shape
            assert np.array_equal(counts, want), (grid, np.flatnonzero(counts != want)[:8])
            assert nowhere == want_nowhere == 0 and counts.sum() == N
        f.wait_read()
    if kind == "cluster":
        assert np.count_nonzero(want) == 1 and np.count_nonzero(hoomd.axis_histograms(pos, box, 4096)) == 3


def test_the_lattice_puts_rows_on_every_edge(cases):
    """What the exactness cases rely on: rows exactly on 0 and on every edge of the 64-bin histogram and of the grids."""
    _, rows = cases["lattice", 70_001]
    f = hoomd._wrapped_fractions(rows['position'], ORTHO, 3)
    for a in range(3):
        assert set((f[a] * 64).tolist()) == set(float(k) for k in range(64))


@pytest.fixture(scope="module")
def special(tmp_path_factory):
    """Small files for the further cases: NaN / infinite rows, a 2-D frame, a frame without positions, a dam break."""
    d = _dir(tmp_path_factory, "census_special")
    rng = np.random.default_rng(77)
    out = {}

    def write(key, frames):
        path = os.path.join(d, "pgsd_census_%d_%s.gsd" % (os.getpid(), key))
        with hoomd.open(path, 'w') as t:
            for fr in frames:
                t.append(fr)
        out[key] = path

    pos = _positions(rng, "tri", 9000)
    pos[::7] = np.nan
    pos[1::11, 2] = np.inf              # z enters every fraction of the triclinic box
    pos[2::13, 0] = -np.inf             # x enters only its own
    pos[3::17, 1] = np.nan              # y enters x and y
    write("nan", [_frame(TRI, pos)])
    out["nan_pos"] = pos

    box2 = np.array([4.0, 4.0, 1.0, 0.5, 0.0, 0.0], np.float32)
    pos2 = _positions(rng, "tri", 9000)
    pos2[:, 2] = 0.0
    write("flat", [_frame(box2, pos2, pos64=False, dimensions=2)])
    out["flat_pos"], out["flat_box"] = pos2, box2

    nowhere = _frame(TRI, None, pos64=False)
    nowhere.particles.N = 5000
    nowhere.particles.mass = rng.uniform(0.5, 2.0, size=5000).astype(np.float32)
    write("default", [nowhere])

    # every particle in one eighth of the box
    dam = ((rng.random((50_000, 3)) * 0.5 - 0.5) * np.array([4.0, 4.0, 2.0]) * 0.999).astype(np.float32)
    dam_box = np.array([4.0, 4.0, 2.0, 0.0, 0.0, 0.0], np.float32)
    f0 = _frame(dam_box, dam, pos64=False)
    f0.particles.velocity = rng.standard_normal((50_000, 3)).astype(np.float32)
    write("dam", [f0])
    out["dam_pos"], out["dam_box"] = dam, dam_box
    yield out
    for key, path in out.items():
        if isinstance(path, str):
            os.unlink(path)


def test_nan_and_infinite_rows_are_counted_nowhere(special):
    pos = special["nan_pos"]
    with hoomd.open(special["nan"], 'r') as t:
        for bins in BINS:
            want = hoomd.axis_histograms(pos, TRI, bins)
            assert np.array_equal(t.axis_histograms_device(0, bins), want)
        assert len(set(want.sum(axis=1).tolist())) == 3 and want.sum(axis=1).max() < len(pos)
        for grid, (n, split) in sorted(GRIDS.items()):
            counts, nowhere = t.domain_counts_device(0, *n, **split)
            want_counts, want_nowhere = hoomd.domain_counts(pos, TRI, *n, **split)
            assert np.array_equal(counts, want_counts) and nowhere == want_nowhere > 1000, grid
            assert counts.sum() + nowhere == len(pos)
        for name in ('pos64',):
            p64 = t[0].log[name]
            got = t.file.domain_histogram_device(0, 'log/' + name, TRI, 64)
            assert np.array_equal(got, hoomd.axis_histograms(p64, TRI, 64))
            counts, nowhere = t.file.domain_counts_device(0, 'log/' + name, TRI, (8, 8, 8), _inner((8, 8, 8), {}))
            want_counts, want_nowhere = hoomd.domain_counts(p64, TRI, 8, 8, 8)
            assert np.array_equal(counts, want_counts) and nowhere == want_nowhere
            t.file.wait_read()


def test_a_two_dimensional_frame(special):
    pos, box = special["flat_pos"], special["flat_box"]
    with hoomd.open(special["flat"], 'r') as t:
        assert int(t[0].configuration.dimensions) == 2
        got = t.axis_histograms_device(0, 64)
        assert np.array_equal(got, hoomd.axis_histograms(pos, box, 64, dimensions=2))
        assert not got[2].any() and got[:2].sum() == 2 * len(pos)
        counts, nowhere = t.domain_counts_device(0, 3, 2, 1, x_split=[0.25, 0.5])
        want, _ = hoomd.domain_counts(pos, box, 3, 2, 1, x_split=[0.25, 0.5], dimensions=2)
        assert np.array_equal(counts, want) and nowhere == 0 and counts.sum() == len(pos)
        with pytest.raises(ValueError, match="nz"):
            t.domain_counts_device(0, 2, 2, 2)
        with pytest.raises(ValueError, match="nz"):
            t.balanced_grid_device(0, 2, 2, 2)
        with pytest.raises(ValueError, match="one z cell"):       # the library's own refusal
            t.file.domain_counts_device(0, 'particles/position', box, (2, 2, 2), [[0.5]] * 3, dimensions=2)
        domains, splits, counts, nowhere = t.balanced_grid_device(0, 4, 2, 1, bins=256)
        want_domains, want_splits = hoomd.balanced_grid(pos, box, 4, 2, 1, bins=256, dimensions=2)
        assert domains == want_domains and splits == want_splits and splits[2] is None
        assert np.array_equal(counts, hoomd.domain_counts(pos, box, 4, 2, 1, *splits, dimensions=2)[0])


def test_an_elided_position_is_answered_from_frame_0(cases):
    path, rows = cases["tri", 70_001]
    pos = rows['position']
    with hoomd.open(path, 'r') as t:
        assert not t.file.chunk_exists(1, 'particles/position') and t.file.chunk_exists(1, 'particles/velocity')
        assert np.array_equal(t.axis_histograms_device(1, 64), hoomd.axis_histograms(pos, TRI, 64))
        counts, nowhere = t.domain_counts_device(1, 3, 1, 2, **UNEQUAL)
        assert np.array_equal(counts, hoomd.domain_counts(pos, TRI, 3, 1, 2, **UNEQUAL)[0]) and nowhere == 0
        assert np.array_equal(t.axis_histograms_device(-1), hoomd.axis_histograms(pos, TRI, 1024))
        with pytest.raises(IndexError):
            t.axis_histograms_device(2)


def test_a_position_stored_nowhere_is_answered_from_the_default_row(special):
    with hoomd.open(special["default"], 'r') as t:
        assert not t.file.chunk_exists(0, 'particles/position')
        zeros = np.zeros((5000, 3), np.float32)
        t.file.device_read_stats(reset=True)
        hist = t.axis_histograms_device(0, 64)
        assert np.array_equal(hist, hoomd.axis_histograms(zeros, TRI, 64)) and hist[:, 32].tolist() == [5000] * 3
        counts, nowhere = t.domain_counts_device(0, 2, 2, 2)
        assert counts.tolist() == hoomd.domain_counts(zeros, TRI, 2, 2, 2)[0].tolist() == [0] * 7 + [5000]
        domains, splits, counts, nowhere = t.balanced_grid_device(0, 2, 2, 2, bins=64)
        want_domains, want_splits = hoomd.balanced_grid(zeros, TRI, 2, 2, 2, bins=64)
        assert domains == want_domains and splits == want_splits
        assert np.array_equal(counts, hoomd.domain_counts(zeros, TRI, 2, 2, 2, *splits)[0]) and nowhere == 0
        assert t.file.device_read_stats()["pread_bytes"] == 0


def test_the_balanced_grid_of_a_dam_break(special):
    pos, box = special["dam_pos"], special["dam_box"]
    N = len(pos)
    with hoomd.open(special["dam"], 'r') as t:
        equal, _ = t.domain_counts_device(0, 2, 2, 2)
        assert equal.tolist() == [N] + [0] * 7
        domains, splits, counts, nowhere = t.balanced_grid_device(0, 2, 2, 2)
        want_domains, want_splits = hoomd.balanced_grid(t[0].particles.position, box, 2, 2, 2)
        assert domains == want_domains and splits == want_splits
        assert np.array_equal(counts, hoomd.domain_counts(pos, box, 2, 2, 2, *splits)[0]) and nowhere == 0
        assert counts.sum() == N and counts.max() < 1.2 * N / 8
        for r, d in enumerate(domains):
            s = t.read_frame_device(0, domain=d)
            assert s.particles.N == counts[r] == len(_host(s.tag))
        # a ghost layer's width as min_bins: no cell narrower than it
        domains, splits, counts, nowhere = t.balanced_grid_device(0, 4, 1, 1, bins=64, min_bins=10)
        assert splits == hoomd.balanced_grid(pos, box, 4, 1, 1, bins=64, min_bins=10)[1]
        assert min(splits[0]) == 10 / 64 and counts.sum() == N


def test_a_histogram_and_a_count_read_the_position_chunk_once(cases):
    path, rows = cases["tri", 70_001]
    N = 70_001
    with hoomd.open(path, 'r') as t:
        f = t.file
        f.device_read_stats(reset=True)
        f.domain_histogram_device(0, 'particles/position', TRI, 1024)
        assert f.device_read_stats()["pread_bytes"] == N * 12
        f.domain_counts_device(0, 'particles/position', TRI, (2, 2, 2), [[0.5]] * 3)
        f.domain_histogram_device(0, 'particles/position', TRI, 64)
        assert f.device_read_stats()["pread_bytes"] == N * 12
        # ... and a selection of the same chunk is served from the same rows
        sel, count = f.select_domain_device(0, 'particles/position', TRI, hoomd.domain_grid(2, 2, 2)[3])
        assert f.device_read_stats()["pread_bytes"] == N * 12
        f.wait_read()
        # after the wait the chunk is released: the next census reads it again
        f.domain_counts_device(0, 'particles/position', TRI, (2, 2, 2), [[0.5]] * 3)
        assert f.device_read_stats()["pread_bytes"] == 2 * N * 12
        f.wait_read()
        # the trajectory's methods release what they staged: one chunk per call, one for the balanced grid's two passes
        f.device_read_stats(reset=True)
        t.axis_histograms_device(0)
        t.domain_counts_device(0, 2, 2, 2)
        assert f.device_read_stats()["pread_bytes"] == 2 * N * 12
        t.balanced_grid_device(0, 2, 2, 2)
        assert f.device_read_stats()["pread_bytes"] == 3 * N * 12


def test_domain_reads_are_unchanged_after_a_census(cases):
    path, rows = cases["tri", 70_001]
    d = hoomd.domain_grid(2, 2, 2)[3]
    want = hoomd.domain_rows(rows['position'], TRI, d)
    with hoomd.open(path, 'r') as t:
        before = t.read_frame_device(1, domain=d, scalar4=True)
        t.balanced_grid_device(1, 3, 1, 2)
        t.axis_histograms_device(0, 4096)
        after = t.read_frame_device(1, domain=d, scalar4=True)
        host = t[1]
    for s in (before, after):
        assert np.array_equal(_host(s.tag), want) and s.particles.N == len(want)
        assert _host(s.particles.position).tobytes() == host.particles.position[want].tobytes()
        assert _host(s.particles.velocity).tobytes() == host.particles.velocity[want].tobytes()
    assert _host(before.particles.pos4).tobytes() == _host(after.particles.pos4).tobytes()


def test_every_refusal_has_its_message_and_leaves_the_handle_usable(cases):
    path, rows = cases["tri", 1000]
    name = 'particles/position'
    with fl.open(path, 'r') as f:
        for bins in (0, 1, 3, 100, 8192):
            with pytest.raises(ValueError, match="bins must be a power of two"):
                f.domain_histogram_device(0, name, TRI, bins)
        for n in ((0, 1, 1), (1, 65, 1)):
            with pytest.raises(ValueError, match="1 to 64 cells"):
                f.domain_counts_device(0, name, TRI, n, [np.linspace(0, 1, max(v, 1) + 1)[1:-1] for v in n])
        with pytest.raises(ValueError, match="at most 4096 cells"):
            f.domain_counts_device(0, name, TRI, (64, 64, 2), [np.linspace(0, 1, v + 1)[1:-1] for v in (64, 64, 2)])
        for bad in ([0.5, 0.5], [0.5, 0.25], [0.0, 0.5], [0.5, 1.0], [0.5, float('nan')], [-0.25, 0.5]):
            with pytest.raises(ValueError, match="ascend strictly inside"):
                f.domain_counts_device(0, name, TRI, (3, 1, 1), [bad, [], []])
        with pytest.raises(ValueError, match="ascend strictly inside"):
            f.domain_counts_device(0, name, TRI, (1, 1, 2), [[], [], [1.5]])
        with pytest.raises(ValueError, match="one z cell"):
            f.domain_counts_device(0, name, TRI, (2, 1, 2), [[0.5], [], [0.5]], dimensions=2)
        with pytest.raises(ValueError):
            f.domain_counts_device(0, name, TRI, (2, 1, 1), [[0.5, 0.75], [], []])       # one bound too many
        with pytest.raises(ValueError, match="N x 3"):
            f.domain_histogram_device(0, 'configuration/box', TRI, 64)
        with pytest.raises(ValueError, match="box lengths"):
            f.domain_histogram_device(0, name, [0, 1, 1, 0, 0, 0], 64)
        with pytest.raises(ValueError):
            f.domain_counts_device(0, name, TRI, (1, 1, 1), [[], [], []], dimensions=4)
        # the handle works as before
        pos = rows['position']
        assert np.array_equal(f.domain_histogram_device(0, name, TRI, 64), hoomd.axis_histograms(pos, TRI, 64))
        counts, nowhere = f.domain_counts_device(0, name, TRI, (1, 1, 1), [[], [], []])
        assert counts.tolist() == [1000] and nowhere == 0
        f.wait_read()


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
res = {}
with hoomd.open(path, 'r') as t:
    res["hist"] = t.axis_histograms_device(1, 4096)
    res["counts"] = t.domain_counts_device(1, 3, 1, 2, x_split=[0.25, 0.5], z_split=[0.375])
    res["grid"] = t.balanced_grid_device(0, 2, 2, 2, bins=256)
    res["hist64"] = t.file.domain_histogram_device(0, 'log/pos64', t[0].configuration.box, 64)
    t.file.wait_read()
pickle.dump(res, open(out_path, "wb"))
'''


def test_census_without_torch(cases, tmp_path):
    path, rows = cases["tri", 70_001]
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, path, str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))
    pos = rows['position']
    assert np.array_equal(res["hist"], hoomd.axis_histograms(pos, TRI, 4096))
    want, want_nowhere = hoomd.domain_counts(pos, TRI, 3, 1, 2, **UNEQUAL)
    assert np.array_equal(res["counts"][0], want) and res["counts"][1] == want_nowhere
    domains, splits = hoomd.balanced_grid(pos, TRI, 2, 2, 2, bins=256)
    assert res["grid"][0] == domains and res["grid"][1] == splits
    assert np.array_equal(res["grid"][2], hoomd.domain_counts(pos, TRI, 2, 2, 2, *splits)[0]) and res["grid"][3] == 0
    assert np.array_equal(res["hist64"], hoomd.axis_histograms(rows['pos64'], TRI, 64))
