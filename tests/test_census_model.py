"""The domain census on the host: pgsd.hoomd.axis_histograms, domain_counts, balanced_splits, balanced_grid and
grid_bounds -- the numpy models the GPU census (tests/test_gpu_census.py) must equal exactly --, tied to the domain
predicate (domain_rows) they bin, and `python -m pgsd info --balance`.  Every result is an integer count: no tolerance
anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pgsd.hoomd as hoomd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORTHO = np.array([16.0, 16.0, 16.0, 0.0, 0.0, 0.0], np.float32)
TRI = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)      # the triclinic box of tests/test_gpu_halo.py
UNEQUAL = dict(x_split=[0.25, 0.5], z_split=[0.375])                # ... and its unequal splits, over 3 x 1 x 2 cells
GRIDS = {
    "1x1x1": ((1, 1, 1), {}),
    "2x2x2": ((2, 2, 2), {}),
    "3x1x2": ((3, 1, 2), {}),
    "unequal": ((3, 1, 2), UNEQUAL),
    "8x8x8": ((8, 8, 8), {}),
}


def lattice(rng, N):
    """Every particle on the 1/64 lattice of fractions of ORTHO, in the box or a periodic image: every operation of
    the fraction is exact, and particles sit exactly on 0 and on every bin edge of 2, 64 (and every 64th of 4096) bins."""
    k = rng.integers(0, 64, size=(N, 3))
    k[:64] = np.arange(64)[:min(N, 64), None]
    p = (k / 64.0 + rng.integers(-1, 2, size=(N, 3)) - 0.5) * 16.0
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32), k


def triclinic(rng, N):
    return rng.uniform(-3.0, 3.0, size=(N, 3)).astype(np.float32)


def loop_histograms(position, box, bins, dimensions=3):
    """axis_histograms as a plain row loop over the fractions domain_rows compares."""
    f = hoomd._wrapped_fractions(position, box, dimensions)
    hist = np.zeros((3, bins), dtype=np.int64)
    for a in range(len(f)):
        for v in f[a].tolist():
            if v == v:
                hist[a, int(v * bins)] += 1
    return hist


# ---------------------------------------------------------------- 1. exactness of the bins
@pytest.mark.parametrize("bins", [2, 64, 4096])
def test_histograms_equal_a_row_loop_on_the_lattice(bins):
    rng = np.random.default_rng(1)
    pos, k = lattice(rng, 3000)
    hist = hoomd.axis_histograms(pos, ORTHO, bins)
    assert hist.dtype == np.int64 and hist.shape == (3, bins)
    assert np.array_equal(hist, loop_histograms(pos, ORTHO, bins))
    # the lattice index is the fraction times 64: the bins are known without any floating-point operation
    for a in range(3):
        want = np.bincount(k[:, a] * bins // 64, minlength=bins)
        assert np.array_equal(hist[a], want)
    assert hist[:, 0].min() > 0                 # particles exactly on 0


@pytest.mark.parametrize("bins", [2, 64, 4096])
def test_histograms_equal_a_row_loop_on_triclinic_rows(bins):
    pos = triclinic(np.random.default_rng(2), 5000)
    hist = hoomd.axis_histograms(pos, TRI, bins)
    assert np.array_equal(hist, loop_histograms(pos, TRI, bins))
    assert hist.sum(axis=1).tolist() == [5000] * 3


def test_nan_and_infinite_rows_are_dropped_per_axis():
    pos = triclinic(np.random.default_rng(3), 1000)
    pos[10] = np.nan                    # no axis
    pos[20, 2] = np.inf                 # z enters every fraction of TRI
    pos[30, 0] = -np.inf                # x enters the x fraction only
    pos[40, 1] = np.nan                 # y enters x and y
    hist = hoomd.axis_histograms(pos, TRI, 64)
    assert hist.sum(axis=1).tolist() == [1000 - 4, 1000 - 3, 1000 - 2]
    assert np.array_equal(hist, loop_histograms(pos, TRI, 64))
    counts, nowhere = hoomd.domain_counts(pos, TRI, 2, 2, 2)
    assert nowhere == 4 and counts.sum() == 996


def test_two_dimensions_leave_the_z_row_zero():
    pos = triclinic(np.random.default_rng(4), 1000)
    pos[5, 2] = np.nan                  # z still enters x and y through the tilts
    box2 = np.array([4.0, 4.0, 0.0, 0.5, 0.0, 0.0], np.float32)
    hist = hoomd.axis_histograms(pos, box2, 64, dimensions=2)
    assert np.array_equal(hist, loop_histograms(pos, box2, 64, 2))
    assert not hist[2].any() and hist[:2].sum(axis=1).tolist() == [999, 999]
    counts, nowhere = hoomd.domain_counts(pos, box2, 3, 2, 1, dimensions=2)
    assert counts.sum() == 999 and nowhere == 1
    with pytest.raises(ValueError):
        hoomd.domain_counts(pos, box2, 2, 2, 2, dimensions=2)
    with pytest.raises(ValueError):
        hoomd.balanced_grid(pos, box2, 2, 2, 2, dimensions=2)
    domains, splits = hoomd.balanced_grid(pos, box2, 2, 2, 1, bins=64, dimensions=2)
    assert splits[2] is None and len(domains) == 4


# ---------------------------------------------------------------- 2. tie to the domain predicate
def test_the_cumulative_histogram_is_the_slab_count_of_domain_rows():
    pos = triclinic(np.random.default_rng(5), 4000)
    hist = hoomd.axis_histograms(pos, TRI, 64)
    for a in range(3):
        cum = np.concatenate(([0], np.cumsum(hist[a])))
        for k in range(1, 65):
            hi = [1.0, 1.0, 1.0]
            hi[a] = k / 64
            assert cum[k] == len(hoomd.domain_rows(pos, TRI, hoomd.Domain((0.0, 0.0, 0.0), hi))), (a, k)


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("kind", ["lattice", "tri"])
def test_counts_equal_the_rows_of_every_cell(kind, grid):
    rng = np.random.default_rng(6)
    (pos, box) = (lattice(rng, 3000)[0], ORTHO) if kind == "lattice" else (triclinic(rng, 3000), TRI)
    pos[17] = np.nan
    n, split = GRIDS[grid]
    counts, nowhere = hoomd.domain_counts(pos, box, *n, **split)
    cells = hoomd.domain_grid(*n, **split)
    assert counts.dtype == np.int64 and counts.shape == (len(cells),)
    assert counts.tolist() == [len(hoomd.domain_rows(pos, box, d)) for d in cells]
    assert nowhere == 1 and counts.sum() + nowhere == 3000


# ---------------------------------------------------------------- 3. balanced_splits
def test_a_uniform_histogram_gives_equal_widths():
    for bins, n in ((8, 2), (64, 4), (1024, 8), (4096, 64)):
        assert hoomd.balanced_splits([3] * bins, n) == [1.0 / n] * (n - 1)
    assert hoomd.balanced_splits([3] * 8, 1) == []


def test_a_hand_worked_example():
    # cum = 0 4 4 4 4 6 8 8 8, total 8
    h = [4, 0, 0, 0, 2, 2, 0, 0]
    assert hoomd.balanced_splits(h, 2) == [1 / 8]                   # cum(k) * 2 >= 8 first at k = 1
    # n = 4: cum * 4 >= 8 at k = 1; >= 16 at k = 1, forced to k_1 + 1 = 2; >= 24 at k = 5
    assert hoomd.balanced_splits(h, 4) == [1 / 8, 1 / 8, 3 / 8]
    # empty bins between the particles: the edge is the first that reaches the quota, not the middle of the gap
    assert hoomd.balanced_splits([1, 0, 0, 0, 0, 0, 0, 1], 2) == [1 / 8]
    assert hoomd.balanced_splits([0, 0, 0, 5, 0, 0, 0, 0], 2) == [4 / 8]


def test_an_empty_histogram_gives_equal_edges():
    assert hoomd.balanced_splits([0] * 8, 4) == [0.25, 0.25, 0.25]
    assert hoomd.balanced_splits([0] * 8, 3) == [2 / 8, 3 / 8]      # edges 8 // 3, 16 // 3
    assert hoomd.balanced_splits([0] * 8, 3, min_bins=2) == [2 / 8, 3 / 8]
    assert hoomd.balanced_splits([0] * 16, 5, min_bins=3) == [3 / 16] * 4       # edges max(j * 16 // 5, 3 j)


def test_min_bins_forces_at_both_ends():
    low = [9, 0, 0, 0, 0, 0, 0, 0]      # every quota is reached at edge 1
    assert hoomd.balanced_splits(low, 4) == [1 / 8, 1 / 8, 1 / 8]
    assert hoomd.balanced_splits(low, 4, min_bins=2) == [2 / 8, 2 / 8, 2 / 8]
    high = [0, 0, 0, 0, 0, 0, 0, 9]     # ... at edge 8, beyond what leaves room for the slabs behind
    assert hoomd.balanced_splits(high, 4) == [5 / 8, 1 / 8, 1 / 8]
    assert hoomd.balanced_splits(high, 4, min_bins=2) == [2 / 8, 2 / 8, 2 / 8]
    assert hoomd.balanced_splits(high, 2, min_bins=3) == [5 / 8]


def test_splits_are_accepted_by_domain_grid():
    rng = np.random.default_rng(7)
    for _ in range(50):
        bins = int(2 ** rng.integers(1, 13))
        n = int(rng.integers(1, min(bins, 64) + 1))
        min_bins = int(rng.integers(1, bins // n + 1))
        h = rng.integers(0, 5, size=bins) * (rng.random(bins) < 0.3)
        w = hoomd.balanced_splits(h, n, min_bins)
        assert len(w) == n - 1 and all(v > 0 for v in w) and sum(w) < 1
        assert all((v * bins) == int(v * bins) >= min_bins for v in w) and (1 - sum(w)) * bins >= min_bins
        cells = hoomd.domain_grid(n, 1, 1, x_split=w)
        assert len(cells) == n
        edges = np.cumsum([0] + [int(v * bins) for v in w])
        assert [c.lo[0] for c in cells] == [e / bins for e in edges]


def test_a_dam_break_is_balanced_within_the_largest_bin():
    """Every particle in one eighth of the box: the equal grid gives one cell everything; the balanced grid's slabs
    each hold total / n within the largest bin's count -- cum(k_j) lies in [j total / n, j total / n + largest bin)."""
    rng = np.random.default_rng(8)
    N = 20000
    pos = (rng.random((N, 3)) * 0.5 - 0.5) * np.array([4.0, 4.0, 2.0]) * 0.999
    pos = pos.astype(np.float32)
    box = np.array([4.0, 4.0, 2.0, 0.0, 0.0, 0.0], np.float32)
    equal, _ = hoomd.domain_counts(pos, box, 2, 2, 2)
    assert equal.tolist() == [N, 0, 0, 0, 0, 0, 0, 0]
    bins = 1024
    hist = hoomd.axis_histograms(pos, box, bins)
    for n in (2, 3, 4, 8):
        for a in range(3):
            w = hoomd.balanced_splits(hist[a], n)
            edges = np.cumsum([0] + [int(v * bins) for v in w] + [0])
            edges[-1] = bins
            cum = np.concatenate(([0], np.cumsum(hist[a])))
            forced = any(cum[edges[j] - 1] * n >= j * N for j in range(1, n))    # not the smallest edge: forced
            assert not forced
            slabs = np.diff(cum[edges])
            assert slabs.sum() == N and np.all(np.abs(slabs * n - N) < hist[a].max() * n)
    domains, splits = hoomd.balanced_grid(pos, box, 2, 2, 2, bins=bins)
    counts, nowhere = hoomd.domain_counts(pos, box, 2, 2, 2, *splits)
    assert nowhere == 0 and counts.sum() == N and counts.max() < 1.2 * N / 8
    assert counts.tolist() == [len(hoomd.domain_rows(pos, box, d)) for d in domains]
    assert domains == hoomd.domain_grid(2, 2, 2, *splits)


def test_every_value_error():
    pos = triclinic(np.random.default_rng(9), 100)
    for bins in (0, 1, 3, 100, 8192, -4):
        with pytest.raises(ValueError):
            hoomd.axis_histograms(pos, TRI, bins)
    with pytest.raises(ValueError):
        hoomd.axis_histograms(pos, TRI, 64, dimensions=4)
    with pytest.raises(ValueError):
        hoomd.balanced_splits([1] * 8, 9)                   # n * min_bins > bins
    with pytest.raises(ValueError):
        hoomd.balanced_splits([1] * 8, 3, min_bins=3)
    with pytest.raises(ValueError):
        hoomd.balanced_splits([1] * 8, 0)
    with pytest.raises(ValueError):
        hoomd.balanced_splits([1] * 8, 2, min_bins=0)
    with pytest.raises(ValueError):
        hoomd.balanced_splits([1] * 6, 2)                   # not a power of two
    with pytest.raises(ValueError):
        hoomd.balanced_splits([1, -1], 2)
    for n in ((0, 1, 1), (65, 1, 1), (64, 64, 2), (17, 16, 16)):
        with pytest.raises(ValueError):
            hoomd.domain_counts(pos, TRI, *n)
    with pytest.raises(ValueError):
        hoomd.domain_counts(pos, TRI, 2, 1, 1, x_split=[0.5, 0.25])      # one width too many
    with pytest.raises(ValueError):
        hoomd.domain_counts(pos, TRI, 3, 1, 1, x_split=[0.5, 1e-20])     # a cell of no width
    with pytest.raises(ValueError):
        hoomd.balanced_grid(pos, TRI, 2, 2, 2, bins=100)
    with pytest.raises(ValueError):
        hoomd.balanced_grid(pos, TRI, 2, 2, 2, bins=8, min_bins=5)


# ---------------------------------------------------------------- 4. grid_bounds and domain_grid
def test_grid_bounds_and_domain_grid_against_literals():
    assert hoomd.grid_bounds(1, 1, 1) == ([0.0, 1.0], [0.0, 1.0], [0.0, 1.0])
    assert hoomd.grid_bounds(2, 2, 2) == ([0.0, 0.5, 1.0],) * 3
    third = [0.0, 1 / 3, 2 / 3, 1.0]
    assert hoomd.grid_bounds(3, 1, 2) == (third, [0.0, 1.0], [0.0, 0.5, 1.0])
    assert hoomd.grid_bounds(3, 1, 2, **UNEQUAL) == ([0.0, 0.25, 0.75, 1.0], [0.0, 1.0], [0.0, 0.375, 1.0])
    eighth = [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0]
    assert hoomd.grid_bounds(8, 8, 8) == (eighth,) * 3
    literal = {
        "1x1x1": ([0.0, 1.0], [0.0, 1.0], [0.0, 1.0]),
        "2x2x2": ([0.0, 0.5, 1.0],) * 3,
        "3x1x2": (third, [0.0, 1.0], [0.0, 0.5, 1.0]),
        "unequal": ([0.0, 0.25, 0.75, 1.0], [0.0, 1.0], [0.0, 0.375, 1.0]),
        "8x8x8": (eighth,) * 3,
    }
    for grid, (n, split) in GRIDS.items():
        bx, by, bz = literal[grid]
        want = []
        for z in range(n[2]):
            for y in range(n[1]):
                for x in range(n[0]):
                    want.append(((bx[x], by[y], bz[z]), (bx[x + 1], by[y + 1], bz[z + 1])))
        got = hoomd.domain_grid(*n, **split)
        assert [(d.lo, d.hi) for d in got] == want, grid
    # the refusals of the split lists are domain_grid's as before
    with pytest.raises(ValueError):
        hoomd.grid_bounds(2, 1, 1, x_split=[1.0])
    with pytest.raises(ValueError):
        hoomd.domain_grid(0, 1, 1)


# ---------------------------------------------------------------- 5. the command line
def test_info_balance_prints_splits_and_counts(tmp_path):
    rng = np.random.default_rng(10)
    N = 4000
    box = np.array([4.0, 4.0, 2.0, 0.0, 0.0, 0.0], np.float32)
    pos = ((rng.random((N, 3)) * 0.5 - 0.5) * np.array([4.0, 4.0, 2.0]) * 0.999).astype(np.float32)
    fr = hoomd.Frame()
    fr.configuration.box = box
    fr.particles.N = N
    fr.particles.position = pos
    path = str(tmp_path / "dam.gsd")
    with hoomd.open(path, 'w') as t:
        t.append(fr)
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pgsd-sph_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "pgsd", "info", path, "--balance", "2,2,2", "--frame", "0", "--bins", "256"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(l.strip().split(':', 1) for l in r.stdout.splitlines() if ':' in l)
    _, splits = hoomd.balanced_grid(pos, box, 2, 2, 2, bins=256)
    for axis, w in zip('xyz', splits):
        assert [float(v) for v in lines['%s_split' % axis].strip(' []').split(',')] == w
    equal, _ = hoomd.domain_counts(pos, box, 2, 2, 2)
    balanced, _ = hoomd.domain_counts(pos, box, 2, 2, 2, *splits)
    assert [int(v) for v in lines['equal grid counts'].split()] == equal.tolist() == [N] + [0] * 7
    assert [int(v) for v in lines['balanced grid counts'].split()] == balanced.tolist()
    assert float(lines['equal grid max / mean']) == 8.0
    assert lines['balanced grid max / mean'].strip() == "%.3f" % (balanced.max() / (N / 8))
    assert balanced.max() < 1.3 * N / 8
    bad = subprocess.run([sys.executable, "-m", "pgsd", "info", path, "--balance", "2,2"], env=env, capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode == 1 and "NX,NY,NZ" in bad.stderr
