"""The life cycle of the per-device scratch space behind the GPU passes over staged chunks: growth after a small first
call, reuse after growth, two families interleaved on one allocation, and the call after a refused one.  The scratch is
per process and grow-only, so inside one pytest session an earlier test has usually grown it already: every case here
runs its fixed sequence in ONE fresh child process (never more than one at a time) and compares every result with the
host model there, exactly as the suites of the families do -- integers with numpy.array_equal, sums bit for bit.
The families that came later, each with a scratch and a lock of its own: tests/test_gpu_scratch_cycle.py.

The "just past the first capacity" sizes follow from the library's constants (csrc/pgsd_scratch.hpp and the families'
launchers); the child works them out from the same formulas:
  compaction, row plan   a set holds 8 + round8(4 * nb) + 8 * nb bytes for nb blocks and the first allocation is 64 KiB:
                         nb <= 5460 fits, so 5461 blocks -- of 4096 flags (pgsd_select_rows), of 256 rows (a row plan)
  cell order             5 * round4(n) + 256 * ceil(n / 4096) + 260 words against 16 Ki words: n = 3201 is past it
  chunk statistics       376 bytes + 128 per tile of 4096 entries at four columns against 64 KiB: 510 tiles
  conservation sums      376 bytes + 324 per tile at four types against 64 KiB: 202 tiles
  census                 a fixed allocation: the smallest and the largest histogram, then a cell count
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import os, sys
root, case, path = sys.argv[1:4]
sys.path[:0] = [os.path.join(root, "pgsd-sph_amd"), os.path.join(root, "tests")]
import numpy as np
import pgsd.fl as fl
import pgsd.hoomd as hoomd

TRI = np.array([4.0, 4.0, 2.0, 0.5, 0.25, -0.125], np.float32)
TILE = 4096                          # SEL_PER_BLOCK: flags / entries per workgroup
FIRST = 1 << 16                      # the first allocation of the compaction and the statistics scratch, bytes
set_bytes = lambda nb: 8 + ((nb * 4 + 7) & ~7) + nb * 8
NB_FIT = max(nb for nb in range(5000, 6000) if set_bytes(nb) <= FIRST)
assert NB_FIT == 5460 and set_bytes(NB_FIT + 1) > FIRST
order_words = lambda n: 5 * ((n + 3) & ~3) + 256 * ((n + TILE - 1) // TILE) + 256 + 4
ORDER_PAST = 3201
assert order_words(7) < (1 << 14) < order_words(ORDER_PAST) and order_words(3100) < (1 << 14)
HEAD = 47 * 8                        # the result words of either reduction and the flag word
stats_bytes = lambda tiles, C=4: HEAD + tiles * (3 * C * 8 + 2 * C * 4)
moments_bytes = lambda tiles, TG=4: HEAD + tiles * (9 * TG * 8 + (2 * TG + 1) * 4)
STATS_TILES = min(t for t in range(1, 1000) if stats_bytes(t) > FIRST)
MOMENTS_TILES = min(t for t in range(1, 1000) if moments_bytes(t) > FIRST)
assert (STATS_TILES, MOMENTS_TILES) == (510, 202)

rng = np.random.default_rng(2024)


def host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else x.to_host()


def wide(n, dtype=np.float32):
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 12, n)).astype(dtype)


# ---- one small file: position chunks of three heights, a four-column chunk of 64 rows, the five inputs of the sums, a
# second position and an image for the displacements
A = {'pos5': rng.uniform(-3.0, 3.0, size=(5, 3)).astype(np.float32),
     'pos4096': rng.uniform(-3.0, 3.0, size=(4096, 3)).astype(np.float32),
     'pos70001': rng.uniform(-3.0, 3.0, size=(70001, 3)).astype(np.float32),
     'c4': wide(64 * 4).reshape(64, 4),
     'tid': (np.arange(64) % 5).astype(np.uint32), 'm': np.abs(wide(64)) + np.float32(0.5), 'v': wide(64 * 3).reshape(64, 3),
     'e': wide(64), 'x': rng.uniform(-3.0, 3.0, size=(64, 3)).astype(np.float32)}
A['c4'][[3, 17, 63], [0, 1, 3]] = [np.nan, np.inf, -0.0]
A['v'][9, 1] = np.nan
A['x2'] = rng.uniform(-3.0, 3.0, size=(64, 3)).astype(np.float32)
A['img'] = rng.integers(-2, 3, size=(64, 3)).astype(np.int32)
with fl.open(path, 'w', application="test", schema="none", schema_version=[1, 0]) as f:
    for name, a in A.items():
        f.write_chunk(name, a.reshape(len(a), -1))
    f.end_frame()
MOMENTS = ['tid', 'm', 'v', 'e', 'x']
DISPLACEMENTS = ['x', None, 'x2', 'img', 'tid']                     # position a, image a, position b, image b, typeid
VECTORS = hoomd.box_vectors(TRI)


def dev(f, rows):
    return fl._device_from_host(np.ascontiguousarray(rows, dtype=np.int32), f.pipeline_device())


def same_fields(got, want, slots, bitwise, what):
    """Integers and extrema with numpy.array_equal, the fields in `bitwise` (float64 sums) bit for bit."""
    for q in slots:
        g, w = getattr(got, q), getattr(want, q)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, q)
        if q in bitwise:
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, q, g.tolist(), w.tolist())
        else:
            assert np.array_equal(g, w), (what, q, g.tolist(), w.tolist())


def check_select_rows(n):
    flags = (rng.random(n) < 0.5).astype(np.uint8) * rng.integers(1, 255, size=n, dtype=np.uint8)
    index, count = fl.select_rows(fl._device_from_host(flags, 0))
    want = np.flatnonzero(flags).astype(np.int32)
    assert count == len(want), (n, count, len(want))
    assert np.array_equal(host(index).astype(np.int32), want), n


def check_plan(f, n, N):
    rows = rng.integers(0, N, size=n).astype(np.int32)
    rows[n // 2] = N                                     # an entry outside: refused, touches nothing
    model = fl.row_plan_model(rows.astype(np.uint32), N, 256)
    plan = f.plan_rows(dev(f, rows), N)
    assert (plan.n, plan.N, plan.block_rows) == (n, N, 256)
    assert plan.touched_blocks == len(model.blocks) and plan.runs == len(model.runs)
    assert plan.staged_rows == model.staged_rows
    assert np.array_equal(plan.blocks(), model.blocks) and np.array_equal(plan.run_list(), model.runs)
    assert np.array_equal(plan.rows2.to_host(), model.rows2)


def check_order(f, n, grid=(8, 8, 4), name='pos4096'):
    N = len(A[name])
    rows = rng.integers(0, N, size=n).astype(np.int32)
    n_owned = n - n // 3
    shift = rng.integers(-1, 2, size=(n - n_owned, 3)).astype(np.int32)
    want_rows, want_cell, perm = hoomd.cell_order(A[name], TRI, rows, grid, n_owned=n_owned)
    d_rows, d_shift = dev(f, rows), fl._device_from_host(shift, f.pipeline_device())
    cell = f.order_rows_by_cell_device(0, name, TRI, grid, d_rows, n_owned=n_owned, shift=d_shift)
    assert np.array_equal(host(d_rows), want_rows) and np.array_equal(host(cell), want_cell), n
    assert np.array_equal(host(d_shift).reshape(-1, 3), shift[perm[n_owned:] - n_owned]), n


def check_stats(f, n):
    rows = rng.integers(0, 64, size=n).astype(np.int32)
    got = f.chunk_stats_device(0, 'c4', rows=dev(f, rows))
    same_fields(got, hoomd.column_stats(A['c4'], rows=rows), hoomd.FieldStats.__slots__, ('sum',), ('stats', n))


def check_moments(f, n, n_types=4):
    rows = rng.integers(0, 64, size=n).astype(np.int32)
    got = f.frame_moments_device([(0, name) for name in MOMENTS], type0=0, n_types=n_types, rows=dev(f, rows))
    want = hoomd.particle_moments(typeid=A['tid'], mass=A['m'], velocity=A['v'], energy=A['e'], position=A['x'], type0=0,
                                  n_types=n_types, rows=rows)
    assert got.other == want.other, n
    sums = ('mass', 'momentum', 'kinetic', 'internal', 'first_moment')
    same_fields(got, want, ('count', 'bad') + sums, sums, ('moments', n))


def displacements(f, rows, n_types=4):
    return f.frame_displacements_device([None if name is None else (0, name) for name in DISPLACEMENTS], VECTORS, VECTORS,
                                        type0=0, n_types=n_types, rows=dev(f, rows))


def check_displacements(f, n, n_types=4):
    rows = rng.integers(0, 64, size=n).astype(np.int32)
    got = displacements(f, rows, n_types)
    want = hoomd.particle_displacements(A['x'], A['x2'], None, A['img'], VECTORS, VECTORS, typeid=A['tid'], type0=0,
                                        n_types=n_types, rows=rows)
    assert got.other == want.other, n
    values = ('drift', 'square', 'largest')
    same_fields(got, want, ('count', 'bad', 'largest_entry') + values, values, ('displacements', n))


def check_domain(f, name, cell):
    rows, count = f.select_domain_device(0, name, TRI, cell)
    want = hoomd.domain_rows(A[name], TRI, cell)
    assert count == len(want) and np.array_equal(host(rows), want), name


def check_halo(f, name, cell, width=0.4):
    owned, ghosts, shift = hoomd.halo_rows(A[name], TRI, cell, width)
    rows, n_owned, n_ghost, got = f.select_halo_device(0, name, TRI, cell, width)
    assert (n_owned, n_ghost) == (len(owned), len(ghosts)) and n_ghost > 0
    assert np.array_equal(host(rows), np.concatenate([owned, ghosts])) and np.array_equal(host(got).reshape(-1, 3), shift)


def check_hist(f, name, bins):
    assert np.array_equal(f.domain_histogram_device(0, name, TRI, bins), hoomd.axis_histograms(A[name], TRI, bins)), bins


def check_counts(f, name, n=(4, 4, 4)):
    counts, nowhere = f.domain_counts_device(0, name, TRI, n, [b[1:-1] for b in hoomd.grid_bounds(*n)])
    want, want_nowhere = hoomd.domain_counts(A[name], TRI, *n)
    assert np.array_equal(counts, want) and nowhere == want_nowhere


def refused(call, message):
    try:
        call()
    except ValueError as e:
        assert message in str(e), str(e)
        return
    raise AssertionError("not refused: " + message)


with fl.open(path, 'r') as f:
    if case == "compaction":            # tiny, just past the first capacity, inside the grown one, tiny
        for n in (7, (NB_FIT + 1) * TILE - 3, 100_003, 7):
            check_select_rows(n)
    elif case == "plan":
        for n, N in ((5, 1000), (3001, NB_FIT * 256 + 1), (5, 1000)):
            check_plan(f, n, N)
    elif case == "order":
        for n in (7, ORDER_PAST, 7):
            check_order(f, n)
    elif case == "stats":
        for n in (5, (STATS_TILES - 1) * TILE + 1, 5):
            check_stats(f, n)
    elif case == "moments":
        for n in (5, (MOMENTS_TILES - 1) * TILE + 1, 5):
            check_moments(f, n)
    elif case == "census":
        check_hist(f, 'pos70001', 2)
        check_hist(f, 'pos70001', 4096)
        check_counts(f, 'pos70001')
        check_hist(f, 'pos5', 2)
    elif case == "interleaved":
        # a halo selection (two compaction sets) between two domain selections of different N; a plan and a compaction of
        # flags on the same allocation; statistics, conservation sums and displacements in turn: one final kernel clears
        # the flag word behind all grouped calls
        cell = hoomd.domain_grid(2, 2, 1)[1]
        check_domain(f, 'pos5', cell)
        check_halo(f, 'pos70001', cell)
        check_domain(f, 'pos4096', cell)
        check_plan(f, 300, 70001)
        check_select_rows(4097)
        check_halo(f, 'pos4096', cell)
        check_domain(f, 'pos70001', cell)
        check_moments(f, 4097)
        check_displacements(f, 5)
        check_stats(f, 70001)
        check_displacements(f, 4097)
        check_moments(f, 5, n_types=2)
        check_displacements(f, 5001, n_types=2)
        check_stats(f, 5)
        check_order(f, 4097)
        check_hist(f, 'pos4096', 64)
        check_domain(f, 'pos5', cell)
    elif case == "refused":
        bad = rng.integers(0, 64, size=5001).astype(np.int32)
        bad[4999] = 64
        refused(lambda: f.chunk_stats_device(0, 'c4', rows=dev(f, bad)), "an entry of the row list lies outside the chunk")
        check_stats(f, 5001)
        refused(lambda: f.frame_moments_device([(0, name) for name in MOMENTS], n_types=4, rows=dev(f, bad)),
                "an entry of the row list lies outside the chunks")
        check_moments(f, 5001)
        check_displacements(f, 5001)
        # a refused displacement between a statistics call and a sums call: the call before and the call after are exact
        check_stats(f, 4097)
        refused(lambda: displacements(f, bad), "an entry of the row list lies outside the chunks")
        check_moments(f, 4097)
        check_displacements(f, 5)
        check_stats(f, 63)
        bad[4999] = 4096
        refused(lambda: f.order_rows_by_cell_device(0, 'pos4096', TRI, (8, 8, 4), dev(f, bad)), "outside the position chunk")
        check_order(f, 5001)
    else:
        raise SystemExit("unknown case " + case)
    f.wait_read()
print("ok", case)
'''

CASES = ["compaction", "plan", "order", "stats", "moments", "census", "interleaved", "refused"]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    d = tmp_path_factory.mktemp("scratch_reuse")
    script = d / "child.py"
    script.write_text(CHILD)
    return script, d


@pytest.mark.parametrize("case", CASES)
def test_the_scratch_serves_a_fresh_process(child, case):
    script, d = child
    r = subprocess.run([sys.executable, str(script), ROOT, case, str(d / (case + ".gsd"))], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok " + case), r.stdout + r.stderr
