"""Indexed device reads (read_chunk_device(..., rows=...)) over every element type, destination shape and route.

At wait_read the staged chunk is gathered through a row list by unpack_rows_kernel<64, 2, F64, G = true> (Scalar4
destinations: four code branches) or by gather_elems_kernel (+ fill_cols_kernel) for everything else; no other entry
point reaches them.  Every comparison is bit exact against a host reference: the poison pattern, the fill over the rows
of good entries, then oracle_pack(chunk[rows]) per chunk in submission order -- the oracle's element rules with numpy's
fancy indexing as the gather.  Destinations are views into poisoned buffers with 64 guard rows on both sides, and the
whole buffer is compared, so a store outside the columns and rows that were asked for shows as well.

A  randomised matrix (fixed seeds)        B  the Scalar4 branch table, both kernel families
C  entries outside the chunk              D  the grid-stride loop of the element gather
E  several launches in one wait_read: submission order decides overlaps, fills see every pending chunk
"""
import os
import shutil
import tempfile

import numpy as np
import pytest

import gpu_common as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import pgsd.fl as fl  # noqa: E402
from pgsd import _lib  # noqa: E402

INTS = ["uint8", "uint16", "uint32", "uint64", "int8", "int16", "int32", "int64"]
FLOATS = ["float32", "float64"]
ALL = INTS + FLOATS
HEIGHTS = (1, 130, 5000)            # 130: just past one 128-row workgroup of the row-per-lane kernel (64 x 2)
BIG = 300_001                       # more elements than the gather's grid covers in one pass (part D)
GUARD = 64
POISON = ((np.arange(251) * 7 + 13) % 256).astype(np.uint8)       # a prime period: no two rows of a buffer look alike
ROUTES = ("plain", "sparse", "whole")
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 1000)
F32_FILL, F64_FILL = 1.2345678, -1.0000000001                     # (the two halves of the double differ)

SPECS = [(dt, m) for dt in ALL for m in (1, 3, 4)] + [(dt, 2) for dt in ("float32", "uint32", "int32")] \
    + [("uint16", 7), ("float64", 5)]
# second float32 chunks of width 1 and 2: a float64 Scalar4 takes float32 chunks only, and two DIFFERENT chunks are
# needed for a swapped pair to show
EXTRA = [("float32x1b", "float32", 1), ("float32x2b", "float32", 2)]
BIG_SPECS = [("uint8", 4), ("float32", 3), ("uint32", 1), ("float64", 2)]


def _name(dt, m):
    return "c/%sx%d" % (dt, m)


def _values(rng, H, dt, m):
    """Seeded values with the special ones at both ends of the chunk (as far as it has room for them)."""
    a = G.rand_array(rng, (H, m), dt)
    if a.dtype.kind == 'f':
        sp = [np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-40 if a.dtype.itemsize == 4 else 5e-320]
        if a.dtype.itemsize == 8:
            sp += [1e300, -3.5e38, 1e-40]       # round to inf, to -inf and to a denormal in float32
        sp = np.array(sp).astype(a.dtype)
        flat = a.reshape(-1)
        k = min(len(sp), flat.size)
        flat[:k] = sp[:k]
        if flat.size >= 2 * len(sp):
            flat[-len(sp):] = sp[::-1]
    return a


def _write(path, H, specs, seed):
    rng = np.random.default_rng(seed)
    data = {}
    with fl.open(path, 'w', application="indexed", schema="raw", schema_version=[1, 0]) as f:
        for name, dt, m in specs:
            data[name] = _values(rng, H, dt, m)
            f.write_chunk(name, data[name])
        f.end_frame()
    return path, data


@pytest.fixture(scope="module")
def files():
    """H -> (path, {chunk name: the (H, M) array written}), written through the host path."""
    d = tempfile.mkdtemp(prefix="pgsd_indexed_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        small = [(_name(dt, m), dt, m) for dt, m in SPECS] + [("c/" + n, dt, m) for n, dt, m in EXTRA]
        out = {H: _write(os.path.join(d, "h%d.gsd" % H), H, small, 100 + H) for H in HEIGHTS}
        out[BIG] = _write(os.path.join(d, "big.gsd"), BIG, [(_name(dt, m), dt, m) for dt, m in BIG_SPECS], 99)
        yield out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _family(monkeypatch, family, block_rows=None):
    if family == "tiles":
        monkeypatch.setenv("PGSD_UNPACK_KERNEL", "tiles")
    else:
        monkeypatch.delenv("PGSD_UNPACK_KERNEL", raising=False)
    if block_rows:
        monkeypatch.setenv("PGSD_PLAN_BLOCK_ROWS", str(block_rows))
    _lib.lib.pgsd_reload_tuning()


def _dev_list(r):
    r = np.ascontiguousarray(np.asarray(r, dtype=np.int64).astype(np.uint32))
    return fl.DeviceBuffer((len(r),), np.uint32, pattern=r)


def _rows_arg(f, route, d_rows, H):
    """What goes into rows=: the plain list (whole-chunk route), a sparse plan (rows2 / staged_rows), or a plan above
    its threshold, which takes the whole-chunk route with the plan's own list."""
    if route == "plain":
        return d_rows
    plan = f.plan_rows(d_rows, H, threshold=1.0 if route == "sparse" else -1.0)
    assert plan.sparse == (route == "sparse")
    return plan


def _accepts(sdt, ddt, bitcast):
    """make_unpack_job's rules"""
    s, d = np.dtype(sdt), np.dtype(ddt)
    if bitcast:
        return s.itemsize == d.itemsize
    return not (s.kind == 'f' and d.kind != 'f') and not (s.kind != 'f' and d.kind == 'f' and s.itemsize == 8)


def _fill_value(dt):
    dt = np.dtype(dt)
    if dt.kind == 'f':
        return F32_FILL if dt.itemsize == 4 else F64_FILL
    return int(np.iinfo(dt).max) - 5


class Dest:
    """n rows of S elements inside a poisoned buffer, GUARD rows before and behind; `off` bytes past a 16-byte
    boundary.  `exp` is the host image of the whole buffer."""

    def __init__(self, n, S, dt, off=0):
        self.n, self.S, self.dt = n, S, np.dtype(dt)
        row = S * self.dt.itemsize
        self.start = GUARD * row + off
        nbytes = (2 * GUARD + n) * row + 16
        self.buf = fl.DeviceBuffer((nbytes,), np.uint8, pattern=POISON)
        assert self.buf.ptr % 16 == 0
        self.out = self.buf.view(dtype=self.dt, shape=(n, S), offset_bytes=self.start)
        self.exp = np.resize(POISON, nbytes).copy()
        self.rows = self.exp[self.start:self.start + n * row].view(self.dt).reshape(n, S)
        self.reads = []
        self.fill = None

    def read(self, f, data, name, c0, rows_arg, bitcast=False, fill=None):
        M = data[name].shape[1]
        f.read_chunk_device(0, name, out=self.out, columns=(c0, c0 + M), bitcast=bitcast, rows=rows_arg, wait=False,
                            fill=fill)
        self.reads.append((name, c0, bitcast))
        if fill is not None:
            self.fill = fill

    def expect(self, data, r, good=None):
        """steps 2 and 3 of the reference over the rows whose entries lie in the chunk (all of them: good = None)"""
        sel = slice(None) if good is None else good
        if self.fill is not None:
            self.rows[sel, :] = np.array(self.fill, dtype=self.dt)
        for name, c0, bitcast in self.reads:
            chunk = data[name]
            M = chunk.shape[1]
            self.rows[sel, c0:c0 + M] = G.oracle_pack(chunk[r[sel]], M, out_dtype=self.dt, bitcast=bitcast)

    def check(self, what):
        got = self.buf.to_host()
        if got.tobytes() != self.exp.tobytes():
            at = int(np.flatnonzero(got != self.exp)[0]) - self.start
            row = self.S * self.dt.itemsize
            pytest.fail("%s: %d bytes differ, the first in destination row %d, column %d (%d rows of %d x %s, reads %r, "
                        "fill %r)" % (what, int((got != self.exp).sum()), at // row, (at % row) // self.dt.itemsize,
                                      self.n, self.S, self.dt, self.reads, self.fill))


def _list(rng, kind, n, H):
    if kind == "random":
        return rng.integers(0, H, size=n)
    if kind in ("ascending", "descending"):
        r = np.sort(rng.choice(H, size=n, replace=False))
        return r if kind == "ascending" else r[::-1].copy()
    if kind == "same":
        return np.full(n, int(rng.integers(0, H)))
    r = rng.integers(0, H, size=n)                  # "ends": row 0 and row H - 1 are in it
    at = rng.choice(n, size=min(n, 2), replace=False)
    r[at[0]] = 0
    r[at[-1]] = H - 1
    return r


def test_the_poison_of_a_fresh_buffer_is_the_pattern_the_reference_starts_from():
    d = Dest(3, 5, "int16", off=4)
    d.check("untouched")


# ------------------------------------------------------------------ A. randomised matrix
def _free_c0(rng, used, S, M, disjoint):
    spots = [c for c in range(S - M + 1) if not disjoint or not any(used[c:c + M])]
    return int(rng.choice(spots)) if spots else None


@pytest.mark.parametrize("seed", range(48))
def test_random_indexed_reads(files, monkeypatch, seed):
    rng = np.random.default_rng(7000 + seed)
    H = int(rng.choice(HEIGHTS))
    route = str(rng.choice(ROUTES))
    family = str(rng.choice(["rows", "rows", "tiles"]))
    _family(monkeypatch, family, int(rng.choice([64, 256])))
    n = min(int(rng.choice(LENGTHS + (H,))), H)
    kind = str(rng.choice(["random", "ascending", "descending", "same", "ends"]))
    r = _list(rng, kind, n, H)
    path, data = files[H]
    what = "seed %d: H %d, %s route, %s family, %d %s rows" % (seed, H, route, family, n, kind)
    dests, used, scalar4 = [], [], set()
    with fl.open(path, 'r') as f:
        rows_arg = _rows_arg(f, route, _dev_list(r), H)         # ONE list object: the reads share a launch
        for _ in range(int(rng.integers(1, 7))):
            d = c0 = None
            if dests and rng.random() < 0.5:
                # one more chunk into a destination that has one already, mostly on columns of its own
                i = int(rng.integers(0, len(dests)))
                single = [k for k in sorted(scalar4) if len(dests[k].reads) == 1]
                if single and rng.random() < 0.7:
                    i = single[int(rng.integers(0, len(single)))]
                d = dests[i]
                fits = [(dt, m, bc) for dt, m in SPECS for bc in (False, True) if m <= d.S and _accepts(dt, d.dt, bc)]
                keep_s4 = i in scalar4 and len(d.reads) == 1 and rng.random() < 0.85
                if keep_s4:     # ... and a second chunk the row-per-lane kernel takes too
                    fits = [(dt, m, dt != "float32") for dt, m in SPECS if m <= 3 and
                            (dt == "float32" or (d.dt == np.float32 and dt in ("uint32", "int32")))]
                sdt, M, bitcast = fits[int(rng.integers(0, len(fits)))]
                c0 = _free_c0(rng, used[i], d.S, M, keep_s4 or rng.random() < 0.75)
                if c0 is None:
                    c0 = _free_c0(rng, used[i], d.S, M, False)
            elif rng.random() < 0.5:
                # Scalar4 style: what the row-per-lane kernel takes while the view is 16-byte aligned
                ddt = str(rng.choice(FLOATS))
                M = int(rng.integers(1, 5))
                sdt, bitcast = "float32", False
                if ddt == "float32" and rng.random() < 0.4:
                    sdt, bitcast = str(rng.choice(["uint32", "int32"])), True
                off = (4 if ddt == "float32" else 8) if rng.random() < 0.2 else 0
                d = Dest(n, 4, ddt, off)
                scalar4.add(len(dests))
            else:
                sdt, M = SPECS[int(rng.integers(0, len(SPECS)))]
                bitcast = rng.random() < 0.3
                ddt = str(rng.choice([t for t in ALL if _accepts(sdt, t, bitcast)]))
                S = int(rng.choice([s for s in (M, M + 1, 4, 8, 17) if s >= M]))
                isz = np.dtype(ddt).itemsize
                d = Dest(n, S, ddt, max(4, isz) if rng.random() < 0.25 else 0)
            if c0 is None:
                dests.append(d)
                used.append([False] * d.S)
                i = len(dests) - 1
                c0 = int(rng.integers(0, d.S - M + 1))
            fill = _fill_value(d.dt) if d.fill is None and rng.random() < (0.5 if i in scalar4 else 0.3) else None
            d.read(f, data, _name(sdt, M), c0, rows_arg, bitcast=bool(bitcast), fill=fill)
            used[i][c0:c0 + M] = [True] * M
        f.wait_read()
    for d in dests:
        d.expect(data, r)
        d.check(what)


# ------------------------------------------------------------------ B. the Scalar4 branch table
# branch -> (reads, fill?); a read = (chunk, c0); "w" = a 32-bit chunk for one column: uint32 bits into a float32
# destination, a second float32 chunk into a float64 one (unrows_group takes only f32 -> f64 in the f64 pass)
W32 = {"float32": ("c/uint32x1", True), "float64": ("c/float32x1b", False)}
BRANCHES = {
    "xyz_fill": ([("c/float32x3", 0)], True),
    "hot_xyz_w": ([("c/float32x3", 0), ("w", 3)], False),
    "compose_w2_at_1": ([("c/float32x2", 1)], True),
    "compose_w1_at_0_and_2": ([("c/float32x1", 0), ("w", 2)], True),
    "compose_w3_at_1": ([("c/float32x3", 1)], True),
    "other_w4": ([("c/float32x4", 0)], False),
    "other_w2_w2": ([("c/float32x2", 0), ("c/float32x2b", 2)], False),
    "other_w1_at_3": ([("c/float32x1", 3)], False),
}


def _branch(f, data, branch, ddt, rows_arg, n, reverse=False):
    """Submit the reads of one branch into a fresh Scalar4 of ddt; the fill rides on the first read."""
    reads, with_fill = BRANCHES[branch]
    d = Dest(n, 4, ddt)
    fill = _fill_value(ddt) if with_fill else None
    for name, c0 in (reads[::-1] if reverse else reads):
        name, bitcast = W32[ddt] if name == "w" else (name, False)
        d.read(f, data, name, c0, rows_arg, bitcast=bitcast, fill=fill)
        fill = None
    return d


@pytest.mark.parametrize("family", ["rows", "tiles"])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 1000])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("ddt", FLOATS)
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_scalar4_branch(files, monkeypatch, branch, ddt, route, n, family):
    H = 5000
    _family(monkeypatch, family, 64)
    rng = np.random.default_rng(n)
    r = _list(rng, "ends", n, H)
    path, data = files[H]
    with fl.open(path, 'r') as f:
        d = _branch(f, data, branch, ddt, _rows_arg(f, route, _dev_list(r), H), n, reverse=(n == 129))
        f.wait_read()
    d.expect(data, r)
    d.check("%s into %s, %s route, %s family" % (branch, ddt, route, family))


# ------------------------------------------------------------------ C. entries outside the chunk
def _list_with_bad_entries(H, n=140):
    rng = np.random.default_rng(n)
    r = _list(rng, "ends", n, H)
    for at, v in ((0, H), (5, 0xFFFFFFFF), (63, H + 63), (64, H), (127, 0xFFFFFFFF), (128, H + 63), (n - 1, H)):
        r[at] = v
    return r, r < H


def _refused(f, d, data, r, good, what):
    with pytest.raises(RuntimeError, match="Invalid pgsd argument"):
        f.wait_read()
    d.expect(data, r, good)         # rows of bad entries keep the poison: no chunk element, no fill
    d.check(what)


@pytest.mark.parametrize("family", ["rows", "tiles"])
@pytest.mark.parametrize("route", ["plain", "sparse"])
@pytest.mark.parametrize("ddt", FLOATS)
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_scalar4_branch_refuses_entries_outside_the_chunk(files, monkeypatch, branch, ddt, route, family):
    H = 5000
    _family(monkeypatch, family, 64)
    r, good = _list_with_bad_entries(H)
    path, data = files[H]
    with fl.open(path, 'r') as f:
        d = _branch(f, data, branch, ddt, _rows_arg(f, route, _dev_list(r), H), len(r))
        _refused(f, d, data, r, good, "%s into %s, %s route, %s family" % (branch, ddt, route, family))
        # the handle is fine afterwards
        ok = r[good]
        d2 = _branch(f, data, branch, ddt, _rows_arg(f, route, _dev_list(ok), H), len(ok))
        f.wait_read()
        d2.expect(data, ok)
        d2.check("the good read behind it")


@pytest.mark.parametrize("with_fill", [False, True])
@pytest.mark.parametrize("route", ["plain", "sparse"])
def test_narrow_gather_refuses_entries_outside_the_chunk(files, monkeypatch, route, with_fill):
    H = 5000
    _family(monkeypatch, "rows", 64)
    r, good = _list_with_bad_entries(H)
    path, data = files[H]
    with fl.open(path, 'r') as f:
        d = Dest(len(r), 5, "int32")
        d.read(f, data, "c/uint8x3", 1, _rows_arg(f, route, _dev_list(r), H), fill=-77 if with_fill else None)
        _refused(f, d, data, r, good, "uint8 x 3 into int32, %s route" % route)
        ok = r[good]
        d2 = Dest(len(ok), 5, "int32")
        d2.read(f, data, "c/uint8x3", 1, _rows_arg(f, route, _dev_list(ok), H))
        f.wait_read()
        d2.expect(data, ok)
        d2.check("the good read behind it")


# ------------------------------------------------------------------ D. the grid-stride loop of the element gather
def _grid_lanes():
    return torch.cuda.get_device_properties(0).multi_processor_count * 16 * 256


def _big_list(n):
    return np.random.default_rng(n).integers(0, BIG, size=n)


def test_gather_grid_stride_loop(files, monkeypatch):
    _family(monkeypatch, "rows")
    n = min(BIG, _grid_lanes() // 4 + 1000)
    assert n * 4 > _grid_lanes(), "the list no longer issues more elements than one pass of the grid takes"
    r = _big_list(n)
    path, data = files[BIG]
    with fl.open(path, 'r') as f:
        d = Dest(n, 5, "int32")
        d.read(f, data, "c/uint8x4", 1, _dev_list(r))
        f.wait_read()
    d.expect(data, r)
    d.check("uint8 x 4 into int32, stride 5")


def test_gather_grid_stride_loop_of_single_column_chunks(files, monkeypatch):
    _family(monkeypatch, "rows")
    n = min(BIG, _grid_lanes() // 4 + 1000)
    r = _big_list(n)
    path, data = files[BIG]
    with fl.open(path, 'r') as f:
        d = Dest(n, 1, "float64")
        d.read(f, data, "c/uint32x1", 0, _dev_list(r))
        f.wait_read()
    d.expect(data, r)
    d.check("uint32 x 1 into float64")      # the M == 1 shortcut over many blocks, whatever the grid
    if not n > _grid_lanes():
        pytest.skip("M == 1 issues one element per entry: its grid-stride loop needs more than %d entries, and a plain "
                    "list holds at most the chunk's %d rows (the bytes above were checked)" % (_grid_lanes(), BIG))


# ------------------------------------------------------------------ E. several launches in one wait
@pytest.mark.parametrize("first", ["float64x2", "float32x3"])
def test_the_later_chunk_wins_by_submission(files, monkeypatch, first):
    """Two chunks that overlap in column 1, read by threads of their own: the one submitted second must win whichever
    pread finishes first."""
    _family(monkeypatch, "rows")
    n = 5000
    r = _big_list(n)
    path, data = files[BIG]
    reads = [("c/float64x2", 0), ("c/float32x3", 1)]
    with fl.open(path, 'r') as f:
        rows = _dev_list(r)
        d = Dest(n, 4, "float64")
        for name, c0 in (reads if first == "float64x2" else reads[::-1]):
            d.read(f, data, name, c0, rows)
        f.wait_read()
    d.expect(data, r)
    d.check("%s first" % first)


@pytest.mark.parametrize("first", ["xyz", "w"])
def test_a_fill_sees_the_chunks_of_other_launches(files, monkeypatch, first):
    """xyz with fill = 1.0 through one list, the type id into w through another of the same contents: two launches,
    and the fill must leave w to the chunk that feeds it (read_chunk_device: "no chunk read before the same
    wait_read")."""
    _family(monkeypatch, "rows")
    H, n = 5000, 1000
    r = _list(np.random.default_rng(3), "ends", n, H)
    path, data = files[H]
    with fl.open(path, 'r') as f:
        rows_a, rows_b = _dev_list(r), _dev_list(r)
        assert rows_a.ptr != rows_b.ptr
        d = Dest(n, 4, "float32")
        for which in (("xyz", "w") if first == "xyz" else ("w", "xyz")):
            if which == "xyz":
                d.read(f, data, "c/float32x3", 0, rows_a, fill=1.0)
            else:
                d.read(f, data, "c/uint32x1", 3, rows_b, bitcast=True)
        f.wait_read()
    d.expect(data, r)
    d.check("%s first" % first)
