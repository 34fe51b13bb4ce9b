"""Particle tracks on the GPU: the row plan of PGSDFile.plan_rows (mark / scan / remap kernels) must equal
pgsd.fl.row_plan_model exactly; a read through a plan must give the host reader's rows byte for byte while reading only
the touched runs of the file (the private read counters say so); read_tracks_device must equal read_tracks."""
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
from pgsd import _lib  # noqa: E402

import test_tracks_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = {"t/f32x3": (np.float32, 3), "t/u32": (np.uint32, 1), "t/i32x3": (np.int32, 3), "t/f64x2": (np.float64, 2)}


def _block_rows(monkeypatch, R):
    monkeypatch.setenv("PGSD_PLAN_BLOCK_ROWS", str(R))
    _lib.lib.pgsd_reload_tuning()


def _dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64).astype(np.uint32).view(dtype))).cuda()


def _write_raw(path, N, seed=0, other_N=None):
    """One frame of raw chunks (float32 x 3, uint32 x 1, int32 x 3, float64 x 2) through the host path."""
    rng = np.random.default_rng(seed)
    data = {}
    with fl.open(path, 'w', application="tracks", schema="raw", schema_version=[1, 0]) as f:
        for name, (dt, m) in CHUNKS.items():
            a = rng.integers(-1000, 1000, size=(N, m)).astype(dt) if np.dtype(dt).kind in 'iu' \
                else rng.standard_normal((N, m)).astype(dt)
            if np.dtype(dt).kind == 'u':
                a = rng.integers(0, 1 << 31, size=(N, m)).astype(dt)
            data[name] = a
            f.write_chunk(name, a)
        if other_N:
            f.write_chunk("t/other", rng.standard_normal((other_N, 3)).astype(np.float32))
        f.end_frame()
    return data


@pytest.fixture(scope="module")
def raw_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tracks") / "raw.gsd")
    return path, _write_raw(path, 100_003, other_N=5000)


def _check_plan(f, rows, N, R):
    model = fl.row_plan_model(np.asarray(rows, dtype=np.int64).astype(np.uint32), N, R)
    d_rows = _dev(rows)
    plan = f.plan_rows(d_rows, N)
    assert (plan.n, plan.N, plan.block_rows) == (len(rows), N, R)
    assert plan.touched_blocks == len(model.blocks) and plan.runs == len(model.runs)
    assert plan.staged_rows == model.staged_rows
    np.testing.assert_array_equal(plan.blocks(), model.blocks)
    np.testing.assert_array_equal(plan.run_list(), model.runs)
    np.testing.assert_array_equal(plan.rows2.to_host(), model.rows2)
    assert plan.rows is d_rows


def test_gpu_plan_equals_the_model_on_the_listed_cases(raw_file, monkeypatch):
    with fl.open(raw_file[0], 'r') as f:
        for name, rows, N, R in M.plan_cases():
            _block_rows(monkeypatch, R)
            _check_plan(f, rows, N, R)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 70_001, 3_000_000])
def test_gpu_plan_equals_the_model_on_random_lists(raw_file, monkeypatch, N):
    _block_rows(monkeypatch, 64)
    rng = np.random.default_rng(N)
    with fl.open(raw_file[0], 'r') as f:
        for n in (1, 17, min(N, 5000), N):
            _check_plan(f, rng.integers(0, N, size=n), N, 64)
        clustered = (rng.integers(0, N, size=8)[:, None] + np.arange(40)[None, :]).reshape(-1) % N
        _check_plan(f, clustered, N, 64)
        _check_plan(f, np.concatenate([clustered, [N, N + 7, 0xFFFFFFFF]]), N, 64)


def _same(t, want):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()


@pytest.mark.parametrize("R", [64, 4096])
def test_planned_read_equals_the_host_readers_rows(raw_file, monkeypatch, R):
    path, data = raw_file
    N = 100_003
    _block_rows(monkeypatch, R)
    rng = np.random.default_rng(R)
    lists = {
        "K = 1": np.array([N - 1]),
        "duplicates, unsorted": np.array([70_000, 5, 5, 99_999, 64, 63, 70_000, 12_345]),
        "clusters": (rng.integers(0, N - 50, size=6)[:, None] + np.arange(50)[None, :]).reshape(-1),
        "K = N": rng.permutation(N),
    }
    with fl.open(path, 'r') as f:
        host = {name: f.read_chunk(0, name) for name in CHUNKS}
        for name in CHUNKS:
            assert host[name].tobytes() == (data[name][:, 0] if CHUNKS[name][1] == 1 else data[name]).tobytes()
        for what, r in lists.items():
            d_rows = _dev(r)
            plan = f.plan_rows(d_rows, N, threshold=1.0)        # always the sparse route
            assert plan.sparse
            n = len(r)
            for name in CHUNKS:                                  # dense destinations of the chunk's own type
                assert _same(f.read_chunk_device(0, name, rows=plan), host[name][r]), (what, name)
            # Scalar4: xyz + uint32 bits in w, one wait, whole rows
            pos4 = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            f.read_chunk_device(0, "t/f32x3", out=pos4, columns=(0, 3), rows=plan, wait=False)
            f.read_chunk_device(0, "t/u32", out=pos4, columns=(3, 4), bitcast=True, rows=plan, wait=False)
            f.wait_read()
            want = np.concatenate([host["t/f32x3"][r], host["t/u32"][r].view(np.float32)[:, None]], 1)
            assert _same(pos4, want), what
            # Scalar4 with a fill
            vel4 = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            f.read_chunk_device(0, "t/f32x3", out=vel4, columns=(0, 3), rows=plan, fill=1.0)
            assert _same(vel4, np.concatenate([host["t/f32x3"][r], np.ones((n, 1), np.float32)], 1)), what
            # the same plan through the whole-chunk route gives the same rows
            whole = f.plan_rows(d_rows, N, threshold=-1.0)
            assert not whole.sparse
            assert _same(f.read_chunk_device(0, "t/i32x3", rows=whole), host["t/i32x3"][r]), what


def test_the_sparse_route_reads_only_the_touched_runs(tmp_path, monkeypatch):
    _block_rows(monkeypatch, 4096)
    N, R = 2_000_000, 4096
    path = str(tmp_path / "big.gsd")
    rng = np.random.default_rng(5)
    pos = rng.standard_normal((N, 3)).astype(np.float32)
    tid = rng.integers(0, 9, size=(N, 1)).astype(np.uint32)
    with fl.open(path, 'w', application="tracks", schema="raw", schema_version=[1, 0]) as f:
        f.write_chunk("t/pos", pos)
        f.write_chunk("t/tid", tid)
        f.end_frame()
    starts = np.array([100, 4090, 700_000, 1_234_567, N - 10])              # the second straddles a block edge
    rows = (starts[:, None] + np.arange(10)[None, :]).reshape(-1)
    rows = rng.permutation(rows)
    model = fl.row_plan_model(rows.astype(np.uint32), N, R)
    assert len(model.blocks) <= 10 and len(model.blocks) < (N + R - 1) // R == 489
    run_rows = sum(min((int(a) + int(c)) * R, N) - int(a) * R for a, c in model.runs)
    assert run_rows == model.staged_rows
    with fl.open(path, 'r') as f:
        plan = f.plan_rows(_dev(rows), N)
        assert plan.sparse and plan.touched_blocks == len(model.blocks)
        f.device_read_stats(reset=True)
        got = f.read_chunk_device(0, "t/pos", rows=plan)
        st = f.device_read_stats(reset=True)
        assert _same(got, pos[rows])
        assert st["pread_bytes"] == run_rows * 12, st
        assert st["h2d_bytes"] in (0, run_rows * 12), st       # (0: the small-read road copies nothing)
        got = f.read_chunk_device(0, "t/tid", rows=plan)
        st = f.device_read_stats(reset=True)
        assert _same(got, tid[rows, 0])
        assert st["pread_bytes"] == run_rows * 4, st
        # a list that touches every block: above any threshold below 1, the whole chunk is read (and at 1.0 the
        # touched runs ARE the chunk)
        spread = np.arange(0, N, R)
        wide = f.plan_rows(_dev(spread), N)
        assert wide.touched_fraction == 1.0
        got = f.read_chunk_device(0, "t/pos", rows=wide)
        st = f.device_read_stats(reset=True)
        assert _same(got, pos[spread])
        assert st["pread_bytes"] == N * 12, st
        # ... and a plain tensor does what it did: the whole chunk
        got = f.read_chunk_device(0, "t/pos", rows=_dev(rows))
        assert _same(got, pos[rows])
        assert f.device_read_stats()["pread_bytes"] == N * 12


def test_an_entry_outside_the_chunk_is_refused_and_nothing_else_is_touched(raw_file, monkeypatch):
    path, _ = raw_file
    N = 100_003
    _block_rows(monkeypatch, 64)
    r = np.array([5, 70_000, N, 64, 0xFFFFFFFF, 99_999, N + 63])
    bad = r >= N
    with fl.open(path, 'r') as f:
        host = f.read_chunk(0, "t/f32x3")
        plan = f.plan_rows(_dev(r), N, threshold=1.0)
        canary = np.float32(-7777.0)
        buf = torch.full((64 + len(r) + 64, 3), float(canary), dtype=torch.float32, device="cuda")
        out = buf[64:64 + len(r)]
        f.read_chunk_device(0, "t/f32x3", out=out, rows=plan, wait=False)
        with pytest.raises(RuntimeError, match="Invalid pgsd argument"):
            f.wait_read()
        got = buf.cpu().numpy()
        assert (got[:64] == canary).all() and (got[64 + len(r):] == canary).all()
        assert got[64:64 + len(r)][~bad].tobytes() == host[r[~bad]].tobytes()
        assert (got[64:64 + len(r)][bad] == canary).all()
        # the pipeline is fine afterwards
        ok = f.plan_rows(_dev(r[~bad]), N, threshold=1.0)
        assert _same(f.read_chunk_device(0, "t/f32x3", rows=ok), host[r[~bad]])


def test_a_plan_for_one_n_is_refused_on_a_chunk_of_another(raw_file):
    with fl.open(raw_file[0], 'r') as f:
        plan = f.plan_rows(_dev([1, 2, 3]), 100_003)
        with pytest.raises(ValueError, match="rows"):
            f.read_chunk_device(0, "t/other", rows=plan)
        small = f.plan_rows(_dev([1, 2, 3]), 5000, threshold=1.0)
        assert f.read_chunk_device(0, "t/other", rows=small).shape == (3, 3)
        with pytest.raises(ValueError):
            f.read_chunk_device(0, "t/f32x3", rows=small)


def test_read_tracks_device_equals_read_tracks(tmp_gsd, monkeypatch):
    _block_rows(monkeypatch, 64)
    keep = []

    def to_device(v):
        if v.dtype == np.uint32:        # type ids travel as the bits of a float (HOOMD's Scalar4 w), as in the suite
            t = torch.from_numpy(v.view(np.float32).copy()).cuda()
            keep.append(t)
            return fl.DeviceField.from_tensor(t, out_dtype=np.uint32, bitcast=True)
        t = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        keep.append(t)
        return t

    M.write_track_trajectory(tmp_gsd, to_device=to_device)
    rows = np.array([3, 499, 0, 3, 250, 17])
    with hoomd.open(tmp_gsd, 'r') as traj:
        host = traj.read_tracks(rows, fields=M.TRACK_FIELDS)
        M.check_tracks_against_frames(traj, host, rows, list(range(6)), M.TRACK_FIELDS)
        for given in (rows, _dev(rows), list(rows)):
            dev = traj.read_tracks_device(given, fields=M.TRACK_FIELDS)
            assert np.array_equal(dev.step, host.step) and dev.step.dtype == np.uint64
            assert np.array_equal(dev.rows.cpu().numpy(), rows)
            for name in M.TRACK_FIELDS:
                assert dev[name].is_cuda and tuple(dev[name].shape) == host[name].shape
                assert _same(dev[name], host[name]), name
            assert sorted(dev.plans) == [500, 700]              # one plan per distinct N
        sub = traj.read_tracks_device(rows, frames=slice(1, 6, 2), fields=('velocity', 'mass'))
        ref = traj.read_tracks(rows, frames=slice(1, 6, 2), fields=('velocity', 'mass'))
        assert np.array_equal(sub.step, ref.step)
        assert _same(sub.velocity, ref.velocity) and _same(sub.mass, ref.mass)
        with pytest.raises(IndexError, match="frame 4"):
            traj.read_tracks_device([1, 500])
        assert traj.read_tracks_device([699], frames=[0, 5]).position.shape == (2, 1, 3)


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
import test_tracks_model as M
rows = np.array([3, 499, 0, 3, 250, 17])
with hoomd.open(path, 'r') as t:
    tr = t.read_tracks_device(rows, fields=M.TRACK_FIELDS)
    assert isinstance(tr.rows, fl.DeviceBuffer) and all(isinstance(tr[n], fl.DeviceBuffer) for n in M.TRACK_FIELDS)
    plan = t.file.plan_rows(tr.rows, 700)
    res = dict(step=tr.step, rows=tr.rows.to_host(), blocks=plan.blocks(), rows2=plan.rows2.to_host(),
               R=plan.block_rows, fields={n: tr[n].to_host() for n in M.TRACK_FIELDS})
pickle.dump(res, open(out_path, "wb"))
'''


def test_read_tracks_device_without_torch(tmp_gsd, tmp_path):
    M.write_track_trajectory(tmp_gsd)
    script, out = tmp_path / "child.py", tmp_path / "res.pkl"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, tmp_gsd, str(out)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = pickle.load(open(out, "rb"))
    rows = np.array([3, 499, 0, 3, 250, 17])
    with hoomd.open(tmp_gsd, 'r') as traj:
        host = traj.read_tracks(rows, fields=M.TRACK_FIELDS)
    assert np.array_equal(res["step"], host.step) and np.array_equal(res["rows"], rows)
    for name in M.TRACK_FIELDS:
        assert res["fields"][name].dtype == host[name].dtype and res["fields"][name].shape == host[name].shape
        assert res["fields"][name].tobytes() == host[name].tobytes(), name
    model = fl.row_plan_model(rows.astype(np.uint32), 700, res["R"])
    np.testing.assert_array_equal(res["blocks"], model.blocks)
    np.testing.assert_array_equal(res["rows2"], model.rows2)


def test_domain_read_of_an_x_sorted_file_reads_fewer_bytes(tmp_gsd, monkeypatch):
    _block_rows(monkeypatch, 4096)
    N, R = 300_000, 4096
    rng = np.random.default_rng(11)
    box = np.array([8.0, 4.0, 4.0, 0.0, 0.0, 0.0], np.float32)
    pos = (rng.uniform(-0.5, 0.5, size=(N, 3)) * box[:3]).astype(np.float32)
    pos = pos[np.argsort(pos[:, 0], kind="stable")]                      # file rows sorted along x
    fr = hoomd.Frame()
    fr.configuration.step = 1
    fr.configuration.box = box
    fr.particles.N = N
    fr.particles.types = ['A', 'B']
    fr.particles.position = pos
    fr.particles.typeid = rng.integers(0, 2, size=N).astype(np.uint32)
    fr.particles.velocity = rng.standard_normal((N, 3)).astype(np.float32)
    fr.particles.image = rng.integers(-3, 4, size=(N, 3)).astype(np.int32)
    fr.particles.density = rng.standard_normal(N).astype(np.float32)
    with hoomd.open(tmp_gsd, 'w') as t:
        t.append(fr)
    stored = {'typeid': 4, 'velocity': 12, 'image': 12, 'density': 4}   # bytes per row of the chunks after the position
    with hoomd.open(tmp_gsd, 'r') as t:
        host = t[0]
        for d in hoomd.domain_grid(4, 1, 1)[1:3]:
            rows = hoomd.domain_rows(host.particles.position, box, d)
            model = fl.row_plan_model(rows.astype(np.uint32), N, R)
            assert 0 < len(rows) < N and len(model.blocks) * R <= 0.5 * N
            t.file.device_read_stats(reset=True)
            s = t.read_frame_device(0, domain=d)
            st = t.file.device_read_stats(reset=True)
            assert np.array_equal(s.tag.cpu().numpy(), rows)
            for name in ('position',) + tuple(stored):
                assert _same(getattr(s.particles, name), getattr(host.particles, name)[rows]), name
            assert _same(s.particles.mass, np.ones(len(rows), np.float32))
            whole = N * (12 + sum(stored.values()))
            assert st["pread_bytes"] == N * 12 + model.staged_rows * sum(stored.values()), st
            assert st["pread_bytes"] < whole
