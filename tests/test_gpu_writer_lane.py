"""The device writer's lane as a warm-then-write pair (`PGSD_WRITE_WARM`, `PGSD_WRITE_SUBPIECE_KIB`): whatever the
sub-piece, and with the pair off, the file is the oracle's byte for byte.  The knobs are read when a pipeline is made, so
every setting runs in a child process of its own (`writer_lane_worker.py`); the four children run side by side."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import scenario as S
import writer_lane_worker as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {
    "off": {"PGSD_WRITE_WARM": "0"},
    "sub4": {"PGSD_WRITE_WARM": "1", "PGSD_WRITE_SUBPIECE_KIB": "4"},
    "sub60": {"PGSD_WRITE_WARM": "1", "PGSD_WRITE_SUBPIECE_KIB": "60"},         # no divisor of the 1 MiB slab
    "sub4096": {"PGSD_WRITE_WARM": "1", "PGSD_WRITE_SUBPIECE_KIB": "4096"},     # larger than the slab
}


def _oracle(path, frames):
    """frames: lists of (name, type id, M, per-particle?, array)"""
    lib = S.oracle_lib()
    rc = ctypes.c_int(0)
    h = lib.oracle_create_and_open(path.encode(), 1, b"app", b"hoomd", lib.oracle_make_version(1, 4), 1, 0, ctypes.byref(rc))
    assert rc.value == 0
    for chunks in frames:
        for name, t, M, per_particle, a in chunks:
            n = a.shape[0]
            assert S.oracle_write_chunk(lib, h, name, t, [np.ascontiguousarray(a)], M, n, M, [0], [n * M], per_particle) == 0
        assert lib.oracle_end_frame(h) == 0
    assert lib.oracle_close(h) == 0
    with open(path, "rb") as f:
        return f.read()


def _run_children(top):
    children = {}
    for tag, knobs in VARIANTS.items():
        os.mkdir(top / tag)
        children[tag] = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "writer_lane_worker.py"), ROOT, str(top / tag)],
                                         env=dict(os.environ, **knobs), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for tag, child in children.items():
        text, _ = child.communicate(timeout=300)
        print(tag, text.strip().replace("\n", " | "))
        assert child.returncode == 0 and text.strip().endswith("ok"), tag + ": " + text[-3000:]
    (top / "done").write_text("done")


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """the bytes of every child's files, and the oracle's for the same frames.  The children run once per session: the
    workers of a distributed run share them (and the GPU is never opened by four children per worker at once)"""
    import fcntl
    base = tmp_path_factory.getbasetemp()
    shared = base.parent if os.environ.get("PYTEST_XDIST_WORKER") else base
    top = shared / "writer_lane"
    with open(shared / "writer_lane.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not (top / "done").exists():
            assert not top.exists(), "an earlier worker's children failed"
            os.mkdir(top)
            _run_children(top)
    files = {}
    for tag in VARIANTS:
        for name in ("sync", "async", "extra"):
            with open(top / tag / (name + ".gsd"), "rb") as f:
                files[tag, name] = f.read()
    frames = []
    for i in range(W.FRAMES):
        step, pos, vel = W.frame(i)
        frames.append([("configuration/step", 4, 1, False, step.reshape(1, 1)),
                       ("particles/position", 9, 3, True, pos[:, :3]),
                       ("particles/typeid", 3, 1, True, pos[:, 3:].view(np.uint32)),
                       ("particles/velocity", 9, 3, True, vel[:, :3])])
    a, b = W.extra_frame()
    extra = [frames[0], [("particles/orientation", 9, 4, True, a), ("particles/position", 9, 3, True, b[:, :3]),
                         ("particles/velocity", 9, 3, True, a[:, :3]), ("particles/mass", 9, 1, True, np.zeros((0, 1), np.float32))]]
    mine = tmp_path_factory.mktemp("lane_oracle")
    return files, _oracle(str(mine / "oracle.gsd"), frames), _oracle(str(mine / "oracle_extra.gsd"), extra)


@pytest.mark.parametrize("seal", ["sync", "async"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_lane_setting_writes_the_oracles_file(written, variant, seal):
    files, oracle, _ = written
    assert len(oracle) > W.FRAMES * W.N * 28
    assert files[variant, seal] == oracle


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_one_slab_plus_one_row_and_a_chunk_without_rows(written, variant):
    """a chunk of exactly one slab plus one row (its second piece is 16 bytes) and a chunk of no rows"""
    files, _, oracle_extra = written
    assert W.N_EXTRA * 16 == W.SLAB + 16
    assert files[variant, "extra"] == oracle_extra
