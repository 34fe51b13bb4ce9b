"""The side lane of the device writer (`PGSD_WRITE_SIDE`, `PGSD_WRITE_SIDE_BLOCK_KIB`; `pgsd_io.cpp`): page insertions
through a shared mapping of a tmpfs file beside the warm-then-write pair.  Whatever the setting -- off, one or three side
threads, a block that is no divisor of the slab or larger than it, the pair off (which means the side lane off), a
populate call that reports failure -- the file is the oracle's byte for byte.  The knobs are read when a pipeline is
made, so every setting runs in a child process of its own (the unchanged `writer_lane_worker.py`), four at a time, and
writes into a directory on /dev/shm: the side lane takes no other file system."""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import scenario as S
import writer_lane_worker as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMPFS_MAGIC = 0x01021994
OFF_MESSAGE = "the side lane of the writer is off from here on"
# 4 KiB sub-pieces: a 1 MiB slab piece is 256 turns of the pair, during which the side threads claim from its back
SIDE = {"PGSD_WRITE_WARM": "1", "PGSD_WRITE_SUBPIECE_KIB": "4"}
VARIANTS = {
    "off": {"PGSD_WRITE_SIDE": "0"},
    "one4": dict(SIDE, PGSD_WRITE_SIDE="1", PGSD_WRITE_SIDE_BLOCK_KIB="4"),
    "three4": dict(SIDE, PGSD_WRITE_SIDE="3", PGSD_WRITE_SIDE_BLOCK_KIB="4"),
    "block60": dict(SIDE, PGSD_WRITE_SIDE="3", PGSD_WRITE_SIDE_BLOCK_KIB="60"),        # no divisor of the 1 MiB slab
    "block4096": dict(SIDE, PGSD_WRITE_SIDE="3", PGSD_WRITE_SIDE_BLOCK_KIB="4096"),    # larger than the slab
    "pair_off": {"PGSD_WRITE_WARM": "0", "PGSD_WRITE_SIDE": "3", "PGSD_WRITE_SIDE_BLOCK_KIB": "4"},   # must mean off
    "fail_first": dict(SIDE, PGSD_WRITE_SIDE="3", PGSD_WRITE_SIDE_BLOCK_KIB="4", PGSD_WRITE_SIDE_FAIL_AT="0"),
    "fail_mid": dict(SIDE, PGSD_WRITE_SIDE="3", PGSD_WRITE_SIDE_BLOCK_KIB="4", PGSD_WRITE_SIDE_FAIL_AT="37"),
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


def _tmpfs_top():
    class StatFs(ctypes.Structure):
        _fields_ = [("f_type", ctypes.c_long), ("rest", ctypes.c_long * 31)]
    fs = StatFs()
    libc = ctypes.CDLL(None, use_errno=True)
    if not os.access("/dev/shm", os.W_OK) or libc.statfs(b"/dev/shm", ctypes.byref(fs)) != 0 or fs.f_type != TMPFS_MAGIC:
        pytest.skip("/dev/shm is no writable tmpfs")
    return tempfile.mkdtemp(prefix="pgsd_side_lane_", dir="/dev/shm")


@pytest.fixture(scope="module")
def written():
    """the bytes of every child's files and what it printed, and the oracle's files for the same frames"""
    top = _tmpfs_top()
    try:
        files, said = {}, {}
        tags = list(VARIANTS)
        for batch in (tags[:4], tags[4:]):
            children = {}
            for tag in batch:
                os.mkdir(os.path.join(top, tag))
                children[tag] = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "writer_lane_worker.py"), ROOT,
                                                  os.path.join(top, tag)], env=dict(os.environ, **VARIANTS[tag]),
                                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            for tag, child in children.items():
                text, _ = child.communicate(timeout=300)
                print(tag, text.strip().replace("\n", " | "))
                assert child.returncode == 0 and text.strip().endswith("ok"), tag + ": " + text[-3000:]
                said[tag] = text
                for name in ("sync", "async", "extra"):
                    with open(os.path.join(top, tag, name + ".gsd"), "rb") as f:
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
        return files, said, _oracle(os.path.join(top, "oracle.gsd"), frames), _oracle(os.path.join(top, "oracle_extra.gsd"), extra)
    finally:
        shutil.rmtree(top, ignore_errors=True)


@pytest.mark.parametrize("seal", ["sync", "async"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_side_lane_setting_writes_the_oracles_file(written, variant, seal):
    files, _, oracle, _ = written
    assert len(oracle) > W.FRAMES * W.N * 28
    assert files[variant, seal] == oracle


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_one_slab_plus_one_row_and_a_chunk_without_rows(written, variant):
    """a chunk of exactly one slab plus one row (its second piece is 16 bytes) and a chunk of no rows"""
    files, _, _, oracle_extra = written
    assert W.N_EXTRA * 16 == W.SLAB + 16
    assert files[variant, "extra"] == oracle_extra


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_side_lane_goes_off_after_a_failed_populate_and_only_then(written, variant):
    """the lane says so once per pipeline when it switches itself off (the worker makes three pipelines; how many
    populate calls the side threads of each get to make is a matter of timing).  That the message is there also says that
    the side threads did populate: the failing call is the first, or the 38th."""
    _, said, _, _ = written
    if variant.startswith("fail"):
        assert 1 <= said[variant].count(OFF_MESSAGE) <= 3, said[variant]
    else:
        assert OFF_MESSAGE not in said[variant], said[variant]


def _one_frame_stats(top, name):
    import torch
    import pgsd.fl as fl
    f = fl.open(os.path.join(top, name), "w", application="app", schema="hoomd", schema_version=[1, 4])
    pos = torch.randn((2_000_003, 4), device="cuda")
    f.write_chunks([("particles/position", fl.DeviceField.from_tensor(pos, columns=(0, 3)))], offset=np.array([pos.shape[0]]))
    f.end_frame()
    stats = f.device_stats()
    f.close()
    print(stats)
    assert stats["written_bytes"] >= pos.shape[0] * 12
    return stats


def test_a_pipeline_on_tmpfs_reports_the_side_lane_and_its_bytes():
    """in this process, with the default knobs: the statistics say that the side lane is on, and part of the 24 MB of
    the frame -- pieces of 1, 4 and 16 MiB -- went through it"""
    top = _tmpfs_top()
    try:
        stats = _one_frame_stats(top, "stats.gsd")
        assert stats["side_on"] == 1
        assert 0 < stats["side_bytes"] < stats["written_bytes"] and stats["side_ms"] > 0
    finally:
        shutil.rmtree(top, ignore_errors=True)


def test_without_the_pair_there_is_no_side_lane(monkeypatch):
    """the knobs are read when the pipeline is made: PGSD_WRITE_WARM=0 with three side threads asked for means off"""
    monkeypatch.setenv("PGSD_WRITE_WARM", "0")
    monkeypatch.setenv("PGSD_WRITE_SIDE", "3")
    top = _tmpfs_top()
    try:
        stats = _one_frame_stats(top, "pair_off.gsd")
        assert stats["side_on"] == 0 and stats["side_bytes"] == 0 and stats["side_ms"] == 0
    finally:
        shutil.rmtree(top, ignore_errors=True)
