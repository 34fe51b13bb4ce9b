"""The side lane of the writer lane (`pgsd_io.cpp`: page insertions through a shared mapping beside the warm-then-write
pair) on the CPU: `drivers/side_lane_check.cpp`, a program of its own that drives the lane with host buffers -- built
plainly, under ThreadSanitizer and under AddressSanitizer + UBSan, and run as a plain executable on a tmpfs directory:
every piece size and file offset at which the cut of a piece changes, checked against plain `pwrite` of the same bytes,
end-of-file watched, and the same with a populate call that reports failure (the first, and one in mid-piece)."""
import os
import shutil
import subprocess
import tempfile

import pytest

import product

CSRC = os.path.join(product.ROOT, "pgsd-sph_amd", "csrc")
SOURCES = [os.path.join(product.TESTS, "drivers", "side_lane_check.cpp"), os.path.join(CSRC, "pgsd_io.cpp"),
           os.path.join(CSRC, "pgsd_comm.cpp")]
TMPFS_MAGIC = 0x01021994


@pytest.fixture(scope="module", params=["", "thread", "address,undefined"], ids=["plain", "thread", "address"])
def side_check(request):
    os.makedirs(product.TBUILD, exist_ok=True)
    out = os.path.join(product.TBUILD, "side_lane_check_" + (request.param.split(",")[0] or "plain"))
    tmp = "%s.%d.tmp" % (out, os.getpid())
    sanitize = ["-fsanitize=" + request.param, "-fno-omit-frame-pointer"] if request.param else []
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17"] + sanitize
                       + ["-I" + os.path.join(product.ROOT, "include"), "-I" + CSRC, "-pthread"] + SOURCES
                       + ["-o", tmp, "-lrt", "-ldl"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    os.replace(tmp, out)   # (workers of a distributed run build the same program: each its own file, then one rename)
    return out


@pytest.fixture
def tmpfs_dir():
    """a directory on tmpfs: the side lane refuses every other file system"""
    import ctypes

    class StatFs(ctypes.Structure):
        _fields_ = [("f_type", ctypes.c_long), ("rest", ctypes.c_long * 31)]
    fs = StatFs()
    libc = ctypes.CDLL(None, use_errno=True)
    if not os.access("/dev/shm", os.W_OK) or libc.statfs(b"/dev/shm", ctypes.byref(fs)) != 0 or fs.f_type != TMPFS_MAGIC:
        pytest.skip("/dev/shm is no writable tmpfs")
    d = tempfile.mkdtemp(prefix="pgsd_side_lane_", dir="/dev/shm")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _run(args):
    r = subprocess.run(args, capture_output=True, timeout=120)   # a lane that waits for what cannot come ends here
    text = r.stdout.decode() + r.stderr.decode()
    assert r.returncode == 0 and r.stdout.decode().strip().endswith("ok"), text[-3000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-3000:]
    return text


def test_every_cut_of_a_piece_writes_what_plain_pwrite_writes(side_check, tmpfs_dir):
    _run([side_check, tmpfs_dir])


@pytest.mark.parametrize("k", [0, 7])
def test_a_failed_populate_gives_the_block_back_and_switches_the_side_lane_off(side_check, tmpfs_dir, k):
    assert "still on: 0" in _run([side_check, tmpfs_dir, str(k)])
