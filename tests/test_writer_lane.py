"""The warm-then-write pair of the writer lane (`pgsd_io.cpp`) on the CPU: `drivers/writer_lane_check.cpp`, a program
of its own that drives the pair with host buffers, built under ThreadSanitizer and under AddressSanitizer + UBSan and
run as a plain executable -- 64 sub-pieces per piece into a file checked by content, and the same into /dev/full."""
import os
import subprocess

import pytest

import product

CSRC = os.path.join(product.ROOT, "pgsd-sph_amd", "csrc")
SOURCES = [os.path.join(product.TESTS, "drivers", "writer_lane_check.cpp"), os.path.join(CSRC, "pgsd_io.cpp"),
           os.path.join(CSRC, "pgsd_comm.cpp")]


@pytest.fixture(scope="module", params=["thread", "address,undefined"])
def lane_check(request):
    os.makedirs(product.TBUILD, exist_ok=True)
    out = os.path.join(product.TBUILD, "writer_lane_check_" + request.param.split(",")[0])
    tmp = "%s.%d.tmp" % (out, os.getpid())
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=" + request.param, "-fno-omit-frame-pointer",
                        "-I" + os.path.join(product.ROOT, "include"), "-I" + CSRC, "-pthread"] + SOURCES
                       + ["-o", tmp, "-lrt", "-ldl"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    os.replace(tmp, out)   # (workers of a distributed run build the same program: each its own file, then one rename)
    return out


def _run(args):
    r = subprocess.run(args, capture_output=True, timeout=60)   # a lane that waits for a ticket that cannot come ends here
    text = r.stdout.decode() + r.stderr.decode()
    assert r.returncode == 0 and r.stdout.decode().strip().endswith("ok"), text[-3000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-3000:]


def test_sub_pieces_reach_the_file_in_submission_order(lane_check, tmp_path):
    _run([lane_check, "file", str(tmp_path / "lane.bin")])


def test_a_full_device_fails_every_piece_once_and_the_lane_shuts_down(lane_check):
    _run([lane_check, "full"])
