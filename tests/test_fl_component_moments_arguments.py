"""What pgsd.fl's component_moments_device refuses on the Python side, before the library is called: the full text of every
message.  All of them are raised before the lists are looked at, so no GPU memory -- and no GPU -- is needed; the library's
own refusals are held by tests/test_gpu_component_moments.py.  Beside them: what the entry point itself answers without a
GPU, and the PGSD_ERROR_NO_DEVICE twin of the pipeline call in the device stub, through a small stand-alone program."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import product
import pgsd.fl as fl
import pgsd.hoomd as hoomd
from pgsd import _lib

N = 8
BOX = [8, 8, 8, 0, 0, 0]
METHOD = 'component_moments_device'
FIELDS = ('mass', 'velocity', 'energy', 'position')


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    name = str(tmp_path_factory.mktemp("component_moments_arguments") / "eight.gsd")
    rng = np.random.default_rng(N)
    with hoomd.open(name, 'w') as t:
        fr = hoomd.Frame()
        fr.configuration.box = BOX
        fr.particles.N = N
        fr.particles.position = rng.uniform(-4, 4, size=(N, 3)).astype(np.float32)
        fr.particles.velocity = rng.standard_normal((N, 3)).astype(np.float32)
        fr.particles.mass = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
        fr.particles.energy = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
        t.append(fr)
    return name


def refusal(call, **kw):
    with pytest.raises(ValueError) as caught:
        call(**kw)
    return str(caught.value)


def test_the_method_refuses_its_chunks_its_defaults_and_its_box(path):
    chunks = [(0, 'particles/' + name) for name in FIELDS]
    with fl.open(path, 'r') as f:
        def call(chunks=chunks, box=BOX, **kw):
            return f.component_moments_device(chunks, box, None, None, None, N, 1, **kw)

        assert refusal(call, chunks=chunks[:3]) == METHOD + ": chunks holds mass, velocity, energy, position (or None)"
        assert refusal(call, chunks=chunks + [None]) == METHOD + ": chunks holds mass, velocity, energy, position (or None)"
        for defaults in ((1.0,), tuple(range(7)), tuple(range(9))):
            assert refusal(call, defaults=defaults) == METHOD + ": defaults holds mass, v[3], energy, x[3]"
        assert refusal(call, box=[8, 8, 8, 0, 0]) == "box must hold 6 values"
        # the chunks are looked at first, then the defaults, then the box
        assert refusal(call, chunks=chunks[:3], defaults=(1.0,)).endswith("position (or None)")
        assert refusal(call, defaults=(1.0,), box=[8]).endswith("x[3]")
        with pytest.raises(Exception, match="particles/nothing|not found|no chunk"):
            call(chunks=chunks[:3] + [(0, 'particles/nothing')])
        # good arguments reach the row lists, which are no GPU memory here
        with pytest.raises((ValueError, AttributeError, TypeError)) as caught:
            call()
        assert "chunks holds" not in str(caught.value) and "defaults" not in str(caught.value)


def test_the_entry_point_checks_its_arguments_before_it_needs_a_gpu(path):
    """Null pointers and the arguments the entry point refuses itself need no device; what passes them ends at the
    pipeline, which answers PGSD_ERROR_NO_DEVICE on a box without a GPU."""
    fn = _lib.lib.pgsd_component_moments_device
    E, D = ctypes.POINTER(_lib.IndexEntry), ctypes.POINTER(ctypes.c_double)
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.POINTER(_lib.Handle), E, E, E, E, D, D, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    with fl.open(path, 'r') as f:
        h = f._h()
        entries = [_lib.IndexEntry.from_buffer_copy(_lib.lib.pgsd_find_chunk(h, 0, ('particles/' + name).encode()).contents)
                   for name in FIELDS]
        defaults, vectors = (ctypes.c_double * 8)(1, 0, 0, 0, 0, 0, 0, 0), (ctypes.c_double * 6)(8, 8, 8, 0, 0, 0)
        summary = (ctypes.c_uint64 * 6)(*([77] * 6))
        fake = ctypes.c_void_p(0x1000)          # never dereferenced on the host

        def call(n=N, components=1, flags=0, dimensions=3, position=True, vec=vectors, lists=fake, out=fake, out_summary=summary):
            given = [ctypes.byref(e) for e in entries]
            if not position:
                given[3] = None
            return fn(h, *given, defaults, vec, dimensions, lists, lists, lists, n, components, flags, out, out, out, out,
                      out_summary)

        INVALID = _lib.ERROR_INVALID_ARGUMENT
        assert call(out_summary=None) == INVALID and call(lists=None) == INVALID and call(out=None) == INVALID
        for kw, message in ((dict(position=False), "the position is stored nowhere"), (dict(dimensions=4), "dimensions is 2 or 3"),
                            (dict(vec=(ctypes.c_double * 6)(8, float('nan'), 8, 0, 0, 0)), "the box vectors are finite"),
                            (dict(vec=(ctypes.c_double * 6)(8, 0, 8, 0, 0, 0)), "the box lengths are positive"),
                            (dict(flags=1), "flags holds undefined bits"), (dict(n=1 << 32), "fewer than 2^32 entries"),
                            (dict(components=N + 1), "1 to n components"), (dict(components=0), "1 to n components"),
                            (dict(n=0, components=1), "1 to n components")):
            assert call(**kw) == INVALID, kw
            assert _lib.last_error().startswith("pgsd_component_moments_device: ") and message in _lib.last_error(), kw
            assert list(summary) == [77] * 6
        if _lib.lib.pgsd_device_available():
            # no entry: six zeros, without a list and without an output
            assert call(n=0, components=0, lists=None, out=None) == 0 and list(summary) == [0] * 6
        else:
            # the chunks' ranges are the pipeline's to give: whatever passes the checks above ends there
            assert call() == _lib.ERROR_NO_DEVICE and call(n=0, components=0) == _lib.ERROR_NO_DEVICE
            assert list(summary) == [77] * 6


PROGRAM = r'''
#include "pgsd_internal.hpp"
int main()
    {
    pgsd_amd::ComponentMomentsArgs a{};
    std::string err;
    const int rc = pgsd_amd::device_pipeline_component_moments(nullptr, nullptr, a, nullptr, nullptr, nullptr, nullptr, nullptr, &err);
    return rc == PGSD_ERROR_NO_DEVICE ? 0 : 1;
    }
'''


def test_the_device_stub_answers_no_device(tmp_path):
    """The host-only builds link pgsd_device_stub.cpp in place of the pipeline: its twin of the new call exists (the
    program links) and answers PGSD_ERROR_NO_DEVICE."""
    csrc = os.path.join(product.ROOT, "pgsd-sph_amd", "csrc")
    source, program = str(tmp_path / "stub_main.cpp"), str(tmp_path / "stub_main")
    with open(source, "w") as fh:
        fh.write(PROGRAM)
    build = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-I" + os.path.join(product.ROOT, "include"), "-I" + csrc,
                            source, os.path.join(csrc, "pgsd_device_stub.cpp"), "-o", program], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    assert subprocess.run([program]).returncode == 0


def test_the_private_entry_point_is_declared_and_the_public_abi_is_unchanged():
    private = open(os.path.join(product.ROOT, "pgsd-sph_amd", "csrc", "pgsd_private.h")).read()
    public = open(os.path.join(product.ROOT, "include", "pgsd.h")).read()
    pxd = open(os.path.join(product.ROOT, "pgsd-sph_amd", "pgsd", "libpgsd_amd.pxd")).read()
    assert "int pgsd_component_moments_device(" in private and "int pgsd_component_moments_device(" in pxd
    assert "pgsd_component_moments_device" not in public
    assert hasattr(_lib.lib, "pgsd_component_moments_device")
