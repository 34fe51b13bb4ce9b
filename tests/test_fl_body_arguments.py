"""What pgsd.fl's sph_body_force_device refuses on the Python side, before the library is called: the full text of every
message.  All of them are raised before the row lists are looked at, so no GPU memory -- and no GPU -- is needed; the
library's own refusals are held by tests/test_gpu_sph_body.py.  The host model's refusals of `about` and of its lists
stand beside them."""
import numpy as np
import pytest

import pgsd.fl as fl
import pgsd.hoomd as hoomd

N = 8
BOX = [8, 8, 8, 0, 0, 0]
METHOD = 'sph_body_force_device'


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    """Two frames of 8 particles with position, velocity, mass, density and pressure, written on the host path."""
    name = str(tmp_path_factory.mktemp("body_arguments") / "eight.gsd")
    rng = np.random.default_rng(N)
    with hoomd.open(name, 'w') as t:
        for step in range(2):
            fr = hoomd.Frame()
            fr.configuration.step = step
            fr.configuration.box = BOX
            fr.particles.N = N
            fr.particles.types = ['fluid', 'wall']
            fr.particles.typeid = np.array([0, 0, 0, 0, 0, 1, 1, 1], np.uint32)
            fr.particles.position = rng.uniform(-4, 4, size=(N, 3)).astype(np.float32)
            fr.particles.velocity = rng.standard_normal((N, 3)).astype(np.float32)
            fr.particles.mass = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
            fr.particles.density = rng.uniform(900, 1100, size=N).astype(np.float32)
            fr.particles.pressure = rng.uniform(0.9e5, 1.1e5, size=N).astype(np.float32)
            t.append(fr)
    return name


def refusal(call, **kw):
    with pytest.raises(ValueError) as caught:
        call(**kw)
    return str(caught.value)


def body_call(f):
    """The method on frame 1's position chunk with good arguments up to the row lists, which are not reached."""
    def call(box=BOX, cells=(4, 4, 4), **kw):
        return f.sph_body_force_device(1, 'particles/position', box, 0.5, cells, None, None, None, None, **kw)
    return call


def test_the_method_refuses_its_box_its_cells_and_its_kernel(path):
    with fl.open(path, 'r') as f:
        call = body_call(f)
        assert refusal(call, box=[8, 8, 8, 0, 0]) == "box must hold 6 values"
        assert refusal(call, cells=(4, 4)) == METHOD + ": cells holds three counts, each 1 to 1024"
        assert refusal(call, cells=(4, -1, 4)) == METHOD + ": cells holds three counts, each 1 to 1024"
        assert refusal(call, kernel='gauss') == METHOD + ": the kernel is one of wendland_c2, cubic_spline: 'gauss'"
        # a call that is wrong twice is refused for its cells, which are looked at first
        assert refusal(call, cells=(4, 4), kernel='gauss') == METHOD + ": cells holds three counts, each 1 to 1024"


def test_the_method_refuses_its_defaults(path):
    with fl.open(path, 'r') as f:
        call = body_call(f)
        for defaults in ((1.0,), (1.0, 1000.0), (1.0, 1000.0, 0.0, 0.0)):
            assert refusal(call, defaults=defaults) == METHOD + ": defaults holds a mass, a density and a pressure"
        # ... and with its optional chunks given (of either frame) for the same thing
        assert refusal(call, mass=(1, 'particles/mass'), density=(0, 'particles/density'), pressure=(1, 'particles/pressure'),
                       velocity=(1, 'particles/velocity'), defaults=(1.0,)) \
            == METHOD + ": defaults holds a mass, a density and a pressure"


def test_the_method_refuses_its_viscosity_and_its_point(path):
    with fl.open(path, 'r') as f:
        call = body_call(f)
        for mu in (-0.5, float('inf'), float('nan')):
            assert refusal(call, viscosity=mu) == METHOD + ": viscosity is a finite number, at least 0, or None: %r" % mu
        for c in ((0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, float('nan'), 0.0), (float('-inf'), 0.0, 0.0)):
            assert refusal(call, about=c) == METHOD + ": about holds three finite numbers, or is None"
        # the viscosity is looked at before the point, the defaults before both
        assert refusal(call, viscosity=-1, about=(0, 0)) == METHOD + ": viscosity is a finite number, at least 0, or None: -1"
        assert refusal(call, defaults=(1.0,), viscosity=-1) == METHOD + ": defaults holds a mass, a density and a pressure"
        # good arguments reach the row lists, which are no GPU memory here
        with pytest.raises((ValueError, AttributeError, TypeError)) as caught:
            call(viscosity=0.5, about=(0, 0, -1.5))
        assert "viscosity" not in str(caught.value) and "about" not in str(caught.value)


def test_the_host_model_refuses_the_same_with_its_own_words(path):
    with hoomd.open(path, 'r') as t:
        fr = t[1]
        body, fluid = {'type': ['wall']}, {'type': ['fluid']}
        call = lambda **kw: t.frame_body_force(1, body, fluid, 0.5, **kw)  # noqa: E731
        for c in ((0.0, 0.0), (0.0, float('nan'), 0.0)):
            assert refusal(call, about=c) == "about holds three finite numbers, or is None"
        assert refusal(call, viscosity=-0.5) == "viscosity is a finite number, at least 0, or None: -0.5"
        assert refusal(lambda: t.frame_body_force(1, body, None, 0.5)) == "body and fluid are where dicts: both are required"
        assert refusal(lambda: t.frame_body_force(1, None, fluid, 0.5)) == "body and fluid are where dicts: both are required"
        p = fr.particles.position
        assert refusal(lambda: hoomd.sph_body_force(p, None, BOX, 0.5, None, [0])) \
            == "body_rows and fluid_rows are row lists: None is not accepted for either"
        assert refusal(lambda: hoomd.sph_body_force(p, None, BOX, 0.5, [0], None)) \
            == "body_rows and fluid_rows are row lists: None is not accepted for either"
        got = call(viscosity=0.5, about=(0, 0, -1.5))
        assert got.n == 3 and got.n_sources == 5 and got.about == (0.0, 0.0, -1.5)
