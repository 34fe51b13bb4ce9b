"""What pgsd.fl's sph_accelerations_device refuses on the Python side, before the library is called: the full text of
every message.  All of them are raised before the row lists are looked at, so no GPU memory -- and no GPU -- is needed;
the library's own refusals are held by tests/test_gpu_sph_forces.py."""
import numpy as np
import pytest

import pgsd.fl as fl
import pgsd.hoomd as hoomd

N = 8
BOX = [8, 8, 8, 0, 0, 0]
METHOD = 'sph_accelerations_device'


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    """Two frames of 8 particles with position, velocity, mass, density and pressure, written on the host path."""
    name = str(tmp_path_factory.mktemp("force_arguments") / "eight.gsd")
    rng = np.random.default_rng(N)
    with hoomd.open(name, 'w') as t:
        for step in range(2):
            fr = hoomd.Frame()
            fr.configuration.step = step
            fr.configuration.box = BOX
            fr.particles.N = N
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


def force_call(f):
    """The method on frame 1's position chunk with good arguments up to the row lists, which are not reached."""
    def call(box=BOX, cells=(4, 4, 4), **kw):
        return f.sph_accelerations_device(1, 'particles/position', box, 0.5, cells=cells, rows=None, cell=None, **kw)
    return call


def test_the_method_refuses_its_box_its_cells_and_its_kernel(path):
    with fl.open(path, 'r') as f:
        call = force_call(f)
        assert refusal(call, box=[8, 8, 8, 0, 0]) == "box must hold 6 values"
        assert refusal(call, cells=(4, 4)) == METHOD + ": cells holds three counts, each 1 to 1024"
        assert refusal(call, cells=(4, -1, 4)) == METHOD + ": cells holds three counts, each 1 to 1024"
        assert refusal(call, kernel='gauss') == METHOD + ": the kernel is one of wendland_c2, cubic_spline: 'gauss'"
        # a call that is wrong twice is refused for its cells, which are looked at first
        assert refusal(call, cells=(4, 4), kernel='gauss') == METHOD + ": cells holds three counts, each 1 to 1024"


def test_the_method_refuses_its_defaults(path):
    with fl.open(path, 'r') as f:
        call = force_call(f)
        for defaults in ((1.0,), (1.0, 1000.0), (1.0, 1000.0, 0.0, 0.0)):
            assert refusal(call, defaults=defaults) == METHOD + ": defaults holds a mass, a density and a pressure"
        # ... and with its optional chunks given (of either frame) for the same thing
        assert refusal(call, mass=(1, 'particles/mass'), density=(0, 'particles/density'), pressure=(1, 'particles/pressure'),
                       velocity=(1, 'particles/velocity'), defaults=(1.0,)) \
            == METHOD + ": defaults holds a mass, a density and a pressure"


def test_the_method_refuses_its_viscosity_and_its_gravity(path):
    with fl.open(path, 'r') as f:
        call = force_call(f)
        for mu in (-0.5, float('inf'), float('nan')):
            assert refusal(call, viscosity=mu) == METHOD + ": viscosity is a finite number, at least 0, or None: %r" % mu
        for g in ((0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, float('nan'), 0.0), (float('-inf'), 0.0, 0.0)):
            assert refusal(call, gravity=g) == METHOD + ": gravity holds three finite numbers, or is None"
        # the viscosity is looked at before the gravity, the defaults before both
        assert refusal(call, viscosity=-1, gravity=(0, 0)) == METHOD + ": viscosity is a finite number, at least 0, or None: -1"
        assert refusal(call, defaults=(1.0,), viscosity=-1) == METHOD + ": defaults holds a mass, a density and a pressure"
        # good arguments reach the row lists, which are no GPU memory here
        with pytest.raises((ValueError, AttributeError, TypeError)) as caught:
            call(viscosity=0.5, gravity=(0, 0, -9.81))
        assert "viscosity" not in str(caught.value) and "gravity" not in str(caught.value)
