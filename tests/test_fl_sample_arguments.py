"""What pgsd.fl's sph_samples_device refuses on the Python side, before the library is called: the full text of every
message.  All of them are raised before the row lists are looked at and before the points are uploaded, so no GPU memory
-- and no GPU -- is needed; the library's own refusals are held by tests/test_gpu_sph_samples.py."""
import numpy as np
import pytest

import pgsd.fl as fl
import pgsd.hoomd as hoomd

N = 8
BOX = [8, 8, 8, 0, 0, 0]
METHOD = 'sph_samples_device'
POINTS = np.zeros((3, 3))


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    """Two frames of 8 particles with position, velocity, mass, density, pressure and orientation, written on the host
    path."""
    name = str(tmp_path_factory.mktemp("sample_arguments") / "eight.gsd")
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
            fr.particles.orientation = rng.standard_normal((N, 4)).astype(np.float32)
            fr.log['wide'] = rng.standard_normal((N, 5)).astype(np.float32)
            t.append(fr)
    return name


def refusal(call, **kw):
    with pytest.raises(ValueError) as caught:
        call(**kw)
    return str(caught.value)


def sample_call(f):
    """The method on frame 1's position chunk with good arguments up to the row lists, which are not reached."""
    def call(box=BOX, cells=(4, 4, 4), points=POINTS, **kw):
        return f.sph_samples_device(1, 'particles/position', box, 0.5, cells, None, None, points, **kw)
    return call


def test_the_method_refuses_its_box_its_cells_its_kernel_and_its_defaults(path):
    with fl.open(path, 'r') as f:
        call = sample_call(f)
        assert refusal(call, box=[8, 8, 8, 0, 0]) == "box must hold 6 values"
        assert refusal(call, cells=(4, 4)) == METHOD + ": cells holds three counts, each 1 to 1024"
        assert refusal(call, cells=(4, -1, 4)) == METHOD + ": cells holds three counts, each 1 to 1024"
        assert refusal(call, kernel='gauss') == METHOD + ": the kernel is one of wendland_c2, cubic_spline: 'gauss'"
        # a call that is wrong twice is refused for its cells, which are looked at first
        assert refusal(call, cells=(4, 4), kernel='gauss') == METHOD + ": cells holds three counts, each 1 to 1024"
        for defaults in ((1.0,), (1.0, 1000.0, 0.0)):
            assert refusal(call, defaults=defaults) == METHOD + ": defaults holds a mass and a density"
        assert refusal(call, mass=(1, 'particles/mass'), density=(0, 'particles/density'), defaults=(1.0,)) \
            == METHOD + ": defaults holds a mass and a density"


def test_the_method_refuses_its_values(path):
    shape = METHOD + ": value %d is (frame, name) of a stored chunk or (chunk or None, columns, default)"
    with fl.open(path, 'r') as f:
        call = sample_call(f)
        velocity, pressure = (1, 'particles/velocity'), (0, 'particles/pressure')
        assert refusal(call, values=[velocity] * 5) == METHOD + ": values holds at most 4 chunks: 5"
        for bad in ('particles/velocity', (1,), (velocity, 3), (1, 'particles/velocity', 0.0), (None, 'three', 0.0), 7):
            assert refusal(call, values=[pressure, bad]) == shape % 1
        assert refusal(call, values=[(velocity, 5, 0.0)]) == METHOD + ": value 0 has 1 to 4 columns: 5"
        assert refusal(call, values=[velocity, (None, 0, 0.0)]) == METHOD + ": value 1 has 1 to 4 columns: 0"
        assert refusal(call, values=[(None, 3, float('nan'))]) == METHOD + ": value 0 is stored nowhere and its default is no number"
        assert refusal(call, values=[(None, 3, 0.0)] * 3) == METHOD + ": the values hold at most 8 columns together: 9"
        # the width of a stored chunk given by its name alone is its own
        assert refusal(call, values=[(1, 'log/wide')]) == METHOD + ": value 0 has 1 to 4 columns: 5"
        orientation = (1, 'particles/orientation')
        assert refusal(call, values=[orientation, orientation, velocity]) == METHOD + ": the values hold at most 8 columns together: 11"
        with pytest.raises(KeyError):
            call(values=[(1, 'particles/nothing')])
        # the defaults are looked at before the values
        assert refusal(call, defaults=(1.0,), values=[velocity] * 5) == METHOD + ": defaults holds a mass and a density"


def test_the_method_refuses_its_points(path):
    bad = METHOD + ": points holds K x 3 float32 or float64 values (numpy) or K x 3 float64 values in GPU memory"
    with fl.open(path, 'r') as f:
        call = sample_call(f)
        for points in (np.zeros((3, 2)), np.zeros(6), np.zeros((3, 3), np.int64), np.zeros((2, 3, 1)), None, "points",
                       [[0, 0, 0]]):
            assert refusal(call, points=points) == bad
        # the values are looked at before the points
        assert refusal(call, points=None, values=[(None, 3, 0.0)] * 3) == METHOD + ": the values hold at most 8 columns together: 9"
        # good arguments reach the row lists, which are no GPU memory here: nothing was uploaded for them
        with pytest.raises((ValueError, AttributeError, TypeError)) as caught:
            call(values=[(1, 'particles/velocity'), (None, 1, 2.5)], normalise=True, points=POINTS.astype(np.float32))
        assert "points" not in str(caught.value) and "value" not in str(caught.value)
