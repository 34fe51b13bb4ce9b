"""What pgsd.fl's sph_tensors_device refuses on the Python side, before the library is called: the full text of every
message (tests/test_fl_pass_arguments.py holds the other pass methods the same way).  All of them are raised before the
row lists are looked at, so no GPU memory -- and no GPU -- is needed; the library's own refusals, det_min among them, are
held by tests/test_gpu_sph_tensors.py."""
import numpy as np
import pytest

import pgsd.fl as fl
import pgsd.hoomd as hoomd

N = 8
BOX = [8, 8, 8, 0, 0, 0]
METHOD = 'sph_tensors_device'


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    """Two frames of 8 particles with position, velocity, mass and density, written on the host path."""
    name = str(tmp_path_factory.mktemp("pass_arguments_tensors") / "eight.gsd")
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
            t.append(fr)
    return name


def refusal(call, **kw):
    with pytest.raises(ValueError) as caught:
        call(**kw)
    return str(caught.value)


def tensors_call(f):
    """The method on frame 1's position chunk with good arguments up to the row lists, which are not reached."""
    def call(box=BOX, cells=(4, 4, 4), **kw):
        return f.sph_tensors_device(1, 'particles/position', box, cells=cells, rows=None, cell=None, h=0.5, **kw)
    return call


def test_the_method_exists_with_its_defaults():
    import inspect
    names = list(inspect.signature(fl.PGSDFile.sph_tensors_device).parameters)
    assert names[1:8] == ['frame', 'name', 'box', 'h', 'cells', 'rows', 'cell']
    assert names[8:] == ['n', 'velocity', 'mass', 'density', 'defaults', 'dimensions', 'kernel', 'det_min', 'return_rows']


def test_it_refuses_its_box_and_its_cells(path):
    with fl.open(path, 'r') as f:
        call = tensors_call(f)
        assert refusal(call, box=[8, 8, 8, 0, 0]) == "box must hold 6 values"
        assert refusal(call, cells=(4, 4)) == METHOD + ": cells holds three counts, each 1 to 1024"
        assert refusal(call, cells=(4, -1, 4)) == METHOD + ": cells holds three counts, each 1 to 1024"


def test_it_refuses_its_kernel_and_its_defaults(path):
    with fl.open(path, 'r') as f:
        call = tensors_call(f)
        assert refusal(call, kernel='gauss') == METHOD + ": the kernel is one of wendland_c2, cubic_spline: 'gauss'"
        assert refusal(call, defaults=(1.0,)) == METHOD + ": defaults holds a mass and a density"
        assert refusal(call, defaults=(1.0, 0.0, 0.0)) == METHOD + ": defaults holds a mass and a density"
        # a call that is wrong twice is refused for its cells, which are looked at first
        assert refusal(call, cells=(4, 4), kernel='gauss') == METHOD + ": cells holds three counts, each 1 to 1024"
        # ... and with its optional chunks given (of either frame) for the same thing
        assert refusal(call, velocity=(1, 'particles/velocity'), mass=(1, 'particles/mass'), density=(0, 'particles/density'),
                       defaults=(1.0,), det_min=0.5) == METHOD + ": defaults holds a mass and a density"
        with pytest.raises(KeyError):
            call(velocity=(1, 'particles/nothing'))
