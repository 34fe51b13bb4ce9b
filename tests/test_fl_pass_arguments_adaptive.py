"""What pgsd.fl's sph_adaptive_sums_device and smoothing_range_device refuse on the Python side, before the library is
called: the full text of every message (tests/test_fl_pass_arguments.py and tests/test_fl_pass_arguments_tensors.py hold
the other pass methods the same way).  All of them are raised before the row lists are looked at, so no GPU memory -- and
no GPU -- is needed; the library's own refusals, h_max and the mode's index among them, are held by
tests/test_gpu_sph_adaptive.py."""
import inspect

import numpy as np
import pytest

import pgsd.fl as fl
import pgsd.hoomd as hoomd

N = 8
BOX = [8, 8, 8, 0, 0, 0]
METHOD = 'sph_adaptive_sums_device'


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    """Two frames of 8 particles with position, slength, mass and density, written on the host path."""
    name = str(tmp_path_factory.mktemp("pass_arguments_adaptive") / "eight.gsd")
    rng = np.random.default_rng(N)
    with hoomd.open(name, 'w') as t:
        for step in range(2):
            fr = hoomd.Frame()
            fr.configuration.step = step
            fr.configuration.box = BOX
            fr.particles.N = N
            fr.particles.position = rng.uniform(-4, 4, size=(N, 3)).astype(np.float32)
            fr.particles.slength = rng.uniform(0.3, 0.5, size=N).astype(np.float32)
            fr.particles.mass = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
            fr.particles.density = rng.uniform(900, 1100, size=N).astype(np.float32)
            t.append(fr)
    return name


def refusal(call, **kw):
    with pytest.raises(ValueError) as caught:
        call(**kw)
    return str(caught.value)


def adaptive_call(f):
    """The method on frame 1's position chunk with good arguments up to the row lists, which are not reached."""
    def call(box=BOX, cells=(4, 4, 4), **kw):
        return f.sph_adaptive_sums_device(1, 'particles/position', box, cells=cells, rows=None, cell=None, h_max=0.5, **kw)
    return call


def test_the_methods_exist_with_their_defaults():
    names = list(inspect.signature(fl.PGSDFile.sph_adaptive_sums_device).parameters)
    assert names[1:8] == ['frame', 'name', 'box', 'h_max', 'cells', 'rows', 'cell']
    assert names[8:] == ['n', 'slength', 'mass', 'density', 'defaults', 'dimensions', 'kernel', 'mode', 'surface_below',
                         'return_rows']
    defaults = inspect.signature(fl.PGSDFile.sph_adaptive_sums_device).parameters
    assert defaults['mode'].default == 'gather' and defaults['kernel'].default == 'wendland_c2'
    assert list(inspect.signature(fl.PGSDFile.smoothing_range_device).parameters)[1:] == ['slength', 'N', 'rows', 'n', 'default']
    sig = inspect.signature(hoomd.HOOMDTrajectory.frame_adaptive_sums_device).parameters
    assert list(sig)[1:] == ['idx', 'kernel', 'mode', 'cells', 'where', 'domain', 'surface_below', 'return_rows']


def test_it_refuses_its_box_and_its_cells(path):
    with fl.open(path, 'r') as f:
        call = adaptive_call(f)
        assert refusal(call, box=[8, 8, 8, 0, 0]) == "box must hold 6 values"
        assert refusal(call, cells=(4, 4)) == METHOD + ": cells holds three counts, each 1 to 1024"
        assert refusal(call, cells=(4, -1, 4)) == METHOD + ": cells holds three counts, each 1 to 1024"


def test_it_refuses_its_kernel_its_mode_and_its_defaults(path):
    with fl.open(path, 'r') as f:
        call = adaptive_call(f)
        assert refusal(call, kernel='gauss') == METHOD + ": the kernel is one of wendland_c2, cubic_spline: 'gauss'"
        assert refusal(call, mode='scatter') == METHOD + ": the mode is one of gather, mean: 'scatter'"
        wrong = METHOD + ": defaults holds a mass, a density and a smoothing length"
        assert refusal(call, defaults=(1.0, 0.0)) == wrong
        assert refusal(call, defaults=(1.0, 0.0, 1.0, 1.0)) == wrong
        # a call that is wrong twice is refused for what is looked at first: the cells, the kernel, the mode, the defaults
        assert refusal(call, cells=(4, 4), kernel='gauss') == METHOD + ": cells holds three counts, each 1 to 1024"
        assert refusal(call, kernel='gauss', mode='scatter').endswith("'gauss'")
        assert refusal(call, mode='scatter', defaults=(1.0,)).endswith("'scatter'")
        # ... and with its optional chunks given (of either frame) for the same thing
        assert refusal(call, slength=(1, 'particles/slength'), mass=(1, 'particles/mass'), density=(0, 'particles/density'),
                       defaults=(1.0,)) == wrong
        with pytest.raises(KeyError):
            call(slength=(1, 'particles/nothing'))


def test_the_range_refuses_n_without_rows(path):
    with fl.open(path, 'r') as f:
        assert refusal(f.smoothing_range_device, slength=(1, 'particles/slength'), N=N, n=4) == \
            "smoothing_range_device: n goes with rows"
        with pytest.raises(KeyError):
            f.smoothing_range_device((1, 'particles/nothing'), N)
