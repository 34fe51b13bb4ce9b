"""What pgsd.fl's GPU pass methods refuse on the Python side, before the library is called: the full text of every
message.  All of them are raised before the row lists are looked at, so no GPU memory -- and no GPU -- is needed; the
library's own refusals are held by the tests of each pass on the GPU."""
import numpy as np
import pytest

import pgsd.fl as fl
import pgsd.hoomd as hoomd

N = 8
BOX = [8, 8, 8, 0, 0, 0]
PAIR_METHODS = ('neighbours_device', 'sph_sums_device', 'sph_gradients_device')
SPH_METHODS = PAIR_METHODS[1:]


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    """Two frames of 8 particles with position, velocity, mass and density, written on the host path."""
    name = str(tmp_path_factory.mktemp("pass_arguments") / "eight.gsd")
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


def pair_call(f, method):
    """The method on frame 1's position chunk with good arguments up to the row lists, which are not reached."""
    def call(box=BOX, cells=(4, 4, 4), **kw):
        reach = dict(r=1.0) if method == 'neighbours_device' else dict(h=0.5)
        return getattr(f, method)(1, 'particles/position', box, cells=cells, rows=None, cell=None, **reach, **kw)
    return call


@pytest.mark.parametrize("method", PAIR_METHODS)
def test_a_pair_method_refuses_its_box_and_its_cells(path, method):
    with fl.open(path, 'r') as f:
        call = pair_call(f, method)
        assert refusal(call, box=[8, 8, 8, 0, 0]) == "box must hold 6 values"
        assert refusal(call, cells=(4, 4)) == method + ": cells holds three counts, each 1 to 1024"
        assert refusal(call, cells=(4, -1, 4)) == method + ": cells holds three counts, each 1 to 1024"


@pytest.mark.parametrize("method", SPH_METHODS)
def test_an_sph_method_refuses_its_kernel_and_its_defaults(path, method):
    with fl.open(path, 'r') as f:
        call = pair_call(f, method)
        assert refusal(call, kernel='gauss') == method + ": the kernel is one of wendland_c2, cubic_spline: 'gauss'"
        assert refusal(call, defaults=(1.0,)) == method + ": defaults holds a mass and a density"
        # a call that is wrong twice is refused for its cells, which are looked at first
        assert refusal(call, cells=(4, 4), kernel='gauss') == method + ": cells holds three counts, each 1 to 1024"
        # ... and with its optional chunks given (of either frame) for the same thing
        assert refusal(call, mass=(1, 'particles/mass'), density=(0, 'particles/density'), defaults=(1.0,)) \
            == method + ": defaults holds a mass and a density"


def test_neighbours_refuses_its_bins(path):
    with fl.open(path, 'r') as f:
        assert refusal(pair_call(f, 'neighbours_device'), bins=-1) == "neighbours_device: bins is 0 or 1 to 1024"


def test_the_moments_methods_refuse_their_chunks_and_defaults(path):
    chunks = [None, (1, 'particles/mass'), (1, 'particles/velocity'), None, (1, 'particles/position')]
    with fl.open(path, 'r') as f:
        assert refusal(f.frame_moments_device, chunks=chunks[:4]) \
            == "frame_moments_device: chunks holds typeid, mass, velocity, energy, position (or None)"
        assert refusal(f.frame_moments_device, chunks=chunks, defaults=[1.0] * 7) \
            == "frame_moments_device: defaults holds mass, v[3], energy, x[3]"
        assert refusal(f.frame_moments_device, chunks=chunks, n_types=-1) \
            == "frame_moments_device: a call takes 1 to 4 types from a type id on"

        def cells(**kw):
            return f.cell_moments_device(rows=None, cell=None, n=None, n_cells=8, **kw)

        assert refusal(cells, chunks=chunks[1:4]) \
            == "cell_moments_device: chunks holds mass, velocity, energy, position (or None)"
        assert refusal(cells, chunks=chunks[1:], defaults=[1.0] * 7) \
            == "cell_moments_device: defaults holds mass, v[3], energy, x[3]"
