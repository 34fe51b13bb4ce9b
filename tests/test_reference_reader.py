"""Files written by this package, as the REFERENCE's own pure-Python reader and schema layer read them.

The readings are stored under tests/golden/reader/ (tests/golden/make_reader_golden.py made them from a reference
checkout): each file below was written by this package, read by the reference's PGSDFile / HOOMDTrajectory, and what
they returned was recorded beside the file's bytes.  Here the package writes the same files again -- they must be
byte-identical to the ones the reference read -- and the reference's readings must be the values that were written."""
import os

import numpy as np

READER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reader")
PARTICLE_FIELDS = ('typeid', 'position', 'velocity', 'density', 'auxiliary2', 'image', 'mass')


def write_hoomd_file(path):
    """Four frames through pgsd.hoomd on one rank (seeded); -> the Frames written."""
    import pgsd.hoomd as hoomd
    rng = np.random.default_rng(0)
    N = 321
    frames = []
    with hoomd.open(path, 'w') as t:
        for i in range(4):
            f = hoomd.Frame()
            f.configuration.step = 1000 + i
            f.configuration.box = [8, 9, 10, 0, 0.5, 0]
            f.particles.N = N
            f.particles.types = ['water', 'wall']
            f.particles.typeid = rng.integers(0, 2, N)
            f.particles.position = rng.standard_normal((N, 3))
            f.particles.velocity = rng.standard_normal((N, 3))
            f.particles.density = rng.random(N)
            f.particles.auxiliary2 = rng.standard_normal((N, 3))
            f.particles.image = rng.integers(-1, 2, (N, 3))
            f.log['pe'] = np.array([float(i)])
            f.validate()
            frames.append(f)
            t.append(f)
    return frames


def write_multi_rank_file(path):
    """A 3-rank file (duplicated replicated chunks, per-rank offsets) written by the product driver."""
    import product
    import scenario as S
    product.run_driver(S.scenario_path("sph_full"), path, 3)


def _same_bytes(path, golden):
    with open(path, 'rb') as a, open(os.path.join(READER, golden), 'rb') as b:
        assert a.read() == b.read(), "the package no longer writes the file the reference's reader was shown: " + golden


def test_reference_reader_reads_our_hoomd_file(tmp_gsd):
    frames = write_hoomd_file(tmp_gsd)
    N = frames[0].particles.N
    _same_bytes(tmp_gsd, "hoomd4.gsd")
    rec = np.load(os.path.join(READER, "hoomd4.reference_read.npz"))
    assert int(rec['len']) == 4
    for i in (0, 2, 3):
        exp = frames[i]
        assert int(rec['%d/step' % i]) == 1000 + i
        np.testing.assert_array_equal(rec['%d/box' % i], exp.configuration.box)
        assert int(rec['%d/N' % i]) == N and list(rec['%d/types' % i]) == ['water', 'wall']
        for name in PARTICLE_FIELDS[:-1]:
            np.testing.assert_array_equal(rec['%d/%s' % (i, name)], getattr(exp.particles, name), err_msg=name)
        np.testing.assert_array_equal(rec['%d/mass' % i], np.ones(N, dtype=np.float32))      # default fallback
        np.testing.assert_array_equal(rec['%d/log/pe' % i], [float(i)])


def test_reference_reader_reads_multi_rank_golden_like_file(tmp_gsd):
    import scenario as S
    from pgsd.pypgsd import PGSDFile
    write_multi_rank_file(tmp_gsd)
    _same_bytes(tmp_gsd, "sph_full3.gsd")
    rec = np.load(os.path.join(READER, "sph_full3.reference_read.npz"))
    assert int(rec['nframes']) == 2 and str(rec['schema']) == 'hoomd'
    np.testing.assert_array_equal(rec['1/particles/position'], S.gen_data(9, 8, 0, 333, 3))
    assert rec['0/particles/N'].dtype == np.uint32
    ours = PGSDFile(open(tmp_gsd, 'rb'))
    for name in rec['names']:
        for frame in range(2):
            exists = '%d/%s' % (frame, name) in rec.files
            assert exists == ours.chunk_exists(frame, name)
            if exists:
                got = ours.read_chunk(frame, name)
                np.testing.assert_array_equal(rec['%d/%s' % (frame, name)], got)
                assert rec['%d/%s' % (frame, name)].dtype == got.dtype
