"""Particle tracks on the CPU: pgsd.fl.row_plan_model (the numpy definition of a row plan, which the GPU plan of
PGSDFile.plan_rows must equal exactly: tests/test_gpu_tracks.py) against a brute-force statement of it, and
HOOMDTrajectory.read_tracks against the per-frame host reads it is defined by."""
import os

import numpy as np
import pytest

import pgsd.fl as fl
import pgsd.hoomd as hoomd

READER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reader")


def brute_plan(rows, N, R):
    """(touched blocks, runs as (first, count), rows2, staged rows), stated the slow way."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    inside = rows[rows < N]
    blocks = np.unique(inside // R)
    runs = []
    for b in blocks:
        if runs and runs[-1][0] + runs[-1][1] == b:
            runs[-1][1] += 1
        else:
            runs.append([int(b), 1])
    rows2 = np.empty(len(rows), dtype=np.uint32)
    for k, r in enumerate(rows):
        rows2[k] = 0xFFFFFFFF if r >= N else int(np.searchsorted(blocks, r // R)) * R + r % R
    staged = sum(min((int(b) + 1) * R, N) - int(b) * R for b in blocks)
    return blocks.astype(np.uint32), np.array(runs, dtype=np.uint32).reshape(-1, 2), rows2, staged


def plan_cases():
    """(name, rows, N, R): the cases the issue lists; shared with the GPU test."""
    edges = np.array([r for b in range(1, 8) for r in (b * 64 - 1, b * 64)])
    return [
        ("empty", [], 1000, 64),
        ("one row", [517], 1000, 64),
        ("all rows", np.arange(1000), 1000, 64),
        ("duplicates", [5, 5, 900, 5, 900, 64, 64], 1000, 64),
        ("descending", np.arange(999, -1, -7), 1000, 64),
        ("both sides of every block edge", edges, 512, 64),
        ("N = 1", [0, 0], 1, 64),
        ("short last block", [0, 960, 999, 130], 1000, 64),
        ("short last block only", [999, 998], 1000, 64),
        ("an entry >= N", [3, 1000, 70, 4000000000, 999], 1000, 64),
        ("only entries >= N", [1000, 1001], 1000, 64),
        ("R larger than N", [7, 0, 99], 100, 4096),
        ("gaps and neighbours", [0, 70, 200, 260, 330, 640], 1000, 64),
    ]


@pytest.mark.parametrize("case", plan_cases(), ids=lambda c: c[0])
def test_row_plan_model_is_the_brute_force_statement(case):
    _, rows, N, R = case
    rows = np.asarray(rows, dtype=np.int64)
    m = fl.row_plan_model(rows.astype(np.uint32), N, R)
    blocks, runs, rows2, staged = brute_plan(rows, N, R)
    assert m.blocks.dtype == np.uint32 and m.rows2.dtype == np.uint32 and m.runs.dtype == np.uint32
    np.testing.assert_array_equal(m.blocks, blocks)
    np.testing.assert_array_equal(m.runs, runs)
    np.testing.assert_array_equal(m.rows2, rows2)
    assert m.staged_rows == staged
    # what the plan is for: gathering the compact staging through rows2 is gathering the chunk through rows
    chunk = np.arange(N, dtype=np.int64) * 3 + 1
    staging = np.concatenate([chunk[int(b) * R:min((int(b) + 1) * R, N)] for b in m.blocks] + [chunk[:0]])
    assert len(staging) == m.staged_rows
    ok = rows < N
    np.testing.assert_array_equal(staging[m.rows2[ok]], chunk[rows[ok]])
    assert (m.rows2[~ok] == 0xFFFFFFFF).all()


@pytest.mark.parametrize("seed", range(8))
def test_row_plan_model_random_lists(seed):
    rng = np.random.default_rng(seed)
    N = int(rng.integers(1, 20000))
    R = int(rng.choice([1, 7, 64, 100, 4096]))
    rows = rng.integers(0, N + (5 if seed % 2 else 0), size=int(rng.integers(0, 300)))
    m = fl.row_plan_model(rows.astype(np.int32), N, R)          # int32, as select_rows types its lists
    blocks, runs, rows2, staged = brute_plan(rows, N, R)
    np.testing.assert_array_equal(m.blocks, blocks)
    np.testing.assert_array_equal(m.runs, runs)
    np.testing.assert_array_equal(m.rows2, rows2)
    assert m.staged_rows == staged


def test_short_last_block_has_the_highest_slot():
    m = fl.row_plan_model(np.array([999, 3], dtype=np.uint32), 1000, 64)
    assert list(m.blocks) == [0, 15] and m.staged_rows == 64 + 40
    assert list(m.rows2) == [64 + 39, 3]


# ---------------------------------------------------------------------------------------------- read_tracks
def write_track_trajectory(path, to_device=None):
    """Six frames on one rank: static arrays elided after frame 0, a density that changes in frame 2 and comes back,
    frame 4 with another particle count, frame 5 back at frame 0's.  `to_device` turns the per-particle arrays into GPU
    arrays before `append` (the GPU test writes the same trajectory from device memory)."""
    rng = np.random.default_rng(42)
    N = 700
    static = dict(typeid=rng.integers(0, 3, N).astype(np.uint32), mass=rng.random(N).astype(np.float32),
                  image=rng.integers(-2, 3, (N, 3)).astype(np.int32), density=rng.random(N).astype(np.float32))
    with hoomd.open(path, 'w') as t:
        for i in range(6):
            n = 500 if i == 4 else N
            f = hoomd.Frame()
            f.configuration.step = 10 * i + 3
            f.configuration.box = [8, 9, 10, 0, 0, 0]
            f.particles.N = n
            f.particles.types = ['a', 'b', 'c']
            arrays = {k: v[:n] for k, v in static.items()}
            arrays['position'] = rng.standard_normal((n, 3)).astype(np.float32)
            if i != 3:
                arrays['velocity'] = rng.standard_normal((n, 3)).astype(np.float32)      # frame 3: no velocity set
            if i == 2:
                arrays['density'] = rng.random(n).astype(np.float32)
            for k, v in arrays.items():
                setattr(f.particles, k, to_device(v) if to_device else v)
            t.append(f)


TRACK_FIELDS = ('position', 'velocity', 'density', 'typeid', 'image', 'mass', 'body')


def check_tracks_against_frames(traj, tracks, rows, frames, fields, to_host=np.asarray):
    assert tracks.step.dtype == np.uint64 and len(tracks.step) == len(frames)
    for i, idx in enumerate(frames):
        frame = traj[idx]
        assert int(tracks.step[i]) == int(frame.configuration.step)
        for name in fields:
            expect = getattr(frame.particles, name)[rows]
            got = to_host(tracks[name])[i]
            assert got.dtype == expect.dtype and got.shape == expect.shape, name
            assert got.tobytes() == expect.tobytes(), (name, idx)


def test_read_tracks_is_the_per_frame_host_read(tmp_gsd):
    write_track_trajectory(tmp_gsd)
    rows = np.array([3, 499, 0, 3, 250, 17])                # unsorted, a repeat; all inside the short frame
    with hoomd.open(tmp_gsd, 'r') as traj:
        # the trajectory is what the docstring says: elided arrays, a changed one, a short frame
        f = traj.file
        assert not f.chunk_exists(1, 'particles/mass') and not f.chunk_exists(1, 'particles/density')
        assert f.chunk_exists(2, 'particles/density') and not f.chunk_exists(3, 'particles/density')
        assert traj[4].particles.N == 500 and traj[5].particles.N == 700
        everything = traj.read_tracks(rows, fields=TRACK_FIELDS)
        check_tracks_against_frames(traj, everything, rows, list(range(6)), TRACK_FIELDS)
        assert everything.position.shape == (6, 6, 3) and everything.density.shape == (6, 6)
        assert everything.typeid.dtype == np.uint32 and everything.image.dtype == np.int32
        np.testing.assert_array_equal(everything.rows, rows)
        sliced = traj.read_tracks(rows, frames=slice(1, 6, 2), fields=('velocity', 'mass'))
        check_tracks_against_frames(traj, sliced, rows, [1, 3, 5], ('velocity', 'mass'))
        listed = traj.read_tracks(rows, frames=[5, 0, -2], fields=('image',))
        check_tracks_against_frames(traj, listed, rows, [5, 0, 4], ('image',))
        default = traj.read_tracks(rows, frames=[2])
        assert default.fields == ('position',)
        check_tracks_against_frames(traj, default, rows, [2], ('position',))
        none = traj.read_tracks([], frames=[0, 1], fields=('position', 'mass'))
        assert none.position.shape == (2, 0, 3) and none.mass.shape == (2, 0)


def test_read_tracks_refuses_a_frame_the_rows_reach_past(tmp_gsd):
    write_track_trajectory(tmp_gsd)
    with hoomd.open(tmp_gsd, 'r') as traj:
        with pytest.raises(IndexError, match="frame 4"):
            traj.read_tracks([1, 500], fields=('position',))
        with pytest.raises(IndexError, match="frame 4"):
            traj.read_tracks([699], frames=slice(3, 6))
        ok = traj.read_tracks([699, 500], frames=[0, 1, 2, 3, 5], fields=('position', 'density'))
        check_tracks_against_frames(traj, ok, np.array([699, 500]), [0, 1, 2, 3, 5], ('position', 'density'))
        with pytest.raises(IndexError):
            traj.read_tracks([0], frames=[6])
        with pytest.raises(ValueError):
            traj.read_tracks([0], fields=('types',))


def test_read_tracks_equals_the_reference_readers_rows_hoomd4():
    rec = np.load(os.path.join(READER, "hoomd4.reference_read.npz"))
    rows = np.array([320, 0, 7, 7, 123, 200])
    fields = ('typeid', 'position', 'velocity', 'density', 'auxiliary2', 'image', 'mass')
    with hoomd.open(os.path.join(READER, "hoomd4.gsd"), 'r') as traj:
        tracks = traj.read_tracks(rows, frames=[0, 2, 3], fields=fields)
        for i, idx in enumerate((0, 2, 3)):
            assert int(tracks.step[i]) == int(rec['%d/step' % idx])
            for name in fields:
                expect = rec['%d/%s' % (idx, name)][rows]
                assert tracks[name][i].dtype == expect.dtype
                np.testing.assert_array_equal(tracks[name][i], expect, err_msg="%s frame %d" % (name, idx))


def test_read_tracks_equals_the_reference_readers_rows_sph_full3():
    rec = np.load(os.path.join(READER, "sph_full3.reference_read.npz"))
    rows = np.array([332, 1, 1, 111, 222, 0])
    per_particle = sorted({k.split('/')[2] for k in rec.files if k[1:].startswith('/particles/')}
                          - {'N', 'types', 'type_shapes'})
    assert len(per_particle) >= 14
    checked = 0
    with hoomd.open(os.path.join(READER, "sph_full3.gsd"), 'r') as traj:
        tracks = traj.read_tracks(rows, fields=per_particle)
        for i in range(int(rec['nframes'])):
            assert int(tracks.step[i]) == int(rec['%d/configuration/step' % i][0])
            for name in per_particle:
                key = '%d/particles/%s' % (i, name)
                if key not in rec.files:
                    key = '0/particles/%s' % name           # elided: the reader hands out frame 0's
                expect = rec[key][rows]
                assert tracks[name][i].dtype == expect.dtype
                np.testing.assert_array_equal(tracks[name][i], expect, err_msg="%s frame %d" % (name, i))
                checked += 1
    assert checked == len(per_particle) * int(rec['nframes'])
