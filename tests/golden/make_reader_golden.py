"""Record what the REFERENCE's pure-Python reader returns for files this package writes (tests/test_reference_reader.py).

    python tests/golden/make_reader_golden.py <reference checkout>/pgsd/pgsd

Run from a built tree.  Writes tests/golden/reader/<name>.gsd (the file the reference read) and
<name>.reference_read.npz (what its PGSDFile / HOOMDTrajectory returned).  The fixtures are data; no reference
source is stored.  The reference's hoomd.py imports mpi4py unconditionally (hoomd.py:29) but never uses it on the
read path, so an empty stand-in module is registered before the import."""
import importlib.util
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "pgsd-sph_amd")]

import test_reference_reader as T  # noqa: E402


def load_reference_module(ref, name):
    """Import the reference's module under a private name (keeps it apart from this repo's `pgsd`)."""
    if "mpi4py" not in sys.modules:
        stub = types.ModuleType("mpi4py")
        stub.MPI = object()
        sys.modules["mpi4py"] = stub
    spec = importlib.util.spec_from_file_location("reference_" + name, os.path.join(ref, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref):
    rp, rh = load_reference_module(ref, "pypgsd"), load_reference_module(ref, "hoomd")
    os.makedirs(T.READER, exist_ok=True)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "hoomd4.gsd")
        T.write_hoomd_file(path)
        traj = rh.HOOMDTrajectory(rp.PGSDFile(open(path, 'rb')))
        rec = {'len': np.array(len(traj))}
        for i in (0, 2, 3):
            s = traj[i]
            rec['%d/step' % i] = np.array(s.configuration.step)
            rec['%d/box' % i] = np.asarray(s.configuration.box)
            rec['%d/N' % i] = np.array(s.particles.N)
            rec['%d/types' % i] = np.array(s.particles.types)
            for name in T.PARTICLE_FIELDS:
                rec['%d/%s' % (i, name)] = np.asarray(getattr(s.particles, name))
            rec['%d/log/pe' % i] = np.asarray(s.log['pe'])
        np.savez_compressed(os.path.join(T.READER, "hoomd4.reference_read.npz"), **rec)
        shutil.copy(path, os.path.join(T.READER, "hoomd4.gsd"))

        path = os.path.join(d, "sph_full3.gsd")
        T.write_multi_rank_file(path)
        f = rp.PGSDFile(open(path, 'rb'))
        names = list(f.find_matching_chunk_names(''))
        rec = {'nframes': np.array(f.nframes), 'schema': np.array(f.schema), 'names': np.array(names)}
        for name in names:
            for frame in range(f.nframes):
                if f.chunk_exists(frame, name):
                    rec['%d/%s' % (frame, name)] = f.read_chunk(frame, name)
        np.savez_compressed(os.path.join(T.READER, "sph_full3.reference_read.npz"), **rec)
        shutil.copy(path, os.path.join(T.READER, "sph_full3.gsd"))


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "pypgsd.py")):
        raise SystemExit(__doc__)
    main(sys.argv[1])
