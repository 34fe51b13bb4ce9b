"""Worker of tests/test_gpu_writer_lane.py: one process per setting of the writer lane's knobs (they are read once, when
a pipeline is made), which writes the same frames from device memory three times -- sealed synchronously, sealed
asynchronously, and the extra frame of `extra_frame()`.

    python writer_lane_worker.py <repository root> <output directory>
"""
import os
import sys

import numpy as np

N = 300_001            # 8.4 MB per frame: above the direct road's 2 MiB, chunk sizes no multiple of any piece
FRAMES = 3
SLAB = 1 << 20
N_EXTRA = SLAB // 16 + 1   # a four-column float32 chunk of exactly one slab plus one row


def frame(i):
    """(step, position + type id in w as float4, velocity as float4) of frame i"""
    rng = np.random.default_rng(4100 + i)
    pos = rng.standard_normal((N, 4)).astype(np.float32)
    vel = rng.standard_normal((N, 4)).astype(np.float32)
    pos[:, 3] = rng.integers(0, 5, size=N).astype(np.uint32).view(np.float32)
    return np.array([10 * i], dtype=np.uint64), pos, vel


def extra_frame():
    rng = np.random.default_rng(4200)
    return rng.standard_normal((N_EXTRA, 4)).astype(np.float32), rng.standard_normal((N_EXTRA, 4)).astype(np.float32)


def main():
    root, out = sys.argv[1], sys.argv[2]
    sys.path.insert(0, os.path.join(root, "pgsd-sph_amd"))
    import torch
    import pgsd.fl as fl

    torch.cuda.set_device(0)
    threads_before = len(os.listdir("/proc/self/task"))
    for tag in ("sync", "async", "extra"):
        f = fl.open(os.path.join(out, tag + ".gsd"), "w", application="app", schema="hoomd", schema_version=[1, 4])
        f.configure_device(slab_bytes=SLAB)
        keep = []
        for i in range(FRAMES if tag != "extra" else 1):
            step, pos, vel = frame(i)
            dpos, dvel = torch.from_numpy(pos).cuda(), torch.from_numpy(vel).cuda()
            keep += [dpos, dvel]
            f.write_chunk("configuration/step", step, write_all=False)
            f.write_chunks([("particles/position", fl.DeviceField.from_tensor(dpos, columns=(0, 3))),
                            ("particles/typeid", fl.DeviceField.from_tensor(dpos, columns=(3, 4), out_dtype=np.uint32, bitcast=True)),
                            ("particles/velocity", fl.DeviceField.from_tensor(dvel, columns=(0, 3)))], offset=np.array([N]))
            f.end_frame(wait=tag != "async")
        if tag == "extra":
            a, b = extra_frame()
            da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
            keep += [da, db]
            f.write_chunks([("particles/orientation", fl.DeviceField.from_tensor(da, columns=(0, 4))),
                            ("particles/position", fl.DeviceField.from_tensor(db, columns=(0, 3))),
                            ("particles/velocity", fl.DeviceField.from_tensor(da, columns=(0, 3)))], offset=np.array([N_EXTRA]))
            z = torch.zeros((0, 4), device="cuda")
            f.write_chunks([("particles/mass", fl.DeviceField(z.data_ptr() or 16, np.float32, 0, 1))], offset=np.array([0]))
            f.end_frame()
        if tag == "async":
            f.frame_sync()
        if tag == "sync":
            print("threads the first pipeline added: %d" % (len(os.listdir("/proc/self/task")) - threads_before))
        f.close()
    print("ok")


if __name__ == "__main__":
    main()
