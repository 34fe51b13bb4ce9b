#!/usr/bin/env python3
"""Relocation-heavy scenarios (the random scripts of tests/test_fuzz_parity.py rarely fill the 128-entry index): many
chunks per frame, many frames, index_entries_to_buffer, flushes in the middle of frames, close + re-open for append,
zero-row ranks, one-rank-only direct writes (logical file size ahead of the true end) -- and, from a second generator,
scripts whose relocations happen at the end of frames of partitioned chunks only (nothing in the write buffer, so the
new block's place comes from the ranks' placements alone).

Host mode (default; build container only, needs oracle/_ref): every script through the compiled reference (under
mpiexec), the oracle and the product in its four placement modes, with PGSD_CHECK_EOF=1 (the computed end of file
against fstat in every relocation) and without.

Device mode (--device; one GPU): every script through the device build of the scenario driver (rows of every chunk
write in HBM) with one exchange per chunk, the frame's exchange and a declared partition (batch 0 / 1 / 3), against
the oracle; dense or strided rows and synchronous or asynchronous seals by seed, PGSD_CHECK_EOF=1 on odd seeds.

    python tools/fuzz_relocation.py [first_seed=1] [n_seeds=40] [--device]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "pgsd-sph_amd"))
import product
import scenario as S
import test_fuzz_parity as F

GENERATORS = [("mixed", F.make_relocation_script), ("partition-only", F.make_partitioned_relocation_script)]


def _set_check_eof(on):
    os.environ.pop("PGSD_CHECK_EOF", None)
    if on:
        os.environ["PGSD_CHECK_EOF"] = "1"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("first", nargs="?", type=int, default=1)
    ap.add_argument("count", nargs="?", type=int, default=40)
    ap.add_argument("--device", action="store_true", help="replay through the device driver (needs a GPU)")
    args = ap.parse_args()
    first, count = args.first, args.count
    ranks = (1, 2, 3, 5) if args.device else (1, 2, 3, 5, 8)
    strip = lambda lines: [re.sub(r"line=\d+ ", "", ln) for ln in lines
                           if not ln.startswith("rc ") or not any(c in ln for c in ("cmd=batch", "cmd=device", "cmd=async"))]
    bad, ran, ref_fail, relocated = [], 0, 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        for seed in range(first, first + count):
            for gen_name, make_script in GENERATORS:
                for P in ranks:
                    scn = os.path.join(tmp, "r.scn")
                    open(scn, "w").write(make_script(seed, P))
                    o_path = os.path.join(tmp, "oracle.gsd")
                    _set_check_eof(False)
                    o_log = S.run_oracle(scn, o_path, P)
                    if [ln for ln in o_log if ln.startswith("rc ")]:
                        continue
                    want = open(o_path, "rb").read()
                    relocated += F._relocated(o_log)
                    p_path = os.path.join(tmp, "p.gsd")
                    if args.device:
                        _set_check_eof(seed % 2)
                        for batch in (0, 1, 3):
                            if os.path.exists(p_path):
                                os.unlink(p_path)
                            s2 = product.device_script(scn, os.path.join(tmp, "d.scn"), 2 if seed % 2 else 1, batch,
                                                       bool((seed // 2) % 2))
                            try:
                                log = product.run_driver(s2, p_path, P, driver=product.DEVICE_DRIVER)
                            except RuntimeError as e:       # a rank's call failed: its exit status says so
                                print(e, flush=True)
                                log = None
                            if log is None or open(p_path, "rb").read() != want or strip(log) != strip(o_log):
                                bad.append((gen_name, seed, P, batch))
                                print("MISMATCH device %s seed %d P %d batch %d check_eof %d"
                                      % (gen_name, seed, P, batch, seed % 2), flush=True)
                        _set_check_eof(False)
                        ran += 1
                        continue
                    for check in (False, True):
                        _set_check_eof(check)
                        for mode in (0, 1, 2, 3):
                            if os.path.exists(p_path):
                                os.unlink(p_path)
                            s2 = scn if mode == 0 else product.batched_script(scn, os.path.join(tmp, "b.scn"), mode)
                            log = product.run_driver(s2, p_path, P, threads=(P == 8))
                            if open(p_path, "rb").read() != want or strip(log) != strip(o_log):
                                bad.append((gen_name, seed, P, mode, check))
                                print("MISMATCH product %s seed %d P %d mode %d check_eof %r"
                                      % (gen_name, seed, P, mode, check), flush=True)
                    _set_check_eof(False)
                    if P <= 5:
                        r_path = os.path.join(tmp, "ref.gsd")
                        if os.path.exists(r_path):
                            os.unlink(r_path)
                        try:
                            out = subprocess.run([F.MPIEXEC, "-n", str(P), F.REF_DRIVER, scn, r_path], capture_output=True,
                                                 timeout=120)
                            finished = out.returncode == 0
                        except subprocess.TimeoutExpired:
                            finished = False
                        if not finished:
                            ref_fail += 1
                        elif open(r_path, "rb").read() != want:
                            bad.append((gen_name, seed, P, "reference"))
                            print("MISMATCH reference vs oracle %s seed %d P %d" % (gen_name, seed, P), flush=True)
                    ran += 1
            if (seed - first + 1) % 10 == 0:
                print("seeds %d..%d: %d scenarios, %d with a relocated index, mismatches %d, reference did not finish %d"
                      % (first, seed, ran, relocated, len(bad), ref_fail), flush=True)
    if args.device:
        print("TOTAL: %d scenarios (mixed and partition-only) x {batch 0, 1, 3} from HBM at 1/2/3/5 ranks, %d with at "
              "least one index relocation: device path == oracle -- mismatches %s" % (ran, relocated, bad))
    else:
        print("TOTAL: %d scenarios (mixed and partition-only) x {4 placement modes} x {PGSD_CHECK_EOF off, on} at 1/2/3/5 "
              "ranks as processes and 8 as threads, %d with at least one index relocation: product == oracle (== reference "
              "wherever it finishes: %d did not) -- mismatches %s" % (ran, relocated, ref_fail, bad))
    sys.exit(1 if bad else 0)
