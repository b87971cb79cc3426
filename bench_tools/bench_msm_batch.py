#!/usr/bin/env python3
"""Batched commit (keaki_hip_msm_g1_batch) against the only route the library had before it: a loop of m keaki_hip_msm_g1_dev calls on one context.

One device, one process, alternating per cell (n, m): the batch call with resident rows (_dev form), the batch call from host memory, the loop of
m single calls over the same resident rows. Every measurement ends in keaki_hip_synchronize; warm-up, then the median of --reps runs (host form
of cells above 256 MB: 5 runs, said in the output). SRS with and without window tables (the batch kernels read the points only; the loop
uses the tables). n = 2^8, 2^10, 2^12, 2^14 = N_BATCH_MAX; m = 1, 2, 4, 8, 16, 256, 1024, 4096 (the loop of 4,096 calls: 3 runs). Random scalars below 2^252 (rows repeat a pool of 2^22:
no kernel's path depends on the values), random on-curve points.

Per n the crossover (the smallest m from which the batch call is not slower than the loop) is printed: kzg::COMMIT_BATCH_MIN of the host mirror.

    python bench_tools/bench_msm_batch.py --tables 0 --out profiles/msm_batch.txt
    python bench_tools/bench_msm_batch.py --tables 1 --out profiles/msm_batch.txt --append
    rocprofv3 --kernel-trace --stats -- python bench_tools/bench_msm_batch.py --trace-only      # ten batch calls at (m, n) = (1024, 4096)
"""
import argparse, faulthandler, os, statistics, sys, time
faulthandler.enable()
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import random_fr_limbs, SEED  # noqa: E402

NS = [1 << 8, 1 << 10, 1 << 12, 1 << 14]
MS = [1, 2, 4, 8, 16, 256, 1024, 4096]          # 2 and 8: the crossover lies between the issue's 1, 4 and 16


def median_ms(f, reps, warm=2):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=0); ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None); ap.add_argument("--append", action="store_true")
    ap.add_argument("--max-m", type=int, default=MS[-1])
    ap.add_argument("--trace-only", action="store_true", help="ten batch _dev calls at (m, n) = (1024, 4096): the run to put under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    import torch
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    hip = KeakiHip(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    mont = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    g1 = np.array(mont(1) + mont(2), np.uint64)
    nmax = NS[-1]
    pts = hip.g1_mul_batch(g1, random_fr_limbs(nmax, SEED + 21))
    srs = hip.srs_g1_upload(pts)
    if a.tables:
        hip.srs_g1_precompute(srs)
    pool = random_fr_limbs(1 << 22, SEED + 22)
    pool[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.trace_only:
        n, m = 4096, 1024
        rows = np.resize(pool, (m * n, 4))
        d_rows, d_out = t(rows), torch.empty((m, 12), dtype=torch.int64, device=dev)
        for _ in range(10):
            hip.msm_g1_batch_dev(srs, d_rows.data_ptr(), n, m, n, d_out.data_ptr())
        hip.synchronize()
        return
    say("# bench_msm_batch: %s, window tables %s, median of %d runs, ms (version %s)" % (torch.cuda.get_device_name(0), "yes" if a.tables else "no", a.reps,
                                                                                        hip.lib.keaki_hip_version().decode() if hasattr(hip.lib.keaki_hip_version, "restype") else ""))
    say("# %7s %6s %12s %12s %12s %9s %14s" % ("n", "m", "batch_dev", "batch_host", "loop_dev", "loop/batch", "batch Mmul/s"))
    for n in NS:
        cross = None
        for m in [x for x in MS if x <= a.max_m]:
            rows = np.resize(pool, (m * n, 4))
            d_rows, d_out = t(rows), torch.empty((m, 12), dtype=torch.int64, device=dev)
            rp, op = d_rows.data_ptr(), d_out.data_ptr()

            def batch_dev():
                hip.msm_g1_batch_dev(srs, rp, n, m, n, op)
                hip.synchronize()

            def loop_dev():
                for j in range(m):
                    hip.msm_g1_dev(srs, rp + j * n * 32, n, op + j * 96)
                hip.synchronize()

            host_reps = a.reps if rows.nbytes <= (256 << 20) else 5
            tb = median_ms(batch_dev, a.reps)
            tl = median_ms(loop_dev, a.reps if m <= 1024 else 3, warm=1)
            th = median_ms(lambda: hip.msm_g1_batch(srs, rows.reshape(m, n, 4)), host_reps, warm=1)
            tb2 = median_ms(batch_dev, a.reps)                     # alternating: the batch call again behind the loop
            tb = min(tb, tb2)
            if cross is None and tb <= tl:
                cross = m
            say("  %7d %6d %12.3f %12.3f %12.3f %9.2f %14.1f%s" % (n, m, tb, th, tl, tl / tb, m * n / tb / 1e3, "" if host_reps == a.reps else "   (host form: 5 runs)"))
            del d_rows, d_out
        say("# n = %d: crossover m = %s" % (n, cross))
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
