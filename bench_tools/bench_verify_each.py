#!/usr/bin/env python3
"""KZG verify_each (keaki_hip_kzg_verify_each: one verdict per opening) at n = 2^10, 2^16, 2^20, resident (_dev) and from host arrays, against
what the library offers beside it, all in ONE process on the same data:

  (a) verify_each, _dev and host form (one commitment, explicit points)
  (b) keaki_hip_pairing_batch_dev over n items: one pairing with lines on the fly per item, the closest existing yardstick
  (c) keaki_hip_pairing_batch_dev over 2n items: two separate pairings per item, what the fused kernel must beat
  (d) keaki_hip_g1_mul_batch_dev over n items: the variable-base ladder the G1 stage adds
  (e) the mean of 64 single keaki_hip_kzg_verify calls times n: EXTRAPOLATED, nobody runs it at 2^20
  (f) keaki_hip_kzg_verify_batch on the same items (one yes/no for all of them)

Per n: warm-up rounds, then --reps rounds; a round runs every candidate once, and the order of the candidates is reversed from round to round.
Every timed call ends in a device synchronisation (verify_each and verify_batch synchronise themselves: their results are host words). Medians
and minima in ms. The inputs are random on-curve points and random scalars: every verdict is "invalid", and no kernel of the call has a path
that depends on the verdict.

    python bench_tools/bench_verify_each.py --out profiles/verify_each_times.txt
"""
import argparse, faulthandler, os, statistics, sys, time
faulthandler.enable()
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import random_fr_limbs, SEED  # noqa: E402
from bench_tools.bench_verify_batch import _g2_gen  # noqa: E402


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[10, 16, 20]); ap.add_argument("--reps", type=int, default=0, help="rounds per n; 0 = 21 / 11 / 7 by size")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    hip = KeakiHip(0)
    nmax = 1 << max(a.log2n)
    P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    mont = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    g1 = np.array(mont(1) + mont(2), np.uint64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    sync = lambda: (hip.synchronize(), torch.cuda.synchronize(dev))
    d_g1 = t(g1)
    d_proofs = torch.empty((nmax, 8), dtype=torch.int64, device=dev)
    d_k = t(random_fr_limbs(nmax, SEED + 21))
    hip.g1_mul_batch_dev(d_g1.data_ptr(), 0, d_k.data_ptr(), nmax, d_proofs.data_ptr())
    sync()
    proofs = d_proofs.cpu().numpy().view(np.uint64)
    com = proofs[nmax - 1:nmax].copy()
    tau_g2 = hip.g2_mul_batch(_g2_gen(), random_fr_limbs(1, SEED + 22))[0]
    zs, ys, gs = random_fr_limbs(nmax, SEED + 23), random_fr_limbs(nmax, SEED + 24), random_fr_limbs(nmax, SEED + 25)
    d_com, d_tau, d_z, d_y, d_g = t(com), t(tau_g2), t(zs), t(ys), t(gs)
    d_status = torch.empty(nmax, dtype=torch.uint8, device=dev)
    d_gt = torch.empty((2 * nmax, 48), dtype=torch.int64, device=dev)
    d_mul = torch.empty((nmax, 8), dtype=torch.int64, device=dev)
    sync()
    singles = [timed(lambda i=i: hip.kzg_verify(com[0], tau_g2, zs[i], ys[i], proofs[i])) for i in range(8 + 64)][8:]
    single = statistics.mean(singles)
    names = ["each_dev", "each_host", "pair_n", "pair_2n", "mul_n", "batch"]
    lines = ["# %s" % hip.version(),
             "# keaki_hip_kzg_verify_each against its yardsticks, ms; per n: warm-up rounds, then `rounds` rounds of every candidate once, order reversed from round",
             "# to round, one process, every call ending in a device synchronisation. median (min) per candidate.",
             "# each_dev / each_host = (a) verify_each resident / from host arrays | pair_n = (b) pairing_batch_dev, n pairings, lines on the fly | pair_2n = (c) the",
             "# same over 2n | mul_n = (d) g1_mul_batch_dev, n ladders | batch = (f) verify_batch (host form) on the same items",
             "# n*single = (e) EXTRAPOLATED: n x the mean of 64 single keaki_hip_kzg_verify calls (%.3f ms each), not run at that size" % single]
    for log2n in a.log2n:
        n = 1 << log2n
        rounds = a.reps or (21 if log2n <= 12 else 11 if log2n <= 17 else 7)
        pair = lambda m: (hip.pairing_batch_dev(d_proofs.data_ptr(), d_tau.data_ptr(), 0, m, d_gt.data_ptr()), hip.synchronize())
        cands = [
            lambda: hip.kzg_verify_each_dev(d_com, 0, d_tau, d_z, 0, d_y, d_proofs, n, d_status),
            lambda: hip.kzg_verify_each(com, tau_g2, zs[:n], ys[:n], proofs[:n]),
            lambda: pair(n),
            # 2n pairings: the proofs twice (the first slot's values do not change the work)
            lambda: (hip.pairing_batch_dev(d_proofs.data_ptr(), d_tau.data_ptr(), 0, n, d_gt.data_ptr()),
                     hip.pairing_batch_dev(d_proofs.data_ptr(), d_tau.data_ptr(), 0, n, d_gt.data_ptr() + n * 384), hip.synchronize()),
            lambda: (hip.g1_mul_batch_dev(d_proofs.data_ptr(), 1, d_z.data_ptr(), n, d_mul.data_ptr()), hip.synchronize()),
            lambda: hip.kzg_verify_batch(com, tau_g2, zs[:n], ys[:n], proofs[:n], gs[:n]),
        ]
        ts = [[] for _ in cands]
        for r in range(2 + rounds):
            order = range(len(cands)) if r % 2 == 0 else reversed(range(len(cands)))
            for i in order:
                ms = timed(cands[i])
                if r >= 2:
                    ts[i].append(ms)
        med = [statistics.median(x) for x in ts]
        lines.append("n = 2^%d, rounds = %d" % (log2n, rounds))
        for nm, x, m in zip(names, ts, med):
            lines.append("  %-10s %10.3f (%.3f)" % (nm, m, min(x)))
        lines.append("  %-10s %10.1f   extrapolated" % ("n*single", n * single))
        lines.append("  ratios: (a)/(b) = %.2f resident | (a)/(c) = %.2f resident | (a)/(e) = 1/%.0f resident, 1/%.0f host | (a)/(f) = %.1f host | items/s resident = %.2f M"
                     % (med[0] / med[2], med[0] / med[3], n * single / med[0], n * single / med[1], med[1] / med[5], n / med[0] / 1e3))
        print("\n".join(lines[-9:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    hip.close()


if __name__ == "__main__":
    main()
