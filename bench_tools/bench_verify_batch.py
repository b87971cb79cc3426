#!/usr/bin/env python3
"""KZG batch verification (keaki_hip_kzg_verify_batch) at n = 2^10 .. 2^20 against the only bulk alternative the library had before it:
keaki_hip_pairing_batch on 2n pairings (the inner points of the 2n pairings are NOT counted, which favours that route), and against n single
keaki_hip_kzg_verify calls (measured on 16 calls, scaled).

Per n: the vector-commitment form (one commitment, point_mode 1) and the general form (n commitments, n points), host and _dev entries:
warm-up, then the median of --reps calls, every call ending in a device synchronisation (the entries synchronise themselves: ok_out is a
host pointer). Where the time goes, from public calls on the same data: upload = host form - _dev form; one MSM over the proofs
(keaki_hip_msm_g1_dev on the proofs wrapped as an SRS without tables, the call the batch entry makes); the two pairings in one launch
(keaki_hip_pairing_batch_dev, n = 2); the rest = scalar preparation + the two single scalar-mults + the final sum + the downloads.
The inputs are random on-curve points and random scalars: the verdict is 0, and no kernel of the call has a path that depends on it.

    python bench_tools/bench_verify_batch.py --out profiles/verify_batch.txt
"""
import argparse, faulthandler, os, statistics, sys, time
faulthandler.enable()
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import random_fr_limbs, SEED  # noqa: E402


def median_ms(f, reps, warm=3):
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
    ap.add_argument("--log2n-min", type=int, default=10); ap.add_argument("--log2n-max", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true", help="only --reps calls of the _dev entry (vector-commitment form) at 2^log2n-max: the run to put under "
                                                                "`rocprofv3 --kernel-trace --stats -- python ...` for per-kernel times")
    a = ap.parse_args()
    import torch
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    hip = KeakiHip(0)
    nmax = 1 << a.log2n_max
    P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    mont = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    g1 = np.array(mont(1) + mont(2), np.uint64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    sync = lambda: (hip.synchronize(), torch.cuda.synchronize(dev))
    # proofs, commitments: multiples of g1 by random scalars (made on the device); [tau]_2 and n G2 points for the pairing route likewise
    d_proofs = torch.empty((nmax, 8), dtype=torch.int64, device=dev)
    d_coms = torch.empty((nmax, 8), dtype=torch.int64, device=dev)
    d_g1 = t(g1)
    for seed, dst in ((11, d_proofs), (12, d_coms)):
        d_k = t(random_fr_limbs(nmax, SEED + seed))
        hip.g1_mul_batch_dev(d_g1.data_ptr(), 0, d_k.data_ptr(), nmax, dst.data_ptr())
        sync()
    proofs, coms = d_proofs.cpu().numpy().view(np.uint64), d_coms.cpu().numpy().view(np.uint64)
    g2 = hip.g2_mul_batch(_g2_gen(), random_fr_limbs(1, SEED + 13))
    tau_g2 = g2[0]
    d_tau = t(tau_g2)
    n_g2 = min(nmax, 1 << 16)                        # the pairing route's second arguments: 2^16 distinct G2 points, tiled
    d_q = torch.empty((n_g2, 16), dtype=torch.int64, device=dev)
    hip.g2_mul_batch_dev(t(tau_g2).data_ptr(), 0, t(random_fr_limbs(n_g2, SEED + 14)).data_ptr(), n_g2, d_q.data_ptr())
    sync()
    zs, ys, gs = random_fr_limbs(nmax, SEED + 15), random_fr_limbs(nmax, SEED + 16), random_fr_limbs(nmax, SEED + 17)
    omega = random_fr_limbs(1, SEED + 18)
    d_z, d_y, d_g, d_omega = t(zs), t(ys), t(gs), t(omega)
    sync()
    if a.trace_only:
        for _ in range(a.reps):
            hip.kzg_verify_batch_dev(d_coms, 0, d_tau, d_omega, 1, d_y, d_proofs, d_g, nmax)
        hip.close()
        return
    single = median_ms(lambda: hip.kzg_verify(coms[0], tau_g2, zs[0], ys[0], proofs[0]), 16)
    lines = ["# %s" % hip.version(),
             "# keaki_hip_kzg_verify_batch: median of %d calls (ms), each ending in a device synchronisation; warm-up 3 calls" % a.reps,
             "# vec = one commitment, point_mode 1 (the vec_verify form); gen = n commitments, n points (general form)",
             "# pair2n = keaki_hip_pairing_batch_dev on 2n pairings, inner points not counted; single = one keaki_hip_kzg_verify: %.3f ms" % single,
             "# msm = ONE keaki_hip_msm_g1_dev over the proofs as an ad-hoc SRS (the batch call runs two; three in the general form); pair2 = the two pairings",
             "# rest = vec_dev - 2 msm - pair2: scalar preparation, g C and t g1 (one scalar-mult launch), the final sum, downloads",
             "%6s %9s %9s %9s %9s %9s %9s %9s %9s %10s %12s %11s" % ("log2n", "vec_host", "vec_dev", "gen_host", "gen_dev", "upload", "msm", "pair2", "rest",
                                                                   "pair2n", "pair2n/vec", "n*single/vec")]
    d_gt = torch.empty((2 * nmax, 48), dtype=torch.int64, device=dev)
    d_out = torch.empty(12, dtype=torch.int64, device=dev)
    for log2n in range(a.log2n_min, a.log2n_max + 1):
        n = 1 << log2n
        vec_host = median_ms(lambda: hip.kzg_verify_batch(coms[:1], tau_g2, omega, ys[:n], proofs[:n], gs[:n], point_mode=1), a.reps)
        vec_dev = median_ms(lambda: hip.kzg_verify_batch_dev(d_coms, 0, d_tau, d_omega, 1, d_y, d_proofs, d_g, n), a.reps)
        gen_host = median_ms(lambda: hip.kzg_verify_batch(coms[:n], tau_g2, zs[:n], ys[:n], proofs[:n], gs[:n]), a.reps)
        gen_dev = median_ms(lambda: hip.kzg_verify_batch_dev(d_coms, 1, d_tau, d_z, 0, d_y, d_proofs, d_g, n), a.reps)
        srs = hip.srs_g1_wrap_dev(d_proofs.data_ptr(), n)
        msm = median_ms(lambda: (hip.msm_g1_dev(srs, d_g.data_ptr(), n, d_out.data_ptr()), hip.synchronize()), a.reps)
        srs.free()
        pair2 = median_ms(lambda: (hip.pairing_batch_dev(d_proofs.data_ptr(), d_q.data_ptr(), 1, 2, d_gt.data_ptr()), hip.synchronize()), a.reps)
        # 2n pairings: proofs against tiled G2 points, in pieces of the tile
        def pair2n():
            done = 0
            while done < 2 * n:
                m = min(n_g2, 2 * n - done)
                hip.pairing_batch_dev(d_proofs.data_ptr() + (done % n) * 64, d_q.data_ptr(), 1, min(m, n - done % n), d_gt.data_ptr() + done * 384)
                done += min(m, n - done % n)
            hip.synchronize()
        p2n = median_ms(pair2n, max(3, a.reps // 4), warm=1)
        lines.append("%6d %9.3f %9.3f %9.3f %9.3f %9.3f %9.3f %9.3f %9.3f %10.3f %12.1f %11.1f" % (
            log2n, vec_host, vec_dev, gen_host, gen_dev, vec_host - vec_dev, msm, pair2, vec_dev - 2 * msm - pair2, p2n, p2n / vec_host,
            n * single / vec_host))
        print(lines[-1], flush=True)
    # crossover against single calls at small n (the mirror's kzg::verify_batch checks item by item below it)
    small = []
    for n in (1, 2, 3, 4, 6, 8, 16):
        small.append((n, median_ms(lambda: hip.kzg_verify_batch(coms[:1], tau_g2, zs[:n], ys[:n], proofs[:n], gs[:n]), a.reps)))
    lines.append("# small n, host form, one commitment: " + ", ".join("n=%d %.3f ms (n single: %.3f)" % (n, ms, n * single) for n, ms in small))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    hip.close()


def _g2_gen():
    """the affine G2 generator in the ABI's layout (Montgomery limbs of x.c0, x.c1, y.c0, y.c1)"""
    P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    c = [10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634,
         8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531]
    out = []
    for v in c:
        m = (v << 256) % P
        out += [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    return np.array(out, np.uint64)


if __name__ == "__main__":
    main()
