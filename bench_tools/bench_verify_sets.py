#!/usr/bin/env python3
"""KZG set batch verification (keaki_hip_kzg_verify_sets): n set proofs over arbitrary sets of k points, one commitment per item, rows of k
(item_stride k), point_mode 0 -- resident (_dev) and from host arrays, against

  (a) the only route the library had before: n calls of keaki_hip_kzg_verify_multi (host arrays; a G2 MSM, a G1 MSM and two pairings each). Timed on
      min(n, 64) calls and EXTRAPOLATED to n, labelled as such;
  (b) keaki_hip_kzg_verify_cosets_dev on coset-shaped inputs of the same n and k (rows, the shifts given): the floor -- the same amount of data with ONE
      G2 point for all items, two MSMs over the proofs instead of k + 1 and two pairings instead of k + 1 Miller loops.

Per shape ALL variants run in one process in alternating rounds, after warm-up rounds; the figures are medians over the rounds. Every call ends in a
device synchronisation (ok_out is a host pointer). The inputs are random on-curve points and random scalars: the verdict is 0, and no kernel of the
call has a path that depends on it. The points of an item are random Fr: distinct except with negligible probability.

The Fr kernels' and the GT product's own share is not visible from the host; --trace-only runs --reps resident calls of ONE shape and nothing else, to
be put under `rocprofv3 --kernel-trace --stats -- python ...` in a run of its own (k_vs_weights, k_vs_polys, k_vs_finish, k_gt_product in its kernel
statistics).

    python bench_tools/bench_verify_sets.py --out profiles/verify_sets_times.txt
    rocprofv3 --kernel-trace --stats --output-format csv -- python bench_tools/bench_verify_sets.py --trace-only --log2n 16 --k 8
"""
import argparse, faulthandler, os, statistics, sys, time
faulthandler.enable()
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import random_fr_limbs, SEED  # noqa: E402
from bench_tools.bench_verify_batch import _g2_gen  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ROOT_28 = pow(5, (R - 1) >> 28, R)
NS = [2, 64, 1 << 12, 1 << 16, 1 << 20]
KS = [2, 8, 64]
K_AT_2_20 = 8                       # n = 2^20 runs for k <= 8 only (n k < 2^31 would allow more; the inputs alone are 64 n k bytes)
POOL = 1 << 22                      # random Fr made once; larger inputs repeat them (whole items: the points of an item stay distinct)


def fr_mont(v):
    m = (v % R << 256) % R
    return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], np.uint64)


def omega(log2n):
    return pow(ROOT_28, 1 << (28 - log2n), R)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9); ap.add_argument("--warm", type=int, default=2); ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true"); ap.add_argument("--log2n", type=int, default=16); ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    hip = KeakiHip(0)
    shapes = [(1 << a.log2n, a.k)] if a.trace_only else [(n, k) for k in KS for n in NS if n < (1 << 20) or k <= K_AT_2_20]
    nmax = max(s[0] for s in shapes)
    emax = max(s[0] * s[1] for s in shapes)
    kmax = max(s[1] for s in shapes)
    P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    mont = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    g1 = np.array(mont(1) + mont(2), np.uint64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    sync = lambda: (hip.synchronize(), torch.cuda.synchronize(dev))
    # proofs and commitments (n of each) and the SRS points [tau^j]_1, j < kmax: multiples of g1 by random scalars, made on the device
    d_pts = torch.empty((2 * nmax + 64, 8), dtype=torch.int64, device=dev)
    d_g1, d_sc = t(g1), t(np.resize(random_fr_limbs(min(2 * nmax + 64, POOL), SEED + 41), (2 * nmax + 64, 4)))
    torch.cuda.synchronize(dev)
    hip.g1_mul_batch_dev(d_g1.data_ptr(), 0, d_sc.data_ptr(), 2 * nmax + 64, d_pts.data_ptr())
    sync()
    del d_sc
    pts = d_pts.cpu().numpy().view(np.uint64)
    proofs, coms = pts[:nmax], pts[nmax:2 * nmax]
    d_proofs, d_coms = d_pts[:nmax], d_pts[nmax:2 * nmax]
    srs1 = hip.srs_g1_upload(pts[2 * nmax:2 * nmax + max(kmax, 2)].copy())
    hip.srs_g1_precompute(srs1)
    g2s = hip.g2_mul_batch(_g2_gen(), random_fr_limbs(kmax + 1, SEED + 42))
    srs2 = hip.srs_g2_upload(g2s)
    pool_z, pool_y = random_fr_limbs(min(emax, POOL), SEED + 43), random_fr_limbs(min(emax, POOL), SEED + 44)
    points, values = np.resize(pool_z, (emax, 4)), np.resize(pool_y, (emax, 4))
    gammas = np.resize(random_fr_limbs(min(nmax, POOL), SEED + 45), (nmax, 4))
    d_points, d_values, d_gammas = t(points), t(values), t(gammas)
    sync()

    def variants(n, k):
        log2k = k.bit_length() - 1
        d_tau = t(g2s[k])
        sync()
        winv, linv = fr_mont(pow(omega(log2k), R - 2, R)), fr_mont(pow(k, R - 2, R))
        m = min(n, 64)

        def multi():
            for i in range(m):
                hip.kzg_verify_multi(srs1, srs2, coms[i], points[i * k:(i + 1) * k], values[i * k:(i + 1) * k], proofs[i])

        return m, {
            "dev": lambda: hip.kzg_verify_sets_dev(srs1, srs2, d_coms, 1, d_points, 0, None, d_values, k, k, d_proofs, d_gammas, n),
            "host": lambda: hip.kzg_verify_sets(srs1, srs2, coms[:n], points[:n * k], values[:n * k], k, proofs[:n], gammas[:n]),
            "cosets_dev": lambda: hip.kzg_verify_cosets_dev(srs1, d_coms, 1, d_tau, d_points, 0, d_values, k, 1, log2k, winv, linv, d_proofs, d_gammas, n),
            "multi": multi,
        }

    if a.trace_only:
        _, v = variants(*shapes[0])
        for _ in range(a.reps):
            v["dev"]()
        hip.close()
        return
    lines = ["# %s" % hip.version(),
             "# keaki_hip_kzg_verify_sets on n items of k points (one commitment per item, rows of k, point_mode 0): medians (ms) of %d alternating rounds" % a.rounds,
             "# in one process after %d warm-up rounds; every call ends in a device synchronisation" % a.warm,
             "# dev = _dev form, host = from host arrays; cosets_dev = keaki_hip_kzg_verify_cosets_dev on coset-shaped inputs of the same n and k (baseline b, the floor)",
             "# multi_m = m = min(n, 64) calls of keaki_hip_kzg_verify_multi, measured; multi_n = multi_m * n / m: n calls, EXTRAPOLATED for n > 64 (baseline a, the",
             "# parent's only route)",
             "%8s %4s %9s %9s %11s %4s %10s %13s %11s %11s" % ("n", "k", "dev", "host", "cosets_dev", "m", "multi_m", "multi_n(ex)", "multi_n/dev", "dev/cosets")]
    for n, k in shapes:
        m, v = variants(n, k)
        ts = {name: [] for name in v}
        for rnd in range(a.warm + a.rounds):
            for name, f in v.items():
                if name == "multi" and rnd not in (0, a.warm, a.warm + a.rounds - 1) and m > 8:
                    continue                                   # 64 calls of 8 - 9 ms: three rounds of them, not nine
                t0 = time.perf_counter()
                f()
                dt = (time.perf_counter() - t0) * 1e3
                if rnd >= a.warm:
                    ts[name].append(dt)
        md = {name: statistics.median(x) for name, x in ts.items()}
        multi_n = md["multi"] * n / m
        lines.append("%8d %4d %9.3f %9.3f %11.3f %4d %10.2f %13.1f %11.2f %11.2f" % (n, k, md["dev"], md["host"], md["cosets_dev"], m, md["multi"], multi_n,
                                                                                   multi_n / md["dev"], md["dev"] / md["cosets_dev"]))
        print(lines[-1], flush=True)
    # the smallest n at which the call beats n calls of verify_multi, per k: both measured, nothing extrapolated
    for k in KS:
        won = None
        for n in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64):
            _, v = variants(n, k)
            for _ in range(a.warm):
                v["host"](); v["multi"]()
            th, tm = [], []
            for _ in range(max(a.rounds // 2, 3)):
                t0 = time.perf_counter(); v["host"](); th.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter(); v["multi"](); tm.append((time.perf_counter() - t0) * 1e3)
            h, mm = statistics.median(th), statistics.median(tm)
            lines.append("# k = %d, n = %d: host form %.3f ms, n verify_multi calls %.3f ms (measured)%s" % (k, n, h, mm, "" if h < mm else "  LOSES"))
            print(lines[-1], flush=True)
            if h < mm and won is None:
                won = n
            if won is not None and n >= 2 * won:
                break
        lines.append("# k = %d: the smallest n tried at which the call beats n calls of verify_multi: %s" % (k, won))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    srs1.free(); srs2.free()
    hip.close()


if __name__ == "__main__":
    main()
