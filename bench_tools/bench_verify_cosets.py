#!/usr/bin/env python3
"""KZG coset batch verification (keaki_hip_kzg_verify_cosets) on all r = d / l cosets of one vector -- the form vec_verify_cosets calls: one
commitment, the evaluations in domain order (item_stride 1, t_stride r), point_mode 1 -- resident (_dev) and from host arrays, against

  (a) the only route the library had before: r calls of keaki_hip_kzg_verify_multi (host arrays; a G2 MSM, a G1 MSM and two pairings each). Timed on
      min(r, 64) calls and EXTRAPOLATED to r, labelled as such;
  (b) keaki_hip_kzg_verify_batch_dev on the same d values as d single openings (one commitment, point_mode 1): the nearest existing call over the
      same amount of data. It needs d proofs where the coset call needs r.

Per shape ALL variants run in one process in alternating rounds (call, verify_batch, call from host arrays, ... again), after warm-up rounds; the
figures are medians over the rounds. Every call ends in a device synchronisation (ok_out is a host pointer). The inputs are random on-curve points and
random scalars: the verdict is 0, and no kernel of the call has a path that depends on it.

The transform kernels' own share is not visible from the host; --trace-only runs --reps resident calls of ONE shape and nothing else, to be put under
`rocprofv3 --kernel-trace --stats -- python ...` in a run of its own (k_vc_prepare, k_vc_transform, k_vc_finish in its kernel statistics).

    python bench_tools/bench_verify_cosets.py --out profiles/verify_cosets_times.txt
    rocprofv3 --kernel-trace --stats --output-format csv -- python bench_tools/bench_verify_cosets.py --trace-only --log2d 20 --log2l 6
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
SHAPES = [(12, 2), (12, 4), (12, 6), (16, 2), (16, 4), (16, 6), (20, 2), (20, 4), (20, 6), (20, 10)]


def fr_mont(v):
    m = (v % R << 256) % R
    return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], np.uint64)


def omega(log2n):
    return pow(ROOT_28, 1 << (28 - log2n), R)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9); ap.add_argument("--warm", type=int, default=2); ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true"); ap.add_argument("--log2d", type=int, default=20); ap.add_argument("--log2l", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    hip = KeakiHip(0)
    shapes = [(a.log2d, a.log2l)] if a.trace_only else SHAPES
    dmax = 1 << max(s[0] for s in shapes)
    lmax = 1 << max(s[1] for s in shapes)
    P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    mont = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    g1 = np.array(mont(1) + mont(2), np.uint64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    sync = lambda: (hip.synchronize(), torch.cuda.synchronize(dev))
    # proofs (d of them: verify_batch needs one per value) and the SRS points [tau^j]_1, j < lmax: multiples of g1 by random scalars, made on the device
    d_proofs = torch.empty((dmax, 8), dtype=torch.int64, device=dev)
    hip.g1_mul_batch_dev(t(g1).data_ptr(), 0, t(random_fr_limbs(dmax, SEED + 31)).data_ptr(), dmax, d_proofs.data_ptr())
    sync()
    proofs = d_proofs.cpu().numpy().view(np.uint64)
    srs1 = hip.srs_g1_upload(proofs[:max(lmax, 2)].copy())
    hip.srs_g1_precompute(srs1)
    g2s = hip.g2_mul_batch(_g2_gen(), random_fr_limbs(lmax + 1, SEED + 32)) if not a.trace_only else hip.g2_mul_batch(_g2_gen(), random_fr_limbs(2, SEED + 32))
    srs2 = hip.srs_g2_upload(g2s)
    tau_l = g2s[-1]
    com = proofs[7:8].copy()
    evals, gammas = random_fr_limbs(dmax, SEED + 33), random_fr_limbs(dmax, SEED + 34)
    d_evals, d_gammas, d_com, d_tau = t(evals), t(gammas), t(com), t(tau_l)
    sync()

    def variants(log2d, log2l):
        d, l = 1 << log2d, 1 << log2l
        r = d // l
        wd = fr_mont(omega(log2d)).reshape(1, 4)
        d_wd = t(wd)
        winv, linv = fr_mont(pow(omega(log2l), R - 2, R)), fr_mont(pow(l, R - 2, R))
        k = min(r, 64)
        zs = random_fr_limbs(k * l, SEED + 35).reshape(k, l, 4)          # distinct points per call: verify_multi does not care that they form no coset
        ys = evals[:k * l].reshape(k, l, 4)

        def multi():
            for i in range(k):
                hip.kzg_verify_multi(srs1, srs2, com[0], zs[i], ys[i], proofs[i])

        return r, k, {
            "dev": lambda: hip.kzg_verify_cosets_dev(srs1, d_com, 0, d_tau, d_wd, 1, d_evals, 1, r, log2l, winv, linv, d_proofs, d_gammas, r),
            "host": lambda: hip.kzg_verify_cosets(srs1, com, tau_l, wd, evals[:d], 1, r, log2l, winv, linv, proofs[:r], gammas[:r], point_mode=1),
            "batch_dev": lambda: hip.kzg_verify_batch_dev(d_com, 0, d_tau, d_wd, 1, d_evals, d_proofs, d_gammas, d),
            "multi": multi,
        }

    if a.trace_only:
        _, _, v = variants(a.log2d, a.log2l)
        for _ in range(a.reps):
            v["dev"]()
        hip.close()
        return
    lines = ["# %s" % hip.version(),
             "# keaki_hip_kzg_verify_cosets on all r = d / l cosets of one vector (one commitment, domain order, point_mode 1): medians (ms) of %d alternating rounds"
             % a.rounds,
             "# in one process after %d warm-up rounds; every call ends in a device synchronisation" % a.warm,
             "# dev = _dev form, host = from host arrays; batch_dev = keaki_hip_kzg_verify_batch_dev on the same d values as d single openings (baseline b)",
             "# multi_k = k = min(r, 64) calls of keaki_hip_kzg_verify_multi, measured; multi_r = multi_k * r / k: r calls, EXTRAPOLATED (baseline a, the parent's only route)",
             "%6s %6s %7s %9s %9s %10s %4s %10s %12s %10s %10s" % ("log2d", "l", "r", "dev", "host", "batch_dev", "k", "multi_k", "multi_r(ex)", "multi_r/dev", "batch/dev")]
    for log2d, log2l in SHAPES:
        r, k, v = variants(log2d, log2l)
        ts = {name: [] for name in v}
        for rnd in range(a.warm + a.rounds):
            for name, f in v.items():
                if name == "multi" and rnd not in (0, a.warm, a.warm + a.rounds - 1) and k > 8:
                    continue                                   # 64 calls of 8 - 9 ms: three rounds of them, not nine
                t0 = time.perf_counter()
                f()
                dt = (time.perf_counter() - t0) * 1e3
                if rnd >= a.warm:
                    ts[name].append(dt)
        m = {name: statistics.median(x) for name, x in ts.items()}
        multi_r = m["multi"] * r / k
        lines.append("%6d %6d %7d %9.3f %9.3f %10.3f %4d %10.2f %12.1f %10.1f %10.2f" % (log2d, 1 << log2l, r, m["dev"], m["host"], m["batch_dev"], k, m["multi"], multi_r,
                                                                                     multi_r / m["dev"], m["batch_dev"] / m["dev"]))
        print(lines[-1], flush=True)
    # the smallest r: two cosets against two verify_multi calls
    for log2l in (2, 6, 10):
        r, k, v = variants(log2l + 1, log2l)
        for _ in range(a.warm):
            v["host"](); v["multi"]()
        th, tm = [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter(); v["host"](); th.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); v["multi"](); tm.append((time.perf_counter() - t0) * 1e3)
        lines.append("# r = 2, l = %d: host form %.3f ms, two verify_multi calls %.3f ms (measured, not extrapolated)" % (1 << log2l, statistics.median(th), statistics.median(tm)))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    srs1.free(); srs2.free()
    hip.close()


if __name__ == "__main__":
    main()
