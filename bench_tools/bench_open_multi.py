#!/usr/bin/env python3
"""keaki_hip_kzg_open_multi_dev (one proof for k points: the fused k-point quotient in front of ONE MSM) against the only route the library
offered before it: k single openings of the same polynomial (keaki_hip_kzg_open_batch_dev) and a k-term MSM of the results with the weights.

One device, one process, resident buffers. Per (n, k) the two routes ALTERNATE round by round; every measurement is a host clock around whole
calls that ends in a device synchronisation; a figure is the median of its rounds (at least three, at least 0.3 s of timed work) after one
warm-up round of each. Two old routes are timed. (a) k calls of keaki_hip_kzg_open from host arrays (the call kzg::open makes; it uploads the
coefficients inside every call, chunked under its kernels from 2^21 on) and the k-term combination. (b) The resident route: it runs kzg_open_batch_dev over k replicated rows up to n = 2^16 (its batch kernels) and, from 2^20 on, as k
calls with one row each over the SAME coefficients: rows that long run the single-MSM pipeline row by row inside the call anyway, and k copies
of 2^24 coefficients would be 32 GB. Its k-term combination (weights on the device, an MSM over the k proofs) is keaki_hip_kzg_aggregate_dev
preceded by the affine conversion it needs, which is NOT timed (in favour of the old route).
The quotient alone: open_multi_dev minus one keaki_hip_msm_g1_dev over the same n - 1 resident scalars (timed in the same rounds), at k and at
k = 1; "k x single" is k times the k = 1 figure -- the 1-point instantiation runs the recurrence of the single-point kernels plus one product per
coefficient, and the weighted sum the single route would need on top is left out (both in favour of the single route).
Also: keaki_hip_kzg_verify_multi against k keaki_hip_kzg_verify calls, and one decapsulation (what a set ciphertext costs) against k.

The SRS is random points (timing does not depend on their discrete logs); the handle has window tables, as in bench.py.

    python bench_tools/bench_open_multi.py --out profiles/open_multi_times.txt [--log2n 12,16,20,24] [--ks 2,8,64]
"""
import argparse, ctypes as C, faulthandler, math, os, statistics, subprocess, sys, time
faulthandler.enable()
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import random_fr_limbs, SEED  # noqa: E402

MIN_TIMED_S = 0.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2n", default="12,16,20,24")
    ap.add_argument("--ks", default="2,8,64")
    a = ap.parse_args()
    import torch
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    hip = KeakiHip(0)
    logs = [int(x) for x in a.log2n.split(",")]
    ks = [int(x) for x in a.ks.split(",")]
    n_max, k_max = 1 << max(logs), max(ks)
    P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    mont = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    g1 = np.array(mont(1) + mont(2), np.uint64)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    except OSError:
        commit = ""
    say("# bench_tools/bench_open_multi.py -- parent commit %s + the set openings; library %s" % (commit or "?", hip.lib.keaki_hip_version().decode()))
    say("# device: %s, one process, resident buffers, medians of alternating rounds, ms" % torch.cuda.get_device_name(0))
    coeffs = random_fr_limbs(n_max, SEED + 51)
    srs_pts = hip.g1_mul_batch(g1, np.roll(coeffs, 7, axis=0))
    srs = hip.srs_g1_upload(srs_pts)
    hip.srs_g1_precompute(srs)
    points = random_fr_limbs(k_max, SEED + 52)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    d_coeffs, d_points = up(coeffs), up(points)
    d_proof, d_vals = torch.zeros(12, dtype=torch.int64, device=dev), torch.zeros(4 * k_max, dtype=torch.int64, device=dev)
    d_proofs, d_vals2 = torch.zeros(12 * k_max, dtype=torch.int64, device=dev), torch.zeros(4 * k_max, dtype=torch.int64, device=dev)
    d_aff = up(srs_pts[:k_max])          # k affine points in place of the converted single proofs
    torch.cuda.synchronize()

    def timed(f):
        t0 = time.perf_counter()
        f()
        hip.synchronize()
        return time.perf_counter() - t0

    def alternate(variants):
        t = {k: [] for k in variants}
        first = {k: timed(f) for k, f in variants.items()}
        rounds = min(100, max(3, int(math.ceil(MIN_TIMED_S / max(min(first.values()), 1e-6)))))
        for _ in range(rounds):
            for k, f in variants.items():
                if sum(t[k]) >= MIN_TIMED_S and len(t[k]) >= 3:
                    continue
                t[k].append(timed(f))
        return {k: statistics.median(v) * 1e3 for k, v in t.items()}

    say("# open: n, k | open_multi_dev | (a) k x kzg_open from host arrays + k-term MSM | (b) k x open_batch_dev rows + k-term MSM | a / new | b / new"
        " || one msm_g1_dev of n - 1 | fused quotient alone (new - msm) | k x the 1-point quotient alone")
    d_q = up(np.roll(coeffs, 3, axis=0))
    torch.cuda.synchronize()
    val1, prf1 = np.zeros(4, np.uint64), np.zeros(12, np.uint64)
    for lg in logs:
        n = 1 << lg
        for k in ks:
            rep = None
            if lg <= 16:
                rep = up(np.broadcast_to(coeffs[:n], (k, n, 4)).copy())
                torch.cuda.synchronize()

            def new():
                hip.kzg_open_multi_dev(srs, d_coeffs.data_ptr(), n, d_points.data_ptr(), k, d_proof.data_ptr(), d_vals.data_ptr())

            def old():
                if rep is not None:
                    hip.kzg_open_batch_dev(srs, rep.data_ptr(), n, k, n, d_points.data_ptr(), d_proofs.data_ptr(), d_vals2.data_ptr())
                else:
                    for j in range(k):
                        hip.kzg_open_batch_dev(srs, d_coeffs.data_ptr(), n, 1, n, d_points.data_ptr() + 32 * j, d_proofs.data_ptr() + 96 * j, d_vals2.data_ptr() + 32 * j)
                hip.kzg_aggregate_dev(d_points.data_ptr(), d_aff.data_ptr(), k, d_proof.data_ptr())

            def old_host():
                for j in range(k):
                    hip._ck(hip.lib.keaki_hip_kzg_open(hip.ctx, srs.handle, coeffs.ctypes.data_as(C.c_void_p), n, points[j].ctypes.data_as(C.c_void_p),
                                                       prf1.ctypes.data_as(C.c_void_p), val1.ctypes.data_as(C.c_void_p)))
                hip.kzg_aggregate_dev(d_points.data_ptr(), d_aff.data_ptr(), k, d_proof.data_ptr())

            def one():
                hip.kzg_open_multi_dev(srs, d_coeffs.data_ptr(), n, d_points.data_ptr(), 1, d_proof.data_ptr(), d_vals.data_ptr())

            def msm():
                hip.msm_g1_dev(srs, d_q.data_ptr(), n - 1, d_proof.data_ptr())

            r = alternate({"new": new, "old": old, "host": old_host, "one": one, "msm": msm})
            say("open 2^%-2d k=%-3d  %9.3f  %10.3f  %10.3f  %6.2fx %7.2fx || %8.3f  %8.3f  %9.3f" % (lg, k, r["new"], r["host"], r["old"], r["host"] / r["new"],
                r["old"] / r["new"], r["msm"], r["new"] - r["msm"], k * (r["one"] - r["msm"])))
            del rep
    # verify_multi against k verify calls; one decapsulation against k (inputs need not verify: the same kernels run either way)
    g2 = _g2_points(hip, k_max + 1)
    srs2 = hip.srs_g2_upload(g2)
    com, proof = srs_pts[3], srs_pts[4]
    vals = random_fr_limbs(k_max, SEED + 53)
    say("# verify: k | verify_multi | k x kzg_verify || decapsulate: 1 item (a set ciphertext) | k calls of 1 item")
    for k in ks:
        r = alternate({"new": lambda: hip.kzg_verify_multi(srs, srs2, com, points[:k], vals[:k], proof),
                       "old": lambda: [hip.kzg_verify(com, g2[1], points[j], vals[j], proof) for j in range(k)]})
        d = alternate({"new": lambda: hip.decap_batch(srs_pts[5:6], g2[1:2]),
                       "old": lambda: [hip.decap_batch(srs_pts[5 + j:6 + j], g2[1:2]) for j in range(k)]})
        say("verify k=%-3d  %9.3f  %9.3f  %6.2fx || decap  %8.3f  %8.3f  %6.2fx" % (k, r["new"], r["old"], r["old"] / r["new"], d["new"], d["old"], d["old"] / d["new"]))
    srs.free(); srs2.free(); hip.close()


def _g2_points(hip, n):
    """n G2 points: random multiples of the generator"""
    Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    mont = lambda v: [((v << 256) % Q >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    gx = (10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634)
    gy = (8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531)
    g2 = np.array(mont(gx[0]) + mont(gx[1]) + mont(gy[0]) + mont(gy[1]), np.uint64)
    return hip.g2_mul_batch(g2, random_fr_limbs(n, SEED + 54))


if __name__ == "__main__":
    main()
