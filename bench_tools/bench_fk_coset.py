#!/usr/bin/env python3
"""keaki_hip_open_fk_cosets_poly (all r = d / l set proofs of the l-point cosets in one call) against the routes the library offered before it for
the same r proofs:
  (a) keaki_hip_open_fk_poly (all d single proofs) + r x keaki_hip_kzg_aggregate_dev, one per coset;
  (b) r x keaki_hip_kzg_open_multi_dev, one full MSM over the polynomial per coset;
  (c) keaki_hip_open_fk_poly alone at the same d (the prediction to test: the coset call comes in under it for l >= 4).
Where r > 64 the per-coset calls of (a) and (b) are timed over 64 cosets and EXTRAPOLATED to r (x r / 64); those figures carry a `~`.

One device, one process. Per shape the routes ALTERNATE round by round; every measurement is a host clock around whole calls that ends in a device
synchronisation; a figure is the median of its rounds (at least three, at least 0.3 s of timed work) after one warm-up round of each. The cache of
the handle (the l transforms of the SRS rows) is warm in every timed call and its build is timed on its own (a fresh key each time). "resident": the
coefficients and the proofs are device buffers (_dev); "host": numpy arrays.
Where the time goes: the device events of keaki_hip_set_timing around the pointwise kernel and the tail (keaki_hip_last_fk_ms: pointwise | gather + the
two transforms | whole pipeline behind the scalar transforms), for the shipped plan, for one ladder per term (option fk_coset_group = 1: the evidence
that the shared doubling chain pays), and for the unsplit launch (option fk_coset_min_lanes = 1) against the split ones (the threshold's evidence).

The SRS is random points (timing does not depend on their discrete logs); the handle has window tables, as in bench.py.

    python bench_tools/bench_fk_coset.py --out profiles/fk_coset_times.txt [--log2d 12,16,20] [--ls 4,16,64]
"""
import argparse, faulthandler, math, os, statistics, subprocess, sys, time
faulthandler.enable()
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import random_fr_limbs, SEED  # noqa: E402

MIN_TIMED_S = 0.3
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
SAMPLE = 64


def fr_mont(v):
    return np.array([((v << 256) % R_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], np.uint64)


def omega(n):
    return pow(pow(5, (R_MOD - 1) >> 28, R_MOD), (1 << 28) // n, R_MOD)


def domain(n):
    """(omega_n, 1 / omega_n, 1 / n) in Montgomery limbs"""
    w = omega(n)
    return fr_mont(w), fr_mont(pow(w, R_MOD - 2, R_MOD)), fr_mont(pow(n, R_MOD - 2, R_MOD))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2d", default="12,16,20")
    ap.add_argument("--ls", default="4,16,64")
    a = ap.parse_args()
    import torch
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    hip = KeakiHip(0)
    logs = [int(x) for x in a.log2d.split(",")]
    ls = [int(x) for x in a.ls.split(",")]
    d_max = 1 << max(logs)
    mont_q = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    g1 = np.array(mont_q(1) + mont_q(2), np.uint64)
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
    say("# bench_tools/bench_fk_coset.py -- parent commit %s + the coset openings; library %s" % (commit or "?", hip.lib.keaki_hip_version().decode()))
    say("# device: %s, one process, medians of alternating rounds, ms; `~`: extrapolated from %d cosets to r" % (torch.cuda.get_device_name(0), SAMPLE))
    coeffs = random_fr_limbs(d_max, SEED + 61)
    srs_pts = hip.g1_mul_batch(g1, np.roll(coeffs, 7, axis=0))
    srs = hip.srs_g1_upload(srs_pts)
    hip.srs_g1_precompute(srs)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    d_coeffs = up(coeffs)
    d_out = torch.zeros(8 * d_max, dtype=torch.int64, device=dev)
    d_proof, d_vals = torch.zeros(12, dtype=torch.int64, device=dev), torch.zeros(4 * max(ls), dtype=torch.int64, device=dev)
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

    def events(f, rounds=5):
        """medians of the device events of `rounds` calls: (pointwise, tail, pipeline)"""
        hip.set_timing(True)
        got = []
        for _ in range(rounds):
            f(); hip.synchronize()
            s = hip.last_fk_stats()
            got.append((s["pointwise_ms"], s["stages_ms"], s["device_ms"]))
        hip.set_timing(False)
        return tuple(statistics.median(x[i] for x in got) for i in range(3))

    say("# d, l, r | cosets resident | cosets host | (c) open_fk_poly resident | host | (a) open_fk_poly + r x aggregate_dev | (b) r x open_multi_dev |"
        " c / new | a / new | b / new || cache build")
    say("# events: pointwise | tail | pipeline, shipped plan (G = 4) || G = 1 || unsplit launch (one lane per position)")
    for lg in logs:
        d = 1 << lg
        w2d = domain(2 * d)
        wd = omega(d)
        for l in ls:
            if l > d:
                continue
            log2l, r = l.bit_length() - 1, d // l
            w2r = domain(2 * r)
            co_host = coeffs[:d]
            m = min(r, SAMPLE)
            # the points of the first m cosets, coset after coset: omega_d^(i + t r)
            pts = np.stack([fr_mont(pow(wd, i + t * r, R_MOD)) for i in range(m) for t in range(l)])
            d_pts = up(pts)
            d_sel = up(srs_pts[:l])                         # l affine points in place of a coset's single proofs
            torch.cuda.synchronize()

            def new_dev():
                hip.open_fk_cosets_poly_dev(srs, lg, log2l, d_coeffs.data_ptr(), *w2r, d_out.data_ptr())

            def new_host():
                hip.open_fk_cosets_poly(srs, lg, log2l, co_host, *w2r)

            def fk_dev():
                hip.open_fk_poly_batch_dev(srs, lg, d_coeffs.data_ptr(), 1, d, *w2d, d_out.data_ptr())

            def fk_host():
                hip.open_fk_poly(srs, lg, co_host, *w2d)

            def agg():
                for i in range(m):
                    hip.kzg_aggregate_dev(d_pts.data_ptr() + 32 * l * i, d_sel.data_ptr(), l, d_proof.data_ptr())

            def multi():
                for i in range(m):
                    hip.kzg_open_multi_dev(srs, d_coeffs.data_ptr(), d, d_pts.data_ptr() + 32 * l * i, l, d_proof.data_ptr(), d_vals.data_ptr())

            # the cache build on its own: another key first, so that the precompute call rebuilds
            builds = []
            for _ in range(3):
                hip.srs_g1_precompute_fk_cosets(srs, lg, log2l + 1, domain(r)[0])
                builds.append(timed(lambda: hip.srs_g1_precompute_fk_cosets(srs, lg, log2l, w2r[0])))
            t = alternate({"new": new_dev, "host": new_host, "fk": fk_dev, "fkh": fk_host, "agg": agg, "multi": multi})
            scale, mark = r / m, "~" if r > m else " "
            ra, rb = t["fkh"] + t["agg"] * scale, t["multi"] * scale
            say("2^%-2d l=%-3d r=%-7d %9.3f %9.3f | %9.3f %9.3f | %s%11.3f | %s%12.3f | %6.2fx %8.2fx %9.2fx || %9.3f" % (
                lg, l, r, t["new"], t["host"], t["fk"], t["fkh"], mark, ra, mark, rb, t["fk"] / t["new"], ra / t["host"], rb / t["new"], statistics.median(builds) * 1e3))
            e4 = events(new_dev)
            hip.set_option("fk_coset_group", 1)
            e1 = events(new_dev)
            hip.set_option("fk_coset_group", 0)
            hip.set_option("fk_coset_min_lanes", 1)
            eu = events(new_dev)
            hip.set_option("fk_coset_min_lanes", 0)
            say("  events 2^%-2d l=%-3d  %8.3f %8.3f %8.3f || %8.3f %8.3f %8.3f || %8.3f %8.3f %8.3f" % ((lg, l) + e4 + e1 + eu))
            del d_pts, d_sel
    # the split threshold: the same call with option fk_coset_min_lanes from 2^14 to 2^19 (S doubles while 2r S stays below it and a lane keeps 4 terms)
    say("# threshold sweep: d, l, 2r | for fk_coset_min_lanes = 2^14 .. 2^19: S: pointwise + tail (events)")
    for lg in logs:
        for l in ls:
            d, log2l = 1 << lg, l.bit_length() - 1
            if l > d or lg < 16:
                continue
            n2, w2r, row = 2 * d // l, domain(2 * d // l), []
            for e in range(14, 20):
                s = 1
                while n2 * s < (1 << e) and l // (2 * s) >= min(4, l):
                    s *= 2
                hip.set_option("fk_coset_min_lanes", 1 << e)
                ev = events(lambda: hip.open_fk_cosets_poly_dev(srs, lg, log2l, d_coeffs.data_ptr(), *w2r, d_out.data_ptr()), rounds=3)
                row.append("S=%-2d %7.3f+%7.3f" % (s, ev[0], ev[1]))
            hip.set_option("fk_coset_min_lanes", 0)
            say("  sweep 2^%-2d l=%-3d 2r=2^%-2d  %s" % (lg, l, n2.bit_length() - 1, " | ".join(row)))
    srs.free(); hip.close()


if __name__ == "__main__":
    main()
