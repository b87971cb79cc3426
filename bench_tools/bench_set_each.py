#!/usr/bin/env python3
"""KZG set pairs and per-set verdicts (keaki_hip_kzg_set_pairs, keaki_hip_kzg_verify_sets_each): n items of k arbitrary points, one commitment per item,
rows of k (item_stride k), point_mode 0 -- resident (_dev) and from host arrays, against

  (a) the only route the library had before: n calls of keaki_hip_kzg_verify_multi. Timed on min(n, 64) calls and EXTRAPOLATED to n, labelled as such;
  (b) keaki_hip_kzg_verify_sets_dev on the same items: the floor (one verdict for the batch);
  (c) keaki_hip_kzg_verify_cosets_each_dev on coset-shaped inputs of the same n and k: the per-item call whose G2 point is shared.

Per shape ALL variants run in one process in alternating rounds, after warm-up rounds; the figures are medians over the rounds. Every timed call ends in
a device synchronisation. The inputs are random on-curve points and random scalars: every verdict is 1 (invalid), and no kernel has a path that depends
on it. Then the sweeps that the defaults of csrc/set_rows_plan.h rest on: the G2 table widths 8 / 10 / 13 (set_rows_wb; 13 bits only where the table
stays under the plan's 512 MiB) and the slice threshold (set_rows_min_lanes), on keaki_hip_kzg_set_pairs_dev; and the table build of a first call,
timed on a fresh handle (keaki_hip_srs_g2_precompute_sets + synchronise).

    python bench_tools/bench_set_each.py --out profiles/set_each_times.txt
"""
import argparse, faulthandler, os, statistics, sys, time
faulthandler.enable()
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import random_fr_limbs, SEED  # noqa: E402
from bench_tools.bench_verify_batch import _g2_gen  # noqa: E402
from bench_tools.bench_verify_sets import fr_mont, omega, R  # noqa: E402

NS = [2, 64, 1 << 12, 1 << 16]
KS = [2, 8, 64]
POOL = 1 << 22
TABLE_CAP = 512 << 20


def table_bytes(k, wb):
    windows = (254 + wb - 1) // wb + (1 if 254 % wb == 0 else 0)
    return windows * ((1 << (wb - 1)) + 1) * k * 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--warm", type=int, default=1); ap.add_argument("--out", default=None)
    ap.add_argument("--nmax", type=int, default=1 << 16)
    ap.add_argument("--routes", action="store_true", help="only the two routes of verify_sets_each at k = 2, n = 2^13 .. 2^20: where the fused kernel would have to win")
    a = ap.parse_args()
    import torch
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    hip = KeakiHip(0)
    route_ns = [1 << e for e in (13, 14, 15, 17, 18, 20)]
    shapes = [(n, 2) for n in route_ns] if a.routes else [(n, k) for k in KS for n in NS if n <= a.nmax]
    nmax, kmax = max(s[0] for s in shapes), max(s[1] for s in shapes)
    emax = max(s[0] * s[1] for s in shapes)
    P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    mont = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    g1 = np.array(mont(1) + mont(2), np.uint64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    sync = lambda: (hip.synchronize(), torch.cuda.synchronize(dev))
    d_pts = torch.empty((2 * nmax + 64, 8), dtype=torch.int64, device=dev)
    d_g1, d_sc = t(g1), t(np.resize(random_fr_limbs(min(2 * nmax + 64, POOL), SEED + 51), (2 * nmax + 64, 4)))
    torch.cuda.synchronize(dev)
    hip.g1_mul_batch_dev(d_g1.data_ptr(), 0, d_sc.data_ptr(), 2 * nmax + 64, d_pts.data_ptr())
    sync()
    del d_sc
    pts = d_pts.cpu().numpy().view(np.uint64)
    proofs, coms = pts[:nmax], pts[nmax:2 * nmax]
    d_proofs, d_coms = d_pts[:nmax], d_pts[nmax:2 * nmax]
    srs_pts = pts[2 * nmax:2 * nmax + 64].copy()
    srs1 = hip.srs_g1_upload(srs_pts)
    hip.srs_g1_precompute(srs1)
    g2s = hip.g2_mul_batch(_g2_gen(), random_fr_limbs(kmax + 1, SEED + 52))
    srs2 = hip.srs_g2_upload(g2s)
    pool_z, pool_y = random_fr_limbs(min(emax, POOL), SEED + 53), random_fr_limbs(min(emax, POOL), SEED + 54)
    points, values = np.resize(pool_z, (emax, 4)), np.resize(pool_y, (emax, 4))
    gammas = np.resize(random_fr_limbs(min(nmax, POOL), SEED + 55), (nmax, 4))
    d_points, d_values, d_gammas = t(points), t(values), t(gammas)
    d_status = torch.zeros(nmax, dtype=torch.uint8, device=dev)
    d_a, d_z = torch.zeros(nmax * 8, dtype=torch.int64, device=dev), torch.zeros(nmax * 16, dtype=torch.int64, device=dev)
    sync()

    def timed(f):
        t0 = time.perf_counter()
        f()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def variants(n, k):
        log2k = k.bit_length() - 1
        d_tau = t(g2s[k])
        sync()
        winv, linv = fr_mont(pow(omega(log2k), R - 2, R)), fr_mont(pow(k, R - 2, R))
        m = min(n, 64)

        def multi():
            for i in range(m):
                hip.kzg_verify_multi(srs1, srs2, coms[i], points[i * k:(i + 1) * k], values[i * k:(i + 1) * k], proofs[i])

        def each_dev(route):
            def f():
                hip.set_option("set_each_route", route)
                hip.kzg_verify_sets_each_dev(srs1, srs2, d_coms, 1, d_points, 0, None, d_values, k, k, d_proofs, n, d_status)
            return f

        return m, {
            "pairs_dev": lambda: hip.kzg_set_pairs_dev(srs1, srs2, d_coms, 1, d_points, 0, None, d_values, k, k, n, d_a, d_z),
            "pairs_host": lambda: hip.kzg_set_pairs(srs1, srs2, coms[:n], points[:n * k], values[:n * k], k, n),
            "each_dev": each_dev(2),
            "each_r1": each_dev(1),
            "each_host": lambda: (hip.set_option("set_each_route", 0), hip.kzg_verify_sets_each(srs1, srs2, coms[:n], points[:n * k], values[:n * k], k, proofs[:n])),
            "sets_dev": lambda: hip.kzg_verify_sets_dev(srs1, srs2, d_coms, 1, d_points, 0, None, d_values, k, k, d_proofs, d_gammas, n),
            "cosets_each": lambda: hip.kzg_verify_cosets_each_dev(srs1, d_coms, 1, d_tau, d_points, 0, d_values, k, 1, log2k, winv, linv, d_proofs, n, d_status),
            "multi": multi,
        }

    if a.routes:
        out = ["# %s" % hip.version(), "# keaki_hip_kzg_verify_sets_each_dev at k = 2, set_each_route 1 (fused) against 2 (two Miller loops per item): medians (ms) of %d rounds" % a.rounds,
               "%8s %9s %9s" % ("n", "route 1", "route 2")]
        for n, k in shapes:
            _, v = variants(n, k)
            ts = {"each_r1": [], "each_dev": []}
            for rnd in range(a.warm + a.rounds):
                for name in ts:
                    dt = timed(v[name])
                    if rnd >= a.warm:
                        ts[name].append(dt)
            out.append("%8d %9.3f %9.3f" % (n, statistics.median(ts["each_r1"]), statistics.median(ts["each_dev"])))
            print(out[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(out) + "\n")
        srs1.free(); srs2.free()
        hip.close()
        return
    lines = ["# %s" % hip.version(),
             "# keaki_hip_kzg_set_pairs / keaki_hip_kzg_verify_sets_each on n items of k points (one commitment per item, rows of k, point_mode 0): medians (ms) of",
             "# %d alternating rounds in one process after %d warm-up rounds; every timed call ends in a device synchronisation. Tables by plan (k = 2, 8: 13 bits," % (a.rounds, a.warm),
             "# k = 64: 10 bits), built before the rounds. pairs = set_pairs, each = verify_sets_each (by plan: route 2, two Miller loops per item), each_r1 = route 1 (the fused",
             "# kernel); dev = _dev form, host = from host arrays; sets_dev = keaki_hip_kzg_verify_sets_dev on the same items (the floor: ONE verdict); cosets_each =",
             "# keaki_hip_kzg_verify_cosets_each_dev on coset-shaped inputs of the same n and k; multi_m = m = min(n, 64) calls of keaki_hip_kzg_verify_multi, measured;",
             "# multi_n = multi_m * n / m: n calls, EXTRAPOLATED for n > 64",
             "%8s %4s %9s %10s %9s %9s %9s %9s %11s %4s %9s %13s %9s" % ("n", "k", "pairs_dev", "pairs_host", "each_dev", "each_r1", "each_host", "sets_dev", "cosets_each", "m",
                                                                         "multi_m", "multi_n(ex)", "multi/each")]
    for n, k in shapes:
        m, v = variants(n, k)
        ts = {name: [] for name in v}
        for rnd in range(a.warm + a.rounds):
            for name, f in v.items():
                if name == "multi" and rnd not in (0, a.warm, a.warm + a.rounds - 1) and m > 8:
                    continue
                dt = timed(f)
                if rnd >= a.warm:
                    ts[name].append(dt)
        md = {name: statistics.median(x) for name, x in ts.items()}
        multi_n = md["multi"] * n / m
        lines.append("%8d %4d %9.3f %10.3f %9.3f %9.3f %9.3f %9.3f %11.3f %4d %9.2f %13.1f %9.1f" % (
            n, k, md["pairs_dev"], md["pairs_host"], md["each_dev"], md["each_r1"], md["each_host"], md["sets_dev"], md["cosets_each"], m, md["multi"], multi_n,
            multi_n / md["each_dev"]))
        print(lines[-1], flush=True)
        for name, other in (("each_dev", "sets_dev"), ("each_dev", "cosets_each"), ("each_dev", "each_r1")):
            if md[name] > md[other]:
                lines.append("#   n = %d, k = %d: %s LOSES to %s (%.2f x)" % (n, k, name, other, md[name] / md[other]))
    hip.set_option("set_each_route", 0)

    # ---- the sweeps: widths and the slice threshold, on set_pairs_dev ----
    lines.append("# width sweep (set_rows_wb) on set_pairs_dev, ms; '-': the table would exceed the plan's 512 MiB and was not built")
    lines.append("%8s %4s %9s %9s %9s   %s" % ("n", "k", "wb=8", "wb=10", "wb=13", "table MB at 8 / 10 / 13"))
    for n, k in [(s, kk) for kk in KS for s in (1 << 12, 1 << 16) if s <= a.nmax]:
        row = []
        for wb in (8, 10, 13):
            if table_bytes(k, wb) > TABLE_CAP:
                row.append(None)
                continue
            hip.set_option("set_rows_wb", wb)
            f = lambda: hip.kzg_set_pairs_dev(srs1, srs2, d_coms, 1, d_points, 0, None, d_values, k, k, n, d_a, d_z)
            timed(f)
            row.append(statistics.median([timed(f) for _ in range(a.rounds)]))
        lines.append("%8d %4d %9s %9s %9s   %.1f / %.1f / %.1f" % ((n, k) + tuple("-" if x is None else "%.3f" % x for x in row) + tuple(table_bytes(k, w) / 1e6 for w in (8, 10, 13))))
        print(lines[-1], flush=True)
    hip.set_option("set_rows_wb", 0)
    lines.append("# slice threshold sweep (set_rows_min_lanes) on set_pairs_dev at the plan's width, ms; 1 = never split")
    lanes = [1, 1 << 14, 1 << 16, 1 << 17, 1 << 18, 1 << 20]
    lines.append("%8s %4s " % ("n", "k") + " ".join("%9s" % ("2^%d" % (x.bit_length() - 1) if x > 1 else "1") for x in lanes))
    for n, k in [(64, 64), (1 << 12, 8), (1 << 12, 64), (1 << 16, 8)]:
        if n > a.nmax:
            continue
        row = []
        for ln in lanes:
            hip.set_option("set_rows_min_lanes", ln)
            f = lambda: hip.kzg_set_pairs_dev(srs1, srs2, d_coms, 1, d_points, 0, None, d_values, k, k, n, d_a, d_z)
            timed(f)
            row.append(statistics.median([timed(f) for _ in range(a.rounds)]))
        lines.append("%8d %4d " % (n, k) + " ".join("%9.3f" % x for x in row))
        print(lines[-1], flush=True)
    hip.set_option("set_rows_min_lanes", 0)
    # ---- the table build of a first call ----
    lines.append("# table build on a fresh G2 handle (keaki_hip_srs_g2_precompute_sets + synchronise), ms: k, width, MB, build")
    for k in KS:
        for wb in (8, 10, 13):
            if table_bytes(k, wb) > TABLE_CAP:
                continue
            h = hip.srs_g2_upload(g2s)
            hip.set_option("set_rows_wb", wb)
            dt = timed(lambda: hip.srs_g2_precompute_sets(h, k))
            h.free()
            lines.append("#   k = %2d  wb = %2d  %7.1f MB  %8.3f ms" % (k, wb, table_bytes(k, wb) / 1e6, dt))
            print(lines[-1], flush=True)
    hip.set_option("set_rows_wb", 0)
    lines.append("# the two routes of verify_sets_each at larger n: python bench_tools/bench_set_each.py --routes (appended below when run)")
    lines.append("# NOT MEASURED here: vec_encrypt_subsets against n encrypt_set calls")
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    srs1.free(); srs2.free()
    hip.close()


if __name__ == "__main__":
    main()
