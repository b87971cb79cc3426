#!/usr/bin/env python3
"""vec_update (keaki_hip_vec_update: k evaluations of a committed vector change, commitment and all d proofs follow) against committing afresh,
at d = 2^12, 2^16, 2^20 and k = 1, 4, 16, 64, 256, all in ONE process on one SRS handle with window tables:

  commit_host   keaki_hip_vec_commit from host arrays: the baseline, the code path every caller had before vec_update existed
  commit_dev    the same pipeline on resident arrays (keaki_hip_vec_commit_batch_dev with one row)
  upd_dev k     keaki_hip_vec_update_dev, indices / deltas / commitment / proofs resident
  upd_host k    keaki_hip_vec_update from host arrays (upload of k entries + 96 B + d x 64 B, download of 96 B + d x 64 B)

Per d: the table build is timed once (keaki_hip_srs_g1_precompute_update on a handle without tables), then two warm-up rounds, then --reps
rounds; a round runs every candidate once and the order is reversed from round to round. Every timed call ends in a device synchronisation.
Medians, minima and maxima in ms: the (min .. max) range is the spread a margin has to exceed. Every round updates the SAME starting
(commitment, proofs): the resident buffers are restored by a device copy outside the timed window. The k = 1 result is compared with
vec_commit of the changed vector before anything is timed.

    python bench_tools/bench_vec_update.py --out profiles/vec_update_times.txt
"""
import argparse, faulthandler, os, statistics, sys, time
faulthandler.enable()
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import random_fr_limbs, SEED  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def fr_mont(v):
    v = (v % R << 256) % R
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], np.uint64)


def fr_int(limbs):
    return sum(int(x) << (64 * i) for i, x in enumerate(limbs)) * pow(1 << 256, -1, R) % R


def root_of_unity(n):
    return pow(pow(5, (R - 1) >> 28, R), (1 << 28) // n, R)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2d", type=int, nargs="+", default=[12, 16, 20]); ap.add_argument("--k", type=int, nargs="+", default=[1, 4, 16, 64, 256])
    ap.add_argument("--reps", type=int, default=0, help="rounds per d; 0 = 15 / 9 / 5 by size")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    hip = KeakiHip(0)
    nmax, kmax = 1 << max(a.log2d), max(a.k)
    P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    qmont = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    t = lambda x, dt=np.int64: torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev)
    sync = lambda: (hip.synchronize(), torch.cuda.synchronize(dev))
    d_pts = torch.empty((nmax, 8), dtype=torch.int64, device=dev)
    d_g1, d_sc = t(np.array(qmont(1) + qmont(2), np.uint64)), t(random_fr_limbs(nmax, SEED + 31))
    hip.g1_mul_batch_dev(d_g1.data_ptr(), 0, d_sc.data_ptr(), nmax, d_pts.data_ptr())
    sync()
    pts = d_pts.cpu().numpy().view(np.uint64)
    srs = hip.srs_g1_upload(pts)
    hip.srs_g1_precompute(srs)
    evals_all = random_fr_limbs(nmax, SEED + 32)
    deltas = random_fr_limbs(kmax, SEED + 33)
    lines = ["# %s" % hip.version(),
             "# keaki_hip_vec_update against keaki_hip_vec_commit at the same d, ms; per d: two warm-up rounds, then `rounds` rounds of every candidate once, order",
             "# reversed from round to round, one process, one SRS handle with window tables, every call ending in a device synchronisation. median (min .. max).",
             "# commit_host = vec_commit from host arrays (the baseline) | commit_dev = the same pipeline resident (vec_commit_batch_dev, one row) |",
             "# upd_dev / upd_host k = vec_update of k entries, resident / from host arrays. The ratios are medians: commit / update.",
             "# tables = keaki_hip_srs_g1_precompute_update on a fresh handle (192 B x d)"]
    for log2d in a.log2d:
        d = 1 << log2d
        rounds = a.reps or (15 if log2d <= 12 else 9 if log2d <= 17 else 5)
        w, w2 = root_of_unity(d), root_of_unity(2 * d)
        uc = [fr_mont(x) for x in (w, pow(w, -1, R), pow(d, -1, R))]
        cc = [fr_mont(x) for x in (pow(w, -1, R), pow(d, -1, R), w2, pow(w2, -1, R), pow(2 * d, -1, R))]
        evals = np.ascontiguousarray(evals_all[:d])
        rng = np.random.default_rng(SEED + log2d)
        idx_all = rng.integers(0, d, size=kmax, dtype=np.uint32)
        # table build on a handle of its own (the timed handle keeps its tables for the rounds)
        fresh = hip.srs_g1_upload(pts[:d])
        before = hip.memory()["tables"]
        build_ms = timed(lambda: hip.srs_g1_precompute_update(fresh, log2d, *uc))
        table_bytes = hip.memory()["tables"] - before
        fresh.free()
        com0, pr0 = hip.vec_commit(srs, evals, None, log2d, *cc)
        # correctness at this size before timing: one change, against committing the changed vector
        chk = evals.copy()
        chk[idx_all[0]] = fr_mont(fr_int(evals[idx_all[0]]) + fr_int(deltas[0]))
        e_com, e_pr = hip.vec_commit(srs, chk, None, log2d, *cc)
        g_com, g_pr = hip.vec_update(srs, log2d, *uc, idx_all[:1], deltas[:1], com0.copy(), pr0.copy())
        if not (np.array_equal(g_com, e_com) and np.array_equal(g_pr, e_pr)):
            raise SystemExit("vec_update differs from vec_commit of the changed vector at d = 2^%d" % log2d)
        d_ev, d_idx, d_dl = t(evals), t(idx_all, np.int32), t(deltas)
        d_com0, d_pr0 = t(com0), t(pr0)
        d_com, d_pr = d_com0.clone(), d_pr0.clone()
        d_cc, d_cp = torch.empty(12, dtype=torch.int64, device=dev), torch.empty((d, 8), dtype=torch.int64, device=dev)
        h_com, h_pr = com0.copy(), pr0.copy()
        sync()

        def restore():
            d_com.copy_(d_com0); d_pr.copy_(d_pr0); h_com[:] = com0; h_pr[:] = pr0
            torch.cuda.synchronize(dev)

        names = ["commit_host", "commit_dev"] + ["upd_dev %d" % k for k in a.k] + ["upd_host %d" % k for k in a.k]
        cands = [lambda: hip.vec_commit(srs, evals, None, log2d, *cc),
                 lambda: (hip.vec_commit_batch_dev(srs, d_ev.data_ptr(), d, 1, d, log2d, *cc, d_cc.data_ptr(), d_cp.data_ptr()), hip.synchronize())]
        cands += [lambda k=k: (hip.vec_update_dev(srs, log2d, *uc, d_idx.data_ptr(), d_dl.data_ptr(), k, d_com.data_ptr(), d_pr.data_ptr()), hip.synchronize()) for k in a.k]
        cands += [lambda k=k: hip.vec_update(srs, log2d, *uc, idx_all[:k], deltas[:k], h_com, h_pr) for k in a.k]
        ts = [[] for _ in cands]
        for r in range(2 + rounds):
            order = range(len(cands)) if r % 2 == 0 else reversed(range(len(cands)))
            for i in order:
                restore()
                ms = timed(cands[i])
                if r >= 2:
                    ts[i].append(ms)
        med = [statistics.median(x) for x in ts]
        nk = len(a.k)
        lines.append("d = 2^%d, rounds = %d, tables: %.1f ms, %d bytes" % (log2d, rounds, build_ms, table_bytes))
        for nm, x, m in zip(names, ts, med):
            lines.append("  %-14s %10.3f (%.3f .. %.3f)" % (nm, m, min(x), max(x)))
        # the baseline is keaki_hip_vec_commit (commit_host); commit_dev is the same pipeline without the copies (at d <= 2^12 a one-row batch takes the batch kernels)
        lines.append("  commit_host / upd_dev:  " + ", ".join("k=%d %.2fx" % (k, med[0] / med[2 + j]) for j, k in enumerate(a.k)))
        lines.append("  commit_host / upd_host: " + ", ".join("k=%d %.2fx" % (k, med[0] / med[2 + nk + j]) for j, k in enumerate(a.k)))
        lines.append("  commit_dev / upd_dev:   " + ", ".join("k=%d %.2fx" % (k, med[1] / med[2 + j]) for j, k in enumerate(a.k)))
        base_min = min(min(ts[0]), min(ts[1]))
        wins = [k for j, k in enumerate(a.k) if max(ts[2 + j]) < base_min and max(ts[2 + nk + j]) < base_min]
        lines.append("  update (both forms) faster than commit (both forms) in EVERY round, max update < min commit, at k = %s" % (wins or "none"))
        print("\n".join(lines[-(5 + len(names)):]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    srs.free()
    hip.close()


if __name__ == "__main__":
    main()
