#!/usr/bin/env python3
"""The per-item side of the KZG coset check on all r = d / l cosets of one vector (one commitment, the evaluations in domain order, point_mode 1):

  (a) keaki_hip_kzg_coset_pairs_dev with "coset_rows_route" 1 (the handle's window table) against 2 (the batched MSM over the rows), alternating, and the
      call from host arrays on the plan's route;
  (b) keaki_hip_kzg_verify_cosets_each_dev against the only route the library had before: r calls of keaki_hip_kzg_verify_multi, timed on min(r, 64)
      calls and EXTRAPOLATED to r, labelled as such; beside it keaki_hip_kzg_verify_cosets_dev on the same items, the floor (two pairings for all);
  (c) encryption to all cosets through the host layer (keaki.vec_encrypt_cosets) against r encrypt_set calls, min(r, 64) timed and EXTRAPOLATED
      (--encrypt; the KZGSetup is built for the largest d of --encrypt-log2d);
  (d) the sweeps behind the plan (--sweep): "coset_rows_min_lanes" (alternating rounds) and "coset_rows_wb" (one width after the other: a change of width
      rebuilds the handle's table) on route 1.

Per shape ALL variants run in one process in alternating rounds after warm-up rounds; the figures are medians over the rounds. The resident calls are
followed by a device synchronisation inside the timed span. The inputs are random on-curve points and random scalars: every verdict is "invalid", and
no kernel has a path that depends on it. --trace-only runs --reps resident calls of ONE shape and nothing else, to be put under
`rocprofv3 --kernel-trace --stats -- python ...` in a run of its own (k_vc_prepare, k_vc_transform, k_cp_rows, k_cp_affine in its statistics).

    python bench_tools/bench_coset_each.py --sweep --encrypt --out profiles/coset_each_times.txt
"""
import argparse, faulthandler, os, statistics, sys, time
faulthandler.enable()
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import random_fr_limbs, SEED  # noqa: E402
from bench_tools.bench_verify_batch import _g2_gen  # noqa: E402
from bench_tools.bench_verify_cosets import R, fr_mont, omega  # noqa: E402

SHAPES = [(12, 2), (12, 4), (12, 6), (16, 2), (16, 4), (16, 6), (20, 2), (20, 4), (20, 6), (20, 10)]


def timed(variants, warm, rounds, sparse=()):
    """medians (ms) of alternating rounds; the names in `sparse` run in three rounds only"""
    ts = {name: [] for name in variants}
    for rnd in range(warm + rounds):
        for name, f in variants.items():
            if name in sparse and rnd not in (0, warm, warm + rounds - 1):
                continue
            t0 = time.perf_counter()
            f()
            dt = (time.perf_counter() - t0) * 1e3
            if rnd >= warm:
                ts[name].append(dt)
    return {name: statistics.median(x) for name, x in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--warm", type=int, default=2); ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", action="store_true"); ap.add_argument("--encrypt", action="store_true"); ap.add_argument("--encrypt-log2d", type=int, nargs="*", default=[12, 16])
    ap.add_argument("--trace-only", action="store_true"); ap.add_argument("--log2d", type=int, default=20); ap.add_argument("--log2l", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--shapes", type=str, default=None, help="log2d:log2l,... instead of the built-in list")
    a = ap.parse_args()
    import torch
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    hip = KeakiHip(0)
    shapes = [(a.log2d, a.log2l)] if a.trace_only else ([tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")] if a.shapes else SHAPES)
    dmax = 1 << max(s[0] for s in shapes)
    lmax = 1 << max(s[1] for s in shapes)
    P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    mont = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    g1 = np.array(mont(1) + mont(2), np.uint64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    sync = lambda: (hip.synchronize(), torch.cuda.synchronize(dev))
    rmax = max(1 << (s[0] - s[1]) for s in shapes)
    npts = max(rmax, lmax, 64)
    d_proofs = torch.empty((npts, 8), dtype=torch.int64, device=dev)
    hip.g1_mul_batch_dev(t(g1).data_ptr(), 0, t(random_fr_limbs(npts, SEED + 31)).data_ptr(), npts, d_proofs.data_ptr())
    sync()
    proofs = d_proofs.cpu().numpy().view(np.uint64)
    srs1 = hip.srs_g1_upload(proofs[:max(lmax, 2)].copy())
    hip.srs_g1_precompute(srs1)
    g2s = hip.g2_mul_batch(_g2_gen(), random_fr_limbs((2 if a.trace_only else lmax + 1), SEED + 32))
    srs2 = hip.srs_g2_upload(g2s)
    tau_l = g2s[-1]
    com = proofs[7:8].copy()
    evals, gammas = random_fr_limbs(dmax, SEED + 33), random_fr_limbs(rmax, SEED + 34)
    d_evals, d_gammas, d_com, d_tau = t(evals), t(gammas), t(com), t(tau_l)
    d_a, d_c = torch.empty((rmax, 8), dtype=torch.int64, device=dev), torch.empty((rmax, 4), dtype=torch.int64, device=dev)
    d_status = torch.empty(rmax, dtype=torch.uint8, device=dev)
    sync()

    def opt(**kw):
        for k, v in kw.items():
            hip.set_option("coset_rows_" + k, v)

    def variants(log2d, log2l):
        d, l = 1 << log2d, 1 << log2l
        r = d // l
        wd = fr_mont(omega(log2d)).reshape(1, 4)
        d_wd = t(wd)
        winv, linv = fr_mont(pow(omega(log2l), R - 2, R)), fr_mont(pow(l, R - 2, R))
        k = min(r, 64)
        zs = random_fr_limbs(k * l, SEED + 35).reshape(k, l, 4)
        ys = evals[:k * l].reshape(k, l, 4)

        def pairs(route=0, **kw):
            def f():
                opt(route=route, **kw)
                hip.kzg_coset_pairs_dev(srs1, d_com, 0, d_wd, 1, d_evals, 1, r, log2l, winv, linv, r, d_a, d_c)
                sync()
                opt(route=0, **{name: 0 for name in kw})
            return f

        def multi():
            for i in range(k):
                hip.kzg_verify_multi(srs1, srs2, com[0], zs[i], ys[i], proofs[i])

        return r, k, pairs, {
            "pairs_table": pairs(1),
            "pairs_msm": pairs(2),
            "pairs_host": lambda: hip.kzg_coset_pairs(srs1, com, wd, evals[:d], 1, r, log2l, winv, linv, r, point_mode=1),
            "each_dev": lambda: hip.kzg_verify_cosets_each_dev(srs1, d_com, 0, d_tau, d_wd, 1, d_evals, 1, r, log2l, winv, linv, d_proofs, r, d_status),
            "each_host": lambda: hip.kzg_verify_cosets_each(srs1, com, tau_l, wd, evals[:d], 1, r, log2l, winv, linv, proofs[:r], point_mode=1),
            "cosets_dev": lambda: hip.kzg_verify_cosets_dev(srs1, d_com, 0, d_tau, d_wd, 1, d_evals, 1, r, log2l, winv, linv, d_proofs, d_gammas, r),
            "multi": multi,
        }

    if a.trace_only:
        _, _, pairs, v = variants(a.log2d, a.log2l)
        for _ in range(a.reps):
            pairs(1)(); pairs(2)()
        hip.close()
        return
    lines = ["# %s" % hip.version(),
             "# all r = d / l cosets of one vector (one commitment, domain order, point_mode 1): medians (ms) of %d alternating rounds in one process after %d warm-up rounds"
             % (a.rounds, a.warm),
             "# (a) pairs_table / pairs_msm = keaki_hip_kzg_coset_pairs_dev + synchronise with coset_rows_route 1 / 2; pairs_host = from host arrays, the plan's route",
             "# (b) each_dev / each_host = keaki_hip_kzg_verify_cosets_each; cosets_dev = keaki_hip_kzg_verify_cosets_dev on the same items (the floor);",
             "#     multi_k = k = min(r, 64) calls of keaki_hip_kzg_verify_multi, measured; multi_r = multi_k * r / k: r calls, EXTRAPOLATED (the parent's only route)",
             "%6s %6s %7s %11s %10s %10s %9s %9s %10s %4s %9s %12s %12s" % ("log2d", "l", "r", "pairs_table", "pairs_msm", "pairs_host", "each_dev", "each_host", "cosets_dev", "k",
                                                                        "multi_k", "multi_r(ex)", "multi_r/each")]
    for log2d, log2l in shapes:
        r, k, _, v = variants(log2d, log2l)
        m = timed(v, a.warm, a.rounds, sparse=("multi",) if k > 8 else ())
        multi_r = m["multi"] * r / k
        lines.append("%6d %6d %7d %11.3f %10.3f %10.3f %9.3f %9.3f %10.3f %4d %9.2f %12.1f %12.1f" % (log2d, 1 << log2l, r, m["pairs_table"], m["pairs_msm"], m["pairs_host"],
                                                                                              m["each_dev"], m["each_host"], m["cosets_dev"], k, m["multi"], multi_r,
                                                                                              multi_r / m["each_dev"]))
        print(lines[-1], flush=True)
    if a.sweep:
        lines.append("# (d) sweeps on route 1 (keaki_hip_kzg_coset_pairs_dev + synchronise, ms): coset_rows_min_lanes, then coset_rows_wb (a refused table means route 2)")
        lanes = [1, 1 << 14, 1 << 16, 1 << 17, 1 << 18, 1 << 20]
        lines.append("%6s %6s %7s " % ("log2d", "l", "r") + " ".join("%10s" % ("lanes=2^%d" % (x.bit_length() - 1)) for x in lanes) + " " + " ".join("%8s" % ("wb=%d" % w) for w in (8, 10, 13)))
        for log2d, log2l in shapes:
            r, k, pairs, _ = variants(log2d, log2l)
            m = timed({("lanes", x): pairs(1, min_lanes=x) for x in lanes}, a.warm, a.rounds)
            for w in (8, 10, 13):                            # one width after the other: a change of width rebuilds the handle's table (the warm-up call)
                if 64 * (1 << log2l) * ((254 + w - 1) // w) * ((1 << (w - 1)) + 1) <= (3 << 29):
                    m.update(timed({("wb", w): pairs(1, wb=w)}, 1, a.rounds))
            lines.append("%6d %6d %7d " % (log2d, 1 << log2l, r) + " ".join("%10.3f" % m[("lanes", x)] for x in lanes) + " "
                         + " ".join(("%8.3f" % m[("wb", w)]) if ("wb", w) in m else "%8s" % "-" for w in (8, 10, 13)))
            print(lines[-1], flush=True)
    if a.encrypt:
        from keaki_amd import keaki as K
        lines.append("# (c) encryption to all r cosets, host layer, 32-byte messages: vec_encrypt_cosets (ms) against k = min(r, 64) encrypt_set calls, measured, and r calls, EXTRAPOLATED")
        lines.append("%6s %6s %7s %12s %4s %10s %12s %10s" % ("log2d", "l", "r", "enc_cosets", "k", "set_k", "set_r(ex)", "set_r/enc"))
        ls = sorted({s[1] for s in shapes if s[1] <= 6})
        setup = K.KZGSetup.setup_with_g2(fr_mont(0x1234567), 1 << max(a.encrypt_log2d), 1 << max(ls))
        try:
            for log2d in a.encrypt_log2d:
                for log2l in ls:
                    d, l = 1 << log2d, 1 << log2l
                    r = d // l
                    k = min(r, 64)
                    kcom = K.commit(setup, evals[:64])
                    dom = K.domain_elements(d)
                    rows = np.ascontiguousarray(evals[:d].reshape(l, r, 4).transpose(1, 0, 2))
                    msgs = np.zeros((r, 32), np.uint8)
                    idx = [np.arange(l) * r + i for i in range(k)]

                    def sets():
                        rng = K.Rng(5)
                        for i in range(k):
                            K.encrypt_set(rng, setup, kcom, dom[idx[i]], rows[i], bytes(32))

                    m = timed({"enc": lambda: K.vec_encrypt_cosets(K.Rng(5), setup, kcom, d, l, np.arange(r), rows, msgs), "sets": sets}, a.warm, a.rounds, sparse=("sets",))
                    lines.append("%6d %6d %7d %12.3f %4d %10.2f %12.1f %10.1f" % (log2d, l, r, m["enc"], k, m["sets"], m["sets"] * r / k, m["sets"] * r / k / m["enc"]))
                    print(lines[-1], flush=True)
        finally:
            setup.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    srs1.free(); srs2.free()
    hip.close()


if __name__ == "__main__":
    main()
