"""One small, successful call for every host-array entry that feeds its arrays through CopyFeed (keaki_amd/csrc/api_host.h), and for the _dev
forms of the KZG verification family, in one process, for a trace:
  rocprofv3 --kernel-trace --memory-copy-trace --output-format csv json -- python bench_tools/host_form_calls.py
run against two builds, every call's ordered (kernel, grid, workgroup) list per stream and its sorted (direction, bytes) list of copies
must be equal (profiles/host_forms_call_order.txt; --compare A B reads the two traces). Every call is followed by a separator the trace
shows, one launch of the one-workgroup field self-test: what lies between two separators belongs to one call. Prints the call list with
a digest of each call's outputs, which must agree between the builds as well. n <= 5000 throughout, except the one verify_batch that
takes the copy-stream route (from 65,536 items on)."""
import glob, hashlib, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEPARATOR = "k_selftest_field"


def run():
    from keaki_amd.hip import KeakiHip
    from bench import random_fr_limbs, mont_words, R_MOD
    from oracle import bn254_py as py
    limbs = lambda x: np.frombuffer(int(x).to_bytes(32, "little"), np.uint64)
    mont = lambda x: limbs(x * (1 << 256) % py.P)
    mont_fr = lambda v: np.frombuffer(((v << 256) % R_MOD).to_bytes(32, "little"), np.uint64).copy()
    G1 = np.concatenate([mont(py.G1_GEN[0]), mont(py.G1_GEN[1])])
    G2 = np.concatenate([mont(c) for xy in py.G2_GEN for c in xy])
    h = KeakiHip(0)

    def call(what, fn, **opts):
        for k, v in {"msm_pipe_chunks": -1, **opts}.items():
            h.set_option(k, v)
        out = fn()
        d = hashlib.sha1()
        for x in (out if isinstance(out, tuple) else (out,)):
            d.update(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else repr(x).encode())
        h.selftest_field(1, 1, 1)
        print("%-64s %s" % (what, d.hexdigest()[:16]), flush=True)
        return out

    # inputs made through calls of the list itself
    sc = random_fr_limbs(70000, 3)
    pts = call("g1_mul_batch n=5000, one base", lambda: h.g1_mul_batch(G1, sc[:5000]))
    call("g1_mul_batch n=1000, a base per item", lambda: h.g1_mul_batch(pts[:1000], sc[5000:6000]))
    q2 = call("g2_mul_batch n=300, one base", lambda: h.g2_mul_batch(G2, sc[:300]))
    call("pairing_batch n=64", lambda: h.pairing_batch(pts[:64], q2[:64]))
    call("pairing_batch n=64, one second argument", lambda: h.pairing_batch(pts[:64], q2[0]))
    call("miller_loop_batch n=4", lambda: h.miller_loop_batch(pts[:4], q2[:4]))
    call("final_exp_batch n=4", lambda: h.final_exp_batch(h.miller_loop_batch(pts[:4], q2[:4])))
    call("g2_prepare", lambda: h.g2_prepare(q2[1]))
    call("g2_check n=300", lambda: h.g2_check(q2))
    call("g2_subgroup_check n=300", lambda: h.g2_subgroup_check(q2))
    wire = call("g1_compress n=5000", lambda: h.g1_compress(pts))
    call("g1_decompress n=5000", lambda: h.g1_decompress(wire))
    call("g2_decompress n=300", lambda: h.g2_decompress(h.g2_compress(q2)))

    srs = h.srs_g1_upload(pts); h.srs_g1_precompute(srs)
    srs2 = h.srs_g2_upload(q2)
    z = sc[6000]
    call("msm_g1 n=5000", lambda: h.msm_g1(srs, sc[:5000]), msm_pipe_chunks=0)
    call("msm_g1 n=5000 msm_pipe_chunks=3", lambda: h.msm_g1(srs, sc[:5000]), msm_pipe_chunks=3)
    call("msm_g1 n=0", lambda: h.msm_g1(srs, sc[:0]), msm_pipe_chunks=0)
    call("msm_g2 n=300", lambda: h.msm_g2(srs2, sc[:300]), msm_pipe_chunks=0)
    call("msm_g2 n=300 msm_pipe_chunks=3", lambda: h.msm_g2(srs2, sc[:300]), msm_pipe_chunks=3)
    call("kzg_open n=5000", lambda: h.kzg_open(srs, sc[:5000], z), msm_pipe_chunks=0)
    call("kzg_open n=5000 msm_pipe_chunks=3", lambda: h.kzg_open(srs, sc[:5000], z), msm_pipe_chunks=3)
    call("kzg_open n=1", lambda: h.kzg_open(srs, sc[:1], z), msm_pipe_chunks=3)
    call("kzg_quotient n=5000", lambda: h.kzg_quotient(sc[:5000], z))
    rows = sc[:8 * 512].reshape(8, 512, 4)
    sums = call("msm_g1_batch m=8 n=512", lambda: h.msm_g1_batch(srs, rows))
    call("kzg_open_batch m=8 n=512", lambda: h.kzg_open_batch(srs, rows, sc[7000:7008]))
    call("g1_sum k=8", lambda: h.g1_sum(sums))

    lg = 8; d = 1 << lg
    w2d = pow(5, (R_MOD - 1) >> (lg + 1), R_MOD); wd = w2d * w2d % R_MOD
    om, omi, inv2d = mont_fr(w2d), mont_fr(pow(w2d, -1, R_MOD)), mont_fr(pow(2 * d, -1, R_MOD))
    call("fr_fft 2^8", lambda: h.fr_fft(sc[:d], lg, mont_fr(wd)))
    call("open_fk_poly 2^8", lambda: h.open_fk_poly(srs, lg, sc[:d], om, omi, inv2d))
    # the form that takes hat_a and the twiddle tables from the caller: the launches do not depend on their values
    call("open_fk 2^8", lambda: h.open_fk(srs, lg, sc[:2 * d], sc[1000:1000 + d], sc[2000:2000 + d], sc[3000:3000 + d // 2]))
    call("vec_commit 2^8, 200 values and the pad", lambda: h.vec_commit(srs, sc[:200], sc[200], lg, mont_fr(pow(wd, -1, R_MOD)), mont_fr(pow(d, -1, R_MOD)), om, omi, inv2d))

    tau = q2[2]
    call("encap_prepare hint=4", lambda: h.encap_prepare(tau, 4))
    ct, gt, key = call("encap_batch n=4", lambda: h.encap_batch(pts[0], tau, sc[:4], sc[4:8], sc[8:12], 32))
    call("decap_batch n=4", lambda: h.decap_batch(pts[:4], ct, 32))
    msgs = np.arange(4 * 32, dtype=np.uint8).reshape(4, 32)
    ct, body = call("encrypt_batch n=4", lambda: h.encrypt_batch(pts[0], tau, sc[:4], sc[4:8], sc[8:12], msgs))
    call("decrypt_batch n=4", lambda: h.decrypt_batch(pts[:4], ct, body))

    # random openings: the verdict is 0, and no launch of the call depends on it
    n = 70000
    proofs = h.g1_mul_batch(G1, sc[:n]); coms = h.g1_mul_batch(pts[1], sc[:n])
    h.selftest_field(1, 1, 1)
    zs, ys, gs = random_fr_limbs(n, 5), random_fr_limbs(n, 6), random_fr_limbs(n, 7)
    call("kzg_verify_batch n=1000, one commitment, points omega^i", lambda: h.kzg_verify_batch(coms[:1], tau, z, ys[:1000], proofs[:1000], gs[:1000], point_mode=1))
    call("kzg_verify_batch n=1000, general form", lambda: h.kzg_verify_batch(coms[:1000], tau, zs[:1000], ys[:1000], proofs[:1000], gs[:1000]))
    call("kzg_verify_batch n=70000, general form (copy stream)", lambda: h.kzg_verify_batch(coms, tau, zs, ys, proofs, gs))
    call("kzg_verify_batch n=70000, general form, pipe_chunks=0", lambda: h.kzg_verify_batch(coms, tau, zs, ys, proofs, gs), pipe_chunks=0)
    h.set_option("pipe_chunks", 1)

    # the rest of the KZG verification family (profiles/kzg_verify_family_call_order.txt): host forms, then the _dev forms on torch tensors
    call("kzg_verify", lambda: h.kzg_verify(coms[0], tau, z, ys[0], proofs[0]))
    call("kzg_verify_multi k=4", lambda: h.kzg_verify_multi(srs, srs2, coms[0], zs[:4], ys[:4], proofs[0], want_pair=True))
    n = 1000
    call("kzg_verify_each n=1000, one commitment, points omega^i", lambda: h.kzg_verify_each(coms[:1], tau, z, ys[:n], proofs[:n], point_mode=1))
    call("kzg_verify_each n=1000, general form", lambda: h.kzg_verify_each(coms[:n], tau, zs[:n], ys[:n], proofs[:n]))
    call("kzg_verify_each n=1000, general form, want_lhs", lambda: h.kzg_verify_each(coms[:n], tau, zs[:n], ys[:n], proofs[:n], want_lhs=True))
    n, ll = 64, 4; l = 1 << ll
    wl = pow(5, (R_MOD - 1) >> ll, R_MOD)
    winv, linv, vals = mont_fr(pow(wl, -1, R_MOD)), mont_fr(pow(l, -1, R_MOD)), random_fr_limbs(n * l, 8)
    call("kzg_verify_cosets n=64 l=16, one commitment, shifts omega^k",
         lambda: h.kzg_verify_cosets(srs, coms[:1], tau, z, vals, l, 1, ll, winv, linv, proofs[:n], gs[:n], point_mode=1))
    call("kzg_verify_cosets n=64 l=16, general form", lambda: h.kzg_verify_cosets(srs, coms[:n], tau, zs[:n], vals, l, 1, ll, winv, linv, proofs[:n], gs[:n]))
    for route in (1, 2):
        call("kzg_coset_pairs n=64 l=16 coset_rows_route=%d" % route, lambda: h.kzg_coset_pairs(srs, coms[:n], zs[:n], vals, l, 1, ll, winv, linv, n),
             coset_rows_route=route)
    h.set_option("coset_rows_route", 0)
    call("kzg_verify_cosets_each n=64 l=16, want_lhs", lambda: h.kzg_verify_cosets_each(srs, coms[:n], tau, zs[:n], vals, l, 1, ll, winv, linv, proofs[:n], want_lhs=True))

    import torch

    def dev(a, dtype=np.uint64):
        return torch.from_numpy(np.ascontiguousarray(a, dtype).view(np.int64 if dtype == np.uint64 else dtype).copy()).cuda()

    def back(*ts):
        h.synchronize()
        return tuple(t.cpu().numpy() for t in ts)

    m = 1000
    def uploads():
        ts = tuple(dev(a) for a in (coms[:m], tau, z, zs[:m], ys[:m], proofs[:m], gs[:m], vals, np.zeros((m, 8)), np.zeros((m, 4)))) + (dev(np.zeros(m), np.uint8),)
        torch.cuda.synchronize()
        return ts

    d_com, d_tau, d_z, d_zs, d_ys, d_pr, d_gs, d_vals, d_lhs, d_c, d_status = call("(uploads for the _dev forms)", uploads)
    call("kzg_verify_batch_dev n=1000, one commitment, points omega^i", lambda: h.kzg_verify_batch_dev(d_com, 0, d_tau, d_z, 1, d_ys, d_pr, d_gs, m))
    call("kzg_verify_batch_dev n=1000, general form", lambda: h.kzg_verify_batch_dev(d_com, 1, d_tau, d_zs, 0, d_ys, d_pr, d_gs, m))
    call("kzg_verify_each_dev n=1000, one commitment, points omega^i",
         lambda: (h.kzg_verify_each_dev(d_com, 0, d_tau, d_z, 1, d_ys, d_pr, m, d_status),) + back(d_status))
    call("kzg_verify_each_dev n=1000, general form, with lhs",
         lambda: (h.kzg_verify_each_dev(d_com, 1, d_tau, d_zs, 0, d_ys, d_pr, m, d_status, d_lhs),) + back(d_status, d_lhs))
    call("kzg_verify_cosets_dev n=64 l=16, one commitment, shifts omega^k",
         lambda: h.kzg_verify_cosets_dev(srs, d_com, 0, d_tau, d_z, 1, d_vals, l, 1, ll, winv, linv, d_pr, d_gs, n))
    call("kzg_verify_cosets_dev n=64 l=16, general form", lambda: h.kzg_verify_cosets_dev(srs, d_com, 1, d_tau, d_zs, 0, d_vals, l, 1, ll, winv, linv, d_pr, d_gs, n))
    for route in (1, 2):
        call("kzg_coset_pairs_dev n=64 l=16 coset_rows_route=%d" % route,
             lambda: (h.kzg_coset_pairs_dev(srs, d_com, 1, d_zs, 0, d_vals, l, 1, ll, winv, linv, n, d_lhs, d_c),) + back(d_lhs[:n], d_c[:n]), coset_rows_route=route)
    h.set_option("coset_rows_route", 0)
    call("kzg_verify_cosets_each_dev n=64 l=16, with lhs",
         lambda: (h.kzg_verify_cosets_each_dev(srs, d_com, 1, d_tau, d_zs, 0, d_vals, l, 1, ll, winv, linv, d_pr, n, d_status, d_lhs),) + back(d_status[:n], d_lhs[:n]))
    srs.free(); srs2.free(); h.close()
    print("done")


COPY_KINDS = {1: "H2H", 2: "H2D", 3: "D2H", 4: "D2D"}


def load(trace_dir):
    """-> per separator-delimited call of a rocprofv3 json trace: ({stream: [(kernel, grid, workgroup), ...]}, sorted [(direction, bytes), ...]).
    Streams are numbered by first use inside the call; the separator's own launches and its 8-byte download are dropped."""
    path = sorted(glob.glob(os.path.join(trace_dir, "**", "*results.json"), recursive=True))[0]
    rec = json.load(open(path))["rocprofiler-sdk-tool"][0]
    names = {k["kernel_id"]: k["formatted_kernel_name"].split("(")[0] for k in rec["kernel_symbols"]}
    ev = []
    for r in rec["buffer_records"]["kernel_dispatch"]:
        di = r["dispatch_info"]
        g, w = di["grid_size"], di["workgroup_size"]
        ev.append((r["start_timestamp"], "k", r["stream_id"]["handle"], (names[di["kernel_id"]], g["x"] * g["y"] * g["z"], w["x"] * w["y"] * w["z"])))
    for r in rec["buffer_records"]["memory_copy"]:
        ev.append((r["start_timestamp"], "c", r["stream_id"]["handle"], (COPY_KINDS.get(r["operation"], r["operation"]), r["bytes"])))
    ev.sort(key=lambda e: e[0])
    calls, kernels, copies, order, in_separator = [], {}, [], {}, False
    for _, kind, st, what in ev:
        if kind == "k" and SEPARATOR in what[0]:
            calls.append((kernels, sorted(copies)))
            kernels, copies, order, in_separator = {}, [], {}, True
        elif in_separator and kind == "k" and "selftest" in what[0]:
            continue
        elif in_separator and what == ("D2H", 8):
            in_separator = False
        elif kind == "c":
            copies.append(what)
        else:
            in_separator = False
            kernels.setdefault(order.setdefault(st, len(order)), []).append(what)
    return calls


def compare(dir_a, dir_b):
    a, b = load(dir_a), load(dir_b)
    print("calls: %d and %d" % (len(a), len(b)))
    bad = len(a) != len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        same_k, same_c = x[0] == y[0], x[1] == y[1]
        bad |= not (same_k and same_c)
        print("call %2d: %4d launches on %d stream(s) %s, %3d copies %s" % (i, sum(len(v) for v in x[0].values()), len(x[0]), "equal" if same_k else "DIFFER",
                                                                         len(x[1]), "equal" if same_c else "DIFFER: %s | %s" % (x[1], y[1])))
    print("DIFFERENT" if bad else "every call equal")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    run()
