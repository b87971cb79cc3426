#!/usr/bin/env python3
"""encrypt_multi (keaki_hip_encrypt_multi / _dev: m commitments, one call) against what the library offered before it -- a loop of m
keaki_hip_encrypt_batch calls on one context -- and against decap_batch on the same number of items (the same pairings and the same KDF:
the floor of the fused route), plus the sweep that places "encap_multi_single_min".

One device, one process. Per shape (m groups x k items, msg_len 32) the variants ALTERNATE round by round in the same process: multi from
host arrays, multi on resident buffers (_dev), the loop from host arrays, the loop on resident buffers, decap host, decap _dev. Every
measurement is a host clock around whole calls that ends in a device synchronisation; a figure is the median of its rounds, and the rounds
of a figure add up to at least 0.5 s of timed work (at least three rounds) after one warm-up round of every variant. Output arrays are
allocated and touched once, before the rounds, for every variant alike. A loop whose full pass would take more than about 20 s is timed
over its first groups only (at least 64) and scaled by m / groups: such figures are labelled "extrapolated".

Threshold sweep: 16 groups of k = 1,024 .. 65,536 items, the fused route for every group ("encap_multi_single_min" = 0) against the
single-commitment route for every group (= 1), alternating. The default of the option is the smallest k at which the single route wins.

    python bench_tools/bench_encap_multi.py --out profiles/encap_multi_times.txt [--resources FILE]
    rocprofv3 --kernel-trace --stats -- python bench_tools/bench_encap_multi.py --trace-only      # five _dev calls at 4,096 x 512

--resources FILE: the compiler's -Rpass-analysis=kernel-resource-usage lines for k_encap_multi_g1 (made where the library is built),
quoted at the end of the profile.
"""
import argparse, ctypes as C, faulthandler, math, os, statistics, sys, time
faulthandler.enable()
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import random_fr_limbs, SEED  # noqa: E402

SHAPES = [(4096, 512), (1024, 64), (65536, 2), (16, 65536)]
SWEEP_K = [1024, 4096, 16384, 65536]
ML = 32
MIN_TIMED_S, LOOP_BUDGET_S = 0.5, 20.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="m:k,... instead of the four shapes of the profile")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--resources", default=None)
    ap.add_argument("--trace-only", action="store_true", help="five _dev calls at 4,096 x 512: the run to put under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    import torch
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    hip = KeakiHip(0)
    lib, ctx = hip.lib, hip.ctx
    P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    mont = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    g1 = np.array(mont(1) + mont(2), np.uint64)
    shapes = SHAPES if not a.shapes else [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    m_max = max([m for m, _ in shapes] + [16])
    n_max = max([m * k for m, k in shapes] + ([16 * max(SWEEP_K)] if not a.no_sweep else []))
    coms_all = hip.g1_mul_batch(g1, random_fr_limbs(m_max, SEED + 41))
    pool = random_fr_limbs(n_max, SEED + 42)
    tau_g2 = _g2_seed(hip, pool)
    pts_all, vals_all, rs_all = pool, np.roll(pool, 1, axis=0), np.roll(pool, 2, axis=0)
    msgs_all = np.frombuffer(np.random.default_rng(SEED + 43).bytes(n_max * ML), np.uint8).reshape(n_max, ML).copy()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    vp = lambda x: C.c_void_p(int(x))
    addr = lambda arr: arr.ctypes.data
    ck = hip._ck

    def timed(f):
        t0 = time.perf_counter()
        f()
        hip.synchronize()
        return time.perf_counter() - t0

    def alternate(variants):
        """variants: {name: f}. One warm-up round, then rounds of every variant in turn until each has >= 3 rounds and >= MIN_TIMED_S of timed work."""
        t = {k: [] for k in variants}
        first = {k: timed(f) for k, f in variants.items()}
        rounds = max(3, max(int(math.ceil(MIN_TIMED_S / max(x, 1e-6))) for x in first.values() if x < MIN_TIMED_S) if any(x < MIN_TIMED_S for x in first.values()) else 3)
        rounds = min(rounds, 200)
        for _ in range(rounds):
            for k, f in variants.items():
                if sum(t[k]) >= MIN_TIMED_S and len(t[k]) >= 3:
                    continue
                t[k].append(timed(f))
        return {k: statistics.median(v) * 1e3 for k, v in t.items()}

    class Case:
        """the arrays of one (m, k) shape, host and device, and the calls over them"""

        def __init__(self, m, k):
            self.m, self.k, self.n = m, k, m * k
            n = self.n
            self.coms = np.ascontiguousarray(coms_all[:m])
            self.off = (np.arange(m + 1, dtype=np.uint64) * np.uint64(k))
            self.pts, self.vals, self.rs = (np.ascontiguousarray(x[:n]) for x in (pts_all, vals_all, rs_all))
            self.msgs = np.ascontiguousarray(msgs_all[:n])
            self.ct, self.body = np.ones((n, 16), np.uint64), np.ones((n, ML), np.uint8)
            self.out2 = np.ones((n, ML), np.uint8)
            up = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
            self.d = {k_: up(v) for k_, v in dict(coms=self.coms, tau=tau_g2, pts=self.pts, vals=self.vals, rs=self.rs, body=self.msgs).items()}
            self.d["ct"] = torch.ones((n, 16), dtype=torch.int64, device=dev)
            self.d["proofs"] = up(np.resize(self.coms, (n, 8)))
            self.proofs = np.resize(self.coms, (n, 8))
            torch.cuda.synchronize()

        def multi_host(self):
            ck(lib.keaki_hip_encrypt_multi(ctx, vp(addr(self.coms)), vp(addr(self.off)), self.m, vp(addr(tau_g2)), vp(addr(self.pts)), vp(addr(self.vals)),
                                           vp(addr(self.rs)), vp(addr(self.msgs)), self.n, vp(addr(self.ct)), vp(addr(self.body)), ML))

        def multi_dev(self):
            d = self.d
            ck(lib.keaki_hip_encrypt_multi_dev(ctx, vp(d["coms"].data_ptr()), vp(addr(self.off)), self.m, vp(d["tau"].data_ptr()), vp(d["pts"].data_ptr()),
                                               vp(d["vals"].data_ptr()), vp(d["rs"].data_ptr()), self.n, vp(d["ct"].data_ptr()), vp(d["body"].data_ptr()), ML))

        def loop_host(self, groups):
            k = self.k
            for j in range(groups):
                lo = j * k
                ck(lib.keaki_hip_encrypt_batch(ctx, vp(addr(self.coms) + 64 * j), vp(addr(tau_g2)), vp(addr(self.pts) + 32 * lo), vp(addr(self.vals) + 32 * lo),
                                               vp(addr(self.rs) + 32 * lo), vp(addr(self.msgs) + ML * lo), k, vp(addr(self.ct) + 128 * lo), vp(addr(self.out2) + ML * lo), ML))

        def loop_dev(self, groups):
            d, k = self.d, self.k
            for j in range(groups):
                lo = j * k
                ck(lib.keaki_hip_encrypt_batch_dev(ctx, vp(d["coms"].data_ptr() + 64 * j), vp(d["tau"].data_ptr()), vp(d["pts"].data_ptr() + 32 * lo),
                                                   vp(d["vals"].data_ptr() + 32 * lo), vp(d["rs"].data_ptr() + 32 * lo), k, vp(d["ct"].data_ptr() + 128 * lo),
                                                   vp(d["body"].data_ptr() + ML * lo), ML))

        def decap_host(self):
            ck(lib.keaki_hip_decap_batch(ctx, vp(addr(self.proofs)), vp(addr(self.ct)), self.n, None, vp(addr(self.out2)), ML))

        def decap_dev(self):
            d = self.d
            ck(lib.keaki_hip_decap_batch_dev(ctx, vp(d["proofs"].data_ptr()), vp(d["ct"].data_ptr()), self.n, None, vp(d["body"].data_ptr()), ML))

    if a.trace_only:
        c = Case(4096, 512)
        for _ in range(5):
            c.multi_dev()
        hip.synchronize()
        return

    say("# bench_encap_multi: %s, ms, msg_len %d (version %s)" % (torch.cuda.get_device_name(0), ML, hip.version()))
    say("# clock: not pinned; the variants of a row alternate round by round in one process on one device. A figure: median of >= 3 rounds and >= 0.5 s of timed work,")
    say("# host clock around whole calls ending in a device synchronisation. host = host arrays in and out; dev = resident buffers (_dev forms).")
    say("# loop = m calls of keaki_hip_encrypt_batch(_dev) on the same items (the only route before encrypt_multi); (x) = extrapolated from the first groups.")
    say("# floor = keaki_hip_decap_batch(_dev) on the same n: the same pairings and KDF without the G1 ladder and the G2 fixed-base sums.")
    say("# default encap_multi_single_min during the shape rows: %d" % _default_single_min())
    say("# %6s %6s %9s | %10s %10s %8s | %10s %10s %8s | %10s %10s %7s %7s | %9s" % ("m", "k", "n", "multi_host", "loop_host", "host x", "multi_dev", "loop_dev", "dev x",
                                                                                   "floor_host", "floor_dev", "host/fl", "dev/fl", "Mitems/s"))
    for m, k in shapes:
        c = Case(m, k)
        # the results agree before anything is timed: the multi call against the loop over the first and the last group
        c.multi_host()
        hip.synchronize()
        ct_ref, body_ref = c.ct.copy(), c.body.copy()
        for j in sorted({0, m - 1}):
            e_ct, e_body = hip.encrypt_batch(c.coms[j], tau_g2, c.pts[j * k:(j + 1) * k], c.vals[j * k:(j + 1) * k], c.rs[j * k:(j + 1) * k], c.msgs[j * k:(j + 1) * k])
            assert np.array_equal(e_ct, ct_ref[j * k:(j + 1) * k]) and np.array_equal(e_body, body_ref[j * k:(j + 1) * k]), (m, k, j)
        # how many groups of the loop fit the budget
        probe = min(m, 64)
        t_probe = max(timed(lambda: c.loop_host(probe)), timed(lambda: c.loop_dev(probe)))
        full = t_probe * m / probe <= LOOP_BUDGET_S
        groups = m if full else max(64, min(m, int(probe * 3.0 / t_probe)))
        scale, mark = m / groups, "" if full else "(x)"
        t = alternate({"multi_host": c.multi_host, "multi_dev": c.multi_dev, "loop_host": lambda: c.loop_host(groups), "loop_dev": lambda: c.loop_dev(groups),
                       "floor_host": c.decap_host, "floor_dev": c.decap_dev})
        lh, ld = t["loop_host"] * scale, t["loop_dev"] * scale
        say("  %6d %6d %9d | %10.2f %10.1f%s %8.1f | %10.2f %10.1f%s %8.1f | %10.2f %10.2f %7.2f %7.2f | %9.2f" % (
            m, k, c.n, t["multi_host"], lh, mark, lh / t["multi_host"], t["multi_dev"], ld, mark, ld / t["multi_dev"], t["floor_host"], t["floor_dev"],
            t["multi_host"] / t["floor_host"], t["multi_dev"] / t["floor_dev"], c.n / t["multi_dev"] / 1e3))
        if not full:
            say("#        (x): loop timed over %d of %d groups and scaled" % (groups, m))
        del c
        torch.cuda.empty_cache()
    if not a.no_sweep:
        say("# threshold sweep: 16 groups of k items; fused = encap_multi_single_min 0, single = 1 (every group through the single-commitment path)")
        say("# %7s %9s | %10s %10s %8s | %10s %10s %8s" % ("k", "n", "fused_host", "single_host", "winner", "fused_dev", "single_dev", "winner"))
        wins = []
        for k in SWEEP_K:
            c = Case(16, k)

            def with_min(v, f):
                def g():
                    hip.set_option("encap_multi_single_min", v)
                    f()
                return g

            t = alternate({"fused_host": with_min(0, c.multi_host), "single_host": with_min(1, c.multi_host), "fused_dev": with_min(0, c.multi_dev),
                           "single_dev": with_min(1, c.multi_dev)})
            wh = "single" if t["single_host"] < t["fused_host"] else "fused"
            wd = "single" if t["single_dev"] < t["fused_dev"] else "fused"
            wins.append((k, wh, wd))
            say("  %7d %9d | %10.2f %10.2f %8s | %10.2f %10.2f %8s" % (k, c.n, t["fused_host"], t["single_host"], wh, t["fused_dev"], t["single_dev"], wd))
            del c
            torch.cuda.empty_cache()
        hip.set_option("encap_multi_single_min", _default_single_min())
        first = next((k for k, wh, wd in wins if wh == "single" and wd == "single"), None)
        say("# smallest measured k at which the single route wins in both forms: %s" % (first if first is not None else "none of the measured k"))
    if a.resources and os.path.exists(a.resources):
        say("# k_encap_multi_g1, compiler report (-Rpass-analysis=kernel-resource-usage, gfx950):")
        for ln in open(a.resources).read().splitlines():
            say("#   " + ln.strip())


def _default_single_min():
    import re
    src = open(os.path.join(ROOT, "keaki_amd", "csrc", "internal.h")).read()
    return int(re.search(r"long long encap_multi_single_min = (\d+);", src).group(1))


def _g2_seed(hip, pool):
    """[tau]_2 for a random tau: the library's own G2 scalar multiplication of the generator"""
    from bench import G2_GEN, mont_words
    gen = np.array(sum([mont_words(c) for c in G2_GEN], []), np.uint64)
    return np.ascontiguousarray(hip.g2_mul_batch(gen, pool[:1])[0])


if __name__ == "__main__":
    main()
