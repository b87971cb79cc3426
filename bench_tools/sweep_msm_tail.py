"""The bucket reduction of the shared-bucket G1 MSM: row and column sums (reduce_l = 0 from ROWCOL_MIN_B buckets on) against the chunked
running sums with the chunk length automatic selection used before (reduce_l = 8 / 16 / 32), whole MSM over window tables, by number
of points and forced table width (msm_c_shared). The library must be built with ROWCOL_MIN_B at its floor (2^12) for the columns below
the committed threshold to mean anything. Results must be equal.

    python bench_tools/sweep_msm_tail.py [log2n ...]  >> profiles/msm_tail_rowcol.txt
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keaki_amd.hip import KeakiHip
from bench import random_fr_limbs
from oracle import bn254_py as py

REPS = 8
WIDTHS = {16: (13, 14, 15, 17), 18: (14, 15, 17, 19), 20: (15, 17, 19, 0), 22: (17, 19, 21, 0), 24: (19, 0)}      # 0: the automatic width


def max_b(c):
    W = (254 + c - 1) // c
    base, rem = 254 // W, 254 % W
    cc, k = (base + 1, rem) if rem else (base, W)
    widths = [cc if w < k else cc - 1 for w in range(W)]
    return max([1 << (wd - 1) for wd in widths[:-1]] + [1 << widths[-1]])


def old_l(b):
    return 32 if b >= 1 << 21 else 16 if b >= 1 << 20 else 8


def main():
    limbs = lambda x: np.frombuffer(int(x).to_bytes(32, "little"), np.uint64)
    g1 = np.concatenate([limbs(py.G1_GEN[0] * (1 << 256) % py.P), limbs(py.G1_GEN[1] * (1 << 256) % py.P)])
    h = KeakiHip(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    print("# %d MSMs per figure, two rounds chain / rowcol / chain / rowcol, ms per MSM (the faster round)" % REPS)
    for ln in [int(a) for a in sys.argv[1:]] or sorted(WIDTHS):
        n = 1 << ln
        d_gen = dev(g1); d_k = dev(random_fr_limbs(n, 9)); d_pts = torch.empty(n * 8, dtype=torch.int64, device="cuda")
        h.g1_mul_batch_dev(d_gen.data_ptr(), 0, d_k.data_ptr(), n, d_pts.data_ptr())
        sc = dev(random_fr_limbs(n, 3))
        out = torch.empty(12, dtype=torch.int64, device="cuda")
        for c in WIDTHS[ln]:
            h.set_option("msm_c_shared", c)
            srs = h.srs_g1_wrap_dev(d_pts.data_ptr(), n)
            h.srs_g1_precompute(srs)
            best, refs = {}, {}
            for rnd in range(2):
                for name in ("old", "new"):
                    h.msm_g1_dev(srs, sc.data_ptr(), n, out.data_ptr()); h.synchronize()
                    cw = h.last_msm_stats()["window_bits"]
                    b = max_b(cw)
                    h.set_option("reduce_l", old_l(b) if name == "old" else 0)
                    h.msm_g1_dev(srs, sc.data_ptr(), n, out.data_ptr()); h.synchronize()
                    refs[name] = out.cpu().numpy().copy()
                    t0 = time.perf_counter()
                    for _ in range(REPS): h.msm_g1_dev(srs, sc.data_ptr(), n, out.data_ptr())
                    h.synchronize()
                    ms = (time.perf_counter() - t0) / REPS * 1e3
                    best[name] = min(best.get(name, 1e9), ms)
            h.set_option("reduce_l", 0)
            same = np.array_equal(refs["old"], refs["new"])
            print("n=2^%d msm_c_shared=%d window_bits=%d buckets=2^%d  chain(L=%d) %.3f ms  rowcol %.3f ms  %+.3f ms%s"
                  % (ln, c, cw, b.bit_length() - 1, old_l(b), best["old"], best["new"], best["new"] - best["old"], "" if same else "  RESULTS DIFFER"), flush=True)
            srs.free()
        del d_pts, d_k, sc
        h.trim()
    h.close()


if __name__ == "__main__":
    main()
