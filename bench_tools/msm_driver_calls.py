"""One small call for every path through the MSM host driver (keaki_amd/csrc/msm_host.hip.h: msm_dev), in one process, for a kernel trace:
  rocprofv3 --kernel-trace -- python bench_tools/msm_driver_calls.py
run against two builds, the ordered (kernel, grid, workgroup) lists must be equal (profiles/msm_driver_kernel_order.txt). Prints the
call list; every result is checked against the first path that computed the same sum. Every shape is small: a few seconds in all."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keaki_amd.hip import KeakiHip, jac_to_affine_words
from bench import random_fr_limbs
from oracle import bn254_py as py

limbs = lambda x: np.frombuffer(int(x).to_bytes(32, "little"), np.uint64)
mont = lambda x: limbs(x * (1 << 256) % py.P)
G1 = np.concatenate([mont(py.G1_GEN[0]), mont(py.G1_GEN[1])])
G2 = np.concatenate([mont(c) for xy in py.G2_GEN for c in xy])
DEFAULTS = {"msm_c": 0, "reduce_l": 0, "msm_short_tables": 1, "acc_u29": 1, "acc_nt": 0, "acc_prefetch": 1, "acc_idxq": 1, "cs_masked": 1,
            "msm_pipe_chunks": 0}

seen = {}
def call(h, what, key, fn, **opts):
    for k, v in {**DEFAULTS, **opts}.items():
        h.set_option(k, v)
    got = jac_to_affine_words(fn()).tolist()           # the host entries return normalised Jacobian points
    assert seen.setdefault(key, got) == got, what
    print(what, flush=True)


h = KeakiHip(0)
sc = random_fr_limbs(16384, 3)
pts = h.g1_mul_batch(G1, random_fr_limbs(16384, 9))
srs = h.srs_g1_upload(pts)                               # no tables: the generic path
for n in (0, 1, 33, 4096):
    call(h, "g1 generic n=%d" % n, ("a", n), lambda: h.msm_g1(srs, sc[:n]))
call(h, "g1 generic n=16384 msm_c=10 reduce_l=1 (k_msm_partial_groups)", ("a", 16384), lambda: h.msm_g1(srs, sc), msm_c=10, reduce_l=1)
for opt, v in (("acc_u29", 0), ("acc_nt", 1), ("acc_prefetch", 0), ("acc_idxq", 0), ("cs_masked", 0)):
    call(h, "g1 generic n=4096 %s=%d" % (opt, v), ("a", 4096), lambda: h.msm_g1(srs, sc[:4096]), **{opt: v})
srs.free()

h.set_option("msm_c_shared", 13)
srs = h.srs_g1_upload(pts[:4096]); h.srs_g1_precompute(srs)
call(h, "g1 tables(13) srs=4096 n=4096 (row/column tail)", ("a", 4096), lambda: h.msm_g1(srs, sc[:4096]))
call(h, "g1 tables(13) srs=4096 n=100", ("a", 100), lambda: h.msm_g1(srs, sc[:100]))
call(h, "g1 tables(13) srs=4096 n=100 msm_short_tables=0 (generic beside tables)", ("a", 100), lambda: h.msm_g1(srs, sc[:100]), msm_short_tables=0)
call(h, "g1 tables(13) srs=4096 n=4096 reduce_l=8 (running sums over tables)", ("a", 4096), lambda: h.msm_g1(srs, sc[:4096]), reduce_l=8)
srs.free()

srs = h.srs_g1_upload(pts[:5000]); h.srs_g1_precompute(srs)
call(h, "g1 tables(13) srs=5000 n=5000 host entry", ("a", 5000), lambda: h.msm_g1(srs, sc[:5000]))
call(h, "g1 tables(13) srs=5000 n=5000 host entry msm_pipe_chunks=3", ("a", 5000), lambda: h.msm_g1(srs, sc[:5000]), msm_pipe_chunks=3)
z = random_fr_limbs(1, 5)[0]
call(h, "kzg_open n=5000", "open", lambda: h.kzg_open(srs, sc[:5000], z)[0])
call(h, "kzg_open n=5000 msm_pipe_chunks=3", "open", lambda: h.kzg_open(srs, sc[:5000], z)[0], msm_pipe_chunks=3)
srs.free()

# the parked registers (Acc29, 144 B per bucket) refused, the canonical buckets (128 B, held since the unchunked call) admitted:
# tests/test_gpu_msm_pipe.py: test_chunked_call_without_room_for_the_parked_registers_falls_back. A context of its own: its workspaces start empty
h2 = KeakiHip(0)
h2.set_option("msm_c_shared", 13)
srs = h2.srs_g1_upload(pts[:5000]); h2.srs_g1_precompute(srs)
call(h2, "g1 second context: tables(13) srs=5000 n=5000 host entry", ("a", 5000), lambda: h2.msm_g1(srs, sc[:5000]))
nb = 1 << (h2.last_msm_stats()["window_bits"] - 1)
h2.debug_set_alloc_limit(nb * 136)
call(h2, "g1 second context: the same, msm_pipe_chunks=3, allocation limit %d (no Acc29)" % (nb * 136), ("a", 5000), lambda: h2.msm_g1(srs, sc[:5000]),
     msm_pipe_chunks=3)
h2.debug_set_alloc_limit(0)
srs.free(); h2.close()

pts2 = h.g2_mul_batch(G2, random_fr_limbs(300, 11))
srs2 = h.srs_g2_upload(pts2)
call(h, "g2 generic n=300", "g2", lambda: h.msm_g2(srs2, sc[:300]))
call(h, "g2 generic n=300 host entry msm_pipe_chunks=3", "g2", lambda: h.msm_g2(srs2, sc[:300]), msm_pipe_chunks=3)
h.srs_g2_precompute(srs2)
call(h, "g2 tables(13) n=300", "g2", lambda: h.msm_g2(srs2, sc[:300]))
call(h, "g2 tables(13) n=300 host entry msm_pipe_chunks=3", "g2", lambda: h.msm_g2(srs2, sc[:300]), msm_pipe_chunks=3)
srs2.free(); h.close()
print("all results agree")
