#!/usr/bin/env python3
"""The compressed point wire format (keaki_hip_g1/g2_compress, _decompress, keaki_hip_g2_subgroup_check) at n = 2^16 and 2^20: points per
second resident (_dev forms) and from host arrays, and -- the yardstick -- keaki_hip_decap_batch_dev on the same n in the same run: validated
G2 decompression guards a decapsulation, so its cost is reported as a fraction of the decapsulation's.

Per entry: warm-up, then the median of --reps calls, each ending in a device synchronisation (the decompress and check entries synchronise
themselves: their counters are host pointers). The points are random multiples of the generators, made on the device.

    python bench_tools/bench_point_codec.py --out profiles/point_codec.txt
    python bench_tools/bench_point_codec.py --kernels-out profiles/point_codec_kernels.txt      (no GPU needed: compiles point_codec.hip, reads the metadata)
    rocprofv3 --kernel-trace --stats -- python bench_tools/bench_point_codec.py --trace-only    (per-kernel times of the validated G2 decompress)
"""
import argparse, faulthandler, os, re, statistics, subprocess, sys, tempfile, time
faulthandler.enable()
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(f, reps, warm=2):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def kernel_resources(out, defines=()):
    """the resource lines of every kernel of point_codec.hip, from the code object's metadata (a compile to assembly, no GPU): only what the code
    object says -- the reading of it is in DESIGN 4.6 and profiles/point_codec.txt"""
    csrc = os.path.join(ROOT, "keaki_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "point_codec.s")
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", asm, os.path.join(csrc, "point_codec.hip")] + ["-D" + d for d in defines])
        text = open(asm).read()
    keys = (".name:", ".vgpr_count:", ".agpr_count:", ".sgpr_count:", ".vgpr_spill_count:", ".sgpr_spill_count:", ".private_segment_fixed_size:")
    lines = ["# kernels of keaki_amd/csrc/point_codec.hip for gfx950: resource lines of the code object metadata (hipcc -O3 -S%s)" % "".join(" -D" + d for d in defines),
             "# scratch instructions in the whole file: %d" % len(re.findall(r"^\s*scratch_(?:load|store)", text, re.M))]
    for ln in text.splitlines():
        t = ln.strip()
        if t.startswith(keys):
            lines.append(("" if t.startswith(".name:") else "    ") + t)
    open(out, "a" if defines else "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--reps", type=int, default=11); ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.kernels_out:
        kernel_resources(a.kernels_out)
        kernel_resources(a.kernels_out, ("KEAKI_CODEC_FQ_CALLS",))      # the register-only form of the ladder's products, appended
        return
    import torch
    from bench import random_fr_limbs, SEED
    from bench_tools.bench_verify_batch import _g2_gen
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    hip = KeakiHip(0)
    nmax = 1 << max(a.log2n)
    P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    mont = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    sync = lambda: (hip.synchronize(), torch.cuda.synchronize(dev))
    d_g1p = torch.empty((nmax, 8), dtype=torch.int64, device=dev)
    d_g2p = torch.empty((nmax, 16), dtype=torch.int64, device=dev)
    hip.g1_mul_batch_dev(t(np.array(mont(1) + mont(2), np.uint64)).data_ptr(), 0, t(random_fr_limbs(nmax, SEED + 31)).data_ptr(), nmax, d_g1p.data_ptr())
    hip.g2_mul_batch_dev(t(_g2_gen()).data_ptr(), 0, t(random_fr_limbs(nmax, SEED + 32)).data_ptr(), nmax, d_g2p.data_ptr())
    sync()
    g1p, g2p = d_g1p.cpu().numpy().view(np.uint64), d_g2p.cpu().numpy().view(np.uint64)
    d_b1 = torch.empty(nmax * 32, dtype=torch.uint8, device=dev); d_b2 = torch.empty(nmax * 64, dtype=torch.uint8, device=dev)
    d_o1 = torch.empty((nmax, 8), dtype=torch.int64, device=dev); d_o2 = torch.empty((nmax, 16), dtype=torch.int64, device=dev)
    d_st = torch.empty(nmax, dtype=torch.uint8, device=dev)
    d_key = torch.empty(nmax * 32, dtype=torch.uint8, device=dev)
    hip.point_codec_dev("g1_compress", d_g1p, nmax, d_b1); hip.point_codec_dev("g2_compress", d_g2p, nmax, d_b2); sync()
    b1, b2 = d_b1.cpu().numpy().reshape(nmax, 32), d_b2.cpu().numpy().reshape(nmax, 64)
    if a.trace_only:
        for _ in range(a.reps):
            hip.point_codec_dev("g2_decompress", d_b2, nmax, d_o2, d_st, 1)
            hip.decap_batch_dev(d_g1p.data_ptr(), d_g2p.data_ptr(), nmax, None, d_key.data_ptr(), 32); sync()
        hip.close()
        return
    lines = ["# %s" % hip.version(),
             "# compressed point wire format: median of %d calls (ms) and M points/s, every call ending in a device synchronisation; warm-up 2 calls" % a.reps,
             "# dev = resident (_dev form), host = from / to host arrays (pageable numpy memory, the stager of the KEM host batches)",
             "# decap = keaki_hip_decap_batch_dev (keys out, 32 B) on the same n: the consumer that validated G2 decompression guards",
             "%-28s %6s %10s %10s %10s %10s" % ("entry", "log2n", "dev_ms", "dev_M/s", "host_ms", "host_M/s")]
    for log2n in a.log2n:
        n = 1 << log2n
        rows = [
            ("g1_compress", lambda: (hip.point_codec_dev("g1_compress", d_g1p, n, d_b1), sync()), lambda: hip.g1_compress(g1p[:n])),
            ("g1_decompress", lambda: hip.point_codec_dev("g1_decompress", d_b1, n, d_o1, d_st), lambda: hip.g1_decompress(b1[:n])),
            ("g2_compress", lambda: (hip.point_codec_dev("g2_compress", d_g2p, n, d_b2), sync()), lambda: hip.g2_compress(g2p[:n])),
            ("g2_decompress check=0", lambda: hip.point_codec_dev("g2_decompress", d_b2, n, d_o2, d_st, 0), lambda: hip.g2_decompress(b2[:n], 0)),
            ("g2_decompress check=1", lambda: hip.point_codec_dev("g2_decompress", d_b2, n, d_o2, d_st, 1), lambda: hip.g2_decompress(b2[:n], 1)),
            ("g2_subgroup_check", lambda: hip.point_codec_dev("g2_subgroup_check", d_g2p, n), lambda: hip.g2_subgroup_check(g2p[:n])),
        ]
        res = {}
        for name, fd, fh in rows:
            md, mh = median_ms(fd, a.reps), median_ms(fh, max(3, a.reps // 2))
            res[name] = md
            lines.append("%-28s %6d %10.3f %10.2f %10.3f %10.2f" % (name, log2n, md, n / md / 1e3, mh, n / mh / 1e3))
            print(lines[-1], flush=True)
        dec = median_ms(lambda: (hip.decap_batch_dev(d_g1p.data_ptr(), d_g2p.data_ptr(), n, None, d_key.data_ptr(), 32), sync()), max(3, a.reps // 2))
        lines.append("%-28s %6d %10.3f %10.2f" % ("decap_batch_dev", log2n, dec, n / dec / 1e3))
        lines.append("# 2^%d: validated G2 decompress / decap = %.3f (subgroup check alone %.3f, decompress without check %.3f)" % (
            log2n, res["g2_decompress check=1"] / dec, res["g2_subgroup_check"] / dec, res["g2_decompress check=0"] / dec))
        print("\n".join(lines[-2:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    hip.close()


if __name__ == "__main__":
    main()
