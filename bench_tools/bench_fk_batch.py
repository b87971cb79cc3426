#!/usr/bin/env python3
"""Batched vec_commit (keaki_hip_vec_commit_batch) against the only route the library had before it: a loop of m keaki_hip_vec_commit calls
on one context.

One device, one process, warm, per cell (log2d, m) = (8, 256), (8, 4096), (10, 1024), (12, 64), alternating: the batch call from host memory,
the loop of m single calls from host memory, the batch call again (the smaller of the two medians counts). Every measurement ends in a
device synchronisation; the median of --reps runs (at least five). Beside the host clock, the device time alone: stream events around the
batch call with resident rows (_dev form), and around every single call of the loop, summed, in the same runs as the host clock (two event
records beside a call of 13 ms and more; a single call is launch-bound: its events span the gaps between its launches). The context runs on a caller-created stream so that the events
and the calls share it. Rows of d random evaluations (n = d), an SRS of 4,096 random points without window tables.

openings/s = m d / time, to hold against the single call at d = 2^21 (2^21 openings in 0.41 s = 5.1 M/s).

    python bench_tools/bench_fk_batch.py --out profiles/fk_batch_times.txt
    rocprofv3 --kernel-trace --stats -- python bench_tools/bench_fk_batch.py --trace-only      # five batch calls at (log2d, m) = (8, 4096)
"""
import argparse, faulthandler, os, statistics, sys, time
faulthandler.enable()
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import random_fr_limbs, SEED  # noqa: E402

CELLS = [(8, 256), (8, 4096), (10, 1024), (12, 64)]
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def fr_mont(v):
    return np.array([((v % R << 256) % R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], np.uint64)


def domain_consts(log2d):
    """(omega_d^-1, 1/d, omega_2d, omega_2d^-1, 1/2d) of ark-poly's Radix2EvaluationDomain, Montgomery limbs"""
    d = 1 << log2d
    w2 = pow(pow(5, (R - 1) >> 28, R), (1 << 28) // (2 * d), R)
    return [fr_mont(x) for x in (pow(w2 * w2, -1, R), pow(d, -1, R), w2, pow(w2, -1, R), pow(2 * d, -1, R))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--out", default=None)
    ap.add_argument("--cells", default=None, help="log2d:m,... instead of the four cells of the profile")
    ap.add_argument("--trace-only", action="store_true", help="five batch _dev calls at (log2d, m) = (8, 4096): the run to put under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    assert a.reps >= 5, "the median of at least five runs"
    import torch
    from keaki_amd.hip import KeakiHip
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    hip = KeakiHip(0, stream=stream.cuda_stream)
    cells = CELLS if not a.cells else [tuple(int(x) for x in c.split(":")) for c in a.cells.split(",")]
    P_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    mont = lambda v: [((v << 256) % P_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    g1 = np.array(mont(1) + mont(2), np.uint64)
    srs = hip.srs_g1_upload(hip.g1_mul_batch(g1, random_fr_limbs(1 << max(l for l, _ in cells), SEED + 31)))
    pool = random_fr_limbs(1 << 20, SEED + 32)
    pool[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def events(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median(f, reps, warm=1):
        for _ in range(warm):
            f()
        return statistics.median(f() for _ in range(reps))

    def host_ms(f):
        t0 = time.perf_counter()
        f()
        hip.synchronize()
        return (time.perf_counter() - t0) * 1e3

    if a.trace_only:
        log2d, m = 8, 4096
        d, c = 1 << log2d, domain_consts(log2d)
        with torch.cuda.stream(stream):
            d_rows = torch.from_numpy(np.resize(pool, (m * d, 4)).view(np.int64)).to(dev)
            d_com, d_pr = torch.empty((m, 12), dtype=torch.int64, device=dev), torch.empty((m * d, 8), dtype=torch.int64, device=dev)
        for _ in range(5):
            hip.vec_commit_batch_dev(srs, d_rows.data_ptr(), d, m, d, log2d, *c, d_com.data_ptr(), d_pr.data_ptr())
        hip.synchronize()
        return
    say("# bench_fk_batch: %s, median of %d runs, ms (version %s)" % (torch.cuda.get_device_name(0), a.reps, hip.version()))
    say("# clock: not pinned. The shader clock of these boxes moves with the load (1.5 GHz under the field arithmetic, 2.4 GHz idle:")
    say("# profiles/r05_ubench_clock.txt); both columns of a row were measured alternately in the same process on the same box.")
    say("# host = host arrays in and out, host clock; dev = stream events (batch: _dev form; loop: around every single call, summed)")
    say("# %5s %6s %12s %12s %12s %12s %10s %10s %14s" % ("log2d", "m", "batch_host", "loop_host", "batch_dev", "loop_dev", "host x", "dev x", "batch Mopen/s"))
    for log2d, m in cells:
        d, c = 1 << log2d, domain_consts(log2d)
        rows = np.resize(pool, (m, d, 4))
        with torch.cuda.stream(stream):
            d_rows = torch.from_numpy(rows.view(np.int64)).to(dev)
            d_com, d_pr = torch.empty((m, 12), dtype=torch.int64, device=dev), torch.empty((m * d, 8), dtype=torch.int64, device=dev)
        stream.synchronize()
        singles = [np.ascontiguousarray(rows[j]) for j in range(m)]

        batch = lambda: hip.vec_commit_batch(srs, rows, log2d, *c)
        batch_dev = lambda: hip.vec_commit_batch_dev(srs, d_rows.data_ptr(), d, m, d, log2d, *c, d_com.data_ptr(), d_pr.data_ptr())
        # the results agree before anything is timed
        com, pr = batch()
        for j in (0, m - 1):
            one = hip.vec_commit(srs, singles[j], None, log2d, *c)
            assert np.array_equal(com[j], one[0]) and np.array_equal(pr[j], one[1])

        def loop_both():
            """one run of the loop: (host clock of the m calls, sum of the events around every call)"""
            ev = 0.0
            t0 = time.perf_counter()
            for j in range(m):
                ev += events(lambda: hip.vec_commit(srs, singles[j], None, log2d, *c))
            return (time.perf_counter() - t0) * 1e3, ev

        tb = median(lambda: host_ms(batch), a.reps)
        eb = median(lambda: events(batch_dev), a.reps)
        runs = []
        for r in range(a.reps):                     # the rows above warmed every workspace of the single call
            runs.append(loop_both())
            print("#   loop run %d of %d at (%d, %d): %.1f ms" % (r + 1, a.reps, log2d, m, runs[-1][0]), flush=True)
        tl, el = statistics.median(x[0] for x in runs), statistics.median(x[1] for x in runs)
        tb = min(tb, median(lambda: host_ms(batch), a.reps))
        eb = min(eb, median(lambda: events(batch_dev), a.reps))
        say("  %5d %6d %12.3f %12.3f %12.3f %12.3f %10.1f %10.1f %14.3f" % (log2d, m, tb, tl, eb, el, tl / tb, el / eb, m * d / tb / 1e3))
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        del d_rows, d_com, d_pr
    say("# the single call at d = 2^21: 2^21 openings in 0.41 s = 5.1 Mopen/s")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
