#!/usr/bin/env python3
"""rocprofv3 target: run the CDNA4 bucketize kernel in a tight loop so
per-kernel stats/counters can be collected (profiles/ evidence).

Usage: profile_bucketize.py [n] [iters] [--stalls] [--reps R]
       profile_bucketize.py --sparse [--reps R]

--stalls gives the same synthetic stream PCSample.flags with issue info
(about 30 % of samples keep flags 0), so the stall-reason launch paths run
instead of the flag-less ones. Each of the R repetitions times `iters`
accumulates of both streams plus the read-back and prints its rate.

--sparse times the read-back alone: one DeviceBucketizer over the largest
layout (1 << 22 buckets), flagged samples touching about 1 % of them, then
the dense read_stalls(False) and the compacting read_sparse(False)
alternated on that one device state. A host clock runs around each call;
both calls end in a device synchronise."""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from parca_agent_amd.gpu import events as ev
from parca_agent_amd.gpu.events import PC_SAMPLE_DTYPE
from parca_agent_amd.gpu.pcbuckets import BucketLayout, DeviceAccumulator


def sparse_readback(reps):
    from parca_agent_amd.native import gpu as native_gpu

    g = native_gpu()
    if g.hip_device_count() == 0:
        raise SystemExit("no HIP device")
    total = 1 << 22
    rng = np.random.default_rng(2)
    touched = rng.choice(total, size=total // 100, replace=False)
    n = 4 * len(touched)   # 4 samples per touched bucket, shuffled
    buckets = rng.permutation(np.repeat(touched, 4)).astype(np.uint64)
    co = np.ones(n, dtype=np.uint64)
    off = buckets * np.uint64(64)
    masks = rng.integers(1, 1 << 63, size=n, dtype=np.uint64)
    flags = (rng.integers(0, 16, size=n).astype(np.uint32)
             << ev.PC_FLAG_REASON_SHIFT) | np.uint32(
                 ev.PC_FLAG_STOCHASTIC | ev.PC_FLAG_ISSUE_VALID)
    flags[rng.random(n) < 0.3] = 0
    b = g.DeviceBucketizer(0, np.array([1], dtype=np.uint64),
                           np.array([0, total], dtype=np.uint32), 6)
    b.accumulate_flagged(co, off, masks, flags)

    # Warm-up of both, and the check that they agree on this state.
    hist, lanes, _, stalls = b.read_stalls(False)
    sb, sc, sl, ss, _ = b.read_sparse(False)
    nz = np.flatnonzero(hist)
    assert np.array_equal(sb, nz) and np.array_equal(sc, hist[nz])
    assert np.array_equal(sl, lanes[nz]) and np.array_equal(ss, stalls[nz])
    dense_bytes = hist.nbytes + lanes.nbytes + stalls.nbytes
    sparse_bytes = sb.nbytes + sc.nbytes + sl.nbytes + ss.nbytes
    del hist, lanes, stalls

    dense_ms, sparse_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        b.read_stalls(False)
        t1 = time.perf_counter()
        b.read_sparse(False)
        t2 = time.perf_counter()
        dense_ms.append((t1 - t0) * 1e3)
        sparse_ms.append((t2 - t1) * 1e3)
    print(f"mode=sparse total_buckets={total} touched={len(nz)} "
          f"samples={n} reps={reps}")
    print(f"bytes copied to host per read: dense={dense_bytes} "
          f"sparse={sparse_bytes}")
    for name, ms in (("dense read_stalls(False)", dense_ms),
                     ("sparse read_sparse(False)", sparse_ms)):
        print(f"{name} ms={[round(m, 3) for m in ms]} "
              f"median={np.median(ms):.3f} min={min(ms):.3f} "
              f"max={max(ms):.3f}")
    print(f"slowest sparse {max(sparse_ms):.3f} ms vs fastest dense "
          f"{min(dense_ms):.3f} ms: "
          f"{'sparse faster' if max(sparse_ms) < min(dense_ms) else 'NOT faster'}"
          f"; median ratio {np.median(dense_ms) / np.median(sparse_ms):.1f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=4_000_000)
    ap.add_argument("iters", nargs="?", type=int, default=20)
    ap.add_argument("--stalls", action="store_true",
                    help="flag the samples: stall-reason kernels")
    ap.add_argument("--reps", type=int, default=1,
                    help="timed repetitions after one warm-up")
    ap.add_argument("--sparse", action="store_true",
                    help="time dense against sparse read-back instead")
    args = ap.parse_args()
    if args.sparse:
        sparse_readback(args.reps)
        return
    n, iters = args.n, args.iters

    rng = np.random.default_rng(1)
    layout = BucketLayout(bucket_shift=6)
    layout.add(pid=1, code_object_id=1, load_size=1 << 20)  # 16K buckets: LDS path
    layout.add(pid=2, code_object_id=1, load_size=64 * 40000)  # 40K: global path
    dev = DeviceAccumulator(layout, device=0)
    samples = np.zeros(n, dtype=PC_SAMPLE_DTYPE)
    samples["code_object_id"] = 1
    samples["code_object_offset"] = rng.integers(0, 1 << 20, size=n)
    samples["exec_mask"] = rng.integers(1, 1 << 63, size=n, dtype=np.uint64)
    big = samples.copy()
    big["code_object_offset"] = rng.integers(0, 64 * 40000, size=n)
    # Drawn whether used or not, so both modes see the same stream.
    flags = (rng.integers(0, 16, size=n).astype(np.uint32)
             << ev.PC_FLAG_REASON_SHIFT) | np.uint32(
                 ev.PC_FLAG_STOCHASTIC | ev.PC_FLAG_ISSUE_VALID)
    flags[rng.random(n) < 0.2] |= np.uint32(ev.PC_FLAG_WAVE_ISSUED)
    flags[rng.random(n) < 0.3] = 0
    if args.stalls:
        samples["flags"] = flags
        big["flags"] = flags

    def one_rep():
        for _ in range(iters):
            dev.accumulate(1, samples)   # LDS-staged variant
            dev.accumulate(2, big)       # global-atomics variant
        if args.stalls:
            hist, _, stalls = dev.read_with_stalls()[-1]
            return int(hist.sum()), int(stalls.sum())
        hist, _ = dev.read()[-1]
        return int(hist.sum()), 0

    one_rep()  # warm-up: allocations, code-object load
    rates = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        total, stalled = one_rep()
        dt = time.perf_counter() - t0
        rates.append(2 * iters * n / dt / 1e6)
        print(f"rep: {rates[-1]:.1f} M samples/s")
    print("total bucketed:", total, "with stall column:", stalled)
    print(f"mode={'stalls' if args.stalls else 'plain'} n={n} iters={iters} "
          f"rates_M_per_s={[round(r, 1) for r in rates]} "
          f"median={np.median(rates):.1f} min={min(rates):.1f} "
          f"max={max(rates):.1f}")


if __name__ == "__main__":
    main()
