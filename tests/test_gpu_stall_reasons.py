"""Stall-reason breakdown on the MI355X: the bucketize kernel's stall
matrix against the host accumulator on the same samples, one case per
launch path the flagged entry point can take. Integer counts throughout,
so every comparison is exact."""

import time

import numpy as np
import pytest

from parca_agent_amd.gpu import events as ev
from parca_agent_amd.gpu.pcbuckets import (
    BucketLayout,
    DeviceAccumulator,
    HostAccumulator,
)

PID = 10
UNKNOWN_CO = 999

# name -> (code object id -> load size at shift 6, n samples, seed).
# LDS budget 128 KiB: 72 B/bucket fully staged (<= 1820 buckets), 8 B with
# counts+lanes staged (<= 16384), 4 B counts only (<= 32768), else global.
SMALL = {11: 4096, 22: 2048, 33: 64}          # 64 + 32 + 1 = 97 buckets
CASES = {
    # The two tiny streams use the first seeds whose 3 or 4 samples pass
    # test_generated_inputs_discriminate (most seeds cannot at that size).
    "full_tail_only": (SMALL, 3, 11),          # one workgroup, no vector step
    "full_one_vector": (SMALL, 4, 35),
    "full_five_workgroups": (SMALL, 4099, 3),  # 5 workgroups + tail of 3
    "partial_counts_and_lanes": ({5: 64 * 4096}, 20_000, 4),
    "partial_counts_only": ({5: 64 * 20_000}, 20_000, 5),
    "global": ({5: 64 * 40_000}, 50_000, 6),
}


def make_stream(sizes, n, seed):
    """Time-correlated synthetic PC samples: runs of 1-8 equal PCs; about
    5 % unknown code object, about 1 % past the end of their code object;
    about 30 % flags 0, a few stochastic-without-issue-info, the rest with
    issue info and reasons drawn from all 16 raw values. Half the runs
    keep one flags word throughout (stall runs merge), the other half
    draw it per sample (the column changes inside the run)."""
    rng = np.random.default_rng(seed)
    run_len = rng.integers(1, 9, size=n)
    run_of = np.repeat(np.arange(n), run_len)[:n]
    n_runs = int(run_of[-1]) + 1

    cos = np.array(list(sizes) + [UNKNOWN_CO], dtype=np.uint64)
    weight = np.array([sizes[c] for c in sizes], dtype=np.float64)
    p = np.append(0.95 * weight / weight.sum(), 0.05)
    run_co = rng.choice(len(cos), size=n_runs, p=p)
    limit = np.array([sizes[c] for c in sizes] + [1 << 16])[run_co]
    run_off = rng.integers(0, limit)
    past_end = rng.random(n_runs) < 0.01
    run_off = np.where(past_end, limit + run_off, run_off)

    def draw_flags(k):
        f = np.array([ev.pack_pc_flags(1, 1, 0, 0, 0)], dtype=np.uint32) | \
            (rng.integers(0, 32, size=k).astype(np.uint32)
             << ev.PC_FLAG_INST_TYPE_SHIFT) | \
            (rng.integers(0, 16, size=k).astype(np.uint32)
             << ev.PC_FLAG_REASON_SHIFT) | \
            np.where(rng.random(k) < 0.2, ev.PC_FLAG_WAVE_ISSUED,
                     0).astype(np.uint32)
        u = rng.random(k)
        f = np.where(u < 0.03, f & ~np.uint32(ev.PC_FLAG_ISSUE_VALID), f)
        return np.where(u >= 0.70, np.uint32(0), f).astype(np.uint32)

    per_run = draw_flags(n_runs)[run_of]
    per_sample = draw_flags(n)
    uniform_run = (rng.random(n_runs) < 0.5)[run_of]

    samples = np.zeros(n, dtype=ev.PC_SAMPLE_DTYPE)
    samples["code_object_id"] = cos[run_co][run_of]
    samples["code_object_offset"] = run_off[run_of]
    samples["exec_mask"] = rng.integers(1, 1 << 63, size=n, dtype=np.uint64)
    samples["flags"] = np.where(uniform_run, per_run, per_sample)
    return samples


def make_layout(sizes):
    layout = BucketLayout(bucket_shift=6)
    for co, size in sizes.items():
        layout.add(pid=PID, code_object_id=co, load_size=size)
    return layout


_ORACLE = {}


def host_oracle(name):
    """(samples, hist, lanes, stalls, unknown, out_of_range) of one case,
    computed once by the host accumulator and then left alone."""
    if name not in _ORACLE:
        sizes, n, seed = CASES[name]
        samples = make_stream(sizes, n, seed)
        host = HostAccumulator(make_layout(sizes))
        host.accumulate(PID, samples)
        hist, lanes, stalls = host.read_with_stalls()[-1]
        for arr in (samples, hist, lanes, stalls):
            arr.setflags(write=False)
        _ORACLE[name] = (samples, hist, lanes, stalls,
                         host.unknown_code_object, host.out_of_range)
    return _ORACLE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_generated_inputs_discriminate(name):
    """CPU check of the inputs themselves: some, but not all, bucketed
    samples carry a stall column, so neither a kernel that writes no
    stall counts nor one that counts every sample can pass below."""
    samples, hist, _, stalls, _, _ = host_oracle(name)
    assert len(samples) == CASES[name][1]
    assert 0 < stalls.sum() < hist.sum()
    assert (stalls.sum(axis=1) <= hist).all()
    assert not stalls[:, 10:14].any()


def test_generated_stream_shape():
    """The big streams really are what the cases are meant to exercise."""
    samples, hist, _, stalls, unknown, out_of_range = host_oracle("global")
    n = len(samples)
    assert 0.25 < (samples["flags"] == 0).mean() < 0.35
    assert 0.03 < unknown / n < 0.07
    assert out_of_range > 0
    reasons = (samples["flags"] >> ev.PC_FLAG_REASON_SHIFT) & 0xF
    assert set(reasons[samples["flags"] != 0].tolist()) == set(range(16))
    assert stalls[:, 14].sum() > 0 and stalls[:, 15].sum() > 0
    # runs: neighbours mostly share a PC, and columns change inside runs
    same_pc = (samples["code_object_offset"][1:] ==
               samples["code_object_offset"][:-1])
    assert same_pc.mean() > 0.5
    cols = ev.stall_column(samples["flags"])
    assert (same_pc & (cols[1:] != cols[:-1])).sum() > n // 20
    assert (same_pc & (cols[1:] == cols[:-1]) & (cols[1:] >= 0)).sum() \
        > n // 20


# -- device ----------------------------------------------------------------


@pytest.fixture(scope="module")
def gpu_native():
    from parca_agent_amd.native import gpu

    g = gpu()
    if g.hip_device_count() == 0:
        pytest.fail("no HIP device — these tests must run on an MI355X box")
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_stall_matrix_matches_host(gpu_native, name):
    sizes, _, _ = CASES[name]
    samples, h_hist, h_lanes, h_stalls, h_unknown, h_range = \
        host_oracle(name)
    dev = DeviceAccumulator(make_layout(sizes), device=0)
    dev.accumulate(PID, samples)
    d_hist, d_lanes, d_stalls = dev.read_with_stalls()[-1]

    assert d_stalls.shape == h_stalls.shape and d_stalls.dtype == np.uint64
    np.testing.assert_array_equal(d_hist, h_hist)
    np.testing.assert_array_equal(d_lanes, h_lanes)
    np.testing.assert_array_equal(d_stalls, h_stalls)
    assert dev.unknown_code_object == h_unknown
    assert dev.out_of_range == h_range
    assert d_stalls.sum() > 0
    assert d_stalls.sum() < d_hist.sum()

    # drained: a second read is all zero, stall matrix included
    for hist, lanes, stalls in dev.read_with_stalls().values():
        assert not hist.any() and not lanes.any() and not stalls.any()


class _SpyBucketizer:
    """Forwards to a DeviceBucketizer, recording which entry point each
    batch took."""

    def __init__(self, real, calls):
        self._real = real
        self._calls = calls

    def accumulate(self, *args):
        self._calls.append("plain")
        return self._real.accumulate(*args)

    def accumulate_flagged(self, *args):
        self._calls.append("flagged")
        return self._real.accumulate_flagged(*args)

    def __getattr__(self, name):
        return getattr(self._real, name)


class _SpyNative:
    def __init__(self, real, calls):
        self._real = real
        self._calls = calls

    def DeviceBucketizer(self, *args):
        return _SpyBucketizer(self._real.DeviceBucketizer(*args),
                              self._calls)

    def __getattr__(self, name):
        return getattr(self._real, name)


@pytest.mark.gpu
def test_mixed_batches_survive_layout_rebuild(gpu_native):
    """Flagged batch, host-trap batch (old entry point), layout grows,
    flagged batch: totals and stall rows must match the host."""
    sizes = {11: 4096, 22: 2048}
    grown = dict(sizes)
    grown[33] = 64
    layout = make_layout(sizes)
    host = HostAccumulator(layout)
    dev = DeviceAccumulator(layout, device=0)
    calls = []
    dev._native = _SpyNative(dev._native, calls)

    first = make_stream(grown, 5000, 21)    # code object 33 still unknown
    second = make_stream(grown, 3001, 22)
    second["flags"] = 0
    third = make_stream(grown, 4002, 23)
    for batch in (first, second):
        host.accumulate(PID, batch)
        dev.accumulate(PID, batch)
    layout.add(pid=PID, code_object_id=33, load_size=64)
    dev.layout_changed()
    host.accumulate(PID, third)
    dev.accumulate(PID, third)
    assert calls == ["flagged", "plain", "flagged"]

    h_hist, h_lanes, h_stalls = host.read_with_stalls()[-1]
    d_hist, d_lanes, d_stalls = dev.read_with_stalls()[-1]
    assert d_stalls.shape == (97, 16)
    np.testing.assert_array_equal(d_hist, h_hist)
    np.testing.assert_array_equal(d_lanes, h_lanes)
    np.testing.assert_array_equal(d_stalls, h_stalls)
    assert dev.unknown_code_object == host.unknown_code_object
    assert dev.out_of_range == host.out_of_range
    assert 0 < d_stalls.sum() < d_hist.sum()
    assert d_hist[96] > 0 and d_stalls[96].sum() > 0  # the new code object


@pytest.mark.gpu
def test_flagged_bucketize_throughput(gpu_native):
    """Same shape as test_bucketize_throughput, through the flagged entry
    point: the project's floor of 100 M samples/s must still hold."""
    rng = np.random.default_rng(1)
    layout = BucketLayout(bucket_shift=6)
    layout.add(pid=1, code_object_id=1, load_size=1 << 20)
    dev = DeviceAccumulator(layout, device=0)
    n = 4_000_000
    samples = np.zeros(n, dtype=ev.PC_SAMPLE_DTYPE)
    samples["code_object_id"] = 1
    samples["code_object_offset"] = rng.integers(0, 1 << 20, size=n)
    samples["exec_mask"] = 1
    flags = (rng.integers(0, 16, size=n).astype(np.uint32)
             << ev.PC_FLAG_REASON_SHIFT) | np.uint32(3)
    flags[rng.random(n) < 0.3] = 0
    samples["flags"] = flags
    with_column = int((flags != 0).sum())
    dev.accumulate(1, samples)  # warm
    dev.read_with_stalls()
    t0 = time.perf_counter()
    for _ in range(5):
        dev.accumulate(1, samples)
    hist, _, stalls = dev.read_with_stalls()[-1]
    dt = time.perf_counter() - t0
    rate = 5 * n / dt
    print(f"flagged bucketize rate: {rate/1e6:.1f} M samples/s")
    assert hist.sum() == 5 * n
    assert stalls.sum() == 5 * with_column
    assert rate > 100e6
