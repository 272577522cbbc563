"""Sparse PC-histogram read on the MI355X: the compaction kernel
(csrc/gpu/compact.hip) behind DeviceBucketizer.read_sparse against the
bucketizer's own dense read of the same state, and DeviceAccumulator's
read_sparse against the host accumulator. Integer counts throughout, so
every comparison is exact."""

import numpy as np
import pytest

from parca_agent_amd.gpu import events as ev
from parca_agent_amd.gpu.pcbuckets import DeviceAccumulator, HostAccumulator

from tests.test_gpu_stall_reasons import (
    CASES,
    PID,
    host_oracle,
    make_layout,
    make_stream,
)
from tests.test_pc_sparse_read import (
    EMPTY,
    assert_entry_equal,
    assert_sparse_equal,
    nonzero_view,
    run_rebuild_scenario,
)

pytestmark = pytest.mark.gpu

CO = 1
N_COLS = ev.N_STALL_COLUMNS
# One grid-stride sweep of the compaction: 2048 workgroups x 256 lanes x 4.
SWEEP = 2048 * 256 * 4

FLAG_CHOICES = np.array([
    0,                                 # host-trap: no column
    ev.pack_pc_flags(1, 0, 0, 0, 3),   # stochastic without issue info
    ev.pack_pc_flags(1, 1, 0, 2, 3),   # waitcnt
    ev.pack_pc_flags(1, 1, 0, 2, 5),   # barrier_wait
    ev.pack_pc_flags(1, 1, 1, 9, 3),   # issued
    ev.pack_pc_flags(1, 1, 0, 0, 13),  # raw reason beyond the enum
], dtype=np.uint32)


@pytest.fixture(scope="module")
def gpu_native():
    from parca_agent_amd.native import gpu

    g = gpu()
    if g.hip_device_count() == 0:
        pytest.fail("no HIP device — these tests must run on an MI355X box")
    return g


def make_bucketizer(g, total):
    """One code object of 64 * total bytes: bucket b is offset 64 * b."""
    return g.DeviceBucketizer(0, np.array([CO], dtype=np.uint64),
                              np.array([0, total], dtype=np.uint32), 6)


def samples_for(buckets, seed):
    """One sample per entry of `buckets` (repeats allowed), seeded exec
    masks (some zero) and flags drawn from FLAG_CHOICES."""
    rng = np.random.default_rng(seed)
    n = len(buckets)
    co = np.full(n, CO, dtype=np.uint64)
    off = np.asarray(buckets, dtype=np.uint64) * np.uint64(64) + \
        rng.integers(0, 64, size=n).astype(np.uint64)
    masks = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    masks[rng.random(n) < 0.2] = 0
    flags = FLAG_CHOICES[rng.integers(0, len(FLAG_CHOICES), size=n)]
    return co, off, masks, flags


def feed(b, columns, flagged):
    co, off, masks, flags = columns
    if len(co) == 0:
        return
    if flagged:
        b.accumulate_flagged(co, off, masks, flags)
    else:
        b.accumulate(co, off, masks)


def dense_nonzero(b, with_stalls=True):
    """The oracle: the bucketizer's own dense read of the current state,
    as the entries read_sparse must return."""
    if with_stalls:
        hist, lanes, overflow, stalls = b.read_stalls(False)
    else:
        hist, lanes, overflow = b.read(False)
        stalls = None
    nz = np.nonzero(hist)[0]
    rows = stalls[nz] if stalls is not None else \
        np.zeros((len(nz), N_COLS), dtype=np.uint32)
    return nz.astype(np.uint32), hist[nz], lanes[nz], rows, overflow


def assert_native_equal(got, want):
    assert len(got) == 5
    buckets, counts, lanes, stalls, overflow = got
    assert buckets.dtype == counts.dtype == stalls.dtype == np.uint32
    assert lanes.dtype == np.uint64 and overflow.dtype == np.uint32
    assert stalls.shape == (len(buckets), N_COLS) and overflow.shape == (2,)
    assert counts.shape == lanes.shape == buckets.shape
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def pattern_buckets(pattern, total):
    if pattern == "none":
        return np.zeros(0, dtype=np.int64)
    if pattern == "first":
        return np.zeros(3, dtype=np.int64)
    if pattern == "last":
        return np.full(3, total - 1, dtype=np.int64)
    if pattern == "all":  # exactly one sample per bucket: capacity == k
        return np.random.default_rng(total).permutation(total)
    assert pattern == "random"
    rng = np.random.default_rng(1000 + total)
    chosen = np.flatnonzero(rng.random(total) < 0.1)
    if len(chosen) == 0:
        chosen = np.array([total // 2])
    return rng.permutation(np.repeat(chosen, 3))


PATTERNS = ("none", "first", "last", "all", "random")
# Scalar tail only; one vector; vector + tail; 4 * 256 + 3 = one full
# workgroup plus tail.
SMALL_TOTALS = (1, 3, 4, 5, 97, 1027)
SMALL_CASES = [(t, p, True) for t in SMALL_TOTALS for p in PATTERNS] + \
    [(t, p, False) for t in (97, 1027) for p in PATTERNS]


@pytest.mark.parametrize("total,pattern,flagged", SMALL_CASES)
def test_read_sparse_matches_dense_small(gpu_native, total, pattern, flagged):
    b = make_bucketizer(gpu_native, total)
    buckets = pattern_buckets(pattern, total)
    feed(b, samples_for(buckets, seed=total), flagged)
    want = dense_nonzero(b)
    got = b.read_sparse(False)
    assert_native_equal(got, want)
    assert len(got[0]) == len(np.unique(buckets))
    if pattern == "all":
        assert len(got[0]) == total == len(buckets)
    if not flagged:
        assert not got[3].any()
    elif len(buckets) >= 97:
        assert got[3].any() and (got[3].sum(axis=1) <= got[1]).all()
        assert (got[3].sum(axis=1) < got[1]).any()
    if len(buckets) >= 97:
        assert (got[2] == 0).sum() < len(got[0])  # lanes are carried


def test_read_sparse_global_stream(gpu_native):
    """total = 40 000: the `global` stream of the stall-reason tests."""
    samples = host_oracle("global")[0]
    total = 40_000
    b = make_bucketizer(gpu_native, total)
    co, off, masks, flags, _ = gpu_native.split_pc_samples(samples)
    co = np.where(co == 5, np.uint64(CO), co)  # that stream's code object
    b.accumulate_flagged(co, off, masks, flags)
    want = dense_nonzero(b)
    got = b.read_sparse(False)
    assert_native_equal(got, want)
    assert len(got[0]) == 9204          # of 40 000, as the host computes
    assert got[4][0] > 0 and got[4][1] > 0
    assert 0 < got[3].any(axis=1).sum() < len(got[0])


def test_read_sparse_crosses_grid_stride_boundary(gpu_native):
    """Two sweeps plus a workgroup's worth and a scalar tail, unflagged: no
    stall matrix is allocated, so the device footprint stays ~25 MiB."""
    total = SWEEP + 1027
    rng = np.random.default_rng(77)
    edge = np.array([0, SWEEP - 1, SWEEP, total - 1])
    buckets = np.concatenate([edge, edge[1:3],
                              rng.integers(0, total, size=1000)])
    b = make_bucketizer(gpu_native, total)
    feed(b, samples_for(buckets, seed=78), flagged=False)
    want = dense_nonzero(b, with_stalls=False)
    got = b.read_sparse(False)
    assert_native_equal(got, want)
    assert len(got[0]) == len(np.unique(buckets))
    assert set(edge.tolist()) <= set(got[0].tolist())
    assert not got[3].any()
    # clearing across the boundary too
    assert_native_equal(b.read_sparse(True), want)
    hist, lanes, overflow = b.read(False)
    assert not hist.any() and not lanes.any() and not overflow.any()


def test_read_sparse_reset_semantics(gpu_native):
    total = 1027
    b = make_bucketizer(gpu_native, total)
    columns = samples_for(pattern_buckets("random", total), seed=5)
    # some unknown-object and out-of-range samples on top
    extra = (np.array([9, 9, CO], dtype=np.uint64),
             np.array([0, 64, 64 * total], dtype=np.uint64),
             np.array([1, 1, 1], dtype=np.uint64),
             np.array([0, 0, 0], dtype=np.uint32))
    columns = tuple(np.concatenate([c, e]) for c, e in zip(columns, extra))
    feed(b, columns, flagged=True)
    dense_before = b.read_stalls(False)
    want = dense_nonzero(b)
    np.testing.assert_array_equal(want[4], [2, 1])
    assert len(want[0]) > 50 and want[3].any()

    # not resetting: repeatable, and the dense state is untouched
    assert_native_equal(b.read_sparse(False), want)
    assert_native_equal(b.read_sparse(False), want)
    for g, w in zip(b.read_stalls(False), dense_before):
        np.testing.assert_array_equal(g, w)

    # resetting: same entries, then everything is zero, overflow included
    assert_native_equal(b.read_sparse(True), want)
    for arr in b.read_stalls(False):
        assert not arr.any()
    empty = b.read_sparse(True)
    assert all(len(a) == 0 for a in empty[:4]) and not empty[4].any()
    assert empty[3].shape == (0, N_COLS)

    # the in-place clear was complete and the sample counter restarted:
    # the same stream gives the same entries again
    feed(b, columns, flagged=True)
    assert_native_equal(b.read_sparse(True), want)
    for arr in b.read_stalls(False):
        assert not arr.any()

    # the dense resets restart the counter as well
    feed(b, columns, flagged=True)
    b.read_stalls(True)
    empty = b.read_sparse(False)
    assert len(empty[0]) == 0 and not empty[4].any()
    feed(b, columns, flagged=True)
    assert_native_equal(b.read_sparse(False), want)


def test_read_sparse_overflow_words(gpu_native):
    total = 97
    b = make_bucketizer(gpu_native, total)
    # only misses: the kernel runs (samples were accumulated) and emits
    # nothing
    misses = (np.array([7, CO, CO, 8], dtype=np.uint64),
              np.array([0, 64 * total, 64 * (total + 5), 64], dtype=np.uint64),
              np.ones(4, dtype=np.uint64), np.zeros(4, dtype=np.uint32))
    feed(b, misses, flagged=True)
    want = dense_nonzero(b)
    np.testing.assert_array_equal(want[4], [2, 2])
    got = b.read_sparse(False)
    assert_native_equal(got, want)
    assert len(got[0]) == 0
    # hits and misses mixed
    feed(b, samples_for(np.arange(0, total, 3), seed=9), flagged=True)
    feed(b, misses, flagged=False)
    want = dense_nonzero(b)
    np.testing.assert_array_equal(want[4], [4, 4])
    assert_native_equal(b.read_sparse(True), want)
    assert not b.read(False)[2].any()


# -- DeviceAccumulator -------------------------------------------------------


@pytest.mark.parametrize("name", list(CASES))
def test_device_accumulator_read_sparse_matches_host(gpu_native, name):
    sizes, _, _ = CASES[name]
    samples, h_hist, h_lanes, h_stalls, h_unknown, h_range = \
        host_oracle(name)
    dev = DeviceAccumulator(make_layout(sizes), device=0)
    dev.accumulate(PID, samples)
    got = dev.read_sparse()
    # HostAccumulator.read_sparse of these samples, from the shared oracle
    # (equal by test_pc_sparse_read)
    assert list(got) == [-1]
    assert_entry_equal(got[-1], nonzero_view(h_hist, h_lanes, h_stalls))
    assert dev.unknown_code_object == h_unknown
    assert dev.out_of_range == h_range
    assert got[-1][3].any()
    for entry in dev.read_sparse().values():
        assert_entry_equal(entry, EMPTY)
    assert (dev.unknown_code_object, dev.out_of_range) == (h_unknown, h_range)


def test_read_sparse_survives_layout_rebuild(gpu_native):
    """The scenario of test_mixed_batches_survive_layout_rebuild — flagged
    batch, host-trap batch, layout grows, flagged batch — ending in the
    sparse read on both sides."""
    sizes = {11: 4096, 22: 2048}
    grown = dict(sizes)
    grown[33] = 64
    layout = make_layout(sizes)
    host = HostAccumulator(layout)
    dev = DeviceAccumulator(layout, device=0)

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

    want = host.read_sparse()
    got = dev.read_sparse()
    assert_sparse_equal(got, want)
    assert dev.unknown_code_object == host.unknown_code_object
    assert dev.out_of_range == host.out_of_range
    buckets, hist, _, stalls = got[-1]
    assert buckets[-1] == 96 and stalls[-1].sum() > 0  # the new code object
    assert 0 < stalls.sum() < hist.sum()


def test_interleaved_pids_rebuild_and_hand_over_on_device(gpu_native):
    """The CPU folding scenario of test_pc_sparse_read (two pids
    interleaved in the layout, two gpus, hand-over, rebuild) with the real
    bucketizers underneath, sparse and dense."""
    def factory(layout):
        return DeviceAccumulator(layout, device=0)

    host, dev = run_rebuild_scenario(factory)
    assert_sparse_equal(dev.read_sparse(), host.read_sparse())
    assert dev.unknown_code_object == host.unknown_code_object
    assert dev.out_of_range == host.out_of_range

    host, dev = run_rebuild_scenario(factory)
    want = host.read_with_stalls()
    got = dev.read_with_stalls()
    for gpu in want:
        for g, w in zip(got[gpu], want[gpu]):
            np.testing.assert_array_equal(g, w)
