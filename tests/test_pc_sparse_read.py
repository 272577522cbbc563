"""Sparse PC-histogram read, CPU side: HostAccumulator.read_sparse against
its own dense read, DeviceAccumulator's sparse folding over a numpy
stand-in for the native bucketizer, its steady-state allocations, and the
service's flush fed from the sparse read against the dense one. Integer
counts throughout, so every comparison is exact."""

import os
import tracemalloc

import numpy as np
import pytest

from parca_agent_amd.elf import ELFFile
from parca_agent_amd.gpu import events as ev
from parca_agent_amd.gpu.pcbuckets import (
    BucketLayout,
    DeviceAccumulator,
    HostAccumulator,
)
from parca_agent_amd.gpu.service import GPUProfilerService

from tests.test_gpu_service import fake_code_object  # noqa: F401  (fixture)
from tests.test_gpu_stall_reasons import (
    CASES,
    PID,
    host_oracle,
    make_layout,
    make_stream,
)

N_COLS = ev.N_STALL_COLUMNS


def nonzero_view(hist, lanes, stalls):
    """What read_sparse must return for one gpu's dense arrays."""
    nz = np.nonzero(hist)[0]
    return nz.astype(np.int64), hist[nz], lanes[nz], stalls[nz]


def assert_entry_equal(got, want):
    buckets, hist, lanes, stalls = got
    assert buckets.dtype == np.int64
    assert hist.dtype == lanes.dtype == stalls.dtype == np.uint64
    assert stalls.shape == (len(buckets), N_COLS)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert (np.diff(buckets) > 0).all()  # ascending, no duplicates


EMPTY = (np.zeros(0, np.int64), np.zeros(0, np.uint64),
         np.zeros(0, np.uint64), np.zeros((0, N_COLS), np.uint64))


def assert_sparse_equal(got, want):
    """Two read_sparse results; a gpu may be absent where it has k == 0."""
    for gpu in set(got) | set(want):
        assert_entry_equal(got.get(gpu, EMPTY), want.get(gpu, EMPTY))


# -- host accumulator ------------------------------------------------------


@pytest.mark.parametrize("name", list(CASES))
def test_host_read_sparse_is_nonzero_view_of_dense(name):
    sizes, _, _ = CASES[name]
    samples, hist, lanes, stalls, unknown, out_of_range = host_oracle(name)
    host = HostAccumulator(make_layout(sizes))
    host.accumulate(PID, samples)

    got = host.read_sparse(False)
    assert list(got) == [-1]
    assert_entry_equal(got[-1], nonzero_view(hist, lanes, stalls))
    k, total = len(got[-1][0]), len(hist)
    with_stalls = int(got[-1][3].any(axis=1).sum())
    print(f"{name}: k/total = {k}/{total}, rows with stalls {with_stalls}")
    # The inputs must keep telling "emit nothing", "emit everything" and
    # "emit rows with stall counts only" apart.
    assert 0 < k
    if name in ("partial_counts_and_lanes", "partial_counts_only", "global"):
        assert k < total
        assert with_stalls < k
    assert (host.unknown_code_object, host.out_of_range) == \
        (unknown, out_of_range)

    # not reset: the dense read still sees everything
    dense = host.read_with_stalls(False)[-1]
    for g, w in zip(dense, (hist, lanes, stalls)):
        np.testing.assert_array_equal(g, w)
    # a resetting read hands the same entries out once
    assert_entry_equal(host.read_sparse(True)[-1],
                       nonzero_view(hist, lanes, stalls))
    for entry in host.read_sparse().values():
        assert len(entry[0]) == 0
        assert_entry_equal(entry, EMPTY)
    for arrays in host.read_with_stalls().values():
        assert not any(a.any() for a in arrays)


def test_host_read_sparse_emits_bucket_of_masked_off_samples():
    """A bucket hit only by exec_mask == 0 samples has a zero lane sum; it
    is still emitted (the count decides)."""
    layout = BucketLayout(bucket_shift=6)
    layout.add(pid=1, code_object_id=7, load_size=64 * 8)
    host = HostAccumulator(layout)
    samples = np.zeros(3, dtype=ev.PC_SAMPLE_DTYPE)
    samples["code_object_id"] = 7
    samples["code_object_offset"] = [64 * 5, 64 * 5 + 8, 64 * 2]
    samples["exec_mask"] = [0, 0, 0xFF]
    host.accumulate(1, samples, gpu=3)
    buckets, hist, lanes, stalls = host.read_sparse()[3]
    np.testing.assert_array_equal(buckets, [2, 5])
    np.testing.assert_array_equal(hist, [1, 2])
    np.testing.assert_array_equal(lanes, [8, 0])
    assert not stalls.any() and stalls.shape == (2, N_COLS)


# -- device accumulator over a numpy stand-in -------------------------------


class FakeBucketizer:
    """numpy DeviceBucketizer: one pid's LOCAL bucket space, the native
    class's methods and dtypes."""

    instances = 0

    def __init__(self, device, slot_ids, slot_offsets, bucket_shift):
        FakeBucketizer.instances += 1
        self.slot_ids = np.asarray(slot_ids, dtype=np.uint64)
        self.offsets = np.asarray(slot_offsets, dtype=np.uint32)
        self.shift = bucket_shift
        total = int(self.offsets[-1])
        self.hist = np.zeros(total, dtype=np.uint32)
        self.lanes = np.zeros(total, dtype=np.uint64)
        self.stalls = None
        self.overflow = np.zeros(2, dtype=np.uint32)

    def _accumulate(self, co, off, exec_masks, flags):
        idx = np.minimum(np.searchsorted(self.slot_ids, co),
                         len(self.slot_ids) - 1)
        known = self.slot_ids[idx] == co
        self.overflow[0] += int((~known).sum())
        slot = idx[known]
        local = off[known] >> np.uint64(self.shift)
        size = (self.offsets[slot + 1] - self.offsets[slot]).astype(np.uint64)
        ok = local < size
        self.overflow[1] += int((~ok).sum())
        buckets = (self.offsets[slot[ok]].astype(np.int64) +
                   local[ok].astype(np.int64))
        np.add.at(self.hist, buckets, 1)
        masks = exec_masks[known][ok]
        pop = np.array([bin(int(m)).count("1") for m in masks],
                       dtype=np.uint64)
        np.add.at(self.lanes, buckets, pop)
        if flags is not None:
            if self.stalls is None:
                self.stalls = np.zeros((len(self.hist), N_COLS), np.uint32)
            cols = ev.stall_column(flags[known][ok])
            has = cols != ev.NO_STALL_COLUMN
            np.add.at(self.stalls, (buckets[has], cols[has]), 1)

    def accumulate(self, co, off, exec_masks):
        self._accumulate(co, off, exec_masks, None)

    def accumulate_flagged(self, co, off, exec_masks, flags):
        self._accumulate(co, off, exec_masks, flags)

    def reset(self):
        self.hist[:] = 0
        self.lanes[:] = 0
        self.overflow[:] = 0
        if self.stalls is not None:
            self.stalls[:] = 0

    def read(self, also_reset=True):
        out = (self.hist.copy(), self.lanes.copy(), self.overflow.copy())
        if also_reset:
            self.reset()
        return out

    def read_stalls(self, also_reset=True):
        stalls = (np.zeros((len(self.hist), N_COLS), np.uint32)
                  if self.stalls is None else self.stalls.copy())
        return self.read(also_reset) + (stalls,)

    def read_sparse(self, also_reset=True):
        nz = np.flatnonzero(self.hist)
        stalls = (np.zeros((len(nz), N_COLS), np.uint32)
                  if self.stalls is None else self.stalls[nz])
        out = (nz.astype(np.uint32), self.hist[nz], self.lanes[nz], stalls,
               self.overflow.copy())
        if also_reset:
            self.hist[nz] = 0
            self.lanes[nz] = 0
            self.overflow[:] = 0
            if self.stalls is not None:
                self.stalls[nz] = 0
        return out


class FakeNative:
    DeviceBucketizer = FakeBucketizer

    @staticmethod
    def hip_device_count():
        return 1

    @staticmethod
    def split_pc_samples(samples):
        flags = np.ascontiguousarray(samples["flags"])
        return (np.ascontiguousarray(samples["code_object_id"]),
                np.ascontiguousarray(samples["code_object_offset"]),
                np.ascontiguousarray(samples["exec_mask"]), flags,
                int(np.bitwise_or.reduce(flags)) if len(flags) else 0)


@pytest.fixture
def fake_native(monkeypatch):
    import parca_agent_amd.native as native_mod

    monkeypatch.setattr(native_mod, "gpu", lambda: FakeNative)
    monkeypatch.setattr(FakeBucketizer, "instances", 0)
    return FakeNative


PID_A, PID_B = 10, 20
SIZES_A = {1: 64 * 400, 2: 64 * 300}
SIZES_B = {1: 64 * 200, 2: 64 * 150}
GROWN_A = dict(SIZES_A)
GROWN_A[3] = 64 * 50                # buckets 1050..1099, added mid-way


def run_rebuild_scenario(dev_factory):
    """Two pids whose code objects interleave in the layout, two gpus,
    flagged and unflagged batches, a host -> device hand-over written into
    the pending arrays, and a code object added between batches. Returns
    (host accumulator, device accumulator) fed the same samples."""
    layout = BucketLayout(bucket_shift=6)
    for co in (1, 2):  # A1 B1 A2 B2: each pid's slots are not contiguous
        layout.add(pid=PID_A, code_object_id=co, load_size=SIZES_A[co])
        layout.add(pid=PID_B, code_object_id=co, load_size=SIZES_B[co])
    host = HostAccumulator(layout)
    dev = dev_factory(layout)

    def both(pid, gpu, batch):
        host.accumulate(pid, batch, gpu=gpu)
        dev.accumulate(pid, batch, gpu=gpu)

    def stream(sizes, n, seed, flagged=True):
        batch = make_stream(sizes, n, seed)
        if not flagged:
            batch["flags"] = 0
        return batch

    both(PID_A, 0, stream(GROWN_A, 3001, 31))   # code object 3 unknown yet
    both(PID_B, 0, stream(SIZES_B, 1002, 32, flagged=False))
    both(PID_A, 1, stream(GROWN_A, 2003, 33))
    both(PID_B, 1, stream(SIZES_B, 1500, 34))
    # The service's hand-over: what a host accumulator gathered before the
    # device one existed goes into the dense pending arrays.
    early = HostAccumulator(layout)
    handed = stream(SIZES_B, 700, 35)
    early.accumulate(PID_B, handed, gpu=1)
    host.accumulate(PID_B, handed, gpu=1)
    for g, (h, l, st) in early.read_with_stalls(True).items():
        pending = dev._pending_arrays(g)
        pending[0][: len(h)] += h
        pending[1][: len(l)] += l
        dev._pending_stall_array(g)[: len(st)] += st
    dev.unknown_code_object += early.unknown_code_object
    dev.out_of_range += early.out_of_range

    layout.add(pid=PID_A, code_object_id=3, load_size=GROWN_A[3])
    dev.layout_changed()
    both(PID_A, 0, stream(GROWN_A, 2500, 36))
    both(PID_B, 0, stream(SIZES_B, 900, 37))
    both(PID_A, 1, stream(GROWN_A, 1100, 38, flagged=False))
    return host, dev


def test_device_accumulator_sparse_folding(fake_native):
    host, dev = run_rebuild_scenario(DeviceAccumulator)
    assert FakeBucketizer.instances == 7  # 4 keys, 3 of them rebuilt
    # the carry-over of the rebuild is sparse, not folded into dense arrays
    assert dev._sparse and 0 not in dev._pending

    want = host.read_sparse()
    got = dev.read_sparse()
    assert sorted(want) == [0, 1]
    assert_sparse_equal(got, want)
    assert dev.unknown_code_object == host.unknown_code_object > 0
    assert dev.out_of_range == host.out_of_range > 0
    for gpu in (0, 1):
        buckets, _, _, stalls = got[gpu]
        assert 0 < stalls.any(axis=1).sum() < len(buckets) < 1100
        assert buckets[-1] >= 1050  # the code object added mid-way
    # drained, and the dense hand-over arrays are gone with it
    assert not dev._pending and not dev._pending_stalls and not dev._sparse
    for entry in dev.read_sparse().values():
        assert_entry_equal(entry, EMPTY)


def test_sparse_carry_over_reaches_dense_read(fake_native):
    host, dev = run_rebuild_scenario(DeviceAccumulator)
    want = host.read_with_stalls()
    got = dev.read_with_stalls()
    assert sorted(got) == sorted(want) == [0, 1]
    for gpu in want:
        for g, w in zip(got[gpu], want[gpu]):
            assert g.dtype == np.uint64 and g.shape == w.shape
            np.testing.assert_array_equal(g, w)
    assert dev.unknown_code_object == host.unknown_code_object
    assert dev.out_of_range == host.out_of_range
    assert not dev._sparse

    # ... and the plain dense read, which drops the stall counts
    host, dev = run_rebuild_scenario(DeviceAccumulator)
    want = host.read()
    got = dev.read()
    for gpu in want:
        np.testing.assert_array_equal(got[gpu][0], want[gpu][0])
        np.testing.assert_array_equal(got[gpu][1], want[gpu][1])
    for arrays in dev.read_with_stalls().values():
        assert not any(a.any() for a in arrays)


def test_steady_state_read_sparse_allocates_no_dense_array(fake_native):
    total = 1 << 20
    layout = BucketLayout(bucket_shift=6)
    layout.add(pid=1, code_object_id=1, load_size=64 * total)
    dev = DeviceAccumulator(layout)
    rng = np.random.default_rng(8)
    samples = np.zeros(400, dtype=ev.PC_SAMPLE_DTYPE)
    samples["code_object_id"] = 1
    touched = rng.choice(total, size=100, replace=False)
    samples["code_object_offset"] = np.repeat(touched, 4) * 64
    samples["exec_mask"] = 0xFFFF
    samples["flags"] = ev.pack_pc_flags(1, 1, 0, 0, 3)

    dev.accumulate(1, samples, gpu=0)
    warm = dev.read_sparse()
    assert len(warm[0][0]) == 100
    dev.accumulate(1, samples, gpu=0)
    tracemalloc.start()
    try:
        got = dev.read_sparse()
        _, peak = tracemalloc.get_traced_memory()
    finally:
        tracemalloc.stop()
    print(f"tracemalloc peak across read_sparse: {peak} B "
          f"(one dense uint64 array: {total * 8} B)")
    # Below one dense uint64 array over the bucket space: a condition on
    # shapes, not a timing.
    assert peak < total * 8
    assert_sparse_equal(got, warm)
    np.testing.assert_array_equal(got[0][0], np.sort(touched))
    assert (got[0][1] == 4).all() and (got[0][3][:, 3] == 4).all()


# -- service ---------------------------------------------------------------


class DenseOnly:
    """An accumulator as it was before the sparse read existed."""

    def __init__(self, inner):
        self._inner = inner

    def accumulate(self, *args, **kwargs):
        return self._inner.accumulate(*args, **kwargs)

    def read(self, also_reset=True):
        return self._inner.read(also_reset)

    def read_with_stalls(self, also_reset=True):
        return self._inner.read_with_stalls(also_reset)


class RecordingReporter:
    def __init__(self):
        self.events = []

    def set_gpu_config(self, *args):
        pass

    def report_trace_event(self, trace, meta):
        self.events.append((trace.frames, trace.custom_labels, meta.pid,
                            meta.origin, meta.value, meta.gpu_id))


def _service_events(tmp_path, code_object, dense, stall_reasons):
    from parca_agent_amd.native import gpu as native_gpu

    g = native_gpu()
    shm = tmp_path / f"shm_{int(dense)}_{int(stall_reasons)}"
    shm.mkdir()
    rep = RecordingReporter()
    svc = GPUProfilerService(rep, shm_dir=str(shm),
                             use_device_bucketize=False, bucket_shift=0,
                             stall_reasons=stall_reasons)
    pid = os.getpid()
    prod = g.TestRingProducer(
        os.path.join(str(shm), f"parca_gpu_{pid}.ring"), 1 << 20)
    size = os.path.getsize(code_object)
    with ELFFile.open(code_object) as elf:
        syms = {s.name: s.value for s in elf.symbols()
                if s.name in ("my_gemm_kernel", "my_softmax_kernel")}
    load_base = 0x7F00_0000_0000
    prod.write(g.EV_CODE_OBJECT_LOAD, ev.encode_code_object_load(
        ev.CodeObjectLoad(
            code_object_id=1, load_base=load_base, load_size=size,
            load_delta=load_base, memory_base=0, memory_size=0,
            storage_type=1,
            uri=f"file://{code_object}#offset=0&size={size}")))
    # A second code object the registry cannot open: the no-info branch.
    prod.write(g.EV_CODE_OBJECT_LOAD, ev.encode_code_object_load(
        ev.CodeObjectLoad(
            code_object_id=2, load_base=0, load_size=256, load_delta=0,
            memory_base=0, memory_size=0, storage_type=1,
            uri="file:///nonexistent/code-object#offset=0&size=256")))
    waitcnt = ev.pack_pc_flags(1, 1, 0, 4, 3)
    issued = ev.pack_pc_flags(1, 1, 1, 1, 0)
    gemm, softmax = syms["my_gemm_kernel"], syms["my_softmax_kernel"]
    rows = {
        0: [(1, gemm, waitcnt, 0xFFFF), (1, gemm, waitcnt, 0xFF),
            (1, gemm, issued, 0xF), (1, gemm, 0, 0xF),
            (1, gemm + 1, 0, 0x3), (1, gemm + 1, 0, 0x1),  # all-zero row
            (1, softmax, issued, 0),                       # zero lane sum
            (2, 17, waitcnt, 0xFFFFFFFF), (2, 200, 0, 0x1)],
        5: [(1, softmax + 2, waitcnt, 0xF0), (1, gemm, issued, 0xFFFF),
            (1, gemm, issued, 0xFFFF), (2, 17, 0, 0x7)],
    }
    for gpu, entries in rows.items():
        samples = np.zeros(len(entries), dtype=ev.PC_SAMPLE_DTYPE)
        for i, (co, off, flags, mask) in enumerate(entries):
            samples[i]["code_object_id"] = co
            samples[i]["code_object_offset"] = off
            samples[i]["flags"] = flags
            samples[i]["exec_mask"] = mask
        prod.write(g.EV_PC_SAMPLE_BATCH,
                   ev.encode_pc_sample_batch(gpu, samples))
    svc.drain_once()
    assert isinstance(svc.accumulator, HostAccumulator)
    sparse_reads = []
    if dense:
        svc.accumulator = DenseOnly(svc.accumulator)
        assert not hasattr(svc.accumulator, "read_sparse")
    else:
        real = svc.accumulator.read_sparse

        def spy(also_reset=True):
            sparse_reads.append(also_reset)
            return real(also_reset)

        svc.accumulator.read_sparse = spy
    svc.flush_pc()
    assert sparse_reads == ([] if dense else [True])
    assert svc.metrics.pc_buckets_reported == len(rep.events)
    return rep.events


@pytest.mark.parametrize("stall_reasons", [True, False])
def test_service_flush_same_events_sparse_and_dense(
        tmp_path, fake_code_object, stall_reasons):  # noqa: F811
    sparse = _service_events(tmp_path, fake_code_object, False,
                             stall_reasons)
    dense = _service_events(tmp_path, fake_code_object, True, stall_reasons)
    assert sparse == dense
    assert {e[5] for e in sparse} == {0, 5}
    assert sum(e[4] for e in sparse) == 13
    labels = [dict(e[1]) for e in sparse]
    if stall_reasons:
        assert len(sparse) == 10
        assert {l.get("stall_reason") for l in labels} == \
            {None, "waitcnt", "issued"}
    else:
        assert len(sparse) == 8  # one per touched (gpu, bucket)
        assert not any("stall_reason" in l for l in labels)
    # the bucket hit only with exec_mask == 0 carries no lane label
    assert sum("avg_active_lanes" not in l for l in labels) == 1
