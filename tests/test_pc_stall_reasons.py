"""Stall-reason breakdown of PC samples, CPU side: the PCSample.flags wire
bits (Python mirror pinned to the C++ packing), the host accumulator's
stall matrix, the service's per-reason gpu_pcsample traces, and the
sampling-method export to the tool."""

import itertools
import os

import numpy as np
import pytest

from parca_agent_amd.elf import ELFFile
from parca_agent_amd.gpu import events as ev
from parca_agent_amd.gpu.pcbuckets import BucketLayout, HostAccumulator
from parca_agent_amd.gpu.service import GPUProfilerService
from parca_agent_amd.model import FrameType
from parca_agent_amd.reporter import Reporter

from tests.test_gpu_service import (  # noqa: F401  (fixture re-export)
    CollectingDestination,
    fake_code_object,
)


def _native():
    from parca_agent_amd.native import gpu

    return gpu()


# -- wire format -----------------------------------------------------------


def test_pack_pc_flags_matches_native_layout():
    g = _native()
    assert g.N_STALL_COLUMNS == ev.N_STALL_COLUMNS == 16
    for reason, issued, valid, stochastic, inst_type in itertools.product(
            range(16), (0, 1), (0, 1), (0, 1), (0, 1, 7, 16, 31)):
        py = ev.pack_pc_flags(stochastic, valid, issued, inst_type, reason)
        cc = g.pack_pc_flags(bool(stochastic), bool(valid), bool(issued),
                             inst_type, reason)
        assert py == cc, (reason, issued, valid, stochastic, inst_type)
        # the documented bit positions, spelled out
        assert py & 1 == stochastic
        assert (py >> 1) & 1 == valid
        assert (py >> 2) & 1 == issued
        assert (py >> 8) & 0x1F == inst_type
        assert (py >> 16) & 0xF == reason
        assert py >> 20 == 0 and (py >> 3) & 0x1F == 0 and (py >> 13) & 7 == 0
    # fields are truncated to their widths, identically on both sides
    assert ev.pack_pc_flags(1, 1, 0, 0x3F, 0x1F) == \
        g.pack_pc_flags(True, True, False, 0x3F, 0x1F) == \
        ev.pack_pc_flags(1, 1, 0, 0x1F, 0xF)


def test_stall_column_table():
    assert len(ev.STALL_COLUMN_NAMES) == ev.N_STALL_COLUMNS == 16
    assert ev.STALL_COLUMN_NAMES[:10] == (
        "none", "no_instruction_available", "alu_dependency", "waitcnt",
        "internal_instruction", "barrier_wait", "arbiter_not_win",
        "arbiter_win_ex_stall", "other_wait", "sleep_wait")
    assert ev.STALL_COLUMN_NAMES[10:14] == (
        "reserved_10", "reserved_11", "reserved_12", "reserved_13")
    assert ev.STALL_COLUMN_NAMES[14:] == ("unknown", "issued")

    for reason in range(16):
        for inst_type in (0, 16, 31):
            # no issue info: no column, whatever the other bits say
            for issued in (0, 1):
                f = ev.pack_pc_flags(1, 0, issued, inst_type, reason)
                assert int(ev.stall_column(f)) == ev.NO_STALL_COLUMN
            # issued overrides the reason
            f = ev.pack_pc_flags(1, 1, 1, inst_type, reason)
            assert int(ev.stall_column(f)) == 15
            f = ev.pack_pc_flags(1, 1, 0, inst_type, reason)
            assert int(ev.stall_column(f)) == (reason if reason <= 9 else 14)
    assert int(ev.stall_column(0)) == ev.NO_STALL_COLUMN  # host-trap
    assert int(ev.stall_column(1)) == ev.NO_STALL_COLUMN  # old stochastic

    # vectorised over the u32 field of a sample array
    flags = np.array([0, ev.pack_pc_flags(1, 1, 0, 3, 3),
                      ev.pack_pc_flags(1, 1, 1, 3, 3),
                      ev.pack_pc_flags(1, 1, 0, 0, 12),
                      ev.pack_pc_flags(1, 1, 0, 0, 0)], dtype=np.uint32)
    np.testing.assert_array_equal(ev.stall_column(flags),
                                  [ev.NO_STALL_COLUMN, 3, 15, 14, 0])


def test_split_pc_samples_matches_numpy_fields():
    """The native one-pass column split the device accumulator feeds the
    bucketizer from: equal to the numpy field gathers, on a decoded ring
    payload (records 8 bytes off alignment), a strided view and an empty
    batch; the OR of the flags decides the entry point."""
    g = _native()
    rng = np.random.default_rng(5)
    samples = np.zeros(1001, dtype=ev.PC_SAMPLE_DTYPE)
    for name in ("code_object_id", "code_object_offset", "exec_mask",
                 "timestamp", "hw_id"):
        samples[name] = rng.integers(0, 1 << 63, size=len(samples),
                                     dtype=np.uint64)
    samples["flags"] = rng.integers(0, 1 << 20, size=len(samples)) & ~2
    _, decoded = ev.decode_pc_sample_batch(
        ev.encode_pc_sample_batch(3, samples))
    assert not decoded.flags.writeable
    for arr in (samples, decoded, samples[::3], samples[:0]):
        co, off, ex, fl, flags_or = g.split_pc_samples(arr)
        np.testing.assert_array_equal(co, arr["code_object_id"])
        np.testing.assert_array_equal(off, arr["code_object_offset"])
        np.testing.assert_array_equal(ex, arr["exec_mask"])
        np.testing.assert_array_equal(fl, arr["flags"])
        assert (co.dtype, ex.dtype, fl.dtype) == (
            np.uint64, np.uint64, np.uint32)
        assert co.flags.c_contiguous and fl.flags.c_contiguous
        expect_or = int(np.bitwise_or.reduce(arr["flags"])) if len(arr) else 0
        assert flags_or == expect_or and not flags_or & 2
    samples["flags"][700] = ev.pack_pc_flags(1, 1, 0, 0, 3)
    assert g.split_pc_samples(samples)[4] & 2
    with pytest.raises(ValueError):
        g.split_pc_samples(np.zeros(4, dtype=np.uint64))


# -- host accumulator ------------------------------------------------------


def _sample(co, off, flags, mask=0xF):
    return (co, off, 0, mask, 0, 0, 0, 0, flags)


def test_host_accumulator_read_with_stalls():
    waitcnt = ev.pack_pc_flags(1, 1, 0, 2, 3)
    barrier = ev.pack_pc_flags(1, 1, 0, 2, 5)
    issued = ev.pack_pc_flags(1, 1, 1, 9, 3)
    weird = ev.pack_pc_flags(1, 1, 0, 0, 13)   # raw reason beyond the enum
    novalid = ev.pack_pc_flags(1, 0, 0, 0, 3)  # stochastic, no issue info

    layout = BucketLayout(bucket_shift=6)
    layout.add(pid=7, code_object_id=10, load_size=256)  # buckets 0..3
    layout.add(pid=7, code_object_id=20, load_size=128)  # buckets 4..5
    acc = HostAccumulator(layout)

    gpu0 = np.array([
        _sample(10, 0, 0),            # host-trap, bucket 0
        _sample(10, 8, waitcnt),      # bucket 0
        _sample(10, 63, waitcnt),     # bucket 0
        _sample(10, 64, issued),      # bucket 1
        _sample(10, 200, weird),      # bucket 3
        _sample(10, 192, novalid),    # bucket 3, total only
        _sample(20, 64, barrier),     # bucket 5
        _sample(20, 70, issued),      # bucket 5
        _sample(99, 0, waitcnt),      # unknown code object
        _sample(10, 256, waitcnt),    # out of range
        _sample(20, 1 << 40, issued),  # out of range
    ], dtype=ev.PC_SAMPLE_DTYPE)
    gpu1 = np.array([
        _sample(20, 0, barrier),      # bucket 4
        _sample(20, 1, 0),            # bucket 4, host-trap
        _sample(10, 130, waitcnt),    # bucket 2
    ], dtype=ev.PC_SAMPLE_DTYPE)
    acc.accumulate(7, gpu0, gpu=0)
    acc.accumulate(7, gpu1, gpu=1)

    exp_hist = {0: [3, 1, 0, 2, 0, 2], 1: [0, 0, 1, 0, 2, 0]}
    exp_stalls = {
        #        0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15
        0: [[0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1],
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0],
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]],
        1: [[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]],
    }

    out = acc.read_with_stalls(also_reset=False)
    assert sorted(out) == [0, 1]
    for gpu in (0, 1):
        hist, lanes, stalls = out[gpu]
        assert stalls.shape == (6, 16) and stalls.dtype == np.uint64
        np.testing.assert_array_equal(hist, exp_hist[gpu])
        np.testing.assert_array_equal(lanes, 4 * np.array(exp_hist[gpu]))
        np.testing.assert_array_equal(stalls, exp_stalls[gpu])
        assert (stalls.sum(axis=1) <= hist).all()
    assert acc.unknown_code_object == 1
    assert acc.out_of_range == 2

    # read() keeps its shape: pairs, same numbers
    pairs = acc.read(also_reset=False)
    for gpu in (0, 1):
        assert len(pairs[gpu]) == 2
        np.testing.assert_array_equal(pairs[gpu][0], exp_hist[gpu])

    # a resetting read hands the data out once, then everything is zero
    out = acc.read_with_stalls()
    np.testing.assert_array_equal(out[0][2], exp_stalls[0])
    for hist, lanes, stalls in acc.read_with_stalls().values():
        assert not hist.any() and not lanes.any() and not stalls.any()
        assert stalls.shape == (6, 16)

    # read() resets the stall matrix too
    acc.accumulate(7, gpu1, gpu=1)
    acc.read()
    for hist, lanes, stalls in acc.read_with_stalls().values():
        assert not hist.any() and not stalls.any()

    # the matrix grows with the layout and keeps its rows
    acc.accumulate(7, gpu1, gpu=1)
    layout.add(pid=7, code_object_id=30, load_size=64)  # bucket 6
    acc.accumulate(7, np.array([_sample(30, 0, issued)],
                               dtype=ev.PC_SAMPLE_DTYPE), gpu=1)
    hist, _, stalls = acc.read_with_stalls()[1]
    assert stalls.shape == (7, 16)
    np.testing.assert_array_equal(stalls[:6], exp_stalls[1])
    assert stalls[6, 15] == 1 and stalls[6].sum() == 1 and hist[6] == 1


# -- service end to end ----------------------------------------------------


def _run_service(tmp_path, code_object, stall_reasons):
    g = _native()
    dest = CollectingDestination()
    rep = Reporter([dest])
    kwargs = {} if stall_reasons is None else {"stall_reasons": stall_reasons}
    svc = GPUProfilerService(rep, shm_dir=str(tmp_path),
                             use_device_bucketize=False, bucket_shift=0,
                             **kwargs)
    pid = os.getpid()
    prod = g.TestRingProducer(
        os.path.join(str(tmp_path), f"parca_gpu_{pid}.ring"), 1 << 20)
    size = os.path.getsize(code_object)
    with ELFFile.open(code_object) as elf:
        sym = next(s for s in elf.symbols() if s.name == "my_gemm_kernel")
    load_base = 0x7F00_0000_0000
    prod.write(g.EV_CODE_OBJECT_LOAD, ev.encode_code_object_load(
        ev.CodeObjectLoad(
            code_object_id=1, load_base=load_base, load_size=size,
            load_delta=load_base, memory_base=0, memory_size=0,
            storage_type=1,
            uri=f"file://{code_object}#offset=0&size={size}")))
    prod.write(g.EV_GPU_CONFIG, ev.encode_gpu_config(
        ev.GpuConfig(gpu_index=0, method=2, unit=2, interval=1 << 20,
                     ns_per_sample=436907.0)))
    samples = np.zeros(7, dtype=ev.PC_SAMPLE_DTYPE)
    samples["code_object_id"] = 1
    samples["code_object_offset"] = sym.value
    samples["exec_mask"] = (1 << 64) - 1
    samples["flags"][0:3] = ev.pack_pc_flags(1, 1, 0, 4, 3)   # waitcnt
    samples["flags"][3:5] = ev.pack_pc_flags(1, 1, 1, 1, 0)   # issued
    prod.write(g.EV_PC_SAMPLE_BATCH, ev.encode_pc_sample_batch(0, samples))
    svc.drain_once()
    svc.flush_pc()
    rep.flush()
    pcs = [s for s in dest.samples
           if s.sample_type.sample_type == "gpu_pcsample"]
    return svc, pcs


def test_service_emits_one_trace_per_stall_reason(tmp_path, fake_code_object):
    svc, pcs = _run_service(tmp_path, fake_code_object, stall_reasons=None)
    assert len(pcs) == 3
    got = sorted((s.labels.get("stall_reason"), s.value) for s in pcs
                 if "stall_reason" in s.labels)
    assert got == [("issued", 2), ("waitcnt", 3)]
    [rest] = [s for s in pcs if "stall_reason" not in s.labels]
    assert rest.value == 2
    assert sum(s.value for s in pcs) == 7
    for s in pcs:
        assert s.trace.frames[0].kind == FrameType.GPU_PC
        assert s.trace.frames[0].function_name == "my_gemm_kernel"
        assert s.trace.frames == pcs[0].trace.frames
        assert s.period == 436907
        assert s.labels["avg_active_lanes"] == "64"
        assert s.labels["gpu"] == "0"
    assert svc.metrics.pc_samples == 7
    assert svc.metrics.pc_buckets_reported == 3


def test_service_stall_reasons_off_is_one_trace(tmp_path, fake_code_object):
    svc, pcs = _run_service(tmp_path, fake_code_object, stall_reasons=False)
    [pc] = pcs
    assert pc.value == 7
    assert "stall_reason" not in pc.labels
    assert pc.labels["avg_active_lanes"] == "64"
    assert pc.trace.frames[0].function_name == "my_gemm_kernel"
    assert svc.metrics.pc_buckets_reported == 1


# -- flags and tool environment -------------------------------------------


def test_tool_env_exports_pc_method():
    from parca_agent_amd.agent import tool_env

    assert tool_env(pc_method="stochastic")["PARCA_GPU_PC_METHOD"] == \
        "stochastic"
    assert "PARCA_GPU_PC_METHOD" not in tool_env()
    assert "PARCA_GPU_PC_METHOD" not in tool_env(pc_method="host_trap")


def test_stall_reasons_flag_and_agent_tool_env(tmp_path):
    from parca_agent_amd import flags as flags_mod
    from parca_agent_amd.agent import Agent

    assert flags_mod.Flags().rocm.pc_stall_reasons is True
    f = flags_mod.parse(["--rocm-pc-stall-reasons=false",
                         "--rocm-pc-sampling-method", "stochastic",
                         "--rocm-shm-dir", str(tmp_path)])
    assert f.rocm.pc_stall_reasons is False
    assert "rocm-pc-stall-reasons" in flags_mod._HELP

    agent = Agent(f, enable_cpu=False, enable_gpu=True)
    assert agent.gpu_service.stall_reasons is False
    env = agent.tool_env()
    assert env["PARCA_GPU_PC_METHOD"] == "stochastic"
    assert env["PARCA_GPU_SHM_DIR"] == str(tmp_path)
    assert "PARCA_GPU_PC_METHOD" not in Agent(
        flags_mod.Flags(), enable_cpu=False, enable_gpu=False).tool_env()
