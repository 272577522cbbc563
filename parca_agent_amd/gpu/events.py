"""GPU ring event decoding: Python mirrors of csrc/rocprof/ring.h layouts.

The u32 event-type discriminator dispatch mirrors the reference's
parcagpu reader (reference: parcagpu/parcagpu.go:149-213). Layouts are
verified against the C++ sizeof()s in tests/test_gpu_ring.py.
"""

from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Tuple

import numpy as np

EV_KERNEL_DISPATCH = 1
EV_CODE_OBJECT_LOAD = 2
EV_CODE_OBJECT_UNLOAD = 3
EV_KERNEL_SYMBOL = 4
EV_PC_SAMPLE_BATCH = 5
EV_GPU_CONFIG = 6
EV_ERROR = 7
EV_LAUNCH_STACK = 8

KERNEL_DISPATCH_FMT = struct.Struct("<6Q2I3I3I2I")
CODE_OBJECT_LOAD_FMT = struct.Struct("<QQQqQQII")
CODE_OBJECT_UNLOAD_FMT = struct.Struct("<Q")
KERNEL_SYMBOL_FMT = struct.Struct("<QQQII")
PC_SAMPLE_BATCH_HEADER_FMT = struct.Struct("<II")
GPU_CONFIG_FMT = struct.Struct("<4IQd")
ERROR_FMT = struct.Struct("<II")
LAUNCH_STACK_FMT = struct.Struct("<QQII")

# numpy dtype of one PCSample (ring.h PCSample, 64 bytes).
PC_SAMPLE_DTYPE = np.dtype([
    ("code_object_id", "<u8"),
    ("code_object_offset", "<u8"),
    ("timestamp", "<u8"),
    ("exec_mask", "<u8"),
    ("dispatch_id", "<u8"),
    ("correlation_id", "<u8"),
    ("hw_id", "<u8"),
    ("wave_in_group", "<u4"),
    ("flags", "<u4"),
])


# -- PCSample.flags (ring.h kPcFlag*, pack_pc_flags) -----------------------
#
#   bit 0       stochastic record
#   bit 1       issue info valid (every stochastic record, no host-trap one)
#   bit 2       wave_issued
#   bits 8-12   inst_type (raw)
#   bits 16-19  snapshot.reason_not_issued (raw)

PC_FLAG_STOCHASTIC = 1 << 0
PC_FLAG_ISSUE_VALID = 1 << 1
PC_FLAG_WAVE_ISSUED = 1 << 2
PC_FLAG_INST_TYPE_SHIFT = 8
PC_FLAG_INST_TYPE_MASK = 0x1F
PC_FLAG_REASON_SHIFT = 16
PC_FLAG_REASON_MASK = 0xF

# Stall-reason histogram columns: 0..9 are the SDK's reason_not_issued
# enum, 10..13 are never produced, 14 collects raw reasons the enum does
# not define, 15 is "the wave issued an instruction".
N_STALL_COLUMNS = 16
STALL_COLUMN_UNKNOWN = 14
STALL_COLUMN_ISSUED = 15
NO_STALL_COLUMN = -1  # stall_column() of a sample without issue info
STALL_COLUMN_NAMES = (
    "none",
    "no_instruction_available",
    "alu_dependency",
    "waitcnt",
    "internal_instruction",
    "barrier_wait",
    "arbiter_not_win",
    "arbiter_win_ex_stall",
    "other_wait",
    "sleep_wait",
    "reserved_10",
    "reserved_11",
    "reserved_12",
    "reserved_13",
    "unknown",
    "issued",
)


def pack_pc_flags(stochastic, valid, issued, inst_type: int,
                  reason: int) -> int:
    """Python mirror of ring.h pack_pc_flags (pinned to it in
    tests/test_pc_stall_reasons.py)."""
    return ((PC_FLAG_STOCHASTIC if stochastic else 0)
            | (PC_FLAG_ISSUE_VALID if valid else 0)
            | (PC_FLAG_WAVE_ISSUED if issued else 0)
            | ((int(inst_type) & PC_FLAG_INST_TYPE_MASK)
               << PC_FLAG_INST_TYPE_SHIFT)
            | ((int(reason) & PC_FLAG_REASON_MASK) << PC_FLAG_REASON_SHIFT))


def stall_column(flags):
    """Stall column of each flags word (vectorised; a scalar gives a
    0-d array): NO_STALL_COLUMN where bit 1 is clear, STALL_COLUMN_ISSUED
    where bit 2 is set, else the raw reason, with reasons above 9 folded
    into STALL_COLUMN_UNKNOWN."""
    f = np.asarray(flags).astype(np.int64)
    reason = (f >> PC_FLAG_REASON_SHIFT) & PC_FLAG_REASON_MASK
    col = np.where(reason <= 9, reason, STALL_COLUMN_UNKNOWN)
    col = np.where(f & PC_FLAG_WAVE_ISSUED, STALL_COLUMN_ISSUED, col)
    return np.where(f & PC_FLAG_ISSUE_VALID, col, NO_STALL_COLUMN)


@dataclass
class KernelDispatch:
    correlation_id: int
    dispatch_id: int
    kernel_id: int
    start_ns: int
    end_ns: int
    tid: int
    gpu_index: int
    pid: int
    grid: Tuple[int, int, int]
    workgroup: Tuple[int, int, int]
    private_segment_size: int
    group_segment_size: int

    @property
    def duration_ns(self) -> int:
        return max(self.end_ns - self.start_ns, 0)


@dataclass
class CodeObjectLoad:
    code_object_id: int
    load_base: int
    load_size: int
    load_delta: int
    memory_base: int
    memory_size: int
    storage_type: int
    uri: str


@dataclass
class KernelSymbol:
    kernel_id: int
    code_object_id: int
    kernel_object: int
    name: str


@dataclass
class GpuConfig:
    gpu_index: int
    method: int
    unit: int
    interval: int
    ns_per_sample: float


@dataclass
class LaunchStack:
    correlation_id: int
    tid: int
    pid: int
    ips: Tuple[int, ...]


@dataclass
class RingError:
    code: int
    message: str


def decode_kernel_dispatch(payload: bytes) -> KernelDispatch:
    v = KERNEL_DISPATCH_FMT.unpack_from(payload)
    return KernelDispatch(
        correlation_id=v[0], dispatch_id=v[1], kernel_id=v[2],
        start_ns=v[3], end_ns=v[4], tid=v[5], gpu_index=v[6], pid=v[7],
        grid=(v[8], v[9], v[10]), workgroup=(v[11], v[12], v[13]),
        private_segment_size=v[14], group_segment_size=v[15])


def decode_code_object_load(payload: bytes) -> CodeObjectLoad:
    v = CODE_OBJECT_LOAD_FMT.unpack_from(payload)
    uri_len = v[7]
    base = CODE_OBJECT_LOAD_FMT.size
    uri = payload[base : base + uri_len].decode("utf-8", "replace")
    return CodeObjectLoad(
        code_object_id=v[0], load_base=v[1], load_size=v[2], load_delta=v[3],
        memory_base=v[4], memory_size=v[5], storage_type=v[6], uri=uri)


def decode_code_object_unload(payload: bytes) -> int:
    return CODE_OBJECT_UNLOAD_FMT.unpack_from(payload)[0]


def decode_kernel_symbol(payload: bytes) -> KernelSymbol:
    v = KERNEL_SYMBOL_FMT.unpack_from(payload)
    base = KERNEL_SYMBOL_FMT.size
    name = payload[base : base + v[3]].decode("utf-8", "replace")
    return KernelSymbol(kernel_id=v[0], code_object_id=v[1],
                        kernel_object=v[2], name=name)


def decode_pc_sample_batch(payload: bytes) -> Tuple[int, np.ndarray]:
    """Returns (gpu_index, structured array of PC samples) — zero-copy."""
    gpu_index, count = PC_SAMPLE_BATCH_HEADER_FMT.unpack_from(payload)
    base = PC_SAMPLE_BATCH_HEADER_FMT.size
    arr = np.frombuffer(payload, dtype=PC_SAMPLE_DTYPE, count=count,
                        offset=base)
    return gpu_index, arr


def decode_gpu_config(payload: bytes) -> GpuConfig:
    v = GPU_CONFIG_FMT.unpack_from(payload)
    return GpuConfig(gpu_index=v[0], method=v[1], unit=v[2], interval=v[4],
                     ns_per_sample=v[5])


def decode_error(payload: bytes) -> RingError:
    code, msg_len = ERROR_FMT.unpack_from(payload)
    base = ERROR_FMT.size
    return RingError(code=code,
                     message=payload[base : base + msg_len].decode(
                         "utf-8", "replace"))


def decode_launch_stack(payload: bytes) -> LaunchStack:
    v = LAUNCH_STACK_FMT.unpack_from(payload)
    n = v[3]
    base = LAUNCH_STACK_FMT.size
    ips = struct.unpack_from(f"<{n}Q", payload, base) if n else ()
    return LaunchStack(correlation_id=v[0], tid=v[1], pid=v[2], ips=ips)


# -- encoding (test + synthetic-event support) ----------------------------


def encode_kernel_dispatch(ev: KernelDispatch) -> bytes:
    return KERNEL_DISPATCH_FMT.pack(
        ev.correlation_id, ev.dispatch_id, ev.kernel_id, ev.start_ns,
        ev.end_ns, ev.tid, ev.gpu_index, ev.pid, *ev.grid, *ev.workgroup,
        ev.private_segment_size, ev.group_segment_size)


def encode_code_object_load(ev: CodeObjectLoad) -> bytes:
    uri = ev.uri.encode()
    return CODE_OBJECT_LOAD_FMT.pack(
        ev.code_object_id, ev.load_base, ev.load_size, ev.load_delta,
        ev.memory_base, ev.memory_size, ev.storage_type, len(uri)) + uri


def encode_kernel_symbol(ev: KernelSymbol) -> bytes:
    name = ev.name.encode()
    return KERNEL_SYMBOL_FMT.pack(ev.kernel_id, ev.code_object_id,
                                  ev.kernel_object, len(name), 0) + name


def encode_pc_sample_batch(gpu_index: int, samples: np.ndarray) -> bytes:
    assert samples.dtype == PC_SAMPLE_DTYPE
    return PC_SAMPLE_BATCH_HEADER_FMT.pack(gpu_index, len(samples)) + \
        samples.tobytes()


def encode_gpu_config(ev: GpuConfig) -> bytes:
    return GPU_CONFIG_FMT.pack(ev.gpu_index, ev.method, ev.unit, 0,
                               ev.interval, ev.ns_per_sample)


def encode_launch_stack(ev: LaunchStack) -> bytes:
    return LAUNCH_STACK_FMT.pack(ev.correlation_id, ev.tid, ev.pid,
                                 len(ev.ips)) + \
        struct.pack(f"<{len(ev.ips)}Q", *ev.ips)


def encode_error(ev: RingError) -> bytes:
    msg = ev.message.encode()
    return ERROR_FMT.pack(ev.code, len(msg)) + msg
