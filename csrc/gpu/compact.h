// Launch interface of the CDNA4 sparse-readback kernel (compact.hip): the
// stream compaction that turns the dense per-bucket arrays the bucketize
// kernel fills into a list of the touched buckets. The one definition of
// CompactArgs: the kernel and the pybind module both include this header.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace parca_gpu {

struct CompactArgs {
  uint32_t* histogram;        // [total_buckets]   in/out
  uint64_t* lane_histogram;   // [total_buckets]   in/out
  uint32_t* stall_histogram;  // [total_buckets*16] in/out, nullable
  uint32_t total_buckets;
  uint32_t capacity;  // entries the out_* arrays hold
  uint32_t clear;     // nonzero: zero every emitted entry in place
  uint32_t* out_bucket;  // [capacity]
  uint32_t* out_count;   // [capacity]
  uint64_t* out_lanes;   // [capacity]
  uint32_t* out_stall;   // [capacity*16], nullable
  uint32_t* out_n;       // [1], zeroed by the launcher before the kernel
};

// Zeroes *out_n on `stream`, then launches the compaction behind it. After
// the kernel *out_n is the number of buckets with a non-zero count; only
// the first min(*out_n, capacity) entries of the out_* arrays are written.
void launch_compact(const CompactArgs& args, hipStream_t stream);

}  // namespace parca_gpu
