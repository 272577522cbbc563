// Launch interface of the CDNA4 PC-sample bucketing kernel
// (bucketize.hip). The one definition of BucketizeArgs: the kernel and
// the pybind module both include this header, so the struct that is
// passed by value to the device cannot drift between them.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace parca_gpu {

// Width of one stall-histogram row: parca::kStallColumns in
// rocprof/ring.h (the column table lives there).
constexpr uint32_t kStallColumns = 16;

struct BucketizeArgs {
  const uint64_t* code_object_ids;  // [n]
  const uint64_t* offsets;          // [n]
  const uint64_t* exec_masks;       // [n] may be null
  uint32_t n;
  // sorted code-object id table and per-slot bucket layout
  const uint64_t* slot_ids;      // [n_slots] sorted
  const uint32_t* slot_offsets;  // [n_slots+1] prefix of bucket counts
  uint32_t n_slots;
  uint32_t bucket_shift;  // PC bytes per bucket = 1 << shift
  uint32_t total_buckets;
  uint32_t* histogram;       // [total_buckets] sample counts
  uint64_t* lane_histogram;  // [total_buckets] active-lane sums (nullable)
  uint32_t* overflow;        // [2]: unknown code-object, out-of-range bucket
  // Per-sample PCSample.flags and the per-(bucket, stall column) counts
  // they feed. Either one null: no stall accounting, and the launch is
  // the one a caller without these fields gets.
  const uint32_t* sample_flags;  // [n] (nullable)
  uint32_t* stall_histogram;     // [total_buckets * kStallColumns], row-major
                                 // by bucket (nullable)
};

void launch_bucketize(const BucketizeArgs& args, hipStream_t stream);

}  // namespace parca_gpu
