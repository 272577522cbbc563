// CDNA4 (gfx950) sparse readback of the PC-sample histograms.
//
// The bucketize kernel (bucketize.hip) keeps three dense per-bucket arrays
// on the device: u32 counts, u64 active-lane sums and a 16 x u32 stall row,
// 76 B per bucket. A report interval touches a tiny fraction of them, but
// a dense read moves all 76 B of every bucket to the host. This kernel
// compacts the touched buckets into (bucket, count, lanes, stall row)
// entries on the device, so the host copies and walks O(touched buckets).
//
// Design for MI355X:
//  - The emit predicate is the count alone: the bucketize kernels add a
//    lane sum or a stall cell only together with a count >= 1 for the same
//    bucket, so count == 0 implies the rest of the bucket is zero. The
//    lane sum cannot be the predicate (it is 0 for exec_mask == 0).
//  - Same grid shape as the bucketize launch: 256-thread workgroups
//    (4 waves of 64), each lane takes 4 consecutive counts with ONE
//    global_load_dwordx4, grid capped at 2048 workgroups with a
//    grid-stride loop (Guideline 11): one sweep covers 2048 x 256 x 4 =
//    2 097 152 buckets, the largest layout (4 Mi) takes two. The
//    total_buckets % 4 tail is read scalar by workgroup 0.
//  - Output reservation, once per workgroup per grid-stride step: a lane
//    has 0..4 hits; four __ballot + popcount give its exclusive prefix
//    inside the wave and the wave's total, the 4 wave totals cross through
//    LDS, and ONE lane issues ONE device-scope atomicAdd(out_n, hits of the
//    workgroup) (Guideline 12). A workgroup-step without a hit issues no
//    atomic and skips the second barrier. Inside a reservation entries are
//    in ascending bucket order; between reservations the order is whatever
//    the atomics gave (the host sorts the k entries).
//  - An entry whose output index is >= capacity is neither written nor
//    cleared; out_n still counts it, so the caller can tell.
//  - Clearing (args.clear): the lane that read a bucket stores zero over
//    its count (one dwordx4 store for the lane's 4 counts), its lane sum
//    and its stall row. All other buckets are zero already, so the dense
//    arrays are all zero afterwards without a memset over 76 B x buckets.
//
// Bytes moved:
//    per bucket scanned   4 B read (the count); the 8 B lane sum and the
//                         64 B stall row of an untouched bucket are never
//                         read — 72 of its 76 B stay where they are.
//    per hit              8 B lane sum + 64 B stall row read (4 x dwordx4),
//                         4 + 4 + 8 + 64 = 80 B entry written; with clear,
//                         16 + 8 + 64 B of zero stores on top.
//  At the largest layout (4 Mi buckets, 1 % touched) that is 16 MiB of
//  counts plus ~6 MiB for the 42 K hits, against 304 MiB dense.
//
// LDS: 2 x 4 wave totals (double-buffered on the step parity, so the
// no-hit path needs one barrier only) + the reservation base = 36 B.
// No dynamic LDS; occupancy is bounded by registers alone.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gpu/bucketize.h"
#include "gpu/compact.h"

namespace parca_gpu {

namespace {

constexpr int kCompactThreads = 256;
constexpr int kCompactWaves = kCompactThreads / 64;
constexpr uint32_t kPerStep = kCompactThreads * 4;  // buckets per wg-step
constexpr uint32_t kMaxBlocks = 2048;

static_assert(kStallColumns == 16, "a stall row is 4 x dwordx4");

// Copy (or zero-fill) one entry's payload behind its bucket and count.
__device__ inline void emit_entry(const CompactArgs& a, uint32_t bucket,
                                  uint32_t count, uint32_t idx) {
  a.out_bucket[idx] = bucket;
  a.out_count[idx] = count;
  a.out_lanes[idx] = a.lane_histogram[bucket];
  if (a.clear) a.lane_histogram[bucket] = 0;
  if (a.out_stall != nullptr) {
    uint4* dst = reinterpret_cast<uint4*>(
        a.out_stall + static_cast<size_t>(idx) * kStallColumns);
    const uint4 zero = make_uint4(0, 0, 0, 0);
    if (a.stall_histogram != nullptr) {
      uint4* src = reinterpret_cast<uint4*>(
          a.stall_histogram + static_cast<size_t>(bucket) * kStallColumns);
      uint4 r0 = src[0], r1 = src[1], r2 = src[2], r3 = src[3];
      dst[0] = r0;
      dst[1] = r1;
      dst[2] = r2;
      dst[3] = r3;
      if (a.clear) {
        src[0] = zero;
        src[1] = zero;
        src[2] = zero;
        src[3] = zero;
      }
    } else {
      dst[0] = zero;
      dst[1] = zero;
      dst[2] = zero;
      dst[3] = zero;
    }
  }
}

// Workgroup-wide reservation for one step. `c` are this lane's 4 counts
// (zero where it has no bucket). Returns the output index of the lane's
// first hit; its further hits follow consecutively. Every thread of the
// workgroup must call this the same number of times (barriers inside).
// `any` is set when the workgroup has at least one hit.
__device__ inline uint32_t reserve(const CompactArgs& a, const uint32_t c[4],
                                   uint32_t step, uint32_t (*s_wave)[4],
                                   uint32_t* s_base, bool* any) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t lane_off = 0, wave_total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint64_t m = __ballot(c[k] != 0);
    lane_off += static_cast<uint32_t>(__popcll(m & below));
    wave_total += static_cast<uint32_t>(__popcll(m));
  }
  uint32_t* totals = s_wave[step & 1u];
  if (lane == 0) totals[wave] = wave_total;
  __syncthreads();
  uint32_t wg_total = 0, wave_off = 0;
#pragma unroll
  for (uint32_t w = 0; w < kCompactWaves; ++w) {
    uint32_t t = totals[w];
    wg_total += t;
    if (w < wave) wave_off += t;
  }
  *any = wg_total != 0;
  if (wg_total == 0) return 0;  // uniform: every thread read the same LDS
  if (threadIdx.x == 0) *s_base = atomicAdd(a.out_n, wg_total);
  __syncthreads();
  return *s_base + wave_off + lane_off;
}

__global__ __launch_bounds__(kCompactThreads) void compact_touched(
    CompactArgs a) {
  __shared__ uint32_t s_wave[2][4];
  __shared__ uint32_t s_base;

  const uint32_t n4 = a.total_buckets & ~3u;
  uint32_t step = 0;
  // The loop bound is the workgroup's first bucket, so all 256 threads run
  // the same number of steps and meet at the barriers in reserve().
  // 64-bit induction: wg_first + stride may pass 2^32 on its last step.
  for (uint64_t wg_first = static_cast<uint64_t>(blockIdx.x) * kPerStep;
       wg_first < n4;
       wg_first += static_cast<uint64_t>(gridDim.x) * kPerStep, ++step) {
    const uint64_t i = wg_first + threadIdx.x * 4;  // multiple of 4
    uint32_t c[4] = {0, 0, 0, 0};
    if (i < n4) {  // then i + 3 < n4 as well
      uint4 v = *reinterpret_cast<const uint4*>(a.histogram + i);
      c[0] = v.x;
      c[1] = v.y;
      c[2] = v.z;
      c[3] = v.w;
    }
    bool any;
    uint32_t idx = reserve(a, c, step, s_wave, &s_base, &any);
    if (!any) continue;
    bool cleared = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (c[k] == 0) continue;
      if (idx < a.capacity) {
        emit_entry(a, static_cast<uint32_t>(i) + k, c[k], idx);
        if (a.clear) {
          c[k] = 0;
          cleared = true;
        }
      }
      ++idx;
    }
    // Counts left over capacity keep their value in the vector store.
    if (cleared)
      *reinterpret_cast<uint4*>(a.histogram + i) =
          make_uint4(c[0], c[1], c[2], c[3]);
  }

  if (blockIdx.x == 0 && n4 != a.total_buckets) {
    const uint32_t b = n4 + threadIdx.x;
    uint32_t c[4] = {0, 0, 0, 0};
    if (b < a.total_buckets) c[0] = a.histogram[b];
    bool any;
    uint32_t idx = reserve(a, c, step, s_wave, &s_base, &any);
    if (any && c[0] != 0 && idx < a.capacity) {
      emit_entry(a, b, c[0], idx);
      if (a.clear) a.histogram[b] = 0;
    }
  }
}

}  // namespace

void launch_compact(const CompactArgs& args, hipStream_t stream) {
  (void)hipMemsetAsync(args.out_n, 0, sizeof(uint32_t), stream);
  if (args.total_buckets == 0) return;
  uint32_t blocks = (args.total_buckets + kPerStep - 1) / kPerStep;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;  // grid-stride the rest (G11)
  hipLaunchKernelGGL(compact_touched, dim3(blocks), dim3(kCompactThreads), 0,
                     stream, args);
}

}  // namespace parca_gpu
