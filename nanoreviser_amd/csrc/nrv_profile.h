// Device-side per-read quality and base profile of a merged call: a Phred histogram and base counts of every revised read.
#pragma once
#include "nrv_merge.h"

namespace nrv {

// ---------------------------------------------------------------------------------------
// hoststage.read_profile is the DEFINITION; include/nanorev.h (nrv_revise_reads_raw_profile_begin) names the 48 columns:
//   0 .. 41  output characters of the read with clip(qual - 33, 0, 41) == k,
//   42 .. 46 output characters equal to 'A', 'C', 'G', 'T' and everything else,   47 reserved (0).
// The profile is that of the FASTQ form of the call whether a quality is written or not: a window's quality is computed HERE
// from p1 / p2 / a1 / a2 by the rule of merge_emit (merge_phred_steps on the thresholds of this call's own args), an edge event
// has Phred 2 ('#').  The quality byte merge_emit left in rec is not read - it is '#' in every FASTA call.
// One launch behind merge_scatter (profile_enqueue in nrv_api.hip), work distribution of report_kernel: one thread per event,
// workgroups of kMergeTile, the read found by merge_emit's binary search.  An event adds its count (0 / 1 / 2, from rec) to
// hist[q] and one to the base column of each character it emitted (first, and second for a count of 2).
// Every counter is an integer, so the bytes do not depend on the order in which tiles run:
//   * a tile inside ONE read adds into 48 LDS counters with LDS atomics and then issues at most 48 global atomicAdds on the
//     read's row, non-zero counters only.  Most characters of a real read share one or two Phred bins, so ahead of the LDS
//     atomic every wave sums the bin of its first emitting lane with two ballots (lanes of that bin with count 1, with count 2)
//     and that lane alone adds the sum; lanes of another bin add their own count.  Integer sums: exact;
//   * a tile that straddles a read boundary: each thread adds its own non-zero contributions to its read's row.
// The caller zeroes the block ahead of the launch.  A read without events has no thread and needs none.
// ---------------------------------------------------------------------------------------
constexpr int kProfileCols = 48;
constexpr int kPfBase = 42;              // 'A', 'C', 'G', 'T', other

struct ProfileArgs {
  const SegRead* reads;
  int n_reads, T;
  long long N;
  const signed char *a1, *a2;            // [N - T]
  const float *p1, *p2;                  // [N - T][6], [N - T][5]
  const unsigned* rec;                   // [N] merge_emit's records: count, first and second character
  unsigned long long* profile;           // [n_reads][kProfileCols], zeroed by the caller
  float thr[kPhredSteps];
};

__device__ __forceinline__ int profile_base_col(const unsigned c) {
  return kPfBase + (c == 'A' ? 0 : (c == 'C' ? 1 : (c == 'G' ? 2 : (c == 'T' ? 3 : 4))));
}

__global__ void __launch_bounds__(256) profile_kernel(const ProfileArgs a) {
  __shared__ unsigned cnt[kProfileCols];
  __shared__ int r_first, r_last;
  const long long E = (long long)blockIdx.x * kMergeTile + threadIdx.x;
  if (threadIdx.x < kProfileCols) cnt[threadIdx.x] = 0;
  int r = 0;
  unsigned count = 0, q = 2;
  int b1 = -1, b2 = -1;                                   // base columns of the first / second character emitted
  if (E < a.N) {
    int lo_r = 0, hi_r = a.n_reads - 1;                   // last read with ev_off <= E
    while (lo_r < hi_r) {
      const int mid = (lo_r + hi_r + 1) >> 1;
      if (a.reads[mid].ev_off <= E) lo_r = mid; else hi_r = mid - 1;
    }
    r = lo_r;
    const SegRead rd = a.reads[r];
    const long long j = E - rd.ev_off, o = (a.T - 1) / 2;
    const long long n_r = rd.ev_len - a.T > 0 ? rd.ev_len - a.T : 0;
    const unsigned rec = a.rec[E];
    count = rec & 3u;
    if (count >= 1) b1 = profile_base_col((rec >> 8) & 255u);
    if (count == 2) b2 = profile_base_col((rec >> 16) & 255u);
    if (j >= o && j < o + n_r) {
      const long long w = E - o;
      const int c1 = a.a1[w], c2 = a.a2[w];
      const int g1 = c1 < 0 ? 0 : (c1 > 5 ? 5 : c1), g2 = c2 < 0 ? 0 : (c2 > 4 ? 4 : c2);
      const float u = a.p1[w * 6 + g1], v = a.p2[w * 5 + g2];
      const float conf = v < u ? v : u;
      q = 1 + merge_phred_steps(a.thr, conf);             // 1 .. 40
    }
    if (threadIdx.x == 0) r_first = r;
    if (E == a.N - 1 || threadIdx.x == kMergeTile - 1) r_last = r;
  }
  __syncthreads();                                        // every workgroup has event blockIdx.x * kMergeTile < N: both are set
  const bool one_read = r_first == r_last;                // reads tile [0, N) in order: the same read at both ends = one read
  if (one_read) {
    // the bin of the wave's first emitting lane, summed over the wave: count is 0 for the lanes behind N
    const unsigned long long emit = __ballot(count != 0);
    if (emit) {
      const int lead = __ffsll((long long)emit) - 1;
      const unsigned q0 = (unsigned)__shfl((int)q, lead);
      const unsigned long long m1 = __ballot(count == 1 && q == q0), m2 = __ballot(count == 2 && q == q0);
      if ((int)(threadIdx.x & 63) == lead) atomicAdd(&cnt[q0], (unsigned)__popcll(m1) + 2u * (unsigned)__popcll(m2));
      else if (count && q != q0) atomicAdd(&cnt[q], count);
    }
    if (b1 >= 0) atomicAdd(&cnt[b1], 1u);
    if (b2 >= 0) atomicAdd(&cnt[b2], 1u);
    __syncthreads();
    if (threadIdx.x < kProfileCols) {
      const unsigned v = cnt[threadIdx.x];
      if (v) atomicAdd(&a.profile[(size_t)r_first * kProfileCols + threadIdx.x], (unsigned long long)v);
    }
  } else if (E < a.N) {
    unsigned long long* row = a.profile + (size_t)r * kProfileCols;
    if (count) atomicAdd(&row[q], (unsigned long long)count);
    if (b1 >= 0) atomicAdd(&row[b1], 1ull);
    if (b2 >= 0) atomicAdd(&row[b2], 1ull);
  }
}

}  // namespace nrv
