// Device-side sliding-window quality trim of a merged call: per revised read the part worth keeping, (lo, hi).
#pragma once
#include "nrv_merge.h"

namespace nrv {

// ---------------------------------------------------------------------------------------
// hoststage.trim_bounds is the DEFINITION; include/nanorev.h (nrv_revise_reads_raw_trim_begin, nrv_trim_reads) names the
// arguments.  Read r has L = off[r + 1] - off[r] output characters with the Phred values q[0 .. L); position i is GOOD when
// i + W <= L (a window never reaches into the next read) and q[i] + ... + q[i + W - 1] >= Q * W; lo = the smallest good i,
// hi = the largest good i + W, no good position: lo = hi = 0.  Q in 1 .. 40, W in 1 .. 64: a sum is at most 2560.  Integers only.
// The qualities are those of the FASTQ form of the call whether one is written or not (the convention of nrv_profile.h).
// Three launches behind merge_scatter (and the report / edit launches), AHEAD of the record launches, which read their result
// (trim_enqueue in nrv_api.hip):
//   trim_qual   one thread per event, workgroups of kMergeTile, the read by merge_emit's binary search.  The event's Phred by the
//               rule of merge_emit (merge_phred_steps on the thresholds of THESE args), 2 for an edge event; the quality byte in
//               rec is not read - it is '#' in every FASTA call.  Written to the event's 0 / 1 / 2 output positions of tq, a
//               position being what edits_scatter forms: the scan of the merge counts in rec inside the tile + the merge's tile[].
//   trim_window the work follows the CHARACTERS, not the events and not the reads: one thread per output character, tiles of
//               256, the character's read by binary search over off.  The tile's q and a halo of W - 1 go into LDS as a prefix
//               sum P (the tile through merge_block_scan, the halo through one wave scan behind it), a window's sum is
//               P[i + W] - P[i].  The smallest and the largest good position of a read are reduced into a pair of 64-bit
//               accumulators per read: acc[r][0] = min i, acc[r][1] = min ~i (the complement: the maximum as a minimum, so that
//               ONE fill of 0xFF bytes initialises both).  A tile inside one read (the common case): per wave two ballots, per
//               workgroup LDS atomics, then at most two global atomicMin.  A tile that straddles a read boundary: one pair per
//               good thread.  Integer minima commute: the bytes do not depend on the order of the workgroups.
//   trim_finish one thread per read: the accumulators -> trim[r] = (lo, hi), one 16-byte store; untouched accumulators (a read
//               without a good position, or without characters: it had no thread in trim_window) -> (0, 0).
// The caller fills the accumulators with 0xFF in stream order ahead of trim_window: a second pass over the same block (the
// re-run of nrv_reads_raw_end) starts from nothing and gives the same bounds.  Grids are sized from the host's bound on the
// characters (N + max(N - T, 0)); threads at or beyond off[n_reads] do nothing and read nothing.
// ---------------------------------------------------------------------------------------
constexpr int kTrimMaxW = 64;

struct TrimQualArgs {
  const SegRead* reads;
  int n_reads, T;
  long long N;
  const signed char *a1, *a2;            // [N - T]
  const float *p1, *p2;                  // [N - T][6], [N - T][5]
  const unsigned* rec;                   // [N] merge_emit's records: the counts
  const unsigned long long* tile;        // [tiles] the merge's exclusive tile offsets
  unsigned char* tq;                     // [N + max(N - T, 0)] out: Phred per output character
  long long cap;                         // characters tq holds
  float thr[kPhredSteps];
};

struct TrimArgs {
  int n_reads, Q, W, bias;               // bias: what a byte of q carries above its Phred (0: trim_qual's; 33: quality characters)
  const long long* off;                  // [n_reads + 1] read offsets into q
  const unsigned char* q;                // [off[n_reads]]
  long long cap;                         // the host's bound on off[n_reads]: nothing at or beyond it is read
  unsigned long long* acc;               // [n_reads][2] filled with 0xFF by the caller
  long long* trim;                       // [n_reads][2] out
};

__global__ void __launch_bounds__(256) trim_qual_kernel(const TrimQualArgs a) {
  const long long E = (long long)blockIdx.x * kMergeTile + threadIdx.x;
  unsigned count = 0, q = 2;
  if (E < a.N) {
    int lo_r = 0, hi_r = a.n_reads - 1;                   // last read with ev_off <= E
    while (lo_r < hi_r) {
      const int mid = (lo_r + hi_r + 1) >> 1;
      if (a.reads[mid].ev_off <= E) lo_r = mid; else hi_r = mid - 1;
    }
    const SegRead rd = a.reads[lo_r];
    const long long j = E - rd.ev_off, o = (a.T - 1) / 2;
    const long long n_r = rd.ev_len - a.T > 0 ? rd.ev_len - a.T : 0;
    count = a.rec[E] & 3u;
    if (j >= o && j < o + n_r) {
      const long long w = E - o;
      const int c1 = a.a1[w], c2 = a.a2[w];
      const int g1 = c1 < 0 ? 0 : (c1 > 5 ? 5 : c1), g2 = c2 < 0 ? 0 : (c2 > 4 ? 4 : c2);
      const float u = a.p1[w * 6 + g1], v = a.p2[w * 5 + g2];
      const float conf = v < u ? v : u;
      q = 1 + merge_phred_steps(a.thr, conf);             // 1 .. 40
    }
  }
  unsigned total;
  const unsigned before = merge_block_scan(count, &total);
  if (E >= a.N) return;
  const long long pos = (long long)a.tile[blockIdx.x] + before;
  if (count >= 1 && pos < a.cap) a.tq[pos] = (unsigned char)q;
  if (count == 2 && pos + 1 < a.cap) a.tq[pos + 1] = (unsigned char)q;
}

__global__ void __launch_bounds__(256) trim_window_kernel(const TrimArgs a) {
  __shared__ unsigned P[256 + kTrimMaxW];                 // P[i] = q[c0] + ... + q[c0 + i - 1], i = 0 .. 256 + W - 1
  __shared__ unsigned t_min, t_max;
  __shared__ int r_first, r_last;
  long long total = a.off[a.n_reads];
  if (total > a.cap) total = a.cap;
  const long long c0 = (long long)blockIdx.x * 256, c = c0 + threadIdx.x;
  if (c0 >= total) return;                                // the whole workgroup: no barrier has been passed
  const int lane = threadIdx.x & 63;
  auto phred = [&](const long long at) -> unsigned {
    if (at >= total) return 0u;
    const int v = (int)a.q[at] - a.bias;
    return v > 0 ? (unsigned)v : 0u;
  };
  unsigned sum;
  const unsigned before = merge_block_scan(phred(c), &sum);
  P[threadIdx.x] = before;
  if (threadIdx.x < 64) {                                 // the halo: characters c0 + 256 .. c0 + 256 + W - 2, one wave
    unsigned x = lane < a.W - 1 ? phred(c0 + 256 + lane) : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane < kTrimMaxW - 1) P[256 + lane + 1] = sum + x;  // W - 1 <= 63 halo values
    if (lane == 0) { P[256] = sum; t_min = 0xFFFFFFFFu; t_max = 0u; }
  }
  int r = 0;
  long long i_read = 0, end = 0;                          // the character's index inside its read, the end of that read
  if (c < total) {
    int lo_r = 0, hi_r = a.n_reads - 1;                   // last read with off <= c: it holds c (an empty read in front does not)
    while (lo_r < hi_r) {
      const int mid = (lo_r + hi_r + 1) >> 1;
      if (a.off[mid] <= c) lo_r = mid; else hi_r = mid - 1;
    }
    r = lo_r;
    i_read = c - a.off[r];
    end = a.off[r + 1];
    if (threadIdx.x == 0) r_first = r;
    if (c == total - 1 || threadIdx.x == 255) r_last = r;
  }
  __syncthreads();                                        // P, t_min / t_max and both reads are set
  const bool good = c < total && c + a.W <= end && P[threadIdx.x + a.W] - P[threadIdx.x] >= (unsigned)(a.Q * a.W);
  if (r_first == r_last) {                                // reads tile [0, total) in order: the same read at both ends = one read
    const unsigned long long m = __ballot(good);
    if (m && lane == 0) {
      const unsigned w0 = threadIdx.x;                    // the wave's first thread
      atomicMin(&t_min, w0 + (unsigned)(__ffsll((long long)m) - 1));
      atomicMax(&t_max, w0 + (unsigned)(63 - __clzll((long long)m)) + 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && t_max) {                      // t_max: largest good thread + 1, 0 when none
      const unsigned long long base = (unsigned long long)(c0 - a.off[r_first]);
      atomicMin(&a.acc[2 * (size_t)r_first], base + t_min);
      atomicMin(&a.acc[2 * (size_t)r_first + 1], ~(base + (t_max - 1u)));
    }
  } else if (good) {
    atomicMin(&a.acc[2 * (size_t)r], (unsigned long long)i_read);
    atomicMin(&a.acc[2 * (size_t)r + 1], ~(unsigned long long)i_read);
  }
}

__global__ void __launch_bounds__(256) trim_finish_kernel(const TrimArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.n_reads) return;
  const unsigned long long lo = a.acc[2 * (size_t)r], hi_c = a.acc[2 * (size_t)r + 1];
  longlong2 v = make_longlong2(0, 0);
  if (lo != ~0ull) v = make_longlong2((long long)lo, (long long)(~hi_c) + a.W);
  *reinterpret_cast<longlong2*>(a.trim + 2 * (size_t)r) = v;
}

}  // namespace nrv
