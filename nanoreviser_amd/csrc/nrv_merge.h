// Device-side merge of the two models' calls into revised reads: characters, Phred characters, read offsets.
#pragma once
#include "nrv_common.h"
#include "nrv_segment.h"       // SegRead

namespace nrv {

// ---------------------------------------------------------------------------------------
// The last host step of a raw-read call (output_handeler.py:83, 104-122 through hoststage.merge_calls /
// expand_calls, cli.phred_chars), on the outputs the call has just left in its slot.  hoststage.emit_calls is the
// DEFINITION; the bytes are the host's:
//   * per event 0, 1 or 2 characters: the first (T - 1) / 2 and the last events of a read keep their base with quality
//     '#', every other event takes what merge_calls says for its window (labels clipped to 0..5 as there);
//   * the quality of a window is 33 + 1 + #{k : thr[k] <= min(p1[a1], p2[a2])}: the 39 thresholds are the steps of
//     cli.phred_chars as a function of the f32 confidence (cli.phred_thresholds), compared in f32 - no log10 here;
//   * positions come from an exclusive scan of the INTEGER counts over all events of the call, tiled: counts differ
//     in nothing with the order in which tiles run.
// Launch order of one call (merge_enqueue in nrv_api.hip), all on the compute stream behind the call's last group:
//   merge_emit (one thread per event: record + its tile's sum) -> merge_tile_scan (one workgroup walks the tile sums)
//   -> merge_scatter (one thread per event: scan inside the tile, characters, read offsets).
// The workgroups of the first and the last follow N, not the number of reads.
// ---------------------------------------------------------------------------------------
constexpr int kMergeTile = 256;          // events per workgroup of merge_emit / merge_scatter = one tile of the scan
constexpr int kPhredSteps = 39;          // Phred 2 .. 40

struct MergeArgs {
  const SegRead* reads;                  // the call's read descriptors (ev_off / ev_len; tile [0, N) in order)
  int n_reads, T;
  long long N;                           // events of the call; N - T windows
  const unsigned char* bases;            // [N] original bases (ASCII)
  const signed char *a1, *a2;            // [N - T] argmax of model1 / model2
  const float *p1, *p2;                  // [N - T][6], [N - T][5]; both null: no quality (FASTA)
  unsigned* rec;                         // [N] scratch: count | first-of-read flag << 2 | first << 8 | second << 16 | q << 24
  unsigned long long* tile;              // [tiles] scratch: sums, then exclusive offsets
  long long* off;                        // [n_reads + 1] out
  unsigned char *seq, *qual;             // [N + max(N - T, 0)] out (qual may be null)
  float thr[kPhredSteps];
};

// exclusive prefix of v over the 256 threads of the workgroup, *total = their sum (wave scan by __shfl_up, four waves through LDS)
__device__ __forceinline__ unsigned merge_block_scan(unsigned v, unsigned* total) {
  __shared__ unsigned ws[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  __syncthreads();                       // ws of an earlier call of this function has been read by everybody
  if (lane == 63) ws[wave] = x;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const unsigned s = ws[w];
    if (w < wave) before += s;
    all += s;
  }
  *total = all;
  return before + x - v;
}

// #{k : thr[k] <= conf}, compared in f32: a window's Phred value is 1 + this (merge_emit, and profile_kernel of nrv_profile.h)
__device__ __forceinline__ unsigned merge_phred_steps(const float (&thr)[kPhredSteps], const float conf) {
  unsigned k = 0;
#pragma unroll
  for (int i = 0; i < kPhredSteps; ++i) k += thr[i] <= conf ? 1u : 0u;
  return k;
}

__global__ void __launch_bounds__(256) merge_emit_kernel(const MergeArgs a) {
  const long long E = (long long)blockIdx.x * kMergeTile + threadIdx.x;
  unsigned count = 0, rec = 0;
  if (E < a.N) {
    int lo_r = 0, hi_r = a.n_reads - 1;                   // last read with ev_off <= E
    while (lo_r < hi_r) {
      const int mid = (lo_r + hi_r + 1) >> 1;
      if (a.reads[mid].ev_off <= E) lo_r = mid; else hi_r = mid - 1;
    }
    const SegRead rd = a.reads[lo_r];
    const long long j = E - rd.ev_off, o = (a.T - 1) / 2;
    const long long n_r = rd.ev_len - a.T > 0 ? rd.ev_len - a.T : 0;
    const unsigned base = a.bases[E];
    unsigned first = base, second = 0, q = '#';
    count = 1;
    if (j >= o && j < o + n_r) {
      const long long w = E - o;                          // window j - o of the read = window ev_off + j - o of the call
      const int c1 = a.a1[w], c2 = a.a2[w];
      const int x = c1, y = c2 + 1;
      const bool agree = x == y && x >= 2, dele = x == 0 && y >= 2, drop = x == 1 && y == 1;
      const int cx = x < 0 ? 0 : (x > 5 ? 5 : x), cy = y < 0 ? 0 : (y > 5 ? 5 : y);
      const unsigned long long lab = 0x414754432D44ull;   // "D-CTGA", label l in byte l (hoststage._LAB2CHR)
      auto chr = [&](int l) -> unsigned { return (unsigned)(lab >> (8 * l)) & 255u; };
      if (agree) first = chr(cx);
      second = chr(cy);
      count = drop ? 0 : (dele ? 2 : 1);
      if (a.p1) {
        const int g1 = c1 < 0 ? 0 : (c1 > 5 ? 5 : c1), g2 = c2 < 0 ? 0 : (c2 > 4 ? 4 : c2);
        const float u = a.p1[w * 6 + g1], v = a.p2[w * 5 + g2];
        const float conf = v < u ? v : u;
        q = 33 + 1 + merge_phred_steps(a.thr, conf);
      }
    }
    rec = count | (j == 0 ? 4u : 0u) | first << 8 | second << 16 | q << 24;
    a.rec[E] = rec;
  }
  unsigned total;
  (void)merge_block_scan(count, &total);
  if (threadIdx.x == 0) a.tile[blockIdx.x] = total;
}

// One workgroup: tile sums -> exclusive offsets, 256 at a time with a running carry; the total goes to off[n_reads] and to the
// empty reads at the end of the call (they have no event that could write it).
__global__ void __launch_bounds__(256) merge_tile_scan_kernel(const MergeArgs a, const int tiles) {
  unsigned long long carry = 0;
  for (int b = 0; b < tiles; b += 256) {
    const int i = b + threadIdx.x;
    const unsigned v = i < tiles ? (unsigned)a.tile[i] : 0u;      // a tile's sum is at most 2 x kMergeTile
    unsigned total;
    const unsigned before = merge_block_scan(v, &total);
    if (i < tiles) a.tile[i] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) {
    a.off[a.n_reads] = (long long)carry;
    for (int r = a.n_reads - 1; r >= 0 && a.reads[r].ev_len == 0; --r) a.off[r] = (long long)carry;
  }
}

__global__ void __launch_bounds__(256) merge_scatter_kernel(const MergeArgs a) {
  const long long E = (long long)blockIdx.x * kMergeTile + threadIdx.x;
  const unsigned rec = E < a.N ? a.rec[E] : 0u;
  const unsigned count = rec & 3u;
  unsigned total;
  const unsigned before = merge_block_scan(count, &total);
  if (E >= a.N) return;
  const long long pos = (long long)a.tile[blockIdx.x] + before;
  if (count >= 1) {
    a.seq[pos] = (unsigned char)(rec >> 8);
    if (a.qual) a.qual[pos] = (unsigned char)(rec >> 24);
  }
  if (count == 2) {
    a.seq[pos + 1] = (unsigned char)(rec >> 16);
    if (a.qual) a.qual[pos + 1] = (unsigned char)(rec >> 24);
  }
  if (rec & 4u) {                                          // first event of a read: its offset, and that of the empty reads in front of it
    int lo_r = 0, hi_r = a.n_reads - 1;
    while (lo_r < hi_r) {
      const int mid = (lo_r + hi_r + 1) >> 1;
      if (a.reads[mid].ev_off <= E) lo_r = mid; else hi_r = mid - 1;
    }
    a.off[lo_r] = pos;
    for (int r = lo_r - 1; r >= 0 && a.reads[r].ev_len == 0; --r) a.off[r] = pos;
  }
}

}  // namespace nrv
