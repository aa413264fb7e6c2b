// Device-side per-read revision report of a merged call: what the merge did to every read, counted where the merge runs.
#pragma once
#include "nrv_merge.h"

namespace nrv {

// ---------------------------------------------------------------------------------------
// hoststage.revision_report is the DEFINITION; include/nanorev.h (nrv_revise_reads_raw_report_begin) names the 24 columns.
// One launch behind merge_scatter (report_enqueue in nrv_api.hip), one thread per event and workgroups of kMergeTile like
// merge_emit, so the workgroups follow N and not the number of reads.  A thread finds its read by merge_emit's binary search and
// classifies its event from the bases, a1 / a2, the p1 / p2 rows (6 + 5 floats per window, for the near-tie column) and the
// record merge_emit left in rec (the count for bases_out, the quality for q_sum).
// Every counter is an integer, so the bytes do not depend on the order in which tiles run:
//   * a tile that lies inside ONE read (the common case: reads have ~9 k events) adds into 24 LDS counters with LDS atomics and
//     then issues at most 24 global atomicAdds on the read's row, non-zero counters only;
//   * a tile that straddles a read boundary: each thread adds its own non-zero contributions to its read's row.
// The caller zeroes the block ahead of the launch; bases_in and windows are stored once, by the read's first event.  A read
// without events has no thread and needs none: all of its columns are 0, which is what the block holds.
// ---------------------------------------------------------------------------------------
constexpr int kReportCols = 24;
enum ReportCol {
  kRcBasesIn = 0, kRcWindows = 1, kRcBasesOut = 2, kRcEdge = 3, kRcConfirmed = 4, kRcSubstituted = 5, kRcInserted = 6,
  kRcDeleted = 7, kRcUndecided = 8, kRcM1 = 9, kRcM2 = 15, kRcAgree2 = 20, kRcNearTie = 21, kRcQSum = 22
};

struct ReportArgs {
  const SegRead* reads;
  int n_reads, T;
  long long N;
  const unsigned char* bases;            // [N]
  const signed char *a1, *a2;            // [N - T]
  const float *p1, *p2;                  // [N - T][6], [N - T][5]; both null: near_tie stays 0
  const unsigned* rec;                   // [N] merge_emit's records
  int want_q;                            // rec carries a quality (FASTQ): q_sum is filled
  float tie_eps;
  unsigned long long* report;            // [n_reads][kReportCols], zeroed by the caller
};

// not (top1 - top2 >= eps) over the K values of one softmax row, in f32; a NaN anywhere in the row is a near-tie
template <int K>
__device__ __forceinline__ bool report_near_tie(const float* __restrict__ p, const float eps) {
  float t1 = p[0], t2 = -INFINITY;
  bool nan = t1 != t1;
#pragma unroll
  for (int k = 1; k < K; ++k) {
    const float v = p[k];
    nan = nan || v != v;
    if (v > t1) { t2 = t1; t1 = v; }
    else if (v > t2) t2 = v;
  }
  if (nan) return true;
  const float d = t1 - t2;
  return !(d >= eps);
}

__global__ void __launch_bounds__(256) report_kernel(const ReportArgs a) {
  __shared__ unsigned cnt[kReportCols];
  __shared__ int r_first, r_last;
  const long long E = (long long)blockIdx.x * kMergeTile + threadIdx.x;
  if (threadIdx.x < kReportCols) cnt[threadIdx.x] = 0;
  // this thread's contributions: up to three single counts (class, m1, m2) and the sums below
  int r = 0;
  int c_class = -1, c_m1 = -1, c_m2 = -1;
  unsigned out = 0, edge = 0, agree2 = 0, tie = 0, qsum = 0;
  bool first_ev = false;
  SegRead rd{};
  long long n_r = 0;
  if (E < a.N) {
    int lo_r = 0, hi_r = a.n_reads - 1;                   // last read with ev_off <= E
    while (lo_r < hi_r) {
      const int mid = (lo_r + hi_r + 1) >> 1;
      if (a.reads[mid].ev_off <= E) lo_r = mid; else hi_r = mid - 1;
    }
    r = lo_r;
    rd = a.reads[r];
    const long long j = E - rd.ev_off, o = (a.T - 1) / 2;
    n_r = rd.ev_len - a.T > 0 ? rd.ev_len - a.T : 0;
    first_ev = j == 0;
    const unsigned rec = a.rec[E];
    out = rec & 3u;
    if (a.want_q) qsum = out * ((rec >> 24) - 33u);
    if (j >= o && j < o + n_r) {
      const long long w = E - o;
      const unsigned base = a.bases[E];
      const int c1 = a.a1[w], c2 = a.a2[w];
      const int x = c1, y = c2 + 1;
      const bool agree = x == y && x >= 2, dele = x == 0 && y >= 2, drop = x == 1 && y == 1;
      const int cx = x < 0 ? 0 : (x > 5 ? 5 : x), cy = y < 0 ? 0 : (y > 5 ? 5 : y);
      const unsigned long long lab = 0x414754432D44ull;   // "D-CTGA" (hoststage._LAB2CHR)
      auto chr = [&](int l) -> unsigned { return (unsigned)(lab >> (8 * l)) & 255u; };
      c_class = agree ? (chr(cx) == base ? kRcConfirmed : kRcSubstituted) : (dele ? kRcInserted : (drop ? kRcDeleted : kRcUndecided));
      c_m1 = kRcM1 + (c1 < 0 ? 0 : (c1 > 5 ? 5 : c1));
      c_m2 = kRcM2 + (c2 < 0 ? 0 : (c2 > 4 ? 4 : c2));
      agree2 = chr(cy) == base ? 1u : 0u;
      if (a.p1) tie = (report_near_tie<6>(a.p1 + w * 6, a.tie_eps) || report_near_tie<5>(a.p2 + w * 5, a.tie_eps)) ? 1u : 0u;
    } else {
      edge = 1;
    }
    if (threadIdx.x == 0) r_first = r;
    if (E == a.N - 1 || threadIdx.x == kMergeTile - 1) r_last = r;
  }
  __syncthreads();                                        // every workgroup has event blockIdx.x * kMergeTile < N: both are set
  const bool one_read = r_first == r_last;                // reads tile [0, N) in order: the same read at both ends = one read
  if (one_read) {
    if (E < a.N) {
      if (out) atomicAdd(&cnt[kRcBasesOut], out);
      if (edge) atomicAdd(&cnt[kRcEdge], 1u);
      if (c_class >= 0) { atomicAdd(&cnt[c_class], 1u); atomicAdd(&cnt[c_m1], 1u); atomicAdd(&cnt[c_m2], 1u); }
      if (agree2) atomicAdd(&cnt[kRcAgree2], 1u);
      if (tie) atomicAdd(&cnt[kRcNearTie], 1u);
      if (qsum) atomicAdd(&cnt[kRcQSum], qsum);
    }
    __syncthreads();
    if (threadIdx.x < kReportCols) {
      const unsigned v = cnt[threadIdx.x];
      if (v) atomicAdd(&a.report[(size_t)r_first * kReportCols + threadIdx.x], (unsigned long long)v);
    }
  } else if (E < a.N) {
    unsigned long long* row = a.report + (size_t)r * kReportCols;
    if (out) atomicAdd(&row[kRcBasesOut], (unsigned long long)out);
    if (edge) atomicAdd(&row[kRcEdge], 1ull);
    if (c_class >= 0) { atomicAdd(&row[c_class], 1ull); atomicAdd(&row[c_m1], 1ull); atomicAdd(&row[c_m2], 1ull); }
    if (agree2) atomicAdd(&row[kRcAgree2], 1ull);
    if (tie) atomicAdd(&row[kRcNearTie], 1ull);
    if (qsum) atomicAdd(&row[kRcQSum], (unsigned long long)qsum);
  }
  if (first_ev) {                                         // nobody adds to these two columns
    unsigned long long* row = a.report + (size_t)r * kReportCols;
    row[kRcBasesIn] = (unsigned long long)rd.ev_len;
    row[kRcWindows] = (unsigned long long)n_r;
  }
}

}  // namespace nrv
