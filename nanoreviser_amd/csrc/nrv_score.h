// Device-side score of a merged call against per-base labels: what the two classifiers answered, joined with what they should have.
#pragma once
#include "nrv_merge.h"

namespace nrv {

// ---------------------------------------------------------------------------------------
// hoststage.score_calls is the DEFINITION; include/nanorev.h (nrv_revise_reads_raw_score_begin) names the 248 columns.
// One launch behind the merge - behind report_kernel where there is one - (score_enqueue in nrv_api.hip), shaped like
// report_kernel: one thread per event, workgroups of kMergeTile, the read found by merge_emit's binary search.  A thread whose
// event is the centre of a window reads the event's label byte (nrv_align_labels' format, 0xFF = unlabelled) and, where the
// window is labelled (code 1 .. 5), a1 / a2 and FOUR floats of the rows: p1[w][c1], p1[w][y1], p2[w][c2], p2[w][y2] - the
// confidence behind the Phred character and the probability given to the true class.  Nothing the merge left is read.
// Every counter is an integer - the loss too: score_nll16 is -log2 p in units of 2^-16 bit, formed from the f32 bit pattern by
// integers alone - so the bytes do not depend on the order in which tiles run:
//   * a tile that lies inside ONE read adds into 248 LDS counters with LDS atomics and then issues global 64-bit atomicAdds on
//     the read's row, non-zero counters only.  The counters are 32 bits wide; the two loss sums fit them: a tile adds at most
//     kMergeTile x (127 << 16) = 256 x 8 323 072 = 2 130 706 432 < 2^32;
//   * a tile that straddles a read boundary: each thread adds its own contributions to its read's row.
// The caller zeroes the block ahead of the launch; `windows` is stored once, by the read's first event.  A read without events
// has no thread and needs none: all of its columns are 0, which is what the block holds.
// ---------------------------------------------------------------------------------------
constexpr int kScoreCols = 248;
constexpr int kScoreBins = kPhredSteps + 1;   // bin b = #{k : thr[k] <= p}: Phred b + 1
enum ScoreCol {
  kScWindows = 0, kScLabelled = 1, kScConf1 = 2, kScConf2 = 38, kScCal1N = 63, kScCal1Ok = 103, kScCal2N = 143, kScCal2Ok = 183,
  kScNll1 = 223, kScNll2 = 224, kScDecKind = 225, kScSubRight = 245
};
static_assert(kScConf2 == kScConf1 + 36 && kScCal1N == kScConf2 + 25 && kScCal1Ok == kScCal1N + kScoreBins &&
              kScCal2N == kScCal1Ok + kScoreBins && kScCal2Ok == kScCal2N + kScoreBins && kScNll1 == kScCal2Ok + kScoreBins &&
              kScSubRight == kScDecKind + 20 && kScSubRight + 3 == kScoreCols, "the score block's columns");
static_assert((unsigned long long)kMergeTile * (127ull << 16) < (1ull << 32), "a tile's loss sum must fit a 32-bit LDS counter");

struct ScoreArgs {
  const SegRead* reads;
  int n_reads, T;
  long long N;
  const unsigned char* bases;            // [N]
  const unsigned char* labels;           // [N] one byte per event
  const signed char *a1, *a2;            // [N - T]
  const float *p1, *p2;                  // [N - T][6], [N - T][5]; both null: columns 63 .. 224 stay 0
  unsigned long long* score;             // [n_reads][kScoreCols], zeroed by the caller
  float thr[kPhredSteps];
};

// -log2 p in units of 2^-16 bit from the bits of p: the exponent gives the integer part, sixteen squarings of the mantissa the
// fraction (a square of 2 and more yields a 1 bit).  NaN, Inf, zero, denormals and negatives: 127 << 16; p >= 1: 0
__device__ __forceinline__ unsigned score_nll16(const float p) {
  const unsigned u = __float_as_uint(p), e = (u >> 23) & 255u;
  if ((u >> 31) || e == 0u || e == 255u) return 127u << 16;
  if (e >= 127u) return 0u;
  unsigned long long y = (1u << 23) | (u & 0x7FFFFFu);
  unsigned f = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    y = (y * y) >> 23;
    f <<= 1;
    if (y >= (1ull << 24)) { f |= 1u; y >>= 1; }
  }
  return ((127u - e) << 16) - f;
}

// What one labelled window adds: columns that get a 1 (a negative one: none), and the two loss terms
struct ScoreHit {
  int conf1 = -1, conf2 = -1, cal1 = -1, ok1 = -1, cal2 = -1, ok2 = -1, dk = -1, sub_right = -1;
  unsigned nll1 = 0, nll2 = 0;
  template <class Add>
  __device__ __forceinline__ void each(Add add) const {
    add(kScLabelled, 1u);
    add(conf1, 1u); add(conf2, 1u); add(dk, 1u);
    if (cal1 >= 0) { add(cal1, 1u); add(cal2, 1u); }
    if (ok1 >= 0) add(ok1, 1u);
    if (ok2 >= 0) add(ok2, 1u);
    if (nll1) add(kScNll1, nll1);
    if (nll2) add(kScNll2, nll2);
    if (sub_right >= 0) add(sub_right, 1u);
  }
};

__global__ void __launch_bounds__(256) score_kernel(const ScoreArgs a) {
  __shared__ unsigned cnt[kScoreCols];
  __shared__ int r_first, r_last;
  const long long E = (long long)blockIdx.x * kMergeTile + threadIdx.x;
  if (threadIdx.x < kScoreCols) cnt[threadIdx.x] = 0;
  int r = 0;
  bool labelled = false, first_ev = false;
  long long n_r = 0;
  ScoreHit hit;
  if (E < a.N) {
    int lo_r = 0, hi_r = a.n_reads - 1;                   // last read with ev_off <= E
    while (lo_r < hi_r) {
      const int mid = (lo_r + hi_r + 1) >> 1;
      if (a.reads[mid].ev_off <= E) lo_r = mid; else hi_r = mid - 1;
    }
    r = lo_r;
    const SegRead rd = a.reads[r];
    const long long j = E - rd.ev_off, o = (a.T - 1) / 2;
    n_r = rd.ev_len - a.T > 0 ? rd.ev_len - a.T : 0;
    first_ev = j == 0;
    if (j >= o && j < o + n_r) {
      const unsigned lb = a.labels[E];
      const int code = (int)(lb & 7u);
      labelled = lb != 0xFFu && code >= 1 && code <= 5;
      if (labelled) {
        const long long w = E - o;
        const unsigned base = a.bases[E];
        const bool del_after = (lb & 16u) != 0;
        const int y1 = del_after ? 0 : code, y2 = code - 1;
        const int x = a.a1[w], g2 = a.a2[w], y = g2 + 1;
        const int c1 = x < 0 ? 0 : (x > 5 ? 5 : x), c2 = g2 < 0 ? 0 : (g2 > 4 ? 4 : g2);
        hit.conf1 = kScConf1 + 6 * y1 + c1;
        hit.conf2 = kScConf2 + 5 * y2 + c2;
        const bool agree = x == y && x >= 2, dele = x == 0 && y >= 2, drop = x == 1 && y == 1;
        const unsigned long long lab = 0x414754432D44ull;   // "D-CTGA" (hoststage._LAB2CHR)
        const bool same = ((unsigned)(lab >> (8 * c1)) & 255u) == base;
        const int d = agree ? (same ? 0 : 1) : (dele ? 2 : (drop ? 3 : 4));
        const int kind = del_after ? 3 : (code == 1 ? 2 : ((lb & 8u) ? 1 : 0));
        hit.dk = kScDecKind + 4 * d + kind;
        if (d == 1 && c1 == code) hit.sub_right = kScSubRight;
        if (a.p1) {
          const float* q1 = a.p1 + w * 6;
          const float* q2 = a.p2 + w * 5;
          const int b1 = (int)merge_phred_steps(a.thr, q1[c1]), b2 = (int)merge_phred_steps(a.thr, q2[c2]);
          hit.cal1 = kScCal1N + b1; hit.cal2 = kScCal2N + b2;
          if (c1 == y1) hit.ok1 = kScCal1Ok + b1;
          if (c2 == y2) hit.ok2 = kScCal2Ok + b2;
          hit.nll1 = score_nll16(q1[y1]);
          hit.nll2 = score_nll16(q2[y2]);
        }
      }
    }
    if (threadIdx.x == 0) r_first = r;
    if (E == a.N - 1 || threadIdx.x == kMergeTile - 1) r_last = r;
  }
  __syncthreads();                                        // every workgroup has event blockIdx.x * kMergeTile < N: both are set
  const bool one_read = r_first == r_last;                // reads tile [0, N) in order: the same read at both ends = one read
  if (one_read) {
    if (labelled) hit.each([&](int col, unsigned v) { atomicAdd(&cnt[col], v); });
    __syncthreads();
    if (threadIdx.x < kScoreCols) {
      const unsigned v = cnt[threadIdx.x];
      if (v) atomicAdd(&a.score[(size_t)r_first * kScoreCols + threadIdx.x], (unsigned long long)v);
    }
  } else if (labelled) {
    unsigned long long* row = a.score + (size_t)r * kScoreCols;
    hit.each([&](int col, unsigned v) { atomicAdd(&row[col], (unsigned long long)v); });
  }
  if (first_ev) a.score[(size_t)r * kScoreCols + kScWindows] = (unsigned long long)n_r;   // nobody adds to this column
}

}  // namespace nrv
