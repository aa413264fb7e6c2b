// Device-side read statistics: median / MAD per read, per-base mean / std, feature columns 1 and 2.
#pragma once
#include "nrv_common.h"
#include "nrv_segment.h"       // SegRead

namespace nrv {

// ---------------------------------------------------------------------------------------
// What the host stage computes between the file and the device call (preprocessing.py:100-101, 134-137
// through hoststage.median_mad / hoststage.event_stats and their C forms median_mad_i16, nrvh_event_stats), on the samples
// the call has uploaded anyway.  The results are the host's bit for bit:
//   * shift / scale come out of INTEGER histograms (order of the atomic increments does not matter) and one exact
//     f64 division by 2 or 4;
//   * mean / std are f64 sums in NumPy's pairwise order, one thread per event, with contraction switched off
//     (NumPy does not fuse x * x + s; hipcc would);
//   * the two feature columns are one correctly rounded f64 division and one rounding to f32 each.
// Launch order of one call (stats_enqueue in nrv_api.hip), all on the compute stream:
//   memset(scratch) -> stats_minmax -> stats_hist<0> -> stats_scan<0> -> stats_hist<1> -> stats_scan<1> -> event_stats
// stats_scan<1> writes shift / scale into the call's device copy of the read descriptors, where segment_kernel reads them.
// A read takes part only when its StatAux.on is non-zero; the others keep what the host sent.
// ---------------------------------------------------------------------------------------
struct StatAux {              // per read, uploaded with the call
  int last_dur;               // samples of the read's last base (3 or 5: hoststage.collapse_events)
  int on;                     // non-zero: statistics of this read are computed on the device
};
constexpr int kStatChunk = 8192;         // samples per workgroup of stats_minmax / stats_hist (32 per thread)
constexpr int kStatLdsWords = 16384;     // LDS counters of stats_hist (64 KiB): copies x bins
constexpr int kStatBins = 65536;         // counters per read and pass in global memory (an int16 spans at most that many values)
// scratch words per read: [0] max(32767 - x), [1] max(x + 32768) (both grow from the zero of the memset), [2] 2 x shift,
// [3..7] unused, then the two histograms
constexpr int kStatHead = 8;
constexpr size_t kStatWords = kStatHead + 2 * (size_t)kStatBins;

struct StatArgs {
  const short* raw;
  const SegRead* reads;       // stats_scan<1> writes shift / scale through the same pointer
  const StatAux* aux;
  unsigned* scratch;          // [n_reads][kStatWords], zeroed by the call
  int n_reads;
};

// grid (chunks of the longest read, n_reads)
__global__ void __launch_bounds__(256) stats_minmax_kernel(const StatArgs a) {
  const int r = blockIdx.y;
  if (!a.aux[r].on) return;
  const SegRead rd = a.reads[r];
  const long long c0 = (long long)blockIdx.x * kStatChunk;
  if (c0 >= rd.raw_len) return;
  const long long c1 = c0 + kStatChunk < rd.raw_len ? c0 + kStatChunk : rd.raw_len;
  const short* x = a.raw + rd.raw_off;
  int lo = 32767, hi = -32768;
  for (long long i = c0 + threadIdx.x; i < c1; i += 256) {
    const int v = x[i];
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  __shared__ int s_lo[256], s_hi[256];
  s_lo[threadIdx.x] = lo; s_hi[threadIdx.x] = hi;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const int l2 = s_lo[threadIdx.x + w], h2 = s_hi[threadIdx.x + w];
      if (l2 < s_lo[threadIdx.x]) s_lo[threadIdx.x] = l2;
      if (h2 > s_hi[threadIdx.x]) s_hi[threadIdx.x] = h2;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    unsigned* sc = a.scratch + (size_t)r * kStatWords;
    atomicMax(sc + 0, (unsigned)(32767 - s_lo[0]));
    atomicMax(sc + 1, (unsigned)(s_hi[0] + 32768));
  }
}

// PASS 0: counts of x - base; PASS 1: counts of |2 x - 2 shift| / 2 (all of one parity, so halving loses nothing).
// Both need `range` = top - base + 1 counters.  Up to 4096 of them: the workgroup counts in LDS, in as many copies as fit
// (a lane uses copy lane % copies: neighbouring samples of a trace are often equal, and equal values in one wave would
// queue behind one counter), then adds what is non-zero to the read's global histogram.  Wider reads (an int16 can span
// 65 536 values; 256 KiB of counters do not fit the LDS) count in global memory directly.
template <int PASS>
__global__ void __launch_bounds__(256) stats_hist_kernel(const StatArgs a) {
  const int r = blockIdx.y;
  if (!a.aux[r].on) return;
  const SegRead rd = a.reads[r];
  const long long c0 = (long long)blockIdx.x * kStatChunk;
  if (c0 >= rd.raw_len) return;
  const long long c1 = c0 + kStatChunk < rd.raw_len ? c0 + kStatChunk : rd.raw_len;
  const short* x = a.raw + rd.raw_off;
  unsigned* sc = a.scratch + (size_t)r * kStatWords;
  const int base = 32767 - (int)sc[0], top = (int)sc[1] - 32768;
  const int range = top - base + 1;
  const int s2 = (int)sc[2];
  unsigned* hist = sc + kStatHead + (PASS ? kStatBins : 0);
  __shared__ unsigned cnt[kStatLdsWords];
  if (range <= 4096) {
    int nb = 64;
    while (nb < range) nb <<= 1;
    int copies = kStatLdsWords / nb;
    if (copies > 16) copies = 16;
    for (int i = threadIdx.x; i < copies * nb; i += 256) cnt[i] = 0;
    __syncthreads();
    unsigned* mine = cnt + (threadIdx.x & (copies - 1)) * nb;
    for (long long i = c0 + threadIdx.x; i < c1; i += 256) {
      const int v = x[i];
      int k;
      if (PASS == 0) k = v - base;
      else { k = 2 * v - s2; k = (k < 0 ? -k : k) >> 1; }
      atomicAdd(mine + k, 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < range; b += 256) {
      unsigned s = 0;
      for (int c = 0; c < copies; ++c) s += cnt[c * nb + b];
      if (s) atomicAdd(hist + b, s);
    }
  } else {
    for (long long i = c0 + threadIdx.x; i < c1; i += 256) {
      const int v = x[i];
      int k;
      if (PASS == 0) k = v - base;
      else { k = 2 * v - s2; k = (k < 0 ? -k : k) >> 1; }
      atomicAdd(hist + k, 1u);
    }
  }
}

// The two middle order statistics of a histogram (two_middle of nrv_host_fast5.c): lo = first bin whose running count
// reaches n / 2, hi = first bin whose running count reaches n / 2 + 1; for odd n both are hi.  One workgroup per read:
// every thread sums a contiguous run of bins, thread 0 walks the 256 sums, the two owners walk their own runs.
template <int PASS>
__global__ void __launch_bounds__(256) stats_scan_kernel(const StatArgs a) {
  const int r = blockIdx.x;
  if (!a.aux[r].on) return;
  SegRead* rd = const_cast<SegRead*>(a.reads) + r;
  const long long n = rd->raw_len;
  unsigned* sc = a.scratch + (size_t)r * kStatWords;
  const int base = 32767 - (int)sc[0], top = (int)sc[1] - 32768;
  const int range = top - base + 1;
  const unsigned* hist = sc + kStatHead + (PASS ? kStatBins : 0);
  const int per = (range + 255) / 256;
  const int b0 = threadIdx.x * per, b1 = b0 + per < range ? b0 + per : range;
  __shared__ unsigned long long part[256];
  __shared__ int found[2];
  unsigned long long s = 0;
  for (int b = b0; b < b1; ++b) s += hist[b];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long cum = 0;
    for (int t = 0; t < 256; ++t) { const unsigned long long v = part[t]; part[t] = cum; cum += v; }   // exclusive
    found[0] = found[1] = -1;
  }
  __syncthreads();
  const unsigned long long before = part[threadIdx.x];
  const unsigned long long want[2] = {(unsigned long long)(n / 2), (unsigned long long)(n / 2 + 1)};
  for (int q = 0; q < 2; ++q) {
    if (want[q] == 0 || before >= want[q] || before + s < want[q]) continue;      // the target lies in another thread's run
    unsigned long long cum = before;
    for (int b = b0; b < b1; ++b) {
      cum += hist[b];
      if (cum >= want[q]) { found[q] = b; break; }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int hi = found[1], lo = (n & 1) ? hi : found[0];
    if (PASS == 0) {
      sc[2] = (unsigned)(lo + hi + 2 * base);                 // 2 x shift
    } else {
      const int s2 = (int)sc[2], odd = s2 & 1;
      rd->shift = (double)s2 / 2.0;
      rd->scale = (double)((2 * lo + odd) + (2 * hi + odd)) / 4.0;
    }
  }
}

// ---- per-base mean / std in NumPy's pairwise order (pairwise_sum of nrv_host.c), feature columns 1 and 2 ----------------
// One run of at most 128 values: SQ == 0 sums x, SQ == 1 sums (x - m) * (x - m), the product rounded before it is added.
template <int SQ>
__device__ __forceinline__ double pw_leaf(const short* x, long long n, double m) {
#pragma clang fp contract(off)
  auto val = [&](long long i) -> double {
    const double v = (double)x[i];
    if (SQ == 0) return v;
    const double d = v - m;
    return d * d;
  };
  if (n < 8) {
    double res = 0.;
    for (long long i = 0; i < n; ++i) res = res + val(i);
    return res;
  }
  double r0 = val(0), r1 = val(1), r2 = val(2), r3 = val(3), r4 = val(4), r5 = val(5), r6 = val(6), r7 = val(7);
  long long i;
  for (i = 8; i < n - (n % 8); i += 8) {
    r0 = r0 + val(i); r1 = r1 + val(i + 1); r2 = r2 + val(i + 2); r3 = r3 + val(i + 3);
    r4 = r4 + val(i + 4); r5 = r5 + val(i + 5); r6 = r6 + val(i + 6); r7 = r7 + val(i + 7);
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res = res + val(i);
  return res;
}
// Longer runs: halved, the first half rounded down to a multiple of 8, the halves' sums added - the recursion of
// pairwise_sum walked with an explicit stack.  Depth: a half is at most l / 2 + 8 long, so level k holds at most
// (n - 16) / 2^k + 16 values; n < 2^32 (int32 starts, an int last_dur) reaches 128 within 27 levels.
template <int SQ>
__device__ double pw_sum(const short* x, long long n, double m) {
#pragma clang fp contract(off)
  if (n <= 128) return pw_leaf<SQ>(x, n, m);
  constexpr int kDepth = 40;
  long long off[kDepth], len[kDepth];
  double left[kDepth];
  int st[kDepth];
  int sp = 0;
  off[0] = 0; len[0] = n; st[0] = 0;
  double ret = 0.;
  while (sp >= 0) {
    const long long o = off[sp], l = len[sp];
    if (st[sp] == 0) {
      if (l <= 128) { ret = pw_leaf<SQ>(x + o, l, m); --sp; continue; }
      long long n2 = l / 2;
      n2 -= n2 % 8;
      st[sp] = 1;
      ++sp; off[sp] = o; len[sp] = n2; st[sp] = 0;
    } else if (st[sp] == 1) {
      long long n2 = l / 2;
      n2 -= n2 % 8;
      left[sp] = ret;
      st[sp] = 2;
      ++sp; off[sp] = o + n2; len[sp] = l - n2; st[sp] = 0;
    } else {
      ret = left[sp] + ret;
      --sp;
    }
  }
  return ret;
}

struct EvStatArgs {
  const short* raw;
  const int* starts;          // [N] relative to the first sample of their own read
  const SegRead* reads;       // shift / scale as stats_scan_kernel<1> left them
  const StatAux* aux;
  int n_reads;
  long long N;
  float* feat;                // [N][6]: columns 1 and 2 are written (may be null)
  double *mean, *std;         // [N] (may be null)
};
// One thread per base: raw[starts[e], starts[e + 1]) of its read, the last base starts[e] + last_dur, clipped to the read
// like a Python slice; an empty range gives NaN (np.mean / np.std of an empty slice).
__global__ void __launch_bounds__(256) event_stats_kernel(const EvStatArgs a) {
#pragma clang fp contract(off)
  const long long E = (long long)blockIdx.x * 256 + threadIdx.x;
  if (E >= a.N) return;
  int lo_r = 0, hi_r = a.n_reads - 1;                   // last read with ev_off <= E
  while (lo_r < hi_r) {
    const int mid = (lo_r + hi_r + 1) >> 1;
    if (a.reads[mid].ev_off <= E) lo_r = mid; else hi_r = mid - 1;
  }
  if (!a.aux[lo_r].on) return;
  const SegRead rd = a.reads[lo_r];
  if (E >= rd.ev_off + rd.ev_len) return;
  long long s = a.starts[E];
  long long t = E + 1 < rd.ev_off + rd.ev_len ? (long long)a.starts[E + 1] : s + a.aux[lo_r].last_dur;
  if (s < 0) s = 0;
  if (s > rd.raw_len) s = rd.raw_len;
  if (t > rd.raw_len) t = rd.raw_len;
  const long long n = t - s;
  double m, sd;
  if (n <= 0) {
    m = sd = __longlong_as_double(0x7ff8000000000000ll);
  } else {
    const short* x = a.raw + rd.raw_off + s;
    m = pw_sum<0>(x, n, 0.) / (double)n;
    sd = sqrt(pw_sum<1>(x, n, m) / (double)n);
  }
  if (a.mean) a.mean[E] = m;
  if (a.std) a.std[E] = sd;
  if (a.feat) {
    a.feat[E * 6 + 1] = (float)(m / rd.shift);
    a.feat[E * 6 + 2] = (float)(sd / rd.scale);
  }
}

}  // namespace nrv
