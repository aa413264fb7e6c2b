// Fitting the per-window tail on the device: the training set (main_out rows of labelled windows), the gradient of one batch
// and the Adam step.
#pragma once
#include "nrv_merge.h"   // SegRead, kMergeTile, merge_block_scan
#include "nrv_head.h"    // kHeadMaxT, head_final_kernel (whose forward tail_grad_kernel repeats operation for operation)

namespace nrv {

// ---------------------------------------------------------------------------------------
// nanoreviser_amd/tailfit.py is the DEFINITION; include/nanorev.h (nrv_fit_*) states the rule.  Only the four tensors behind
// Flatten(main_out) are fitted - feature.kernel Wf [6T][16], feature.bias bf [16], final_out.kernel Wo [16][C], final_out.bias
// bo [C] - and the centres Ce [C][16] of the reference's centre loss; the 56 tensors in front stay as they are, so a window is
// its 6T main_out values for the whole fit.  One parameter vector per model, P = 96T + 16 + 16C + C + 16C floats:
//   [Wf | bf | Wo | bo | Ce]
// THE SET (per model): flat [rows][6T] f32 (index t * 6 + k) and y [rows] u8.  nrv_fit_add_reads_raw fills it behind the f32
// kernels' head launch of every launch group (fit_enqueue in nrv_api.hip):
//   fit_label_count -> fit_tile_scan -> fit_label_scatter   once per call, one thread per event as score_kernel: an integer
//     exclusive scan of "this event is the centre of a labelled window of its own read" in event (= window) order gives the
//     window's slot; the scatter stores the slot into slot[w] (the caller filled it with -1) and y1 / y2 into the set;
//   tail_gather_kernel   behind each group: one thread per (window of the group, t * 6 + k); a labelled window's value moves
//     from main_out [tile][t][32 rows][8] to flat[slot][t * 6 + k].
// Plain stores, no atomics.
// THE STEP: 2 launches per batch of b rows, enqueued back to back:
//   tail_grad_kernel   one workgroup per 32 rows of the batch.  Forward IN head_final_kernel's OPERATION ORDER (same LDS
//     images, same fmaf chains, same expf and division), so p is what nrv_predict* gives in f32 mode, bit for bit.  Then
//     per row  dl = cw[y] (p - onehot(y)),  df = Wo dl + 2 lambda (f - Ce[y]),  dz = df where f > 0 (f = relu(z): z > 0
//     exactly where f > 0),  and the 32 rows summed in ascending row order into one partial vector [P]; the statistics of
//     the 32 rows in f64.  Nothing is divided by b here.
//   tail_adam_kernel   ONE workgroup: thread per parameter, g = (sum of the partials in ascending workgroup order) / b, the
//     finite check over all of g, then Adam in f32 with every operation rounded on its own (no contraction), sqrt and / the
//     correctly rounded ones.  lr_t comes from a table the host computed in f64, indexed by the step counter that lives on
//     the device (a skipped batch does not advance it, and the host does not look in between).
// No atomics anywhere: two runs give the same bytes.
// ---------------------------------------------------------------------------------------
constexpr int kFitMaxB = 65536;                    // rows of one batch
constexpr int kFitAdamThreads = 1024;
constexpr int kFitMaxP = 96 * kHeadMaxT + 16 + 16 * 6 + 6 + 16 * 6;
static_assert(kFitMaxP <= 4 * kFitAdamThreads, "tail_adam_kernel keeps four parameters per thread");

struct FitLabelArgs {
  const SegRead* reads;
  int n_reads, T;
  long long N;
  const unsigned char* labels;           // [N] nrv_align_labels' bytes, 0xFF = unlabelled
  unsigned long long* tile;              // [tiles + 1] scratch: sums, then exclusive offsets; [tiles] = the total
  int* slot;                             // [N - T], -1 where the window is not labelled (filled by the caller)
  long long base, cap;                   // rows the set holds already; rows it can hold
  unsigned char *y1, *y2;                // the set's labels
};

// the event's label byte if it is the centre of a labelled window of its own read, else -1; *w = the window
__device__ __forceinline__ int fit_classify(const FitLabelArgs& a, const long long E, long long* w) {
  int lo_r = 0, hi_r = a.n_reads - 1;                     // last read with ev_off <= E
  while (lo_r < hi_r) {
    const int mid = (lo_r + hi_r + 1) >> 1;
    if (a.reads[mid].ev_off <= E) lo_r = mid; else hi_r = mid - 1;
  }
  const SegRead rd = a.reads[lo_r];
  const long long j = E - rd.ev_off, o = (a.T - 1) / 2;
  const long long n_r = rd.ev_len - a.T > 0 ? rd.ev_len - a.T : 0;
  if (j < o || j >= o + n_r) return -1;
  const unsigned lb = a.labels[E];
  const int code = (int)(lb & 7u);
  if (lb == 0xFFu || code < 1 || code > 5) return -1;
  *w = E - o;
  return (int)lb;
}

__global__ void __launch_bounds__(256) fit_label_count_kernel(const FitLabelArgs a) {
  const long long E = (long long)blockIdx.x * kMergeTile + threadIdx.x;
  long long w = 0;
  const unsigned flag = (E < a.N && fit_classify(a, E, &w) >= 0) ? 1u : 0u;
  unsigned total;
  (void)merge_block_scan(flag, &total);
  if (threadIdx.x == 0) a.tile[blockIdx.x] = total;
}

// One workgroup: tile sums -> exclusive offsets, 256 at a time with a running carry; the total behind them.
__global__ void __launch_bounds__(256) fit_tile_scan_kernel(const FitLabelArgs a, const int tiles) {
  unsigned long long carry = 0;
  for (int b = 0; b < tiles; b += 256) {
    const int i = b + threadIdx.x;
    const unsigned v = i < tiles ? (unsigned)a.tile[i] : 0u;      // a tile's sum is at most kMergeTile
    unsigned total;
    const unsigned before = merge_block_scan(v, &total);
    if (i < tiles) a.tile[i] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) a.tile[tiles] = carry;
}

__global__ void __launch_bounds__(256) fit_label_scatter_kernel(const FitLabelArgs a) {
  const long long E = (long long)blockIdx.x * kMergeTile + threadIdx.x;
  long long w = 0;
  const int lb = E < a.N ? fit_classify(a, E, &w) : -1;
  unsigned total;
  const unsigned before = merge_block_scan(lb >= 0 ? 1u : 0u, &total);
  if (lb < 0) return;
  const long long s = a.base + (long long)a.tile[blockIdx.x] + before;
  if (s >= a.cap || w < 0 || w >= a.N - a.T) return;      // (the host counted by the same rule and sized the set: never taken)
  const int code = lb & 7;
  a.slot[w] = (int)s;
  a.y1[s] = (unsigned char)((lb & 16) ? 0 : code);
  a.y2[s] = (unsigned char)(code - 1);
}

struct TailGatherArgs {
  const float* mo[2];                    // main_out of the group [tile][t][32 rows][8]
  float* flat[2];                        // the set [cap][6T]
  const int* slot;                       // the group's first window
  int n, T;                              // windows of the group
  long long cap;
};
// grid = (ceil(n * 6T / 256), 2 models)
__global__ void __launch_bounds__(256) tail_gather_kernel(const TailGatherArgs a) {
  const int K = 6 * a.T;
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)a.n * K) return;
  const int i = (int)(g / K), j = (int)(g % K);
  const long long s = a.slot[i];
  if (s < 0 || s >= a.cap) return;
  const int t = j / 6, k = j % 6;
  a.flat[blockIdx.y][s * K + j] = a.mo[blockIdx.y][((size_t)(i >> 5) * a.T + t) * 256 + (i & 31) * 8 + k];
}

// ---- the step ----------------------------------------------------------------------------------------------------------
struct TailStat { double ce, center; long long correct, rows; };         // of one workgroup's rows
struct TailState { long long t, rows, correct, steps, nonfinite; double ce, center; };   // of one model, on the device

struct TailGradArgs {
  const float* flat;                     // the set's rows [.][6T]
  const unsigned char* y;
  const unsigned* rows;                  // [b] row indices of this batch (checked by the host)
  const float* par;                      // [P]
  float* partial;                        // [workgroups][P]           (GRAD only)
  TailStat* pstat;                       // [workgroups]
  float* p_out;                          // [b][C] or null
  int T, C, b;
  float lambda;
  float cw[6];
};

template <bool GRAD>
__global__ void __launch_bounds__(256) tail_grad_kernel(const TailGradArgs a) {
  constexpr int KPMAX = 6 * kHeadMaxT;           // head_final_kernel's images
  constexpr int FSM = KPMAX + 4;
  __shared__ __attribute__((aligned(16))) float flatv[32 * FSM];
  __shared__ __attribute__((aligned(16))) float fwT[16 * FSM];
  __shared__ float featv[32 * 17];
  __shared__ float logit[32 * 8];
  __shared__ float dl[32 * 8];
  __shared__ float dz[32 * 17];
  __shared__ float wo[16 * 8];
  __shared__ float cen[8 * 16];
  __shared__ int ys[32];
  __shared__ float r_ce[32], r_cen[32];
  __shared__ int r_ok[32];
  const int T = a.T, C = a.C, tile = blockIdx.x, tid = threadIdx.x;
  const int K = 6 * T, KP = (K + 3) & ~3;
  const int oBf = 16 * K, oWo = oBf + 16, oBo = oWo + 16 * C, oCe = oBo + C, P = oCe + 16 * C;
  const float* featw = a.par;
  const float* featb = a.par + oBf;
  const float* outw = a.par + oWo;
  const float* outb = a.par + oBo;
  const int n_here = a.b - tile * 32 < 32 ? a.b - tile * 32 : 32;
  for (int i = tid; i < 16 * KP; i += 256) {
    const int f = i / KP, k = i % KP;
    fwT[f * FSM + k] = k < K ? featw[k * 16 + f] : 0.f;
  }
  for (int i = tid; i < 32 * KP; i += 256) {
    const int r = i / KP, k = i % KP;
    flatv[r * FSM + k] = (r < n_here && k < K) ? a.flat[(size_t)a.rows[tile * 32 + r] * K + k] : 0.f;
  }
  if (tid < 32) ys[tid] = tid < n_here ? (int)a.y[a.rows[tile * 32 + tid]] : 0;
  if (tid < 16 * C) { wo[(tid / C) * 8 + tid % C] = outw[tid]; cen[(tid / 16) * 16 + tid % 16] = a.par[oCe + tid]; }
  __syncthreads();
  for (int it = tid; it < 32 * 16; it += 256) {
    const int r = it >> 4, f = it & 15;
    float v = featb[f];
    const f32x4* fr = (const f32x4*)(flatv + r * FSM);
    const f32x4* fw = (const f32x4*)(fwT + f * FSM);
#pragma unroll 4
    for (int k4 = 0; k4 < KP / 4; ++k4) {
      const f32x4 x = fr[k4], w = fw[k4];
      v = __builtin_fmaf(x[0], w[0], v);
      v = __builtin_fmaf(x[1], w[1], v);
      v = __builtin_fmaf(x[2], w[2], v);
      v = __builtin_fmaf(x[3], w[3], v);
    }
    featv[r * 17 + f] = relu_nan(v);
  }
  __syncthreads();
  {
    const int r = tid >> 3, cc = tid & 7;
    if (cc < C) {
      float v = outb[cc];
#pragma unroll
      for (int f = 0; f < 16; ++f) v = __builtin_fmaf(featv[r * 17 + f], outw[f * C + cc], v);
      logit[r * 8 + cc] = v;
    }
  }
  __syncthreads();
  if (tid < 32) {
    float ce = 0.f, cn = 0.f;
    int ok = 0;
    if (tid < n_here) {
      float mx = logit[tid * 8];
      for (int cc = 1; cc < C; ++cc) mx = __builtin_fmaxf(mx, logit[tid * 8 + cc]);
      float e[8], sum = 0.f;
      for (int cc = 0; cc < C; ++cc) { e[cc] = expf(logit[tid * 8 + cc] - mx); sum += e[cc]; }
      const int yy = ys[tid];
      const float w = a.cw[yy];
      int best = 0; float bv = -1.f, py = 0.f;
      for (int cc = 0; cc < C; ++cc) {
        const float p = e[cc] / sum;
        if (a.p_out) a.p_out[((size_t)tile * 32 + tid) * C + cc] = p;
        if (p > bv) { bv = p; best = cc; }     // strict > : ties -> lowest index
        if (cc == yy) py = p;
        dl[tid * 8 + cc] = w * (p - (cc == yy ? 1.f : 0.f));
      }
      ok = best == yy;
      ce = w * -logf(py);
      for (int f = 0; f < 16; ++f) {
        const float d = featv[tid * 17 + f] - cen[yy * 16 + f];
        cn = __builtin_fmaf(d, d, cn);
      }
    } else {
      for (int cc = 0; cc < C; ++cc) dl[tid * 8 + cc] = 0.f;
    }
    r_ce[tid] = ce; r_cen[tid] = cn; r_ok[tid] = ok;
  }
  __syncthreads();
  if (tid == 0) {
    TailStat s{0.0, 0.0, 0, n_here};
    for (int r = 0; r < n_here; ++r) { s.ce += (double)r_ce[r]; s.center += (double)r_cen[r]; s.correct += r_ok[r]; }
    a.pstat[tile] = s;
  }
  if constexpr (GRAD) {
    const float two_l = 2.f * a.lambda;
    for (int it = tid; it < 32 * 16; it += 256) {
      const int r = it >> 4, f = it & 15;
      float v = 0.f;
      if (r < n_here) {
        const float fv = featv[r * 17 + f];
        for (int cc = 0; cc < C; ++cc) v = __builtin_fmaf(dl[r * 8 + cc], wo[f * 8 + cc], v);
        v = __builtin_fmaf(two_l, fv - cen[ys[r] * 16 + f], v);
        if (!(fv > 0.f)) v = 0.f;
      }
      dz[r * 17 + f] = v;
    }
    __syncthreads();
    float* out = a.partial + (size_t)tile * P;
    for (int idx = tid; idx < P; idx += 256) {
      float s = 0.f;
      if (idx < oBf) {                                     // dWf[k][f] = sum_r flat[r][k] dz[r][f]
        const int k = idx >> 4, f = idx & 15;
        for (int r = 0; r < 32; ++r) s = __builtin_fmaf(flatv[r * FSM + k], dz[r * 17 + f], s);
      } else if (idx < oWo) {                              // dbf
        const int f = idx - oBf;
        for (int r = 0; r < 32; ++r) s += dz[r * 17 + f];
      } else if (idx < oBo) {                              // dWo[f][c] = sum_r f[r][f] dl[r][c]
        const int f = (idx - oWo) / C, cc = (idx - oWo) % C;
        for (int r = 0; r < 32; ++r) s = __builtin_fmaf(featv[r * 17 + f], dl[r * 8 + cc], s);
      } else if (idx < oCe) {                              // dbo
        const int cc = idx - oBo;
        for (int r = 0; r < 32; ++r) s += dl[r * 8 + cc];
      } else {                                             // dCe[c][f] = -2 lambda sum_{r : y_r = c} (f[r][f] - Ce[c][f])
        const int cc = (idx - oCe) >> 4, f = (idx - oCe) & 15;
        for (int r = 0; r < n_here; ++r)
          if (ys[r] == cc) s = __builtin_fmaf(-two_l, featv[r * 17 + f] - cen[cc * 16 + f], s);
      }
      out[idx] = s;
    }
  }
}

enum TailMode { kTailGradOnly = 0, kTailTrain = 1, kTailEval = 2 };
struct TailAdamArgs {
  const float* partial;                  // [n_wg][P]
  const TailStat* pstat;                 // [n_wg]
  int n_wg, b, P, mode;
  float *par, *m, *v, *g;                // [P] each
  TailState* st;
  const float* lr;                       // lr_t for t = t0 + 1 ..: lr[t - t0] is the step that takes t to t + 1
  long long t0, n_lr;
  float beta1, beta2, eps;
};

__device__ __forceinline__ bool fit_nonfinite(const float x) { return (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u; }

__global__ void __launch_bounds__(kFitAdamThreads) tail_adam_kernel(const TailAdamArgs a) {
#pragma clang fp contract(off)
  __shared__ int bad;
  const int tid = threadIdx.x;
  const long long t = a.st->t;                             // read by everybody before thread 0 moves it (behind the barriers)
  if (tid == 0) bad = 0;
  __syncthreads();
  float g[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.mode != kTailEval) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = tid + j * kFitAdamThreads;
      if (idx < a.P) {
        float s = 0.f;
        for (int w = 0; w < a.n_wg; ++w) s += a.partial[(size_t)w * a.P + idx];
        g[j] = s / (float)a.b;
        a.g[idx] = g[j];
        if (fit_nonfinite(g[j])) bad = 1;
      }
    }
  }
  __syncthreads();
  const bool skip = bad != 0;
  if (a.mode == kTailTrain && !skip && t - a.t0 >= 0 && t - a.t0 < a.n_lr) {
    const float lr = a.lr[t - a.t0];
    const float c1 = 1.f - a.beta1, c2 = 1.f - a.beta2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = tid + j * kFitAdamThreads;
      if (idx < a.P) {
        const float mm = a.beta1 * a.m[idx] + c1 * g[j];
        const float vv = a.beta2 * a.v[idx] + c2 * (g[j] * g[j]);
        a.m[idx] = mm;
        a.v[idx] = vv;
        a.par[idx] = a.par[idx] - (lr * mm) / (__builtin_sqrtf(vv) + a.eps);
      }
    }
  }
  if (tid == 0) {
    TailState s = *a.st;
    if (a.mode == kTailTrain && skip) {
      s.nonfinite += 1;                                    // a skipped batch: counted, nothing else of it
    } else {
      double ce = 0.0, cn = 0.0;
      long long ok = 0, rows = 0;
      for (int w = 0; w < a.n_wg; ++w) { ce += a.pstat[w].ce; cn += a.pstat[w].center; ok += a.pstat[w].correct; rows += a.pstat[w].rows; }
      s.ce += ce; s.center += cn; s.correct += ok; s.rows += rows;
      if (a.mode == kTailGradOnly && skip) s.nonfinite += 1;
      if (a.mode == kTailTrain) { s.steps += 1; s.t = t + 1; }
    }
    *a.st = s;
  }
}

}  // namespace nrv
