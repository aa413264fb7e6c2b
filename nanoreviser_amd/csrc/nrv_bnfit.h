// Re-estimating the BatchNorm statistics inside the fitted section from rows of the set (nrv_fit_bn_reestimate): per-channel
// moments of the activations a BatchNorm normalises, formed on the device.
#pragma once
#include "nrv_fullfit.h"   // the forward launches run unchanged; sig_conv_image is the conv image of this depth's launches

namespace nrv {

// ---------------------------------------------------------------------------------------
// nanoreviser_amd/bnfit.py is the DEFINITION; include/nanorev.h (nrv_fit_bn_*) states the rule.  Per channel, with the pivot
// p = the LOADED moving mean widened to f64:  S1 = sum (x - p), S2 = sum (x - p)^2 in f64 over every element the BatchNorm
// normalises, m = S1 / N, mean = p + m, var = max(S2 / N - m m, 0), no contraction, each rounded once to f32.  gamma and beta
// are never touched.  THE FIT-OWNED BLOCK per model, kBnFloats floats, is what every fit launch reads a BatchNorm from:
//   [conv 264: the handle's image, s1 h1 at 32 / 40, s2 h2 at 248 / 256 | s_l1 h_l1 32 | s_l2 h_l2 128 | s_l3 h_l3 256 |
//    pivot 432 | mean 432 | var 432]                 channels of bn_c1, bn_c2, bn_l1, bn_l2, bn_l3 at 0, 8, 16, 48, 176
// ONE PASS per stage, in the fit's chunks; M = chunk rows x T (row, t) pairs; per chunk, behind the forward launches:
//   bn_col_moments_kernel<C>   H1 / H2 / H3 [M][C] as the forward launch left it.  Workgroup per kBnRows pairs; thread (pair
//     lane tid / C, channel tid % C) walks its pairs ascending, the 256 / C pair lanes are added ascending through LDS: one f64
//     pair per (workgroup, channel).
//   bn_conv_moments_kernel<STAGE>   a1 / a2 exist only in registers of sig_forward_kernel, so they are recomputed in its
//     thread layout and operation order (thread per (pair, 6 or 7 samples), conv_positions' fma chains; stage 2 with the block's
//     s1, h1 - those of stage 1).  Workgroup per kBnTiles x 32 pairs; a thread adds its samples and tiles ascending, the 256
//     threads are added through LDS in two ascending rounds of 16: one f64 pair per (workgroup, channel).
//   bn_reduce_kernel   workgroup per BatchNorm of the stage, thread per channel: adds the chunk's partials ascending onto the
//     running sums of the chunks before; behind the last chunk it forms mean and var.
// No atomics, no workgroup waits for another: the order of every sum is a function of (rows, T) alone.
// ---------------------------------------------------------------------------------------
constexpr int kBnConv = 0, kBnS1 = 264, kBnH1 = 296, kBnS2 = 328, kBnH2 = 456, kBnS3 = 584, kBnH3 = 840, kBnFold = 1096;
constexpr int kBnCh = 8 + 8 + 32 + 128 + 256;              // 432 channels of the five BatchNorms
constexpr int kBnPivot = kBnFold, kBnMean = kBnPivot + kBnCh, kBnVar = kBnMean + kBnCh, kBnFloats = kBnVar + kBnCh;
constexpr int kBnRows = 64, kBnTiles = 8;
static_assert(kBnFloats == 2392 && kBnS1 % 4 == 0 && kBnPivot % 4 == 0, "the fit's BatchNorm block");

struct BnColArgs {
  const float* x;                        // [M][C]
  const float* pivot;                    // [C]
  double* part;                          // [workgroups][2][C]: S1 | S2
  int M;
};
// grid = ceil(M / kBnRows)
template <int C>
__global__ void __launch_bounds__(256) bn_col_moments_kernel(const BnColArgs a) {
#pragma clang fp contract(off)
  static_assert(C == 32 || C == 128 || C == 256, "whole pair lanes");
  constexpr int RL = 256 / C;
  __shared__ double red[2][256];
  const int tid = threadIdx.x, c = tid % C, rl = tid / C;
  const double p = (double)a.pivot[c];
  const int m0 = blockIdx.x * kBnRows, m1 = m0 + kBnRows < a.M ? m0 + kBnRows : a.M;
  double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
  for (int m = m0 + rl; m < m1; m += RL) {
    const double d = (double)a.x[(size_t)m * C + c] - p;
    s1 += d;
    s2 += d * d;
  }
  if (RL > 1) {
    red[0][tid] = s1;
    red[1][tid] = s2;
    __syncthreads();
    if (tid < C)
      for (int k = 1; k < RL; ++k) {
        s1 += red[0][k * C + tid];
        s2 += red[1][k * C + tid];
      }
  }
  if (tid < C) {
    double* out = a.part + (size_t)blockIdx.x * 2 * C;
    out[c] = s1;
    out[C + c] = s2;
  }
}

// the NP samples p0 .. of one pair: a1 (STAGE 1) or a2 (STAGE 2) in conv_positions' operation order, added to s1 / s2
template <int STAGE, int NP>
__device__ __forceinline__ void bn_conv_samples(const float* cw, const float (&x)[11], int p0, const double (&pv)[8], double (&s1)[8],
                                                double (&s2)[8]) {
#pragma clang fp contract(off)
  float b1v[NP + 2][8];                                    // STAGE 1: a1; STAGE 2: c1, zero outside the 50 samples
#pragma unroll
  for (int q = 0; q < NP + 2; ++q) {
    const int p = p0 - 1 + q;
    const bool inside = (p >= 0) && (p < kSig);
    const float xm = x[q], xc = x[q + 1], xp = x[q + 2];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      float v = cw[24 + o];
      v = __builtin_fmaf(xm, cw[0 * 8 + o], v);
      v = __builtin_fmaf(xc, cw[1 * 8 + o], v);
      v = __builtin_fmaf(xp, cw[2 * 8 + o], v);
      v = __builtin_fmaxf(v, 0.f);
      if (STAGE == 2) v = __builtin_fmaf(v, cw[32 + o], cw[40 + o]);    // (contracted, as the forward launch's v * s + h is)
      b1v[q][o] = inside ? v : 0.f;
    }
  }
  if (STAGE == 1) {
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        const double d = (double)b1v[q + 1][o] - pv[o];
        s1[o] += d;
        s2[o] += d * d;
      }
    return;
  }
  // conv2 weight-stationary as in conv_positions: each (tap k, in-channel ci) row of 8 weights is fetched once; per output
  // the chain is the bias, then (k, ci) ascending
  const float* w2 = cw + 48;
  float acc[NP][8];
#pragma unroll
  for (int q = 0; q < NP; ++q)
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[q][o] = w2[192 + o];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int ci = 0; ci < 8; ++ci) {
      float wrow[8];
#pragma unroll
      for (int o = 0; o < 8; ++o) wrow[o] = w2[(k * 8 + ci) * 8 + o];
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const float av = b1v[q + k][ci];
#pragma unroll
        for (int o = 0; o < 8; ++o) acc[q][o] = __builtin_fmaf(av, wrow[o], acc[q][o]);
      }
    }
#pragma unroll
  for (int q = 0; q < NP; ++q)
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      const double d = (double)__builtin_fmaxf(acc[q][o], 0.f) - pv[o];
      s1[o] += d;
      s2[o] += d * d;
    }
}

struct BnConvArgs {
  SigArgs s;                             // the forward launch's own arguments: sig, rows, par, conv, T, M
  const float* pivot;                    // [8]
  double* part;                          // [workgroups][2][8]
};
// grid = ceil(M / (32 kBnTiles))
template <int STAGE>
__global__ void __launch_bounds__(256) bn_conv_moments_kernel(const BnConvArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float cwl[264];
  __shared__ double red[16][256];
  __shared__ double red2[16][16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  sig_conv_image(a.s, cwl, tid);
  __syncthreads();
  const int chunk = wave * 2 + (lane >> 5), r = lane & 31;
  const int p0 = chunk < 2 ? 7 * chunk : 14 + 6 * (chunk - 2);
  double pv[8], s1[8], s2[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) { pv[o] = (double)a.pivot[o]; s1[o] = 0.0; s2[o] = 0.0; }
#pragma clang loop unroll(disable)
  for (int tile = 0; tile < kBnTiles; ++tile) {
    asm volatile("" ::: "memory");                         // the 264 constants are read from LDS per tile, not hoisted into registers
    const int m = (blockIdx.x * kBnTiles + tile) * 32 + r;
    if (m >= a.s.M) continue;
    const float* srow = a.s.sig + ((size_t)a.s.rows[m / a.s.T] * a.s.T + m % a.s.T) * kSig;
    float x[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) {
      const int p = p0 - 2 + i;
      x[i] = (p >= 0 && p < kSig) ? srow[p] : 0.f;
    }
    if (wave == 0) bn_conv_samples<STAGE, 7>(cwl, x, p0, pv, s1, s2);
    else bn_conv_samples<STAGE, 6>(cwl, x, p0, pv, s1, s2);
  }
#pragma unroll
  for (int o = 0; o < 8; ++o) { red[o][tid] = s1[o]; red[8 + o][tid] = s2[o]; }
  __syncthreads();
  {
    const int q = tid >> 4, sub = tid & 15;
    double s = red[q][sub * 16];
    for (int j = 1; j < 16; ++j) s += red[q][sub * 16 + j];
    red2[q][sub] = s;
  }
  __syncthreads();
  if (tid < 16) {
    double s = red2[tid][0];
    for (int j = 1; j < 16; ++j) s += red2[tid][j];
    a.part[(size_t)blockIdx.x * 16 + tid] = s;
  }
}

struct BnReduceArgs {
  struct One {
    const double* part;                  // [n_part][2][C]
    int n_part, C, at;                   // at: the BatchNorm's first channel of the 432
    long long n;                         // elements per channel of the whole pass
  } bn[2];
  double* acc;                           // [2][kBnCh]: S1 | S2, running over the chunks
  float* blk;                            // the model's block: pivot read, mean / var written
  int cont, last;                        // not the pass's first chunk; its last
};
// grid = BatchNorms of the stage
__global__ void __launch_bounds__(256) bn_reduce_kernel(const BnReduceArgs a) {
#pragma clang fp contract(off)
  const BnReduceArgs::One& b = a.bn[blockIdx.x];
  const int c = threadIdx.x;
  if (c >= b.C) return;
  double s1 = a.cont ? a.acc[b.at + c] : 0.0, s2 = a.cont ? a.acc[kBnCh + b.at + c] : 0.0;
  for (int k = 0; k < b.n_part; ++k) {
    s1 += b.part[(size_t)k * 2 * b.C + c];
    s2 += b.part[(size_t)k * 2 * b.C + b.C + c];
  }
  a.acc[b.at + c] = s1;
  a.acc[kBnCh + b.at + c] = s2;
  if (!a.last) return;
  const double n = (double)b.n, m = s1 / n;
  const double mean = (double)a.blk[kBnPivot + b.at + c] + m;
  const double var = __builtin_fmax(s2 / n - m * m, 0.0);
  a.blk[kBnMean + b.at + c] = (float)mean;
  a.blk[kBnVar + b.at + c] = (float)var;
}

}  // namespace nrv
