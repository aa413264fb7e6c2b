// Fitting the last Bi-LSTM with the head on the device (depth NRV_FIT_LSTM4): the training set of BatchNorm'd lstm3 outputs,
// the forward and the backward pass of the 256->64 Bi-LSTM over a batch, and its weight gradients.
#pragma once
#include "nrv_headfit.h"   // head_grad_kernel<GRAD, true> runs the head on this depth's scratch and hands back dh1

namespace nrv {

// ---------------------------------------------------------------------------------------
// nanoreviser_amd/lstm4fit.py is the DEFINITION; include/nanorev.h (nrv_fit_*, "depth") states the rule.  Fitted are tensors
// 44 .. 59 and the centres.  One parameter vector per model, P = 164352 + NRV_FIT_PARAMS_HEAD:
//   [W4f [256][256] | U4f [64][256] | b4f [256] | W4b | U4b | b4b | the head's vector]     gate columns i, f, c, o
// THE SET (per model): xb [rows][T][256] f32 - the BatchNorm'd f32 lstm3 output of a labelled window, as the f32 lstm4 launch
// reads it - and y [rows] u8.  Behind each launch group
//   l4_gather_kernel   one thread per (window of the group, t, kq): 16 bytes from X3 [tile][t][kq 64][32 rows][4] to
//     xb[slot][t][kq * 4 ..].  Plain stores.  (The f32 lstm3 launch applies sc / sh in its epilogue, so X3 holds Xb already.)
// THE STEP of a batch of b rows, in CHUNKS of kL4ChunkTiles 32-row tiles in ascending order (the scratch is sized for one
// chunk); per chunk four launches, then two reduce launches and one Adam launch for the batch:
//   l4_forward_kernel   workgroup per (tile, direction), four waves; wave w owns gate w's 64 columns.  Per step
//     z = b + Xb_t W (k ascending, W read from L2) + h_{s-1} U (U resident in LDS), v_mfma_f32_32x32x2_f32; z through LDS to
//     one thread per (row, unit) for nrv_lstm_f32.h's gate functions; h to LDS and to X4 [rows][T][128], the activated gates
//     to GZ [rows][T][2][256] and c to CS [rows][T][2][64] (kept, not recomputed: 3.5 KB per row and step against a second
//     256-wide product per step).
//   head_grad_kernel<GRAD, true>   nrv_headfit.h's kernel on X4; it also stores dh1 [rows][T][128] and, from the second chunk
//     on, continues the partial vector of its workgroup - workgroup g sees the tiles g, g + 128, ... of the BATCH in ascending
//     order.  (dX4 = dh1 W1^T is NOT formed there: that kernel holds gW1 and gW2 in 128 accumulator registers and sits at the
//     256-register limit; a fifth product in it spilled 34 registers to scratch memory.)
//   l4_backward_kernel  workgroup per (tile, direction).  For s descending: dh = dh1_t W1^T (this direction's 64 rows of W1,
//     resident in LDS) + dz_{s+1} U^T (A = dz_{s+1} and B = U from LDS), one MFMA chain per wave, both k ranges split over
//     two wave pairs and the halves added in that order; the gate derivatives one thread per
//     (row, unit) with dc_{s+1} f_{s+1} carried in a register, dz to LDS and IN PLACE over GZ.
//   l4_wgrad_kernel     workgroup per (32 rows of [W | U | b], 64 columns, direction): gW = Xb^T dZ, gU = H_{s-1}^T dZ, gb =
//     1^T dZ on the MFMA pipe with k = (row, t) ascending, pair p of k values on wave p % 4; the four waves are added in
//     ascending order and the block is stored (first chunk) or added to what the chunks before left.  No partials.
//   head_reduce_kernel twice (the LSTM block as one "partial", the head's partials), head_adam_kernel once over all of P.
// No atomics, no workgroup waits for another: every sum's order is a function of (b, T) alone.
// ---------------------------------------------------------------------------------------
constexpr int kL4U = 256 * 256, kL4B = kL4U + 64 * 256, kL4Dir = kL4B + 256, kL4N = 2 * kL4Dir;      // 164352
constexpr int kL4ChunkTiles = kHeadFitMaxWg;
constexpr int kL4ChunkRows = 32 * kL4ChunkTiles;
static_assert(kL4N == 164352 && kL4N % 256 == 0, "the reduce launches of the two blocks share one flag array");

struct L4GatherArgs {
  const float* in[2];                    // X3 of the group [tile][t][kq 64][32 rows][4]
  float* x[2];                           // the set [cap][T][256]
  const int* slot;
  int n, T;
  long long cap;
};
// grid = (ceil(n * T * 64 / 256), 2 models)
__global__ void __launch_bounds__(256) l4_gather_kernel(const L4GatherArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int per = a.T * 64;
  if (g >= (long long)a.n * per) return;
  const int i = (int)(g / per), j = (int)(g % per), t = j >> 6, kq = j & 63;
  const long long s = a.slot[i];
  if (s < 0 || s >= a.cap) return;
  const f32x4 v = *(const f32x4*)(a.in[blockIdx.y] + ((size_t)(i >> 5) * a.T + t) * 8192 + kq * 128 + (i & 31) * 4);
  *(f32x4*)(a.x[blockIdx.y] + ((size_t)s * a.T + t) * 256 + kq * 4) = v;
}

struct L4Args {
  const float* xb;                       // the set's rows [.][T][256]
  const unsigned* rows;                  // [b] row indices of this chunk
  const float* par;                      // the vector: the LSTM block [kL4N], the head's behind it
  float* x4;                             // [chunk rows][T][128]
  float* gz;                             // [chunk rows][T][2][256]: activated gates i f g o, then dz in their place
  float* cs;                             // [chunk rows][T][2][64]
  const float* dh1;                      // [chunk rows][T][128]: the head's dh1 (dX4 = dh1 W1^T is formed by l4_backward_kernel)
  float* glstm;                          // [kL4N] gradient sums, not yet divided by b
  int T, b, keep, cont;                  // rows of this chunk; keep: GZ / CS are wanted; cont: not the batch's first chunk
};

constexpr int kL4Zs = 256 + 4, kL4Hs = 64 + 4, kL4Ws = 128 + 4;

// grid = (tiles of the chunk, 2 directions)
template <int ACT>
__global__ void __launch_bounds__(256) l4_forward_kernel(const L4Args a) {
  __shared__ __attribute__((aligned(16))) float ul[64 * 256];
  __shared__ __attribute__((aligned(16))) float zl[32 * kL4Zs];
  __shared__ __attribute__((aligned(16))) float hl[32 * kL4Hs];
  __shared__ long long rix[32];
  const int T = a.T, tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y, tile = blockIdx.x;
  const int n_here = a.b - tile * 32 < 32 ? a.b - tile * 32 : 32;
  const float* W = a.par + (size_t)dir * kL4Dir;
  const float* U = W + kL4U;
  const float* bias = W + kL4B;
  for (int i = tid; i < 64 * 64; i += 256) *(f32x4*)(ul + i * 4) = *(const f32x4*)(U + i * 4);
  for (int i = tid; i < 32 * kL4Hs; i += 256) hl[i] = 0.f;
  if (tid < 32) rix[tid] = tid < n_here ? (long long)a.rows[tile * 32 + tid] : -1;
  __syncthreads();
  const float* xrow = rix[l31] >= 0 ? a.xb + (size_t)rix[l31] * T * 256 : nullptr;
  const int col = wave * 64 + l31;                          // this lane's column of tile nt is col + 32 nt
  const float b0 = bias[col], b1 = bias[col + 32];
  float c[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) c[q] = 0.f;
  for (int s = 0; s < T; ++s) {
    const int t = dir ? T - 1 - s : s;
    f32x16 acc[2] = {splat16(b0), splat16(b1)};
#pragma unroll 2
    for (int kg = 0; kg < 32; ++kg) {
      f32x4 av = {0.f, 0.f, 0.f, 0.f};
      if (xrow) av = *(const f32x4*)(xrow + t * 256 + kg * 8 + half * 4);
      const float* wr = W + (kg * 8 + half * 4) * 256 + col;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[0] = mfma32(av[j], wr[j * 256], acc[0]);
        acc[1] = mfma32(av[j], wr[j * 256 + 32], acc[1]);
      }
    }
    if (s > 0) {
#pragma unroll 2
      for (int kg = 0; kg < 8; ++kg) {
        const f32x4 av = *(const f32x4*)(hl + l31 * kL4Hs + kg * 8 + half * 4);
        const float* ur = ul + (kg * 8 + half * 4) * 256 + col;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[0] = mfma32(av[j], ur[j * 256], acc[0]);
          acc[1] = mfma32(av[j], ur[j * 256 + 32], acc[1]);
        }
      }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) zl[acc_row(reg, lane) * kL4Zs + col + nt * 32] = acc[nt][reg];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = (tid >> 6) + 4 * q, u = lane;
      const float* zp = zl + r * kL4Zs + u;
      const float ig = gate_act<ACT>(zp[0]), fg = gate_act<ACT>(zp[64]), gg = tanh_fast(zp[128]), og = gate_act<ACT>(zp[192]);
      const float cn = __builtin_fmaf(fg, c[q], ig * gg);
      c[q] = cn;
      const float hv = og * tanh_fast(cn);
      hl[r * kL4Hs + u] = hv;
      if (r < n_here) {
        const size_t at = (size_t)(tile * 32 + r) * T + t;
        a.x4[at * 128 + dir * 64 + u] = hv;
        if (a.keep) {
          float* gp = a.gz + (at * 2 + dir) * 256 + u;
          gp[0] = ig; gp[64] = fg; gp[128] = gg; gp[192] = og;
          a.cs[(at * 2 + dir) * 64 + u] = cn;
        }
      }
    }
    __syncthreads();                                        // h_s before the next step reads it; zl is free again
  }
}

// act' decided on the forward VALUE
template <int ACT>
__device__ __forceinline__ float l4_act_d(float v) {
  if constexpr (ACT == 0) return (v > 0.f && v < 1.f) ? 0.2f : 0.f;
  else return v * (1.f - v);
}

// grid = (tiles of the chunk, 2 directions)
template <int ACT>
__global__ void __launch_bounds__(256) l4_backward_kernel(const L4Args a) {
  __shared__ __attribute__((aligned(16))) float ul[64 * kL4Zs];         // U [u][n]
  __shared__ __attribute__((aligned(16))) float dzl[32 * kL4Zs];        // dz of the step behind [row][n]
  __shared__ __attribute__((aligned(16))) float dhp[2 * 32 * 64];       // dh, the two halves of both k ranges
  __shared__ __attribute__((aligned(16))) float w1l[64 * kL4Ws];        // W1 [64 dir + k][n]: this direction's rows
  const int T = a.T, tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y, tile = blockIdx.x;
  const int n_here = a.b - tile * 32 < 32 ? a.b - tile * 32 : 32;
  const float* U = a.par + (size_t)dir * kL4Dir + kL4U;
  for (int i = tid; i < 64 * 64; i += 256) *(f32x4*)(ul + (i >> 6) * kL4Zs + (i & 63) * 4) = *(const f32x4*)(U + i * 4);
  const float* W1 = a.par + kL4N + kHfW1 + (size_t)dir * 64 * 128;
  for (int i = tid; i < 64 * 32; i += 256) *(f32x4*)(w1l + (i >> 5) * kL4Ws + (i & 31) * 4) = *(const f32x4*)(W1 + i * 4);
  float dcf[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) dcf[q] = 0.f;
  __syncthreads();
  const int nt = wave & 1, kh = wave >> 1;
  const float* drow = l31 < n_here ? a.dh1 + (size_t)(tile * 32 + l31) * T * 128 : nullptr;
  for (int s = T - 1; s >= 0; --s) {
    const int t = dir ? T - 1 - s : s;
    const bool rec = s < T - 1;
    {
      // dh[r][u] = sum_n dh1_t[r][n] W1[64 dir + u][n] + sum_n dz_{s+1}[r][n] U[u][n]: wave (nt, kh) takes 32 columns u and
      // the half kh of both k ranges
      f32x16 acc = splat16(0.f);
#pragma unroll 4
      for (int kg = kh * 8; kg < kh * 8 + 8; ++kg) {
        f32x4 av = {0.f, 0.f, 0.f, 0.f};
        if (drow) av = *(const f32x4*)(drow + t * 128 + kg * 8 + half * 4);
        const f32x4 bv = *(const f32x4*)(w1l + (nt * 32 + l31) * kL4Ws + kg * 8 + half * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = mfma32(av[j], bv[j], acc);
      }
      if (rec) {
#pragma unroll 4
        for (int kg = kh * 16; kg < kh * 16 + 16; ++kg) {
          const f32x4 av = *(const f32x4*)(dzl + l31 * kL4Zs + kg * 8 + half * 4);
          const f32x4 bv = *(const f32x4*)(ul + (nt * 32 + l31) * kL4Zs + kg * 8 + half * 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc = mfma32(av[j], bv[j], acc);
        }
      }
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) dhp[kh * 2048 + acc_row(reg, lane) * 64 + nt * 32 + l31] = acc[reg];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = (tid >> 6) + 4 * q, u = lane;
      float dzi = 0.f, dzf = 0.f, dzg = 0.f, dzo = 0.f;
      if (r < n_here) {
        const size_t lr = (size_t)(tile * 32 + r), at = lr * T + t;
        float* gp = a.gz + (at * 2 + dir) * 256 + u;
        const float ig = gp[0], fg = gp[64], gg = gp[128], og = gp[192];
        const float cn = a.cs[(at * 2 + dir) * 64 + u];
        const float cp = s > 0 ? a.cs[((lr * T + (dir ? t + 1 : t - 1)) * 2 + dir) * 64 + u] : 0.f;
        const float dh = dhp[r * 64 + u] + dhp[2048 + r * 64 + u];
        const float tc = tanh_fast(cn);
        const float dc = __builtin_fmaf(dh * og, 1.f - tc * tc, dcf[q]);
        dcf[q] = dc * fg;
        dzi = (dc * gg) * l4_act_d<ACT>(ig);
        dzf = (dc * cp) * l4_act_d<ACT>(fg);
        dzg = (dc * ig) * (1.f - gg * gg);
        dzo = (dh * tc) * l4_act_d<ACT>(og);
        gp[0] = dzi; gp[64] = dzf; gp[128] = dzg; gp[192] = dzo;
      }
      float* zp = dzl + r * kL4Zs + u;
      zp[0] = dzi; zp[64] = dzf; zp[128] = dzg; zp[192] = dzo;
    }
    __syncthreads();
  }
}

constexpr int kL4WgM = 11, kL4WgN = 4;                     // row blocks of [W 8 | U 2 | b 1], column blocks of 64
// grid = (kL4WgM * kL4WgN, 2 directions)
__global__ void __launch_bounds__(256) l4_wgrad_kernel(const L4Args a) {
  __shared__ unsigned rowl[kL4ChunkRows];
  __shared__ __attribute__((aligned(16))) float red[4 * 2048];
  const int T = a.T, tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y, mt = blockIdx.x / kL4WgN, ng = blockIdx.x % kL4WgN;
  const int nrow = a.b < kL4ChunkRows ? a.b : kL4ChunkRows;
  for (int i = tid; i < nrow; i += 256) rowl[i] = a.rows[i];
  __syncthreads();
  const int K = nrow * T, npair = (K + 1) / 2;              // at most 2^17
  f32x16 acc[2] = {splat16(0.f), splat16(0.f)};
  for (int p0 = wave; p0 < npair; p0 += 16) {              // four pairs at a time: their loads are in flight together
    float av[4], bv0[4], bv1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kk = 2 * (p0 + 4 * i) + half;
      av[i] = 0.f; bv0[i] = 0.f; bv1[i] = 0.f;
      if (kk < K) {
        const int lr = kk / T, t = kk - lr * T;
        const float* zp = a.gz + ((size_t)kk * 2 + dir) * 256 + ng * 64 + l31;
        bv0[i] = zp[0]; bv1[i] = zp[32];
        if (mt < 8) av[i] = a.xb[((size_t)rowl[lr] * T + t) * 256 + mt * 32 + l31];
        else if (mt < 10) {
          const int tp = dir ? t + 1 : t - 1;               // the step before in this direction's order
          if (tp >= 0 && tp < T) av[i] = a.x4[((size_t)lr * T + tp) * 128 + dir * 64 + (mt - 8) * 32 + l31];
        } else av[i] = l31 == 0 ? 1.f : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[0] = mfma32(av[i], bv0[i], acc[0]);
      acc[1] = mfma32(av[i], bv1[i], acc[1]);
    }
  }
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) red[wave * 2048 + acc_row(reg, lane) * 64 + nt * 32 + l31] = acc[nt][reg];
  __syncthreads();
  float* out = a.glstm + (size_t)dir * kL4Dir;
  for (int i = tid; i < 2048; i += 256) {
    const int m = i >> 6, n = ng * 64 + (i & 63);
    float s = 0.f;
    for (int w = 0; w < 4; ++w) s += red[w * 2048 + i];
    float* o;
    if (mt < 8) o = out + (mt * 32 + m) * 256 + n;
    else if (mt < 10) o = out + kL4U + ((mt - 8) * 32 + m) * 256 + n;
    else { if (m != 0) continue; o = out + kL4B + n; }
    *o = a.cont ? *o + s : s;
  }
}

}  // namespace nrv
