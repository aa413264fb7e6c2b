// Fitting the 192->128 Bi-LSTM with everything behind it on the device (depth NRV_FIT_LSTM3): the training set of lstm3 inputs,
// the forward and the backward pass of that Bi-LSTM over a batch, the data gradient out of lstm4, and lstm3's weight gradients.
#pragma once
#include "nrv_lstm4fit.h"  // its four launches run unchanged on this depth's scratch Xb4
#include "nrv_bnaffine.h"  // the variant of l4_dx_kernel that also leaves bn_l3's two sums

namespace nrv {

// ---------------------------------------------------------------------------------------
// nanoreviser_amd/lstm3fit.py is the DEFINITION; include/nanorev.h (nrv_fit_*, "depth") states the rule.  Fitted are tensors
// 34 .. 39, 44 .. 59 and the centres; the BatchNorm between the two LSTMs (tensors 40 .. 43) is FROZEN and applied in its
// inference form.  One parameter vector per model, P = 328704 + NRV_FIT_PARAMS_LSTM4:
//   [W3f [192][512] | U3f [128][512] | b3f [512] | W3b | U3b | b3b | the lstm4 depth's vector]     gate columns i, f, c, o
// THE SET (per model): xin [rows][T][192] f32 - the BatchNorm'd f32 lstm2 output (128), then signal_x_out (64), as the f32 lstm3
// launch reads them - and y [rows] u8.  Inside each launch group, behind the lstm2 launch and in front of the lstm4 launch
// (whose output overwrites lstm2's):
//   l3_gather_kernel   one thread per (window of the group, t, kq of 48): 16 bytes through the ActView the lstm3 launch reads
//     (kq < 32: lstm2's output, window-major; else the signal branch's, event-major in the raw-read path) to
//     xin[slot][t][kq * 4 ..].  Plain stores.
// THE STEP of a batch of b rows, in the lstm4 depth's CHUNKS of kL4ChunkRows rows; per chunk
//   l3_forward_kernel   workgroup per (tile, direction), four waves; wave w owns gate w's 128 columns.  Per step
//     z = b + Xin_t W (k ascending) + h_{s-1} U, v_mfma_f32_32x32x2_f32, W AND U read from L2: U is 256 KB in f32 and does not
//     fit in LDS; all workgroups of a direction read the same 640 KB, which stay in L2.  z through LDS to one thread per
//     (row, unit) for nrv_lstm_f32.h's gate functions; raw h to LDS and to H3 [rows][T][256], Xb4 = h * sc + sh (one multiply,
//     one add) to XB [rows][T][256], the activated gates to GZ [rows][T][2][512] and c to CS [rows][T][2][128].
//   the lstm4 depth's four launches on XB with an identity row list (the head reads its labels through the batch's own list).
//   l4_dx_kernel        workgroup per 32 (row, t) pairs: dX3 = (dz4_fw W4f^T + dz4_bw W4b^T) * sc, k ascending, forward
//     direction first; dz4 is what l4_backward_kernel left in place of lstm4's gates.
//   l3_backward_kernel  workgroup per (tile, direction).  For s descending: dh = dX3_t[this direction's half] + dz_{s+1} U^T
//     (A = dz_{s+1} from LDS, B = U from L2, wave w the units 32 w ..), the gate derivatives one thread per (row, unit) with
//     dc_{s+1} f_{s+1} carried in a register, dz to LDS and IN PLACE over GZ.
//   l3_wgrad_kernel     workgroup per (32 rows of [W | U | b], 64 columns, direction): gW = Xin^T dZ, gU = H3_{s-1}^T dZ, gb =
//     1^T dZ with k = (row, t) ascending, pair p of k values on wave p % 4; the four waves are added in ascending order and
//     the block is stored (first chunk) or added to what the chunks before left.  No partials.
//   head_reduce_kernel three times (the lstm3 block and the lstm4 block as one "partial" each, the head's partials),
//   head_adam_kernel once over all of P.
// No atomics, no workgroup waits for another: every sum's order is a function of (b, T) alone.
// ---------------------------------------------------------------------------------------
constexpr int kL3U = 192 * 512, kL3B = kL3U + 128 * 512, kL3Dir = kL3B + 512, kL3N = 2 * kL3Dir;     // 328704
static_assert(kL3N == 328704 && kL3N % 256 == 0, "the reduce launches of the three blocks share one flag array");

struct L3GatherArgs {
  ActView in0[2], in1[2];                // the lstm3 launch's two inputs: lstm2's output (KQ 32), the signal branch's (KQ 16)
  float* x[2];                           // the set [cap][T][192]
  const int* slot;
  int n, T;
  long long cap;
};
// grid = (ceil(n * T * 48 / 256), 2 models)
__global__ void __launch_bounds__(256) l3_gather_kernel(const L3GatherArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int per = a.T * 48;
  if (g >= (long long)a.n * per) return;
  const int i = (int)(g / per), j = (int)(g % per), t = j / 48, kq = j % 48;
  const long long s = a.slot[i];
  if (s < 0 || s >= a.cap) return;
  const int m = blockIdx.y;
  const f32x4 v = *(const f32x4*)(kq < 32 ? a.in0[m].chunk(i, t, kq) : a.in1[m].chunk(i, t, kq - 32));
  *(f32x4*)(a.x[m] + ((size_t)s * a.T + t) * 192 + kq * 4) = v;
}

struct L3Args {
  const float* xin;                      // the set's rows [.][T][192]
  const unsigned* rows;                  // [b] row indices of this chunk
  const float* par;                      // the vector: the lstm3 block [kL3N] in front
  const float* sc;                       // [256] the frozen BatchNorm behind lstm3: Xb4 = h sc + sh
  const float* sh;
  float* h3;                             // [chunk rows][T][256] raw h
  float* xb4;                            // [chunk rows][T][256]
  float* gz;                             // [chunk rows][T][2][512]: activated gates i f g o, then dz in their place
  float* cs;                             // [chunk rows][T][2][128]
  float* dx3;                            // [chunk rows][T][256]
  const float* gz4;                      // lstm4's [chunk rows][T][2][256] holding dz4 (l4_dx_kernel)
  float* glstm;                          // [kL3N] gradient sums, not yet divided by b
  int T, b, keep, cont;                  // rows of this chunk; keep: GZ / CS are wanted; cont: not the batch's first chunk
};

constexpr int kL3Zs = 512 + 4, kL3Hs = 128 + 4;

// grid = (tiles of the chunk, 2 directions)
template <int ACT>
__global__ void __launch_bounds__(256) l3_forward_kernel(const L3Args a) {
  __shared__ __attribute__((aligned(16))) float zl[32 * kL3Zs];
  __shared__ __attribute__((aligned(16))) float hl[32 * kL3Hs];
  __shared__ long long rix[32];
  const int T = a.T, tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y, tile = blockIdx.x;
  const int n_here = a.b - tile * 32 < 32 ? a.b - tile * 32 : 32;
  const float* W = a.par + (size_t)dir * kL3Dir;
  const float* U = W + kL3U;
  const float* bias = W + kL3B;
  for (int i = tid; i < 32 * kL3Hs; i += 256) hl[i] = 0.f;
  if (tid < 32) rix[tid] = tid < n_here ? (long long)a.rows[tile * 32 + tid] : -1;
  __syncthreads();
  const float* xrow = rix[l31] >= 0 ? a.xin + (size_t)rix[l31] * T * 192 : nullptr;
  const int col = wave * 128 + l31;                         // this lane's column of tile nt is col + 32 nt
  float bs[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) bs[nt] = bias[col + nt * 32];
  const int u = tid & 127;
  const float scu = a.sc[dir * 128 + u], shu = a.sh[dir * 128 + u];
  float c[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) c[q] = 0.f;
  for (int s = 0; s < T; ++s) {
    const int t = dir ? T - 1 - s : s;
    f32x16 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = splat16(bs[nt]);
#pragma unroll 2
    for (int kg = 0; kg < 24; ++kg) {
      f32x4 av = {0.f, 0.f, 0.f, 0.f};
      if (xrow) av = *(const f32x4*)(xrow + t * 192 + kg * 8 + half * 4);
      const float* wr = W + (kg * 8 + half * 4) * 512 + col;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = mfma32(av[j], wr[j * 512 + nt * 32], acc[nt]);
    }
    if (s > 0) {
#pragma unroll 2
      for (int kg = 0; kg < 16; ++kg) {
        const f32x4 av = *(const f32x4*)(hl + l31 * kL3Hs + kg * 8 + half * 4);
        const float* ur = U + (kg * 8 + half * 4) * 512 + col;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) acc[nt] = mfma32(av[j], ur[j * 512 + nt * 32], acc[nt]);
      }
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) zl[acc_row(reg, lane) * kL3Zs + col + nt * 32] = acc[nt][reg];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = (tid >> 7) + 2 * q;
      const float* zp = zl + r * kL3Zs + u;
      const float ig = gate_act<ACT>(zp[0]), fg = gate_act<ACT>(zp[128]), gg = tanh_fast(zp[256]), og = gate_act<ACT>(zp[384]);
      const float cn = __builtin_fmaf(fg, c[q], ig * gg);
      c[q] = cn;
      const float hv = og * tanh_fast(cn);
      hl[r * kL3Hs + u] = hv;
      if (r < n_here) {
        const size_t at = (size_t)(tile * 32 + r) * T + t;
        a.h3[at * 256 + dir * 128 + u] = hv;
        a.xb4[at * 256 + dir * 128 + u] = __fadd_rn(__fmul_rn(hv, scu), shu);
        if (a.keep) {
          float* gp = a.gz + (at * 2 + dir) * 512 + u;
          gp[0] = ig; gp[128] = fg; gp[256] = gg; gp[384] = og;
          a.cs[(at * 2 + dir) * 128 + u] = cn;
        }
      }
    }
    __syncthreads();                                        // h_s before the next step reads it; zl is free again
  }
}

struct L4DxArgs {
  const float* gz4;                      // [M][2][256] dz4
  const float* par4;                     // the lstm4 block [kL4N]
  const float* sc;                       // [256]
  float* dx3;                            // [M][256]
  int M;                                 // chunk rows x T
};
struct L4DxBnArgs : L4DxArgs { BnAffArgs bn; };             // nrv_fit_set_bn_affine: acc is bn_l3's dy before the scale
// grid = ceil(M / 32); wave w owns the 64 output columns 64 w ..  A = L4DxBnArgs also leaves bn_l3's two sums (nrv_bnaffine.h)
template <class A = L4DxArgs>
__global__ void __launch_bounds__(256) l4_dx_kernel(const A a) {
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * 32;
  const bool live = m0 + l31 < a.M;
  f32x16 acc[2] = {splat16(0.f), splat16(0.f)};
  for (int dir = 0; dir < 2; ++dir) {
    const float* arow = a.gz4 + ((size_t)(m0 + l31) * 2 + dir) * 256;
    const float* W = a.par4 + (size_t)dir * kL4Dir;         // [256 in][256 gate columns]: B[k][n] = W[n][k]
    const float* w0 = W + (size_t)(wave * 64 + l31) * 256;
#pragma unroll 4
    for (int kg = 0; kg < 32; ++kg) {
      f32x4 av = {0.f, 0.f, 0.f, 0.f};
      if (live) av = *(const f32x4*)(arow + kg * 8 + half * 4);
      const f32x4 b0 = *(const f32x4*)(w0 + kg * 8 + half * 4);
      const f32x4 b1 = *(const f32x4*)(w0 + 32 * 256 + kg * 8 + half * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[0] = mfma32(av[j], b0[j], acc[0]);
        acc[1] = mfma32(av[j], b1[j], acc[1]);
      }
    }
  }
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int n = wave * 64 + nt * 32 + l31;
    const float scn = a.sc[n];
    if constexpr (std::is_same_v<A, L4DxBnArgs>) bn_dy_partial<256>(a.bn, acc[nt], lane, m0, a.M, n);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int m = m0 + acc_row(reg, lane);
      if (m < a.M) a.dx3[(size_t)m * 256 + n] = acc[nt][reg] * scn;
    }
  }
}

// grid = (tiles of the chunk, 2 directions)
template <int ACT>
__global__ void __launch_bounds__(256) l3_backward_kernel(const L3Args a) {
  __shared__ __attribute__((aligned(16))) float dzl[32 * kL3Zs];        // dz of the step behind [row][n]
  __shared__ __attribute__((aligned(16))) float dhl[32 * kL3Hs];        // dz_{s+1} U^T [row][u]
  const int T = a.T, tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y, tile = blockIdx.x;
  const int n_here = a.b - tile * 32 < 32 ? a.b - tile * 32 : 32;
  const float* U = a.par + (size_t)dir * kL3Dir + kL3U;    // [128 u][512 n]: B[k = n][u] = U[u][n]
  const float* u0 = U + (size_t)(wave * 32 + l31) * 512;
  const int u = tid & 127;
  float dcf[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) dcf[q] = 0.f;
  for (int s = T - 1; s >= 0; --s) {
    const int t = dir ? T - 1 - s : s;
    if (s < T - 1) {
      f32x16 acc = splat16(0.f);
#pragma unroll 4
      for (int kg = 0; kg < 64; ++kg) {
        const f32x4 av = *(const f32x4*)(dzl + l31 * kL3Zs + kg * 8 + half * 4);
        const f32x4 bv = *(const f32x4*)(u0 + kg * 8 + half * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = mfma32(av[j], bv[j], acc);
      }
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) dhl[acc_row(reg, lane) * kL3Hs + wave * 32 + l31] = acc[reg];
    }
    __syncthreads();                                        // dhl is whole; every wave is done reading dzl
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = (tid >> 7) + 2 * q;
      float dzi = 0.f, dzf = 0.f, dzg = 0.f, dzo = 0.f;
      if (r < n_here) {
        const size_t lr = (size_t)(tile * 32 + r), at = lr * T + t;
        float* gp = a.gz + (at * 2 + dir) * 512 + u;
        const float ig = gp[0], fg = gp[128], gg = gp[256], og = gp[384];
        const float cn = a.cs[(at * 2 + dir) * 128 + u];
        const float cp = s > 0 ? a.cs[((lr * T + (dir ? t + 1 : t - 1)) * 2 + dir) * 128 + u] : 0.f;
        float dh = a.dx3[at * 256 + dir * 128 + u];
        if (s < T - 1) dh += dhl[r * kL3Hs + u];
        const float tc = tanh_fast(cn);
        const float dc = __builtin_fmaf(dh * og, 1.f - tc * tc, dcf[q]);
        dcf[q] = dc * fg;
        dzi = (dc * gg) * l4_act_d<ACT>(ig);
        dzf = (dc * cp) * l4_act_d<ACT>(fg);
        dzg = (dc * ig) * (1.f - gg * gg);
        dzo = (dh * tc) * l4_act_d<ACT>(og);
        gp[0] = dzi; gp[128] = dzf; gp[256] = dzg; gp[384] = dzo;
      }
      float* zp = dzl + r * kL3Zs + u;
      zp[0] = dzi; zp[128] = dzf; zp[256] = dzg; zp[384] = dzo;
    }
    __syncthreads();
  }
}

constexpr int kL3WgM = 11, kL3WgN = 8;                     // row blocks of [W 6 | U 4 | b 1], column blocks of 64
// grid = (kL3WgM * kL3WgN, 2 directions)
__global__ void __launch_bounds__(256) l3_wgrad_kernel(const L3Args a) {
  __shared__ unsigned rowl[kL4ChunkRows];
  __shared__ __attribute__((aligned(16))) float red[4 * 2048];
  const int T = a.T, tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y, mt = blockIdx.x / kL3WgN, ng = blockIdx.x % kL3WgN;
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
        const float* zp = a.gz + ((size_t)kk * 2 + dir) * 512 + ng * 64 + l31;
        bv0[i] = zp[0]; bv1[i] = zp[32];
        if (mt < 6) av[i] = a.xin[((size_t)rowl[lr] * T + t) * 192 + mt * 32 + l31];
        else if (mt < 10) {
          const int tp = dir ? t + 1 : t - 1;               // the step before in this direction's order
          if (tp >= 0 && tp < T) av[i] = a.h3[((size_t)lr * T + tp) * 256 + dir * 128 + (mt - 6) * 32 + l31];
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
  float* out = a.glstm + (size_t)dir * kL3Dir;
  for (int i = tid; i < 2048; i += 256) {
    const int m = i >> 6, n = ng * 64 + (i & 63);
    float s = 0.f;
    for (int w = 0; w < 4; ++w) s += red[w * 2048 + i];
    float* o;
    if (mt < 6) o = out + (mt * 32 + m) * 512 + n;
    else if (mt < 10) o = out + kL3U + ((mt - 6) * 32 + m) * 512 + n;
    else { if (m != 0) continue; o = out + kL3B + n; }
    *o = a.cont ? *o + s : s;
  }
}

}  // namespace nrv
