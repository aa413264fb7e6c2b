// Fitting the read branch too - the whole model - on the device (depth NRV_FIT_FULL): the training set of raw windows, the forward
// and the backward pass of lstm1 (6 -> 16) and lstm2 (32 -> 64) over a batch, their weight gradients, and the data gradient out
// of lstm2.
#pragma once
#include "nrv_signalfit.h"  // its launches run unchanged on this depth's scratch Xin

namespace nrv {

// ---------------------------------------------------------------------------------------
// nanoreviser_amd/fullfit.py is the DEFINITION; include/nanorev.h (nrv_fit_*, "depth") states the rule.  Fitted is every tensor
// that is no BatchNorm's; the five BatchNorms are FROZEN and applied in their inference form, and the reference's Dropout is not
// applied.  One vector per model, P = 52608 + NRV_FIT_PARAMS_SIGNAL:
//   [W1f [6][64] | U1f [16][64] | b1f [64] | W1b | U1b | b1b | W2f [32][256] | U2f [64][256] | b2f [256] | W2b | U2b | b2b |
//    the signal depth's vector]                                                                        gate columns i, f, c, o
// THE SET: ONE sig [rows][T][50] f32 and ONE feat [rows][T][6] f32 for both models (they read the same inputs), y [rows] u8 per
// model.  Nothing of the set depends on the network, so no launch group runs for it:
//   full_gather_kernel  one thread per (window of the stage, t, q of 28): q < 25 is 8 bytes of the stage's event-major samples,
//     q >= 25 is 8 bytes of its event-major features (window w, step t is event w + t).  Plain stores.
// THE STEP of a batch of b rows, in the lstm4 depth's CHUNKS; M = chunk rows x T (row, t) pairs.  The two layers run ONE family
// of launches, rl_*<DX, H>, lstm3fit's launches with the widths as template arguments; per chunk
//   rl_forward_kernel<6, 16>   workgroup per (32 rows, direction), two waves, wave w the gate columns 32 w ..; reads feat through
//     the batch's row list; writes raw h to H1, X1b = h s_l1 + h_l1, keeps the gates and c.
//   rl_forward_kernel<32, 64>  four waves, wave w the gate columns 64 w ..; reads X1b; writes raw h to H2 and X2b = h s_l2 + h_l2
//     straight into columns 0 .. 127 of the scratch Xin.
//     Both: z = b + x_t W (k ascending) + h_{s-1} U on v_mfma_f32_32x32x2_f32, W and U read from the vector (L2), z through LDS to
//     one thread per (row, unit).
//   sig_forward_kernel<false>  writes columns 128 .. 191 of Xin only; sig through the batch's row list, Xin by position.
//   the signal depth's launches on Xin, unchanged; l3_dx_kernel<true> forms all 192 columns of dXin: dH2 = dXin[.., :128] s_l2
//     and dS.
//   rl_backward_kernel<32, 64>, rl_dx_kernel (dH1 = (sum over the directions of dz2 W2^T) s_l1), rl_backward_kernel<6, 16>:
//     lstm3fit's rule, dz in place of the gates.
//   rl_wgrad_kernel<DX, H>     workgroup per (32 rows of [W | U | b], 64 columns, direction, slice of kRdSlices): the slice's
//     (row, t) pairs ascending, pair p on wave p % 4, the four waves added in ascending order into the slice's own partial,
//     stored (first chunk) or added to (later chunks).
//   head_reduce_kernel once more over the kRdSlices partials with a flag range of its own (52608 is no multiple of 256), the ONE
//   head_adam_kernel over all of P.
// No atomics, no workgroup waits for another: every sum's order is a function of (b, T) alone.
// ---------------------------------------------------------------------------------------
constexpr int kR1Dir = (6 + 16 + 1) * 64, kR1N = 2 * kR1Dir, kR2Dir = (32 + 64 + 1) * 256, kR2N = 2 * kR2Dir, kRdN = kR1N + kR2N;
static_assert(kR1N == 2944 && kR2N == 49664 && kRdN == 52608 && kRdN % 4 == 0, "the read block of the vector");
constexpr int kRdSlices = 8;                               // partials of the read block's weight gradients
constexpr int kRdPair = 32 + 32 + 128, kRdPairGrad = kRdPair + 128 + 32 + 32 + 128 + 128 + 512;     // scratch floats per (row, t)

struct FullGatherArgs {
  const float* sig_ev;                   // the stage's samples [events][50]
  const float* feat_ev;                  // the stage's features [events][6]
  float* sig;                            // the set [cap][T][50]
  float* feat;                           // the set [cap][T][6]
  const int* slot;
  int n, T;
  long long cap;
};
// grid = ceil(n * T * 28 / 256)
__global__ void __launch_bounds__(256) full_gather_kernel(const FullGatherArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int per = a.T * 28;
  if (g >= (long long)a.n * per) return;
  const int i = (int)(g / per), j = (int)(g % per), t = j / 28, q = j % 28;
  const long long s = a.slot[i];
  if (s < 0 || s >= a.cap) return;
  if (q < 25) *(f32x2*)(a.sig + ((size_t)s * a.T + t) * kSig + q * 2) = *(const f32x2*)(a.sig_ev + (size_t)(i + t) * kSig + q * 2);
  else *(f32x2*)(a.feat + ((size_t)s * a.T + t) * kFeat + (q - 25) * 2) = *(const f32x2*)(a.feat_ev + (size_t)(i + t) * kFeat + (q - 25) * 2);
}

struct RlArgs {
  const float* x;                        // the layer's input rows [.][T][DX]
  const unsigned* rows;                  // row indices of this chunk into x
  const float* par;                      // the layer's block of the vector: per direction [W [DX][4H] | U [H][4H] | b [4H]]
  const float* sc;                       // [2H] the frozen BatchNorm behind the layer: xb = h sc + sh
  const float* sh;
  float* h;                              // [M][2H] raw h
  float* xb;                             // [M][ldxb]: columns 0 .. 2H - 1 are written
  float* gz;                             // [M][2][4H]: activated gates i f g o, then dz in their place
  float* cs;                             // [M][2][H]
  const float* dh;                       // [M][2H] the derivative by the raw h from the layer behind
  float* gsum;                           // [kRdSlices][kRdN] partial sums at this layer's offset, not yet divided by b
  int ldxb, T, b, keep, cont;            // rows of this chunk; keep: gz / cs are wanted; cont: not the batch's first chunk
};

template <int H> struct RlShape {
  static constexpr int G = 4 * H, NW = H >= 64 ? 4 : 2, NTH = NW * 64, NTL = G / NW / 32, Zs = G + 4, Hs = H + 4, RP = NTH / H, Q = 32 / RP;
  static_assert(NTL * NW * 32 == G && RP * Q == 32, "a wave owns whole column tiles; the gate threads cover the 32 rows");
};

// grid = (tiles of the chunk, 2 directions)
template <int DX, int H, int ACT>
__global__ void __launch_bounds__(RlShape<H>::NTH) rl_forward_kernel(const RlArgs a) {
  using S = RlShape<H>;
  constexpr int G = S::G, NTH = S::NTH, NTL = S::NTL, Zs = S::Zs, Hs = S::Hs, RP = S::RP, Q = S::Q;
  __shared__ __attribute__((aligned(16))) float zl[32 * Zs];
  __shared__ __attribute__((aligned(16))) float hl[32 * Hs];
  __shared__ long long rix[32];
  const int T = a.T, tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y, tile = blockIdx.x;
  const int n_here = a.b - tile * 32 < 32 ? a.b - tile * 32 : 32;
  const float* W = a.par + (size_t)dir * (DX + H + 1) * G;
  const float* U = W + DX * G;
  const float* bias = U + H * G;
  for (int i = tid; i < 32 * Hs; i += NTH) hl[i] = 0.f;
  if (tid < 32) rix[tid] = tid < n_here ? (long long)a.rows[tile * 32 + tid] : -1;
  __syncthreads();
  const float* xrow = rix[l31] >= 0 ? a.x + (size_t)rix[l31] * T * DX : nullptr;
  const int col = wave * (G / S::NW) + l31;                 // this lane's column of tile nt is col + 32 nt
  float bs[NTL];
#pragma unroll
  for (int nt = 0; nt < NTL; ++nt) bs[nt] = bias[col + nt * 32];
  const int u = tid % H, r0 = tid / H;
  const float scu = a.sc[dir * H + u], shu = a.sh[dir * H + u];
  float c[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) c[q] = 0.f;
  for (int s = 0; s < T; ++s) {
    const int t = dir ? T - 1 - s : s;
    f32x16 acc[NTL];
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt) acc[nt] = splat16(bs[nt]);
#pragma unroll
    for (int kg = 0; kg < (DX + 7) / 8; ++kg) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = kg * 8 + half * 4 + j;                // (DX = 6: the two k past the input are zero on both sides)
        const bool in = k < DX;
        const float av = (xrow && in) ? xrow[t * DX + k] : 0.f;
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) acc[nt] = mfma32(av, in ? W[k * G + col + nt * 32] : 0.f, acc[nt]);
      }
    }
    if (s > 0) {
#pragma unroll 2
      for (int kg = 0; kg < H / 8; ++kg) {
        const f32x4 av = *(const f32x4*)(hl + l31 * Hs + kg * 8 + half * 4);
        const float* ur = U + (kg * 8 + half * 4) * G + col;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int nt = 0; nt < NTL; ++nt) acc[nt] = mfma32(av[j], ur[j * G + nt * 32], acc[nt]);
      }
    }
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) zl[acc_row(reg, lane) * Zs + col + nt * 32] = acc[nt][reg];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int r = r0 + RP * q;
      const float* zp = zl + r * Zs + u;
      const float ig = gate_act<ACT>(zp[0]), fg = gate_act<ACT>(zp[H]), gg = tanh_fast(zp[2 * H]), og = gate_act<ACT>(zp[3 * H]);
      const float cn = __builtin_fmaf(fg, c[q], ig * gg);
      c[q] = cn;
      const float hv = og * tanh_fast(cn);
      hl[r * Hs + u] = hv;
      if (r < n_here) {
        const size_t at = (size_t)(tile * 32 + r) * T + t;
        a.h[at * (2 * H) + dir * H + u] = hv;
        a.xb[at * a.ldxb + dir * H + u] = __fadd_rn(__fmul_rn(hv, scu), shu);
        if (a.keep) {
          float* gp = a.gz + (at * 2 + dir) * G + u;
          gp[0] = ig; gp[H] = fg; gp[2 * H] = gg; gp[3 * H] = og;
          a.cs[(at * 2 + dir) * H + u] = cn;
        }
      }
    }
    __syncthreads();                                        // h_s before the next step reads it; zl is free again
  }
}

// grid = (tiles of the chunk, 2 directions)
template <int DX, int H, int ACT>
__global__ void __launch_bounds__(RlShape<H>::NTH) rl_backward_kernel(const RlArgs a) {
  using S = RlShape<H>;
  constexpr int G = S::G, Zs = S::Zs, Hs = S::Hs, RP = S::RP, Q = S::Q, NWM = (H + 31) / 32;
  __shared__ __attribute__((aligned(16))) float dzl[32 * Zs];          // dz of the step behind [row][n]
  __shared__ __attribute__((aligned(16))) float dhl[32 * Hs];          // dz_{s+1} U^T [row][u]
  const int T = a.T, tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y, tile = blockIdx.x;
  const int n_here = a.b - tile * 32 < 32 ? a.b - tile * 32 : 32;
  const float* U = a.par + (size_t)dir * (DX + H + 1) * G + DX * G;     // [H u][4H n]: B[k = n][u] = U[u][n]
  const int un = wave * 32 + l31;                           // the unit this lane's B column and accumulator column are
  const float* u0 = U + (size_t)(un < H ? un : 0) * G;
  const int u = tid % H, r0 = tid / H;
  float dcf[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) dcf[q] = 0.f;
  for (int s = T - 1; s >= 0; --s) {
    const int t = dir ? T - 1 - s : s;
    if (s < T - 1 && wave < NWM) {
      f32x16 acc = splat16(0.f);
#pragma unroll 4
      for (int kg = 0; kg < G / 8; ++kg) {
        const f32x4 av = *(const f32x4*)(dzl + l31 * Zs + kg * 8 + half * 4);
        f32x4 bv = *(const f32x4*)(u0 + kg * 8 + half * 4);
        if (un >= H) bv = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = mfma32(av[j], bv[j], acc);
      }
      if (un < H)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) dhl[acc_row(reg, lane) * Hs + un] = acc[reg];
    }
    __syncthreads();                                        // dhl is whole; every wave is done reading dzl
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int r = r0 + RP * q;
      float dzi = 0.f, dzf = 0.f, dzg = 0.f, dzo = 0.f;
      if (r < n_here) {
        const size_t lr = (size_t)(tile * 32 + r), at = lr * T + t;
        float* gp = a.gz + (at * 2 + dir) * G + u;
        const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
        const float cn = a.cs[(at * 2 + dir) * H + u];
        const float cp = s > 0 ? a.cs[((lr * T + (dir ? t + 1 : t - 1)) * 2 + dir) * H + u] : 0.f;
        float dh = a.dh[at * (2 * H) + dir * H + u];
        if (s < T - 1) dh += dhl[r * Hs + u];
        const float tc = tanh_fast(cn);
        const float dc = __builtin_fmaf(dh * og, 1.f - tc * tc, dcf[q]);
        dcf[q] = dc * fg;
        dzi = (dc * gg) * l4_act_d<ACT>(ig);
        dzf = (dc * cp) * l4_act_d<ACT>(fg);
        dzg = (dc * ig) * (1.f - gg * gg);
        dzo = (dh * tc) * l4_act_d<ACT>(og);
        gp[0] = dzi; gp[H] = dzf; gp[2 * H] = dzg; gp[3 * H] = dzo;
      }
      float* zp = dzl + r * Zs + u;
      zp[0] = dzi; zp[H] = dzf; zp[2 * H] = dzg; zp[3 * H] = dzo;
    }
    __syncthreads();
  }
}

struct RlDxArgs {
  const float* gz;                       // [M][2][4H] dz
  const float* par;                      // the layer's block
  const float* sc;                       // [DX] the frozen BatchNorm in front of the layer
  float* dx;                             // [M][DX]
  int M;                                 // chunk rows x T
};
// grid = ceil(M / 32), one wave per 32 input columns: dx = (dz_fw W_f^T + dz_bw W_b^T) sc, k ascending, forward direction first
struct RlDxBnArgs : RlDxArgs { BnAffArgs bn; };             // nrv_fit_set_bn_affine: acc is dy of the BatchNorm in front of the layer
// A = RlDxBnArgs also leaves that BatchNorm's two sums (nrv_bnaffine.h)
template <int DX, int H, class A = RlDxArgs>
__global__ void __launch_bounds__(DX * 2) rl_dx_kernel(const A a) {
  static_assert(DX % 32 == 0, "whole column tiles");
  constexpr int G = 4 * H;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * 32, n = wave * 32 + l31;
  const bool live = m0 + l31 < a.M;
  f32x16 acc = splat16(0.f);
  for (int dir = 0; dir < 2; ++dir) {
    const float* arow = a.gz + ((size_t)(m0 + l31) * 2 + dir) * G;
    const float* w0 = a.par + (size_t)dir * (DX + H + 1) * G + (size_t)n * G;        // W [DX in][4H]: B[k][n] = W[n][k]
#pragma unroll 4
    for (int kg = 0; kg < G / 8; ++kg) {
      f32x4 av = {0.f, 0.f, 0.f, 0.f};
      if (live) av = *(const f32x4*)(arow + kg * 8 + half * 4);
      const f32x4 bv = *(const f32x4*)(w0 + kg * 8 + half * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = mfma32(av[j], bv[j], acc);
    }
  }
  const float scn = a.sc[n];
  if constexpr (std::is_same_v<A, RlDxBnArgs>) bn_dy_partial<DX>(a.bn, acc, lane, m0, a.M, n);
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int m = m0 + acc_row(reg, lane);
    if (m < a.M) a.dx[(size_t)m * DX + n] = acc[reg] * scn;
  }
}

// grid = (row blocks of 32 of [W | U | b] x column blocks of 64, 2 directions, kRdSlices)
template <int DX, int H>
__global__ void __launch_bounds__(256) rl_wgrad_kernel(const RlArgs a) {
  constexpr int G = 4 * H, NB = G / 64, R = DX + H + 1;     // row R - 1 of the direction's block is the bias
  __shared__ __attribute__((aligned(16))) float red[4 * 2048];
  const int T = a.T, tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dir = blockIdx.y, mt = blockIdx.x / NB, ng = blockIdx.x % NB, ks = blockIdx.z;
  const int nrow = a.b < kL4ChunkRows ? a.b : kL4ChunkRows;
  const int K = nrow * T, npair = (K + 1) / 2, per = (npair + kRdSlices - 1) / kRdSlices;
  const int pend = (ks + 1) * per < npair ? (ks + 1) * per : npair;
  const int row = mt * 32 + l31;
  f32x16 acc[2] = {splat16(0.f), splat16(0.f)};
  for (int p0 = ks * per + wave; p0 < pend; p0 += 16) {    // four pairs at a time: their loads are in flight together
    float av[4], bv0[4], bv1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kk = 2 * (p0 + 4 * i) + half;
      av[i] = 0.f; bv0[i] = 0.f; bv1[i] = 0.f;
      if (p0 + 4 * i < pend && kk < K) {
        const int lr = kk / T, t = kk - lr * T;
        const float* zp = a.gz + ((size_t)kk * 2 + dir) * G + ng * 64 + l31;
        bv0[i] = zp[0]; bv1[i] = zp[32];
        if (row < DX) av[i] = a.x[((size_t)a.rows[lr] * T + t) * DX + row];
        else if (row < DX + H) {
          const int tp = dir ? t + 1 : t - 1;               // the step before in this direction's order
          if (tp >= 0 && tp < T) av[i] = a.h[((size_t)lr * T + tp) * (2 * H) + dir * H + row - DX];
        } else av[i] = row == DX + H ? 1.f : 0.f;
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
  float* out = a.gsum + (size_t)ks * kRdN + (size_t)dir * R * G;
  for (int i = tid; i < 2048; i += 256) {
    const int m = mt * 32 + (i >> 6), n = ng * 64 + (i & 63);
    if (m >= R) continue;
    float s = 0.f;
    for (int w = 0; w < 4; ++w) s += red[w * 2048 + i];
    float* o = out + (size_t)m * G + n;                     // W, U and b lie behind one another in rows of 4H
    *o = a.cont ? *o + s : s;
  }
}

}  // namespace nrv
