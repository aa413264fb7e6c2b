// Fitting the signal branch with lstm3 and everything behind it on the device (depth NRV_FIT_SIGNAL): the training set of lstm2
// outputs and normalised samples, the forward and the backward pass of conv1 / conv2 / sig_dense over a batch, and the data
// gradient out of lstm3.
#pragma once
#include "nrv_cnn.h"       // conv_positions: the convolutions of the forward launch are the inference kernel's, not restated
#include "nrv_dropout.h"   // nrv_fit_set_dropout: the keep bits of F's quads
#include "nrv_lstm3fit.h"  // its launches run unchanged on this depth's scratch Xin

namespace nrv {

// ---------------------------------------------------------------------------------------
// nanoreviser_amd/signalfit.py is the DEFINITION; include/nanorev.h (nrv_fit_*, "depth") states the rule.  Fitted are tensors 0, 1,
// 6, 7, 32 .. 39, 44 .. 59 and the centres; the three BatchNorms inside the fitted section are FROZEN and applied in their
// inference form (behind a convolution: relu(conv) * s + h), and the reference's Dropout is applied only while nrv_fit_set_dropout
// is on (the DROP instantiations below; off, every launch is the instantiation it was).  One vector per model,
// P = 25896 + NRV_FIT_PARAMS_LSTM3:
//   [w1 [3][8] | b1 [8] | w2 [3][8][8] | b2 [8] | Ws [400][64] | bs [64] | the lstm3 depth's vector]
// THE SET: per model x2 [rows][T][128] f32 (the BatchNorm'd f32 lstm2 output) and y [rows] u8; ONE sig [rows][T][50] f32 for both
// models (they read the same samples).  Inside each launch group, where the lstm3 depth gathers:
//   sig_gather_kernel   one thread per (window of the group, t, q of 57): q < 32 is 16 bytes of lstm2's output through the
//     ActView the lstm3 launch reads, per model; q >= 32 is 8 bytes of the group's event-major samples (window w, step t is event
//     w + t), once.  Plain stores.
// THE STEP of a batch of b rows, in the lstm4 depth's CHUNKS; M = chunk rows x T (row, t) pairs; per chunk
//   sig_forward_kernel  workgroup per 32 pairs, four waves.  The convolutions on the VALU through conv_positions (thread per
//     (pair, 6 or 7 samples)) into cnn_kernel's A-fragment image in LDS, the conv constants from a 264-float image in LDS: the
//     vector's w1, b1, w2, b2 with the handle's frozen s, h.  Then S = F Ws + bs on v_mfma_f32_16x16x4_f32 in cnn_kernel<false>'s
//     k order, wave w the 16 columns 16 w .., Ws read from the vector (L2).  Writes Xin [M][192] = [x2 | S] and KEEPS F [M][400].
//   the lstm3 depth's launches on Xin with an identity row list (the head reads its labels through the batch's own list).
//   l3_dx_kernel        workgroup per 32 pairs, two waves, wave w the 32 columns 32 w ..: dS = dz3_fw W3f[128 ..]^T +
//     dz3_bw W3b[128 ..]^T, v_mfma_f32_32x32x2_f32, k ascending, forward direction first; dz3 is what l3_backward_kernel left in
//     place of lstm3's gates (it lies there by input time t for both directions).  Only the 64 signal columns are formed.
//   sig_backward_kernel workgroup per 32 pairs.  dF = dS Ws^T on the matrix pipe into LDS; z1, a1's side and c1 recomputed on
//     the VALU in the forward launch's operation order; da2 = dF s2 where z2 > 0, in place; gw2 / gb2 one thread per element
//     over (pair, sample) ascending; dc1, da1 = dc1 s1 where a1 > 0 in place of c1; gw1 / gb1 likewise.  The workgroup's 232
//     sums are stored as ONE partial (first chunk) or added to the partial the same workgroup index left (later chunks).
//   sig_wgrad_kernel    workgroup per (32 rows of [Ws | bs], 32 columns), eight waves: gWs = F^T dS, gbs = 1^T dS with k = (row, t)
//     ascending, pair p of k values on wave p % 8; the eight waves are added in ascending order and the block is stored (first
//     chunk) or added to what the chunks before left.  No partials.
//   head_reduce_kernel five times, each with a flag range of its own (25896 is no multiple of 256), head_adam_kernel once over
//   all of P on as many workgroups as there are flags.
// No atomics, no workgroup waits for another: every sum's order is a function of (b, T) alone.
// ---------------------------------------------------------------------------------------
constexpr int kSgB1 = 24, kSgW2 = 32, kSgB2 = 224, kSgConv = 232, kSgWs = 232, kSgBs = kSgWs + 400 * 64, kSgN = kSgBs + 64;
constexpr int kSgDense = 400 * 64 + 64;                    // [Ws | bs]
static_assert(kSgN == 25896 && kSgDense == 25664, "the signal block of the vector");

struct SigGatherArgs {
  ActView in0[2];                        // lstm2's output as the lstm3 launch reads it (KQ 32)
  const float* sig_ev;                   // the group's samples [events][50]
  float* x2[2];                          // the set [cap][T][128]
  float* sig;                            // the set [cap][T][50]
  const int* slot;
  int n, T;
  long long cap;
};
// grid = (ceil(n * T * 57 / 256), 2 models)
__global__ void __launch_bounds__(256) sig_gather_kernel(const SigGatherArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int per = a.T * 57;
  if (g >= (long long)a.n * per) return;
  const int i = (int)(g / per), j = (int)(g % per), t = j / 57, q = j % 57;
  const long long s = a.slot[i];
  if (s < 0 || s >= a.cap) return;
  const int m = blockIdx.y;
  if (q < 32) {
    *(f32x4*)(a.x2[m] + ((size_t)s * a.T + t) * 128 + q * 4) = *(const f32x4*)a.in0[m].chunk(i, t, q);
  } else if (m == 0) {
    *(f32x2*)(a.sig + ((size_t)s * a.T + t) * kSig + (q - 32) * 2) = *(const f32x2*)(a.sig_ev + (size_t)(i + t) * kSig + (q - 32) * 2);
  }
}

struct SigArgs {
  const float* x2;                       // the set's rows [.][T][128]
  const float* sig;                      // the set's samples [.][T][50]
  const unsigned* rows;                  // row indices of this chunk
  const float* par;                      // the vector: the signal block [kSgN], the lstm3 block [kL3N], ...
  const float* conv;                     // the handle's 264 conv constants: the frozen s1, h1 at 32, s2, h2 at 248
  float* xin;                            // [M][192]
  float* F;                              // [M][400]
  float* dS;                             // [M][64]
  const float* gz3;                      // lstm3's [M][2][512] holding dz3
  float* pconv;                          // [workgroups][kSgConv] partial sums, not yet divided by b
  float* gdense;                         // [kSgDense] sums
  int T, M, keep, cont;                  // pairs of this chunk; keep: F is wanted; cont: not the batch's first chunk
  float* dh2 = nullptr;                  // depth NRV_FIT_FULL: [M][128], dXin's lstm2 columns times s2 (l3_dx_kernel<true>)
  const float* s2 = nullptr;             // [128] the frozen BatchNorm behind lstm2
};

struct SigBnArgs : SigArgs { BnAffArgs bn; };               // nrv_fit_set_bn_affine: the launches that also leave a BatchNorm's two sums
template <class A> struct SigDrop : A { DropArgs drop; };   // nrv_fit_set_dropout: the DROP instantiations' arguments
template <class A, bool DROP> using SigDropOf = std::conditional_t<DROP, SigDrop<A>, A>;

// the 264-float image conv_positions reads: the vector's kernels and biases with the handle's frozen scales and shifts
__device__ __forceinline__ void sig_conv_image(const SigArgs& a, float* cwl, int tid) {
  for (int i = tid; i < 264; i += 256)
    cwl[i] = i < 32 ? a.par[i] : i < 48 ? a.conv[i] : i < 240 ? a.par[kSgW2 + i - 48] : i < 248 ? a.par[kSgB2 + i - 240] : a.conv[i];
}

// grid = ceil(M / 32).  X2 = false (depth NRV_FIT_FULL): columns 0 .. 127 of Xin are another launch's, x2 is not read
// DROP (nrv_fit_set_dropout): behind the convolutions every f32x4 of the img planes - quad kq of pair r - goes through the
// dropout in place, one Philox call each, thread (r = tid % 32, kq = tid / 32 + 8 j); the product and a.F see the dropped F
template <bool X2 = true, bool DROP = false>
__global__ void __launch_bounds__(256) sig_forward_kernel(const SigDropOf<SigArgs, DROP> a) {
  constexpr int PLANE = 32 * 4 + 4;
  __shared__ __attribute__((aligned(16))) float img[100 * PLANE];
  __shared__ __attribute__((aligned(16))) float cwl[264];
  __shared__ long long off[32];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * 32;
  sig_conv_image(a, cwl, tid);
  if (tid < 32) {
    const int m = m0 + tid;
    off[tid] = m < a.M ? (long long)a.rows[m / a.T] * a.T + m % a.T : -1;
  }
  __syncthreads();
  {
    const int chunk = wave * 2 + (lane >> 5), r = lane & 31;
    const int p0 = chunk < 2 ? 7 * chunk : 14 + 6 * (chunk - 2);
    const float* srow = off[r] >= 0 ? a.sig + (size_t)off[r] * kSig : nullptr;
    float x[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) {
      const int p = p0 - 2 + i;
      x[i] = (srow && p >= 0 && p < kSig) ? srow[p] : 0.f;
    }
    if (wave == 0) conv_positions<7>(cwl, x, p0, r, img, PLANE);
    else conv_positions<6>(cwl, x, p0, r, img, PLANE);
  }
  __syncthreads();
  if constexpr (DROP) {
    const int r = tid & 31;
    if (off[r] >= 0) {
      const unsigned row = a.rows[(m0 + r) / a.T];
      const int t = (m0 + r) % a.T;
      for (int kq = tid >> 5; kq < 100; kq += 8) {
        f32x4* const v = (f32x4*)(img + kq * PLANE + r * 4);
        const unsigned keep = drop_keep4(a.drop, row, t, kq);
        f32x4 x = *v;
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = drop_apply(x[j], keep >> j & 1u, a.drop.keepf);
        *v = x;
      }
    }
    __syncthreads();
  }
  {
    const int ct = wave, q4 = lane >> 4, r16 = lane & 15;
    const float* Ws = a.par + kSgWs + ct * 16 + r16;
    const float bias = a.par[kSgBs + ct * 16 + r16];
    f32x4 acc0 = {bias, bias, bias, bias}, acc1 = acc0;
    const float* ap = img + q4 * PLANE + r16 * 4;
#pragma unroll 5
    for (int kg = 0; kg < 25; ++kg) {
      const f32x4 a0 = *(const f32x4*)(ap + kg * 4 * PLANE);
      const f32x4 a1 = *(const f32x4*)(ap + kg * 4 * PLANE + 64);
      const float* wr = Ws + (size_t)(16 * kg + 4 * q4) * 64;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bw = wr[j * 64];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], bw, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], bw, acc1, 0, 0, 0);
      }
    }
    const int u = ct * 16 + r16;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = 4 * q4 + reg;
      if (m0 + row < a.M) a.xin[(size_t)(m0 + row) * 192 + 128 + u] = acc0[reg];
      if (m0 + row + 16 < a.M) a.xin[(size_t)(m0 + row + 16) * 192 + 128 + u] = acc1[reg];
    }
  }
  if (X2) for (int i = tid; i < 32 * 32; i += 256) {
    const int r = i >> 5, q = i & 31;
    if (off[r] >= 0) *(f32x4*)(a.xin + (size_t)(m0 + r) * 192 + q * 4) = *(const f32x4*)(a.x2 + (size_t)off[r] * 128 + q * 4);
  }
  if (a.keep)
    for (int i = tid; i < 32 * 100; i += 256) {
      const int r = i / 100, kq = i - r * 100;
      if (off[r] >= 0) *(f32x4*)(a.F + (size_t)(m0 + r) * 400 + kq * 4) = *(const f32x4*)(img + kq * PLANE + r * 4);
    }
}

// grid = ceil(M / 32), 128 threads.  FULL (depth NRV_FIT_FULL): 384 threads, the same product over all 192 columns of dXin - wave w
// the columns 32 w .. - whose first 128 go to dh2 times s2
// A = SigBnArgs (nrv_fit_set_bn_affine, FULL only): the first 128 columns are bn_l2's dy before the scale, and their two sums are left
template <bool FULL = false, class A = SigArgs>
__global__ void __launch_bounds__(FULL ? 384 : 128) l3_dx_kernel(const A a) {
  static_assert(FULL || std::is_same_v<A, SigArgs>, "bn_l2 lies inside the section at depth NRV_FIT_FULL only");
  constexpr int C0 = FULL ? 0 : 128;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * 32;
  const bool live = m0 + l31 < a.M;
  f32x16 acc = splat16(0.f);
  for (int dir = 0; dir < 2; ++dir) {
    const float* arow = a.gz3 + ((size_t)(m0 + l31) * 2 + dir) * 512;
    // W3 [192 in][512 gate columns]: B[k = gate column][n = signal column] = W3[128 + n][k]
    const float* w0 = a.par + kSgN + (size_t)dir * kL3Dir + (size_t)(C0 + wave * 32 + l31) * 512;
#pragma unroll 4
    for (int kg = 0; kg < 64; ++kg) {
      f32x4 av = {0.f, 0.f, 0.f, 0.f};
      if (live) av = *(const f32x4*)(arow + kg * 8 + half * 4);
      const f32x4 bv = *(const f32x4*)(w0 + kg * 8 + half * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = mfma32(av[j], bv[j], acc);
    }
  }
  if constexpr (std::is_same_v<A, SigBnArgs>)
    if (wave < 4) bn_dy_partial<128>(a.bn, acc, lane, m0, a.M, wave * 32 + l31);
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int m = m0 + acc_row(reg, lane);
    if (m >= a.M) continue;
    if (FULL && wave < 4) a.dh2[(size_t)m * 128 + wave * 32 + l31] = acc[reg] * a.s2[wave * 32 + l31];
    else a.dS[(size_t)m * 64 + C0 + wave * 32 + l31 - 128] = acc[reg];
  }
}


constexpr int kSgDfs = 401, kSgC1s = 52 * 8 + 1, kSgSs = 53;          // odd row strides: the pairs' rows on different banks

// The 16 sums (gamma [8] then beta [8]) every thread holds of one conv BatchNorm -> the workgroup's partial: the 256 threads are
// added through LDS in two ascending rounds of 16, r is applied to the gamma sums, and the partial is stored or added (cont)
__device__ __forceinline__ void bn_conv_partial(const BnAffArgs& b, const float (&sg)[8], const float (&sb)[8], int which, int tid) {
#pragma clang fp contract(off)
  __shared__ float red[16 * 256];
  __shared__ float red2[16 * 16];
#pragma unroll
  for (int o = 0; o < 8; ++o) { red[o * 256 + tid] = sg[o]; red[(8 + o) * 256 + tid] = sb[o]; }
  __syncthreads();
  {
    const int q = tid >> 4, sub = tid & 15;
    float s = red[q * 256 + sub * 16];
    for (int j = 1; j < 16; ++j) s += red[q * 256 + sub * 16 + j];
    red2[q * 16 + sub] = s;
  }
  __syncthreads();
  if (tid < 16) {
    float s = red2[tid * 16];
    for (int j = 1; j < 16; ++j) s += red2[tid * 16 + j];
    if (tid < 8) s *= 1.f / __builtin_sqrtf(b.var[which * 8 + tid] + kBnEps);
    float* out = b.part + (size_t)blockIdx.x * b.stride + which * 16 + tid;
    *out = b.cont ? *out + s : s;
  }
  __syncthreads();
}

// grid = ceil(M / 32).  A = SigBnArgs (nrv_fit_set_bn_affine): also the two sums of bn_c2 (dy = dF, x = a2) and of bn_c1 (dy = dc1,
// x = a1 recomputed in the forward launch's operation order), each thread over its own samples ascending
// DROP (nrv_fit_set_dropout): dF goes through the dropout in a pass of its own behind the product, before anything reads it -
// thread (pair r = tid % 32, quad q = tid / 32 + 8 j), one Philox call per quad; bn_c2's sums (dy = dF) see the masked dF.  z2, a1
// and c1 lie in front of the dropout and are recomputed as they were
template <class A = SigArgs, bool DROP = false>
__global__ void __launch_bounds__(256) sig_backward_kernel(const SigDropOf<A, DROP> a) {
  constexpr bool BN = std::is_same_v<A, SigBnArgs>;
  __shared__ float dfl[32 * kSgDfs];     // dF [pair][p * 8 + o], then da2 in its place
  __shared__ float c1l[32 * kSgC1s];     // c1 [pair][(p + 1) * 8 + ci] with a zero sample on either side, then da1 in its place
  __shared__ float sgl[32 * kSgSs];      // sig [pair][p + 1], likewise
  __shared__ unsigned char m1l[32 * 52]; // bit o: a1[p][o] > 0
  __shared__ __attribute__((aligned(16))) float cwl[264];
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * 32;
  sig_conv_image(a, cwl, tid);
  for (int i = tid; i < 32 * 52; i += 256) {
    const int r = i / 52, q = i - r * 52, m = m0 + r, p = q - 1;
    float v = 0.f;
    if (m < a.M && p >= 0 && p < kSig) v = a.sig[((size_t)a.rows[m / a.T] * a.T + m % a.T) * kSig + p];
    sgl[r * kSgSs + q] = v;
  }
  for (int i = tid; i < 32 * 16; i += 256) {               // c1 of the two samples outside: zero (`same` padding)
    const int r = i >> 4, j = i & 15;
    c1l[r * kSgC1s + (j < 8 ? j : 51 * 8 + j - 8)] = 0.f;
  }
  // dF = dS Ws^T: wave w takes the column tiles w, w + 4, ...; B[k = u][n = f] = Ws[f][u]
  {
    const bool live = m0 + l31 < a.M;
    f32x4 av[8];
#pragma unroll
    for (int kg = 0; kg < 8; ++kg) {
      av[kg] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (live) av[kg] = *(const f32x4*)(a.dS + (size_t)(m0 + l31) * 64 + kg * 8 + half * 4);
    }
    for (int nt = wave; nt < 13; nt += 4) {
      const int f = nt * 32 + l31;
      f32x16 acc = splat16(0.f);
#pragma unroll
      for (int kg = 0; kg < 8; ++kg) {
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (f < 400) bv = *(const f32x4*)(a.par + kSgWs + (size_t)f * 64 + kg * 8 + half * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = mfma32(av[kg][j], bv[j], acc);
      }
      if (f < 400)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) dfl[acc_row(reg, lane) * kSgDfs + f] = acc[reg];
    }
  }
  __syncthreads();
  if constexpr (DROP) {
    const int rr = tid & 31;
    if (m0 + rr < a.M) {
      const unsigned row = a.rows[(m0 + rr) / a.T];
      const int t = (m0 + rr) % a.T;
      for (int q = tid >> 5; q < 100; q += 8) {
        float* const v = dfl + rr * kSgDfs + q * 4;
        const unsigned keep = drop_keep4(a.drop, row, t, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = drop_apply(v[j], keep >> j & 1u, a.drop.keepf);
      }
    }
    __syncthreads();
  }
  // thread (pair r, sample chunk) as in the forward launch; the same operations in the same order, so the same sides
  const int chunk = wave * 2 + (lane >> 5), r = lane & 31;
  const int p0 = chunk < 2 ? 7 * chunk : 14 + 6 * (chunk - 2), np = chunk < 2 ? 7 : 6;
  const float* sg = sgl + r * kSgSs;
  float* c1 = c1l + r * kSgC1s;
  float* df = dfl + r * kSgDfs;
  for (int p = p0; p < p0 + np; ++p) {
    const float xm = sg[p], xc = sg[p + 1], xp = sg[p + 2];
    unsigned bits = 0;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      float v = cwl[24 + o];
      v = __builtin_fmaf(xm, cwl[o], v);
      v = __builtin_fmaf(xc, cwl[8 + o], v);
      v = __builtin_fmaf(xp, cwl[16 + o], v);
      v = __builtin_fmaxf(v, 0.f);
      if (v > 0.f) bits |= 1u << o;
      c1[(p + 1) * 8 + o] = v * cwl[32 + o] + cwl[40 + o];
    }
    m1l[r * 52 + p] = (unsigned char)bits;
  }
  __syncthreads();
  const float* w2 = cwl + 48;
  float bsg[8], bsb[8];                                     // BN: this thread's sums of one conv BatchNorm
  if constexpr (BN) {
#pragma unroll
    for (int o = 0; o < 8; ++o) { bsg[o] = 0.f; bsb[o] = 0.f; }
  }
  for (int p = p0; p < p0 + np; ++p) {
    float z[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) z[o] = w2[192 + o];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int ci = 0; ci < 8; ++ci) {
        const float cv = c1[(p + k) * 8 + ci];
#pragma unroll
        for (int o = 0; o < 8; ++o) z[o] = __builtin_fmaf(cv, w2[(k * 8 + ci) * 8 + o], z[o]);
      }
    if constexpr (BN) {
#pragma clang fp contract(off)
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        const float dy = df[p * 8 + o];
        bsb[o] += dy;
        bsg[o] += dy * (__builtin_fmaxf(z[o], 0.f) - a.bn.mean[8 + o]);
      }
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) df[p * 8 + o] = z[o] > 0.f ? df[p * 8 + o] * w2[200 + o] : 0.f;
  }
  __syncthreads();
  if constexpr (BN) {
    bn_conv_partial(a.bn, bsg, bsb, 1, tid);
#pragma unroll
    for (int o = 0; o < 8; ++o) { bsg[o] = 0.f; bsb[o] = 0.f; }
  }
  // gw2 [k][ci][o] and gb2 [o]: one thread per element, (pair, sample) ascending
  float* part = a.pconv + (size_t)blockIdx.x * kSgConv;
  if (tid < 200) {
    const int o = tid & 7, kc = tid >> 3;                   // kc = k * 8 + ci; 24: the bias
    float s = 0.f;
    for (int rr = 0; rr < 32; ++rr) {
      const float* cr = c1l + rr * kSgC1s + kc;             // c1[p + k - 1][ci] lies at ((p + k) * 8 + ci)
      const float* dr = dfl + rr * kSgDfs + o;
      if (kc < 24) for (int p = 0; p < kSig; ++p) s = __builtin_fmaf(cr[p * 8], dr[p * 8], s);
      else for (int p = 0; p < kSig; ++p) s += dr[p * 8];
    }
    float* out = part + (kc < 24 ? kSgW2 + tid : kSgB2 + o);
    *out = a.cont ? *out + s : s;
  }
  __syncthreads();
  // dc1[p][ci] = sum over k, o of w2[k][ci][o] da2[p - k + 1][o]; da1 = dc1 s1 where a1 > 0, in place of c1
  for (int p = p0; p < p0 + np; ++p) {
    float d[8];
#pragma unroll
    for (int ci = 0; ci < 8; ++ci) d[ci] = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int q = p - k + 1;
      if (q < 0 || q >= kSig) continue;
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        const float dv = df[q * 8 + o];
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) d[ci] = __builtin_fmaf(w2[(k * 8 + ci) * 8 + o], dv, d[ci]);
      }
    }
    if constexpr (BN) {
#pragma clang fp contract(off)
      const float xm = sg[p], xc = sg[p + 1], xp = sg[p + 2];
#pragma unroll
      for (int ci = 0; ci < 8; ++ci) {
        float v = cwl[24 + ci];
        v = __builtin_fmaf(xm, cwl[ci], v);
        v = __builtin_fmaf(xc, cwl[8 + ci], v);
        v = __builtin_fmaf(xp, cwl[16 + ci], v);
        v = __builtin_fmaxf(v, 0.f);
        bsb[ci] += d[ci];
        bsg[ci] += d[ci] * (v - a.bn.mean[ci]);
      }
    }
    const unsigned bits = m1l[r * 52 + p];
#pragma unroll
    for (int ci = 0; ci < 8; ++ci) c1[(p + 1) * 8 + ci] = (bits >> ci & 1u) ? d[ci] * cwl[32 + ci] : 0.f;
  }
  __syncthreads();
  if constexpr (BN) bn_conv_partial(a.bn, bsg, bsb, 0, tid);
  // gw1 [k][o] and gb1 [o]
  if (tid < 32) {
    const int o = tid & 7, k = tid >> 3;                    // 3: the bias
    float s = 0.f;
    for (int rr = 0; rr < 32; ++rr) {
      const float* xr = sgl + rr * kSgSs + k;               // sig[p + k - 1] lies at (p + k)
      const float* dr = c1l + rr * kSgC1s + 8 + o;
      if (k < 3) for (int p = 0; p < kSig; ++p) s = __builtin_fmaf(xr[p], dr[p * 8], s);
      else for (int p = 0; p < kSig; ++p) s += dr[p * 8];
    }
    float* out = part + (k < 3 ? tid : kSgB1 + o);
    *out = a.cont ? *out + s : s;
  }
}

constexpr int kSgWgM = 13;                                 // row blocks of 32 of [Ws 400 | bs 1]
// grid = (kSgWgM, 2 column tiles of 32), 512 threads
__global__ void __launch_bounds__(512) sig_wgrad_kernel(const SigArgs a) {
  __shared__ __attribute__((aligned(16))) float red[8 * 1024];
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mt = blockIdx.x, nt = blockIdx.y;
  const int K = a.M, npair = (K + 1) / 2;
  const int f = mt * 32 + l31;
  f32x16 acc = splat16(0.f);
  for (int pb = wave; pb < npair; pb += 32) {              // four pairs at a time: their loads are in flight together
    float av[4], bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kk = 2 * (pb + 8 * i) + half;
      av[i] = 0.f; bv[i] = 0.f;
      if (pb + 8 * i < npair && kk < K) {
        bv[i] = a.dS[(size_t)kk * 64 + nt * 32 + l31];
        av[i] = f < 400 ? a.F[(size_t)kk * 400 + f] : f == 400 ? 1.f : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = mfma32(av[i], bv[i], acc);
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) red[wave * 1024 + acc_row(reg, lane) * 32 + l31] = acc[reg];
  __syncthreads();
  for (int i = tid; i < 1024; i += 512) {
    const int row = mt * 32 + (i >> 5), n = nt * 32 + (i & 31);
    if (row > 400) continue;
    float s = 0.f;
    for (int w = 0; w < 8; ++w) s += red[w * 1024 + i];
    float* o = a.gdense + (size_t)row * 64 + n;              // row 400 is bs, which follows Ws in the vector
    *o = a.cont ? *o + s : s;
  }
}

}  // namespace nrv
