// Fitting the whole head on the device (depth NRV_FIT_HEAD): the training set of lstm4 outputs, the gradient of one batch
// through the three per-timestep dense layers and the per-window tail, and the reduce / Adam launches of the long vector.
#pragma once
#include "nrv_tailfit.h"   // TailStat, TailState, TailMode, fit_nonfinite; tail_grad_kernel, whose tail this kernel repeats

namespace nrv {

// ---------------------------------------------------------------------------------------
// nanoreviser_amd/headfit.py is the DEFINITION; include/nanorev.h (nrv_fit_*, "depth") states the rule.  Fitted are tensors
// 50 .. 59 - dense1 W1 [128][128] b1, dense2 W2 [128][32] b2, main_out Wm [32][6] bm, each behind a ReLU and run per
// timestep, then the tail of nrv_tailfit.h - and the centres.  One parameter vector per model, P = 20838 + NRV_FIT_PARAMS:
//   [W1 | b1 | W2 | b2 | Wm | bm | Wf | bf | Wo | bo | Ce]        every kernel row-major [in][out], as the weight file has it
// THE SET (per model): x4 [rows][T][128] f32 - the f32 lstm4 output of a labelled window - and y [rows] u8.  Slots come from
// nrv_tailfit.h's fit_label_count -> fit_tile_scan -> fit_label_scatter; behind each launch group
//   head_gather_kernel   one thread per (window of the group, t, kq): a labelled window's 16 bytes move from the head's input
//     [tile][t][kq 32][32 rows][4] to x4[slot][t][kq * 4 ..].  Plain stores.
// THE STEP: 3 launches per batch of b rows, enqueued back to back:
//   head_grad_kernel   min(tiles, kHeadFitMaxWg) workgroups of four waves; workgroup g takes the 32-row tiles g, g + G, ...
//     of the batch in ascending order.  Per tile:
//       forward   wave w runs timesteps w, w + 4, ... IN head_mlp_kernel's OPERATION ORDER (the same v_mfma_f32_32x32x2_f32
//         chains in the same k order from the same bias splat, the same relu_nan, activations through a wave-private LDS
//         image in the same layout), main_out straight into the tile's flat image; then the block runs the tail IN
//         head_final_kernel's ORDER as tail_grad_kernel does.  p is what nrv_predict* gives in f32 mode, bit for bit.
//       backward  tail_grad_kernel's dz and its five gradients; dF = dz Wf^T masked by mo > 0 (VALU) replaces the flat
//         image.  Then four timesteps at a time, one per wave: h1 and h2 of the timestep are RECOMPUTED (the forward's two
//         128-wide products again - nothing of a timestep is kept but its six main_out values: h1 of 32 rows x T = 32 is
//         512 KB and would have to travel through memory twice, the recomputation is 2 of 8 matrix products), then
//           dmo (6 wide), gWm = h2^T dmo, gbm, dh2 = dmo Wm^T where h2 > 0, gb2            VALU, in place over h2
//           gW2 += h1^T dh2      MFMA: A[k1][r] = h1 read down the image's rows, B[r][n] = dh2
//           dh1 = dh2 W2^T where h1 > 0      MFMA: A[r][n] = dh2, B[n][k1] = W2[k1][n]; in place over h1
//         and behind a barrier wave w adds the four timesteps, ascending, to ITS 32 rows of gW1 (k1 = 32w ..):
//           gW1 += X_t^T dh1_t   MFMA: A[k][r] = X (read from the set), B[r][n] = dh1_t (the image of the wave that made it)
//         gb1 = column sums of the four dh1 images.  gW1 / gW2 / gb* stay in registers over all tiles of the workgroup.
//     At the end the waves' gW2, gWm, gbm, gb2 are added in ascending wave order and the workgroup stores one partial
//     vector [P]; nothing is divided by b here.  Every sum's order is a function of (b, T) alone.
//   head_reduce_kernel   thread per parameter: g = (sum of the partials in ascending workgroup order) / b, and per workgroup a
//     flag "some g of mine is not finite" (a plain store).
//   head_adam_kernel     thread per parameter: every workgroup reads ALL flags first - the finite check covers the whole vector
//     before any parameter moves - then tail_adam_kernel's arithmetic, operation for operation (fp contract off, correctly
//     rounded sqrt and division, lr_t from the host's f64 table).  Workgroup 0 moves the state; the step counter the update
//     reads (t_cur) is a copy head_reduce_kernel made, so no workgroup can see the new one.
// No atomics anywhere: two runs give the same bytes.
// head_grad_kernel<GRAD, true> is the same kernel at depth NRV_FIT_LSTM4 (nrv_lstm4fit.h): x is the scratch X4 of one chunk of
// the batch in batch order, the dh1 images are copied out for l4_backward_kernel, and a later chunk continues the partials.
// ---------------------------------------------------------------------------------------
constexpr int kHfW1 = 0, kHfB1 = 128 * 128, kHfW2 = kHfB1 + 128, kHfB2 = kHfW2 + 128 * 32, kHfWm = kHfB2 + 32,
              kHfBm = kHfWm + 32 * 6, kHfMlp = kHfBm + 6;                 // 20838: where the tail's vector starts
constexpr int kHeadFitMaxWg = 128;
constexpr int kHeadFitMaxP = kHfMlp + kFitMaxP;
constexpr int kHfPlane = 32 * 4 + 4;                                      // head_mlp_kernel's image: [u >> 2][row][u & 3]

struct HeadGatherArgs {
  const float* in[2];                    // the head's f32 input of the group [tile][t][kq 32][32 rows][4]
  float* x[2];                           // the set [cap][T][128]
  const int* slot;                       // the group's first window
  int n, T;                              // windows of the group
  long long cap;
};
// grid = (ceil(n * T * 32 / 256), 2 models)
__global__ void __launch_bounds__(256) head_gather_kernel(const HeadGatherArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int per = a.T * 32;
  if (g >= (long long)a.n * per) return;
  const int i = (int)(g / per), j = (int)(g % per), t = j >> 5, kq = j & 31;
  const long long s = a.slot[i];
  if (s < 0 || s >= a.cap) return;
  const f32x4 v = *(const f32x4*)(a.in[blockIdx.y] + ((size_t)(i >> 5) * a.T + t) * 4096 + kq * 128 + (i & 31) * 4);
  *(f32x4*)(a.x[blockIdx.y] + ((size_t)s * a.T + t) * 128 + kq * 4) = v;
}

struct HeadState { TailState s; long long t_cur; };       // s as the tail has it; t_cur: s.t as the batch's update reads it

struct HeadGradArgs {
  const float* x;                        // the set's rows [.][T][128]
  const unsigned char* y;
  const unsigned* rows;                  // [b] row indices of this batch (checked by the host)
  const float* par;                      // [P]
  float* partial;                        // [workgroups][P]           (GRAD only)
  TailStat* pstat;                       // [workgroups]
  float* p_out;                          // [b][C] or null
  int T, C, b;
  float lambda;
  float cw[6];
  // depth NRV_FIT_LSTM4 (head_grad_kernel<., true>, nrv_lstm4fit.h): x holds the rows of one CHUNK of the batch in batch order
  // (row i of the chunk is x[i], its label y[rows[i]]), dh1 [.][T][128] receives dh1 (l4_backward_kernel forms dX4 = dh1 W1^T
  // from it: this kernel has no registers left for a fifth product), and with cont != 0 the
  // workgroup continues the partial vector and the statistics that the chunks before left
  float* dh1;
  int cont;
};

// h1 and h2 of (32 rows, timestep t) into the wave's images; with MO main_out into flat[row * fsm + t * 6 + k] (0 behind
// the batch's end, as tail_grad_kernel has it)
template <bool MO>
__device__ __forceinline__ void hf_forward(const float* __restrict__ par, const float* xrow, float* im1, float* im2, float* flat,
                                           const int fsm, const int t, const int n_here, const int lane) {
  const int half = lane >> 5, l31 = lane & 31;
  f32x16 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = splat16(par[kHfB1 + nt * 32 + l31]);
#pragma unroll 2
  for (int kg = 0; kg < 16; ++kg) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (xrow) a = *(const f32x4*)(xrow + kg * 8 + half * 4);
    const float* wr = par + kHfW1 + (kg * 8 + half * 4) * 128 + l31;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt] = mfma32(a[j], wr[j * 128 + nt * 32], acc[nt]);
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int u = nt * 32 + l31;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) im1[(u >> 2) * kHfPlane + acc_row(reg, lane) * 4 + (u & 3)] = relu_nan(acc[nt][reg]);
  }
  wave_lds_fence();
  f32x16 a2 = splat16(par[kHfB2 + l31]);
  {
    const float* hp = im1 + half * kHfPlane + l31 * 4;
#pragma unroll 4
    for (int kg = 0; kg < 16; ++kg) {
      const f32x4 a = *(const f32x4*)(hp + kg * 2 * kHfPlane);
      const float* wr = par + kHfW2 + (kg * 8 + half * 4) * 32 + l31;
#pragma unroll
      for (int j = 0; j < 4; ++j) a2 = mfma32(a[j], wr[j * 32], a2);
    }
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) im2[(l31 >> 2) * kHfPlane + acc_row(reg, lane) * 4 + (l31 & 3)] = relu_nan(a2[reg]);
  wave_lds_fence();
  if constexpr (MO) {
    f32x16 a3 = splat16(l31 < 6 ? par[kHfBm + l31] : 0.f);
    const float* hp = im2 + half * kHfPlane + l31 * 4;
#pragma unroll
    for (int kg = 0; kg < 4; ++kg) {
      const f32x4 a = *(const f32x4*)(hp + kg * 2 * kHfPlane);
#pragma unroll
      for (int j = 0; j < 4; ++j) a3 = mfma32(a[j], l31 < 6 ? par[kHfWm + (kg * 8 + half * 4 + j) * 6 + l31] : 0.f, a3);
    }
    if (l31 < 6) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) flat[acc_row(reg, lane) * fsm + t * 6 + l31] = acc_row(reg, lane) < n_here ? relu_nan(a3[reg]) : 0.f;
    }
  }
}

template <bool GRAD, bool L4 = false>
__global__ void __launch_bounds__(256) head_grad_kernel(const HeadGradArgs a) {
  constexpr int KPMAX = 6 * kHeadMaxT;           // head_final_kernel's flat image
  constexpr int FSM = KPMAX + 4;
  constexpr int IM1 = 32 * kHfPlane, IM2 = 8 * kHfPlane, WIM = IM1 + IM2 + 256;     // a wave's h1 | h2 | dmo
  __shared__ __attribute__((aligned(16))) float wim[4 * WIM];
  __shared__ __attribute__((aligned(16))) float flatv[32 * FSM];
  __shared__ float featv[32 * 17];
  __shared__ float logit[32 * 8];
  __shared__ float dl[32 * 8];
  __shared__ float dz[32 * 17];
  __shared__ float wo[16 * 8];
  __shared__ float cen[8 * 16];
  __shared__ int ys[32];
  __shared__ long long rix[32];                  // the tile's rows in the set, -1 behind the batch's end
  __shared__ float r_ce[32], r_cen[32];
  __shared__ int r_ok[32];
  const int T = a.T, C = a.C, tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = 6 * T, KP = (K + 3) & ~3;
  const int oBf = 16 * K, oWo = oBf + 16, oBo = oWo + 16 * C, oCe = oBo + C, PT = oCe + 16 * C, P = kHfMlp + PT;
  const float* par = a.par;
  const float* tpar = a.par + kHfMlp;            // the tail's vector
  const float* featw = tpar;
  const float* featb = tpar + oBf;
  const float* outw = tpar + oWo;
  const float* outb = tpar + oBo;
  float* im1 = wim + wave * WIM;
  float* im2 = im1 + IM1;
  float* dmo = im2 + IM2;
  const int n_tiles = (a.b + 31) / 32;
  float* out = GRAD ? a.partial + (size_t)blockIdx.x * P : nullptr;
  // what a wave carries over all tiles of the workgroup
  f32x16 gW1[4], gW2[4];
  float gWm[3] = {0.f, 0.f, 0.f}, gbm = 0.f, gb2 = 0.f, gb1 = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) { gW1[i] = splat16(0.f); gW2[i] = splat16(0.f); }
  TailStat wst{0.0, 0.0, 0, 0};                  // thread 0's
  bool first = true;
  bool cont = false;
  if constexpr (L4) cont = a.cont != 0;

  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, first = false) {
    const int n_here = a.b - tile * 32 < 32 ? a.b - tile * 32 : 32;
    __syncthreads();                             // the tile before is done with every image
    if (tid < 32) {
      long long row = tid < n_here ? (long long)a.rows[tile * 32 + tid] : -1;
      ys[tid] = row >= 0 ? (int)a.y[row] : 0;
      if constexpr (L4) row = tid < n_here ? (long long)tile * 32 + tid : -1;
      rix[tid] = row;
    }
    for (int i = tid; i < 32 * (KP - K); i += 256) flatv[(i / (KP - K)) * FSM + K + i % (KP - K)] = 0.f;
    if (tid < 16 * C) { wo[(tid / C) * 8 + tid % C] = outw[tid]; cen[(tid / 16) * 16 + tid % 16] = tpar[oCe + tid]; }
    __syncthreads();
    const float* xrow = rix[l31] >= 0 ? a.x + (size_t)rix[l31] * T * 128 : nullptr;      // the A operand's row of this lane
    for (int t = wave; t < T; t += 4) hf_forward<true>(par, xrow ? xrow + t * 128 : nullptr, im1, im2, flatv, FSM, t, n_here, lane);
    __syncthreads();
    // ---- the tail, as tail_grad_kernel runs it ----
    for (int it = tid; it < 32 * 16; it += 256) {
      const int r = it >> 4, f = it & 15;
      float v = featb[f];
      const f32x4* fr = (const f32x4*)(flatv + r * FSM);
#pragma unroll 2
      for (int k4 = 0; k4 < KP / 4; ++k4) {
        const f32x4 x = fr[k4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v = __builtin_fmaf(x[j], k4 * 4 + j < K ? featw[(k4 * 4 + j) * 16 + f] : 0.f, v);
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
      for (int r = 0; r < n_here; ++r) { wst.ce += (double)r_ce[r]; wst.center += (double)r_cen[r]; wst.correct += r_ok[r]; }
      wst.rows += n_here;
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
      for (int idx = tid; idx < PT; idx += 256) {          // the tail's five gradients, this tile added to the tiles before
        float s = 0.f;
        if (idx < oBf) {
          const int k = idx >> 4, f = idx & 15;
#pragma unroll 4
          for (int r = 0; r < 32; ++r) s = __builtin_fmaf(flatv[r * FSM + k], dz[r * 17 + f], s);
        } else if (idx < oWo) {
          const int f = idx - oBf;
#pragma unroll 4
          for (int r = 0; r < 32; ++r) s += dz[r * 17 + f];
        } else if (idx < oBo) {
          const int f = (idx - oWo) / C, cc = (idx - oWo) % C;
#pragma unroll 4
          for (int r = 0; r < 32; ++r) s = __builtin_fmaf(featv[r * 17 + f], dl[r * 8 + cc], s);
        } else if (idx < oCe) {
          const int cc = idx - oBo;
#pragma unroll 4
          for (int r = 0; r < 32; ++r) s += dl[r * 8 + cc];
        } else {
          const int cc = (idx - oCe) >> 4, f = (idx - oCe) & 15;
#pragma unroll 4
          for (int r = 0; r < n_here; ++r)
            if (ys[r] == cc) s = __builtin_fmaf(-two_l, featv[r * 17 + f] - cen[cc * 16 + f], s);
        }
        out[kHfMlp + idx] = (first && !cont) ? s : out[kHfMlp + idx] + s;
      }
      __syncthreads();
      // dF = dz Wf^T where mo > 0, in place of the flat image
      for (int it = tid; it < 32 * K; it += 256) {
        const int r = it / K, k = it % K;
        float v = 0.f;
#pragma unroll
        for (int f = 0; f < 16; ++f) v = __builtin_fmaf(dz[r * 17 + f], featw[k * 16 + f], v);
        flatv[r * FSM + k] = flatv[r * FSM + k] > 0.f ? v : 0.f;
      }
      __syncthreads();
      for (int tg = 0; tg < T; tg += 4) {
        const int t = tg + wave;
        if (t < T) {
          hf_forward<false>(par, xrow ? xrow + t * 128 : nullptr, im1, im2, nullptr, 0, t, n_here, lane);
          for (int i = lane; i < 256; i += 64) dmo[i] = (i & 7) < 6 ? flatv[(i >> 3) * FSM + t * 6 + (i & 7)] : 0.f;
          wave_lds_fence();
#pragma unroll 1
          for (int q = 0; q < 3; ++q) {                    // gWm[k2][c] = sum_r h2[r][k2] dmo[r][c]
            const int idx = lane + 64 * q, k2 = idx / 6, c = idx % 6;
            const float* hp = im2 + (k2 >> 2) * kHfPlane + (k2 & 3);
            float s = 0.f;
#pragma unroll 4
            for (int r = 0; r < 32; ++r) s = __builtin_fmaf(hp[r * 4], dmo[r * 8 + c], s);
            gWm[q] += s;
          }
          if (lane < 6) {
            float s = 0.f;
#pragma unroll 4
            for (int r = 0; r < 32; ++r) s += dmo[r * 8 + lane];
            gbm += s;
          }
          wave_lds_fence();
#pragma unroll 2
          for (int q = 0; q < 16; ++q) {                   // dh2[r][k2] = sum_c dmo[r][c] Wm[k2][c] where h2 > 0
            const int e = lane + 64 * q, r = e >> 5, k2 = e & 31;
            float v = 0.f;
#pragma unroll
            for (int c = 0; c < 6; ++c) v = __builtin_fmaf(dmo[r * 8 + c], par[kHfWm + k2 * 6 + c], v);
            float* hp = im2 + (k2 >> 2) * kHfPlane + r * 4 + (k2 & 3);
            *hp = *hp > 0.f ? v : 0.f;
          }
          wave_lds_fence();
          if (lane < 32) {
            const float* hp = im2 + (lane >> 2) * kHfPlane + (lane & 3);
            float s = 0.f;
#pragma unroll 4
            for (int r = 0; r < 32; ++r) s += hp[r * 4];
            gb2 += s;
          }
          // gW2[k1][n] += sum_r h1[r][k1] dh2[r][n]          (k-groups not unrolled: their loads would all be hoisted)
#pragma unroll 1
          for (int kg = 0; kg < 4; ++kg)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int r = kg * 8 + half * 4 + j;
              const float bv = im2[(l31 >> 2) * kHfPlane + r * 4 + (l31 & 3)];
#pragma unroll
              for (int mt = 0; mt < 4; ++mt)
                gW2[mt] = mfma32(im1[((mt * 32 + l31) >> 2) * kHfPlane + r * 4 + (l31 & 3)], bv, gW2[mt]);
            }
          // dh1[r][k1] = sum_n dh2[r][n] W2[k1][n] where h1 > 0
          f32x16 d[4];
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) d[nt] = splat16(0.f);
#pragma unroll 1
          for (int kg = 0; kg < 4; ++kg) {
            const f32x4 av = *(const f32x4*)(im2 + (kg * 2 + half) * kHfPlane + l31 * 4);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
              const f32x4 bv = *(const f32x4*)(par + kHfW2 + (nt * 32 + l31) * 32 + kg * 8 + half * 4);
#pragma unroll
              for (int j = 0; j < 4; ++j) d[nt] = mfma32(av[j], bv[j], d[nt]);
            }
          }
          wave_lds_fence();                                // gW2's reads of h1 before it is overwritten
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const int u = nt * 32 + l31;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
              float* hp = im1 + (u >> 2) * kHfPlane + acc_row(reg, lane) * 4 + (u & 3);
              *hp = *hp > 0.f ? d[nt][reg] : 0.f;
            }
          }
        }
        __syncthreads();
        const int nt_here = T - tg < 4 ? T - tg : 4;
        for (int tt = 0; tt < nt_here; ++tt) {             // gW1[k][n] += sum_r X[r][t][k] dh1_t[r][n], k = 32 wave ..
          const float* img = wim + tt * WIM;
#pragma unroll 1
          for (int kg = 0; kg < 4; ++kg)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int r = kg * 8 + half * 4 + j;
              const long long row = rix[r];
              const float av = row >= 0 ? a.x[((size_t)row * T + tg + tt) * 128 + wave * 32 + l31] : 0.f;
#pragma unroll
              for (int nt = 0; nt < 4; ++nt)
                gW1[nt] = mfma32(av, img[((nt * 32 + l31) >> 2) * kHfPlane + r * 4 + (l31 & 3)], gW1[nt]);
            }
        }
        if constexpr (L4) {                                // the four dh1 images to the chunk's scratch, 16 bytes a move
          for (int i = tid; i < nt_here * 1024; i += 256) {
            const int tt = i >> 10, kq = (i >> 5) & 31, r = i & 31;
            if (r < n_here)
              *(f32x4*)(a.dh1 + ((size_t)(tile * 32 + r) * T + tg + tt) * 128 + kq * 4) = *(const f32x4*)(wim + tt * WIM + kq * kHfPlane + r * 4);
          }
        }
        if (tid < 128) {
          for (int tt = 0; tt < nt_here; ++tt) {
            const float* hp = wim + tt * WIM + (tid >> 2) * kHfPlane + (tid & 3);
            float s = 0.f;
#pragma unroll 4
            for (int r = 0; r < 32; ++r) s += hp[r * 4];
            gb1 += s;
          }
        }
        __syncthreads();
      }
    }
  }
  if (tid == 0) {
    if (cont) {
      const TailStat o = a.pstat[blockIdx.x];
      wst.ce = o.ce + wst.ce; wst.center = o.center + wst.center; wst.correct += o.correct; wst.rows += o.rows;
    }
    a.pstat[blockIdx.x] = wst;
  }
  if constexpr (GRAD) {
    auto keep = [&](float* o, float v) { *o = cont ? *o + v : v; };
    // gW1: wave w owns rows 32 w .. of it; everything else is summed over the waves in ascending order
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) keep(out + kHfW1 + (wave * 32 + acc_row(reg, lane)) * 128 + nt * 32 + l31, gW1[nt][reg]);
    if (tid < 128) keep(out + kHfB1 + tid, gb1);
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) im1[(mt * 32 + acc_row(reg, lane)) * 32 + l31] = gW2[mt][reg];
#pragma unroll
    for (int q = 0; q < 3; ++q) im2[lane + 64 * q] = gWm[q];
    if (lane < 6) im2[192 + lane] = gbm;
    if (lane < 32) im2[200 + lane] = gb2;
    __syncthreads();
    for (int i = tid; i < 128 * 32; i += 256) {
      float s = 0.f;
      for (int w = 0; w < 4; ++w) s += wim[w * WIM + i];
      keep(out + kHfW2 + i, s);
    }
    if (tid < 232 && (tid < 198 || tid >= 200)) {
      float s = 0.f;
      for (int w = 0; w < 4; ++w) s += wim[w * WIM + IM1 + tid];
      keep(out + (tid < 192 ? kHfWm + tid : tid < 198 ? kHfBm + tid - 192 : kHfB2 + tid - 200), s);
    }
  }
}

// ---- reduce and update ---------------------------------------------------------------------------------------------------
struct HeadAdamArgs {
  const float* partial;                  // [n_wg][P]
  const TailStat* pstat;                 // [n_wg]
  int n_wg, b, P, mode;
  float *par, *m, *v, *g;                // [P] each
  HeadState* st;
  int* flag;                             // [gridDim.x] of the two launches
  const float* lr;                       // as TailAdamArgs
  long long t0, n_lr;
  float beta1, beta2, eps;
};

// grid = ceil(P / 256)
__global__ void __launch_bounds__(256) head_reduce_kernel(const HeadAdamArgs a) {
#pragma clang fp contract(off)
  __shared__ int bad;
  const int tid = threadIdx.x, idx = blockIdx.x * 256 + tid;
  if (tid == 0) bad = 0;
  __syncthreads();
  if (a.mode != kTailEval && idx < a.P) {
    float s = 0.f;
    for (int w = 0; w < a.n_wg; ++w) s += a.partial[(size_t)w * a.P + idx];
    const float g = s / (float)a.b;
    a.g[idx] = g;
    if (fit_nonfinite(g)) bad = 1;
  }
  __syncthreads();
  if (tid == 0) {
    a.flag[blockIdx.x] = bad;
    if (blockIdx.x == 0) a.st->t_cur = a.st->s.t;
  }
}

__global__ void __launch_bounds__(256) head_adam_kernel(const HeadAdamArgs a) {
#pragma clang fp contract(off)
  __shared__ int bad;
  const int tid = threadIdx.x, idx = blockIdx.x * 256 + tid;
  const long long t = a.st->t_cur;
  if (tid == 0) bad = 0;
  __syncthreads();
  if (a.mode != kTailEval)
    for (int i = tid; i < (int)gridDim.x; i += 256)
      if (a.flag[i]) bad = 1;
  __syncthreads();
  const bool skip = bad != 0;
  if (a.mode == kTailTrain && !skip && t - a.t0 >= 0 && t - a.t0 < a.n_lr && idx < a.P) {
    const float lr = a.lr[t - a.t0];
    const float c1 = 1.f - a.beta1, c2 = 1.f - a.beta2;
    const float g = a.g[idx];
    const float mm = a.beta1 * a.m[idx] + c1 * g;
    const float vv = a.beta2 * a.v[idx] + c2 * (g * g);
    a.m[idx] = mm;
    a.v[idx] = vv;
    a.par[idx] = a.par[idx] - (lr * mm) / (__builtin_sqrtf(vv) + a.eps);
  }
  if (blockIdx.x == 0 && tid == 0) {
    TailState s = a.st->s;
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
    a.st->s = s;
  }
}

}  // namespace nrv
