// Fitting gamma and beta of the BatchNorms inside the fitted section (nrv_fit_set_bn_affine): the two per-channel sums of a
// BatchNorm, formed where its unscaled dy exists, and the refold of the fit's (scale, shift) pairs behind an update.
#pragma once
#include "nrv_common.h"

namespace nrv {

// ---------------------------------------------------------------------------------------
// nanoreviser_amd/bnaffine.py is the DEFINITION; include/nanorev.h (nrv_fit_set_bn_affine) states the rule.  Per channel, with dy
// the derivative of the batch's SUM of row losses by the BatchNorm's output, x the activation it normalises, mean / var the
// block's CURRENT statistics and r = 1 / sqrt(var + 1e-3):
//     g_gamma = r sum dy (x - mean) / b          g_beta = sum dy / b
// in the pivoted form, f32, no contraction.  THE BLOCK is the front of the vector: for every BatchNorm inside, in tensor order,
// gamma [C] then beta [C].  dy exists unscaled only inside the launch that multiplies it by the scale, so each of those is a
// template on its argument struct: with the struct that carries a BnAffArgs it ALSO stores one partial per workgroup, with the
// plain struct it is the kernel it was, instruction for instruction:
//   l4_dx_kernel<L4DxBnArgs>            bn_l3: dy = dXb4, x = the raw H3          (nrv_lstm3fit.h)
//   l3_dx_kernel<true, SigBnArgs>       bn_l2: dy = dXin[..., :128], x = the raw H2   (nrv_signalfit.h; depth NRV_FIT_FULL)
//   rl_dx_kernel<32, 64, RlDxBnArgs>    bn_l1: dy = dX1b, x = the raw H1          (nrv_fullfit.h)
//   sig_backward_kernel<SigBnArgs>      bn_c2: dy = dF, x = a2;  bn_c1: dy = dc1, x = a1 recomputed   (nrv_signalfit.h)
// Every one of them runs on ceil(M / 32) workgroups, workgroup w on the pairs 32 w ..; the partials are ONE array
// [workgroups of the batch's first chunk][block], a BatchNorm's sums at its place in the block, r already applied.  A later
// chunk (cont) adds its partial onto what the same workgroup index left.  head_reduce_kernel adds the workgroups in ascending
// order and divides by b - with a flag range of its own -, head_adam_kernel updates the block with the rest of the vector, and
//   bn_refold_kernel         workgroup per BatchNorm inside, thread per channel: s = gamma / sqrt(var + 1e-3), h = beta - mean s
// in the host's bn_fold's operation order, so that the pairs of an untouched block are the bytes nrv_create folded.
// No atomics, no workgroup waits for another: the order of every sum is a function of (b, T) alone.
// ---------------------------------------------------------------------------------------
constexpr float kBnEps = 1e-3f;

struct BnAffArgs {
  const float* x;                        // [M][C] the raw activation of this chunk (the three Bi-LSTM BatchNorms)
  const float* mean;                     // [C] current statistics, out of the fit's block
  const float* var;
  float* part;                           // [workgroups][stride], already at this BatchNorm's gamma; its beta C floats behind
  int stride, cont;
};

// The epilogue of a dx launch: this lane holds column n of C (a wave's 32 columns, both halves the same n) and the 16 rows
// acc_row(reg, lane) of the workgroup's 32 pairs m0 ..; acc is dy, not yet scaled.  The lane adds its rows ascending, the upper
// half's sum is added to the lower's, and lanes 0 .. 31 store the workgroup's partial of column n.
template <int C>
__device__ __forceinline__ void bn_dy_partial(const BnAffArgs& b, const f32x16& acc, int lane, int m0, int M, int n) {
#pragma clang fp contract(off)
  const float mu = b.mean[n];
  float sg = 0.f, sb = 0.f;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int m = m0 + acc_row(reg, lane);
    if (m < M) {
      const float dy = acc[reg];
      sb += dy;
      sg += dy * (b.x[(size_t)m * C + n] - mu);
    }
  }
  const float og = __shfl_down(sg, 32), ob = __shfl_down(sb, 32);
  if (lane < 32) {
    const float r = 1.f / __builtin_sqrtf(b.var[n] + kBnEps);
    float* out = b.part + (size_t)blockIdx.x * b.stride;
    const float g = (sg + og) * r, be = sb + ob;
    out[n] = b.cont ? out[n] + g : g;
    out[C + n] = b.cont ? out[C + n] + be : be;
  }
}

struct BnRefoldArgs {
  struct One { int C, par_at, s_at, h_at, stat_at; } bn[5];   // gamma at par_at of the vector (beta C behind); s, h, mean in the block
  const float* par;                      // the vector
  float* blk;                            // the model's block; var lies var_off floats behind mean
  int var_off;
};
// grid = BatchNorms inside the section
__global__ void __launch_bounds__(256) bn_refold_kernel(const BnRefoldArgs a) {
#pragma clang fp contract(off)
  const BnRefoldArgs::One& b = a.bn[blockIdx.x];
  const int c = threadIdx.x;
  if (c >= b.C) return;
  const float inv = a.par[b.par_at + c] / __builtin_sqrtf(a.blk[b.stat_at + a.var_off + c] + kBnEps);
  a.blk[b.s_at + c] = inv;
  a.blk[b.h_at + c] = a.par[b.par_at + b.C + c] - a.blk[b.stat_at + c] * inv;
}

}  // namespace nrv
