// Second read-branch layer, Bi-LSTM(32 -> 64), f16x2 mode: transposed products, weights in REGISTERS, 32-row chains (r07).
#pragma once
#include "nrv_lstm_f16x2s.h"   // mfma16_f16

namespace nrv {

// ---------------------------------------------------------------------------------------
// lstm2_r_kernel.  output_handeler.py:220 (Bidirectional(LSTM(64)) on the 32 features of read_rnn1).
//
// The layer is small (10.5 GFLOP per 4096-window group, 98 KB of f16x2 weights per direction) and was LATENCY-bound with
// hidden units on the lanes (round 2: 44-48 us, matrix pipe 27 % busy).  Here the products are TRANSPOSED,
// z^T = [W | U]^T [x ; h]: the weights are the A operand (M = the 256 gate-units), the activations the B operand (N = 16 data
// rows), so a result tile has the data row on the lane and the gate-units in the registers: tile (gate g, unit tile ut) of
// v_mfma_f32_16x16x32_f16 gives lane l = (row n = l & 15, q = l >> 4) the units 16 ut + 4 q + r, r = 0..3; i, f, g, o of a
// (row, unit) meet in one lane, c never leaves the lane, and the values of h_t the lanes (n, q) compute are - as two f16x8
// terms, elements 8 kb + j = unit 16 (2 kb + (j >> 2)) + 4 q + (j & 3) - B fragments of the next step's recurrent k-blocks:
// the host packs the rows of U in that k order (pack_lstm2_t).
//   * output: h x 2^13 as f16 split planes, RAW - the BatchNorm(128) behind this layer lives in the weights of the 192->128
//     layer's first 128 input rows (nrv_api.hip upload_model) - each lane's 4 units of a unit tile are 8 contiguous bytes.
//
// Earlier forms (HISTORY.md): lstm2_t_kernel (r03/r04, one wave per 16-row chain) and lstm2_u_kernel (r05, two waves per
// 16-row chain) copied one direction's whole weight set, 96 KiB + a 16 KiB bias image, into LDS in every workgroup and read
// each wave's share back from there on EVERY step: 48 of the 60 ds_read_b128 of a step, 13 % of the launch in the copy.
//
// Here a chain is one 32-row tile of one (direction, model) - exactly one [tile32] block of the X1 / X2 layouts - and a
// workgroup is one chain of FOUR waves.  Wave w owns unit tile w: 16 hidden units x 4 gates x 2 row tiles of 16 = 8
// accumulator tiles, 8 cell states per lane.  Its weights are then only [kb 3][gate 4][term 2] = 24 fragments of 1 KiB
// (tile g * 4 + w of pack_lstm2_t's layout): 96 VGPRs, loaded ONCE at kernel entry straight from global memory, every
// fragment feeding both row tiles.  The bias tiles (4, the same for both row tiles) are 16 more VGPRs and enter as the C
// operand of an accumulator's first product.  No LDS weight image, no staging loop, no staging barrier.
//   * h exchange: per row tile and term the wave holds 4 units per lane (8 bytes), half w & 1 of the B fragment of recurrent
//     k-block w >> 1.  Per row tile and step 2 ds_write_b64, one workgroup barrier, 4 ds_read_b128 ([kb][term]) through that
//     row tile's 4 KiB image: 8 KiB is all the LDS the kernel uses.
//   * the two row tiles of a wave are independent chains, and they run HALF A STEP APART (below): the gates of one lie between
//     the products of the other, two or three vector instructions behind every MFMA, so a wave's own stream keeps both the
//     matrix pipe and the vector issue fed.  (The first form built, both row tiles in one phase and one barrier per step:
//     32.8 us bracketed against 35.0 for lstm2_u_kernel and 31.5 for this one, same box - profiles/r07b_variants.txt.)
//   * order per accumulator as in both earlier forms: bias, input k-block (hi*hi, hi*lo, lo*hi), recurrent k-block 1, 2;
//     step 0 without recurrent product: results bit-identical to lstm2_u_kernel.
// Two workgroups per CU, two waves per SIMD from DIFFERENT workgroups: their barriers do not couple.
// grid = (2 ceil(rows / 64), 2 directions, 2 models) - whole 64-row blocks, as the layers around it -, block = 256.
// T is uniform and there is no row guard: the only exit in front of a barrier (T = 1) is taken by the whole workgroup.
// ---------------------------------------------------------------------------------------
constexpr int kL2rThreads = 256;

struct Lstm2RModelParams {
  const void* wfrag;      // [dir][kb 3 (input, rec 0, rec 1)][tile 16][term 2][64 lanes][8 f16], x 2^(E - s)
  const float* bias;      // [dir][tile 16][64 lanes][4], x 2^E, in accumulator layout
  const float* in;        // X1 split planes [tile32][T][kb16 2][term][half][32][8 f16]
  float* out;             // X2 split planes [tile32][T][kb16 8][term][half][32][8 f16], h x 2^13
  float descale;          // 2^-E
};
struct Lstm2RArgs {
  Lstm2RModelParams m[2];
  int T;
  int n_rows;
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int kL2rWFrags = 3 * 16 * 2;                 // 1 KiB fragments of one direction's weights

template <int ACT>
__device__ __forceinline__ void lstm2_r_chain(const Lstm2RModelParams& P, const int T, const int dir, const int tile,
                                              const int lane, const int w, char* hx) {
  const int n = lane & 15, q = lane >> 4;
  const float dsc = P.descale, dsc02 = 0.2f * dsc, dsc2 = 2.885390081777927f * dsc;

  // ---- this wave's weights: fragment (kb, gate g, term) of unit tile w, and its four bias tiles: resident for the launch.
  // Requests in the order of first use: the input block and the bias here, x_0 and x_1 (below), then the recurrent blocks,
  // which step 0 does not need - it runs while they arrive.
  f32x4 Wr[3][4][2];
  f32x4 bias[4];
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc((const char*)P.wfrag + (size_t)dir * kL2rWFrags * 1024, kL2rWFrags * 1024);
  auto load_wblock = [&](int kb) __attribute__((always_inline)) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
        Wr[kb][g][tm] = buf_load16(wrs, (unsigned)lane * 16, (unsigned)(((kb * 16 + g * 4 + w) * 2 + tm) * 1024));
  };
  load_wblock(0);
  {
    const __amdgpu_buffer_rsrc_t brs = make_rsrc(P.bias + (size_t)dir * 16 * 256, 16 * 1024);
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = buf_load16(brs, (unsigned)lane * 16, (unsigned)((g * 4 + w) * 1024));
  }

  const __amdgpu_buffer_rsrc_t xrs = make_rsrc(P.in + (size_t)tile * T * 8 * 128, (unsigned)T * 8 * 512);
  const unsigned xv = (unsigned)((4 * (q >> 1) + (q & 1)) * 512 + n * 16);   // row tile rt: + rt * 256
  auto t_of = [&](int s) __attribute__((always_inline)) { const int sc = s < T ? s : T - 1; return dir ? (T - 1 - sc) : sc; };
  struct XFrag { f32x4 hi, lo; };
  auto load_x = [&](int rt, int s) __attribute__((always_inline)) {
    XFrag x;
    const unsigned so = (unsigned)t_of(s) * 8 * 512;
    x.lo = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, xv + rt * 256 + 1024, so, 0));
    x.hi = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, xv + rt * 256, so, 0));
    return x;
  };
  // output block of unit tile w: kb16 = dir * 4 + w; row tile rt: + rt * 16 rows
  float* const obase = P.out + ((size_t)tile * T * 32 + (dir * 4 + w) * 4 + (q >> 1)) * 128 + n * 4 + (q & 1) * 2;

  f32x4 Z[8];                                          // tile g * 2 + rt
  float c[8];                                          // cell state of (row 16 rt + n, unit 16 w + 4 q + r) at index 4 rt + r
  f16x8 hB[2][2][2];                                   // h_{s-1} x 2^13 as B fragments [rt][kb][term], from LDS
  f16x8 hN[2];                                         // this wave's units of h_s [term], elements 4 rt + r
#pragma unroll
  for (int i = 0; i < 8; ++i) c[i] = 0.f;

  constexpr int GST = 13;
  struct GateSt { float zi, zf, zg, zo, cp, p, t; };
  GateSt gsr;                                          // the element of the row tile in flight
  float hv[4];
  auto gate_stage = [&](int u, int r, int st, int t_out) __attribute__((always_inline)) {   // u: row tile
    const int e = 4 * u + r;
    GateSt& gs = gsr;
    if (st == 0) { gs.zi = Z[0 + u][r]; gs.zf = Z[2 + u][r]; gs.cp = c[e]; }
    else if (st == 1) { gs.zg = Z[4 + u][r]; gs.zo = Z[6 + u][r]; }
    else if (st == 2) {
      if constexpr (ACT == 0) {
        gs.zi = __builtin_fminf(__builtin_fmaxf(__builtin_fmaf(gs.zi, dsc02, 0.5f), 0.0f), 1.0f);
        gs.zf = __builtin_fminf(__builtin_fmaxf(__builtin_fmaf(gs.zf, dsc02, 0.5f), 0.0f), 1.0f);
      } else {
        gs.zi = sigmoid_exact(gs.zi * dsc);
        gs.zf = sigmoid_exact(gs.zf * dsc);
      }
    } else if (st == 3) {
      if constexpr (ACT == 0) gs.zo = __builtin_fminf(__builtin_fmaxf(__builtin_fmaf(gs.zo, dsc02, 0.5f), 0.0f), 1.0f);
      else gs.zo = sigmoid_exact(gs.zo * dsc);
      gs.zg = gs.zg * dsc2;
    } else if (st == 4) gs.zg = __builtin_amdgcn_exp2f(gs.zg);
    else if (st == 5) gs.t = __builtin_amdgcn_rcpf(gs.zg + 1.0f);
    else if (st == 6) gs.p = gs.zi * __builtin_fmaf(gs.t, -2.0f, 1.0f);
    else if (st == 7) {
      const float cn = __builtin_fmaf(gs.zf, gs.cp, gs.p);
      c[e] = cn;
      gs.zg = cn * 2.885390081777927f;
    } else if (st == 8) gs.zg = __builtin_amdgcn_exp2f(gs.zg);
    else if (st == 9) gs.t = __builtin_amdgcn_rcpf(gs.zg + 1.0f);
    else if (st == 10) hv[r] = gs.zo * __builtin_fmaf(gs.t, -2.0f * kHScale, kHScale);   // o tanh(c) 2^13
    else if (st == 11) {
      if (r & 1) {
        const f16x2 hp = __builtin_convertvector(f32x2{hv[r - 1], hv[r]}, f16x2);
        hN[0][4 * u + r - 1] = hp[0];
        hN[0][4 * u + r] = hp[1];
      }
    } else {
      if (r & 1) {
        const int j = 4 * u + r;
        const f16x2 lp = __builtin_convertvector(
            f32x2{hv[r - 1] - (float)hN[0][j - 1], hv[r] - (float)hN[0][j]}, f16x2);
        hN[1][j - 1] = lp[0];
        hN[1][j] = lp[1];
      }
      if (r == 3) {                                    // the row tile is complete: its 4 units are 8 contiguous bytes per term
        float* d = obase + (size_t)t_out * 32 * 128 + u * 16 * 4;
        const f16x8 a = hN[0], b = hN[1];
        const int o = 4 * u;
        *(f16x4*)d = f16x4{a[o], a[o + 1], a[o + 2], a[o + 3]};
        *(f16x4*)(d + 2 * 128) = f16x4{b[o], b[o + 1], b[o + 2], b[o + 3]};
      }
    }
  };
  // piece pc (0 .. 4 GST - 1) of a row tile, element-major: pc = GST r + st.  (Stage-major - the four elements' stages as
  // independent neighbours - was measured in r05: 35.3-36.0 vs 34.9-35.7 us, nothing: the launch is issue-bound.)
  auto gate_piece = [&](int u, int pc, int t_out) __attribute__((always_inline)) { gate_stage(u, pc / GST, pc % GST, t_out); };
  auto gates_plain = [&](int u, int t_out) __attribute__((always_inline)) {
#pragma unroll
    for (int pc = 0; pc < 4 * GST; ++pc) {
      gate_piece(u, pc, t_out);
      if ((pc & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
  };
  constexpr int NGP = 4 * GST;                         // stage pieces of one row tile
  constexpr int PA[3] = {0, 0, 1}, PB[3] = {0, 1, 0};  // (weight term, activation term): hi*hi, hi*lo, lo*hi

  // The two row tiles of a wave are independent chains that share the weights, and they run HALF A STEP APART: while the
  // gates of one (about 85 vector instructions) are computed, the products of the other (12 input + 24 recurrent MFMAs)
  // feed the matrix pipe, so every MFMA has two or three vector instructions behind it and neither kind runs alone:
  //   half A(s): in(rt 1, s),     rec(rt 1, s)      with  gates(rt 0, s)  between them;  h(rt 0, s) through LDS
  //   half B(s): in(rt 0, s + 1), rec(rt 0, s + 1)  with  gates(rt 1, s)  between them;  h(rt 1, s) through LDS
  // The input products stand in front: they do not need h, and cover the LDS round trip behind the barrier.
  // Order inside a half.  Products and gate pieces are pure register arithmetic: nothing in them holds the place they have
  // in the source (with the weights in registers no load stands between them any more), so the interleave is stated to
  // the scheduler instead: a half is one scheduling region, described behind its last instruction as ticks of one MFMA
  // and 2-3 vector / transcendental instructions, and closed by a full barrier.  Independent accumulators take turns
  // (gate g innermost), so no product waits for the one in front of it; per accumulator the order is the one above.
  // in: Z[rp] = b + W^T x (the bias is the C operand of an accumulator's first product);  REC: Z[rp] += U^T h(rp);
  // GATES: the gate pieces of row tile ug != rp.
  auto half = [&](auto rec_tag, auto gates_tag, int ug, int rp, const XFrag& x, int t_out) __attribute__((always_inline)) {
    constexpr bool REC = decltype(rec_tag)::value, GATES = decltype(gates_tag)::value;
    constexpr int NM = 12 + (REC ? 24 : 0);
    auto pieces = [&](int tk) __attribute__((always_inline)) {
      if constexpr (GATES) {
#pragma unroll
        for (int pc = (tk * NGP) / NM; pc < ((tk + 1) * NGP) / NM; ++pc) gate_piece(ug, pc, t_out);
      }
    };
    const f16x8 xb[2] = {__builtin_bit_cast(f16x8, x.hi), __builtin_bit_cast(f16x8, x.lo)};
#pragma unroll
    for (int pr = 0; pr < 3; ++pr)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f16x8 a = __builtin_bit_cast(f16x8, Wr[0][g][PA[pr]]);
        Z[g * 2 + rp] = mfma16_f16(a, xb[PB[pr]], pr == 0 ? bias[g] : Z[g * 2 + rp]);
        pieces(pr * 4 + g);
      }
    if constexpr (REC) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int pr = 0; pr < 3; ++pr)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f16x8 a = __builtin_bit_cast(f16x8, Wr[1 + kb][g][PA[pr]]);
            Z[g * 2 + rp] = mfma16_f16(a, hB[rp][kb][PB[pr]], Z[g * 2 + rp]);
            pieces(12 + (kb * 3 + pr) * 4 + g);
          }
    }
#pragma unroll
    for (int i = 0; i < NM; i += 3) {                                      // 0x008: MFMA, 0x402: VALU | TRANS
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      if constexpr (GATES) __builtin_amdgcn_sched_group_barrier(0x402, 3, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      if constexpr (GATES) __builtin_amdgcn_sched_group_barrier(0x402, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      if constexpr (GATES) __builtin_amdgcn_sched_group_barrier(0x402, 2, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  // h_s of row tile rt: this wave's 4 units per term into the tile's image, one barrier, the whole of it back.
  // image [rt 2][kb 2][term 2][64 lanes][16 B]; this wave's 8 bytes are half w & 1 of k-block w >> 1.  One image per row
  // tile is enough: between two writes of it lies the other row tile's barrier, behind every wave's reads of the first.
  auto exchange = [&](int rt) __attribute__((always_inline)) {
    char* const img = hx + rt * 4 * 1024 + lane * 16;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
      const f16x8 v = hN[tm];
      *(f16x4*)(img + ((w >> 1) * 2 + tm) * 1024 + (w & 1) * 8) = f16x4{v[4 * rt], v[4 * rt + 1], v[4 * rt + 2], v[4 * rt + 3]};
    }
    __syncthreads();
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
        hB[rt][kb][tm] = __builtin_bit_cast(f16x8, *(const f32x4*)(img + (kb * 2 + tm) * 1024));
    __builtin_amdgcn_sched_barrier(0);                 // all four reads at once: the input products that follow cover them
  };
  using No = std::false_type;
  using Yes = std::true_type;

  // prologue: in(0) of both row tiles straight into Z (no gates yet)
  XFrag xn[2];
  {
    const XFrag x0[2] = {load_x(0, 0), load_x(1, 0)};
    xn[0] = load_x(0, 1);
    xn[1] = load_x(1, 1);
    load_wblock(1);
    load_wblock(2);
    half(No{}, No{}, 0, 0, x0[0], 0);
    half(No{}, No{}, 0, 1, x0[1], 0);
  }
  const int t0 = t_of(0);
  if (T == 1) {                                        // uniform: no barrier behind it
    gates_plain(0, t0);
    gates_plain(1, t0);
    return;
  }
  // step 0: h_{-1} = 0, no recurrent product; row tile 1 already has its in(0), so half A is the gates of row tile 0 alone
  gates_plain(0, t0);
  exchange(0);
  half(Yes{}, Yes{}, 1, 0, xn[0], t0);                 // half B(0)
  xn[0] = load_x(0, 2);
  exchange(1);
#pragma unroll 1
  for (int s = 1; s + 1 < T; ++s) {
    const int t = t_of(s);
    half(Yes{}, Yes{}, 0, 1, xn[1], t);                // half A(s)
    xn[1] = load_x(1, s + 1);
    exchange(0);
    half(Yes{}, Yes{}, 1, 0, xn[0], t);                // half B(s)
    xn[0] = load_x(0, s + 2);
    exchange(1);
  }
  // the last step: half A, then the gates of row tile 1 with nothing to hide behind; no hand-over
  {
    const int t = t_of(T - 1);
    half(Yes{}, Yes{}, 0, 1, xn[1], t);
    gates_plain(1, t);
  }
}

template <int ACT>
__global__ void __launch_bounds__(kL2rThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
lstm2_r_kernel(const Lstm2RArgs args) {
  __shared__ __attribute__((aligned(16))) char hx[2 * 4 * 1024];            // 8 KiB: [rt][kb][term][lane][16 B]
  const Lstm2RModelParams& P = args.m[blockIdx.z];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  lstm2_r_chain<ACT>(P, args.T, blockIdx.y, blockIdx.x, lane, wave, hx);
}

}  // namespace nrv
