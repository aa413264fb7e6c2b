// 256->64 Bi-LSTM of the f16x2 mode: lstm_h2s_kernel<64, 0, 64, 2, 1, 1, ...> with weight entries in the wave's idle registers.
#pragma once
#include "nrv_lstm_f16x2s.h"

namespace nrv {

// ---------------------------------------------------------------------------------------
// lstm4_r_kernel: the ownership (4 waves x 16 units x 4 gates x 64 rows, 12 products per weight entry), the schedule
// (rec(s) -> in(s+1) with the gate and copy-out pieces of step s between its products -> Z <- N), the operand layouts
// (pack_lstm_h2s), the raw copy-out, the double-buffered split image of h, the peeled last step and THE ORDER OF EVERY
// ACCUMULATOR'S PRODUCTS are lstm_h2s_kernel's at those template values (nrv_lstm_f16x2s.h, where they are described):
// every output bit is the same.
//
// What differs is where a wave's 40 weight entries (10 k-blocks of 4 entries x 2 terms x 1 KB) come from.  The kernel
// runs one wave per SIMD, so a wave may hold 512 registers, and lstm_h2s_kernel uses 367 of them.  Here
//   * the LAST KBR k-blocks of a step's block sequence - the two recurrent blocks, whose requests sat in the serial
//     phase rec(s) with nothing to hide behind, then the last KBR - 2 input blocks - stay in registers for the whole
//     launch: 8 registers per entry, requested once, behind the products of in(0)'s first entries, in the order of
//     first use; indexed by compile-time entry number only;
//   * the first KBL input blocks stay in LDS (as before);
//   * the blocks between them are streamed from L2 through the ring of NBG entries, LBG = NBG - 1 entries ahead.
// The ring serves the entries [0, NS) only and wraps from NS - 1 to the next step's entry 0, so rec() issues no weight
// request at all and the ring's leads never name a resident entry.
// Shipped: KBL = 3, KBR = 5, NBG = 4 - 24 + 16 entries never requested again, 8 entries = 16 requests per wave and step
// left (lstm_h2s_kernel: 56), 244 + 236 registers, no scratch (sigmoid variant: 238 + 256).  What else was measured
// (DESIGN.md 3): KBR = 4 with the ring of 8, the LDS blocks last instead of first, rings of 5, KBL = 2, the ring's requests
// one at a time inside the product chains, and x once per workgroup through LDS.
// ---------------------------------------------------------------------------------------
#ifndef NRV_L4_KBL
#define NRV_L4_KBL 3
#endif
#ifndef NRV_L4_KBR
#define NRV_L4_KBR 5
#endif
#ifndef NRV_L4_NBG
#define NRV_L4_NBG 4
#endif
constexpr int kL4rThreads = 256;

template <int ACT, int KBL = NRV_L4_KBL, int KBR = NRV_L4_KBR, int NBG = NRV_L4_NBG>
__global__ void __launch_bounds__(kL4rThreads)
lstm4_r_kernel(const LstmH2Args args) {
  constexpr int H = 64, R = 2, NA = 2;
  constexpr int NG = H / 16;                                   // unit groups = waves
  constexpr int KK_IN = 8, KK_REC = H / 32, KK = KK_IN + KK_REC;
  constexpr int RT = 2 * R;                                    // 16-row tiles of a wave
  constexpr int EPK = 4, TPE = 3 * RT;                         // weight entries per k-block / MFMA ticks per entry
  constexpr int ROWS = 32 * R;
  constexpr int GS = ROWS * 8 + 8;                             // f16 per unit group of the h image (8 of padding)
  constexpr int TERM = (H / 8) * GS;                           // f16 per term plane
  constexpr int HBUF = TERM;                                   // floats per image = 2 terms x TERM f16
  constexpr int NTHREADS = kL4rThreads;
  constexpr int LBG = NBG - 1, LA = NA - 1;
  constexpr int NS = EPK * (KK - KBR);                         // entries [0, NS): LDS or ring; [NS, EPK KK): registers
  constexpr int NRES = EPK * KBR;
  static_assert(KBR >= KK_REC && KBL + KBR <= KK, "the recurrent blocks are resident; LDS and register blocks are disjoint");
  static_assert(NS % NBG == 0 && LBG <= NS, "the ring must divide the entries it serves");
  static_assert(NRES <= NS, "the resident entries are requested behind in(0)'s ring-served entries");

  constexpr int NE = RT * 4;                                   // gate elements per lane
  __shared__ __attribute__((aligned(16))) float hbuf[2 * HBUF];
  __shared__ __attribute__((aligned(16))) float wl[KBL > 0 ? NG * KBL * EPK * 512 : 4];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hg = wave;
  const int l15 = lane & 15, kq = lane >> 4;
  const LstmBlock blk = lstm_block();
  if (blk.rowblk >= args.n_blk) return;
  const int dir = blk.dir;
  const LstmH2ModelParams& P = args.m[blk.model];
  const int T = args.T;
  const int row0 = blk.rowblk * ROWS;

  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(
      (const char*)P.wsplit + ((size_t)(dir * NG + hg) * KK) * (EPK * 2 * 1024), KK * EPK * 2 * 1024);
  const unsigned wlane = lane * 16;
  // the bias (x 2^E) rides on the gate constants (see lstm_h2o_kernel)
  const float* bp = P.bias + (size_t)(dir * NG + hg) * 4 * 16 + l15;
  const float dsc = P.descale, dsc02 = 0.2f * dsc, dsc2 = 2.885390081777927f * dsc;
  const float bi = bp[0 * 16] * dsc, bf = bp[1 * 16] * dsc, bg = bp[2 * 16] * dsc, bo = bp[3 * 16] * dsc;
  const float kI = __builtin_fmaf(bi, 0.2f, 0.5f), kF = __builtin_fmaf(bf, 0.2f, 0.5f), kO = __builtin_fmaf(bo, 0.2f, 0.5f),
              kG = bg * 2.885390081777927f;
  const int u0 = hg * 16 + l15;                                // this lane's unit
  const int hw_off = (u0 >> 3) * GS + (4 * kq) * 8 + (u0 & 7);                  // f16; + (16 rt + reg) 8; lo: + TERM
  const int hp_off = kq * GS + l15 * 8;                                         // f16; + kkr 4 GS + rt 128; lo: + TERM

  float* const wlw = wl + (wave * KBL * EPK) * 512 + lane * 4;     // this wave's LDS-resident weight fragments
  if constexpr (KBL > 0) {
#pragma unroll 1
    for (int e0 = 0; e0 < KBL * EPK; e0 += 4) {
      f32x4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = buf_load16(wrs, wlane, ((e0 + j / 2) * 2 + (j & 1)) * 1024);
#pragma unroll
      for (int j = 0; j < 8; ++j) *(f32x4*)(wlw + ((e0 + j / 2) * 2 + (j & 1)) * 256) = v[j];
    }
  }
  for (int i = threadIdx.x; i < HBUF; i += NTHREADS) hbuf[i] = 0.f;          // image of h_{-1} (buffer 0)
  float c[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) c[i] = 0.f;
  __syncthreads();

  struct ABase {
    __amdgpu_buffer_rsrc_t r0[R];
    unsigned v0[R][2];
  };
  auto mk_base = [&](int s) __attribute__((always_inline)) {
    const int sc = s < T ? s : T - 1;                    // a step past the end aliases the last one (requests nobody consumes)
    const int t = dir ? (T - 1 - sc) : sc;
    ABase ab;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      ab.r0[r] = make_rsrc(P.in0.ubase(row0 + r * 32, t), 0xffffffffu);
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
        ab.v0[r][sub] = (P.in0.voff(row0 + r * 32, t, l15 + 16 * sub, kq & 1) + (kq >> 1) * 512) * 4;
    }
    return ab;
  };
  struct BReg { f16x8 t[2]; };
  struct AReg { f32x4 v[2]; };
  BReg b[NBG];                                           // the ring: entries [0, NS)
  BReg wres[NRES];                                       // entry NS + i, for the whole launch
  AReg a[NA][RT];
  auto loadB = [&](int e, BReg& bb) __attribute__((always_inline)) {
    if (e < KBL * EPK) {
      bb.t[0] = __builtin_bit_cast(f16x8, *(const f32x4*)(wlw + (e * 2) * 256));
      bb.t[1] = __builtin_bit_cast(f16x8, *(const f32x4*)(wlw + (e * 2 + 1) * 256));
    } else {
      bb.t[0] = __builtin_bit_cast(f16x8, buf_load16(wrs, wlane, (e * 2) * 1024));
      bb.t[1] = __builtin_bit_cast(f16x8, buf_load16(wrs, wlane, (e * 2 + 1) * 1024));
    }
  };
  auto loadA_in = [&](const ABase& ab, int kk, int rt, AReg& d) __attribute__((always_inline)) {
    const int r = rt >> 1, sub = rt & 1;
    // the lo term first: the block's first product takes the hi term, so ONE counted wait covers both
    d.v[1] = buf_load16(ab.r0[r], ab.v0[r][sub], kk * 4096 + 1024);
    d.v[0] = buf_load16(ab.r0[r], ab.v0[r][sub], kk * 4096);
  };
  auto loadA_rec = [&](const _Float16* hp, int kkr, int rt, AReg& d) __attribute__((always_inline)) {
    const _Float16* qh = hp + kkr * 4 * GS + rt * 128;
    d.v[1] = *(const f32x4*)(qh + TERM);                 // lo first, as for x
    d.v[0] = *(const f32x4*)(qh);
  };
  // one fragment piece at a time, issued BEHIND a product inside a chain of three (tools/microbench/tick_cost.hip)
  auto loadA_in1 = [&](const ABase& ab, int kk, int rt, int term, AReg& d) __attribute__((always_inline)) {
    const int r = rt >> 1, sub = rt & 1;
    d.v[term] = buf_load16(ab.r0[r], ab.v0[r][sub], kk * 4096 + term * 1024);
  };
  auto loadA_rec1 = [&](const _Float16* hp, int kkr, int rt, int term, AReg& d) __attribute__((always_inline)) {
    d.v[term] = *(const f32x4*)(hp + kkr * 4 * GS + rt * 128 + term * TERM);
  };
  constexpr int APPE = (2 * RT + EPK - 1) / EPK;             // fragment pieces (row tile, term) per entry, behind products 4..
  static_assert(4 + APPE <= 3 * RT, "fragment pieces must fit behind an entry's products");
  // hi*lo, lo*hi, hi*hi: the first product of an entry takes the LAST-requested fragment of both operands
  constexpr int PA[3] = {0, 1, 0}, PB[3] = {1, 0, 0};

  // ---- the VALU work of a step, cut into pieces of at most ~5 instructions (see lstm_h2s_kernel) ----
  constexpr int GST = 14;
  struct GateSt { float zi, zf, zg, zo, cp, p, hv, t; _Float16 hh, hl; };
  auto gate_stage = [&](GateSt& g, const f32x4 (&Z)[4][RT], _Float16* hw, int e, int st) __attribute__((always_inline)) {
    const int rt = (e / 4) % RT, reg = e % 4;
    if (st == 0) {
      g.zi = Z[0][rt][reg]; g.zf = Z[1][rt][reg];
      g.cp = c[e];
    } else if (st == 1) {
      g.zg = Z[2][rt][reg]; g.zo = Z[3][rt][reg];
    } else if (st == 2) {
      if constexpr (ACT == 0) {
        g.zi = __builtin_fminf(__builtin_fmaxf(__builtin_fmaf(g.zi, dsc02, kI), 0.0f), 1.0f);
        g.zf = __builtin_fminf(__builtin_fmaxf(__builtin_fmaf(g.zf, dsc02, kF), 0.0f), 1.0f);
      } else {
        g.zi = sigmoid_exact(__builtin_fmaf(g.zi, dsc, bi));
        g.zf = sigmoid_exact(__builtin_fmaf(g.zf, dsc, bf));
      }
    } else if (st == 3) {
      if constexpr (ACT == 0) g.zo = __builtin_fminf(__builtin_fmaxf(__builtin_fmaf(g.zo, dsc02, kO), 0.0f), 1.0f);
      else g.zo = sigmoid_exact(__builtin_fmaf(g.zo, dsc, bo));
      g.zg = __builtin_fmaf(g.zg, dsc2, kG);
    } else if (st == 4) {
      g.zg = __builtin_amdgcn_exp2f(g.zg);
    } else if (st == 5) {
      g.t = __builtin_amdgcn_rcpf(g.zg + 1.0f);
    } else if (st == 6) {
      g.p = g.zi * __builtin_fmaf(g.t, -2.0f, 1.0f);
    } else if (st == 7) {
      const float cn = __builtin_fmaf(g.zf, g.cp, g.p);
      c[e] = cn;
      g.zg = cn * 2.885390081777927f;
    } else if (st == 8) {
      g.zg = __builtin_amdgcn_exp2f(g.zg);
    } else if (st == 9) {
      g.t = __builtin_amdgcn_rcpf(g.zg + 1.0f);
    } else if (st == 10) {
      // og * tanh(c) * 2^13, the scale riding on tanh's last fma
      g.hv = g.zo * __builtin_fmaf(g.t, -2.0f * kHScale, kHScale);
    } else if (st == 11) {
      g.hh = (_Float16)g.hv;
    } else if (st == 12) {
      g.hl = (_Float16)(g.hv - (float)g.hh);
    } else {
      hw[(rt * 16 + reg) * 8] = g.hh;
      hw[(rt * 16 + reg) * 8 + TERM] = g.hl;
    }
  };
  constexpr int ITEMS = (H / 16) * 2 * ROWS;
  constexpr int NIT = ITEMS / NTHREADS;
  static_assert(ITEMS % NTHREADS == 0, "copy-out items must divide evenly");
  constexpr int CST = 4;                                       // stages of one (raw) copy-out item
  struct CopySt { f16x8 hi, lo; float* dst; };
  auto copy_stage = [&](CopySt& k, const _Float16* himg, int t, int i, int st) __attribute__((always_inline)) {
    const int it = threadIdx.x + i * NTHREADS;
    constexpr int KBH = H / 16;
    const int kbh = it / ROWS, rr = it % ROWS;          // kbh = 2*kbo + hf: features 8*kbh .. 8*kbh + 7 = unit group kbh
    if (st == 0) {
      k.hi = *(const f16x8*)(himg + kbh * GS + rr * 8);
      k.lo = *(const f16x8*)(himg + kbh * GS + rr * 8 + TERM);
      const int tile = blk.rowblk * R + rr / 32;
      k.dst = P.out + ((size_t)(tile * T + t) * (2 * H / 4) + (dir * KBH + (kbh >> 1)) * 4 + (kbh & 1)) * 128 + (rr & 31) * 4;
    } else if (st == 1) {
      *(f16x8*)k.dst = k.hi;
    } else if (st == 2) {
      *(f16x8*)(k.dst + 2 * 128) = k.lo;
    }
  };

  // ---- in(): N = x W over the input blocks, one MFMA per TICK of 16 cycles; the gate stages of Z take the
  // ticks [0, TG), the barrier follows tick TG - 1, the copy-out stages take the ticks behind it.
  constexpr int NTICK = KK_IN * EPK * TPE;
  constexpr int NGP = NE * GST, NCP = NIT * CST;               // pieces
  constexpr int TG_WANT = NGP < (2 * NTICK) / 3 ? NGP : (2 * NTICK) / 3;
  constexpr int TG_MAX = (KK_IN - LA) * EPK * TPE;             // the rec() operands are requested from block KK_IN - LA on
  constexpr int TG = TG_WANT < TG_MAX ? TG_WANT : TG_MAX;
  constexpr int TC = NTICK - TG;
  static_assert(TG >= 1 && TC >= 1, "no room for the gates / copy-out in the input phase");
  auto in_phase = [&](auto work_tag, f32x4 (&N)[4][RT], const f32x4 (&Z)[4][RT], const ABase& xb,
                      const _Float16* hp_next, _Float16* himg_w, int t_out, const ABase& xb_wrap) __attribute__((always_inline)) {
    constexpr bool WORK = decltype(work_tag)::value;
    GateSt gs;
    CopySt cs;
    // (N is not zeroed: the first product of every tile takes a constant 0 as its C operand)
#pragma unroll
    for (int kk = 0; kk < KK_IN; ++kk) {
      const int ka = kk + LA;                            // activations LA blocks ahead: input, then recurrent
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        if (ka < KK_IN) loadA_in(xb, ka, rt, a[ka % NA][rt]);
        else if (WORK) loadA_rec(hp_next, ka - KK_IN, rt, a[ka % NA][rt]);
        else loadA_in(xb_wrap, ka - KK_IN, rt, a[ka % NA][rt]);
      }
#pragma unroll
      for (int ge = 0; ge < EPK; ++ge) {
        const int e = EPK * kk + ge, g = ge;
        if (e < NS) loadB((e + LBG) % NS, b[(e + LBG) % NBG]);
        // in(0) only: the register-resident entries, one behind each of its first entries, in the order of first use
        if (!WORK && e < NRES) {
          wres[e].t[0] = __builtin_bit_cast(f16x8, buf_load16(wrs, wlane, ((NS + e) * 2) * 1024));
          wres[e].t[1] = __builtin_bit_cast(f16x8, buf_load16(wrs, wlane, ((NS + e) * 2 + 1) * 1024));
        }
        __builtin_amdgcn_sched_barrier(0);
        const BReg& be = e < NS ? b[e % NBG] : wres[e < NS ? 0 : e - NS];   // (the inner guard only keeps the index in range)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int pr = 0; pr < 3; ++pr) {
            const int tk = (e * RT + rt) * 3 + pr;
            N[g][rt] = mfma16_f16(__builtin_bit_cast(f16x8, a[kk % NA][rt].v[PA[pr]]), be.t[PB[pr]],
                                  (kk == 0 && pr == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : N[g][rt]);
            if constexpr (WORK) {
              if (tk < TG) {
#pragma unroll
                for (int pc = (tk * NGP) / TG; pc < ((tk + 1) * NGP) / TG; ++pc)
                  gate_stage(gs, Z, himg_w + hw_off, pc / GST, pc % GST);
              } else {
#pragma unroll
                for (int pc = ((tk - TG) * NCP) / TC; pc < ((tk - TG + 1) * NCP) / TC; ++pc)
                  copy_stage(cs, himg_w, t_out, pc / CST, pc % CST);
              }
              __builtin_amdgcn_sched_barrier(0);
              if (tk == TG - 1) __syncthreads();         // h_s complete: rec(s+1) operands and the copy-out may read it
            }
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  // ---- rec(): Z += h U over the recurrent blocks: MFMAs on resident weights and the fragment requests of the blocks
  // behind them (the operand arrives split).
  auto rec_phase = [&](f32x4 (&Z)[4][RT], const _Float16* hp, const ABase& xb_next) __attribute__((always_inline)) {
#pragma unroll
    for (int kr = 0; kr < KK_REC; ++kr) {
      const int kk = KK_IN + kr;
      const int ka = kk + LA;
#pragma unroll
      for (int ge = 0; ge < EPK; ++ge) {
        const int e = EPK * kk + ge, g = ge;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int pr = 0; pr < 3; ++pr) {
            Z[g][rt] = mfma16_f16(__builtin_bit_cast(f16x8, a[kk % NA][rt].v[PA[pr]]), wres[e - NS].t[PB[pr]], Z[g][rt]);
            const int m = rt * 3 + pr, pa = ge * APPE + (m - 4);
            if (m >= 4 && m < 4 + APPE && pa < 2 * RT) {
              __builtin_amdgcn_sched_barrier(0);
              const int rn = pa / 2, tn = pa % 2;
              if (ka < KK) loadA_rec1(hp, ka - KK_IN, rn, tn, a[ka % NA][rn]);
              else loadA_in1(xb_next, ka - KK, rn, tn, a[ka % NA][rn]);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  f32x4 Z[4][RT], N[4][RT];
  auto himg = [&](int s) __attribute__((always_inline)) { return (_Float16*)(hbuf + ((s + 1) & 1) * HBUF); };   // image of h_s
  auto t_of = [&](int s) __attribute__((always_inline)) { return dir ? (T - 1 - s) : s; };

  // prologue: the rings' first entries, then in(0) straight into Z
  {
    const ABase x0 = mk_base(0), x1 = mk_base(1);
#pragma unroll
    for (int e = 0; e < LBG; ++e) loadB(e, b[e]);
#pragma unroll
    for (int i = 0; i < LA; ++i)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) loadA_in(x0, i, rt, a[i][rt]);
    in_phase(std::false_type{}, Z, Z, x0, nullptr, nullptr, 0, x1);
  }
  // The resident entries live in the accumulator half of the register file from here on: an MFMA takes its B operand from
  // there as it is.  Left to itself the register allocator treats that half as spill space of the other one and copies
  // 8 registers back in front of every entry's products (64 v_accvgpr_read in rec(), where nothing hides them).
#pragma unroll
  for (int i = 0; i < NRES; ++i) {
    asm volatile("" : "+a"(wres[i].t[0]));
    asm volatile("" : "+a"(wres[i].t[1]));
  }
  // The steps 0 .. T - 2 (rec, then in() of the next step with this step's gates between its products) are the loop;
  // the LAST step (rec, plain gates, copy-out) stands behind it (see lstm_h2s_kernel).
  auto last_step = [&](int s) __attribute__((always_inline)) {
    GateSt gs;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
#pragma unroll
      for (int st = 0; st < GST; ++st) gate_stage(gs, Z, himg(s) + hw_off, e, st);
      if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    CopySt cs;
#pragma unroll
    for (int i = 0; i < NIT; ++i)
#pragma unroll
      for (int st = 0; st < CST; ++st) copy_stage(cs, himg(s), t_of(s), i, st);
  };
#pragma unroll 1
  for (int s = 0; s + 1 < T; ++s) {
    // step s: Z holds x_s W on entry; on exit it holds x_{s+1} W and h_s has been written out
    const ABase xn = mk_base(s + 1);
    if (s > 0) rec_phase(Z, himg(s - 1) + hp_off, xn);
    in_phase(std::true_type{}, N, Z, xn, himg(s) + hp_off, himg(s), t_of(s), xn);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) Z[g][rt] = N[g][rt];
  }
  {
    const int s = T - 1;
    const ABase xn = mk_base(s + 1);
    if (s > 0) rec_phase(Z, himg(s - 1) + hp_off, xn);
    last_step(s);
  }
}

}  // namespace nrv
