// nrv_api.hip - host side of libnanorev_hip.so: weight packing, workspace, launch sequence and
// the C-ABI declared in include/nanorev.h.  gfx950 only; no CPU path.
#include "../../include/nanorev.h"
#include "nrv_kernels.h"
#include "nrv_tailfit.h"      // the training set and the two kernels of a fitting step (nrv_fit_*, opt-in)
#include "nrv_headfit.h"      // ... at depth NRV_FIT_HEAD: lstm4 outputs as the set, the gradient through the three dense layers
#include "nrv_lstm4fit.h"     // ... at depth NRV_FIT_LSTM4: BatchNorm'd lstm3 outputs as the set, the last Bi-LSTM's forward and backward
#include "nrv_lstm3fit.h"     // ... at depth NRV_FIT_LSTM3: lstm3's inputs as the set, the 192->128 Bi-LSTM's forward and backward, dX out of lstm4
#include "nrv_signalfit.h"    // ... at depth NRV_FIT_SIGNAL: lstm2's outputs and the samples as the set, the signal branch's forward and backward, dS out of lstm3
#include "nrv_fullfit.h"      // ... at depth NRV_FIT_FULL: the raw windows as the set, lstm1 and lstm2 forward and backward, all of dXin out of lstm3
#include "nrv_bnfit.h"        // ... nrv_fit_bn_reestimate: the moments of the BatchNorms inside the fitted section, the fit-owned BatchNorm block
#include "nrv_bnaffine.h"     // ... nrv_fit_set_bn_affine: gamma / beta of those BatchNorms as parameters - the sums' epilogue, the refold
#include "nrv_dropout.h"      // ... nrv_fit_set_dropout: the Dropout behind the identity block - the random stream, the unit door's launch
#include "nrv_block.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <chrono>
#include <vector>

using namespace nrv;

// -DNRV_DEV_FAST (tools/lstm_exp.sh D:...): a development build of the f16x2 mode with hard_sigmoid only - a quarter
// of the compile time; the other precision modes and recurrent_act = 1 launch nothing there.  Never the product.
#ifdef NRV_DEV_FAST
#define NRV_ACT1(...)
#else
#define NRV_ACT1(...) __VA_ARGS__
#endif

namespace {

thread_local std::string g_create_error = "";

constexpr int kMaxT = kHeadMaxT;
constexpr int kRowPad = 128;           // workspace rows are padded to a multiple of this
constexpr int kOutBytes = 6 * 4 + 5 * 4 + 1 + 1;   // p1, p2, a1, a2 of one window

// ---- tensor table of one model blob (Keras positional order) --------
struct Blob {
  const float* p;
  std::vector<size_t> off;
  const float* t(int i) const { return p + off[i]; }
};

static std::vector<size_t> tensor_sizes(int T, int C) {
  std::vector<size_t> s;
  auto bn = [&](size_t c) { for (int i = 0; i < 4; ++i) s.push_back(c); };
  auto bil = [&](size_t d, size_t h) {
    for (int i = 0; i < 2; ++i) { s.push_back(d * 4 * h); s.push_back(h * 4 * h); s.push_back(4 * h); }
  };
  s.push_back(24); s.push_back(8); bn(8);
  s.push_back(192); s.push_back(8); bn(8);
  bil(6, 16); bn(32);
  bil(32, 64); bn(128);
  s.push_back(400 * 64); s.push_back(64);
  bil(192, 128); bn(256);
  bil(256, 64);
  s.push_back(128 * 128); s.push_back(128);
  s.push_back(128 * 32); s.push_back(32);
  s.push_back(32 * 6); s.push_back(6);
  s.push_back((size_t)6 * T * 16); s.push_back(16);
  s.push_back((size_t)16 * C); s.push_back(C);
  return s;
}

static bool make_blob(const nrv_weights* w, int T, int C, Blob* b) {
  auto sz = tensor_sizes(T, C);
  size_t tot = 0;
  b->off.clear();
  for (size_t v : sz) { b->off.push_back(tot); tot += v; }
  if (!w || !w->data || (size_t)w->n_f32 != tot) return false;
  b->p = w->data;
  return true;
}

// ---- B-fragment packing ---------------------------------------------------------------------
// The unroll thresholds this file is compiled with (needed by lstm_layer_kernel) also reach the
// HOST optimiser, which would fully unroll the constant-bound packing loops below (an 11-minute
// host compile).  Every loop of the packing code therefore carries an explicit "do not unroll" - the code
// is still optimised otherwise (round 2 had the optimiser off altogether: 0.12 s of packing per nrv_create).
#define NRV_HOST_COLD __attribute__((noinline))
#define NRV_FOR _Pragma("clang loop unroll(disable)") for
// One packed k-group for one 32-column tile: dst[lane][j] = get(k = 8*kg + 4*(lane>>5) + j, lane&31)
template <class G>
NRV_HOST_COLD static void pack_kgroup(float* dst, int kg, G get) {
  NRV_FOR (int lane = 0; lane < 64; ++lane)
    NRV_FOR (int j = 0; j < 4; ++j) dst[lane * 4 + j] = get(8 * kg + 4 * (lane >> 5) + j, lane & 31);
}

// Bi-LSTM layer: [dir][hg][kg][gate][64][4] ; bias [dir][hg][gate][32]
NRV_HOST_COLD static void pack_lstm(const Blob& b, int base, int Kin, int H, std::vector<float>& wpack,
                      std::vector<float>& bias) {
  const int NG = (H + 31) / 32;
  const int KG_IN = (Kin + 7) / 8, KG_REC = H / 8, KG = KG_IN + KG_REC;
  wpack.assign((size_t)2 * NG * KG * 4 * 256, 0.f);
  bias.assign((size_t)2 * NG * 4 * 32, 0.f);
  NRV_FOR (int dir = 0; dir < 2; ++dir) {
    const float* W = b.t(base + dir * 3 + 0);   // (Kin, 4H)
    const float* U = b.t(base + dir * 3 + 1);   // (H, 4H)
    const float* B = b.t(base + dir * 3 + 2);   // (4H)
    NRV_FOR (int hg = 0; hg < NG; ++hg) {
      NRV_FOR (int kg = 0; kg < KG; ++kg)
        NRV_FOR (int g = 0; g < 4; ++g) {
          float* dst = wpack.data() + ((((size_t)(dir * NG + hg) * KG + kg) * 4 + g) * 256);
          pack_kgroup(dst, kg < KG_IN ? kg : kg - KG_IN, [&](int k, int c) -> float {
            int u = hg * 32 + c;
            if (u >= H) return 0.f;
            if (kg < KG_IN) return k < Kin ? W[(size_t)k * 4 * H + g * H + u] : 0.f;
            return U[(size_t)k * 4 * H + g * H + u];
          });
        }
      NRV_FOR (int g = 0; g < 4; ++g)
        NRV_FOR (int c = 0; c < 32; ++c) {
          int u = hg * 32 + c;
          bias[((size_t)(dir * NG + hg) * 4 + g) * 32 + c] = u < H ? B[g * H + u] : 0.f;
        }
    }
  }
}

// ---- split-bf16 packing (lstm_split_kernel) ----------------------------------------------------
static inline uint16_t f32_to_bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float bf16_to_f32_host(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// [dir][hg][kb][gate][term 3][64 lanes][8 bf16], kb = input k-blocks (16 k each) then recurrent;
// lane l holds k = 16*kb + 8*(l>>5) + j, column (gate, unit hg*32 + (l&31)).  Stored as uint16 in a
// float vector (two per float) so it travels with the other packed tensors.
NRV_HOST_COLD static void pack_lstm_split(const Blob& b, int base, int Kin, int H, std::vector<float>& out) {
  const int NG = (H + 31) / 32, KB_IN = Kin / 16, KB = KB_IN + H / 16;
  std::vector<uint16_t> w((size_t)2 * NG * KB * 4 * 3 * 64 * 8, 0);
  NRV_FOR (int dir = 0; dir < 2; ++dir) {
    const float* W = b.t(base + dir * 3 + 0);
    const float* U = b.t(base + dir * 3 + 1);
    NRV_FOR (int hg = 0; hg < NG; ++hg)
      NRV_FOR (int kb = 0; kb < KB; ++kb)
        NRV_FOR (int g = 0; g < 4; ++g)
          NRV_FOR (int lane = 0; lane < 64; ++lane)
            NRV_FOR (int j = 0; j < 8; ++j) {
              const int unit = hg * 32 + (lane & 31);
              float v = 0.f;
              if (unit < H) {
                const int k = 16 * (kb < KB_IN ? kb : kb - KB_IN) + 8 * (lane >> 5) + j;
                v = (kb < KB_IN ? W : U)[(size_t)k * 4 * H + g * H + unit];
              }
              float rem = v;
              NRV_FOR (int tm = 0; tm < 3; ++tm) {
                const uint16_t q = f32_to_bf16_rne(rem);
                rem -= bf16_to_f32_host(q);
                w[((((((size_t)(dir * NG + hg) * KB + kb) * 4 + g) * 3 + tm) * 64) + lane) * 8 + j] = q;
              }
            }
  }
  out.assign((w.size() + 1) / 2, 0.f);
  memcpy(out.data(), w.data(), w.size() * 2);
}


// ---- f16x2 packing (nrv_lstm_f16x2.h) -----------------------------------------------
// largest s with bound * 2^s <= 2^14 (f16 overflows at 65504: two binades of head-room)
static int pow2_room(float bound) {
  if (!(bound > 0.f)) return 14;
  int e;
  (void)std::frexp(bound, &e);                    // bound = m 2^e, m in [0.5, 1)
  return 14 - e;
}
static float max_abs(const float* p, size_t n) {
  float m = 0.f;
  NRV_FOR (size_t i = 0; i < n; ++i) m = std::fmax(m, std::fabs(p[i]));
  return m;
}
// The layer's accumulator exponent E: every operand tensor t enters the matrix pipe as t * 2^(its
// exponent), activations with their buffer's exponent s_in (fixed by the producer), weights with
// E - s_in, so that all products of a layer carry the same 2^E and add up in one accumulator.  E is
// the largest value that keeps every scaled weight block below 2^14.
static int plan_exponent(const Blob& b, int base, int K0, int s0, int K1, int s1, int H) {
  int E = 1 << 20;
  NRV_FOR (int dir = 0; dir < 2; ++dir) {
    const float* W = b.t(base + dir * 3 + 0);
    const float* U = b.t(base + dir * 3 + 1);
    E = std::min(E, s0 + pow2_room(max_abs(W, (size_t)K0 * 4 * H)));
    if (K1) E = std::min(E, s1 + pow2_room(max_abs(W + (size_t)K0 * 4 * H, (size_t)K1 * 4 * H)));
    E = std::min(E, 13 + pow2_room(max_abs(U, (size_t)H * 4 * H)));
  }
  return E;
}
static inline void split_f16(float v, uint16_t* hi, uint16_t* lo) {
  const _Float16 h = (_Float16)v;                 // round to nearest even
  const _Float16 l = (_Float16)(v - (float)h);
  memcpy(hi, &h, 2);
  memcpy(lo, &l, 2);
}
// lstm_h2s_kernel (16x16x32 tiles): [dir][wave group of 16 uh units][kk 32-k blocks: input, then recurrent]
// [gate][unit half][term][64 lanes][8 f16]; lane l: k = 32 kk + 8 (l >> 4) + j, unit = 16 (wg uh + h) + (l & 15).
NRV_HOST_COLD static void pack_lstm_h2s(const Blob& b, int base, int K0, int s0, int K1, int s1, int H, int E,
                                        std::vector<float>& out, std::vector<float>& bias, int uh) {
  const int Kin = K0 + K1;
  const int NG = H / (16 * uh), KK_IN = Kin / 32, KK = KK_IN + H / 32, epk = 4 * uh;
  std::vector<uint16_t> w((size_t)2 * NG * KK * epk * 2 * 64 * 8, 0);
  bias.assign((size_t)2 * NG * 4 * 16 * uh, 0.f);
  NRV_FOR (int dir = 0; dir < 2; ++dir) {
    const float* W = b.t(base + dir * 3 + 0);
    const float* U = b.t(base + dir * 3 + 1);
    const float* B = b.t(base + dir * 3 + 2);
    NRV_FOR (int wg = 0; wg < NG; ++wg) {
      NRV_FOR (int kk = 0; kk < KK; ++kk)
        NRV_FOR (int g = 0; g < 4; ++g)
          NRV_FOR (int h = 0; h < uh; ++h)
            NRV_FOR (int lane = 0; lane < 64; ++lane)
              NRV_FOR (int j = 0; j < 8; ++j) {
                const int unit = 16 * (wg * uh + h) + (lane & 15);
                const int k = 32 * (kk < KK_IN ? kk : kk - KK_IN) + 8 * (lane >> 4) + j;
                float v;
                if (kk < KK_IN) v = std::ldexp(W[(size_t)k * 4 * H + g * H + unit], E - (k < K0 ? s0 : s1));
                else v = std::ldexp(U[(size_t)k * 4 * H + g * H + unit], E - 13);
                const size_t o = ((((((size_t)(dir * NG + wg) * KK + kk) * 4 + g) * uh + h) * 2) * 64 + lane) * 8 + j;
                split_f16(v, &w[o], &w[o + 64 * 8]);
              }
      NRV_FOR (int g = 0; g < 4; ++g)
        NRV_FOR (int c = 0; c < 16 * uh; ++c)
          bias[((size_t)(dir * NG + wg) * 4 + g) * 16 * uh + c] = std::ldexp(B[g * H + wg * 16 * uh + c], E);
    }
  }
  out.assign((w.size() + 1) / 2, 0.f);
  memcpy(out.data(), w.data(), w.size() * 2);
}

// lstm2_r_kernel (nrv_lstm2_u.h): the 32->64 layer's weights as A operands of the transposed product.
// [dir][kb 3: input, recurrent 0, recurrent 1][tile mt 16][term 2][64 lanes][8 f16]; tile mt = gate g * 4 + unit tile ut;
// lane l = (m = l & 15, q = l >> 4) holds gate-unit (g, u = 16 ut + m) for the k slots 8 q + j:
//   input block      feature 8 q + j                                   x 2^(E - s_in)
//   recurrent block  unit 16 (2 (kb - 1) + (j >> 2)) + 4 q + (j & 3)   x 2^(E - 13)   (the order in which a lane holds h)
// bias [dir][mt][64 lanes][4] x 2^E in accumulator layout: register r of lane (n, q) is unit 16 ut + 4 q + r.
NRV_HOST_COLD static void pack_lstm2_t(const Blob& b, int base, int s_in, int E, std::vector<float>& out,
                                       std::vector<float>& bias) {
  constexpr int H = 64, Kin = 32;
  std::vector<uint16_t> w((size_t)2 * 3 * 16 * 2 * 64 * 8, 0);
  bias.assign((size_t)2 * 16 * 64 * 4, 0.f);
  NRV_FOR (int dir = 0; dir < 2; ++dir) {
    const float* W = b.t(base + dir * 3 + 0);
    const float* U = b.t(base + dir * 3 + 1);
    const float* B = b.t(base + dir * 3 + 2);
    NRV_FOR (int kb = 0; kb < 3; ++kb)
      NRV_FOR (int mt = 0; mt < 16; ++mt)
        NRV_FOR (int lane = 0; lane < 64; ++lane)
          NRV_FOR (int j = 0; j < 8; ++j) {
            const int g = mt >> 2, ut = mt & 3, u = 16 * ut + (lane & 15), q = lane >> 4;
            float v;
            if (kb == 0) {
              const int f = 8 * q + j;
              v = f < Kin ? std::ldexp(W[(size_t)f * 4 * H + g * H + u], E - s_in) : 0.f;
            } else {
              const int uk = 16 * (2 * (kb - 1) + (j >> 2)) + 4 * q + (j & 3);
              v = std::ldexp(U[(size_t)uk * 4 * H + g * H + u], E - 13);
            }
            const size_t o = ((((size_t)(dir * 3 + kb) * 16 + mt) * 2) * 64 + lane) * 8 + j;
            split_f16(v, &w[o], &w[o + 64 * 8]);
          }
    NRV_FOR (int mt = 0; mt < 16; ++mt)
      NRV_FOR (int lane = 0; lane < 64; ++lane)
        NRV_FOR (int r = 0; r < 4; ++r) {
          const int g = mt >> 2, ut = mt & 3, q = lane >> 4;
          bias[(((size_t)dir * 16 + mt) * 64 + lane) * 4 + r] = std::ldexp(B[g * H + 16 * ut + 4 * q + r], E);
        }
  }
  out.assign((w.size() + 1) / 2, 0.f);
  memcpy(out.data(), w.data(), w.size() * 2);
}

// head_mlp_split_kernel: the three per-timestep dense layers as A operands of the transposed
// product, 126 fragments [64 lanes][8 bf16] (x3 terms): lane l, element j of a fragment hold
// W[f][n] with n = 32*mt + (l&31) and f the input feature that the B operand carries in slot
// (h = l>>5, j):  dense1 (B from the tiled input)            f = 16*kb + 8*h + j
//                 dense2 / main_out (B = accumulator regs)   reg = 8*(kb&1) + j,
//                                                            f = 32*(kb>>1) + (reg&3) + 8*(reg>>2) + 4*h
NRV_HOST_COLD static void pack_head_split(const Blob& b, std::vector<float>& out, std::vector<float>& bias) {
  std::vector<uint16_t> w((size_t)126 * 512, 0);
  auto emit = [&](int fragbase, float v, int lane, int j) {
    float rem = v;
    NRV_FOR (int tm = 0; tm < 3; ++tm) {
      const uint16_t q = f32_to_bf16_rne(rem);
      rem -= bf16_to_f32_host(q);
      w[((size_t)(fragbase + tm) * 64 + lane) * 8 + j] = q;
    }
  };
  const float *W1 = b.t(50), *W2 = b.t(52), *W3 = b.t(54);
  NRV_FOR (int lane = 0; lane < 64; ++lane)
    NRV_FOR (int j = 0; j < 8; ++j) {
      const int h = lane >> 5, n = lane & 31;
      NRV_FOR (int mt = 0; mt < 4; ++mt)
        NRV_FOR (int kb = 0; kb < 8; ++kb)
          emit((mt * 8 + kb) * 3, W1[(size_t)(16 * kb + 8 * h + j) * 128 + mt * 32 + n], lane, j);
      NRV_FOR (int kb = 0; kb < 8; ++kb) {
        const int reg = 8 * (kb & 1) + j, f = 32 * (kb >> 1) + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        emit(96 + kb * 3, W2[(size_t)f * 32 + n], lane, j);
      }
      NRV_FOR (int kb = 0; kb < 2; ++kb) {
        const int reg = 8 * kb + j, f = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        emit(120 + kb * 3, n < 6 ? W3[(size_t)f * 6 + n] : 0.f, lane, j);
      }
    }
  out.assign(w.size() / 2, 0.f);
  memcpy(out.data(), w.data(), w.size() * 2);
  bias.assign(192, 0.f);
  memcpy(bias.data(), b.t(51), 128 * 4);
  memcpy(bias.data() + 128, b.t(53), 32 * 4);
  memcpy(bias.data() + 160, b.t(55), 6 * 4);
}

// cnn_kernel<true>: dense 400->64 as split-bf16 B fragments [kb 25][nh 2][term 3][64 lanes][8 bf16];
// lane l, element j hold W[k][n] with k = 16*kb + 8*(l>>5) + j (flatten index p*8+o), n = 32*nh + (l&31).
NRV_HOST_COLD static void pack_cnn_split(const float* W, std::vector<float>& out) {
  std::vector<uint16_t> w((size_t)25 * 2 * 3 * 512, 0);
  NRV_FOR (int kb = 0; kb < 25; ++kb)
    NRV_FOR (int nh = 0; nh < 2; ++nh)
      NRV_FOR (int lane = 0; lane < 64; ++lane)
        NRV_FOR (int j = 0; j < 8; ++j) {
          float rem = W[(size_t)(16 * kb + 8 * (lane >> 5) + j) * 64 + 32 * nh + (lane & 31)];
          NRV_FOR (int tm = 0; tm < 3; ++tm) {
            const uint16_t q = f32_to_bf16_rne(rem);
            rem -= bf16_to_f32_host(q);
            w[((size_t)((kb * 2 + nh) * 3 + tm) * 64 + lane) * 8 + j] = q;
          }
        }
  out.assign(w.size() / 2, 0.f);
  memcpy(out.data(), w.data(), w.size() * 2);
}

// head_h2_kernel: the three per-timestep dense layers as f16x2 A operands of the transposed product,
// 42 fragments x 2 terms [64 lanes][8 f16], in the k order of pack_head_split (dense1: f = 16*kb + 8*h + j;
// dense2 / main_out: reg = 8*(kb&1) + j, f = 32*(kb>>1) + (reg&3) + 8*(reg>>2) + 4*h), each layer's weights
// x 2^u, biases x 2^E.  The scales: the input is h x 2^13 (|h| < 1); layer outputs are bounded by
// sum|W| * (input bound) + |b|, which fixes the exponent s that brings them into the f16 range;
// E1 = 13 + u1, E2 = s1 + u2, E3 = s2 + u3 are the accumulator exponents.
struct HeadH2Scales { float c12, c23, c3o; };
NRV_HOST_COLD static HeadH2Scales pack_head_h2(const Blob& b, std::vector<float>& out, std::vector<float>& bias) {
  const float *W1 = b.t(50), *B1 = b.t(51), *W2 = b.t(52), *B2 = b.t(53), *W3 = b.t(54), *B3 = b.t(55);
  const int u1 = pow2_room(max_abs(W1, 128 * 128)), u2 = pow2_room(max_abs(W2, 128 * 32)), u3 = pow2_room(max_abs(W3, 32 * 6));
  float bound1 = 0.f, bound2 = 0.f;
  NRV_FOR (int n = 0; n < 128; ++n) {
    float a = std::fabs(B1[n]);
    NRV_FOR (int k = 0; k < 128; ++k) a += std::fabs(W1[(size_t)k * 128 + n]);
    bound1 = std::fmax(bound1, a);
  }
  NRV_FOR (int n = 0; n < 32; ++n) {
    float a = std::fabs(B2[n]);
    NRV_FOR (int k = 0; k < 128; ++k) a += std::fabs(W2[(size_t)k * 32 + n]) * bound1;
    bound2 = std::fmax(bound2, a);
  }
  const int s1 = pow2_room(bound1), s2 = pow2_room(bound2);
  const int E1 = 13 + u1, E2 = s1 + u2, E3 = s2 + u3;
  std::vector<uint16_t> w((size_t)84 * 512, 0);
  auto emit = [&](int fragbase, float v, int lane, int j) {
    const size_t o = ((size_t)fragbase * 64 + lane) * 8 + j;
    split_f16(v, &w[o], &w[o + 512]);
  };
  NRV_FOR (int lane = 0; lane < 64; ++lane)
    NRV_FOR (int j = 0; j < 8; ++j) {
      const int h = lane >> 5, n = lane & 31;
      NRV_FOR (int mt = 0; mt < 4; ++mt)
        NRV_FOR (int kb = 0; kb < 8; ++kb)
          emit((mt * 8 + kb) * 2, std::ldexp(W1[(size_t)(16 * kb + 8 * h + j) * 128 + mt * 32 + n], u1), lane, j);
      NRV_FOR (int kb = 0; kb < 8; ++kb) {
        const int reg = 8 * (kb & 1) + j, f = 32 * (kb >> 1) + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        emit(64 + kb * 2, std::ldexp(W2[(size_t)f * 32 + n], u2), lane, j);
      }
      NRV_FOR (int kb = 0; kb < 2; ++kb) {
        const int reg = 8 * kb + j, f = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        emit(80 + kb * 2, n < 6 ? std::ldexp(W3[(size_t)f * 6 + n], u3) : 0.f, lane, j);
      }
    }
  out.assign(w.size() / 2, 0.f);
  memcpy(out.data(), w.data(), w.size() * 2);
  bias.assign(192, 0.f);
  NRV_FOR (int i = 0; i < 128; ++i) bias[i] = std::ldexp(B1[i], E1);
  NRV_FOR (int i = 0; i < 32; ++i) bias[128 + i] = std::ldexp(B2[i], E2);
  NRV_FOR (int i = 0; i < 6; ++i) bias[160 + i] = std::ldexp(B3[i], E3);
  return HeadH2Scales{std::ldexp(1.f, s1 - E1), std::ldexp(1.f, s2 - E2), std::ldexp(1.f, -E3)};
}


// lstm1 (6 -> 16) for the 16x16x4 kernel.  Per direction [6][gate 4][64 lanes]:
//   input k-step s (0,1):   W[k = 4s + (lane>>4)][g*16 + (lane&15)]       (k >= 6 -> 0)
//   recurrent step s (0..3): U[unit = 4*(lane>>4) + s][g*16 + (lane&15)]  (lane quarter q holds the
//                            A values h[row][4q..4q+3], so k-step s pairs unit 4q+s)
NRV_HOST_COLD static void pack_lstm1_16(const Blob& b, int base, std::vector<float>& wpack, std::vector<float>& bias) {
  const int H = 16, Kin = 6;
  wpack.assign((size_t)2 * 6 * 4 * 64, 0.f);
  bias.assign((size_t)2 * 4 * 16, 0.f);
  NRV_FOR (int dir = 0; dir < 2; ++dir) {
    const float* W = b.t(base + dir * 3 + 0);
    const float* U = b.t(base + dir * 3 + 1);
    const float* B = b.t(base + dir * 3 + 2);
    NRV_FOR (int g = 0; g < 4; ++g) {
      NRV_FOR (int lane = 0; lane < 64; ++lane) {
        const int q = lane >> 4, c = lane & 15;
        NRV_FOR (int s = 0; s < 2; ++s) {
          int k = 4 * s + q;
          wpack[(((size_t)dir * 6 + s) * 4 + g) * 64 + lane] = k < Kin ? W[(size_t)k * 4 * H + g * H + c] : 0.f;
        }
        NRV_FOR (int s = 0; s < 4; ++s) {
          int u = 4 * q + s;
          wpack[(((size_t)dir * 6 + 2 + s) * 4 + g) * 64 + lane] = U[(size_t)u * 4 * H + g * H + c];
        }
      }
      NRV_FOR (int c = 0; c < 16; ++c) bias[((size_t)dir * 4 + g) * 16 + c] = B[g * H + c];
    }
  }
}

// Dense (K x N row-major) -> [ntile][kg][64][4], columns >= N zero
NRV_HOST_COLD static void pack_dense(const float* W, int K, int N, std::vector<float>& out) {
  const int NT = (N + 31) / 32, KG = (K + 7) / 8;
  out.assign((size_t)NT * KG * 256, 0.f);
  NRV_FOR (int nt = 0; nt < NT; ++nt)
    NRV_FOR (int kg = 0; kg < KG; ++kg)
      pack_kgroup(out.data() + ((size_t)nt * KG + kg) * 256, kg, [&](int k, int c) -> float {
        int col = nt * 32 + c;
        return (k < K && col < N) ? W[(size_t)k * N + col] : 0.f;
      });
}

// Dense (K x N row-major) for the 16x16x4 MFMA: [ct][kg][64][4], K multiple of 16,
//   pack[lane][j] = W[16*kg + 4*(lane>>4) + j][16*ct + (lane&15)]
NRV_HOST_COLD static void pack_dense16(const float* W, int K, int N, std::vector<float>& out) {
  const int CT = (N + 15) / 16, KG = (K + 15) / 16;
  out.assign((size_t)CT * KG * 256, 0.f);
  NRV_FOR (int ct = 0; ct < CT; ++ct)
    NRV_FOR (int kg = 0; kg < KG; ++kg)
      NRV_FOR (int lane = 0; lane < 64; ++lane)
        NRV_FOR (int j = 0; j < 4; ++j) {
          int k = 16 * kg + 4 * (lane >> 4) + j, col = 16 * ct + (lane & 15);
          out[((size_t)ct * KG + kg) * 256 + lane * 4 + j] = (k < K && col < N) ? W[(size_t)k * N + col] : 0.f;
        }
}

// Keras inference BatchNorm as scale/shift:  x*inv + (beta - mean*inv), inv = gamma/sqrt(var+eps)
static void bn_fold(const float* g, const float* be, const float* mu, const float* var, int n,
                    float* scale, float* shift) {
  NRV_FOR (int i = 0; i < n; ++i) {
    float inv = g[i] / std::sqrt(var[i] + 1e-3f);
    scale[i] = inv;
    shift[i] = be[i] - mu[i] * inv;
  }
}

// the five BatchNorms nrv_fit_bn_* knows, in tensor order: first tensor (gamma), channels, first channel of the block's kBnCh
static const struct { int tensor, C, at; } kFitBn[5] = {{2, 8, 0}, {8, 8, 8}, {18, 32, 16}, {28, 128, 48}, {40, 256, 176}};

// The fit depths of nrv_fit_*, in depth order: everything that differs between them on the host.  The set of a depth is its row
// arrays, each [rows][T][per_t] f32 and either one per model or one shared by both, and y per model; the doors take and return
// them in this order, a per-model array as two pointers.
struct FitDepth {
  int code;                                  // NRV_FIT_*
  const char *name, *code_name, *suffix;     // in messages; the constant's name; of the nrv_fit_set_rows* / _get_rows* doors
  const char* phrase;                        // "rows are ..."
  int n_arrays;
  struct { int per_t; bool shared; } arrays[2];
  int (*params)(int T, int C);               // the length of a model's vector
  int64_t max_rows;                          // the row cap's default ...
  const char *env, *at;                      // ... its environment variable, and how a cap message names the depth
  bool mlp, l4, l3, sg, rd;                  // inside the fitted section: the head MLP, lstm4, lstm3, the signal branch, the read branch
  int n_bn, bn[5];                           // the BatchNorms inside it, as indices into kFitBn, in tensor order
};
static const FitDepth kFitDepths[6] = {
    {NRV_FIT_TAIL, "tail", "NRV_FIT_TAIL", "", "main_out values", 1, {{6, false}}, [](int T, int C) { return NRV_FIT_PARAMS(T, C); },
     (int64_t)1 << 24, "NRV_FIT_MAX_ROWS", "", false, false, false, false, false, 0, {}},
    {NRV_FIT_HEAD, "head", "NRV_FIT_HEAD", "_head", "lstm4 outputs", 1, {{128, false}},
     [](int T, int C) { return NRV_FIT_PARAMS_HEAD(T, C); }, (int64_t)1 << 21, "NRV_FIT_MAX_HEAD_ROWS", " at head depth", true, false, false,
     false, false, 0, {}},
    {NRV_FIT_LSTM4, "lstm4", "NRV_FIT_LSTM4", "_lstm4", "BatchNorm'd lstm3 outputs", 1, {{256, false}},
     [](int T, int C) { return NRV_FIT_PARAMS_LSTM4(T, C); }, (int64_t)1 << 20, "NRV_FIT_MAX_LSTM4_ROWS", " at lstm4 depth", true, true, false,
     false, false, 0, {}},
    {NRV_FIT_LSTM3, "lstm3", "NRV_FIT_LSTM3", "_lstm3", "lstm3's inputs", 1, {{192, false}},
     [](int T, int C) { return NRV_FIT_PARAMS_LSTM3(T, C); }, (int64_t)1 << 20, "NRV_FIT_MAX_LSTM3_ROWS", " at lstm3 depth", true, true, true,
     false, false, 1, {4}},
    {NRV_FIT_SIGNAL, "signal", "NRV_FIT_SIGNAL", "_signal", "lstm2 outputs and samples", 2, {{128, false}, {kSig, true}},
     [](int T, int C) { return NRV_FIT_PARAMS_SIGNAL(T, C); }, (int64_t)1 << 20, "NRV_FIT_MAX_SIGNAL_ROWS", " at signal depth", true, true, true,
     true, false, 3, {0, 1, 4}},
    {NRV_FIT_FULL, "full", "NRV_FIT_FULL", "_full", "samples and read features", 2, {{kSig, true}, {kFeat, true}},
     [](int T, int C) { return NRV_FIT_PARAMS_FULL(T, C); }, (int64_t)1 << 22, "NRV_FIT_MAX_FULL_ROWS", " at full depth", true, true, true,
     true, true, 5, {0, 1, 2, 3, 4}},
};
// the descriptor of a depth code, null for a number that is no depth
static const FitDepth* fit_desc(int depth) {
  for (const FitDepth& D : kFitDepths)
    if (D.code == depth) return &D;
  return nullptr;
}

struct DevModel {
  float* all = nullptr;       // one allocation holding every packed tensor of the model
  size_t n = 0;
  // offsets (floats) into `all`
  size_t conv, dpack, dbias, dsplit;
  size_t l_w[4], l_b[4], l_s[4], l_h[4];
  size_t l1w16, l1b16;        // lstm1 packed for the 16x16x4 kernel
  size_t l_ws[4];             // lstm2..4 weights split into three bf16 terms (index 1..3)
  size_t d1p, d1b, d2p, d2b, mop, mob, fw, fb, ow, ob;
  size_t l3raw = 0;           // tensors 34 .. 39 as the file has them (... at depth NRV_FIT_LSTM3)
  size_t sdraw = 0;           // tensor 32 as the file has it (... at depth NRV_FIT_SIGNAL)
  size_t l1raw = 0, l2raw = 0;   // tensors 12 .. 17 and 22 .. 27 as the file has them (... at depth NRV_FIT_FULL)
  size_t l4raw = 0;           // tensors 44 .. 49 as the file has them (nrv_fit_begin at depth NRV_FIT_LSTM4 starts from them)
  // host copies of the five BatchNorms' gamma, beta, moving mean and moving variance, kBnCh channels each in the order of the
  // fit's BatchNorm block: what nrv_fit_bn_reestimate folds new statistics with
  std::vector<float> bn_raw[4];
  size_t h_ws, h_wb;          // head_mlp_split_kernel: split weights / biases
  // f16x2 mode (nrv_lstm_f16x2.h): lstm2..4 weights as two f16 terms, scaled biases, output scale /
  // shift with the buffer exponents folded in, the producers' scaled epilogue constants
  size_t l_s2[4], l_h2[4];
  // layers 2, 3 (192->128, 256->64) with the BatchNorm IN FRONT of them folded into their weights and bias:
  // their BatchNorm'd input segment is then the raw h x 2^13 of the layer before (lstm2_r / lstm_h2s RAW copy-out)
  size_t l_w2sf[4] = {0, 0, 0, 0}, l_b2sf[4] = {0, 0, 0, 0};
  float descale_f[4] = {1.f, 1.f, 1.f, 1.f};
  size_t l2t_w = 0, l2t_b = 0;      // lstm2_r_kernel: transposed fragments / bias image of the 32->64 layer
  float descale[4];
  size_t l1s2, l1h2;
  size_t cr_dbias = 0;                   // cnn_r_kernel: dense bias x 2^16
  size_t cr_w2 = 0, cr_ep = 0, cr_d = 0; // cnn_r_kernel: conv2 in its two-position form, epilogue constants, dense A fragments
  size_t fw8 = 0;                        // head_h2_kernel: feature kernel as its LDS image [16][T][8]
  CnnRConsts cr_k;                       // ... and the first convolution's constants (kernel arguments)
  size_t h_w2, h_b2;          // head_h2_kernel: f16x2 weights, scaled biases
  HeadH2Scales hsc;
  int C;
};

// ---- a merged raw-read call (nrv_revise_reads_raw*_begin; nrv_merge_calls* is its test twin) -------------------------------
// The merged block of a call of N events, n windows, n_reads reads - offsets into one device allocation:
//   [off i64 x (n_reads + 1) | seq | qual | report u64 x n_reads x 24 | edit_off i64 x (n_reads + 1) | rec_off i64 x (n_reads + 1) |
//    profile u64 x n_reads x 48 | trim i64 x n_reads x 2 | accu u64 x n_reads x 4 | ecls u64 x n_reads x 6 |
//    infx u64 x n_reads x 18 | scor u64 x n_reads x 248]
//                                     what comes back in one copy of `dl` bytes, mirrored in page-locked memory (nrv_merge.h,
//                                     nrv_report.h, nrv_edits.h, nrv_pack.h, nrv_profile.h, nrv_trim.h, nrv_align.h, nrv_errclass.h, nrv_infix.h, nrv_score.h); the report,
//                                     edit_off, rec_off, the profile, the trim, the accuracy, the error classes, the infix block and the score only where asked for - without
//                                     them the layout is the merge's own.  A records call that hands back neither seq nor qual leaves those two on
//                                     the device
//   [rec u32 x N | tile u64]          the merge kernels' scratch
//   [edits nrv_edit x n | etile u64]  the edit records, fetched by their used prefix in a copy of their own, and their scratch;
//                                     only where asked for
//   [blob]                            the FASTA / FASTQ records of blob_cap bytes, fetched by their used prefix like the edit
//                                     records; only where asked for
//   [tq u8 x (N + n) | acc u64 x n_reads x 2]   the trim kernels' scratch: Phred per output character, the bounds' accumulators;
//                                     only where asked for
//   [hc u8 x N | hc u8 x (N + n)]     the alignment's stripe carries, one byte per character of the original and of the revised
//                                     reads; only where asked for
//   [hc8 i64 x N | hc8 i64 x (N + n)] the error classes' stripe carries, one packed cell per character of the original and of the
//                                     revised reads; only where asked for
//   [hci i64 x N x 2 | hci i64 x (N + n) x 2]  the infix block's stripe carries, the same per strand; only where asked for
// Every part is 256-byte aligned.
struct MergeLayout { size_t seq, qual, rep, eoff, roff, prof, trim, rec, tile, edits, etile, blob, tq, acc, dl, bytes, accu, hc, ecls, hc8, infx, hci, scor; };

// What a merged call reads besides the raw reads.  Consumed inside _begin: the caller's pointers are dead once it returns, so
// nothing that outlives _begin keeps one (the slot keeps the VALUES of both threshold sets for the re-run of nrv_reads_raw_end)
struct MergeIn {
  const uint8_t* bases = nullptr;
  const float* q_thr = nullptr;         // null: FASTA
  const uint8_t* names = nullptr;       // nrv_revise_reads_raw_records_begin
  const int64_t* name_off = nullptr;
  const float* prof_thr = nullptr;      // nrv_revise_reads_raw_profile_begin: its own 39 thresholds
  const float* trim_thr = nullptr;      // nrv_revise_reads_raw_trim_begin: its own 39 thresholds, and the rule
  int Q = 0, W = 0;
  int64_t min_len = 0;
  const uint8_t* truth = nullptr;       // nrv_revise_reads_raw_accuracy_begin: the true sequences and [n_reads + 1]
  const int64_t* truth_off = nullptr;
  const uint8_t* labels = nullptr;      // nrv_revise_reads_raw_score_begin: one label byte per event and its own 39 thresholds
  const float* score_thr = nullptr;
};
// The trim's rule as the kernels take it: the VALUES a slot keeps for the re-run are of this form too (thr points into the slot)
struct TrimRule { const float* thr = nullptr; int Q = 0, W = 0; int64_t min_len = 0; };
// What a merged call hands back and where: the caller keeps these arrays alive until _end.  A null pointer: not asked for.
// The entry points fill it (and MergeIn, and RawIn) as a positional aggregate: the ORDER of the members is relied on
struct MergeOut {
  uint8_t *seq = nullptr, *qual = nullptr;
  int64_t* off = nullptr;               // every merged call has it: null = not a merged call
  uint64_t* report = nullptr;           // [n_reads][24], and the near-tie margin
  float tie_eps = 0.f;
  nrv_edit* edits = nullptr;            // [max(N - T, 0)] and [n_reads + 1]; edit_off decides
  int64_t* edit_off = nullptr;
  uint8_t* blob = nullptr;              // the records and [n_reads + 1]; rec_off decides
  int64_t* rec_off = nullptr;
  uint64_t* profile = nullptr;          // [n_reads][48]
  int64_t* trim = nullptr;              // [n_reads][2]
  uint64_t* accuracy = nullptr;         // [n_reads][4]
  uint64_t* errclass = nullptr;         // [n_reads][6]
  uint64_t* infix = nullptr;            // [n_reads][18]
  int strands = 2;                      // of the infix block: 1 (forward) or 2
  uint64_t* score = nullptr;            // [n_reads][248]
  bool wants_truth() const { return accuracy != nullptr || errclass != nullptr || infix != nullptr; }
};
// Where a merged call's inputs lie on the device, and its merged block
struct MergeView {
  const SegRead* reads;
  int n_reads;
  int64_t N;
  const unsigned char* bases;
  const signed char *a1, *a2;
  const float *p1, *p2;                  // both null: the call has no rows (nrv_merge_calls* without them)
  const long long* name_off;             // records only
  const unsigned char* names;
  char* blk;                             // MergeLayout offsets count from here
  const unsigned char* truth = nullptr;  // accuracy and error classes only
  const long long* truth_off = nullptr;
  const unsigned char* labels = nullptr; // the score only
};
// The quality rule: characters get a Phred quality when there are thresholds and somebody reads it - the caller's qual or the
// FASTQ records (nrv_merge_calls* has no records: q_thr && qual there)
static bool wants_quality(const float* q_thr, const MergeOut& o) { return q_thr && (o.qual || o.rec_off); }

}  // namespace

struct nrv_handle {
  int device = 0, T = 0, act = 0, batch = 4096;
  hipStream_t own_stream = nullptr, stream = nullptr;

  DevModel dm[2];
  // workspace (per model)
  int cap_rows = 0;                // padded rows the workspace holds
  float *S[2] = {0, 0}, *X1[2] = {0, 0}, *X2[2] = {0, 0}, *X3[2] = {0, 0}, *MO[2] = {0, 0};
  size_t act_n[5] = {0, 0, 0, 0, 0};   // floats of each buffer of the activation set above (S, X1, X2, X3, MO; for_groups swaps it)
  // NRV_POISON=<32-bit hex> (read by nrv_create, per handle): a DEBUG switch.  Every workspace, staging and output buffer the
  // engine allocates holds this pattern instead of zeros / whatever the allocator left; the activation set of a launch group is
  // filled again before the group, staging and output buffers before each upload or stage.  A kernel then sees only what an
  // earlier kernel of its own group (or the upload) wrote, or the pattern.  Untouched: the weights and the range-guard counters.
  bool poison_on = false;
  unsigned poison = 0;
  size_t sig_bytes = 0, feat_bytes = 0;   // capacity of each d_sig / d_feat staging buffer
  // Lanes: a launch group of <= 2048 windows leaves most of the 256 CUs idle (512 windows = 32 workgroups per
  // Bi-LSTM launch), so the device-pointer entry points run consecutive groups on up to kMaxLanes streams,
  // each with its own activation buffers; results do not depend on the grouping.  NRV_LANES=0 turns it off.
  static constexpr int kMaxLanes = 8;
  struct Lane {
    float *S[2] = {0, 0}, *X1[2] = {0, 0}, *X2[2] = {0, 0}, *X3[2] = {0, 0}, *MO[2] = {0, 0};
    size_t act_n[5] = {0, 0, 0, 0, 0};
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
  } lanes[kMaxLanes];
  int n_lanes = 0, lane_rows = 0, lanes_on = 1;
  int coalesce = 1;                // launch groups below kCoalesce windows are merged (NRV_COALESCE=0: run them as they are, on the lanes)
  hipEvent_t ev_fork = nullptr;
  // staging for the host-pointer entry points
  // two staging sets [set][..]: the upload of group g+1 (copy stream) overlaps the kernels of group g
  // inputs: THREE staging sets (stage g uses set g % 3): the upload of stage g+1 is enqueued before the kernels of stage g, so it
  // has two stages' time to arrive (with two sets it could only be enqueued after stage g-1's results had been handed over, and
  // ended a few % after the running stage did: r05, 0.359 ms per stage against 0.327 device-resident); outputs: two sets
  static constexpr int kIn = 3;
  float *d_sig[kIn] = {0, 0, 0}, *d_feat[kIn] = {0, 0, 0}, *d_p[2][2] = {{0, 0}, {0, 0}};
  int8_t* d_a[2][2] = {{0, 0}, {0, 0}};
  // ONE device block per staging set, laid out as its page-locked mirror pin_out: [range-guard counter, 64 B | p1 r x 6 f32 |
  // p2 r x 5 f32 | a1 r | a2 r], r = the stage's rows padded to kRowPad: a stage's results come back in ONE copy of its own size (r05: six copies of ~13 us each stood between a
  // stage's last kernel and the host's hand-over, and the next upload, enqueued behind that, ended after the running stage did)
  char* d_out[2] = {0, 0};
  unsigned* d_sat_st[2] = {nullptr, nullptr};
  hipStream_t copy_stream = nullptr;      // host -> device
  hipStream_t d2h_stream = nullptr;       // device -> host (its own stream: an upload never queues behind a download)
  hipStream_t edit_stream = nullptr;      // nrv_revise_reads_raw_edits_begin / _records_begin only, created with the first such call: the
                                          // second download of nrv_reads_raw_end (d2h_stream may already wait for the OTHER slot's kernels)
  hipEvent_t ev_in[kIn] = {0, 0, 0}, ev_done[2] = {0, 0}, ev_out[2] = {0, 0};
  // page-locked host staging: outputs always land here first (46 B per window); inputs only when the
  // caller's arrays could not be registered in place (bounce copies)
  char* pin_out[2] = {0, 0};
  char *pin_sig[kIn] = {0, 0, 0}, *pin_feat[kIn] = {0, 0, 0};
  size_t pin_sig_cap = 0, pin_feat_cap = 0;
  int host_register = 1;                  // NRV_HOST_REGISTER=0: never hipHostRegister caller memory
  // raw-read entry points: samples, event starts and read descriptors of the current call
  int16_t* d_raw = nullptr;
  int32_t* d_starts = nullptr;
  SegRead* d_reads = nullptr;
  size_t cap_raw = 0, cap_starts = 0, cap_reads = 0;
  hipEvent_t ev_raw = nullptr;
  // Whole-call raw-read calls (nrv_reads_raw_begin / _end, r06): a call's inputs are 92 B per base, so ALL of them go up in one
  // copy and ALL its stages are enqueued on the compute stream in one go - no per-stage hand-over between streams - and its
  // results come back in one block.  Two slots, so that a caller can enqueue call k+1 before it collects call k.
  struct RawSlot {
    char* d_in = nullptr; char* pin_in = nullptr; size_t cap_in = 0;     // [raw i16 | starts i32 | reads | feat f32], 256-B aligned parts
    char* d_out = nullptr; char* pin_out = nullptr; size_t cap_out = 0;   // [counter 64 B | p1 | p2 | a1 | a2]
    size_t off_starts = 0, off_reads = 0, off_feat = 0, rows = 0;
    size_t off_aux = 0;                                                   // nrv_reads_raw_stats_begin: [.. | StatAux per read] behind feat
    unsigned* d_stat = nullptr; size_t cap_stat = 0;                      // ... and its scratch (min / max, histograms: nrv_stats.h)
    // a merged call: its bases and, for records, its names [.. | bases u8 | name_off i64 x (n_reads + 1) | names u8] at the end of
    // d_in (and behind them, for the accuracy, the truth); the merged block (MergeLayout) with its page-locked mirror - the ONLY part such a call downloads, with the 64-byte
    // counter of d_out; where the results go; and the values the re-run of nrv_reads_raw_end needs once the inputs are gone
    size_t off_bases = 0, off_noff = 0, off_names = 0;
    size_t off_toff = 0, off_truth = 0;                                   // accuracy: [.. | truth_off i64 x (n_reads + 1) | truth u8] behind names
    size_t off_labels = 0;                                                // score: [.. | labels u8 x N] behind the truth
    float score_thr[kPhredSteps] = {0};
    char* d_mrg = nullptr; char* pin_mrg = nullptr; size_t cap_mrg = 0;
    MergeLayout m = {};
    MergeOut out;
    bool want_q = false;
    float thr[kPhredSteps] = {0}, prof_thr[kPhredSteps] = {0}, trim_thr[kPhredSteps] = {0};
    int trim_Q = 0, trim_W = 0;
    int64_t trim_min_len = 0;
    size_t blob_cap = 0;
    int64_t N = 0, n = 0;
    int n_reads = 0;
    float *p1 = nullptr, *p2 = nullptr;
    int8_t *a1 = nullptr, *a2 = nullptr;
    hipEvent_t ev_in = nullptr, ev_done = nullptr, ev_out = nullptr;
    unsigned sat_seen = 0;
    bool busy = false;
  } raw_slot[2];
  // f16x2 range guard (cnn_h2_kernel): device counters [0], [1] = the staging sets of the host-pointer entry
  // points (downloaded with each stage's outputs), [2] = device-pointer calls (read by nrv_saturated)
  unsigned* d_sat = nullptr;
  unsigned* pin_sat[2] = {nullptr, nullptr};
  unsigned sat_seen[2] = {0, 0};   // the staging sets' counters only grow: a stage fired iff its counter moved since the last look
  bool host_call_open = false;     // a host-pointer call that left through an error path: its stages may have moved the counters
                                   // without anybody looking - the next call reads them back first
  // nrv_align_labels: ONE block of its own [inputs | hc | outputs | direction words], grown on demand and kept, on a non-blocking
  // stream of its own - the call touches nothing else of the handle but err, so it may run while a raw call is in flight.  A
  // block that became too small is RETIRED, not freed (hipFree would wait for the raw call in flight): nrv_destroy frees them.
  char* d_lab = nullptr;
  size_t cap_lab = 0;
  std::vector<char*> lab_retired;
  hipStream_t lab_stream = nullptr;
  size_t lab_budget = kLabelsBudget;     // bytes of direction words per batch of pairs (NRV_LABELS_BUDGET, read by nrv_create)
  // nrv_fit_*: the training set at the current depth (its arrays are kFitDepths' - x [cap][T][per_t] f32 per model, the arrays
  // both models share, y [cap] u8 per model, both models the same rows; grown on demand, poisoned under NRV_POISON, freed by
  // nrv_destroy), the scratch of a step, and per model the parameter block [theta | m | v | g] with its state on the device.
  // Everything runs on the handle's stream.
  struct Fit {
    float* x[2] = {nullptr, nullptr};                         // the depth's per-model array (null at depth NRV_FIT_FULL)
    float* shared[2] = {nullptr, nullptr};                    // the depth's shared arrays in door order: sig; at NRV_FIT_FULL sig, feat
    uint8_t* y[2] = {nullptr, nullptr};
    int64_t rows = 0, cap = 0;
    int64_t max_rows[6] = {};                                 // the row cap of each depth of kFitDepths, set by nrv_create
    // nrv_fit_set_depth (on an empty set only) frees the set and both models' parameter blocks when the depth changes, so
    // `cap` counts one kind of row
    int depth = NRV_FIT_TAIL;
    // depth NRV_FIT_LSTM4 and deeper: the scratch of one chunk of a batch (nrv_lstm4fit.h) and the LSTM block's gradient sums
    float* d_l4 = nullptr; size_t cap_l4 = 0;                 // [X4 | dX4 | CS | GZ] of kL4ChunkRows rows
    float* d_gl4 = nullptr; size_t cap_gl4 = 0;               // [kL4N]
    // depth NRV_FIT_LSTM3 and deeper: one chunk's [H3 | XB | dX3 | CS | GZ] (nrv_lstm3fit.h) in front of the lstm4 depth's
    // scratch, the lstm3 block's gradient sums, the identity row list of the lstm4 launches; while nrv_fit_add_reads_raw runs,
    // l3_slot is the slot list of the group run_group is at (the gather runs inside the group)
    float* d_l3 = nullptr; size_t cap_l3 = 0;
    float* d_gl3 = nullptr; size_t cap_gl3 = 0;               // [kL3N]
    unsigned* d_ident = nullptr;                              // [kL4ChunkRows] 0, 1, 2, ...
    const int* l3_slot = nullptr;
    // depth NRV_FIT_SIGNAL and deeper: one chunk's [Xin | F | dS] (nrv_signalfit.h) in front of the lstm3 depth's scratch, the
    // conv block's partials and the dense block's sums; the gather runs where the lstm3 depth's does, on l3_slot
    float* d_sg = nullptr; size_t cap_sg = 0;
    float* d_pconv = nullptr; size_t cap_pconv = 0;           // [workgroups][kSgConv]
    float* d_gdense = nullptr; size_t cap_gdense = 0;         // [kSgDense]
    // depth NRV_FIT_FULL: one chunk's [X1b | H1 | H2 | dH2 | dH1 | CS1 | CS2 | GZ1 | GZ2] (nrv_fullfit.h) in front of the signal
    // depth's scratch, the read block's kRdSlices partials
    float* d_rd = nullptr; size_t cap_rd = 0;
    float* d_grd = nullptr; size_t cap_grd = 0;               // [kRdSlices][kRdN]
    int* d_flag = nullptr; size_t cap_flag = 0;               // head_reduce_kernel's per-workgroup flags
    float* d_partial = nullptr; size_t cap_partial = 0;       // [workgroups][P]
    TailStat* d_pstat = nullptr; size_t cap_pstat = 0;        // [workgroups]
    unsigned* d_order = nullptr; size_t cap_order = 0;        // row indices of a call
    float* d_p = nullptr; size_t cap_p = 0;                   // nrv_fit_eval's rows
    double* d_bnpart = nullptr; size_t cap_bnpart = 0;        // nrv_fit_bn_reestimate: one chunk's partial moments of a stage
    // nrv_fit_set_bn_affine: gamma / beta of the BatchNorms inside the section are the front of the vector; the partials of
    // their sums [workgroups of a batch's first chunk][NRV_FIT_PARAMS_BN] (nrv_bnaffine.h)
    bool bn_affine = false;
    float* d_pbn = nullptr; size_t cap_pbn = 0;
    // nrv_fit_set_dropout: the rate (0: off), what the launches compare and divide by, the seed; each model's draw counter is
    // a host counter (Model::draw); nrv_fit_dropout_mask's bytes
    double drop_rate = 0.0;
    unsigned drop_thr = 0;
    float drop_keepf = 1.f;
    uint64_t drop_seed = 0;
    unsigned char* d_mask = nullptr; size_t cap_mask = 0;
    struct Model {
      float* d_par = nullptr;                                 // [4][P]
      // depths NRV_FIT_LSTM3 and deeper: the fit's own BatchNorm block [kBnFloats] (nrv_bnfit.h) - every fit launch reads its
      // (scale, shift) pairs here - the running sums [2][kBnCh] of a re-estimation, and what nrv_fit_bn_get returns
      float* d_bn = nullptr;
      double* d_bnacc = nullptr;
      std::vector<float> bn_mean, bn_var;
      std::vector<double> bn_s1, bn_s2;
      int64_t bn_n[5] = {0, 0, 0, 0, 0};
      TailState* d_state = nullptr;
      float* d_lr = nullptr; size_t cap_lr = 0;
      bool begun = false;
      long long t = 0;
      int64_t draw = 0;                                       // nrv_fit_set_dropout: the next batch's draw
      nrv_fit_opts o = {};
    } m[2];
  } fit;
  int64_t sat_reruns = 0;          // pipeline stages the host entry points re-ran on the f32 kernels
  int h2 = 1;                      // 1: f16x2 mode (the default) - lstm2..4 on lstm_h2o / lstm_h2s_kernel, activations between the kernels
                                   // as f16 split planes (cnn dense and head stay on their bf16x3 kernels)
  int split = 62;                  // bit l set: layer l (1..3 = lstm2..4, 4 = head dense layers, 5 = signal-branch
                                   // dense) runs its split-bf16 kernel (nrv_set_precision: BF16X3 = 62, F32 = 0)
  std::string err;
  // profiling
  int prof = 0;                      // 0 off, 1 every kernel, 2 only slot 3 (lstm3, the dominant kernel),
                                     // 3 slot 3 on every 8th group
  unsigned prof_tick = 0;
  std::vector<hipEvent_t> ev_pool;   // groups of NRV_N_KERNELS+1 events
  size_t ev_used = 0;
  double prof_ms[NRV_N_KERNELS] = {0};
  int64_t prof_n[NRV_N_KERNELS] = {0};
};

namespace {

#define HIPCHK(h, call)                                                                  \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess) {                                                              \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                      \
      return NRV_E_HIP;                                                                  \
    }                                                                                    \
  } while (0)

// the descriptor of the handle's fit depth (nrv_fit_set_depth lets nothing else in)
static const FitDepth& fit_at(const nrv_handle* h) { return *fit_desc(h->fit.depth); }

// NRV_POISON: the handle's pattern into the 32-bit words of [p, p + bytes), on stream s (nothing when the switch is off)
static int poison_fill(nrv_handle* h, void* p, size_t bytes, hipStream_t s) {
  if (!h->poison_on || !p || bytes < 4) return NRV_OK;
  HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)p, (int)h->poison, bytes / 4, s));
  return NRV_OK;
}
// a freshly allocated activation buffer: zeros, or the pattern (synchronous, like the hipMemset it replaces)
static int alloc_fill(nrv_handle* h, void* p, size_t bytes) {
  if (h->poison_on) HIPCHK(h, hipMemsetD32((hipDeviceptr_t)p, (int)h->poison, bytes / 4));
  else HIPCHK(h, hipMemset(p, 0, bytes));
  return NRV_OK;
}
// host -> device on stream s; a length of 0 copies nothing (src may be null then)
static int put(nrv_handle* h, void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (bytes > 0) HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
  return NRV_OK;
}
// "One block of its own" (layouts: nrv_block.h): allocated, NRV_POISON over all of it, body(d) - the uploads, the kernels, the
// downloads and the wait for them, all on stream s - and freed.  What a failed body left in flight is waited for before the block goes
template <class Body>
static int with_block(nrv_handle* h, size_t bytes, hipStream_t s, Body&& body) {
  char* d = nullptr;
  HIPCHK(h, hipMalloc((void**)&d, bytes));
  int rc = poison_fill(h, d, bytes, s);
  if (!rc) rc = body(d);
  if (rc) (void)hipStreamSynchronize(s);
  (void)hipFree(d);
  return rc;
}

// unit halves (16 units each) per wave of the f16x2 kernels of lstm2..4: lstm_h2w_kernel (192 -> 128) and lstm_h2s_kernel (256 -> 64)
// both give a wave one unit group of 16
static const int kUhS[4] = {0, 1, 1, 1};

NRV_HOST_COLD static int upload_model(nrv_handle* h, int mi, const Blob& b, int C) {
  const int T = h->T;
  DevModel& d = h->dm[mi];
  d.C = C;
  std::vector<float> host;
  auto put = [&](const float* p, size_t n) {
    size_t o = host.size();
    host.insert(host.end(), p, p + n);
    while (host.size() % 4) host.push_back(0.f);      // keep every tensor 16-byte aligned
    return o;
  };
  // conv block (nanorevcnn.py:29-38): w1[k][o], b1, bn1 scale/shift, w2[k][c][o], b2, bn2 scale/shift
  {
    float cv[264];
    memcpy(cv, b.t(0), 24 * 4);
    memcpy(cv + 24, b.t(1), 8 * 4);
    bn_fold(b.t(2), b.t(3), b.t(4), b.t(5), 8, cv + 32, cv + 40);
    memcpy(cv + 48, b.t(6), 192 * 4);
    memcpy(cv + 240, b.t(7), 8 * 4);
    bn_fold(b.t(8), b.t(9), b.t(10), b.t(11), 8, cv + 248, cv + 256);
    d.conv = put(cv, 264);
  }
  for (int i = 0; i < 4; ++i) {
    d.bn_raw[i].clear();
    for (const auto& k : kFitBn) d.bn_raw[i].insert(d.bn_raw[i].end(), b.t(k.tensor + i), b.t(k.tensor + i) + k.C);
  }
  {
    static const size_t n3[6] = {192 * 512, 128 * 512, 512, 192 * 512, 128 * 512, 512};
    d.l3raw = put(b.t(34), n3[0]);
    for (int i = 1; i < 6; ++i) (void)put(b.t(34 + i), n3[i]);
  }
  {
    static const size_t n4[6] = {256 * 256, 64 * 256, 256, 256 * 256, 64 * 256, 256};
    d.l4raw = put(b.t(44), n4[0]);
    for (int i = 1; i < 6; ++i) (void)put(b.t(44 + i), n4[i]);
  }
  {
    static const size_t n1[3] = {6 * 64, 16 * 64, 64}, n2[3] = {32 * 256, 64 * 256, 256};
    d.l1raw = put(b.t(12), n1[0]);
    for (int i = 1; i < 6; ++i) (void)put(b.t(12 + i), n1[i % 3]);
    d.l2raw = put(b.t(22), n2[0]);
    for (int i = 1; i < 6; ++i) (void)put(b.t(22 + i), n2[i % 3]);
  }
  std::vector<float> wp, bs;
  pack_dense16(b.t(32), 400, 64, wp);
  d.dpack = put(wp.data(), wp.size());
  d.dbias = put(b.t(33), 64);
  d.sdraw = put(b.t(32), 400 * 64);
  pack_cnn_split(b.t(32), wp);
  d.dsplit = put(wp.data(), wp.size());
  const int lbase[4] = {12, 22, 34, 44}, lK[4] = {6, 32, 192, 256}, lH[4] = {16, 64, 128, 64};
  const int bnbase[4] = {18, 28, 40, -1};
  NRV_FOR (int l = 0; l < 4; ++l) {
    pack_lstm(b, lbase[l], lK[l], lH[l], wp, bs);
    d.l_w[l] = put(wp.data(), wp.size());
    d.l_b[l] = put(bs.data(), bs.size());
    std::vector<float> sc(2 * lH[l], 1.f), sh(2 * lH[l], 0.f);
    if (bnbase[l] >= 0)
      bn_fold(b.t(bnbase[l]), b.t(bnbase[l] + 1), b.t(bnbase[l] + 2), b.t(bnbase[l] + 3), 2 * lH[l],
              sc.data(), sh.data());
    d.l_s[l] = put(sc.data(), sc.size());
    d.l_h[l] = put(sh.data(), sh.size());
  }
  NRV_FOR (int l = 1; l < 4; ++l) {
    pack_lstm_split(b, lbase[l], lK[l], lH[l], wp);
    d.l_ws[l] = put(wp.data(), wp.size());
  }
  {
    // f16x2 plan.  Buffer exponents: BatchNorm'd LSTM outputs are bounded by |scale| + |shift| per
    // channel (|h| < 1); the signal branch's output has no static bound: 2^6 (|S| <= 92 on the fixture
    // reads); beyond +-65504 / 2^6 the producer's range guard fires and the group is re-run in f32.
    auto bn_exp = [&](int bnb, int n, std::vector<float>& sc, std::vector<float>& sh) {
      sc.assign(n, 1.f); sh.assign(n, 0.f);
      bn_fold(b.t(bnb), b.t(bnb + 1), b.t(bnb + 2), b.t(bnb + 3), n, sc.data(), sh.data());
      float bound = 0.f;
      NRV_FOR (int i = 0; i < n; ++i) bound = std::fmax(bound, std::fabs(sc[i]) + std::fabs(sh[i]));
      return pow2_room(bound);
    };
    std::vector<float> sc1, sh1, sc2, sh2, sc3, sh3;
    const int sX1 = bn_exp(18, 32, sc1, sh1), sX2 = bn_exp(28, 128, sc2, sh2), sX3 = bn_exp(40, 256, sc3, sh3);
    constexpr int sS = 6;
    auto put_scaled = [&](const std::vector<float>& v, int e) {
      std::vector<float> t(v.size());
      NRV_FOR (size_t i = 0; i < v.size(); ++i) t[i] = std::ldexp(v[i], e);
      return put(t.data(), t.size());
    };
    d.l1s2 = put_scaled(sc1, sX1);                       // lstm1 keeps h unscaled in its LDS image
    d.l1h2 = put_scaled(sh1, sX1);
    {
      // cnn_r_kernel (nrv_cnn_r.h): c1 and the conv features travel x 2^6 as f16 pairs, the dense weights x 2^10
      static_assert(sS == 6, "kCnnRImgScale / kCnnRDenseDescale in nrv_cnn_r.h assume S x 2^6");
      float cv[264];
      memcpy(cv, host.data() + d.conv, 264 * 4);
      NRV_FOR (int o = 0; o < 8; ++o) { cv[248 + o] = std::ldexp(cv[248 + o], 6); cv[256 + o] = std::ldexp(cv[256 + o], 6); }
      // the second convolution x 2^u is the A operand of a transposed product; c1 is kept x 2^6, so its accumulator
      // holds z x 2^(6+u)
      std::vector<float> db(b.t(33), b.t(33) + 64);
      d.cr_dbias = put_scaled(db, 16);                         // dense bias x 2^16
      const float* w2 = host.data() + d.conv + 48;             // [tap][ci][co]
      const int u = pow2_room(max_abs(w2, 192));
      float ep[48] = {0};
      NRV_FOR (int co = 0; co < 8; ++co) {
        ep[co] = std::ldexp(cv[240 + co], 6 + u);              // bias of the second convolution
        ep[16 + co] = std::ldexp(cv[248 + co], -6 - u);        // cv[248..]: BatchNorm 2 scale, already x 2^6 -> s2 x 2^-u
        ep[32 + co] = cv[256 + co];                            // BatchNorm 2 shift x 2^6
      }
      {
        // cnn_r_kernel (nrv_cnn_r.h).  conv2's A operand gives TWO positions per product: rows 0-7 take tap = k-group,
        // rows 8-15 tap = k-group - 1 (the B operand's k-groups hold c1 at positions p - 1 .. p + 2).
        std::vector<uint16_t> fr((size_t)2 * 64 * 8, 0);
        NRV_FOR (int lane = 0; lane < 64; ++lane)
          NRV_FOR (int j = 0; j < 8; ++j) {
            const int m = lane & 15, kg = lane >> 4;
            const int co = m & 7, tap = m < 8 ? kg : kg - 1;
            const float v = (tap >= 0 && tap < 3) ? std::ldexp(w2[(tap * 8 + j) * 8 + co], u) : 0.f;
            split_f16(v, &fr[(size_t)lane * 8 + j], &fr[(size_t)512 + lane * 8 + j]);
          }
        std::vector<float> f2(fr.size() / 2);
        memcpy(f2.data(), fr.data(), fr.size() * 2);
        d.cr_w2 = put(f2.data(), f2.size());
        float e2[25];
        NRV_FOR (int co = 0; co < 8; ++co) { e2[co] = ep[co]; e2[8 + co] = ep[16 + co]; e2[16 + co] = ep[32 + co]; }
        // Range guard of conv1's output (kept x 2^6 as an f16 pair: |c1| must stay below 65504 / 64): a STATIC bound on
        // the samples.  |c1[o]| <= |s1[o]| (|b1[o]| + sum_k |w1[k][o]| xmax) + |h1[o]|, so with every |x| <= xlim no
        // conv1 output can leave the f16 range; a unit that sees a larger sample counts as out of range (re-run in f32).
        {
          const float* c0u = host.data() + d.conv;             // w1 24, b1 8, s1 8 (BatchNorm scale), h1 8 (shift)
          double xl = 1e30;
          NRV_FOR (int o = 0; o < 8; ++o) {
            const double sw = std::fabs((double)c0u[o]) + std::fabs((double)c0u[8 + o]) + std::fabs((double)c0u[16 + o]);
            const double sc = std::fabs((double)c0u[32 + o]), room = 1000.0 - std::fabs((double)c0u[40 + o]);
            if (sc > 0 && sw > 0) { const double l = (room / sc - std::fabs((double)c0u[24 + o])) / sw; if (l < xl) xl = l; }
          }
          e2[24] = (float)(xl > 0 ? xl : 0.0);
        }
        d.cr_ep = put(e2, 25);
        // dense 400 -> 64 x 2^10 as A fragments in the k order the conv2 result tiles arrive in:
        // [ks 13][mt 4][term 2][64 lanes][8 f16]; lane (m = l & 15, kg = l >> 4), element j:
        //   position 4 ks + 2 (j >> 2) + (kg >> 1), channel 4 (kg & 1) + (j & 3), output feature 16 mt + m
        const float* Wd = b.t(32);
        std::vector<uint16_t> df((size_t)13 * 4 * 2 * 512, 0);
        NRV_FOR (int ks = 0; ks < 13; ++ks)
          NRV_FOR (int mt = 0; mt < 4; ++mt)
            NRV_FOR (int lane = 0; lane < 64; ++lane)
              NRV_FOR (int j = 0; j < 8; ++j) {
                const int m = lane & 15, kg = lane >> 4;
                const int pos = 4 * ks + 2 * (j >> 2) + (kg >> 1), ch = 4 * (kg & 1) + (j & 3);
                const float v = pos < 50 ? std::ldexp(Wd[(size_t)(pos * 8 + ch) * 64 + 16 * mt + m], 10) : 0.f;
                const size_t o = ((size_t)((ks * 4 + mt) * 2) * 64 + lane) * 8 + j;
                split_f16(v, &df[o], &df[o + 512]);
              }
        std::vector<float> d2(df.size() / 2);
        memcpy(d2.data(), df.data(), df.size() * 2);
        d.cr_d = put(d2.data(), d2.size());
      }
      const float* c0 = host.data() + d.conv;                  // unscaled: w1 24, b1 8, s1 8, h1 8
      memcpy(d.cr_k.w1, c0, 24 * 4);
      memcpy(d.cr_k.b1, c0 + 24, 8 * 4);
      NRV_FOR (int o = 0; o < 8; ++o) { d.cr_k.s1[o] = std::ldexp(c0[32 + o], 6); d.cr_k.h1[o] = std::ldexp(c0[40 + o], 6); }
    }
    const int K0[4] = {0, 32, 128, 256}, K1[4] = {0, 0, 64, 0}, s0[4] = {0, sX1, sX2, sX3}, s1[4] = {0, 0, sS, 0};
    const std::vector<float>* osc[4] = {nullptr, &sc2, &sc3, nullptr};
    const std::vector<float>* osh[4] = {nullptr, &sh2, &sh3, nullptr};
    const int sout[4] = {0, sX2, sX3, 13};           // the 256->64 layer has no BatchNorm: its output stays h x 2^13
    d.hsc = pack_head_h2(b, wp, bs);
    d.h_w2 = put(wp.data(), wp.size());
    d.h_b2 = put(bs.data(), bs.size());
    NRV_FOR (int l = 1; l < 4; ++l) {
      const int E = plan_exponent(b, lbase[l], K0[l], s0[l], K1[l], s1[l], lH[l]);
      if (l == 1) {
        pack_lstm2_t(b, lbase[1], sX1, E, wp, bs);
        d.l2t_w = put(wp.data(), wp.size());
        d.l2t_b = put(bs.data(), bs.size());
      }
      if (l >= 2) {
        // The BatchNorm in front of this layer - BatchNorm(128) on the first 128 input rows of the 192->128 layer (its
        // other 64 rows come from the signal branch), BatchNorm(256) on all rows of the 256->64 layer - folded into it:
        //   (h sc + sh) W + b = h (diag(sc) W) + (b + sh W),
        // so that the layer before hands over its h x 2^13 as it stands (no BatchNorm, no second split in its epilogue).
        const int Kf = l == 2 ? 128 : 256;
        const std::vector<float>& fsc = l == 2 ? sc2 : sc3;
        const std::vector<float>& fsh = l == 2 ? sh2 : sh3;
        std::vector<float> all(b.p, b.p + b.off.back() + (size_t)C);          // the blob ends with final_out's bias [C]
        NRV_FOR (int dir = 0; dir < 2; ++dir) {
          float* W = all.data() + b.off[lbase[l] + dir * 3 + 0];
          float* B = all.data() + b.off[lbase[l] + dir * 3 + 2];
          const int N4 = 4 * lH[l];
          NRV_FOR (int c = 0; c < N4; ++c) {
            double acc = B[c];
            NRV_FOR (int k = 0; k < Kf; ++k) acc += (double)fsh[k] * (double)W[(size_t)k * N4 + c];
            B[c] = (float)acc;
          }
          NRV_FOR (int k = 0; k < Kf; ++k)
            NRV_FOR (int c = 0; c < N4; ++c) W[(size_t)k * N4 + c] *= fsc[k];
        }
        const Blob bf{all.data(), b.off};
        const int Ef = plan_exponent(bf, lbase[l], K0[l], 13, K1[l], s1[l], lH[l]);
        pack_lstm_h2s(bf, lbase[l], K0[l], 13, K1[l], s1[l], lH[l], Ef, wp, bs, kUhS[l]);
        d.l_w2sf[l] = put(wp.data(), wp.size());
        d.l_b2sf[l] = put(bs.data(), bs.size());
        d.descale_f[l] = std::ldexp(1.f, -Ef);
      }
      d.descale[l] = std::ldexp(1.f, -E);
      // the LDS image holds h * 2^13: scale' = scale * 2^(s_out - 13), shift' = shift * 2^s_out
      std::vector<float> one(2 * lH[l], 1.f), zero(2 * lH[l], 0.f);
      d.l_s2[l] = put_scaled(osc[l] ? *osc[l] : one, sout[l] - 13);
      d.l_h2[l] = put_scaled(osh[l] ? *osh[l] : zero, sout[l]);
    }
  }
  pack_lstm1_16(b, 12, wp, bs);
  d.l1w16 = put(wp.data(), wp.size());
  d.l1b16 = put(bs.data(), bs.size());
  pack_dense(b.t(50), 128, 128, wp); d.d1p = put(wp.data(), wp.size());
  d.d1b = put(b.t(51), 128);
  pack_dense(b.t(52), 128, 32, wp); d.d2p = put(wp.data(), wp.size());
  d.d2b = put(b.t(53), 32);
  pack_dense(b.t(54), 32, 6, wp); d.mop = put(wp.data(), wp.size());
  {
    float mb[32] = {0};
    memcpy(mb, b.t(55), 6 * 4);
    d.mob = put(mb, 32);
  }
  pack_head_split(b, wp, bs);
  d.h_ws = put(wp.data(), wp.size());
  d.h_wb = put(bs.data(), bs.size());
  d.fw = put(b.t(56), (size_t)6 * T * 16);
  {
    // head_h2_kernel's LDS image of the feature kernel, [f 16][t][8] (k padded 6 -> 8), packed here: the kernel built it itself
    // until r05 (four dependent scalar-indexed loads + two integer divisions per thread in front of its first barrier)
    std::vector<float> f8((size_t)16 * T * 8, 0.f);
    const float* fwp = b.t(56);
    NRV_FOR (int f = 0; f < 16; ++f)
      NRV_FOR (int t = 0; t < T; ++t)
        NRV_FOR (int k = 0; k < 6; ++k) f8[((size_t)f * T + t) * 8 + k] = fwp[(size_t)(t * 6 + k) * 16 + f];
    d.fw8 = put(f8.data(), f8.size());
  }
  d.fb = put(b.t(57), 16);
  d.ow = put(b.t(58), (size_t)16 * C);
  d.ob = put(b.t(59), C);
  d.n = host.size();
  HIPCHK(h, hipMalloc(&d.all, d.n * sizeof(float)));
  HIPCHK(h, hipMemcpy(d.all, host.data(), d.n * sizeof(float), hipMemcpyHostToDevice));
  return NRV_OK;
}

static void free_workspace(nrv_handle* h) {
  for (int m = 0; m < 2; ++m) {
    (void)hipFree(h->S[m]); (void)hipFree(h->X1[m]); (void)hipFree(h->X2[m]); (void)hipFree(h->X3[m]);
    (void)hipFree(h->MO[m]); h->MO[m] = nullptr;
    for (int st = 0; st < 2; ++st) { h->d_p[st][m] = nullptr; h->d_a[st][m] = nullptr; }
    h->S[m] = h->X1[m] = h->X2[m] = h->X3[m] = nullptr;
  }
  for (int st = 0; st < 2; ++st) {
    (void)hipFree(h->d_out[st]);
    h->d_out[st] = nullptr; h->d_sat_st[st] = nullptr; h->pin_sat[st] = nullptr; h->sat_seen[st] = 0;
    (void)hipHostFree(h->pin_out[st]);
    h->pin_out[st] = nullptr;
  }
  for (int st = 0; st < nrv_handle::kIn; ++st) {
    (void)hipFree(h->d_sig[st]); (void)hipFree(h->d_feat[st]);
    h->d_sig[st] = h->d_feat[st] = nullptr;
    (void)hipHostFree(h->pin_sig[st]); (void)hipHostFree(h->pin_feat[st]);
    h->pin_sig[st] = h->pin_feat[st] = nullptr;
  }
  h->pin_sig_cap = h->pin_feat_cap = 0;
  h->cap_rows = 0;
}

// Windows per LAUNCH group.  Results do not depend on how the windows of a call are grouped (every window is its own
// row of every kernel; tests/test_gpu_parity.py pins it bit for bit), and a launch group below 4096 windows leaves most
// of the chip idle - 512 windows are 32 workgroups of a Bi-LSTM launch on 256 CUs - while every launch pays its fixed
// cost (staging of weights into LDS, launch boundaries: ~10 % of a 4096-window group's time, all of a 512-window
// group's).  So consecutive small groups of ONE call are coalesced into launches of kCoalesce windows; `batch` stays
// what the caller set (nrv_get_batch) and keeps bounding the group from above when it is larger.  r04, config C2
// (batch 512, E. coli weights): 8.6 M bases/s on eight stream lanes -> the rate of 4096-window groups.
constexpr int kCoalesce = 4096;
static int group_windows(const nrv_handle* h) { return (h->coalesce && h->batch < kCoalesce) ? kCoalesce : h->batch; }

// Lanes the current batch asks for (only with NRV_COALESCE=0): 4096 / batch (2 .. kMaxLanes) when a group is <= 2048 windows.
static int lanes_wanted(const nrv_handle* h) {
  if (h->coalesce) return 0;
  if (!h->lanes_on || h->batch > 2048 || h->batch % 32) return 0;      // whole row tiles only
  const int w = 4096 / h->batch;
  return w > nrv_handle::kMaxLanes ? nrv_handle::kMaxLanes : w;
}
// Windows per pipeline stage of the host-pointer entry points (one upload, its groups, one download).
// READ modes (one event per window crosses PCIe, 92-270 B per base) take several full-size groups per stage
// (NRV_READ_STAGE, default kReadStageGroups): fewer uploads, events and hand-overs per call - r03, same box:
// nrv_predict_reads_raw 11.9 / 12.4 / 12.5 M bases/s with 1 / 2 / 4 groups per stage, nrv_predict_read 11.6 / 11.7 /
// 12.0.  The same stage in WINDOW mode (2958 B per base) halves nrv_predict (9.3 -> 4.7 M with 2): its pipeline
// then has too few stages to hide PCIe behind the kernels, so window mode keeps one group per stage.
constexpr int kReadStageGroups = 4;
static int read_stage_groups(const nrv_handle* h) {
  static const int env = getenv("NRV_READ_STAGE") ? atoi(getenv("NRV_READ_STAGE")) : kReadStageGroups;
  return (lanes_wanted(h) > 1 || env < 1) ? 1 : (env > 8 ? 8 : env);
}
static int stage_windows(const nrv_handle* h, bool read_mode = false) {
  const int w = lanes_wanted(h);
  if (w > 1) return w * h->batch;
  return read_mode ? read_stage_groups(h) * group_windows(h) : group_windows(h);
}

static int ensure_workspace(nrv_handle* h) {
  const int T = h->T;
  const int rows = ((stage_windows(h, true) + kRowPad - 1) / kRowPad) * kRowPad;   // staging: the larger (read-mode) stage
  if (rows <= h->cap_rows) return NRV_OK;
  free_workspace(h);
  int rc;
  // activations: ONE launch group (a stage's groups run one after the other on these, or on the lanes' own sets)
  const size_t tiles = (size_t)(((group_windows(h) + kRowPad - 1) / kRowPad) * kRowPad) / 32;
  // event-major S needs (rows + T + 32) events; window-major S needs rows*T "events"
  for (int m = 0; m < 2; ++m) {
    size_t nS = (tiles * T + 2) * 16 * 128, n1 = tiles * T * 8 * 128, n2 = tiles * T * 32 * 128,
           n3 = tiles * T * 64 * 128;
    HIPCHK(h, hipMalloc(&h->S[m], nS * 4));
    HIPCHK(h, hipMalloc(&h->X1[m], n1 * 4));
    HIPCHK(h, hipMalloc(&h->X2[m], n2 * 4));
    HIPCHK(h, hipMalloc(&h->X3[m], n3 * 4));
    HIPCHK(h, hipMalloc(&h->MO[m], tiles * T * 256 * 4));
    const size_t nm = tiles * T * 256;
    if ((rc = alloc_fill(h, h->MO[m], nm * 4)) || (rc = alloc_fill(h, h->S[m], nS * 4)) || (rc = alloc_fill(h, h->X1[m], n1 * 4)) ||
        (rc = alloc_fill(h, h->X2[m], n2 * 4)) || (rc = alloc_fill(h, h->X3[m], n3 * 4)))
      return rc;
    if (m == 0) { h->act_n[0] = nS; h->act_n[1] = n1; h->act_n[2] = n2; h->act_n[3] = n3; h->act_n[4] = nm; }
  }
  h->sig_bytes = (size_t)rows * T * kSig * 4 + 4096;
  h->feat_bytes = (size_t)rows * T * kFeat * 4 + 4096;
  for (int st = 0; st < nrv_handle::kIn; ++st) {
    HIPCHK(h, hipMalloc(&h->d_sig[st], h->sig_bytes));
    HIPCHK(h, hipMalloc(&h->d_feat[st], h->feat_bytes));
    if ((rc = poison_fill(h, h->d_sig[st], h->sig_bytes, nullptr)) || (rc = poison_fill(h, h->d_feat[st], h->feat_bytes, nullptr)))
      return rc;
  }
  for (int st = 0; st < 2; ++st) {
    const size_t ob = (size_t)rows * kOutBytes;              // rows is a multiple of kRowPad: the counter behind it is aligned
    HIPCHK(h, hipMalloc((void**)&h->d_out[st], ob + 64));
    HIPCHK(h, hipMemset(h->d_out[st], 0, ob + 64));
    if ((rc = poison_fill(h, h->d_out[st] + 64, ob, nullptr))) return rc;     // not the counter
    HIPCHK(h, hipHostMalloc((void**)&h->pin_out[st], ob + 64, hipHostMallocDefault));
    memset(h->pin_out[st], 0, ob + 64);
    // [range-guard counter, 64 B][p1 r x 6 f32 | p2 r x 5 f32 | a1 r | a2 r], r = the STAGE's rows padded to kRowPad: the
    // counter sits in front so that one copy of 64 + r x 46 bytes carries a short stage whole (a call of one short
    // read downloaded the block of the largest stage); the defaults below are the full-size layout
    h->d_p[st][0] = (float*)(h->d_out[st] + 64);
    h->d_p[st][1] = (float*)(h->d_out[st] + 64 + (size_t)rows * 24);
    h->d_a[st][0] = (int8_t*)(h->d_out[st] + 64 + (size_t)rows * 44);
    h->d_a[st][1] = (int8_t*)(h->d_out[st] + 64 + (size_t)rows * 45);
    h->d_sat_st[st] = (unsigned*)h->d_out[st];
    h->pin_sat[st] = (unsigned*)h->pin_out[st];
    h->sat_seen[st] = 0;
  }
  // the pattern fills above went to the null stream; the copy streams, which fill staging next, are not ordered behind it
  if (h->poison_on) HIPCHK(h, hipDeviceSynchronize());
  h->cap_rows = rows;
  return NRV_OK;
}

static void free_lanes(nrv_handle* h) {
  for (int l = 0; l < nrv_handle::kMaxLanes; ++l) {
    nrv_handle::Lane& L = h->lanes[l];
    if (L.stream) (void)hipStreamSynchronize(L.stream);
    for (int m = 0; m < 2; ++m) {
      (void)hipFree(L.S[m]); (void)hipFree(L.X1[m]); (void)hipFree(L.X2[m]); (void)hipFree(L.X3[m]); (void)hipFree(L.MO[m]);
      L.S[m] = L.X1[m] = L.X2[m] = L.X3[m] = L.MO[m] = nullptr;
    }
  }
  h->n_lanes = 0;
  h->lane_rows = 0;
}

static int ensure_lanes(nrv_handle* h) {
  const int T = h->T;
  const int rows = ((h->batch + kRowPad - 1) / kRowPad) * kRowPad;
  const int want = lanes_wanted(h);
  if (want == h->n_lanes && (want == 0 || rows <= h->lane_rows)) return NRV_OK;
  free_lanes(h);
  if (want == 0) return NRV_OK;
  const size_t tiles = rows / 32;
  const size_t nS = (tiles * T + 2) * 16 * 128, n1 = tiles * T * 8 * 128, n2 = tiles * T * 32 * 128,
               n3 = tiles * T * 64 * 128, nm = tiles * T * 256;
  if (!h->ev_fork) HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
  for (int l = 0; l < want; ++l) {
    nrv_handle::Lane& L = h->lanes[l];
    if (!L.stream) HIPCHK(h, hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    if (!L.done) HIPCHK(h, hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
    for (int m = 0; m < 2; ++m) {
      float** bufs[5] = {&L.S[m], &L.X1[m], &L.X2[m], &L.X3[m], &L.MO[m]};
      const size_t sz[5] = {nS, n1, n2, n3, nm};
      for (int i = 0; i < 5; ++i) {
        HIPCHK(h, hipMalloc(bufs[i], sz[i] * 4));
        const int rc = alloc_fill(h, *bufs[i], sz[i] * 4);
        if (rc) return rc;
        L.act_n[i] = sz[i];
      }
    }
  }
  HIPCHK(h, hipDeviceSynchronize());
  h->n_lanes = want;
  h->lane_rows = rows;
  return NRV_OK;
}

// Wave geometry of a Bi-LSTM launch: R row tiles per wave, WR wave-rows per workgroup.
// f32 mode: the geometry of each layer is fixed (tuned on MI355X at 4096 windows): 32->64 and 256->64 run
// (R, WR) = (1, 2), 192->128 (1, 1); the experiments build can pick others with NRV_GEO.
template <int KQ0, int KQ1, int H, int R, int WR>
static void launch_lstm_f32(nrv_handle* h, const LstmArgs& a, int tiles) {
  constexpr int NG = (H + 31) / 32;
  static_assert(NG * WR <= 4, "at most 4 waves per workgroup (one per SIMD, 512 registers each)");
#ifdef NRV_DEV_FAST
  return;
#else
  LstmArgs la = a;
  la.n_blk = (tiles + R * WR - 1) / (R * WR);
  dim3 grid(lstm_grid(la.n_blk)), blk(64 * NG * WR);
  if (h->act == 0) hipLaunchKernelGGL((lstm_layer_kernel<KQ0, KQ1, H, R, WR, false, 0>), grid, blk, 0, h->stream, la);
  NRV_ACT1(else hipLaunchKernelGGL((lstm_layer_kernel<KQ0, KQ1, H, R, WR, false, 1>), grid, blk, 0, h->stream, la);)
#endif
}


template <int KQ0, int KQ1, int H, int R, int WR>
static void launch_lstm_split(nrv_handle* h, const LstmArgs& a, const float* const ws[2], int tiles) {
  constexpr int NG = (H + 31) / 32;
#ifdef NRV_DEV_FAST
  return;
#else
  LstmSplitArgs sa;
  sa.T = a.T; sa.n_rows = a.n_rows;
  for (int m = 0; m < 2; ++m)
    sa.m[m] = LstmSplitModelParams{ws[m], a.m[m].bias, a.m[m].bn_scale, a.m[m].bn_shift, a.m[m].in0, a.m[m].in1,
                                   a.m[m].out};
  sa.n_blk = (tiles + R * WR - 1) / (R * WR);
  dim3 grid(lstm_grid(sa.n_blk)), blk(64 * NG * WR);
  // Timestep pairs (lstm_pair_kernel) pay for the layers that run one row tile per wave (32->64,
  // 256->64: -7 % / -5 %); at R = 2 the second accumulator set leaves too few registers (192->128
  // measured 335 -> 362 us even with the cell state moved to LDS: the remaining spill reloads drain
  // the in-order prefetch queue), so that layer keeps lstm_split_kernel.
  if constexpr (R == 1) {
    {
      if (h->act == 0) hipLaunchKernelGGL((lstm_pair_kernel<KQ0, KQ1, H, R, WR, 0>), grid, blk, 0, h->stream, sa);
      NRV_ACT1(else hipLaunchKernelGGL((lstm_pair_kernel<KQ0, KQ1, H, R, WR, 1>), grid, blk, 0, h->stream, sa);)
      return;
    }
  }
  if constexpr (R != 1)
  {
    if (h->act == 0) hipLaunchKernelGGL((lstm_split_kernel<KQ0, KQ1, H, R, WR, 0>), grid, blk, 0, h->stream, sa);
    NRV_ACT1(else hipLaunchKernelGGL((lstm_split_kernel<KQ0, KQ1, H, R, WR, 1>), grid, blk, 0, h->stream, sa);)
  }
#endif
}

template <int KQ0, int KQ1, int H, int R, int WR, int UH, int NBG, int NA, int KBL = 0, bool RAW = false>
static void launch_lstm_h2s(nrv_handle* h, int layer, const ActView (&in0)[2], const ActView (&in1)[2],
                            float* const out[2], int T, int n, int tiles) {
  constexpr int NG = H / (16 * UH);
  LstmH2Args sa;
  sa.T = T; sa.n_rows = n;
  for (int m = 0; m < 2; ++m) {
    const DevModel& d = h->dm[m];
    // weights with the BatchNorm in FRONT of the layer folded in (upload_model)
    sa.m[m] = LstmH2ModelParams{d.all + d.l_w2sf[layer], d.all + d.l_b2sf[layer],
                                d.all + d.l_s2[layer], d.all + d.l_h2[layer], in0[m], in1[m], out[m],
                                d.descale_f[layer]};
  }
  sa.n_blk = (tiles + R * WR - 1) / (R * WR);
  dim3 grid(lstm_grid(sa.n_blk)), blk(64 * NG * WR);
  if (h->act == 0) hipLaunchKernelGGL((lstm_h2s_kernel<KQ0, KQ1, H, R, WR, UH, 0, NBG, NA, KBL, RAW>), grid, blk, 0, h->stream, sa);
  NRV_ACT1(else hipLaunchKernelGGL((lstm_h2s_kernel<KQ0, KQ1, H, R, WR, UH, 1, NBG, NA, KBL, RAW>), grid, blk, 0, h->stream, sa);)
}

// lstm4_r_kernel (nrv_lstm4_r.h): the 256->64 layer; lstm_h2s_kernel's arguments, packing and grid at <64, 0, 64, 2, 1, 1, ...>
static void launch_lstm4_r(nrv_handle* h, int layer, const ActView (&in0)[2], float* const out[2], int T, int n, int tiles) {
  LstmH2Args sa;
  sa.T = T; sa.n_rows = n;
  for (int m = 0; m < 2; ++m) {
    const DevModel& d = h->dm[m];
    sa.m[m] = LstmH2ModelParams{d.all + d.l_w2sf[layer], d.all + d.l_b2sf[layer], d.all + d.l_s2[layer], d.all + d.l_h2[layer],
                                in0[m], ActView{}, out[m], d.descale_f[layer]};
  }
  sa.n_blk = (tiles + 1) / 2;                        // 64 rows per workgroup
  dim3 grid(lstm_grid(sa.n_blk)), blk(kL4rThreads);
  if (h->act == 0) hipLaunchKernelGGL(lstm4_r_kernel<0>, grid, blk, 0, h->stream, sa);
  NRV_ACT1(else hipLaunchKernelGGL(lstm4_r_kernel<1>, grid, blk, 0, h->stream, sa);)
}

#ifndef NRV_L3_WS_NBG
#define NRV_L3_WS_NBG 4                              // weight ring: 4 entries (8: 36 B of scratch and 2 % slower, r04w)
#endif
template <int KQ0, int KQ1, int H>
static void launch_lstm_h2w(nrv_handle* h, int layer, const ActView (&in0)[2], const ActView (&in1)[2],
                            float* const out[2], int T, int n, int tiles) {
  LstmH2Args sa;
  sa.T = T; sa.n_rows = n;
  for (int m = 0; m < 2; ++m) {
    const DevModel& d = h->dm[m];
    sa.m[m] = LstmH2ModelParams{d.all + d.l_w2sf[layer], d.all + d.l_b2sf[layer], d.all + d.l_s2[layer], d.all + d.l_h2[layer],
                                in0[m], in1[m], out[m], d.descale_f[layer]};
  }
  sa.n_blk = (tiles + 1) / 2;                        // 64 rows per workgroup
  dim3 grid(lstm_grid(sa.n_blk)), blk(512);
  if (h->act == 0) hipLaunchKernelGGL((lstm_h2w_kernel<KQ0, KQ1, H, 0, NRV_L3_WS_NBG>), grid, blk, 0, h->stream, sa);
  NRV_ACT1(else hipLaunchKernelGGL((lstm_h2w_kernel<KQ0, KQ1, H, 1, NRV_L3_WS_NBG>), grid, blk, 0, h->stream, sa);)
}

// Diagnostic build only (-DNRV_STAMP=1): nrv_exp_only_stage(k) makes every later group launch ONLY stage k of the f16x2 mode
// (0 signal branch, 2 32->64, 3 192->128, 4 256->64, 5 head; -1 all) on whatever the buffers hold - for per-kernel power /
// clock readings (scripts/gpu_power_probe.sh).  The product has no such switch.
#if NRV_STAMP
static int g_only_stage = -1;
#define NRV_RUN_STAGE(k) (g_only_stage < 0 || g_only_stage == (k))
#else
#define NRV_RUN_STAGE(k) true
#endif

// One launch group: n windows (n <= batch).  read_mode: inputs are per-event arrays holding
// n + T - 1 events and the windows are formed on the device.  sat: the range-guard counter of the f16x2
// signal branch for this group (one of h->d_sat's).
static int run_group(nrv_handle* h, const float* d_sig, const float* d_feat, int n, bool read_mode,
                     float* d_p1, float* d_p2, int8_t* d_a1, int8_t* d_a2, unsigned* sat) {
  const int T = h->T;
  const int tiles = (n + 31) / 32;
  if (h->poison_on) {                // NRV_POISON: this group's activation set holds nothing but the pattern
    for (int m = 0; m < 2; ++m) {
      float* const bufs[5] = {h->S[m], h->X1[m], h->X2[m], h->X3[m], h->MO[m]};
      for (int i = 0; i < 5; ++i) {
        const int rc0 = poison_fill(h, bufs[i], h->act_n[i] * 4, h->stream);
        if (rc0) return rc0;
      }
    }
  }
  hipEvent_t* ev = nullptr;
  // prof 3: only every 8th group is bracketed (an event record costs ~6 us of idle pipe)
  if (h->prof && (h->prof != 3 || (h->prof_tick++ & 7) == 0)) {
    if (h->ev_used + NRV_N_KERNELS + 1 > h->ev_pool.size()) {
      for (int i = 0; i < NRV_N_KERNELS + 1; ++i) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreate(&e));
        h->ev_pool.push_back(e);
      }
    }
    ev = h->ev_pool.data() + h->ev_used;
    h->ev_used += NRV_N_KERNELS + 1;
    if (h->prof == 1) HIPCHK(h, hipEventRecord(ev[0], h->stream));
  }
  auto mark = [&](int k) -> int {
    if (ev && (h->prof == 1 || k == 3 || k == 4)) HIPCHK(h, hipEventRecord(ev[k], h->stream));
    return NRV_OK;
  };
  int rc;

  bool h2_fused_l1 = false;          // f16x2 mode: the 6 -> 16 Bi-LSTM ran inside the signal-branch launch
  // 0: signal branch.  (Running it on a second stream beside lstm1/lstm2 was measured: the
  // dispatcher serialises the two launches anyway - each fills the LDS/register file of every CU -
  // and the event fork/join costs ~20 us per group, so everything stays on one stream.)
  {
    const int n_rows = read_mode ? n + T - 1 : n, Tc = read_mode ? 1 : T;
    const int n_tiles = read_mode ? (n + T - 1 + 31) / 32 : tiles * T;
    // persistent workgroups, one per CU: 128 per model (blockIdx.y) on the 256 CUs
    const int blocks = n_tiles < 128 ? n_tiles : 128;
    if (h->h2) {
      CnnRArgs a2;
      for (int m = 0; m < 2; ++m) {
        const DevModel& d = h->dm[m];
        a2.m[m] = CnnRModelParams{d.all + d.cr_w2, d.all + d.cr_ep, d.all + d.cr_d, d.all + d.cr_dbias, h->S[m]};
        a2.k[m] = d.cr_k;
      }
      a2.signal = d_sig; a2.T = Tc; a2.n_rows = n_rows; a2.n_tiles = n_tiles; a2.sat = sat;
      // the 6 -> 16 Bi-LSTM of this group rides along as four more waves per workgroup (nrv_cnn_r.h)
      a2.l1_T = T; a2.l1_rows = n;
      for (int m = 0; m < 2; ++m) {
        const DevModel& d = h->dm[m];
        a2.l1[m] = Lstm1ModelParams{d.all + d.l1w16, d.all + d.l1b16, d.all + d.l1s2, d.all + d.l1h2, d_feat,
                                    read_mode ? 1 : 0, h->X1[m]};
      }
      // persistent, one workgroup of eight + four waves per CU and model; a conv wave takes 16-event units round-robin
      // workgroups per model: enough for the conv units (8 waves each) AND for the 6 -> 16 layer's units (4 waves each,
      // 2 units per 16 windows) - in read mode the signal branch runs per EVENT (n + T - 1 of them) but the 6 -> 16 layer
      // still per (window, step): sized by the conv units alone its 512 units queued on 33 workgroups
      const int wg_c = (2 * n_tiles + kCnnRWaves - 1) / kCnnRWaves, wg_l = (2 * ((n + 15) / 16) + kCnnRL1Waves - 1) / kCnnRL1Waves;
      const int wg = wg_c > wg_l ? wg_c : wg_l;
      if (!NRV_RUN_STAGE(0)) {}
      else if (h->act == 0) hipLaunchKernelGGL(cnn_r_kernel<0>, dim3(wg < 128 ? wg : 128, 2), dim3(kCnnRThreads), 0, h->stream, a2);
      NRV_ACT1(else hipLaunchKernelGGL(cnn_r_kernel<1>, dim3(wg < 128 ? wg : 128, 2), dim3(kCnnRThreads), 0, h->stream, a2);)
      h2_fused_l1 = true;
    } else {
      CnnArgs a;
      for (int m = 0; m < 2; ++m) {
        const DevModel& d = h->dm[m];
        a.m[m] = CnnModelParams{d.all + d.conv, d.all + d.dpack, d.all + d.dbias, d.all + d.dsplit, h->S[m]};
      }
      a.signal = d_sig; a.T = Tc; a.n_rows = n_rows; a.n_tiles = n_tiles;
#ifndef NRV_DEV_FAST
      if (h->split & 32) hipLaunchKernelGGL(cnn_kernel<true>, dim3(blocks, 2), dim3(kCnnThreads), 0, h->stream, a);
      else hipLaunchKernelGGL(cnn_kernel<false>, dim3(blocks, 2), dim3(kCnnThreads), 0, h->stream, a);
#endif
    }
    if ((rc = mark(1))) return rc;
  }
  auto win_view = [&](const float* p, int kq) { return ActView{p, kq, 0, T, 1}; };
  // 1..4: Bi-LSTM layers
  {
    LstmArgs a;
    a.T = T; a.n_rows = n;
    if (!h2_fused_l1) {                          // the dedicated 16x16x4 kernel (f32 in every mode)
      Lstm1Args a1;
      a1.T = T; a1.n_rows = n;
      for (int m = 0; m < 2; ++m) {
        const DevModel& d = h->dm[m];
        a1.m[m] = Lstm1ModelParams{d.all + d.l1w16, d.all + d.l1b16, d.all + (h->h2 ? d.l1s2 : d.l_s[0]),
                                   d.all + (h->h2 ? d.l1h2 : d.l_h[0]), d_feat, read_mode ? 1 : 0, h->X1[m]};
      }
      dim3 grid((n + 63) / 64, 2, 2);
      if (h->h2) {
        if (h->act == 0) hipLaunchKernelGGL((lstm1_kernel<0, true>), grid, dim3(256), 0, h->stream, a1);
        NRV_ACT1(else hipLaunchKernelGGL((lstm1_kernel<1, true>), grid, dim3(256), 0, h->stream, a1);)
      } else if (h->act == 0) hipLaunchKernelGGL(lstm1_kernel<0>, grid, dim3(256), 0, h->stream, a1);
      NRV_ACT1(else hipLaunchKernelGGL(lstm1_kernel<1>, grid, dim3(256), 0, h->stream, a1);)
    }
    if ((rc = mark(2))) return rc;
    for (int m = 0; m < 2; ++m) {
      const DevModel& d = h->dm[m];
      a.m[m] = LstmModelParams{d.all + d.l_w[1], d.all + d.l_b[1], d.all + d.l_s[1], d.all + d.l_h[1],
                               win_view(h->X1[m], 8), ActView{}, nullptr, 0, h->X2[m]};
    }
    const ActView none[2] = {ActView{}, ActView{}};
    if (h->h2) {
      // transposed kernel, one 32-row chain per workgroup; hands over h x 2^13 (BatchNorm(128) is in the 192->128 layer's
      // weights).  Whole 64-row blocks, as the layers around it: two chains per block.
      Lstm2RArgs ta;
      ta.T = T; ta.n_rows = n;
      for (int m = 0; m < 2; ++m) {
        const DevModel& d = h->dm[m];
        ta.m[m] = Lstm2RModelParams{d.all + d.l2t_w, d.all + d.l2t_b, h->X1[m], h->X2[m], d.descale[1]};
      }
      dim3 grid(2 * ((n + 63) / 64), 2, 2);
      if (!NRV_RUN_STAGE(2)) {}
      else if (h->act == 0) hipLaunchKernelGGL(lstm2_r_kernel<0>, grid, dim3(kL2rThreads), 0, h->stream, ta);
      NRV_ACT1(else hipLaunchKernelGGL(lstm2_r_kernel<1>, grid, dim3(kL2rThreads), 0, h->stream, ta);)
    }
    else if (h->split & 2) {
      const float* ws[2] = {h->dm[0].all + h->dm[0].l_ws[1], h->dm[1].all + h->dm[1].l_ws[1]};
      launch_lstm_split<8, 0, 64, 1, 2>(h, a, ws, tiles);
    } else {
      launch_lstm_f32<8, 0, 64, 1, 2>(h, a, tiles);
    }
    if ((rc = mark(3))) return rc;
    for (int m = 0; m < 2; ++m) {
      const DevModel& d = h->dm[m];
      ActView sv = read_mode ? ActView{h->S[m], 16, 1, 1, 0} : win_view(h->S[m], 16);
      a.m[m] = LstmModelParams{d.all + d.l_w[2], d.all + d.l_b[2], d.all + d.l_s[2], d.all + d.l_h[2],
                               win_view(h->X2[m], 32), sv, nullptr, 0, h->X3[m]};
    }
    if (h->h2) {
      const ActView i0[2] = {win_view(h->X2[0], 32), win_view(h->X2[1], 32)};
      const ActView i1[2] = {read_mode ? ActView{h->S[0], 16, 1, 1, 0} : win_view(h->S[0], 16),
                             read_mode ? ActView{h->S[1], 16, 1, 1, 0} : win_view(h->S[1], 16)};
      float* const o[2] = {h->X3[0], h->X3[1]};
      // both big layers on lstm_h2s_kernel: this one hands over h x 2^13 as it lies in LDS and the BatchNorm
      // behind it lives in the next layer's weights
      // (cell state in registers; 1 of its 10 weight k-blocks of 32 resident in LDS: 64 KB)
      if (NRV_RUN_STAGE(3)) launch_lstm_h2w<32, 16, 128>(h, 2, i0, i1, o, T, n, tiles);
    } else if (h->split & 4) {
      const float* ws[2] = {h->dm[0].all + h->dm[0].l_ws[2], h->dm[1].all + h->dm[1].l_ws[2]};
      launch_lstm_split<32, 16, 128, 2, 1>(h, a, ws, tiles);
    } else {
      launch_lstm_f32<32, 16, 128, 1, 1>(h, a, tiles);
    }
    if ((rc = mark(4))) return rc;
    if (h->fit.l3_slot && fit_at(h).sg) {        // ... at depth NRV_FIT_SIGNAL: lstm2's output and the samples
      SigGatherArgs g;
      for (int m = 0; m < 2; ++m) { g.in0[m] = win_view(h->X2[m], 32); g.x2[m] = h->fit.x[m]; }
      g.sig_ev = d_sig; g.sig = h->fit.shared[0];
      g.slot = h->fit.l3_slot; g.n = n; g.T = T; g.cap = h->fit.cap;
      const long long total = (long long)n * T * 57;
      hipLaunchKernelGGL(sig_gather_kernel, dim3((unsigned)((total + 255) / 256), 2), dim3(256), 0, h->stream, g);
    } else
    if (h->fit.l3_slot) {                        // nrv_fit_add_reads_raw at depth NRV_FIT_LSTM3: lstm3's two inputs of the group's
      L3GatherArgs g;                            // labelled windows, before the next launch writes X4 over X2
      for (int m = 0; m < 2; ++m) {
        g.in0[m] = win_view(h->X2[m], 32);
        g.in1[m] = read_mode ? ActView{h->S[m], 16, 1, 1, 0} : win_view(h->S[m], 16);
        g.x[m] = h->fit.x[m];
      }
      g.slot = h->fit.l3_slot; g.n = n; g.T = T; g.cap = h->fit.cap;
      const long long total = (long long)n * T * 48;
      hipLaunchKernelGGL(l3_gather_kernel, dim3((unsigned)((total + 255) / 256), 2), dim3(256), 0, h->stream, g);
    }
    for (int m = 0; m < 2; ++m) {
      const DevModel& d = h->dm[m];
      a.m[m] = LstmModelParams{d.all + d.l_w[3], d.all + d.l_b[3], d.all + d.l_s[3], d.all + d.l_h[3],
                               win_view(h->X3[m], 64), ActView{}, nullptr, 0, h->X2[m] /* X4 aliases X2 */};
    }
    if (h->h2) {
      const ActView i0[2] = {win_view(h->X3[0], 64), win_view(h->X3[1], 64)};
      float* const o[2] = {h->X2[0], h->X2[1]};           // X4 aliases X2; split planes for head_h2_kernel
      // no BatchNorm behind this layer (raw copy-out); the one in front of it is folded into its weights;
      // of its 10 weight k-blocks of 32, 3 stay in LDS (96 KB), 5 in registers, 2 are streamed (lstm4_r_kernel)
#if defined(NRV_L4_H2S) || NRV_STAMP                      // development builds: the kernel before r08, to time one against the other; the stamps live in it
      if (NRV_RUN_STAGE(4)) launch_lstm_h2s<64, 0, 64, 2, 1, 1, 8, 2, 3, true>(h, 3, i0, none, o, T, n, tiles);
#else
      if (NRV_RUN_STAGE(4)) launch_lstm4_r(h, 3, i0, o, T, n, tiles);
#endif
    } else if (h->split & 8) {
      const float* ws[2] = {h->dm[0].all + h->dm[0].l_ws[3], h->dm[1].all + h->dm[1].l_ws[3]};
      launch_lstm_split<64, 0, 64, 1, 2>(h, a, ws, tiles);
    } else {
      launch_lstm_f32<64, 0, 64, 1, 2>(h, a, tiles);
    }
    if ((rc = mark(5))) return rc;
  }
  // 5: head
  {
    float* dp[2] = {d_p1 ? d_p1 : h->d_p[0][0], d_p2 ? d_p2 : h->d_p[0][1]};
    int8_t* da[2] = {d_a1 ? d_a1 : h->d_a[0][0], d_a2 ? d_a2 : h->d_a[0][1]};
    if (h->h2) {
      HeadH2Args ha;
      ha.T = T; ha.n_rows = n; ha.n_tiles = tiles;
      for (int m = 0; m < 2; ++m) {
        const DevModel& d = h->dm[m];
        ha.m[m] = HeadH2ModelParams{d.all + d.h_w2, d.all + d.h_b2, h->X2[m], d.all + d.fw8, d.all + d.fb, d.all + d.ow,
                                    d.all + d.ob, dp[m], da[m], d.hsc.c12, d.hsc.c23, d.hsc.c3o, d.C};
      }
      if (NRV_RUN_STAGE(5)) hipLaunchKernelGGL(head_h2_kernel, dim3(tiles < 128 ? tiles : 128, 2), dim3(kHeadH2Threads), 0, h->stream, ha);
      if ((rc = mark(6))) return rc;
      HIPCHK(h, hipGetLastError());
      return NRV_OK;
    }
    HeadArgs a;
    a.T = T; a.n_rows = n;
    for (int m = 0; m < 2; ++m) {
      const DevModel& d = h->dm[m];
      a.m[m] = HeadModelParams{d.all + d.d1p, d.all + d.d1b, d.all + d.d2p, d.all + d.d2b,
                               d.all + d.mop, d.all + d.mob, d.all + d.fw, d.all + d.fb,
                               d.all + d.ow, d.all + d.ob, h->X2[m], h->MO[m], dp[m], da[m], d.C};
    }
    if (h->split & 16) {
      HeadSplitArgs sa;
      sa.n_units = tiles * T;
      for (int m = 0; m < 2; ++m) {
        const DevModel& d = h->dm[m];
        sa.m[m] = HeadSplitModelParams{d.all + d.h_ws, d.all + d.h_wb, h->X2[m], h->MO[m]};
      }
      const int blocks = sa.n_units < 512 ? (sa.n_units + 3) / 4 : 128;    // persistent: one per CU and model
#ifndef NRV_DEV_FAST
      hipLaunchKernelGGL(head_mlp_split_kernel, dim3(blocks, 2), dim3(256), 0, h->stream, sa);
    } else {
      hipLaunchKernelGGL(head_mlp_kernel, dim3(tiles * T, 2), dim3(64), 0, h->stream, a);
#endif
    }
#ifndef NRV_DEV_FAST
    hipLaunchKernelGGL(head_final_kernel, dim3(tiles, 2), dim3(256), 0, h->stream, a);
#endif
    if ((rc = mark(6))) return rc;
  }
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}

static int prof_collect(nrv_handle* h) {
  if (h->ev_used == 0) return NRV_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t g = 0; g + NRV_N_KERNELS + 1 <= h->ev_used; g += NRV_N_KERNELS + 1)
    for (int k = 0; k < NRV_N_KERNELS; ++k) {
      if (h->prof != 1 && k != 3) continue;
      float ms = 0.f;
      HIPCHK(h, hipEventElapsedTime(&ms, h->ev_pool[g + k], h->ev_pool[g + k + 1]));
      h->prof_ms[k] += ms;
      h->prof_n[k] += 1;
    }
  h->ev_used = 0;
  return NRV_OK;
}

static int check_handle(nrv_handle* h) {
  if (!h) return NRV_E_INVALID;
  hipError_t e = hipSetDevice(h->device);
  if (e != hipSuccess) { h->err = std::string("hipSetDevice: ") + hipGetErrorString(e); return NRV_E_HIP; }
  return NRV_OK;
}

}  // namespace

extern "C" {

int nrv_create(const nrv_weights* m1, const nrv_weights* m2, int T, int device, int recurrent_act,
               nrv_handle** out) {
  if (!out) { g_create_error = "nrv_create: out is NULL"; return NRV_E_INVALID; }
  *out = nullptr;
  if (T < 1 || T > kMaxT) { g_create_error = "nrv_create: window length T out of range [1,32]"; return NRV_E_INVALID; }
  if (recurrent_act != 0 && recurrent_act != 1) { g_create_error = "nrv_create: recurrent_act must be 0 or 1"; return NRV_E_INVALID; }
  Blob b1, b2;
  if (!make_blob(m1, T, 6, &b1)) { g_create_error = "nrv_create: model1 blob size does not match the graph for this T (expect 6 classes)"; return NRV_E_WEIGHTS; }
  if (!make_blob(m2, T, 5, &b2)) { g_create_error = "nrv_create: model2 blob size does not match the graph for this T (expect 5 classes)"; return NRV_E_WEIGHTS; }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_create_error = std::string("nrv_create: no HIP device (") + hipGetErrorString(e) + "); this library has no CPU fallback";
    return NRV_E_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) { g_create_error = "nrv_create: device index out of range"; return NRV_E_NO_DEVICE; }
  e = hipSetDevice(device);
  if (e != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return NRV_E_HIP; }
  nrv_handle* h = new (std::nothrow) nrv_handle();
  if (!h) { g_create_error = "out of host memory"; return NRV_E_NOMEM; }
  h->device = device; h->T = T; h->act = recurrent_act;
  if (const char* s = getenv("NRV_PRECISION")) {                       // initial nrv_set_precision mode
    if (!strcmp(s, "f32")) { h->split = 0; h->h2 = 0; }
    else if (!strcmp(s, "bf16x3")) { h->split = 62; h->h2 = 0; }
    else if (!strcmp(s, "f16x2")) { h->split = 62; h->h2 = 1; }
  }
  int rc = NRV_OK;
  // a BLOCKING stream: it orders itself against the legacy default stream, so inputs produced on
  // the default stream (torch's default) are complete before our first kernel reads them
  e = hipStreamCreateWithFlags(&h->own_stream, hipStreamDefault);
  if (e != hipSuccess) { g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e); delete h; return NRV_E_HIP; }
  h->stream = h->own_stream;
  bool ok = hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&h->d2h_stream, hipStreamNonBlocking) == hipSuccess;
  for (int st = 0; st < nrv_handle::kIn && ok; ++st) ok = hipEventCreateWithFlags(&h->ev_in[st], hipEventDisableTiming) == hipSuccess;
  for (int st = 0; st < 2 && ok; ++st)
    ok = hipEventCreateWithFlags(&h->ev_done[st], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&h->ev_out[st], hipEventDisableTiming) == hipSuccess;
  if (const char* e2 = getenv("NRV_HOST_REGISTER")) h->host_register = atoi(e2) != 0;
  if (const char* e3 = getenv("NRV_LANES")) h->lanes_on = atoi(e3) != 0;
  if (const char* e4 = getenv("NRV_COALESCE")) h->coalesce = atoi(e4) != 0;
  if (const char* e6 = getenv("NRV_LABELS_BUDGET"); e6 && *e6) { const long long v = atoll(e6); if (v > 0) h->lab_budget = (size_t)v; }
  for (int i = 0; i < 6; ++i) {                             // the row caps of the fit depths: the default, or the depth's variable
    const long long lim = ((long long)1 << 31) - 1;
    const char* e = getenv(kFitDepths[i].env);
    const long long v = e && *e ? atoll(e) : 0;
    h->fit.max_rows[i] = v > 0 ? (v > lim ? lim : v) : kFitDepths[i].max_rows;
  }
  if (const char* e5 = getenv("NRV_POISON"); e5 && *e5) { h->poison_on = true; h->poison = (unsigned)strtoul(e5, nullptr, 16); }
  ok = ok && hipMalloc((void**)&h->d_sat, 4 * sizeof(unsigned)) == hipSuccess &&
       hipMemset(h->d_sat, 0, 4 * sizeof(unsigned)) == hipSuccess;
  if (!ok) { g_create_error = "nrv_create: could not create the copy stream / events / counters"; nrv_destroy(h); return NRV_E_HIP; }
  if ((rc = upload_model(h, 0, b1, 6)) || (rc = upload_model(h, 1, b2, 5)) || (rc = ensure_workspace(h))) {
    g_create_error = h->err;
    nrv_destroy(h);
    return rc;
  }
  *out = h;
  return NRV_OK;
}

void nrv_destroy(nrv_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  free_workspace(h);
  free_lanes(h);
  for (int l = 0; l < nrv_handle::kMaxLanes; ++l) {
    if (h->lanes[l].done) (void)hipEventDestroy(h->lanes[l].done);
    if (h->lanes[l].stream) (void)hipStreamDestroy(h->lanes[l].stream);
  }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  for (int m = 0; m < 2; ++m) (void)hipFree(h->dm[m].all);
  for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
  if (h->copy_stream) { (void)hipStreamSynchronize(h->copy_stream); (void)hipStreamDestroy(h->copy_stream); }
  if (h->d2h_stream) { (void)hipStreamSynchronize(h->d2h_stream); (void)hipStreamDestroy(h->d2h_stream); }
  if (h->edit_stream) { (void)hipStreamSynchronize(h->edit_stream); (void)hipStreamDestroy(h->edit_stream); }
  if (h->lab_stream) { (void)hipStreamSynchronize(h->lab_stream); (void)hipStreamDestroy(h->lab_stream); }
  (void)hipFree(h->d_lab);
  for (char* p : h->lab_retired) (void)hipFree(p);
  for (int m = 0; m < 2; ++m) {
    (void)hipFree(h->fit.x[m]); (void)hipFree(h->fit.shared[m]); (void)hipFree(h->fit.y[m]);
    (void)hipFree(h->fit.m[m].d_par); (void)hipFree(h->fit.m[m].d_state); (void)hipFree(h->fit.m[m].d_lr);
    (void)hipFree(h->fit.m[m].d_bn); (void)hipFree(h->fit.m[m].d_bnacc);
  }
  (void)hipFree(h->fit.d_partial); (void)hipFree(h->fit.d_pstat); (void)hipFree(h->fit.d_order); (void)hipFree(h->fit.d_p); (void)hipFree(h->fit.d_flag);
  (void)hipFree(h->fit.d_l4); (void)hipFree(h->fit.d_gl4); (void)hipFree(h->fit.d_bnpart); (void)hipFree(h->fit.d_pbn); (void)hipFree(h->fit.d_mask);
  (void)hipFree(h->fit.d_l3); (void)hipFree(h->fit.d_gl3); (void)hipFree(h->fit.d_ident);
  (void)hipFree(h->fit.d_rd); (void)hipFree(h->fit.d_grd);
  (void)hipFree(h->fit.d_sg); (void)hipFree(h->fit.d_pconv); (void)hipFree(h->fit.d_gdense);
  for (int st = 0; st < nrv_handle::kIn; ++st) if (h->ev_in[st]) (void)hipEventDestroy(h->ev_in[st]);
  for (int st = 0; st < 2; ++st) {
    if (h->ev_done[st]) (void)hipEventDestroy(h->ev_done[st]);
    if (h->ev_out[st]) (void)hipEventDestroy(h->ev_out[st]);
  }
  (void)hipFree(h->d_raw); (void)hipFree(h->d_starts); (void)hipFree(h->d_reads);
  for (auto& sl : h->raw_slot) {
    (void)hipFree(sl.d_in); (void)hipFree(sl.d_out); (void)hipHostFree(sl.pin_in); (void)hipHostFree(sl.pin_out);
    (void)hipFree(sl.d_stat);
    (void)hipFree(sl.d_mrg); (void)hipHostFree(sl.pin_mrg);
    if (sl.ev_in) (void)hipEventDestroy(sl.ev_in);
    if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
    if (sl.ev_out) (void)hipEventDestroy(sl.ev_out);
  }
  (void)hipFree(h->d_sat);
  if (h->ev_raw) (void)hipEventDestroy(h->ev_raw);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
}

int nrv_set_batch(nrv_handle* h, int batch) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (batch < 1 || batch > (1 << 20)) { h->err = "nrv_set_batch: batch out of range"; return NRV_E_INVALID; }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->batch = batch;
  if ((rc = ensure_workspace(h))) return rc;
  return ensure_lanes(h);
}
int nrv_get_batch(nrv_handle* h) { return h ? h->batch : NRV_E_INVALID; }

int nrv_set_precision(nrv_handle* h, int mode) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (mode != NRV_PREC_F32 && mode != NRV_PREC_BF16X3 && mode != NRV_PREC_F16X2) {
    h->err = "nrv_set_precision: unknown mode";
    return NRV_E_INVALID;
  }
  h->split = mode == NRV_PREC_F32 ? 0 : 62;
  h->h2 = mode == NRV_PREC_F16X2;
  return NRV_OK;
}
int nrv_get_precision(nrv_handle* h) {
  if (!h) return NRV_E_INVALID;
  return h->h2 ? NRV_PREC_F16X2 : (h->split ? NRV_PREC_BF16X3 : NRV_PREC_F32);
}

int nrv_set_stream(nrv_handle* h, void* s) {
  int rc = check_handle(h);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->stream = s ? (hipStream_t)s : h->own_stream;
  return NRV_OK;
}

int nrv_sync(nrv_handle* h) {
  int rc = check_handle(h);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return NRV_OK;
}

}  // extern "C"

// The launch groups of a device-pointer call: in order on the handle's stream, or - small groups -
// round-robin over the lanes: every lane stream starts behind what the handle's stream holds at entry
// (the caller's inputs) and the handle's stream ends behind every lane.  body(first window, windows).
template <class F>
static int for_groups(nrv_handle* h, int64_t n, F&& body) {
  const int64_t G = group_windows(h);
  const int64_t ng = (n + G - 1) / G;
  int nl = (h->n_lanes > 1 && ng > 1 && h->prof == 0) ? h->n_lanes : 0;
  if ((int64_t)nl > ng) nl = (int)ng;
  hipStream_t main = h->stream;
  float* keep[5][2];
  for (int m = 0; m < 2; ++m) { keep[0][m] = h->S[m]; keep[1][m] = h->X1[m]; keep[2][m] = h->X2[m]; keep[3][m] = h->X3[m]; keep[4][m] = h->MO[m]; }
  size_t keep_n[5];
  memcpy(keep_n, h->act_n, sizeof keep_n);
  auto restore = [&]() {
    for (int m = 0; m < 2; ++m) { h->S[m] = keep[0][m]; h->X1[m] = keep[1][m]; h->X2[m] = keep[2][m]; h->X3[m] = keep[3][m]; h->MO[m] = keep[4][m]; }
    memcpy(h->act_n, keep_n, sizeof keep_n);
    h->stream = main;
  };
  if (nl) {
    HIPCHK(h, hipEventRecord(h->ev_fork, main));
    for (int l = 0; l < nl; ++l) HIPCHK(h, hipStreamWaitEvent(h->lanes[l].stream, h->ev_fork, 0));
  }
  int rc = NRV_OK;
  int64_t g = 0;
  for (int64_t s = 0; s < n && !rc; s += G, ++g) {
    const int nb = (int)((n - s < G) ? (n - s) : G);
    if (nl) {
      const nrv_handle::Lane& L = h->lanes[g % nl];
      for (int m = 0; m < 2; ++m) { h->S[m] = L.S[m]; h->X1[m] = L.X1[m]; h->X2[m] = L.X2[m]; h->X3[m] = L.X3[m]; h->MO[m] = L.MO[m]; }
      memcpy(h->act_n, L.act_n, sizeof L.act_n);
      h->stream = L.stream;
    }
    rc = body(s, nb);
  }
  restore();
  if (nl) {
    for (int l = 0; l < nl; ++l) {
      hipError_t e = hipEventRecord(h->lanes[l].done, h->lanes[l].stream);
      if (e == hipSuccess) e = hipStreamWaitEvent(main, h->lanes[l].done, 0);
      if (e != hipSuccess && !rc) { h->err = std::string("lane join: ") + hipGetErrorString(e); rc = NRV_E_HIP; }
    }
  }
  return rc;
}

// a synchronous entry point of the raw-read family: its _begin, then nrv_reads_raw_end
template <class Begin>
static int begin_then_end(nrv_handle* h, Begin begin) {
  int t = -1;
  const int rc = begin(&t);
  return rc ? rc : nrv_reads_raw_end(h, t);
}
// What a merged call hands back, from `head`, the host's copy of the first m.dl bytes of the block v.blk: the three totals are
// checked against what the block can hold, the blocks copied out, and the used prefix of the edit records and of the blob fetched
// with fetch(dst, offset into the block, bytes) -> status, the caller's way of reading the device block.  who names the entry point
// in the error texts, who_edits in the edit list's (nrv_merge_calls_edits has a text of its own)
template <class Fetch>
static int merged_collect(nrv_handle* h, const char* who, const char* who_edits, const char* head, const MergeView& v,
                          const MergeLayout& m, const MergeOut& o, bool want_q, size_t blob_cap, Fetch fetch) {
  const int64_t n = v.N - h->T > 0 ? v.N - h->T : 0;
  const size_t nb = ((size_t)v.n_reads + 1) * 8;
  const int64_t total = ((const int64_t*)head)[v.n_reads];
  if (total < 0 || total > v.N + n) { h->err = std::string(who) + ": merged block out of range"; return NRV_E_HIP; }
  memcpy(o.off, head, nb);
  if (o.seq) memcpy(o.seq, head + m.seq, (size_t)total);
  if (want_q && o.qual) memcpy(o.qual, head + m.qual, (size_t)total);
  if (o.report) memcpy(o.report, head + m.rep, (size_t)v.n_reads * kReportCols * 8);
  if (o.profile) memcpy(o.profile, head + m.prof, (size_t)v.n_reads * kProfileCols * 8);
  if (o.trim) memcpy(o.trim, head + m.trim, (size_t)v.n_reads * 16);
  if (o.accuracy) memcpy(o.accuracy, head + m.accu, (size_t)v.n_reads * kAccuracyCols * 8);
  if (o.errclass) memcpy(o.errclass, head + m.ecls, (size_t)v.n_reads * kErrclassCols * 8);
  if (o.infix) memcpy(o.infix, head + m.infx, (size_t)v.n_reads * kInfixCols * 8);
  if (o.score) memcpy(o.score, head + m.scor, (size_t)v.n_reads * kScoreCols * 8);
  int rc = NRV_OK;
  if (o.edit_off) {
    const int64_t n_ed = ((const int64_t*)(head + m.eoff))[v.n_reads];
    if (n_ed < 0 || n_ed > n) { h->err = std::string(who_edits) + ": edit list out of range"; return NRV_E_HIP; }
    memcpy(o.edit_off, head + m.eoff, nb);
    if (n_ed > 0 && (rc = fetch(o.edits, m.edits, (size_t)n_ed * sizeof(nrv_edit)))) return rc;
  }
  if (o.rec_off) {
    const int64_t n_b = ((const int64_t*)(head + m.roff))[v.n_reads];
    if (n_b < 0 || (uint64_t)n_b > blob_cap) { h->err = std::string(who) + ": records out of range"; return NRV_E_HIP; }
    memcpy(o.rec_off, head + m.roff, nb);
    if (n_b > 0 && (rc = fetch(o.blob, m.blob, (size_t)n_b))) return rc;
  }
  return NRV_OK;
}

// the lengths of an infix call: no sequence (region, or - lens given - read that has a region) above NRV_INFIX_MAX_LEN
static bool infix_lengths_ok(const int64_t* truth_off, int n, const int64_t* len_off = nullptr, const nrv_read_desc* reads = nullptr) {
  for (int r = 0; r < n; ++r) {
    const int64_t m = truth_off[r + 1] - truth_off[r];
    if (m > NRV_INFIX_MAX_LEN) return false;
    if (m > 0 && len_off && len_off[r + 1] - len_off[r] > NRV_INFIX_MAX_LEN) return false;
    if (m > 0 && reads && reads[r].ev_len > NRV_INFIX_MAX_LEN) return false;
  }
  return true;
}
// a truth set: offsets that ascend from 0, bytes where there are any, and no sequence of 2^31 - 64 characters or more
static bool truth_ok(const uint8_t* truth, const int64_t* truth_off, int n_reads) {
  if (!truth_off || truth_off[0] != 0) return false;
  for (int r = 0; r < n_reads; ++r)
    if (truth_off[r + 1] < truth_off[r] || truth_off[r + 1] - truth_off[r] >= ((int64_t)1 << 31) - 64) return false;
  return truth != nullptr || truth_off[n_reads] == 0;
}
// What one of the three pair doors (nrv_edit_distance, nrv_edit_classes, nrv_infix_classes) brings to pair_door: its refusals
// to the letter and in the order they are tried, the bytes of carry per character of b, and its k outputs of int64[n_pairs]
struct PairDoor {
  const char* bad_args;                  // n_pairs < 0, or a null output
  const char* refused;                   // a refusal of the door's own, decided by the caller (null: none)
  const char* bad_pair;                  // a or b is no truth set (truth_ok)
  const char* bad_lengths;               // infix_lengths_ok (null: the door has no such limit)
  size_t carry;
  int k;
  int64_t* out[kPairMaxOuts];
};
// A pair door: the checks, one block of its own (pair_layout), the pair up, enqueue(the shared arguments, the carry, the k
// outputs on the device) for the door's own kernel, the k outputs down
template <class Enqueue>
static int pair_door(nrv_handle* h, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off, int n_pairs,
                     const PairDoor& w, Enqueue&& enqueue) {
  int rc = check_handle(h);
  if (rc) return rc;
  bool outs = true;
  for (int q = 0; q < w.k; ++q) outs = outs && w.out[q];
  if (n_pairs < 0 || (n_pairs > 0 && !outs)) { h->err = w.bad_args; return NRV_E_INVALID; }
  if (w.refused) { h->err = w.refused; return NRV_E_INVALID; }
  if (!truth_ok(a, a_off, n_pairs) || !truth_ok(b, b_off, n_pairs)) { h->err = w.bad_pair; return NRV_E_INVALID; }
  if (w.bad_lengths && !infix_lengths_ok(a_off, n_pairs, b_off)) { h->err = w.bad_lengths; return NRV_E_INVALID; }
  if (n_pairs == 0) return NRV_OK;
  const size_t nb = ((size_t)n_pairs + 1) * 8, ta = (size_t)a_off[n_pairs], tb = (size_t)b_off[n_pairs];
  const PairLayout l = pair_layout((size_t)n_pairs, ta, tb, w.carry, w.k);
  hipStream_t const s = h->stream;
  return with_block(h, l.bytes, s, [&](char* d) -> int {
    int rc2;
    if ((rc2 = put(h, d + l.a_off, a_off, nb, s)) || (rc2 = put(h, d + l.b_off, b_off, nb, s)) ||
        (rc2 = put(h, d + l.a, a, ta, s)) || (rc2 = put(h, d + l.b, b, tb, s)))
      return rc2;
    PairArgs k;                                           // one kind: a is the truth, b the text
    k.n_reads = n_pairs; k.kinds = 1;
    k.truth = (const unsigned char*)(d + l.a); k.truth_off = (const long long*)(d + l.a_off);
    k.reads = nullptr; k.bases = nullptr; k.cap0 = 0;
    k.off = (const long long*)(d + l.b_off); k.seq = (const unsigned char*)(d + l.b); k.cap1 = (long long)tb;
    long long* out[kPairMaxOuts] = {};
    for (int q = 0; q < w.k; ++q) out[q] = (long long*)(d + l.out[q]);
    if ((rc2 = enqueue(k, d + l.hc, out))) return rc2;
    for (int q = 0; q < w.k; ++q) HIPCHK(h, hipMemcpyAsync(w.out[q], d + l.out[q], (size_t)n_pairs * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return NRV_OK;
  });
}

extern "C" {

int nrv_predict_device(nrv_handle* h, const float* d_signal, const float* d_read, int64_t n,
                       float* d_p1, float* d_p2, int8_t* d_a1, int8_t* d_a2) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!d_signal || !d_read))) { h->err = "nrv_predict_device: bad arguments"; return NRV_E_INVALID; }
  const int T = h->T;
  return for_groups(h, n, [&](int64_t s, int nb) {
    return run_group(h, d_signal + s * T * kSig, d_read + s * T * kFeat, nb, false,
                     d_p1 ? d_p1 + s * 6 : nullptr, d_p2 ? d_p2 + s * 5 : nullptr,
                     d_a1 ? d_a1 + s : nullptr, d_a2 ? d_a2 + s : nullptr, h->d_sat + 2);
  });
}

int nrv_predict_read_device(nrv_handle* h, const float* d_sig_ev, const float* d_feat_ev, int64_t N,
                            float* d_p1, float* d_p2, int8_t* d_a1, int8_t* d_a2) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (N < 0 || (N > 0 && (!d_sig_ev || !d_feat_ev))) { h->err = "nrv_predict_read_device: bad arguments"; return NRV_E_INVALID; }
  const int T = h->T;
  const int64_t n = N - T;
  return for_groups(h, n, [&](int64_t s, int nb) {
    return run_group(h, d_sig_ev + s * kSig, d_feat_ev + s * kFeat, nb, true,
                     d_p1 ? d_p1 + s * 6 : nullptr, d_p2 ? d_p2 + s * 5 : nullptr,
                     d_a1 ? d_a1 + s : nullptr, d_a2 ? d_a2 + s : nullptr, h->d_sat + 2);
  });
}

// ---- raw-read path: upload samples / starts / descriptors once per call, cut windows per group ----
static int upload_raw(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts, int64_t N,
                      const nrv_read_desc* reads, int n_reads) {
  if (n_raw < 0 || N < 0 || n_reads < 0 || (n_raw > 0 && !raw) || (N > 0 && (!starts || !reads || n_reads == 0))) {
    h->err = "nrv raw reads: bad arguments";
    return NRV_E_INVALID;
  }
  int64_t ev = 0;
  for (int r = 0; r < n_reads; ++r) {          // descriptors must tile [0, N) in order and stay inside raw
    const nrv_read_desc& d = reads[r];
    if (d.ev_off != ev || d.ev_len < 0 || d.raw_off < 0 || d.raw_len < 0 || d.raw_off + d.raw_len > n_raw) {
      h->err = "nrv raw reads: read descriptors do not tile the event range / exceed the sample array";
      return NRV_E_INVALID;
    }
    ev += d.ev_len;
  }
  if (ev != N) { h->err = "nrv raw reads: read descriptors do not cover N events"; return NRV_E_INVALID; }
  static_assert(sizeof(SegRead) == sizeof(nrv_read_desc), "descriptor layouts must match");
  auto grow = [&](void** p, size_t* cap, size_t need) -> int {
    if (need <= *cap) return NRV_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    const size_t c = need + need / 2 + 4096;
    HIPCHK(h, hipMalloc(p, c));
    *cap = c;
    return NRV_OK;
  };
  int rc;
  if ((rc = grow((void**)&h->d_raw, &h->cap_raw, (size_t)n_raw * 2)) ||
      (rc = grow((void**)&h->d_starts, &h->cap_starts, (size_t)N * 4)) ||
      (rc = grow((void**)&h->d_reads, &h->cap_reads, (size_t)n_reads * sizeof(SegRead))))
    return rc;
  if (!h->ev_raw) HIPCHK(h, hipEventCreateWithFlags(&h->ev_raw, hipEventDisableTiming));
  // the previous call's kernels may still read these buffers only if the caller did not sync; the
  // host entry points always end synchronised, so plain stream order on the copy stream is enough
  if ((rc = poison_fill(h, h->d_raw, h->cap_raw, h->copy_stream)) || (rc = poison_fill(h, h->d_starts, h->cap_starts, h->copy_stream)) ||
      (rc = poison_fill(h, h->d_reads, h->cap_reads, h->copy_stream)))
    return rc;
  if (n_raw) HIPCHK(h, hipMemcpyAsync(h->d_raw, raw, (size_t)n_raw * 2, hipMemcpyHostToDevice, h->copy_stream));
  if (N) HIPCHK(h, hipMemcpyAsync(h->d_starts, starts, (size_t)N * 4, hipMemcpyHostToDevice, h->copy_stream));
  if (n_reads) HIPCHK(h, hipMemcpyAsync(h->d_reads, reads, (size_t)n_reads * sizeof(SegRead), hipMemcpyHostToDevice, h->copy_stream));
  HIPCHK(h, hipEventRecord(h->ev_raw, h->copy_stream));
  HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_raw, 0));
  return NRV_OK;
}

static void launch_segment(nrv_handle* h, int n_reads, int64_t ev0, int n_ev, float* d_out, const int16_t* d_raw = nullptr,
                           const int32_t* d_starts = nullptr, const SegRead* d_reads = nullptr) {
  if (n_ev <= 0) return;
  SegArgs a{(const short*)(d_raw ? d_raw : h->d_raw), (const int*)(d_starts ? d_starts : h->d_starts), d_reads ? d_reads : h->d_reads,
            n_reads, (long long)ev0, n_ev, d_out};
  const long long total = (long long)n_ev * 50;
  hipLaunchKernelGGL(segment_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, a);
}

// Caller memory registered (page-locked in place) for the duration of one call.
struct HostPin {
  void* p = nullptr;
  bool on = false;
  nrv_handle* owner = nullptr;
  bool settled = false;                           // the success path ends with its streams synchronised
  bool pin(nrv_handle* h, const void* ptr, size_t bytes) {
    owner = h;
    // below a few MB the registration costs more than the bounce copy it saves
    if (!h->host_register || !ptr || bytes < ((size_t)4 << 20)) return false;
    if (hipHostRegister(const_cast<void*>(ptr), bytes, hipHostRegisterDefault) != hipSuccess) {
      (void)hipGetLastError();                    // not registrable (e.g. a read-only mapping): bounce instead
      return false;
    }
    p = const_cast<void*>(ptr);
    on = true;
    return true;
  }
  void release() {
    if (!on) return;
    if (!settled) {                             // error paths: no DMA of THIS handle may still be reading the range
      (void)hipStreamSynchronize(owner->copy_stream);
      (void)hipStreamSynchronize(owner->stream);
      (void)hipStreamSynchronize(owner->d2h_stream);
    }
    (void)hipHostUnregister(p);
    on = false;
  }
  ~HostPin() { release(); }
};

static int grow_pinned(nrv_handle* h, char* (&buf)[nrv_handle::kIn], size_t* cap, size_t need) {
  if (need <= *cap) return NRV_OK;
  for (int st = 0; st < nrv_handle::kIn; ++st) {
    (void)hipHostFree(buf[st]);
    buf[st] = nullptr;
  }
  *cap = 0;
  for (int st = 0; st < nrv_handle::kIn; ++st) HIPCHK(h, hipHostMalloc((void**)&buf[st], need, hipHostMallocDefault));
  *cap = need;
  return NRV_OK;
}

// Host-pointer entry points.  raw_reads != 0: read mode with the per-event signal windows cut on the
// device from the samples already uploaded by upload_raw() (sig is ignored).
//
// Pipeline over launch groups, two staging sets, three streams; every transfer is a true DMA from / to
// PAGE-LOCKED memory, so the host thread never sits inside a copy:
//   inputs   the caller's arrays are registered in place for the call (hipHostRegister) and copied
//            straight from there; arrays too small to be worth it, or not registrable, are bounced
//            through pinned staging by a host memcpy that overlaps the previous group's kernels;
//   outputs  land in pinned staging (46 B per window) and are handed to the caller one group behind.
//   h2d:      upload(g+1) -> in(g+1)          (three input sets: enqueued before the kernels of stage g)
//   compute:  wait in(g); kernels(g) -> done(g)
//   d2h:      wait done(g); download(g) -> out(g)   (one block: p1 | p2 | a1 | a2 | range-guard counter)
//   host:     wait out(g-1); copy it to the caller; next iteration
static int predict_host(nrv_handle* h, const float* sig, const float* feat, int64_t n_in, bool read_mode,
                        float* p1, float* p2, int8_t* a1, int8_t* a2, int raw_reads = 0) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (n_in < 0 || (n_in > 0 && ((!sig && !raw_reads) || !feat))) { h->err = "nrv_predict: bad arguments"; return NRV_E_INVALID; }
  const int T = h->T;
  const int64_t n = read_mode ? n_in - T : n_in;
  if (n <= 0) return NRV_OK;
  const size_t ev_all = read_mode ? (size_t)n_in : (size_t)n_in * T;
  if (h->host_call_open) {                                 // the previous call failed somewhere in its pipeline
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int st = 0; st < 2; ++st)
      if (h->d_sat_st[st]) HIPCHK(h, hipMemcpy(&h->sat_seen[st], h->d_sat_st[st], sizeof(unsigned), hipMemcpyDeviceToHost));
  }
  h->host_call_open = true;
  // NRV_HOST_TRACE=1: where a host-pointer call's wall time goes (registration, pipeline, drain, unregistration), to stderr
  static const bool trace = getenv("NRV_HOST_TRACE") && atoi(getenv("NRV_HOST_TRACE")) > 0;
  const auto t_0 = std::chrono::steady_clock::now();
  auto since = [&](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
  HostPin pin_s, pin_f;
  const bool direct_s = !raw_reads && pin_s.pin(h, sig, ev_all * kSig * 4);
  const bool direct_f = pin_f.pin(h, feat, ev_all * kFeat * 4);
  const double ms_reg = since(t_0);
  // a pipeline stage = one upload, its launch groups (on the lanes when groups are small), one download.
  // WINDOW mode (2958 B per base over PCIe) ramps its stages: 1, 1, 2, then kWinStageMax launch groups - the first upload, which
  // nothing can hide, stays one group (12 MB, 0.22 ms), and the later stages pay the cross-stream hand-over (~10-15 us) once per
  // 2-4 groups instead of once per group (r06; NRV_WINDOW_STAGE_MAX=1: one group per stage as before).  Read modes: constant.
  static const int kWinStageMax = [] { const char* e = getenv("NRV_WINDOW_STAGE_MAX"); const int v = e ? atoi(e) : 4; return v < 1 ? 1 : (v > 8 ? 8 : v); }();
  const int stage0 = stage_windows(h, read_mode);
  const bool ramp = !read_mode && lanes_wanted(h) <= 1 && kWinStageMax > 1;
  const int max_groups = ramp ? std::min(kWinStageMax, std::max(1, h->cap_rows / stage0)) : 1;
  const int stage = stage0 * max_groups;                       // the largest stage: staging capacity
  auto stage_size = [&](int64_t k) -> int {                  // windows of stage k
    if (!ramp) return stage0;
    const int g = k < 2 ? 1 : (k == 2 ? 2 : max_groups);
    return stage0 * (g < max_groups ? g : max_groups);
  };
  const size_t ev_grp = read_mode ? (size_t)(stage + T - 1) : (size_t)stage * T;
  if (!raw_reads && !direct_s && (rc = grow_pinned(h, h->pin_sig, &h->pin_sig_cap, ev_grp * kSig * 4))) return rc;
  if (!direct_f && (rc = grow_pinned(h, h->pin_feat, &h->pin_feat_cap, ev_grp * kFeat * 4))) return rc;

  // One stage's launch groups (on the lanes when they are small): inputs from staging set si, outputs to set st, laid out
  // for the stage's own row count (block_rows): counter | p1 | p2 | a1 | a2.
  auto block_rows = [](int nb) -> size_t { return ((size_t)nb + kRowPad - 1) / kRowPad * kRowPad; };
  auto run_stage = [&](int nb, int si, int st) -> int {
    const size_t r = block_rows(nb);
    char* const d = h->d_out[st] + 64;
    const int rc0 = poison_fill(h, d, (size_t)h->cap_rows * kOutBytes, h->stream);   // NRV_POISON: the outputs, not the counter
    if (rc0) return rc0;
    return for_groups(h, nb, [&](int64_t w, int nw) {
      return run_group(h, h->d_sig[si] + (read_mode ? w * kSig : w * T * kSig),
                       h->d_feat[si] + (read_mode ? w * kFeat : w * T * kFeat), nw, read_mode,
                       (float*)d + w * 6, (float*)(d + r * 24) + w * 5, (int8_t*)(d + r * 44) + w, (int8_t*)(d + r * 45) + w,
                       h->d_sat_st[st]);
    });
  };
  auto finalize = [&](int64_t s, int nb, int si, int st) -> int {  // stage -> caller, one stage behind
    HIPCHK(h, hipEventSynchronize(h->ev_out[st]));
    char* o = h->pin_out[st] + 64;
    const size_t rows = block_rows(nb);
    if (*h->pin_sat[st] != h->sat_seen[st]) {
      // f16x2 range guard: the signal branch of this stage left the f16 range (a spike sample, a tiny MAD, a
      // NaN).  Its inputs are still in staging set si (a set is reused three stages later): run the stage
      // again on the f32 kernels, which have no range limit, and take those results.
      const int h2 = h->h2, split = h->split;
      h->h2 = 0; h->split = 0;
      int rc2 = run_stage(nb, si, st);
      h->h2 = h2; h->split = split;
      if (rc2) return rc2;
      HIPCHK(h, hipMemcpyAsync(h->pin_out[st], h->d_out[st], 64 + rows * kOutBytes, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      h->sat_seen[st] = *h->pin_sat[st];
      h->sat_reruns += 1;
    }
    if (p1) memcpy(p1 + s * 6, o, (size_t)nb * 24);
    if (p2) memcpy(p2 + s * 5, o + rows * 24, (size_t)nb * 20);
    if (a1) memcpy(a1 + s, o + rows * 44, (size_t)nb);
    if (a2) memcpy(a2 + s, o + rows * 45, (size_t)nb);
    return NRV_OK;
  };
  // Upload of the stage that starts at window s into input set si (raw-read mode: the features only; the samples went up
  // with upload_raw and the windows are cut on the device).  ONE copy per array: two halves on two copy streams were measured
  // (r05c: 3.40 vs 3.30 ms per 8-stage call) - a single stream already moves 53-57 GB/s whichever way the memory was
  // page-locked (tools/microbench/h2d_rate.hip).
  auto upload = [&](int64_t s, int si, int want) -> int {
    const int nb = (int)((n - s < want) ? (n - s) : want);
    const size_t ev = read_mode ? (size_t)(nb + T - 1) : (size_t)nb * T;
    // NRV_POISON: the whole input set, ahead of the copies (raw reads: d_sig is cut by segment_kernel after ev_in)
    int rc0;
    if ((rc0 = poison_fill(h, h->d_sig[si], h->sig_bytes, h->copy_stream)) || (rc0 = poison_fill(h, h->d_feat[si], h->feat_bytes, h->copy_stream)))
      return rc0;
    if (!raw_reads) {
      const float* hs = sig + (read_mode ? s * kSig : s * T * kSig);
      const void* src = hs;
      if (!direct_s) { memcpy(h->pin_sig[si], hs, ev * kSig * 4); src = h->pin_sig[si]; }
      HIPCHK(h, hipMemcpyAsync(h->d_sig[si], src, ev * kSig * 4, hipMemcpyHostToDevice, h->copy_stream));
    }
    const float* hf = feat + (read_mode ? s * kFeat : s * T * kFeat);
    const void* src = hf;
    if (!direct_f) { memcpy(h->pin_feat[si], hf, ev * kFeat * 4); src = h->pin_feat[si]; }
    HIPCHK(h, hipMemcpyAsync(h->d_feat[si], src, ev * kFeat * 4, hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(h, hipEventRecord(h->ev_in[si], h->copy_stream));
    return NRV_OK;
  };
  int64_t g = 0, prev_s = 0;
  int prev_nb = 0;
  // NRV_HOST_TRACE=2: timing events around every stage's kernels (span of the kernels, gap to the previous stage's)
  static const bool trace2 = getenv("NRV_HOST_TRACE") && atoi(getenv("NRV_HOST_TRACE")) > 1;
  std::vector<hipEvent_t> tev;
  if ((rc = upload(0, 0, stage_size(0)))) return rc;
  for (int64_t s = 0; s < n; s += stage_size(g), ++g) {
    const int si = (int)(g % nrv_handle::kIn), st = (int)(g & 1);
    const int cur = stage_size(g);
    const int nb = (int)((n - s < cur) ? (n - s) : cur);
    const size_t ev = read_mode ? (size_t)(nb + T - 1) : (size_t)nb * T;
    // Stage g+1's upload goes out FIRST, into the input set stage g-2 used.  Nothing has to be waited for: the previous
    // iteration ended with finalize(g-2) - a HOST wait for that stage's download (ev_out), which ran behind its kernels
    // (ev_done), which ran behind its upload (ev_in) - so that set's bounce buffers and d_sig / d_feat are free, and so are
    // the output set d_p / d_a of stage g-2 that this stage's kernels write.  (Until r05 three waits stood here, one of them
    // a barrier packet on the compute stream per stage.)
    if (s + cur < n && (rc = upload(s + cur, (int)((g + 1) % nrv_handle::kIn), stage_size(g + 1)))) return rc;
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_in[si], 0));
    if (trace2 && tev.size() < 128) { hipEvent_t e; HIPCHK(h, hipEventCreate(&e)); HIPCHK(h, hipEventRecord(e, h->stream)); tev.push_back(e); }
    if (raw_reads) launch_segment(h, raw_reads, s, (int)ev, h->d_sig[si]);
    if ((rc = run_stage(nb, si, st))) return rc;
    if (trace2 && tev.size() < 128) { hipEvent_t e; HIPCHK(h, hipEventCreate(&e)); HIPCHK(h, hipEventRecord(e, h->stream)); tev.push_back(e); }
    HIPCHK(h, hipEventRecord(h->ev_done[st], h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->d2h_stream, h->ev_done[st], 0));
    HIPCHK(h, hipMemcpyAsync(h->pin_out[st], h->d_out[st], 64 + block_rows(nb) * kOutBytes, hipMemcpyDeviceToHost, h->d2h_stream));
    HIPCHK(h, hipEventRecord(h->ev_out[st], h->d2h_stream));
    if (g >= 1 && (rc = finalize(prev_s, prev_nb, (int)((g - 1) % nrv_handle::kIn), st ^ 1))) return rc;
    prev_s = s;
    prev_nb = nb;
  }
  if ((rc = finalize(prev_s, prev_nb, (int)((g - 1) % nrv_handle::kIn), (int)((g - 1) & 1)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->copy_stream));
  HIPCHK(h, hipStreamSynchronize(h->d2h_stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  pin_s.settled = pin_f.settled = true;
  if (trace2 && tev.size() >= 2) {
    double span = 0, gap = 0; float ms = 0;
    for (size_t i = 0; i + 1 < tev.size(); i += 2) { (void)hipEventElapsedTime(&ms, tev[i], tev[i + 1]); span += ms; }
    for (size_t i = 1; i + 1 < tev.size(); i += 2) { (void)hipEventElapsedTime(&ms, tev[i], tev[i + 1]); gap += ms; }
    (void)hipEventElapsedTime(&ms, tev.front(), tev.back());
    fprintf(stderr, "[nrv host trace] %zu stages: kernels %.4f ms per stage, gap between stages %.4f ms, first kernel to last %.3f ms\n",
            tev.size() / 2, span / (tev.size() / 2), tev.size() > 2 ? gap / (tev.size() / 2 - 1) : 0.0, ms);
    for (hipEvent_t e : tev) (void)hipEventDestroy(e);
  }
  if (trace) {
    const double ms_run = since(t_0) - ms_reg;
    const auto t_u = std::chrono::steady_clock::now();
    pin_s.release(); pin_f.release();
    fprintf(stderr, "[nrv host trace] %lld windows, %d stages: register %.3f ms (sig %d, feat %d), pipeline %.3f ms, unregister %.3f ms\n",
            (long long)n, (int)g, ms_reg, (int)direct_s, (int)direct_f, ms_run, since(t_u));
  }
  h->host_call_open = false;
  return NRV_OK;
}

int nrv_predict(nrv_handle* h, const float* signal, const float* read, int64_t n, float* p1, float* p2,
                int8_t* a1, int8_t* a2) {
  return predict_host(h, signal, read, n, false, p1, p2, a1, a2);
}

int nrv_predict_read(nrv_handle* h, const float* sig_ev, const float* feat_ev, int64_t N, float* p1,
                     float* p2, int8_t* a1, int8_t* a2) {
  return predict_host(h, sig_ev, feat_ev, N, true, p1, p2, a1, a2);
}

// ---- whole-call raw reads (r06) ----------------------------------------------------------------------------------------
static int raw_check(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts, const float* feat, int64_t N,
                     const nrv_read_desc* reads, int n_reads) {
  if (n_raw < 0 || N < 0 || n_reads < 0 || (n_raw > 0 && !raw) || (N > 0 && (!starts || !reads || !feat || n_reads == 0))) {
    h->err = "nrv raw reads: bad arguments";
    return NRV_E_INVALID;
  }
  int64_t ev = 0;
  for (int r = 0; r < n_reads; ++r) {          // descriptors must tile [0, N) in order and stay inside raw
    const nrv_read_desc& d = reads[r];
    if (d.ev_off != ev || d.ev_len < 0 || d.raw_off < 0 || d.raw_len < 0 || d.raw_off + d.raw_len > n_raw) {
      h->err = "nrv raw reads: read descriptors do not tile the event range / exceed the sample array";
      return NRV_E_INVALID;
    }
    ev += d.ev_len;
  }
  if (ev != N) { h->err = "nrv raw reads: read descriptors do not cover N events"; return NRV_E_INVALID; }
  return NRV_OK;
}

// every stage of a slot's call onto the compute stream: segmentation of the stage's events, then its launch groups
static int raw_enqueue(nrv_handle* h, nrv_handle::RawSlot& sl) {
  const int T = h->T;
  const int stage = stage_windows(h, true);
  char* const d = sl.d_out + 64;
  const float* d_feat = (const float*)(sl.d_in + sl.off_feat);
  for (int64_t s = 0; s < sl.n; s += stage) {
    const int nb = (int)((sl.n - s < stage) ? (sl.n - s) : stage);
    const int rc0 = poison_fill(h, h->d_sig[0], h->sig_bytes, h->stream);
    if (rc0) return rc0;
    launch_segment(h, sl.n_reads, s, nb + T - 1, h->d_sig[0], (const int16_t*)sl.d_in, (const int32_t*)(sl.d_in + sl.off_starts),
                   (const SegRead*)(sl.d_in + sl.off_reads));
    const int rc = for_groups(h, nb, [&](int64_t w, int nw) {
      return run_group(h, h->d_sig[0] + w * kSig, d_feat + (s + w) * kFeat, nw, true,
                       (float*)d + (s + w) * 6, (float*)(d + sl.rows * 24) + (s + w) * 5, (int8_t*)(d + sl.rows * 44) + (s + w),
                       (int8_t*)(d + sl.rows * 45) + (s + w), (unsigned*)sl.d_out);
    });
    if (rc) return rc;
  }
  return NRV_OK;
}

// Read statistics on the device (nrv_stats.h) for the reads whose aux says so: shift / scale into d_reads, feature columns
// 1 and 2 into d_feat (or mean / std / both).  The scratch is zeroed HERE, on the compute stream; max_len = the longest such read.
static int stats_enqueue(nrv_handle* h, const int16_t* d_raw, const int32_t* d_starts, SegRead* d_reads, const StatAux* d_aux,
                         unsigned* d_scratch, int n_reads, int64_t N, int64_t max_len, float* d_feat, double* d_mean, double* d_std) {
  if (n_reads <= 0 || max_len <= 0) return NRV_OK;
  HIPCHK(h, hipMemsetAsync(d_scratch, 0, (size_t)n_reads * kStatWords * 4, h->stream));
  const StatArgs a{(const short*)d_raw, d_reads, d_aux, d_scratch, n_reads};
  const dim3 grid((unsigned)((max_len + kStatChunk - 1) / kStatChunk), (unsigned)n_reads);
  hipLaunchKernelGGL(stats_minmax_kernel, grid, dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(stats_hist_kernel<0>, grid, dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(stats_scan_kernel<0>, dim3((unsigned)n_reads), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(stats_hist_kernel<1>, grid, dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(stats_scan_kernel<1>, dim3((unsigned)n_reads), dim3(256), 0, h->stream, a);
  if (N > 0) {
    const EvStatArgs e{(const short*)d_raw, (const int*)d_starts, d_reads, d_aux, n_reads, (long long)N, d_feat, d_mean, d_std};
    hipLaunchKernelGGL(event_stats_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, e);
  }
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}
// the reads of a call that take their statistics from the device: each needs 1 .. 2^32 - 1 samples (32-bit counters; the host's
// median_mad_i16 declines the same).  Returns the longest of them (0: none) or -1.
static int64_t stats_check(nrv_handle* h, const nrv_read_desc* reads, int n_reads, const int32_t* last_dur, const uint8_t* on_device) {
  if (n_reads > 0 && (!last_dur || !on_device)) { h->err = "nrv read statistics: null last_dur / flags"; return -1; }
  int64_t max_len = 0;
  for (int r = 0; r < n_reads; ++r) {
    if (!on_device[r]) continue;
    if (reads[r].raw_len < 1 || reads[r].raw_len >= ((int64_t)1 << 32)) { h->err = "nrv read statistics: a read without samples (or with 2^32 or more)"; return -1; }
    max_len = reads[r].raw_len > max_len ? reads[r].raw_len : max_len;
  }
  return max_len;
}

// The merge kernels (nrv_merge.h) behind whatever produced a.a1 / a2 / p1 / p2 on the compute stream: N >= 1 events
static int merge_enqueue(nrv_handle* h, const MergeArgs& a) {
  const unsigned tiles = (unsigned)((a.N + kMergeTile - 1) / kMergeTile);
  hipLaunchKernelGGL(merge_emit_kernel, dim3(tiles), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(merge_tile_scan_kernel, dim3(1), dim3(256), 0, h->stream, a, (int)tiles);
  hipLaunchKernelGGL(merge_scatter_kernel, dim3(tiles), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}
// The report kernel (nrv_report.h) behind merge_enqueue on the same stream: it reads the records the merge left in a.rec.  The
// block is zeroed here, in stream order ahead of the launch - every call of this function starts its counts from nothing.
static int report_enqueue(nrv_handle* h, const ReportArgs& a) {
  if (a.n_reads <= 0 || a.N <= 0) return NRV_OK;
  HIPCHK(h, hipMemsetAsync(a.report, 0, (size_t)a.n_reads * kReportCols * 8, h->stream));
  const unsigned tiles = (unsigned)((a.N + kMergeTile - 1) / kMergeTile);
  hipLaunchKernelGGL(report_kernel, dim3(tiles), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}
static ReportArgs report_args(const MergeArgs& m, const float* p1, const float* p2, bool want_q, float tie_eps, void* report) {
  ReportArgs a;
  a.reads = m.reads; a.n_reads = m.n_reads; a.T = m.T; a.N = m.N;
  a.bases = m.bases; a.a1 = m.a1; a.a2 = m.a2;
  a.p1 = p1 && p2 ? p1 : nullptr; a.p2 = p1 && p2 ? p2 : nullptr;
  a.rec = m.rec; a.want_q = want_q ? 1 : 0; a.tie_eps = tie_eps;
  a.report = (unsigned long long*)report;
  return a;
}
// The score kernel (nrv_score.h) behind merge_enqueue (and report_enqueue) on the same stream: it reads what the merge read and
// the label bytes, nothing the merge left.  The block is zeroed here, in stream order ahead of the launch, as the report's is.
static int score_enqueue(nrv_handle* h, const ScoreArgs& a) {
  if (a.n_reads <= 0 || a.N <= 0) return NRV_OK;
  HIPCHK(h, hipMemsetAsync(a.score, 0, (size_t)a.n_reads * kScoreCols * 8, h->stream));
  const unsigned tiles = (unsigned)((a.N + kMergeTile - 1) / kMergeTile);
  hipLaunchKernelGGL(score_kernel, dim3(tiles), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}
static ScoreArgs score_args(const MergeArgs& m, const float* p1, const float* p2, const unsigned char* labels, const float* thr, void* score) {
  ScoreArgs a;
  a.reads = m.reads; a.n_reads = m.n_reads; a.T = m.T; a.N = m.N;
  a.bases = m.bases; a.labels = labels; a.a1 = m.a1; a.a2 = m.a2;
  a.p1 = p1 && p2 ? p1 : nullptr; a.p2 = p1 && p2 ? p2 : nullptr;
  a.score = (unsigned long long*)score;
  memcpy(a.thr, thr, sizeof a.thr);
  return a;
}
// The edit kernels (nrv_edits.h) behind merge_enqueue (and report_enqueue) on the same stream: they read the records, the tile
// offsets and the read offsets the merge left.  Plain stores into every word that is read back: a second pass accumulates nothing.
static int edits_enqueue(nrv_handle* h, const EditsArgs& a) {
  if (a.n_reads <= 0 || a.N <= 0) return NRV_OK;
  const unsigned tiles = (unsigned)((a.N + kMergeTile - 1) / kMergeTile);
  hipLaunchKernelGGL(edits_count_kernel, dim3(tiles), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(edits_tile_scan_kernel, dim3(1), dim3(256), 0, h->stream, a, (int)tiles);
  hipLaunchKernelGGL(edits_scatter_kernel, dim3(tiles), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}
static EditsArgs edits_args(const MergeArgs& m, const float* p1, const float* p2, bool want_q, void* etile, void* edit_off, void* edits) {
  static_assert(sizeof(EditRec) == sizeof(nrv_edit), "nanorev.h and nrv_edits.h disagree on the edit record");
  EditsArgs a;
  a.reads = m.reads; a.n_reads = m.n_reads; a.T = m.T; a.N = m.N;
  a.cap = m.N - m.T > 0 ? m.N - m.T : 0;
  a.bases = m.bases; a.a1 = m.a1; a.a2 = m.a2;
  a.p1 = p1 && p2 ? p1 : nullptr; a.p2 = p1 && p2 ? p2 : nullptr;
  a.rec = m.rec; a.tile = m.tile; a.off = m.off; a.want_q = want_q ? 1 : 0;
  a.etile = (unsigned long long*)etile; a.edit_off = (long long*)edit_off; a.edits = (EditRec*)edits;
  return a;
}
// The record kernels (nrv_pack.h) behind merge_enqueue (and report_enqueue / edits_enqueue) on the same stream: they read seq /
// qual / off as the merge left them.  Plain stores, each byte by one thread: a second pass accumulates nothing.
static int pack_enqueue(nrv_handle* h, const PackArgs& a) {
  if (a.n_reads <= 0) {
    HIPCHK(h, hipMemsetAsync(a.rec_off, 0, 8, h->stream));
    return NRV_OK;
  }
  hipLaunchKernelGGL(pack_offsets_kernel, dim3(1), dim3(256), 0, h->stream, a);
  const unsigned long long words = (a.cap + 3) / 4;
  if (words > 0) hipLaunchKernelGGL(pack_copy_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}
// The profile kernel (nrv_profile.h) behind merge_enqueue (and the report / edit / record launches) on the same stream: it reads
// the records the merge left in rec.  The block is zeroed here, in stream order ahead of the launch, as the report's is.
static int profile_enqueue(nrv_handle* h, const ProfileArgs& a) {
  if (a.n_reads <= 0 || a.N <= 0) return NRV_OK;
  HIPCHK(h, hipMemsetAsync(a.profile, 0, (size_t)a.n_reads * kProfileCols * 8, h->stream));
  const unsigned tiles = (unsigned)((a.N + kMergeTile - 1) / kMergeTile);
  hipLaunchKernelGGL(profile_kernel, dim3(tiles), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}
static ProfileArgs profile_args(const MergeArgs& m, const float* p1, const float* p2, const float* thr, void* profile) {
  ProfileArgs a;
  a.reads = m.reads; a.n_reads = m.n_reads; a.T = m.T; a.N = m.N;
  a.a1 = m.a1; a.a2 = m.a2; a.p1 = p1; a.p2 = p2;
  a.rec = m.rec;
  a.profile = (unsigned long long*)profile;
  memcpy(a.thr, thr, sizeof a.thr);
  return a;
}
// The window and finish kernels (nrv_trim.h) on the qualities a.q: the accumulators start from 0xFF bytes HERE, in stream order
// ahead of the launch (and behind any NRV_POISON fill) - every call of this function starts its bounds from nothing.
static int trim_bounds_enqueue(nrv_handle* h, const TrimArgs& a) {
  if (a.n_reads <= 0) return NRV_OK;
  HIPCHK(h, hipMemsetAsync(a.acc, 0xFF, (size_t)a.n_reads * 16, h->stream));
  const unsigned tiles = (unsigned)((a.cap + 255) / 256);
  if (tiles > 0) hipLaunchKernelGGL(trim_window_kernel, dim3(tiles), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL(trim_finish_kernel, dim3((unsigned)((a.n_reads + 255) / 256)), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}
// The trim kernels behind merge_enqueue (and the report / edit launches), AHEAD of pack_enqueue, which reads `trim`: they read the
// records, the tile offsets and the read offsets the merge left, and the rows
static int trim_enqueue(nrv_handle* h, const MergeArgs& m, const float* p1, const float* p2, const TrimRule& t, void* tq, void* acc,
                        void* trim) {
  if (m.n_reads <= 0 || m.N <= 0) return NRV_OK;
  TrimQualArgs q;
  q.reads = m.reads; q.n_reads = m.n_reads; q.T = m.T; q.N = m.N;
  q.a1 = m.a1; q.a2 = m.a2; q.p1 = p1; q.p2 = p2;
  q.rec = m.rec; q.tile = m.tile; q.tq = (unsigned char*)tq;
  q.cap = m.N + (m.N - m.T > 0 ? m.N - m.T : 0);
  memcpy(q.thr, t.thr, sizeof q.thr);
  const unsigned tiles = (unsigned)((m.N + kMergeTile - 1) / kMergeTile);
  hipLaunchKernelGGL(trim_qual_kernel, dim3(tiles), dim3(256), 0, h->stream, q);
  TrimArgs a;
  a.n_reads = m.n_reads; a.Q = t.Q; a.W = t.W; a.bias = 0;
  a.off = m.off; a.q = (const unsigned char*)tq; a.cap = q.cap;
  a.acc = (unsigned long long*)acc; a.trim = (long long*)trim;
  return trim_bounds_enqueue(h, a);
}
// align_kernel (nrv_align.h): one wave per (read, kind) pair; every word of its result is stored plainly
static int align_enqueue(nrv_handle* h, const AlignArgs& a) {
  if (a.n_reads <= 0) return NRV_OK;
  hipLaunchKernelGGL(align_kernel, dim3((unsigned)a.n_reads * (unsigned)a.kinds), dim3(64), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}
// errclass_kernel (nrv_errclass.h): one wave per (read, kind) pair; every word of its result is stored plainly
static int errclass_enqueue(nrv_handle* h, const ErrclassArgs& a) {
  if (a.n_reads <= 0) return NRV_OK;
  hipLaunchKernelGGL(errclass_kernel, dim3((unsigned)a.n_reads * (unsigned)a.kinds), dim3(64), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}
// infix_kernel (nrv_infix.h): one wave per (read, kind, strand) triple; every word of its result is stored plainly
static int infix_enqueue(nrv_handle* h, const InfixArgs& a) {
  if (a.n_reads <= 0) return NRV_OK;
  hipLaunchKernelGGL(infix_kernel, dim3((unsigned)a.n_reads * (unsigned)(a.kinds * a.strands)), dim3(64), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}
static bool trim_rule_ok(int Q, int W, int64_t min_len) { return Q >= 1 && Q <= 40 && W >= 1 && W <= kTrimMaxW && min_len >= 0; }
// bytes the records of a call can take: hoststage.pack_records on N + max(N - T, 0) characters at the most
static size_t blob_capacity(int64_t N, int64_t n, int n_reads, int64_t name_bytes, bool fastq) {
  const size_t q = fastq ? 2 : 1;
  return (size_t)name_bytes + q * (size_t)(N + n) + 3 * q * (size_t)n_reads;
}
// names / name_off of a records call: offsets from 0, ascending
static bool names_ok(const uint8_t* names, const int64_t* name_off, int n_reads) {
  if (!name_off || name_off[0] != 0) return false;
  for (int r = 0; r < n_reads; ++r) if (name_off[r + 1] < name_off[r]) return false;
  return names != nullptr || name_off[n_reads] == 0;
}
// hoststage.pack_records on the host, for the calls that have no window (N <= T): qual == nullptr with fastq: every quality is '#'
// trim / min_len: as nrv_pack_records_trim (null: the whole reads)
static void records_host(const uint8_t* seq, const uint8_t* qual, const int64_t* off, int n_reads, const uint8_t* names,
                         const int64_t* name_off, bool fastq, uint8_t* blob, int64_t* rec_off, const int64_t* trim = nullptr,
                         int64_t min_len = 0) {
  int64_t p = 0;
  for (int r = 0; r < n_reads; ++r) {
    const int64_t nl = name_off[r + 1] - name_off[r];
    const int64_t s0 = off[r] + (trim ? trim[2 * r] : 0), L = trim ? trim[2 * r + 1] - trim[2 * r] : off[r + 1] - off[r];
    rec_off[r] = p;
    if (trim && L < min_len) continue;
    blob[p++] = fastq ? '@' : '>';
    if (nl > 0) memcpy(blob + p, names + name_off[r], (size_t)nl);
    p += nl;
    blob[p++] = '\n';
    if (L > 0) memcpy(blob + p, seq + s0, (size_t)L);
    p += L;
    blob[p++] = '\n';
    if (fastq) {
      blob[p++] = '+';
      blob[p++] = '\n';
      if (L > 0) { if (qual) memcpy(blob + p, qual + s0, (size_t)L); else memset(blob + p, '#', (size_t)L); }
      p += L;
      blob[p++] = '\n';
    }
  }
  rec_off[n_reads] = p;
}
// the merged block (MergeLayout) of a call that hands back what `o` asks for
static MergeLayout merge_layout(int64_t N, int64_t n, int n_reads, const MergeOut& o, size_t blob_cap) {
  MergeLayout m;
  const size_t cap = (size_t)(N + n), tiles = (size_t)((N + kMergeTile - 1) / kMergeTile);
  m.seq = up256(((size_t)n_reads + 1) * 8);
  m.qual = m.seq + up256(cap);
  m.rep = m.qual + up256(cap);
  m.eoff = m.rep + (o.report ? up256((size_t)n_reads * kReportCols * 8) : 0);
  m.roff = m.eoff + (o.edit_off ? up256(((size_t)n_reads + 1) * 8) : 0);
  m.prof = m.roff + (o.rec_off ? up256(((size_t)n_reads + 1) * 8) : 0);
  m.trim = m.prof + (o.profile ? up256((size_t)n_reads * kProfileCols * 8) : 0);
  m.accu = m.trim + (o.trim ? up256((size_t)n_reads * 16) : 0);
  m.ecls = m.accu + (o.accuracy ? up256((size_t)n_reads * kAccuracyCols * 8) : 0);
  m.infx = m.ecls + (o.errclass ? up256((size_t)n_reads * kErrclassCols * 8) : 0);
  m.scor = m.infx + (o.infix ? up256((size_t)n_reads * kInfixCols * 8) : 0);
  m.dl = m.scor + (o.score ? up256((size_t)n_reads * kScoreCols * 8) : 0);
  m.rec = m.dl;
  m.tile = m.rec + up256((size_t)N * 4);
  m.edits = m.tile + up256(tiles * 8);
  m.etile = m.edits + (o.edit_off ? up256((size_t)n * sizeof(nrv_edit)) : 0);
  m.blob = m.etile + (o.edit_off ? up256(tiles * 8) : 0);
  m.tq = m.blob + (o.rec_off ? up256(blob_cap) : 0);
  m.acc = m.tq + (o.trim ? up256(cap) : 0);
  m.hc = m.acc + (o.trim ? up256((size_t)n_reads * 16) : 0);
  m.hc8 = m.hc + (o.accuracy ? carry_layout((size_t)N, cap, 1, 1).bytes : 0);
  m.hci = m.hc8 + (o.errclass ? carry_layout((size_t)N, cap, 8, 1).bytes : 0);
  m.bytes = m.hci + (o.infix ? carry_layout((size_t)N, cap, 8, 2).bytes : 0);
  return m;
}
// No window at all (N <= T): the reads come back as they are, on the host
static void merge_nothing(const uint8_t* bases, const nrv_read_desc* reads, int n_reads, int64_t N, uint8_t* seq, uint8_t* qual, int64_t* off) {
  if (seq && N > 0) memcpy(seq, bases, (size_t)N);
  if (qual && N > 0) memset(qual, '#', (size_t)N);
  for (int r = 0; r < n_reads; ++r) off[r] = reads[r].ev_off;
  off[n_reads] = N;
}
// ... and its report (hoststage.revision_report on a call without a window): edge = bases_in = bases_out = ev_len; with a
// quality every character is '#', which is 2 above the Phred offset
static void report_nothing(const nrv_read_desc* reads, int n_reads, bool want_q, uint64_t* report) {
  static_assert(NRV_REPORT_COLS == kReportCols, "nanorev.h and nrv_report.h disagree on the report's columns");
  memset(report, 0, (size_t)n_reads * kReportCols * 8);
  for (int r = 0; r < n_reads; ++r) {
    uint64_t* row = report + (size_t)r * kReportCols;
    row[kRcBasesIn] = row[kRcBasesOut] = row[kRcEdge] = (uint64_t)reads[r].ev_len;
    if (want_q) row[kRcQSum] = 2 * (uint64_t)reads[r].ev_len;
  }
}
// ... and its profile (hoststage.read_profile on a call without a window): every character is an original base with '#', Phred 2
static void profile_nothing(const uint8_t* bases, const nrv_read_desc* reads, int n_reads, uint64_t* profile) {
  static_assert(NRV_PROFILE_COLS == kProfileCols, "nanorev.h and nrv_profile.h disagree on the profile's columns");
  memset(profile, 0, (size_t)n_reads * kProfileCols * 8);
  for (int r = 0; r < n_reads; ++r) {
    uint64_t* row = profile + (size_t)r * kProfileCols;
    row[2] = (uint64_t)reads[r].ev_len;
    for (int64_t e = reads[r].ev_off; e < reads[r].ev_off + reads[r].ev_len; ++e) {
      const uint8_t c = bases[e];
      row[kPfBase + (c == 'A' ? 0 : (c == 'C' ? 1 : (c == 'G' ? 2 : (c == 'T' ? 3 : 4))))] += 1;
    }
  }
}
// ... and its trim (hoststage.trim_bounds on a call without a window): every character has Phred 2, so every position with a
// whole window in the read is good or none is
static void trim_nothing(const nrv_read_desc* reads, int n_reads, int Q, int W, int64_t* trim) {
  for (int r = 0; r < n_reads; ++r) {
    const bool any = reads[r].ev_len >= W && 2 * W >= Q * W;
    trim[2 * r] = 0;
    trim[2 * r + 1] = any ? reads[r].ev_len : 0;
  }
}
// hoststage.edit_distance by two rows of the table, on the host: the calls without a window and nothing else
static int64_t edit_distance_host(const uint8_t* t, int64_t m, const uint8_t* s, int64_t n) {
  std::vector<int64_t> row((size_t)n + 1);
  for (int64_t j = 0; j <= n; ++j) row[(size_t)j] = j;
  for (int64_t i = 1; i <= m; ++i) {
    int64_t diag = row[0];
    row[0] = i;
    const uint8_t c = t[i - 1];
    const bool base = c == 'A' || c == 'C' || c == 'G' || c == 'T';
    for (int64_t j = 1; j <= n; ++j) {
      const int64_t up_ = row[(size_t)j] + 1, left = row[(size_t)j - 1] + 1, dg = diag + ((base && c == s[j - 1]) ? 0 : 1);
      diag = row[(size_t)j];
      row[(size_t)j] = std::min(std::min(up_, left), dg);
    }
  }
  return row[(size_t)n];
}
// ... and its accuracy (hoststage.read_accuracy on a call without a window): the reads come back as they are, dist_out = dist_in
static void accuracy_nothing(const uint8_t* bases, const nrv_read_desc* reads, int n_reads, const uint8_t* truth, const int64_t* truth_off,
                             uint64_t* accuracy) {
  static_assert(NRV_ACCURACY_COLS == kAccuracyCols, "nanorev.h and nrv_align.h disagree on the accuracy's columns");
  memset(accuracy, 0, (size_t)n_reads * kAccuracyCols * 8);
  for (int r = 0; r < n_reads; ++r) {
    const int64_t m = truth_off[r + 1] - truth_off[r];
    if (m <= 0) continue;
    uint64_t* row = accuracy + (size_t)r * kAccuracyCols;
    row[0] = (uint64_t)m;
    row[1] = row[2] = (uint64_t)edit_distance_host(truth + truth_off[r], m, bases + reads[r].ev_off, reads[r].ev_len);
  }
}
// hoststage.edit_classes by two rows of the table of packed cells (d << 32) - M, on the host: the calls without a window, as above
static void edit_classes_host(const uint8_t* t, int64_t m, const uint8_t* s, int64_t n, uint64_t* d_out, uint64_t* M_out) {
  std::vector<int64_t> row((size_t)n + 1);
  for (int64_t j = 0; j <= n; ++j) row[(size_t)j] = j * kEdit;
  for (int64_t i = 1; i <= m; ++i) {
    int64_t diag = row[0];
    row[0] = i * kEdit;
    const uint8_t c = t[i - 1];
    const bool base = c == 'A' || c == 'C' || c == 'G' || c == 'T';
    for (int64_t j = 1; j <= n; ++j) {
      const int64_t up_ = row[(size_t)j] + kEdit, left = row[(size_t)j - 1] + kEdit, dg = diag + ((base && c == s[j - 1]) ? -1 : kEdit);
      diag = row[(size_t)j];
      row[(size_t)j] = std::min(std::min(up_, left), dg);
    }
  }
  const int64_t w = row[(size_t)n], d = (w + kEdit - 1) >> 32;
  *d_out = (uint64_t)d; *M_out = (uint64_t)(d * kEdit - w);
}
// ... and its error classes (hoststage.read_error_classes on a call without a window): out = in
static void errclass_nothing(const uint8_t* bases, const nrv_read_desc* reads, int n_reads, const uint8_t* truth, const int64_t* truth_off,
                             uint64_t* errclass) {
  static_assert(NRV_ERRCLASS_COLS == kErrclassCols, "nanorev.h and nrv_errclass.h disagree on the error classes' columns");
  memset(errclass, 0, (size_t)n_reads * kErrclassCols * 8);
  for (int r = 0; r < n_reads; ++r) {
    const int64_t m = truth_off[r + 1] - truth_off[r];
    if (m <= 0) continue;
    uint64_t* row = errclass + (size_t)r * kErrclassCols;
    row[0] = (uint64_t)m;
    edit_classes_host(truth + truth_off[r], m, bases + reads[r].ev_off, reads[r].ev_len, row + 1, row + 2);
    row[3] = row[1]; row[4] = row[2];
  }
}
// hoststage.infix_classes by two rows of the table of packed cells d 2^42 - M 2^21 - start, on the host: the calls without a window
static void infix_classes_host(const uint8_t* t, int64_t m, const uint8_t* s, int64_t n, bool rev, uint64_t* out4) {
  std::vector<int64_t> row((size_t)n + 1);
  for (int64_t j = 0; j <= n; ++j) row[(size_t)j] = j * kInfixEdit;
  int64_t best = row[(size_t)n], best_i = 0;
  for (int64_t i = 1; i <= m; ++i) {
    int64_t diag = row[0];
    row[0] = -i;
    uint8_t c = t[rev ? m - i : i - 1];
    if (rev) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 0;
    const bool base = c == 'A' || c == 'C' || c == 'G' || c == 'T';
    for (int64_t j = 1; j <= n; ++j) {
      const int64_t up_ = row[(size_t)j] + kInfixEdit, left = row[(size_t)j - 1] + kInfixEdit;
      const int64_t dg = diag + ((base && c == s[j - 1]) ? -kInfixMatch : kInfixEdit);
      diag = row[(size_t)j];
      row[(size_t)j] = std::min(std::min(up_, left), dg);
    }
    if (row[(size_t)n] < best) { best = row[(size_t)n]; best_i = i; }
  }
  const int64_t d = (best + kInfixEdit - 1) >> 42, rest = d * kInfixEdit - best;
  out4[0] = (uint64_t)d; out4[1] = (uint64_t)(rest >> 21); out4[2] = (uint64_t)(rest & kInfixMaxLen); out4[3] = (uint64_t)best_i;
}
// ... and its infix block (hoststage.read_infix on a call without a window): out = in
static void infix_nothing(const uint8_t* bases, const nrv_read_desc* reads, int n_reads, const uint8_t* truth, const int64_t* truth_off,
                          int strands, uint64_t* infix) {
  static_assert(NRV_INFIX_COLS == kInfixCols && NRV_INFIX_MAX_LEN == kInfixMaxLen, "nanorev.h and nrv_infix.h disagree on the infix block");
  memset(infix, 0, (size_t)n_reads * kInfixCols * 8);
  for (int r = 0; r < n_reads; ++r) {
    const int64_t m = truth_off[r + 1] - truth_off[r];
    if (m <= 0) continue;
    uint64_t* row = infix + (size_t)r * kInfixCols;
    row[0] = (uint64_t)m; row[1] = (uint64_t)strands;
    for (int rev = 0; rev < strands; ++rev) {
      infix_classes_host(truth + truth_off[r], m, bases + reads[r].ev_off, reads[r].ev_len, rev != 0, row + 2 + 4 * rev);
      memcpy(row + 10 + 4 * rev, row + 2 + 4 * rev, 32);
    }
  }
}
// ... and everything a merged call asks for, for both callers that can meet N <= T
static void merged_nothing(const MergeIn& in, const MergeOut& o, const nrv_read_desc* reads, int n_reads, int64_t N) {
  merge_nothing(in.bases, reads, n_reads, N, o.seq, in.q_thr ? o.qual : nullptr, o.off);
  if (o.report) report_nothing(reads, n_reads, wants_quality(in.q_thr, o), o.report);
  if (o.edit_off) memset(o.edit_off, 0, ((size_t)n_reads + 1) * 8);   // no window, no record
  if (o.trim) trim_nothing(reads, n_reads, in.Q, in.W, o.trim);
  if (o.rec_off) records_host(in.bases, nullptr, o.off, n_reads, in.names, in.name_off, in.q_thr != nullptr, o.blob, o.rec_off,
                              o.trim, in.min_len);
  if (o.profile) profile_nothing(in.bases, reads, n_reads, o.profile);
  if (o.accuracy) accuracy_nothing(in.bases, reads, n_reads, in.truth, in.truth_off, o.accuracy);
  if (o.errclass) errclass_nothing(in.bases, reads, n_reads, in.truth, in.truth_off, o.errclass);
  if (o.infix) infix_nothing(in.bases, reads, n_reads, in.truth, in.truth_off, o.strands, o.infix);
  static_assert(NRV_SCORE_COLS == kScoreCols, "nanorev.h and nrv_score.h disagree on the score's columns");
  if (o.score) memset(o.score, 0, (size_t)n_reads * kScoreCols * 8);   // hoststage.score_calls on a call without a window: nothing to score
}

// What the three truth kernels share (PairArgs, nrv_align.h) in a merged call: both kinds of every read, the revised text as
// the merge (a) leaves it
static PairArgs pair_args(const MergeView& v, const MergeArgs& a, int T) {
  PairArgs k;
  k.n_reads = v.n_reads; k.kinds = 2;
  k.truth = v.truth; k.truth_off = v.truth_off;
  k.reads = v.reads; k.bases = v.bases; k.off = a.off; k.seq = a.seq;
  k.cap0 = v.N; k.cap1 = v.N + (v.N - T > 0 ? v.N - T : 0);
  return k;
}
// The kernels of a merged call behind whatever produced v.a1 / a2 / p1 / p2 on the compute stream: the merge, then what `o` asks
// for - report, edit list, records, profile - each reading what the merge left.  q_thr: the thresholds of the quality (null:
// none is written); the merge reads the rows only for a quality, the report and the edits whenever there are rows, the profile
// always, and so does the trim (t: its rule), whose bounds the records are then cut to.  A second pass over the same block (the
// re-run of nrv_reads_raw_end) counts nothing twice: report_enqueue and profile_enqueue zero their blocks and trim_bounds_enqueue
// resets its accumulators in stream order, the edit and record kernels store plainly into every word that is read back; the
// score (score_thr: its own thresholds) is zeroed by score_enqueue like the report
static int merged_enqueue(nrv_handle* h, const MergeView& v, const MergeLayout& m, const MergeOut& o, const float* q_thr,
                          const float* prof_thr, size_t blob_cap, const TrimRule& t = TrimRule{}, const float* score_thr = nullptr) {
  const bool want_q = q_thr != nullptr;
  MergeArgs a;
  a.reads = v.reads; a.n_reads = v.n_reads; a.T = h->T; a.N = v.N;
  a.bases = v.bases; a.a1 = v.a1; a.a2 = v.a2;
  a.p1 = want_q ? v.p1 : nullptr; a.p2 = want_q ? v.p2 : nullptr;
  a.rec = (unsigned*)(v.blk + m.rec); a.tile = (unsigned long long*)(v.blk + m.tile);
  a.off = (long long*)v.blk; a.seq = (unsigned char*)(v.blk + m.seq);
  a.qual = want_q ? (unsigned char*)(v.blk + m.qual) : nullptr;
  memset(a.thr, 0, sizeof a.thr);
  if (want_q) memcpy(a.thr, q_thr, sizeof a.thr);
  int rc = merge_enqueue(h, a);
  if (!rc && o.report) rc = report_enqueue(h, report_args(a, v.p1, v.p2, want_q, o.tie_eps, v.blk + m.rep));
  if (!rc && o.score) rc = score_enqueue(h, score_args(a, v.p1, v.p2, v.labels, score_thr, v.blk + m.scor));
  if (!rc && o.edit_off) rc = edits_enqueue(h, edits_args(a, v.p1, v.p2, want_q, v.blk + m.etile, v.blk + m.eoff, v.blk + m.edits));
  if (!rc && o.trim) rc = trim_enqueue(h, a, v.p1, v.p2, t, v.blk + m.tq, v.blk + m.acc, v.blk + m.trim);
  if (!rc && o.rec_off) {
    PackArgs k;
    k.n_reads = v.n_reads; k.fastq = want_q ? 1 : 0;
    k.off = a.off; k.name_off = v.name_off; k.names = v.names;
    k.seq = a.seq; k.qual = (const unsigned char*)(v.blk + m.qual);
    k.rec_off = (long long*)(v.blk + m.roff); k.blob = (unsigned char*)(v.blk + m.blob);
    k.cap = blob_cap;
    k.trim = o.trim ? (const long long*)(v.blk + m.trim) : nullptr; k.min_len = t.min_len;
    rc = pack_enqueue(h, k);
  }
  if (!rc && o.profile) rc = profile_enqueue(h, profile_args(a, v.p1, v.p2, prof_thr, v.blk + m.prof));
  const PairArgs pa = pair_args(v, a, h->T);
  const size_t cap = (size_t)pa.cap1;                      // the carries lie where merge_layout put them
  if (!rc && o.accuracy) {                                 // behind everything that writes off / seq: it reads bases, the descriptors, off / seq and the truth
    AlignArgs k;
    static_cast<PairArgs&>(k) = pa;
    k.hc0 = (unsigned char*)(v.blk + m.hc); k.hc1 = k.hc0 + carry_layout((size_t)v.N, cap, 1, 1).hc1;
    k.accu = (unsigned long long*)(v.blk + m.accu); k.dist = nullptr;
    rc = align_enqueue(h, k);
  }
  if (!rc && o.errclass) {                                 // ... and behind it: the same inputs, carry words of its own
    ErrclassArgs k;
    static_cast<PairArgs&>(k) = pa;
    k.hc0 = (long long*)(v.blk + m.hc8); k.hc1 = (long long*)(v.blk + m.hc8 + carry_layout((size_t)v.N, cap, 8, 1).hc1);
    k.ecls = (unsigned long long*)(v.blk + m.ecls); k.dist = nullptr; k.match = nullptr;
    rc = errclass_enqueue(h, k);
  }
  if (!rc && o.infix) {                                    // ... and LAST: the same inputs on one strand or on both, carry words per strand
    const CarryLayout c = carry_layout((size_t)v.N, cap, 8, 2);
    InfixArgs k;
    static_cast<PairArgs&>(k) = pa;
    k.strands = o.strands; k.reverse = 0;
    k.hc0 = (long long*)(v.blk + m.hci); k.hs0 = (long long)(c.hs0 / 8);
    k.hc1 = (long long*)(v.blk + m.hci + c.hc1); k.hs1 = (long long)(c.hs1 / 8);
    k.infx = (unsigned long long*)(v.blk + m.infx); k.dist = k.match = k.start = k.end = nullptr;
    rc = infix_enqueue(h, k);
  }
  return rc;
}
// the trim rule a slot keeps
static TrimRule slot_trim(const nrv_handle::RawSlot& sl) { return TrimRule{sl.trim_thr, sl.trim_Q, sl.trim_W, sl.trim_min_len}; }
// the merged part of a slot's call
static MergeView slot_view(const nrv_handle::RawSlot& sl) {
  const char* const d = sl.d_out + 64;   // p1 / p2 are in the output block whether a quality is wanted or not
  return MergeView{(const SegRead*)(sl.d_in + sl.off_reads), sl.n_reads, sl.N, (const unsigned char*)(sl.d_in + sl.off_bases),
                   (const signed char*)(d + sl.rows * 44), (const signed char*)(d + sl.rows * 45), (const float*)d,
                   (const float*)(d + sl.rows * 24), (const long long*)(sl.d_in + sl.off_noff),
                   (const unsigned char*)(sl.d_in + sl.off_names), sl.d_mrg,
                   (const unsigned char*)(sl.d_in + sl.off_truth), (const long long*)(sl.d_in + sl.off_toff),
                   (const unsigned char*)(sl.d_in + sl.off_labels)};
}
// What comes back of a slot's call, on stream s.  A plain call: its output block.  A merged call: the counter and the merged block,
// all of [0, m.dl) - or, for a records call that hands back neither seq nor qual, the parts in front of and behind them; p1 / p2 /
// a1 / a2 stay on the device
static int slot_download(nrv_handle* h, nrv_handle::RawSlot& sl, hipStream_t s) {
  if (!sl.out.off) {
    HIPCHK(h, hipMemcpyAsync(sl.pin_out, sl.d_out, 64 + sl.rows * kOutBytes, hipMemcpyDeviceToHost, s));
    return NRV_OK;
  }
  HIPCHK(h, hipMemcpyAsync(sl.pin_out, sl.d_out, 64, hipMemcpyDeviceToHost, s));
  const MergeLayout& m = sl.m;
  const bool skip = sl.out.rec_off && !sl.out.seq && !sl.out.qual;
  HIPCHK(h, hipMemcpyAsync(sl.pin_mrg, sl.d_mrg, skip ? m.seq : m.dl, hipMemcpyDeviceToHost, s));
  if (skip) HIPCHK(h, hipMemcpyAsync(sl.pin_mrg + m.rep, sl.d_mrg + m.rep, m.dl - m.rep, hipMemcpyDeviceToHost, s));
  return NRV_OK;
}

// the arguments every raw-read entry point shares, and the two of the device statistics (filled positionally: keep the order)
struct RawIn {
  const int16_t* raw; int64_t n_raw; const int32_t* starts; const float* feat_ev; int64_t N; const nrv_read_desc* reads; int n_reads;
  const int32_t* last_dur = nullptr; const uint8_t* on_device = nullptr;
};
// nrv_reads_raw_begin (last_dur == nullptr: today's call, to the byte), nrv_reads_raw_stats_begin and (mr != nullptr: the inputs,
// with mo, what to hand back) nrv_revise_reads_raw_begin and the forms behind it
static int raw_begin(nrv_handle* h, const RawIn& in, float* p1, float* p2, int8_t* a1, int8_t* a2, int* ticket,
                     const MergeIn* mr = nullptr, const MergeOut* mo = nullptr) {
  int rc = check_handle(h);
  if (rc) return rc;
  const auto [raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device] = in;
  if (!ticket) { h->err = "nrv_reads_raw_begin: null ticket"; return NRV_E_INVALID; }
  if ((rc = raw_check(h, raw, n_raw, starts, feat_ev, N, reads, n_reads))) return rc;
  if (mr && (!mo->off || (N > 0 && (!mr->bases || (!mo->seq && !mo->rec_off))) || N >= ((int64_t)1 << 31))) {
    h->err = "nrv_revise_reads_raw_begin: null bases / seq / off (or 2^31 events and more)";
    return NRV_E_INVALID;
  }
  if (mr && mo->edit_off && N > h->T && !mo->edits) { h->err = "nrv_revise_reads_raw_edits_begin: null edits"; return NRV_E_INVALID; }
  const bool records = mr != nullptr && mo->rec_off != nullptr;
  size_t blob_cap = 0;
  if (records) {
    if (!names_ok(mr->names, mr->name_off, n_reads)) { h->err = "nrv_revise_reads_raw_records_begin: null names / name_off, or offsets that do not ascend from 0"; return NRV_E_INVALID; }
    // FASTQ or FASTA: by q_thr, whether qual is handed back or not
    blob_cap = blob_capacity(N, N - h->T > 0 ? N - h->T : 0, n_reads, mr->name_off[n_reads], mr->q_thr != nullptr);
    if (blob_cap > 0 && !mo->blob) { h->err = "nrv_revise_reads_raw_records_begin: null blob"; return NRV_E_INVALID; }
    if (blob_cap >= ((size_t)1 << 32)) { h->err = "nrv_revise_reads_raw_records_begin: records of 4 GiB and more in one call"; return NRV_E_INVALID; }
  }
  const bool accuracy = mr != nullptr && mo->wants_truth();   // (revise_begin has checked the truth)
  const bool with_stats = last_dur != nullptr || on_device != nullptr;
  const int64_t stat_len = with_stats ? stats_check(h, reads, n_reads, last_dur, on_device) : 0;
  if (stat_len < 0) return NRV_E_INVALID;
  int k = -1;
  for (int i = 0; i < 2; ++i) if (!h->raw_slot[i].busy) { k = i; break; }
  if (k < 0) { h->err = "nrv_reads_raw_begin: two calls are in flight already (collect one with nrv_reads_raw_end)"; return NRV_E_INVALID; }
  nrv_handle::RawSlot& sl = h->raw_slot[k];
  const int T = h->T;
  sl.N = N; sl.n = N - T > 0 ? N - T : 0; sl.n_reads = n_reads;
  sl.p1 = p1; sl.p2 = p2; sl.a1 = a1; sl.a2 = a2;
  *ticket = k;
  sl.out = mr ? *mo : MergeOut{};
  if (sl.n == 0) {                                              // nothing to compute: _end returns at once
    if (mr) merged_nothing(*mr, sl.out, reads, n_reads, N);
    sl.busy = true;
    return NRV_OK;
  }
  static_assert(sizeof(SegRead) == sizeof(nrv_read_desc), "descriptor layouts must match");
  sl.off_starts = up256((size_t)n_raw * 2);
  sl.off_reads = sl.off_starts + up256((size_t)N * 4);
  sl.off_feat = sl.off_reads + up256((size_t)n_reads * sizeof(SegRead));
  sl.off_aux = sl.off_feat + up256((size_t)N * kFeat * 4);
  sl.off_bases = sl.off_aux + (with_stats ? up256((size_t)n_reads * sizeof(StatAux)) : 0);
  sl.off_noff = sl.off_bases + (mr ? up256((size_t)N) : 0);
  sl.off_names = sl.off_noff + (records ? up256(((size_t)n_reads + 1) * 8) : 0);
  sl.off_toff = sl.off_names + (records ? up256((size_t)mr->name_off[n_reads]) : 0);
  sl.off_truth = sl.off_toff + (accuracy ? up256(((size_t)n_reads + 1) * 8) : 0);
  const bool score = mr != nullptr && mo->score != nullptr;   // (the entry point has checked labels / score_thr)
  sl.off_labels = sl.off_truth + (accuracy ? up256((size_t)mr->truth_off[n_reads]) : 0);
  const size_t in_bytes = sl.off_labels + (score ? up256((size_t)N) : 0);
  sl.rows = ((size_t)sl.n + kRowPad - 1) / kRowPad * kRowPad;
  const size_t out_bytes = 64 + sl.rows * kOutBytes;
  if (!sl.ev_in) {
    HIPCHK(h, hipEventCreateWithFlags(&sl.ev_in, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&sl.ev_out, hipEventDisableTiming));
  }
  if (in_bytes > sl.cap_in) {                                   // the slot is free: nothing of it is in flight
    (void)hipFree(sl.d_in); (void)hipHostFree(sl.pin_in);
    sl.d_in = sl.pin_in = nullptr; sl.cap_in = 0;
    const size_t c = in_bytes + in_bytes / 2 + 4096;
    HIPCHK(h, hipMalloc((void**)&sl.d_in, c));
    HIPCHK(h, hipHostMalloc((void**)&sl.pin_in, c, hipHostMallocDefault));
    sl.cap_in = c;
  }
  if (out_bytes > sl.cap_out) {
    (void)hipFree(sl.d_out); (void)hipHostFree(sl.pin_out);
    sl.d_out = sl.pin_out = nullptr; sl.cap_out = 0;
    const size_t c = out_bytes + out_bytes / 2 + 4096;
    HIPCHK(h, hipMalloc((void**)&sl.d_out, c));
    HIPCHK(h, hipMemset(sl.d_out, 0, 64));                      // the range-guard counter only ever grows
    HIPCHK(h, hipHostMalloc((void**)&sl.pin_out, c, hipHostMallocDefault));
    memset(sl.pin_out, 0, 64);
    sl.cap_out = c;
    sl.sat_seen = 0;
  }
  if (mr) {
    const MergeLayout& m = sl.m = merge_layout(N, sl.n, n_reads, sl.out, blob_cap);
    sl.blob_cap = blob_cap;
    sl.want_q = wants_quality(mr->q_thr, sl.out);
    if (sl.want_q) memcpy(sl.thr, mr->q_thr, sizeof sl.thr);    // the VALUES: the caller's inputs are gone when _end re-runs the call
    if (sl.out.profile) memcpy(sl.prof_thr, mr->prof_thr, sizeof sl.prof_thr);
    if (sl.out.trim) {
      memcpy(sl.trim_thr, mr->trim_thr, sizeof sl.trim_thr);
      sl.trim_Q = mr->Q; sl.trim_W = mr->W; sl.trim_min_len = mr->min_len;
    }
    if (score) memcpy(sl.score_thr, mr->score_thr, sizeof sl.score_thr);
    if ((sl.out.edit_off || records) && !h->edit_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->edit_stream, hipStreamNonBlocking));
    if (m.bytes > sl.cap_mrg) {
      (void)hipFree(sl.d_mrg); (void)hipHostFree(sl.pin_mrg);
      sl.d_mrg = sl.pin_mrg = nullptr; sl.cap_mrg = 0;
      const size_t c = m.bytes + m.bytes / 2 + 4096;
      HIPCHK(h, hipMalloc((void**)&sl.d_mrg, c));
      HIPCHK(h, hipHostMalloc((void**)&sl.pin_mrg, c, hipHostMallocDefault));
      sl.cap_mrg = c;
    }
  }
  const size_t stat_bytes = stat_len > 0 ? (size_t)n_reads * kStatWords * 4 : 0;
  if (stat_bytes > sl.cap_stat) {
    (void)hipFree(sl.d_stat);
    sl.d_stat = nullptr; sl.cap_stat = 0;
    HIPCHK(h, hipMalloc((void**)&sl.d_stat, stat_bytes));
    sl.cap_stat = stat_bytes;
  }
  if ((rc = ensure_workspace(h))) return rc;
  if (stat_bytes && (rc = poison_fill(h, sl.d_stat, sl.cap_stat, h->stream))) return rc;   // NRV_POISON: stats_enqueue zeroes what it uses
  // inputs -> page-locked staging (a host copy of 92 B per base that overlaps the previous call's kernels) -> ONE upload
  if (h->poison_on) {          // NRV_POISON: the slot's buffers (the alignment gaps between the input parts included), not the counter
    for (size_t i = 0; i + 4 <= in_bytes; i += 4) memcpy(sl.pin_in + i, &h->poison, 4);
    if ((rc = poison_fill(h, sl.d_in, sl.cap_in, h->copy_stream)) || (rc = poison_fill(h, sl.d_out + 64, sl.cap_out - 64, h->stream)))
      return rc;
    if (mr) {
      for (size_t i = 0; i + 4 <= sl.m.dl; i += 4) memcpy(sl.pin_mrg + i, &h->poison, 4);
      if (sl.out.edit_off) for (size_t i = sl.m.edits; i + 4 <= sl.m.etile; i += 4) memcpy(sl.pin_mrg + i, &h->poison, 4);
      if (records) for (size_t i = sl.m.blob; i + 4 <= sl.m.tq; i += 4) memcpy(sl.pin_mrg + i, &h->poison, 4);
      if ((rc = poison_fill(h, sl.d_mrg, sl.cap_mrg, h->stream))) return rc;
    }
  }
  memcpy(sl.pin_in, raw, (size_t)n_raw * 2);
  if (mr) memcpy(sl.pin_in + sl.off_bases, mr->bases, (size_t)N);
  if (records) {
    memcpy(sl.pin_in + sl.off_noff, mr->name_off, ((size_t)n_reads + 1) * 8);
    if (mr->name_off[n_reads] > 0) memcpy(sl.pin_in + sl.off_names, mr->names, (size_t)mr->name_off[n_reads]);
  }
  if (accuracy) {
    memcpy(sl.pin_in + sl.off_toff, mr->truth_off, ((size_t)n_reads + 1) * 8);
    if (mr->truth_off[n_reads] > 0) memcpy(sl.pin_in + sl.off_truth, mr->truth, (size_t)mr->truth_off[n_reads]);
  }
  if (score) memcpy(sl.pin_in + sl.off_labels, mr->labels, (size_t)N);
  memcpy(sl.pin_in + sl.off_starts, starts, (size_t)N * 4);
  memcpy(sl.pin_in + sl.off_reads, reads, (size_t)n_reads * sizeof(SegRead));
  memcpy(sl.pin_in + sl.off_feat, feat_ev, (size_t)N * kFeat * 4);
  if (with_stats) {
    StatAux* ax = (StatAux*)(sl.pin_in + sl.off_aux);
    for (int r = 0; r < n_reads; ++r) ax[r] = StatAux{last_dur[r], on_device[r] ? 1 : 0};
  }
  HIPCHK(h, hipMemcpyAsync(sl.d_in, sl.pin_in, in_bytes, hipMemcpyHostToDevice, h->copy_stream));
  HIPCHK(h, hipEventRecord(sl.ev_in, h->copy_stream));
  HIPCHK(h, hipStreamWaitEvent(h->stream, sl.ev_in, 0));
  // statistics first: every segmentation stage below (and the f32 re-run of _end, which reuses the slot's inputs) reads the
  // descriptors and feature columns they leave in d_in
  if (stat_len > 0)
    rc = stats_enqueue(h, (const int16_t*)sl.d_in, (const int32_t*)(sl.d_in + sl.off_starts), (SegRead*)(sl.d_in + sl.off_reads),
                       (const StatAux*)(sl.d_in + sl.off_aux), sl.d_stat, n_reads, N, stat_len, (float*)(sl.d_in + sl.off_feat),
                       nullptr, nullptr);
  // the merge reads the slot's output block: behind the call's last launch group, ahead of ev_done
  if (rc || (rc = raw_enqueue(h, sl)) ||
      (mr && (rc = merged_enqueue(h, slot_view(sl), sl.m, sl.out, sl.want_q ? sl.thr : nullptr, sl.prof_thr, sl.blob_cap, slot_trim(sl), sl.score_thr)))) {
    (void)hipStreamSynchronize(h->stream);                      // part of the call may be enqueued: nothing of it may outlive the slot
    return rc;
  }
  HIPCHK(h, hipEventRecord(sl.ev_done, h->stream));
  HIPCHK(h, hipStreamWaitEvent(h->d2h_stream, sl.ev_done, 0));
  if ((rc = slot_download(h, sl, h->d2h_stream))) return rc;
  HIPCHK(h, hipEventRecord(sl.ev_out, h->d2h_stream));
  HIPCHK(h, hipGetLastError());
  sl.busy = true;
  return NRV_OK;
}

// Every nrv_revise_reads_raw*_begin: the argument checks they share, under the entry point's name `who`, then raw_begin.
// missing: what the entry point itself requires and did not get ("null report", ...), or null
static int revise_begin(nrv_handle* h, const char* who, const char* missing, const RawIn& in, const MergeIn& mr, const MergeOut& mo,
                        int* ticket) {
  const char* bad = nullptr;
  if ((in.last_dur == nullptr) != (in.on_device == nullptr)) bad = "last_dur and on_device go together";
  else if (missing) bad = missing;
  else if (mo.edits && !mo.edit_off) bad = "edits without edit_off";
  else if (!mo.rec_off && (mr.names || mr.name_off || mo.blob)) bad = "names / name_off / blob without rec_off";
  else if ((mr.prof_thr == nullptr) != (mo.profile == nullptr)) bad = "prof_thr and profile go together";
  else if (mo.trim && !trim_rule_ok(mr.Q, mr.W, mr.min_len)) bad = "Q must be in 1 .. 40, W in 1 .. 64 and min_len >= 0";
  else if (mo.wants_truth() && (in.n_reads < 0 || !truth_ok(mr.truth, mr.truth_off, in.n_reads)))
    bad = "null truth / truth_off, offsets that do not ascend from 0, or a truth of 2^31 - 64 characters and more";
  else if (mo.wants_truth() && in.N >= ((int64_t)1 << 30)) bad = "2^30 events and more in a call with a truth";
  else if (mo.infix && mo.strands != 1 && mo.strands != 2) bad = "strands must be 1 or 2";
  else if (mo.infix && !infix_lengths_ok(mr.truth_off, in.n_reads, nullptr, in.reads))
    bad = "a truth region, or a read that has one, above NRV_INFIX_MAX_LEN = 2^21 - 1 characters";
  if (h && bad) { h->err = std::string(who) + ": " + bad; return NRV_E_INVALID; }
  return raw_begin(h, in, nullptr, nullptr, nullptr, nullptr, ticket, &mr, &mo);
}

int nrv_reads_raw_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                        const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                        float* p1, float* p2, int8_t* a1, int8_t* a2, int* ticket) {
  return raw_begin(h, RawIn{raw, n_raw, starts, feat_ev, N, reads, n_reads}, p1, p2, a1, a2, ticket);
}

int nrv_reads_raw_stats_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                              const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                              const int32_t* last_dur, const uint8_t* on_device,
                              float* p1, float* p2, int8_t* a1, int8_t* a2, int* ticket) {
  if (h && n_reads > 0 && (!last_dur || !on_device)) { h->err = "nrv_reads_raw_stats_begin: null last_dur / flags"; return NRV_E_INVALID; }
  static const int32_t no_dur = 0;
  static const uint8_t no_flag = 0;
  return raw_begin(h, RawIn{raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur ? last_dur : &no_dur, on_device ? on_device : &no_flag},
                   p1, p2, a1, a2, ticket);
}

int nrv_predict_reads_raw_stats(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                const int32_t* last_dur, const uint8_t* on_device,
                                float* p1, float* p2, int8_t* a1, int8_t* a2) {
  return begin_then_end(h, [&](int* t) {
    return nrv_reads_raw_stats_begin(h, raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device, p1, p2, a1, a2, t);
  });
}

int nrv_revise_reads_raw_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                               const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                               const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                               uint8_t* seq, uint8_t* qual, int64_t* off, int* ticket) {
  return revise_begin(h, "nrv_revise_reads_raw_begin", nullptr, RawIn{raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device},
                      MergeIn{bases, q_thr}, MergeOut{seq, qual, off}, ticket);
}

int nrv_revise_reads_raw(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                         const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                         const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                         uint8_t* seq, uint8_t* qual, int64_t* off) {
  return begin_then_end(h, [&](int* t) {
    return nrv_revise_reads_raw_begin(h, raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device, bases, q_thr, seq, qual, off, t);
  });
}

int nrv_revise_reads_raw_report_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                      const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                      const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                      uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report, int* ticket) {
  return revise_begin(h, "nrv_revise_reads_raw_report_begin", report ? nullptr : "null report",
                      RawIn{raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device}, MergeIn{bases, q_thr},
                      MergeOut{seq, qual, off, report, tie_eps}, ticket);
}

int nrv_revise_reads_raw_report(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report) {
  return begin_then_end(h, [&](int* t) {
    return nrv_revise_reads_raw_report_begin(h, raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device, bases, q_thr,
                                             seq, qual, off, tie_eps, report, t);
  });
}

// report == NULL: none is counted (here and in the forms below)
int nrv_revise_reads_raw_edits_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                     const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                     const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                     uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                     nrv_edit* edits, int64_t* edit_off, int* ticket) {
  return revise_begin(h, "nrv_revise_reads_raw_edits_begin", edit_off ? nullptr : "null edit_off",
                      RawIn{raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device}, MergeIn{bases, q_thr},
                      MergeOut{seq, qual, off, report, tie_eps, edits, edit_off}, ticket);
}

int nrv_revise_reads_raw_edits(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                               const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                               const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                               uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                               nrv_edit* edits, int64_t* edit_off) {
  return begin_then_end(h, [&](int* t) {
    return nrv_revise_reads_raw_edits_begin(h, raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device, bases, q_thr,
                                            seq, qual, off, tie_eps, report, edits, edit_off, t);
  });
}

// edit_off == NULL: no edit list (here and in the form below)
int nrv_revise_reads_raw_records_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                       const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                       const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                       uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                       nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                       uint8_t* blob, int64_t* rec_off, int* ticket) {
  return revise_begin(h, "nrv_revise_reads_raw_records_begin", rec_off ? nullptr : "null rec_off",
                      RawIn{raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device}, MergeIn{bases, q_thr, names, name_off},
                      MergeOut{seq, qual, off, report, tie_eps, edits, edit_off, blob, rec_off}, ticket);
}

int nrv_revise_reads_raw_records(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                 const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                 const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                 uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                 nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                 uint8_t* blob, int64_t* rec_off) {
  return begin_then_end(h, [&](int* t) {
    return nrv_revise_reads_raw_records_begin(h, raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device, bases, q_thr,
                                              seq, qual, off, tie_eps, report, edits, edit_off, names, name_off, blob, rec_off, t);
  });
}

// rec_off == NULL: no records
int nrv_revise_reads_raw_profile_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                       const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                       const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                       uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                       nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                       uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile, int* ticket) {
  return revise_begin(h, "nrv_revise_reads_raw_profile_begin", prof_thr && profile ? nullptr : "null prof_thr / profile",
                      RawIn{raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device},
                      MergeIn{bases, q_thr, names, name_off, prof_thr},
                      MergeOut{seq, qual, off, report, tie_eps, edits, edit_off, blob, rec_off, profile}, ticket);
}

int nrv_revise_reads_raw_profile(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                 const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                 const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                 uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                 nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                 uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile) {
  return begin_then_end(h, [&](int* t) {
    return nrv_revise_reads_raw_profile_begin(h, raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device, bases, q_thr,
                                              seq, qual, off, tie_eps, report, edits, edit_off, names, name_off, blob, rec_off,
                                              prof_thr, profile, t);
  });
}

// prof_thr / profile == NULL: no profile
int nrv_revise_reads_raw_trim_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                    const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                    const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                    uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                    nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                    uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                    const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim, int* ticket) {
  return revise_begin(h, "nrv_revise_reads_raw_trim_begin", trim_thr && trim ? nullptr : "null trim_thr / trim",
                      RawIn{raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device},
                      MergeIn{bases, q_thr, names, name_off, prof_thr, trim_thr, Q, W, min_len},
                      MergeOut{seq, qual, off, report, tie_eps, edits, edit_off, blob, rec_off, profile, trim}, ticket);
}

int nrv_revise_reads_raw_trim(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                              const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                              const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                              uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                              nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                              uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                              const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim) {
  return begin_then_end(h, [&](int* t) {
    return nrv_revise_reads_raw_trim_begin(h, raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device, bases, q_thr,
                                           seq, qual, off, tie_eps, report, edits, edit_off, names, name_off, blob, rec_off,
                                           prof_thr, profile, trim_thr, Q, W, min_len, trim, t);
  });
}

// every earlier block may be NULL, the trim included: trim == NULL, no rule is checked and no trim enqueued
int nrv_revise_reads_raw_accuracy_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                        const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                        const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                        uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                        nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                        uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                        const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                                        const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, int* ticket) {
  const char* missing = nullptr;
  if (!accuracy || !truth_off) missing = "null truth_off / accuracy";
  else if (trim && !trim_thr) missing = "trim without trim_thr";
  return revise_begin(h, "nrv_revise_reads_raw_accuracy_begin", missing,
                      RawIn{raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device},
                      MergeIn{bases, q_thr, names, name_off, prof_thr, trim_thr, Q, W, min_len, truth, truth_off},
                      MergeOut{seq, qual, off, report, tie_eps, edits, edit_off, blob, rec_off, profile, trim, accuracy}, ticket);
}

int nrv_revise_reads_raw_accuracy(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                  const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                  const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                  uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                  nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                  uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                  const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                                  const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy) {
  return begin_then_end(h, [&](int* t) {
    return nrv_revise_reads_raw_accuracy_begin(h, raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device, bases, q_thr,
                                               seq, qual, off, tie_eps, report, edits, edit_off, names, name_off, blob, rec_off,
                                               prof_thr, profile, trim_thr, Q, W, min_len, trim, truth, truth_off, accuracy, t);
  });
}

// every earlier block may be NULL, the accuracy included: the truth is then read by the error classes alone
int nrv_revise_reads_raw_errclass_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                        const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                        const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                        uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                        nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                        uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                        const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                                        const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, uint64_t* errclass, int* ticket) {
  const char* missing = nullptr;
  if (!errclass || !truth_off) missing = "null truth_off / errclass";
  else if (trim && !trim_thr) missing = "trim without trim_thr";
  MergeOut mo{seq, qual, off, report, tie_eps, edits, edit_off, blob, rec_off, profile, trim, accuracy};
  mo.errclass = errclass;
  return revise_begin(h, "nrv_revise_reads_raw_errclass_begin", missing,
                      RawIn{raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device},
                      MergeIn{bases, q_thr, names, name_off, prof_thr, trim_thr, Q, W, min_len, truth, truth_off}, mo, ticket);
}

int nrv_revise_reads_raw_errclass(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                  const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                  const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                  uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                  nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                  uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                  const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                                  const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, uint64_t* errclass) {
  return begin_then_end(h, [&](int* t) {
    return nrv_revise_reads_raw_errclass_begin(h, raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device, bases, q_thr,
                                               seq, qual, off, tie_eps, report, edits, edit_off, names, name_off, blob, rec_off,
                                               prof_thr, profile, trim_thr, Q, W, min_len, trim, truth, truth_off, accuracy, errclass, t);
  });
}

// every earlier block may be NULL, the accuracy and the error classes included: the truth is then read by the infix block alone
int nrv_revise_reads_raw_infix_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                     const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                     const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                     uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                     nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                     uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                     const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                                     const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, uint64_t* errclass,
                                     int strands, uint64_t* infix, int* ticket) {
  const char* missing = nullptr;
  if (!infix || !truth_off) missing = "null truth_off / infix";
  else if (trim && !trim_thr) missing = "trim without trim_thr";
  MergeOut mo{seq, qual, off, report, tie_eps, edits, edit_off, blob, rec_off, profile, trim, accuracy};
  mo.errclass = errclass; mo.infix = infix; mo.strands = strands;
  return revise_begin(h, "nrv_revise_reads_raw_infix_begin", missing,
                      RawIn{raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device},
                      MergeIn{bases, q_thr, names, name_off, prof_thr, trim_thr, Q, W, min_len, truth, truth_off}, mo, ticket);
}

int nrv_revise_reads_raw_infix(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                               const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                               const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                               uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                               nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                               uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                               const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                               const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, uint64_t* errclass,
                               int strands, uint64_t* infix) {
  return begin_then_end(h, [&](int* t) {
    return nrv_revise_reads_raw_infix_begin(h, raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device, bases, q_thr,
                                            seq, qual, off, tie_eps, report, edits, edit_off, names, name_off, blob, rec_off,
                                            prof_thr, profile, trim_thr, Q, W, min_len, trim, truth, truth_off, accuracy, errclass,
                                            strands, infix, t);
  });
}

// every earlier block may be NULL, the truth and the infix block included: the score reads the labels, not the truth
int nrv_revise_reads_raw_score_begin(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                                     const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                                     const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                                     uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                                     nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                                     uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                                     const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                                     const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, uint64_t* errclass,
                                     int strands, uint64_t* infix, const uint8_t* labels, const float* score_thr, uint64_t* score,
                                     int* ticket) {
  const char* missing = nullptr;
  if (!labels || !score_thr || !score) missing = "null labels / score_thr / score";
  else if (trim && !trim_thr) missing = "trim without trim_thr";
  MergeOut mo{seq, qual, off, report, tie_eps, edits, edit_off, blob, rec_off, profile, trim, accuracy};
  mo.errclass = errclass; mo.infix = infix; mo.strands = strands; mo.score = score;
  MergeIn mi{bases, q_thr, names, name_off, prof_thr, trim_thr, Q, W, min_len, truth, truth_off};
  mi.labels = labels; mi.score_thr = score_thr;
  return revise_begin(h, "nrv_revise_reads_raw_score_begin", missing,
                      RawIn{raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device}, mi, mo, ticket);
}

int nrv_revise_reads_raw_score(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                               const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                               const int32_t* last_dur, const uint8_t* on_device, const uint8_t* bases, const float* q_thr,
                               uint8_t* seq, uint8_t* qual, int64_t* off, float tie_eps, uint64_t* report,
                               nrv_edit* edits, int64_t* edit_off, const uint8_t* names, const int64_t* name_off,
                               uint8_t* blob, int64_t* rec_off, const float* prof_thr, uint64_t* profile,
                               const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                               const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy, uint64_t* errclass,
                               int strands, uint64_t* infix, const uint8_t* labels, const float* score_thr, uint64_t* score) {
  return begin_then_end(h, [&](int* t) {
    return nrv_revise_reads_raw_score_begin(h, raw, n_raw, starts, feat_ev, N, reads, n_reads, last_dur, on_device, bases, q_thr,
                                            seq, qual, off, tie_eps, report, edits, edit_off, names, name_off, blob, rec_off,
                                            prof_thr, profile, trim_thr, Q, W, min_len, trim, truth, truth_off, accuracy, errclass,
                                            strands, infix, labels, score_thr, score, t);
  });
}

int nrv_reads_raw_end(nrv_handle* h, int ticket) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (ticket < 0 || ticket > 1 || !h->raw_slot[ticket].busy) { h->err = "nrv_reads_raw_end: no such call in flight"; return NRV_E_INVALID; }
  nrv_handle::RawSlot& sl = h->raw_slot[ticket];
  sl.busy = false;                                              // whatever happens below, the slot is the caller's again
  if (sl.n == 0) return NRV_OK;
  HIPCHK(h, hipEventSynchronize(sl.ev_out));
  if (*(unsigned*)sl.pin_out != sl.sat_seen) {
    // f16x2 range guard: some stage of this call left the f16 range.  Its inputs are still in the slot: the whole call
    // again on the f32 kernels, which have no range limit (behind whatever the other slot has enqueued meanwhile).
    const int h2 = h->h2, split = h->split;
    if ((rc = poison_fill(h, sl.d_out + 64, sl.cap_out - 64, h->stream))) return rc;
    h->h2 = 0; h->split = 0;
    const int rc2 = raw_enqueue(h, sl);
    h->h2 = h2; h->split = split;
    if (rc2) return rc2;
    // a merged call: its kernels again, in stream order behind the re-run they read, on a block that holds nothing of the first pass
    if (sl.out.off && ((rc = poison_fill(h, sl.d_mrg, sl.cap_mrg, h->stream)) ||
                       (rc = merged_enqueue(h, slot_view(sl), sl.m, sl.out, sl.want_q ? sl.thr : nullptr, sl.prof_thr, sl.blob_cap, slot_trim(sl), sl.score_thr))))
      return rc;
    if ((rc = slot_download(h, sl, h->stream))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    sl.sat_seen = *(unsigned*)sl.pin_out;
    h->sat_reruns += 1;
  }
  if (sl.out.off) {
    // the used prefix alone: a copy of its own size on a stream of its own - the records are complete (ev_done lies behind the
    // edit kernels, or the re-run above was waited for), and neither the compute stream nor d2h_stream, which may hold the other
    // slot's kernels or wait for them, stands in front of it
    auto fetch = [&](void* dst, size_t at, size_t bytes) -> int {
      HIPCHK(h, hipMemcpyAsync(sl.pin_mrg + at, sl.d_mrg + at, bytes, hipMemcpyDeviceToHost, h->edit_stream));
      HIPCHK(h, hipStreamSynchronize(h->edit_stream));
      memcpy(dst, sl.pin_mrg + at, bytes);
      return NRV_OK;
    };
    return merged_collect(h, "nrv_reads_raw_end", "nrv_reads_raw_end", sl.pin_mrg, slot_view(sl), sl.m, sl.out, sl.want_q, sl.blob_cap, fetch);
  }
  const char* o = sl.pin_out + 64;
  const size_t n = (size_t)sl.n;
  if (sl.p1) memcpy(sl.p1, o, n * 24);
  if (sl.p2) memcpy(sl.p2, o + sl.rows * 24, n * 20);
  if (sl.a1) memcpy(sl.a1, o + sl.rows * 44, n);
  if (sl.a2) memcpy(sl.a2, o + sl.rows * 45, n);
  return NRV_OK;
}

int nrv_predict_reads_raw(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts,
                          const float* feat_ev, int64_t N, const nrv_read_desc* reads, int n_reads,
                          float* p1, float* p2, int8_t* a1, int8_t* a2) {
  int rc = check_handle(h);
  if (rc) return rc;
  // NRV_RAW_STAGED=1: round 5's form (per-stage uploads and downloads through predict_host's staging sets); default since r06:
  // the whole call at once (nrv_reads_raw_begin + _end).  Same kernels on the same windows: the same bits.
  static const bool staged = getenv("NRV_RAW_STAGED") && atoi(getenv("NRV_RAW_STAGED")) != 0;
  if (!staged && !h->raw_slot[0].busy && !h->raw_slot[1].busy) {
    return begin_then_end(h, [&](int* t) { return nrv_reads_raw_begin(h, raw, n_raw, starts, feat_ev, N, reads, n_reads, p1, p2, a1, a2, t); });
  }
  if ((rc = upload_raw(h, raw, n_raw, starts, N, reads, n_reads))) return rc;
  return predict_host(h, nullptr, feat_ev, N, true, p1, p2, a1, a2, n_reads);
}

int nrv_segment_reads(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts, int64_t N,
                      const nrv_read_desc* reads, int n_reads, float* sig_ev) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (N > 0 && !sig_ev) { h->err = "nrv_segment_reads: null output"; return NRV_E_INVALID; }
  if ((rc = upload_raw(h, raw, n_raw, starts, N, reads, n_reads))) return rc;
  const int64_t chunk = (int64_t)h->cap_rows * h->T;        // events the staging buffer holds
  for (int64_t e0 = 0; e0 < N; e0 += chunk) {
    const int ne = (int)((N - e0 < chunk) ? (N - e0) : chunk);
    if ((rc = poison_fill(h, h->d_sig[0], h->sig_bytes, h->stream))) return rc;
    launch_segment(h, n_reads, e0, ne, h->d_sig[0]);
    HIPCHK(h, hipMemcpyAsync(sig_ev + e0 * kSig, h->d_sig[0], (size_t)ne * kSig * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return NRV_OK;
}

int nrv_read_stats(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts, int64_t N,
                   const nrv_read_desc* reads, int n_reads, const int32_t* last_dur, double* shift, double* scale,
                   double* mean, double* std, float* feat12) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((n_reads > 0 && (!last_dur || !shift || !scale)) || (N > 0 && (!mean || !std || !feat12))) { h->err = "nrv_read_stats: null argument"; return NRV_E_INVALID; }
  if ((rc = upload_raw(h, raw, n_raw, starts, N, reads, n_reads))) return rc;
  if (n_reads == 0) return NRV_OK;
  const std::vector<uint8_t> on((size_t)n_reads, 1);
  const int64_t max_len = stats_check(h, reads, n_reads, last_dur, on.data());
  if (max_len < 0) return NRV_E_INVALID;
  // one block of its own for everything the kernels write besides the descriptors: [aux | scratch | mean | std | feat]
  const size_t o_scr = up256((size_t)n_reads * sizeof(StatAux)), o_mean = o_scr + up256((size_t)n_reads * kStatWords * 4);
  const size_t o_std = o_mean + up256((size_t)N * 8), o_feat = o_std + up256((size_t)N * 8), bytes = o_feat + up256((size_t)N * kFeat * 4);
  std::vector<StatAux> ax((size_t)n_reads);
  for (int r = 0; r < n_reads; ++r) ax[r] = StatAux{last_dur[r], 1};
  std::vector<float> feat((size_t)N * kFeat);
  std::vector<SegRead> back((size_t)n_reads);
  char* d = nullptr;
  HIPCHK(h, hipMalloc((void**)&d, bytes));
  auto run = [&]() -> int {
    int rc2 = poison_fill(h, d, bytes, h->stream);
    if (rc2) return rc2;
    HIPCHK(h, hipMemcpyAsync(d, ax.data(), (size_t)n_reads * sizeof(StatAux), hipMemcpyHostToDevice, h->stream));
    if ((rc2 = stats_enqueue(h, h->d_raw, h->d_starts, h->d_reads, (const StatAux*)d, (unsigned*)(d + o_scr), n_reads, N, max_len,
                             (float*)(d + o_feat), (double*)(d + o_mean), (double*)(d + o_std))))
      return rc2;
    HIPCHK(h, hipMemcpyAsync(back.data(), h->d_reads, (size_t)n_reads * sizeof(SegRead), hipMemcpyDeviceToHost, h->stream));
    if (N) {
      HIPCHK(h, hipMemcpyAsync(mean, d + o_mean, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipMemcpyAsync(std, d + o_std, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipMemcpyAsync(feat.data(), d + o_feat, (size_t)N * kFeat * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return NRV_OK;
  };
  rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  (void)hipFree(d);
  if (rc) return rc;
  for (int r = 0; r < n_reads; ++r) { shift[r] = back[r].shift; scale[r] = back[r].scale; }
  for (int64_t e = 0; e < N; ++e) { feat12[2 * e] = feat[e * kFeat + 1]; feat12[2 * e + 1] = feat[e * kFeat + 2]; }
  return NRV_OK;
}

// nrv_merge_calls (o.report == nullptr: that call, to the byte), nrv_merge_calls_report, (o.edit_off != nullptr)
// nrv_merge_calls_edits, (o.profile != nullptr) nrv_merge_calls_profile and (o.trim != nullptr; `more`: its rule, and the names of
// its records) nrv_merge_calls_trim, (o.accuracy != nullptr; `more`: the truth) nrv_merge_calls_accuracy and (o.errclass != nullptr;
// `more`: the truth) nrv_merge_calls_errclass and (o.infix != nullptr; `more`: the truth) nrv_merge_calls_infix and (o.score !=
// nullptr; `more`: the labels and their thresholds) nrv_merge_calls_score
static int merge_calls_impl(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                            const float* p1, const float* p2, int64_t n_win, const float* q_thr, const MergeOut& o,
                            const float* prof_thr = nullptr, const MergeIn& more = MergeIn{}) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (n_reads < 0 || n_win < 0 || !o.off || (n_reads > 0 && !ev_len)) { h->err = "nrv_merge_calls: bad arguments"; return NRV_E_INVALID; }
  std::vector<nrv_read_desc> rd((size_t)n_reads);
  int64_t N = 0;
  for (int r = 0; r < n_reads; ++r) {
    if (ev_len[r] < 0 || N + ev_len[r] >= ((int64_t)1 << 31)) { h->err = "nrv_merge_calls: a negative read length (or 2^31 events and more)"; return NRV_E_INVALID; }
    rd[r] = nrv_read_desc{0, 0, N, ev_len[r], 0., 0.};
    N += ev_len[r];
  }
  const int64_t n = N - h->T > 0 ? N - h->T : 0;
  const bool want_q = wants_quality(q_thr, o);
  if (n_win != n || (N > 0 && (!bases || !o.seq)) || (n > 0 && (!a1 || !a2 || (want_q && (!p1 || !p2))))) {
    h->err = "nrv_merge_calls: n_win is not sum(ev_len) - T, or a null array";
    return NRV_E_INVALID;
  }
  size_t blob_cap = 0;
  if (o.rec_off) {
    if (!names_ok(more.names, more.name_off, n_reads)) { h->err = "nrv_merge_calls_trim: null names / name_off, or offsets that do not ascend from 0"; return NRV_E_INVALID; }
    blob_cap = blob_capacity(N, n, n_reads, more.name_off[n_reads], q_thr != nullptr);
    if ((blob_cap > 0 && !o.blob) || blob_cap >= ((size_t)1 << 32)) { h->err = "nrv_merge_calls_trim: null blob (or records of 4 GiB and more)"; return NRV_E_INVALID; }
  }
  const std::string who_truth = o.infix ? "nrv_merge_calls_infix" : o.errclass ? "nrv_merge_calls_errclass" : "nrv_merge_calls_accuracy";
  if (o.wants_truth() && !truth_ok(more.truth, more.truth_off, n_reads)) {
    h->err = who_truth + ": null truth / truth_off, offsets that do not ascend from 0, or a truth of 2^31 - 64 characters and more";
    return NRV_E_INVALID;
  }
  if (o.wants_truth() && N >= ((int64_t)1 << 30)) { h->err = who_truth + ": 2^30 events and more"; return NRV_E_INVALID; }
  if (o.infix) {
    bool ok = o.strands == 1 || o.strands == 2;
    for (int r = 0; ok && r < n_reads; ++r) {
      const int64_t tl = more.truth_off[r + 1] - more.truth_off[r];
      ok = tl <= NRV_INFIX_MAX_LEN && (tl == 0 || ev_len[r] <= NRV_INFIX_MAX_LEN);
    }
    if (!ok) { h->err = who_truth + ": strands must be 1 or 2, and no truth region or read that has one above NRV_INFIX_MAX_LEN = 2^21 - 1 characters"; return NRV_E_INVALID; }
  }
  if (n == 0) {
    MergeIn in = more;
    in.bases = bases; in.q_thr = q_thr;
    merged_nothing(in, o, rd.data(), n_reads, N);
    return NRV_OK;
  }
  if (o.edit_off && !o.edits) { h->err = "nrv_merge_calls_edits: null edits"; return NRV_E_INVALID; }
  // one block of its own: [reads | bases | a1 | a2 | p1 | p2 | name_off | names | truth_off | truth | merged block]
  const MergeLayout m = merge_layout(N, n, n_reads, o, blob_cap);
  // the rows go up for a quality - and without one where they are given and the report's near-tie column, the edits' conf, the
  // profile or the trim reads them
  const bool have_p = want_q || ((o.report || o.edit_off || o.profile || o.trim || o.score) && p1 && p2);
  const bool records = o.rec_off != nullptr, truth = o.wants_truth();
  const size_t name_bytes = records ? (size_t)more.name_off[n_reads] : 0, truth_bytes = truth ? (size_t)more.truth_off[n_reads] : 0;
  const size_t nb = ((size_t)n_reads + 1) * 8;
  const MergeInLayout l = merge_in_layout((size_t)n_reads, sizeof(SegRead), (size_t)N, (size_t)n, have_p, records, name_bytes, truth,
                                          truth_bytes, m.bytes, o.score != nullptr);
  std::vector<char> back(m.dl);
  hipStream_t const s = h->stream;
  return with_block(h, l.bytes, s, [&](char* d) -> int {
    int rc2;
    if ((rc2 = put(h, d + l.reads, rd.data(), (size_t)n_reads * sizeof(SegRead), s)) || (rc2 = put(h, d + l.bases, bases, (size_t)N, s)) ||
        (rc2 = put(h, d + l.a1, a1, (size_t)n, s)) || (rc2 = put(h, d + l.a2, a2, (size_t)n, s)) ||
        (rc2 = put(h, d + l.p1, p1, have_p ? (size_t)n * 24 : 0, s)) || (rc2 = put(h, d + l.p2, p2, have_p ? (size_t)n * 20 : 0, s)) ||
        (rc2 = put(h, d + l.name_off, more.name_off, records ? nb : 0, s)) || (rc2 = put(h, d + l.names, more.names, name_bytes, s)) ||
        (rc2 = put(h, d + l.truth_off, more.truth_off, truth ? nb : 0, s)) || (rc2 = put(h, d + l.truth, more.truth, truth_bytes, s)) ||
        (rc2 = put(h, d + l.labels, more.labels, o.score ? (size_t)N : 0, s)))
      return rc2;
    const MergeView v{(const SegRead*)(d + l.reads), n_reads, N, (const unsigned char*)(d + l.bases), (const signed char*)(d + l.a1),
                      (const signed char*)(d + l.a2), have_p ? (const float*)(d + l.p1) : nullptr,
                      have_p ? (const float*)(d + l.p2) : nullptr, (const long long*)(d + l.name_off), (const unsigned char*)(d + l.names),
                      d + l.merged, (const unsigned char*)(d + l.truth), (const long long*)(d + l.truth_off),
                      (const unsigned char*)(d + l.labels)};
    if ((rc2 = merged_enqueue(h, v, m, o, want_q ? q_thr : nullptr, prof_thr, blob_cap, TrimRule{more.trim_thr, more.Q, more.W, more.min_len},
                              more.score_thr)))
      return rc2;
    HIPCHK(h, hipMemcpyAsync(back.data(), d + l.merged, m.dl, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    // a test twin, not timed: the used prefix of the edit records in a plain copy, straight into the caller's array
    auto fetch = [&](void* dst, size_t at, size_t bytes) -> int {
      HIPCHK(h, hipMemcpy(dst, d + l.merged + at, bytes, hipMemcpyDeviceToHost));
      return NRV_OK;
    };
    return merged_collect(h, "nrv_merge_calls", "nrv_merge_calls_edits", back.data(), v, m, o, want_q, blob_cap, fetch);
  });
}

int nrv_merge_calls(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                    const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off) {
  return merge_calls_impl(h, bases, ev_len, n_reads, a1, a2, p1, p2, n_win, q_thr, MergeOut{seq, qual, off});
}

int nrv_merge_calls_report(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                           const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                           float tie_eps, uint64_t* report) {
  if (h && n_reads > 0 && !report) { h->err = "nrv_merge_calls_report: null report"; return NRV_E_INVALID; }
  static uint64_t none[NRV_REPORT_COLS];
  return merge_calls_impl(h, bases, ev_len, n_reads, a1, a2, p1, p2, n_win, q_thr, MergeOut{seq, qual, off, report ? report : none, tie_eps});
}

int nrv_merge_calls_edits(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                          const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                          float tie_eps, uint64_t* report, nrv_edit* edits, int64_t* edit_off) {
  if (h && !edit_off) { h->err = "nrv_merge_calls_edits: null edit_off"; return NRV_E_INVALID; }
  return merge_calls_impl(h, bases, ev_len, n_reads, a1, a2, p1, p2, n_win, q_thr, MergeOut{seq, qual, off, report, tie_eps, edits, edit_off});
}

int nrv_merge_calls_profile(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                            const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                            const float* prof_thr, uint64_t* profile) {
  if (h && (!prof_thr || !profile)) { h->err = "nrv_merge_calls_profile: null prof_thr / profile"; return NRV_E_INVALID; }
  if (h && (!p1 || !p2)) { h->err = "nrv_merge_calls_profile: null p1 / p2"; return NRV_E_INVALID; }
  MergeOut o{seq, qual, off};
  o.profile = profile;
  return merge_calls_impl(h, bases, ev_len, n_reads, a1, a2, p1, p2, n_win, q_thr, o, prof_thr);
}

int nrv_merge_calls_trim(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                         const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                         const float* trim_thr, int Q, int W, int64_t min_len, int64_t* trim,
                         const uint8_t* names, const int64_t* name_off, uint8_t* blob, int64_t* rec_off) {
  if (h && (!trim_thr || (n_reads > 0 && !trim))) { h->err = "nrv_merge_calls_trim: null trim_thr / trim"; return NRV_E_INVALID; }
  if (h && (!p1 || !p2) && n_win > 0) { h->err = "nrv_merge_calls_trim: null p1 / p2"; return NRV_E_INVALID; }
  if (h && !trim_rule_ok(Q, W, min_len)) { h->err = "nrv_merge_calls_trim: Q must be in 1 .. 40, W in 1 .. 64 and min_len >= 0"; return NRV_E_INVALID; }
  if (h && !rec_off && (names || name_off || blob)) { h->err = "nrv_merge_calls_trim: names / name_off / blob without rec_off"; return NRV_E_INVALID; }
  static int64_t none[2];
  MergeOut o{seq, qual, off};
  o.blob = blob; o.rec_off = rec_off;
  o.trim = trim ? trim : none;
  MergeIn more;
  more.names = names; more.name_off = name_off;
  more.trim_thr = trim_thr; more.Q = Q; more.W = W; more.min_len = min_len;
  return merge_calls_impl(h, bases, ev_len, n_reads, a1, a2, p1, p2, n_win, q_thr, o, nullptr, more);
}

int nrv_merge_calls_accuracy(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                             const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                             const uint8_t* truth, const int64_t* truth_off, uint64_t* accuracy) {
  if (h && (!truth_off || (n_reads > 0 && !accuracy))) { h->err = "nrv_merge_calls_accuracy: null truth_off / accuracy"; return NRV_E_INVALID; }
  static uint64_t none[NRV_ACCURACY_COLS];
  MergeOut o{seq, qual, off};
  o.accuracy = accuracy ? accuracy : none;
  MergeIn more;
  more.truth = truth; more.truth_off = truth_off;
  return merge_calls_impl(h, bases, ev_len, n_reads, a1, a2, p1, p2, n_win, q_thr, o, nullptr, more);
}

int nrv_merge_calls_errclass(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                             const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                             const uint8_t* truth, const int64_t* truth_off, uint64_t* errclass) {
  if (h && (!truth_off || (n_reads > 0 && !errclass))) { h->err = "nrv_merge_calls_errclass: null truth_off / errclass"; return NRV_E_INVALID; }
  static uint64_t none[NRV_ERRCLASS_COLS];
  MergeOut o{seq, qual, off};
  o.errclass = errclass ? errclass : none;
  MergeIn more;
  more.truth = truth; more.truth_off = truth_off;
  return merge_calls_impl(h, bases, ev_len, n_reads, a1, a2, p1, p2, n_win, q_thr, o, nullptr, more);
}

int nrv_merge_calls_infix(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                          const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                          const uint8_t* truth, const int64_t* truth_off, int strands, uint64_t* infix) {
  if (h && (!truth_off || (n_reads > 0 && !infix))) { h->err = "nrv_merge_calls_infix: null truth_off / infix"; return NRV_E_INVALID; }
  static uint64_t none[NRV_INFIX_COLS];
  MergeOut o{seq, qual, off};
  o.infix = infix ? infix : none; o.strands = strands;
  MergeIn more;
  more.truth = truth; more.truth_off = truth_off;
  return merge_calls_impl(h, bases, ev_len, n_reads, a1, a2, p1, p2, n_win, q_thr, o, nullptr, more);
}

int nrv_merge_calls_score(nrv_handle* h, const uint8_t* bases, const int64_t* ev_len, int n_reads, const int8_t* a1, const int8_t* a2,
                          const float* p1, const float* p2, int64_t n_win, const float* q_thr, uint8_t* seq, uint8_t* qual, int64_t* off,
                          const uint8_t* labels, const float* score_thr, uint64_t* score) {
  if (h && (!labels || !score_thr || (n_reads > 0 && !score))) { h->err = "nrv_merge_calls_score: null labels / score_thr / score"; return NRV_E_INVALID; }
  static uint64_t none[NRV_SCORE_COLS];
  MergeOut o{seq, qual, off};
  o.score = score ? score : none;
  MergeIn more;
  more.labels = labels; more.score_thr = score_thr;
  return merge_calls_impl(h, bases, ev_len, n_reads, a1, a2, p1, p2, n_win, q_thr, o, nullptr, more);
}

int nrv_edit_distance(nrv_handle* h, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off, int n_pairs,
                      int64_t* dist) {
  const PairDoor w{"nrv_edit_distance: bad arguments", nullptr,
                   "nrv_edit_distance: null sequences / offsets, offsets that do not ascend from 0, or a sequence of 2^31 - 64 characters and more",
                   nullptr, 1, 1, {dist}};
  return pair_door(h, a, a_off, b, b_off, n_pairs, w, [&](const PairArgs& p, char* hc, long long* const* out) {
    AlignArgs k;
    static_cast<PairArgs&>(k) = p;
    k.hc0 = nullptr; k.hc1 = (unsigned char*)hc;
    k.accu = nullptr; k.dist = out[0];
    return align_enqueue(h, k);
  });
}

int nrv_edit_classes(nrv_handle* h, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off, int n_pairs,
                     int64_t* dist, int64_t* match) {
  const PairDoor w{"nrv_edit_classes: bad arguments", nullptr,
                   "nrv_edit_classes: null sequences / offsets, offsets that do not ascend from 0, or a sequence of 2^31 - 64 characters and more",
                   nullptr, 8, 2, {dist, match}};
  return pair_door(h, a, a_off, b, b_off, n_pairs, w, [&](const PairArgs& p, char* hc, long long* const* out) {
    ErrclassArgs k;
    static_cast<PairArgs&>(k) = p;
    k.hc0 = nullptr; k.hc1 = (long long*)hc;
    k.ecls = nullptr; k.dist = out[0]; k.match = out[1];
    return errclass_enqueue(h, k);
  });
}

int nrv_infix_classes(nrv_handle* h, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off, int n_pairs,
                      int reverse, int64_t* dist, int64_t* match, int64_t* start, int64_t* end) {
  const PairDoor w{"nrv_infix_classes: bad arguments", (reverse != 0 && reverse != 1) ? "nrv_infix_classes: reverse must be 0 or 1" : nullptr,
                   "nrv_infix_classes: null sequences / offsets, or offsets that do not ascend from 0",
                   "nrv_infix_classes: a truth region, or a read that has one, above NRV_INFIX_MAX_LEN = 2^21 - 1 characters",
                   8, 4, {dist, match, start, end}};
  return pair_door(h, a, a_off, b, b_off, n_pairs, w, [&](const PairArgs& p, char* hc, long long* const* out) {
    InfixArgs k;
    static_cast<PairArgs&>(k) = p;
    k.strands = 1; k.reverse = reverse;
    k.hc0 = nullptr; k.hs0 = 0; k.hc1 = (long long*)hc; k.hs1 = 0;          // one strand per call: one set of carry words
    k.infx = nullptr; k.dist = out[0]; k.match = out[1]; k.start = out[2]; k.end = out[3];
    return infix_enqueue(h, k);
  });
}

// labels_kernel + labels_walk_kernel (nrv_labels.h) on the pairs of one batch, the walk behind the forward pass on the labels' stream
static int labels_enqueue(nrv_handle* h, const LabelsArgs& a) {
  if (a.n_pairs <= 0) return NRV_OK;
  hipLaunchKernelGGL(labels_kernel, dim3((unsigned)a.n_pairs), dim3(64), 0, h->lab_stream, a);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(labels_walk_kernel, dim3(((unsigned)a.n_pairs + 63u) / 64u), dim3(64), 0, h->lab_stream, a);
  HIPCHK(h, hipGetLastError());
  return NRV_OK;
}

int nrv_align_labels(nrv_handle* h, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off, int n_pairs,
                     const uint8_t* reverse, const int64_t* start, const int64_t* end, uint8_t* labels, int64_t* summary) {
  static_assert(NRV_LABEL_COLS == kLabelCols && NRV_LABELS_MAX_LEN == kLabelsMaxLen, "nanorev.h and nrv_labels.h disagree on the labels");
  int rc = check_handle(h);
  if (rc) return rc;
  if (n_pairs < 0 || (n_pairs > 0 && (!reverse || !start || !end || !summary))) { h->err = "nrv_align_labels: bad arguments"; return NRV_E_INVALID; }
  if (!truth_ok(a, a_off, n_pairs) || !truth_ok(b, b_off, n_pairs) || (b_off[n_pairs] > 0 && !labels)) {
    h->err = "nrv_align_labels: null sequences / offsets / labels, or offsets that do not ascend from 0";
    return NRV_E_INVALID;
  }
  for (int r = 0; r < n_pairs; ++r) {
    if (reverse[r] > 1) { h->err = "nrv_align_labels: reverse must be 0 or 1"; return NRV_E_INVALID; }
    if (start[r] < 0 || end[r] < start[r] || end[r] > a_off[r + 1] - a_off[r]) {
      h->err = "nrv_align_labels: bounds outside the region (0 <= start <= end <= its length)";
      return NRV_E_INVALID;
    }
    if (b_off[r + 1] - b_off[r] > kLabelsMaxLen || end[r] - start[r] > kLabelsMaxLen) {
      h->err = "nrv_align_labels: a read, or an end - start, above NRV_LABELS_MAX_LEN = 65536 characters";
      return NRV_E_INVALID;
    }
  }
  if (n_pairs == 0) return NRV_OK;
  const int64_t ta = a_off[n_pairs], tb = b_off[n_pairs];
  // consecutive batches whose direction words fit the budget (a pair alone if need be); dir_off: a pair's words inside its batch's
  std::vector<int64_t> dir_off((size_t)n_pairs);
  std::vector<int> batch_end;
  size_t words = 0, max_words = 0;
  for (int r = 0; r < n_pairs; ++r) {
    const int64_t L = end[r] - start[r], n = b_off[r + 1] - b_off[r];
    const size_t w = (a_off[r + 1] > a_off[r] && L > 0 && n > 0) ? (size_t)((L + kLabelsStripe - 1) / kLabelsStripe) * (size_t)(n + 63) * 64 : 0;
    if (words > 0 && (words + w) * 4 > h->lab_budget) { batch_end.push_back(r); words = 0; }
    dir_off[(size_t)r] = (int64_t)words;
    words += w;
    max_words = std::max(max_words, words);
  }
  batch_end.push_back(n_pairs);
  // the handle's block: [a_off | b_off | start | end | dir_off | reverse | a | b | hc | labels | summary | direction words]
  const size_t nb = ((size_t)n_pairs + 1) * 8, np8 = (size_t)n_pairs * 8;
  const LabelsLayout l = labels_layout((size_t)n_pairs, (size_t)ta, (size_t)tb, kLabelCols, max_words);
  const size_t bytes = l.bytes;
  if (!h->lab_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->lab_stream, hipStreamNonBlocking));
  if (bytes > h->cap_lab) {                                // grown on demand; the old block is retired (no hipFree on this path)
    const size_t want = std::max(bytes, h->cap_lab + h->cap_lab / 2);
    char* p = nullptr;
    HIPCHK(h, hipMalloc((void**)&p, want));
    if (h->d_lab) h->lab_retired.push_back(h->d_lab);
    h->d_lab = p; h->cap_lab = want;
  }
  char* const d = h->d_lab;
  hipStream_t const s = h->lab_stream;
  auto run = [&]() -> int {
    int rc2 = poison_fill(h, d, bytes, s);                // NRV_POISON: the part this call uses
    if (rc2 || (rc2 = put(h, d + l.a_off, a_off, nb, s)) || (rc2 = put(h, d + l.b_off, b_off, nb, s)) ||
        (rc2 = put(h, d + l.start, start, np8, s)) || (rc2 = put(h, d + l.end, end, np8, s)) ||
        (rc2 = put(h, d + l.dir_off, dir_off.data(), np8, s)) || (rc2 = put(h, d + l.reverse, reverse, (size_t)n_pairs, s)) ||
        (rc2 = put(h, d + l.a, a, (size_t)ta, s)) || (rc2 = put(h, d + l.b, b, (size_t)tb, s)))
      return rc2;
    LabelsArgs k;
    k.truth = (const unsigned char*)(d + l.a); k.truth_off = (const long long*)(d + l.a_off);
    k.seq = (const unsigned char*)(d + l.b); k.off = (const long long*)(d + l.b_off);
    k.reverse = (const unsigned char*)(d + l.reverse); k.start = (const long long*)(d + l.start); k.end = (const long long*)(d + l.end);
    k.hc = (long long*)(d + l.hc); k.dirw = (unsigned*)(d + l.dir); k.dir_off = (const long long*)(d + l.dir_off);
    k.labels = (unsigned char*)(d + l.labels); k.summary = (long long*)(d + l.summary);
    int p0 = 0;
    for (int p1 : batch_end) {                            // in stream order: a batch's walk ends before the next forward pass stores
      k.pair0 = p0; k.n_pairs = p1 - p0;
      if ((rc2 = labels_enqueue(h, k))) return rc2;
      p0 = p1;
    }
    if (tb > 0) HIPCHK(h, hipMemcpyAsync(labels, d + l.labels, (size_t)tb, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(summary, d + l.summary, (size_t)n_pairs * kLabelCols * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return NRV_OK;
  };
  rc = run();
  if (rc) (void)hipStreamSynchronize(s);
  return rc;
}

int nrv_trim_reads(nrv_handle* h, const uint8_t* qual, const int64_t* off, int n_reads, int Q, int W, int64_t* trim) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (n_reads < 0 || !off || off[0] != 0 || (n_reads > 0 && !trim)) { h->err = "nrv_trim_reads: bad arguments"; return NRV_E_INVALID; }
  if (!trim_rule_ok(Q, W, 0)) { h->err = "nrv_trim_reads: Q must be in 1 .. 40 and W in 1 .. 64"; return NRV_E_INVALID; }
  for (int r = 0; r < n_reads; ++r) if (off[r + 1] < off[r]) { h->err = "nrv_trim_reads: off does not ascend"; return NRV_E_INVALID; }
  if (n_reads == 0) return NRV_OK;
  const int64_t total = off[n_reads];
  if (total > 0 && !qual) { h->err = "nrv_trim_reads: null qual"; return NRV_E_INVALID; }
  const TrimLayout l = trim_layout((size_t)n_reads, (size_t)total);
  hipStream_t const s = h->stream;
  return with_block(h, l.bytes, s, [&](char* d) -> int {
    int rc2;
    if ((rc2 = put(h, d + l.off, off, ((size_t)n_reads + 1) * 8, s)) || (rc2 = put(h, d + l.qual, qual, (size_t)total, s))) return rc2;
    TrimArgs a;
    a.n_reads = n_reads; a.Q = Q; a.W = W; a.bias = 33;
    a.off = (const long long*)(d + l.off); a.q = (const unsigned char*)(d + l.qual); a.cap = total;
    a.acc = (unsigned long long*)(d + l.acc); a.trim = (long long*)(d + l.trim);
    if ((rc2 = trim_bounds_enqueue(h, a))) return rc2;
    HIPCHK(h, hipMemcpyAsync(trim, d + l.trim, (size_t)n_reads * 16, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return NRV_OK;
  });
}

int nrv_pack_records(nrv_handle* h, const uint8_t* seq, const uint8_t* qual, const int64_t* off, int n_reads,
                     const uint8_t* names, const int64_t* name_off, uint8_t* blob, int64_t* rec_off) {
  return nrv_pack_records_trim(h, seq, qual, off, n_reads, names, name_off, nullptr, 0, blob, rec_off);
}

int nrv_pack_records_trim(nrv_handle* h, const uint8_t* seq, const uint8_t* qual, const int64_t* off, int n_reads,
                          const uint8_t* names, const int64_t* name_off, const int64_t* trim, int64_t min_len,
                          uint8_t* blob, int64_t* rec_off) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (n_reads < 0 || !off || !rec_off || off[0] != 0) { h->err = "nrv_pack_records: bad arguments"; return NRV_E_INVALID; }
  for (int r = 0; r < n_reads; ++r) if (off[r + 1] < off[r]) { h->err = "nrv_pack_records: off does not ascend"; return NRV_E_INVALID; }
  if (trim) {
    if (min_len < 0) { h->err = "nrv_pack_records_trim: negative min_len"; return NRV_E_INVALID; }
    for (int r = 0; r < n_reads; ++r)
      if (trim[2 * r] < 0 || trim[2 * r + 1] < trim[2 * r] || trim[2 * r + 1] > off[r + 1] - off[r]) {
        h->err = "nrv_pack_records_trim: a trim outside its read";
        return NRV_E_INVALID;
      }
  }
  if (!names_ok(names, name_off, n_reads)) { h->err = "nrv_pack_records: null names / name_off, or offsets that do not ascend from 0"; return NRV_E_INVALID; }
  const int64_t total_in = off[n_reads], name_bytes = name_off[n_reads];
  const bool fastq = qual != nullptr;
  const size_t cap = blob_capacity(total_in, 0, n_reads, name_bytes, fastq);
  if ((total_in > 0 && !seq) || (cap > 0 && !blob)) { h->err = "nrv_pack_records: null seq / blob"; return NRV_E_INVALID; }
  if (cap >= ((size_t)1 << 32)) { h->err = "nrv_pack_records: records of 4 GiB and more in one call"; return NRV_E_INVALID; }
  if (n_reads == 0) { rec_off[0] = 0; return NRV_OK; }
  const size_t nb = ((size_t)n_reads + 1) * 8;
  const RecordLayout l = record_layout((size_t)n_reads, (size_t)name_bytes, (size_t)total_in, fastq, cap, trim != nullptr);
  hipStream_t const s = h->stream;
  return with_block(h, l.bytes, s, [&](char* d) -> int {
    int rc2;
    if ((rc2 = put(h, d + l.off, off, nb, s)) || (rc2 = put(h, d + l.name_off, name_off, nb, s)) ||
        (rc2 = put(h, d + l.names, names, (size_t)name_bytes, s)) || (rc2 = put(h, d + l.seq, seq, (size_t)total_in, s)) ||
        (rc2 = put(h, d + l.qual, qual, fastq ? (size_t)total_in : 0, s)) || (rc2 = put(h, d + l.trim, trim, trim ? (size_t)n_reads * 16 : 0, s)))
      return rc2;
    PackArgs a;
    a.n_reads = n_reads; a.fastq = fastq ? 1 : 0;
    a.off = (const long long*)(d + l.off); a.name_off = (const long long*)(d + l.name_off); a.names = (const unsigned char*)(d + l.names);
    a.seq = (const unsigned char*)(d + l.seq); a.qual = (const unsigned char*)(d + l.qual);
    a.rec_off = (long long*)(d + l.rec_off); a.blob = (unsigned char*)(d + l.blob); a.cap = cap;
    a.trim = trim ? (const long long*)(d + l.trim) : nullptr; a.min_len = min_len;
    if ((rc2 = pack_enqueue(h, a))) return rc2;
    HIPCHK(h, hipMemcpyAsync(rec_off, d + l.rec_off, nb, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    const int64_t n_b = rec_off[n_reads];                       // the used prefix of the blob, once the total is known
    if (n_b < 0 || (uint64_t)n_b > cap) { h->err = "nrv_pack_records: records out of range"; return NRV_E_HIP; }
    if (n_b > 0) HIPCHK(h, hipMemcpy(blob, d + l.blob, (size_t)n_b, hipMemcpyDeviceToHost));
    return NRV_OK;
  });
}

// ---- nrv_fit_*: the per-window tail fitted on the device (csrc/nrv_tailfit.h; nanoreviser_amd/tailfit.py is the definition) ----
// every nrv_fit_* call: a usable handle and no raw-read call in flight (they share the stream, the activation set and d_sig)
static int fit_enter(nrv_handle* h, const char* who) {
  const int rc = check_handle(h);
  if (rc) return rc;
  if (h->raw_slot[0].busy || h->raw_slot[1].busy) {
    h->err = std::string(who) + ": a raw-read call is in flight (collect it with nrv_reads_raw_end first)";
    return NRV_E_INVALID;
  }
  return NRV_OK;
}
static int fit_refuse(nrv_handle* h, const char* who, const std::string& what) {
  h->err = std::string(who) + ": " + what;
  return NRV_E_INVALID;
}
// a scratch buffer of at least `bytes`, contents not kept
static int fit_scratch(nrv_handle* h, void** p, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return NRV_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  (void)hipFree(*p);
  *p = nullptr; *cap = 0;
  const size_t c = bytes + bytes / 2 + 4096;
  HIPCHK(h, hipMalloc(p, c));
  *cap = c;
  return poison_fill(h, *p, c, h->stream);
}
// the parameters of a model's vector at the handle's depth, and the depth's row cap with the words a refusal names it by
static int fit_bn_block(const nrv_handle* h) { return h->fit.bn_affine ? NRV_FIT_PARAMS_BN(h->fit.depth) : 0; }   // the gamma / beta block in front
static int fit_params_n(const nrv_handle* h, int model) { return fit_bn_block(h) + fit_at(h).params(h->T, h->dm[model].C); }
static int64_t fit_cap_rows(const nrv_handle* h) { return h->fit.max_rows[&fit_at(h) - kFitDepths]; }
static std::string fit_cap_words(const nrv_handle* h) { return std::string(fit_at(h).at) + " (" + fit_at(h).env + ")"; }
// the arrays of the set at the handle's depth - where the handle keeps each and its bytes per row - in door order: the depth's
// row arrays, then y of model 0 and of model 1 -> their number
struct FitArr { void** p; size_t row; };
static int fit_arrays(nrv_handle* h, FitArr (&a)[6]) {
  nrv_handle::Fit& F = h->fit;
  const FitDepth& D = fit_at(h);
  int n = 0, s = 0;
  for (int i = 0; i < D.n_arrays; ++i) {
    const size_t row = (size_t)h->T * D.arrays[i].per_t * 4;
    if (D.arrays[i].shared) a[n++] = FitArr{(void**)&F.shared[s++], row};
    else for (int m = 0; m < 2; ++m) a[n++] = FitArr{(void**)&F.x[m], row};
  }
  for (int m = 0; m < 2; ++m) a[n++] = FitArr{(void**)&F.y[m], 1};
  return n;
}
// room for `need` rows in the set, the rows it holds kept
static int fit_reserve(nrv_handle* h, int64_t need) {
  nrv_handle::Fit& F = h->fit;
  if (need <= F.cap) return NRV_OK;
  int64_t c = F.cap * 2 > need ? F.cap * 2 : need;
  if (c < 1024) c = 1024;
  const int64_t cmax = fit_cap_rows(h);
  if (c > cmax) c = cmax;
  FitArr a[6];
  const int n = fit_arrays(h, a);
  void* grown[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int rc = NRV_OK;
  for (int i = 0; i < n && !rc; ++i) {
    const size_t bytes = ((size_t)c * a[i].row + 3) / 4 * 4;
    if (hipMalloc(&grown[i], bytes) != hipSuccess) {
      h->err = "nrv_fit: out of device memory for the training set";
      rc = NRV_E_NOMEM;
    } else if (!(rc = poison_fill(h, grown[i], bytes, h->stream)) && F.rows > 0 &&
               hipMemcpyAsync(grown[i], *a[i].p, (size_t)F.rows * a[i].row, hipMemcpyDeviceToDevice, h->stream) != hipSuccess) {
      h->err = "nrv_fit: copying the training set failed";
      rc = NRV_E_HIP;
    }
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess && !rc) { h->err = "nrv_fit: growing the training set failed"; rc = NRV_E_HIP; }
  for (int i = 0; i < n; ++i) {                            // all of the new arrays, or none
    if (rc) { (void)hipFree(grown[i]); continue; }
    (void)hipFree(*a[i].p);
    *a[i].p = grown[i];
  }
  if (!rc) F.cap = c;
  return rc;
}

// Every stage of the call onto the compute stream as raw_enqueue does it, on the kernels the handle's mode selects (the caller
// has selected the f32 ones), and behind each launch group the gather of its labelled windows out of h->MO
static int fit_enqueue(nrv_handle* h, const char* d_in, size_t off_starts, size_t off_reads, size_t off_feat, const int* d_slot,
                       int n_reads, int64_t n) {
  const int T = h->T;
  const FitDepth& D = fit_at(h);                           // which gather fills the set: the deepest stage inside the fitted section
  const int stage = stage_windows(h, true);
  const float* d_feat = (const float*)(d_in + off_feat);
  for (int64_t s = 0; s < n; s += stage) {
    const int nb = (int)((n - s < stage) ? (n - s) : stage);
    const int rc0 = poison_fill(h, h->d_sig[0], h->sig_bytes, h->stream);
    if (rc0) return rc0;
    launch_segment(h, n_reads, s, nb + T - 1, h->d_sig[0], (const int16_t*)d_in, (const int32_t*)(d_in + off_starts),
                   (const SegRead*)(d_in + off_reads));
    if (D.rd) {                                            // the set is the stage's raw inputs: no launch group runs for it
      const FullGatherArgs g{h->d_sig[0], d_feat + s * kFeat, h->fit.shared[0], h->fit.shared[1], d_slot + s, nb, T, (long long)h->fit.cap};
      const long long total = (long long)nb * T * 28;
      hipLaunchKernelGGL(full_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, g);
      HIPCHK(h, hipGetLastError());
      continue;
    }
    const int rc = for_groups(h, nb, [&](int64_t w, int nw) -> int {
      if (D.l3) {                                          // lstm3's or the signal branch's inputs: the gather runs INSIDE the group, between lstm2 and lstm4
        h->fit.l3_slot = d_slot + s + w;
        const int rc3 = run_group(h, h->d_sig[0] + w * kSig, d_feat + (s + w) * kFeat, nw, true, h->d_p[0][0] + w * 6, h->d_p[0][1] + w * 5,
                                  h->d_a[0][0] + w, h->d_a[0][1] + w, h->d_sat + 3);
        h->fit.l3_slot = nullptr;
        return rc3;
      }
      const int rc1 = run_group(h, h->d_sig[0] + w * kSig, d_feat + (s + w) * kFeat, nw, true, h->d_p[0][0] + w * 6, h->d_p[0][1] + w * 5,
                                h->d_a[0][0] + w, h->d_a[0][1] + w, h->d_sat + 3);
      if (rc1) return rc1;
      if (D.l4) {                                          // lstm4's f32 input (lstm3's output behind its BatchNorm), still in X3
        L4GatherArgs g;
        for (int m = 0; m < 2; ++m) { g.in[m] = h->X3[m]; g.x[m] = h->fit.x[m]; }
        g.slot = d_slot + s + w; g.n = nw; g.T = T; g.cap = h->fit.cap;
        const long long total = (long long)nw * T * 64;
        hipLaunchKernelGGL(l4_gather_kernel, dim3((unsigned)((total + 255) / 256), 2), dim3(256), 0, h->stream, g);
        HIPCHK(h, hipGetLastError());
        return (int)NRV_OK;
      }
      if (D.mlp) {                                         // the head's f32 input (lstm4's output) of the group, still in X2
        HeadGatherArgs g;
        for (int m = 0; m < 2; ++m) { g.in[m] = h->X2[m]; g.x[m] = h->fit.x[m]; }
        g.slot = d_slot + s + w; g.n = nw; g.T = T; g.cap = h->fit.cap;
        const long long total = (long long)nw * T * 32;
        hipLaunchKernelGGL(head_gather_kernel, dim3((unsigned)((total + 255) / 256), 2), dim3(256), 0, h->stream, g);
        HIPCHK(h, hipGetLastError());
        return (int)NRV_OK;
      }
      TailGatherArgs g;
      for (int m = 0; m < 2; ++m) { g.mo[m] = h->MO[m]; g.flat[m] = h->fit.x[m]; }
      g.slot = d_slot + s + w; g.n = nw; g.T = T; g.cap = h->fit.cap;
      const long long total = (long long)nw * 6 * T;
      hipLaunchKernelGGL(tail_gather_kernel, dim3((unsigned)((total + 255) / 256), 2), dim3(256), 0, h->stream, g);
      HIPCHK(h, hipGetLastError());
      return (int)NRV_OK;
    });
    if (rc) return rc;
  }
  return NRV_OK;
}

int nrv_fit_reset(nrv_handle* h) {
  const int rc = fit_enter(h, "nrv_fit_reset");
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->fit.rows = 0;
  return NRV_OK;
}

int64_t nrv_fit_count(nrv_handle* h) {
  const int rc = fit_enter(h, "nrv_fit_count");
  return rc ? (int64_t)rc : h->fit.rows;
}

int nrv_fit_add_reads_raw(nrv_handle* h, const int16_t* raw, int64_t n_raw, const int32_t* starts, const float* feat_ev, int64_t N,
                          const nrv_read_desc* reads, int n_reads, const int32_t* last_dur, const uint8_t* on_device,
                          const uint8_t* labels, int64_t* n_added) {
  static const char* who = "nrv_fit_add_reads_raw";
  int rc = fit_enter(h, who);
  if (rc) return rc;
  if (!n_added || (N > 0 && !labels)) return fit_refuse(h, who, "null labels / n_added");
  if ((last_dur == nullptr) != (on_device == nullptr)) return fit_refuse(h, who, "last_dur and on_device go together");
  if ((rc = raw_check(h, raw, n_raw, starts, feat_ev, N, reads, n_reads))) { h->err = std::string(who) + ": " + h->err; return rc; }
  if (N >= ((int64_t)1 << 31)) return fit_refuse(h, who, "2^31 events and more in one call");
  const bool with_stats = last_dur != nullptr;
  const int64_t stat_len = with_stats ? stats_check(h, reads, n_reads, last_dur, on_device) : 0;
  if (stat_len < 0) { h->err = std::string(who) + ": " + h->err; return NRV_E_INVALID; }
  const int T = h->T;
  const int64_t n = N - T > 0 ? N - T : 0;
  *n_added = 0;
  if (n == 0) return NRV_OK;
  // the rows this call adds, by the rule of the device's scan: the set is sized, and the cap checked, before anything runs
  int64_t add = 0;
  const int64_t o = (T - 1) / 2;
  for (int r = 0; r < n_reads; ++r) {
    const int64_t n_r = reads[r].ev_len - T > 0 ? reads[r].ev_len - T : 0;
    const uint8_t* lb = labels + reads[r].ev_off + o;
    for (int64_t i = 0; i < n_r; ++i) add += lb[i] != 0xFF && (lb[i] & 7) >= 1 && (lb[i] & 7) <= 5;
  }
  nrv_handle::Fit& F = h->fit;
  if (F.rows + add > fit_cap_rows(h)) return fit_refuse(h, who, "the call would pass the row cap of the training set" + fit_cap_words(h));
  if (add == 0) return NRV_OK;
  if ((rc = fit_reserve(h, F.rows + add)) || (rc = ensure_workspace(h))) return rc;
  const int tiles = (int)((N + kMergeTile - 1) / kMergeTile);
  const size_t off_starts = up256((size_t)n_raw * 2), off_reads = off_starts + up256((size_t)N * 4);
  const size_t off_feat = off_reads + up256((size_t)n_reads * sizeof(SegRead)), off_aux = off_feat + up256((size_t)N * kFeat * 4);
  const size_t off_labels = off_aux + (with_stats ? up256((size_t)n_reads * sizeof(StatAux)) : 0);
  const size_t off_slot = off_labels + up256((size_t)N), off_tile = off_slot + up256((size_t)n * 4);
  const size_t off_stat = off_tile + up256(((size_t)tiles + 1) * 8);
  const size_t bytes = off_stat + (stat_len > 0 ? up256((size_t)n_reads * kStatWords * 4) : 0);
  std::vector<StatAux> aux;
  if (with_stats) for (int r = 0; r < n_reads; ++r) aux.push_back(StatAux{last_dur[r], on_device[r] ? 1 : 0});
  const int h2 = h->h2, split = h->split;
  rc = with_block(h, bytes, h->stream, [&](char* d) -> int {
    int rc2;
    if ((rc2 = put(h, d, raw, (size_t)n_raw * 2, h->stream)) || (rc2 = put(h, d + off_starts, starts, (size_t)N * 4, h->stream)) ||
        (rc2 = put(h, d + off_reads, reads, (size_t)n_reads * sizeof(SegRead), h->stream)) ||
        (rc2 = put(h, d + off_feat, feat_ev, (size_t)N * kFeat * 4, h->stream)) ||
        (rc2 = put(h, d + off_aux, aux.data(), aux.size() * sizeof(StatAux), h->stream)) ||
        (rc2 = put(h, d + off_labels, labels, (size_t)N, h->stream)))
      return rc2;
    HIPCHK(h, hipMemsetAsync(d + off_slot, 0xFF, (size_t)n * 4, h->stream));
    if (stat_len > 0 &&
        (rc2 = stats_enqueue(h, (const int16_t*)d, (const int32_t*)(d + off_starts), (SegRead*)(d + off_reads), (const StatAux*)(d + off_aux),
                             (unsigned*)(d + off_stat), n_reads, N, stat_len, (float*)(d + off_feat), nullptr, nullptr)))
      return rc2;
    const FitLabelArgs la{(const SegRead*)(d + off_reads), n_reads, T, (long long)N, (const unsigned char*)(d + off_labels),
                          (unsigned long long*)(d + off_tile), (int*)(d + off_slot), (long long)F.rows, (long long)F.cap, F.y[0], F.y[1]};
    hipLaunchKernelGGL(fit_label_count_kernel, dim3((unsigned)tiles), dim3(256), 0, h->stream, la);
    hipLaunchKernelGGL(fit_tile_scan_kernel, dim3(1), dim3(256), 0, h->stream, la, tiles);
    hipLaunchKernelGGL(fit_label_scatter_kernel, dim3((unsigned)tiles), dim3(256), 0, h->stream, la);
    HIPCHK(h, hipGetLastError());
    h->h2 = 0; h->split = 0;                               // the f32 kernels, as the range guard's re-run selects them
    rc2 = fit_enqueue(h, d, off_starts, off_reads, off_feat, (const int*)(d + off_slot), n_reads, n);
    h->h2 = h2; h->split = split;
    if (rc2) return rc2;
    unsigned long long total = 0;
    HIPCHK(h, hipMemcpyAsync(&total, d + off_tile + (size_t)tiles * 8, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if ((int64_t)total != add) { h->err = std::string(who) + ": the device counted other labelled windows than the host"; return NRV_E_HIP; }
    return NRV_OK;
  });
  if (rc) return rc;
  F.rows += add;
  *n_added = add;
  return NRV_OK;
}

// The row doors.  A door belongs to one depth; at another the refusal names the set's depth and its own doors - or, from a set
// door at the depth a handle starts at, the nrv_fit_set_depth call that was left out
static int fit_door_depth(nrv_handle* h, const char* who, int door_depth, bool set) {
  const FitDepth &at = fit_at(h), &door = *fit_desc(door_depth);
  if (&at == &door) return NRV_OK;
  const std::string where = std::string("the set is at ") + at.name + " depth (";
  if (set && &at == kFitDepths) return fit_refuse(h, who, where + "call nrv_fit_set_depth(" + door.code_name + ") on an empty set first)");
  return fit_refuse(h, who, where + "rows are " + at.phrase + ": nrv_fit_" + (set ? "set" : "get") + "_rows" + at.suffix + ")");
}
// nrv_fit_set_rows*: `arrays` are the depth's row arrays in door order
static int fit_rows_put(nrv_handle* h, const char* who, int door_depth, const float* const* arrays, const uint8_t* y1, const uint8_t* y2,
                        int64_t n) {
  int rc = fit_enter(h, who);
  if (rc || (rc = fit_door_depth(h, who, door_depth, true))) return rc;
  FitArr a[6];
  const int na = fit_arrays(h, a);
  const void* src[6];
  for (int i = 0; i < na - 2; ++i) src[i] = arrays[i];
  src[na - 2] = y1; src[na - 1] = y2;
  bool all = true;
  for (int i = 0; i < na; ++i) all = all && src[i];
  if (n < 0 || (n > 0 && !all)) return fit_refuse(h, who, "null rows (or a negative count)");
  if (n > fit_cap_rows(h)) return fit_refuse(h, who, "more rows than the cap of the training set" + fit_cap_words(h));
  for (int64_t i = 0; i < n; ++i)
    if (y1[i] > 5 || y2[i] > 4) return fit_refuse(h, who, "a label outside the model's classes (y1 0 .. 5, y2 0 .. 4)");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->fit.rows = 0;
  if (n == 0) return NRV_OK;
  if ((rc = fit_reserve(h, n))) return rc;
  for (int i = 0; i < na; ++i)
    if ((rc = put(h, *a[i].p, src[i], (size_t)n * a[i].row, h->stream))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->fit.rows = n;
  return NRV_OK;
}
// nrv_fit_get_rows*: any output may be null
static int fit_rows_get(nrv_handle* h, const char* who, int door_depth, int64_t first, int64_t count, float* const* arrays, uint8_t* y1,
                        uint8_t* y2) {
  int rc = fit_enter(h, who);
  if (rc || (rc = fit_door_depth(h, who, door_depth, false))) return rc;
  if (first < 0 || count < 0 || first > h->fit.rows || count > h->fit.rows - first) return fit_refuse(h, who, "rows outside the training set");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (count == 0) return NRV_OK;
  FitArr a[6];
  const int na = fit_arrays(h, a);
  void* dst[6];
  for (int i = 0; i < na - 2; ++i) dst[i] = arrays[i];
  dst[na - 2] = y1; dst[na - 1] = y2;
  for (int i = 0; i < na; ++i)
    if (dst[i]) HIPCHK(h, hipMemcpy(dst[i], (const char*)*a[i].p + (size_t)first * a[i].row, (size_t)count * a[i].row, hipMemcpyDeviceToHost));
  return NRV_OK;
}

int nrv_fit_set_rows(nrv_handle* h, const float* flat1, const float* flat2, const uint8_t* y1, const uint8_t* y2, int64_t n) {
  const float* const arrays[] = {flat1, flat2};
  return fit_rows_put(h, "nrv_fit_set_rows", NRV_FIT_TAIL, arrays, y1, y2, n);
}
int nrv_fit_get_rows(nrv_handle* h, int64_t first, int64_t count, float* flat1, float* flat2, uint8_t* y1, uint8_t* y2) {
  float* const arrays[] = {flat1, flat2};
  return fit_rows_get(h, "nrv_fit_get_rows", NRV_FIT_TAIL, first, count, arrays, y1, y2);
}
int nrv_fit_set_rows_head(nrv_handle* h, const float* x1, const float* x2, const uint8_t* y1, const uint8_t* y2, int64_t n) {
  const float* const arrays[] = {x1, x2};
  return fit_rows_put(h, "nrv_fit_set_rows_head", NRV_FIT_HEAD, arrays, y1, y2, n);
}
int nrv_fit_get_rows_head(nrv_handle* h, int64_t first, int64_t count, float* x1, float* x2, uint8_t* y1, uint8_t* y2) {
  float* const arrays[] = {x1, x2};
  return fit_rows_get(h, "nrv_fit_get_rows_head", NRV_FIT_HEAD, first, count, arrays, y1, y2);
}
int nrv_fit_set_rows_lstm4(nrv_handle* h, const float* xb1, const float* xb2, const uint8_t* y1, const uint8_t* y2, int64_t n) {
  const float* const arrays[] = {xb1, xb2};
  return fit_rows_put(h, "nrv_fit_set_rows_lstm4", NRV_FIT_LSTM4, arrays, y1, y2, n);
}
int nrv_fit_get_rows_lstm4(nrv_handle* h, int64_t first, int64_t count, float* xb1, float* xb2, uint8_t* y1, uint8_t* y2) {
  float* const arrays[] = {xb1, xb2};
  return fit_rows_get(h, "nrv_fit_get_rows_lstm4", NRV_FIT_LSTM4, first, count, arrays, y1, y2);
}
int nrv_fit_set_rows_lstm3(nrv_handle* h, const float* x1, const float* x2, const uint8_t* y1, const uint8_t* y2, int64_t n) {
  const float* const arrays[] = {x1, x2};
  return fit_rows_put(h, "nrv_fit_set_rows_lstm3", NRV_FIT_LSTM3, arrays, y1, y2, n);
}
int nrv_fit_get_rows_lstm3(nrv_handle* h, int64_t first, int64_t count, float* x1, float* x2, uint8_t* y1, uint8_t* y2) {
  float* const arrays[] = {x1, x2};
  return fit_rows_get(h, "nrv_fit_get_rows_lstm3", NRV_FIT_LSTM3, first, count, arrays, y1, y2);
}
int nrv_fit_set_rows_signal(nrv_handle* h, const float* x2_1, const float* x2_2, const float* sig, const uint8_t* y1, const uint8_t* y2,
                            int64_t n) {
  const float* const arrays[] = {x2_1, x2_2, sig};
  return fit_rows_put(h, "nrv_fit_set_rows_signal", NRV_FIT_SIGNAL, arrays, y1, y2, n);
}
int nrv_fit_get_rows_signal(nrv_handle* h, int64_t first, int64_t count, float* x2_1, float* x2_2, float* sig, uint8_t* y1, uint8_t* y2) {
  float* const arrays[] = {x2_1, x2_2, sig};
  return fit_rows_get(h, "nrv_fit_get_rows_signal", NRV_FIT_SIGNAL, first, count, arrays, y1, y2);
}
int nrv_fit_set_rows_full(nrv_handle* h, const float* sig, const float* feat, const uint8_t* y1, const uint8_t* y2, int64_t n) {
  const float* const arrays[] = {sig, feat};
  return fit_rows_put(h, "nrv_fit_set_rows_full", NRV_FIT_FULL, arrays, y1, y2, n);
}
int nrv_fit_get_rows_full(nrv_handle* h, int64_t first, int64_t count, float* sig, float* feat, uint8_t* y1, uint8_t* y2) {
  float* const arrays[] = {sig, feat};
  return fit_rows_get(h, "nrv_fit_get_rows_full", NRV_FIT_FULL, first, count, arrays, y1, y2);
}

int nrv_fit_depth(nrv_handle* h) {
  const int rc = check_handle(h);
  return rc ? rc : h->fit.depth;
}

// the parameter blocks of both models are those of the other vector length: freed, nrv_fit_begin allocates them again
static void fit_bn_affine_off(nrv_handle* h) {
  for (int m = 0; m < 2; ++m) {
    (void)hipFree(h->fit.m[m].d_par); (void)hipFree(h->fit.m[m].d_state);
    h->fit.m[m].d_par = nullptr; h->fit.m[m].d_state = nullptr;
  }
  h->fit.bn_affine = false;
}

int nrv_fit_set_depth(nrv_handle* h, int depth) {
  static const char* who = "nrv_fit_set_depth";
  const int rc = fit_enter(h, who);
  if (rc) return rc;
  if (!fit_desc(depth))
    return fit_refuse(h, who, "depth must be NRV_FIT_TAIL or NRV_FIT_HEAD, or NRV_FIT_LSTM4, or NRV_FIT_LSTM3, or NRV_FIT_SIGNAL, or NRV_FIT_FULL");
  nrv_handle::Fit& F = h->fit;
  if (F.rows != 0) return fit_refuse(h, who, "the training set is not empty (call nrv_fit_reset first)");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int m = 0; m < 2; ++m) {                            // any nrv_fit_begin is forgotten: its vector has the other length
    F.m[m].begun = false;
    F.m[m].t = 0;
  }
  if (F.bn_affine) fit_bn_affine_off(h);                   // the switch is off at every depth until it is set again
  F.drop_rate = 0.0; F.drop_thr = 0; F.drop_keepf = 1.f;   // and so is the dropout
  F.m[0].draw = F.m[1].draw = 0;
  if (depth == F.depth) return NRV_OK;
  for (int m = 0; m < 2; ++m) {                            // the set and the parameter blocks are the other depth's
    (void)hipFree(F.x[m]); (void)hipFree(F.shared[m]); (void)hipFree(F.y[m]);
    F.x[m] = nullptr; F.shared[m] = nullptr; F.y[m] = nullptr;
    (void)hipFree(F.m[m].d_par); (void)hipFree(F.m[m].d_state);
    F.m[m].d_par = nullptr; F.m[m].d_state = nullptr;
  }
  F.cap = 0;
  F.depth = depth;
  return NRV_OK;
}

// tensors 50 .. 55 of the handle's own model, row-major as the parameter vector has them, to the front of d_par: the device
// holds the three kernels only in pack_dense's fragment order, which is undone here; the biases are there as they are
static int fit_head_own(nrv_handle* h, int model, float* d_par) {
  const DevModel& d = h->dm[model];
  const struct { size_t src; int K, N, at; } ker[3] = {{d.d1p, 128, 128, kHfW1}, {d.d2p, 128, 32, kHfW2}, {d.mop, 32, 6, kHfWm}};
  std::vector<float> own((size_t)kHfMlp), pk;
  for (const auto& k : ker) {
    const int NT = (k.N + 31) / 32, KG = k.K / 8;
    pk.resize((size_t)NT * KG * 256);
    HIPCHK(h, hipMemcpy(pk.data(), d.all + k.src, pk.size() * 4, hipMemcpyDeviceToHost));
    for (int nt = 0; nt < NT; ++nt)
      for (int kg = 0; kg < KG; ++kg)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 4; ++j) {
            const int kk = 8 * kg + 4 * (lane >> 5) + j, col = nt * 32 + (lane & 31);
            if (col < k.N) own[(size_t)k.at + (size_t)kk * k.N + col] = pk[((size_t)nt * KG + kg) * 256 + lane * 4 + j];
          }
  }
  HIPCHK(h, hipMemcpy(own.data() + kHfB1, d.all + d.d1b, 128 * 4, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(own.data() + kHfB2, d.all + d.d2b, 32 * 4, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(own.data() + kHfBm, d.all + d.mob, 6 * 4, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(d_par, own.data(), own.size() * 4, hipMemcpyHostToDevice));
  return NRV_OK;
}

// bn_refold_kernel's arguments: every BatchNorm inside the section, gamma / beta in the vector's block, (s, h) and the
// statistics in the model's block
static BnRefoldArgs fit_refold_args(nrv_handle* h, int model) {
  static const int at_s[5] = {kBnConv + 32, kBnConv + 248, kBnS1, kBnS2, kBnS3}, at_h[5] = {kBnConv + 40, kBnConv + 256, kBnH1, kBnH2, kBnH3};
  const FitDepth& D = fit_at(h);
  BnRefoldArgs a{};
  int at = 0;
  for (int i = 0; i < D.n_bn; ++i) {
    const int w = D.bn[i];
    a.bn[i] = BnRefoldArgs::One{kFitBn[w].C, at, at_s[w], at_h[w], kBnMean + kFitBn[w].at};
    at += 2 * kFitBn[w].C;
  }
  a.par = h->fit.m[model].d_par; a.blk = h->fit.m[model].d_bn; a.var_off = kBnVar - kBnMean;
  return a;
}

int nrv_fit_begin(nrv_handle* h, int model, const float* params, const nrv_fit_opts* opts) {
  static const char* who = "nrv_fit_begin";
  const int rc = fit_enter(h, who);
  if (rc) return rc;
  if (model != 0 && model != 1) return fit_refuse(h, who, "model must be 0 or 1");
  nrv_fit_opts o;
  if (opts) o = *opts;
  else {
    o.B = 512; o.lr = 1e-3f; o.beta1 = 0.9f; o.beta2 = 0.999f; o.eps = 1e-7f; o.lambda = 0.4f;
    static const float cw1[6] = {3.f, 5.f, 1.f, 1.f, 1.f, 1.f}, cw2[6] = {5.f, 1.f, 1.f, 1.f, 1.f, 0.f};
    memcpy(o.cw, model == 0 ? cw1 : cw2, sizeof o.cw);
  }
  if (o.B < 1 || o.B > NRV_FIT_MAX_BATCH) return fit_refuse(h, who, "B outside 1 .. NRV_FIT_MAX_BATCH");
  nrv_handle::Fit::Model& M = h->fit.m[model];
  const DevModel& d = h->dm[model];
  const FitDepth& D = fit_at(h);
  const int C = d.C, K = 6 * h->T, P = fit_params_n(h, model), ob = fit_bn_block(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  M.begun = false;
  if (!M.d_par) {
    HIPCHK(h, hipMalloc((void**)&M.d_par, (size_t)4 * P * 4));
    HIPCHK(h, hipMalloc((void**)&M.d_state, sizeof(HeadState)));      // (the tail's state is its front)
  }
  HIPCHK(h, hipMemsetAsync(M.d_par, 0, (size_t)4 * P * 4, h->stream));
  if (params) HIPCHK(h, hipMemcpyAsync(M.d_par, params, (size_t)P * 4, hipMemcpyHostToDevice, h->stream));
  else {
    float* const par0 = M.d_par + ob;                       // the depth's own vector, behind the gamma / beta block
    if (ob) {                                               // the block: gamma, beta of every BatchNorm inside as the file has them
      std::vector<float> gb;
      for (int i = 0; i < D.n_bn; ++i)
        for (int k = 0; k < 2; ++k) gb.insert(gb.end(), d.bn_raw[k].begin() + kFitBn[D.bn[i]].at, d.bn_raw[k].begin() + kFitBn[D.bn[i]].at + kFitBn[D.bn[i]].C);
      HIPCHK(h, hipMemcpyAsync(M.d_par, gb.data(), (size_t)ob * 4, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));           // (gb is a local)
    }
    const size_t src[4] = {d.fw, d.fb, d.ow, d.ob}, cnt[4] = {(size_t)16 * K, 16, (size_t)16 * C, (size_t)C};
    size_t at = 0;
    float* const sgp = par0 + (D.rd ? kRdN : 0);            // where the signal depth's vector starts
    if (D.rd) {                                             // tensors 12 .. 17 and 22 .. 27, unfolded as the file has them
      HIPCHK(h, hipMemcpyAsync(par0, d.all + d.l1raw, (size_t)kR1N * 4, hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(par0 + kR1N, d.all + d.l2raw, (size_t)kR2N * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    if (D.sg) {                                             // tensors 0, 1 and 6, 7 out of the conv image, 32 and 33 as the file has them
      HIPCHK(h, hipMemcpyAsync(sgp, d.all + d.conv, (size_t)32 * 4, hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(sgp + kSgW2, d.all + d.conv + 48, (size_t)200 * 4, hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(sgp + kSgWs, d.all + d.sdraw, (size_t)400 * 64 * 4, hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(sgp + kSgBs, d.all + d.dbias, (size_t)64 * 4, hipMemcpyDeviceToDevice, h->stream));
      at = (D.rd ? kRdN : 0) + kSgN;
    }
    if (D.l3) {                                             // tensors 34 .. 39, unfolded as the file has them
      HIPCHK(h, hipMemcpyAsync(par0 + at, d.all + d.l3raw, (size_t)kL3N * 4, hipMemcpyDeviceToDevice, h->stream));
      at += kL3N;
    }
    if (D.l4) {                                             // tensors 44 .. 49, unfolded as the file has them
      HIPCHK(h, hipMemcpyAsync(par0 + at, d.all + d.l4raw, (size_t)kL4N * 4, hipMemcpyDeviceToDevice, h->stream));
      at += kL4N;
    }
    if (D.mlp) {
      HIPCHK(h, hipStreamSynchronize(h->stream));
      const int rc2 = fit_head_own(h, model, par0 + at);
      if (rc2) return rc2;
      at += kHfMlp;
    }
    for (int i = 0; i < 4; ++i) {
      HIPCHK(h, hipMemcpyAsync(par0 + at, d.all + src[i], cnt[i] * 4, hipMemcpyDeviceToDevice, h->stream));
      at += cnt[i];
    }
  }
  if (D.l3) {                                               // the fit's own BatchNorm block: the handle's folded pairs, the loaded statistics
    if (!M.d_bn) {
      HIPCHK(h, hipMalloc((void**)&M.d_bn, (size_t)kBnFloats * 4));
      HIPCHK(h, hipMalloc((void**)&M.d_bnacc, (size_t)2 * kBnCh * 8));
    }
    int rcp;
    if ((rcp = poison_fill(h, M.d_bn, (size_t)kBnFloats * 4, h->stream)) || (rcp = poison_fill(h, M.d_bnacc, (size_t)2 * kBnCh * 8, h->stream))) return rcp;
    static const int ats[3] = {kBnS1, kBnS2, kBnS3}, ath[3] = {kBnH1, kBnH2, kBnH3}, nl[3] = {32, 128, 256};
    HIPCHK(h, hipMemcpyAsync(M.d_bn + kBnConv, d.all + d.conv, (size_t)264 * 4, hipMemcpyDeviceToDevice, h->stream));
    for (int l = 0; l < 3; ++l) {
      HIPCHK(h, hipMemcpyAsync(M.d_bn + ats[l], d.all + d.l_s[l], (size_t)nl[l] * 4, hipMemcpyDeviceToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(M.d_bn + ath[l], d.all + d.l_h[l], (size_t)nl[l] * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(M.d_bn + kBnPivot, d.bn_raw[2].data(), (size_t)kBnCh * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(M.d_bn + kBnMean, d.bn_raw[2].data(), (size_t)kBnCh * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(M.d_bn + kBnVar, d.bn_raw[3].data(), (size_t)kBnCh * 4, hipMemcpyHostToDevice, h->stream));
    // with gamma / beta in the vector the pairs are folded from it on the device: from the handle's own they are nrv_create's bytes
    if (ob) hipLaunchKernelGGL(bn_refold_kernel, dim3(D.n_bn), dim3(256), 0, h->stream, fit_refold_args(h, model));
    M.bn_mean = d.bn_raw[2]; M.bn_var = d.bn_raw[3];
    M.bn_s1.assign(kBnCh, 0.0); M.bn_s2.assign(kBnCh, 0.0);
    for (int i = 0; i < 5; ++i) M.bn_n[i] = 0;
  }
  HIPCHK(h, hipMemsetAsync(M.d_state, 0, sizeof(TailState), h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  M.o = o; M.t = 0; M.begun = true;
  M.draw = 0;
  return NRV_OK;
}

// the checks nrv_fit_grad / _epoch / _eval share, and the upload of their row indices
static int fit_rows_in(nrv_handle* h, const char* who, int model, const uint32_t* rows, int64_t n) {
  if (model != 0 && model != 1) return fit_refuse(h, who, "model must be 0 or 1");
  if (!h->fit.m[model].begun) return fit_refuse(h, who, "no fit in progress for this model (call nrv_fit_begin first)");
  if (n < 0 || (n > 0 && !rows)) return fit_refuse(h, who, "null row indices (or a negative count)");
  for (int64_t i = 0; i < n; ++i)
    if ((int64_t)rows[i] >= h->fit.rows) return fit_refuse(h, who, "a row index outside the training set (>= nrv_fit_count)");
  int rc;
  if ((rc = fit_scratch(h, (void**)&h->fit.d_order, &h->fit.cap_order, (size_t)(n > 0 ? n : 1) * 4))) return rc;
  return put(h, h->fit.d_order, rows, (size_t)n * 4, h->stream);
}
static TailGradArgs fit_grad_args(nrv_handle* h, int model, const unsigned* d_rows, int b, float* d_p) {
  const nrv_handle::Fit::Model& M = h->fit.m[model];
  TailGradArgs a;
  a.flat = h->fit.x[model]; a.y = h->fit.y[model]; a.rows = d_rows; a.par = M.d_par;
  a.partial = h->fit.d_partial; a.pstat = h->fit.d_pstat; a.p_out = d_p;
  a.T = h->T; a.C = h->dm[model].C; a.b = b; a.lambda = M.o.lambda;
  memcpy(a.cw, M.o.cw, sizeof a.cw);
  return a;
}
static TailAdamArgs fit_adam_args(nrv_handle* h, int model, int n_wg, int b, int mode, long long n_lr) {
  nrv_handle::Fit::Model& M = h->fit.m[model];
  const int P = fit_params_n(h, model);
  return TailAdamArgs{h->fit.d_partial, h->fit.d_pstat, n_wg, b, P, mode, M.d_par, M.d_par + P, M.d_par + 2 * P, M.d_par + 3 * P,
                      M.d_state, M.d_lr, M.t, n_lr, M.o.beta1, M.o.beta2, M.o.eps};
}
// the device's state of a model as a call starts (t kept, the sums zero) and what it holds once the call's launches are done
static int fit_state_put(nrv_handle* h, int model) {
  TailState s{};
  s.t = h->fit.m[model].t;
  HIPCHK(h, hipMemcpyAsync(h->fit.m[model].d_state, &s, sizeof s, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));              // (s is a local)
  return NRV_OK;
}
static int fit_state_get(nrv_handle* h, int model, nrv_fit_stats* stats) {
  TailState s{};
  HIPCHK(h, hipMemcpyAsync(&s, h->fit.m[model].d_state, sizeof s, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->fit.m[model].t = s.t;
  if (stats) *stats = nrv_fit_stats{s.rows, s.correct, s.steps, s.nonfinite, s.ce, s.center};
  return NRV_OK;
}
static int fit_head_wgs(int b) { const int tiles = (b + 31) / 32; return tiles < kHeadFitMaxWg ? tiles : kHeadFitMaxWg; }
static int fit_step_scratch(nrv_handle* h, int model, int b_max, bool grad) {
  const FitDepth& D = fit_at(h);
  size_t wg = ((size_t)b_max + 31) / 32;
  int rc;
  if (D.mlp) {
    wg = (size_t)fit_head_wgs(b_max);
    if ((rc = fit_scratch(h, (void**)&h->fit.d_flag, &h->fit.cap_flag,
                          (size_t)((NRV_FIT_PARAMS_BN(NRV_FIT_FULL) + 255) / 256 + (kRdN + 255) / 256 + 1 + (kSgDense + 255) / 256 + kL3N / 256 + kL4N / 256 +
                                   (kHeadFitMaxP + 255) / 256) * 4)))
      return rc;
  }
  size_t pn = (size_t)fit_params_n(h, model);
  if (fit_bn_block(h)) {                                     // the block's partials: one per workgroup of a chunk's ceil(M / 32)
    const size_t rows = (size_t)(b_max < kL4ChunkRows ? (b_max + 31) / 32 * 32 : kL4ChunkRows);
    if (grad && (rc = fit_scratch(h, (void**)&h->fit.d_pbn, &h->fit.cap_pbn, (rows * h->T + 31) / 32 * fit_bn_block(h) * 4))) return rc;
    pn -= fit_bn_block(h);
  }
  if (D.rd) {                                                // one chunk's nine arrays of nrv_fullfit.h, the read block's partials
    const size_t rows = (size_t)(b_max < kL4ChunkRows ? (b_max + 31) / 32 * 32 : kL4ChunkRows);
    if ((rc = fit_scratch(h, (void**)&h->fit.d_rd, &h->fit.cap_rd, rows * h->T * (grad ? kRdPairGrad : kRdPair) * 4)) ||
        (grad && (rc = fit_scratch(h, (void**)&h->fit.d_grd, &h->fit.cap_grd, (size_t)kRdSlices * kRdN * 4))))
      return rc;
    pn -= kRdN;
  }
  if (D.sg) {                                                // one chunk's [Xin | F | dS], the conv block's partials, the dense block's sums
    const size_t rows = (size_t)(b_max < kL4ChunkRows ? (b_max + 31) / 32 * 32 : kL4ChunkRows);
    if ((rc = fit_scratch(h, (void**)&h->fit.d_sg, &h->fit.cap_sg, rows * h->T * (grad ? 656 : 192) * 4)) ||
        (grad && (rc = fit_scratch(h, (void**)&h->fit.d_pconv, &h->fit.cap_pconv, (rows * h->T + 31) / 32 * kSgConv * 4))) ||
        (rc = fit_scratch(h, (void**)&h->fit.d_gdense, &h->fit.cap_gdense, (size_t)kSgDense * 4)))
      return rc;
    pn -= kSgN;
  }
  if (D.l3) {                                                // one chunk's [H3 | XB | dX3 | CS | GZ], the lstm3 block's sums, the identity list
    const size_t rows = (size_t)(b_max < kL4ChunkRows ? (b_max + 31) / 32 * 32 : kL4ChunkRows);
    if ((rc = fit_scratch(h, (void**)&h->fit.d_l3, &h->fit.cap_l3, rows * h->T * (grad ? 2048 : 512) * 4)) ||
        (rc = fit_scratch(h, (void**)&h->fit.d_gl3, &h->fit.cap_gl3, (size_t)kL3N * 4)))
      return rc;
    if (!h->fit.d_ident) {
      std::vector<unsigned> id(kL4ChunkRows);
      for (int i = 0; i < kL4ChunkRows; ++i) id[i] = (unsigned)i;
      HIPCHK(h, hipMalloc((void**)&h->fit.d_ident, (size_t)kL4ChunkRows * 4));
      HIPCHK(h, hipMemcpy(h->fit.d_ident, id.data(), (size_t)kL4ChunkRows * 4, hipMemcpyHostToDevice));
    }
    pn -= kL3N;
  }
  if (D.l4) {                                                // one chunk's [X4 | dX4 | CS | GZ], the LSTM block's sums; partials of the head alone
    const size_t rows = (size_t)(b_max < kL4ChunkRows ? (b_max + 31) / 32 * 32 : kL4ChunkRows);
    if ((rc = fit_scratch(h, (void**)&h->fit.d_l4, &h->fit.cap_l4, rows * h->T * (grad ? 896 : 128) * 4)) ||
        (rc = fit_scratch(h, (void**)&h->fit.d_gl4, &h->fit.cap_gl4, (size_t)kL4N * 4)))
      return rc;
    pn -= kL4N;
  }
  if (grad && (rc = fit_scratch(h, (void**)&h->fit.d_partial, &h->fit.cap_partial, wg * pn * 4))) return rc;
  return fit_scratch(h, (void**)&h->fit.d_pstat, &h->fit.cap_pstat, wg * sizeof(TailStat));
}

// nrv_fit_set_dropout: what the DROP launches and the unit door take, at `draw` of `model`
static DropArgs fit_drop_args(const nrv_handle* h, int model, int64_t draw) {
  const nrv_handle::Fit& F = h->fit;
  return DropArgs{(unsigned)(F.drop_seed & 0xffffffffu), (unsigned)(F.drop_seed >> 32), (unsigned)((uint64_t)draw & 0xffffffffu),
                  (unsigned)((uint64_t)draw >> 32), (unsigned)model << 16, F.drop_thr, F.drop_keepf};
}

// nrv_fit_bn_reestimate: behind the forward launches of one chunk (rows c0 .. c0 + bc - 1 of b), the moments of the stage's
// BatchNorms - stage 0: bn_c1, bn_l1; 1: bn_c2, bn_l2; 2: bn_l3, each only where it lies inside the fitted section - into the
// partials, and their reduction onto the model's running sums (nrv_bnfit.h)
static void fit_bn_moments(nrv_handle* h, int model, int stage, int c0, int bc, int b, const SigArgs& sa, const float* h1, const float* h2,
                           const float* h3) {
  nrv_handle::Fit::Model& M = h->fit.m[model];
  const int T = h->T, Mc = bc * T, wg_col = (Mc + kBnRows - 1) / kBnRows, wg_conv = (Mc + 32 * kBnTiles - 1) / (32 * kBnTiles);
  const bool full = fit_at(h).rd, sg = fit_at(h).sg;
  double* const pcol = h->fit.d_bnpart;                     // the two regions nrv_fit_bn_reestimate sized
  double* const pconv = pcol + (size_t)kL4ChunkRows * T / kBnRows * 512 + 512;
  BnReduceArgs ra{};
  int nb = 0;
  auto add = [&](int which, const double* part, int n_part, long long per_pair) {
    ra.bn[nb++] = BnReduceArgs::One{part, n_part, kFitBn[which].C, kFitBn[which].at, (long long)b * T * per_pair};
  };
  if (stage < 2 && sg) {
    const BnConvArgs ca{sa, M.d_bn + kBnPivot + kFitBn[stage].at, pconv};
    if (stage == 0) hipLaunchKernelGGL(bn_conv_moments_kernel<1>, dim3(wg_conv), dim3(256), 0, h->stream, ca);
    else hipLaunchKernelGGL(bn_conv_moments_kernel<2>, dim3(wg_conv), dim3(256), 0, h->stream, ca);
    add(stage, pconv, wg_conv, kSig);
  }
  if (stage == 0 && full) {
    hipLaunchKernelGGL(bn_col_moments_kernel<32>, dim3(wg_col), dim3(256), 0, h->stream, BnColArgs{h1, M.d_bn + kBnPivot + kFitBn[2].at, pcol, Mc});
    add(2, pcol, wg_col, 1);
  } else if (stage == 1 && full) {
    hipLaunchKernelGGL(bn_col_moments_kernel<128>, dim3(wg_col), dim3(256), 0, h->stream, BnColArgs{h2, M.d_bn + kBnPivot + kFitBn[3].at, pcol, Mc});
    add(3, pcol, wg_col, 1);
  } else if (stage == 2) {
    hipLaunchKernelGGL(bn_col_moments_kernel<256>, dim3(wg_col), dim3(256), 0, h->stream, BnColArgs{h3, M.d_bn + kBnPivot + kFitBn[4].at, pcol, Mc});
    add(4, pcol, wg_col, 1);
  }
  ra.acc = M.d_bnacc; ra.blk = M.d_bn; ra.cont = c0 > 0 ? 1 : 0; ra.last = c0 + bc == b ? 1 : 0;
  hipLaunchKernelGGL(bn_reduce_kernel, dim3(nb), dim3(256), 0, h->stream, ra);
}

// one batch of b rows onto the stream: the gradient (mode kTailGradOnly / kTailTrain) or the forward alone (kTailEval) and the
// reduce / update behind it - two launches at tail depth, three at head depth.  bn_stage >= 0 (nrv_fit_bn_reestimate, mode
// kTailEval, depth NRV_FIT_LSTM3 or deeper): per chunk the forward launches up to lstm3 and fit_bn_moments, nothing else
// draw >= 0 (nrv_fit_grad / _epoch while nrv_fit_set_dropout is on): the DROP instantiations of the two signal launches, at that draw
static void fit_launch(nrv_handle* h, int model, const unsigned* d_rows, int b, int mode, long long n_lr, float* d_p, int bn_stage = -1,
                       int64_t draw = -1) {
  const FitDepth& D = fit_at(h);
  const bool full = D.rd, sg = D.sg, l3 = D.l3;
  if (!D.mlp) {
    const int wg = (b + 31) / 32;
    if (mode == kTailEval) hipLaunchKernelGGL(tail_grad_kernel<false>, dim3(wg), dim3(256), 0, h->stream, fit_grad_args(h, model, d_rows, b, d_p));
    else hipLaunchKernelGGL(tail_grad_kernel<true>, dim3(wg), dim3(256), 0, h->stream, fit_grad_args(h, model, d_rows, b, d_p));
    hipLaunchKernelGGL(tail_adam_kernel, dim3(1), dim3(kFitAdamThreads), 0, h->stream, fit_adam_args(h, model, wg, b, mode, n_lr));
    return;
  }
  nrv_handle::Fit::Model& M = h->fit.m[model];
  const int wg = fit_head_wgs(b), P = fit_params_n(h, model), blocks = (P + 255) / 256;
  // the update of one block of the vector: `src` holds n_part partials of len gradients, the block starts at parameter `at`
  // and its reduce launch's flags at `flag`
  auto adam = [&](const float* src, int n_part, int len, int at, int flag) {
    return HeadAdamArgs{src, h->fit.d_pstat, n_part, b, len, mode, M.d_par + at, M.d_par + P + at, M.d_par + 2 * P + at, M.d_par + 3 * P + at,
                        (HeadState*)M.d_state, h->fit.d_flag + flag, M.d_lr, M.t, n_lr, M.o.beta1, M.o.beta2, M.o.eps};
  };
  if (D.l4) {
    const int T = h->T;
    const bool grad = mode != kTailEval;
    const int ob = fit_bn_block(h);                         // nrv_fit_set_bn_affine: the gamma / beta block in front of everything
    const int obr = ob + (full ? kR1N : 0);                 // where lstm2's block starts
    const int orr = ob + (full ? kRdN : 0);                 // where the signal depth's vector starts
    const int os = orr + (sg ? kSgN : 0);                   // where the lstm3 depth's vector starts
    const int o3 = os + (l3 ? kL3N : 0);                    // where the lstm4 depth's vector starts
    // every BatchNorm inside the fitted section is read from the fit's own block (the handle's pairs until nrv_fit_bn_reestimate);
    // the arguments that point into it are used at depth NRV_FIT_LSTM3 and deeper only, where the block exists
    const float* const fbn = l3 ? M.d_bn : h->dm[model].all;
    const size_t rcap = (size_t)(b < kL4ChunkRows ? (b + 31) / 32 * 32 : kL4ChunkRows) * T;
    float* const x4 = h->fit.d_l4;                          // the four arrays of fit_step_scratch, dX4 .. GZ only with grad
    float* const dx4 = x4 + rcap * 128;
    float* const cs = dx4 + rcap * 128;
    float* const gz = cs + rcap * 128;
    float* const h3 = h->fit.d_l3;                          // depth NRV_FIT_LSTM3: the five arrays of fit_step_scratch, dX3 .. GZ only with grad
    float* const xb4 = l3 ? h3 + rcap * 256 : nullptr;
    float* const dx3 = l3 ? xb4 + rcap * 256 : nullptr;
    float* const cs3 = l3 ? dx3 + rcap * 256 : nullptr;
    float* const gz3 = l3 ? cs3 + rcap * 256 : nullptr;
    float* const xin = h->fit.d_sg;                         // depth NRV_FIT_SIGNAL: the three arrays of fit_step_scratch, F and dS only with grad
    float* const fkeep = sg ? xin + rcap * 192 : nullptr;
    float* const ds = sg ? fkeep + rcap * 400 : nullptr;
    float* const x1b = h->fit.d_rd;                         // depth NRV_FIT_FULL: the nine arrays of fit_step_scratch, dH2 .. GZ2 only with grad
    float* const h1 = full ? x1b + rcap * 32 : nullptr;
    float* const h2 = full ? h1 + rcap * 32 : nullptr;
    float* const dh2 = full ? h2 + rcap * 128 : nullptr;
    float* const dh1 = full ? dh2 + rcap * 128 : nullptr;
    float* const cs1 = full ? dh1 + rcap * 32 : nullptr;
    float* const cs2 = full ? cs1 + rcap * 32 : nullptr;
    float* const gz1 = full ? cs2 + rcap * 128 : nullptr;
    float* const gz2 = full ? gz1 + rcap * 128 : nullptr;
    const int sg_wg = sg ? ((b < kL4ChunkRows ? b : kL4ChunkRows) * T + 31) / 32 : 0;     // workgroups of sig_backward_kernel in the first chunk: the conv block's partials
    const bool drop = sg && grad && draw >= 0 && h->fit.drop_rate > 0.0;
    const DropArgs dr = fit_drop_args(h, model, draw < 0 ? 0 : draw);
    const int bn_wg = ((b < kL4ChunkRows ? b : kL4ChunkRows) * T + 31) / 32;              // ... of the launches that leave the gamma / beta block's
    // the sums of BatchNorm `which` (of kFitBn) over this chunk: its place in the block's partials, the block's current statistics
    int bn_at[5] = {0, 0, 0, 0, 0};
    for (int i = 0, at = 0; i < D.n_bn; at += 2 * kFitBn[D.bn[i]].C, ++i) bn_at[D.bn[i]] = at;
    auto bn_sums = [&](int which, const float* x, int c0) {
      return BnAffArgs{x, M.d_bn + kBnMean + kFitBn[which].at, M.d_bn + kBnVar + kFitBn[which].at, h->fit.d_pbn + bn_at[which], ob, c0 > 0 ? 1 : 0};
    };
    for (int c0 = 0; c0 < b; c0 += kL4ChunkRows) {
      const int bc = b - c0 < kL4ChunkRows ? b - c0 : kL4ChunkRows, tiles = (bc + 31) / 32;
      const SigArgs sa{sg ? h->fit.x[model] : nullptr, h->fit.shared[0], d_rows + c0, M.d_par + orr, fbn + kBnConv, xin, fkeep, ds, gz3,
                       h->fit.d_pconv, h->fit.d_gdense, T, bc * T, grad ? 1 : 0, c0 > 0 ? 1 : 0, dh2, fbn + kBnS2};
      const RlArgs r1{h->fit.shared[1], d_rows + c0, M.d_par + ob, fbn + kBnS1, fbn + kBnH1, h1, x1b, gz1, cs1, dh1,
                      h->fit.d_grd, 32, T, bc, grad ? 1 : 0, c0 > 0 ? 1 : 0};
      const RlArgs r2{x1b, h->fit.d_ident, M.d_par + obr, fbn + kBnS2, fbn + kBnH2, h2, xin, gz2, cs2, dh2,
                      full ? h->fit.d_grd + kR1N : nullptr, 192, T, bc, grad ? 1 : 0, c0 > 0 ? 1 : 0};
      if (full) {                                           // lstm1, lstm2 (X2b into columns 0 .. 127 of Xin), then S into the rest
        if (h->act == 0) {
          hipLaunchKernelGGL((rl_forward_kernel<6, 16, 0>), dim3(tiles, 2), dim3(128), 0, h->stream, r1);
          hipLaunchKernelGGL((rl_forward_kernel<32, 64, 0>), dim3(tiles, 2), dim3(256), 0, h->stream, r2);
        } else {
          hipLaunchKernelGGL((rl_forward_kernel<6, 16, 1>), dim3(tiles, 2), dim3(128), 0, h->stream, r1);
          hipLaunchKernelGGL((rl_forward_kernel<32, 64, 1>), dim3(tiles, 2), dim3(256), 0, h->stream, r2);
        }
        if (drop) hipLaunchKernelGGL((sig_forward_kernel<false, true>), dim3((bc * T + 31) / 32), dim3(256), 0, h->stream, SigDrop<SigArgs>{sa, dr});
        else hipLaunchKernelGGL(sig_forward_kernel<false>, dim3((bc * T + 31) / 32), dim3(256), 0, h->stream, sa);
      } else if (sg && drop) hipLaunchKernelGGL((sig_forward_kernel<true, true>), dim3((bc * T + 31) / 32), dim3(256), 0, h->stream, SigDrop<SigArgs>{sa, dr});
      else if (sg) hipLaunchKernelGGL(sig_forward_kernel<true>, dim3((bc * T + 31) / 32), dim3(256), 0, h->stream, sa);
      const L3Args l3a{sg ? xin : l3 ? h->fit.x[model] : nullptr, sg ? h->fit.d_ident : d_rows + c0, M.d_par + os, fbn + kBnS3, fbn + kBnH3, h3, xb4, gz3, cs3, dx3, gz,
                       h->fit.d_gl3, T, bc, grad ? 1 : 0, c0 > 0 ? 1 : 0};
      if (l3) {                                             // lstm3 forward: the scratch XB is "the set" of the lstm4 launches
        if (h->act == 0) hipLaunchKernelGGL(l3_forward_kernel<0>, dim3(tiles, 2), dim3(256), 0, h->stream, l3a);
        else hipLaunchKernelGGL(l3_forward_kernel<1>, dim3(tiles, 2), dim3(256), 0, h->stream, l3a);
      }
      if (bn_stage >= 0) { fit_bn_moments(h, model, bn_stage, c0, bc, b, sa, h1, h2, h3); continue; }
      const L4Args la{l3 ? xb4 : h->fit.x[model], l3 ? h->fit.d_ident : d_rows + c0, M.d_par + o3, x4, gz, cs, dx4, h->fit.d_gl4, T, bc,
                      grad ? 1 : 0, c0 > 0 ? 1 : 0};
      if (h->act == 0) hipLaunchKernelGGL(l4_forward_kernel<0>, dim3(tiles, 2), dim3(256), 0, h->stream, la);
      else hipLaunchKernelGGL(l4_forward_kernel<1>, dim3(tiles, 2), dim3(256), 0, h->stream, la);
      HeadGradArgs a;
      a.x = x4; a.y = h->fit.y[model]; a.rows = d_rows + c0; a.par = M.d_par + o3 + kL4N;
      a.partial = h->fit.d_partial; a.pstat = h->fit.d_pstat; a.p_out = d_p ? d_p + (size_t)c0 * h->dm[model].C : nullptr;
      a.T = T; a.C = h->dm[model].C; a.b = bc; a.lambda = M.o.lambda;
      memcpy(a.cw, M.o.cw, sizeof a.cw);
      a.dh1 = dx4; a.cont = c0 > 0 ? 1 : 0;
      if (!grad) { hipLaunchKernelGGL((head_grad_kernel<false, true>), dim3(tiles), dim3(256), 0, h->stream, a); continue; }
      hipLaunchKernelGGL((head_grad_kernel<true, true>), dim3(tiles), dim3(256), 0, h->stream, a);
      if (h->act == 0) hipLaunchKernelGGL(l4_backward_kernel<0>, dim3(tiles, 2), dim3(256), 0, h->stream, la);
      else hipLaunchKernelGGL(l4_backward_kernel<1>, dim3(tiles, 2), dim3(256), 0, h->stream, la);
      hipLaunchKernelGGL(l4_wgrad_kernel, dim3(kL4WgM * kL4WgN, 2), dim3(256), 0, h->stream, la);
      if (l3) {
        const L4DxArgs da{gz, M.d_par + o3, fbn + kBnS3, dx3, bc * T};
        if (ob) hipLaunchKernelGGL(l4_dx_kernel<L4DxBnArgs>, dim3((bc * T + 31) / 32), dim3(256), 0, h->stream, L4DxBnArgs{da, bn_sums(4, h3, c0)});
        else hipLaunchKernelGGL(l4_dx_kernel<L4DxArgs>, dim3((bc * T + 31) / 32), dim3(256), 0, h->stream, da);
        if (h->act == 0) hipLaunchKernelGGL(l3_backward_kernel<0>, dim3(tiles, 2), dim3(256), 0, h->stream, l3a);
        else hipLaunchKernelGGL(l3_backward_kernel<1>, dim3(tiles, 2), dim3(256), 0, h->stream, l3a);
        hipLaunchKernelGGL(l3_wgrad_kernel, dim3(kL3WgM * kL3WgN, 2), dim3(256), 0, h->stream, l3a);
      }
      if (sg) {
        if (full && ob) hipLaunchKernelGGL((l3_dx_kernel<true, SigBnArgs>), dim3((bc * T + 31) / 32), dim3(384), 0, h->stream, SigBnArgs{sa, bn_sums(3, h2, c0)});
        else if (full) hipLaunchKernelGGL(l3_dx_kernel<true>, dim3((bc * T + 31) / 32), dim3(384), 0, h->stream, sa);
        else hipLaunchKernelGGL(l3_dx_kernel<false>, dim3((bc * T + 31) / 32), dim3(128), 0, h->stream, sa);
        if (ob && drop) hipLaunchKernelGGL((sig_backward_kernel<SigBnArgs, true>), dim3((bc * T + 31) / 32), dim3(256), 0, h->stream,
                                           SigDrop<SigBnArgs>{SigBnArgs{sa, bn_sums(0, nullptr, c0)}, dr});
        else if (ob) hipLaunchKernelGGL(sig_backward_kernel<SigBnArgs>, dim3((bc * T + 31) / 32), dim3(256), 0, h->stream, SigBnArgs{sa, bn_sums(0, nullptr, c0)});
        else if (drop) hipLaunchKernelGGL((sig_backward_kernel<SigArgs, true>), dim3((bc * T + 31) / 32), dim3(256), 0, h->stream, SigDrop<SigArgs>{sa, dr});
        else hipLaunchKernelGGL(sig_backward_kernel<SigArgs>, dim3((bc * T + 31) / 32), dim3(256), 0, h->stream, sa);
        hipLaunchKernelGGL(sig_wgrad_kernel, dim3(kSgWgM, 2), dim3(512), 0, h->stream, sa);
      }
      if (full) {
        const RlDxArgs dxa{gz2, M.d_par + obr, fbn + kBnS1, dh1, bc * T};
        if (h->act == 0) hipLaunchKernelGGL((rl_backward_kernel<32, 64, 0>), dim3(tiles, 2), dim3(256), 0, h->stream, r2);
        else hipLaunchKernelGGL((rl_backward_kernel<32, 64, 1>), dim3(tiles, 2), dim3(256), 0, h->stream, r2);
        if (ob) hipLaunchKernelGGL((rl_dx_kernel<32, 64, RlDxBnArgs>), dim3((bc * T + 31) / 32), dim3(64), 0, h->stream, RlDxBnArgs{dxa, bn_sums(2, h1, c0)});
        else hipLaunchKernelGGL((rl_dx_kernel<32, 64>), dim3((bc * T + 31) / 32), dim3(64), 0, h->stream, dxa);
        if (h->act == 0) hipLaunchKernelGGL((rl_backward_kernel<6, 16, 0>), dim3(tiles, 2), dim3(128), 0, h->stream, r1);
        else hipLaunchKernelGGL((rl_backward_kernel<6, 16, 1>), dim3(tiles, 2), dim3(128), 0, h->stream, r1);
        hipLaunchKernelGGL((rl_wgrad_kernel<32, 64>), dim3(4 * 4, 2, kRdSlices), dim3(256), 0, h->stream, r2);
        hipLaunchKernelGGL((rl_wgrad_kernel<6, 16>), dim3(1, 2, kRdSlices), dim3(256), 0, h->stream, r1);
      }
    }
    if (bn_stage >= 0) return;
    // the LSTM block is one "partial" of its own; the head's partials behind it; the flags of both launches in one array
    // (at depth NRV_FIT_LSTM3 the lstm3 block is one more single "partial" in front)
    // (at depth NRV_FIT_SIGNAL the conv block's partials and the dense block in front of that; 25896 is no multiple of 256, so
    // every reduce launch has a flag range of its own and the update launch has as many workgroups as there are flags)
    const int o4 = o3 + kL4N, PH = P - o4, bl3 = l3 ? kL3N / 256 : 0, bl4 = kL4N / 256;
    // (at depth NRV_FIT_FULL the read block's kRdSlices partials in front of everything, with 206 flags of their own)
    // (with nrv_fit_set_bn_affine the gamma / beta block's partials in front of that, with 2, 3 or 4 flags of their own, and behind
    // the update the refold of the fit's pairs)
    const int blb = (ob + 255) / 256;
    const int blr = blb + (full ? (kRdN + 255) / 256 : 0);
    if (ob) hipLaunchKernelGGL(head_reduce_kernel, dim3(blb), dim3(256), 0, h->stream, adam(h->fit.d_pbn, bn_wg, ob, 0, 0));
    const int bls = blr + (sg ? 1 + (kSgDense + 255) / 256 : 0);
    if (full) hipLaunchKernelGGL(head_reduce_kernel, dim3(blr - blb), dim3(256), 0, h->stream, adam(h->fit.d_grd, kRdSlices, kRdN, ob, blb));
    if (sg) {
      hipLaunchKernelGGL(head_reduce_kernel, dim3(1), dim3(256), 0, h->stream, adam(h->fit.d_pconv, sg_wg, kSgConv, orr, blr));
      hipLaunchKernelGGL(head_reduce_kernel, dim3(bls - blr - 1), dim3(256), 0, h->stream, adam(h->fit.d_gdense, 1, kSgDense, orr + kSgWs, blr + 1));
    }
    if (l3) hipLaunchKernelGGL(head_reduce_kernel, dim3(bl3), dim3(256), 0, h->stream, adam(h->fit.d_gl3, 1, kL3N, os, bls));
    hipLaunchKernelGGL(head_reduce_kernel, dim3(bl4), dim3(256), 0, h->stream, adam(h->fit.d_gl4, 1, kL4N, o3, bls + bl3));
    hipLaunchKernelGGL(head_reduce_kernel, dim3((PH + 255) / 256), dim3(256), 0, h->stream, adam(h->fit.d_partial, wg, PH, o4, bls + bl3 + bl4));
    hipLaunchKernelGGL(head_adam_kernel, dim3(sg || ob ? bls + bl3 + bl4 + (PH + 255) / 256 : blocks), dim3(256), 0, h->stream,
                       adam(h->fit.d_partial, wg, P, 0, 0));
    if (ob && mode == kTailTrain) hipLaunchKernelGGL(bn_refold_kernel, dim3(D.n_bn), dim3(256), 0, h->stream, fit_refold_args(h, model));
    return;
  }
  HeadGradArgs a;
  a.dh1 = nullptr; a.cont = 0;
  a.x = h->fit.x[model]; a.y = h->fit.y[model]; a.rows = d_rows; a.par = M.d_par;
  a.partial = h->fit.d_partial; a.pstat = h->fit.d_pstat; a.p_out = d_p;
  a.T = h->T; a.C = h->dm[model].C; a.b = b; a.lambda = M.o.lambda;
  memcpy(a.cw, M.o.cw, sizeof a.cw);
  if (mode == kTailEval) hipLaunchKernelGGL(head_grad_kernel<false>, dim3(wg), dim3(256), 0, h->stream, a);
  else hipLaunchKernelGGL(head_grad_kernel<true>, dim3(wg), dim3(256), 0, h->stream, a);
  const HeadAdamArgs u = adam(h->fit.d_partial, wg, P, 0, 0);
  hipLaunchKernelGGL(head_reduce_kernel, dim3(blocks), dim3(256), 0, h->stream, u);
  hipLaunchKernelGGL(head_adam_kernel, dim3(blocks), dim3(256), 0, h->stream, u);
}

int nrv_fit_grad(nrv_handle* h, int model, const uint32_t* rows, int b, float* grad, nrv_fit_stats* stats) {
  static const char* who = "nrv_fit_grad";
  int rc = fit_enter(h, who);
  if (rc) return rc;
  if (b < 1 || b > NRV_FIT_MAX_BATCH) return fit_refuse(h, who, "b outside 1 .. NRV_FIT_MAX_BATCH");
  if (!grad || !rows) return fit_refuse(h, who, "null rows / grad");
  if ((rc = fit_rows_in(h, who, model, rows, b)) || (rc = fit_step_scratch(h, model, b, true)) || (rc = fit_state_put(h, model))) return rc;
  const int P = fit_params_n(h, model);
  fit_launch(h, model, h->fit.d_order, b, kTailGradOnly, 0, nullptr, -1, h->fit.drop_rate > 0.0 ? h->fit.m[model].draw : -1);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(grad, h->fit.m[model].d_par + 3 * (size_t)P, (size_t)P * 4, hipMemcpyDeviceToHost, h->stream));
  return fit_state_get(h, model, stats);
}

int nrv_fit_epoch(nrv_handle* h, int model, const uint32_t* order, int64_t n, nrv_fit_stats* stats) {
  static const char* who = "nrv_fit_epoch";
  int rc = fit_enter(h, who);
  if (rc) return rc;
  if ((rc = fit_rows_in(h, who, model, order, n))) return rc;
  nrv_handle::Fit::Model& M = h->fit.m[model];
  const int B = M.o.B;
  const int64_t nb = (n + B - 1) / B;
  if ((rc = fit_step_scratch(h, model, B, true)) || (rc = fit_scratch(h, (void**)&M.d_lr, &M.cap_lr, (size_t)(nb > 0 ? nb : 1) * 4))) return rc;
  std::vector<float> lr((size_t)nb);
  for (int64_t k = 0; k < nb; ++k) {                       // lr_t for t = M.t + 1 .. M.t + nb, in f64, rounded once
    const double t = (double)(M.t + k + 1);
    lr[(size_t)k] = (float)((double)M.o.lr * std::sqrt(1.0 - std::pow((double)M.o.beta2, t)) / (1.0 - std::pow((double)M.o.beta1, t)));
  }
  if ((rc = put(h, M.d_lr, lr.data(), (size_t)nb * 4, h->stream)) || (rc = fit_state_put(h, model))) return rc;
  for (int64_t k = 0; k < nb; ++k) {
    const int b = (int)(n - k * B < B ? n - k * B : B);
    fit_launch(h, model, h->fit.d_order + k * B, b, kTailTrain, nb, nullptr, -1, h->fit.drop_rate > 0.0 ? M.draw + k : -1);
  }
  if (h->fit.drop_rate > 0.0) M.draw += nb;                 // skipped non-finite batches included: a host counter
  HIPCHK(h, hipGetLastError());
  return fit_state_get(h, model, stats);
}

int nrv_fit_eval(nrv_handle* h, int model, const uint32_t* order, int64_t n, float* p, nrv_fit_stats* stats) {
  static const char* who = "nrv_fit_eval";
  int rc = fit_enter(h, who);
  if (rc) return rc;
  if ((rc = fit_rows_in(h, who, model, order, n))) return rc;
  const int C = h->dm[model].C;
  if ((rc = fit_step_scratch(h, model, kFitMaxB, false)) ||
      (p && (rc = fit_scratch(h, (void**)&h->fit.d_p, &h->fit.cap_p, (size_t)(n > 0 ? n : 1) * C * 4))) || (rc = fit_state_put(h, model)))
    return rc;
  for (int64_t s = 0; s < n; s += kFitMaxB) {
    const int b = (int)(n - s < kFitMaxB ? n - s : kFitMaxB);
    fit_launch(h, model, h->fit.d_order + s, b, kTailEval, 0, p ? h->fit.d_p + (size_t)s * C : nullptr);
  }
  HIPCHK(h, hipGetLastError());
  if (p && n > 0) HIPCHK(h, hipMemcpyAsync(p, h->fit.d_p, (size_t)n * C * 4, hipMemcpyDeviceToHost, h->stream));
  return fit_state_get(h, model, stats);
}

int nrv_fit_params(nrv_handle* h, int model, float* params, int64_t* t) {
  static const char* who = "nrv_fit_params";
  const int rc = fit_enter(h, who);
  if (rc) return rc;
  if (model != 0 && model != 1) return fit_refuse(h, who, "model must be 0 or 1");
  if (!h->fit.m[model].begun) return fit_refuse(h, who, "no fit in progress for this model (call nrv_fit_begin first)");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (params) HIPCHK(h, hipMemcpy(params, h->fit.m[model].d_par, (size_t)fit_params_n(h, model) * 4, hipMemcpyDeviceToHost));
  if (t) *t = h->fit.m[model].t;
  return NRV_OK;
}

// the BatchNorms inside the fitted section, as indices into kFitBn, in tensor order -> their number
static int fit_bn_list(const nrv_handle* h, int (&list)[5]) {
  const FitDepth& D = fit_at(h);
  for (int i = 0; i < D.n_bn; ++i) list[i] = D.bn[i];
  return D.n_bn;
}

int nrv_fit_bn_count(nrv_handle* h) {
  const int rc = check_handle(h);
  int list[5];
  return rc ? rc : fit_bn_list(h, list);
}

int nrv_fit_bn_reestimate(nrv_handle* h, int model, const uint32_t* rows, int64_t n_rows) {
  static const char* who = "nrv_fit_bn_reestimate";
  int rc = fit_enter(h, who);
  if (rc) return rc;
  int list[5];
  const int nbn = fit_bn_list(h, list);
  if (!nbn) return fit_refuse(h, who, "no BatchNorm lies inside the fitted section (depths NRV_FIT_LSTM3, NRV_FIT_SIGNAL and NRV_FIT_FULL have one)");
  if (n_rows <= 0 || n_rows > INT32_MAX) return fit_refuse(h, who, "n_rows outside 1 .. 2^31 - 1");
  if ((rc = fit_rows_in(h, who, model, rows, n_rows))) return rc;
  nrv_handle::Fit::Model& M = h->fit.m[model];
  const DevModel& d = h->dm[model];
  const int T = h->T, b = (int)n_rows;
  if ((rc = fit_step_scratch(h, model, b < kL4ChunkRows ? b : kL4ChunkRows, false)) ||
      (rc = fit_scratch(h, (void**)&h->fit.d_bnpart, &h->fit.cap_bnpart, ((size_t)kL4ChunkRows * T / kBnRows * 512 + 512 + ((size_t)kL4ChunkRows * T / 256 + 1) * 16) * 8)))
    return rc;
  std::vector<float> blk((size_t)kBnFloats);
  std::vector<double> acc((size_t)2 * kBnCh);
  std::vector<float> gb((size_t)fit_bn_block(h));            // nrv_fit_set_bn_affine: the stages are folded with the vector's CURRENT gamma / beta
  if (!gb.empty()) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(gb.data(), M.d_par, gb.size() * 4, hipMemcpyDeviceToHost));
  }
  for (int stage = nbn == 1 ? 2 : 0; stage < 3; ++stage) {
    fit_launch(h, model, h->fit.d_order, b, kTailEval, 0, nullptr, stage);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(blk.data(), M.d_bn, blk.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(acc.data(), M.d_bnacc, acc.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // the stage's BatchNorms: the new statistics folded as nrv_create folds the tensors of a file, into the block
    static const int stage_of[5] = {0, 1, 0, 1, 2}, at_s[5] = {kBnConv + 32, kBnConv + 248, kBnS1, kBnS2, kBnS3},
                     at_h[5] = {kBnConv + 40, kBnConv + 256, kBnH1, kBnH2, kBnH3};
    for (int i = 0, gb_at = 0; i < nbn; gb_at += 2 * kFitBn[list[i]].C, ++i) {
      const int w = list[i], at = kFitBn[w].at, C = kFitBn[w].C;
      if (stage_of[w] != stage) continue;
      for (int c = 0; c < C; ++c) {
        M.bn_mean[at + c] = blk[kBnMean + at + c]; M.bn_var[at + c] = blk[kBnVar + at + c];
        M.bn_s1[at + c] = acc[at + c]; M.bn_s2[at + c] = acc[kBnCh + at + c];
      }
      M.bn_n[w] = (int64_t)b * T * (w < 2 ? kSig : 1);
      std::vector<float> sc(C), sh(C);
      bn_fold(gb.empty() ? d.bn_raw[0].data() + at : gb.data() + gb_at, gb.empty() ? d.bn_raw[1].data() + at : gb.data() + gb_at + C,
              M.bn_mean.data() + at, M.bn_var.data() + at, C, sc.data(), sh.data());
      HIPCHK(h, hipMemcpy(M.d_bn + at_s[w], sc.data(), (size_t)C * 4, hipMemcpyHostToDevice));
      HIPCHK(h, hipMemcpy(M.d_bn + at_h[w], sh.data(), (size_t)C * 4, hipMemcpyHostToDevice));
    }
  }
  return NRV_OK;
}

int nrv_fit_set_bn_affine(nrv_handle* h, int on) {
  static const char* who = "nrv_fit_set_bn_affine";
  const int rc = fit_enter(h, who);
  if (rc) return rc;
  if (on && !fit_at(h).n_bn)
    return fit_refuse(h, who, "no BatchNorm lies inside the fitted section (depths NRV_FIT_LSTM3, NRV_FIT_SIGNAL and NRV_FIT_FULL have one)");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int m = 0; m < 2; ++m) {                            // any nrv_fit_begin is forgotten: its vector has the other length
    h->fit.m[m].begun = false;
    h->fit.m[m].t = 0;
  }
  if ((on != 0) == h->fit.bn_affine) return NRV_OK;
  fit_bn_affine_off(h);
  h->fit.bn_affine = on != 0;
  return NRV_OK;
}

int nrv_fit_bn_affine(nrv_handle* h) {
  const int rc = check_handle(h);
  return rc ? rc : (h->fit.bn_affine ? 1 : 0);
}

int nrv_fit_set_dropout(nrv_handle* h, double rate, uint64_t seed) {
  static const char* who = "nrv_fit_set_dropout";
  const int rc = fit_enter(h, who);
  if (rc) return rc;
  if (!(rate >= 0.0 && rate < 1.0)) return fit_refuse(h, who, "rate must lie in [0, 1)");
  if (rate > 0.0 && !fit_at(h).sg)
    return fit_refuse(h, who, "the signal branch is frozen at this depth, there is nothing to drop (depths NRV_FIT_SIGNAL and NRV_FIT_FULL fit it)");
  if (rate > 0.0 && h->T > 655) return fit_refuse(h, who, "T > 655: t * 100 + q would not fit the counter's 16 bits");
  nrv_handle::Fit& F = h->fit;
  F.drop_rate = rate;
  F.drop_thr = (unsigned)std::floor(rate * 4294967296.0);
  F.drop_keepf = (float)(1.0 - rate);
  F.drop_seed = seed;
  F.m[0].draw = F.m[1].draw = 0;
  return NRV_OK;
}

int nrv_fit_dropout(nrv_handle* h, double* rate, uint64_t* seed, int64_t draw[2]) {
  const int rc = check_handle(h);
  if (rc) return rc;
  if (rate) *rate = h->fit.drop_rate;
  if (seed) *seed = h->fit.drop_seed;
  if (draw) { draw[0] = h->fit.m[0].draw; draw[1] = h->fit.m[1].draw; }
  return NRV_OK;
}

int nrv_fit_set_dropout_draw(nrv_handle* h, int model, int64_t draw) {
  static const char* who = "nrv_fit_set_dropout_draw";
  const int rc = fit_enter(h, who);
  if (rc) return rc;
  if (model != 0 && model != 1) return fit_refuse(h, who, "model must be 0 or 1");
  if (draw < 0) return fit_refuse(h, who, "draw must not be negative");
  h->fit.m[model].draw = draw;
  return NRV_OK;
}

int nrv_fit_dropout_mask(nrv_handle* h, int model, const uint32_t* rows, int b, int64_t draw, uint8_t* mask) {
  static const char* who = "nrv_fit_dropout_mask";
  int rc = fit_enter(h, who);
  if (rc) return rc;
  if (model != 0 && model != 1) return fit_refuse(h, who, "model must be 0 or 1");
  if (!(h->fit.drop_rate > 0.0)) return fit_refuse(h, who, "the dropout is off (call nrv_fit_set_dropout with a rate above 0 first)");
  if (b < 1 || b > NRV_FIT_MAX_BATCH) return fit_refuse(h, who, "b outside 1 .. NRV_FIT_MAX_BATCH");
  if (!rows || !mask) return fit_refuse(h, who, "null rows / mask");
  if (draw < 0) return fit_refuse(h, who, "draw must not be negative");
  const long long quads = (long long)b * h->T * 100;
  if ((rc = fit_scratch(h, (void**)&h->fit.d_order, &h->fit.cap_order, (size_t)b * 4)) ||
      (rc = fit_scratch(h, (void**)&h->fit.d_mask, &h->fit.cap_mask, (size_t)quads * 4)) ||
      (rc = put(h, h->fit.d_order, rows, (size_t)b * 4, h->stream)))
    return rc;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, h->stream,
                     DropMaskArgs{fit_drop_args(h, model, draw), h->fit.d_order, h->fit.d_mask, h->T, quads});
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(mask, h->fit.d_mask, (size_t)quads * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return NRV_OK;
}

int nrv_fit_bn_get(nrv_handle* h, int model, int which, nrv_fit_bn_info* info, float* mean, float* var, double* s1, double* s2) {
  static const char* who = "nrv_fit_bn_get";
  const int rc = fit_enter(h, who);
  if (rc) return rc;
  if (model != 0 && model != 1) return fit_refuse(h, who, "model must be 0 or 1");
  int list[5];
  const int nbn = fit_bn_list(h, list);
  if (!nbn) return fit_refuse(h, who, "no BatchNorm lies inside the fitted section (depths NRV_FIT_LSTM3, NRV_FIT_SIGNAL and NRV_FIT_FULL have one)");
  const nrv_handle::Fit::Model& M = h->fit.m[model];
  if (!M.begun) return fit_refuse(h, who, "no fit in progress for this model (call nrv_fit_begin first)");
  if (which < 0 || which >= nbn) return fit_refuse(h, who, "which outside 0 .. nrv_fit_bn_count - 1");
  const int w = list[which], at = kFitBn[w].at, C = kFitBn[w].C;
  if (info) *info = nrv_fit_bn_info{kFitBn[w].tensor, C, M.bn_n[w]};
  if (mean) memcpy(mean, M.bn_mean.data() + at, (size_t)C * 4);
  if (var) memcpy(var, M.bn_var.data() + at, (size_t)C * 4);
  if (s1) memcpy(s1, M.bn_s1.data() + at, (size_t)C * 8);
  if (s2) memcpy(s2, M.bn_s2.data() + at, (size_t)C * 8);
  return NRV_OK;
}

int nrv_saturated(nrv_handle* h, int64_t* pending, int64_t* reruns) {
  int rc = check_handle(h);
  if (rc) return rc;
  unsigned v = 0;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(&v, h->d_sat + 2, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (v) HIPCHK(h, hipMemset(h->d_sat + 2, 0, sizeof(unsigned)));
  if (pending) *pending = (int64_t)v;
  if (reruns) *reruns = h->sat_reruns;
  return NRV_OK;
}

int nrv_prof_enable(nrv_handle* h, int on) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = prof_collect(h))) return rc;
  h->prof = (on == 2 || on == 3) ? on : (on != 0);
  h->prof_tick = 0;
  return NRV_OK;
}

int nrv_prof_read(nrv_handle* h, double* ms_total, int64_t* launches) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = prof_collect(h))) return rc;
  for (int k = 0; k < NRV_N_KERNELS; ++k) {
    if (ms_total) ms_total[k] = h->prof_ms[k];
    if (launches) launches[k] = h->prof_n[k];
    h->prof_ms[k] = 0;
    h->prof_n[k] = 0;
  }
  return NRV_OK;
}

int nrv_prof_overhead(nrv_handle* h, double* us) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!us) { h->err = "nrv_prof_overhead: null output"; return NRV_E_INVALID; }
  // what a bracket measures beyond the kernel it encloses: two event records back to back on the launch stream
  constexpr int N = 64;
  struct Events {                                    // destroyed on every path out of this function
    hipEvent_t ev[2 * N];
    int n = 0;
    ~Events() { for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]); }
  } E;
  for (; E.n < 2 * N; ++E.n) HIPCHK(h, hipEventCreate(&E.ev[E.n]));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < 2 * N; ++i) HIPCHK(h, hipEventRecord(E.ev[i], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  double tot = 0;
  for (int i = 0; i < N; ++i) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, E.ev[2 * i], E.ev[2 * i + 1]));
    tot += ms;
  }
  *us = tot / N * 1e3;
  return NRV_OK;
}

#if NRV_STAMP
// diagnostic build only (not in include/nanorev.h): the phase stamps of the last lstm_h2s_kernel launches
int nrv_exp_only_stage(int k) {
  g_only_stage = k;
  return 0;
}
int nrv_exp_stamps(void* dst, size_t bytes) {
  if (bytes > sizeof(nrv::nrv_stamp_buf)) bytes = sizeof(nrv::nrv_stamp_buf);
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(nrv::nrv_stamp_buf), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? (int)0 : -1;
}
#endif

const char* nrv_kernel_name(int slot) {
  // slots are pipeline stages; which kernel runs a stage depends on nrv_set_precision
  // (lstm_split_kernel / head_mlp_split_kernel for bf16x3, lstm_layer_kernel / head_mlp_kernel for f32)
  static const char* names[NRV_N_KERNELS] = {"cnn_kernel", "lstm1_kernel 6->16", "lstm2 32->64", "lstm3 192->128",
                                             "lstm4 256->64", "head_mlp+head_final"};
  return (slot >= 0 && slot < NRV_N_KERNELS) ? names[slot] : "";
}

const char* nrv_last_error(nrv_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }
int nrv_backend(nrv_handle* h) { (void)h; return NRV_BACKEND_HIP; }
int nrv_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess && n > 0 ? n : 0;
}
int nrv_window(nrv_handle* h) { return h ? h->T : NRV_E_INVALID; }

}  // extern "C"
