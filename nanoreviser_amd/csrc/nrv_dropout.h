// The reference's Dropout(0.2) behind the identity block, on the device (nrv_fit_set_dropout): the counter-based random stream,
// the keep bits of four elements of F, and the unit door's launch.
#pragma once
#include <cstdint>

namespace nrv {

// ---------------------------------------------------------------------------------------
// nanoreviser_amd/dropout.py is the DEFINITION; include/nanorev.h (nrv_fit_set_dropout) states the rule.  The mask is a pure
// function of (seed, draw, model, set row, t, element): element f = p * 8 + o of F belongs to quad q = f / 4, and the four
// words of
//   philox4x32_10(counter = (row, model << 16 | t * 100 + q, draw low, draw high), key = (seed low, seed high))
// serve f = 4 q .. 4 q + 3 in order; an element is kept iff its word >= thr = floor(rate * 2^32).  Kept elements are DIVIDED by
// keepf = float32(1 - rate), forward (F) and backward (dF) alike.  Nothing here has a state: batch position, chunk and
// workgroup layout do not enter, so the same calls give the same bytes.
// Users: sig_forward_kernel<., true> (the img planes before the 400 -> 64 product; a.F keeps the dropped F),
// sig_backward_kernel<., true> (dF in LDS before anything reads it) and dropout_mask_kernel (nrv_fit_dropout_mask).
// ---------------------------------------------------------------------------------------
struct DropArgs {
  unsigned key0, key1;                   // the seed's words
  unsigned draw0, draw1;                 // the draw's words
  unsigned model16;                      // model << 16
  unsigned thr;                          // floor(rate * 2^32)
  float keepf;                           // float32(1 - rate)
};

// the standard generator: ten rounds, the key bumped by the Weyl constants between them.  Multiply-high is __umulhi
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// the keep bits of quad q of (row, t): bit j is element 4 q + j
__device__ __forceinline__ unsigned drop_keep4(const DropArgs& d, unsigned row, int t, int q) {
  unsigned c[4] = {row, d.model16 | (unsigned)(t * 100 + q), d.draw0, d.draw1};
  philox4x32_10(c, d.key0, d.key1);
  return (c[0] >= d.thr ? 1u : 0u) | (c[1] >= d.thr ? 2u : 0u) | (c[2] >= d.thr ? 4u : 0u) | (c[3] >= d.thr ? 8u : 0u);
}

// one element through the dropout: a correctly rounded division where kept (x / 1 is x, so rate -> 0 is the parent's bytes)
__device__ __forceinline__ float drop_apply(float v, unsigned keep, float keepf) { return keep ? v / keepf : 0.f; }

struct DropMaskArgs {
  DropArgs d;
  const unsigned* rows;                  // [b] set rows
  unsigned char* mask;                   // [b][T][400]
  int T;
  long long quads;                       // b * T * 100
};
// grid = ceil(b * T * 100 / 256): one thread per quad, its four bytes in one store
__global__ void __launch_bounds__(256) dropout_mask_kernel(const DropMaskArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.quads) return;
  const int per = a.T * 100;
  const int i = (int)(g / per), j = (int)(g % per), t = j / 100, q = j % 100;
  const unsigned k = drop_keep4(a.d, a.rows[i], t, q);
  *(unsigned*)(a.mask + (size_t)g * 4) = (k & 1u) | (k & 2u) << 7 | (k & 4u) << 14 | (k & 8u) << 21;
}

}  // namespace nrv
