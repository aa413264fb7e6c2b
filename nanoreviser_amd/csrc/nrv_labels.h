// Device-side per-base training labels: the truth alignment of a read inside its region WITH its traceback - per read base a label byte, per pair seven figures.
#pragma once
#include "nrv_infix.h"

namespace nrv {

// ---------------------------------------------------------------------------------------
// hoststage.align_labels is the DEFINITION; include/nanorev.h (nrv_align_labels) names the arguments, the bits of a label byte
// and the seven columns.  For a region t (m bytes), a read s (n bytes), a strand and bounds 0 <= start <= end <= m:
// u = strand(t)[start:end], L = end - start bytes (the strand as in nrv_infix.h), and the recurrence is nrv_errclass.h's on
// (u, s) - G[0][j] = (j, 0), G[i][0] = (i, 0), a packed cell (d << 32) - M - with the three candidates kept apart: 0 the
// diagonal, 1 "I" (the read character alone, from G[i][j-1]), 2 "D" (the truth character alone, from G[i-1][j]); dir[i][j] is
// the FIRST of them, in this order, that attains the minimum.  The path walks back from (L, n): I where i == 0, D where
// j == 0, dir[i][j] otherwise.
// Two launches per batch of pairs, the second behind the first on one stream (labels_enqueue in nrv_api.hip):
//   labels_kernel       the forward pass: errclass_kernel's wavefront, unchanged in shape - one wave per pair, lane b owns
//                       kLabelsR = 16 rows of u and their cells of the current column in registers, works on text column j at
//                       step j + b, hands its bottom cell and the text character to lane b + 1 by __shfl_up; lane 0 feeds the
//                       text in chunks of 64 characters and the first row; a u of more than kLabelsStripe characters is walked
//                       stripe by stripe through the carry words hc with a device-scope fence between two stripes.  Added:
//                       the lane reads its characters from t + start, mirrored and complemented on the reverse strand as
//                       infix_kernel does; inside the k loop the 2-bit dir of each of the 16 cells is shifted into ONE 32-bit
//                       word per lane and step; that word is stored with a plain vector store.
//   labels_walk_kernel  one THREAD per pair walks back from (L, n), stores labels[j] by index (no compaction), carries "the
//                       column just visited was D", counts the seven figures and stores them.  What it reads of the direction
//                       words becomes visible by the launch boundary, not by a fence inside a wave.
// The direction words of a pair lie [stripe][step][lane] (the layout CHOSEN; the other candidate, [stripe][lane][column], was
// not tried): the word of cell (i, j), p = i - 1, is at ((p / kLabelsStripe) (n + 63) + (j - 1) + lane) 64 + lane with
// lane = (p % kLabelsStripe) / kLabelsR, its bits at 2 (p % kLabelsR).  Why this one: the forward pass is where the work is -
// L n / 16 words are stored, the walk loads about L + n of them - and here the 64 words of a step are ONE 256-byte store of
// the wave, where the other layout scatters every store over 64 rows (n + 63) words apart.  The price is the walk's: a
// diagonal move changes the step by one and the row's bits by two, so its consecutive loads are 256 bytes apart (the same
// 16 rows of one lane: 16 loads in 16 different lines).  Neither kernel has been timed.  A pair takes
// ceil(L / kLabelsStripe) (n + 63) 256 bytes; the indices are 64-bit (64 stripes x 65599 steps x 64 words at the most).
// Every word the walk reads is written by the forward launch of the same batch: cell (i, j) with 1 <= i <= L, 1 <= j <= n
// belongs to an ACTIVE (lane, step) - lane < B, 0 <= step - lane < n - and an active lane stores its word at every such step.
// The cells of a partly valid strip (rows beyond L) write bits that nobody reads; steps at which a lane is idle write nothing.
// No atomics, nothing accumulates: a second pass over the same block gives the same bytes.  The walk takes a word's value 3
// (never written) for a diagonal, so it ends after at most L + n moves inside its arrays whatever the words hold.
// Lengths are 32-bit in here: the entry point refuses a read, or an end - start, above kLabelsMaxLen and a region of
// 2^31 - 64 bytes and more.  n = 0, L = 0 and m = 0 (no truth: zero bytes, -1 in the seven columns) need no forward pass.
// ---------------------------------------------------------------------------------------
constexpr int kLabelCols = 7;
constexpr int kLabelsMaxLen = 65536;                   // of a read and of end - start
constexpr int kLabelsR = kErrclassR;                   // rows of u (and cells) per lane: 16 x 2 bits = one word
constexpr int kLabelsStripe = 64 * kLabelsR;           // rows per stripe
constexpr size_t kLabelsBudget = (size_t)2 << 30;      // bytes of direction words per batch of pairs (a pair alone if it needs more)
static_assert(kLabelsR == 16, "a lane's directions of one step fill one 32-bit word");

struct LabelsArgs {
  int pair0, n_pairs;                    // the batch: pairs pair0 .. pair0 + n_pairs - 1 (one wave / one thread each)
  const unsigned char* truth;            // the regions
  const long long* truth_off;            // [pairs + 1] ascending from 0
  const unsigned char* seq;              // the reads
  const long long* off;                  // [pairs + 1] ascending from 0
  const unsigned char* reverse;          // [pairs] 0 or 1
  const long long *start, *end;          // [pairs] 0 <= start <= end <= m
  long long* hc;                         // carry words, one per read character: hc[off[r] + j]
  unsigned* dirw;                        // the batch's direction words ...
  const long long* dir_off;              // ... [pairs]: those of pair r begin at dirw[dir_off[r]]
  unsigned char* labels;                 // [off[pairs]]
  long long* summary;                    // [pairs][kLabelCols]
};

// the character of the strand at position q of the region's strand: -1 for a byte that matches nothing; raw: the byte itself
// after the complement (what the label's code is taken from)
__device__ inline int labels_char(const unsigned char* t, int m, int rev, int q, int* raw) {
  const unsigned c = t[rev ? m - 1 - q : q];
  const int fw = (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? (int)c : -1;
  const int rc = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : -1;
  const int v = rev ? rc : fw;
  if (raw) *raw = v < 0 ? (int)c : v;
  return v;
}

__global__ void __launch_bounds__(64) labels_kernel(const LabelsArgs a) {
  constexpr int R = kLabelsR;
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= a.n_pairs) return;
  const int r = a.pair0 + (int)blockIdx.x;
  const long long t_at = a.truth_off[r];
  const int m = (int)(a.truth_off[r + 1] - t_at);
  const int st = (int)a.start[r];
  const int L = (int)(a.end[r] - a.start[r]);
  const int n = (int)(a.off[r + 1] - a.off[r]);
  if (m <= 0 || L <= 0 || n <= 0) return;                 // no cell with i, j >= 1: the walk needs no word
  const int rev = a.reverse[r] != 0;
  const unsigned char* t = a.truth + t_at;
  const unsigned char* s = a.seq + a.off[r];
  long long* hc = a.hc + a.off[r];
  unsigned* dw = a.dirw + a.dir_off[r];
  const long long per_stripe = ((long long)n + 63) * 64;  // words
  for (int base = 0, sidx = 0; base < L; base += kLabelsStripe, ++sidx) {
    const int rem = L - base;
    const int B = rem >= kLabelsStripe ? 64 : (rem + R - 1) / R;
    const bool last_stripe = rem <= kLabelsStripe;
    const bool first = base == 0;
    // the lane's strip: its own characters of the strand (-1: a byte that matches nothing) and column 0, G[i][0] = (i, 0)
    int valid = rem - lane * R;
    valid = valid < 0 ? 0 : (valid > R ? R : valid);
    int tc[R];
    long long w[R];
    const int row0 = base + lane * R;                         // the table row above the strip
#pragma unroll
    for (int i = 0; i < R; ++i) {
      tc[i] = i < valid ? labels_char(t, m, rev, st + row0 + i, nullptr) : -1;
      w[i] = (long long)(row0 + i + 1) * kEdit;
    }
    long long diag = (long long)row0 * kEdit;             // G[row0][j]: the cell got one step earlier
    long long send = 0;                                   // what the lane hands to the next: its bottom cell ...
    int send_c = 0;                                       // ... and the text character
    const int steps = n + B - 1;
    unsigned* dws = dw + (long long)sidx * per_stripe + lane;
    // lane 0's feed, a chunk of 64 columns ahead: the text and (behind the first stripe) the carry words
    int txt_n = lane < n ? (int)s[lane] : 0;
    long long hc_n = (!first && lane < n) ? hc[lane] : 0;
    for (int s0 = 0; s0 < steps; s0 += 64) {
      const int txt = txt_n;
      const long long hcv = hc_n;
      const int ahead = s0 + 64 + lane;
      txt_n = ahead < n ? (int)s[ahead] : 0;
      hc_n = (!first && ahead < n) ? hc[ahead] : 0;
      const int lim = steps - s0 < 64 ? steps - s0 : 64;
      for (int i = 0; i < lim; ++i) {
        long long up = __shfl_up(send, 1);
        int c = __shfl_up(send_c, 1);
        const int f_c = __builtin_amdgcn_readlane(txt, i);
        const unsigned f_lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)hcv, i);
        const unsigned f_hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)hcv >> 32), i);
        if (lane == 0) {
          c = f_c;
          up = first ? (long long)(s0 + i + 1) * kEdit : (long long)(((unsigned long long)f_hi << 32) | f_lo);
        }
        const int j = s0 + i - lane;
        if (lane < B && j >= 0 && j < n) {
          long long above = up, dg = diag;                // G[i-1][j], G[i-1][j-1] while walking down the strip
          unsigned word = 0;
#pragma unroll
          for (int k = 0; k < R; ++k) {
            const long long left = w[k];
            const long long c0 = dg + ((c == tc[k]) ? -1ll : kEdit);
            const bool i_first = left <= above;           // I stands before D
            const long long e = (i_first ? left : above) + kEdit;
            const bool d_first = c0 <= e;                 // the diagonal before both
            const long long best = d_first ? c0 : e;
            word |= (d_first ? 0u : (i_first ? 1u : 2u)) << (2 * k);
            dg = left;
            w[k] = best;
            above = best;
          }
          diag = up;
          send = w[R - 1];
          send_c = c;
          dws[(long long)(s0 + i) * 64] = word;           // [stripe][step][lane]: the wave's words of a step are one 256-byte store
          if (lane == B - 1 && !last_stripe) hc[j] = send;
        }
      }
    }
    if (!last_stripe) __threadfence();                    // the carry words: stored by lane 63, loaded by every lane
  }
}

__global__ void __launch_bounds__(64) labels_walk_kernel(const LabelsArgs a) {
  const int q = (int)(blockIdx.x * 64u + threadIdx.x);
  if (q >= a.n_pairs) return;
  const int r = a.pair0 + q;
  const long long t_at = a.truth_off[r];
  const int m = (int)(a.truth_off[r + 1] - t_at);
  const int n = (int)(a.off[r + 1] - a.off[r]);
  unsigned char* lab = a.labels + a.off[r];
  long long* out = a.summary + (size_t)r * kLabelCols;
  if (m <= 0) {                                           // no truth: zero bytes, -1 in the seven columns
    for (int j = 0; j < n; ++j) lab[j] = 0;
    for (int k = 0; k < kLabelCols; ++k) out[k] = -1;
    return;
  }
  const int st = (int)a.start[r];
  const int L = (int)(a.end[r] - a.start[r]);
  const int rev = a.reverse[r] != 0;
  const unsigned char* t = a.truth + t_at;
  const unsigned char* s = a.seq + a.off[r];
  const unsigned* dw = a.dirw + a.dir_off[r];
  const long long per_stripe = ((long long)n + 63) * 64;
  long long match = 0, sub = 0, ins = 0, del = 0, lead = 0, run = 0, clip_end = -1;
  unsigned was_d = 0;
  int i = L, j = n;
  while (i > 0 || j > 0) {
    unsigned mv;
    if (i == 0) mv = 1;
    else if (j == 0) mv = 2;
    else {
      const int p = i - 1, in = p % kLabelsStripe, ln = in / kLabelsR;
      const long long at = (long long)(p / kLabelsStripe) * per_stripe + ((long long)(j - 1) + ln) * 64 + ln;
      mv = (dw[at] >> (2 * (in % kLabelsR))) & 3u;
    }
    if (mv == 2) {                                        // D: the truth character alone
      ++del; lead += j == 0; was_d = 16; --i;
    } else if (mv == 1) {                                 // I: the read character alone
      lab[j - 1] = (unsigned char)(1u | was_d);
      ++ins; ++run; was_d = 0; --j;
    } else {                                              // the diagonal
      int raw;
      const int c = labels_char(t, m, rev, st + i - 1, &raw);
      const bool hit = c == (int)s[j - 1];
      const unsigned code = raw == 'A' ? 5u : raw == 'G' ? 4u : raw == 'T' ? 3u : raw == 'C' ? 2u : 0u;
      lab[j - 1] = (unsigned char)(code | (hit ? 0u : 8u) | was_d);
      match += hit; sub += !hit;
      if (clip_end < 0) clip_end = run;
      run = 0; was_d = 0; --i; --j;
    }
  }
  out[0] = match; out[1] = sub; out[2] = ins; out[3] = del;
  out[4] = clip_end >= 0 ? run : n; out[5] = clip_end >= 0 ? clip_end : 0; out[6] = lead;
}

}  // namespace nrv
