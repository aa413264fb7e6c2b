// Device-side edit distance of a merged call's reads to a truth set: per read d(truth, original) and d(truth, revised).
#pragma once
#include "nrv_merge.h"

namespace nrv {

// ---------------------------------------------------------------------------------------
// hoststage.edit_distance is the DEFINITION; include/nanorev.h (nrv_revise_reads_raw_accuracy_begin, nrv_edit_distance) names
// the arguments and the four columns.  d(t, s) is the global unit-cost edit distance of a truth t (m bytes) and a read s
// (n bytes): D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + c), c = 0 exactly when
// t[i-1] == s[j-1] and that byte is one of A C G T - any other byte matches nothing, itself included.  Integers only.
// One launch, LAST in a merged call (align_enqueue in nrv_api.hip): one wave per (read, kind) pair, kind 0 = the original bases
// of the read, kind 1 = its merged characters seq[off[r] .. off[r + 1]).  The recurrence is Myers' bit-vector form in Hyyro's
// block version, laid out ACROSS the wave: the truth is the pattern, lane b owns 64 truth characters (Pv, Mv and the four
// match words of A / C / G / T in registers: a byte outside ACGT sets no bit), the read is the text, and lane b handles text
// column j at step j + b - the horizontal delta hout in {-1, 0, +1} of its block moves to lane b + 1 together with the text
// character in one __shfl_up per step.  64 lanes x 64 bits = a stripe of 4096 truth characters; a stripe of B <= 64 blocks
// runs n + B - 1 steps.  Lane 0 feeds the text (a chunk of 64 characters per coalesced load, handed out by readlane) and takes
// the constant +1 of D[0][j] in the first stripe.  In the last block of the truth only the low m - 64 (blocks - 1) bits are
// valid: hout is read at the last valid bit, the match words are 0 above it, and a carry only ever moves up.  The score is
// m + the sum of the last block's hout, kept by that block's lane.
// A truth of more than 4096 characters: the same wave walks the stripes in turn.  The last lane of stripe k stores its hout + 1
// per text column into the pair's carry bytes hc; lane 0 of stripe k + 1 reads them instead of the constant.  Stripe 0 reads
// nothing of hc - no byte is read that this launch did not write - and a device-scope fence stands between two stripes (the
// stores come from one lane, the loads from others).  Inside a stripe column j of hc is loaded (at step <= j, and waited for
// there) before it is overwritten (at step j + 63) for the stripe behind.
// Every stored word is a function of the pair alone: plain vector stores, no atomics, nothing accumulates - a second pass over
// the same block (the re-run of nrv_reads_raw_end) gives the same bytes whatever the order of the workgroups.
// Lengths and distances are 32-bit in here: the entry points refuse a length of 2^31 - 64 and more.
// ---------------------------------------------------------------------------------------
constexpr int kAccuracyCols = 4;
constexpr int kAlignStripe = 4096;       // truth characters per stripe: 64 lanes x 64 bits

// What align_kernel, errclass_kernel and infix_kernel share: the pairs, the truth and the two places a text can come from
struct PairArgs {
  int n_reads;                           // pairs of the unit door; reads of a merged call (kinds waves each; infix: x strands)
  int kinds;                             // 2: a merged call, one row per read; 1: the unit door (texts by off / seq alone), one array per figure
  const unsigned char* truth;
  const long long* truth_off;            // [n_reads + 1] ascending from 0
  const SegRead* reads;                  // kind 0: bases[ev_off .. ev_off + ev_len)
  const unsigned char* bases;
  const long long* off;                  // kind 1 (and the unit door): seq[off[r] .. off[r + 1])
  const unsigned char* seq;
  long long cap0, cap1;                  // characters bases / seq hold: a text that is not inside them counts as empty
};

// Pair (r, kind) resolved: the truth t (m bytes; m <= 0: no truth, and nothing of the text is read) and the text s (n bytes),
// which starts `at` characters into bases (kind 0) or seq (kind 1) - the pair's carry starts as far into its own array.  A
// text that is not inside cap0 / cap1, or longer than max_len, counts as empty and lies at 0
struct PairText {
  const unsigned char *t, *s;
  int m, n;
  long long at;
};
__device__ inline PairText pair_text(const PairArgs& a, int r, int kind, long long max_len = 0x7fffffffffffffffll) {
  PairText p;
  const long long t_at = a.truth_off[r];
  p.t = a.truth + t_at; p.m = (int)(a.truth_off[r + 1] - t_at);
  p.s = a.seq; p.n = 0; p.at = 0;
  if (p.m <= 0) return p;
  if (kind == 0) {
    const SegRead rd = a.reads[r];
    const bool ok = rd.ev_off >= 0 && rd.ev_len >= 0 && rd.ev_len <= max_len && rd.ev_off + rd.ev_len <= a.cap0;
    p.at = ok ? rd.ev_off : 0; p.s = a.bases + p.at; p.n = ok ? (int)rd.ev_len : 0;
  } else {
    const long long o0 = a.off[r], o1 = a.off[r + 1];
    const bool ok = o0 >= 0 && o1 >= o0 && o1 - o0 <= max_len && o1 <= a.cap1;
    p.at = ok ? o0 : 0; p.s = a.seq + p.at; p.n = ok ? (int)(o1 - o0) : 0;
  }
  return p;
}

struct AlignArgs : PairArgs {
  unsigned char *hc0, *hc1;              // carry bytes, one per text character: hc0[ev_off + j], hc1[off[r] + j]
  unsigned long long* accu;              // [n_reads][kAccuracyCols] (kinds == 2)
  long long* dist;                       // [n_reads] (kinds == 1): -1 for an empty truth
};

__global__ void __launch_bounds__(64) align_kernel(const AlignArgs a) {
  const int lane = threadIdx.x;
  const int r = (int)(blockIdx.x / (unsigned)a.kinds), kind = a.kinds == 2 ? (int)(blockIdx.x & 1u) : 1;
  if (r >= a.n_reads) return;
  const PairText p = pair_text(a, r, kind);
  const int m = p.m, n = p.n;
  if (m <= 0) {                                           // no truth: the row is zeros and no distance is formed
    if (lane == 0) {
      if (a.kinds == 2) {
        unsigned long long* row = a.accu + (size_t)r * kAccuracyCols + 2 * kind;
        row[0] = 0; row[1] = 0;
      } else {
        a.dist[r] = -1;
      }
    }
    return;
  }
  const unsigned char *t = p.t, *s = p.s;
  unsigned char* hc = (kind == 0 ? a.hc0 : a.hc1) + p.at;
  int score = 0;                                          // the sum of hout of the truth's last block (its lane only)
  int last_lane = 0;
  for (int base = 0; base < m; base += kAlignStripe) {
    const int rem = m - base;
    const int B = rem >= kAlignStripe ? 64 : (rem + 63) >> 6;
    const bool last_stripe = rem <= kAlignStripe;
    // the lane's block: the match words of its own 64 bytes
    int valid = rem - lane * 64;
    valid = valid < 0 ? 0 : (valid > 64 ? 64 : valid);
    unsigned long long pa = 0, pc = 0, pg = 0, pt = 0;
    for (int i = 0; i < valid; ++i) {
      const unsigned c = t[base + lane * 64 + i];
      const unsigned long long bit = 1ull << i;
      pa |= c == 'A' ? bit : 0ull; pc |= c == 'C' ? bit : 0ull; pg |= c == 'G' ? bit : 0ull; pt |= c == 'T' ? bit : 0ull;
    }
    const unsigned long long top = valid > 0 ? 1ull << (valid - 1) : 0ull;
    unsigned long long Pv = ~0ull, Mv = 0ull;             // D[i][0] = i: every vertical delta is +1
    const bool first = base == 0;
    const int steps = n > 0 ? n + B - 1 : 0;
    int carry = 0;                                        // what the lane hands to the next: character | (hout + 1) << 8
    // lane 0's feed, a chunk of 64 columns ahead: the text and (behind the first stripe) the carry bytes; 2 = the constant +1
    int txt_n = lane < n ? (int)s[lane] : 0;
    int hc_n = (!first && lane < n) ? (int)hc[lane] : 2;
    for (int s0 = 0; s0 < steps; s0 += 64) {
      const int txt = txt_n, hcv = hc_n;
      const int ahead = s0 + 64 + lane;
      txt_n = ahead < n ? (int)s[ahead] : 0;
      hc_n = (!first && ahead < n) ? (int)hc[ahead] : 2;
      const int lim = steps - s0 < 64 ? steps - s0 : 64;
      for (int i = 0; i < lim; ++i) {
        int in = __shfl_up(carry, 1);
        const int feed = __builtin_amdgcn_readlane(txt, i) | (__builtin_amdgcn_readlane(hcv, i) << 8);
        if (lane == 0) in = feed;
        const int j = s0 + i - lane;
        const bool act = lane < B && j >= 0 && j < n;
        const int c = in & 255, hin = ((in >> 8) & 3) - 1;
        unsigned long long Eq = c == 'A' ? pa : (c == 'C' ? pc : (c == 'G' ? pg : (c == 'T' ? pt : 0ull)));
        const unsigned long long Xv = Eq | Mv;
        if (hin < 0) Eq |= 1ull;
        const unsigned long long Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        unsigned long long Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
        const int hout = (Ph & top) ? 1 : ((Mh & top) ? -1 : 0);
        Ph <<= 1; Mh <<= 1;
        if (hin < 0) Mh |= 1ull; else if (hin > 0) Ph |= 1ull;
        if (act) {
          Pv = Mh | ~(Xv | Ph);
          Mv = Ph & Xv;
          carry = c | ((hout + 1) << 8);
          if (lane == B - 1) {
            if (last_stripe) score += hout; else hc[j] = (unsigned char)(hout + 1);
          }
        }
      }
    }
    last_lane = B - 1;
    if (!last_stripe) __threadfence();                    // the carry bytes: stored by lane 63, loaded by every lane
  }
  const int d = m + __shfl(score, last_lane);
  if (lane == 0) {
    if (a.kinds == 2) {
      unsigned long long* row = a.accu + (size_t)r * kAccuracyCols;
      if (kind == 0) { row[0] = (unsigned long long)m; row[1] = (unsigned long long)d; }
      else { row[2] = (unsigned long long)d; row[3] = 0; }
    } else {
      a.dist[r] = d;
    }
  }
}

}  // namespace nrv
