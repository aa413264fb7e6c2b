// Device-side error classes of a merged call's reads against a truth set: per read (d, M) of the original and of the revised read.
#pragma once
#include "nrv_align.h"

namespace nrv {

// ---------------------------------------------------------------------------------------
// hoststage.edit_classes is the DEFINITION; include/nanorev.h (nrv_revise_reads_raw_errclass_begin, nrv_edit_classes) names the
// arguments and the six columns.  For a truth t (m bytes) and a read s (n bytes), bytes matching as in nrv_align.h (equal, and
// one of A C G T): d = the minimum number of edits of a global alignment, M = the largest number of matched columns among the
// alignments with d edits.  W[0][j] = (j, 0), W[i][0] = (i, 0), W[i][j] = the lexicographic minimum on (d, -M) of
// W[i-1][j] + (1, 0), W[i][j-1] + (1, 0) and W[i-1][j-1] + ((0, -1) on a match, (1, 0) otherwise); (d, -M) = W[m][n].
// A cell is ONE signed 64-bit value (d << 32) - M: the lexicographic order is the order of the integers, a step that costs an
// edit adds kEdit = 1 << 32, a match subtracts 1.  Integers only; no traceback, no tie-break rule.
// One launch, LAST in a merged call behind align_kernel (errclass_enqueue in nrv_api.hip): one wave per (read, kind) pair as
// there.  This is a WAVEFRONT recurrence, not a bit-vector one: the truth lies down the lanes, lane b owns kErrclassR
// consecutive truth characters and their cells of the current column of W in registers; the read is the text, and lane b works
// on text column j at step j + b.  Its bottom cell and the text character move to lane b + 1 by __shfl_up; lane b + 1 keeps the
// cell it got one step earlier as its diagonal.  Lane 0 feeds the text (a chunk of 64 characters per coalesced load, handed out
// by readlane) and the table's first row (j + 1, 0).  64 lanes x kErrclassR = a stripe of kErrclassStripe truth characters; a
// stripe of B <= 64 lanes runs n + B - 1 steps.
// kErrclassR = 16: the cells of a lane update one after the other (each needs the one above), so a step costs kErrclassR times
// ~10 dependent vector instructions and the cross-lane moves are ~1/6 of it; 32 cells + 16 characters + the feed fit in well
// under 128 registers.  32 would halve the moves' share but use half the lanes on a truth of up to 1024 characters - the steps
// of a pair are m n / 64 cells per lane either way once the truth fills a stripe.
// A truth of more than one stripe: the same wave walks the stripes in turn.  The last lane of stripe k stores its bottom cell
// per text column into the pair's carry words hc (8 bytes per text character); lane 0 of stripe k + 1 reads them instead of
// the first row.  Stripe 0 reads nothing of hc - no byte is read that this launch did not write - and a device-scope fence
// stands between two stripes (the stores come from one lane, the loads from others).  Inside a stripe column j of hc is loaded
// (issued one chunk ahead, and waited for at step <= j) before it is overwritten (at step j + 63) for the stripe behind.
// Every stored word is a function of the pair alone: plain vector stores, no atomics, nothing accumulates - a second pass over
// the same block (the re-run of nrv_reads_raw_end) gives the same bytes whatever the order of the workgroups.
// Lengths, d and M are 32-bit in here: the entry points refuse a length of 2^31 - 64 and more.
// ---------------------------------------------------------------------------------------
constexpr int kErrclassCols = 6;
constexpr int kErrclassR = 16;                         // truth characters (and cells) per lane
constexpr int kErrclassStripe = 64 * kErrclassR;       // truth characters per stripe
constexpr long long kEdit = 1ll << 32;                 // one edit in a packed cell

struct ErrclassArgs : PairArgs {         // (nrv_align.h)
  long long *hc0, *hc1;                  // carry words, one per text character: hc0[ev_off + j], hc1[off[r] + j]
  unsigned long long* ecls;              // [n_reads][kErrclassCols] (kinds == 2)
  long long *dist, *match;               // [n_reads] each (kinds == 1): -1 / -1 for an empty truth
};

__global__ void __launch_bounds__(64) errclass_kernel(const ErrclassArgs a) {
  constexpr int R = kErrclassR;
  const int lane = threadIdx.x;
  const int r = (int)(blockIdx.x / (unsigned)a.kinds), kind = a.kinds == 2 ? (int)(blockIdx.x & 1u) : 1;
  if (r >= a.n_reads) return;
  const PairText p = pair_text(a, r, kind);
  const int m = p.m, n = p.n;
  if (m <= 0) {                                           // no truth: the row is zeros and nothing is formed
    if (lane == 0) {
      if (a.kinds == 2) {
        unsigned long long* row = a.ecls + (size_t)r * kErrclassCols + 3 * kind;
        row[0] = 0; row[1] = 0; row[2] = 0;
      } else {
        a.dist[r] = -1; a.match[r] = -1;
      }
    }
    return;
  }
  const unsigned char *t = p.t, *s = p.s;
  long long* hc = (kind == 0 ? a.hc0 : a.hc1) + p.at;
  long long res = 0;                                      // W[m][n], picked by the lane that owns row m
  int res_lane = 0;
  for (long long base = 0; base < m; base += kErrclassStripe) {
    const int rem = (int)(m - base);
    const int B = rem >= kErrclassStripe ? 64 : (rem + R - 1) / R;
    const bool last_stripe = rem <= kErrclassStripe;
    const bool first = base == 0;
    // the lane's strip: its own characters (-1: a byte that matches nothing) and column 0 of the table, W[i][0] = (i, 0)
    int valid = rem - lane * R;
    valid = valid < 0 ? 0 : (valid > R ? R : valid);
    int tc[R];
    long long w[R];
    const long long row0 = base + lane * R;                   // the table row above the strip
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const unsigned c = i < valid ? t[row0 + i] : 0u;
      tc[i] = (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? (int)c : -1;
      w[i] = (row0 + i + 1) * kEdit;
    }
    long long diag = row0 * kEdit;            // W[row0][j]: the cell got one step earlier
    long long send = 0;                                   // what the lane hands to the next: its bottom cell ...
    int send_c = 0;                                       // ... and the text character
    const int steps = n > 0 ? n + B - 1 : 0;
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
          long long above = up, dg = diag;                // W[i-1][j], W[i-1][j-1] while walking down the strip
#pragma unroll
          for (int k = 0; k < R; ++k) {
            const long long left = w[k];
            long long best = dg + ((c == tc[k]) ? -1ll : kEdit);
            const long long e = (above < left ? above : left) + kEdit;
            best = e < best ? e : best;
            dg = left;
            w[k] = best;
            above = best;
          }
          diag = up;
          send = w[R - 1];
          send_c = c;
          if (lane == B - 1 && !last_stripe) hc[j] = send;
        }
      }
    }
    if (last_stripe) {
      res_lane = B - 1;
      const int pick = rem - (B - 1) * R - 1;             // the strip cell of row m in lane B - 1
#pragma unroll
      for (int k = 0; k < R; ++k) res = k == pick ? w[k] : res;
    } else {
      __threadfence();                                    // the carry words: stored by lane 63, loaded by every lane
    }
  }
  res = __shfl(res, res_lane);
  if (lane == 0) {
    const unsigned M = 0u - (unsigned)(unsigned long long)res;
    const long long d = (res + (long long)M) >> 32;
    if (a.kinds == 2) {
      unsigned long long* row = a.ecls + (size_t)r * kErrclassCols;
      if (kind == 0) { row[0] = (unsigned long long)m; row[1] = (unsigned long long)d; row[2] = M; }
      else { row[3] = (unsigned long long)d; row[4] = M; row[5] = 0; }
    } else {
      a.dist[r] = d; a.match[r] = (long long)M;
    }
  }
}

}  // namespace nrv
