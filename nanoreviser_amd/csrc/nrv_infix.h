// Device-side infix alignment of a merged call's reads inside truth REGIONS, on both strands: per read and strand (d, M, start, end).
#pragma once
#include "nrv_errclass.h"

namespace nrv {

// ---------------------------------------------------------------------------------------
// hoststage.infix_classes is the DEFINITION; include/nanorev.h (nrv_revise_reads_raw_infix_begin, nrv_infix_classes) names the
// arguments and the eighteen columns.  For a truth region t (m bytes) and a read s (n bytes), bytes matching as in nrv_align.h
// (equal, and one of A C G T): among all substrings t[start:end] the fewest edits d of a global alignment with s, then the most
// matched columns M, then the largest start, then the smallest end.  On the reverse strand t is its reverse complement
// (A<->T, C<->G, any other byte matches nothing) and start / end count on that.  A cell is a triple (d, -M, -start) compared
// lexicographically: W[0][j] = (j, 0, 0), W[i][0] = (0, 0, -i) - a leading stretch of the region is free -, W[i][j] = the
// minimum of W[i-1][j] + (1, 0, 0), W[i][j-1] + (1, 0, 0) and W[i-1][j-1] + ((0, -1, 0) on a match, (1, 0, 0) otherwise); the
// result is the minimum over i of (W[i][n], i) - a trailing stretch is free too.  Row 0 never wins alone when m >= 1
// ((n, 0, -1) = W[1][n] at the worst is below (n, 0, 0)), so the rows of the strips are all there is to reduce.
// A cell is ONE signed 64-bit value d 2^42 - M 2^21 - start: the lexicographic order is the order of the integers, an edit
// adds kInfixEdit = 1 << 42, a match subtracts kInfixMatch = 1 << 21; both lengths are at most kInfixMaxLen = 2^21 - 1, which
// the entry points see to (the revised text is only known here: one longer than that counts as empty).  Integers only; no
// traceback.
// One launch, LAST in a merged call behind errclass_kernel (infix_enqueue in nrv_api.hip): one wave per (read, original |
// revised, forward | reverse) triple.  The layout is errclass_kernel's: the region lies down the lanes, lane b owns kInfixR
// consecutive region characters and their cells of the current column of W in registers; the read is the text, and lane b
// works on text column j at step j + b.  Its bottom cell and the text character move to lane b + 1 by __shfl_up; lane b + 1
// keeps the cell it got one step earlier as its diagonal.  Lane 0 feeds the text (a chunk of 64 characters per coalesced
// load, handed out by readlane) and the table's first row (j + 1) << 42.  64 lanes x kInfixR = a stripe of kInfixStripe region
// characters; a stripe of B <= 64 lanes runs n + B - 1 steps.  kInfixR = 16 for the reasons given in nrv_errclass.h: the
// registers and the dependent chain of a step are the same, the three differences are outside the chain:
//   * column 0 of a strip is -(row) per cell, not row edits;
//   * on the reverse strand a lane reads its characters mirrored (t[m - 1 - p] for position p) and complemented straight
//     from the region - there is no second copy of the truth;
//   * the final column is REDUCED, not picked: after its last step each lane holds W[i][n] of its rows, takes the minimum of
//     (cell, row) over its valid cells, a butterfly of __shfl_xor takes it across the wave, and a running minimum is kept
//     across the stripes (strictly below: the rows of a later stripe are larger).
// A region of more than one stripe: the same wave walks the stripes in turn.  The last lane of stripe k stores its bottom
// cell per text column into the triple's carry words hc (8 bytes per text character, a set per strand: two waves share a
// text); lane 0 of stripe k + 1 reads them instead of the first row.  Stripe 0 reads nothing of hc - no byte is read that this
// launch did not write - and a device-scope fence stands between two stripes (the stores come from one lane, the loads from
// others).  Inside a stripe column j of hc is loaded (issued one chunk ahead, and waited for at step <= j) before it is
// overwritten (at step j + 63) for the stripe behind.
// Every stored word is a function of the triple alone: plain vector stores, no atomics, nothing accumulates - a second pass
// over the same block (the re-run of nrv_reads_raw_end) gives the same bytes whatever the order of the workgroups.  The wave
// of (kind, forward) stores the zeros of (kind, reverse) when one strand is run, the wave of (original, forward) columns 0, 1.
// n = 0 stores (0, 0, m, m) without a step; m = 0 is "no truth": zeros (the unit door: -1 in all four).
// ---------------------------------------------------------------------------------------
constexpr int kInfixCols = 18;
constexpr int kInfixR = 16;                            // region characters (and cells) per lane
constexpr int kInfixStripe = 64 * kInfixR;             // region characters per stripe
constexpr int kInfixMaxLen = (1 << 21) - 1;            // of a region and of a read: M and start have 21 bits each
constexpr long long kInfixEdit = 1ll << 42;            // one edit in a packed cell
constexpr long long kInfixMatch = 1ll << 21;           // one matched column

struct InfixArgs : PairArgs {            // (nrv_align.h)
  int strands;                           // a merged call: 1 or 2 waves per (read, kind); the unit door: 1
  int reverse;                           // the unit door's strand
  long long *hc0, *hc1;                  // carry words, one per text character and strand: hc0[rev * hs0 + ev_off + j], hc1[rev * hs1 + off[r] + j]
  long long hs0, hs1;                    // words between the forward and the reverse strand's carry words
  unsigned long long* infx;              // [n_reads][kInfixCols] (kinds == 2)
  long long *dist, *match, *start, *end; // [n_reads] each (kinds == 1): -1 in all four for an empty truth
};

// the four figures of a triple to where they belong (one lane)
__device__ inline void infix_store(const InfixArgs& a, int r, int kind, int rev, long long m, long long d, long long M, long long st, long long en) {
  if (a.kinds == 2) {
    unsigned long long* row = a.infx + (size_t)r * kInfixCols;
    if (kind == 0 && rev == 0) { row[0] = (unsigned long long)m; row[1] = m > 0 ? (unsigned long long)a.strands : 0ull; }
    unsigned long long* g = row + 2 + 4 * (2 * kind + rev);
    g[0] = (unsigned long long)d; g[1] = (unsigned long long)M; g[2] = (unsigned long long)st; g[3] = (unsigned long long)en;
    if (a.strands == 1) { g[4] = 0; g[5] = 0; g[6] = 0; g[7] = 0; }     // the reverse group of this kind: not run
  } else {
    a.dist[r] = d; a.match[r] = M; a.start[r] = st; a.end[r] = en;
  }
}

__global__ void __launch_bounds__(64) infix_kernel(const InfixArgs a) {
  constexpr int R = kInfixR;
  const int lane = threadIdx.x;
  const unsigned per = (unsigned)(a.kinds * a.strands);
  const int r = (int)(blockIdx.x / per), sub = (int)(blockIdx.x % per);
  if (r >= a.n_reads) return;
  const int kind = a.kinds == 2 ? sub / a.strands : 1;
  const int rev = a.kinds == 2 ? sub % a.strands : (a.reverse != 0);
  const PairText p = pair_text(a, r, kind, kInfixMaxLen);
  const int m = p.m, n = p.n;
  if (m <= 0) {                                           // no truth: zeros (the unit door: -1) and nothing is formed
    if (lane == 0) {
      const long long v = a.kinds == 2 ? 0 : -1;
      infix_store(a, r, kind, rev, 0, v, v, v, v);
    }
    return;
  }
  const unsigned char *t = p.t, *s = p.s;
  long long* hc = (kind == 0 ? a.hc0 + (rev ? a.hs0 : 0) : a.hc1 + (rev ? a.hs1 : 0)) + p.at;
  if (n == 0) {                                           // nothing to place: the empty substring at the region's end
    if (lane == 0) infix_store(a, r, kind, rev, m, 0, 0, m, m);
    return;
  }
  long long res = 0x7fffffffffffffffll;                   // the running minimum of (W[i][n], i) over the stripes
  int res_row = 0;
  for (long long base = 0; base < m; base += kInfixStripe) {
    const int rem = (int)(m - base);
    const int B = rem >= kInfixStripe ? 64 : (rem + R - 1) / R;
    const bool last_stripe = rem <= kInfixStripe;
    const bool first = base == 0;
    // the lane's strip: its own characters of the strand (-1: a byte that matches nothing) and column 0, W[i][0] = (0, 0, -i)
    int valid = rem - lane * R;
    valid = valid < 0 ? 0 : (valid > R ? R : valid);
    int tc[R];
    long long w[R];
    const int row0 = (int)base + lane * R;                    // the table row above the strip
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int p = row0 + i;                                 // the position on the strand; mirrored on the reverse one
      const unsigned c = i < valid ? t[rev ? m - 1 - p : p] : 0u;
      const int fw = (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? (int)c : -1;
      const int rc = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : -1;
      tc[i] = rev ? rc : fw;
      w[i] = -(long long)(row0 + i + 1);
    }
    long long diag = -(long long)row0;                    // W[row0][j]: the cell got one step earlier
    long long send = 0;                                   // what the lane hands to the next: its bottom cell ...
    int send_c = 0;                                       // ... and the text character
    const int steps = n + B - 1;
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
          up = first ? (long long)(s0 + i + 1) * kInfixEdit : (long long)(((unsigned long long)f_hi << 32) | f_lo);
        }
        const int j = s0 + i - lane;
        if (lane < B && j >= 0 && j < n) {
          long long above = up, dg = diag;                // W[i-1][j], W[i-1][j-1] while walking down the strip
#pragma unroll
          for (int k = 0; k < R; ++k) {
            const long long left = w[k];
            long long best = dg + ((c == tc[k]) ? -kInfixMatch : kInfixEdit);
            const long long e = (above < left ? above : left) + kInfixEdit;
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
    // the final column: the lane's minimum of (W[i][n], i) over its valid rows, then the wave's
    long long bc = 0x7fffffffffffffffll;
    int br = 0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const bool take = k < valid && w[k] < bc;           // strictly below: the smaller row stays
      bc = take ? w[k] : bc;
      br = take ? row0 + k + 1 : br;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long oc = __shfl_xor(bc, o);
      const int orow = __shfl_xor(br, o);
      const bool take = oc < bc || (oc == bc && orow < br);
      bc = take ? oc : bc;
      br = take ? orow : br;
    }
    if (bc < res) { res = bc; res_row = br; }
    if (!last_stripe) __threadfence();                    // the carry words: stored by lane 63, loaded by every lane
  }
  if (lane == 0) {
    const long long d = (res + kInfixEdit - 1) >> 42;
    const long long rest = d * kInfixEdit - res;          // M 2^21 + start
    infix_store(a, r, kind, rev, m, d, rest >> 21, rest & (long long)kInfixMaxLen, res_row);
  }
}

}  // namespace nrv
