// Device-side per-read edit list of a merged call: which bases the merge changed, where, and with what confidence.
#pragma once
#include "nrv_merge.h"

namespace nrv {

// ---------------------------------------------------------------------------------------
// hoststage.revision_edits is the DEFINITION; include/nanorev.h (nrv_edit, nrv_revise_reads_raw_edits_begin) names the fields.
// A stream compaction in event order behind merge_scatter (edits_enqueue in nrv_api.hip), three launches shaped like the merge's:
//   edits_count (one thread per event: the edit flag and its tile's sum) -> edits_tile_scan (one workgroup walks the tile sums)
//   -> edits_scatter (one thread per event: the flag's scan inside the tile = the record's slot, the scan of the merge counts
//   in rec inside the tile + the merge's tile[] - which merge_scatter left as exclusive offsets - = the event's position in
//   seq, and minus off[r], which merge_scatter wrote earlier in stream order, pos_out).
// An event is an edit when its window says substituted (agree on another base), inserted (dele) or deleted (drop): the rules of
// report_kernel's columns 5 - 7.  Slots come from an exclusive scan of INTEGER flags over all events of the call, so the bytes
// do not depend on the order in which tiles run; no atomics.  One 16-byte store per record.  At most one record per window, and
// the windows of all reads are at most max(N - T, 0): the block of `cap` records always suffices (and no slot beyond it is
// written, whatever the descriptors say).
// ---------------------------------------------------------------------------------------
struct EditRec { unsigned pos_in, pos_out, bytes, conf; };   // nrv_edit: bytes = kind | ref << 8 | alt << 16 | qual << 24, conf = f32 bits
static_assert(sizeof(EditRec) == 16, "an edit record is 16 bytes");

struct EditsArgs {
  const SegRead* reads;
  int n_reads, T;
  long long N, cap;                      // events of the call; records the block holds = max(N - T, 0)
  const unsigned char* bases;            // [N]
  const signed char *a1, *a2;            // [N - T]
  const float *p1, *p2;                  // [N - T][6], [N - T][5]; both null: conf is 0
  const unsigned* rec;                   // [N] merge_emit's records
  const unsigned long long* tile;        // [tiles] the merge's exclusive tile offsets
  const long long* off;                  // [n_reads + 1] the merge's read offsets
  int want_q;                            // rec carries a quality (FASTQ): qual is filled
  unsigned long long* etile;             // [tiles] scratch: flag sums, then exclusive offsets
  long long* edit_off;                   // [n_reads + 1] out
  EditRec* edits;                        // [cap] out
};

// what one event is: its read, its index inside it, and - for an edit - kind (1 substituted, 2 inserted, 3 deleted; 0: none) and alt
struct EditEvent { int r; long long j, w; unsigned kind, alt; };

__device__ __forceinline__ EditEvent edits_classify(const EditsArgs& a, const long long E) {
  EditEvent ev{0, 0, 0, 0u, 0u};
  int lo_r = 0, hi_r = a.n_reads - 1;                     // last read with ev_off <= E
  while (lo_r < hi_r) {
    const int mid = (lo_r + hi_r + 1) >> 1;
    if (a.reads[mid].ev_off <= E) lo_r = mid; else hi_r = mid - 1;
  }
  const SegRead rd = a.reads[lo_r];
  const long long j = E - rd.ev_off, o = (a.T - 1) / 2;
  const long long n_r = rd.ev_len - a.T > 0 ? rd.ev_len - a.T : 0;
  ev.r = lo_r; ev.j = j;
  if (j >= o && j < o + n_r) {
    const long long w = E - o;
    const unsigned base = a.bases[E];
    const int x = a.a1[w], y = a.a2[w] + 1;
    const bool agree = x == y && x >= 2, dele = x == 0 && y >= 2, drop = x == 1 && y == 1;
    const int cx = x < 0 ? 0 : (x > 5 ? 5 : x), cy = y < 0 ? 0 : (y > 5 ? 5 : y);
    const unsigned long long lab = 0x414754432D44ull;     // "D-CTGA" (hoststage._LAB2CHR)
    auto chr = [&](int l) -> unsigned { return (unsigned)(lab >> (8 * l)) & 255u; };
    ev.w = w;
    if (agree) { if (chr(cx) != base) { ev.kind = 1; ev.alt = chr(cx); } }
    else if (dele) { ev.kind = 2; ev.alt = chr(cy); }
    else if (drop) { ev.kind = 3; ev.alt = '-'; }
  }
  return ev;
}

__global__ void __launch_bounds__(256) edits_count_kernel(const EditsArgs a) {
  const long long E = (long long)blockIdx.x * kMergeTile + threadIdx.x;
  unsigned flag = 0;
  if (E < a.N) flag = edits_classify(a, E).kind ? 1u : 0u;
  unsigned total;
  (void)merge_block_scan(flag, &total);
  if (threadIdx.x == 0) a.etile[blockIdx.x] = total;
}

// One workgroup: tile sums -> exclusive offsets, 256 at a time with a running carry; the total goes to edit_off[n_reads] and to
// the empty reads at the end of the call.
__global__ void __launch_bounds__(256) edits_tile_scan_kernel(const EditsArgs a, const int tiles) {
  unsigned long long carry = 0;
  for (int b = 0; b < tiles; b += 256) {
    const int i = b + threadIdx.x;
    const unsigned v = i < tiles ? (unsigned)a.etile[i] : 0u;     // a tile's sum is at most kMergeTile
    unsigned total;
    const unsigned before = merge_block_scan(v, &total);
    if (i < tiles) a.etile[i] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) {
    a.edit_off[a.n_reads] = (long long)carry;
    for (int r = a.n_reads - 1; r >= 0 && a.reads[r].ev_len == 0; --r) a.edit_off[r] = (long long)carry;
  }
}

__global__ void __launch_bounds__(256) edits_scatter_kernel(const EditsArgs a) {
  const long long E = (long long)blockIdx.x * kMergeTile + threadIdx.x;
  EditEvent ev{0, 0, 0, 0u, 0u};
  unsigned rec = 0;
  if (E < a.N) { ev = edits_classify(a, E); rec = a.rec[E]; }
  unsigned total;
  const unsigned slot_in = merge_block_scan(ev.kind ? 1u : 0u, &total);
  const unsigned pos_in_tile = merge_block_scan(rec & 3u, &total);
  if (E >= a.N) return;
  const long long slot = (long long)a.etile[blockIdx.x] + slot_in;
  if (ev.kind && slot < a.cap) {
    const long long pos = (long long)a.tile[blockIdx.x] + pos_in_tile;
    float conf = 0.f;
    if (a.p1) {                                           // merge_emit's operand, gathered as it gathers it
      const int c1 = a.a1[ev.w], c2 = a.a2[ev.w];
      const int g1 = c1 < 0 ? 0 : (c1 > 5 ? 5 : c1), g2 = c2 < 0 ? 0 : (c2 > 4 ? 4 : c2);
      const float u = a.p1[ev.w * 6 + g1], v = a.p2[ev.w * 5 + g2];
      conf = v < u ? v : u;
    }
    EditRec e;
    e.pos_in = (unsigned)ev.j;
    e.pos_out = (unsigned)(pos - a.off[ev.r]);
    e.bytes = ev.kind | (unsigned)a.bases[E] << 8 | ev.alt << 16 | (a.want_q ? rec >> 24 : 0u) << 24;
    e.conf = __float_as_uint(conf);
    *reinterpret_cast<uint4*>(a.edits + slot) = make_uint4(e.pos_in, e.pos_out, e.bytes, e.conf);
  }
  if (ev.j == 0) {                                        // first event of a read: its offset, and that of the empty reads in front of it
    a.edit_off[ev.r] = slot;
    for (int r = ev.r - 1; r >= 0 && a.reads[r].ev_len == 0; --r) a.edit_off[r] = slot;
  }
}

}  // namespace nrv
