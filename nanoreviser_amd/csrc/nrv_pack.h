// Device-side FASTA / FASTQ records of a merged call: the bytes of the output file, laid out behind the merge.
#pragma once
#include "nrv_merge.h"

namespace nrv {

// ---------------------------------------------------------------------------------------
// hoststage.pack_records is the DEFINITION; include/nanorev.h (nrv_revise_reads_raw_records_begin, nrv_pack_records) names the
// arguments.  Read r of a call owns blob[rec_off[r] .. rec_off[r + 1]), with L = off[r + 1] - off[r] and its name of
// nl = name_off[r + 1] - name_off[r] bytes:
//   FASTA  '>' name '\n' seq '\n'                        nl + L + 3 bytes
//   FASTQ  '@' name '\n' seq '\n' '+' '\n' qual '\n'     nl + 2 L + 6 bytes
// no line wrapping; a read without bases still has its record.  Two launches behind merge_scatter (and the report / edit
// launches) on the compute stream (pack_enqueue in nrv_api.hip), reading seq / qual / off as the merge left them:
//   pack_offsets (one workgroup: record lengths -> exclusive offsets, 256 reads at a time with a running carry, as
//   merge_tile_scan walks its tiles) -> pack_copy (the work follows the BYTES of the blob, not the reads: one thread per aligned
//   4-byte word, the read of its first byte found by binary search over rec_off, as merge_emit finds the read of an event).
// Store width: 32 bits.  A thread forms the four bytes of its word one by one (a word may span the end of one record and the
// heads of the following ones: a record that exists has at least 3 bytes) and writes them with ONE 4-byte store; the blob's
// base is 256-byte aligned.  The last word of the blob, when the total is no multiple of 4, is written byte by byte, so nothing at or beyond
// rec_off[n_reads] is touched.  Integers and copies only, no atomics, every byte written by exactly one thread and a function
// of its position alone: the bytes do not depend on the order of the workgroups, and a second pass accumulates nothing.
// The grid is sized from the host's bound `cap` on the blob; threads beyond rec_off[n_reads] (or beyond cap, whatever the
// offsets say) do nothing.  A pass of 256 record lengths is summed in 32 bits: the host declines a blob of 4 GiB and more.
// With `trim` (nrv_trim.h; hoststage.pack_records with trim / min_len) read r's record holds seq[lo:hi] (and qual[lo:hi]) of the
// read when hi - lo >= min_len, and a read below that is DROPPED: it has no record at all, rec_off[r + 1] == rec_off[r].
// rec_off is then ascending, not strictly so: pack_copy's search takes the LAST read with rec_off <= B, which is the one whose
// record holds byte B (rec_off[r + 1] > B), whether the empty records lie at the head, in runs in the middle or at the tail -
// and its walk to the next byte's record steps over every empty record in between.  trim == NULL: the whole reads, all of them.
// ---------------------------------------------------------------------------------------
struct PackArgs {
  int n_reads, fastq;
  const long long* off;                  // [n_reads + 1] the merge's read offsets into seq / qual
  const long long* name_off;             // [n_reads + 1] offsets into names
  const unsigned char* names;            // [name_off[n_reads]]
  const unsigned char *seq, *qual;       // the merged reads; qual is read only with fastq
  long long* rec_off;                    // [n_reads + 1] out
  unsigned char* blob;                   // [cap] out, 4-byte aligned
  unsigned long long cap;                // bytes the blob holds
  const long long* trim;                 // [n_reads][2] (lo, hi) inside each read, or null: the whole reads
  long long min_len;                     // with trim: a read with hi - lo below this has no record
};

// the part of read r that goes into its record: *s0 its first character in seq / qual, *L their number; false: no record
__device__ __forceinline__ bool pack_part(const PackArgs& a, const int r, long long* s0, long long* L) {
  *s0 = a.off[r]; *L = a.off[r + 1] - a.off[r];
  if (!a.trim) return true;
  const long long lo = a.trim[2 * r], hi = a.trim[2 * r + 1];
  if (lo < 0 || hi < lo || hi > *L) { *L = 0; return false; }       // (never from trim_finish: nothing outside the read is read)
  *s0 += lo; *L = hi - lo;
  return hi - lo >= a.min_len;
}

// One workgroup: per-read record lengths -> exclusive offsets, 256 at a time with a running carry; the total goes to rec_off[n_reads].
__global__ void __launch_bounds__(256) pack_offsets_kernel(const PackArgs a) {
  unsigned long long carry = 0;
  const unsigned q = a.fastq ? 2u : 1u;
  for (int b = 0; b < a.n_reads; b += 256) {
    const int r = b + threadIdx.x;
    unsigned v = 0;
    long long s0, L;
    if (r < a.n_reads && pack_part(a, r, &s0, &L)) v = (unsigned)(a.name_off[r + 1] - a.name_off[r]) + q * (unsigned)L + 3u * q;
    unsigned total;
    const unsigned before = merge_block_scan(v, &total);
    if (r < a.n_reads) a.rec_off[r] = (long long)(carry + before);
    carry += total;
  }
  if (threadIdx.x == 0) a.rec_off[a.n_reads] = (long long)carry;
}

// byte k of read r's record
__device__ __forceinline__ unsigned pack_byte(const PackArgs& a, const int r, long long k) {
  const long long n0 = a.name_off[r], nl = a.name_off[r + 1] - n0;
  long long s0, L;
  (void)pack_part(a, r, &s0, &L);
  if (k == 0) return a.fastq ? '@' : '>';
  k -= 1;
  if (k < nl) return a.names[n0 + k];
  k -= nl;
  if (k == 0) return '\n';
  k -= 1;
  if (k < L) return a.seq[s0 + k];
  k -= L;
  if (k == 0) return '\n';
  if (k == 1) return '+';                                 // (FASTQ from here on: a FASTA record has ended)
  if (k == 2) return '\n';
  k -= 3;
  if (k < L) return a.qual[s0 + k];
  return '\n';
}

__global__ void __launch_bounds__(256) pack_copy_kernel(const PackArgs a) {
  const unsigned long long B = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * 4;      // this thread's word of the blob
  unsigned long long total = (unsigned long long)a.rec_off[a.n_reads];
  if (total > a.cap) total = a.cap;
  if (B >= total) return;
  int r = 0, hi_r = a.n_reads - 1;                        // LAST read with rec_off <= B: rec_off[r + 1] > B, so its record holds B
  while (r < hi_r) {
    const int mid = (r + hi_r + 1) >> 1;
    if ((unsigned long long)a.rec_off[mid] <= B) r = mid; else hi_r = mid - 1;
  }
  unsigned word = 0;
  int nb = 0;
  for (int i = 0; i < 4 && B + i < total; ++i) {
    while (r + 1 < a.n_reads && (unsigned long long)a.rec_off[r + 1] <= B + i) ++r;
    word |= (pack_byte(a, r, (long long)(B + i) - a.rec_off[r]) & 255u) << (8 * i);
    nb = i + 1;
  }
  if (nb == 4) {
    *reinterpret_cast<unsigned*>(a.blob + B) = word;
  } else {
    for (int i = 0; i < nb; ++i) a.blob[B + i] = (unsigned char)(word >> (8 * i));
  }
}

}  // namespace nrv
