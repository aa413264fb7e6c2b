// Host-side layouts of the device blocks the entry points of nrv_api.hip allocate: plain C++, no HIP, so that every offset and
// every size can be checked on a CPU (tests/test_block_layout_host.py) - a region too small is an out-of-bounds store on the device.
#pragma once
#include <cstddef>

namespace nrv {

// every region of every block starts on a multiple of 256 bytes
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// A block under construction: regions come out in the order they are taken.  take(n) = where a region of n bytes starts; a
// region of 0 bytes takes nothing and starts where the next one does
struct Block {
  size_t bytes = 0;
  size_t take(size_t n) {
    const size_t at = bytes;
    bytes += up256(n);
    return at;
  }
};

// nrv_edit_distance / nrv_edit_classes / nrv_infix_classes: [a_off | b_off | a | b | carry | k outputs of int64[n_pairs]].
// ta / tb: the bytes of a / b; the carry has `carry` bytes per character of b (align_kernel 1, errclass_kernel and infix_kernel 8)
constexpr int kPairMaxOuts = 4;
struct PairLayout { size_t a_off, b_off, a, b, hc, out[kPairMaxOuts], bytes; };
inline PairLayout pair_layout(size_t n_pairs, size_t ta, size_t tb, size_t carry, int k) {
  Block blk;
  PairLayout l{};
  l.a_off = blk.take((n_pairs + 1) * 8); l.b_off = blk.take((n_pairs + 1) * 8);
  l.a = blk.take(ta); l.b = blk.take(tb);
  l.hc = blk.take(tb * carry);
  for (int q = 0; q < k && q < kPairMaxOuts; ++q) l.out[q] = blk.take(n_pairs * 8);
  l.bytes = blk.bytes;
  return l;
}

// nrv_trim_reads: [off | qual | acc | trim]; total: the bytes of qual; acc and trim are two 64-bit words per read
struct TrimLayout { size_t off, qual, acc, trim, bytes; };
inline TrimLayout trim_layout(size_t n_reads, size_t total) {
  Block blk;
  TrimLayout l{};
  l.off = blk.take((n_reads + 1) * 8);
  l.qual = blk.take(total);
  l.acc = blk.take(n_reads * 16); l.trim = blk.take(n_reads * 16);
  l.bytes = blk.bytes;
  return l;
}

// nrv_pack_records_trim: [off | name_off | names | seq | qual | rec_off | blob | trim]; qual only for FASTQ, trim only with
// bounds; cap: the bytes the records can take (blob_capacity)
struct RecordLayout { size_t off, name_off, names, seq, qual, rec_off, blob, trim, bytes; };
inline RecordLayout record_layout(size_t n_reads, size_t name_bytes, size_t total, bool fastq, size_t cap, bool trim) {
  Block blk;
  RecordLayout l{};
  l.off = blk.take((n_reads + 1) * 8); l.name_off = blk.take((n_reads + 1) * 8);
  l.names = blk.take(name_bytes);
  l.seq = blk.take(total); l.qual = blk.take(fastq ? total : 0);
  l.rec_off = blk.take((n_reads + 1) * 8);
  l.blob = blk.take(cap);
  l.trim = blk.take(trim ? n_reads * 16 : 0);
  l.bytes = blk.bytes;
  return l;
}

// nrv_align_labels: [a_off | b_off | start | end | dir_off | reverse | a | b | hc | labels | summary | direction words]; hc:
// 8 bytes per character of b, labels 1; cols: the int64 columns of a summary row; max_words: the 32-bit direction words of
// the largest batch
struct LabelsLayout { size_t a_off, b_off, start, end, dir_off, reverse, a, b, hc, labels, summary, dir, bytes; };
inline LabelsLayout labels_layout(size_t n_pairs, size_t ta, size_t tb, size_t cols, size_t max_words) {
  Block blk;
  LabelsLayout l{};
  l.a_off = blk.take((n_pairs + 1) * 8); l.b_off = blk.take((n_pairs + 1) * 8);
  l.start = blk.take(n_pairs * 8); l.end = blk.take(n_pairs * 8); l.dir_off = blk.take(n_pairs * 8);
  l.reverse = blk.take(n_pairs);
  l.a = blk.take(ta); l.b = blk.take(tb);
  l.hc = blk.take(tb * 8);
  l.labels = blk.take(tb);
  l.summary = blk.take(n_pairs * cols * 8);
  l.dir = blk.take(max_words * 4);
  l.bytes = blk.bytes;
  return l;
}

// nrv_merge_calls*: [reads | bases | a1 | a2 | p1 | p2 | name_off | names | truth_off | truth | labels | merged block].  desc: the
// bytes of a read's descriptor; N events, n windows; p1 / p2 (24 and 20 bytes a window) only where the rows go up, the names only
// for records, the truth only where one is asked for, the labels (one byte per event) only for the score; merged: the bytes of
// the merged block (MergeLayout)
struct MergeInLayout { size_t reads, bases, a1, a2, p1, p2, name_off, names, truth_off, truth, merged, bytes, labels; };
inline MergeInLayout merge_in_layout(size_t n_reads, size_t desc, size_t N, size_t n, bool have_p, bool records, size_t name_bytes,
                                     bool truth, size_t truth_bytes, size_t merged, bool labels = false) {
  Block blk;
  MergeInLayout l{};
  l.reads = blk.take(n_reads * desc);
  l.bases = blk.take(N);
  l.a1 = blk.take(n); l.a2 = blk.take(n);
  l.p1 = blk.take(have_p ? n * 24 : 0); l.p2 = blk.take(have_p ? n * 20 : 0);
  l.name_off = blk.take(records ? (n_reads + 1) * 8 : 0); l.names = blk.take(records ? name_bytes : 0);
  l.truth_off = blk.take(truth ? (n_reads + 1) * 8 : 0); l.truth = blk.take(truth ? truth_bytes : 0);
  l.labels = blk.take(labels ? N : 0);
  l.merged = blk.take(merged);
  l.bytes = blk.bytes;
  return l;
}

// The stripe carries of a merged call inside its merged block: `sets` of [N words] for the original reads, then `sets` of
// [cap words] for the revised ones, a word being `word` bytes (align_kernel 1, errclass_kernel 8, infix_kernel 8 and a set per
// strand).  hs0 / hs1: the bytes from one set to the next; hc1: where the revised reads' carries start
struct CarryLayout { size_t hc1, hs0, hs1, bytes; };
inline CarryLayout carry_layout(size_t N, size_t cap, size_t word, size_t sets) {
  CarryLayout l{};
  l.hs0 = up256(N * word); l.hs1 = up256(cap * word);
  l.hc1 = sets * l.hs0;
  l.bytes = sets * (l.hs0 + l.hs1);
  return l;
}

}  // namespace nrv
