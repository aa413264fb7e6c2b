// The block layouts of csrc/nrv_block.h as text, for tests/test_block_layout_host.py: one request per line on standard input -
// a layout's name and its arguments as decimal numbers -, one answer per line: the layout's offsets and its total as name=value.
// Plain C++ with a main of its own: the test builds it with AddressSanitizer and UndefinedBehaviorSanitizer and runs it directly.
#include "../nanoreviser_amd/csrc/nrv_block.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace nrv;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    std::vector<size_t> v;
    for (unsigned long long x; in >> x;) v.push_back((size_t)x);
    auto need = [&](size_t n) { return v.size() == n; };
    if (what == "pair" && need(5) && v[4] <= (size_t)kPairMaxOuts) {          // n_pairs ta tb carry k
      const PairLayout l = pair_layout(v[0], v[1], v[2], v[3], (int)v[4]);
      std::printf("a_off=%zu b_off=%zu a=%zu b=%zu hc=%zu", l.a_off, l.b_off, l.a, l.b, l.hc);
      for (size_t q = 0; q < v[4]; ++q) std::printf(" out%zu=%zu", q, l.out[q]);
      std::printf(" bytes=%zu\n", l.bytes);
    } else if (what == "trim" && need(2)) {                                    // n_reads total
      const TrimLayout l = trim_layout(v[0], v[1]);
      std::printf("off=%zu qual=%zu acc=%zu trim=%zu bytes=%zu\n", l.off, l.qual, l.acc, l.trim, l.bytes);
    } else if (what == "record" && need(6)) {                                  // n_reads name_bytes total fastq cap trim
      const RecordLayout l = record_layout(v[0], v[1], v[2], v[3] != 0, v[4], v[5] != 0);
      std::printf("off=%zu name_off=%zu names=%zu seq=%zu qual=%zu rec_off=%zu blob=%zu trim=%zu bytes=%zu\n", l.off, l.name_off,
                  l.names, l.seq, l.qual, l.rec_off, l.blob, l.trim, l.bytes);
    } else if (what == "labels" && need(5)) {                                  // n_pairs ta tb cols max_words
      const LabelsLayout l = labels_layout(v[0], v[1], v[2], v[3], v[4]);
      std::printf("a_off=%zu b_off=%zu start=%zu end=%zu dir_off=%zu reverse=%zu a=%zu b=%zu hc=%zu labels=%zu summary=%zu dir=%zu bytes=%zu\n",
                  l.a_off, l.b_off, l.start, l.end, l.dir_off, l.reverse, l.a, l.b, l.hc, l.labels, l.summary, l.dir, l.bytes);
    } else if (what == "merge_in" && need(10)) {             // n_reads desc N n have_p records name_bytes truth truth_bytes merged
      const MergeInLayout l = merge_in_layout(v[0], v[1], v[2], v[3], v[4] != 0, v[5] != 0, v[6], v[7] != 0, v[8], v[9]);
      std::printf("reads=%zu bases=%zu a1=%zu a2=%zu p1=%zu p2=%zu name_off=%zu names=%zu truth_off=%zu truth=%zu merged=%zu bytes=%zu\n",
                  l.reads, l.bases, l.a1, l.a2, l.p1, l.p2, l.name_off, l.names, l.truth_off, l.truth, l.merged, l.bytes);
    } else if (what == "carry" && need(4)) {                                   // N cap word sets
      const CarryLayout l = carry_layout(v[0], v[1], v[2], v[3]);
      std::printf("hc1=%zu hs0=%zu hs1=%zu bytes=%zu\n", l.hc1, l.hs0, l.hs1, l.bytes);
    } else if (what == "up256" && need(1)) {
      std::printf("up256=%zu\n", up256(v[0]));
    } else {
      std::fprintf(stderr, "block_layout_main: bad request: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
