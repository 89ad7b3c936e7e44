// edlib_host_check.cpp -- the host side of the aligner pair.hip, fs.hip and gfa.hip share
// (canu_amd/csrc/edlib_host.h) as a program of its own, built with -fsanitize=address,undefined
// by tests/test_edlib_host.py.
//
//   edlib_host_check sizes <leaf_bytes> <max_query> <max_target> [...]
//                                  a line per pair: leaf_entries, max_blocks, ops_bytes, grow_words
//                                  of path_size, grow_words(max_target), LDS_COLUMNS, STRIPE_ROWS
//   edlib_host_check leaf <leaf_bytes> <qn> <tn> [...]
//                                  a line per pair: is_leaf, leaf_entries(leaf_bytes)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../canu_amd/csrc/edlib_host.h"

int main(int argc, char **argv) {
  if (argc >= 5 && (argc - 3) % 2 == 0 && !strcmp(argv[1], "sizes")) {
    const long long leaf_bytes = atoll(argv[2]);
    for (int a = 3; a < argc; a += 2) {
      const uint32_t q = (uint32_t)strtoul(argv[a], nullptr, 10), t = (uint32_t)strtoul(argv[a + 1], nullptr, 10);
      const edw::PathSize Z = edw::path_size(q, t, leaf_bytes);
      printf("%u %u %llu %llu %llu %d %d\n", Z.leaf_entries, Z.max_blocks,
             (unsigned long long)Z.ops_bytes, (unsigned long long)Z.grow_words,
             (unsigned long long)edw::grow_words(t), edw::LDS_COLUMNS, edw::STRIPE_ROWS);
    }
    return 0;
  }
  if (argc >= 5 && (argc - 3) % 2 == 0 && !strcmp(argv[1], "leaf")) {
    const long long leaf_bytes = atoll(argv[2]);
    for (int a = 3; a < argc; a += 2)
      printf("%d %d\n", edw::is_leaf(atoi(argv[a]), atoi(argv[a + 1]), leaf_bytes) ? 1 : 0,
             edw::leaf_entries(leaf_bytes));
    return 0;
  }
  fprintf(stderr, "usage: edlib_host_check sizes <leaf_bytes> <max_query> <max_target> [...] | "
                  "leaf <leaf_bytes> <qn> <tn> [...]\n");
  return 1;
}
