// co_host_check.cpp -- correctOverlaps' host-side file readers (canu_amd/csrc/co_files.h) as a
// program of its own, built with -fsanitize=address,undefined by tests/test_co_cpu.py.
//
//   co_host_check red <file.red>                  "red ok: N records, R reads", or
//                                                 "error: ..." on stderr and status 2
//   co_host_check oea <file.oea>                  "oea ok: bgn end n sum"
//   co_host_check copy <in.oea> <out.oea>         read, write again
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../canu_amd/csrc/co_files.h"

int main(int argc, char **argv) {
  std::string err;
  if (argc == 3 && !strcmp(argv[1], "red")) {
    std::vector<fe_correction> red;
    if (!cofiles::read_red(argv[2], red, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    size_t reads = 0;
    for (size_t k = 0; k < red.size(); k++) reads += k == 0 || red[k].read_id != red[k - 1].read_id;
    printf("red ok: %zu records, %zu reads\n", red.size(), reads);
    return 0;
  }
  if ((argc == 3 && !strcmp(argv[1], "oea")) || (argc == 4 && !strcmp(argv[1], "copy"))) {
    cofiles::Oea o;
    if (!cofiles::read_oea(argv[2], o, err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    if (argc == 4 && !cofiles::write_oea(argv[3], o, err)) {
      fprintf(stderr, "error: %s\n", err.c_str());
      return 2;
    }
    unsigned long long sum = 0;
    for (uint16_t v : o.evalues) sum += v;
    printf("oea ok: %u %u %zu %llu\n", o.bgn_id, o.end_id, o.evalues.size(), sum);
    return 0;
  }
  fprintf(stderr, "usage: co_host_check red <file> | oea <file> | copy <in> <out>\n");
  return 1;
}
