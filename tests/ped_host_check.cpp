// ped_host_check.cpp -- the host side of the shared aligner (canu_amd/csrc/ped_host.h) as a
// program of its own, built with -fsanitize=address,undefined by tests/test_ped_host.py.
//
//   ped_host_check limit <erate> <max_errors> <upto> [...]   a line per triple: the upto + 1
//                                                           entries of init_match_limit
//   ped_host_check sizes <per_error> <limit> [<limit> ...]   a line per limit: rows worst first,
//                                                           the regrown cap from `first` and
//                                                           from `worst`, ROW_LOG_MAX
//   ped_host_check launch <n_cu> <log_cap> <limit> <extra> <todo> [...]
//                                                           a line per quadruple: ok, per_wave,
//                                                           nwaves, blocks, scratch_bytes of
//                                                           launch_size, WAVES_PER_BLOCK,
//                                                           SCRATCH_BUDGET
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../canu_amd/csrc/ped_host.h"

int main(int argc, char **argv) {
  if (argc >= 5 && (argc - 2) % 3 == 0 && !strcmp(argv[1], "limit")) {
    for (int a = 2; a < argc; a += 3) {
      std::vector<int32_t> ml;
      ped::init_match_limit(ml, strtod(argv[a], nullptr), atoi(argv[a + 1]), atoi(argv[a + 2]));
      for (size_t e = 0; e < ml.size(); e++) printf("%s%d", e ? " " : "", ml[e]);
      printf("\n");
    }
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "sizes")) {
    const int per_error = atoi(argv[2]);
    for (int a = 3; a < argc; a++) {
      const int32_t limit = atoi(argv[a]);
      const uint64_t first = ped::row_log_first(per_error, limit), worst = ped::row_log_worst(limit);
      printf("%llu %llu %llu %llu %llu %llu\n", (unsigned long long)ped::row_log_rows(limit),
             (unsigned long long)worst, (unsigned long long)first,
             (unsigned long long)ped::row_log_regrown(first, limit),
             (unsigned long long)ped::row_log_regrown(worst, limit),
             (unsigned long long)ped::ROW_LOG_MAX);
    }
    return 0;
  }
  if (argc >= 7 && (argc - 3) % 4 == 0 && !strcmp(argv[1], "launch")) {
    const int n_cu = atoi(argv[2]);
    for (int a = 3; a < argc; a += 4) {
      const ped::LaunchSize L = ped::launch_size(strtoull(argv[a], nullptr, 10), atoi(argv[a + 1]),
                                                 strtoull(argv[a + 2], nullptr, 10),
                                                 strtoull(argv[a + 3], nullptr, 10), n_cu);
      printf("%d %llu %llu %u %llu %d %llu\n", L.ok ? 1 : 0, (unsigned long long)L.per_wave,
             (unsigned long long)L.nwaves, L.blocks, (unsigned long long)L.scratch_bytes,
             ped::WAVES_PER_BLOCK, (unsigned long long)ped::SCRATCH_BUDGET);
    }
    return 0;
  }
  fprintf(stderr, "usage: ped_host_check limit <erate> <max_errors> <upto> [...] | "
                  "sizes <per_error> <limit> [...] | launch <n_cu> <log_cap> <limit> <extra> <todo> "
                  "[...]\n");
  return 1;
}
