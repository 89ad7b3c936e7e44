// fe_host_check.cpp -- the overlap store reader (canu_amd/csrc/ovs_reader.h) as a program of
// its own, built with -fsanitize=address,undefined by tests/test_fe_cpu.py.
//
//   fe_host_check read <store> <bgn> <end> <out.bin>   the range's records (a, b, w0, w1), or
//                                                      "error: ..." on stderr and status 2
//   fe_host_check info <store>                         the ovStoreInfo fields
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../canu_amd/csrc/ovs_reader.h"

int main(int argc, char **argv) {
  std::string err;
  ovs::Store S;
  if (argc == 3 && !strcmp(argv[1], "info")) {
    if (!S.open(argv[2], err)) { fprintf(stderr, "error: %s\n", err.c_str()); return 2; }
    const ovs::Info &I = S.info();
    printf("version %llu smallest %llu largest %llu overlaps %llu files %llu bits %llu index %llu\n",
           (unsigned long long)I.version, (unsigned long long)I.smallest_iid,
           (unsigned long long)I.largest_iid, (unsigned long long)I.num_overlaps,
           (unsigned long long)I.highest_file, (unsigned long long)I.max_readlen_bits,
           (unsigned long long)S.index_records());
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "read")) {
    std::vector<ovl_record> recs;
    if (!S.open(argv[2], err) ||
        !S.read_range((uint32_t)strtoul(argv[3], nullptr, 10), (uint32_t)strtoul(argv[4], nullptr, 10),
                      recs, err)) {
      fprintf(stderr, "error: %s\n", err.c_str());
      return 2;
    }
    FILE *O = fopen(argv[5], "wb");
    if (!O) { fprintf(stderr, "error: can't write '%s'\n", argv[5]); return 2; }
    for (const ovl_record &r : recs) {
      fwrite(&r.a_iid, 4, 1, O);
      fwrite(&r.b_iid, 4, 1, O);
      fwrite(r.dat, 8, 2, O);
    }
    fclose(O);
    printf("fe_host_check ok: %zu records\n", recs.size());
    return 0;
  }
  fprintf(stderr, "usage: fe_host_check read <store> <bgn> <end> <out.bin> | info <store>\n");
  return 1;
}
