// fs_fasta.h -- how falconsense writes a consensus (falconsense.C:164-188): the pieces between
// lower-case letters, those longer than the minimum as FASTA records of 60-column lines
// (AS_UTL_writeFastA), and the "Generated read" line of each.  Host only.
#ifndef CANU_FS_FASTA_H
#define CANU_FS_FASTA_H

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

// AS_UTL_writeFastA(f, s, n, 60, ">read%u_%d\n", tig, k): a newline after every 60th base and
// one at the end unless the last line was full.
inline void fs_fasta_record(std::string &out, uint32_t tig, uint32_t k, const uint8_t *s, size_t n) {
  char head[64];
  snprintf(head, sizeof head, ">read%u_%d\n", tig, (int)k);
  out += head;
  for (size_t i = 0; i < n; i++) {
    out += (char)s[i];
    if ((i + 1) % 60 == 0) out += '\n';
  }
  if (out.back() != '\n') out += '\n';
}

// strtok(seq, "acgt"): the maximal runs without a lower-case a, c, g or t; a run is written when
// strlen(run) > min_output_length.  Returns the number of records; `log`, if given, gets the
// "Generated read" lines.
inline uint32_t fs_fasta_pieces(std::string &out, std::string *log, uint32_t tig, const uint8_t *cns,
                                size_t n, uint32_t min_output_length) {
  uint32_t k = 0;
  size_t i = 0;
  auto low = [](uint8_t c) { return c == 'a' || c == 'c' || c == 'g' || c == 't'; };
  while (i < n) {
    while (i < n && low(cns[i])) i++;
    size_t j = i;
    while (j < n && !low(cns[j])) j++;
    if (j - i > (size_t)min_output_length) {
      if (log) {
        char line[96];
        snprintf(line, sizeof line, "Generated read %u_%u of length %lu.\n", tig, k,
                 (unsigned long)(j - i));
        *log += line;
      }
      fs_fasta_record(out, tig, k, cns + i, j - i);
      k++;
    }
    i = j;
  }
  return k;
}

#endif
