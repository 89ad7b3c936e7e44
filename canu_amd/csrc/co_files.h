// co_files.h -- the two files of correctOverlaps, read on the host with every length checked.
//
//   .red   Correction_Output_t records (correctionOutput.H:40-46), 8 bytes each, as findErrors
//          writes them: ascending by read, each read's IDENT record first.
//   .oea   int32 bgnID, int32 endID, uint64 n, uint16 evalue[n] (correctOverlaps.C:203-215).
//
// Host only; used by co_main.cpp and, under the sanitizers, by tests/co_host_check.cpp.
#ifndef CANU_CO_FILES_H
#define CANU_CO_FILES_H

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/canu_fe.h"

namespace cofiles {

inline bool slurp(const std::string &path, std::vector<uint8_t> &out, std::string &err) {
  FILE *F = fopen(path.c_str(), "rb");
  if (!F) {
    err = "can't open '" + path + "': " + strerror(errno);
    return false;
  }
  out.clear();
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, F)) > 0) out.insert(out.end(), buf, buf + n);
  const bool bad = ferror(F) != 0;
  fclose(F);
  if (bad) err = "read error on '" + path + "'";
  return !bad;
}

// The records of a .red file.  A file that ends inside a record, or whose reads do not ascend,
// is refused; an empty file holds no records.
inline bool parse_red(const uint8_t *p, uint64_t bytes, std::vector<fe_correction> &out,
                      std::string &err) {
  static_assert(sizeof(fe_correction) == 8, "Correction_Output_t is 8 bytes");
  out.clear();
  if (bytes % sizeof(fe_correction)) {
    err = "a .red file of " + std::to_string(bytes) + " bytes ends inside a record";
    return false;
  }
  out.resize(bytes / sizeof(fe_correction));
  if (bytes) memcpy(out.data(), p, bytes);
  for (size_t k = 1; k < out.size(); k++)
    if (out[k].read_id < out[k - 1].read_id) {
      err = "record " + std::to_string(k) + " of the .red file is of read " +
            std::to_string(out[k].read_id) + ", the one before of read " +
            std::to_string(out[k - 1].read_id);
      out.clear();
      return false;
    }
  return true;
}

inline bool read_red(const std::string &path, std::vector<fe_correction> &out, std::string &err) {
  std::vector<uint8_t> raw;
  return slurp(path, raw, err) && parse_red(raw.data(), raw.size(), out, err);
}

struct Oea {
  uint32_t bgn_id = 0, end_id = 0;
  std::vector<uint16_t> evalues;
};

inline bool parse_oea(const uint8_t *p, uint64_t bytes, Oea &out, std::string &err) {
  out = Oea();
  if (bytes < 16) {
    err = "an .oea file of " + std::to_string(bytes) + " bytes has no header";
    return false;
  }
  uint64_t n;
  memcpy(&out.bgn_id, p, 4);
  memcpy(&out.end_id, p + 4, 4);
  memcpy(&n, p + 8, 8);
  if (n > (bytes - 16) / 2 || 16 + 2 * n != bytes) {
    err = "an .oea file of " + std::to_string(bytes) + " bytes does not hold its " +
          std::to_string(n) + " evalues";
    return false;
  }
  out.evalues.resize(n);
  if (n) memcpy(out.evalues.data(), p + 16, 2 * n);
  return true;
}

inline bool read_oea(const std::string &path, Oea &out, std::string &err) {
  std::vector<uint8_t> raw;
  return slurp(path, raw, err) && parse_oea(raw.data(), raw.size(), out, err);
}

inline bool write_oea(const std::string &path, const Oea &o, std::string &err) {
  FILE *F = fopen(path.c_str(), "wb");
  if (!F) {
    err = "can't open '" + path + "' for writing: " + strerror(errno);
    return false;
  }
  const uint64_t n = o.evalues.size();
  size_t w = fwrite(&o.bgn_id, 4, 1, F) + fwrite(&o.end_id, 4, 1, F) + fwrite(&n, 8, 1, F);
  if (n) w += fwrite(o.evalues.data(), 2, n, F);
  if (fclose(F) != 0 || w != 3 + n) {
    err = "short write to '" + path + "'";
    return false;
  }
  return true;
}

}  // namespace cofiles
#endif
