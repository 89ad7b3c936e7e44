// ovb_reader.h -- read an ovFileFull .ovb back into ovOverlap records (host code).
//
// Reference:
//   src/stores/ovStoreFile.C:266   ovFile::readBuffer: per block a size_t compressed length
//                                   and a raw snappy stream (ovStore.H:40 defines SNAPPY)
//   src/stores/ovStoreFile.C:330   readOverlap, full format: a_iid, b_iid, then each 64-bit
//                                   dat word as (hi32, lo32)
//   src/stores/ovStoreFile.C:66    the reader's buffer: 1 MiB, the most a block can hold
// The writer next door (ovl_ovb.h) emits literal-only streams; the reference's own writers
// (mhapConvert, overlapInCore) compress, so this decoder knows the whole raw format:
// literals and the copies with 1-, 2- and 4-byte offsets
// (https://github.com/google/snappy/blob/main/format_description.txt).
// Every length is checked against the file and the block; a malformed file gives `false`
// and a message, never a read or write out of bounds.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/canu_ovl.h"

namespace ovb {

constexpr size_t MAX_BLOCK_BYTES = 1u << 20;     // ovFile's buffer (ovStoreFile.C:66)

// Raw snappy: `in[0..n)` -> out (resized to the stream's stated length).
inline bool snappy_uncompress(const uint8_t *in, size_t n, std::vector<uint8_t> &out,
                              std::string &err) {
  size_t p = 0;
  uint64_t ol = 0;
  int shift = 0;
  while (true) {                                  // preamble: varint32
    if (p >= n) { err = "snappy: stream ends inside its length"; return false; }
    if (shift > 28) { err = "snappy: length longer than 32 bits"; return false; }
    const uint8_t b = in[p++];
    ol |= (uint64_t)(b & 0x7f) << shift;
    shift += 7;
    if (!(b & 0x80)) break;
  }
  if (ol > MAX_BLOCK_BYTES) {
    err = "snappy: block of " + std::to_string(ol) + " bytes, more than an ovFile buffer";
    return false;
  }
  out.resize((size_t)ol);
  size_t o = 0;
  while (p < n) {
    const uint8_t tag = in[p++];
    size_t len, off = 0;
    if ((tag & 3) == 0) {                         // literal
      len = (size_t)(tag >> 2) + 1;
      if (len > 60) {
        const size_t nb = len - 60;               // 1..4 bytes of (length - 1)
        if (n - p < nb) { err = "snappy: literal length past the block"; return false; }
        uint32_t v = 0;
        for (size_t i = 0; i < nb; i++) v |= (uint32_t)in[p + i] << (8 * i);
        p += nb;
        len = (size_t)v + 1;
      }
      if (len > n - p) { err = "snappy: literal past the block"; return false; }
      if (len > out.size() - o) { err = "snappy: literal past the stated length"; return false; }
      memcpy(out.data() + o, in + p, len);
      p += len;
      o += len;
      continue;
    }
    if ((tag & 3) == 1) {                         // copy, 11-bit offset
      if (n - p < 1) { err = "snappy: copy offset past the block"; return false; }
      len = 4 + ((tag >> 2) & 7);
      off = ((size_t)(tag >> 5) << 8) | in[p];
      p += 1;
    } else if ((tag & 3) == 2) {                  // copy, 16-bit offset
      if (n - p < 2) { err = "snappy: copy offset past the block"; return false; }
      len = (size_t)(tag >> 2) + 1;
      off = (size_t)in[p] | ((size_t)in[p + 1] << 8);
      p += 2;
    } else {                                      // copy, 32-bit offset
      if (n - p < 4) { err = "snappy: copy offset past the block"; return false; }
      len = (size_t)(tag >> 2) + 1;
      off = (size_t)in[p] | ((size_t)in[p + 1] << 8) | ((size_t)in[p + 2] << 16) |
            ((size_t)in[p + 3] << 24);
      p += 4;
    }
    if (off == 0 || off > o) { err = "snappy: copy from before the block"; return false; }
    if (len > out.size() - o) { err = "snappy: copy past the stated length"; return false; }
    for (size_t i = 0; i < len; i++) out[o + i] = out[o + i - off];   // may overlap itself
    o += len;
  }
  if (o != out.size()) { err = "snappy: stream shorter than its stated length"; return false; }
  return true;
}

// Every record of an ovFileFull file, in file order.
inline bool read_ovb_file(const char *path, std::vector<ovl_record> &recs, std::string &err) {
  recs.clear();
  FILE *F = fopen(path, "rb");
  if (!F) { err = std::string("can't open '") + path + "'"; return false; }
  bool ok = true;
  uint64_t left = 0;
  if (fseeko(F, 0, SEEK_END) != 0) ok = false;
  const off_t size = ok ? ftello(F) : -1;
  if (size < 0 || fseeko(F, 0, SEEK_SET) != 0) ok = false;
  if (!ok) { err = std::string("can't size '") + path + "'"; fclose(F); return false; }
  left = (uint64_t)size;
  std::vector<uint8_t> comp, raw;
  uint64_t block = 0;
  while (left) {
    uint64_t cl = 0;
    static_assert(sizeof(size_t) == 8, "the block length is a 64-bit size_t on disk");
    if (left < 8 || fread(&cl, 8, 1, F) != 1) {
      err = "block " + std::to_string(block) + ": file ends inside the block length";
      ok = false;
      break;
    }
    left -= 8;
    if (cl > left) {
      err = "block " + std::to_string(block) + ": " + std::to_string(cl) +
            " compressed bytes stated, " + std::to_string(left) + " left in the file";
      ok = false;
      break;
    }
    comp.resize((size_t)cl);
    if (cl && fread(comp.data(), 1, (size_t)cl, F) != cl) {
      err = "block " + std::to_string(block) + ": short read";
      ok = false;
      break;
    }
    left -= cl;
    std::string serr;
    if (!snappy_uncompress(comp.data(), comp.size(), raw, serr)) {
      err = "block " + std::to_string(block) + ": " + serr;
      ok = false;
      break;
    }
    if (raw.size() % 24) {
      err = "block " + std::to_string(block) + ": " + std::to_string(raw.size()) +
            " bytes are no whole number of records";
      ok = false;
      break;
    }
    for (size_t p = 0; p < raw.size(); p += 24) {
      uint32_t w[6];
      memcpy(w, raw.data() + p, 24);
      ovl_record r;
      r.a_iid = w[0];
      r.b_iid = w[1];
      r.dat[0] = ((uint64_t)w[2] << 32) | w[3];
      r.dat[1] = ((uint64_t)w[4] << 32) | w[5];
      recs.push_back(r);
    }
    block++;
  }
  fclose(F);
  if (!ok) recs.clear();
  return ok;
}

}  // namespace ovb
