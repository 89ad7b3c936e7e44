// ovs_reader.h -- a read-only reader of canu's overlap store (src/stores/ovStore.H, ovStore.C,
// ovStoreFile.C), host C++17, no dependency.
//
//   <store>/info    ovStoreInfo (ovStore.H:53-175): eight uint64 -- magic, version, unused,
//                   smallest and largest a_iid, overlaps in the store, highest data file index,
//                   AS_MAX_READLEN_BITS
//   <store>/index   ovStoreOfft records (ovStore.H:178-200), 24 bytes each, one per read ID from
//                   0 to the largest a_iid: a_iid, data file, offset in it (in records), number of
//                   overlaps, ID of the first overlap.  A read with no overlaps points at the next
//                   read's overlaps and counts 0 (ovStoreWriter.C:188-205).
//   <store>/NNNN    data files 0001 ..: ovFileNormal records, uncompressed, 20 bytes each: b_iid,
//                   then the two 64-bit words of the ovOverlap, high half first (ovStoreFile.C:
//                   206-220).  a_iid is the index record's.  The overlaps of one read may run on
//                   into the next file (ovStoreWriter.C:166-184).
//   <store>/evalues may exist (updated error rates); it is not read here.
//
// read_range restates ovStore::setRange (ovStore.C:380) and ovStore::readOverlap (:149-189):
// seek to the first read's index record, open its data file at its offset, then stream; every
// later index record with overlaps must point at where the stream then stands.  Every
// length and offset is checked against the file sizes; a store that does not add up is an error
// with a message, never a read outside a buffer.
#ifndef CANU_OVS_READER_H
#define CANU_OVS_READER_H

#include <sys/stat.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/canu_ovl.h" /* ovl_record */

namespace ovs {

constexpr uint64_t MAGIC = 0x53564f3a756e6163ull;              // "canu:OVS", ovStore.H:49
constexpr uint64_t MAGIC_INCOMPLETE = 0x50564f3a756e6163ull;   // "canu:OVP", ovStore.H:50
constexpr uint64_t VERSION = 2;                                // ovStore.H:48
constexpr uint64_t READLEN_BITS = 21;                          // AS_MAX_READLEN_BITS
constexpr uint64_t RECORD_BYTES = 20, INDEX_BYTES = 24;

struct Info {
  uint64_t magic, version, unused, smallest_iid, largest_iid, num_overlaps, highest_file,
      max_readlen_bits;
};
static_assert(sizeof(Info) == 64, "ovStoreInfo is 64 bytes on disk");

struct Offt {
  uint32_t a_iid, fileno, offset, num_olaps;
  uint64_t overlap_id;
};
static_assert(sizeof(Offt) == 24, "ovStoreOfft is 24 bytes on disk");

inline bool file_size(const std::string &p, uint64_t &n) {
  struct stat sb;
  if (stat(p.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return false;
  n = (uint64_t)sb.st_size;
  return true;
}

class Store {
 public:
  // Opens <path>: false with a message when it is not a complete store of this version.
  bool open(const std::string &path, std::string &err) {
    path_ = path;
    index_.clear();
    uint64_t n = 0;
    const std::string iname = path + "/info";
    if (!file_size(iname, n)) { err = "'" + path + "' is not an overlap store: no '" + iname + "'"; return false; }
    if (n < sizeof(Info)) { err = "'" + iname + "' is " + std::to_string(n) + " bytes, not 64"; return false; }
    FILE *F = fopen(iname.c_str(), "rb");
    if (!F) { err = "can't open '" + iname + "'"; return false; }
    const bool ok = fread(&info_, sizeof(Info), 1, F) == 1;
    fclose(F);
    if (!ok) { err = "short read of '" + iname + "'"; return false; }
    if (info_.magic == MAGIC_INCOMPLETE) { err = "'" + path + "' is an incomplete overlap store, remove and rebuild"; return false; }
    if (info_.magic != MAGIC) { err = "'" + path + "' is not an overlap store"; return false; }
    if (info_.version != VERSION) {
      err = "'" + path + "' is store version " + std::to_string(info_.version) + ", supported is 2";
      return false;
    }
    if (info_.max_readlen_bits != READLEN_BITS) {
      err = "'" + path + "' was built for " + std::to_string(info_.max_readlen_bits) +
            "-bit read lengths, supported is 21";
      return false;
    }
    if (info_.highest_file > 9999) { err = "'" + iname + "' names " + std::to_string(info_.highest_file) + " data files"; return false; }
    const std::string xname = path + "/index";
    if (!file_size(xname, n)) { err = "no '" + xname + "'"; return false; }
    if (n % INDEX_BYTES) { err = "'" + xname + "' is not a whole number of 24-byte records"; return false; }
    if (n / INDEX_BYTES > (1ull << 32)) { err = "'" + xname + "' has more records than read IDs"; return false; }
    index_.resize(n / INDEX_BYTES);
    F = fopen(xname.c_str(), "rb");
    if (!F) { err = "can't open '" + xname + "'"; return false; }
    const bool iok = index_.empty() || fread(index_.data(), INDEX_BYTES, index_.size(), F) == index_.size();
    fclose(F);
    if (!iok) { err = "short read of '" + xname + "'"; return false; }
    return true;
  }

  const Info &info() const { return info_; }
  uint64_t index_records() const { return index_.size(); }

  // The overlaps whose a_iid is in [first, last], in store order (setRange + readOverlap).
  bool read_range(uint32_t first, uint32_t last, std::vector<ovl_record> &out, std::string &err) {
    out.clear();
    uint64_t f = first, l = last;
    if (f > info_.largest_iid) f = info_.largest_iid + 1;          // ovStore.C:387-390
    if (l >= info_.largest_iid) l = info_.largest_iid;
    if (f > l || f >= index_.size()) return true;                  // nothing to stream
    Stream S;
    bool ok = true;
    for (uint64_t i = f; ok && i < index_.size(); i++) {
      const Offt &o = index_[i];
      if (i == f) ok = S.open(path_, info_, o.fileno, o.offset, err);
      if (!ok || o.num_olaps == 0) continue;
      if (o.a_iid > l) break;                                      // ovStore.C:161
      if (o.a_iid != i) {
        err = "index record " + std::to_string(i) + " is for read " + std::to_string(o.a_iid);
        ok = false;
        break;
      }
      if (i != f && !S.at(o.fileno, o.offset)) {                   // the stream is the truth
        err = "index record " + std::to_string(i) + " points at file " + std::to_string(o.fileno) +
              " record " + std::to_string(o.offset) + ", the overlaps before it end at file " +
              std::to_string(S.fileno) + " record " + std::to_string(S.pos);
        ok = false;
        break;
      }
      if (out.size() + o.num_olaps > info_.num_overlaps) {
        err = "the index holds more overlaps than the store's " + std::to_string(info_.num_overlaps);
        ok = false;
        break;
      }
      for (uint32_t k = 0; ok && k < o.num_olaps; k++) {
        ovl_record r;
        ok = S.next(path_, info_, r, err);
        r.a_iid = o.a_iid;
        if (ok) out.push_back(r);
      }
    }
    S.close();
    if (!ok) out.clear();
    return ok;
  }

 private:
  struct Stream {
    FILE *F = nullptr;
    uint64_t fileno = 0, left = 0, pos = 0;   // records left in the open file, records passed

    // Is (no, offset) where the stream stands?  At the end of a file that is also the start
    // of the next one (ovStoreWriter.C:166-184).
    bool at(uint64_t no, uint64_t offset) const {
      return (no == fileno && offset == pos) || (left == 0 && no == fileno + 1 && offset == 0);
    }

    void close() {
      if (F) fclose(F);
      F = nullptr;
    }
    bool open_file(const std::string &path, const Info &I, uint64_t no, uint64_t offset, std::string &err) {
      close();
      if (no < 1 || no > I.highest_file) {
        err = "data file " + std::to_string(no) + " is outside 1.." + std::to_string(I.highest_file);
        return false;
      }
      char name[16];
      snprintf(name, sizeof name, "/%04u", (unsigned)no);
      const std::string p = path + name;
      uint64_t n = 0;
      if (!file_size(p, n)) { err = "no data file '" + p + "'"; return false; }
      if (n % RECORD_BYTES) { err = "'" + p + "' is not a whole number of 20-byte records"; return false; }
      if (offset > n / RECORD_BYTES) {
        err = "offset " + std::to_string(offset) + " is past the " + std::to_string(n / RECORD_BYTES) + " records of '" + p + "'";
        return false;
      }
      F = fopen(p.c_str(), "rb");
      if (!F || fseeko(F, (off_t)(offset * RECORD_BYTES), SEEK_SET) != 0) { err = "can't open '" + p + "'"; return false; }
      fileno = no;
      left = n / RECORD_BYTES - offset;
      pos = offset;
      return true;
    }
    bool open(const std::string &path, const Info &I, uint64_t no, uint64_t offset, std::string &err) {
      return open_file(path, I, no, offset, err);
    }
    bool next(const std::string &path, const Info &I, ovl_record &r, std::string &err) {
      while (left == 0)                                            // ovStore.C:164-177
        if (!open_file(path, I, fileno + 1, 0, err)) {
          err = "the index promises more overlaps than the data files hold (" + err + ")";
          return false;
        }
      uint32_t w[5];
      if (fread(w, 4, 5, F) != 5) { err = "short read of data file " + std::to_string(fileno); return false; }
      left--;
      pos++;
      r.a_iid = 0;
      r.b_iid = w[0];
      r.dat[0] = ((uint64_t)w[1] << 32) | w[2];
      r.dat[1] = ((uint64_t)w[3] << 32) | w[4];
      return true;
    }
  };

  std::string path_;
  Info info_{};
  std::vector<Offt> index_;
};

}  // namespace ovs

#endif
