/* canu_meryl.h -- C ABI of libcanu_meryl.so: meryl's k-mer count (the 0-mercounts stage of
 * canu, src/pipelines/canu/Meryl.pm:373-771) on one gfx950 device.
 *
 * What it reproduces of the reference (src/meryl):
 *   meryl -B -C -L <low> -m <k> -s <reads> -o <prefix>   mer_count + mer_save
 *   meryl -Dh -s <prefix>                                 mer_write_histogram
 *   meryl -Dt -n <thresh> -s <prefix>                     mer_write_threshold
 * The texts are byte-identical to the reference's; the database files (prefix.mcdat /
 * prefix.mcidx) are a format of this library and NOT interchangeable with the reference's.
 *
 * Semantics (reference lines in DESIGN.md): a mer never spans two reads or a non-ACGT byte;
 * lower case counts as upper case; canonical = the numerically smaller of the mer and its
 * reverse complement under A<C<G<T, first base most significant; mers with a count below
 * low_count are left out of the kept list but stay in the totals and the histogram.
 *
 * Every call returns MER_OK (0) or a negative status; mer_last_error() describes the last
 * failure of the calling thread.  A context is used by one thread at a time.
 */
#ifndef CANU_MERYL_H
#define CANU_MERYL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MER_ABI_VERSION 1

enum {
  MER_OK = 0,
  MER_ERR_NO_DEVICE = -1,
  MER_ERR_BAD_PARAM = -2,
  MER_ERR_UNSUPPORTED = -3,
  MER_ERR_BAD_INPUT = -4,
  MER_ERR_HIP = -5,
  MER_ERR_OOM = -6,
  MER_ERR_STATE = -7,
  MER_ERR_IO = -8
};

/* Device bytes a counting context holds beside the packed reads and the per-pass buffers
 * (prefix and count histograms, bucket tables, the overflow list, the read-start table of
 * mer_load_reads_device excluded: that one is 8 bytes per read).  A test of the budget
 * checks peak_device_bytes <= hbm_budget_bytes + packed_read_bytes + MER_FIXED_OVERHEAD_BYTES. */
#define MER_FIXED_OVERHEAD_BYTES (48ull << 20)

/* Smallest budget mer_count accepts (one pass buffer of 4096 mers). */
#define MER_MIN_BUDGET_BYTES (4096ull * 24ull)

typedef struct mer_params {
  uint32_t kmer_len;          /* 1..32 */
  int32_t  canonical;         /* meryl -C */
  uint32_t low_count;         /* meryl -L: smallest count kept in the database (>= 1) */
  uint64_t hbm_budget_bytes;  /* per-pass buffers; 0 = derive from free HBM */
} mer_params;

typedef struct mer_stats {
  uint64_t total_mers;        /* "Found N mers." */
  uint64_t distinct_mers;
  uint64_t unique_mers;       /* count == 1 */
  uint64_t largest_count;
  uint64_t kept_mers;         /* distinct mers with count >= low_count */
  uint64_t passes;            /* key ranges sorted on the device */
  uint64_t direct_keys;       /* single keys larger than a pass, counted by the planner */
  uint64_t plan_scans;        /* prefix-histogram scans of the reads */
  uint64_t oversize_buckets;  /* fine buckets larger than the LDS sort */
  uint64_t peak_device_bytes;
  uint64_t packed_read_bytes;
  uint64_t budget_bytes;      /* the budget in force */
  uint64_t overflow_counts;   /* counts beyond the dense device histogram, folded on the host */
  double   ms_plan;           /* prefix histograms (emit) */
  double   ms_partition;      /* scan + coarse scatter */
  double   ms_sort;           /* fine sort + run lengths + compaction */
  double   ms_total;          /* wall clock of mer_count */
} mer_stats;

typedef struct mer_ctx mer_ctx;

void        mer_params_init(mer_params *p);    /* k=22, canonical, low_count 2, budget 0 */
const char *mer_last_error(void);
int         mer_abi_version(void);

int  mer_ctx_create(const mer_params *p, int device, mer_ctx **out);
void mer_ctx_destroy(mer_ctx *ctx);

/* Reads as one byte per base: read i is bases[offsets[i] .. offsets[i]+lengths[i]).  */
int mer_load_reads(mer_ctx *ctx, uint32_t nreads, const uint8_t *bases,
                   const uint64_t *offsets, const uint32_t *lengths);
/* The same with bases and offsets in device memory (lengths on the host). */
int mer_load_reads_device(mer_ctx *ctx, uint32_t nreads, const uint8_t *d_bases,
                          const uint64_t *d_offsets, const uint32_t *lengths);

int mer_count(mer_ctx *ctx);
int mer_get_stats(const mer_ctx *ctx, mer_stats *out);
/* Counts below dense_len go to a dense histogram on the device, larger ones to a list of
 * overflow_cap entries that the host drains after every pass; a pass is cut to at most
 * dense_len x overflow_cap mers, so the list cannot fill whatever the input.  The defaults
 * (65536, 4096) are also the largest values; smaller ones only cost passes and exist so that a
 * test can drive many counts through the list. */
int mer_set_histogram_limits(mer_ctx *ctx, uint32_t dense_len, uint32_t overflow_cap);
/* The parameters in force (of a reopened database: the ones it was counted with). */
int mer_get_params(const mer_ctx *ctx, mer_params *out);

/* hist[c] = number of distinct mers with count c, for c < cap; *len = largest count + 1
 * (the length a full copy needs).  hist may be NULL to ask for *len only. */
int mer_histogram(const mer_ctx *ctx, uint64_t *hist, uint64_t cap, uint64_t *len);

/* Mers with count >= max(min_count, low_count), ascending by 2-bit value (the reference's
 * dump order).  *n = how many there are; at most cap are written (mers/counts may be NULL). */
int mer_frequent(const mer_ctx *ctx, uint64_t min_count, uint64_t *mers, uint32_t *counts,
                 uint64_t cap, uint64_t *n);

int mer_save(const mer_ctx *ctx, const char *prefix);
/* Host only: no device is touched.  Everything but load/count works on the result. */
int mer_open(const char *prefix, mer_ctx **out);

/* meryl -Dh: the histogram rows (its stdout) and the four info lines (its stderr).
 * Either path may be NULL. */
int mer_write_histogram(const mer_ctx *ctx, const char *hist_path, const char *info_path);
/* meryl -Dt -n min_count: ">count\nMER\n" per mer. */
int mer_write_threshold(const mer_ctx *ctx, uint64_t min_count, const char *path);

#ifdef __cplusplus
}
#endif
#endif
