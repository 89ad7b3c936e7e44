/* canu_tr.h -- C ABI of libcanu_tr.so: canu's trimReads (overlap based trimming,
 * src/overlapBasedTrimming/trimReads*.C) on one gfx950 device.
 *
 * What it reproduces: the per-read loop of trimReads.C:268-437 with no -Ci / -Cm file.  For every
 * read of an inclusive ID range the overlaps of the read (ovl_record, sorted by a_iid, as an
 * overlap store streams them) give a clear range by the rule of the read's library --
 * 1 largestCovered (trimReads-largestCovered.C), 2 bestEdge (trimReads-bestEdge.C) -- and the
 * read is classified NOV (no overlaps), DEL (nothing found, or shorter than min_read_length),
 * NOC (unchanged) or MOD.  Only a_iid, ahg5, ahg3 and the evalue of a record are read, and no
 * base of any read.
 *
 * Every call returns TR_OK (0) or a negative status; tr_last_error() describes the last failure
 * of the calling thread.  A context is used by one thread at a time.  There is no CPU fallback.
 */
#ifndef CANU_TR_H
#define CANU_TR_H

#include <stdint.h>

#include "canu_ovl.h" /* ovl_record */

#ifdef __cplusplus
extern "C" {
#endif

#define TR_ABI_VERSION 1

enum {
  TR_OK = 0,
  TR_ERR_NO_DEVICE = -1,
  TR_ERR_BAD_PARAM = -2,
  TR_ERR_UNSUPPORTED = -3,
  TR_ERR_BAD_INPUT = -4,
  TR_ERR_HIP = -5,
  TR_ERR_OOM = -6,
  TR_ERR_STATE = -7
};

/* trimReads' options that change the result (trimReads.C:112-126). */
typedef struct tr_params {
  double   erate;                 /* -e          (0.015): overlaps above it are skipped       */
  uint32_t min_read_length;       /* -minlength  (64)                                        */
  uint32_t min_evidence_overlap;  /* -ol         (40)                                        */
  uint32_t min_evidence_coverage; /* -oc         (1)                                         */
} tr_params;

enum { TR_NOT_IN_RANGE = 0, TR_NOV = 1, TR_DEL = 2, TR_NOC = 3, TR_MOD = 4 };

/* tr_result.flags */
#define TR_FLAG_NO_HQ 1 /* largestCovered found nothing: "no high quality overlaps"           */
#define TR_FLAG_RESET 2 /* bestEdge's trim points crossed and were reset (it prints "iid =")  */

typedef struct tr_count {
  uint64_t reads, bases;
} tr_count;

typedef struct tr_stats {
  /* the nine trimStat of trimReads.C:130-140 */
  tr_count reads_in, deleted_in, no_trim_in, reads_out, no_ovl_out, deleted_out, no_change_out,
      trim5, trim3;
  uint32_t id_min, id_max;  /* the range after clamping to 1 .. num_reads                     */
  uint64_t n_overlaps;      /* overlaps of the reads in the range                             */
  uint64_t n_wave_reads;    /* reads trimmed by a wave in LDS                                 */
  uint64_t n_large_reads;   /* reads with more than tr_wave_capacity() overlaps               */
  uint64_t n_literal;       /* reads whose depth list was walked event by event               */
  uint64_t scratch_bytes;   /* device memory of the large reads' lists                        */
  double   ms_segment;      /* k_tr_segment + k_tr_offsets                                    */
  double   ms_wave;         /* k_tr_wave                                                      */
  double   ms_large;        /* k_tr_large_keys, the two segmented sorts, k_tr_large           */
} tr_stats;

/* Per-read results, each array num_reads long, entry i for read i + 1.  bgn / end are what the
 * rule left (the log's finalL / finalR): 0 .. length where nothing was found or the read is not
 * in the range. */
typedef struct tr_result {
  uint32_t *bgn, *end;
  uint8_t  *status;  /* TR_NOT_IN_RANGE .. TR_MOD */
  uint8_t  *flags;   /* TR_FLAG_* */
  uint32_t *n_skipped, *n_used;
} tr_result;

typedef struct tr_ctx tr_ctx;

void        tr_params_init(tr_params *p);
const char *tr_last_error(void);
int         tr_abi_version(void);
/* The overlaps of one read a wave sorts and sweeps in its LDS; a read with more goes through
 * lists in device memory. */
uint32_t    tr_wave_capacity(void);

int  tr_ctx_create(const tr_params *p, int device, tr_ctx **out);
void tr_ctx_destroy(tr_ctx *ctx);
int  tr_set_params(tr_ctx *ctx, const tr_params *p);

/* trimReads -t id_min-id_max over reads 1 .. num_reads.  lengths[i] and rules[i] (0 none,
 * 1 largestCovered, 2 bestEdge: the library's finalTrim) belong to read i + 1.  records: n
 * overlaps sorted by a_iid, in host memory, or in device memory when records_on_device is set.
 * TR_ERR_BAD_INPUT: records not sorted by a_iid or naming a read outside 1 .. num_reads, an
 * overlap with a_bgn >= a_end or hangs longer than its read, a read longer than 2^21 - 1, a read
 * of the range whose rule is not 1 or 2 (the reference asserts there). */
int tr_trim_reads(tr_ctx *ctx, uint32_t num_reads, const uint32_t *lengths, const uint8_t *rules,
                  const ovl_record *records, uint64_t n, int records_on_device, uint32_t id_min,
                  uint32_t id_max, tr_result *out);
int tr_get_stats(const tr_ctx *ctx, tr_stats *out);

#ifdef __cplusplus
}
#endif
#endif
