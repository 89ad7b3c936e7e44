/* canu_sr.h -- C ABI of libcanu_sr.so: canu's splitReads (overlap based trimming,
 * src/overlapBasedTrimming/splitReads*.C, adjustNormal.C, adjustFlipped.C) on one gfx950 device.
 *
 * What it reproduces: the per-read loop of splitReads.C:232-373.  For every read of an inclusive
 * ID range that the input clear ranges have not deleted and whose library asks for it, the
 * overlaps of the read (ovl_record, sorted by (a_iid, b_iid), as an overlap store streams them)
 * are adjusted to both reads' input clear ranges; pairs of overlaps with one B read in opposite
 * orientations give suspected subread junctions (detectSubReads); the confirmed ones are cut out
 * and the largest piece left becomes the read's clear range (trimBadInterval), or the read is
 * deleted when that piece is shorter than min_read_length.  Spur and chimera detection are
 * commented out in the reference; their counters exist and stay 0.  No base of any read is read.
 *
 * Every call returns SR_OK (0) or a negative status; sr_last_error() describes the last failure
 * of the calling thread.  A context is used by one thread at a time.  There is no CPU fallback.
 */
#ifndef CANU_SR_H
#define CANU_SR_H

#include <stdint.h>

#include "canu_ovl.h" /* ovl_record */

#ifdef __cplusplus
extern "C" {
#endif

#define SR_ABI_VERSION 1

enum {
  SR_OK = 0,
  SR_ERR_NO_DEVICE = -1,
  SR_ERR_BAD_PARAM = -2,
  SR_ERR_UNSUPPORTED = -3,
  SR_ERR_BAD_INPUT = -4,
  SR_ERR_HIP = -5,
  SR_ERR_OOM = -6,
  SR_ERR_STATE = -7
};

/* splitReads' options (splitReads.C:120-152). */
typedef struct sr_params {
  double   erate;            /* -e          (0.015): printed, never used (workUnit.C:148)     */
  uint32_t min_read_length;  /* -minlength  (64)                                              */
} sr_params;

/* lib_flags of a read: its library's switches (gkStore.H:186-193). */
#define SR_LIB_ELIGIBLE 1 /* removeSpurReads, removeChimericReads or checkForSubReads         */
#define SR_LIB_SUBREADS 2 /* checkForSubReads                                                 */

/* the `on_device` argument of sr_split_reads */
#define SR_RECORDS_ON_DEVICE 1
#define SR_CLEAR_ON_DEVICE   2

/* sr_result.status */
enum {
  SR_NOT_IN_RANGE = 0,
  SR_DELETED_IN = 1,   /* deleted by the input clear ranges                                   */
  SR_NO_TRIM = 2,      /* its library asks for nothing                                        */
  SR_NO_OVERLAPS = 3,
  SR_NO_COVERAGE = 4,  /* no overlap left after the adjustment                                */
  SR_NO_CHANGE = 5,    /* no bad region confirmed                                             */
  SR_TRIMMED = 6,
  SR_DELETED_OUT = 7   /* the largest good piece is shorter than min_read_length              */
};

/* sr_result.fate */
enum {
  SR_FATE_NOT_IN_RANGE = 0, /* its A read was not processed                                   */
  SR_FATE_DROPPED = 1,      /* a deleted B read, or it misses a clear range                   */
  SR_FATE_KEPT = 2,
  SR_FATE_MANY = 3,         /* one of more than two overlaps of a pair: "ERROR: more overlaps" */
  SR_FATE_SAME_ORIENT = 4   /* the first of two in one orientation: "ERROR: same orient"      */
};

typedef struct sr_count {
  uint64_t reads, bases;
} sr_count;

typedef struct sr_stats {
  /* the trimStat of splitReads.C:64-114 */
  sr_count reads_in, deleted_in, no_trim_in, no_overlaps, no_coverage, proc_chimera, proc_spur,
      proc_subread, reads_bad_spur5, reads_bad_spur3, reads_bad_chimera, reads_bad_subread,
      bases_bad_spur5, bases_bad_spur3, bases_bad_chimera, bases_bad_subread, trimmed5, trimmed3,
      no_change, deleted_out;
  uint32_t id_min, id_max;  /* the range after clamping to 1 .. num_reads                     */
  uint64_t n_overlaps;      /* overlaps of the processed reads                                */
  uint64_t n_wave_reads;    /* reads handled by a wave in LDS                                 */
  uint64_t n_large_reads;   /* reads with more than sr_wave_capacity() overlaps               */
  uint64_t n_regions;       /* confirmed bad regions                                          */
  uint64_t scratch_bytes;   /* device memory of the large reads' lists                        */
  double   ms_records;      /* k_sr_reads + k_sr_adjust + k_sr_pairs                          */
  double   ms_wave;         /* k_sr_wave                                                      */
  double   ms_large;        /* k_sr_large                                                     */
} sr_stats;

typedef struct sr_region {
  uint32_t read, bgn, end;
} sr_region;

/* The caller allocates every array.  Per read (num_reads entries, entry i for read i + 1): bgn /
 * end are the final clear range as trimBadInterval left it (also for a read deleted on output),
 * the input range where nothing was done.  fate has one byte per input record.  regions holds
 * the confirmed bad regions in read order, region_off[i] .. region_off[i + 1] those of read
 * i + 1 (num_reads + 1 entries); at most n / 2 regions exist, regions_cap is the room given and
 * SR_ERR_BAD_PARAM the answer when it does not suffice. */
typedef struct sr_result {
  uint32_t  *bgn, *end;
  uint8_t   *status;
  uint32_t  *n_adjusted, *n_bad_regions;
  uint8_t   *fate;
  sr_region *regions;
  uint64_t   regions_cap;
  uint64_t  *region_off;
} sr_result;

typedef struct sr_ctx sr_ctx;

void        sr_params_init(sr_params *p);
const char *sr_last_error(void);
int         sr_abi_version(void);
/* The overlaps of one read a wave handles with its lists in LDS; a read with more goes through
 * lists in device memory. */
uint32_t    sr_wave_capacity(void);

int  sr_ctx_create(const sr_params *p, int device, sr_ctx **out);
void sr_ctx_destroy(sr_ctx *ctx);
int  sr_set_params(sr_ctx *ctx, const sr_params *p);

/* splitReads -t id_min-id_max over reads 1 .. num_reads.  lengths[i] and lib_flags[i] (SR_LIB_*)
 * belong to read i + 1.  clr_bgn / clr_end: the input clear ranges (-Ci), num_reads entries,
 * UINT32_MAX twice for a deleted read; both NULL: 0 .. length for every read; device pointers
 * when on_device has SR_CLEAR_ON_DEVICE (what an earlier stage left in HBM).  records: n overlaps
 * sorted by (a_iid, b_iid), in host memory, or in device memory with SR_RECORDS_ON_DEVICE; within
 * a pair the order given is the order of detectSubReads' ii / jj.
 * SR_ERR_BAD_INPUT, where the reference asserts or computes on a wrapped value: records not
 * sorted or naming a read outside 1 .. num_reads; a_bgn >= a_end or b_bgn >= b_end (hangs as long
 * as their read); a clear range with bgn > end or end > length that is not the deleted mark; a
 * read longer than 2^21 - 1; a result clear range outside the input one (splitReads.C:365). */
int sr_split_reads(sr_ctx *ctx, uint32_t num_reads, const uint32_t *lengths, const uint8_t *lib_flags,
                   const uint32_t *clr_bgn, const uint32_t *clr_end, const ovl_record *records,
                   uint64_t n, int on_device, uint32_t id_min, uint32_t id_max, sr_result *out);
int sr_get_stats(const sr_ctx *ctx, sr_stats *out);

#ifdef __cplusplus
}
#endif
#endif
