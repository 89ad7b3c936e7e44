/* canu_fe.h -- C ABI of libcanu_fe.so: canu's findErrors ("RED", read error detection; the
 * first half of overlap error adjustment, src/overlapErrorAdjustment/findErrors*.C) on one
 * gfx950 device.
 *
 * What it reproduces: for every overlap whose A read is in [bgn_id, end_id], Process_Olap
 * (findErrors-Process_Olap.C:59-164) -- the degrees, Prefix_Edit_Dist with its branch-point
 * score and Compute_Delta (findErrors-Prefix_Edit_Distance.C), the rescue rule, the error test
 * -- then Analyze_Alignment's votes (findErrors-Analyze_Alignment.C) and Output_Corrections'
 * two ladders (findErrors-Output.C), giving the Correction_Output_t records of the .red file
 * byte for byte.  Every tally is a saturating count, so the result does not depend on the
 * order of the overlaps.
 *
 * Read bytes outside "ACGTacgt" become 'a', as Read_Frags and Extract_Needed_Frags make them;
 * the library applies that filter itself.  Overlaps use the ovOverlap layout of canu_ovl.h
 * (ovl_record); only the IDs, the four hangs and the flipped bit are read.
 *
 * Every call returns FE_OK (0) or a negative status; fe_last_error() describes the last
 * failure of the calling thread.  A context is used by one thread at a time.  There is no CPU
 * fallback.
 */
#ifndef CANU_FE_H
#define CANU_FE_H

#include <stdint.h>

#include "canu_ovl.h" /* ovl_record */

#ifdef __cplusplus
extern "C" {
#endif

#define FE_ABI_VERSION 1

enum {
  FE_OK = 0,
  FE_ERR_NO_DEVICE = -1,
  FE_ERR_BAD_PARAM = -2,
  FE_ERR_UNSUPPORTED = -3,
  FE_ERR_BAD_INPUT = -4,
  FE_ERR_HIP = -5,
  FE_ERR_OOM = -6,
  FE_ERR_STATE = -7
};

/* findErrors' options (findErrors.H:304-337, findErrors.C:381-425). */
typedef struct fe_params {
  double  error_rate;        /* -e  (0.06), a double as atof gives it          */
  int32_t degree_threshold;  /* -d  (2)                                        */
  int32_t kmer_len;          /* -k  (9)                                        */
  int32_t vote_qualify_len;  /* -V  (9)                                        */
  int32_t end_exclude_len;   /* -x  (3)                                        */
  int32_t use_haplo_ct;      /* 1; -p makes it 0                               */
} fe_params;

/* One record of the .red file (correctionOutput.H:40-46): word = keep_left | keep_right << 1 |
 * type << 2 | pos << 6. */
typedef struct fe_correction {
  uint32_t word;
  uint32_t read_id;
} fe_correction;

typedef struct fe_stats {
  uint64_t n_passed, n_failed;   /* the reference's "Passed overlaps" / "Failed overlaps"   */
  uint64_t n_generic;            /* alignments with a row wider than FE_WINDOW_DIAGS        */
  uint64_t n_staged;             /* alignments whose two spans were staged in LDS           */
  uint64_t rows;                 /* edit-distance rows computed (first attempts and re-runs)*/
  uint64_t bases;                /* sum of min(a_part_len, b_part_len) over the overlaps    */
  uint64_t regrows;              /* launches repeated with a larger row log                 */
  uint64_t scratch_bytes;        /* row logs of the last launch                             */
  double   ms_align;             /* k_fe_align, every launch of the call                    */
  double   ms_decide;            /* k_fe_decide, both passes                                */
} fe_stats;

/* Diagonals of one row a wave keeps in registers (one per lane); a wider row reads its
 * predecessor from the row log in global memory. */
#define FE_WINDOW_DIAGS 64
/* Bases of each span a wave can stage in its LDS strands, 2 bits each.  The spans are what the
 * aligner can reach: min(a_part_len, b_part_len + limit) bases of A and min(b_part_len,
 * a_part_len + limit) of B, limit = Error_Bound[min(a_part_len, b_part_len)].  An overlap with
 * a longer span is aligned from global memory. */
#define FE_LDS_BASES 8192
/* Row-log entries (int32) a wave gets per allowed error on the first attempt; an alignment
 * whose rows need more is run again with the worst case, (limit + 1)^2.  Measured on 12 kb
 * reads at 1 % under erate 0.045: 128 holds every alignment, 48 sent the widest to a re-run
 * that took four fifths of the time. */
#define FE_LOG_PER_ERROR 128

typedef struct fe_ctx fe_ctx;

void        fe_params_init(fe_params *p);
const char *fe_last_error(void);
int         fe_abi_version(void);

int  fe_ctx_create(const fe_params *p, int device, fe_ctx **out);
void fe_ctx_destroy(fe_ctx *ctx);
int  fe_set_params(fe_ctx *ctx, const fe_params *p);

/* Reads first_iid .. first_iid+nreads-1: read i is bases[offsets[i] .. offsets[i]+lengths[i]).
 * A second call replaces the reads. */
int fe_load_reads(fe_ctx *ctx, uint32_t first_iid, uint32_t nreads, const uint8_t *bases,
                  const uint64_t *offsets, const uint32_t *lengths);
/* The same with bases and offsets in device memory (lengths on the host), the buffers
 * ovl_load_reads_device and pair_load_reads_device take. */
int fe_load_reads_device(fe_ctx *ctx, uint32_t first_iid, uint32_t nreads,
                         const uint8_t *d_bases, const uint64_t *d_offsets,
                         const uint32_t *h_lengths);

/* findErrors -R bgn_id end_id over these overlaps (any order).  Every a_iid must be in the
 * range, both reads loaded and no hang longer than its read (FE_ERR_BAD_INPUT: the reference
 * reads outside the sequence there).  n == 0 gives the IDENT records alone. */
int fe_find_errors(fe_ctx *ctx, uint32_t bgn_id, uint32_t end_id, const ovl_record *overlaps,
                   uint64_t n, uint64_t *n_corrections);
/* The records of the last fe_find_errors in file order. */
int fe_fetch_corrections(fe_ctx *ctx, fe_correction *out, uint64_t cap, uint64_t *n);
int fe_write_red(fe_ctx *ctx, const char *path);
int fe_get_stats(const fe_ctx *ctx, fe_stats *out);

#ifdef __cplusplus
}
#endif
#endif
