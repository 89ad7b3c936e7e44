/* canu_co.h -- C ABI of libcanu_co.so: canu's correctOverlaps (the second half of overlap
 * error adjustment, src/overlapErrorAdjustment/correctOverlaps*.C) on one gfx950 device.
 *
 * What it reproduces: Correct_Frags / correctRead (correctOverlaps-Correct_Frags.C:38-179)
 * applies the corrections of a .red file to every loaded read; Redo_Olaps
 * (correctOverlaps-Redo_Olaps.C:273-553) then realigns every overlap of a read range on the
 * corrected reads -- Hang_Adjust, correctOverlaps' own Prefix_Edit_Dist
 * (correctOverlaps-Prefix_Edit_Distance.C:165-312), the leading-gap trim, the failure tests --
 * and gives the 12-bit evalue of each overlap, AS_OVS_encodeEvalue(errors / olapLen), or the
 * evalue the overlap came with where the realignment failed.  The evalues in input order are
 * the content of the .oea file (correctOverlaps.C:203-215) that ovStoreBuild -evalues adds to
 * the store.
 *
 * Read bytes outside "ACGTacgt" become 'a'.  Overlaps use the ovOverlap layout of canu_ovl.h
 * (ovl_record); the IDs, the four hangs, the flipped bit and the evalue are read.  Corrections
 * are the records of canu_fe.h (fe_correction), ascending by read.
 *
 * Every call returns CO_OK (0) or a negative status; co_last_error() describes the last
 * failure of the calling thread.  A context is used by one thread at a time.  There is no CPU
 * fallback.
 */
#ifndef CANU_CO_H
#define CANU_CO_H

#include <stdint.h>

#include "canu_fe.h"  /* fe_correction */
#include "canu_ovl.h" /* ovl_record */

#ifdef __cplusplus
extern "C" {
#endif

#define CO_ABI_VERSION 1

enum {
  CO_OK = 0,
  CO_ERR_NO_DEVICE = -1,
  CO_ERR_BAD_PARAM = -2,
  CO_ERR_UNSUPPORTED = -3,
  CO_ERR_BAD_INPUT = -4,
  CO_ERR_HIP = -5,
  CO_ERR_OOM = -6,
  CO_ERR_STATE = -7
};

/* correctOverlaps' one option that changes the result (correctOverlaps.C:70-71). */
typedef struct co_params {
  double error_rate; /* -e  (0.06), a double as atof gives it */
} co_params;

typedef struct co_stats {
  /* the nine counters Redo_Olaps prints (correctOverlaps-Redo_Olaps.C:543-552) */
  uint64_t olaps_fwd, olaps_rev, total;
  uint64_t failed_both, failed_either, failed_end, failed_length;
  uint64_t rha_fail, rha_pass;
  /* the "Corrected ... bases with ..." line of Correct_Frags (:327-331), over the A reads of
   * the last range; the base count has one terminator per read */
  uint64_t corrected_bases, substitutions, deletions, insertions;
  uint64_t rows;          /* edit-distance rows computed (first attempts and re-runs)   */
  uint64_t bases;         /* sum of min(a_part_len, b_part_len) over the overlaps       */
  uint64_t regrows;       /* launches repeated with a larger row log                    */
  uint64_t n_staged;      /* alignments whose two spans were staged in LDS              */
  uint64_t n_generic;     /* alignments with a row wider than CO_WINDOW_DIAGS           */
  uint64_t scratch_bytes; /* row logs of the last launch                                */
  double   ms_correct;    /* k_co_correct, the last co_set_corrections                  */
  double   ms_align;      /* k_co_align, every launch of the last co_correct_overlaps   */
} co_stats;

/* Diagonals of one row a wave keeps in registers (one per lane); a wider row reads its
 * predecessor from the row log in global memory. */
#define CO_WINDOW_DIAGS 64
/* Bases of each span a wave can stage in its LDS strands, 2 bits each: min(a_part_len,
 * b_part_len + limit) bases of A and min(b_part_len, a_part_len + limit) of B, limit =
 * Error_Bound[min(a_part_len, b_part_len)].  An overlap with a longer span is aligned from
 * global memory. */
#define CO_LDS_BASES 8192
/* Row-log entries (int32) a wave gets per allowed error on the first attempt; an alignment
 * whose rows need more is run again with the worst case, (limit + 1)^2.  The figure is
 * k_fe_align's: the aligner and the reads are the same. */
#define CO_LOG_PER_ERROR 128

typedef struct co_ctx co_ctx;

void        co_params_init(co_params *p);
const char *co_last_error(void);
int         co_abi_version(void);

int  co_ctx_create(const co_params *p, int device, co_ctx **out);
void co_ctx_destroy(co_ctx *ctx);
int  co_set_params(co_ctx *ctx, const co_params *p);

/* Reads first_iid .. first_iid+nreads-1: read i is bases[offsets[i] .. offsets[i]+lengths[i]).
 * A second call replaces the reads and drops the corrections. */
int co_load_reads(co_ctx *ctx, uint32_t first_iid, uint32_t nreads, const uint8_t *bases,
                  const uint64_t *offsets, const uint32_t *lengths);
/* The same with bases and offsets in device memory (lengths on the host), the buffers
 * fe_load_reads_device takes. */
int co_load_reads_device(co_ctx *ctx, uint32_t first_iid, uint32_t nreads,
                         const uint8_t *d_bases, const uint64_t *d_offsets,
                         const uint32_t *h_lengths);

/* The records of a .red file, ascending by read (CO_ERR_BAD_INPUT otherwise).  Corrects every
 * loaded read on the device.  A loaded read without an IDENT record, or with a correction that
 * trips correctRead's position assertion (:95-96) or is of no vote type, is remembered and
 * refused when an overlap needs it. */
int co_set_corrections(co_ctx *ctx, const fe_correction *red, uint64_t n);

/* correctOverlaps -R bgn_id end_id over these overlaps (any order): evalues[i] belongs to
 * overlaps[i].  CO_ERR_BAD_INPUT: an a_iid outside the range, a read that is not loaded, a
 * needed read refused by co_set_corrections, a hang longer than its read or an adjusted hang
 * past the end of its corrected read (the reference reads outside the string there).  n == 0
 * gives an empty result. */
int co_correct_overlaps(co_ctx *ctx, uint32_t bgn_id, uint32_t end_id, const ovl_record *overlaps,
                        uint64_t n, uint16_t *evalues);
/* The .oea file of the last co_correct_overlaps: int32 bgn_id, int32 end_id, uint64 n,
 * uint16 evalue[n]. */
int co_write_oea(co_ctx *ctx, const char *path);
int co_get_stats(const co_ctx *ctx, co_stats *out);

#ifdef __cplusplus
}
#endif
#endif
