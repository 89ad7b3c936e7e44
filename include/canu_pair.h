/* canu_pair.h -- C ABI of libcanu_pair.so: canu's overlapPair (src/overlapInCore/overlapPair.C),
 * the exact realignment of MHAP / minimap overlaps (corMhapReAlign, obtMhapReAlign,
 * utgMhapReAlign; OverlapMhap.pm:522-537), on one gfx950 device.
 *
 * What it reproduces: recomputeOverlaps (overlapPair.C:346-662) per overlap, in input order --
 * the two extendAlignment calls with MHAP_SLOP, the four dovetail extensions, finalAlignment,
 * the error-rate test and the flags -- with edlib's results restated in closed form:
 *   infix  (EDLIB_MODE_HW):  best = min over end columns j of ED(query, any substring of the
 *           target ending at j); fails iff best > k; end = the smallest such j; start = the
 *           smallest s with ED(query, target[s..end]) == best
 *   global (EDLIB_MODE_NW):  the edit distance; fails iff > k
 * Bases compare by value; N equals only N.  Records keep the ovOverlap layout of canu_ovl.h
 * (ovl_record) and the output order is the input order.
 *
 * Reads are bytes out of "ACGTN"; anything else is PAIR_ERR_BAD_INPUT (the gkpStore holds
 * nothing else).  An overlap whose hangs exceed its read, or that names a read that is not
 * loaded, is PAIR_ERR_BAD_INPUT: the reference reads outside the sequence there.
 * min_overlap_length 0 is PAIR_ERR_BAD_PARAM (the reference hands edlib empty sequences).
 *
 * Every call returns PAIR_OK (0) or a negative status; pair_last_error() describes the last
 * failure of the calling thread.  A context is used by one thread at a time.  There is no CPU
 * fallback.
 */
#ifndef CANU_PAIR_H
#define CANU_PAIR_H

#include <stdint.h>

#include "canu_ovl.h" /* ovl_record */

#ifdef __cplusplus
extern "C" {
#endif

#define PAIR_ABI_VERSION 1

enum {
  PAIR_OK = 0,
  PAIR_ERR_NO_DEVICE = -1,
  PAIR_ERR_BAD_PARAM = -2,
  PAIR_ERR_UNSUPPORTED = -3,
  PAIR_ERR_BAD_INPUT = -4,
  PAIR_ERR_HIP = -5,
  PAIR_ERR_OOM = -6,
  PAIR_ERR_STATE = -7
};

/* overlapPair's options (overlapPair.C:680-729). */
typedef struct pair_params {
  double   max_erate;           /* -erate   (0.12)                                */
  uint32_t min_overlap_length;  /* -len     (the reference's 0 is refused: 1)     */
  int32_t  partial;             /* -partial                                       */
  int32_t  invert;              /* -invert                                        */
} pair_params;

/* alignStats::reportFinal's counters (overlapPair.C:138-153) of the last pair_realign, the
 * DP cells of its alignments (query rows x target columns of every pass) and the device time
 * of k_pair. */
typedef struct pair_stats {
  uint64_t n_skipped, n_passed, n_failed;
  uint64_t n_fail_ext_a, n_fail_ext_b, n_fail_ext;
  uint64_t n_partial, n_dovetail;
  uint64_t n_ext5a, n_ext3a, n_ext5b, n_ext3b;
  uint64_t dp_cells;
  uint64_t dp_passes;
  uint64_t dp_steps;            /* wavefront steps of those passes: one 64-row block column per
                                   active lane each (columns + lanes - 1 per stripe) */
  uint64_t scratch_bytes;       /* global boundary rows (targets longer than PAIR_LDS_COLUMNS) */
  double   ms_kernel;
} pair_stats;

/* Target columns whose stripe-boundary row (2 bits each) a wave keeps in LDS; a longer target
 * under a query of more than one stripe (PAIR_STRIPE_ROWS rows) uses a global scratch row. */
#define PAIR_LDS_COLUMNS 16384
#define PAIR_STRIPE_ROWS 4096

typedef struct pair_ctx pair_ctx;

void        pair_params_init(pair_params *p);
const char *pair_last_error(void);
int         pair_abi_version(void);

int  pair_ctx_create(const pair_params *p, int device, pair_ctx **out);
void pair_ctx_destroy(pair_ctx *ctx);
int  pair_set_params(pair_ctx *ctx, const pair_params *p);

/* Reads first_iid .. first_iid+nreads-1: read i is bases[offsets[i] .. offsets[i]+lengths[i]). */
int pair_load_reads(pair_ctx *ctx, uint32_t first_iid, uint32_t nreads, const uint8_t *bases,
                    const uint64_t *offsets, const uint32_t *lengths);
/* The same with bases and offsets in device memory (lengths on the host), the buffers
 * ovl_load_reads_device takes. */
int pair_load_reads_device(pair_ctx *ctx, uint32_t first_iid, uint32_t nreads,
                           const uint8_t *d_bases, const uint64_t *d_offsets,
                           const uint32_t *h_lengths);

/* recomputeOverlaps over in[0..n): out[i] is in[i] realigned (out may be in). */
int pair_realign(pair_ctx *ctx, const ovl_record *in, uint64_t n, ovl_record *out);
int pair_get_stats(const pair_ctx *ctx, pair_stats *out);

#ifdef __cplusplus
}
#endif
#endif
