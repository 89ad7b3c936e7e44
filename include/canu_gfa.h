/* canu_gfa.h -- C ABI of libcanu_gfa.so: canu's alignGFA (src/gfa/alignGFA.C), the realignment
 * of graph links and unitig placements after consensus, on one gfx950 device.
 *
 * What it reproduces.  checkLink (alignGFA.C:156-317), per graph link: the two infix
 * (EDLIB_MODE_HW) alignments that move B's end and A's begin, then the global (EDLIB_MODE_NW,
 * EDLIB_TASK_PATH) alignment whose path becomes the link's CIGAR (edlibAlignmentToCigar,
 * EDLIB_CIGAR_STANDARD).  checkRecord / checkRecord_align (:324-537), per unitig placement: the
 * loop of infix alignments against a growing contig window, whole for unitigs shorter than
 * GFA_END_BASES, else for the two ends.  edlib's results are restated in closed form: the
 * distance, the first best end, the longest start, and the path of obtainAlignment's leaf /
 * Hirschberg recursion (edlib.C:945-1404).  The reference's double arithmetic stays on the host
 * (canu_amd/csrc/gfa_host.h).
 *
 * Tigs are ungapped bytes out of "ACGTN".  A reversed tig is the reference's
 * reverseComplementCopy: ACGT are complemented and N becomes NUL, which equals only the NUL of
 * another reversed N.
 *
 * Where the reference asserts or reads outside a sequence the library answers
 * GFA_ERR_BAD_INPUT: a tig ID outside the loaded set, a tig of length 0, alignment lengths that
 * leave a query or target empty, BED coordinates outside the contig.
 *
 * Every call returns GFA_OK (0) or a negative status; gfa_last_error() describes the last
 * failure of the calling thread.  A context is used by one thread at a time.  There is no CPU
 * fallback.
 */
#ifndef CANU_GFA_H
#define CANU_GFA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFA_ABI_VERSION 1

enum {
  GFA_OK = 0,
  GFA_ERR_NO_DEVICE = -1,
  GFA_ERR_BAD_PARAM = -2,
  GFA_ERR_UNSUPPORTED = -3,
  GFA_ERR_BAD_INPUT = -4,
  GFA_ERR_HIP = -5,
  GFA_ERR_OOM = -6,
  GFA_ERR_STATE = -7
};

/* the two tig sets: -T (the tigs of a GFA, the unitigs of a BED) and -C (the contigs of a BED) */
enum { GFA_SET_T = 0, GFA_SET_C = 1 };

#define GFA_END_BASES 50000    /* alignGFA.C:480: a longer unitig is placed by its two ends */
/* obtainAlignment's leaf rule (edlib.C:1191-1193): with nb = ceil(q / 64), a (q, t) problem is
 * traced back directly when 20 * nb * t + 8 * t < GFA_LEAF_BYTES, else split. */
#define GFA_LEAF_BYTES 1048576
#define GFA_MAX_TIGLEN 0x7fff0000  /* int32 coordinates, as there, less a stripe of slack */

typedef struct gfa_params {
  uint64_t hbm_budget;         /* bytes of per-link / per-record device buffers per batch (0: 4 GiB) */
} gfa_params;

typedef struct gfa_link {      /* one L line; the three lengths are gfaLink::alignmentLength's */
  uint32_t a_id, a_fwd;
  uint32_t b_id, b_fwd;
  int32_t  a_align, b_align, align;
} gfa_link;

typedef struct gfa_link_result {
  int32_t  success;            /* the final alignment exists: the link is kept             */
  int32_t  max_edit;           /* ceil(align * 0.12)                                        */
  int32_t  a_len, b_len;
  int32_t  abgn_b, bend_b;     /* extend B: A[abgn_b .. a_len) in B[0 .. bend_b)            */
  int32_t  dist_b;             /* -1: failed                                                */
  int32_t  bend;               /* B's end after it                                          */
  int32_t  abgn_a;             /* extend A: B[0 .. bend) in A[abgn_a .. a_len)              */
  int32_t  dist_a;
  int32_t  abgn;               /* A's begin after it                                        */
  int32_t  dist_f;             /* final: A[abgn .. a_len) against B[0 .. bend), -1: failed  */
  int32_t  align_len;          /* operations of the path (0 when failed)                    */
  uint32_t n_runs;             /* the CIGAR: runs[run_off .. run_off + n_runs)              */
  uint64_t run_off;
  uint32_t n_leaves, n_splits; /* of obtainAlignment's recursion                            */
} gfa_link_result;

typedef struct gfa_run {       /* <count><op>, op one of 'M' 'I' 'D' */
  uint32_t count;
  uint32_t op;
} gfa_run;

typedef struct gfa_record {    /* one BED line: unitig b_id placed at [bgn, end) of contig a_id */
  uint32_t a_id, b_id, b_fwd;
  int32_t  bgn, end;
} gfa_record;

typedef struct gfa_record_result {
  int32_t  success;
  int32_t  bgn, end;           /* the new coordinates (the old ones when failed)            */
  uint32_t n_tries;            /* tries[try_off .. try_off + n_tries), in the order of -V   */
  uint64_t try_off;
} gfa_record_result;

enum { GFA_CALL_ALL = 0, GFA_CALL_LEFT = 1, GFA_CALL_RIGHT = 2 };
enum { GFA_TRY_ACCEPT = 0, GFA_TRY_EXTEND = 1, GFA_TRY_RELAX = 2, GFA_TRY_ABORT = 3 };

typedef struct gfa_try {       /* one pass of checkRecord_align's loop */
  uint32_t record;
  uint32_t call;               /* GFA_CALL_*                                                */
  int32_t  b_len;              /* bases aligned: the unitig, or GFA_END_BASES of it         */
  int32_t  abgn, aend;         /* the window                                                */
  int32_t  max_edit;
  int32_t  dist;               /* -1: no alignment within max_edit                          */
  int32_t  nbgn, nend;         /* where it aligned (when dist >= 0)                         */
  int32_t  outcome;            /* GFA_TRY_*                                                 */
} gfa_try;

typedef struct gfa_stats {
  uint64_t n_links, n_records;
  uint64_t n_alignments;       /* edlibAlign calls restated                                 */
  uint64_t dp_cells;           /* rows x columns of every pass                              */
  uint64_t n_passes;           /* dp passes                                                 */
  uint64_t n_rounds;           /* kernel launches                                           */
  uint64_t n_leaves, n_splits;
  uint64_t n_batches;
  uint64_t scratch_bytes;      /* device scratch of the largest launch                      */
  double   ms_extend_b, ms_extend_a, ms_final, ms_records;
} gfa_stats;

typedef struct gfa_ctx gfa_ctx;

void        gfa_params_init(gfa_params *p);
const char *gfa_last_error(void);
int         gfa_abi_version(void);

int  gfa_ctx_create(const gfa_params *p, int device, gfa_ctx **out);
void gfa_ctx_destroy(gfa_ctx *ctx);
int  gfa_set_params(gfa_ctx *ctx, const gfa_params *p);

/* Tigs 0 .. n-1 of set `which`: tig i is bases[offsets[i] .. offsets[i] + lengths[i]), ungapped;
 * a deleted tig has length 0.  GFA_ERR_BAD_INPUT: a byte outside ACGTN. */
int gfa_load_tigs(gfa_ctx *ctx, int which, uint32_t n, const uint8_t *bases,
                  const uint64_t *offsets, const uint32_t *lengths);

/* checkLink for every link, tigs from GFA_SET_T; results[i] is link i's.  The runs are kept in
 * the context until the next call: gfa_runs_size, then gfa_fetch_runs. */
int gfa_check_links(gfa_ctx *ctx, const gfa_link *links, uint64_t n, gfa_link_result *results);
int gfa_runs_size(const gfa_ctx *ctx, uint64_t *n_runs);
int gfa_fetch_runs(const gfa_ctx *ctx, gfa_run *runs);

/* checkRecord for every record, unitigs from GFA_SET_T and contigs from GFA_SET_C.  The tries
 * are kept in the context until the next call: gfa_tries_size, then gfa_fetch_tries. */
int gfa_check_records(gfa_ctx *ctx, const gfa_record *records, uint64_t n,
                      gfa_record_result *results);
int gfa_tries_size(const gfa_ctx *ctx, uint64_t *n_tries);
int gfa_fetch_tries(const gfa_ctx *ctx, gfa_try *tries);

/* The counters of the last gfa_check_links or gfa_check_records. */
int gfa_get_stats(const gfa_ctx *ctx, gfa_stats *out);

#ifdef __cplusplus
}
#endif
#endif
