/* canu_fs.h -- C ABI of libcanu_fs.so: canu's falconsense (src/correction/falconsense.C,
 * falconConsensus*.C), the consensus step of read correction, on one gfx950 device.
 *
 * What it reproduces, per correction layout (a template read and its evidence reads, the tig
 * of the corStore): generateFalconConsensus (falconsense.C:91-192) -- every child oriented and
 * trimmed by askip / bskip, cut to the template's length, left out below 500 bases --
 * alignReadsToTemplate (falconConsensus-alignTag.C:120-232) with edlib's EDLIB_MODE_HW /
 * EDLIB_TASK_PATH result restated in closed form (distance, first best end, longest start, the
 * path of obtainAlignment's leaf / Hirschberg recursion, edlib.C:945-1404), getAlignTags, and
 * getConsensus (falconConsensus.C:76-310): coverage, links in order of first appearance, the
 * scan, the walk back -- whose first letter is chosen by the index of the best link, as there
 * -- and the lower case at or below min_coverage.  fs_write_fasta splits at lower case and
 * writes the pieces longer than min_output_length as the reference does.
 *
 * Where the reference dies, the library answers: a template none of whose evidence aligns
 * (one shorter than 500, say) gives an empty consensus (assert(g_best_score > DBL_MIN));
 * more than 65,535 children is FS_ERR_BAD_INPUT (uint16 counts); the reverse complement of N is
 * N (the reference's table gives NUL, and its next assertion fails).
 *
 * Reads are bytes out of "ACGTN", read IDs as in the gkpStore.  Every call returns FS_OK (0) or
 * a negative status; fs_last_error() describes the last failure of the calling thread.  A
 * context is used by one thread at a time.  There is no CPU fallback.
 */
#ifndef CANU_FS_H
#define CANU_FS_H

#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS_ABI_VERSION 1

enum {
  FS_OK = 0,
  FS_ERR_NO_DEVICE = -1,
  FS_ERR_BAD_PARAM = -2,
  FS_ERR_UNSUPPORTED = -3,
  FS_ERR_BAD_INPUT = -4,
  FS_ERR_HIP = -5,
  FS_ERR_OOM = -6,
  FS_ERR_STATE = -7
};

#define FS_MIN_EVIDENCE 500    /* falconConsensus-alignTag.C:144 */
#define FS_MAX_CHILDREN 65535  /* coverage and link counts are uint16 there */
/* obtainAlignment's leaf rule (edlib.C:1191-1193): with nb = ceil(q / 64), a (q, t) problem is
 * traced back directly when 20 * nb * t + 8 * t < FS_LEAF_BYTES, else split.  A wave's leaf
 * scratch is therefore fixed: FS_LEAF_BYTES / 20 block columns. */
#define FS_LEAF_BYTES 1048576

typedef struct fs_params {
  uint32_t min_coverage;       /* -cc (4): a base with coverage <= this is lower case   */
  double   min_identity;       /* -ci as a double; the program's atoi makes canu's 0.x 0 */
  uint32_t min_output_length;  /* -cl (500): a piece must be longer                      */
  uint64_t hbm_budget;         /* bytes of device scratch per batch of layouts (0: 4 GiB) */
} fs_params;

typedef struct fs_layout {
  uint32_t tig_id;             /* the template read */
  uint32_t first_child;        /* into the children array */
  uint32_t n_children;
} fs_layout;

typedef struct fs_child {      /* tgPosition: ident, isReverse, min, max, askip, bskip */
  uint32_t ident;
  uint32_t reverse;
  int32_t  min, max;
  int32_t  askip, bskip;
} fs_child;

typedef struct fs_stats {
  uint64_t n_layouts, n_evidence;          /* evidence reads, templates included            */
  uint64_t n_aligned, n_skipped, n_rejected;
  uint64_t n_tags;
  uint64_t dp_cells;                       /* rows x columns of every pass                  */
  uint64_t n_leaves, n_splits;
  uint64_t n_batches;
  uint64_t scratch_bytes;                  /* device scratch of the largest batch           */
  double   ms_locate, ms_path, ms_sort, ms_consensus;
} fs_stats;

typedef struct fs_ctx fs_ctx;

void        fs_params_init(fs_params *p);
const char *fs_last_error(void);
int         fs_abi_version(void);

int  fs_ctx_create(const fs_params *p, int device, fs_ctx **out);
void fs_ctx_destroy(fs_ctx *ctx);
int  fs_set_params(fs_ctx *ctx, const fs_params *p);

/* Reads first_iid .. first_iid+nreads-1: read i is bases[offsets[i] .. offsets[i]+lengths[i]). */
int fs_load_reads(fs_ctx *ctx, uint32_t first_iid, uint32_t nreads, const uint8_t *bases,
                  const uint64_t *offsets, const uint32_t *lengths);
/* The same with bases and offsets in device memory (lengths on the host), the buffers
 * co_load_reads_device takes. */
int fs_load_reads_device(fs_ctx *ctx, uint32_t first_iid, uint32_t nreads,
                         const uint8_t *d_bases, const uint64_t *d_offsets,
                         const uint32_t *h_lengths);

/* The consensus of every layout, in order.  FS_ERR_BAD_INPUT: a template or child that is not
 * loaded, skips that are negative or longer than the read, max <= min, more than
 * FS_MAX_CHILDREN children. */
int fs_consensus(fs_ctx *ctx, const fs_layout *layouts, uint64_t n_layouts,
                 const fs_child *children, uint64_t n_children);
/* The size of the last result, then the result: layout i's consensus (with its lower case) is
 * bases[offsets[i] .. offsets[i+1]), and counts[3*i ..] its evidence reads aligned, skipped
 * (< FS_MIN_EVIDENCE) and rejected, the template among them.  Any pointer may be null. */
int fs_result_size(const fs_ctx *ctx, uint64_t *n_layouts, uint64_t *n_bases);
int fs_fetch(const fs_ctx *ctx, uint8_t *bases, uint64_t *offsets, uint32_t *counts);
/* The corrected reads of the last result as falconsense writes them to stdout. */
int fs_write_fasta_file(const fs_ctx *ctx, FILE *f);
int fs_write_fasta(const fs_ctx *ctx, const char *path);
int fs_get_stats(const fs_ctx *ctx, fs_stats *out);

#ifdef __cplusplus
}
#endif
#endif
