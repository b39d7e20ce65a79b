/*
 * vqvdb_hip_rate.h — the size sweep of the scalar handle's quantised residuals and a compress into a byte budget (DESIGN.md
 * §19).  vqvdb_hip_residual.h answers "given a tolerance, how many bytes?"; these calls answer the converse: the class
 * histogram of the leaves at up to VQHIP_RATE_MAX_TOLS tolerances ("rungs") in one pass over them, from which the payload and
 * the .vqres v2 sidecar of a compress at each rung follow to the byte, and a file compress that picks the tightest rung whose
 * sidecar fits a budget.  No call, kernel or file format of the other headers changes.
 *
 * Histogram: int64 [n_tols][VQHIP_RATE_CLASSES], row t for tols[t].  Column k = 0 .. 16 counts the leaves of class k (quantised,
 * a record of 64 * k bytes), column 17 the raw leaves (VQHIP_RES_RAW, 2048 bytes), column 18 the kept leaves (VQHIP_RES_KEPT,
 * no record): exactly the classes that vqhip_residual_encode_device gives at that tolerance, leaf by leaf.  Every row sums to
 * the number of leaves.  Any float is a legal rung, in any order: duplicates, 0, negative values, NaN (every leaf raw) and
 * +inf (only leaves with a NaN error are selected) included.
 *
 * Sizes are integer sums of the row: equal to what a compress at that rung writes, not an estimate.
 *
 * The rules of the scalar handle hold (status codes, vqhip_last_error, one call in flight per handle, nothing throws).
 */
#ifndef VQVDB_HIP_RATE_H
#define VQVDB_HIP_RATE_H

#include "vqvdb_hip_residual.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQHIP_RATE_MAX_TOLS 64 /* rungs of one sweep at the most                                  */
#define VQHIP_RATE_CLASSES 19  /* columns of a histogram row: 0 .. 16 quantised, 17 raw, 18 kept  */

/* Pure host arithmetic on one histogram row: no handle, no device.  A NULL row gives -1.
 * payload: the sum of 64 * b * row[b] over b = 0 .. 16, plus 2048 * row[17] (vqhip_residual_stats.payload_bytes).
 * sidecar: 11 + 4 * n_grids + 5 * (row[0] + .. + row[17]) + payload, the size of the .vqres v2 file of n_grids grids. */
int64_t vqhip_rate_payload_bytes(const int64_t* hist_row);
int64_t vqhip_rate_sidecar_bytes(const int64_t* hist_row, int n_grids);

/* Device pointers but tols.  leaves_dev, recon_dev [n][512] and leaf_err_dev [n][VQHIP_ERR_FLOATS] are what
 * vqhip_roundtrip_device takes and leaves behind; the codec's model is not run.  tols [n_tols] is host memory, read before the
 * call returns.  hist_dev [n_tols][VQHIP_RATE_CLASSES] int64: the call ADDS the counts of its n leaves to it and never clears
 * it, so the caller zeroes it before the first call and several calls (chunks, streams in order) accumulate into one histogram
 * without a read-back; rows at and beyond n_tols are not touched.  The sums are integers: the same bits for every split of the
 * leaves over calls.  Nothing is read back and nothing is synchronised inside the call.  hip_stream NULL: the handle's
 * stream.  n_tols outside 1 .. VQHIP_RATE_MAX_TOLS returns VQHIP_ERR_INVALID; then n == 0 returns VQHIP_OK and touches
 * nothing; then a null pointer returns VQHIP_ERR_INVALID. */
int vqhip_rate_sweep_device(vqhip_codec* codec, const float* leaves_dev, const float* recon_dev, const float* leaf_err_dev, int64_t n,
                            const float* tols, int n_tols, int64_t* hist_dev, void* hip_stream);

/* Host pointers.  Chunked and serial like vqhip_compress_residual: per chunk the round trip, then the sweep; the histogram
 * stays on the device (in memory the handle owns, freed in vqhip_destroy) and is read back once at the end.  hist
 * [n_tols][VQHIP_RATE_CLASSES] is overwritten.  n == 0 writes zeros. */
int vqhip_rate_sweep(vqhip_codec* codec, const float* leaves, int64_t n, const float* tols, int n_tols, int64_t* hist);

/* The sweep over the grids of a file compress, through the host pipeline of vqhip_compress_file: gather, encode, decode,
 * measure and sweep every batch.  No file is opened and nothing is written; hist [n_tols][VQHIP_RATE_CLASSES] is overwritten
 * with the histogram of all grids together, read back once after the last grid.  Row t then predicts
 * vqhip_compress_file_residual at tols[t] on the same grids: vqhip_rate_sidecar_bytes is its sidecar's size, the payload,
 * quantised, raw and outlier counts of its statistics are the row's sums.  stats may be NULL. */
int vqhip_rate_sweep_file(vqhip_codec* codec, const vqhip_grid_source* grids, int n_grids, int64_t batch_leaves, const float* tols,
                          int n_tols, int64_t* hist, vqhip_stream_stats* stats);

/* Compress into a sidecar budget: vqhip_rate_sweep_file over tols, then vqhip_compress_file_residual at the SMALLEST tols[t]
 * by value whose predicted sidecar has at most sidecar_budget bytes; *tol_used receives it.  The sizes are not assumed to fall
 * as the tolerance grows (raw leaves can make them rise); NaN rungs are never chosen.  The .vqvdb's size does not depend on
 * the tolerance, so the budget is the sidecar's alone.  If no rung fits, the call returns VQHIP_ERR_INVALID before any file is
 * opened, and vqhip_last_error names the smallest size found and the budget.  The second pass runs the model again, so the
 * call costs about twice vqhip_compress_file_residual.  hist [n_tols][VQHIP_RATE_CLASSES] may be NULL; stats, bstats and rstats
 * (of the compress pass) may be NULL. */
int vqhip_rate_compress_file(vqhip_codec* codec, const char* path, const char* residual_path, const vqhip_grid_source* grids, int n_grids,
                             int64_t batch_leaves, const float* tols, int n_tols, int64_t sidecar_budget, float* tol_used, int64_t* hist,
                             vqhip_stream_stats* stats, vqhip_bounded_stats* bstats, vqhip_residual_stats* rstats);

#ifdef __cplusplus
}
#endif

#endif
