/*
 * vqvdb_hip_vec3_rate.h — the size sweep of a vqhip_vec3_codec handle's quantised residuals and a compress into a byte budget
 * (the scalar handle's form of both is DESIGN.md §19).  vqvdb_hip_vec3_residual.h answers "given a tolerance, how
 * many bytes?"; these calls answer the converse: the histogram of the leaves over their record sizes at up to
 * VQHIP_VEC3_RATE_MAX_TOLS tolerances ("rungs") in one pass over them, from which the payload of a compress at each rung follows
 * to the byte, and a compress that picks the tightest rung whose payload fits a budget.  No call, kernel or format of the other
 * headers changes.  These calls work in memory (on disk: vqvdb_hip_vec3_file.h); there is no sidecar, hence no sidecar size.
 *
 * Histogram: int64 [n_tols][VQHIP_VEC3_RATE_CLASSES], row t for tols[t].  Column s = 0 .. 48 counts the quantised leaves whose
 * code b0 | b1 << 5 | b2 << 10 has s = b0 + b1 + b2 planes (a record of 64 * s bytes), column 49 the raw leaves
 * (VQHIP_VEC3_RES_RAW, 6144 bytes), column 50 the kept leaves (VQHIP_VEC3_RES_KEPT, no record): exactly the codes that
 * vqhip_vec3_residual_encode_device gives at that tolerance, leaf by leaf.  Every row sums to the number of leaves.  Any float is
 * a legal rung, in any order: duplicates, 0, negative values, NaN (every leaf raw) and +inf (only leaves with a NaN error are
 * selected) included.
 *
 * Sizes are integer sums of the row: equal to what a compress at that rung writes, not an estimate.
 *
 * Precision mode: a histogram belongs to the x^ of the mode (vqvdb_hip_vec3_precision.h) that made it, as the records do.
 *
 * The rules of the Vec3 handle hold (status codes, vqhip_vec3_last_error, one call in flight per handle, nothing throws).
 */
#ifndef VQVDB_HIP_VEC3_RATE_H
#define VQVDB_HIP_VEC3_RATE_H

#include "vqvdb_hip_vec3_residual.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQHIP_VEC3_RATE_MAX_TOLS 64 /* rungs of one sweep at the most                                          */
#define VQHIP_VEC3_RATE_CLASSES 51  /* columns of a histogram row: 0 .. 48 quantised by planes, 49 raw, 50 kept */

/* Pure host arithmetic on one histogram row: no handle, no device.  The sum of 64 * s * row[s] over s = 0 .. 48, plus
 * 6144 * row[49], in 64 bits: *payload_bytes of vqhip_vec3_residual_compress at that rung.  A NULL row gives -1. */
int64_t vqhip_vec3_rate_payload_bytes(const int64_t* hist_row);

/* Device pointers but tols.  leaves_dev, recon_dev [n][512][3] and leaf_err_dev [n][VQHIP_VEC3_ERR_FLOATS] are what
 * vqhip_vec3_roundtrip_device takes and leaves behind; the codec's model is not run.  tols [n_tols] is host memory, read before
 * the call returns.  hist_dev [n_tols][VQHIP_VEC3_RATE_CLASSES] int64: the call ADDS the counts of its n leaves to it and never
 * clears it, so the caller zeroes it before the first call and several calls (chunks, streams in order) accumulate into one
 * histogram without a read-back; rows at and beyond n_tols are not touched.  The sums are integers: the same bits for every
 * split of the leaves over calls.  Nothing is read back and nothing is synchronised inside the call.  hip_stream NULL: the
 * handle's stream.  n_tols outside 1 .. VQHIP_VEC3_RATE_MAX_TOLS returns VQHIP_ERR_INVALID; then n == 0 returns VQHIP_OK and
 * touches nothing; then a null pointer returns VQHIP_ERR_INVALID. */
int vqhip_vec3_rate_sweep_device(vqhip_vec3_codec* c, const float* leaves_dev, const float* recon_dev, const float* leaf_err_dev, int64_t n,
                                 const float* tols, int n_tols, int64_t* hist_dev, void* hip_stream);

/* Host pointers, in the handle's precision mode.  Chunked and serial like vqhip_vec3_residual_compress: per chunk the round trip,
 * then the sweep; the histogram stays on the device (in memory the handle owns, freed in vqhip_vec3_destroy) and is read back
 * once at the end.  hist [n_tols][VQHIP_VEC3_RATE_CLASSES] is overwritten.  n == 0 writes zeros. */
int vqhip_vec3_rate_sweep(vqhip_vec3_codec* c, const float* leaves, int64_t n, const float* tols, int n_tols, int64_t* hist);

/* Compress into a payload budget.  Pass 1 is vqhip_vec3_rate_sweep over tols, which also brings every chunk's indices to
 * `indices` [n][64] and its leaf errors to `leaf_err` [n][VQHIP_VEC3_ERR_FLOATS] (NULL: to a host buffer of the call's own).
 * vqhip_vec3_rate_pick then chooses the SMALLEST tols[t] by value whose payload has at most payload_budget bytes; *tol_used
 * receives it.  Pass 2 does not run the encoder: per chunk it uploads the leaves, pass 1's indices and errors, decodes the
 * indices, and encodes the records at the chosen tolerance.  indices, leaf_err, leaf_code [n], payload (room for n * 6144
 * bytes) and *payload_bytes end as vqhip_vec3_residual_compress(c, leaves, n, *tol_used, ...) leaves them, byte for byte.
 * The budget is the payload's alone: indices (128 bytes per leaf) and codes (2 bytes per leaf) do not depend on the tolerance.
 * If no rung fits, the call returns VQHIP_ERR_INVALID before pass 2 with *payload_bytes = 0; leaf_code, payload and *tol_used
 * are untouched, indices and leaf_err hold pass 1's values, and vqhip_vec3_last_error names the smallest size found and the
 * budget.  hist [n_tols][VQHIP_VEC3_RATE_CLASSES] may be NULL; tol_used and payload_bytes may not.  payload_budget < 0 is
 * invalid.  n == 0 returns VQHIP_OK with *payload_bytes = 0 and, where hist is given, a histogram of zeros; every rung then needs
 * 0 bytes, and *tol_used receives the smallest that is not NaN, if there is one. */
int vqhip_vec3_rate_compress(vqhip_vec3_codec* c, const float* leaves, int64_t n, const float* tols, int n_tols, int64_t payload_budget,
                             float* tol_used, int64_t* hist, uint16_t* indices, float* leaf_err, uint16_t* leaf_code, uint8_t* payload,
                             int64_t* payload_bytes);

/* Pure host arithmetic: the index of the smallest tols[t] by value whose row of hist [n_tols][VQHIP_VEC3_RATE_CLASSES] has a
 * payload of at most payload_budget bytes.  The sizes are not assumed to fall as the tolerance grows (raw leaves can make them
 * rise); NaN rungs are never chosen; of duplicate rungs the first is returned.  -1 if no rung fits or an argument is invalid
 * (a NULL pointer, n_tols outside 1 .. VQHIP_VEC3_RATE_MAX_TOLS, payload_budget < 0).  For callers that sweep on the device. */
int vqhip_vec3_rate_pick(const int64_t* hist, const float* tols, int n_tols, int64_t payload_budget);

#ifdef __cplusplus
}
#endif

#endif
