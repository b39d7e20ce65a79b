/*
 * vqvdb_hip_vec3_bounded.h — error-bounded compression on a vqhip_vec3_codec handle: the fused
 * encode -> decode round trip with each leaf's reconstruction error, the selection of the leaves over a tolerance, and the
 * host call that joins both.
 *
 * Round trip: the encoder chain and the codebook search exactly as vqhip_vec3_encode_device runs them, then the decoder
 * exactly as vqhip_vec3_decode_device runs it, in the handle's current precision mode (vqvdb_hip_vec3_precision.h) and in
 * chunks like both.  The indices are bit-identical to vqhip_vec3_encode_device's, the reconstruction, when asked for, is
 * bit-identical to vqhip_vec3_decode_device of those indices.
 *
 * Leaf error: per leaf VQHIP_VEC3_ERR_FLOATS float32, {max |x - x^|, sum (x - x^)^2} over its 1536 values, x the input, x^ the
 * reconstruction, d = x - x^ in float32.  The sum has a fixed order (unfused float32 products and sums; DESIGN.md §15 spells
 * it out), so a leaf's two numbers depend only on that leaf: the same bits across calls, batch sizes, the leaf's place in the
 * batch, chunk sizes, streams and whether the reconstruction is stored.
 *
 * Non-finite values: the maximum keeps NaN, and a difference that is not finite (NaN, or +-inf from an infinite input voxel)
 * counts as NaN.  A leaf with any such value reports NaN as its maximum and is therefore selected at every tolerance,
 * +inf included.  Its sum is whatever float32 arithmetic gives (NaN or +inf).  Other leaves of the batch are not affected.
 *
 * Selection: leaf i is an outlier iff !(leaf_err[i][0] <= tol).  Equality is not an outlier; a NaN error or a NaN tol selects
 * the leaf; tol = +inf selects the leaves with a NaN error only.  The ids come out ascending, by a stable compaction without
 * atomics.
 *
 * The rules of the Vec3 handle hold (status codes, vqhip_vec3_last_error, one call in flight per handle).
 */
#ifndef VQVDB_HIP_VEC3_BOUNDED_H
#define VQVDB_HIP_VEC3_BOUNDED_H

#include "vqvdb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQHIP_VEC3_ERR_FLOATS 2 /* per leaf: max |x - x^|, sum (x - x^)^2 over its 1536 values */

/* Device pointers.  leaves_dev [n][512][3] must stay readable until the call's work on the stream has run: the tail of
 * every chunk reads it again.  indices_dev [n][64] may be NULL (the indices then stay in the workspace).  recon_dev
 * [n][512][3] may be NULL: then no reconstruction is stored.  leaf_err_dev [n][VQHIP_VEC3_ERR_FLOATS] is required.
 * hip_stream NULL: the handle's stream.  n == 0 returns VQHIP_OK and touches nothing. */
int vqhip_vec3_roundtrip_device(vqhip_vec3_codec* c, const float* leaves_dev, int64_t n, uint16_t* indices_dev, float* recon_dev,
                                float* leaf_err_dev, void* hip_stream);

/* outlier_ids_dev has room for n ids; the first *count_dev of them are written, ascending.  count_dev is one int64 in
 * device memory.  n is not limited by the chunk.  n == 0 writes *count_dev = 0. */
int vqhip_vec3_select_outliers_device(vqhip_vec3_codec* c, const float* leaf_err_dev, int64_t n, float tol, int64_t* outlier_ids_dev,
                                      int64_t* count_dev, void* hip_stream);

/* Host pointers in and out, chunked like vqhip_vec3_encode.  Runs the round trip without storing a reconstruction and
 * selects per chunk; the ids are ascending over the whole call.  leaf_err [n][VQHIP_VEC3_ERR_FLOATS] may be NULL;
 * outlier_ids has room for n ids; *n_outliers receives their number.  n == 0 returns VQHIP_OK with *n_outliers = 0. */
int vqhip_vec3_compress_bounded(vqhip_vec3_codec* c, const float* leaves, int64_t n, float tol, uint16_t* indices, float* leaf_err,
                                int64_t* outlier_ids, int64_t* n_outliers);

#ifdef __cplusplus
}
#endif

#endif
