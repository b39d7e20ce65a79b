/*
 * vqvdb_hip_bounded.h — error-bounded compression on a vqhip_codec handle (the scalar model): the
 * encode -> decode round trip with each leaf's reconstruction error, the selection of the leaves over a tolerance, the host
 * pair that joins both, and the file pair that writes the leaves over the tolerance raw into a sidecar beside the .vqvdb.
 *
 * Round trip: per chunk the encoder exactly as vqhip_encode_device runs it, the decoder exactly as vqhip_decode_device runs
 * it on that chunk's indices (the small-batch kernels are chosen as in both), then one pass that measures every leaf.  The
 * indices are bit-identical to vqhip_encode_device's, the reconstruction to vqhip_decode_device's of those indices.
 *
 * Leaf error: per leaf VQHIP_ERR_FLOATS float32, {max |x - x^|, sum (x - x^)^2} over its 512 values, x the input, x^ the
 * reconstruction, d = x - x^ in float32.  The sum has a fixed order (unfused float32 products and sums; DESIGN.md §16 spells
 * it out), so a leaf's two numbers depend only on that leaf: the same bits across calls, batch sizes, the leaf's place in the
 * batch, chunk sizes, streams, kernel families and whether the reconstruction is stored.
 *
 * Non-finite values: the maximum keeps NaN, and a difference that is not finite (NaN, or +-inf from an infinite input voxel)
 * counts as NaN.  A leaf with any such value reports NaN as its maximum and is therefore selected at every tolerance,
 * +inf included, and comes back bit-exact from the bounded decompress calls.  Its sum is whatever float32 arithmetic gives
 * (NaN or +inf).  Other leaves of the batch are not affected.
 *
 * Selection: leaf i is an outlier iff !(leaf_err[i][0] <= tol).  Equality is not an outlier; a NaN error or a NaN tol selects
 * the leaf; tol = +inf selects the leaves with a NaN error only.  The ids come out ascending, by a stable compaction without
 * atomics.
 *
 * Guarantee: max |x - decompress_bounded(compress_bounded(x, tol))| <= tol over every finite value, and the selected leaves
 * return bit for bit.
 *
 * The rules of the scalar handle hold (status codes, vqhip_last_error, one call in flight per handle, nothing throws).
 */
#ifndef VQVDB_HIP_BOUNDED_H
#define VQVDB_HIP_BOUNDED_H

#include "vqvdb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQHIP_ERR_FLOATS 2 /* per leaf: max |x - x^|, sum (x - x^)^2 over its 512 values */

/* Device pointers.  leaves_dev [n][512] must stay readable until the call's work on the stream has run: the error pass of
 * every chunk reads it again.  indices_dev [n][64] and recon_dev [n][512] may be NULL: the chunk's indices / reconstruction
 * then live in memory the handle owns (sized to the chunk, freed in vqhip_destroy).  leaf_err_dev [n][VQHIP_ERR_FLOATS] is
 * required.  leaves_dev and recon_dev are 16-byte aligned (any hipMalloc result is).  hip_stream NULL: the handle's stream.
 * n == 0 returns VQHIP_OK and touches nothing. */
int vqhip_roundtrip_device(vqhip_codec* codec, const float* leaves_dev, int64_t n, uint8_t* indices_dev, float* recon_dev,
                           float* leaf_err_dev, void* hip_stream);

/* outlier_ids_dev has room for n ids; the first *count_dev of them are written, ascending.  count_dev is one int64 in
 * device memory.  n is not limited by the chunk.  n == 0 writes *count_dev = 0. */
int vqhip_select_outliers_device(vqhip_codec* codec, const float* leaf_err_dev, int64_t n, float tol, int64_t* outlier_ids_dev,
                                 int64_t* count_dev, void* hip_stream);

/* Host pointers in and out, chunked like vqhip_encode.  Runs the round trip and selects per chunk; the ids are ascending
 * over the whole call.  leaf_err [n][VQHIP_ERR_FLOATS] may be NULL; outlier_ids has room for n ids; *n_outliers receives
 * their number.  n == 0 returns VQHIP_OK with *n_outliers = 0. */
int vqhip_compress_bounded(vqhip_codec* codec, const float* leaves, int64_t n, float tol, uint8_t* indices, float* leaf_err,
                           int64_t* outlier_ids, int64_t* n_outliers);

/* Decodes through the host pipeline of vqhip_decode, then overwrites the leaves outlier_ids (ascending, unique, < n; checked
 * before any GPU work) with outlier_leaves [n_outliers][512].  n == 0 returns VQHIP_OK and touches nothing. */
int vqhip_decompress_bounded(vqhip_codec* codec, const uint8_t* indices, int64_t n, const int64_t* outlier_ids, int64_t n_outliers,
                             const float* outlier_leaves, float* leaves);

/* ---- file pair: the .vqvdb v3 stream of vqhip_compress_file, byte for byte, and a sidecar of raw leaves -------------------
 * Sidecar (.vqres v1, little endian):
 *   file : "VQRES" | u8 version=1 | u8 numGrids | f32 tol
 *   grid : u32 nOutliers | nOutliers x { u32 record_index | f32 leaf[512] }      (grids in the .vqvdb's order)
 * record_index is the leaf's position among that grid's records, ascending.  A reader that ignores the sidecar gets the
 * plain lossy result. */
typedef struct vqhip_bounded_stats {
    int64_t leaves, outliers;   /* leaves seen, leaves written raw                                   */
    float max_err_kept;         /* largest max |x - x^| over the leaves that were NOT selected       */
    double sum_sq_kept;         /* sum (x - x^)^2 over those leaves (a PSNR follows from it)          */
} vqhip_bounded_stats;

/* vqhip_compress_file with a tolerance.  The raw leaves are read from grids[].leaf_ptrs.  stats and bstats may be NULL. */
int vqhip_compress_file_bounded(vqhip_codec* codec, const char* path, const char* residual_path, const vqhip_grid_source* grids,
                                int n_grids, int64_t batch_leaves, float tol, vqhip_stream_stats* stats, vqhip_bounded_stats* bstats);

/* vqhip_decompress_file, then the leaves the sidecar names are overwritten with its floats.  A sidecar whose grid count
 * differs from the .vqvdb's, or with a record_index >= the grid's totalBlocks or not ascending, fails with
 * VQHIP_ERR_INVALID before that entry is written anywhere. */
int vqhip_decompress_file_bounded(vqhip_codec* codec, const char* path, const char* residual_path, int64_t batch_leaves,
                                  vqhip_grid_begin_fn grid_begin, vqhip_leaf_alloc_fn leaf_alloc, void* user, vqhip_stream_stats* stats);

#ifdef __cplusplus
}
#endif

#endif
