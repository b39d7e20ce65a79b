/*
 * vqvdb_hip_residual.h — quantised, bit-packed residuals for the error-bounded compression of a vqhip_codec handle (the
 * scalar model).  vqvdb_hip_bounded.h keeps max |x - x~| <= tol by storing every leaf over the tolerance raw
 * (2048 bytes); these calls store x - x^ of such a leaf on a grid of 1.875 * tol instead, a few bits per voxel, and keep a leaf
 * raw only where that grid cannot hold it.  The calls of vqvdb_hip_bounded.h and the .vqres v1 sidecar are unchanged.
 *
 * Arithmetic, all float32 and never fused (x the input leaf, x^ the decoded leaf, per voxel):
 *   step = 1.875f * tol      d = x - x^      t = d / step      q = rintf(t), ties to even      x~ = x^ + (float)q * step
 *   the voxel verifies iff |t| <= 32767 and |x - x~| <= tol; both comparisons are false on NaN.
 *
 * Classes, one byte per leaf:
 *   VQHIP_RES_KEPT  leaf_err[leaf][0] <= tol (the selection rule of vqvdb_hip_bounded.h): no record, the decoded leaf stands.
 *   0 .. 16         a selected leaf whose 512 voxels all verify: b = the number of bits of max zz(q) over the leaf,
 *                   zz(q) = (q << 1) ^ (q >> 31) on int32; its record has 64 * b bytes.
 *   VQHIP_RES_RAW   any other selected leaf (a non-finite voxel, tol 0 or NaN, a step that is not finite, a residual too wide
 *                   for 16 bits, a voxel that the rounding of x^ + q * step pushed past tol): its record is its 2048 bytes.
 * Nothing but the verification decides between quantised and raw: it is the guarantee.
 *
 * Record of a quantised leaf: bit planes k = 0 .. b-1, least significant first, each eight little-endian u64 words; bit L
 * of word j of plane k, at byte (8 k + j) * 8 of the record, is bit k of zz(q) of voxel 64 j + L.
 *
 * Payload: the records of the selected leaves in leaf order, without gaps; offsets[i] is the byte at which leaf i's record
 * starts (the exclusive sum of the sizes), offsets[n] the payload's size.  Every size is a multiple of 64.
 *
 * Guarantee: max |x - decompress_residual(compress_residual(x, tol))| <= tol over every leaf with finite input, measured
 * with the float32 subtraction of vqvdb_hip_bounded.h; raw leaves return bit for bit, NaN payloads included.  A leaf's class
 * and record depend on that leaf alone: the same bits at every batch size, place in the batch, chunk size and stream.
 *
 * The rules of the scalar handle hold (status codes, vqhip_last_error, one call in flight per handle, nothing throws).
 */
#ifndef VQVDB_HIP_RESIDUAL_H
#define VQVDB_HIP_RESIDUAL_H

#include "vqvdb_hip_bounded.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQHIP_RES_KEPT 254 /* class of a leaf within the tolerance: no record            */
#define VQHIP_RES_RAW 255  /* class of a selected leaf stored as its 2048 bytes           */

/* Device pointers.  leaves_dev, recon_dev [n][512] and leaf_err_dev [n][VQHIP_ERR_FLOATS] are what vqhip_roundtrip_device
 * takes and leaves behind (any x^ and error of the caller's will do: the codec's model is not run).  class_dev [n] bytes,
 * offsets_dev [n + 1] int64, payload_dev 8-byte aligned with room for payload_capacity bytes.  After the call's work on the
 * stream offsets_dev[n] is the payload's size; the caller compares it with its capacity (n * 2048 always suffices).  A record
 * that would end beyond payload_capacity is not written at all, bytes beyond the total are not touched, and nothing is read
 * back to the host inside the call.  hip_stream NULL: the handle's stream.  n == 0 returns VQHIP_OK and touches nothing. */
int vqhip_residual_encode_device(vqhip_codec* codec, const float* leaves_dev, const float* recon_dev, const float* leaf_err_dev, int64_t n,
                                 float tol, uint8_t* class_dev, int64_t* offsets_dev, uint8_t* payload_dev, int64_t payload_capacity,
                                 void* hip_stream);

/* leaves_dev [n][512] holds decoded leaves and is corrected in place: quantised leaves become x^ + q * step, raw leaves their
 * record, kept leaves stay.  The call trusts its device arrays: classes outside {0 .. 16, 254, 255} or offsets that leave
 * payload_dev are not detected.  n == 0 returns VQHIP_OK and touches nothing. */
int vqhip_residual_apply_device(vqhip_codec* codec, float* leaves_dev, int64_t n, float tol, const uint8_t* class_dev,
                                const int64_t* offsets_dev, const uint8_t* payload_dev, void* hip_stream);

/* Host pointers in and out, chunked and serial like vqhip_compress_bounded.  leaf_err [n][VQHIP_ERR_FLOATS] may be NULL;
 * leaf_class [n]; payload has room for n * 2048 bytes and receives the records in leaf order over the whole call,
 * *payload_bytes their size.  n == 0 returns VQHIP_OK with *payload_bytes = 0. */
int vqhip_compress_residual(vqhip_codec* codec, const float* leaves, int64_t n, float tol, uint8_t* indices, float* leaf_err,
                            uint8_t* leaf_class, uint8_t* payload, int64_t* payload_bytes);

/* Decodes and applies the records.  Before any GPU work: every class is in {0 .. 16, 254, 255} and the record sizes sum to
 * payload_bytes, else VQHIP_ERR_INVALID.  n == 0 returns VQHIP_OK and touches nothing. */
int vqhip_decompress_residual(vqhip_codec* codec, const uint8_t* indices, int64_t n, float tol, const uint8_t* leaf_class,
                              const uint8_t* payload, int64_t payload_bytes, float* leaves);

/* ---- file pair: the .vqvdb v3 stream of vqhip_compress_file, byte for byte, and a sidecar of records -----------------------
 * Sidecar (.vqres v2, little endian):
 *   file : "VQRES" | u8 version=2 | u8 numGrids | f32 tol
 *   grid : u32 nRecords | nRecords x { u32 record_index | u8 class | u8 bytes[class==255 ? 2048 : 64*class] }
 * record_index is the leaf's position among that grid's records, ascending; class is 0 .. 16 or 255 (kept leaves have no
 * entry).  A reader that ignores the sidecar gets the plain lossy result. */
typedef struct vqhip_residual_stats {
    int64_t quantised, raw; /* selected leaves stored as bit planes / as their 2048 bytes (bstats->outliers = their sum) */
    int64_t payload_bytes;  /* bytes of all records, without the 5 bytes of framing each                              */
} vqhip_residual_stats;

/* vqhip_compress_file_bounded with quantised records.  bstats->outliers counts the selected leaves.  stats, bstats and
 * rstats may be NULL. */
int vqhip_compress_file_residual(vqhip_codec* codec, const char* path, const char* residual_path, const vqhip_grid_source* grids,
                                 int n_grids, int64_t batch_leaves, float tol, vqhip_stream_stats* stats, vqhip_bounded_stats* bstats,
                                 vqhip_residual_stats* rstats);

/* vqhip_decompress_file with the sidecar's records applied to every decoded batch on the GPU (tol is the sidecar's).  A
 * sidecar whose grid count differs from the .vqvdb's, with a record_index >= the grid's totalBlocks or not above its
 * predecessor, with a class outside {0 .. 16, 255}, or truncated, fails with VQHIP_ERR_INVALID before that entry is applied
 * anywhere. */
int vqhip_decompress_file_residual(vqhip_codec* codec, const char* path, const char* residual_path, int64_t batch_leaves,
                                   vqhip_grid_begin_fn grid_begin, vqhip_leaf_alloc_fn leaf_alloc, void* user, vqhip_stream_stats* stats);

#ifdef __cplusplus
}
#endif

#endif
