/*
 * vqvdb_hip_vec3_active.h — compact records for the quantised residuals of a vqhip_vec3_codec handle: records
 * that hold only the ACTIVE voxels of a leaf, and a decode side that knows the mask.  The masked calls of vqvdb_hip_vec3_mask.h
 * write a record of 512 voxels whatever the mask; here a record shrinks with the leaf's active count, and apply can write a
 * background into the inactive voxels.  On disk: the .vqv3 container of vqvdb_hip_vec3_file.h.  The scalar handle has no such calls.
 *
 * Mask.  As in vqvdb_hip_vec3_mask.h: uint64 [n][8], little endian, bit L of word j of a leaf is voxel 64 j + L, one bit for the
 * three channels of its voxel; device masks are 8-byte aligned.  Encode and decode must be given the same masks.
 *
 * Notation.  A = the popcount of a leaf's eight words, W = ceil(A / 64), the rank of an active voxel = the number of active voxels
 * of the leaf with a smaller index.
 *
 * Codes.  Unchanged: a leaf's code is the one the masked encode of vqvdb_hip_vec3_mask.h gives on the same arrays (kept iff the
 * masked leaf_err[0] <= tol; otherwise quantised iff every active value verifies, one width per channel from zz(q) of the active
 * values; otherwise raw; a selected leaf with A = 0 has code 0).
 *
 * Records.
 *   kept                                        none
 *   quantised, code b0 | b1 << 5 | b2 << 10     8 W (b0 + b1 + b2) bytes
 *   raw                                         8 ceil(3 A / 2) bytes
 * Quantised: channel 0's planes, then channel 1's, then channel 2's; plane k of channel c is W little-endian u64 words; bit L of
 * word j is bit k of zz(q) of the active voxel of rank 64 j + L in channel c; bits at ranks >= A are 0.  Raw: the active voxels'
 * three float32 values each, in rank order, bit for bit, then zero bytes up to a multiple of 8.
 * Every size is a multiple of 8; offsets is the exclusive sum and offsets[n] the payload's size; n * 6144 bytes always suffice.
 * Per leaf a compact record is never larger than the masked record, and with A = 512 it is the same bytes.  A leaf's code and
 * record depend on that leaf and its mask alone.
 *
 * The calls work in both precision modes (vqvdb_hip_vec3_precision.h); records belong to the x^ of the mode that made them.  The
 * rules of the Vec3 handle hold (status codes, vqhip_vec3_last_error, one call in flight per handle); a NULL handle returns -1,
 * n == 0 returns VQHIP_OK and touches nothing, null pointers are refused.
 */
#ifndef VQVDB_HIP_VEC3_ACTIVE_H
#define VQVDB_HIP_VEC3_ACTIVE_H

#include "vqvdb_hip_vec3_mask.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The table above on the host, no handle: the bytes of the record of `code` on a leaf with `active` active voxels.  -1 for a code
 * that is neither a sentinel nor three widths of 0..16, or for `active` outside 0..512. */
int64_t vqhip_vec3_active_record_bytes(int code, int active);

/* Device pointers; the argument list of the masked encode of vqvdb_hip_vec3_mask.h, leaf_err_dev is the masked error.  code_dev
 * [n], offsets_dev [n + 1] and the compact records at payload_dev + offsets_dev[leaf].  A record that would end beyond
 * payload_capacity is not written at all; bytes beyond offsets_dev[n] are untouched; nothing is read back or synchronised.
 * hip_stream NULL: the handle's stream. */
int vqhip_vec3_active_encode_device(vqhip_vec3_codec* codec, const float* leaves_dev, const float* recon_dev, const uint64_t* mask_dev,
                                    const float* leaf_err_dev, int64_t n, float tol, uint16_t* code_dev, int64_t* offsets_dev,
                                    uint8_t* payload_dev, int64_t payload_capacity, void* hip_stream);

/* In place on decoded leaves leaves_dev [n][512][3], with the masks, codes, offsets and payload of the encode above.  An active
 * value of a quantised leaf becomes x^ + (float)q * step, unfused, step = 1.875f * tol (a channel of width 0: x^ + 0 * step), of a
 * raw leaf the record's value; a kept leaf's stay.  background is a HOST pointer to 3 floats or NULL.  NULL: inactive voxels keep
 * their bits, whatever they are.  Otherwise every inactive voxel of every leaf, kept leaves included, receives those three values
 * bit for bit.  The device arrays are trusted. */
int vqhip_vec3_active_apply_device(vqhip_vec3_codec* codec, float* leaves_dev, const uint64_t* mask_dev, int64_t n, float tol,
                                   const uint16_t* code_dev, const int64_t* offsets_dev, const uint8_t* payload_dev, const float* background,
                                   void* hip_stream);

/* ADDS to bytes_dev[t] (int64 [n_tols], zeroed by the caller before the first call) the compact payload bytes of the n leaves at
 * tols[t]: offsets_dev[n] of the encode above at that rung.  64-bit integer sums: the same bits in every order and for every split
 * of the leaves over calls.  tols is a host pointer, n_tols 1..VQHIP_VEC3_RATE_MAX_TOLS. */
int vqhip_vec3_active_sweep_device(vqhip_vec3_codec* codec, const float* leaves_dev, const float* recon_dev, const uint64_t* mask_dev,
                                   const float* leaf_err_dev, int64_t n, const float* tols, int n_tols, int64_t* bytes_dev, void* hip_stream);

/* Host pointers.  Chunked and serial like the masked compress of vqvdb_hip_vec3_mask.h, in the handle's precision mode: per chunk
 * the round trip, the masked error, the compact encode.  leaf_err (may be NULL) receives the masked errors; payload has room for
 * n * 6144 bytes and *payload_bytes receives what was written. */
int vqhip_vec3_active_compress(vqhip_vec3_codec* codec, const float* leaves, const uint64_t* masks, int64_t n, float tol, uint16_t* indices,
                               float* leaf_err, uint16_t* leaf_code, uint8_t* payload, int64_t* payload_bytes);

/* Host pointers: leaves [n][512][3] = the decoded indices with the compact records applied (background as in the apply call; with
 * NULL an inactive voxel holds what the decoder gave).  Before any GPU work every code is checked and the record sizes of the codes
 * and the masks' popcounts must sum to payload_bytes: otherwise VQHIP_ERR_INVALID and leaves is untouched. */
int vqhip_vec3_active_decompress(vqhip_vec3_codec* codec, const uint16_t* indices, const uint64_t* masks, int64_t n, float tol,
                                 const uint16_t* leaf_code, const uint8_t* payload, int64_t payload_bytes, const float* background,
                                 float* leaves);

/* Host pointers: bytes [n_tols] is overwritten with the payload bytes of the compress above at every rung. */
int vqhip_vec3_active_sweep(vqhip_vec3_codec* codec, const float* leaves, const uint64_t* masks, int64_t n, const float* tols, int n_tols,
                            int64_t* bytes);

#ifdef __cplusplus
}
#endif

#endif
