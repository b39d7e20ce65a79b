/*
 * vqvdb_hip_vec3_mask.h — active-voxel masks for the quantised residuals of a vqhip_vec3_codec handle (the
 * scalar handle has no masked calls).  Only the encode side knows a
 * mask: a masked encode produces ordinary codes and records, and vqhip_vec3_residual_apply_device and
 * vqhip_vec3_residual_decompress read them unchanged.  These calls work in memory; on disk: vqvdb_hip_vec3_file.h.
 *
 * Mask.  uint64 [n][8], little endian.  Bit L of word j of a leaf is voxel 64 j + L (the words of OpenVDB's NodeMask<3>,
 * leaf.valueMask(), unconverted); one bit covers the three channels of its voxel.  Device masks are 8-byte aligned.
 *
 * Inactive values take no part in anything: they add +0.0f to both error numbers, have q = 0 and verify without any arithmetic
 * on them, whatever x and x^ hold there, NaN and inf included.
 *
 * Masked leaf error.  {max |d|, sum d^2} over the active values, d = x - x^ in float32, unfused, in the reduction order of
 * vqhip_vec3_roundtrip_device's error with the sq and |d| of an inactive value replaced by +0.0f.  An all-ones mask gives the
 * bits of the unmasked error, an all-zero mask {+0, +0}, a non-finite active d gives NaN as before.
 *
 * Selection, code, record.  The rules of vqvdb_hip_vec3_residual.h on the masked error and the active values: kept iff
 * leaf_err[0] <= tol; otherwise quantised iff every active value verifies, with one width per channel from zz(q) of the active
 * values; otherwise raw.  A quantised record has the existing layout and an inactive voxel's bits are 0; a raw record is the
 * leaf's 6144 bytes as given.  A selected leaf without active voxels has code 0 and an empty record.
 *
 * Substitution.  For finite x^ every masked result equals the unmasked result on x' = where(active, x, x^), bit for bit; raw
 * records hold x, not x'; and a selected leaf without active voxels has code 0 also at a tolerance (NaN, below zero) at which x'
 * would be raw.  Per leaf the record with a mask is never larger than without, and a kept leaf stays kept.
 *
 * The calls work in both precision modes (vqvdb_hip_vec3_precision.h); masked errors and records belong to the x^ of the mode
 * that made them.  The rules of the Vec3 handle hold (status codes, vqhip_vec3_last_error, one call in flight per handle); a
 * NULL handle returns -1, n == 0 returns VQHIP_OK and touches nothing, null pointers are refused.
 */
#ifndef VQVDB_HIP_VEC3_MASK_H
#define VQVDB_HIP_VEC3_MASK_H

#include "vqvdb_hip_vec3_rate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQHIP_VEC3_MASK_WORDS 8 /* uint64 words of one leaf's mask */

/* Device pointers.  leaves_dev, recon_dev [n][512][3], mask_dev [n][VQHIP_VEC3_MASK_WORDS] -> leaf_err_dev
 * [n][VQHIP_VEC3_ERR_FLOATS], the masked leaf error.  The model is not run; nothing is read back or synchronised.  n is at most
 * 2^31 - 1.  hip_stream NULL: the handle's stream. */
int vqhip_vec3_mask_leaf_err_device(vqhip_vec3_codec* codec, const float* leaves_dev, const float* recon_dev, const uint64_t* mask_dev,
                                    int64_t n, float* leaf_err_dev, void* hip_stream);

/* vqhip_vec3_residual_encode_device with masks: leaf_err_dev is the masked error. */
int vqhip_vec3_mask_residual_encode_device(vqhip_vec3_codec* codec, const float* leaves_dev, const float* recon_dev, const uint64_t* mask_dev,
                                           const float* leaf_err_dev, int64_t n, float tol, uint16_t* code_dev, int64_t* offsets_dev,
                                           uint8_t* payload_dev, int64_t payload_capacity, void* hip_stream);

/* The sweep-device call of vqvdb_hip_vec3_rate.h with masks: ADDS the histogram of the n leaves at every rung to hist_dev
 * [n_tols][VQHIP_VEC3_RATE_CLASSES]; row t counts the codes of vqhip_vec3_mask_residual_encode_device at tols[t]. */
int vqhip_vec3_mask_sweep_device(vqhip_vec3_codec* codec, const float* leaves_dev, const float* recon_dev, const uint64_t* mask_dev,
                                 const float* leaf_err_dev, int64_t n, const float* tols, int n_tols, int64_t* hist_dev, void* hip_stream);

/* Host pointers.  Chunked and serial like vqhip_vec3_residual_compress: per chunk the round trip, the masked error, the masked
 * encode.  leaf_err (may be NULL) receives the masked errors.  The output decompresses with vqhip_vec3_residual_decompress. */
int vqhip_vec3_mask_compress_residual(vqhip_vec3_codec* codec, const float* leaves, const uint64_t* masks, int64_t n, float tol,
                                      uint16_t* indices, float* leaf_err, uint16_t* leaf_code, uint8_t* payload, int64_t* payload_bytes);

/* Host pointers: the sweep of vqvdb_hip_vec3_rate.h with masks; hist [n_tols][VQHIP_VEC3_RATE_CLASSES] is overwritten. */
int vqhip_vec3_mask_sweep(vqhip_vec3_codec* codec, const float* leaves, const uint64_t* masks, int64_t n, const float* tols, int n_tols,
                          int64_t* hist);

#ifdef __cplusplus
}
#endif

#endif
