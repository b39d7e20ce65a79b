/*
 * vqvdb_hip_vec3_residual.h — quantised, bit-packed residuals for the error-bounded compression of a vqhip_vec3_codec handle (the
 * Vec3 model).  vqvdb_hip_vec3_bounded.h keeps max |x - x~| <= tol by naming every leaf over the tolerance, which
 * the caller then stores raw (6144 bytes); these calls store x - x^ of such a leaf on a grid of 1.875 * tol instead, a few bits
 * per value with one bit width per channel, and keep a leaf raw only where that grid cannot hold it.  The calls of
 * vqvdb_hip_vec3_bounded.h are unchanged.  These calls work in memory; on disk: vqvdb_hip_vec3_file.h.
 *
 * A leaf is [512][3] float32, voxel-major and channels last, as everywhere on this handle.
 *
 * Arithmetic, all float32 and never fused (x the input leaf, x^ the decoded leaf, per value; vqvdb_hip_residual.h's, to the bit):
 *   step = 1.875f * tol      d = x - x^      t = d / step      q = rintf(t), ties to even      x~ = x^ + (float)q * step
 *   the value verifies iff |t| <= 32767 and |x - x~| <= tol; both comparisons are false on NaN.
 *
 * Codes, one uint16_t per leaf:
 *   VQHIP_VEC3_RES_KEPT  leaf_err[leaf][0] <= tol (the selection rule of vqvdb_hip_vec3_bounded.h, equality kept): no record, the
 *                        decoded leaf stands.
 *   b0 | b1 << 5 | b2 << 10
 *                        a selected leaf whose 1536 values all verify: b_c = the number of bits of max zz(q) over channel c's 512
 *                        values, zz(q) = (q << 1) ^ (q >> 31) on int32, each b_c in 0 .. 16; its record has 64 * (b0 + b1 + b2)
 *                        bytes.  Bit 15 is clear and every field is <= 16.  Code 0: every residual rounds to 0, a record of 0 bytes.
 *   VQHIP_VEC3_RES_RAW   any other selected leaf (a non-finite value, tol 0, negative or NaN, a step that is not finite, a residual
 *                        too wide for 16 bits in one channel, a value that the rounding of x^ + q * step pushed past tol): its
 *                        record is its 6144 bytes, bit for bit.
 * Nothing but the verification decides between quantised and raw: it is the guarantee.
 *
 * Record of a quantised leaf: channel 0's planes, then channel 1's, then channel 2's.  Inside channel c: bit planes
 * k = 0 .. b_c - 1, least significant first, each eight little-endian u64 words; bit L of word j of plane k, at byte
 * (8 (b_0 + .. + b_{c-1}) + 8 k + j) * 8 of the record, is bit k of zz(q) of voxel 64 j + L in channel c.
 *
 * Payload: the records of the leaves in leaf order, without gaps; offsets[i] is the byte at which leaf i's record starts (the
 * exclusive sum of the sizes), offsets[n] the payload's size.  Every size is a multiple of 64; n * 6144 bytes always suffice.
 *
 * Guarantee: max |x - residual_decompress(residual_compress(x, tol))| <= tol over every leaf with finite input, measured with the
 * float32 subtraction of vqvdb_hip_vec3_bounded.h; raw leaves return bit for bit, NaN payloads included.  A leaf's code and record
 * depend on that leaf alone: the same bits at every batch size, place in the batch, chunk size and stream.
 *
 * Precision mode: the records belong to the x^ of the mode (vqvdb_hip_vec3_precision.h) in which compress ran.
 * vqhip_vec3_residual_decompress must run in the same mode; the records do not say which it was, so no check is possible, and
 * records applied to the other mode's x^ are outside the guarantee.
 *
 * The rules of the Vec3 handle hold (status codes, vqhip_vec3_last_error, one call in flight per handle, nothing throws).
 *
 * Naming: all four calls begin with vqhip_vec3_residual_.  The host pair is not called vqhip_vec3_compress_residual /
 * _decompress_residual after the scalar handle's pair, because the names vqhip_vec3_compress* are pinned to
 * vqvdb_hip_vec3_bounded.h (tests/test_vec3_bounded_host.py holds the exported set to exactly that header's three).
 */
#ifndef VQVDB_HIP_VEC3_RESIDUAL_H
#define VQVDB_HIP_VEC3_RESIDUAL_H

#include "vqvdb_hip_vec3_bounded.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQHIP_VEC3_RES_KEPT 0xFFFE /* code of a leaf within the tolerance: no record              */
#define VQHIP_VEC3_RES_RAW 0xFFFF  /* code of a selected leaf stored as its 6144 bytes            */

/* Device pointers.  leaves_dev, recon_dev [n][512][3] and leaf_err_dev [n][VQHIP_VEC3_ERR_FLOATS] are what
 * vqhip_vec3_roundtrip_device takes and leaves behind (any x^ and error of the caller's will do: the codec's model is not run).
 * code_dev [n] uint16, offsets_dev [n + 1] int64, payload_dev 8-byte aligned with room for payload_capacity bytes.  After the
 * call's work on the stream offsets_dev[n] is the payload's size; the caller compares it with its capacity (n * 6144 always
 * suffices).  A record that would end beyond payload_capacity is not written at all, bytes beyond the total are not touched, and
 * nothing is read back to the host inside the call.  hip_stream NULL: the handle's stream.  n == 0 returns VQHIP_OK and touches
 * nothing. */
int vqhip_vec3_residual_encode_device(vqhip_vec3_codec* c, const float* leaves_dev, const float* recon_dev, const float* leaf_err_dev, int64_t n,
                                      float tol, uint16_t* code_dev, int64_t* offsets_dev, uint8_t* payload_dev, int64_t payload_capacity,
                                      void* hip_stream);

/* leaves_dev [n][512][3] holds decoded leaves and is corrected in place: quantised leaves become x^ + q * step, raw leaves their
 * record, kept leaves stay.  The call trusts its device arrays: codes that are neither a sentinel nor three fields <= 16, or
 * offsets that leave payload_dev, are not detected.  n == 0 returns VQHIP_OK and touches nothing. */
int vqhip_vec3_residual_apply_device(vqhip_vec3_codec* c, float* leaves_dev, int64_t n, float tol, const uint16_t* code_dev,
                                     const int64_t* offsets_dev, const uint8_t* payload_dev, void* hip_stream);

/* Host pointers in and out, chunked and serial like vqhip_vec3_compress_bounded, in the handle's precision mode.  indices [n][64];
 * leaf_err [n][VQHIP_VEC3_ERR_FLOATS] may be NULL; leaf_code [n]; payload has room for n * 6144 bytes and receives the records in
 * leaf order over the whole call, *payload_bytes their size.  n == 0 returns VQHIP_OK with *payload_bytes = 0. */
int vqhip_vec3_residual_compress(vqhip_vec3_codec* c, const float* leaves, int64_t n, float tol, uint16_t* indices, float* leaf_err,
                                 uint16_t* leaf_code, uint8_t* payload, int64_t* payload_bytes);

/* Decodes (in the handle's precision mode: the one compress ran in) and applies the records.  Before any GPU work: every code is
 * VQHIP_VEC3_RES_KEPT, VQHIP_VEC3_RES_RAW or has bit 15 clear and three fields <= 16, and the record sizes sum to payload_bytes,
 * else VQHIP_ERR_INVALID with `leaves` untouched.  n == 0 returns VQHIP_OK and touches nothing. */
int vqhip_vec3_residual_decompress(vqhip_vec3_codec* c, const uint16_t* indices, int64_t n, float tol, const uint16_t* leaf_code,
                                   const uint8_t* payload, int64_t payload_bytes, float* leaves);

#ifdef __cplusplus
}
#endif

#endif
