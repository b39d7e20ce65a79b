/*
 * vqvdb_hip_vec3_budget.h — the Vec3 handle's compress into a byte budget on compact active-voxel records, in memory and into a
 * .vqv3 file.  vqvdb_hip_vec3_rate.h fits a payload budget without masks and in memory only; vqvdb_hip_vec3_active.h
 * sweeps the compact sizes but acts on none; vqvdb_hip_vec3_file.h writes a file at one tolerance, whatever its size turns out to
 * be.  These calls join the three: "make these leaves (these grids) fit in N bytes".  No call, kernel, record or file format of the
 * other headers changes; a file written here is a .vqv3 version 1 file of kind 1 and vqhip_vec3_file_decompress reads it.
 *
 * Two passes with a pick between them.  Pass 1 is the sequence of vqhip_vec3_active_sweep per chunk (round trip with a stored
 * reconstruction, masked error, the compact sizes at every rung) and also brings every chunk's indices and masked errors to the
 * host.  The pick takes the SMALLEST tols[t] by value that fits; the caller's rungs are the only candidates.  Pass 2 does not run
 * the encoder, and it works on the SELECTED leaves only: a leaf's code and record depend on that leaf and its mask alone, and a leaf
 * is selected exactly when !(leaf_err[0] <= tol) on the masked error that pass 1 brought to the host.  So per chunk pass 2 gathers
 * and uploads the selected leaves with their indices, masks and errors, decodes the indices, encodes the compact records in leaf
 * order, and writes VQHIP_VEC3_RES_KEPT for the others; a chunk without a selected leaf does no GPU work at all.  The payload's
 * total is checked against the sweep's bytes[best]; a difference is VQHIP_ERR_DEVICE.
 *
 * Precision mode: sizes, records and files belong to the mode (vqvdb_hip_vec3_precision.h) that made them.
 *
 * The rules of the Vec3 handle hold (status codes, vqhip_vec3_last_error, one call in flight per handle, nothing throws); a NULL
 * handle returns -1.  The five names share the prefix vqhip_vec3_budget_: the prefixes of the headers these calls build on are each
 * held to their own header's list by that header's test.
 */
#ifndef VQVDB_HIP_VEC3_BUDGET_H
#define VQVDB_HIP_VEC3_BUDGET_H

#include "vqvdb_hip_vec3_file.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pure host arithmetic, no handle, no device: the rules of the pick of vqvdb_hip_vec3_rate.h on the bytes [n_tols] that
 * vqhip_vec3_active_sweep returns.  The index of the smallest tols[t] by value with bytes[t] <= budget.  Sizes are not assumed to fall as the tolerance
 * grows; NaN rungs are never chosen; of duplicate rungs the first is returned.  -1 if none fits, or on a NULL pointer, n_tols
 * outside 1 .. VQHIP_VEC3_RATE_MAX_TOLS, budget < 0 or a negative bytes[t]. */
int vqhip_vec3_budget_pick(const int64_t* bytes, const float* tols, int n_tols, int64_t budget);

/* Pure host arithmetic: the size of the .vqv3 file that vqhip_vec3_file_compress (kind 0) or vqhip_vec3_file_compress_active
 * (kind 1) writes for these grids when grid g's payload has payload_bytes[g] bytes:
 *   24 + sum_g (102 + nameLength_g + n_g * (12 + 128 + (kind == 1 ? 64 + 2 : 0))) + sum_g payload_bytes[g],
 * 140 bytes per leaf for kind 0 and 206 for kind 1, a name counted to its NUL as the writer stores it.  Only the fields the size
 * depends on are read; the leaf, origin and mask pointers are checked for NULL as the writer checks them and never followed.
 * kind 0 has no payload: payload_bytes may be NULL and must hold zeros otherwise.  -1 on arguments the writer would refuse (no grid
 * list, n_grids outside 1 .. 255, a kind that is neither, a grid without a name, with more than 2^32 - 1 leaves or with leaves but no
 * leaf pointers, origins or, for kind 1, masks), on a negative payload, and on a total beyond 2^63 - 1. */
int64_t vqhip_vec3_budget_file_bytes(const vqhip_vec3_grid_source* grids, int n_grids, int kind, const int64_t* payload_bytes);

/* Compress into a payload budget, in memory.  leaves [n][512][3], masks [n][VQHIP_VEC3_MASK_WORDS], tols [n_tols] are host memory.
 * *tol_used receives the smallest tols[t] by value whose compact payload has at most payload_budget bytes; bytes [n_tols] (may be
 * NULL) receives what vqhip_vec3_active_sweep gives.  indices [n][64], leaf_err [n][VQHIP_VEC3_ERR_FLOATS] (NULL: a host buffer of
 * the call's own), leaf_code [n], payload (room for n * 6144 bytes) and *payload_bytes end as
 * vqhip_vec3_active_compress(c, leaves, masks, n, *tol_used, ...) leaves them, byte for byte.  The budget is the payload's alone.
 * If no rung fits, the call returns VQHIP_ERR_INVALID before pass 2 with *payload_bytes = 0; leaf_code, payload and *tol_used are
 * untouched, indices, leaf_err and bytes hold pass 1's values, and vqhip_vec3_last_error names the smallest size found and the
 * budget.  tol_used and payload_bytes may not be NULL; payload_budget < 0 is invalid.  n == 0 returns VQHIP_OK with
 * *payload_bytes = 0 and zeros in bytes; every rung then needs 0 bytes and *tol_used receives the smallest that is not NaN, if there
 * is one. */
int vqhip_vec3_budget_compress(vqhip_vec3_codec* c, const float* leaves, const uint64_t* masks, int64_t n, const float* tols, int n_tols,
                               int64_t payload_budget, float* tol_used, int64_t* bytes, uint16_t* indices, float* leaf_err, uint16_t* leaf_code,
                               uint8_t* payload, int64_t* payload_bytes);

/* Pass 1 alone over leaf pointers: bytes [n_grids][n_tols] receives, for every grid, what vqhip_vec3_active_sweep gives on its
 * leaves and masks, that is the payloadBytes of that grid in a file written at tols[t].  Nothing is written.  Grids and
 * batch_leaves as in vqhip_vec3_file_compress_active; masks are required. */
int vqhip_vec3_budget_file_sweep(vqhip_vec3_codec* c, const vqhip_vec3_grid_source* grids, int n_grids, const float* tols, int n_tols,
                                 int64_t batch_leaves, int64_t* bytes);

/* Compress into a FILE budget.  A .vqv3 file has one tolerance (the header has one tol field), so one rung is picked for all
 * grids: the smallest tols[t] by value with vqhip_vec3_budget_file_bytes(grids, n_grids, 1, payload of every grid at tols[t]) <=
 * file_budget.  The budget is the file's size, headers, origins, indices, masks and codes included.  Pass 1 runs over all grids
 * before anything is written and KEEPS THE INDICES AND THE MASKED ERRORS OF EVERY LEAF ON THE HOST, 136 bytes per leaf (128 + 8),
 * until the call returns.  If no rung fits, the call returns VQHIP_ERR_INVALID before the output is opened: a file that already
 * exists at `path` keeps its bytes, *tol_used and *file_bytes are untouched, and the message names the smallest file size found and
 * the budget.  Pass 2 writes the file; it equals that of vqhip_vec3_file_compress_active(c, path, grids, n_grids, *tol_used,
 * batch_leaves, ...) byte for byte, for every batch_leaves, and *file_bytes is its length.  payload_bytes [n_grids] may be NULL;
 * tol_used and file_bytes may not.  stats may be NULL: wall_s covers both passes, copy_s the gathers of both, read_s the writes.
 * Mask and pointer checks and the removal of a partial output on failure are those of vqhip_vec3_file_compress_active; a leaf
 * pointer that is NULL is found in pass 1, before the output is opened. */
int vqhip_vec3_budget_file_compress(vqhip_vec3_codec* c, const char* path, const vqhip_vec3_grid_source* grids, int n_grids, const float* tols,
                                    int n_tols, int64_t file_budget, int64_t batch_leaves, vqhip_stream_stats* stats, float* tol_used,
                                    int64_t* payload_bytes, int64_t* file_bytes);

#ifdef __cplusplus
}
#endif

#endif
