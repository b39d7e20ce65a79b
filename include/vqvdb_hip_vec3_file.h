/*
 * vqvdb_hip_vec3_file.h — the Vec3 handle on OpenVDB leaves and on disk: leaf-pointer encode / decode, and the
 * .vqv3 container with whole-file compress / decompress calls.  A Vec3f leaf buffer is [512][3] floats, the layout the handle
 * takes, so a caller passes leaf.buffer().data() as it is.
 *
 * Format .vqv3, version 1.  Little endian, no padding.
 *   File header, 24 B:
 *     char magic[6]="VQVEC3" | u8 version=1 | u8 numGrids (1..255) | u32 numCodes (K of the model)
 *     u8 kind (0 = indices only, 1 = masks + compact records of vqvdb_hip_vec3_active.h)
 *     u8 mode (kind 1: decoder mode the records belong to, 0 fp32 / 1 bf16; kind 0: 0)
 *     u16 zero | f32 tol (kind 1: the tolerance; kind 0: +0.0f) | u32 zero
 *   Per grid:
 *     u32 nameLength | char name[nameLength] | f32 transform[16] | u16 latentShape[3]={4,4,4}
 *     u32 totalBlocks (n) | u8 hasBackground | u8 zero[3] | f32 background[3] (+0.0f where absent)
 *     u64 payloadBytes (kind 0: 0)
 *     i32 origins[n][3] | u16 indices[n][64]
 *     kind 1 only: u64 masks[n][8] | u16 codes[n] | u8 payload[payloadBytes]
 * A grid is a set of whole sections, not per-leaf records: every section's size except the payload's is known from totalBlocks, so a
 * chunk goes to disk as a few positioned writes and the file's bytes do not depend on batch_leaves or on the handle's chunk size.
 * payloadBytes is patched when the grid ends.  Masks, codes and records are those of vqvdb_hip_vec3_active.h, bit for bit, in leaf
 * order; a leaf's record starts at the exclusive sum of the sizes before it.  vqvdb_amd/vqvdbfile.py (write_vec3 / read_vec3)
 * restates the layout in numpy.
 *
 * The header carries no hash of the model: the indices mean something, and the bound |x - out| <= tol holds, only with the weights
 * that wrote the file.  numCodes and, for kind 1, mode are checked against the handle; the weights are the caller's to keep.
 *
 * The rules of the Vec3 handle hold (status codes, vqhip_vec3_last_error, one call in flight per handle); a NULL handle returns -1,
 * n == 0 returns VQHIP_OK and touches nothing, null pointers are refused.  Gather and scatter between leaf buffers and pinned
 * staging run on the library's copy threads (VQHIP_COPY_THREADS, at most 16 by default).  Chunked and serial: file I/O, copies and
 * kernels do not overlap.
 */
#ifndef VQVDB_HIP_VEC3_FILE_H
#define VQVDB_HIP_VEC3_FILE_H

#include "vqvdb_hip_vec3_active.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQHIP_VEC3_FILE_VERSION 1
#define VQHIP_VEC3_FILE_HEADER_BYTES 24
#define VQHIP_VEC3_FILE_KIND_INDICES 0
#define VQHIP_VEC3_FILE_KIND_ACTIVE 1

/* Leaf-pointer entry points: leaf_ptrs[i] addresses the 1536 floats of leaf i.  The same bits as vqhip_vec3_encode / _decode on
 * the packed array, in the handle's mode.  Every index is checked against K before anything is launched. */
int vqhip_vec3_encode_leaves(vqhip_vec3_codec* codec, const float* const* leaf_ptrs, int64_t n, uint16_t* indices);
int vqhip_vec3_decode_leaves(vqhip_vec3_codec* codec, const uint16_t* indices, int64_t n, float* const* leaf_ptrs);

typedef struct vqhip_vec3_grid_source {
    const char* name;
    const float* transform;          /* 16 floats, NULL = identity                 */
    const float* const* leaf_ptrs;   /* n_leaves pointers to 1536 floats each      */
    const int32_t* origins;          /* [n_leaves][3]                              */
    int64_t n_leaves;                /* < 2^32 (file field is u32)                 */
    const uint64_t* masks;           /* [n_leaves][8]; kind 1: required; kind 0: ignored */
    const float* background;         /* 3 floats or NULL                           */
} vqhip_vec3_grid_source;

/* Kind 0: the file is the origins and the indices of vqhip_vec3_encode.  batch_leaves <= 0: the handle's chunk; larger values are
 * cut to it.  stats may be NULL.  On any failure after the output was opened the partial file is closed and removed. */
int vqhip_vec3_file_compress(vqhip_vec3_codec* codec, const char* path, const vqhip_vec3_grid_source* grids, int n_grids, int64_t batch_leaves,
                             vqhip_stream_stats* stats);

/* Kind 1: per chunk the sequence of vqhip_vec3_active_compress (round trip, masked error, compact encode) in the handle's mode; the
 * file holds that call's indices, codes and payload with the caller's masks, origins and backgrounds, mode = the handle's and tol as
 * given (any value, NaN included, as in vqhip_vec3_active_compress).  payload_bytes [n_grids] or NULL: every grid's payloadBytes. */
int vqhip_vec3_file_compress_active(vqhip_vec3_codec* codec, const char* path, const vqhip_vec3_grid_source* grids, int n_grids, float tol,
                                    int64_t batch_leaves, vqhip_stream_stats* stats, int64_t* payload_bytes);

typedef struct vqhip_vec3_grid_info {
    const char* name;          /* NUL-terminated, valid during the callback only */
    float transform[16];
    uint32_t num_codes;
    uint64_t total_blocks;
    int grid_index;
    int kind;
    int mode;
    float tol;
    int has_background;
    float background[3];
} vqhip_vec3_grid_info;
/* Called on the calling thread once per grid, before its leaves.  != 0 aborts. */
typedef int (*vqhip_vec3_grid_begin_fn)(void* user, const vqhip_vec3_grid_info* grid);
/* Called on the calling thread once per batch, in file order: store where each leaf's 1536 floats go.  masks [n][8] are the batch's
 * (NULL for kind 0).  The library fills the leaves before the next callback.  != 0 aborts. */
typedef int (*vqhip_vec3_leaf_alloc_fn)(void* user, int grid_index, const int32_t* origins, const uint64_t* masks, int64_t n, float** leaf_ptrs);

/* Either kind.  Kind 0: vqhip_vec3_decode into the leaf pointers.  Kind 1: the sequence of vqhip_vec3_active_decompress with the
 * file's tol, codes, masks and payload; inactive voxels receive the grid's background when it has one and keep the decoder's values
 * otherwise.  Refused with VQHIP_ERR_INVALID before any callback: a file whose length is not what its headers imply or whose
 * fields are not as stated above, numCodes != the handle's K, a kind-1 file whose mode is not the handle's (switch the handle with
 * the set call of vqvdb_hip_vec3_precision.h).  Refused before a grid's grid_begin and before any GPU work on it: an index >= K, an
 * illegal code, record sizes that do not sum to payloadBytes.  grid_begin may be NULL. */
int vqhip_vec3_file_decompress(vqhip_vec3_codec* codec, const char* path, int64_t batch_leaves, vqhip_vec3_grid_begin_fn grid_begin,
                               vqhip_vec3_leaf_alloc_fn leaf_alloc, void* user, vqhip_stream_stats* stats);

/* The header fields of a .vqv3 file after the whole-file length check; no handle, no GPU.  total_blocks and payload_bytes are sums
 * over the grids; any out pointer may be NULL.  A failure's message is at vqhip_vec3_last_error(NULL). */
int vqhip_vec3_file_info(const char* path, int* n_grids, uint32_t* num_codes, int* kind, int* mode, float* tol, int64_t* total_blocks,
                         int64_t* payload_bytes);

#ifdef __cplusplus
}
#endif

#endif
