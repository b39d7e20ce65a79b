/*
 * vqvdb_hip_vec3_train.h — codebook (EMA) training of the Vec3 model VQVAE(3, 64, K) on a vqhip_vec3_codec handle
 * (DESIGN.md §12).  The training-mode forward of the reference's VectorQuantizerEMA (python/VQVAE_v2.py:107-156) on the
 * Vec3 encoder's latent, its eval forward (VQVAE.forward in eval mode, :344-348; python/training.py:183-199), and the
 * buffers check_and_reset_dead_codes (:382-417) works on.  Encoder and decoder weights stay frozen.
 *
 * Data parallel like the scalar stage 1 (vqvdb_hip.h, "Codebook training"): every rank computes the statistics of its own
 * batch, the host all-reduces them (SUM), and every rank applies the identical update, so the codebooks stay replicated.
 *
 * The rules of the Vec3 handle hold (vqvdb_hip.h): status codes, vqhip_vec3_last_error, nothing throws or aborts, one
 * call in flight per handle.  In addition:
 *   - every call below except the stats-size query fails with VQHIP_ERR_INVALID before vqhip_vec3_train_begin, and so do a
 *     NULL stats buffer, a decay outside [0, 1] and eps <= 0; nothing is launched then and the handle stays usable;
 *   - device entry points take n <= vqhip_vec3_chunk_leaves(c) leaves ([n][512][3] float32 channels last, device memory);
 *     n == 0 writes zero statistics (and zero reconstruction sums) and returns VQHIP_OK;
 *   - stream NULL = the handle's own stream; results are ordered on the stream given, as for vqhip_vec3_encode_device.
 */
#ifndef VQVDB_HIP_VEC3_TRAIN_H
#define VQVDB_HIP_VEC3_TRAIN_H

#include "vqvdb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of the statistics buffer: 66*K + 1, laid out as
 *   [0,K)      encodings_sum (:134)                         rows per code
 *   [K,65K)    dw[K][64] = encodings^T flat (:137)          each code's rows summed in ascending row order
 *   [65K,66K)  sum over the code's rows of |z - e|^2        e = the codebook before the update (commitment loss, :146)
 *   [66K]      rows (= 64 n)
 * Every entry is a sum, so per-rank buffers are combined by an all-reduce (SUM).  The same bits on every call.
 * Returns -1 for a NULL handle. */
int64_t vqhip_vec3_train_stats_floats(const vqhip_vec3_codec* c);

/* Start training: cluster_size [K] (NULL = ones, :104) and embed_avg [K][64] (NULL = the current embedding, :105), host
 * memory.  The codebook itself is the handle's (from the pack, or as trained so far).  Encode results do not change.  The
 * training workspace (flat latent, sorted row lists, partial sums: about 17 KB per leaf) is counted from now on when the
 * chunk is fitted to free memory.  May be called again to restart the EMA buffers. */
int vqhip_vec3_train_begin(vqhip_vec3_codec* c, const float* cluster_size, const float* embed_avg);

/* Training-mode statistics of one batch: encoder -> latent -> nearest code against the live codebook (the expanded
 * distance of :117-124, first minimum) -> stats_dev [66K+1].  Optionally the indices [n][64] (uint16) and the flat latent
 * [n*64][64] (row = leaf*64 + position, the reference's `flat`, :111-114; the input of the dead-code reset). */
int vqhip_vec3_train_vq_stats_device(vqhip_vec3_codec* c, const float* leaves_dev, int64_t n, float* stats_dev, uint16_t* indices_dev,
                                     float* latent_dev, void* stream);

/* Eval forward: the statistics as above (nothing is updated), then the decoder on the straight-through value z + (e - z)
 * (:149), then recon_sums_dev[3] = {sum (recon-x)^2, sum |recon-x|, voxel values (= 1536 n)} (F.mse_loss / F.l1_loss of
 * training.py:183-199 before the division).  recon_dev [n][512][3] receives the reconstruction unless NULL. */
int vqhip_vec3_train_eval_device(vqhip_vec3_codec* c, const float* leaves_dev, int64_t n, float* stats_dev, float* recon_sums_dev,
                                 float* recon_dev, void* stream);

/* EMA update from (all-reduced) statistics (:135-144):
 *   cluster_size = decay cluster_size + (1-decay) encodings_sum;  embed_avg likewise with dw;
 *   embedding = embed_avg / clamp(cluster_size, min = eps)
 * then the search tables of the live codebook are rebuilt on the device, bit-identical to what vqhip_vec3_create builds
 * for a pack holding this embedding.  encode / decode and the next statistics see the new codebook; no commit call. */
int vqhip_vec3_train_vq_update_device(vqhip_vec3_codec* c, const float* stats_dev, float decay, float eps, void* stream);

/* Host copies of embedding [K][64], cluster_size [K], embed_avg [K][64]; any may be NULL.  Waits for the device. */
int vqhip_vec3_train_get_state(vqhip_vec3_codec* c, float* embedding, float* cluster_size, float* embed_avg);

/* Replace any of the three buffers (NULL = keep); a new embedding rebuilds the search tables (checkpoint resume, dead-code
 * reset).  Waits for the device. */
int vqhip_vec3_train_set_state(vqhip_vec3_codec* c, const float* embedding, const float* cluster_size, const float* embed_avg);

#ifdef __cplusplus
}
#endif

#endif /* VQVDB_HIP_VEC3_TRAIN_H */
