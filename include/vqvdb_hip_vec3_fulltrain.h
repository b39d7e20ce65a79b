/*
 * vqvdb_hip_vec3_fulltrain.h — full training of the Vec3 model VQVAE(3, 64, K) on a vqhip_vec3_codec handle:
 * forward, backward, AdamW and the EMA codebook update of the reference loop (python/training.py with the Vec3 notebook's
 * settings), in fp32.  Loss = 0.8 mse + 0.2 l1 + vq_loss, vq_loss = 0.25 mean((z - e)^2); the decoder reads the
 * straight-through value z + (e - z) against the codebook before the step's EMA update.
 *
 * Data parallel like the scalar stage 2 (vqvdb_hip.h, "Full training") and the Vec3 stage 1 (vqvdb_hip_vec3_train.h):
 *
 *     fwdbwd (per rank)  ->  host all-reduce (SUM) of the gradient vector and the aux buffer  ->  apply (identical on every rank)
 *
 * Means are taken over the global batch n_global, so the sum of the ranks' gradients is the global gradient.
 *
 * The rules of the Vec3 handle and of vqvdb_hip_vec3_train.h hold: status codes, vqhip_vec3_last_error, nothing throws or
 * aborts.  Every call below except the size queries fails with VQHIP_ERR_INVALID before vqhip_vec3_fulltrain_begin, and
 * so do n > vqhip_vec3_chunk_leaves(c), n_global < n and a NULL gradient buffer; nothing is launched then and the handle
 * stays usable.  n == 0 writes zeros.  stream NULL = the handle's own stream.  The training workspace (saved activations,
 * gradient buffers and weight-gradient partials, about 1.7 MB per leaf) is allocated at the first call, sized to that
 * call's n, and counted when the chunk is fitted to free memory once begin has run.
 *
 * The parameter vector holds the 60 tensors of model.parameters() in order (encoder first, then decoder), PyTorch layouts
 * ([OC][IC][k][k][k] for convs, [out][in] for Linear); the quantizer buffers are not in it.  Same inputs give the same
 * gradient bits on every call and stream.
 */
#ifndef VQVDB_HIP_VEC3_FULLTRAIN_H
#define VQVDB_HIP_VEC3_FULLTRAIN_H

#include "vqvdb_hip_vec3_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of the parameter vector: 5 124 067 (-1 for a NULL handle). */
int64_t vqhip_vec3_fulltrain_param_count(const vqhip_vec3_codec* c);

/* Index of the first decoder parameter in the vector: 2 235 712 (-1 for a NULL handle). */
int64_t vqhip_vec3_fulltrain_decoder_offset(const vqhip_vec3_codec* c);

/* Floats of the aux buffer: 66 K + 4 =
 *   [0, 66K+1)  the stage-1 statistics of the batch (vqhip_vec3_train_stats_floats's layout)
 *   [66K+1]     sum (recon - x)^2     [66K+2]  sum |recon - x|     [66K+3]  voxel values (1536 n)
 * Every entry is a sum (all-reduce SUM).  -1 for a NULL handle. */
int64_t vqhip_vec3_fulltrain_aux_floats(const vqhip_vec3_codec* c);

/* Start full training from the handle's current model: the parameter vector is read back from its tables, the AdamW
 * moments are zeroed, and the stage-1 EMA state is started (cluster_size = ones, embed_avg = embedding) unless
 * vqhip_vec3_train_begin has already run.  May be called again to restart the moments. */
int vqhip_vec3_fulltrain_begin(vqhip_vec3_codec* c);

/* One rank's forward and backward: grads_dev [param_count] receives the local sum of d(loss)/d(params) with the means over
 * n_global leaves; aux_dev [aux_floats] (required) the statistics and loss sums above.  latent_dev, if not NULL, receives
 * the flat latent [n*64][64] (row = leaf*64 + position; the input of the dead-code reset). */
int vqhip_vec3_fulltrain_fwdbwd_device(vqhip_vec3_codec* c, const float* leaves_dev, int64_t n, int64_t n_global, float* grads_dev,
                                       float* aux_dev, float* latent_dev, void* stream);

/* Test hook: the training-mode forward only.  Activations are kept for vqhip_vec3_debug_fetch under the layer names of the
 * inference handle when debug is on; indices_dev [n][64] and recon_dev [n][512][3] receive the code assignment and the
 * reconstruction unless NULL. */
int vqhip_vec3_fulltrain_forward_device(vqhip_vec3_codec* c, const float* leaves_dev, int64_t n, uint16_t* indices_dev, float* recon_dev,
                                        void* stream);

/* The optimizer step from (all-reduced) gradients and aux: torch.optim.AdamW on the whole vector (bias corrections of
 * `step`, counted from 1; weight decay on every parameter), then the stage-1 EMA update of the codebook from the aux
 * statistics (skipped when aux_dev is NULL), then every weight-derived device table is rebuilt from the new parameters.
 * vqhip_vec3_encode* / decode* run the trained model afterwards. */
int vqhip_vec3_fulltrain_apply_device(vqhip_vec3_codec* c, const float* grads_dev, const float* aux_dev, float lr, int64_t step, float beta1,
                                      float beta2, float adam_eps, float weight_decay, float ema_decay, float ema_eps, void* stream);

/* Host copies of the parameter vector / replacement (rebuilds the tables).  Wait for the device. */
int vqhip_vec3_fulltrain_get_params(vqhip_vec3_codec* c, float* params);
int vqhip_vec3_fulltrain_set_params(vqhip_vec3_codec* c, const float* params);

/* AdamW moments (exp_avg, exp_avg_sq; each param_count floats; NULL = skip) for checkpoints.  Wait for the device. */
int vqhip_vec3_fulltrain_get_opt_state(vqhip_vec3_codec* c, float* exp_avg, float* exp_avg_sq);
int vqhip_vec3_fulltrain_set_opt_state(vqhip_vec3_codec* c, const float* exp_avg, const float* exp_avg_sq);

#ifdef __cplusplus
}
#endif

#endif /* VQVDB_HIP_VEC3_FULLTRAIN_H */
