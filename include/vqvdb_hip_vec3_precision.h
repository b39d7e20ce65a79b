/*
 * vqvdb_hip_vec3_precision.h — precision mode of the Vec3 model's inference on a vqhip_vec3_codec handle.
 *
 * The default, VQHIP_VEC3_PRECISION_FP32, is the path of vqvdb_hip.h unchanged, bit for bit.  VQHIP_VEC3_PRECISION_BF16
 * rounds both operands of every convolution product to bf16 (round to nearest even): the weights once, when their
 * fragments are packed, the activations after the fused input transform (leaf read, GroupNorm + ReLU, attention gate) has
 * been evaluated in fp32.  Products are accumulated in fp32; bias, residual adds, GroupNorm statistics, attention gates, the
 * codebook search (fp32 codebook, first minimum), the code gather and the final conv + tanh stay fp32, and so does every
 * tensor in device memory.  A leaf's result depends only on that leaf, as in fp32 mode.
 *
 * vqhip_vec3_encode, _decode, _encode_device, _decode_device and vqhip_vec3_debug_fetch follow the mode.  Training
 * (vqhip_vec3_train_*, vqhip_vec3_fulltrain_*) always runs in fp32; after a training update the bf16 weight fragments are
 * rebuilt on the device together with the fp32 tables.  The rules of the Vec3 handle hold (status codes,
 * vqhip_vec3_last_error, one call in flight per handle).
 */
#ifndef VQVDB_HIP_VEC3_PRECISION_H
#define VQVDB_HIP_VEC3_PRECISION_H

#include "vqvdb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQHIP_VEC3_PRECISION_FP32 0
#define VQHIP_VEC3_PRECISION_BF16 1

/* Switch the mode between calls.  Synchronises the handle's stream.  The bf16 weight fragments (10.2 MB of device memory)
 * are built at the first switch to bf16, so a handle that never asks pays nothing.  Any other mode value returns
 * VQHIP_ERR_INVALID with a message and leaves the mode unchanged. */
int vqhip_vec3_set_precision(vqhip_vec3_codec* c, int mode);

/* The current mode.  VQHIP_ERR_INVALID for a NULL handle or a NULL mode. */
int vqhip_vec3_get_precision(const vqhip_vec3_codec* c, int* mode);

#ifdef __cplusplus
}
#endif

#endif
