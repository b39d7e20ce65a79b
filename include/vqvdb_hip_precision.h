/*
 * vqvdb_hip_precision.h — precision mode of the scalar codec's decode on a vqhip_codec handle.
 *
 * The default, VQHIP_PRECISION_FP32, is the path of vqvdb_hip.h unchanged, bit for bit.  VQHIP_PRECISION_BF16 rounds both
 * operands of every product of the decoder's two 64-channel convolutions (decoder.res_stack.0.conv1 and .conv2, 80 % of the
 * decoder's time) to bf16, round to nearest even: the weights once, when their fragments are packed, the activations after
 * GroupNorm + ReLU has been evaluated in fp32.  Products are accumulated in fp32; bias, the residual add, GroupNorm statistics,
 * the attention gate, the decoder stem and the folded tail stay fp32, and so does every tensor in device memory.  A leaf's
 * result depends only on that leaf: the same bits for any batch size, place in the batch, chunk size, stream and entry point.
 * The input of a decode is indices, so no code can change, and .vqvdb files are the same bytes in either mode.
 *
 * Calls that follow the mode: vqhip_decode, vqhip_decode_device, vqhip_decode_leaves, vqhip_decompress_file, and
 * vqhip_debug_fetch of decoder tensors after such a call.
 *
 * Calls that ignore it and always run the fp32 decoder: every call that states or checks an error bound against the fp32
 * reconstruction and stores no mode in its records (vqhip_roundtrip_device, the *_bounded and *_residual* calls, the size sweep
 * of vqvdb_hip_rate.h, and their file forms), both training families (vqhip_train_*, vqhip_fulltrain_*) and vqhip_multi_*.  Encoding has a
 * mode of its own, independent of this one: vqvdb_hip_encode_mode.h.  After a training update (vqhip_train_commit, vqhip_fulltrain_apply_device, _set_params, _set_state) the next
 * bf16 decode packs its weight fragments again from the live parameters: they equal those of a fresh handle built from the
 * exported pack.
 *
 * The C++ adapter vqvdb_hip_backend.hpp (HipBackend) has no switch: it decodes in fp32.
 *
 * The rules of vqvdb_hip.h hold (status codes, vqhip_last_error, one call in flight per handle).
 */
#ifndef VQVDB_HIP_PRECISION_H
#define VQVDB_HIP_PRECISION_H

#include "vqvdb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQHIP_PRECISION_FP32 0
#define VQHIP_PRECISION_BF16 1

/* (The two calls say "mode", not "precision": the library's exported names that contain "precision" are the Vec3 pair of
 * vqvdb_hip_vec3_precision.h and nothing else, which tests/test_masked_host.py holds.)
 *
 * Switch the mode between calls.  Synchronises the handle's stream.  The bf16 weight fragments (0.44 MB of device memory) are
 * built at the first switch to bf16, so a handle that never asks pays nothing; if they cannot be allocated the call returns
 * VQHIP_ERR_NOMEM, the mode is unchanged and the handle stays usable.  Any other mode value returns VQHIP_ERR_INVALID with a
 * message and leaves the mode unchanged. */
int vqhip_set_decode_mode(vqhip_codec* c, int mode);

/* The current mode.  VQHIP_ERR_INVALID for a NULL handle or a NULL mode. */
int vqhip_get_decode_mode(const vqhip_codec* c, int* mode);

#ifdef __cplusplus
}
#endif

#endif
