/*
 * vqvdb_hip_encode_mode.h — operand mode of the scalar codec's encode on a vqhip_codec handle.
 *
 * The default, VQHIP_PRECISION_FP32, is the path of vqvdb_hip.h unchanged, bit for bit.  VQHIP_PRECISION_BF16 rounds both
 * operands of every product of the encoder's two 16-channel convolutions (encoder.pre.3.conv1 and .conv2, 54 % of the encoder's
 * time) to bf16, round to nearest even: the weights once, when their fragments are packed, the activations after GroupNorm + ReLU
 * has been evaluated in fp32.  Products are accumulated in fp32; bias, the residual add, GroupNorm statistics, the first layer,
 * the down conv, the 32-channel convs, the gate and the code search stay fp32, and so does every tensor in device memory.  A leaf's
 * result depends only on that leaf: the same bits for any batch size, place in the batch, chunk size, stream and entry point.
 * An encode in bf16 mode can choose other codes than an fp32 encode does; every index row is a valid .vqvdb payload, and the
 * reconstruction error of the two modes is compared in DESIGN.md §24.  This mode and the decode mode of vqvdb_hip_precision.h are
 * independent: neither touches the other.
 *
 * Calls that follow the mode: the plain encode, its device-pointer form, its leaf-pointer form, the plain compress to a file,
 * and the debug fetch of encoder tensors after such a call.
 *
 * Calls that ignore it and always run the fp32 encoder: the device round trip, every error-bounded, residual and size-sweep call
 * and their file forms (a compress that writes a sidecar included), both training families and the multi-GPU calls.  After a
 * training update the next bf16 encode packs its weight fragments again from the live parameters: they equal those of a fresh
 * handle built from the exported pack.
 *
 * The C++ adapter vqvdb_hip_backend.hpp (HipBackend) has no switch: it encodes in fp32.
 *
 * The rules of vqvdb_hip.h hold (status codes, the last-error text, one call in flight per handle).
 */
#ifndef VQVDB_HIP_ENCODE_MODE_H
#define VQVDB_HIP_ENCODE_MODE_H

#include "vqvdb_hip_precision.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Switch the mode between calls; mode is VQHIP_PRECISION_FP32 or VQHIP_PRECISION_BF16.  Synchronises the handle's stream.  The
 * bf16 weight fragments (28 KB of device memory) are built at the first switch to bf16, so a handle that never asks pays
 * nothing; if they cannot be allocated the call returns VQHIP_ERR_NOMEM, the mode is unchanged and the handle stays usable.  Any
 * other mode value returns VQHIP_ERR_INVALID with a message and leaves the mode unchanged. */
int vqhip_set_encode_mode(vqhip_codec* c, int mode);

/* The current mode.  VQHIP_ERR_INVALID for a NULL handle or a NULL mode. */
int vqhip_get_encode_mode(const vqhip_codec* c, int* mode);

#ifdef __cplusplus
}
#endif

#endif
