// vq_mask.h — kernel of the Vec3 handle's active-voxel masks (include/vqvdb_hip_vec3_mask.h): each leaf's
// reconstruction error over its ACTIVE values.  The masked class, pack and sweep are the MASKED instantiations of vq_residual.h and
// vq_rate.h; nothing of the decode side knows a mask.
//
// Mask: uint64 [n][8], bit L of word j of a leaf = voxel 64 j + L (the words of OpenVDB's NodeMask<3>); one bit covers the three
// channels of its voxel.
//
// err[leaf] = {max |d|, sum d^2} over the active values, d = x - x^ in float32 (__fsub_rn), in the reduction order of
// v3e::final_err_k (vq_vec3_bounded.h) with the sq and |d| of an inactive value replaced by +0.0f before they enter it, as a pass of
// its own over (x, x^, mask).  One workgroup of 512 lanes per leaf; lane p holds voxel p, chains its three channels, each wave runs
// the xor butterfly 32 .. 1 and lane 0 chains the eight wave results in wave order through 16 floats of LDS.  Wave w holds the voxels
// 64 w + lane: its mask word w is uniform (the leaf is the workgroup's, the wave index a scalar), arrives by a scalar load, and a
// lane tests bit `lane`.
// An all-ones mask gives the bits of the unmasked error, an all-zero mask {+0, +0}; a non-finite active d gives NaN as before;
// whatever x and x^ hold at an inactive voxel, NaN and inf included, does not reach the result.  No atomics; lane 0 writes the two
// floats with ordinary stores.
#pragma once

#include "vq_residual.h"
#include "vq_vec3_bounded.h"

namespace vqm {

// one value's terms of the chain: its square and its |d| (NaN where d is not finite), +0 for an inactive voxel
__device__ __forceinline__ void terms(float x, float r, bool active, float& sq, float& av)
{
    const float df = __fsub_rn(x, r), ad = fabsf(df);
    sq = active ? __fmul_rn(df, df) : 0.0f;
    av = active ? (ad <= 3.402823466e+38f ? ad : __builtin_nanf("")) : 0.0f;
}

__global__ void __launch_bounds__(512) leaf_err_masked_k(const float* __restrict__ orig, const float* __restrict__ recon,
                                                         const unsigned long long* __restrict__ mask, float* __restrict__ err, int64_t n)
{
    __shared__ float ws[16];   // the eight wave sums, then the eight wave maxima
    const int lane = threadIdx.x & 63;
    const int64_t leaf = blockIdx.x;
    if (leaf >= n) return;
    const int wave = vqr::uniform((int)(threadIdx.x >> 6));
    const bool active = (mask[leaf * 8 + wave] >> lane) & 1ull;
    const int64_t at = leaf * 1536 + (64 * wave + lane) * 3;
    float q = 0.0f, a = 0.0f;
#pragma unroll
    for (int co = 0; co < 3; ++co) {
        float sq, av;
        terms(orig[at + co], recon[at + co], active, sq, av);
        q = co == 0 ? sq : __fadd_rn(q, sq);
        a = co == 0 ? av : v3e::nanmax(a, av);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        q = __fadd_rn(q, __shfl_xor(q, m));
        a = v3e::nanmax(a, __shfl_xor(a, m));
    }
    if (lane == 0) {
        ws[wave] = q;
        ws[8 + wave] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float qs = ws[0], as = ws[8];
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            qs = __fadd_rn(qs, ws[k]);
            as = v3e::nanmax(as, ws[8 + k]);
        }
        err[leaf * 2] = as;
        err[leaf * 2 + 1] = qs;
    }
}

}  // namespace vqm
