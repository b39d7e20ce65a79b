// vq_bounded.h — kernel of the scalar handle's error-bounded round trip (include/vqvdb_hip_bounded.h): each
// leaf's reconstruction error from the caller's leaves and the decoded chunk.  The decoder's tail kernels are not touched:
// the error is a pass of its own behind decode_chunk.  The selection of the leaves over a tolerance reuses the three-launch
// stable compaction of vq_vec3_bounded.h (v3e::select_k / select_scan_k) on the same [n][2] error layout.
#pragma once

#include "vq_vec3_bounded.h"

namespace vqe {

constexpr int ERR_WAVES = 4;   // leaves (waves) per workgroup of leaf_err_k

// err[leaf] = {max |d|, sum d^2} over the leaf's 512 values, d = x - x^ in float32 (__fsub_rn).  One wave per leaf, ERR_WAVES
// leaves per workgroup, no LDS, no barrier: a wave never leaves its leaf, so a leaf's two numbers depend on that leaf only.
//
// Reduction order (fixed; tests/torch_ref_bounded.py restates it in numpy float32):
//   lane L (0..63) holds the voxels 4L .. 4L+3 (first 16-byte load) and 256+4L .. 256+4L+3 (second 16-byte load), v0 .. v7 in
//          that order:  q = d(v0)*d(v0);  q = q + d(vk)*d(vk) for k = 1 .. 7      (__fmul_rn / __fadd_rn, never fused)
//          a = nanmax(.. nanmax(|d(v0)|, |d(v1)|) .., |d(v7)|), where |d| of a non-finite d counts as NaN
//   wave:  xor butterfly over the 64 lanes, masks 32, 16, 8, 4, 2, 1:  q = q + q[lane ^ mask], a = nanmax(a, a[lane ^ mask])
//          (every lane ends with the same bits; lane 0 stores them)
// 13 chained additions per leaf (7 in the lane, 6 wave levels).  The maximum is exact and order-free for finite values and
// keeps NaN at every step (v3e::nanmax).
__global__ void __launch_bounds__(64 * ERR_WAVES) leaf_err_k(const float* __restrict__ orig, const float* __restrict__ recon,
                                                            float* __restrict__ err, int64_t n)
{
    const int lane = threadIdx.x & 63;
    const int64_t leaf = (int64_t)blockIdx.x * ERR_WAVES + (threadIdx.x >> 6);
    if (leaf >= n) return;   // whole waves leave: the shuffles below always see 64 live lanes
    const float4* x4 = reinterpret_cast<const float4*>(orig + leaf * 512);
    const float4* r4 = reinterpret_cast<const float4*>(recon + leaf * 512);
    const float4 xa = x4[lane], xb = x4[64 + lane], ra = r4[lane], rb = r4[64 + lane];
    const float x[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
    const float r[8] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w};
    float q = 0.0f, a = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float df = __fsub_rn(x[k], r[k]), ad = fabsf(df);
        const float sq = __fmul_rn(df, df);
        q = k == 0 ? sq : __fadd_rn(q, sq);
        const float av = ad <= 3.402823466e+38f ? ad : __builtin_nanf("");
        a = k == 0 ? av : v3e::nanmax(a, av);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        q = __fadd_rn(q, __shfl_xor(q, m));
        a = v3e::nanmax(a, __shfl_xor(a, m));
    }
    if (lane == 0) {
        err[leaf * 2] = a;
        err[leaf * 2 + 1] = q;
    }
}

}  // namespace vqe
