// vq_vec3_rate.h — the size sweep of the Vec3 handle's quantised residuals (include/vqvdb_hip_vec3_rate.h): the
// histogram of a batch of leaves over their record sizes at up to 64 tolerances in one pass.  sweep_k classes every leaf at every
// rung exactly as v3r::class_k (vq_vec3_residual.h) classes it at one tolerance, with vqr::quantise and vqr::zigzag of
// vq_residual.h, and counts instead of storing: hist[t][s] grows by the number of quantised leaves whose code at tols.t[t] has
// b0 + b1 + b2 = s planes (a record of 64 * s bytes), hist[t][49] by the raw leaves, hist[t][50] by the kept ones.  The row fixes
// the payload of a compress at that tolerance to the byte (vqhip_vec3_rate_payload_bytes).
//
// The shape is vqrate::sweep_k's (vq_rate.h): one wave per leaf, RATE_WAVES leaves per workgroup and step, a capped grid with a
// stride loop.  The wave reads the leaf's error; a leaf kept at every rung (its error is <= the smallest rung and no rung is NaN)
// reads nothing else.  Otherwise lane l loads its 24 values of x and of x^ once (voxels 64 j + l, j = 0 .. 7, three channels each:
// the layout of v3r::leaf_zigzag) and a wave-uniform loop over the rungs follows: a rung that keeps the leaf does no arithmetic,
// any other runs the 24 quantise calls, one OR butterfly per channel and the one ballot of class_k.  Inside a rung the channels
// go one after the other and a failed value is kept as a bit, not as a lane mask: with 24 masks alive beside the 64 rungs the
// scalar registers spilled.  Lane 0 counts into an LDS table [64][51] of int32; at the end the workgroup adds its non-zero cells to
// the global histogram with 64-bit integer atomics.  Integer sums: the histogram is the same bits at every grid size, on every
// stream and for every split of the leaves over calls.  No float atomics, no scratch, no spills.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vq_vec3_residual.h"

namespace v3rate {

constexpr int RATE_WAVES = v3r::RES_WAVES;   // leaves (waves) per workgroup and step
constexpr int RATE_MAX_TOLS = 64;            // VQHIP_VEC3_RATE_MAX_TOLS
constexpr int RATE_CLASSES = 51;             // VQHIP_VEC3_RATE_CLASSES: columns 0 .. 48 quantised by planes, 49 raw, 50 kept
constexpr int COL_RAW = 49, COL_KEPT = 50;
// workgroups at the most: four per CU of 256; a workgroup's share of 2^32 leaves stays far below 2^31, the range of its LDS
// counters, and the flush costs at most RATE_MAX_GRID * count * 51 global atomics
constexpr int RATE_MAX_GRID = 1024;

struct Tols {   // by value in the kernel's arguments: the rungs are read with scalar loads
    int count;
    float t[RATE_MAX_TOLS];
};

__global__ void __launch_bounds__(64 * RATE_WAVES) sweep_k(const float* __restrict__ orig, const float* __restrict__ recon, const float* __restrict__ err,
                                                          int64_t n, const Tols tols, unsigned long long* __restrict__ hist)
{
    __shared__ int tab[RATE_MAX_TOLS * RATE_CLASSES];
    const int lane = threadIdx.x & 63;
    const int count = tols.count;
    for (int i = threadIdx.x; i < count * RATE_CLASSES; i += 64 * RATE_WAVES) tab[i] = 0;
    // e <= every rung iff e <= the smallest and no rung is NaN: the rungs are walked once per workgroup, not once per leaf
    float least = tols.t[0];
    bool nan_rung = false;
#pragma unroll 1
    for (int t = 0; t < count; ++t) {
        const float tol = tols.t[t];
        nan_rung = nan_rung || tol != tol;
        least = tol < least ? tol : least;
    }
    __syncthreads();
    for (int64_t leaf = (int64_t)blockIdx.x * RATE_WAVES + (threadIdx.x >> 6); leaf < n; leaf += (int64_t)gridDim.x * RATE_WAVES) {
        const float e = __int_as_float(vqr::uniform(__float_as_int(err[leaf * 2])));
        if (!nan_rung && e <= least) {   // kept at every rung: nothing else of the leaf is read
            if (lane < count) atomicAdd(&tab[lane * RATE_CLASSES + COL_KEPT], 1);
            continue;
        }
        const float* x = orig + leaf * v3r::LEAF_FLOATS;
        const float* r = recon + leaf * v3r::LEAF_FLOATS;
        float xv[8][3], rv[8][3];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int at = 3 * (64 * j + lane);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) xv[j][ch] = x[at + ch], rv[j][ch] = r[at + ch];
        }
#pragma unroll 1
        for (int t = 0; t < count; ++t) {
            const float tol = tols.t[t];
            if (e <= tol) {      // the selection rule of class_k: equality keeps, NaN on either side selects
                if (lane == 0) atomicAdd(&tab[t * RATE_CLASSES + COL_KEPT], 1);
                continue;
            }
            const float step = __fmul_rn(1.875f, tol);
            unsigned bad = 0, any[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {   // one channel after the other: its union and whether one of its values failed
                unsigned u = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    int q;
                    bad |= vqr::quantise(xv[j][ch], rv[j][ch], step, tol, q) ? 0u : 1u;
                    u |= vqr::zigzag(q);
                }
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) u |= __shfl_xor(u, m);   // the bits of the maximum are the bits of the union
                any[ch] = u;
            }
            const bool failed = __ballot(bad) != 0ull;
            // |q| <= 32767 where nothing failed: 16 bits at the most per channel, 48 planes at the most
            if (lane == 0) atomicAdd(&tab[t * RATE_CLASSES + (failed ? COL_RAW : 96 - __clz(any[0]) - __clz(any[1]) - __clz(any[2]))], 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < count * RATE_CLASSES; i += 64 * RATE_WAVES) {
        const int v = tab[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

}  // namespace v3rate
