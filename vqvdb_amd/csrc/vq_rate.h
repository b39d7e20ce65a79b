// vq_rate.h — the size sweep of the quantised residuals of both handles (include/vqvdb_hip_rate.h and
// include/vqvdb_hip_vec3_rate.h), templated on the channels C of a voxel as vq_residual.h is: the histogram
// of a batch of leaves over their record sizes at up to 64 tolerances in one pass.  sweep_k classes every leaf at every rung exactly
// as vqr::resid_class_k classes it at one tolerance, with that file's quantise and zigzag, and counts instead of storing:
// hist[t][s] grows by the number of quantised leaves whose code at tols.t[t] has b_0 + .. = s planes (a record of 64 * s bytes; with
// one channel s is the class), hist[t][16 C + 1] by the raw leaves, hist[t][16 C + 2] by the kept ones.  The row fixes the payload of
// a compress at that tolerance to the byte.
//
// One wave per leaf, RATE_WAVES leaves per workgroup and step, a capped grid with a stride loop.  The wave reads the leaf's error;
// a leaf kept at every rung (its error is <= the smallest rung and no rung is NaN) reads nothing else.  Otherwise lane l loads its
// 8 * C values of x and of x^ once (the layout of vqr::leaf_zigzag) and a wave-uniform loop over the rungs follows: a rung that
// keeps the leaf does no arithmetic, any other runs the 8 * C quantise calls, one OR butterfly per channel and the one ballot of
// resid_class_k.  Inside a rung the channels go one after the other and a failed value is kept as a bit, not as a lane mask: with
// 24 masks alive beside the 64 rungs the scalar registers spilled at C = 3.  Lane 0 counts into an LDS table [64][16 C + 3] of
// int32; at the end the workgroup adds its non-zero cells to the global histogram with 64-bit integer atomics.  Integer sums: the
// histogram is the same bits at every grid size, on every stream and for every split of the leaves over calls.  No float atomics,
// no scratch, no spills.
//
// MASKED (vq_mask.h, include/vqvdb_hip_vec3_mask.h; instantiated for C = 3): err is the masked error and mask [n][8] the leaves' value masks.  The
// wave's leaf index is uniform, so the eight words of a leaf arrive by scalar loads and lane l tests bit l of each.  The rung loop
// keeps no mask: the lane's values of an inactive voxel are loaded as x = x^ = +0, whatever the arrays hold there.  Such a pair
// gives q = 0 (nothing in the union) and verifies at every rung with a finite step > 0; it fails only where the step is 0, NaN or
// infinite or the rung negative, and there every active value fails as well (t is NaN or infinite, x^ + 0 * inf is NaN, or
// |x - x~| <= tol < 0 is false), so the leaf is raw by its active values alone.  That leaves the leaf without an active voxel, a
// wave-uniform case: where it is selected it counts in column 0.  The early exit uses the masked error.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vq_residual.h"

namespace vqrate {

constexpr int RATE_WAVES = vqr::RES_WAVES;   // leaves (waves) per workgroup and step
constexpr int RATE_MAX_TOLS = 64;            // VQHIP_RATE_MAX_TOLS, VQHIP_VEC3_RATE_MAX_TOLS
// columns 0 .. 16 C quantised by planes, then raw, then kept: VQHIP_RATE_CLASSES, VQHIP_VEC3_RATE_CLASSES
template <int C>
constexpr int CLASSES = 16 * C + 3;
template <int C>
constexpr int COL_RAW = 16 * C + 1;
template <int C>
constexpr int COL_KEPT = 16 * C + 2;
// workgroups at the most: four per CU of 256, i.e. four waves per SIMD of arithmetic-bound work; a workgroup's share of 2^32 leaves
// stays far below 2^31, the range of its LDS counters, and the flush costs at most RATE_MAX_GRID * count * CLASSES global atomics
constexpr int RATE_MAX_GRID = 1024;

struct Tols {   // by value in the kernel's arguments: the rungs are read with scalar loads
    int count;
    float t[RATE_MAX_TOLS];
};

template <int C, bool MASKED = false>
__global__ void __launch_bounds__(64 * RATE_WAVES) sweep_k(const float* __restrict__ orig, const float* __restrict__ recon, const float* __restrict__ err,
                                                          int64_t n, const Tols tols, unsigned long long* __restrict__ hist,
                                                          const unsigned long long* __restrict__ mask = nullptr)
{
    __shared__ int tab[RATE_MAX_TOLS * CLASSES<C>];
    const int lane = threadIdx.x & 63;
    const int count = tols.count;
    for (int i = threadIdx.x; i < count * CLASSES<C>; i += 64 * RATE_WAVES) tab[i] = 0;
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
    for (int64_t leaf = (int64_t)blockIdx.x * RATE_WAVES + vqr::wave_of_block<MASKED>(); leaf < n; leaf += (int64_t)gridDim.x * RATE_WAVES) {
        const float e = __int_as_float(vqr::uniform(__float_as_int(err[leaf * 2])));
        if (!nan_rung && e <= least) {   // kept at every rung: nothing else of the leaf is read
            if (lane < count) atomicAdd(&tab[lane * CLASSES<C> + COL_KEPT<C>], 1);
            continue;
        }
        const float* x = orig + leaf * (512 * C);
        const float* r = recon + leaf * (512 * C);
        float xv[8][C], rv[8][C];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int at = C * (64 * j + lane);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) xv[j][ch] = x[at + ch], rv[j][ch] = r[at + ch];
        }
        [[maybe_unused]] bool empty = false;   // MASKED: the leaf has no active voxel
        if constexpr (MASKED) {
            unsigned long long some = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned long long w = mask[leaf * 8 + j];
                some |= w;
                if (!((w >> lane) & 1ull)) {
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) xv[j][ch] = 0.0f, rv[j][ch] = 0.0f;
                }
            }
            empty = some == 0ull;
        }
#pragma unroll 1
        for (int t = 0; t < count; ++t) {
            const float tol = tols.t[t];
            if (e <= tol) {      // the selection rule of resid_class_k: equality keeps, NaN on either side selects
                if (lane == 0) atomicAdd(&tab[t * CLASSES<C> + COL_KEPT<C>], 1);
                continue;
            }
            if constexpr (MASKED) {
                if (empty) {     // selected without an active voxel: code 0, no record
                    if (lane == 0) atomicAdd(&tab[t * CLASSES<C>], 1);
                    continue;
                }
            }
            const float step = __fmul_rn(1.875f, tol);
            unsigned bad = 0, any[C];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {   // one channel after the other: its union and whether one of its values failed
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
            if (lane == 0) {
                int planes = 32 * C;   // |q| <= 32767 where nothing failed: 16 bits at the most per channel
#pragma unroll
                for (int ch = 0; ch < C; ++ch) planes -= __clz(any[ch]);
                atomicAdd(&tab[t * CLASSES<C> + (failed ? COL_RAW<C> : planes)], 1);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < count * CLASSES<C>; i += 64 * RATE_WAVES) {
        const int v = tab[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

}  // namespace vqrate
