// vq_rate.h — the size sweep of the scalar handle's quantised residuals (include/vqvdb_hip_rate.h): the class
// histogram of a batch of leaves at up to 64 tolerances in one pass.  sweep_k classes every leaf at every rung exactly as
// vqr::resid_class_k (vq_residual.h) classes it at one tolerance, with that file's quantise and zigzag, and counts instead of
// storing: hist[t][k] grows by the number of leaves whose class at tols.t[t] is k.  The histogram fixes the payload and the
// .vqres v2 sidecar of a compress at that tolerance to the byte (vqhip_rate_payload_bytes / _sidecar_bytes).
//
// One wave per leaf, RATE_WAVES leaves per workgroup and step, a capped grid with a stride loop.  The wave reads the leaf's error;
// a leaf kept at every rung reads nothing else.  Otherwise each lane loads its eight voxels of x and x^ once and a wave-uniform loop
// over the rungs follows: a rung that keeps the leaf does no arithmetic, any other runs the eight quantise calls, the OR butterfly
// and the one ballot of resid_class_k.  Lane 0 counts into an LDS table [64][19] of int32 (ds_add_u32); at the end the workgroup
// adds its non-zero cells to the global histogram with 64-bit integer atomics.  Integer sums: the histogram is the same bits at
// every grid size, on every stream and for every split of the leaves over calls.  No float atomics, no scratch, no spills.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vq_residual.h"

namespace vqrate {

constexpr int RATE_WAVES = vqr::RES_WAVES;   // leaves (waves) per workgroup and step
constexpr int RATE_MAX_TOLS = 64;            // VQHIP_RATE_MAX_TOLS
constexpr int RATE_CLASSES = 19;             // VQHIP_RATE_CLASSES: columns 0 .. 16 quantised, 17 raw, 18 kept
constexpr int COL_RAW = 17, COL_KEPT = 18;
// workgroups at the most: four per CU of 256, i.e. four waves per SIMD of arithmetic-bound work; a workgroup's share of 2^32 leaves
// stays far below 2^31, the range of its LDS counters, and the flush costs at most RATE_MAX_GRID * count * 19 global atomics
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
    __syncthreads();
    for (int64_t leaf = (int64_t)blockIdx.x * RATE_WAVES + (threadIdx.x >> 6); leaf < n; leaf += (int64_t)gridDim.x * RATE_WAVES) {
        const float e = __int_as_float(vqr::uniform(__float_as_int(err[leaf * 2])));
        bool selected = false;   // at one rung at least
        for (int t = 0; t < count; ++t) selected = selected || !(e <= tols.t[t]);
        if (!selected) {         // kept at every rung: nothing else of the leaf is read
            if (lane < count) atomicAdd(&tab[lane * RATE_CLASSES + COL_KEPT], 1);
            continue;
        }
        const float* x = orig + leaf * 512;
        const float* r = recon + leaf * 512;
        float xv[8], rv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[j] = x[64 * j + lane], rv[j] = r[64 * j + lane];
        for (int t = 0; t < count; ++t) {
            const float tol = tols.t[t];
            if (e <= tol) {      // the selection rule of resid_class_k: equality keeps, NaN on either side selects
                if (lane == 0) atomicAdd(&tab[t * RATE_CLASSES + COL_KEPT], 1);
                continue;
            }
            const float step = __fmul_rn(1.875f, tol);
            bool ok = true;
            unsigned any = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int q;
                ok = vqr::quantise(xv[j], rv[j], step, tol, q) && ok;
                any |= vqr::zigzag(q);
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) any |= __shfl_xor(any, m);   // the bits of the maximum are the bits of the union
            const bool failed = __ballot(!ok) != 0ull;
            if (lane == 0) atomicAdd(&tab[t * RATE_CLASSES + (failed ? COL_RAW : 32 - __clz(any))], 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < count * RATE_CLASSES; i += 64 * RATE_WAVES) {
        const int v = tab[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

}  // namespace vqrate
