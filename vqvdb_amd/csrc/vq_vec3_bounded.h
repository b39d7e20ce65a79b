// vq_vec3_bounded.h — kernels of the Vec3 handle's error-bounded round trip (include/vqvdb_hip_vec3_bounded.h):
// the decoder tail that also measures each leaf's reconstruction error, and the stable selection of the leaves over a tolerance.
#pragma once

#include "vq_vec3.h"

namespace v3e {

// max that keeps a NaN of either side (fmaxf would drop it)
__device__ __forceinline__ float nanmax(float a, float b) { return (a != a || a > b) ? a : b; }

// final_k (vq_vec3.h) with the error of the leaf beside it: the same PixelShuffle staging, fmaf order, bias and tanh, so the
// voxel bits are final_k's.  Lane p (one output position, 512 lanes) also holds the leaf's original values x[p][0..2]
// (channels last, read before the convolution so that the loads are in flight under it) and forms d = x - x^ per value.
//
// Reduction order (fixed; tests/torch_ref_vec3_bounded.py restates it in numpy float32):
//   lane:  q = d0*d0;  q = q + d1*d1;  q = q + d2*d2          (__fmul_rn / __fadd_rn, channel order)
//          a = max(|d0|, |d1|, |d2|) where |d| of a non-finite d counts as NaN
//   wave:  xor butterfly over the 64 lanes, masks 32, 16, 8, 4, 2, 1:  q = q + q[lane ^ mask]  (every lane ends with the same bits)
//   leaf:  the 8 wave results through LDS, chained in wave order by lane 0:  ((((((w0 + w1) + w2) + w3) + w4) + w5) + w6) + w7
// max is exact and order-free for finite values and keeps NaN at every step.  err[leaf] = {max |d|, sum d^2}.
// The wave results reuse the first 16 floats of the staging area once every lane is done with it.  out may be NULL: then
// nothing of the reconstruction is stored.
__global__ void __launch_bounds__(512) final_err_k(const float* __restrict__ u, const float* __restrict__ w, const float* __restrict__ bias,
                                                   const float* __restrict__ orig, float* __restrict__ out, float* __restrict__ err, int64_t n)
{
    extern __shared__ float xs[];   // [32][512]
    const int64_t leaf = blockIdx.x;
    if (leaf >= n) return;
    const int tid = threadIdx.x;
    float x0[3];
#pragma unroll
    for (int co = 0; co < 3; ++co) x0[co] = orig[leaf * 1536 + tid * 3 + co];
    const float* ul = u + leaf * (256 * 64);
    for (int i = tid; i < 32 * 512; i += 512) {
        const int oc = i >> 9, p = i & 511, d = p >> 6, h = (p >> 3) & 7, wx = p & 7;
        const int uc = oc * 8 + (d & 1) * 4 + (h & 1) * 2 + (wx & 1);
        xs[i] = ul[uc * 64 + (d >> 1) * 16 + (h >> 1) * 4 + (wx >> 1)];
    }
    __syncthreads();
    const int d = tid >> 6, h = (tid >> 3) & 7, wx = tid & 7;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int ci = 0; ci < 32; ++ci) {
        const float* x = xs + ci * 512;
#pragma unroll
        for (int tap = 0; tap < 27; ++tap) {
            const int id = d + tap / 9 - 1, ih = h + (tap / 3) % 3 - 1, iw = wx + tap % 3 - 1;
            if (id < 0 || id > 7 || ih < 0 || ih > 7 || iw < 0 || iw > 7) continue;
            const float v = x[id * 64 + ih * 8 + iw];
#pragma unroll
            for (int co = 0; co < 3; ++co) acc[co] = __builtin_fmaf(w[(co * 32 + ci) * 27 + tap], v, acc[co]);
        }
    }
    float q = 0.0f, a = 0.0f;
#pragma unroll
    for (int co = 0; co < 3; ++co) {
        const float r = tanhf(acc[co] + bias[co]);
        if (out) out[leaf * 1536 + tid * 3 + co] = r;
        const float df = __fsub_rn(x0[co], r), ad = fabsf(df);
        const float sq = __fmul_rn(df, df);
        q = co == 0 ? sq : __fadd_rn(q, sq);
        const float av = ad <= 3.402823466e+38f ? ad : __builtin_nanf("");
        a = co == 0 ? av : nanmax(a, av);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        q = __fadd_rn(q, __shfl_xor(q, m));
        a = nanmax(a, __shfl_xor(a, m));
    }
    __syncthreads();   // every lane is done with the staged input: its first 16 floats now carry the wave results
    if ((tid & 63) == 0) {
        xs[tid >> 6] = q;
        xs[8 + (tid >> 6)] = a;
    }
    __syncthreads();
    if (tid == 0) {
        float qs = xs[0], as = xs[8];
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            qs = __fadd_rn(qs, xs[k]);
            as = nanmax(as, xs[8 + k]);
        }
        err[leaf * 2] = as;
        err[leaf * 2 + 1] = qs;
    }
}

// ---- selection: leaf i is an outlier iff !(err[i][0] <= tol) ----------------------------------------------------------
// Stable compaction over fixed blocks of SEL_BLOCK leaves, three launches: the count of every block, one exclusive scan of
// the counts (a single workgroup walks them in order with a running carry), then every block writes its ids at its offset,
// each lane at the rank of its leaf (ballot + popcount of the lower lanes + the counts of the lower waves).  Integer
// arithmetic only and no atomics: ids ascend, the output does not depend on timing.
constexpr int SEL_BLOCK = 1024;

// WRITE false: counts[block] = outliers of the block.  WRITE true: counts holds the exclusive offsets; ids are written.
template <bool WRITE>
__global__ void __launch_bounds__(SEL_BLOCK) select_k(const float* __restrict__ err, int64_t n, float tol, int64_t* __restrict__ counts,
                                                      int64_t* __restrict__ ids)
{
    __shared__ int wcount[SEL_BLOCK / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t i = (int64_t)blockIdx.x * SEL_BLOCK + tid;
    const bool sel = i < n && !(err[i * 2] <= tol);
    const unsigned long long ballot = __ballot(sel);
    if (lane == 0) wcount[wave] = __popcll(ballot);
    __syncthreads();
    if constexpr (!WRITE) {
        if (tid == 0) {
            int t = 0;
            for (int k = 0; k < SEL_BLOCK / 64; ++k) t += wcount[k];
            counts[blockIdx.x] = t;
        }
    } else {
        if (sel) {
            int rank = __popcll(ballot & ((1ull << lane) - 1ull));
            for (int k = 0; k < wave; ++k) rank += wcount[k];
            ids[counts[blockIdx.x] + rank] = i;
        }
    }
}

// counts[0..nb) -> exclusive prefix sums in place, *total = their sum.  One workgroup of 1024 lanes, 1024 counts per step.
__global__ void __launch_bounds__(1024) select_scan_k(int64_t* __restrict__ counts, int64_t nb, int64_t* __restrict__ total)
{
    __shared__ int64_t wsum[16];
    __shared__ int64_t carry_s;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < nb; base += 1024) {
        const int64_t i = base + tid;
        const int64_t v = i < nb ? counts[i] : 0;
        int64_t inc = v;   // inclusive scan inside the wave
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int64_t o = __shfl_up(inc, m);
            if (lane >= m) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int64_t before = carry_s;
        for (int k = 0; k < wave; ++k) before += wsum[k];
        if (i < nb) counts[i] = before + inc - v;
        __syncthreads();
        if (tid == 1023) carry_s = before + inc;
        __syncthreads();
    }
    if (tid == 0) *total = carry_s;
}

}  // namespace v3e
