// vq_residual.h — kernels of the scalar handle's quantised residuals (include/vqvdb_hip_residual.h): a leaf over
// the tolerance is stored as x - x^ on a grid of 1.875 * tol, bit-packed in planes, instead of raw; a leaf that the grid cannot
// hold within the tolerance stays raw.  resid_class_k decides, resid_scan_k places, resid_pack_k writes, resid_apply_k undoes.
//
// Arithmetic (pinned by the format; tests/torch_ref_residual.py restates it in numpy float32, to the bit).  Float32, never fused:
//   step = 1.875f * tol        d = x - x^        t = d / step        q = rintf(t)  (ties to even)        x~ = x^ + (float)q * step
//   the voxel verifies iff |t| <= 32767 and |x - x~| <= tol            (both false on NaN)
// A leaf with leaf_err[leaf][0] <= tol is kept (class 254, no record).  A selected leaf whose 512 voxels verify is quantised:
// class b = the bits of max zz(q), zz(q) = (q << 1) ^ (q >> 31), 0 .. 16, record 64 * b bytes.  Any other selected leaf is raw:
// class 255, record = its 2048 bytes.
//
// Record of a quantised leaf: bit planes k = 0 .. b-1, least significant first, eight u64 words each; bit L of word j of plane k
// (at byte (8k + j) * 8) is bit k of zz(q) of voxel 64 j + L.  The wave that holds voxel 64 j + lane makes the word with one
// ballot and finds its bit again with one shift.
//
// One wave per leaf, RES_WAVES leaves per workgroup, whole waves leave early; no LDS, no barrier, no atomics (the scan aside,
// which is one workgroup with a running carry): what is written for a leaf depends on that leaf and its offset alone.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vqr {

constexpr int RES_WAVES = 4;        // leaves (waves) per workgroup
constexpr int CLASS_KEPT = 254;     // VQHIP_RES_KEPT
constexpr int CLASS_RAW = 255;      // VQHIP_RES_RAW
constexpr int SCAN_PER_LANE = 8;    // sizes per lane and step of resid_scan_k
constexpr int SCAN_TILE = 1024 * SCAN_PER_LANE;

__device__ __forceinline__ int64_t record_size(int cls)
{
    return cls == CLASS_KEPT ? 0 : cls == CLASS_RAW ? 2048 : 64 * cls;
}

// q of one voxel and whether the decoder's x^ + q * step lands within tol of x
__device__ __forceinline__ bool quantise(float x, float r, float step, float tol, int& q)
{
    const float t = __fdiv_rn(__fsub_rn(x, r), step);
    const bool fits = fabsf(t) <= 32767.0f;
    q = fits ? (int)rintf(t) : 0;
    const float xt = __fadd_rn(r, __fmul_rn((float)q, step));
    return fits && fabsf(__fsub_rn(x, xt)) <= tol;
}

// a value every lane of the wave holds alike, as the scalar the compiler cannot prove it to be (loops on it stay uniform)
__device__ __forceinline__ int uniform(int v)
{
    return __builtin_amdgcn_readfirstlane(v);
}

__device__ __forceinline__ unsigned zigzag(int q)
{
    return ((unsigned)q << 1) ^ (unsigned)(q >> 31);
}

// the lane's eight voxels 64 j + lane of x and x^ -> zz(q) of each; false if one of them does not verify
__device__ __forceinline__ bool leaf_zigzag(const float* __restrict__ x, const float* __restrict__ r, int lane, float step, float tol, unsigned (&zz)[8])
{
    float xv[8], rv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) xv[j] = x[64 * j + lane], rv[j] = r[64 * j + lane];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int q;
        ok = quantise(xv[j], rv[j], step, tol, q) && ok;
        zz[j] = zigzag(q);
    }
    return ok;
}

// cls[leaf] and size[leaf] (the record's bytes; resid_scan_k turns them into offsets in place) of every leaf
__global__ void __launch_bounds__(64 * RES_WAVES) resid_class_k(const float* __restrict__ orig, const float* __restrict__ recon,
                                                               const float* __restrict__ err, int64_t n, float tol, uint8_t* __restrict__ cls,
                                                               int64_t* __restrict__ size)
{
    const int lane = threadIdx.x & 63;
    const int64_t leaf = (int64_t)blockIdx.x * RES_WAVES + (threadIdx.x >> 6);
    if (leaf >= n) return;
    if (err[leaf * 2] <= tol) {   // kept: nothing else of the leaf is read
        if (lane == 0) cls[leaf] = (uint8_t)CLASS_KEPT, size[leaf] = 0;
        return;
    }
    unsigned zz[8];
    const bool ok = leaf_zigzag(orig + leaf * 512, recon + leaf * 512, lane, __fmul_rn(1.875f, tol), tol, zz);
    unsigned any = zz[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) any |= zz[j];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) any |= __shfl_xor(any, m);   // the bits of the maximum are the bits of the union
    const bool failed = __ballot(!ok) != 0ull;
    if (lane == 0) {
        const int c = failed ? CLASS_RAW : 32 - __clz(any);   // |q| <= 32767: zz <= 65534, 16 bits at the most
        cls[leaf] = (uint8_t)c;
        size[leaf] = record_size(c);
    }
}

// size[0..n) -> exclusive prefix sums in place, size[n] = their sum.  One workgroup of 1024 lanes with a running carry,
// SCAN_PER_LANE consecutive sizes per lane and step: integer sums in a fixed order.
__global__ void __launch_bounds__(1024) resid_scan_k(int64_t* __restrict__ size, int64_t n)
{
    __shared__ int64_t wsum[16];
    __shared__ int64_t carry_s;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += SCAN_TILE) {
        const int64_t i0 = base + (int64_t)tid * SCAN_PER_LANE;
        int64_t v[SCAN_PER_LANE], sum = 0;
#pragma unroll
        for (int k = 0; k < SCAN_PER_LANE; ++k) {
            v[k] = i0 + k < n ? size[i0 + k] : 0;
            sum += v[k];
        }
        int64_t inc = sum;   // inclusive scan inside the wave
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int64_t o = __shfl_up(inc, m);
            if (lane >= m) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int64_t before = carry_s;
        for (int k = 0; k < wave; ++k) before += wsum[k];
        int64_t run = before + inc - sum;
#pragma unroll
        for (int k = 0; k < SCAN_PER_LANE; ++k) {
            if (i0 + k < n) size[i0 + k] = run;
            run += v[k];
        }
        __syncthreads();
        if (tid == 1023) carry_s = before + inc;
        __syncthreads();
    }
    if (tid == 0) size[n] = carry_s;
}

// every selected leaf's record at payload + off[leaf]; a record that ends beyond `capacity` is not written at all
__global__ void __launch_bounds__(64 * RES_WAVES) resid_pack_k(const float* __restrict__ orig, const float* __restrict__ recon, int64_t n, float tol,
                                                              const uint8_t* __restrict__ cls, const int64_t* __restrict__ off,
                                                              uint8_t* __restrict__ payload, int64_t capacity)
{
    const int lane = threadIdx.x & 63;
    const int64_t leaf = (int64_t)blockIdx.x * RES_WAVES + (threadIdx.x >> 6);
    if (leaf >= n) return;
    const int c = uniform(cls[leaf]);
    if (c == CLASS_KEPT || c == 0) return;
    const int64_t at = off[leaf];
    if (at + record_size(c) > capacity) return;
    const float* x = orig + leaf * 512;
    if (c == CLASS_RAW) {
        uint32_t* dst = reinterpret_cast<uint32_t*>(payload + at);
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[64 * j + lane] = __float_as_uint(x[64 * j + lane]);
        return;
    }
    unsigned zz[8];
    leaf_zigzag(x, recon + leaf * 512, lane, __fmul_rn(1.875f, tol), tol, zz);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(payload + at);
#pragma unroll
    for (int round = 0; round < 2; ++round) {   // planes 0 .. 7, then 8 .. 15: lane t of a round keeps its word 64 * round + t
        if (8 * round >= c) break;
        unsigned long long mine = 0;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int k = 8 * round + kk;
            if (k >= c) break;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned long long w = __ballot((zz[j] >> k) & 1u);
                if (lane == 8 * kk + j) mine = w;
            }
        }
        if (lane < 8 * (c - 8 * round)) dst[64 * round + lane] = mine;
    }
}

// in place on decoded leaves: a quantised leaf becomes x^ + q * step, a raw leaf its record, a kept leaf stays
__global__ void __launch_bounds__(64 * RES_WAVES) resid_apply_k(float* __restrict__ leaves, int64_t n, float tol, const uint8_t* __restrict__ cls,
                                                               const int64_t* __restrict__ off, const uint8_t* __restrict__ payload)
{
    const int lane = threadIdx.x & 63;
    const int64_t leaf = (int64_t)blockIdx.x * RES_WAVES + (threadIdx.x >> 6);
    if (leaf >= n) return;
    const int c = uniform(cls[leaf]);
    if (c == CLASS_KEPT) return;
    float* r = leaves + leaf * 512;
    const int64_t at = off[leaf];
    if (c == CLASS_RAW) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(payload + at);
#pragma unroll
        for (int j = 0; j < 8; ++j) r[64 * j + lane] = __uint_as_float(src[64 * j + lane]);
        return;
    }
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(payload + at);
    unsigned zz[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int round = 0; round < 2; ++round) {   // lane t of a round loads word 64 * round + t; every lane then reads bit `lane` of each
        if (8 * round >= c) break;
        const unsigned long long mine = lane < 8 * (c - 8 * round) ? src[64 * round + lane] : 0ull;
        const unsigned lo = (unsigned)mine, hi = (unsigned)(mine >> 32);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int k = 8 * round + kk;
            if (k >= c) break;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned long long w = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hi, 8 * kk + j) << 32) |
                                             (unsigned)__builtin_amdgcn_readlane((int)lo, 8 * kk + j);
                zz[j] |= (unsigned)((w >> lane) & 1ull) << k;
            }
        }
    }
    const float step = __fmul_rn(1.875f, tol);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int q = (int)(zz[j] >> 1) ^ -(int)(zz[j] & 1u);
        r[64 * j + lane] = __fadd_rn(r[64 * j + lane], __fmul_rn((float)q, step));
    }
}

}  // namespace vqr
