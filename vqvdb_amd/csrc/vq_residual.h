// vq_residual.h — kernels of the quantised residuals of both handles (include/vqvdb_hip_residual.h and
// include/vqvdb_hip_vec3_residual.h), templated on the channels C of a voxel: 1 for the scalar handle, 3 for
// the Vec3 one.  A leaf over the tolerance is stored as x - x^ on a grid of 1.875 * tol, bit-packed in planes with one width per
// channel, instead of raw; a leaf that the grid cannot hold within the tolerance stays raw.  resid_class_k decides, resid_scan_k
// places, resid_pack_k writes, resid_apply_k undoes.
//
// Arithmetic (pinned by the format; tests/torch_ref_residual.py and tests/torch_ref_vec3_residual.py restate it in numpy float32,
// to the bit).  Float32, never fused:
//   step = 1.875f * tol        d = x - x^        t = d / step        q = rintf(t)  (ties to even)        x~ = x^ + (float)q * step
//   the value verifies iff |t| <= 32767 and |x - x~| <= tol            (both false on NaN)
// A leaf with leaf_err[leaf][0] <= tol is kept (code KEPT, no record).  A selected leaf whose 512 * C values verify is quantised:
// code b_0 | b_1 << 5 | .. (one field of five bits per channel), b_c = the bits of max zz(q) over channel c's 512 values,
// zz(q) = (q << 1) ^ (q >> 31), 0 .. 16 each, record 64 * (b_0 + ..) bytes.  Any other selected leaf is raw: code RAW, record = its
// 2048 * C bytes.  Format<C> holds the code's type and the two sentinels.
//
// Record of a quantised leaf: channel 0's planes, then channel 1's, ..; inside a channel planes k = 0 .. b_c - 1, least
// significant first, eight u64 words each; bit L of word j of plane k is bit k of zz(q) of voxel 64 j + L in that channel.
// Channel c starts at word 8 * (b_0 + .. + b_{c-1}).
//
// A leaf is [512][C], channels last: lane l of the leaf's wave holds the voxels 64 j + l, j = 0 .. 7, with their C channels
// (consecutive floats), so a plane word is one ballot and a lane finds its bit again with one shift.  One wave per leaf,
// RES_WAVES leaves per workgroup, whole waves leave early; no LDS, no barrier, no atomics (the scan aside, which is one workgroup
// with a running carry): what is written for a leaf depends on that leaf and its offset alone.
//
// MASKED (vq_mask.h, include/vqvdb_hip_vec3_mask.h; instantiated for C = 3): leaf_zigzag, resid_class_k and resid_pack_k also take the leaves'
// value masks, uint64 [n][8], bit L of word j = voxel 64 j + L, which is the lane-to-voxel map above: the wave's leaf index is made
// uniform, word j arrives by a scalar load and lane l tests bit l.  A value of an inactive voxel has zz = 0 and verifies whatever
// x and x^ hold there; everything else is the rule above on the active values.  The records and resid_apply_k do not change.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vqr {

constexpr int RES_WAVES = 4;        // leaves (waves) per workgroup
constexpr int SCAN_PER_LANE = 8;    // sizes per lane and step of resid_scan_k
constexpr int SCAN_TILE = 1024 * SCAN_PER_LANE;

template <int C>
struct Format;
template <>
struct Format<1> {
    using code_t = uint8_t;
    static constexpr int KEPT = 254, RAW = 255;         // VQHIP_RES_KEPT, VQHIP_RES_RAW
};
template <>
struct Format<3> {
    using code_t = uint16_t;
    static constexpr int KEPT = 0xFFFE, RAW = 0xFFFF;   // VQHIP_VEC3_RES_KEPT, VQHIP_VEC3_RES_RAW
};

__host__ __device__ __forceinline__ int width(int code, int ch)
{
    return (code >> (5 * ch)) & 31;
}

template <int C>
__host__ __device__ __forceinline__ int64_t record_size(int code)
{
    if (code == Format<C>::KEPT) return 0;
    if (code == Format<C>::RAW) return 2048 * C;
    int planes = 0;
    for (int ch = 0; ch < C; ++ch) planes += width(code, ch);
    return 64 * planes;
}

// what a caller's array or a file may hold: a sentinel, or C widths of 0 .. 16 and nothing above them
template <int C>
__host__ __device__ __forceinline__ bool code_ok(int code)
{
    if (code == Format<C>::KEPT || code == Format<C>::RAW) return true;
    bool ok = (code >> (5 * C)) == 0;
    for (int ch = 0; ch < C; ++ch) ok = ok && width(code, ch) <= 16;
    return ok;
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

// the wave of a workgroup of 64-lane waves, and with MASKED as a scalar: the leaf index and with it the address of the leaf's mask
// words are then uniform by construction
template <bool MASKED>
__device__ __forceinline__ int wave_of_block()
{
    if constexpr (MASKED) return uniform((int)(threadIdx.x >> 6));
    else return (int)(threadIdx.x >> 6);
}

// the lane's 8 * C values (voxels 64 j + lane, C channels each) of x and x^ -> zz(q) of each; false if one of them does not verify.
// MASKED: mask is the leaf's eight words (a uniform address); an inactive voxel's values give zz = 0 and never fail
template <int C, bool MASKED = false>
__device__ __forceinline__ bool leaf_zigzag(const float* __restrict__ x, const float* __restrict__ r, int lane, float step, float tol,
                                            unsigned (&zz)[8][C], const unsigned long long* __restrict__ mask = nullptr)
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int at = C * (64 * j + lane);
        float xv[C], rv[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) xv[ch] = x[at + ch], rv[ch] = r[at + ch];
        bool active = true;
        if constexpr (MASKED) active = (mask[j] >> lane) & 1ull;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            int q;
            const bool fine = quantise(xv[ch], rv[ch], step, tol, q);
            if constexpr (MASKED) {
                ok = (fine || !active) && ok;
                zz[j][ch] = active ? zigzag(q) : 0u;
            } else {
                ok = fine && ok;
                zz[j][ch] = zigzag(q);
            }
        }
    }
    return ok;
}

// code[leaf] and size[leaf] (the record's bytes; resid_scan_k turns them into offsets in place) of every leaf.  MASKED: err is the
// masked error and mask [n][8] the value masks; a selected leaf without an active voxel gets code 0
template <int C, bool MASKED = false>
__global__ void __launch_bounds__(64 * RES_WAVES) resid_class_k(const float* __restrict__ orig, const float* __restrict__ recon,
                                                               const float* __restrict__ err, int64_t n, float tol,
                                                               typename Format<C>::code_t* __restrict__ code, int64_t* __restrict__ size,
                                                               const unsigned long long* __restrict__ mask = nullptr)
{
    using code_t = typename Format<C>::code_t;
    const int lane = threadIdx.x & 63;
    const int64_t leaf = (int64_t)blockIdx.x * RES_WAVES + wave_of_block<MASKED>();
    if (leaf >= n) return;
    if (err[leaf * 2] <= tol) {   // kept: nothing else of the leaf is read
        if (lane == 0) code[leaf] = (code_t)Format<C>::KEPT, size[leaf] = 0;
        return;
    }
    unsigned zz[8][C];
    const bool ok = leaf_zigzag<C, MASKED>(orig + leaf * (512 * C), recon + leaf * (512 * C), lane, __fmul_rn(1.875f, tol), tol, zz,
                                           MASKED ? mask + leaf * 8 : nullptr);
    unsigned any[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        any[ch] = zz[0][ch];
#pragma unroll
        for (int j = 1; j < 8; ++j) any[ch] |= zz[j][ch];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) any[ch] |= __shfl_xor(any[ch], m);   // the bits of the maximum are the bits of the union
    }
    const bool failed = __ballot(!ok) != 0ull;
    if (lane == 0) {
        int c = 0;   // |q| <= 32767: zz <= 65534, 16 bits at the most in every field
#pragma unroll
        for (int ch = 0; ch < C; ++ch) c |= (32 - __clz(any[ch])) << (5 * ch);
        if (failed) c = Format<C>::RAW;
        code[leaf] = (code_t)c;
        size[leaf] = record_size<C>(c);
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

// every selected leaf's record at payload + off[leaf]; a record that ends beyond `capacity` is not written at all.  MASKED: the
// bits of an inactive voxel are 0 in a quantised record; a raw record is the leaf as given, inactive voxels included
template <int C, bool MASKED = false>
__global__ void __launch_bounds__(64 * RES_WAVES) resid_pack_k(const float* __restrict__ orig, const float* __restrict__ recon, int64_t n, float tol,
                                                              const typename Format<C>::code_t* __restrict__ code, const int64_t* __restrict__ off,
                                                              uint8_t* __restrict__ payload, int64_t capacity,
                                                              const unsigned long long* __restrict__ mask = nullptr)
{
    const int lane = threadIdx.x & 63;
    const int64_t leaf = (int64_t)blockIdx.x * RES_WAVES + wave_of_block<MASKED>();
    if (leaf >= n) return;
    const int c = uniform(code[leaf]);
    if (c == Format<C>::KEPT || c == 0) return;
    const int64_t at = off[leaf];
    if (at + record_size<C>(c) > capacity) return;
    const float* x = orig + leaf * (512 * C);
    if (c == Format<C>::RAW) {
        uint32_t* dst = reinterpret_cast<uint32_t*>(payload + at);
#pragma unroll
        for (int i = 0; i < 8 * C; ++i) dst[64 * i + lane] = __float_as_uint(x[64 * i + lane]);
        return;
    }
    unsigned zz[8][C];
    leaf_zigzag<C, MASKED>(x, recon + leaf * (512 * C), lane, __fmul_rn(1.875f, tol), tol, zz, MASKED ? mask + leaf * 8 : nullptr);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(payload + at);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const int b = width(c, ch);   // wave-uniform with c: every ballot below runs with the full wave
#pragma unroll
        for (int round = 0; round < 2; ++round) {   // planes 0 .. 7, then 8 .. 15: lane t of a round keeps its word 64 * round + t
            if (8 * round >= b) break;
            unsigned long long mine = 0;
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const int k = 8 * round + kk;
                if (k >= b) break;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned long long w = __ballot((zz[j][ch] >> k) & 1u);
                    if (lane == 8 * kk + j) mine = w;
                }
            }
            if (lane < 8 * (b - 8 * round)) dst[64 * round + lane] = mine;
        }
        dst += 8 * b;
    }
}

// in place on decoded leaves: a quantised leaf becomes x^ + q * step, a raw leaf its record, a kept leaf stays
template <int C>
__global__ void __launch_bounds__(64 * RES_WAVES) resid_apply_k(float* __restrict__ leaves, int64_t n, float tol,
                                                               const typename Format<C>::code_t* __restrict__ code, const int64_t* __restrict__ off,
                                                               const uint8_t* __restrict__ payload)
{
    const int lane = threadIdx.x & 63;
    const int64_t leaf = (int64_t)blockIdx.x * RES_WAVES + (threadIdx.x >> 6);
    if (leaf >= n) return;
    const int c = uniform(code[leaf]);
    if (c == Format<C>::KEPT) return;
    float* r = leaves + leaf * (512 * C);
    const int64_t at = off[leaf];
    if (c == Format<C>::RAW) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(payload + at);
#pragma unroll
        for (int i = 0; i < 8 * C; ++i) r[64 * i + lane] = __uint_as_float(src[64 * i + lane]);
        return;
    }
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(payload + at);
    const float step = __fmul_rn(1.875f, tol);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const int b = width(c, ch);   // 0: the channel still becomes x^ + 0 * step, as the format says (a -0 turns into +0)
        unsigned zz[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int round = 0; round < 2; ++round) {   // lane t of a round loads word 64 * round + t; every lane then reads bit `lane` of each
            if (8 * round >= b) break;
            const unsigned long long mine = lane < 8 * (b - 8 * round) ? src[64 * round + lane] : 0ull;
            const unsigned lo = (unsigned)mine, hi = (unsigned)(mine >> 32);
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const int k = 8 * round + kk;
                if (k >= b) break;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned long long w = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hi, 8 * kk + j) << 32) |
                                                 (unsigned)__builtin_amdgcn_readlane((int)lo, 8 * kk + j);
                    zz[j] |= (unsigned)((w >> lane) & 1ull) << k;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int q = (int)(zz[j] >> 1) ^ -(int)(zz[j] & 1u);
            float* v = r + C * (64 * j + lane) + ch;
            *v = __fadd_rn(*v, __fmul_rn((float)q, step));
        }
        src += 8 * b;
    }
}

}  // namespace vqr
