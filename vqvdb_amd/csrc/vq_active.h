// vq_active.h — kernels of the Vec3 handle's compact residual records (include/vqvdb_hip_vec3_active.h): records
// that hold only the ACTIVE voxels of a leaf.  The codes are those of vqr::resid_class_k<3, true> (vq_residual.h), value for value;
// what changes is the record.  With A the popcount of the leaf's eight mask words, W = ceil(A / 64) and the rank of an active voxel
// the number of active voxels with a smaller index:
//   kept                                   no record
//   quantised, code b_0 | b_1 << 5 | b_2 << 10     8 W (b_0 + b_1 + b_2) bytes: channel 0's planes, then channel 1's, then channel 2's;
//                                          plane k of channel c is W u64 words, bit L of word j = bit k of zz(q) of the active voxel of
//                                          rank 64 j + L in channel c, 0 at ranks >= A
//   raw                                    8 ceil(3 A / 2) bytes: the active voxels' three floats each in rank order, then zeros
// With A = 512 both are the records of vq_residual.h, byte for byte.
//
// The shape is vq_residual.h's: one wave per leaf, RES_WAVES leaves per workgroup, lane l holds the voxels 64 j + l, the leaf index is
// a scalar (vqr::wave_of_block<true>) and the eight mask words arrive at a wave-uniform address.  The rank of voxel 64 j + l is the
// popcount of the words below j (scalar) plus the mask bits of word j below lane l (one mbcnt pair).
//
// Compaction goes through LDS, 3 KB per wave (3 x 512 u16: zz <= 65534), the three channels in one trip.  Pack: an active voxel
// writes its zz to slot `rank` of each channel, lane L then reads the slots 64 j' + L, j' < W (0 from A on) and one ballot per plane
// and j' is a word of the record.  Apply is the inverse: lane L rebuilds the zz of the ranks 64 j' + L from the plane words, writes
// them to their slots and every active voxel reads slot `rank`.  A leaf with all 512 voxels active (wave-uniform) skips the trip:
// rank 64 j + l is voxel 64 j + l.  The words of a channel leave and arrive G = floor(64 / W) planes at a time: word k W + j' of such
// a group sits in lane (k - k0) W + j', so one coalesced store or load moves up to 64 words and the loop over planes and j' has no
// branch but its own.
// A wave's slice is used by that wave alone, once per launch, so no workgroup barrier stands between its writes and its reads: the
// LDS serves the ds instructions of one wave in the order of their issue, the compiler's own s_waitcnt lgkmcnt stands before the
// first use of a value read, and lds_order() (a wavefront-scope fence with a scheduling barrier) keeps the compiler from moving a
// read above the writes.  Every branch around a ballot, a readlane or lds_order() is on wave-uniform values (the code, A, W, the
// loop counters), so they run with the full wave.
//
// Everything global is written with ordinary vector stores; the sweep adds with 64-bit integer atomics (LDS, then global), so its
// sums are the same bits in every order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vq_rate.h"
#include "vq_residual.h"

namespace vqa {

using vqr::Format;
using vqr::RES_WAVES;
using code_t = Format<3>::code_t;

// the table above
__host__ __device__ __forceinline__ int64_t record_bytes(int code, int active)
{
    if (code == Format<3>::KEPT) return 0;
    if (code == Format<3>::RAW) return 8 * (int64_t)((3 * active + 1) / 2);
    return 8 * (int64_t)((active + 63) / 64) * (vqr::width(code, 0) + vqr::width(code, 1) + vqr::width(code, 2));
}

// a leaf's mask as its wave sees it: the eight words and the active voxels before each of them as scalars, the rank of the lane's
// eight voxels (meaningful where the voxel is active) per lane
struct LeafMask {
    unsigned long long word[8];
    int before[8];
    int active;

    __device__ __forceinline__ LeafMask(const unsigned long long* __restrict__ m)
    {
        int sum = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            word[j] = m[j];
            before[j] = sum;
            sum += __popcll(word[j]);
        }
        active = sum;
    }
    __device__ __forceinline__ bool on(int j, int lane) const { return (word[j] >> lane) & 1ull; }
    __device__ __forceinline__ int rank(int j) const   // of voxel 64 j + this lane
    {
        return before[j] + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(word[j] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)word[j], 0u));
    }
};

// between a wave's LDS writes and its reads of them (and back): see the head of the file
__device__ __forceinline__ void lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// resid_class_k<3, true> with the compact size: code[leaf] as there, size[leaf] = record_bytes(code, A)
__global__ void __launch_bounds__(64 * RES_WAVES) active_class_k(const float* __restrict__ orig, const float* __restrict__ recon,
                                                                const float* __restrict__ err, int64_t n, float tol, code_t* __restrict__ code,
                                                                int64_t* __restrict__ size, const unsigned long long* __restrict__ mask)
{
    const int lane = threadIdx.x & 63;
    const int64_t leaf = (int64_t)blockIdx.x * RES_WAVES + vqr::wave_of_block<true>();
    if (leaf >= n) return;
    if (err[leaf * 2] <= tol) {   // kept: nothing else of the leaf is read
        if (lane == 0) code[leaf] = (code_t)Format<3>::KEPT, size[leaf] = 0;
        return;
    }
    const unsigned long long* m = mask + leaf * 8;
    unsigned zz[8][3];
    const bool ok = vqr::leaf_zigzag<3, true>(orig + leaf * 1536, recon + leaf * 1536, lane, __fmul_rn(1.875f, tol), tol, zz, m);
    unsigned any[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        any[ch] = zz[0][ch];
#pragma unroll
        for (int j = 1; j < 8; ++j) any[ch] |= zz[j][ch];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) any[ch] |= __shfl_xor(any[ch], s);   // the bits of the maximum are the bits of the union
    }
    const bool failed = __ballot(!ok) != 0ull;
    if (lane == 0) {
        int active = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) active += __popcll(m[j]);
        int c = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c |= (32 - __clz(any[ch])) << (5 * ch);
        if (failed) c = Format<3>::RAW;
        code[leaf] = (code_t)c;
        size[leaf] = record_bytes(c, active);
    }
}

// every selected leaf's compact record at payload + off[leaf]; a record that ends beyond `capacity` is not written at all
__global__ void __launch_bounds__(64 * RES_WAVES) active_pack_k(const float* __restrict__ orig, const float* __restrict__ recon, int64_t n, float tol,
                                                               const code_t* __restrict__ code, const int64_t* __restrict__ off,
                                                               uint8_t* __restrict__ payload, int64_t capacity,
                                                               const unsigned long long* __restrict__ mask)
{
    __shared__ uint16_t slots[RES_WAVES][3 * 512];
    const int lane = threadIdx.x & 63;
    const int wave = vqr::wave_of_block<true>();
    const int64_t leaf = (int64_t)blockIdx.x * RES_WAVES + wave;
    if (leaf >= n) return;
    const int c = vqr::uniform(code[leaf]);
    if (c == Format<3>::KEPT || c == 0) return;
    const LeafMask lm(mask + leaf * 8);
    const int A = vqr::uniform(lm.active);
    if (A == 0) return;   // raw without an active voxel: an empty record
    const int64_t at = off[leaf];
    if (at + record_bytes(c, A) > capacity) return;
    const float* x = orig + leaf * 1536;
    if (c == Format<3>::RAW) {
        uint32_t* dst = reinterpret_cast<uint32_t*>(payload + at);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (!lm.on(j, lane)) continue;
            const int r = lm.rank(j);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) dst[3 * r + ch] = __float_as_uint(x[3 * (64 * j + lane) + ch]);
        }
        if ((A & 1) && lane == 0) dst[3 * A] = 0u;   // 12 A bytes end on a half word: four zero bytes to the multiple of 8
        return;
    }
    unsigned zz[8][3];
    vqr::leaf_zigzag<3, true>(x, recon + leaf * 1536, lane, __fmul_rn(1.875f, tol), tol, zz, mask + leaf * 8);
    const int W = (A + 63) >> 6, G = 64 / W;
    unsigned v[8][3];   // zz of the ranks 64 j' + lane
    if (A == 512) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[j][ch] = zz[j][ch];
    } else {
        uint16_t* slot = slots[wave];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (!lm.on(j, lane)) continue;
            const int r = lm.rank(j);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) slot[512 * ch + r] = (uint16_t)zz[j][ch];
        }
        lds_order();
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const bool held = 64 * jj + lane < A;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[jj][ch] = held ? slot[512 * ch + 64 * jj + lane] : 0u;
        }
    }
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(payload + at);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int b = vqr::width(c, ch);   // wave-uniform with c
        for (int k0 = 0; k0 < b; k0 += G) {
            const int planes = b - k0 < G ? b - k0 : G;
            unsigned long long mine = 0;
#pragma unroll 1
            for (int kk = 0; kk < planes; ++kk) {
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {   // j' >= W: a ballot of zeros that no lane keeps
                    const unsigned long long w = __ballot((v[jj][ch] >> (k0 + kk)) & 1u);
                    if (lane == (jj < W ? kk * W + jj : -1)) mine = w;
                }
            }
            if (lane < planes * W) dst[k0 * W + lane] = mine;
        }
        dst += b * W;
    }
}

// in place on decoded leaves, the inverse of active_pack_k: an active voxel of a quantised leaf becomes x^ + q * step (a channel of
// width 0: x^ + 0 * step), of a raw leaf the record's value, of a kept leaf it stays; an inactive voxel of every leaf receives the
// background where one is given and is not touched otherwise
__global__ void __launch_bounds__(64 * RES_WAVES) active_apply_k(float* __restrict__ leaves, int64_t n, float tol, const code_t* __restrict__ code,
                                                                const int64_t* __restrict__ off, const uint8_t* __restrict__ payload,
                                                                const unsigned long long* __restrict__ mask, int has_background, float bg0,
                                                                float bg1, float bg2)
{
    __shared__ uint16_t slots[RES_WAVES][3 * 512];
    const int lane = threadIdx.x & 63;
    const int wave = vqr::wave_of_block<true>();
    const int64_t leaf = (int64_t)blockIdx.x * RES_WAVES + wave;
    if (leaf >= n) return;
    const int c = vqr::uniform(code[leaf]);
    if (c == Format<3>::KEPT && !has_background) return;
    const LeafMask lm(mask + leaf * 8);
    const int A = vqr::uniform(lm.active);
    float* r = leaves + leaf * 1536;
    if (has_background && A < 512) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (lm.on(j, lane)) continue;
            float* v = r + 3 * (64 * j + lane);
            v[0] = bg0, v[1] = bg1, v[2] = bg2;
        }
    }
    if (c == Format<3>::KEPT || A == 0) return;
    const int64_t at = off[leaf];
    if (c == Format<3>::RAW) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(payload + at);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (!lm.on(j, lane)) continue;
            const int rk = lm.rank(j);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) r[3 * (64 * j + lane) + ch] = __uint_as_float(src[3 * rk + ch]);
        }
        return;
    }
    const int W = (A + 63) >> 6, G = 64 / W;
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(payload + at);
    unsigned v[8][3];   // zz of the ranks 64 j' + lane
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int b = vqr::width(c, ch);   // wave-uniform with c
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) v[jj][ch] = 0u;
        for (int k0 = 0; k0 < b; k0 += G) {
            const int planes = b - k0 < G ? b - k0 : G;
            const unsigned long long mine = lane < planes * W ? src[k0 * W + lane] : 0ull;
            const unsigned lo = (unsigned)mine, hi = (unsigned)(mine >> 32);
#pragma unroll 1
            for (int kk = 0; kk < planes; ++kk) {
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {   // j' >= W: lane 0's word, masked out
                    const int from = jj < W ? kk * W + jj : 0;
                    const unsigned long long w = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hi, from) << 32) |
                                                 (unsigned)__builtin_amdgcn_readlane((int)lo, from);
                    v[jj][ch] |= (jj < W ? (unsigned)((w >> lane) & 1ull) : 0u) << (k0 + kk);
                }
            }
        }
        src += b * W;
    }
    unsigned zz[8][3];   // of the lane's voxels 64 j + lane, meaningful where the voxel is active
    if (A == 512) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) zz[j][ch] = v[j][ch];
    } else {
        uint16_t* slot = slots[wave];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            if (jj >= W) break;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) slot[512 * ch + 64 * jj + lane] = (uint16_t)v[jj][ch];
        }
        lds_order();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int rk = lm.on(j, lane) ? lm.rank(j) : 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) zz[j][ch] = slot[512 * ch + rk];
        }
    }
    const float step = __fmul_rn(1.875f, tol);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (!lm.on(j, lane)) continue;
        float* p = r + 3 * (64 * j + lane);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {   // a channel of width 0 has zz = 0: x^ + 0 * step
            const int q = (int)(zz[j][ch] >> 1) ^ -(int)(zz[j][ch] & 1u);
            p[ch] = __fadd_rn(p[ch], __fmul_rn((float)q, step));
        }
    }
}

// bytes[t] grows by the compact payload bytes of the n leaves at tols.t[t]: vqrate::sweep_k<3, true>'s classification of every leaf at
// every rung (that kernel's comment explains why a lane's values of an inactive voxel are loaded as x = x^ = +0), with
// record_bytes(code, A) summed instead of a class counted.  The sums are 64-bit from the wave on: lane 0 adds to an LDS table of
// u64 per rung, the workgroup adds its non-zero cells to bytes[] with 64-bit integer atomics.  A leaf kept at every rung and a leaf
// without an active voxel add nothing and read nothing but the error and the mask.
__global__ void __launch_bounds__(64 * vqrate::RATE_WAVES) active_sweep_k(const float* __restrict__ orig, const float* __restrict__ recon,
                                                                         const float* __restrict__ err, int64_t n, const vqrate::Tols tols,
                                                                         unsigned long long* __restrict__ bytes,
                                                                         const unsigned long long* __restrict__ mask)
{
    __shared__ unsigned long long tab[vqrate::RATE_MAX_TOLS];
    const int lane = threadIdx.x & 63;
    const int count = tols.count;
    for (int i = threadIdx.x; i < count; i += 64 * vqrate::RATE_WAVES) tab[i] = 0ull;
    float least = tols.t[0];
    bool nan_rung = false;
#pragma unroll 1
    for (int t = 0; t < count; ++t) {
        const float tol = tols.t[t];
        nan_rung = nan_rung || tol != tol;
        least = tol < least ? tol : least;
    }
    __syncthreads();
    for (int64_t leaf = (int64_t)blockIdx.x * vqrate::RATE_WAVES + vqr::wave_of_block<true>(); leaf < n;
         leaf += (int64_t)gridDim.x * vqrate::RATE_WAVES) {
        const float e = __int_as_float(vqr::uniform(__float_as_int(err[leaf * 2])));
        if (!nan_rung && e <= least) continue;   // kept at every rung
        int A = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) A += __popcll(mask[leaf * 8 + j]);
        A = vqr::uniform(A);
        if (A == 0) continue;                    // kept, or selected with code 0: no record at any rung
        const float* x = orig + leaf * 1536;
        const float* r = recon + leaf * 1536;
        float xv[8][3], rv[8][3];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int at = 3 * (64 * j + lane);
            const bool on = (mask[leaf * 8 + j] >> lane) & 1ull;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) xv[j][ch] = on ? x[at + ch] : 0.0f, rv[j][ch] = on ? r[at + ch] : 0.0f;
        }
        const unsigned long long raw = 8ull * (unsigned)((3 * A + 1) >> 1), per_plane = 8ull * (unsigned)((A + 63) >> 6);
#pragma unroll 1
        for (int t = 0; t < count; ++t) {
            const float tol = tols.t[t];
            if (e <= tol) continue;              // the selection rule of resid_class_k: equality keeps, NaN on either side selects
            const float step = __fmul_rn(1.875f, tol);
            unsigned bad = 0, any[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                unsigned u = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    int q;
                    bad |= vqr::quantise(xv[j][ch], rv[j][ch], step, tol, q) ? 0u : 1u;
                    u |= vqr::zigzag(q);
                }
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) u |= __shfl_xor(u, s);
                any[ch] = u;
            }
            const bool failed = __ballot(bad) != 0ull;
            if (lane == 0) {
                int planes = 96;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) planes -= __clz(any[ch]);
                const unsigned long long add = failed ? raw : per_plane * (unsigned)planes;
                if (add) atomicAdd(&tab[t], add);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < count; i += 64 * vqrate::RATE_WAVES) {
        const unsigned long long v = tab[i];
        if (v) atomicAdd(&bytes[i], v);
    }
}

}  // namespace vqa
