// vq_vec3_residual.h — kernels of the Vec3 handle's quantised residuals (include/vqvdb_hip_vec3_residual.h): a
// leaf over the tolerance is stored as x - x^ on a grid of 1.875 * tol, bit-packed in planes with one width per channel, instead
// of raw; a leaf that the grid cannot hold within the tolerance stays raw.  class_k decides, vqr::resid_scan_k (vq_residual.h,
// unchanged) places, pack_k writes, apply_k undoes.
//
// Arithmetic per value: vqr::quantise of vq_residual.h, the scalar format's, to the bit (tests/torch_ref_vec3_residual.py restates
// the Vec3 format in numpy float32).  A leaf with leaf_err[leaf][0] <= tol is kept (code 0xFFFE, no record).  A selected leaf whose
// 1536 values verify is quantised: code b0 | b1 << 5 | b2 << 10, b_c = the bits of max zz(q) over channel c's 512 values, 0 .. 16
// each, record 64 * (b0 + b1 + b2) bytes.  Any other selected leaf is raw: code 0xFFFF, record = its 6144 bytes.
//
// Record of a quantised leaf: channel 0's planes, then channel 1's, then channel 2's; inside a channel planes k = 0 .. b_c - 1,
// least significant first, eight u64 words each; bit L of word j of plane k is bit k of zz(q) of voxel 64 j + L in that channel.
// Channel c starts at word 8 * (b_0 + .. + b_{c-1}).
//
// A leaf is [512][3], channels last: lane l of the leaf's wave holds the voxels 64 j + l, j = 0 .. 7, with their three channels
// (three consecutive floats per voxel), so a plane word is one ballot and a lane finds its bit again with one shift, as in vqr.
// One wave per leaf, RES_WAVES leaves per workgroup, whole waves leave early; no LDS, no barrier, no atomics: what is written
// for a leaf depends on that leaf and its offset alone.
#pragma once

#include "vq_residual.h"

namespace v3r {

constexpr int RES_WAVES = 4;         // leaves (waves) per workgroup
constexpr int CODE_KEPT = 0xFFFE;    // VQHIP_VEC3_RES_KEPT
constexpr int CODE_RAW = 0xFFFF;     // VQHIP_VEC3_RES_RAW
constexpr int LEAF_FLOATS = 1536;
constexpr int RAW_BYTES = LEAF_FLOATS * 4;

__device__ __forceinline__ int width(int code, int ch)
{
    return (code >> (5 * ch)) & 31;
}

__device__ __forceinline__ int64_t record_size(int code)
{
    return code == CODE_KEPT ? 0 : code == CODE_RAW ? RAW_BYTES : 64 * (width(code, 0) + width(code, 1) + width(code, 2));
}

// the lane's 24 values (voxels 64 j + lane, three channels each) of x and x^ -> zz(q) of each; false if one of them does not verify
__device__ __forceinline__ bool leaf_zigzag(const float* __restrict__ x, const float* __restrict__ r, int lane, float step, float tol,
                                            unsigned (&zz)[8][3])
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int at = 3 * (64 * j + lane);
        float xv[3], rv[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) xv[ch] = x[at + ch], rv[ch] = r[at + ch];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            int q;
            ok = vqr::quantise(xv[ch], rv[ch], step, tol, q) && ok;
            zz[j][ch] = vqr::zigzag(q);
        }
    }
    return ok;
}

// code[leaf] and size[leaf] (the record's bytes; vqr::resid_scan_k turns them into offsets in place) of every leaf
__global__ void __launch_bounds__(64 * RES_WAVES) class_k(const float* __restrict__ orig, const float* __restrict__ recon, const float* __restrict__ err,
                                                         int64_t n, float tol, uint16_t* __restrict__ code, int64_t* __restrict__ size)
{
    const int lane = threadIdx.x & 63;
    const int64_t leaf = (int64_t)blockIdx.x * RES_WAVES + (threadIdx.x >> 6);
    if (leaf >= n) return;
    if (err[leaf * 2] <= tol) {   // kept: nothing else of the leaf is read
        if (lane == 0) code[leaf] = (uint16_t)CODE_KEPT, size[leaf] = 0;
        return;
    }
    unsigned zz[8][3];
    const bool ok = leaf_zigzag(orig + leaf * LEAF_FLOATS, recon + leaf * LEAF_FLOATS, lane, __fmul_rn(1.875f, tol), tol, zz);
    unsigned any[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        any[ch] = zz[0][ch];
#pragma unroll
        for (int j = 1; j < 8; ++j) any[ch] |= zz[j][ch];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) any[ch] |= __shfl_xor(any[ch], m);   // the bits of the maximum are the bits of the union
    }
    const bool failed = __ballot(!ok) != 0ull;
    if (lane == 0) {
        // |q| <= 32767: zz <= 65534, 16 bits at the most in every field
        const int c = failed ? CODE_RAW : (32 - __clz(any[0])) | (32 - __clz(any[1])) << 5 | (32 - __clz(any[2])) << 10;
        code[leaf] = (uint16_t)c;
        size[leaf] = record_size(c);
    }
}

// every selected leaf's record at payload + off[leaf]; a record that ends beyond `capacity` is not written at all
__global__ void __launch_bounds__(64 * RES_WAVES) pack_k(const float* __restrict__ orig, const float* __restrict__ recon, int64_t n, float tol,
                                                        const uint16_t* __restrict__ code, const int64_t* __restrict__ off,
                                                        uint8_t* __restrict__ payload, int64_t capacity)
{
    const int lane = threadIdx.x & 63;
    const int64_t leaf = (int64_t)blockIdx.x * RES_WAVES + (threadIdx.x >> 6);
    if (leaf >= n) return;
    const int c = vqr::uniform(code[leaf]);
    if (c == CODE_KEPT || c == 0) return;
    const int64_t at = off[leaf];
    if (at + record_size(c) > capacity) return;
    const float* x = orig + leaf * LEAF_FLOATS;
    if (c == CODE_RAW) {
        uint32_t* dst = reinterpret_cast<uint32_t*>(payload + at);
#pragma unroll
        for (int i = 0; i < LEAF_FLOATS / 64; ++i) dst[64 * i + lane] = __float_as_uint(x[64 * i + lane]);
        return;
    }
    unsigned zz[8][3];
    leaf_zigzag(x, recon + leaf * LEAF_FLOATS, lane, __fmul_rn(1.875f, tol), tol, zz);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(payload + at);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
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
__global__ void __launch_bounds__(64 * RES_WAVES) apply_k(float* __restrict__ leaves, int64_t n, float tol, const uint16_t* __restrict__ code,
                                                         const int64_t* __restrict__ off, const uint8_t* __restrict__ payload)
{
    const int lane = threadIdx.x & 63;
    const int64_t leaf = (int64_t)blockIdx.x * RES_WAVES + (threadIdx.x >> 6);
    if (leaf >= n) return;
    const int c = vqr::uniform(code[leaf]);
    if (c == CODE_KEPT) return;
    float* r = leaves + leaf * LEAF_FLOATS;
    const int64_t at = off[leaf];
    if (c == CODE_RAW) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(payload + at);
#pragma unroll
        for (int i = 0; i < LEAF_FLOATS / 64; ++i) r[64 * i + lane] = __uint_as_float(src[64 * i + lane]);
        return;
    }
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(payload + at);
    const float step = __fmul_rn(1.875f, tol);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
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
            float* v = r + 3 * (64 * j + lane) + ch;
            *v = __fadd_rn(*v, __fmul_rn((float)q, step));
        }
        src += 8 * b;
    }
}

}  // namespace v3r
