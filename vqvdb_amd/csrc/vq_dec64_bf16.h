// vq_dec64_bf16.h — the decoder's two 64 -> 64 convs at 4^3 (ResidualBlock(64), decoder.res_stack.0.conv1 / .conv2) with bf16
// matrix operands: the opt-in decode mode vqhip_set_decode_mode(VQHIP_PRECISION_BF16), DESIGN.md §23.  Everything else of the
// decoder keeps its fp32 kernels, and every tensor in global memory stays fp32 in the leaf-tile layout act[tile][pos][C/4][32][4].
//
// Arithmetic: both operands of every product are bf16 (round to nearest even, v3b::bf16_bits): the weight when its fragments are
// packed (frag_k), the activation when the LDS image is filled, after GroupNorm + ReLU has been evaluated in fp32 with the fp32
// path's formula, max(fmaf(x, rstd*gamma, fmaf(-mean, rstd*gamma, beta)), 0).  v_mfma_f32_16x16x32_bf16 accumulates the (exact)
// products in fp32: valid taps ascending (kd,kh,kw), padding taps skipped, the two 32-channel blocks of a tap ascending; acc + bias
// at the end; conv2 stores skip + 0.1 (acc + bias) with two roundings.
//
// Shape: one workgroup of 8 waves per 16-leaf HALF tile.  The half tile's whole input (64 positions x 64 channels x 16 leaves)
// is transformed once and sits in LDS as bf16, 128 KiB: image[pos][chunk of 8 channels][leaf][8 bf16], so the B fragment of
// (position, 32-channel block) is one conflict-free ds_read_b128 per lane (lane = leaf + 16 * chunk-in-block), and no transpose is
// needed: a lane's 8 consecutive channels are two adjacent float4 of the tile layout, 512 B apart.  GEMM: M = 16 output channels,
// N = the 16 leaves, K = 32 input channels of one tap at one position.  A wave owns one output row (od,oh) of 4 positions and all
// 64 output channels (16 accumulators), two rows one after the other; per valid (kd,kh) it reads the input row's eight B fragments
// once and walks kw x channel block, the four A fragments of each (bf16, fragment order) coming straight from L1 / L2.  The result
// (lane = leaf, registers = 4 consecutive output channels) goes back as float4 like the fp32 kernels' stores.
//
// Statistics: an output row is one block of §4's 16-block rule.  The wave stores the block's sums as the position-split launches
// of conv_rows16_k do — fp64 (sum, sum of squares) per 4-channel quad for conv1 (gn2), fp32 channel sums for conv2 (attention
// gate) — and gn_combine_k<true> / csum_combine_k<64> add the 16 blocks in order: the fp32 path's definitions on the bf16 tensors.
#pragma once

#include "vq_bf16.h"
#include "vq_kernels.h"

namespace d64b {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct Args {
    const float* in;        // [tile][64][16][32][4]
    float* out;             // the same layout
    const uint16_t* wf;     // bf16 A fragments [27 taps][2 channel blocks][4 cout tiles][64 lanes][8]
    const float* bias;      // plain [64]
    const float* skip;      // conv2: the residual input, layout of out
    const float* in_mean;   // [tile][8][32]
    const float* in_rstd;
    const float* in_gamma;  // [64]
    const float* in_beta;
    double* part_s;         // conv1: [tile][16 blocks][16 quads][32]
    double* part_q;
    float* part_c;          // conv2: [tile][16 blocks][64 channels][32]
};

constexpr int THREADS = 512;
constexpr int FRAG_ELEMS = 27 * 2 * 4 * 64 * 8;    // bf16 elements of one conv's fragments (221 184 B)
constexpr size_t LDS_BYTES = 64 * 8 * 16 * 16;     // 128 KiB: the half tile's input as bf16

// byte offset of the 8 channels 8 chunk .. 8 chunk + 7 of (position, leaf of the half tile) in the LDS image
__device__ __forceinline__ int img_off(int pos, int chunk, int leaf) { return ((pos * 8 + chunk) * 16 + leaf) * 16; }

// RESID false: conv1 (GroupNorm partials of its output); true: conv2 (skip + 0.1 y, channel-sum partials).  grid = 2 * n_tiles.
template <bool RESID>
__global__ __launch_bounds__(THREADS, 1) void conv_k(Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xb[];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x >> 1, l0 = 16 * (blockIdx.x & 1);   // first leaf of the half tile inside its tile

    // ---- fill: one item = 8 channels (one GroupNorm group) of one position of one leaf; fp32 transform, then bf16 ----
    {
        const int leaf = tid & 15, c8 = (tid >> 4) & 7, p0 = tid >> 7;
        const int jj = l0 + leaf;
        const float mean = a.in_mean[((size_t)tile * 8 + c8) * 32 + jj], rstd = a.in_rstd[((size_t)tile * 8 + c8) * 32 + jj];
        float ta[8], tb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ta[j] = rstd * a.in_gamma[8 * c8 + j];
            tb[j] = __builtin_fmaf(-mean, ta[j], a.in_beta[8 * c8 + j]);
        }
        const f32x4* src = (const f32x4*)a.in + (size_t)tile * (64 * 16 * 32) + (2 * c8) * 32 + jj;
#pragma unroll 8
        for (int it = 0; it < 16; ++it) {
            const int p = p0 + 4 * it;
            const f32x4 lo = src[p * 512], hi = src[p * 512 + 32];
            const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            u32x4 pk;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v0 = fmaxf(__builtin_fmaf(x[2 * j], ta[2 * j], tb[2 * j]), 0.0f);
                const float v1 = fmaxf(__builtin_fmaf(x[2 * j + 1], ta[2 * j + 1], tb[2 * j + 1]), 0.0f);
                pk[j] = v3b::bf16_bits(v0) | (v3b::bf16_bits(v1) << 16);
            }
            *reinterpret_cast<u32x4*>(xb + img_off(p, c8, leaf)) = pk;
        }
    }
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int jl = lane & 15, q4 = lane >> 4, jj = l0 + jl;
    const bf16x8* wf = reinterpret_cast<const bf16x8*>(a.wf) + lane;
    const unsigned lane_b = (unsigned)(q4 * 32 + jj) * 16u;
    const vq_buf outb = buf_of((const f32x4*)a.out + (size_t)tile * (64 * 16 * 32));
    const vq_buf skb = buf_of(RESID ? (const f32x4*)a.skip + (size_t)tile * (64 * 16 * 32) : (const f32x4*)a.out);
    f32x4 bq[4];   // this lane's bias quads: output channels 16 mt + 4 q4 ..
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) bq[mt] = ((const f32x4*)a.bias)[4 * mt + q4];

    for (int rr = 0; rr < 2; ++rr) {
        const int row = wave + 8 * rr, od = row >> 2, oh = row & 3;   // (wave-uniform)
        f32x4 acc[4][4];
#pragma unroll
        for (int ow = 0; ow < 4; ++ow)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[ow][mt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        for (int kd = 0; kd < 3; ++kd) {
            const int id = od + kd - 1;
            if (id < 0 || id > 3) continue;
            for (int kh = 0; kh < 3; ++kh) {
                const int ih = oh + kh - 1;
                if (ih < 0 || ih > 3) continue;
                const int prow = (id * 4 + ih) * 4;
                bf16x8 b[4][2];   // the input row: position iw, channel block kb
#pragma unroll
                for (int iw = 0; iw < 4; ++iw)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) b[iw][kb] = *reinterpret_cast<const bf16x8*>(xb + img_off(prow + iw, 4 * kb + q4, jl));
                const bf16x8* wt = wf + (size_t)((kd * 3 + kh) * 3) * (2 * 4 * 64);
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) {
                        bf16x8 av[4];
#pragma unroll
                        for (int mt = 0; mt < 4; ++mt) av[mt] = wt[((kw * 2 + kb) * 4 + mt) * 64];
#pragma unroll
                        for (int ow = 0; ow < 4; ++ow) {
                            const int iw = ow + kw - 1;
                            if (iw < 0 || iw > 3) continue;   // (compile time: the padding taps along w)
#pragma unroll
                            for (int mt = 0; mt < 4; ++mt) acc[ow][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[mt], b[iw][kb], acc[ow][mt], 0, 0, 0);
                        }
                    }
            }
        }
        // ---- epilogue: the 4 positions of the row ascending; the row is one statistics block ----
        GnAcc st[4];
        f32x4 csb[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) st[mt].init(), csb[mt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ow = 0; ow < 4; ++ow) {
            const unsigned pos_b = (unsigned)(row * 4 + ow) * 8192u;
            f32x4 sk[4];
            if (RESID) {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) sk[mt] = buf_ld16(skb, lane_b + mt * 2048, pos_b);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                f32x4 v = acc[ow][mt] + bq[mt];
                if (RESID) {
                    const f32x4 u = v * 0.1f;
                    v = sk[mt] + u;
                }
                buf_st16_nt(v, outb, lane_b + mt * 2048, pos_b);
                if (RESID) {
                    csb[mt] = csb[mt] + v;
                } else {
                    st[mt].add(v.x);
                    st[mt].add(v.y);
                    st[mt].add(v.z);
                    st[mt].add(v.w);
                }
            }
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            if (RESID) {
                const float v4[4] = {csb[mt].x, csb[mt].y, csb[mt].z, csb[mt].w};
#pragma unroll
                for (int r = 0; r < 4; ++r) a.part_c[(((size_t)tile * 16 + row) * 64 + 16 * mt + 4 * q4 + r) * 32 + jj] = v4[r];
            } else {
                const size_t i = part_index(tile, row, 4 * mt + q4, jj);
                a.part_s[i] = st[mt].bs, a.part_q[i] = st[mt].bq;
            }
        }
    }
}

// bf16 A fragments of one conv from the fp32 16x16x4 fragments of conv_rows16_k (w16[((tap*4 + cb)*4 + mt)*64 + lane][i] =
// W[16 mt + (lane&15)][16 cb + 4 (lane>>4) + i][tap]), on the device: one thread per lane fragment of 8.  Element j of lane l of
// fragment (tap, kb, mt) is W[16 mt + (l&15)][32 kb + 8 (l>>4) + j][tap].  grid = 54 x 256 threads.
__global__ __launch_bounds__(256) void frag_k(const float* __restrict__ w16, uint16_t* __restrict__ dst)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= FRAG_ELEMS / 8) return;
    const int lane = i & 63, mt = (i >> 6) & 3, kb = (i >> 8) & 1, tap = i >> 9;
    u32x4 pk;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = 32 * kb + 8 * (lane >> 4) + j;
        const float v = w16[((((size_t)tap * 4 + ci / 16) * 4 + mt) * 64 + ((ci & 15) >> 2) * 16 + (lane & 15)) * 4 + (ci & 3)];
        const uint32_t h = v3b::bf16_bits(v);
        if (j & 1) pk[j >> 1] |= h << 16;
        else pk[j >> 1] = h;
    }
    reinterpret_cast<u32x4*>(dst)[i] = pk;
}

}  // namespace d64b
