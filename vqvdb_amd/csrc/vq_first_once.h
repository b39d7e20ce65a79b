// vq_first_once.h — Conv3d(1->16,k3,p1) @8^3 + GroupNorm(4,16) + ReLU (VQVAE_v2.py:235-237) with the conv issued ONCE.
//
// conv_first_k / conv_first_roll_k run the conv twice (statistics pass, then recompute + normalise + store) because GroupNorm needs the
// whole leaf's statistics before any element can be normalised and a 16-leaf MFMA tile's share of y1 = conv(x) + b does not fit on chip.
// Here the 16 columns of the 16x16x4 MFMA are 8 LEAVES x 2 POSITIONS, so a workgroup of 8 waves keeps the y1 of an 8-leaf group (a
// quarter of a 32-leaf tile, 65 536 floats) in its accumulators: 8 waves x 64 lanes x 128 registers.
//
//   wave w            output plane od = w (kd = 0 does not exist at od = 0, kd = 2 not at od = 7: wave-uniform skips)
//   column n = lane&15   leaf j8 = n & 7 of the group, s = n >> 3: the s = 0 lanes compute output rows oh = 0..3, the s = 1 lanes oh + 4
//   rows / K          the 16 couts / K slot q4 = lane >> 4 = kw, slot 3 = pad — conv_first_k's, with its w[9] A values per lane
//   accumulators      acc[rp 0..3][ow 0..7]: output row rp + 4s, one chain per output element
//   B operands        for (kd, kh): the 8 floats from element kw of record (plane od+kd-1, row rp+4s+kh-1, leaf) of xr, two 16-byte
//                     loads; the row differs per lane through s, so it sits in the per-lane offset
//
// Per input plane a lane meets six rows, t = rp + kh = 0..5 (row t-1+4s).  Row -1 (t = 0, s = 0) and row 8 (t = 5, s = 1) lie outside
// the leaf: those lanes carry an out-of-range lane offset, which the buffer load answers with zeros like the pad slot's, while the other
// half of the columns reads real data.  The MFMA is issued, not skipped.  The six rows sit in a register ring (slot = t); a slot is
// re-requested for the NEXT plane (after kd = 2: for plane kd = 0 of the workgroup's next group) right after its last MFMA, so every
// load is one plane of MFMAs ahead (the next group's first plane is under way before the current group's barriers, so its stores drain
// beside the next group's MFMAs), the loop is entered with nothing in flight and no load sits inside a branch.
// The steps walk t outermost: an accumulator (rp, ow) sees kh = t - rp ascending inside kd ascending.
//
// Bits.  Every output element sees the same MFMAs with the same A row and B column values as in conv_first_k, in the same order:
// (kd, kh) ascending, K = {kw0, kw1, kw2, pad}, then + bias.  One difference: a (kd, kh) step that conv_first_k skips for a border row
// is issued here with an all-zero B column.  That adds exact zeros to an accumulator that is never -0 — a chain starts at +0 (the first
// MFMA's C operand is the literal 0), a sum that cancels exactly rounds to +0, and the pad slot's fmaf(0, 0, acc) closes every MFMA —
// so the result has the same bits.
//
// Statistics.  The contract's 16 blocks of 32 positions (GnAcc) are the half planes: block 2 od + s is what the s half of
// wave od's lanes holds.  A lane runs the block's fp64 chain locally (positions ascending, channels ascending, from zero); the block
// sums of (leaf, group) meet in LDS (8 KB for y1's GroupNorm(4,16), group = q4; 16 KB for a1's GroupNorm(8,16), groups (x,y), (z,w))
// and after a workgroup barrier are added in block order 0..15 starting from 0.0, which is what fold() does in sequence, then gn_finish.
// Two barriers per group, reached by every wave the same number of times: the group loop's trip count is the workgroup's, no wave
// leaves it early, whole tiles (padding leaves included) are processed; a workgroup without a group returns before its first barrier.
//
// Work: a persistent workgroup per CU walks groups blockIdx.x + k gridDim.x.  MFMA work per SIMD (waves w, w + 4) in units of 96 MFMAs:
// 5 / 6 / 6 / 5 — the two border planes sit on SIMDs 0 and 3, which idle a sixth of the MFMA phase; an od-per-wave split cannot do
// better.  The two light waves finish a1's statistics (one group half each).  264 MFMAs per leaf instead of 2 x 242.
#pragma once
#include "vq_conv8_lds.h"   // lds_barrier

__global__ __launch_bounds__(512, 1) void conv_first_once_k(ConvArgs A, float* __restrict__ y1_out, float* __restrict__ y1_mean, float* __restrict__ y1_rstd)
{
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    __shared__ f64x2 sh_y[16 * 4 * 8];   // [block][group of 4 couts][leaf]: (sum, sum of squares) of y1
    __shared__ f64x2 sh_a[16 * 8 * 8];   // [block][group of 2 couts][leaf]: ... of a1
    __shared__ f32x4 sh_gb[8];           // GroupNorm(4,16) gamma [q4], beta [4 + q4]: eight registers less across the MFMA phase
    const int lane = threadIdx.x & 63;
    const int od = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_groups = 4 * A.n_tiles;
    if ((int)blockIdx.x >= n_groups) return;   // (the whole workgroup, before any barrier)
    const int j8 = lane & 7, s = (lane >> 3) & 1, q4 = lane >> 4;
    float w[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) w[t] = A.wfrag[t * 64 + lane];
    const f32x4 bias4 = ((const f32x4*)A.bias_frag)[q4];
    if (threadIdx.x < 16) sh_gb[threadIdx.x >> 2][threadIdx.x & 3] = A.in_gamma[threadIdx.x], sh_gb[4 + (threadIdx.x >> 2)][threadIdx.x & 3] = A.in_beta[threadIdx.x];   // (read behind the first barrier)
    // per-lane byte offsets into a tile of xr: record of leaf j8 from element kw; the s = 1 lanes four rows further.  Rows t = 0 / t = 5
    // are addressed from row 0 / row 4 of the plane, the half that would leave the leaf (and the pad slot always) out of range: zeros
    constexpr unsigned OOB = 0x80000000u, ROWB = 32 * VQ_XR_REC * 4;
    const unsigned rec = (unsigned)(j8 * VQ_XR_REC + q4) * 4u;
    const unsigned lane_mid = q4 < 3 ? rec + (unsigned)s * 4u * ROWB : OOB;
    const unsigned lane_t0 = (q4 < 3 && s == 1) ? rec + 3u * ROWB : OOB;
    const unsigned lane_t5 = (q4 < 3 && s == 0) ? rec : OOB;
    auto ldrow = [&](vq_buf b, int plane, int qt, int t, int hf) __attribute__((always_inline)) -> f32x4 {
        const int rowu = t == 0 ? 0 : (t == 5 ? 4 : t - 1);
        return buf_ld16(b, t == 0 ? lane_t0 : (t == 5 ? lane_t5 : lane_mid), (unsigned)(((plane * 8 + rowu) * 32 + 8 * qt) * VQ_XR_REC + hf * 4) * 4u);
    };
    const unsigned lane_o = (unsigned)s * 65536u + (unsigned)(q4 * 32 + j8) * 16u;   // a1 / y1: position (rp + 4 s, .), channel quad q4, leaf j8

    int G = (int)blockIdx.x;
    f32x4 ring[6][2];   // [t][half row]
    {
        const vq_buf xb = buf_of(A.in + (size_t)(G >> 2) * VQ_XR_TILE);
        const int pc = max(od - 1, 0);
#pragma unroll
        for (int t = 0; t < 6; ++t) ring[t][0] = ldrow(xb, pc, G & 3, t, 0), ring[t][1] = ldrow(xb, pc, G & 3, t, 1);
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);   // enter the loop with nothing in flight
    for (; G < n_groups; G += (int)gridDim.x) {
        const int tile = G >> 2, qt = G & 3;
        const int Gn = G + (int)gridDim.x < n_groups ? G + (int)gridDim.x : G;   // (last group: its own rows again, nobody reads them)
        const vq_buf xbc = buf_of(A.in + (size_t)tile * VQ_XR_TILE), xbn = buf_of(A.in + (size_t)(Gn >> 2) * VQ_XR_TILE);
        f32x4 acc[4][8];
        // the MFMAs of row t of input plane od + kd - 1; first: this kd opens the chains (C = literal 0 at kh = 0)
        auto mfma_row = [&](int kd, int t, bool first) __attribute__((always_inline)) {
            const f32x4 x0 = ring[t][0], x1 = ring[t][1];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int rp = t - kh;
                if (rp < 0 || rp > 3) continue;
                const float wv = w[kd * 3 + kh];
#pragma unroll
                for (int ow = 0; ow < 8; ++ow)
                    acc[rp][ow] = mfma16(wv, ow < 4 ? x0[ow & 3] : x1[ow & 3], (first && kh == 0) ? (f32x4){0, 0, 0, 0} : acc[rp][ow]);
            }
        };
#pragma unroll
        for (int kd = 0; kd < 3; ++kd) {
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                if (kd == 0) {   // (plane 0 has no kd = 0: its chains open as zeros — 128 moves on the wave with the least MFMA work)
                    if (od > 0) mfma_row(0, t, true);
                    else if (t < 4) {
#pragma unroll
                        for (int ow = 0; ow < 8; ++ow) acc[t][ow] = (f32x4){0, 0, 0, 0};
                    }
                } else if (kd == 1 || od < 7) mfma_row(kd, t, false);
                // the slot's row of the next plane (unconditional, clamped where the plane does not exist)
                __builtin_amdgcn_sched_barrier(0);
                if (kd < 2) ring[t][0] = ldrow(xbc, min(od + kd, 7), qt, t, 0), ring[t][1] = ldrow(xbc, min(od + kd, 7), qt, t, 1);
                else ring[t][0] = ldrow(xbn, max(od - 1, 0), Gn & 3, t, 0), ring[t][1] = ldrow(xbn, max(od - 1, 0), Gn & 3, t, 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // y1 = conv + bias stays in the accumulators; its block chain
        GnAcc sy;
        sy.init();
#pragma unroll
        for (int rp = 0; rp < 4; ++rp)
#pragma unroll
            for (int ow = 0; ow < 8; ++ow) {
                const f32x4 v = acc[rp][ow] + bias4;
                acc[rp][ow] = v;
                sy.add(v.x);
                sy.add(v.y);
                sy.add(v.z);
                sy.add(v.w);
                __builtin_amdgcn_sched_barrier(0);   // element by element: the chain is serial, and hoisting the other elements' work costs registers
            }
        sh_y[((2 * od + s) * 4 + q4) * 8 + j8] = (f64x2){sy.bs, sy.bq};
        if (y1_out) {   // debug / keep_y1 only
            const vq_buf yb = buf_of((const f32x4*)y1_out + (size_t)tile * 512 * 4 * 32);
#pragma unroll
            for (int rp = 0; rp < 4; ++rp)
#pragma unroll
                for (int ow = 0; ow < 8; ++ow) buf_st16(acc[rp][ow], yb, lane_o, (unsigned)(((od * 8 + rp) * 8 + ow) * 128 + 8 * qt) * 16u);
        }
        lds_barrier();
        f32x4 ia, ib;
        {
            double S = 0.0, Q = 0.0;
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const f64x2 p = sh_y[(b * 4 + q4) * 8 + j8];
                S += p.x;
                Q += p.y;
            }
            float mean, rstd;
            gn_finish(S, Q, 1.0 / 2048.0, mean, rstd);
            if (od == 0 && s == 0) {   // (buffer stores: a per-lane 64-bit address would have to live across the whole group)
                buf_st4(mean, buf_of(y1_mean + (size_t)tile * 4 * 32), (unsigned)(q4 * 32 + j8) * 4u, (unsigned)(8 * qt) * 4u);
                buf_st4(rstd, buf_of(y1_rstd + (size_t)tile * 4 * 32), (unsigned)(q4 * 32 + j8) * 4u, (unsigned)(8 * qt) * 4u);
            }
            const f32x4 gam = sh_gb[q4], bet = sh_gb[4 + q4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ia[i] = rstd * gam[i];
                ib[i] = __builtin_fmaf(-mean, ia[i], bet[i]);
            }
        }
        // a1 = relu(gn(y1)) -> streaming store (see conv_first_k), its block chains
        const vq_buf outb = buf_of((const f32x4*)A.out + (size_t)tile * 512 * 4 * 32);
        GnAcc sa[2];
        sa[0].init(), sa[1].init();
#pragma unroll
        for (int rp = 0; rp < 4; ++rp)
#pragma unroll
            for (int ow = 0; ow < 8; ++ow) {
                const f32x4 v = gn_relu4(acc[rp][ow], ia, ib);
                buf_st16_nt(v, outb, lane_o, (unsigned)(((od * 8 + rp) * 8 + ow) * 128 + 8 * qt) * 16u);
                sa[0].add(v.x);
                sa[0].add(v.y);
                sa[1].add(v.z);
                sa[1].add(v.w);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
        for (int k = 0; k < 2; ++k) sh_a[((2 * od + s) * 8 + 2 * q4 + k) * 8 + j8] = (f64x2){sa[k].bs, sa[k].bq};
        lds_barrier();
        if (od == 0 || od == 7) {   // (wave-uniform) the two light waves finish one group half each
            const int k = od == 0 ? 0 : 1;
            double S = 0.0, Q = 0.0;
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const f64x2 p = sh_a[(b * 8 + 2 * q4 + k) * 8 + j8];
                S += p.x;
                Q += p.y;
            }
            float mean, rstd;
            gn_finish(S, Q, 1.0 / 1024.0, mean, rstd);
            if (s == 0) {
                buf_st4(mean, buf_of(A.out_mean + (size_t)tile * 8 * 32), (unsigned)(2 * q4 * 32 + j8) * 4u, (unsigned)(k * 32 + 8 * qt) * 4u);
                buf_st4(rstd, buf_of(A.out_rstd + (size_t)tile * 8 * 32), (unsigned)(2 * q4 * 32 + j8) * 4u, (unsigned)(k * 32 + 8 * qt) * 4u);
            }
        }
    }
}
