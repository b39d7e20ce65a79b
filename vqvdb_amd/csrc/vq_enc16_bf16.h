// vq_enc16_bf16.h — the encoder's two 16 -> 16 convs at 8^3 (ResidualBlock(16), encoder.pre.3.conv1 / .conv2) with bf16 matrix
// operands: the opt-in encode mode vqhip_set_encode_mode(VQHIP_PRECISION_BF16), DESIGN.md §24.  Everything else of the encoder
// keeps its fp32 kernels, and every tensor in global memory stays fp32 in the leaf-tile layout act[tile][pos 512][4 quads][32][4].
//
// Arithmetic: both operands of every product are bf16 (round to nearest even, v3b::bf16_bits): the weight when its fragments are
// packed (frag_k), the activation when the LDS image is filled, after GroupNorm(8,16) + ReLU has been evaluated in fp32 with the
// fp32 path's formula, max(fmaf(x, rstd*gamma, fmaf(-mean, rstd*gamma, beta)), 0).  v_mfma_f32_16x16x32_bf16 accumulates the
// (exact) products in fp32.  K = 32 is TWO TAPS x 16 channels: MFMA m = 0 .. 13 takes taps 2m (lanes 0-31) and 2m+1 (lanes 32-63)
// of the ascending (kd,kh,kw) list; tap 27 does not exist and has zero weights.  A padding tap meets a constructed +0 activation
// (a 16-byte zero slot in LDS); an MFMA whose two taps both lie outside the volume along d is skipped.  Per output the MFMAs come
// in ascending m from a zero accumulator; acc + bias at the end; conv2 stores skip + 0.1 (acc + bias) with two roundings.
//
// Shape: one persistent workgroup of 8 waves walks 8-LEAF groups (4 per tile).  The group's whole input (512 positions x 16
// channels x 8 leaves) is transformed once and sits in LDS as bf16, 128 KiB.  GEMM: M = 16 output channels, N = 16 columns = 8
// leaves x the 2 positions (od, oh, ow) and (od, oh, ow + 4), K as above.  Wave w owns output row oh = w of every plane: per plane
// 4 accumulators (ow = 0 .. 3), 14 MFMAs each, the 14 A fragments (56 VGPRs) held in registers for the whole kernel, so the only
// LDS traffic of the GEMM is one ds_read_b128 per lane and MFMA.  The image is [d][h][w & 3][8-channel chunk][w >> 2][leaf][8 bf16]:
// the 16 lanes of a ds_read_b128 group cover one 256-byte bank row (conflict-free), and so do 16 consecutive lanes of the fill's
// ds_write_b128.  A lane's byte offsets relative to its row (tap, h / w validity, chunk, leaf) never change and are tabulated once.
//
// Statistics (conv1, for gn2): a lane's four positions ow .. of a plane ARE one half row (oh, hw = ow >> 2) of §4's rule: one fp64
// chain from zero over 4 positions x the group's 2 channels, folded into t_(oh,hw) over the planes od ascending, and the sixteen t
// go to the 16 blocks of the partial buffers; gn_combine_k<false> adds them in (oh, hw) order — what conv8_lds_k does.
#pragma once

#include "vq_bf16.h"
#include "vq_kernels.h"

namespace e16b {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct Args {
    const float* in;        // [tile][512][4][32][4]
    float* out;             // the same layout
    const uint16_t* wf;     // bf16 A fragments [14 tap pairs][64 lanes][8]
    const float* bias;      // plain [16]
    const float* skip;      // conv2: the residual input, layout of out
    const float* in_mean;   // [tile][8][32]
    const float* in_rstd;
    const float* in_gamma;  // [16]
    const float* in_beta;
    double* part_s;         // conv1: [tile][16 half rows (oh, hw)][16 slots, 8 used][32]
    double* part_q;
    int n_groups;           // 4 * tiles
};

constexpr int THREADS = 512;
constexpr int NPAIR = 14;                           // MFMAs per output: 27 taps + 1 pad, two per MFMA
constexpr int FRAG_ELEMS = NPAIR * 64 * 8;          // bf16 elements of one conv's fragments (14 336 B)
constexpr int IMG_BYTES = 512 * 2 * 8 * 16;         // 128 KiB: the 8-leaf group's input as bf16
constexpr int ZERO_OFF = IMG_BYTES;                 // 16 bytes of +0: the operand of a padding tap
constexpr size_t LDS_BYTES = IMG_BYTES + 256;
constexpr int INVALID = 1 << 30;                    // table entry of a tap that is padding for this lane whatever the plane
static_assert(LDS_BYTES <= 160 * 1024, "gfx950: 160 KB of LDS per workgroup");
static_assert(ZERO_OFF + 16 <= (int)LDS_BYTES, "the zero slot lies inside the allocation");

// byte offset of the 8 channels 8 c8 .. 8 c8 + 7 of (input row = d * 8 + h, w, leaf of the group) in the LDS image
__device__ __forceinline__ int img_off(int row, int w, int c8, int leaf) { return (row * 4 + (w & 3)) * 512 + c8 * 256 + (w >> 2) * 128 + leaf * 16; }

// RESID false: conv1 (GroupNorm half-row totals of its output); true: conv2 (skip + 0.1 y).  grid = min(4 * n_tiles, CUs).
template <bool RESID>
__global__ __launch_bounds__(THREADS, 1) void conv_k(Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char xb[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int oh = __builtin_amdgcn_readfirstlane(tid >> 6);   // this wave's output row of every plane
    const int q4 = lane >> 4, leaf = lane & 7, ps = (lane >> 3) & 1, c8 = q4 & 1, half = q4 >> 1;
    if (tid < 4) reinterpret_cast<uint32_t*>(xb + ZERO_OFF)[tid] = 0u;

    bf16x8 af[NPAIR];
#pragma unroll
    for (int m = 0; m < NPAIR; ++m) af[m] = reinterpret_cast<const bf16x8*>(a.wf)[m * 64 + lane];
    const f32x4 bias4 = ((const f32x4*)a.bias)[q4];

    // off[m][ow]: where this lane's B fragment of MFMA m for output (od, oh, ow + 4 ps) lies, relative to input row (od, oh) of the
    // image; INVALID where the lane's tap is padding along h or w (or is tap 27).  Padding along d depends on the plane: below.
    int off[NPAIR][4];
#pragma unroll
    for (int m = 0; m < NPAIR; ++m) {
        const int tap = 2 * m + half, kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
        const int ih = oh + kh - 1;
#pragma unroll
        for (int ow = 0; ow < 4; ++ow) {
            const int iw = ow + 4 * ps + kw - 1;
            const bool ok = tap < 27 && ih >= 0 && ih <= 7 && iw >= 0 && iw <= 7;
            off[m][ow] = ok ? ((kd - 1) * 8 + (kh - 1)) * 2048 + img_off(0, iw, c8, leaf) : INVALID;
        }
    }

#pragma unroll 1
    for (int g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
        const int tile = g >> 2, l0 = 8 * (g & 3);   // first leaf of the group inside its tile
        __syncthreads();                              // every wave has finished reading the previous group's image
        // ---- fill: one item = 8 channels (four GroupNorm groups) of one position of one leaf; fp32 transform, then bf16 ----
        {
            const int fl = tid & 7, wh = (tid >> 3) & 1, fc = (tid >> 4) & 1, wl = (tid >> 5) & 3, r0 = tid >> 7;
            const int jj = l0 + fl;
            float ta[8], tb[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float mean = a.in_mean[((size_t)tile * 8 + 4 * fc + k) * 32 + jj], rstd = a.in_rstd[((size_t)tile * 8 + 4 * fc + k) * 32 + jj];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int j = 2 * k + i;
                    ta[j] = rstd * a.in_gamma[8 * fc + j];
                    tb[j] = __builtin_fmaf(-mean, ta[j], a.in_beta[8 * fc + j]);
                }
            }
            const f32x4* src = (const f32x4*)a.in + (size_t)tile * (512 * 4 * 32) + (2 * fc) * 32 + jj;
            const int w = wl + 4 * wh;
#pragma unroll 8
            for (int it = 0; it < 16; ++it) {
                const int row = r0 + 4 * it, p = row * 8 + w;
                const f32x4 lo = src[p * 128], hi = src[p * 128 + 32];
                const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                u32x4 pk;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v0 = fmaxf(__builtin_fmaf(x[2 * j], ta[2 * j], tb[2 * j]), 0.0f);
                    const float v1 = fmaxf(__builtin_fmaf(x[2 * j + 1], ta[2 * j + 1], tb[2 * j + 1]), 0.0f);
                    pk[j] = v3b::bf16_bits(v0) | (v3b::bf16_bits(v1) << 16);
                }
                *reinterpret_cast<u32x4*>(xb + img_off(row, w, fc, fl)) = pk;
            }
        }
        __syncthreads();

        const int jj = l0 + leaf;
        const unsigned lane_b = (unsigned)(q4 * 32 + jj) * 16u + (unsigned)ps * (4u * 2048u);
        const vq_buf outb = buf_of((const f32x4*)a.out + (size_t)tile * (512 * 4 * 32));
        const vq_buf skb = buf_of(RESID ? (const f32x4*)a.skip + (size_t)tile * (512 * 4 * 32) : (const f32x4*)a.out);
        GnAcc st[2];   // GroupNorm(8,16) groups 2 q4 and 2 q4 + 1 of this lane's half row (oh, ps), over the planes
        st[0].init(), st[1].init();

#pragma unroll 1
        for (int od = 0; od < 8; ++od) {
            const int rowb = (od * 8 + oh) * 2048;                // input row (od, oh) of the image
            const unsigned pos_b = (unsigned)((od * 8 + oh) * 8) * 2048u;
            const int kd_out = od == 0 ? 0 : od == 7 ? 2 : -1;    // the kd whose plane lies outside the volume (wave-uniform)
            f32x4 sk[4];
            if (RESID) {
#pragma unroll
                for (int ow = 0; ow < 4; ++ow) sk[ow] = buf_ld16(skb, lane_b, pos_b + (unsigned)ow * 2048u);
            }
            f32x4 acc[4];
#pragma unroll
            for (int ow = 0; ow < 4; ++ow) acc[ow] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int m = 0; m < NPAIR; ++m) {
                const int kd_lo = (2 * m) / 9, kd_hi = (2 * m + 1) / 9;   // (compile time) kd of the two taps; tap 27 counts as kd 3
                if (kd_lo == kd_hi && kd_lo == kd_out) continue;          // (wave-uniform) both taps are padding for every column
                bf16x8 b[4];
#pragma unroll
                for (int ow = 0; ow < 4; ++ow) {
                    // One unsigned min sends every padding tap to the zero slot: an INVALID entry lands beyond the image whatever
                    // the row; a tap whose plane lies before the volume (od = 0, kd = 0) gives a negative offset, a huge unsigned
                    // one; a tap whose plane lies behind it (od = 7, kd = 2) gives row 64 or more, at or beyond IMG_BYTES.
                    const unsigned ad = min((unsigned)(rowb + off[m][ow]), (unsigned)ZERO_OFF);
                    b[ow] = *reinterpret_cast<const bf16x8*>(xb + ad);
                }
#pragma unroll
                for (int ow = 0; ow < 4; ++ow) acc[ow] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m], b[ow], acc[ow], 0, 0, 0);
            }
            // ---- epilogue: the lane's 4 positions of the plane ascending: one half row ----
#pragma unroll
            for (int ow = 0; ow < 4; ++ow) {
                f32x4 v = acc[ow] + bias4;
                if (RESID) {
                    const f32x4 u = v * 0.1f;
                    v = sk[ow] + u;
                }
                buf_st16_nt(v, outb, lane_b, pos_b + (unsigned)ow * 2048u);
                if (!RESID) {
                    st[0].add(v.x);
                    st[0].add(v.y);
                    st[1].add(v.z);
                    st[1].add(v.w);
                }
            }
            if (!RESID) st[0].fold(), st[1].fold();
        }
        if (!RESID) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const size_t i = part_index(tile, 2 * oh + ps, 2 * q4 + k, jj);
                a.part_s[i] = st[k].s, a.part_q[i] = st[k].q;
            }
        }
    }
}

// bf16 A fragments of one conv from the fp32 16x16x4 fragments of conv8_lds_k (w[(tap * 64 + lane) * 4 + i] =
// W[lane & 15][4 (lane >> 4) + i][tap]), on the device: one thread per lane fragment of 8.  Element j of lane l of MFMA m is
// W[l & 15][8 ((l >> 4) & 1) + j][tap 2 m + (l >> 5)], and +0 for tap 27.  grid = 4 x 256 threads.
__global__ __launch_bounds__(256) void frag_k(const float* __restrict__ w, uint16_t* __restrict__ dst)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= FRAG_ELEMS / 8) return;
    const int lane = i & 63, m = i >> 6, tap = 2 * m + (lane >> 5);
    u32x4 pk;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = 8 * ((lane >> 4) & 1) + j;
        const uint32_t h = tap < 27 ? v3b::bf16_bits(w[((size_t)tap * 64 + (ci >> 2) * 16 + (lane & 15)) * 4 + (ci & 3)]) : 0u;
        if (j & 1) pk[j >> 1] |= h << 16;
        else pk[j >> 1] = h;
    }
    reinterpret_cast<u32x4*>(dst)[i] = pk;
}

}  // namespace e16b
