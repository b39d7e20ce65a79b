// vq_vec3.h — kernels of the Vec3 model (VQVAE(3, 64, K): EncoderVec3 / DecoderVec3).
//
// Layout: one leaf's activation is [C][S^3] fp32 (NCDHW per leaf, position d*S*S + h*S + w), leaves back to back.
// The leaf is the unit of every launch: a workgroup holds whole leaves in LDS, so no arithmetic mixes leaves and the
// accumulation order of every output depends only on its own leaf (bit-identical results for any batch or chunk size).
//
// Convolutions are implicit GEMMs on v_mfma_f32_32x32x2_f32: M = output channels (32-channel tiles), N = output positions
// of one leaf (32-position tiles), K = taps x input channels, walked tap-major, input-channel pairs minor.  The input leaf
// sits in LDS; a lane reads its B element at the tap-shifted position (zero outside the leaf), its A element from the
// weight fragments prepacked at create ([ctile][tap][cin/2][lane]).  A tap that is outside the leaf for every lane of a
// wave is skipped (its products are all zero).  The MFMA is an exact fp32 fmaf chain in K order (vqhip_selftest_mfma).
#pragma once

#include "vq_device.h"

namespace v3 {

constexpr int IN_PLAIN = 0;    // act[leaf][CIN][SI^3]
constexpr int IN_LEAF3 = 1;    // channels-last leaves [leaf][512][3], channel 3 zero (CIN = 4)
constexpr int IN_GNRELU = 2;   // relu(GroupNorm(8)(act)) from per-leaf statistics [leaf][8][mean, rstd]
constexpr int IN_GATE = 3;     // act * gate[leaf][CIN] (ChannelAttention)

constexpr int OUT_BIAS = 0;    // acc + bias
constexpr int OUT_RESID = 1;   // res + 0.1 * (acc + bias)   (ResidualBlock: residual + scale * conv2(...))

struct ConvArgs {
    const float* in;
    const float* stats;   // IN_GNRELU
    const float* gamma;   // IN_GNRELU
    const float* beta;    // IN_GNRELU
    const float* gate;    // IN_GATE
    const float* wf;      // fragments [COUT/32][KS^3][CIN/2][64]
    const float* bias;    // [COUT]
    const float* res;     // OUT_RESID (may alias out: each element is read, then written, by the same lane)
    float* out;           // [leaf][COUT][SO^3]
    int64_t n;
};

template <int CIN, int COUT, int SO, int MT, int NT>
struct ConvShape {
    static constexpr int NPO = SO * SO * SO;
    static constexpr int MG = COUT / 32 / MT;   // cout groups per leaf
    static constexpr int NG = NPO / 32 / NT;    // position groups per leaf
    static constexpr int WPL = MG * NG;         // waves per leaf
    static_assert(COUT % (32 * MT) == 0 && NPO % (32 * NT) == 0 && CIN % 2 == 0, "tile shape");
};

constexpr int conv_threads(int cout, int so, int lpb, int mt, int nt) { return lpb * (cout / 32 / mt) * (so * so * so / 32 / nt) * 64; }

template <int CIN, int COUT, int SI, int SO, int KS, int STRIDE, int PAD, int LPB, int MT, int NT, int INMODE, int OUTMODE>
__global__ void __launch_bounds__(conv_threads(COUT, SO, LPB, MT, NT))
conv_k(ConvArgs a)
{
    using S = ConvShape<CIN, COUT, SO, MT, NT>;
    constexpr int NPI = SI * SI * SI, NPO = S::NPO, KT = KS * KS * KS, CP = CIN / 2;
    extern __shared__ float xs[];   // [LPB][CIN][NPI]
    const int tid = threadIdx.x;
    const int64_t leaf0 = (int64_t)blockIdx.x * LPB;

    // ---- fill: LPB input leaves into LDS, transformed by INMODE ----
    for (int i = tid; i < LPB * CIN * NPI; i += blockDim.x) {
        const int l = i / (CIN * NPI), e = i % (CIN * NPI), c = e / NPI;
        const int64_t leaf = leaf0 + l;
        float v = 0.0f;
        if (leaf < a.n) {
            if constexpr (INMODE == IN_LEAF3) {
                const int p = e % NPI;
                v = c < 3 ? a.in[leaf * 1536 + p * 3 + c] : 0.0f;
            } else {
                v = a.in[leaf * (CIN * NPI) + e];
                if constexpr (INMODE == IN_GNRELU) {
                    const int g = c / (CIN / 8);
                    const float mean = a.stats[leaf * 16 + 2 * g], rstd = a.stats[leaf * 16 + 2 * g + 1];
                    v = (v - mean) * rstd;
                    v = v * a.gamma[c] + a.beta[c];
                    v = v > 0.0f ? v : 0.0f;
                } else if constexpr (INMODE == IN_GATE) {
                    v = v * a.gate[leaf * CIN + c];
                }
            }
        }
        xs[i] = v;
    }
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int l = wave / S::WPL, wl = wave % S::WPL;
    const int64_t leaf = leaf0 + l;
    if (leaf >= a.n) return;
    const int ct0 = (wl % S::MG) * MT, pt0 = (wl / S::MG) * NT;
    const int n = lane & 31, kh = lane >> 5;
    const float* x = xs + l * (CIN * NPI) + kh * NPI;

    int od[NT], oh[NT], ow[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int p = (pt0 + j) * 32 + n;
        od[j] = p / (SO * SO), oh[j] = (p / SO) % SO, ow[j] = p % SO;
    }
    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    for (int tap = 0; tap < KT; ++tap) {
        const int kd = tap / (KS * KS), khh = (tap / KS) % KS, kw = tap % KS;
        int off[NT];
        bool any = false;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int id = od[j] * STRIDE - PAD + kd, ih = oh[j] * STRIDE - PAD + khh, iw = ow[j] * STRIDE - PAD + kw;
            const bool ok = id >= 0 && id < SI && ih >= 0 && ih < SI && iw >= 0 && iw < SI;
            off[j] = ok ? (id * SI + ih) * SI + iw : -1;
            any |= ok;
        }
        if (__ballot(any) == 0) continue;   // wave-uniform: every product of this tap is zero
        const float* w = a.wf + ((size_t)ct0 * KT + tap) * CP * 64 + lane;
#pragma unroll 8
        for (int cp = 0; cp < CP; ++cp) {
            float b[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) b[j] = off[j] >= 0 ? x[cp * 2 * NPI + off[j]] : 0.0f;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const float av = w[((size_t)i * KT * CP + cp) * 64];
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = mfma32(av, b[j], acc[i][j]);
            }
        }
    }

    // ---- store: reg r of lane -> cout row (r&3) + 8(r>>2) + 4kh, position column n ----
    float* out = a.out + leaf * (COUT * NPO);
    const float* res = a.res + leaf * (COUT * NPO);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = (ct0 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh, p = (pt0 + j) * 32 + n;
                float v = acc[i][j][r] + a.bias[co];
                if constexpr (OUTMODE == OUT_RESID) v = res[co * NPO + p] + 0.1f * v;
                out[co * NPO + p] = v;
            }
}

// GroupNorm(8, C) statistics of one leaf per workgroup (256 threads: 32 lanes per group).  A group is a contiguous range of
// C/8 * NP floats; lane j sums elements j, j+32, ... in order, then a fixed xor-butterfly over the 32 lanes.  Two passes
// (mean, then the mean of squared deviations, biased), eps 1e-5 as nn.GroupNorm.  Out: [leaf][8][mean, rstd].
template <int C, int NP>
__global__ void __launch_bounds__(256) gn_stats_k(const float* __restrict__ act, float* __restrict__ stats, int64_t n)
{
    constexpr int NG = (C / 8) * NP;
    const int64_t leaf = blockIdx.x;
    if (leaf >= n) return;
    const int g = threadIdx.x >> 5, j = threadIdx.x & 31;
    const float* x = act + leaf * (C * NP) + g * NG;
    float s = 0.0f;
    for (int i = j; i < NG; i += 32) s += x[i];
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) s += __shfl_xor(s, m, 32);
    const float mean = s / (float)NG;
    float q = 0.0f;
    for (int i = j; i < NG; i += 32) {
        const float d = x[i] - mean;
        q = __builtin_fmaf(d, d, q);
    }
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) q += __shfl_xor(q, m, 32);
    if (j == 0) {
        stats[leaf * 16 + 2 * g] = mean;
        stats[leaf * 16 + 2 * g + 1] = 1.0f / sqrtf(q / (float)NG + 1e-5f);
    }
}

// In place: act = relu(GroupNorm(act)) with the same per-element formula as conv_k's IN_GNRELU fill (grid-stride loop).
template <int C, int NP>
__global__ void __launch_bounds__(256) gn_relu_k(float* __restrict__ act, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * (C * NP); i += (int64_t)gridDim.x * 256) {
        const int64_t leaf = i / (C * NP);
        const int c = (int)(i % (C * NP)) / NP, g = c / (C / 8);
        float v = (act[i] - stats[leaf * 16 + 2 * g]) * stats[leaf * 16 + 2 * g + 1];
        v = v * gamma[c] + beta[c];
        act[i] = v > 0.0f ? v : 0.0f;
    }
}

// ChannelAttention(128) gates of one leaf per workgroup: mean over 64 positions (sequential sum), fc 128->32, ReLU,
// fc 32->128, sigmoid.  Out: gate[leaf][128].
__global__ void __launch_bounds__(128) se_k(const float* __restrict__ act, const float* __restrict__ w1, const float* __restrict__ w2,
                                            float* __restrict__ gate, int64_t n)
{
    __shared__ float m[128], h[32];
    const int64_t leaf = blockIdx.x;
    if (leaf >= n) return;
    const int c = threadIdx.x;
    const float* x = act + leaf * (128 * 64) + c * 64;
    float s = 0.0f;
    for (int p = 0; p < 64; ++p) s += x[p];
    m[c] = s / 64.0f;
    __syncthreads();
    if (c < 32) {
        float t = 0.0f;
        for (int k = 0; k < 128; ++k) t = __builtin_fmaf(w1[c * 128 + k], m[k], t);
        h[c] = t > 0.0f ? t : 0.0f;
    }
    __syncthreads();
    float t = 0.0f;
    for (int k = 0; k < 32; ++k) t = __builtin_fmaf(w2[c * 32 + k], h[k], t);
    gate[leaf * 128 + c] = 1.0f / (1.0f + expf(-t));
}

// Nearest code of every latent position: d = (|z|^2 + |e|^2) - 2 z.e, first minimum (torch.argmin).  One wave per leaf
// (both 32-position tiles), 4 leaves per workgroup; the codebook streams through LDS in blocks of 128 codes as MFMA
// A-fragments ef[tile][k-pair][lane] with |e|^2 beside them (padding codes: zero rows, |e|^2 = +inf, never chosen).
// Each lane scans its 16 codes of a tile in increasing order (strict <), the two half-waves then merge with the lower
// index winning ties.  Out: uint16 [leaf][64].
constexpr int VQ_BLOCK_CODES = 128;
constexpr int VQ_LDS_FLOATS = VQ_BLOCK_CODES * 64 + VQ_BLOCK_CODES;
__global__ void __launch_bounds__(256) vq_k(const float* __restrict__ z, const float* __restrict__ ef, const float* __restrict__ ee,
                                            int kpad, uint16_t* __restrict__ idx, int64_t n)
{
    __shared__ __attribute__((aligned(16))) float es[VQ_LDS_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, kh = lane >> 5, col = lane & 31;
    const int64_t leaf = (int64_t)blockIdx.x * 4 + (tid >> 6);
    const bool live = leaf < n;
    float zb[2][32];
    float zz[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            zb[j][k] = live ? z[leaf * 4096 + (2 * k + kh) * 64 + 32 * j + col] : 0.0f;
            s = __builtin_fmaf(zb[j][k], zb[j][k], s);
        }
        const float o = __shfl_xor(s, 32);
        zz[j] = kh == 0 ? s + o : o + s;
    }
    float best[2] = {INFINITY, INFINITY};
    int bi[2] = {0, 0};
    for (int base = 0; base < kpad; base += VQ_BLOCK_CODES) {
        __syncthreads();
        const f32x4* src = reinterpret_cast<const f32x4*>(ef + (size_t)base * 64);
        for (int i = tid; i < VQ_BLOCK_CODES * 16; i += 256) reinterpret_cast<f32x4*>(es)[i] = src[i];
        if (tid < VQ_BLOCK_CODES) es[VQ_BLOCK_CODES * 64 + tid] = ee[base + tid];
        __syncthreads();
#pragma unroll
        for (int t = 0; t < VQ_BLOCK_CODES / 32; ++t) {
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                const float av = es[(t * 32 + k) * 64 + lane];
                acc[0] = mfma32(av, zb[0][k], acc[0]);
                acc[1] = mfma32(av, zb[1][k], acc[1]);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cl = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                const float e2 = es[VQ_BLOCK_CODES * 64 + cl];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float d = (zz[j] + e2) - 2.0f * acc[j][r];
                    if (d < best[j]) best[j] = d, bi[j] = base + cl;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float od = __shfl_xor(best[j], 32);
        const int oi = __shfl_xor(bi[j], 32);
        if (od < best[j] || (od == best[j] && oi < bi[j])) best[j] = od, bi[j] = oi;
        if (live && kh == 0) idx[leaf * 64 + 32 * j + col] = (uint16_t)bi[j];
    }
}

// Decoder input: q[leaf][c][p] = codebook[min(idx[leaf][p], K-1)][c].  The clamp keeps a caller's out-of-range index
// (a precondition violation on the device path) inside the codebook.  Grid-stride loop.
__global__ void __launch_bounds__(256) gather_k(const uint16_t* __restrict__ idx, const float* __restrict__ emb, int k_codes,
                                                float* __restrict__ q, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * 4096; i += (int64_t)gridDim.x * 256) {
        const int64_t leaf = i >> 12;
        const int c = (int)(i >> 6) & 63, p = (int)i & 63;
        const int code = min((int)idx[leaf * 64 + p], k_codes - 1);
        q[i] = emb[(size_t)code * 64 + c];
    }
}

// Decoder tail after up_conv: PixelShuffle3D(2) of u[leaf][256][4^3] into 32 channels at 8^3 (LDS), conv 32->3 k3 p1
// (fmaf, input channel major, taps in d,h,w order, zero-padding taps skipped), + bias, tanh, channels-last store
// out[leaf][512][3].  One leaf per workgroup, one output position per lane; the weights are wave-uniform (scalar loads).
__global__ void __launch_bounds__(512) final_k(const float* __restrict__ u, const float* __restrict__ w, const float* __restrict__ bias,
                                               float* __restrict__ out, int64_t n)
{
    extern __shared__ float xs[];   // [32][512]
    const int64_t leaf = blockIdx.x;
    if (leaf >= n) return;
    const int tid = threadIdx.x;
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
#pragma unroll
    for (int co = 0; co < 3; ++co) out[leaf * 1536 + tid * 3 + co] = tanhf(acc[co] + bias[co]);
}

}  // namespace v3
