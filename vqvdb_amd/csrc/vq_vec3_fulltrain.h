// vq_vec3_fulltrain.h — backward and optimizer kernels of the full Vec3 training step (include/vqvdb_hip_vec3_fulltrain.h,
// DESIGN.md §13).  The forward of a training step runs the inference kernels of vq_vec3.h unchanged; the data gradients of
// the stride-1 convs run conv_k of vq_vec3.h on transposed, tap-flipped fragments (built by dfrag_k).  The rest is here:
//
//   loss_final_bwd_k  d(loss)/d(pre-tanh) of 0.8 mse + 0.2 l1, the data gradient of decoder.final (VALU, 3 output
//                     channels) and the inverse PixelShuffle3D into the [256][4^3] gradient of up_conv
//   wgrad_k           weight gradient of any conv on v_mfma_f32_32x32x2_f32: M = output channels, N = input channels,
//                     K = the output positions of a leaf; one workgroup per (cout tile, cin tile, leaf group), the leaves
//                     of its group in order, the input re-formed on the LDS fill as the forward formed it
//   bias_part_k       bias gradient partials of a leaf group (sequential sums)
//   reduce_k          partials [groups][count] -> the flat gradient, groups added in ascending order in fp64
//   gn_bwd_k          GroupNorm(8) + ReLU backward of one leaf: mask from the saved pre-norm tensor, dx, and per-leaf
//                     dgamma / dbeta partials
//   se_bwd_k          ChannelAttention backward of one leaf: gate, sigmoid, both fc weight gradients, the mean-pool path
//   down_dgrad_k      data gradient of encoder.down1 (k3 s2 p1): a transposed conv 4^3 x 128 -> 8^3 x 64, one wave per
//                     parity class of the 8^3 positions (1 tap per even coordinate, at most 2 per odd one)
//   dz_k              d/dz of the straight-through decoder input plus the commitment term
//   frag_k / dfrag_k / downT_k   device rebuild of the forward fragments, the dgrad fragments and down1's transposed table
//                     from the flat parameter vector (permutations; dfrag_k also folds the residual scale in)
//
// Every sum has a fixed order and no kernel uses float atomics, so a call gives the same bits on any stream.
#pragma once

#include "vq_vec3.h"

namespace v3f {

constexpr int IN_SHUF = 4;    // wgrad_k input: PixelShuffle3D(2) of u[leaf][256][4^3] -> 32 channels at 8^3
constexpr int WG_THREADS = 256;
constexpr int WG_TAPS_PER_WAVE = 7;   // ceil(27 / 4)

// dpre[leaf][3][512] = (1 - r^2) (0.8 * 2 (r - x) + 0.2 sign(r - x)) * inv_count   (r = tanh output, sign(0) = 0)
// du[leaf][256][64]  = PixelUnshuffle3D(d/dx of final's input), final: conv 32->3 k3 p1.  One leaf per workgroup, one 8^3
// position per lane.
__global__ void __launch_bounds__(512) loss_final_bwd_k(const float* __restrict__ recon, const float* __restrict__ x, const float* __restrict__ w,
                                                        float inv_count, float* __restrict__ dpre, float* __restrict__ du, int64_t n)
{
    __shared__ float g[3][512];
    const int64_t leaf = blockIdx.x;
    if (leaf >= n) return;
    const int tid = threadIdx.x;
    for (int co = 0; co < 3; ++co) {
        const float r = recon[leaf * 1536 + tid * 3 + co], xv = x[leaf * 1536 + tid * 3 + co];
        const float d = r - xv;
        const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
        const float v = (1.0f - r * r) * (0.8f * 2.0f * d + 0.2f * sg) * inv_count;
        g[co][tid] = v;
        dpre[leaf * 1536 + co * 512 + tid] = v;
    }
    __syncthreads();
    const int d = tid >> 6, h = (tid >> 3) & 7, wx = tid & 7;
    float* dul = du + leaf * (256 * 64);
    for (int ci = 0; ci < 32; ++ci) {
        float acc = 0.0f;
        for (int tap = 0; tap < 27; ++tap) {
            // forward: out[p] += w[co][ci][tap] x[p + off(tap)]  ->  dx[q] += w dY[q - off(tap)]
            const int pd = d - (tap / 9 - 1), ph = h - ((tap / 3) % 3 - 1), pw = wx - (tap % 3 - 1);
            if (pd < 0 || pd > 7 || ph < 0 || ph > 7 || pw < 0 || pw > 7) continue;
            const int p = pd * 64 + ph * 8 + pw;
#pragma unroll
            for (int co = 0; co < 3; ++co) acc = __builtin_fmaf(w[(co * 32 + ci) * 27 + tap], g[co][p], acc);
        }
        const int uc = ci * 8 + (d & 1) * 4 + (h & 1) * 2 + (wx & 1);
        dul[uc * 64 + (d >> 1) * 16 + (h >> 1) * 4 + (wx >> 1)] = acc;
    }
}

struct WgradArgs {
    const float* dy;      // [leaf][COUT][SO^3]
    const float* in;      // the conv's input as stored (leaves [leaf][512][3] for IN_LEAF3, u for IN_SHUF)
    const float* stats;   // IN_GNRELU
    const float* gamma;
    const float* beta;
    const float* gate;    // IN_GATE
    float dy_scale;       // multiplies dy on load (the residual scale of a ResidualBlock's conv2)
    float* part;          // [groups][COUT][CIN][KS^3]
    int64_t n;
    int group;            // leaves per workgroup
};

// Weight-gradient partials of a conv: part[g][co][ci][tap] = sum over the leaves of group g (ascending) and over the output
// positions (ascending, two per MFMA step) of dy[co][p] * x'[ci][in(p, tap)].  Four waves per workgroup; wave w owns taps
// w, w+4, ...  The leaf's dy tile [32][SO^3] and input tile [32][SI^3] sit in LDS (rows padded by one float).
template <int CIN, int COUT, int SI, int SO, int KS, int STRIDE, int PAD, int INMODE>
__global__ void __launch_bounds__(WG_THREADS) wgrad_k(WgradArgs a)
{
    constexpr int NPI = SI * SI * SI, NPO = SO * SO * SO, KT = KS * KS * KS;
    constexpr int CT = (CIN + 31) / 32, OT = (COUT + 31) / 32;
    constexpr int RI = NPI + 1, RO = NPO + 1;
    extern __shared__ float sm[];
    float* ys = sm;              // [32][RO]
    float* xs = sm + 32 * RO;    // [32][RI]
    const int tid = threadIdx.x, lane = tid & 63, kh = lane >> 5, col = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ot = blockIdx.x / CT, ct = blockIdx.x % CT;
    const int64_t l0 = (int64_t)blockIdx.y * a.group;
    const int64_t l1 = l0 + a.group < a.n ? l0 + a.group : a.n;

    f32x16 acc[WG_TAPS_PER_WAVE];
#pragma unroll
    for (int j = 0; j < WG_TAPS_PER_WAVE; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

    for (int64_t leaf = l0; leaf < l1; ++leaf) {
        __syncthreads();   // the previous leaf's tiles are consumed
        for (int i = tid; i < 32 * NPO; i += WG_THREADS) {
            const int r = i / NPO, p = i % NPO, co = ot * 32 + r;
            ys[r * RO + p] = co < COUT ? a.dy[(leaf * COUT + co) * NPO + p] * a.dy_scale : 0.0f;
        }
        for (int i = tid; i < 32 * NPI; i += WG_THREADS) {
            const int r = i / NPI, p = i % NPI, c = ct * 32 + r;
            float v = 0.0f;
            if (c < CIN) {
                if constexpr (INMODE == v3::IN_LEAF3) {
                    v = a.in[leaf * 1536 + p * 3 + c];
                } else if constexpr (INMODE == IN_SHUF) {
                    const int d = p >> 6, h = (p >> 3) & 7, wx = p & 7;
                    const int uc = c * 8 + (d & 1) * 4 + (h & 1) * 2 + (wx & 1);
                    v = a.in[leaf * (256 * 64) + uc * 64 + (d >> 1) * 16 + (h >> 1) * 4 + (wx >> 1)];
                } else {
                    v = a.in[(leaf * CIN + c) * NPI + p];
                    if constexpr (INMODE == v3::IN_GNRELU) {
                        const int g = c / (CIN / 8);
                        const float mean = a.stats[leaf * 16 + 2 * g], rstd = a.stats[leaf * 16 + 2 * g + 1];
                        v = (v - mean) * rstd;
                        v = v * a.gamma[c] + a.beta[c];
                        v = v > 0.0f ? v : 0.0f;
                    } else if constexpr (INMODE == v3::IN_GATE) {
                        v = v * a.gate[leaf * CIN + c];
                    }
                }
            }
            xs[r * RI + p] = v;
        }
        __syncthreads();
        if (wave < KT) {
            const float* yrow = ys + col * RO;
            const float* xrow = xs + col * RI;
            for (int s = 0; s < NPO / 2; ++s) {
                const int p = 2 * s + kh;
                const int od = p / (SO * SO), oh = (p / SO) % SO, ow = p % SO;
                const float av = yrow[p];
#pragma unroll
                for (int j = 0; j < WG_TAPS_PER_WAVE; ++j) {
                    const int tap = wave + 4 * j;
                    if (tap < KT) {
                        const int kd = tap / (KS * KS), khh = (tap / KS) % KS, kw = tap % KS;
                        const int id = od * STRIDE - PAD + kd, ih = oh * STRIDE - PAD + khh, iw = ow * STRIDE - PAD + kw;
                        const bool ok = id >= 0 && id < SI && ih >= 0 && ih < SI && iw >= 0 && iw < SI;
                        const float bv = ok ? xrow[(id * SI + ih) * SI + iw] : 0.0f;
                        acc[j] = mfma32(av, bv, acc[j]);
                    }
                }
            }
        }
    }
    if (wave >= KT) return;
    const int ci = ct * 32 + col;
    if (ci >= CIN) return;
    float* out = a.part + (size_t)blockIdx.y * COUT * CIN * KT;
#pragma unroll
    for (int j = 0; j < WG_TAPS_PER_WAVE; ++j) {
        const int tap = wave + 4 * j;
        if (tap >= KT) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = ot * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (co < COUT) out[((size_t)co * CIN + ci) * KT + tap] = acc[j][r];
        }
    }
}

template <int CIN, int COUT, int SI, int SO, int KS>
constexpr unsigned wgrad_blocks() { return (unsigned)(((CIN + 31) / 32) * ((COUT + 31) / 32)); }
template <int SI, int SO>
constexpr size_t wgrad_lds() { return (size_t)32 * (SO * SO * SO + 1 + SI * SI * SI + 1) * sizeof(float); }

// part[g][c] = sum over the leaves of group g (ascending), then positions (ascending) of dy_scale * dy[leaf][c][p]
__global__ void __launch_bounds__(256) bias_part_k(const float* __restrict__ dy, int c_n, int np, int64_t n, int group, float dy_scale,
                                                   float* __restrict__ part)
{
    const int64_t l0 = (int64_t)blockIdx.x * group;
    const int64_t l1 = l0 + group < n ? l0 + group : n;
    for (int c = threadIdx.x; c < c_n; c += 256) {
        float s = 0.0f;
        for (int64_t leaf = l0; leaf < l1; ++leaf) {
            const float* y = dy + (leaf * c_n + c) * np;
            for (int p = 0; p < np; ++p) s += y[p] * dy_scale;
        }
        part[(size_t)blockIdx.x * c_n + c] = s;
    }
}

// out[i] = sum over g ascending of part[g * stride + i] (fp64), i < count
__global__ void __launch_bounds__(256) reduce_k(const float* __restrict__ part, int64_t groups, int64_t stride, int64_t count, float* __restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        double s = 0.0;
        for (int64_t g = 0; g < groups; ++g) s += (double)part[g * stride + i];
        out[i] = (float)s;
    }
}

// GroupNorm(8, C) + ReLU backward of one leaf per workgroup (256 threads, 32 lanes per group as gn_stats_k).
//   v = ((x - mean) rstd) gamma + beta (the forward's formula), dv = [v > 0] da, dxhat = dv gamma
//   dx = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)) + addend        (addend may alias dx, never da)
//   part[leaf][c] = sum_p dv xhat (dgamma),  part[leaf][C + c] = sum_p dv (dbeta), positions ascending
template <int C, int NP>
__global__ void __launch_bounds__(256) gn_bwd_k(const float* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, const float* __restrict__ da, const float* addend, float* dx,
                                                float* __restrict__ part, int64_t n)
{
    constexpr int CG = C / 8, NG = CG * NP;
    const int64_t leaf = blockIdx.x;
    if (leaf >= n) return;
    const int tid = threadIdx.x, g = tid >> 5, j = tid & 31;
    const float mean = stats[leaf * 16 + 2 * g], rstd = stats[leaf * 16 + 2 * g + 1];
    const int64_t base = leaf * (C * NP) + (int64_t)g * NG;
    float s1 = 0.0f, s2 = 0.0f;
    for (int i = j; i < NG; i += 32) {
        const int c = g * CG + i / NP;
        const float xh = (x[base + i] - mean) * rstd;
        const float v = xh * gamma[c] + beta[c];
        const float dxh = v > 0.0f ? da[base + i] * gamma[c] : 0.0f;
        s1 += dxh;
        s2 = __builtin_fmaf(dxh, xh, s2);
    }
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) s1 += __shfl_xor(s1, m, 32), s2 += __shfl_xor(s2, m, 32);
    const float m1 = s1 / (float)NG, m2 = s2 / (float)NG;
    if (tid < C) {
        const int c = tid, gc = c / CG;
        const float mc = stats[leaf * 16 + 2 * gc], rc = stats[leaf * 16 + 2 * gc + 1];
        const float* xc = x + leaf * (C * NP) + (int64_t)c * NP;
        const float* dc = da + leaf * (C * NP) + (int64_t)c * NP;
        float dg = 0.0f, db = 0.0f;
        for (int p = 0; p < NP; ++p) {
            const float xh = (xc[p] - mc) * rc;
            const float v = xh * gamma[c] + beta[c];
            const float dv = v > 0.0f ? dc[p] : 0.0f;
            dg = __builtin_fmaf(dv, xh, dg);
            db += dv;
        }
        part[leaf * (2 * C) + c] = dg;
        part[leaf * (2 * C) + C + c] = db;
    }
    for (int i = j; i < NG; i += 32) {
        const int c = g * CG + i / NP;
        const float xh = (x[base + i] - mean) * rstd;
        const float v = xh * gamma[c] + beta[c];
        const float dxh = v > 0.0f ? da[base + i] * gamma[c] : 0.0f;
        float r = rstd * (dxh - m1 - xh * m2);
        if (addend) r += addend[base + i];
        dx[base + i] = r;
    }
}

// ChannelAttention(128) backward of one leaf per workgroup (128 threads).  Forward (se_k): m = mean_p x, hp = W1 m,
// h = relu(hp), t = W2 h, g = sigmoid(t), out = x g.  In: dout [128][64].  Out: dx [128][64],
// part[leaf][0, 4096) = dW1 [32][128], part[leaf][4096, 8192) = dW2 [128][32].
__global__ void __launch_bounds__(128) se_bwd_k(const float* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ w2,
                                                const float* __restrict__ dout, float* __restrict__ dx, float* __restrict__ part, int64_t n)
{
    __shared__ float m[128], hp[32], h[32], ds[128], dh[32];
    const int64_t leaf = blockIdx.x;
    if (leaf >= n) return;
    const int c = threadIdx.x;
    const float* xc = x + leaf * (128 * 64) + c * 64;
    const float* dc = dout + leaf * (128 * 64) + c * 64;
    float s = 0.0f;
    for (int p = 0; p < 64; ++p) s += xc[p];
    m[c] = s / 64.0f;
    __syncthreads();
    if (c < 32) {
        float t = 0.0f;
        for (int k = 0; k < 128; ++k) t = __builtin_fmaf(w1[c * 128 + k], m[k], t);
        hp[c] = t;
        h[c] = t > 0.0f ? t : 0.0f;
    }
    __syncthreads();
    float t = 0.0f;
    for (int k = 0; k < 32; ++k) t = __builtin_fmaf(w2[c * 32 + k], h[k], t);
    const float gt = 1.0f / (1.0f + expf(-t));
    float dg = 0.0f;
    for (int p = 0; p < 64; ++p) dg = __builtin_fmaf(dc[p], xc[p], dg);
    ds[c] = dg * gt * (1.0f - gt);
    __syncthreads();
    float* pl = part + leaf * 8192;
    for (int k = 0; k < 32; ++k) pl[4096 + c * 32 + k] = ds[c] * h[k];
    if (c < 32) {
        float a = 0.0f;
        for (int k = 0; k < 128; ++k) a = __builtin_fmaf(w2[k * 32 + c], ds[k], a);
        dh[c] = hp[c] > 0.0f ? a : 0.0f;
    }
    __syncthreads();
    for (int k = 0; k < 32; ++k) pl[k * 128 + c] = dh[k] * m[c];
    float dm = 0.0f;
    for (int k = 0; k < 32; ++k) dm = __builtin_fmaf(w1[k * 128 + c], dh[k], dm);
    dm = dm / 64.0f;
    float* o = dx + leaf * (128 * 64) + c * 64;
    for (int p = 0; p < 64; ++p) o[p] = __builtin_fmaf(dc[p], gt, dm);
}

// encoder.down1 data gradient: dx[ci][i] = sum over co and the taps with i = 2 o + k - 1 (per axis) of W[co][ci][k] dy[co][o].
// One leaf per workgroup of 512 threads; wave = parity class (pd, ph, pw) of i, lane = (jd, jh, jw) with i = 2 j + parity:
// an even coordinate has the one tap k = 1 (o = j), an odd one k = 2 (o = j) and k = 0 (o = j + 1 < 4).  The taps and the
// weights wt[ci][tap][co] are wave-uniform; dy [128][64] sits in LDS.
__global__ void __launch_bounds__(512) down_dgrad_k(const float* __restrict__ dy, const float* __restrict__ wt, float* __restrict__ dx, int64_t n)
{
    __shared__ float ys[128 * 64];
    const int64_t leaf = blockIdx.x;
    if (leaf >= n) return;
    const int tid = threadIdx.x;
    for (int i = tid; i < 128 * 64; i += 512) ys[i] = dy[leaf * 8192 + i];
    __syncthreads();
    const int par = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int pd = par >> 2, ph = (par >> 1) & 1, pw = par & 1;
    const int jd = lane >> 4, jh = (lane >> 2) & 3, jw = lane & 3;
    const int nd = pd ? 2 : 1, nh = ph ? 2 : 1, nw = pw ? 2 : 1;
    int tap[8], pos[8];
    bool ok[8];
    int nt = 0;
    for (int a = 0; a < nd; ++a)
        for (int b = 0; b < nh; ++b)
            for (int e = 0; e < nw; ++e) {
                const int kd = pd ? (a ? 0 : 2) : 1, kh = ph ? (b ? 0 : 2) : 1, kw = pw ? (e ? 0 : 2) : 1;
                const int od = jd + (pd && a), oh = jh + (ph && b), ow = jw + (pw && e);
                tap[nt] = kd * 9 + kh * 3 + kw;
                ok[nt] = od < 4 && oh < 4 && ow < 4;
                pos[nt] = ok[nt] ? od * 16 + oh * 4 + ow : 0;
                ++nt;
            }
    const int i = (2 * jd + pd) * 64 + (2 * jh + ph) * 8 + (2 * jw + pw);
    float* o = dx + leaf * (64 * 512);
    for (int ci = 0; ci < 64; ++ci) {
        float acc = 0.0f;
        for (int t = 0; t < nt; ++t) {
            const float* w = wt + ((size_t)ci * 27 + tap[t]) * 128;
            const float* y = ys + pos[t];
            const bool v = ok[t];
            for (int co = 0; co < 128; ++co) acc = __builtin_fmaf(w[co], v ? y[co * 64] : 0.0f, acc);
        }
        o[ci * 512 + i] = acc;
    }
}

// dz[leaf][c][p] = dq[leaf][c][p] + coef (z - e[idx][c]),  coef = 2 * commitment / (n_global * 4096)   (grid-stride)
__global__ void __launch_bounds__(256) dz_k(const float* __restrict__ dq, const float* __restrict__ z, const uint16_t* __restrict__ idx,
                                            const float* __restrict__ cb, float coef, float* __restrict__ dz, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * 4096; i += (int64_t)gridDim.x * 256) {
        const int64_t leaf = i >> 12;
        const int c = (int)(i >> 6) & 63, p = (int)i & 63;
        dz[i] = dq[i] + coef * (z[i] - cb[(size_t)idx[leaf * 64 + p] * 64 + c]);
    }
}

// forward fragments from W [cout][cin_real][kt] (v3_frag's index arithmetic): f[((ct kt + t) cp_n + cp) 64 + l]
__global__ void __launch_bounds__(256) frag_k(const float* __restrict__ W, int cout, int cin_real, int cin_pad, int kt, float* __restrict__ f)
{
    const int cp_n = cin_pad / 2;
    const int64_t total = (int64_t)cout * cin_pad * kt;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int l = (int)(i & 63);
        int64_t r = i >> 6;
        const int cp = (int)(r % cp_n);
        r /= cp_n;
        const int t = (int)(r % kt), ct = (int)(r / kt);
        const int co = 32 * ct + (l & 31), ci = 2 * cp + (l >> 5);
        f[i] = ci < cin_real ? W[((size_t)co * cin_real + ci) * kt + t] : 0.0f;
    }
}

// dgrad fragments of a stride-1 conv W [cout][cin][kt]: the fragments of the conv cin <- cout with tap kt-1-t, times scale
__global__ void __launch_bounds__(256) dfrag_k(const float* __restrict__ W, int cout, int cin, int kt, float scale, float* __restrict__ f)
{
    const int cp_n = cout / 2;   // the dgrad conv's input channels are the forward's outputs
    const int64_t total = (int64_t)cin * cout * kt;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int l = (int)(i & 63);
        int64_t r = i >> 6;
        const int cp = (int)(r % cp_n);
        r /= cp_n;
        const int t = (int)(r % kt), ct = (int)(r / kt);
        const int oc = 32 * ct + (l & 31), ic = 2 * cp + (l >> 5);   // oc: forward input channel, ic: forward output channel
        f[i] = scale * W[((size_t)ic * cin + oc) * kt + (kt - 1 - t)];
    }
}

// down1's transposed table wt[ci][tap][co] = W[co][ci][tap]  (W [128][64][27])
__global__ void __launch_bounds__(256) downT_k(const float* __restrict__ W, float* __restrict__ wt)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 128 * 64 * 27; i += gridDim.x * 256) {
        const int co = i % 128, tap = (i / 128) % 27, ci = i / (128 * 27);
        wt[i] = W[((size_t)co * 64 + ci) * 27 + tap];
    }
}

}  // namespace v3f
