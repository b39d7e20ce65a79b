// vq_vec3_bf16.h — convolutions of the Vec3 model with bf16 matrix operands (the opt-in inference mode
// vqhip_vec3_set_precision(VQHIP_VEC3_PRECISION_BF16)).  Everything that is not a convolution operand keeps the fp32 kernels
// of vq_vec3.h.
//
// Arithmetic: both operands of every product are bf16 (round to nearest even): the weight when its fragments are packed
// (frag_bf16_k), the activation when the LDS tile is filled, after the fused input transform has been evaluated in fp32 with
// the per-element formula of v3::conv_k's fill.  v_mfma_f32_32x32x16_bf16 accumulates the (exact) products in fp32; bias,
// the res + 0.1 y store and every tensor in global memory stay fp32.
//
// Layout: M = output channels (32-channel tiles), N = output positions (32-position tiles of the workgroup's LPB leaves),
// K = taps x input channels, tap-major, input channels minor; one MFMA takes 16 consecutive input channels of one tap, lane
// l holding channels 8 (l >> 5) .. + 7 of row / column l & 31.  The input leaves sit in LDS as bf16, channels minor:
// a position is a row of CINP bf16, cut into 16-byte chunks of 8 channels, and a lane's B fragment is one ds_read_b128 of
// the chunk at the tap-shifted position; positions outside the leaf read a row of zeros.  The chunk index is XORed with a
// key of the position (Tile::off) so that the 16 lanes ds_read_b128 serves together fall on 16 different 16-byte slots of
// the 256-byte bank row.  encoder.pre.0 (3 input channels) pads a tap to 8 channels and gives the two lane halves two
// consecutive taps (PAIR): 14 MFMAs for 27 taps, 81 of 224 K slots real.
#pragma once

#include "vq_bf16.h"   // v3b::bf16_bits
#include "vq_vec3.h"

namespace v3b {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// LDS image of one leaf: NPI rows of CINP bf16.  off(pos, chunk) is the byte offset of 8 channels of a position.
// Stride-1 convs read 32 consecutive positions (shifted by the tap) per wave: the key is the row's index among the rows
// that share a 256-byte bank row, modulo the chunks of a row (256-byte rows: pos & 15; 128-byte rows: (pos >> 1) & 7, the
// row's parity choosing the half).  The stride-2 conv (down1, 8^3 -> 4^3) reads positions 2 apart in w and 2 rows apart in
// h: its image swaps bits 0 and 4 of the row index (the half then follows h) and keys on bits 1, 2 (w) and 5 (h).
template <int CINP, int STRIDE>
struct Tile {
    static constexpr int ROWB = CINP * 2, NCH = CINP / 8;
    static_assert(CINP == 8 || ((CINP == 64 || CINP == 128) && (STRIDE == 1 || CINP == 64)), "tile layout");
    __device__ static inline int off(int pos, int chunk)
    {
        if constexpr (NCH == 1) return pos * ROWB;
        else if constexpr (STRIDE == 2) {
            const int row = (pos & ~17) | ((pos & 1) << 4) | ((pos >> 4) & 1);
            const int key = ((pos >> 1) & 3) | (((pos >> 5) & 1) << 2);
            return row * ROWB + ((chunk ^ key) << 4);
        } else {
            const int key = (pos / (256 / ROWB)) % NCH;
            return pos * ROWB + ((chunk ^ key) << 4);
        }
    }
};

template <int COUT, int SO, int LPB, int MT, int NT>
struct Shape {
    static constexpr int NPO = SO * SO * SO, TPL = NPO / 32;   // position tiles per leaf
    static constexpr int MG = COUT / 32 / MT;                 // cout groups
    static constexpr int NG = LPB * TPL / NT;                 // position-tile groups of the workgroup
    static constexpr int THREADS = MG * NG * 64;
    static_assert(COUT % (32 * MT) == 0 && NPO % 32 == 0 && (LPB * TPL) % NT == 0 && THREADS <= 1024, "tile shape");
};

constexpr int conv_threads(int cout, int so, int lpb, int mt, int nt) { return (cout / 32 / mt) * (lpb * (so * so * so / 32) / nt) * 64; }

// CIN: real input channels (3 for IN_LEAF3), CINP: channels of an LDS row (8 with PAIR, else CIN).
// wf: bf16 fragments [COUT/32][NTQ][KC][64 lanes][8], NTQ = taps (PAIR: tap pairs), KC = CINP/16 (PAIR: 1).
template <int CIN, int CINP, int COUT, int SI, int SO, int KS, int STRIDE, int PAD, int LPB, int MT, int NT, int INMODE, int OUTMODE>
__global__ void __launch_bounds__(conv_threads(COUT, SO, LPB, MT, NT))
conv_k(v3::ConvArgs a)
{
    using S = Shape<COUT, SO, LPB, MT, NT>;
    using T = Tile<CINP, STRIDE>;
    constexpr bool PAIR = INMODE == v3::IN_LEAF3;
    constexpr int NPI = SI * SI * SI, NPO = S::NPO, KT = KS * KS * KS;
    constexpr int NTQ = PAIR ? (KT + 1) / 2 : KT, KC = PAIR ? 1 : CINP / 16;
    constexpr int LEAFB = NPI * T::ROWB, ZERO = LPB * LEAFB;   // one row of zeros after the leaves
    static_assert(PAIR ? (CINP == 8 && CIN == 3) : (CINP == CIN && CIN % 16 == 0), "channel padding");
    extern __shared__ __attribute__((aligned(16))) unsigned char xb[];   // [LPB][NPI rows][CINP] bf16 + zero row
    const int tid = threadIdx.x;
    const int64_t leaf0 = (int64_t)blockIdx.x * LPB;

    // ---- fill: one item = 8 channels of one position; the transform in fp32 as v3::conv_k, then bf16 ----
    for (int i = tid; i < LPB * T::NCH * NPI; i += S::THREADS) {
        const int l = i / (T::NCH * NPI), ch = (i / NPI) % T::NCH, p = i % NPI;
        const int64_t leaf = leaf0 + l;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.0f;
        if (leaf < a.n) {
            if constexpr (INMODE == v3::IN_LEAF3) {
#pragma unroll
                for (int j = 0; j < 3; ++j) v[j] = a.in[leaf * 1536 + p * 3 + j];
            } else {
                const float* src = a.in + leaf * (CIN * NPI) + (ch * 8) * NPI + p;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = src[j * NPI];
                if constexpr (INMODE == v3::IN_GNRELU) {
                    const int g = (ch * 8) / (CIN / 8);
                    const float mean = a.stats[leaf * 16 + 2 * g], rstd = a.stats[leaf * 16 + 2 * g + 1];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float t = (v[j] - mean) * rstd;
                        t = t * a.gamma[ch * 8 + j] + a.beta[ch * 8 + j];
                        v[j] = t > 0.0f ? t : 0.0f;
                    }
                } else if constexpr (INMODE == v3::IN_GATE) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = v[j] * a.gate[leaf * CIN + ch * 8 + j];
                }
            }
        }
        u32x4 pk;
#pragma unroll
        for (int j = 0; j < 4; ++j) pk[j] = bf16_bits(v[2 * j]) | (bf16_bits(v[2 * j + 1]) << 16);
        *reinterpret_cast<u32x4*>(xb + l * LEAFB + T::off(p, ch)) = pk;
    }
    for (int i = tid; i < T::ROWB / 4; i += S::THREADS) reinterpret_cast<uint32_t*>(xb + ZERO)[i] = 0u;
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int ct0 = (wave % S::MG) * MT, gt0 = (wave / S::MG) * NT;   // first cout tile, first position tile of the workgroup
    const int n = lane & 31, kh = lane >> 5;

    int od[NT], oh[NT], ow[NT], lb[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int g = gt0 + j, p = (g % S::TPL) * 32 + n;
        lb[j] = (g / S::TPL) * LEAFB;
        od[j] = p / (SO * SO), oh[j] = (p / SO) % SO, ow[j] = p % SO;
    }
    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    for (int tq = 0; tq < NTQ; ++tq) {
        const int tap = PAIR ? 2 * tq + kh : tq;
        const int kd = tap / (KS * KS), khh = (tap / KS) % KS, kw = tap % KS;
        int base[NT], key[NT];
        bool any = false;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int id = od[j] * STRIDE - PAD + kd, ih = oh[j] * STRIDE - PAD + khh, iw = ow[j] * STRIDE - PAD + kw;
            const bool ok = tap < KT && id >= 0 && id < SI && ih >= 0 && ih < SI && iw >= 0 && iw < SI;
            const int pos = (id * SI + ih) * SI + iw;
            // chunk c of the position sits at off(pos, 0) ^ (c << 4): base and key separate the row from the XOR
            const int o0 = ok ? T::off(pos, 0) : 0;
            base[j] = ok ? lb[j] + (o0 & ~(T::ROWB - 1)) : ZERO;
            key[j] = PAIR ? 0 : (((o0 & (T::ROWB - 1)) >> 4) ^ kh);
            any |= ok;
        }
        if (__ballot(any) == 0) continue;   // wave-uniform: every product of this step is zero
        const bf16x8* w = reinterpret_cast<const bf16x8*>(a.wf) + ((size_t)ct0 * NTQ + tq) * KC * 64 + lane;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
            bf16x8 b[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) b[j] = *reinterpret_cast<const bf16x8*>(xb + base[j] + (((2 * kc) ^ key[j]) << 4));
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const bf16x8 av = w[((size_t)i * NTQ * KC + kc) * 64];
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, b[j], acc[i][j], 0, 0, 0);
            }
        }
    }

    // ---- store (v3::conv_k's epilogue): reg r of lane -> cout row (r&3) + 8(r>>2) + 4kh, position column n ----
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int g = gt0 + j;
        const int64_t leaf = leaf0 + g / S::TPL;
        if (leaf >= a.n) continue;
        float* out = a.out + leaf * (COUT * NPO);
        const float* res = a.res + leaf * (COUT * NPO);
        const int p = (g % S::TPL) * 32 + n;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = (ct0 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                float v = acc[i][j][r] + a.bias[co];
                if constexpr (OUTMODE == v3::OUT_RESID) v = res[co * NPO + p] + 0.1f * v;
                out[co * NPO + p] = v;
            }
    }
}

// bf16 fragments of one conv from its fp32 fragments (v3_frag: [ctile][tap][cin_src/2][64]), on the device: one thread per
// lane fragment of 8.  pair = 1 (encoder.pre.0): element j is input channel j of tap 2 tq + (lane >> 5); else input channel
// 16 kc + 8 (lane >> 5) + j of tap tq.  Channels >= cin_src and tap 27 are zero.
__global__ void __launch_bounds__(256) frag_bf16_k(const float* __restrict__ src, int cout, int cin_src, int kt, int pair, uint16_t* __restrict__ dst)
{
    const int ntq = pair ? (kt + 1) / 2 : kt, kc_n = pair ? 1 : cin_src / 16;
    const int64_t total = (int64_t)(cout / 32) * ntq * kc_n * 64;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int lane = (int)(i & 63), kc = (int)((i >> 6) % kc_n), tq = (int)((i >> 6) / kc_n % ntq), ct = (int)((i >> 6) / kc_n / ntq);
        const int tap = pair ? 2 * tq + (lane >> 5) : tq;
        u32x4 pk;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ci = pair ? j : 16 * kc + 8 * (lane >> 5) + j;
            float v = 0.0f;
            if (ci < cin_src && tap < kt) v = src[(((int64_t)ct * kt + tap) * (cin_src / 2) + ci / 2) * 64 + (ci & 1) * 32 + (lane & 31)];
            const uint32_t h = bf16_bits(v);
            if (j & 1) pk[j >> 1] |= h << 16;
            else pk[j >> 1] = h;
        }
        reinterpret_cast<u32x4*>(dst)[i] = pk;
    }
}

}  // namespace v3b
