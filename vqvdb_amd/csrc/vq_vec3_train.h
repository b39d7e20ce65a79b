// vq_vec3_train.h — codebook (EMA) training kernels of the Vec3 model (include/vqvdb_hip_vec3_train.h): the
// training-mode forward of VectorQuantizerEMA (python/VQVAE_v2.py:107-156) on the encoder's latent, K codes of D = 64.
//
//   flat_k        W.z [leaf][64 ch][64 pos] -> flat [leaf*64 + pos][64] (the reference's `flat`, :111-114)
//   (assignment)  vq_k of vq_vec3.h, unchanged, against the live tables cb.f / cb.ee
//   statistics    encodings_sum, dw = encodings^T flat, sum |z - e|^2 per code (:134-137,146), deterministic, no one-hots and
//                 no float atomics.  A stable counting sort puts every code's rows into one ascending list:
//                   seg_hist_k     per segment of seg_rows consecutive rows: rows per code (integer counts)
//                   seg_scan_k     per code: exclusive scan of its segment counts (segments ascending) -> offsets, totals
//                   code_scan_k    over the codes: list start of each code, and the start of its pieces (PIECE rows each)
//                   seg_scatter_k  per segment, 64 rows at a time in row order: row ids to their code's list (stable)
//                   piece_sum_k    one wave per piece, lane = dimension: the piece's rows added in list (= row) order
//                   code_reduce_k  one wave per code: its pieces added in ascending order (fp64)
//                 A hot code is spread over rows/PIECE waves, so 2^20 rows of one code do not serialise on one wave.
//   ema_update_k  cluster_size / embed_avg EMA, embedding = embed_avg / clamp(cluster_size, eps)  (:135-144), into cb
//   tables_k      cb -> cb.f (vq_k's MFMA fragments) and cb.ee (|e|^2, sum in dimension order of unfused products): the
//                 arithmetic of v3_load's host build, bit for bit
//   straight_k    eval-mode decoder input z + (e - z) (:149), in place on W.z
#pragma once

#include "vq_vec3.h"

namespace v3t {

constexpr int D = 64;
constexpr int PIECE = 256;   // rows per statistics piece

// flat[(leaf*64 + p)*64 + c] = z[leaf][c][p]; one leaf per workgroup through LDS (reads and writes coalesced)
__global__ void __launch_bounds__(256) flat_k(const float* __restrict__ z, float* __restrict__ flat, int64_t n)
{
    __shared__ float t[64][65];
    const int64_t leaf = blockIdx.x;
    if (leaf >= n) return;
    const float* src = z + leaf * 4096;
    for (int i = threadIdx.x; i < 4096; i += 256) t[i >> 6][i & 63] = src[i];
    __syncthreads();
    float* dst = flat + leaf * 4096;
    for (int i = threadIdx.x; i < 4096; i += 256) dst[i] = t[i & 63][i >> 6];
}

// lanes of this wave whose (live) code equals mine: one ballot per code bit
__device__ inline unsigned long long same_code_mask(int code, bool live, int kbits)
{
    unsigned long long m = __ballot(live);
    for (int b = 0; b < kbits; ++b) {
        const unsigned long long bal = __ballot((code >> b) & 1);
        m &= ((code >> b) & 1) ? bal : ~bal;
    }
    return m;
}

// one wave per segment: cnt[seg][code] += rows of the segment with that code (one integer atomic per code group per 64 rows;
// only this wave touches the segment's row of the table, so the counts are exact and order-free)
__global__ void __launch_bounds__(64) seg_hist_k(const uint16_t* __restrict__ idx, int64_t rows, int seg_rows, int k_codes, int kbits,
                                                 int* __restrict__ cnt)
{
    const int seg = blockIdx.x, lane = threadIdx.x;
    const int64_t r0 = (int64_t)seg * seg_rows, r1 = r0 + seg_rows < rows ? r0 + seg_rows : rows;
    int* c = cnt + (size_t)seg * k_codes;
    for (int64_t rb = r0; rb < r1; rb += 64) {
        const int64_t r = rb + lane;
        const bool live = r < r1;
        const int code = live ? (int)idx[r] : 0;
        const unsigned long long m = same_code_mask(code, live, kbits);
        if (live && __builtin_ctzll(m) == lane) atomicAdd(c + code, __popcll(m));
    }
}

// one thread per code: cnt[s][k] -> exclusive offset of segment s inside code k's list; total[k] = rows of code k
__global__ void __launch_bounds__(256) seg_scan_k(int* __restrict__ cnt, int n_seg, int k_codes, int* __restrict__ total)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= k_codes) return;
    int s = 0;
    for (int g = 0; g < n_seg; ++g) {
        const int v = cnt[(size_t)g * k_codes + k];
        cnt[(size_t)g * k_codes + k] = s;
        s += v;
    }
    total[k] = s;
}

// one workgroup of 1024 threads: start[k] = sum of total[j < k], pstart[k] = sum of ceil(total[j] / PIECE) for j < k;
// start[K] = rows, pstart[K] = pieces
__global__ void __launch_bounds__(1024) code_scan_k(const int* __restrict__ total, int k_codes, int* __restrict__ start, int* __restrict__ pstart)
{
    __shared__ int sa[1024], sp[1024];
    const int t = threadIdx.x, per = (k_codes + 1023) / 1024;
    const int k0 = t * per, k1 = k0 + per < k_codes ? k0 + per : k_codes;
    int a = 0, p = 0;
    for (int k = k0; k < k1; ++k) a += total[k], p += (total[k] + PIECE - 1) / PIECE;
    sa[t] = a, sp[t] = p;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {   // inclusive Hillis-Steele scan
        const int va = t >= d ? sa[t - d] : 0, vp = t >= d ? sp[t - d] : 0;
        __syncthreads();
        sa[t] += va, sp[t] += vp;
        __syncthreads();
    }
    a = sa[t] - a, p = sp[t] - p;
    for (int k = k0; k < k1; ++k) {
        start[k] = a, pstart[k] = p;
        a += total[k], p += (total[k] + PIECE - 1) / PIECE;
    }
    if (t == 1023) start[k_codes] = sa[t], pstart[k_codes] = sp[t];
}

// one wave per segment, 64 rows at a time in row order: row r goes to list[start[code] + off[seg][code] + rank], rank = its
// place among the earlier rows of the segment with the same code.  off is advanced by one integer atomic per code group
// (only this wave touches the segment's offsets), so the lists are stable: every code's rows in ascending order.
__global__ void __launch_bounds__(64) seg_scatter_k(const uint16_t* __restrict__ idx, int64_t rows, int seg_rows, int k_codes, int kbits,
                                                    int* __restrict__ off, const int* __restrict__ start, int* __restrict__ list)
{
    const int seg = blockIdx.x, lane = threadIdx.x;
    const int64_t r0 = (int64_t)seg * seg_rows, r1 = r0 + seg_rows < rows ? r0 + seg_rows : rows;
    int* o = off + (size_t)seg * k_codes;
    for (int64_t rb = r0; rb < r1; rb += 64) {
        const int64_t r = rb + lane;
        const bool live = r < r1;
        const int code = live ? (int)idx[r] : 0;
        const unsigned long long m = same_code_mask(code, live, kbits);
        const int leader = live ? __builtin_ctzll(m) : lane;
        int base = 0;
        if (live && leader == lane) base = atomicAdd(o + code, __popcll(m));
        base = __shfl(base, leader);
        if (live) list[start[code] + base + __popcll(m & ((1ull << lane) - 1ull))] = (int)r;
    }
}

// one wave per piece (4 per workgroup), lane = dimension.  Piece p belongs to the code k with pstart[k] <= p < pstart[k+1]
// and covers list entries [start[k] + PIECE (p - pstart[k]), +PIECE) of that code.  Its rows are added in list order (fp32),
// the squared distance to e_k (the codebook before the update) as a per-lane fmaf chain, then lanes ascending in fp64.
__global__ void __launch_bounds__(256) piece_sum_k(const float* __restrict__ flat, const int* __restrict__ list, const int* __restrict__ start,
                                                   const int* __restrict__ pstart, const float* __restrict__ E, int k_codes, int max_pieces,
                                                   float* __restrict__ part, double* __restrict__ sqpart)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (p >= max_pieces || p >= pstart[k_codes]) return;
    int lo = 0, hi = k_codes;   // last k with pstart[k] <= p (pstart[K] > p; empty codes share their successor's start)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pstart[mid] <= p) lo = mid;
        else hi = mid;
    }
    const int k = lo;
    const int b = start[k] + (p - pstart[k]) * PIECE, e = min(b + PIECE, start[k + 1]);
    const float ek = E[(size_t)k * D + lane];
    float a = 0.0f, sq = 0.0f;
    for (int b0 = b; b0 < e; b0 += 64) {
        const int nb = min(64, e - b0);
        const int mine = lane < nb ? list[b0 + lane] : 0;   // this batch's member rows, one per lane
        for (int j0 = 0; j0 < nb; j0 += 8) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = __builtin_amdgcn_readlane(mine, (j0 + i) & 63);
                v[i] = j0 + i < nb ? flat[(size_t)r * D + lane] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (j0 + i < nb) {
                    a = a + v[i];
                    const float d = v[i] - ek;
                    sq = __builtin_fmaf(d, d, sq);
                }
        }
    }
    part[(size_t)p * D + lane] = a;
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += (double)__shfl(sq, l, 64);
    if (lane == 0) sqpart[p] = s;
}

// one wave per code (4 per workgroup), pieces added in ascending order in fp64, rounded once to fp32 (a code of one piece
// gets its fp32 piece sum unchanged): stats = [0,K) counts | [K,65K) dw[K][64] | [65K,66K) sum |z-e|^2 | [66K] rows
__global__ void __launch_bounds__(256) code_reduce_k(const float* __restrict__ part, const double* __restrict__ sqpart, const int* __restrict__ total,
                                                     const int* __restrict__ pstart, int k_codes, int64_t rows, float* __restrict__ stats)
{
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= k_codes) return;
    const int p0 = pstart[k], p1 = pstart[k + 1];
    // fp64 across pieces (a hot code's 2^20 rows are 4096 pieces); eight loads in flight, added in order
    double s = 0.0;
    int p = p0;
    for (; p + 8 <= p1; p += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = part[(size_t)(p + i) * D + lane];
#pragma unroll
        for (int i = 0; i < 8; ++i) s += (double)v[i];
    }
    for (; p < p1; ++p) s += (double)part[(size_t)p * D + lane];
    stats[k_codes + (size_t)k * D + lane] = (float)s;
    // squared error: 64 pieces per load (one per lane), added in order by every lane
    double q = 0.0;
    for (int b = p0; b < p1; b += 64) {
        const double v = b + lane < p1 ? sqpart[b + lane] : 0.0;
        const int nb = min(64, p1 - b);
        for (int l = 0; l < nb; ++l) q += __shfl(v, l, 64);
    }
    if (lane == 0) {
        stats[(size_t)65 * k_codes + k] = (float)q;
        stats[k] = (float)total[k];
        if (k == 0) stats[(size_t)66 * k_codes] = (float)rows;
    }
}

// one wave per code (4 per workgroup), lane = dimension: the EMA step of :135-144 from the (all-reduced) statistics;
// the new embedding row goes to cb (raw rows; tables_k then rebuilds the search tables from it)
__global__ void __launch_bounds__(256) ema_update_k(const float* __restrict__ stats, int k_codes, float decay, float alpha, float eps,
                                                    float* __restrict__ cluster_size, float* __restrict__ embed_avg, float* __restrict__ cb)
{
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= k_codes) return;
    const float cs = __builtin_fmaf(alpha, stats[k], cluster_size[k] * decay);
    const float avg = __builtin_fmaf(alpha, stats[k_codes + (size_t)k * D + lane], embed_avg[(size_t)k * D + lane] * decay);
    embed_avg[(size_t)k * D + lane] = avg;
    cb[(size_t)k * D + lane] = avg / (cs < eps ? eps : cs);
    if (lane == 0) cluster_size[k] = cs;   // (every lane read cluster_size[k] above: one wave, one instruction stream)
}

// the search tables of vq_k from the raw rows, as v3_load builds them on the host:
//   ef[((code/32)*32 + d/2)*64 + (d&1)*32 + code%32] = E[code][d]     ee[code] = sum over d ascending of E[code][d]^2
// (unfused multiply, then add: __fmul_rn / __fadd_rn never contract).  Padding codes keep their create-time values.
__global__ void __launch_bounds__(256) tables_k(const float* __restrict__ cb, int k_codes, float* __restrict__ ef, float* __restrict__ ee)
{
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (k >= k_codes) return;
    const float v = cb[(size_t)k * D + lane];
    ef[(((size_t)(k / 32) * 32 + lane / 2) * 64) + (lane & 1) * 32 + (k & 31)] = v;
    float s = 0.0f;
    for (int d = 0; d < D; ++d) {
        const float x = __shfl(v, d, 64);
        s = __fadd_rn(s, __fmul_rn(x, x));
    }
    if (lane == 0) ee[k] = s;
}

// eval-mode decoder input (:149 quantized = x + (quantized - x).detach()): z[leaf][c][p] = z + (e[idx] - z), fp32, in place
__global__ void __launch_bounds__(256) straight_k(float* __restrict__ z, const uint16_t* __restrict__ idx, const float* __restrict__ cb,
                                                  int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * 4096; i += (int64_t)gridDim.x * 256) {
        const int64_t leaf = i >> 12;
        const int c = (int)(i >> 6) & 63, p = (int)i & 63;
        const float x = z[i];
        z[i] = x + (cb[(size_t)idx[leaf * 64 + p] * D + c] - x);
    }
}

}  // namespace v3t
