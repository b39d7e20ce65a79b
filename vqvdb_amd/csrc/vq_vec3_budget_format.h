// vq_vec3_budget_format.h — the host arithmetic of the Vec3 handle's byte-budget calls (include/vqvdb_hip_vec3_budget.h):
// the pick of a rung from the sizes of vqhip_vec3_active_sweep, and the size of the .vqv3 file that vq_vec3_file.inc's writer
// produces for a list of grids.  The file size comes from vqv3f::layout, the function the writer places its sections with, so the two
// cannot drift apart.  Includes nothing of the GPU runtime: tests/host/vec3_budget_check.cpp builds it alone.  file_bytes is a
// template over the grid description (the fields name, leaf_ptrs, origins, n_leaves and masks of vqhip_vec3_grid_source) for that
// reason alone.
//
// Every sum is an int64 whose terms are bounded first or added with an overflow check: a total that would pass 2^63 - 1 is refused.
#pragma once

#include <cstdint>
#include <cstring>

#include "vq_vec3_file_format.h"

namespace vqv3b {

constexpr int MAX_TOLS = 64;   // VQHIP_VEC3_RATE_MAX_TOLS

// the index of the smallest tols[t] by value whose bytes[t] <= budget: NaN rungs are never chosen, of equal rungs the first wins,
// sizes need not fall as the tolerance grows.  -1: none fits, or an argument is not as stated.  *smallest (may be NULL) receives the
// smallest size of a rung that is not NaN, -1 where there is none.
inline int active_rate_pick(const int64_t* bytes, const float* tols, int n_tols, int64_t budget, int64_t* smallest = nullptr)
{
    if (smallest) *smallest = -1;
    if (!bytes || !tols || n_tols < 1 || n_tols > MAX_TOLS || budget < 0) return -1;
    for (int t = 0; t < n_tols; ++t)
        if (bytes[t] < 0) return -1;
    int best = -1;
    int64_t least = -1;
    for (int t = 0; t < n_tols; ++t) {
        if (tols[t] != tols[t]) continue;
        if (least < 0 || bytes[t] < least) least = bytes[t];
        if (bytes[t] <= budget && (best < 0 || tols[t] < tols[best])) best = t;
    }
    if (smallest) *smallest = least;
    return best;
}

// what the writer refuses of a grid list before it opens the output (v3f_compress_file)
template <typename GridSource>
inline bool grids_ok(const GridSource* grids, int n_grids, int kind)
{
    if (!grids || n_grids < 1 || n_grids > 255 || (kind != vqv3f::KIND_INDICES && kind != vqv3f::KIND_ACTIVE)) return false;
    for (int g = 0; g < n_grids; ++g) {
        const GridSource& G = grids[g];
        if (!G.name || G.n_leaves < 0 || G.n_leaves > 0xFFFFFFFFll || (G.n_leaves > 0 && (!G.leaf_ptrs || !G.origins))) return false;
        if (kind == vqv3f::KIND_ACTIVE && G.n_leaves > 0 && !G.masks) return false;
    }
    return true;
}

// the bytes of the .vqv3 file of these grids: 24 + sum_g (102 + nameLength_g + n_g (12 + 128 + (kind 1: 64 + 2))) + sum_g
// payload_bytes[g], every grid laid out by vqv3f::layout where the grid before it ends.  kind 0 has no payload: payload_bytes may be
// NULL and must hold zeros otherwise.  -1: the writer would refuse the grids, a payload is negative, or the sum passes 2^63 - 1.
template <typename GridSource>
inline int64_t file_bytes(const GridSource* grids, int n_grids, int kind, const int64_t* payload_bytes)
{
    if (!grids_ok(grids, n_grids, kind)) return -1;
    if (kind == vqv3f::KIND_ACTIVE && !payload_bytes) return -1;
    uint64_t at = vqv3f::FILE_HEADER_BYTES;
    for (int g = 0; g < n_grids; ++g) {
        const int64_t payload = payload_bytes ? payload_bytes[g] : 0;
        if (payload < 0 || (kind == vqv3f::KIND_INDICES && payload != 0)) return -1;
        const size_t name_len = std::strlen(grids[g].name);
        if (name_len > 0xFFFFFFFFull) return -1;   // nameLength is a u32
        vqv3f::Grid M;
        M.name.assign(grids[g].name, name_len);    // as the writer's M.name = G.name
        M.total = (uint32_t)grids[g].n_leaves;
        vqv3f::layout(M, kind, at);                // payload_bytes 0: end_at is where the payload begins; at most 2^32 + 206 * 2^32 more
        if (M.end_at > (uint64_t)INT64_MAX) return -1;
        int64_t end = 0;
        if (__builtin_add_overflow((int64_t)M.end_at, payload, &end)) return -1;
        at = (uint64_t)end;
    }
    return (int64_t)at;
}

}  // namespace vqv3b
