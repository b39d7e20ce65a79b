// The kernel switches of the scalar handle: the VQHIP_* environment variables, read once at vqhip_create.  Three things live here and
// nowhere else: the fields they control (struct Switches, which vqhip_codec derives from), ONE table of every switch (SWITCHES: name,
// legal values with the default first or an integer range, what it selects, the test that runs a non-default value), and ONE parser
// (parse_switches).  THE CONTRACT:
//   - unset or empty means the default;
//   - a word the table does not list, an integer that strtol does not consume whole, that starts with white space, or that lies
//     outside the documented range fails with VQHIP_ERR_INVALID and a message that names the switch, the value and what is legal.
//     Nothing is clamped;
//   - on failure the caller's struct is untouched.
// INTEGRATION.md's "Kernel switches" table is printed from SWITCHES by tests/host/switches_check.cpp, and tests/test_switches_host.py
// holds the two together.  This header includes nothing of HIP.
#pragma once

#include <cerrno>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/vqvdb_hip.h"

struct Switches {
    int n_cus = 256;         // compute units the persistent-workgroup launches, the weight-gradient slices and the launch policies count on: the device's, or fewer (VQHIP_CUS)
    bool stem_fused = true;  // decoder front of large passes: one kernel; VQHIP_STEM=split selects stem_lut_k + gn_relu_stats_k
    bool stem_taps = true;   // ... the (tap, code) table streamed through an LDS ring tap by tap (stem_taps_k, vq_stem_taps.h: 0.81 -> 0.57 ms); VQHIP_STEM=gather selects stem_fused_k (gather through the L1)
    bool stem_small_fused = true;   // decoder front of small-batch passes: one kernel (stem_fused_k); VQHIP_STEM_SMALL=split selects gather + combine + normalise + combine
    bool tail_groups = false; // ... VQHIP_TAIL=groups: the output planes in three groups instead of five units, every input plane read 2.5x instead of 3.5x (tail_groups16_k, vq_tail_groups.h; measured equal in time, 33 spilled registers)
    bool tail_rows32 = false; // ... VQHIP_TAIL=rows32: a whole 32-leaf tile per wave, one wave per SIMD (tail_rows32_k; measured 4 % slower)
    bool tail_rows = true;   // folded decoder tail of full chunks: 16-voxel tiles, zeros skipped along D and H (tail_rows16_k, vq_tail_rows.h); VQHIP_TAIL=slab selects conv_mfma32_k<OUTMODE 2> (depth only)
    int host_split = 8;      // host-memory calls of one chunk are cut into up to host_split pieces of >= host_split_min leaves (VQHIP_HOST_SPLIT=n[,min]; 1 = off)
    int64_t host_split_min = 8192;
    int tail16_tiles = 48;   // small-batch folded tail on the 16x16x4 MFMA up to this many tiles (VQHIP_TAIL16_TILES; measured: 1024 leaves 90 -> 56 us, 2048 leaves 92 -> 103 us)
    bool r64s_resident = true;   // small-batch 64->64 convs: their quarter of the weights LDS-resident (VQHIP_R64S=stream: streamed)
    int vq_split = 2;        // position ranges per tile in the VQ search of full chunks (VQHIP_VQ_SPLIT)
    bool conv8_w16 = true;   // ... with 16 waves (one half row each; a half row is a statistics block); VQHIP_CONV8=w8 selects 8 (one row each)
    bool convdown_lds = true;   // down conv of large passes: input planes streamed through LDS once, weights from L1 / L2 (vq_convdown_lds.h); VQHIP_DOWN=rows selects the row kernel (input re-fetched 3.06x)
    bool conv4_lds = true;   // 32-channel 4^3 convs of large passes: input planes in an LDS ring, weights straight from L1 / L2 (vq_conv4_lds.h); VQHIP_CONV4=rows selects the row kernel (weights LDS-resident, every input row re-fetched 6.25x)
    bool first_once = true;  // first conv of full chunks issued once, an 8-leaf group's output held in the accumulators of one workgroup (conv_first_once_k, vq_first_once.h); VQHIP_FIRST=twopass|steps|roll0 and VQHIP_FIRST_SRC=raw select the two-pass sequence below
    bool first_roll_stats = false;   // ... for the statistics pass too (VQHIP_FIRST=roll0; measured slower)
    bool first_raw = false;  // VQHIP_FIRST_SRC=raw: the first conv reads the caller's float[leaf][512] layout itself and pack_leaves_k is not launched (round 6; measured SLOWER: 0.425 + 0.465 ms against 0.069 + 0.322 + 0.396 ms with the row layout — 16 cache lines per load instead of 6)
    bool first_roll = true;  // first conv of large passes, normalising pass: rolling row window in registers (vq_first_roll.h); VQHIP_FIRST=steps selects conv_first_k ((row, kd) steps, nine row loads per output row)
    bool conv8_lds = true;   // 16-channel 8^3 convs of large passes: LDS-plane kernel (vq_conv8_lds.h); VQHIP_CONV8=rows selects the row-group kernel

    // full training step (vq_train_full.inc)
    bool train_gn_fused = true;      // GroupNorm + ReLU backward as one pass per layer (gn_bwd_fused_k); VQHIP_TRAIN_GNBWD=split: sums + finish + apply
    bool train_bias_main = true;     // bias gradients on the data-gradient stream when there is no reduction stream (VQHIP_TRAIN_BIAS=side: beside the weight gradients)
    bool train_red_stream = false;   // round 6, first attempt: bias sums, GroupNorm-affine / attention-weight reductions on a third stream (VQHIP_TRAIN_BIAS=third; fast or slow depending on the hardware queue the stream lands on)
    bool train_red_deferred = true;  // round 6: ... as two multi-job launches at the end of the data-gradient chain (csum_multi_k, reduce_multi_k); VQHIP_TRAIN_BIAS=main|side|third: the other arrangements
    bool train_ema_early = true;     // round 6: the codebook statistics start on the side stream as soon as the assignment exists, beside the decoder's forward (VQHIP_TRAIN_EMA_AT=backward: with the backward pass)
    bool train_side_stream = true;   // training backward: weight / bias gradients on a second stream beside the data-gradient chain (VQHIP_TRAIN_STREAMS=1: one stream)
    int train_side_prio = 0;         // ... that stream's queue priority against the data-gradient stream (the caller's): 0 a plain non-blocking stream, +1 / -1 the highest / lowest priority the device offers (VQHIP_TRAIN_SIDE_PRIO=high|low)
    bool train_red_queue_mask = true;   // the reduction stream's own hardware queue comes from a full CU mask at normal priority; VQHIP_TRAIN_RED_QUEUE=prio: from a high stream priority (side_stream, vq_train_full.inc)
    int train_red_prio = 0;          // reduction stream of a step: 0 by the batch (train_red_own_leaves), +1 always the one with its own queue, -1 always the shared one (VQHIP_TRAIN_RED_PRIO=own|normal)
    int64_t train_red_own_leaves = 2048;   // batches up to this size use ft_red (VQHIP_TRAIN_RED_OWN_LEAVES)
    bool train_r64_quarters = true;        // 64 -> 64 convs of small training batches in four cout quarters with resident weights (VQHIP_TRAIN_R64=whole: one workgroup per row)
    bool train_dgrad_small_lds = true;     // data gradients of the 4^3 layers with streamed weight windows (VQHIP_TRAIN_DGRAD=resident: LDS-resident weights)
    int train_wgrad_cu_pct = 100;          // wgrad_rows4_k: slices as a percentage of one-per-CU (VQHIP_TRAIN_WGRAD_CU_PCT)
    bool train_wgrad_rows = true;    // training backward: weight gradients of the k3 layers at 4^3 by wgrad_rows4_k (VQHIP_TRAIN_WGRAD=pairs: wgrad32_k)
    bool train_stem_lut = true;      // training forward: decoder stem through the (tap, code) table rebuilt every step (VQHIP_TRAIN_STEM=conv: the real conv)
    bool train_ema_lists = true;     // codebook statistics from per-(segment, code) member lists (vq_ema_lists_k + vq_ema_gather_k); VQHIP_TRAIN_EMA=scan: every (code, segment) wave scans the indices
    bool train_folded_tail = true;   // training step: up_conv + PixelShuffle3D + final as one folded operator (vq_train_tail.h); VQHIP_TRAIN_TAIL=unfolded keeps the layer-by-layer tail
};

namespace vqsw {

constexpr long NO_MAX = LONG_MAX;   // an integer range without an upper bound
constexpr long DEVICE_CUS = -1;     // ... whose upper bound is the device's compute-unit count

struct Word {
    const char* word = nullptr;
    void (*apply)(Switches&) = nullptr;   // what the word does to the defaults; null for the default's own name
};

// One switch.  Enumerated: words[] (default first).  Integer: words[] empty, the value in [lo, hi] goes to set (null: the value is
// only validated here, its reader is elsewhere).  An integer pair "n" or "n,m" has set2 too, m >= lo2.
struct Switch {
    const char* name;
    Word words[4];
    long lo, hi;
    void (*set)(Switches&, long);
    long lo2;
    void (*set2)(Switches&, long);
    const char* selects;
    const char* covered_by;   // tests/<file>::<function> that runs a non-default value, or ""
    bool is_integer() const { return words[0].word == nullptr; }
};

#define VQSW(stmt) [](Switches& s) { stmt; }
#define VQSW_INT(stmt) [](Switches& s, long v) { stmt; }
constexpr Switch SWITCHES[] = {
    {"VQHIP_CUS", {}, 1, DEVICE_CUS, VQSW_INT(s.n_cus = (int)v), 0, nullptr,
     "launch geometry as on a device with this many compute units (default: the device's count); masks no compute unit off",
     "tests/test_gpu_cu_counts.py::test_results_do_not_depend_on_the_count"},
    {"VQHIP_CONV8", {{"w16"}, {"w8", VQSW(s.conv8_w16 = false)}, {"rows", VQSW(s.conv8_lds = false)}}, 0, 0, nullptr, 0, nullptr,
     "16-channel 8^3 convs of full chunks: LDS-plane kernel with 16 waves / with 8 waves / row-group kernel",
     "tests/test_gpu_parity.py::test_large_path_kernel_variants_agree"},
    {"VQHIP_CONV4", {{"lds"}, {"rows", VQSW(s.conv4_lds = false)}}, 0, 0, nullptr, 0, nullptr,
     "32-channel 4^3 convs of full chunks: input planes in an LDS ring / row kernel with LDS-resident weights",
     "tests/test_gpu_parity.py::test_large_path_kernel_variants_agree"},
    {"VQHIP_DOWN", {{"lds"}, {"rows", VQSW(s.convdown_lds = false)}}, 0, 0, nullptr, 0, nullptr,
     "down conv of full chunks: input planes streamed through LDS once / row kernel",
     "tests/test_gpu_parity.py::test_large_path_kernel_variants_agree"},
    {"VQHIP_FIRST",
     {{"once"},
      {"twopass", VQSW(s.first_once = false)},
      {"steps", VQSW(s.first_once = false; s.first_roll = false)},
      {"roll0", VQSW(s.first_once = false; s.first_roll_stats = true)}},
     0, 0, nullptr, 0, nullptr,
     "first conv of full chunks: one pass (conv_first_once_k) / two passes with their default kernels / conv_first_k for both passes / the row window for both",
     "tests/test_gpu_parity.py::test_large_path_kernel_variants_agree"},
    {"VQHIP_FIRST_SRC", {{"packed"}, {"raw", VQSW(s.first_raw = true)}}, 0, 0, nullptr, 0, nullptr,
     "first conv reads the packed row layout / the caller's float[leaf][512] layout itself (two-pass sequence, no pack_leaves_k)",
     "tests/test_gpu_parity.py::test_large_path_kernel_variants_agree"},
    {"VQHIP_STEM", {{"taps"}, {"gather", VQSW(s.stem_taps = false)}, {"split", VQSW(s.stem_fused = false)}}, 0, 0, nullptr, 0, nullptr,
     "decoder front of large and mid-size passes: table streamed through an LDS ring (stem_taps_k) / gathered through the L1 (stem_fused_k) / gather and GroupNorm as two kernels",
     "tests/test_gpu_parity.py::test_large_path_kernel_variants_agree"},
    {"VQHIP_STEM_SMALL", {{"fused"}, {"split", VQSW(s.stem_small_fused = false)}}, 0, 0, nullptr, 0, nullptr,
     "decoder front of small-batch passes: one kernel (stem_fused_k) / gather, combine, normalise, combine",
     "tests/test_gpu_switches.py::test_stem_small_split_decodes_the_default_bits"},
    {"VQHIP_TAIL",
     {{"rows16"},
      {"rows32", VQSW(s.tail_rows32 = true)},
      {"groups", VQSW(s.tail_groups = true)},
      {"slab", VQSW(s.tail_rows = false)}},
     0, 0, nullptr, 0, nullptr,
     "folded decoder tail of full chunks: 16-voxel tiles (tail_rows16_k) / a 32-leaf tile per wave / output planes in three groups / the slab kernel (zeros skipped along depth only)",
     "tests/test_gpu_parity.py::test_large_path_kernel_variants_agree"},
    {"VQHIP_TAIL16_TILES", {}, 0, INT_MAX, VQSW_INT(s.tail16_tiles = (int)v), 0, nullptr,
     "small-batch folded tail on the 16x16x4 MFMA up to this many tiles (default 48)",
     "tests/test_gpu_parity.py::test_small_path_kernel_variants_agree"},
    {"VQHIP_R64S", {{"resident"}, {"stream", VQSW(s.r64s_resident = false)}}, 0, 0, nullptr, 0, nullptr,
     "small-batch 64->64 convs: their quarter of the weights LDS-resident / streamed",
     "tests/test_gpu_parity.py::test_small_path_kernel_variants_agree"},
    {"VQHIP_VQ_SPLIT", {}, 1, 64, VQSW_INT(s.vq_split = (int)v), 0, nullptr,
     "position ranges per tile in the VQ search of full chunks (default 2; a tile has 64 positions)", ""},
    {"VQHIP_HOST_SPLIT", {}, 1, INT_MAX, VQSW_INT(s.host_split = (int)v), 32, VQSW_INT(s.host_split_min = v),
     "host-memory calls of one chunk are cut into up to n pieces of at least min leaves (default 8,8192; 1 = off)",
     "tests/test_gpu_parity.py::test_large_one_chunk_host_calls_are_cut_into_pieces_without_changing_a_bit"},
    {"VQHIP_TRAIN_STEM", {{"lut"}, {"conv", VQSW(s.train_stem_lut = false)}}, 0, 0, nullptr, 0, nullptr,
     "training forward: decoder stem through the (tap, code) table rebuilt every step / the real conv", ""},
    {"VQHIP_TRAIN_WGRAD", {{"rows"}, {"pairs", VQSW(s.train_wgrad_rows = false)}}, 0, 0, nullptr, 0, nullptr,
     "training backward: weight gradients of the 4^3 layers by wgrad_rows4_k / by the pair-per-step kernel wgrad32_k",
     "tests/test_gpu_fulltrain.py::test_weight_gradient_kernel_families_agree"},
    {"VQHIP_TRAIN_STREAMS", {{"2"}, {"1", VQSW(s.train_side_stream = false)}}, 0, 0, nullptr, 0, nullptr,
     "training backward: weight / bias gradients on a second stream / everything on the step's own stream",
     "tests/test_gpu_fulltrain.py::test_side_stream_gives_the_single_stream_gradients_bit_for_bit"},
    {"VQHIP_TRAIN_GNBWD", {{"fused"}, {"split", VQSW(s.train_gn_fused = false)}}, 0, 0, nullptr, 0, nullptr,
     "GroupNorm + ReLU backward: one pass per layer / sums, finish, apply",
     "tests/test_gpu_fulltrain.py::test_groupnorm_backward_paths_agree"},
    {"VQHIP_TRAIN_BIAS",
     {{"deferred"},
      {"main", VQSW(s.train_red_deferred = false)},
      {"side", VQSW(s.train_red_deferred = false; s.train_bias_main = false)},
      {"third", VQSW(s.train_red_deferred = false; s.train_red_stream = true)}},
     0, 0, nullptr, 0, nullptr,
     "bias sums and small reductions: two multi-job launches at the end of the data-gradient chain / between the chain's kernels / beside the weight gradients / on a third stream",
     "tests/test_gpu_fulltrain.py::test_groupnorm_backward_paths_agree"},
    {"VQHIP_TRAIN_R64", {{"quarters"}, {"whole", VQSW(s.train_r64_quarters = false)}}, 0, 0, nullptr, 0, nullptr,
     "64->64 convs of small training batches: four cout quarters with resident weights / one workgroup per row",
     "tests/test_gpu_kernel_configs.py::test_training_conv_configurations_give_the_same_gradient_bits"},
    {"VQHIP_TRAIN_DGRAD", {{"streamed"}, {"resident", VQSW(s.train_dgrad_small_lds = false)}}, 0, 0, nullptr, 0, nullptr,
     "data gradients of the 4^3 layers: streamed weight windows / LDS-resident weights",
     "tests/test_gpu_kernel_configs.py::test_training_conv_configurations_give_the_same_gradient_bits"},
    {"VQHIP_TRAIN_WGRAD_CU_PCT", {}, 10, 100, VQSW_INT(s.train_wgrad_cu_pct = (int)v), 0, nullptr,
     "wgrad_rows4_k: slices as a percentage of one per compute unit (default 100)",
     "tests/test_gpu_cu_counts.py::test_gradients_against_fp64"},
    {"VQHIP_TRAIN_RED_OWN_LEAVES", {}, 0, NO_MAX, VQSW_INT(s.train_red_own_leaves = v), 0, nullptr,
     "VQHIP_TRAIN_BIAS=third: batches up to this many leaves use the reduction stream with its own queue (default 2048)", ""},
    {"VQHIP_TRAIN_EMA_AT", {{"forward"}, {"backward", VQSW(s.train_ema_early = false)}}, 0, 0, nullptr, 0, nullptr,
     "codebook statistics start beside the decoder's forward / with the backward pass",
     "tests/test_gpu_fulltrain.py::test_groupnorm_backward_paths_agree"},
    {"VQHIP_TRAIN_EMA", {{"lists"}, {"scan", VQSW(s.train_ema_lists = false)}}, 0, 0, nullptr, 0, nullptr,
     "codebook statistics from per-(segment, code) member lists / every (code, segment) wave scans the indices",
     "tests/test_gpu_training.py::test_statistics_kernels_agree"},
    {"VQHIP_TRAIN_TAIL", {{"folded"}, {"unfolded", VQSW(s.train_folded_tail = false)}}, 0, 0, nullptr, 0, nullptr,
     "training step: up_conv + PixelShuffle3D + final as one folded operator / layer by layer (the arrangement vqhip_fulltrain_set_folded_tail selects too, which is how the test reaches it)",
     "tests/test_gpu_fulltrain_edges.py::test_gradients_with_the_unfolded_tail"},
    {"VQHIP_TRAIN_SIDE_PRIO", {{"plain"}, {"high", VQSW(s.train_side_prio = 1)}, {"low", VQSW(s.train_side_prio = -1)}}, 0, 0, nullptr, 0, nullptr,
     "weight-gradient stream: a non-blocking stream without priority / the highest / the lowest queue priority", ""},
    {"VQHIP_TRAIN_RED_QUEUE", {{"mask"}, {"prio", VQSW(s.train_red_queue_mask = false)}}, 0, 0, nullptr, 0, nullptr,
     "VQHIP_TRAIN_BIAS=third: the reduction stream gets its own hardware queue from a full CU mask / from a high stream priority", ""},
    {"VQHIP_TRAIN_RED_PRIO", {{"auto"}, {"own", VQSW(s.train_red_prio = 1)}, {"normal", VQSW(s.train_red_prio = -1)}}, 0, 0, nullptr, 0, nullptr,
     "VQHIP_TRAIN_BIAS=third: reduction stream by the batch size (VQHIP_TRAIN_RED_OWN_LEAVES) / always the one with its own queue / always the shared one", ""},
    {"VQHIP_COPY_THREADS", {}, 1, INT_MAX, nullptr, 0, nullptr,
     "cap on the host gather / scatter threads of one calling thread; process-wide, read at the first host call (default 16, lowered per device by the multi-device front end)", ""},
};
#undef VQSW
#undef VQSW_INT

inline const Switch* find_switch(const char* name)
{
    for (const Switch& w : SWITCHES)
        if (std::strcmp(w.name, name) == 0) return &w;
    return nullptr;
}

// "a | b | c" for an enumerated switch, "integer in [lo, hi]" / "integer >= lo" for an integer one: the table's values column and
// the tail of the error messages
inline std::string legal_values(const Switch& w, int n_cus_device = 0)
{
    std::string t;
    if (!w.is_integer()) {
        for (const Word& x : w.words)
            if (x.word) t += (t.empty() ? "" : " | ") + std::string(x.word);
        return t;
    }
    auto range = [&](long lo, long hi) {
        if (hi == NO_MAX) return "integer >= " + std::to_string(lo);
        if (hi == DEVICE_CUS && n_cus_device <= 0) return "integer in [" + std::to_string(lo) + ", the device's compute units]";
        return "integer in [" + std::to_string(lo) + ", " + std::to_string(hi == DEVICE_CUS ? (long)n_cus_device : hi) + "]" +
               (hi == DEVICE_CUS ? " (the device's compute units)" : "");
    };
    t = range(w.lo, w.hi);
    if (w.set2) t = "n or n,min: n " + t + ", min integer >= " + std::to_string(w.lo2);
    return t;
}

// strict integer: all of [p, end) consumed by strtol, no leading white space, inside long and inside [lo, hi]
inline bool parse_integer(const char* p, const char* end, long lo, long hi, long& v)
{
    if (p == end || !(*p == '-' || *p == '+' || (*p >= '0' && *p <= '9'))) return false;
    const std::string text(p, end);   // (strtol wants a terminator at end)
    char* stop = nullptr;
    errno = 0;
    v = std::strtol(text.c_str(), &stop, 10);
    return !errno && stop == text.c_str() + text.size() && v >= lo && v <= hi;
}

// The value of one integer switch: out[0], and out[1] for the second number of a pair (n_out tells how many were given; 0 for an
// unset or empty value).  The one place where an integer switch's text is read.
inline int parse_switch_integers(const Switch& w, const char* text, int n_cus_device, long out[2], int& n_out, std::string& err)
{
    n_out = 0;
    if (!text || !*text) return VQHIP_OK;
    const char* end = text + std::strlen(text);
    const char* comma = w.set2 ? std::strchr(text, ',') : nullptr;
    const long hi = w.hi == DEVICE_CUS ? (long)n_cus_device : w.hi;
    bool ok = parse_integer(text, comma ? comma : end, w.lo, hi, out[0]);
    if (ok && comma) ok = parse_integer(comma + 1, end, w.lo2, NO_MAX, out[1]);
    if (!ok) {
        err = std::string(w.name) + "=" + text + ": not " + (w.set2 ? "" : "an ") + legal_values(w, n_cus_device);
        return VQHIP_ERR_INVALID;
    }
    n_out = comma ? 2 : 1;
    return VQHIP_OK;
}

}  // namespace vqsw

// Every switch from `lookup` (std::getenv in the library) into `s`: the defaults, n_cus = n_cus_device, then what each set variable
// selects.  VQHIP_OK, or VQHIP_ERR_INVALID with `err` written and `s` untouched.
inline int parse_switches(Switches& s, const char* (*lookup)(const char*), int n_cus_device, std::string& err)
{
    Switches t;
    t.n_cus = n_cus_device;
    for (const vqsw::Switch& w : vqsw::SWITCHES) {
        const char* text = lookup(w.name);
        if (!text || !*text) continue;
        if (w.is_integer()) {
            long v[2];
            int n = 0;
            if (int rc = vqsw::parse_switch_integers(w, text, n_cus_device, v, n, err)) return rc;
            if (w.set) w.set(t, v[0]);
            if (n == 2) w.set2(t, v[1]);
            continue;
        }
        const vqsw::Word* hit = nullptr;
        for (const vqsw::Word& x : w.words)
            if (x.word && std::strcmp(x.word, text) == 0) hit = &x;
        if (!hit) {
            err = std::string(w.name) + "=" + text + ": unknown value (" + vqsw::legal_values(w) + ")";
            return VQHIP_ERR_INVALID;
        }
        if (hit->apply) hit->apply(t);
    }
    s = t;
    return VQHIP_OK;
}
