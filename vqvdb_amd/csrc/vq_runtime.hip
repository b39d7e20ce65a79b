// vq_runtime.hip — host runtime and C ABI of libvqvdb_hip.so (include/vqvdb_hip.h).
//
// One vqhip_codec = one device context: fragment-ordered weights resident in HBM, a
// workspace of leaf-tile activations sized for one chunk of leaves, a compute stream and
// pinned staging buffers for the host-pointer entry points.  No PyTorch / ONNX / CPU
// fallback: if HIP is unavailable every entry point fails with VQHIP_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <array>
#include <cctype>
#include <cerrno>
#include <cstdlib>
#include <memory>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/vqvdb_hip.h"
#include "../../include/vqvdb_hip_bounded.h"
#include "../../include/vqvdb_hip_residual.h"
#include "../../include/vqvdb_hip_precision.h"
#include "../../include/vqvdb_hip_encode_mode.h"
#include "vq_buffers.h"
#include "vq_switches.h"
#include "vq_kernels.h"
#include "vq_conv8_lds.h"
#include "vq_stem_taps.h"
#include "vq_conv4_lds.h"
#include "vq_first_roll.h"
#include "vq_first_once.h"
#include "vq_convdown_lds.h"
#include "vq_train_kernels.h"
#include "vq_grad_kernels.h"
#include "vq_train_tail.h"
#include "vq_tail_rows.h"
#include "vq_tail_groups.h"
#include "vq_dec64_bf16.h"
#include "vq_enc16_bf16.h"

namespace {

thread_local std::string g_create_error = "";

struct PackTensor {
    std::vector<uint32_t> dims;
    const float* data = nullptr;
    size_t count = 0;
};

// Name -> value table with a cheap lookup: every launch resolves its ~45 buffers by name (a["e_a1"], w["r16c1.w"]); as
// std::map<std::string, ...> that was a heap of string constructions and tree walks per pass — measurable in the 0.14-0.2 ms
// calls of SOP-sized batches.  Open addressing over an FNV-1a hash of the characters, no allocation on lookup; entries keep
// their insertion order and their addresses' CONTENT stays put (values are only ever added), iteration yields .first / .second.
template <typename T>
struct NameMap {
    struct Ent {
        std::string first;
        T second;
    };
    NameMap() = default;
    NameMap(const NameMap&) = delete;              // (a copy would have capacity == size: the next insertion would look like an overflow)
    NameMap& operator=(const NameMap&) = delete;
    static constexpr size_t kMaxNames = 1024;   // (the largest table, the device-buffer names of a training handle, holds ~250)
    std::vector<Ent> ents;
    std::vector<int> slots;   // index into ents, -1 = empty; size is a power of two > 2 * ents.size()
    static uint32_t hash(const char* s)
    {
        uint32_t h = 2166136261u;
        for (; *s; ++s) h = (h ^ (unsigned char)*s) * 16777619u;
        return h;
    }
    int lookup(const char* s) const
    {
        if (slots.empty()) return -1;
        const uint32_t mask = (uint32_t)slots.size() - 1;
        for (uint32_t i = hash(s) & mask;; i = (i + 1) & mask) {
            const int e = slots[i];
            if (e < 0) return -1;
            if (ents[e].first == s) return e;
        }
    }
    void rehash()
    {
        size_t n = 64;
        while (n < 4 * ents.size()) n *= 2;
        slots.assign(n, -1);
        for (size_t e = 0; e < ents.size(); ++e) {
            uint32_t i = hash(ents[e].first.c_str()) & (uint32_t)(n - 1);
            while (slots[i] >= 0) i = (i + 1) & (uint32_t)(n - 1);
            slots[i] = (int)e;
        }
    }
    T& operator[](const char* s)
    {
        int e = lookup(s);
        if (e < 0) {
            // references handed out by operator[] must stay valid across later insertions (callers hold `auto& w = c->dw` and lambdas capture
            // it): the entries live in storage reserved once; a table that outgrows it is a programming error and stops loudly
            if (ents.capacity() == 0) ents.reserve(kMaxNames);
            if (ents.size() == ents.capacity()) {
                fprintf(stderr, "vqvdb_hip: NameMap overflow (%zu names) at '%s'\n", ents.size(), s);
                abort();
            }
            ents.push_back(Ent{s, T()});
            e = (int)ents.size() - 1;
            if (slots.size() < 4 * ents.size()) rehash();
            else {
                uint32_t i = hash(s) & (uint32_t)(slots.size() - 1);
                while (slots[i] >= 0) i = (i + 1) & (uint32_t)(slots.size() - 1);
                slots[i] = e;
            }
        }
        return ents[e].second;
    }
    T& operator[](const std::string& s) { return (*this)[s.c_str()]; }
    const Ent* find(const char* s) const { const int e = lookup(s); return e < 0 ? end() : &ents[e]; }
    const Ent* find(const std::string& s) const { return find(s.c_str()); }
    Ent* find(const char* s) { const int e = lookup(s); return e < 0 ? end() : &ents[e]; }
    Ent* find(const std::string& s) { return find(s.c_str()); }
    size_t count(const char* s) const { return lookup(s) >= 0; }
    size_t count(const std::string& s) const { return lookup(s.c_str()) >= 0; }
    Ent* begin() { return ents.data(); }
    Ent* end() { return ents.data() + ents.size(); }
    const Ent* begin() const { return ents.data(); }
    const Ent* end() const { return ents.data() + ents.size(); }
};

struct KernelTimer {
    std::string name;
    hipEvent_t start, stop;
    int64_t leaves;
};

struct KernelInfo {
    double flops, eff_flops;
};

// FLOPs per leaf of each compute kernel: {nominal, issued}.  nominal = dense count of the reference ops the
// kernel replaces (zero-padding taps included); issued = what the kernel really executes
// on the matrix pipe (padding taps skipped, folded/looked-up operators counted at their folded cost) — the
// honest utilisation numerator.
const std::map<std::string, KernelInfo>& kernel_info()
{
    static const std::map<std::string, KernelInfo> m = {
        {"enc_conv_first_stats", {0.0, 2.0 * 221184 * 0.7703}},   // recomputation: the op is counted once, on the second pass
        {"enc_conv_first_gn", {2.0 * 221184, 2.0 * 221184 * 0.7703}},
        {"enc_conv_first", {2.0 * 221184, 264.0 * 2048}},   // conv_first_once_k: 264 16x16x4 MFMAs per leaf (kd skipped at the border planes, kh issued in full)
        {"enc_res16_conv1", {2.0 * 3538944, 2.0 * 3538944 * 0.7703}},
        {"enc_res16_conv2", {2.0 * 3538944, 2.0 * 3538944 * 0.7703}},
        {"enc_res16_conv1_bf16", {2.0 * 3538944, 2.0 * 3538944 * 0.7703}},   // bf16 encode mode (vq_enc16_bf16.h): the same taps on the bf16 MFMA
        {"enc_res16_conv2_bf16", {2.0 * 3538944, 2.0 * 3538944 * 0.7703}},
        {"enc_down", {2.0 * 2097152, 2.0 * 2097152 * 0.669922}},
        {"enc_res32_conv1", {2.0 * 1769472, 2.0 * 1769472 * 0.578704}},
        {"enc_res32_conv2", {2.0 * 1769472, 2.0 * 1769472 * 0.578704}},
        {"enc_vq", {2.0 * (262144 + 2097152 + 512), 2.0 * (524288 + 512)}},  // attn + proj + VQ; projection folded into the search
        {"dec_stem", {0.0, 0.0}},
        {"dec_stem_gn", {0.0, 0.0}},  // table lookups: the 14.2 M MAC/leaf of the reference op are not executed (stem_lut_k)
        {"dec_res64_conv1", {2.0 * 7077888, 2.0 * 7077888 * 0.578704}},
        {"dec_res64_conv2", {2.0 * 7077888, 2.0 * 7077888 * 0.578704}},
        {"dec_res64_conv1_bf16", {2.0 * 7077888, 2.0 * 7077888 * 0.578704}},   // bf16 decode mode (vq_dec64_bf16.h): the same taps on the bf16 MFMA
        {"dec_res64_conv2_bf16", {2.0 * 7077888, 2.0 * 7077888 * 0.578704}},
        // folded up_conv+pixshuf+final: nominal = the reference ops' dense count; "effective" = the MACs the
        // folded map really needs (884 736/leaf); the kernel issues (160 steps x 4 + 64 steps x 2 cout tiles) x 32 voxels x 64
        // channels = 1 572 864 MAC/leaf (round 3: the MFMAs of a voxel plane against input planes it cannot depend on are skipped;
        // 224 steps x 128 x 64 = 1 835 008 before)
        {"dec_tail_slab", {2.0 * (28311552 + 2048 + 442368), 2.0 * 1572864}},
        // round 5 (tail_rows16_k): 16-voxel tiles of two (od,oh) cells with one reach box: the structural zeros are skipped along D and H,
        // 296 (tile, input row) pairs x 64 MFMAs of 1024 MACs per 16 leaves = 1 212 416 MAC/leaf (exact D x H: 1 179 648; useful 884 736)
        {"dec_tail", {2.0 * (28311552 + 2048 + 442368), 2.0 * 1212416}},
        {"dec_tail_rows32", {2.0 * (28311552 + 2048 + 442368), 2.0 * 1212416}},   // the same tiles, a whole 32-leaf tile per wave
        {"dec_tail_groups", {2.0 * (28311552 + 2048 + 442368), 2.0 * 1212416}},   // the same (tile, input row) pairs in three plane groups
    };
    return m;
}

}  // namespace

struct vqhip_codec : Switches {   // the switch-controlled fields (n_cus, conv8_lds, train_* ...): vq_switches.h
    int device = 0;
    std::string err;
    hipStream_t stream = nullptr;
    int64_t chunk = 65536;
    int n_cus_device = 256;  // compute units of the device itself (CU mask of the reduction stream)
    int split_tiles = -1;    // position-split path: -1 = automatic (measured crossovers, use_split), >= 0 = plain tile threshold

    // device weights
    NameMap<float*> dw;
    NameMap<int> nsteps;
    float e_final_bias = 0.0f;

    // workspace
    int64_t ws_tiles = 0;
    bool ws_full = false;    // workspace layout: full (every activation at its own address: debug, training) or compact (inference)
    bool chunk_fitted = false;
    DevBuf<char> ws;
    NameMap<float*> act;  // named activation buffers inside ws
    NameMap<std::pair<int, int>> act_shape;

    // host-pointer entry points: two I/O slots so H2D(i+1), compute(i) and D2H(i-1) overlap
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    PinBuf<unsigned char> pin_out[2];   // pinned landing zone for results (chunk * 2048 B each)
    PinBuf<unsigned char> pin_in[2];    // pinned gather buffers of the leaf-pointer entry points
    DevBuf<float> dev_leaves[2];        // chunk * 512 floats
    DevBuf<uint8_t> dev_idx[2];         // chunk * 64 bytes

    // profiling
    bool profiling = false;
    std::vector<KernelTimer> timers;

    bool debug = false;

    // codebook training (vqhip_train_*): host copies of what the inference tables are rebuilt from, live state flag,
    // latent / index scratch for one training batch
    std::vector<float> h_proj_w, h_proj_b;
    bool training = false, tables_stale = false;
    DevBuf<float> tr_z;
    DevBuf<uint8_t> tr_idx;
    // full training step (vq_train_full.inc)
    std::vector<float> h_params;                                   // raw tensors, state_dict order
    std::map<std::string, std::pair<int64_t, int64_t>> p_off;      // name -> (offset, count) in the flat parameter vector
    DevBuf<float> ft_P, ft_M, ft_V;                                // parameters, AdamW moments (device, flat)
    DevBuf<unsigned char> ft_refrag_jobs;                          // device job table of refrag_multi_k (vq_train_full.inc: refrag_all)
    int ft_refrag_n = 0, ft_refrag_wgs = 0;
    const void* ft_refrag_P = nullptr;                              // the parameter block the cached job table points into
    DevBuf<char> ft_ws;                                            // training workspace (saved activations, gradients)
    int64_t ft_tiles = 0;                                          // ... laid out for this many tiles
    DevBuf<char> ft_part;                                          // partial-gradient scratch
    bool full_training = false, weights_stale = false;
    hipStream_t ft_side = nullptr;
    hipStream_t ft_red_shared = nullptr;   // ... the same on a plain stream (shares a hardware queue with the weight-gradient stream): large batches
    bool ft_egate_early = false;           // this step's encoder attention gates were computed beside the forward pass
    hipStream_t ft_red = nullptr;    // third stream of the training step (round 6): the small reductions nothing on the data-gradient chain waits for (bias sums, GroupNorm-affine and attention-weight reductions)
    std::vector<hipEvent_t> ft_ev;   // fork / join events of the side stream, reused every step
    size_t ft_ev_next = 0;
    DevBuf<char> tr_part;      // per-(code, row segment) partial statistics
    DevBuf<float> tr_recon;    // reconstruction scratch of vqhip_train_eval_device
    DevBuf<double> tr_loss_part;
    // error-bounded calls (vq_bounded.inc)
    DevBuf<float> bd_recon;        // a chunk's reconstruction when the caller wants none stored
    DevBuf<uint8_t> bd_idx;        // a chunk's indices when the caller wants none
    DevBuf<float> bd_err[2];       // leaf errors of the host calls, one per I/O slot ...
    PinBuf<float> bd_pin_err[2];   // ... and their pinned landing zones
    DevBuf<int64_t> bd_ids;        // outlier ids of one chunk, the count behind them
    DevBuf<int64_t> bd_scan;       // block counts / offsets of the selection
    // quantised residuals (vq_residual.inc): one set per I/O slot
    DevBuf<uint8_t> rs_class[2];
    DevBuf<int64_t> rs_off[2];
    DevBuf<uint8_t> rs_payload[2];
    PinBuf<unsigned char> rs_pin[2];   // the file pair's pinned block: total, offsets, payload, classes ...
    int64_t rs_pin_leaves = 0;         // ... whose sections are positioned for this many leaves
    // size sweep (vq_rate.inc): the histogram [64][19] of the host calls
    DevBuf<int64_t> rate_hist;
    // bf16 decode mode (vqvdb_hip_precision.h): the mode of the plain decode calls, the bf16 A fragments of the two 64 -> 64
    // convs (grown at the first switch), and whether the fp32 fragments they are packed from have changed since (training)
    int decode_precision = VQHIP_PRECISION_FP32;
    DevBuf<uint16_t> bf_r64c1, bf_r64c2;
    bool bf_stale = true;
    // bf16 encode mode (vqvdb_hip_encode_mode.h): the mode of the plain encode calls, the bf16 A fragments of the two 16 -> 16
    // convs (grown at the first switch), and whether the fp32 fragments they are packed from have changed since (training)
    int encode_precision = VQHIP_PRECISION_FP32;
    DevBuf<uint16_t> bf_r16c1, bf_r16c2;
    bool bf_enc_stale = true;
};

namespace {

#define HIPCHK(c, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            (void)hipGetLastError(); /* the slot is sticky until read: do not let it fail the next launch check */ \
            (c)->err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
            return VQHIP_ERR_DEVICE;                                                            \
        }                                                                                       \
    } while (0)

int fail(vqhip_codec* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

// ---------------- weight pack (vqvdb_amd/weightpack.py) ----------------
bool parse_pack(const unsigned char* p, size_t n, std::map<std::string, PackTensor>& out, std::string& err)
{
    if (n < 16 || std::memcmp(p, "VQWPACK1", 8) != 0) {
        err = "weight pack: bad magic (expected VQWPACK1)";
        return false;
    }
    uint32_t nt;
    std::memcpy(&nt, p + 8, 4);
    const size_t ent = 108;
    if (16 + (size_t)nt * ent > n) {
        err = "weight pack: truncated table";
        return false;
    }
    for (uint32_t i = 0; i < nt; ++i) {
        const unsigned char* e = p + 16 + (size_t)i * ent;
        char name[65];
        std::memcpy(name, e, 64);
        name[64] = 0;
        uint32_t ndim, dims[6];
        uint64_t off, cnt;
        std::memcpy(&ndim, e + 64, 4);
        std::memcpy(dims, e + 68, 24);
        std::memcpy(&off, e + 92, 8);
        std::memcpy(&cnt, e + 100, 8);
        // overflow-safe bounds: off and cnt come from the (user-supplied) file
        if (ndim > 6 || (off & 3) || off > n || cnt > (n - off) / 4) {
            err = std::string("weight pack: tensor '") + name + "' out of bounds";
            return false;
        }
        uint64_t prod = 1;
        for (uint32_t d = 0; d < ndim; ++d) {
            if (dims[d] != 0 && prod > UINT64_MAX / dims[d]) prod = UINT64_MAX;
            else prod *= dims[d];
        }
        if (prod != cnt) {   // every consumer reads prod(dims) floats from the tensor
            err = std::string("weight pack: tensor '") + name + "' count does not match its shape";
            return false;
        }
        PackTensor t;
        t.dims.assign(dims, dims + ndim);
        t.data = reinterpret_cast<const float*>(p + off);
        t.count = cnt;
        out[name] = t;
    }
    return true;
}

const PackTensor* need(const std::map<std::string, PackTensor>& pk, const char* name, std::initializer_list<uint32_t> dims, std::string& err)
{
    auto it = pk.find(name);
    if (it == pk.end()) {
        err = std::string("weight pack: missing tensor '") + name + "'";
        return nullptr;
    }
    if (it->second.dims != std::vector<uint32_t>(dims)) {
        err = std::string("weight pack: tensor '") + name + "' has unexpected shape";
        return nullptr;
    }
    return &it->second;
}

// ---------------- fragment repacks (host, once at create) ----------------
// 32x32x2 A-fragments: [tap][u][mt][lane][i] = W[cout = 32mt + (lane&31)][cin = 8u + 4(lane>>5) + i][tap]
std::vector<float> frag32(const float* W, int COUT, int CIN, int KT)
{
    const int NU = CIN / 8, NMT = COUT / 32;
    std::vector<float> f((size_t)KT * NU * NMT * 64 * 4);
    for (int tap = 0; tap < KT; ++tap)
        for (int u = 0; u < NU; ++u)
            for (int mt = 0; mt < NMT; ++mt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < 4; ++i) {
                        const int co = 32 * mt + (lane & 31), ci = 8 * u + 4 * (lane >> 5) + i;
                        f[((((size_t)tap * NU + u) * NMT + mt) * 64 + lane) * 4 + i] = W[((size_t)co * CIN + ci) * KT + tap];
                    }
    return f;
}
// D-fragment order of a per-cout vector: [(mt*2+q)*16 + r] = v[32mt + (r&3) + 8(r>>2) + 4q]
std::vector<float> dfrag32(const float* v, int COUT)
{
    std::vector<float> f(COUT);
    for (int mt = 0; mt < COUT / 32; ++mt)
        for (int q = 0; q < 2; ++q)
            for (int r = 0; r < 16; ++r) f[(mt * 2 + q) * 16 + r] = v[32 * mt + (r & 3) + 8 * (r >> 2) + 4 * q];
    return f;
}
// 16x16x4 A-fragments for Cin = Cout = 16: [tap][lane][i] = W[cout = lane&15][cin = 4(lane>>4) + i][tap]
std::vector<float> frag16(const float* W, int KT)
{
    std::vector<float> f((size_t)KT * 64 * 4);
    for (int tap = 0; tap < KT; ++tap)
        for (int lane = 0; lane < 64; ++lane)
            for (int i = 0; i < 4; ++i) f[((size_t)tap * 64 + lane) * 4 + i] = W[((size_t)(lane & 15) * 16 + 4 * (lane >> 4) + i) * KT + tap];
    return f;
}
// 16x16x4 A-fragments of conv_rows16_k: [tap][cb][mt][lane][i] = W[16mt + (lane&15)][16cb + 4(lane>>4) + i][tap]
std::vector<float> frag16g(const float* W, int COUT, int CIN, int KT)
{
    const int CBN = CIN / 16, MTN = COUT / 16;
    std::vector<float> f((size_t)KT * CBN * MTN * 64 * 4);
    for (int tap = 0; tap < KT; ++tap)
        for (int cb = 0; cb < CBN; ++cb)
            for (int mt = 0; mt < MTN; ++mt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < 4; ++i)
                        f[((((size_t)tap * CBN + cb) * MTN + mt) * 64 + lane) * 4 + i] =
                            W[((size_t)(16 * mt + (lane & 15)) * CIN + 16 * cb + 4 * (lane >> 4) + i) * KT + tap];
    return f;
}
// first conv: [(kd*3+kh)][lane] = W[cout = lane&15][0][kd][kh][kw = lane>>4] (0 for the pad slot)
std::vector<float> frag_first(const float* W)
{
    std::vector<float> f(9 * 64);
    for (int t = 0; t < 9; ++t)
        for (int lane = 0; lane < 64; ++lane) {
            const int kw = lane >> 4;
            f[t * 64 + lane] = kw < 3 ? W[(lane & 15) * 27 + t * 3 + kw] : 0.0f;
        }
    return f;
}

// Flattened (output, valid tap) schedules (StepEnt, vq_kernels.h).  Zero-padding taps never enter
// the table; taps appear in ascending (kd,kh,kw) order per output (arithmetic contract).
std::vector<int> steps_conv(int SI, int SO, int KS, int STRIDE, int PAD, int KWG)
{
    std::vector<int> t;
    for (int od = 0; od < SO; ++od)
        for (int oh = 0; oh < SO; ++oh)
            for (int ow = 0; ow < SO; ++ow) {
                const size_t first = t.size();
                for (int kd = 0; kd < KS; ++kd)
                    for (int kh = 0; kh < KS; ++kh) {
                        const int id = od * STRIDE - PAD + kd, ih = oh * STRIDE - PAD + kh;
                        if (id < 0 || id >= SI || ih < 0 || ih >= SI) continue;
                        int run = 0;  // valid taps along kw are contiguous in input position and tap index
                        for (int kw = 0; kw < KS; ++kw) {
                            const int iw = ow * STRIDE - PAD + kw;
                            if (iw < 0 || iw >= SI) continue;
                            if (run == 0 || run == KWG) {
                                t.insert(t.end(), {(id * SI + ih) * SI + iw, (kd * KS + kh) * KS + kw, (od * SO + oh) * SO + ow, 0});
                                run = 0;
                            }
                            ++run;
                            t[t.size() - 1] = (t[t.size() - 1] & 0xff) | (run << 8);
                        }
                    }
                t[first + 3] |= 1;
                t[t.size() - 1] |= 2;
            }
    return t;
}
// row schedule for conv_rows16_k: one step = (output row (od,oh) of SO positions, valid (kd,kh));
// x = input row base position, y = first tap (kw = 0) of the (kd,kh) run, z = output row base
std::vector<int> steps_rows(int SI, int SO, int KS, int STRIDE, int PAD)
{
    std::vector<int> t;
    for (int od = 0; od < SO; ++od)
        for (int oh = 0; oh < SO; ++oh) {
            const size_t first = t.size();
            for (int kd = 0; kd < KS; ++kd)
                for (int kh = 0; kh < KS; ++kh) {
                    const int id = od * STRIDE - PAD + kd, ih = oh * STRIDE - PAD + kh;
                    if (id < 0 || id >= SI || ih < 0 || ih >= SI) continue;
                    t.insert(t.end(), {(id * SI + ih) * SI, (kd * KS + kh) * KS, (od * SO + oh) * SO, 1 << 8});
                }
            t[first + 3] |= 1;
            t[t.size() - 1] |= 2;
        }
    return t;
}

// conv8_c16_k<NR>: one step = (od, output row group oh0 = NR*g, valid kd, input row ih in [oh0-1, oh0+NR]);
// w bits 8+4*rw.. = kh+1 of output row oh0+rw (0 = that row is not fed by this input row)
std::vector<int> steps_rowgroups8(int NR)
{
    std::vector<int> t;
    for (int od = 0; od < 8; ++od) {
        for (int g = 0; g < 8 / NR; ++g) {
            const int oh0 = NR * g;
            const size_t first = t.size();
            for (int kd = 0; kd < 3; ++kd) {
                const int id = od + kd - 1;
                if (id < 0 || id > 7) continue;
                for (int ih = oh0 - 1; ih <= oh0 + NR; ++ih) {
                    if (ih < 0 || ih > 7) continue;
                    int feeds = 0;
                    for (int rw = 0; rw < NR; ++rw) {
                        const int kh = ih - (oh0 + rw) + 1;
                        if (kh >= 0 && kh <= 2) feeds |= (kh + 1) << (8 + 4 * rw);
                    }
                    t.insert(t.end(), {(id * 8 + ih) * 8, kd * 3, (od * 8 + oh0) * 8, feeds});
                }
            }
            t[first + 3] |= 1;
            t[t.size() - 1] |= 2;
        }
    }
    return t;
}

// first conv: one step = (output row, valid kd); kh validity as a 3-bit mask
std::vector<int> steps_rows8_kd()
{
    std::vector<int> t;
    for (int od = 0; od < 8; ++od)
        for (int oh = 0; oh < 8; ++oh) {
            const size_t first = t.size();
            for (int kd = 0; kd < 3; ++kd) {
                const int id = od + kd - 1;
                if (id < 0 || id > 7) continue;
                int mask = 0;
                for (int kh = 0; kh < 3; ++kh)
                    if (oh + kh - 1 >= 0 && oh + kh - 1 <= 7) mask |= 1 << kh;
                t.insert(t.end(), {(id * 8 + oh) * 8, kd, (od * 8 + oh) * 8, mask << 8});
            }
            t[first + 3] |= 1;
            t[t.size() - 1] |= 2;
        }
    return t;
}

int upload_i(vqhip_codec* c, const char* name, const std::vector<int>& v)
{
    int* d = nullptr;
    HIPCHK(c, hipMalloc(&d, v.size() * sizeof(int)));
    HIPCHK(c, hipMemcpy(d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    c->dw[name] = reinterpret_cast<float*>(d);
    c->nsteps[name] = (int)(v.size() / 4);
    return VQHIP_OK;
}

// schedule + index of the first step of every output group (first-flagged steps), for position-split launches
int upload_steps(vqhip_codec* c, const std::string& name, const std::vector<int>& t)
{
    int rc = upload_i(c, name.c_str(), t);
    if (rc) return rc;
    std::vector<int> g;
    for (size_t i = 0; i < t.size() / 4; ++i)
        if (t[4 * i + 3] & 1) g.push_back((int)i);
    g.push_back((int)(t.size() / 4));
    while (g.size() % 4) g.push_back(g.back());  // upload_i counts int4 entries
    const int n_steps = c->nsteps[name];
    rc = upload_i(c, (name + ".grp").c_str(), g);
    c->nsteps[name] = n_steps;
    return rc;
}

int upload(vqhip_codec* c, const char* name, const std::vector<float>& v)
{
    float* d = nullptr;
    auto it = c->dw.find(name);
    if (it != c->dw.end()) {  // refresh of a derived table (same size by construction)
        HIPCHK(c, hipMemcpy(it->second, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
        return VQHIP_OK;
    }
    HIPCHK(c, hipMalloc(&d, v.size() * sizeof(float)));
    HIPCHK(c, hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    c->dw[name] = d;
    return VQHIP_OK;
}
int upload(vqhip_codec* c, const char* name, const PackTensor* t)
{
    return upload(c, name, std::vector<float>(t->data, t->data + t->count));
}

// Projection folded into the codebook (contract: oracle vqfold_build): Ep = E P in fp64 (j ascending),
// h_k = sum b e - (sum e^2) / 2, both rounded to fp32 once.  E = codebook [256][128] on the host.
int build_vq_fold(vqhip_codec* c, const float* E)
{
    std::vector<float> ep(256 * 32), ck(256);
    const float* P = c->h_proj_w.data();  // [128][32]
    const float* pb = c->h_proj_b.data();
    for (int k = 0; k < 256; ++k) {
        for (int ch = 0; ch < 32; ++ch) {
            double acc = 0.0;
            for (int jx = 0; jx < 128; ++jx) acc = __builtin_fma((double)E[k * 128 + jx], (double)P[jx * 32 + ch], acc);
            ep[k * 32 + ch] = (float)acc;
        }
        double cc = 0.0, bb = 0.0;
        for (int jx = 0; jx < 128; ++jx) {
            cc = __builtin_fma((double)E[k * 128 + jx], (double)E[k * 128 + jx], cc);
            bb = __builtin_fma((double)pb[jx], (double)E[k * 128 + jx], bb);
        }
        ck[k] = (float)(bb - 0.5 * cc);   // h_k = -c_k / 2: where the score chain of code k starts (oracle vqfold_build)
    }
    int rc;
    if ((rc = upload(c, "vq.ep", frag32(ep.data(), 256, 32, 1)))) return rc;
    return upload(c, "vq.ck", dfrag32(ck.data(), 256));
}

// Folded decoder tail: up_conv (64->256,k3 @4^3) -> PixelShuffle3D(2) -> final (32->1,k3 @8^3) is one
// linear map (no nonlinearity in between, VQVAE_v2.py:274-275).  Composite weights per output voxel,
// built in fp64 in the contract's order (see oracle tail_build) and rounded to fp32 once; laid out as
// MFMA A-fragments per (output slab d, input position p) with the 128 voxels of the slab as rows.
int build_folded_tail(vqhip_codec* c, const float* Wu, const float* bu, const float* Wf, const float* bf)
{
    std::vector<double> G((size_t)27 * 8 * 27 * 64);
    double Bg[27][8];
    for (int dl = 0; dl < 27; ++dl)
        for (int sb = 0; sb < 8; ++sb) {
            double b = 0.0;
            for (int oc = 0; oc < 32; ++oc) b = __builtin_fma((double)Wf[oc * 27 + dl], (double)bu[oc * 8 + sb], b);
            Bg[dl][sb] = b;
            for (int t = 0; t < 27; ++t)
                for (int ci = 0; ci < 64; ++ci) {
                    double a = 0.0;
                    for (int oc = 0; oc < 32; ++oc)
                        a = __builtin_fma((double)Wf[oc * 27 + dl], (double)Wu[((size_t)(oc * 8 + sb) * 64 + ci) * 27 + t], a);
                    G[(((size_t)dl * 8 + sb) * 27 + t) * 64 + ci] = a;
                }
        }
    std::vector<float> wc((size_t)512 * 64 * 64), bc(512);
    std::vector<double> acc(64 * 64);
    for (int od = 0; od < 8; ++od)
        for (int oh = 0; oh < 8; ++oh)
            for (int ow = 0; ow < 8; ++ow) {
                const int ov = (od * 8 + oh) * 8 + ow;
                double b = (double)bf[0];
                std::fill(acc.begin(), acc.end(), 0.0);
                for (int dd = 0; dd < 3; ++dd)
                    for (int dh = 0; dh < 3; ++dh)
                        for (int dw = 0; dw < 3; ++dw) {
                            const int zd = od + dd - 1, zh = oh + dh - 1, zw = ow + dw - 1;
                            if (zd < 0 || zd > 7 || zh < 0 || zh > 7 || zw < 0 || zw > 7) continue;
                            const int dl = (dd * 3 + dh) * 3 + dw;
                            const int cd = zd >> 1, ch = zh >> 1, cw = zw >> 1, sb = (zd & 1) * 4 + (zh & 1) * 2 + (zw & 1);
                            b = b + Bg[dl][sb];
                            for (int td = 0; td < 3; ++td)
                                for (int th = 0; th < 3; ++th)
                                    for (int tw = 0; tw < 3; ++tw) {
                                        const int pd = cd + td - 1, ph = ch + th - 1, pw = cw + tw - 1;
                                        if (pd < 0 || pd > 3 || ph < 0 || ph > 3 || pw < 0 || pw > 3) continue;
                                        const double* g = &G[(((size_t)dl * 8 + sb) * 27 + (td * 3 + th) * 3 + tw) * 64];
                                        double* a = &acc[(size_t)((pd * 4 + ph) * 4 + pw) * 64];
                                        for (int ci = 0; ci < 64; ++ci) a[ci] = a[ci] + g[ci];
                                    }
                        }
                bc[ov] = (float)b;
                for (int i = 0; i < 64 * 64; ++i) wc[(size_t)ov * 4096 + i] = (float)acc[i];
            }
    // fragments + schedule: slab d visits positions pd in [max(0,d-2), min(3,d+2)] x all (ph,pw), ascending
    std::vector<float> frags, bias;
    std::vector<int> steps;
    std::vector<float> wslab((size_t)128 * 64);
    for (int d = 0; d < 4; ++d) {
        const size_t first = steps.size();
        for (int p = std::max(0, d - 2) * 16; p < (std::min(3, d + 2) + 1) * 16; ++p) {
            for (int row = 0; row < 128; ++row)
                for (int ci = 0; ci < 64; ++ci) wslab[(size_t)row * 64 + ci] = wc[((size_t)(d * 128 + row) * 64 + p) * 64 + ci];
            const std::vector<float> f = frag32(wslab.data(), 128, 64, 1);
            steps.insert(steps.end(), {p, (int)(frags.size() / f.size()), d, 1 << 8});
            frags.insert(frags.end(), f.begin(), f.end());
        }
        steps[first + 3] |= 1;
        steps[steps.size() - 1] |= 2;
        const std::vector<float> bfrag = dfrag32(bc.data() + d * 128, 128);
        bias.insert(bias.end(), bfrag.begin(), bfrag.end());
    }
    // the same operator as 16x16x4 fragments for the smallest batches (tail_small16_k): [step][voxel block 8][uu 4][lane][e]
    std::vector<float> frags16((size_t)224 * 8 * 4 * 64 * 4);
    {
        size_t step = 0;
        for (int d = 0; d < 4; ++d)
            for (int p = std::max(0, d - 2) * 16; p < (std::min(3, d + 2) + 1) * 16; ++p, ++step)
                for (int mb = 0; mb < 8; ++mb)
                    for (int uu = 0; uu < 4; ++uu)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int e = 0; e < 4; ++e) {
                                const int u = 2 * uu + (e >> 1), mf = e & 1, m = lane & 15, k = lane >> 4;
                                const int ch = 8 * u + 4 * (k & 1) + (k >> 1) + 2 * mf;
                                frags16[((((step * 8 + mb) * 4 + uu) * 64) + lane) * 4 + e] = wc[((size_t)(d * 128 + 16 * mb + m) * 64 + p) * 64 + ch];
                            }
    }
    // ... and as the weight stream of tail_rows16_k (vq_tail_rows.h): one 32 KB slice per phase (unit, pd, ph, pw) in the order the
    // kernel walks them, a slice = the 4 KB blocks [uu 4][lane][e] of the tiles that input row feeds, dense, ascending tile id
    std::vector<float> wrows((size_t)TR_STREAM_SLICES * (TR_SLICE / 4), 0.0f);   // (padded: the kernel requests slices three phases ahead)
    {
        size_t t = 0, tile_rows = 0;
        for (int unit = 0; unit < 5; ++unit) {
            const bool pair = unit >= 1 && unit <= 3;
            const int od0 = unit == 0 ? 0 : unit == 4 ? 7 : 2 * unit - 1;
            for (int pd = tr_lo(od0); pd <= tr_hi(od0); ++pd)
                for (int ph = 0; ph < 4; ++ph) {
                    const unsigned mask = tr_mask(pair, ph);
                    tile_rows += tr_popc(mask);
                    for (int pw = 0; pw < 4; ++pw, ++t) {
                        const int p = (pd * 4 + ph) * 4 + pw;
                        for (int i = 0; i < tr_popc(mask); ++i) {
                            const int tid = tr_nth(mask, i), ca = tr_cell_a(pair, od0, tid), cb = tr_cell_b(pair, od0, tid);
                            float* blk = &wrows[t * (TR_SLICE / 4) + (size_t)i * 1024];
                            for (int uu = 0; uu < 4; ++uu)
                                for (int lane = 0; lane < 64; ++lane)
                                    for (int e = 0; e < 4; ++e) {
                                        const int u = 2 * uu + (e >> 1), mf = e & 1, m = lane & 15, k = lane >> 4;
                                        const int ch = 8 * u + 4 * (k & 1) + (k >> 1) + 2 * mf;
                                        const int vox = (m < 8 ? ca : cb) * 8 + (m & 7);
                                        blk[(uu * 64 + lane) * 4 + e] = wc[((size_t)vox * 64 + p) * 64 + ch];
                                    }
                        }
                    }
                }
        }
        if (t != TR_PHASES || tile_rows != TR_TILE_ROWS) return fail(c, VQHIP_ERR_MODEL, "folded tail: row schedule does not match tail_rows16_k");
    }
    // ... and of tail_groups16_k (vq_tail_groups.h): three groups of output planes, 48 KB slices of up to 11 blocks (pair tiles, then the
    // group's single tiles while their planes last)
    // (built and uploaded only when VQHIP_TAIL=groups selects that kernel: 7.8 MB of host work per weight refresh otherwise spent for nothing)
    std::vector<float> wgroups;
    if (c->tail_groups) {
        wgroups.assign((size_t)TG_STREAM_SLICES * (TG_SLICE / 4), 0.0f);
        size_t t = 0, tile_rows = 0;
        for (int g = 0; g < 3; ++g)
            for (int pd = tg_pd_lo(g); pd <= tg_pd_hi(g); ++pd)
                for (int ph = 0; ph < 4; ++ph) {
                    const unsigned mask = tg_mask(tg_with_single(g, pd), ph);
                    tile_rows += tr_popc(mask);
                    for (int pw = 0; pw < 4; ++pw, ++t) {
                        const int p = (pd * 4 + ph) * 4 + pw;
                        for (int i = 0; i < tr_popc(mask); ++i) {
                            const int tid = tr_nth(mask, i), ca = tg_cell_a(g, tid), cb = tg_cell_b(g, tid);
                            float* blk = &wgroups[t * (TG_SLICE / 4) + (size_t)i * 1024];
                            for (int uu = 0; uu < 4; ++uu)
                                for (int lane = 0; lane < 64; ++lane)
                                    for (int e = 0; e < 4; ++e) {
                                        const int u = 2 * uu + (e >> 1), mf = e & 1, m = lane & 15, k = lane >> 4;
                                        const int ch = 8 * u + 4 * (k & 1) + (k >> 1) + 2 * mf;
                                        const int vox = (m < 8 ? ca : cb) * 8 + (m & 7);
                                        blk[(uu * 64 + lane) * 4 + e] = wc[((size_t)vox * 64 + p) * 64 + ch];
                                    }
                        }
                    }
                }
        if (t != TG_PHASES || tile_rows != TR_TILE_ROWS) return fail(c, VQHIP_ERR_MODEL, "folded tail: group schedule does not match tail_groups16_k");
    }
    int rc;
    if (c->tail_groups && (rc = upload(c, "tail.wgroups", wgroups))) return rc;
    if ((rc = upload(c, "tail.wrows", wrows))) return rc;
    if ((rc = upload(c, "tail.w", frags))) return rc;
    if ((rc = upload(c, "tail.b", bias))) return rc;
    if ((rc = upload(c, "tail.w16", frags16))) return rc;
    if ((rc = upload(c, "tail.braw", bc))) return rc;
    return c->dw.count("steps.tail") ? VQHIP_OK : upload_steps(c, "steps.tail", steps);  // the schedule does not depend on the weights
}

// the 44 trainable tensors in the reference's parameter order (model.parameters(), python/VQVAE_v2.py)
const char* const kTrainable[] = {
    "encoder.pre.0.weight", "encoder.pre.0.bias", "encoder.pre.1.weight", "encoder.pre.1.bias",
    "encoder.pre.3.gn1.weight", "encoder.pre.3.gn1.bias", "encoder.pre.3.conv1.weight", "encoder.pre.3.conv1.bias",
    "encoder.pre.3.gn2.weight", "encoder.pre.3.gn2.bias", "encoder.pre.3.conv2.weight", "encoder.pre.3.conv2.bias",
    "encoder.down.weight", "encoder.down.bias",
    "encoder.res_stack.0.gn1.weight", "encoder.res_stack.0.gn1.bias", "encoder.res_stack.0.conv1.weight", "encoder.res_stack.0.conv1.bias",
    "encoder.res_stack.0.gn2.weight", "encoder.res_stack.0.gn2.bias", "encoder.res_stack.0.conv2.weight", "encoder.res_stack.0.conv2.bias",
    "encoder.attn.fc.0.weight", "encoder.attn.fc.2.weight", "encoder.proj.weight", "encoder.proj.bias",
    "decoder.stem.0.weight", "decoder.stem.0.bias", "decoder.stem.1.weight", "decoder.stem.1.bias",
    "decoder.res_stack.0.gn1.weight", "decoder.res_stack.0.gn1.bias", "decoder.res_stack.0.conv1.weight", "decoder.res_stack.0.conv1.bias",
    "decoder.res_stack.0.gn2.weight", "decoder.res_stack.0.gn2.bias", "decoder.res_stack.0.conv2.weight", "decoder.res_stack.0.conv2.bias",
    "decoder.attn.fc.0.weight", "decoder.attn.fc.2.weight", "decoder.up_conv.weight", "decoder.up_conv.bias",
    "decoder.final.weight", "decoder.final.bias",
};

int load_weights(vqhip_codec* c, const std::map<std::string, PackTensor>& pk)
{
    std::string err;
#define NEED(var, name, ...)                                  \
    const PackTensor* var = need(pk, name, {__VA_ARGS__}, err); \
    if (!var) return fail(c, VQHIP_ERR_MODEL, err);
    NEED(e0w, "encoder.pre.0.weight", 16, 1, 3, 3, 3) NEED(e0b, "encoder.pre.0.bias", 16)
    NEED(eg0w, "encoder.pre.1.weight", 16) NEED(eg0b, "encoder.pre.1.bias", 16)
    NEED(r16g1w, "encoder.pre.3.gn1.weight", 16) NEED(r16g1b, "encoder.pre.3.gn1.bias", 16)
    NEED(r16c1w, "encoder.pre.3.conv1.weight", 16, 16, 3, 3, 3) NEED(r16c1b, "encoder.pre.3.conv1.bias", 16)
    NEED(r16g2w, "encoder.pre.3.gn2.weight", 16) NEED(r16g2b, "encoder.pre.3.gn2.bias", 16)
    NEED(r16c2w, "encoder.pre.3.conv2.weight", 16, 16, 3, 3, 3) NEED(r16c2b, "encoder.pre.3.conv2.bias", 16)
    NEED(edw, "encoder.down.weight", 32, 16, 4, 4, 4) NEED(edb, "encoder.down.bias", 32)
    NEED(r32g1w, "encoder.res_stack.0.gn1.weight", 32) NEED(r32g1b, "encoder.res_stack.0.gn1.bias", 32)
    NEED(r32c1w, "encoder.res_stack.0.conv1.weight", 32, 32, 3, 3, 3) NEED(r32c1b, "encoder.res_stack.0.conv1.bias", 32)
    NEED(r32g2w, "encoder.res_stack.0.gn2.weight", 32) NEED(r32g2b, "encoder.res_stack.0.gn2.bias", 32)
    NEED(r32c2w, "encoder.res_stack.0.conv2.weight", 32, 32, 3, 3, 3) NEED(r32c2b, "encoder.res_stack.0.conv2.bias", 32)
    NEED(efc0, "encoder.attn.fc.0.weight", 8, 32) NEED(efc2, "encoder.attn.fc.2.weight", 32, 8)
    NEED(epw, "encoder.proj.weight", 128, 32, 1, 1, 1) NEED(epb, "encoder.proj.bias", 128)
    NEED(dsw, "decoder.stem.0.weight", 64, 128, 3, 3, 3) NEED(dsb, "decoder.stem.0.bias", 64)
    NEED(dg0w, "decoder.stem.1.weight", 64) NEED(dg0b, "decoder.stem.1.bias", 64)
    NEED(r64g1w, "decoder.res_stack.0.gn1.weight", 64) NEED(r64g1b, "decoder.res_stack.0.gn1.bias", 64)
    NEED(r64c1w, "decoder.res_stack.0.conv1.weight", 64, 64, 3, 3, 3) NEED(r64c1b, "decoder.res_stack.0.conv1.bias", 64)
    NEED(r64g2w, "decoder.res_stack.0.gn2.weight", 64) NEED(r64g2b, "decoder.res_stack.0.gn2.bias", 64)
    NEED(r64c2w, "decoder.res_stack.0.conv2.weight", 64, 64, 3, 3, 3) NEED(r64c2b, "decoder.res_stack.0.conv2.bias", 64)
    NEED(dfc0, "decoder.attn.fc.0.weight", 16, 64) NEED(dfc2, "decoder.attn.fc.2.weight", 64, 16)
    NEED(duw, "decoder.up_conv.weight", 256, 64, 3, 3, 3) NEED(dub, "decoder.up_conv.bias", 256)
    NEED(dfw, "decoder.final.weight", 1, 32, 3, 3, 3) NEED(dfb, "decoder.final.bias", 1)
    NEED(cb, "quantizer.embedding", 256, 128)
#undef NEED
    // raw tensors in state_dict order, for the full training step (vq_train_full.inc): flat parameter vector + offsets
    c->h_params.clear();
    c->p_off.clear();
    for (const char* tn : kTrainable) {
        const PackTensor& t = pk.at(tn);
        c->p_off[tn] = {(int64_t)c->h_params.size(), (int64_t)t.count};
        c->h_params.insert(c->h_params.end(), t.data, t.data + t.count);
    }
    int rc;
#define UP(...)                                 \
    if ((rc = upload(c, __VA_ARGS__)) != VQHIP_OK) return rc;
    UP("e0.w", frag_first(e0w->data)) UP("e0.b", e0b) UP("eg0.w", eg0w) UP("eg0.b", eg0b)
    UP("r16g1.w", r16g1w) UP("r16g1.b", r16g1b) UP("r16c1.w", frag16(r16c1w->data, 27)) UP("r16c1.b", r16c1b)
    UP("r16g2.w", r16g2w) UP("r16g2.b", r16g2b) UP("r16c2.w", frag16(r16c2w->data, 27)) UP("r16c2.b", r16c2b)
    UP("ed.w", frag32(edw->data, 32, 16, 64)) UP("ed.b", dfrag32(edb->data, 32))
    UP("r32g1.w", r32g1w) UP("r32g1.b", r32g1b) UP("r32c1.w", frag32(r32c1w->data, 32, 32, 27)) UP("r32c1.b", dfrag32(r32c1b->data, 32))
    UP("r32g2.w", r32g2w) UP("r32g2.b", r32g2b) UP("r32c2.w", frag32(r32c2w->data, 32, 32, 27)) UP("r32c2.b", dfrag32(r32c2b->data, 32))
    UP("efc0", efc0) UP("efc2", efc2) 
    UP("ds.w", dsw) UP("ds.b", dsb) UP("dg0.w", dg0w) UP("dg0.b", dg0b)
    UP("r64g1.w", r64g1w) UP("r64g1.b", r64g1b) UP("r64c1.w", frag32(r64c1w->data, 64, 64, 27)) UP("r64c1.b", dfrag32(r64c1b->data, 64))
    UP("r64g2.w", r64g2w) UP("r64g2.b", r64g2b) UP("r64c2.w", frag32(r64c2w->data, 64, 64, 27)) UP("r64c2.b", dfrag32(r64c2b->data, 64))
    UP("r64c1.w16", frag16g(r64c1w->data, 64, 64, 27)) UP("r64c1.braw", r64c1b) UP("r64c2.w16", frag16g(r64c2w->data, 64, 64, 27)) UP("r64c2.braw", r64c2b)
    UP("r32c1.w16", frag16g(r32c1w->data, 32, 32, 27)) UP("r32c1.braw", r32c1b) UP("r32c2.w16", frag16g(r32c2w->data, 32, 32, 27)) UP("r32c2.braw", r32c2b)
    UP("ed.w16", frag16g(edw->data, 32, 16, 64)) UP("ed.braw", edb)
    UP("dfc0", dfc0) UP("dfc2", dfc2) if ((rc = build_folded_tail(c, duw->data, dub->data, dfw->data, dfb->data))) return rc;
    UP("cb", cb)
    c->h_proj_w.assign(epw->data, epw->data + 128 * 32);
    c->h_proj_b.assign(epb->data, epb->data + 128);
    UP("tr.wproj", frag32(epw->data, 128, 32, 1)) UP("tr.bproj", dfrag32(epb->data, 128))
    if ((rc = build_vq_fold(c, cb->data))) return rc;
#undef UP
    if ((rc = upload_steps(c, "steps.k3s1_4", steps_conv(4, 4, 3, 1, 1, 1)))) return rc;     // one tap per step (streamed layers)
    if ((rc = upload_steps(c, "steps.rowgroups8_4", steps_rowgroups8(4)))) return rc;
    if ((rc = upload_steps(c, "steps.rowgroups8_2", steps_rowgroups8(2)))) return rc;   // tiny batches: 32 groups of 2 rows
    if ((rc = upload_steps(c, "steps.rows_k3_4", steps_rows(4, 4, 3, 1, 1)))) return rc;
    if ((rc = upload_steps(c, "steps.rows_k4s2_8", steps_rows(8, 4, 4, 2, 1)))) return rc;
    if ((rc = upload_steps(c, "steps.rows8kd", steps_rows8_kd()))) return rc;
    {
        // decoder stem as a per-(tap, code) partial-sum table (stem_lut_k), built on the device once
        float* T = nullptr;
        HIPCHK(c, hipMalloc(&T, (size_t)27 * 256 * 64 * sizeof(float)));
        c->dw["ds.lut"] = T;
        hipLaunchKernelGGL(build_stem_lut_k, dim3(27 * 256), dim3(64), 0, c->stream, c->dw["ds.w"], c->dw["cb"], T);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VQHIP_OK;
}

// ---------------- workspace ----------------
// Inference keeps at most three large activations alive at a time (a conv reads its input and, for the second conv of a residual
// block, the skip tensor, and writes its output), and encode and decode never overlap on one handle — so the COMPACT layout packs
// every large activation of both directions into three regions of 32 KiB per leaf (0.1 MB per leaf, 6.8 GB for a 65 536-leaf
// chunk instead of 15 GB).  Debug mode and the training step need every intermediate at its own address: FULL layout.
struct ActSpec {
    const char* name;
    int C, NP;     // floats per leaf = C*NP ; C==0 -> per-leaf scalars, NP = count
    int region;    // compact layout: -1 own buffer, 0..2 shared region, -2 not allocated (full layout only)
};
const ActSpec kActs[] = {
    {"xr", 1, 768, -1},        // first-conv input, row layout with halo (pack_leaves_k): 64 rows x 12 floats per leaf
    {"xt", 1, 512, -2},        // position-major copy of the input: training / debug only
    // encode: xr -> a1 (R0) -> y4 (R1) -> a6 (R2, skip a1) -> x7 (R0) -> y9 (R1) -> x11 (R2, skip x7); y1 exists only in the
    // small-batch path (written and consumed before y4) and in debug / training
    {"e_y1", 16, 512, 1},      {"e_a1", 16, 512, 0},    {"e_y4", 16, 512, 1},    {"e_a6", 16, 512, 2},
    {"e_x7", 32, 64, 0},       {"e_y9", 32, 64, 1},     {"e_x11", 32, 64, 2},
    // decode: ystem (R0) -> d2 (R1) -> y4 (R2) -> x6 (R0, skip d2) -> voxels
    {"d_ystem", 64, 64, 0},    {"d_d2", 64, 64, 1},     {"d_y4", 64, 64, 2},     {"d_x6", 64, 64, 0},
    {"st_a.mean", 0, 8, -1},   {"st_a.rstd", 0, 8, -1}, {"st_b.mean", 0, 8, -1}, {"st_b.rstd", 0, 8, -1}, {"csum", 0, 64, -1}, {"gate", 0, 64, -1},
    {"part_s", 0, 1024, -1},   {"part_q", 0, 1024, -1},  {"part_c", 0, 1024, -1},   // per-block statistics partials of split launches (fp64 x 512: 16 blocks x 16 slots; fp32 x 1024); the 128 half-row partials of enc conv1 borrow e_a6
};
constexpr int kRegions = 3;

bool want_full_layout(const vqhip_codec* c) { return c->debug || c->training || c->full_training; }

size_t workspace_bytes(int64_t tiles, bool full)
{
    auto sz = [&](size_t per_leaf_floats) { return ((per_leaf_floats * sizeof(float) * 32 * (size_t)tiles) + 255) / 256 * 256; };
    size_t total = 0, region[kRegions] = {0, 0, 0};
    for (const ActSpec& a : kActs) {
        const size_t fl = a.C ? (size_t)a.C * a.NP : (size_t)a.NP;
        if (full || a.region == -1) total += sz(fl);
        else if (a.region >= 0) region[a.region] = std::max(region[a.region], sz(fl));
    }
    if (!full)
        for (size_t r : region) total += r;
    return total;
}

int ensure_workspace(vqhip_codec* c, int64_t n_leaves)
{
    const int64_t tiles = (n_leaves + 31) / 32;
    const bool full = want_full_layout(c);
    if (tiles <= c->ws_tiles && (c->ws_full || !full)) return VQHIP_OK;   // a full layout also serves inference
    // growing within a layout keeps the larger size; a switch to the full layout (debug, training: 2.4x the bytes per leaf) is sized
    // for what THIS call needs — a 32-leaf debug pass on a handle reserved for 65 536 leaves must not ask for 16 GB
    int64_t new_tiles = (full && !c->ws_full) ? tiles : std::max(tiles, c->ws_tiles);
    // the old block goes first, whatever its size: a switch to the full layout may ask for fewer bytes than the handle holds
    if (c->ws) HIPCHK(c, hipDeviceSynchronize());   // the workspace may be in use on a caller's stream
    c->ws.reset();
    c->ws_tiles = 0;
    for (const ActSpec& a : kActs) c->act[a.name] = nullptr;   // (only this workspace's names: the training step registers its own buffers in the same table)
    size_t total = workspace_bytes(new_tiles, full);
    hipError_t e = c->ws.grow(total);
    if (e != hipSuccess && new_tiles > tiles) {   // the larger-than-needed size did not fit: what the call needs
        new_tiles = tiles;
        total = workspace_bytes(new_tiles, full);
        e = c->ws.grow(total);
    }
    if (e != hipSuccess) {
        // the handle holds no workspace now (every activation pointer null); the chunk is re-fitted to the free memory
        // at the next host-pointer call, so a caller that retries after a transient shortage gets a smaller chunk instead of this error
        c->chunk_fitted = false;
        return fail(c, VQHIP_ERR_NOMEM, std::string("workspace hipMalloc of ") + std::to_string(total >> 20) + " MiB failed: " + hipGetErrorString(e));
    }
    auto sz = [&](size_t per_leaf_floats) { return ((per_leaf_floats * sizeof(float) * 32 * (size_t)new_tiles) + 255) / 256 * 256; };
    size_t off = 0, region_off[kRegions] = {0, 0, 0};
    if (!full) {   // the three shared regions first
        size_t region[kRegions] = {0, 0, 0};
        for (const ActSpec& a : kActs)
            if (a.region >= 0) region[a.region] = std::max(region[a.region], sz((size_t)a.C * a.NP));
        for (int r = 0; r < kRegions; ++r) region_off[r] = off, off += region[r];
    }
    for (const ActSpec& a : kActs) {
        const size_t fl = a.C ? (size_t)a.C * a.NP : (size_t)a.NP;
        c->act_shape[a.name] = {a.C, a.NP};
        if (full || a.region == -1) {
            c->act[a.name] = reinterpret_cast<float*>(c->ws + off);
            off += sz(fl);
        } else if (a.region >= 0) {
            c->act[a.name] = reinterpret_cast<float*>(c->ws + region_off[a.region]);
        } else {
            c->act[a.name] = nullptr;
        }
    }
    c->ws_tiles = new_tiles;
    c->ws_full = full;
    return VQHIP_OK;
}

// A shared GPU may not have room for the default chunk: halve the chunk until workspace + I/O slots fit into 80 % of the free
// memory (never below 2048 leaves; results do not depend on the chunk size).
void fit_chunk_to_free_memory(vqhip_codec* c)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;
    free_b += c->ws.bytes();   // what this handle already holds can be re-used
    while (c->chunk > 2048) {
        const size_t need = workspace_bytes((c->chunk + 31) / 32, want_full_layout(c)) + (size_t)c->chunk * (2 * 2048 + 2 * 64);
        if (need <= free_b / 5 * 4) break;
        c->chunk = (c->chunk / 2 + 31) / 32 * 32;
    }
}

// ---------------- launches ----------------
struct Launcher {
    vqhip_codec* c;
    hipStream_t s;
    int64_t leaves;
    int rc = VQHIP_OK;
    int64_t on_main = 0;   // launch groups put on s so far (Bwd::fork skips the event when nothing new has been enqueued)
    template <typename F>
    void run(const char* name, F&& f)
    {
        run_on(s, name, f);
    }
    // the same for launches that f() puts on another stream (profiling events go to that stream)
    template <typename F>
    void run_on(hipStream_t st, const char* name, F&& f)
    {
        if (rc != VQHIP_OK) return;
        if (st == s) ++on_main;
        KernelTimer t;
        if (c->profiling) {
            t.name = name;
            t.leaves = leaves;
            hipEventCreate(&t.start);
            hipEventCreate(&t.stop);
            hipEventRecord(t.start, st);
        }
        f();
        if (c->profiling) {
            hipEventRecord(t.stop, st);
            c->timers.push_back(t);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            c->err = std::string("launch ") + name + ": " + hipGetErrorString(e);
            rc = VQHIP_ERR_DEVICE;
        }
    }
};

template <typename K>
int set_lds(vqhip_codec* c, K kernel, size_t bytes)
{
    if (bytes > 64 * 1024) HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return VQHIP_OK;
}

// kernel instantiations -------------------------------------------------------------------
// decoder front of full chunks: gathers row by row (PIPE 0: the tap loop is bound by the LDS itself, reads in flight ahead bought nothing),
// the two position halves of a leaf octet on one SIMD (HMAP 1), the first taps of a pass not waiting for the previous pass's stores (RELAX)
constexpr auto k_stem_taps = stem_taps_k<0, 1, 0, true, 0, true>;   // (+ checkerboard row ownership: equal valid rows per wave in every tap)

// The two generic convs, conv_rows16_k and conv_mfma32_k, are instantiated on the named configurations of vq_kernels.h.  Every
// configuration the library launches stands in one of three lists: inference, and the decoder / encoder halves of the full training
// step (vq_train_full.inc).  From a list follows the table of its kernels with their dynamic LDS, which the init functions walk
// (set_lds); the launch helpers below refuse a configuration that is in no list.  Each table is defined where its kernels have
// always been instantiated, in that order: the order of the kernels in the code object follows it.
template <class... Cfg>
struct ConvList {
    template <class T>
    static constexpr bool has = (std::is_same_v<T, Cfg> || ...);
};
using InferConvs = ConvList<DecTailSlab, DecR64C1Full, DecR64C2Full, TrainR64C1, TrainR64C2, DecR64C1Split, DecR64C2Split, EncDownFull, EncDownSplit,
                            EncR32C1Full, EncR32C1Split, EncR32C2Full, EncR32C2Split, DecR64C1Split4, DecR64C2Split4, DecR64C1Split4Res, DecR64C2Split4Res,
                            EncDownSplit2, EncR32C1Split2, EncR32C2Split2>;
using TrainDecConvs = ConvList<TrainStem, TrainUp, DgradR64, DgradStem, TrainR64C1Split4Res, TrainR64C2Split4Res, DgradR64Split4Res, DgradR64Split4,
                               DgradR32Split2, DgradTail>;
using TrainEncConvs = ConvList<DgradProj, DgradR32>;

struct ConvKernel {
    void (*fn)(ConvArgs, const int4*);
    size_t lds;
};
template <class Cfg>
constexpr ConvKernel conv_kernel()
{
    if constexpr (std::is_base_of_v<RowsCfg, Cfg>) return {conv_rows16_k<Cfg>, rows_lds<Cfg>()};
    else return {conv_mfma32_k<Cfg>, mfma32_lds<Cfg>()};
}
template <class... Cfg>
constexpr std::array<ConvKernel, sizeof...(Cfg)> conv_kernels(ConvList<Cfg...>)
{
    return {{conv_kernel<Cfg>()...}};
}
template <size_t N>
int set_lds(vqhip_codec* c, const std::array<ConvKernel, N>& kernels)
{
    for (const ConvKernel& k : kernels)
        if (int rc = set_lds(c, k.fn, k.lds)) return rc;
    return VQHIP_OK;
}
constexpr auto kInferConvs = conv_kernels(InferConvs{});

// Launches of the two generic convs: block, grid and dynamic LDS follow from the configuration.  nt: leaf tiles of the batch; psplit:
// gridDim.y, the ranges of output groups of a position-split launch.
template <class Cfg>
constexpr bool conv_listed = InferConvs::has<Cfg> || TrainDecConvs::has<Cfg> || TrainEncConvs::has<Cfg>;
template <class Cfg>
void launch_rows(hipStream_t s, const ConvArgs& A, const void* steps, int nt, int psplit = 1)
{
    static_assert(conv_listed<Cfg>, "list the configuration above: init sets the dynamic LDS limit of the listed kernels");
    // NWV half tiles per workgroup, MSPLIT blocks of output channels over gridDim.z
    hipLaunchKernelGGL(conv_rows16_k<Cfg>, dim3((2 * nt + Cfg::NWV - 1) / Cfg::NWV, psplit, Cfg::MSPLIT), dim3(Cfg::NWV * 64), rows_lds<Cfg>(), s, A, (const int4*)steps);
}
template <class Cfg>
void launch_mfma32(hipStream_t s, const ConvArgs& A, const void* steps, int nt, int psplit = 1)
{
    static_assert(conv_listed<Cfg>, "list the configuration above: init sets the dynamic LDS limit of the listed kernels");
    hipLaunchKernelGGL(conv_mfma32_k<Cfg>, dim3((nt + Cfg::NW - 1) / Cfg::NW, psplit), dim3(Cfg::NW * 64), mfma32_lds<Cfg>(), s, A, (const int4*)steps);   // NW tiles per workgroup
}

constexpr size_t LDS_LATENT = (16 * 8 * 64 + 4 * 4 * 64) * 16;  // codebook + projection A-fragments (144 KB)

int init_kernel_attrs(vqhip_codec* c)
{
    int rc;
    if ((rc = set_lds(c, kInferConvs))) return rc;
    if ((rc = set_lds(c, conv8_lds_k<false, true, 8, 0, true>, LDS_CONV8))) return rc;
    if ((rc = set_lds(c, conv8_lds_k<false, true, 16, 0, false>, LDS_CONV8))) return rc;
    if ((rc = set_lds(c, conv8_lds_k<true, false, 16, 0, false>, LDS_CONV8))) return rc;
    if ((rc = set_lds(c, conv8_lds_k<true, false, 8, 0, true>, LDS_CONV8))) return rc;
    if ((rc = set_lds(c, k_stem_taps, LDS_STEM_TAPS))) return rc;
    if ((rc = set_lds(c, tail_rows16_k<0>, LDS_TAIL_ROWS))) return rc;
    if ((rc = set_lds(c, tail_rows32_k<0>, LDS_TAIL_ROWS))) return rc;
    if ((rc = set_lds(c, tail_groups16_k<0>, LDS_TAIL_GROUPS))) return rc;
    if ((rc = set_lds(c, conv_down_lds_k<0>, LDS_CONVDOWN))) return rc;
    if ((rc = set_lds(c, conv4_lds_k<false, true, false, 0, 1>, LDS_CONV4))) return rc;
    if ((rc = set_lds(c, conv4_lds_k<true, false, true, 0, 0>, LDS_CONV4))) return rc;
    if ((rc = set_lds(c, latent_assign_k<8>, LDS_LATENT))) return rc;
    if ((rc = set_lds(c, latent_assign_k<2>, LDS_LATENT))) return rc;
    if ((rc = set_lds(c, latent_assign_k<4>, LDS_LATENT))) return rc;
    return VQHIP_OK;
}
// The order of the other inference templates, as the list above keeps that of its kernels: a template is instantiated, and so placed
// in the code object, at its first mention in this file, and tools/kernel_isa_diff.py pairs the kernels of two builds by position.
// The layer stages below name them in the order of the layers, which is not the order they have in the code object.
[[maybe_unused]] const void* const kInstantiationOrder[] = {
    (const void*)e16b::conv_k<false>, (const void*)e16b::conv_k<true>, (const void*)gn_combine_k<false>, (const void*)conv_first_k<0, 0, true>,
    (const void*)conv_first_k<0>, (const void*)conv_first_roll_k<1, true>, (const void*)conv_first_roll_k<1>, (const void*)conv_first_k<1>,
    (const void*)conv_first_k<2, 0, true>, (const void*)conv_first_k<2>, (const void*)gn_relu_stats_k<16, 512, 4>, (const void*)conv8_c16_k<2, false, true>,
    (const void*)conv8_c16_k<4, false, true>, (const void*)gn_combine_k<false, true>, (const void*)conv8_c16_k<2, true, false>,
    (const void*)conv8_c16_k<4, true, false>, (const void*)csum_combine_k<32>, (const void*)vq_folded_k<8>, (const void*)vq_folded_k<2>,
    (const void*)conv_first_roll_k<0, true>, (const void*)conv_first_roll_k<0>, (const void*)d64b::conv_k<false>, (const void*)d64b::conv_k<true>,
    (const void*)gn_combine_k<true>, (const void*)csum_combine_k<64>, (const void*)stem_fused_k<16>, (const void*)stem_fused_k<8>,
    (const void*)gn_relu_stats_k<64, 64, 8>,
};

// Where the encoder's GroupNorm statistics and channel sums live.  Inference ping-pongs two buffers (st_a / st_b); the full training
// step needs every layer's statistics again in its backward pass, so there each tensor's statistics go to their own buffer of the
// training workspace (ts_*) — the forward used to overwrite them and a pass of six sequential statistics kernels recomputed them
// from the stored activations (0.17 ms of a 7 ms step).
struct EncStats {
    float *y1m, *y1r, *a1m, *a1r, *y4m, *y4r, *x7m, *x7r, *y9m, *y9r, *csum;
};
EncStats enc_stats_of(vqhip_codec* c, bool train_forward)
{
    auto& a = c->act;
    if (train_forward)
        return {a["ts_gn0.mean"], a["ts_gn0.rstd"], a["ts_r16g1.mean"], a["ts_r16g1.rstd"], a["ts_r16g2.mean"], a["ts_r16g2.rstd"],
                a["ts_r32g1.mean"], a["ts_r32g1.rstd"], a["ts_r32g2.mean"], a["ts_r32g2.rstd"], a["ts_ecsum"]};
    return {a["st_a.mean"], a["st_a.rstd"], a["st_b.mean"], a["st_b.rstd"], a["st_a.mean"], a["st_a.rstd"],
            a["st_b.mean"], a["st_b.rstd"], a["st_a.mean"], a["st_a.rstd"], a["csum"]};
}

// gridDim.y for a position-split launch of `wgs` workgroups: enough ranges to reach `target` workgroups (about two rounds
// of what the chip holds at once given the kernel's LDS / register footprint), at least `lo` (the factor used near the
// crossover), at most the kernel's number of output groups (a power of two)
int split_factor(int wgs, int lo, int n_groups, int target)
{
    int ps = lo;
    while (ps < n_groups && (int64_t)wgs * ps < target) ps *= 2;
    return std::min(ps, n_groups);
}

// Which path a pass of nt 32-leaf tiles takes.  One wave per tile fills the chip in rounds of 1024 tiles (1024 SIMDs), so its
// time is a staircase (encode: 7.7 ms at 1024 tiles, 10.2 ms at 1536); the split path is linear (about 6.4 us per tile for
// encode, 5.9 us for decode) and wins up to about 88 % of a full 2048-tile chunk.  Crossovers measured with
// tools/small_batch_probe.py.
bool use_split(const vqhip_codec* c, int nt, bool decode)
{
    if (c->split_tiles >= 0) return nt <= (decode ? 5 * c->split_tiles / 4 : c->split_tiles);
    return nt <= (decode ? 1728 : 1600);   // measured crossovers (r02 v8 kernels): encode 51 200 leaves, decode 55 296
}

// One encode or decode pass of n leaves on stream s: what the layer stages below take.  A stage states its layer's tensors, weights,
// GroupNorm inputs and step table once; the path decides the kernel, the launch geometry and the route of the output statistics.
//   split false: one wave (or workgroup) per tile, and the kernel finishes its statistics itself (out_mean / out_rstd / out_csum).
//   split true: small batches (too few leaf tiles to fill 1024 SIMDs with one wave per tile).  Every layer is launched with its
//     output groups split over gridDim.y (and, for the tiniest batches, its output channels over gridDim.z) workgroups.  Each
//     workgroup covers whole statistics blocks (16 per leaf, the contract's 16-block rule) and stores their partial sums (part_s /
//     part_q / part_c, found through grp_start); gn_combine_k / csum_combine_k add the blocks in order.  Same results bit for bit,
//     15-25x lower latency.  The names of these launches end in _s.
struct Pass {
    vqhip_codec* c;
    hipStream_t s;
    Launcher L;
    int64_t n;
    int nt;             // 32-leaf tiles
    const bool split;   // use_split
    int precision;      // VQHIP_PRECISION_* of the two 16 -> 16 convs (encode) / 64 -> 64 convs (decode)
};
struct EncPass : Pass {
    EncStats S;
    const float* d_leaves;
    bool raw;           // the first conv reads d_leaves itself, not the row layout xr
    uint8_t* d_idx;
    float* d_latent;    // training: the latent rows are stored and assigned against the live codebook
    float* latent_l4;   // the forward of the full training step: the latent in the L4 layout as well ...
    bool keep_y1;       // ... the first conv's raw output kept, and every layer's statistics in a buffer of their own (EncStats)
};
struct DecPass : Pass {
    const uint8_t* d_idx;
    float* d_out;
};

double* part_s(vqhip_codec* c) { return reinterpret_cast<double*>(c->act["part_s"]); }
double* part_q(vqhip_codec* c) { return reinterpret_cast<double*>(c->act["part_q"]); }
// the first step of each output group in a step table, by the table's name + ".grp" (a literal: no string is built per launch)
const int* grp(vqhip_codec* c, const char* name) { return reinterpret_cast<const int*>(c->dw[name]); }

// The combine kernels behind a launch that stored per-block partials.  GroupNorm statistics of `groups` groups from part_s / part_q:
void combine(Pass& P, const char* name, int groups, double inv_n, float* mean, float* rstd)
{
    P.L.run(name, [&] { hipLaunchKernelGGL(gn_combine_k<false>, dim3(P.nt), dim3(groups * 32), 0, P.s, part_s(P.c), part_q(P.c), mean, rstd, groups, inv_n); });
}
// ... of GroupNorm(8,16) from one partial per output half row (ps, pq), added row-major
void combine_rows(Pass& P, const char* name, const double* ps, const double* pq, float* mean, float* rstd)
{
    P.L.run(name, [&] { hipLaunchKernelGGL((gn_combine_k<false, true>), dim3(P.nt), dim3(8 * 32), 0, P.s, ps, pq, mean, rstd, 8, 1.0 / 1024.0); });
}
// ... of GroupNorm(8,64): 16 slots = the 4-channel halves of a group
void combine_pairs(Pass& P, const char* name, float* mean, float* rstd)
{
    P.L.run(name, [&] { hipLaunchKernelGGL(gn_combine_k<true>, dim3(P.nt), dim3(512), 0, P.s, part_s(P.c), part_q(P.c), mean, rstd, 8, 1.0 / 512.0); });
}
// ... and the channel sums of C channels from part_c, with the attention gates (computed once per tile here, read by the next stage)
template <int C>
void combine_csum(Pass& P, const char* name, float* csum, const float* fc0, const float* fc2)
{
    auto& a = P.c->act;
    P.L.run(name, [&] { hipLaunchKernelGGL((csum_combine_k<C>), dim3(P.nt), dim3(64 * C / 8), 0, P.s, a["part_c"], csum, fc0, fc2, a["gate"]); });
}

// ---- bf16 modes (vqvdb_hip_encode_mode.h, DESIGN 24, kernels in vq_enc16_bf16.h; vqvdb_hip_precision.h, DESIGN 23, vq_dec64_bf16.h) ----
// The bf16 A fragments of a mode's two convs, packed on the device from the live fp32 fragments `src` (uploaded at create, rebuilt by
// refrag_all after every training update, which marks the mode's fragments stale).  Buffers first, so that a failed allocation
// leaves the handle as it was.  The pack is followed by a wait: it happens once per weight change, and a later call may use
// another stream.
struct Bf16Conv {
    DevBuf<uint16_t>& frag;
    const char* src;
    const void* kernel;
    const char* what;
};
int ensure_bf16_frags(vqhip_codec* c, hipStream_t s, bool& stale, Bf16Conv (&&convs)[2], size_t frag_elems, void (*pack)(const float*, uint16_t*), size_t lds)
{
    if (!stale && convs[0].frag && convs[1].frag) return VQHIP_OK;
    for (Bf16Conv& v : convs)
        if (int rc = ensure(c, v.frag, frag_elems, v.what)) return rc;
    for (Bf16Conv& v : convs) HIPCHK(c, hipFuncSetAttribute(v.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (Bf16Conv& v : convs) hipLaunchKernelGGL(pack, dim3((frag_elems / 8 + 255) / 256), dim3(256), 0, s, c->dw[v.src], v.frag.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    stale = false;
    return VQHIP_OK;
}
int ensure_enc_bf16_frags(vqhip_codec* c, hipStream_t s)
{
    return ensure_bf16_frags(c, s, c->bf_enc_stale,
                             {{c->bf_r16c1, "r16c1.w", reinterpret_cast<const void*>(e16b::conv_k<false>), "the bf16 fragments of encoder.pre.3.conv1"},
                              {c->bf_r16c2, "r16c2.w", reinterpret_cast<const void*>(e16b::conv_k<true>), "the bf16 fragments of encoder.pre.3.conv2"}},
                             e16b::FRAG_ELEMS, e16b::frag_k, e16b::LDS_BYTES);
}
int ensure_dec_bf16_frags(vqhip_codec* c, hipStream_t s)
{
    return ensure_bf16_frags(c, s, c->bf_stale,
                             {{c->bf_r64c1, "r64c1.w16", reinterpret_cast<const void*>(d64b::conv_k<false>), "the bf16 fragments of decoder.res_stack.0.conv1"},
                              {c->bf_r64c2, "r64c2.w16", reinterpret_cast<const void*>(d64b::conv_k<true>), "the bf16 fragments of decoder.res_stack.0.conv2"}},
                             d64b::FRAG_ELEMS, d64b::frag_k, d64b::LDS_BYTES);
}

// ---- the encoder's stages: xr -> a1 -> y4 -> a6 (skip a1) -> x7 -> y9 -> x11 (skip x7) -> indices ----
// first conv + GroupNorm(4,16) + ReLU: xr (or the caller's leaves) -> e_a1, with the statistics of y1 and those of a1 for res.gn1
void enc_first(EncPass& P)
{
    vqhip_codec* c = P.c;
    auto &a = c->act, &w = c->dw;
    const int nt = P.nt, g4 = (nt + 3) / 4, gq = (2 * nt + 3) / 4, psf = P.split ? split_factor(g4, 8, 16, 1024) : 1;
    const int4* steps = (const int4*)w["steps.rows8kd"];
    float* y1 = (c->debug || P.keep_y1) ? a["e_y1"] : nullptr;
    ConvArgs A{};
    A.in = P.raw ? P.d_leaves : a["xr"], A.wfrag = w["e0.w"], A.bias_frag = w["e0.b"], A.n_tiles = nt, A.n_leaves = P.n;
    A.n_steps = c->nsteps["steps.rows8kd"];
    if (P.split) A.grp_start = grp(c, "steps.rows8kd.grp"), A.part_s = part_s(c), A.part_q = part_q(c);
    if (!P.split && c->first_once && !c->first_raw && !c->training && !c->full_training) {
        // first conv once: conv + GroupNorm(4,16) + ReLU + statistics for res.gn1 out of the accumulators of a workgroup per 8-leaf group
        A.out = a["e_a1"], A.in_gamma = w["eg0.w"], A.in_beta = w["eg0.b"], A.out_mean = P.S.a1m, A.out_rstd = P.S.a1r;
        P.L.run("enc_conv_first", [&] { hipLaunchKernelGGL(conv_first_once_k, dim3(std::min(4 * nt, c->n_cus)), dim3(512), 0, P.s, A, y1, P.S.y1m, P.S.y1r); });
        return;
    }
    if (P.split && nt < 256) {   // small batches: the raw output stored, normalised in an elementwise pass
        A.out = a["e_y1"];
        P.L.run("enc_conv_first_s", [&] {
            if (P.raw) hipLaunchKernelGGL((conv_first_k<2, 0, true>), dim3(g4, psf), dim3(256), 0, P.s, A, steps);
            else hipLaunchKernelGGL(conv_first_k<2>, dim3(g4, psf), dim3(256), 0, P.s, A, steps);
        });
        combine(P, "enc_stats_y1", 4, 1.0 / 2048.0, P.S.y1m, P.S.y1r);
        ConvArgs B{};
        B.in = a["e_y1"], B.out = a["e_a1"], B.in_mean = P.S.y1m, B.in_rstd = P.S.y1r, B.in_gamma = w["eg0.w"], B.in_beta = w["eg0.b"];
        B.n_tiles = nt, B.part_s = A.part_s, B.part_q = A.part_q;
        P.L.run("enc_gn_relu_a1", [&] { hipLaunchKernelGGL((gn_relu_stats_k<16, 512, 4>), dim3(g4, psf), dim3(256), 0, P.s, B); });
        combine(P, "enc_stats_a1", 8, 1.0 / 1024.0, P.S.a1m, P.S.a1r);
        return;
    }
    // first conv twice: statistics pass, then recompute + GroupNorm(4,16) + ReLU + statistics for res.gn1.  Mid-size batches
    // (split, nt >= 256) take it too, like the one-wave-per-tile path, instead of storing the raw output and normalising it in an
    // elementwise pass (2 x 32 KiB per leaf less traffic)
    A.out = y1;
    if (!P.split) A.out_mean = P.S.y1m, A.out_rstd = P.S.y1r;
    // first_roll: a wave per 16-leaf sub-tile with a rolling 3 x 3 row window in registers (three row loads per output row instead of nine)
    // (the normalising pass only: its stores compete with the loads — 0.458 -> 0.393 ms; the statistics pass runs 0.322 ms on the
    // (row, kd) kernel and 0.353 ms with the window, whose plane starts it cannot hide; VQHIP_FIRST=roll0 selects that as well)
    const bool roll_stats = !P.split && c->first_roll_stats;
    P.L.run(P.split ? "enc_conv_first_stats_s" : "enc_conv_first_stats", [&] {
        if (P.raw && roll_stats) hipLaunchKernelGGL((conv_first_roll_k<0, true>), dim3(gq), dim3(256), 0, P.s, A);
        else if (P.raw) hipLaunchKernelGGL((conv_first_k<0, 0, true>), dim3(g4, psf), dim3(256), 0, P.s, A, steps);
        else if (roll_stats) hipLaunchKernelGGL(conv_first_roll_k<0>, dim3(gq), dim3(256), 0, P.s, A);
        else hipLaunchKernelGGL(conv_first_k<0>, dim3(g4, psf), dim3(256), 0, P.s, A, steps);
    });
    if (P.split) combine(P, "enc_stats_y1", 4, 1.0 / 2048.0, P.S.y1m, P.S.y1r);
    A.out = a["e_a1"], A.in_mean = P.S.y1m, A.in_rstd = P.S.y1r, A.in_gamma = w["eg0.w"], A.in_beta = w["eg0.b"];
    if (!P.split) A.out_mean = P.S.a1m, A.out_rstd = P.S.a1r;
    P.L.run(P.split ? "enc_conv_first_gn_s" : "enc_conv_first_gn", [&] {   // (rolling row window: vq_first_roll.h)
        if (P.raw) hipLaunchKernelGGL((conv_first_roll_k<1, true>), dim3(gq, psf), dim3(256), 0, P.s, A);
        else if (c->first_roll) hipLaunchKernelGGL(conv_first_roll_k<1>, dim3(gq, psf), dim3(256), 0, P.s, A);
        else hipLaunchKernelGGL(conv_first_k<1>, dim3(g4, psf), dim3(256), 0, P.s, A, steps);
    });
    if (P.split) combine(P, "enc_stats_a1", 8, 1.0 / 1024.0, P.S.a1m, P.S.a1r);
}

// the 16-channel residual block: e_a1 (+ its statistics) -> e_y4 (+ gn2's statistics) -> e_a6.  On every path conv1 stores partials
// of its output's statistics and a combine kernel finishes them.
void enc_res16(EncPass& P)
{
    vqhip_codec* c = P.c;
    auto &a = c->act, &w = c->dw;
    const int nt = P.nt, gq = (2 * nt + 3) / 4;
    if (P.precision == VQHIP_PRECISION_BF16) {
        // ONE kernel per conv whatever the batch size and launch path, so a leaf's bits do not depend on the path.  conv1 stores the
        // sixteen half-row totals per leaf and gn_combine_k<false> adds them in (oh, hw) order, as after conv8_lds_k.  The workgroups
        // are persistent: grid from n_cus.
        const int grid = std::min(4 * nt, c->n_cus);
        e16b::Args B{};
        B.in = a["e_a1"], B.out = a["e_y4"], B.wf = c->bf_r16c1, B.bias = w["r16c1.b"], B.n_groups = 4 * nt;
        B.in_mean = P.S.a1m, B.in_rstd = P.S.a1r, B.in_gamma = w["r16g1.w"], B.in_beta = w["r16g1.b"];
        B.part_s = part_s(c), B.part_q = part_q(c);
        P.L.run("enc_res16_conv1_bf16", [&] { hipLaunchKernelGGL(e16b::conv_k<false>, dim3(grid), dim3(e16b::THREADS), e16b::LDS_BYTES, P.s, B); });
        combine(P, "enc_stats_y4", 8, 1.0 / 1024.0, P.S.y4m, P.S.y4r);
        B.in = a["e_y4"], B.out = a["e_a6"], B.wf = c->bf_r16c2, B.bias = w["r16c2.b"], B.skip = a["e_a1"];
        B.in_mean = P.S.y4m, B.in_rstd = P.S.y4r, B.in_gamma = w["r16g2.w"], B.in_beta = w["r16g2.b"];
        B.part_s = nullptr, B.part_q = nullptr;
        P.L.run("enc_res16_conv2_bf16", [&] { hipLaunchKernelGGL(e16b::conv_k<true>, dim3(grid), dim3(e16b::THREADS), e16b::LDS_BYTES, P.s, B); });
        return;
    }
    // lds: input planes staged in LDS by a persistent workgroup per CU; statistics as 16 half-row totals.  Otherwise the row-group kernel
    const bool lds = !P.split && c->conv8_lds;
    const int lds_grid = std::min(2 * nt, c->n_cus);
    // a handful of tiles take two-row groups (32 ranges, half the serial chain per wave; same taps in the same order) — both convs:
    // the statistics blocks are half rows, whatever the row grouping
    const bool two = P.split && gq * 32 <= 512;   // up to 1024 leaves (measured)
    const char* tab = two ? "steps.rowgroups8_2" : "steps.rowgroups8_4";
    const int4* steps = (const int4*)w[tab];
    const int psr = !P.split ? 1 : two ? 32 : split_factor(gq, 8, 16, 1024);
    ConvArgs A{};
    A.in = a["e_a1"], A.out = a["e_y4"], A.wfrag = w["r16c1.w"], A.bias_frag = w["r16c1.b"];
    A.in_mean = P.S.a1m, A.in_rstd = P.S.a1r, A.in_gamma = w["r16g1.w"], A.in_beta = w["r16g1.b"], A.n_tiles = nt;
    A.n_steps = c->nsteps[tab];
    if (P.split) A.grp_start = grp(c, two ? "steps.rowgroups8_2.grp" : "steps.rowgroups8_4.grp");
    if (lds) A.part_s = part_s(c), A.part_q = part_q(c);
    else {
        // conv1 carries the statistics.  The row-group kernel's statistics blocks are its 128 output half rows: 2 x 1024 doubles per leaf
        // of partials, which live in the region of conv2's output (e_a6: free until conv2 runs, after the combine)
        A.part_s = reinterpret_cast<double*>(a["e_a6"]), A.part_q = A.part_s + (size_t)nt * 128 * 8 * 32;
    }
    P.L.run(P.split ? "enc_res16_conv1_s" : "enc_res16_conv1", [&] {
        if (lds && c->conv8_w16) hipLaunchKernelGGL((conv8_lds_k<false, true, 16, 0, false>), dim3(lds_grid), dim3(1024), LDS_CONV8, P.s, A);
        else if (lds) hipLaunchKernelGGL((conv8_lds_k<false, true, 8, 0, true>), dim3(lds_grid), dim3(512), LDS_CONV8, P.s, A);
        else if (two) hipLaunchKernelGGL((conv8_c16_k<2, false, true>), dim3(gq, psr), dim3(256), 0, P.s, A, steps);
        else hipLaunchKernelGGL((conv8_c16_k<4, false, true>), dim3(gq, psr), dim3(256), 0, P.s, A, steps);
    });
    if (lds) combine(P, "enc_stats_y4", 8, 1.0 / 1024.0, P.S.y4m, P.S.y4r);
    else combine_rows(P, "enc_stats_y4", A.part_s, A.part_q, P.S.y4m, P.S.y4r);
    ConvArgs B{};
    B.in = a["e_y4"], B.out = a["e_a6"], B.wfrag = w["r16c2.w"], B.bias_frag = w["r16c2.b"], B.skip = a["e_a1"];
    B.in_mean = P.S.y4m, B.in_rstd = P.S.y4r, B.in_gamma = w["r16g2.w"], B.in_beta = w["r16g2.b"], B.n_tiles = nt;
    B.n_steps = A.n_steps, B.grp_start = A.grp_start;
    P.L.run(P.split ? "enc_res16_conv2_s" : "enc_res16_conv2", [&] {
        if (lds && c->conv8_w16) hipLaunchKernelGGL((conv8_lds_k<true, false, 16, 0, false>), dim3(lds_grid), dim3(1024), LDS_CONV8, P.s, B);
        else if (lds) hipLaunchKernelGGL((conv8_lds_k<true, false, 8, 0, true>), dim3(lds_grid), dim3(512), LDS_CONV8, P.s, B);
        else if (two) hipLaunchKernelGGL((conv8_c16_k<2, true, false>), dim3(gq, psr), dim3(256), 0, P.s, B, steps);
        else hipLaunchKernelGGL((conv8_c16_k<4, true, false>), dim3(gq, psr), dim3(256), 0, P.s, B, steps);
    });
}

// down conv: e_a6 -> e_x7 with the statistics for res32.gn1
void enc_down(EncPass& P)
{
    vqhip_codec* c = P.c;
    auto &a = c->act, &w = c->dw;
    const int nt = P.nt;
    const float* steps = w["steps.rows_k4s2_8"];
    ConvArgs A{};
    A.in = a["e_a6"], A.out = a["e_x7"], A.wfrag = w["ed.w16"], A.bias_frag = w["ed.braw"], A.n_tiles = nt;
    A.n_steps = c->nsteps["steps.rows_k4s2_8"], A.n_taps = 64;
    if (!P.split) {
        A.out_mean = P.S.x7m, A.out_rstd = P.S.x7r;
        P.L.run("enc_down", [&] {
            if (c->convdown_lds) hipLaunchKernelGGL(conv_down_lds_k<0>, dim3(std::min(2 * nt, c->n_cus)), dim3(1024), LDS_CONVDOWN, P.s, A);
            else launch_rows<EncDownFull>(P.s, A, steps, nt);
        });
        return;
    }
    A.grp_start = grp(c, "steps.rows_k4s2_8.grp"), A.part_s = part_s(c), A.part_q = part_q(c);
    const int gh = (2 * nt + 7) / 8, psr = split_factor(gh, 4, 16, 512);   // gh: workgroups of 8 half tiles (conv_rows16_k)
    P.L.run("enc_down_s", [&] {
        if (gh * psr * 2 <= 256) launch_rows<EncDownSplit2>(P.s, A, steps, nt, psr);
        else launch_rows<EncDownSplit>(P.s, A, steps, nt, psr);
    });
    combine(P, "enc_stats_x7", 8, 1.0 / 256.0, P.S.x7m, P.S.x7r);
}

// the 32-channel residual block: e_x7 -> e_y9 (+ gn2's statistics) -> e_x11 with the channel sums of the attention
void enc_res32(EncPass& P)
{
    vqhip_codec* c = P.c;
    auto &a = c->act, &w = c->dw;
    const int nt = P.nt;
    const float* steps = w["steps.rows_k3_4"];
    const int gh = (2 * nt + 7) / 8, psr = split_factor(gh, 4, 16, 512);
    const bool ms = gh * psr * 2 <= 256;   // (split) up to 1024 leaves (measured): also split the 32 couts over gridDim.z
    ConvArgs A{};
    A.in = a["e_x7"], A.out = a["e_y9"], A.wfrag = w["r32c1.w16"], A.bias_frag = w["r32c1.braw"];
    A.in_mean = P.S.x7m, A.in_rstd = P.S.x7r, A.in_gamma = w["r32g1.w"], A.in_beta = w["r32g1.b"], A.n_tiles = nt;
    A.n_steps = c->nsteps["steps.rows_k3_4"], A.n_taps = 27;
    ConvArgs B{};
    B.in = a["e_y9"], B.out = a["e_x11"], B.wfrag = w["r32c2.w16"], B.bias_frag = w["r32c2.braw"], B.skip = a["e_x7"];
    B.in_mean = P.S.y9m, B.in_rstd = P.S.y9r, B.in_gamma = w["r32g2.w"], B.in_beta = w["r32g2.b"], B.n_tiles = nt;
    B.n_steps = A.n_steps, B.n_taps = 27;
    if (!P.split) {
        A.out_mean = P.S.y9m, A.out_rstd = P.S.y9r;
        P.L.run("enc_res32_conv1", [&] {
            if (c->conv4_lds) hipLaunchKernelGGL((conv4_lds_k<false, true, false, 0, 1>), dim3(std::min(2 * nt, c->n_cus)), dim3(512), LDS_CONV4, P.s, A);
            else launch_rows<EncR32C1Full>(P.s, A, steps, nt);
        });
        B.out_csum = P.S.csum;
        P.L.run("enc_res32_conv2", [&] {
            if (c->conv4_lds) hipLaunchKernelGGL((conv4_lds_k<true, false, true, 0, 0>), dim3(std::min(2 * nt, c->n_cus)), dim3(512), LDS_CONV4, P.s, B);
            else launch_rows<EncR32C2Full>(P.s, B, steps, nt);
        });
        return;
    }
    A.grp_start = B.grp_start = grp(c, "steps.rows_k3_4.grp");
    A.part_s = part_s(c), A.part_q = part_q(c);
    P.L.run("enc_res32_conv1_s", [&] {
        if (ms) launch_rows<EncR32C1Split2>(P.s, A, steps, nt, psr);
        else launch_rows<EncR32C1Split>(P.s, A, steps, nt, psr);
    });
    combine(P, "enc_stats_y9", 8, 1.0 / 256.0, P.S.y9m, P.S.y9r);
    B.part_c = a["part_c"];
    P.L.run("enc_res32_conv2_s", [&] {
        if (ms) launch_rows<EncR32C2Split2>(P.s, B, steps, nt, psr);
        else launch_rows<EncR32C2Split>(P.s, B, steps, nt, psr);
    });
    combine_csum<32>(P, "enc_csum_x11", P.S.csum, w["efc0"], w["efc2"]);
}

// training forward instead of the VQ: latent materialised, reference-faithful distance against the live codebook
void enc_latent_assign(EncPass& P)
{
    vqhip_codec* c = P.c;
    auto &a = c->act, &w = c->dw;
    const int nt = P.nt;
    P.L.run("train_codebook_frag", [&] { hipLaunchKernelGGL(codebook_frag_k, dim3(33), dim3(256), 0, P.s, w["cb"], w["tr.efrag"], w["tr.ee"]); });
    LatentArgs A{};
    A.in = a["e_x11"], A.se_csum = P.S.csum, A.se_fc0 = w["efc0"], A.se_fc2 = w["efc2"];
    A.wproj = w["tr.wproj"], A.bproj = w["tr.bproj"], A.efrag = w["tr.efrag"], A.ee_frag = w["tr.ee"];
    A.idx = P.d_idx, A.z = P.d_latent, A.z4 = P.latent_l4, A.n_leaves = P.n, A.n_tiles = nt;
    const int split = P.split ? split_factor((nt + 1) / 2, 8, 32, 512) : 1;   // position ranges per tile
    if (!P.split && nt >= 1024) P.L.run("train_latent_assign", [&] { hipLaunchKernelGGL(latent_assign_k<8>, dim3((nt + 7) / 8), dim3(512), LDS_LATENT, P.s, A); });
    else if (P.split && nt >= 8) {
        // small training batches: 144 KB of LDS = one workgroup per CU, so FOUR waves per workgroup (every SIMD busy; two left half of
        // the CU idle) and twice the position ranges: 0.236 -> 0.13 ms at 2048 leaves
        const int sp = std::min(64, 2 * split);
        P.L.run("train_latent_assign", [&] { hipLaunchKernelGGL(latent_assign_k<4>, dim3((nt + 3) / 4, sp), dim3(256), LDS_LATENT, P.s, A); });
    } else P.L.run("train_latent_assign", [&] { hipLaunchKernelGGL(latent_assign_k<2>, dim3((nt + 1) / 2, split), dim3(128), LDS_LATENT, P.s, A); });
}

// attention gates + projection + nearest code, folded: e_x11 -> indices
void enc_vq(EncPass& P)
{
    vqhip_codec* c = P.c;
    auto &a = c->act, &w = c->dw;
    const int nt = P.nt, g2 = (nt + 1) / 2, g8 = (nt + 7) / 8;
    VqArgs A{};
    A.in = a["e_x11"], A.se_csum = P.S.csum, A.se_fc0 = w["efc0"], A.se_fc2 = w["efc2"];
    A.epfrag = w["vq.ep"], A.ck_frag = w["vq.ck"], A.idx = P.d_idx, A.n_leaves = P.n, A.n_tiles = nt;
    if (P.split) A.se_gate = a["gate"];   // computed once per tile by enc_csum_x11
    P.L.run(P.split ? "enc_vq_s" : "enc_vq", [&] {
        // one wave per tile: two position ranges per tile, 2 x n_tiles waves = 4 per SIMD on a full chunk (one wave per tile leaves 2,
        // and the wave's MFMA chain -> argmin scan -> next chain sequence has nobody to overlap with)
        if (!P.split) hipLaunchKernelGGL(vq_folded_k<8>, dim3(g8, c->vq_split), dim3(512), 0, P.s, A);
        // mid-size batches: 8 tiles behind one copy of the folded codebook in LDS (33 KB) instead of 2
        else if (nt >= 256) hipLaunchKernelGGL(vq_folded_k<8>, dim3(g8, split_factor(g8, 2, 32, 512)), dim3(512), 0, P.s, A);
        else hipLaunchKernelGGL(vq_folded_k<2>, dim3(g2, split_factor(g2, 8, 32, 2048)), dim3(128), 0, P.s, A);
    });
}

// precision: VQHIP_PRECISION_* of the two 16 -> 16 convs.  Only the plain encode entry points pass the handle's mode; the round
// trip, every bounded, residual and size-sweep call, training and vqhip_multi_* take the default.  latent_l4: the forward of the
// full training step (EncPass).
int encode_chunk(vqhip_codec* c, const float* d_leaves, int64_t n, uint8_t* d_idx, hipStream_t s, float* d_latent = nullptr,
                 int precision = VQHIP_PRECISION_FP32, float* latent_l4 = nullptr)
{
    int rc = ensure_workspace(c, n);
    if (rc) return rc;
    if (precision == VQHIP_PRECISION_BF16 && (rc = ensure_enc_bf16_frags(c, s))) return rc;
    const int nt = (int)((n + 31) / 32);
    // raw: the first conv reads d_leaves itself; the row layout is still written when something else reads it (training, debug fetches, VQHIP_FIRST=steps' normalising pass)
    const bool raw = c->first_raw && c->first_roll && !c->training && !c->full_training;
    const bool train_forward = latent_l4 != nullptr;
    EncPass P{{c, s, {c, s, n}, n, nt, use_split(c, nt, false), precision}, enc_stats_of(c, train_forward), d_leaves, raw, d_idx, d_latent, latent_l4, train_forward};
    // the position-major copy xt is only read by the training step (loss, first-conv weight gradients) and by debug fetches
    float* xt = (c->training || c->full_training || c->debug) ? c->act["xt"] : nullptr;
    if (!raw || xt) P.L.run("pack_leaves", [&] { hipLaunchKernelGGL(pack_leaves_k, dim3(nt, nt <= 128 ? 8 : 1), dim3(256), 0, s, d_leaves, c->act["xr"], xt, n); });
    enc_first(P);
    enc_res16(P);
    enc_down(P);
    enc_res32(P);
    if (d_latent) enc_latent_assign(P);
    else enc_vq(P);
    return P.L.rc;
}

// ---- the decoder's stages: indices -> d2 -> y4 -> x6 (skip d2) -> voxels ----
// decoder front: code gather + stem conv (a table lookup) + GroupNorm(8,64) + ReLU -> d_d2 with its statistics in st_b
void dec_stem(DecPass& P)
{
    vqhip_codec* c = P.c;
    auto &a = c->act, &w = c->dw;
    const int nt = P.nt, g4 = (nt + 3) / 4;
    const int4* steps = (const int4*)w["steps.k3s1_4"];
    // one kernel: the table through the LDS ring (stem_taps_k) — on the split path for mid-size passes, a tile per CU and more — or
    // gathered through the L1 by a workgroup per four leaves that normalises out of LDS and finishes both sets of statistics itself
    // (stem_fused_k: at SOP-sized passes instead of four launches of 6-23 us each at 64 leaves).  Same d2 and statistics bit for bit
    // as gather + combine + normalise + combine.
    const bool taps = c->stem_fused && c->stem_taps && (!P.split || nt >= c->n_cus);
    if (taps || (c->stem_fused && (!P.split || c->stem_small_fused))) {
        StemFusedArgs F{};
        F.idx = P.d_idx, F.T = w["ds.lut"], F.bias = w["ds.b"], F.gamma = w["dg0.w"], F.beta = w["dg0.b"], F.d2 = a["d_d2"];
        F.out_mean = a["st_b.mean"], F.out_rstd = a["st_b.rstd"], F.ystem_dbg = c->debug ? a["d_ystem"] : nullptr;
        F.steps = steps, F.grp_start = grp(c, "steps.k3s1_4.grp"), F.n_steps = c->nsteps["steps.k3s1_4"];
        F.n_leaves = P.n, F.n_tiles = nt;
        P.L.run(P.split ? "dec_stem_gn_s" : "dec_stem_gn", [&] {
            if (taps) hipLaunchKernelGGL(k_stem_taps, dim3(std::min(nt, c->n_cus)), dim3(512), LDS_STEM_TAPS, P.s, F);
            else if (P.split && nt <= 64) hipLaunchKernelGGL(stem_fused_k<16>, dim3(8 * nt), dim3(1024), 0, P.s, F);   // up to 2048 leaves: sixteen waves, half the gather chain each
            else hipLaunchKernelGGL(stem_fused_k<8>, dim3(8 * nt), dim3(512), 0, P.s, F);
        });
        return;
    }
    ConvArgs A{};
    A.in = a["d_ystem"], A.out = a["d_d2"], A.in_mean = a["st_a.mean"], A.in_rstd = a["st_a.rstd"];
    A.in_gamma = w["dg0.w"], A.in_beta = w["dg0.b"], A.n_tiles = nt;
    if (!P.split) {
        P.L.run("dec_stem", [&] {
            hipLaunchKernelGGL(stem_lut_k, dim3(2 * nt), dim3(256), 0, P.s, P.d_idx, w["ds.lut"], w["ds.b"], a["d_ystem"], a["st_a.mean"], a["st_a.rstd"],
                               steps, c->nsteps["steps.k3s1_4"], P.n, nt, (const int*)nullptr);
        });
        A.out_mean = a["st_b.mean"], A.out_rstd = a["st_b.rstd"];
        P.L.run("dec_gn_relu_stats", [&] { hipLaunchKernelGGL((gn_relu_stats_k<64, 64, 8>), dim3(g4), dim3(256), 0, P.s, A); });
        return;
    }
    P.L.run("dec_stem_s", [&] {
        hipLaunchKernelGGL(stem_lut_k, dim3(2 * nt, split_factor(2 * nt, 2, 16, 2048)), dim3(256), 0, P.s, P.d_idx, w["ds.lut"], w["ds.b"], a["d_ystem"], (float*)nullptr, (float*)nullptr,
                           steps, c->nsteps["steps.k3s1_4"], P.n, nt, grp(c, "steps.k3s1_4.grp"), part_s(c), part_q(c));
    });
    combine_pairs(P, "dec_stats_ystem", a["st_a.mean"], a["st_a.rstd"]);
    A.part_s = part_s(c), A.part_q = part_q(c);
    P.L.run("dec_gn_relu_d2", [&] { hipLaunchKernelGGL((gn_relu_stats_k<64, 64, 8>), dim3(g4, split_factor(g4, 2, 16, 1024)), dim3(256), 0, P.s, A); });
    combine_pairs(P, "dec_stats_d2", a["st_b.mean"], a["st_b.rstd"]);
}

// the 64-channel residual block: d_d2 (+ its statistics in st_b) -> d_y4 (gn2's statistics in st_a) -> d_x6 with the channel sums and
// attention gates the tail needs
void dec_res64(DecPass& P)
{
    vqhip_codec* c = P.c;
    auto &a = c->act, &w = c->dw;
    const int nt = P.nt;
    if (P.precision == VQHIP_PRECISION_BF16) {
        // ONE kernel per conv whatever the batch size, so a leaf's bits do not depend on the launch path.  Each conv stores per-block
        // partials and the combine kernels of the position-split path finish them.
        d64b::Args B{};
        B.in = a["d_d2"], B.out = a["d_y4"], B.wf = c->bf_r64c1, B.bias = w["r64c1.braw"];
        B.in_mean = a["st_b.mean"], B.in_rstd = a["st_b.rstd"], B.in_gamma = w["r64g1.w"], B.in_beta = w["r64g1.b"];
        B.part_s = part_s(c), B.part_q = part_q(c);
        P.L.run("dec_res64_conv1_bf16", [&] { hipLaunchKernelGGL(d64b::conv_k<false>, dim3(2 * nt), dim3(d64b::THREADS), d64b::LDS_BYTES, P.s, B); });
        combine_pairs(P, "dec_stats_y4", a["st_a.mean"], a["st_a.rstd"]);
        B.in = a["d_y4"], B.out = a["d_x6"], B.wf = c->bf_r64c2, B.bias = w["r64c2.braw"], B.skip = a["d_d2"];
        B.in_mean = a["st_a.mean"], B.in_rstd = a["st_a.rstd"], B.in_gamma = w["r64g2.w"], B.in_beta = w["r64g2.b"];
        B.part_s = nullptr, B.part_q = nullptr, B.part_c = a["part_c"];
        P.L.run("dec_res64_conv2_bf16", [&] { hipLaunchKernelGGL(d64b::conv_k<true>, dim3(2 * nt), dim3(d64b::THREADS), d64b::LDS_BYTES, P.s, B); });
        combine_csum<64>(P, "dec_csum_x6", a["csum"], w["dfc0"], w["dfc2"]);
        return;
    }
    const float* steps = w["steps.rows_k3_4"];
    ConvArgs A{};
    A.in = a["d_d2"], A.out = a["d_y4"], A.wfrag = w["r64c1.w16"], A.bias_frag = w["r64c1.braw"];
    A.in_mean = a["st_b.mean"], A.in_rstd = a["st_b.rstd"], A.in_gamma = w["r64g1.w"], A.in_beta = w["r64g1.b"], A.n_tiles = nt;
    A.n_steps = c->nsteps["steps.rows_k3_4"], A.n_taps = 27;
    ConvArgs B{};
    B.in = a["d_y4"], B.out = a["d_x6"], B.wfrag = w["r64c2.w16"], B.bias_frag = w["r64c2.braw"], B.skip = a["d_d2"];
    B.in_mean = a["st_a.mean"], B.in_rstd = a["st_a.rstd"], B.in_gamma = w["r64g2.w"], B.in_beta = w["r64g2.b"], B.n_tiles = nt;
    B.n_steps = A.n_steps, B.n_taps = 27;
    if (!P.split) {
        A.out_mean = a["st_a.mean"], A.out_rstd = a["st_a.rstd"];
        P.L.run("dec_res64_conv1", [&] { launch_rows<DecR64C1Full>(P.s, A, steps, nt); });
        B.out_csum = a["csum"];
        P.L.run("dec_res64_conv2", [&] { launch_rows<DecR64C2Full>(P.s, B, steps, nt); });
        return;
    }
    const int gh = (2 * nt + 7) / 8, psr = split_factor(gh, 4, 16, 512);   // 8 half tiles per workgroup, 16 output rows to split
    const bool ms = gh * psr * 4 <= 1024;   // up to 2048 leaves (measured): also split the 64 couts over gridDim.z
    const bool r64res = c->r64s_resident;
    A.grp_start = B.grp_start = grp(c, "steps.rows_k3_4.grp");
    A.part_s = part_s(c), A.part_q = part_q(c);
    P.L.run("dec_res64_conv1_s", [&] {
        if (ms && r64res) launch_rows<DecR64C1Split4Res>(P.s, A, steps, nt, psr);
        else if (ms) launch_rows<DecR64C1Split4>(P.s, A, steps, nt, psr);
        else launch_rows<DecR64C1Split>(P.s, A, steps, nt, psr);
    });
    combine_pairs(P, "dec_stats_y4", a["st_a.mean"], a["st_a.rstd"]);
    B.part_c = a["part_c"];
    P.L.run("dec_res64_conv2_s", [&] {
        if (ms && r64res) launch_rows<DecR64C2Split4Res>(P.s, B, steps, nt, psr);
        else if (ms) launch_rows<DecR64C2Split4>(P.s, B, steps, nt, psr);
        else launch_rows<DecR64C2Split>(P.s, B, steps, nt, psr);
    });
    combine_csum<64>(P, "dec_csum_x6", a["csum"], w["dfc0"], w["dfc2"]);
}

// attention gates + up conv + final conv + sigmoid, folded: d_x6 -> voxels
void dec_tail(DecPass& P)
{
    vqhip_codec* c = P.c;
    auto &a = c->act, &w = c->dw;
    const int nt = P.nt;
    ConvArgs A{};
    A.in = a["d_x6"], A.out = P.d_out, A.wfrag = w["tail.w"], A.bias_frag = w["tail.b"];
    A.se_csum = a["csum"], A.se_fc0 = w["dfc0"], A.se_fc2 = w["dfc2"], A.n_tiles = nt, A.n_leaves = P.n;
    A.n_steps = c->nsteps["steps.tail"], A.n_taps = 0;
    if (P.split) {
        A.grp_start = grp(c, "steps.tail.grp");
        A.se_gate = a["gate"];   // computed once per tile by dec_csum_x6
        // a few tiles: sixteen waves per (tile, slab) on the 16x16x4 MFMA (a quarter of the serial chain per wave)
        if (nt <= c->tail16_tiles) {
            A.wfrag = w["tail.w16"], A.bias_frag = w["tail.braw"];
            P.L.run("dec_tail_s", [&] { hipLaunchKernelGGL(tail_small16_k<4>, dim3(nt, 4, 4), dim3(256), 0, P.s, A); });
        } else {
            P.L.run("dec_tail_s", [&] { hipLaunchKernelGGL(tail_small_k<false>, dim3(nt, 4), dim3(256), 0, P.s, A); });
        }
    } else if (c->tail_rows) {
        A.wfrag = c->tail_groups ? w["tail.wgroups"] : w["tail.wrows"], A.bias_frag = w["tail.braw"];
        if (c->tail_groups) P.L.run("dec_tail_groups", [&] { hipLaunchKernelGGL(tail_groups16_k<0>, dim3((2 * nt + 7) / 8), dim3(512), LDS_TAIL_GROUPS, P.s, A); });
        else if (c->tail_rows32) P.L.run("dec_tail_rows32", [&] { hipLaunchKernelGGL(tail_rows32_k<0>, dim3((nt + 3) / 4), dim3(256), LDS_TAIL_ROWS, P.s, A); });
        else P.L.run("dec_tail", [&] { hipLaunchKernelGGL(tail_rows16_k<0>, dim3((2 * nt + 7) / 8), dim3(512), LDS_TAIL_ROWS, P.s, A); });
    } else {
        P.L.run("dec_tail_slab", [&] { launch_mfma32<DecTailSlab>(P.s, A, w["steps.tail"], nt); });
    }
}

// precision: VQHIP_PRECISION_* of the two 64 -> 64 convs.  Only the plain decode entry points pass the handle's mode; every call that
// states or checks an error bound (bounded, residual, rate, round trip), training and vqhip_multi_* take the default.
int decode_chunk(vqhip_codec* c, const uint8_t* d_idx, int64_t n, float* d_out, hipStream_t s, int precision = VQHIP_PRECISION_FP32)
{
    int rc = ensure_workspace(c, n);
    if (rc) return rc;
    if (precision == VQHIP_PRECISION_BF16 && (rc = ensure_dec_bf16_frags(c, s))) return rc;
    const int nt = (int)((n + 31) / 32);
    DecPass P{{c, s, {c, s, n}, n, nt, use_split(c, nt, true), precision}, d_idx, d_out};
    dec_stem(P);
    dec_res64(P);
    dec_tail(P);
    return P.L.rc;
}

int ensure_io(vqhip_codec* c, int64_t n)
{
    if (!c->s_in) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
        HIPCHK(c, hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_in[i], hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_done[i], hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_out[i], hipEventDisableTiming));
        }
    }
    for (int i = 0; i < 2; ++i) {
        if (int rc = ensure(c, c->dev_leaves[i], (size_t)n * 512, "the device leaf slot")) return rc;
        if (int rc = ensure(c, c->dev_idx[i], (size_t)n * 64, "the device index slot")) return rc;
        if (int rc = ensure(c, c->pin_out[i], (size_t)n * 2048, "the pinned result slot")) return rc;
    }
    return VQHIP_OK;
}

// pinned input staging (leaf blocks: gathered leaf buffers or the caller's pageable block; index blocks of single-chunk decodes)
int ensure_stage(vqhip_codec* c, size_t bytes)
{
    for (int i = 0; i < 2; ++i)
        if (int rc = ensure(c, c->pin_in[i], bytes, "the pinned input stage")) return rc;
    return VQHIP_OK;
}

// Cap on the copy threads one calling thread may fan out to (host_parallel_for).  Default 16; the in-process multi-device front
// end lowers it per device worker so that G devices never run more than min(cores, 64) copy threads together; the environment
// variable VQHIP_COPY_THREADS overrides both.
thread_local int g_copy_threads_cap = 16;

int copy_threads_cap()
{
    static const int env = [] {   // (the switch table's strict integer: a malformed value means "not set" here and refuses every vqhip_create)
        long v[2];
        int n = 0;
        std::string err;
        const bool ok = vqsw::parse_switch_integers(*vqsw::find_switch("VQHIP_COPY_THREADS"), std::getenv("VQHIP_COPY_THREADS"), 0, v, n, err) == VQHIP_OK;
        return ok && n ? (int)v[0] : 0;
    }();
    return env ? env : g_copy_threads_cap;
}

// parallel-for over [0,n) on host threads (the library's stand-in for the orchestrator's tbb::parallel_for)
template <typename F>
void host_parallel_for(int64_t n, F&& f, int64_t grain = 2048)
{
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)hw / 2, (int64_t)copy_threads_cap(), n / grain}));
    if (nt <= 1) {
        f(0, n);
        return;
    }
    std::vector<std::thread> th;
    const int64_t per = (n + nt - 1) / nt;
    for (int t = 0; t < nt; ++t) th.emplace_back([=, &f] { f(std::min(n, t * per), std::min(n, (t + 1) * per)); });
    for (auto& x : th) x.join();
}

// multi-threaded memcpy for the large host-side block copies (pageable <-> pinned staging): one thread tops out
// near 10 GB/s, below both the PCIe link and the kernels' leaf rate
void host_parallel_copy(void* dst, const void* src, size_t bytes)
{
    constexpr size_t BLK = size_t(1) << 20;
    const int64_t nb = (int64_t)((bytes + BLK - 1) / BLK);
    char* d = static_cast<char*>(dst);
    const char* s = static_cast<const char*>(src);
    host_parallel_for(nb, [=](int64_t a, int64_t b) {
        const size_t lo = (size_t)a * BLK, hi = std::min(bytes, (size_t)b * BLK);
        if (hi > lo) std::memcpy(d + lo, s + lo, hi - lo);
    }, 4);
}

int refresh_tables(vqhip_codec* c)
{
    std::vector<float> E(256 * 128);
    HIPCHK(c, hipDeviceSynchronize());  // the codebook may have been updated on a caller's stream
    HIPCHK(c, hipMemcpy(E.data(), c->dw["cb"], E.size() * sizeof(float), hipMemcpyDeviceToHost));
    int rc;
    if (c->weights_stale) {
        // full training changed the encoder / decoder weights: the device fragments were rebuilt after the optimizer step;
        // what is folded on the host in fp64 (decoder tail, projection inside the VQ search) is rebuilt here from the parameters
        HIPCHK(c, hipMemcpy(c->h_params.data(), c->ft_P, c->h_params.size() * sizeof(float), hipMemcpyDeviceToHost));
        auto hp = [&](const char* n) { return c->h_params.data() + c->p_off.at(n).first; };
        c->h_proj_w.assign(hp("encoder.proj.weight"), hp("encoder.proj.weight") + 128 * 32);
        c->h_proj_b.assign(hp("encoder.proj.bias"), hp("encoder.proj.bias") + 128);
        if ((rc = build_folded_tail(c, hp("decoder.up_conv.weight"), hp("decoder.up_conv.bias"), hp("decoder.final.weight"), hp("decoder.final.bias")))) return rc;
        c->weights_stale = false;
    }
    if ((rc = build_vq_fold(c, E.data()))) return rc;
    hipLaunchKernelGGL(build_stem_lut_k, dim3(27 * 256), dim3(64), 0, c->stream, c->dw["ds.w"], c->dw["cb"], c->dw["ds.lut"]);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tables_stale = false;
    c->bf_stale = true;   // every table that follows the live parameters is rebuilt after a training update, the bf16 decode mode's at its next call
    c->bf_enc_stale = true;   // ... and the bf16 encode mode's (ensure_enc_bf16_frags)
    return VQHIP_OK;
}

// inference entry points after codebook training: the folded VQ tables and the decoder stem table follow the live codebook
int ensure_tables(vqhip_codec* c)
{
    return c->tables_stale ? refresh_tables(c) : VQHIP_OK;
}

// Host-side pipeline shared by every entry point that takes host memory (the path the reference orchestrator
// calls, VQVAECodec.cpp:120,178).  Chunk i: produce() -> H2D on s_in -> kernels on the compute stream -> D2H into
// pinned memory on s_out; consume() of chunk i-1 runs on the calling thread while the GPU works on chunk i.
// encode: in = leaves (2048 B/leaf), out = indices (64 B/leaf); decode: the reverse.
//   produce(o, m, stage): returns the host address of chunk [o, o+m)'s input; `stage` is this slot's pinned
//                         buffer (nullptr unless want_stage) which produce may fill and return.
//   consume(chunk): the chunk's output lies in pinned memory at chunk.result.
//   stage (optional): more work behind every chunk, built where its buffers live (vq_bounded.inc, vq_residual.inc).
struct PipeChunk {
    int64_t o, m;         // leaves [o, o + m) of the call
    int slot;             // the I/O slot they went through: its buffers are not written again before consume() returns
    const void* result;
    hipStream_t idle;     // a stream with nothing queued while consume() runs, for a consumer that fetches more of the slot
};
using ProduceFn = std::function<const void*(int64_t, int64_t, void*)>;
using ConsumeFn = std::function<int(const PipeChunk&)>;
struct PipeStage {   // empty members are skipped
    std::function<int(int64_t step)> ensure;                                    // buffers for chunks of <= step leaves, both slots
    std::function<int(int64_t o, int64_t m, int slot, hipStream_t s)> device;   // on the compute stream, behind the chunk's encode / decode
    std::function<hipError_t(int64_t m, int slot, hipStream_t s)> copy_out;     // on the output stream, behind the result's D2H
};

int run_pipeline(vqhip_codec* c, bool is_encode, int64_t n, int64_t step, bool want_stage, const ProduceFn& produce, const ConsumeFn& consume,
                 const PipeStage* stage = nullptr, int decode_precision = VQHIP_PRECISION_FP32, int encode_precision = VQHIP_PRECISION_FP32)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->chunk_fitted) fit_chunk_to_free_memory(c), c->chunk_fitted = true;
    step = std::min(step > 0 ? std::min(step, c->chunk) : c->chunk, n);
    // A call that fits ONE chunk but is large (a 65 536-leaf batch from the orchestrator loop or the leaf-pointer entry points) would run
    // gather -> H2D -> kernels -> D2H -> scatter back to back (17.5 ms for 65 536 leaves against a 9.8 ms device pass): it is cut into
    // host_split pieces so that the host phases of one piece overlap the device pass of its neighbours.  Results never depend on the cut.
    if (n <= step && c->host_split > 1 && n >= 2 * c->host_split_min && !c->debug) {   // (debug mode keeps a call's activations whole for vqhip_debug_fetch)
        const int64_t pieces = std::min<int64_t>(c->host_split, n / c->host_split_min);
        step = ((n + pieces - 1) / pieces + 31) / 32 * 32;
    }
    int rc = ensure_tables(c);
    if (!rc) rc = ensure_io(c, step);
    if (rc) return rc;
    const size_t in_b = is_encode ? 2048 : 64, out_b = is_encode ? 64 : 2048;
    if (want_stage && (rc = ensure_stage(c, (size_t)step * in_b))) return rc;
    if (stage && stage->ensure && (rc = stage->ensure(step))) return rc;
    // what every chunk gets, in either arrangement below: its kernels on the compute stream ...
    auto chunk_work = [&](int64_t o, int64_t m, int slot) -> int {
        int r = is_encode ? encode_chunk(c, c->dev_leaves[slot], m, c->dev_idx[slot], c->stream, nullptr, encode_precision)
                          : decode_chunk(c, c->dev_idx[slot], m, c->dev_leaves[slot], c->stream, decode_precision);
        if (!r && stage && stage->device) r = stage->device(o, m, slot, c->stream);
        return r;
    };
    // ... and its results on their way to pinned memory on stream s, the stage's behind the main one
    auto copy_out = [&](int64_t m, int slot, hipStream_t s) -> hipError_t {
        const void* d_out = is_encode ? (const void*)c->dev_idx[slot] : (const void*)c->dev_leaves[slot];
        hipError_t e = hipMemcpyAsync(c->pin_out[slot], d_out, (size_t)m * out_b, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && stage && stage->copy_out) e = stage->copy_out(m, slot, s);
        return e;
    };
    if (n <= step) {
        // One chunk: there is nothing to overlap — H2D, kernels and D2H go down the compute stream in order and the call waits once.
        // (The three-stream form below costs such a call three cross-stream event hand-overs and as many extra API calls: the SOP's
        // default batch of 64 leaves is a 0.14-0.20 ms pass, so they showed: 0.26 / 0.21 ms per call through the adapter.)
        void* d_in = is_encode ? (void*)c->dev_leaves[0] : (void*)c->dev_idx[0];
        const void* src = produce(0, n, want_stage ? c->pin_in[0] : nullptr);
        if (!src) return c->err.empty() ? fail(c, VQHIP_ERR_INVALID, "input source failed") : VQHIP_ERR_INVALID;
        auto sync_fail = [&](int code) {   // leave no copy in flight that references caller or slot memory
            hipStreamSynchronize(c->stream);
            return code;
        };
        hipError_t e = hipMemcpyAsync(d_in, src, (size_t)n * in_b, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return sync_fail(fail(c, VQHIP_ERR_DEVICE, std::string("hipMemcpyAsync H2D: ") + hipGetErrorString(e)));
        if ((rc = chunk_work(0, n, 0))) return sync_fail(rc);
        e = copy_out(n, 0, c->stream);
        if (e != hipSuccess) return sync_fail(fail(c, VQHIP_ERR_DEVICE, std::string("hipMemcpyAsync D2H: ") + hipGetErrorString(e)));
        e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, VQHIP_ERR_DEVICE, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
        return consume({0, n, 0, c->pin_out[0], c->stream});
    }
    int64_t prev_off = -1, prev_m = 0;
    int prev_slot = 0, i = 0;
    auto drain = [&]() -> int {
        if (prev_off < 0) return VQHIP_OK;
        HIPCHK(c, hipEventSynchronize(c->ev_out[prev_slot]));
        const int64_t o = prev_off;
        prev_off = -1;
        return consume({o, prev_m, prev_slot, c->pin_out[prev_slot], c->s_out});   // s_out is idle here: the next chunk's copies are queued after this drain
    };
    auto abort_run = [&](int code) {  // leave no work in flight that still references caller memory
        hipStreamSynchronize(c->s_in);
        hipStreamSynchronize(c->stream);
        hipStreamSynchronize(c->s_out);
        return code;
    };
    // inside the loop every error exit goes through abort_run: async copies may still reference caller / slot memory
#define PIPECHK(call)                                                        \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) {                                              \
            c->err = std::string(#call) + ": " + hipGetErrorString(e_);      \
            return abort_run(VQHIP_ERR_DEVICE);                              \
        }                                                                    \
    } while (0)
    for (int64_t o = 0; o < n; o += step, ++i) {
        const int64_t m = std::min(step, n - o);
        const int slot = i & 1;
        void* d_in = is_encode ? (void*)c->dev_leaves[slot] : (void*)c->dev_idx[slot];
        if (i >= 2) PIPECHK(hipStreamWaitEvent(c->s_in, c->ev_done[slot], 0));  // slot's previous input consumed
        if (want_stage && i >= 2) PIPECHK(hipEventSynchronize(c->ev_in[slot]));  // the H2D that last read this pinned buffer is done
        const void* src = produce(o, m, want_stage ? c->pin_in[slot] : nullptr);
        if (!src) return abort_run(c->err.empty() ? fail(c, VQHIP_ERR_INVALID, "input source failed") : VQHIP_ERR_INVALID);
        PIPECHK(hipMemcpyAsync(d_in, src, (size_t)m * in_b, hipMemcpyHostToDevice, c->s_in));
        PIPECHK(hipEventRecord(c->ev_in[slot], c->s_in));
        PIPECHK(hipStreamWaitEvent(c->stream, c->ev_in[slot], 0));
        if (i >= 2) PIPECHK(hipStreamWaitEvent(c->stream, c->ev_out[slot], 0));  // slot's previous output drained to pinned
        if ((rc = chunk_work(o, m, slot))) return abort_run(rc);
        PIPECHK(hipEventRecord(c->ev_done[slot], c->stream));
        if ((rc = drain())) return abort_run(rc);  // chunk i-1 -> caller, overlapped with chunk i on the GPU
        PIPECHK(hipStreamWaitEvent(c->s_out, c->ev_done[slot], 0));
        PIPECHK(copy_out(m, slot, c->s_out));
        PIPECHK(hipEventRecord(c->ev_out[slot], c->s_out));
        prev_off = o, prev_m = m, prev_slot = slot;
    }
    if ((rc = drain())) return abort_run(rc);
    PIPECHK(hipStreamSynchronize(c->stream));
#undef PIPECHK
    return VQHIP_OK;
}

// gather per-leaf buffers into a contiguous (pinned) block / scatter a block into per-leaf buffers
void gather_leaves(float* stage, const float* const* lp, int64_t m)
{
    host_parallel_for(m, [=](int64_t a, int64_t b) {
        for (int64_t l = a; l < b; ++l) std::memcpy(stage + l * 512, lp[l], 2048);
    });
}
void scatter_leaves(float* const* dst, const float* src, int64_t m)
{
    host_parallel_for(m, [=](int64_t a, int64_t b) {
        for (int64_t l = a; l < b; ++l) std::memcpy(dst[l], src + l * 512, 2048);
    });
}

// contiguous blocks or leaf-pointer arrays (vqhip_encode / _decode / _encode_leaves / _decode_leaves)
int run_host_pipeline(vqhip_codec* c, bool is_encode, const void* in, void* out, int64_t n, const float* const* in_ptrs = nullptr,
                      float* const* out_ptrs = nullptr, int decode_precision = VQHIP_PRECISION_FP32, int encode_precision = VQHIP_PRECISION_FP32)
{
    const size_t in_b = is_encode ? 2048 : 64, out_b = is_encode ? 64 : 2048;
    // leaf blocks go through pinned staging (copied by threads when large), not the runtime's pageable-copy path; a call that fits one
    // chunk stages whatever it gets (decode: 64 B per leaf) so that its H2D is an asynchronous copy on the compute stream
    const bool stage_in = in_ptrs || (is_encode && n >= 4096) || n <= c->chunk;
    return run_pipeline(
        c, is_encode, n, 0, stage_in,
        [=](int64_t o, int64_t m, void* stage) -> const void* {
            const void* src = static_cast<const char*>(in) + (size_t)o * in_b;
            if (!stage) return src;
            if (in_ptrs) gather_leaves(static_cast<float*>(stage), in_ptrs + o, m);
            else host_parallel_copy(stage, src, (size_t)m * in_b);
            return stage;
        },
        [=](const PipeChunk& ch) -> int {
            if (out_ptrs) scatter_leaves(out_ptrs + ch.o, static_cast<const float*>(ch.result), ch.m);
            else host_parallel_copy(static_cast<char*>(out) + (size_t)ch.o * out_b, ch.result, (size_t)ch.m * out_b);
            return VQHIP_OK;
        },
        nullptr, decode_precision, encode_precision);
}

}  // namespace

// =============================== C ABI ===============================
extern "C" {

const char* vqhip_version(void) { return "vqvdb-hip 0.1 (gfx950)"; }

const char* vqhip_last_error(const vqhip_codec* codec) { return codec ? codec->err.c_str() : g_create_error.c_str(); }

int vqhip_create(const char* pack_path, const void* pack_bytes, size_t pack_size, int device_id, vqhip_codec** out)
{
    if (!out) return fail(nullptr, VQHIP_ERR_INVALID, "vqhip_create: out is NULL");
    *out = nullptr;
    std::vector<unsigned char> file;
    const unsigned char* p = static_cast<const unsigned char*>(pack_bytes);
    size_t n = pack_size;
    if (pack_path) {
        std::ifstream f(pack_path, std::ios::binary);
        if (!f) return fail(nullptr, VQHIP_ERR_MODEL, std::string("Model file not found at path: ") + pack_path);
        file.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
        p = file.data();
        n = file.size();
    }
    if (!p || !n) return fail(nullptr, VQHIP_ERR_MODEL, "vqhip_create: no weight pack given (embedded model absent from this build)");
    std::map<std::string, PackTensor> pk;
    std::string err;
    if (!parse_pack(p, n, pk, err)) return fail(nullptr, VQHIP_ERR_MODEL, err);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, VQHIP_ERR_DEVICE, std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0"));
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, VQHIP_ERR_INVALID, "vqhip_create: device_id out of range");
    vqhip_codec* c = new vqhip_codec();
    c->device = device_id;
    auto bail = [&](int rc) {
        g_create_error = c->err;
        vqhip_destroy(c);
        return rc;
    };
    if (hipSetDevice(device_id) != hipSuccess) {
        c->err = "hipSetDevice failed";
        return bail(VQHIP_ERR_DEVICE);
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        c->err = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
        return bail(VQHIP_ERR_DEVICE);
    }
    c->n_cus_device = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // every VQHIP_* switch, read here and nowhere later (vq_switches.h: the table, the legal values, what each selects)
    if (int rc = parse_switches(*c, [](const char* name) -> const char* { return std::getenv(name); }, c->n_cus_device, c->err)) return bail(rc);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        c->err = "hipStreamCreate failed";
        return bail(VQHIP_ERR_DEVICE);
    }
    int rc = load_weights(c, pk);
    if (rc) return bail(rc);
    if ((rc = init_kernel_attrs(c))) return bail(rc);
    *out = c;
    return VQHIP_OK;
}

void vqhip_destroy(vqhip_codec* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (auto& kv : c->dw) hipFree(kv.second);
    for (hipEvent_t e : c->ft_ev) hipEventDestroy(e);
    if (c->ft_side) hipStreamDestroy(c->ft_side);
    if (c->ft_red) hipStreamDestroy(c->ft_red);
    if (c->ft_red_shared) hipStreamDestroy(c->ft_red_shared);
    for (int i = 0; i < 2; ++i) {
        if (c->ev_in[i]) hipEventDestroy(c->ev_in[i]);
        if (c->ev_done[i]) hipEventDestroy(c->ev_done[i]);
        if (c->ev_out[i]) hipEventDestroy(c->ev_out[i]);
    }
    if (c->s_in) hipStreamDestroy(c->s_in);
    if (c->s_out) hipStreamDestroy(c->s_out);
    for (auto& t : c->timers) {
        hipEventDestroy(t.start);
        hipEventDestroy(t.stop);
    }
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;   // the buffers go in the struct's destructor, with the device still current
}

int vqhip_latent_shape(const vqhip_codec* c, int64_t out[3])
{
    if (!c || !out) return VQHIP_ERR_INVALID;
    out[0] = out[1] = out[2] = 4;  // 8^3 leaf through the k4/s2 down-conv (weights validated at create)
    return VQHIP_OK;
}

int vqhip_set_chunk_leaves(vqhip_codec* c, int64_t chunk)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (chunk < 32 || chunk > (1 << 22)) return fail(c, VQHIP_ERR_INVALID, "chunk_leaves must be in [32, 4194304]");
    c->chunk = (chunk + 31) / 32 * 32;
    c->chunk_fitted = false;   // re-checked against the free device memory at the next call
    return VQHIP_OK;
}

int vqhip_set_small_batch_tiles(vqhip_codec* c, int tiles)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (tiles < -1) return fail(c, VQHIP_ERR_INVALID, "small_batch_tiles must be >= 0, or -1 for the automatic choice");
    c->split_tiles = tiles;
    return VQHIP_OK;
}

int vqhip_reserve(vqhip_codec* c, int64_t n)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 1) return fail(c, VQHIP_ERR_INVALID, "reserve: n_leaves < 1");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->chunk_fitted) fit_chunk_to_free_memory(c), c->chunk_fitted = true;
    const int64_t m = std::min(n, c->chunk);
    int rc = ensure_workspace(c, m);
    if (!rc) rc = ensure_io(c, m);
    if (!rc) rc = ensure_stage(c, (size_t)m * 2048);
    return rc;
}

int64_t vqhip_workspace_bytes(const vqhip_codec* c) { return c ? (int64_t)c->ws.bytes() : -1; }

int64_t vqhip_chunk_leaves(const vqhip_codec* c) { return c ? c->chunk : -1; }

int vqhip_compute_units(const vqhip_codec* c, int* device, int* in_use)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (device) *device = c->n_cus_device;
    if (in_use) *in_use = c->n_cus;
    return VQHIP_OK;
}

int vqhip_encode_device(vqhip_codec* c, const float* d_leaves, int64_t n, uint8_t* d_idx, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!d_leaves || !d_idx || n < 1) return fail(c, VQHIP_ERR_INVALID, "encode: null pointer or n_leaves < 1");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->chunk_fitted) fit_chunk_to_free_memory(c), c->chunk_fitted = true;
    if (int trc = ensure_tables(c)) return trc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        int rc = encode_chunk(c, d_leaves + o * 512, m, d_idx + o * 64, s, nullptr, c->encode_precision);
        if (rc) return rc;
    }
    return VQHIP_OK;
}

int vqhip_decode_device(vqhip_codec* c, const uint8_t* d_idx, int64_t n, float* d_out, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!d_idx || !d_out || n < 1) return fail(c, VQHIP_ERR_INVALID, "decode: null pointer or n_leaves < 1");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->chunk_fitted) fit_chunk_to_free_memory(c), c->chunk_fitted = true;
    if (int trc = ensure_tables(c)) return trc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    for (int64_t o = 0; o < n; o += c->chunk) {
        const int64_t m = std::min(c->chunk, n - o);
        int rc = decode_chunk(c, d_idx + o * 64, m, d_out + o * 512, s, c->decode_precision);
        if (rc) return rc;
    }
    return VQHIP_OK;
}

int vqhip_encode(vqhip_codec* c, const float* leaves, int64_t n, uint8_t* indices)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!leaves || !indices || n < 1) return fail(c, VQHIP_ERR_INVALID, "encode: null pointer or n_leaves < 1");
    return run_host_pipeline(c, true, leaves, indices, n, nullptr, nullptr, VQHIP_PRECISION_FP32, c->encode_precision);
}

int vqhip_decode(vqhip_codec* c, const uint8_t* indices, int64_t n, float* leaves)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!leaves || !indices || n < 1) return fail(c, VQHIP_ERR_INVALID, "decode: null pointer or n_leaves < 1");
    return run_host_pipeline(c, false, indices, leaves, n, nullptr, nullptr, c->decode_precision);
}

int vqhip_encode_leaves(vqhip_codec* c, const float* const* leaf_ptrs, int64_t n, uint8_t* indices)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!leaf_ptrs || !indices || n < 1) return fail(c, VQHIP_ERR_INVALID, "encode_leaves: null pointer or n_leaves < 1");
    return run_host_pipeline(c, true, nullptr, indices, n, leaf_ptrs, nullptr, VQHIP_PRECISION_FP32, c->encode_precision);
}

int vqhip_decode_leaves(vqhip_codec* c, const uint8_t* indices, int64_t n, float* const* leaf_ptrs)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!leaf_ptrs || !indices || n < 1) return fail(c, VQHIP_ERR_INVALID, "decode_leaves: null pointer or n_leaves < 1");
    return run_host_pipeline(c, false, indices, nullptr, n, nullptr, leaf_ptrs, c->decode_precision);
}

// ---- codebook training (stage 1): VectorQuantizerEMA.forward in training mode, VQVAE_v2.py:107-156 ----
int vqhip_train_begin(vqhip_codec* c, const float* cluster_size, const float* embed_avg)
{
    if (!c) return VQHIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if (!c->training) {
        if ((rc = upload(c, "tr.efrag", std::vector<float>(16 * 8 * 64 * 4, 0.0f)))) return rc;
        if ((rc = upload(c, "tr.ee", std::vector<float>(256, 0.0f)))) return rc;
    }
    std::vector<float> cs(256, 1.0f), avg(256 * 128);  // reference initial buffers (VQVAE_v2.py:104-105)
    if (cluster_size) cs.assign(cluster_size, cluster_size + 256);
    if (embed_avg) avg.assign(embed_avg, embed_avg + 256 * 128);
    else HIPCHK(c, hipMemcpy(avg.data(), c->dw["cb"], avg.size() * sizeof(float), hipMemcpyDeviceToHost));
    if ((rc = upload(c, "tr.cs", cs))) return rc;
    if ((rc = upload(c, "tr.avg", avg))) return rc;
    c->training = true;
    return VQHIP_OK;
}

// scratch of the codebook statistics (tr_part): per-(code, segment) partial sums, squared errors and counts, then the per-segment member
// lists of vq_ema_lists_k and their (start, count) table
struct EmaScratch {
    float* part;
    double* sqpart;
    int* cntpart;
    unsigned short* lists;
    int* starts;
};
size_t ema_scratch_bytes(int n_seg)
{
    return (size_t)256 * n_seg * (128 * sizeof(float) + sizeof(double) + sizeof(int)) + (size_t)n_seg * VQ_SEG_ROWS * sizeof(unsigned short) +
           (size_t)n_seg * 256 * 2 * sizeof(int);
}
EmaScratch ema_scratch(char* base, int n_seg)
{
    EmaScratch e;
    e.part = reinterpret_cast<float*>(base);
    e.sqpart = reinterpret_cast<double*>(base + (size_t)256 * n_seg * 128 * sizeof(float));
    e.cntpart = reinterpret_cast<int*>(base + (size_t)256 * n_seg * (128 * sizeof(float) + sizeof(double)));
    e.lists = reinterpret_cast<unsigned short*>(base + (size_t)256 * n_seg * (128 * sizeof(float) + sizeof(double) + sizeof(int)));
    e.starts = reinterpret_cast<int*>(reinterpret_cast<char*>(e.lists) + (size_t)n_seg * VQ_SEG_ROWS * sizeof(unsigned short));
    return e;
}
// encodings_sum / dw / squared error of one batch into `stats` (VQ_STATS_* layout): member lists per (segment, code), ordered partial sums,
// ordered reduction.  VQHIP_TRAIN_EMA=scan: every (code, segment) wave scans the segment's indices itself (rounds 1-4; the same bits)
void launch_vq_ema(vqhip_codec* c, hipStream_t s, const float* z, const uint8_t* idx, int64_t rows, int n_seg, float* stats)
{
    const EmaScratch e = ema_scratch(c->tr_part, n_seg);
    if (c->train_ema_lists) {
        hipLaunchKernelGGL(vq_ema_lists_k, dim3(n_seg), dim3(64), 0, s, idx, rows, e.lists, e.starts);
        hipLaunchKernelGGL(vq_ema_gather_k, dim3(256, (n_seg + 15) / 16), dim3(1024), 0, s, z, e.lists, e.starts, c->dw["cb"], rows, n_seg, e.part, e.sqpart, e.cntpart);
    } else {
        hipLaunchKernelGGL(vq_ema_partials_k, dim3(256, (n_seg + 15) / 16), dim3(1024), 0, s, z, idx, c->dw["cb"], rows, n_seg, e.part, e.sqpart, e.cntpart);
    }
    hipLaunchKernelGGL(vq_ema_reduce_k, dim3(256), dim3(128), 0, s, e.part, e.sqpart, e.cntpart, rows, n_seg, stats);
}

int vqhip_train_vq_stats_device(vqhip_codec* c, const float* d_leaves, int64_t n, float* d_stats, uint8_t* d_idx, float* d_latent, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!c->training) return fail(c, VQHIP_ERR_INVALID, "train_vq_stats: call vqhip_train_begin first");
    if (!d_leaves || !d_stats || n < 1) return fail(c, VQHIP_ERR_INVALID, "train_vq_stats: null pointer or n_leaves < 1");
    if (n > c->chunk) return fail(c, VQHIP_ERR_INVALID, "train_vq_stats: a training batch may not exceed the chunk size (" + std::to_string(c->chunk) + " leaves)");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (!d_latent || !d_idx) {
        if (int rc = ensure(c, c->tr_z, (size_t)n * 64 * 128, "the training latents")) return rc;
        if (int rc = ensure(c, c->tr_idx, (size_t)n * 64, "the training indices")) return rc;
    }
    if (int rc = ensure(c, c->tr_part, ema_scratch_bytes((int)((n * 64 + VQ_SEG_ROWS - 1) / VQ_SEG_ROWS)), "the codebook statistics partials")) return rc;
    float* z = d_latent ? d_latent : c->tr_z;
    uint8_t* idx = d_idx ? d_idx : c->tr_idx;
    int rc = encode_chunk(c, d_leaves, n, idx, s, z);
    if (rc) return rc;
    const int64_t rows = n * 64;
    const int n_seg = (int)((rows + VQ_SEG_ROWS - 1) / VQ_SEG_ROWS);
    Launcher L{c, s, n};
    L.run("train_vq_ema_stats", [&] { launch_vq_ema(c, s, z, idx, rows, n_seg, d_stats); });
    return L.rc;
}

int vqhip_train_eval_device(vqhip_codec* c, const float* d_leaves, int64_t n, float* d_stats, float* d_recon_sums, float* d_recon, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!c->training) return fail(c, VQHIP_ERR_INVALID, "train_eval: call vqhip_train_begin first");
    if (!d_leaves || !d_stats || !d_recon_sums || n < 1) return fail(c, VQHIP_ERR_INVALID, "train_eval: null pointer or n_leaves < 1");
    if (n > c->chunk) return fail(c, VQHIP_ERR_INVALID, "train_eval: a batch may not exceed the chunk size (" + std::to_string(c->chunk) + " leaves)");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // forward in eval mode (VQVAE.forward, VQVAE_v2.py:344-348): assignment + statistics exactly as in training, no update
    int rc = vqhip_train_vq_stats_device(c, d_leaves, n, d_stats, nullptr, nullptr, s);
    if (rc) return rc;
    if ((rc = ensure_tables(c))) return rc;  // the decoder's stem table follows the live codebook
    float* recon = d_recon;
    if (!recon) {
        if ((rc = ensure(c, c->tr_recon, (size_t)n * 512, "the evaluation's reconstruction"))) return rc;
        recon = c->tr_recon;
    }
    if ((rc = ensure(c, c->tr_loss_part, (size_t)RL_BLOCKS * 2, "the loss partials"))) return rc;
    if ((rc = decode_chunk(c, c->tr_idx, n, recon, s))) return rc;
    Launcher L{c, s, n};
    L.run("train_recon_loss", [&] {
        hipLaunchKernelGGL(recon_loss_partials_k, dim3(RL_BLOCKS), dim3(256), 0, s, d_leaves, recon, n * 512, c->tr_loss_part);
        hipLaunchKernelGGL(recon_loss_reduce_k, dim3(1), dim3(1), 0, s, c->tr_loss_part, n * 512, d_recon_sums);
    });
    return L.rc;
}

int vqhip_train_vq_update_device(vqhip_codec* c, const float* d_stats, float decay, float eps, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!c->training) return fail(c, VQHIP_ERR_INVALID, "train_vq_update: call vqhip_train_begin first");
    if (!d_stats || !(decay >= 0.0f && decay <= 1.0f) || !(eps > 0.0f)) return fail(c, VQHIP_ERR_INVALID, "train_vq_update: null stats, decay outside [0,1] or eps <= 0");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const float alpha = (float)(1.0 - (double)decay);
    Launcher L{c, s, 0};
    L.run("train_vq_ema_update", [&] {
        hipLaunchKernelGGL(vq_ema_update_k, dim3(256), dim3(128), 0, s, d_stats, decay, alpha, eps, c->dw["tr.cs"], c->dw["tr.avg"], c->dw["cb"]);
    });
    c->tables_stale = true;
    return L.rc;
}

int vqhip_train_get_state(vqhip_codec* c, float* embedding, float* cluster_size, float* embed_avg)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!c->training && (cluster_size || embed_avg)) return fail(c, VQHIP_ERR_INVALID, "train_get_state: call vqhip_train_begin first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (embedding) HIPCHK(c, hipMemcpy(embedding, c->dw["cb"], 256 * 128 * sizeof(float), hipMemcpyDeviceToHost));
    if (cluster_size) HIPCHK(c, hipMemcpy(cluster_size, c->dw["tr.cs"], 256 * sizeof(float), hipMemcpyDeviceToHost));
    if (embed_avg) HIPCHK(c, hipMemcpy(embed_avg, c->dw["tr.avg"], 256 * 128 * sizeof(float), hipMemcpyDeviceToHost));
    return VQHIP_OK;
}

int vqhip_train_set_state(vqhip_codec* c, const float* embedding, const float* cluster_size, const float* embed_avg)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!c->training && (cluster_size || embed_avg)) return fail(c, VQHIP_ERR_INVALID, "train_set_state: call vqhip_train_begin first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (embedding) {
        HIPCHK(c, hipMemcpy(c->dw["cb"], embedding, 256 * 128 * sizeof(float), hipMemcpyHostToDevice));
        c->tables_stale = true;
    }
    if (cluster_size) HIPCHK(c, hipMemcpy(c->dw["tr.cs"], cluster_size, 256 * sizeof(float), hipMemcpyHostToDevice));
    if (embed_avg) HIPCHK(c, hipMemcpy(c->dw["tr.avg"], embed_avg, 256 * 128 * sizeof(float), hipMemcpyHostToDevice));
    return VQHIP_OK;
}

int vqhip_train_commit(vqhip_codec* c)
{
    if (!c) return VQHIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    return c->tables_stale ? refresh_tables(c) : VQHIP_OK;
}

// ---- in-process multi-GPU front end: one codec + one host thread per device, contiguous leaf ranges ----
// One persistent host thread per device: it owns the device's handle for the lifetime of the front end (hipSetDevice once, pinned
// staging allocated from this thread, i.e. on the memory node of the cores it is bound to), sleeps on a condition variable between
// calls and runs one leaf range per call.  The thread is bound to the cores of its GPU's NUMA node when /sys exposes it; the
// copy threads a call fans out to inherit that mask.
struct MultiWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    bool has_job = false, done = true, quit = false;
    bool is_encode = false;
    const void* in = nullptr;
    void* out = nullptr;
    int64_t n = 0;
    int rc = VQHIP_OK;
    int numa_node = -1, cpus_bound = 0;
};

struct vqhip_multi {
    std::vector<vqhip_codec*> dev;
    std::vector<std::unique_ptr<MultiWorker>> workers;
    std::string err;
};

// cores of the NUMA node the device hangs off (empty if unknown)
static std::vector<int> device_numa_cpus(int device, int* node_out)
{
    std::vector<int> cpus;
    char bus[64] = {0};
    *node_out = -1;
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess) return cpus;
    for (char* p = bus; *p; ++p) *p = (char)std::tolower(*p);
    std::ifstream fn(std::string("/sys/bus/pci/devices/") + bus + "/numa_node");
    int node = -1;
    if (!(fn >> node) || node < 0) return cpus;
    *node_out = node;
    std::ifstream fl("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist");
    std::string list;
    if (!std::getline(fl, list)) return cpus;
    size_t pos = 0;
    while (pos < list.size()) {
        size_t end = list.find(',', pos);
        if (end == std::string::npos) end = list.size();
        const std::string part = list.substr(pos, end - pos);
        const size_t dash = part.find('-');
        try {
            const int lo = std::stoi(part.substr(0, dash)), hi = dash == std::string::npos ? lo : std::stoi(part.substr(dash + 1));
            for (int cpu = lo; cpu <= hi; ++cpu) cpus.push_back(cpu);
        } catch (...) {
            return {};
        }
        pos = end + 1;
    }
    return cpus;
}

static void multi_worker_main(vqhip_multi* m, int g, int copy_cap)
{
    MultiWorker& w = *m->workers[g];
    g_copy_threads_cap = copy_cap;
    hipSetDevice(m->dev[g]->device);
    {   // NUMA-local: restrict this thread (and the copy threads it spawns) to the device's node, within the process's mask
        int node = -1;
        const std::vector<int> cpus = device_numa_cpus(m->dev[g]->device, &node);
        cpu_set_t cur, want;
        CPU_ZERO(&want);
        if (!cpus.empty() && sched_getaffinity(0, sizeof(cur), &cur) == 0) {
            int cnt = 0;
            for (int cpu : cpus)
                if (cpu < CPU_SETSIZE && CPU_ISSET(cpu, &cur)) CPU_SET(cpu, &want), ++cnt;
            if (cnt > 0 && sched_setaffinity(0, sizeof(want), &want) == 0) w.numa_node = node, w.cpus_bound = cnt;
        }
    }
    std::unique_lock<std::mutex> lk(w.mu);
    for (;;) {
        w.cv.wait(lk, [&] { return w.has_job || w.quit; });
        if (w.quit) return;
        w.has_job = false;
        lk.unlock();
        const int rc = w.is_encode ? vqhip_encode(m->dev[g], static_cast<const float*>(w.in), w.n, static_cast<uint8_t*>(w.out))
                                   : vqhip_decode(m->dev[g], static_cast<const uint8_t*>(w.in), w.n, static_cast<float*>(w.out));
        lk.lock();
        w.rc = rc;
        w.done = true;
        w.cv.notify_all();
    }
}

int vqhip_multi_create(const char* pack_path, const void* pack_bytes, size_t pack_size, const int* device_ids, int n_devices, vqhip_multi** out)
{
    if (!out) return fail(nullptr, VQHIP_ERR_INVALID, "vqhip_multi_create: out is NULL");
    *out = nullptr;
    if (!device_ids || n_devices < 1) return fail(nullptr, VQHIP_ERR_INVALID, "vqhip_multi_create: need at least one device id");
    vqhip_multi* m = new vqhip_multi();
    for (int i = 0; i < n_devices; ++i) {
        vqhip_codec* c = nullptr;
        const int rc = vqhip_create(pack_path, pack_bytes, pack_size, device_ids[i], &c);
        if (rc != VQHIP_OK) {
            for (vqhip_codec* d : m->dev) vqhip_destroy(d);
            delete m;
            return rc;  // message already in the thread-local create error
        }
        m->dev.push_back(c);
    }
    // all devices together never run more than min(cores, 64) copy threads: 8 GPUs x 16 threads each would oversubscribe the
    // memory controllers long before they help a 57 GB/s PCIe link
    const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
    const int cap = std::max(2, std::min(16, std::min(hw, 64) / n_devices));
    for (int g = 0; g < n_devices; ++g) m->workers.emplace_back(new MultiWorker());
    for (int g = 0; g < n_devices; ++g) m->workers[g]->th = std::thread(multi_worker_main, m, g, cap);
    *out = m;
    return VQHIP_OK;
}

void vqhip_multi_destroy(vqhip_multi* m)
{
    if (!m) return;
    for (auto& w : m->workers) {
        {
            std::lock_guard<std::mutex> lk(w->mu);
            w->quit = true;
        }
        w->cv.notify_all();
        if (w->th.joinable()) w->th.join();
    }
    for (vqhip_codec* d : m->dev) vqhip_destroy(d);
    delete m;
}

const char* vqhip_multi_last_error(const vqhip_multi* m) { return m ? m->err.c_str() : g_create_error.c_str(); }

int vqhip_multi_worker_info(const vqhip_multi* m, int index, int* device_id, int* numa_node, int* cpus_bound)
{
    if (!m || index < 0 || index >= (int)m->workers.size()) return VQHIP_ERR_INVALID;
    if (device_id) *device_id = m->dev[index]->device;
    if (numa_node) *numa_node = m->workers[index]->numa_node;
    if (cpus_bound) *cpus_bound = m->workers[index]->cpus_bound;
    return VQHIP_OK;
}

// rank g of G takes leaves [g*ceil(n/G), min(n,(g+1)*ceil(n/G))); results land at the same
// offsets of the caller's buffer, so leaf order is preserved and there is no collective.
static int multi_run(vqhip_multi* m, bool is_encode, const void* in, void* out, int64_t n)
{
    if (!m) return VQHIP_ERR_INVALID;
    if (!in || !out || n < 1) {
        m->err = "multi: null pointer or n_leaves < 1";
        return VQHIP_ERR_INVALID;
    }
    const int G = (int)m->dev.size();
    const int64_t per = (n + G - 1) / G;
    std::vector<char> posted(G, 0);
    for (int g = 0; g < G; ++g) {
        const int64_t lo = std::min(n, g * per), hi = std::min(n, lo + per);
        if (hi == lo) continue;
        MultiWorker& w = *m->workers[g];
        {
            std::lock_guard<std::mutex> lk(w.mu);
            w.is_encode = is_encode;
            w.in = is_encode ? static_cast<const void*>(static_cast<const float*>(in) + lo * 512) : static_cast<const void*>(static_cast<const uint8_t*>(in) + lo * 64);
            w.out = is_encode ? static_cast<void*>(static_cast<uint8_t*>(out) + lo * 64) : static_cast<void*>(static_cast<float*>(out) + lo * 512);
            w.n = hi - lo;
            w.done = false;
            w.has_job = true;
        }
        w.cv.notify_all();
        posted[g] = 1;
    }
    int first_bad = -1, rc_bad = VQHIP_OK;
    for (int g = 0; g < G; ++g) {
        if (!posted[g]) continue;
        MultiWorker& w = *m->workers[g];
        std::unique_lock<std::mutex> lk(w.mu);
        w.cv.wait(lk, [&] { return w.done; });
        if (w.rc != VQHIP_OK && first_bad < 0) first_bad = g, rc_bad = w.rc;
    }
    if (first_bad >= 0) {
        m->err = "device " + std::to_string(m->dev[first_bad]->device) + ": " + m->dev[first_bad]->err;
        return rc_bad;
    }
    return VQHIP_OK;
}

int vqhip_multi_encode(vqhip_multi* m, const float* leaves, int64_t n, uint8_t* indices) { return multi_run(m, true, leaves, indices, n); }
int vqhip_multi_decode(vqhip_multi* m, const uint8_t* indices, int64_t n, float* leaves) { return multi_run(m, false, indices, leaves, n); }

// include/vqvdb_hip_precision.h
int vqhip_set_decode_mode(vqhip_codec* c, int mode)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (mode != VQHIP_PRECISION_FP32 && mode != VQHIP_PRECISION_BF16)
        return fail(c, VQHIP_ERR_INVALID, "set_decode_mode: mode " + std::to_string(mode) + " is neither VQHIP_PRECISION_FP32 (0) nor VQHIP_PRECISION_BF16 (1)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (mode == VQHIP_PRECISION_BF16)
        if (int rc = ensure_dec_bf16_frags(c, c->stream)) return rc;   // (a failed allocation: VQHIP_ERR_NOMEM, the mode as it was)
    c->decode_precision = mode;
    return VQHIP_OK;
}

int vqhip_get_decode_mode(const vqhip_codec* c, int* mode)
{
    if (!c || !mode) return VQHIP_ERR_INVALID;
    *mode = c->decode_precision;
    return VQHIP_OK;
}

// include/vqvdb_hip_encode_mode.h
int vqhip_set_encode_mode(vqhip_codec* c, int mode)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (mode != VQHIP_PRECISION_FP32 && mode != VQHIP_PRECISION_BF16)
        return fail(c, VQHIP_ERR_INVALID, "set_encode_mode: mode " + std::to_string(mode) + " is neither VQHIP_PRECISION_FP32 (0) nor VQHIP_PRECISION_BF16 (1)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (mode == VQHIP_PRECISION_BF16)
        if (int rc = ensure_enc_bf16_frags(c, c->stream)) return rc;   // (a failed allocation: VQHIP_ERR_NOMEM, the mode as it was)
    c->encode_precision = mode;
    return VQHIP_OK;
}

int vqhip_get_encode_mode(const vqhip_codec* c, int* mode)
{
    if (!c || !mode) return VQHIP_ERR_INVALID;
    *mode = c->encode_precision;
    return VQHIP_OK;
}

int vqhip_debug_enable(vqhip_codec* c, int enable)
{
    if (!c) return VQHIP_ERR_INVALID;
    c->debug = enable != 0;
    return VQHIP_OK;
}

int vqhip_profile_enable(vqhip_codec* c, int enable)
{
    if (!c) return VQHIP_ERR_INVALID;
    c->profiling = enable != 0;
    return VQHIP_OK;
}

int vqhip_profile_read(vqhip_codec* c, vqhip_kernel_stat* stats, int cap, int* count)
{
    if (!c || !count) return VQHIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<std::string> order;
    std::map<std::string, vqhip_kernel_stat> agg;
    for (auto& t : c->timers) {
        HIPCHK(c, hipEventSynchronize(t.stop));
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, t.start, t.stop));
        auto it = agg.find(t.name);
        if (it == agg.end()) {
            vqhip_kernel_stat s{};
            std::snprintf(s.name, sizeof(s.name), "%s", t.name.c_str());
            auto ki = kernel_info().find(t.name);
            if (ki != kernel_info().end()) s.flops_per_leaf = ki->second.flops, s.eff_flops_per_leaf = ki->second.eff_flops;
            it = agg.emplace(t.name, s).first;
            order.push_back(t.name);
        }
        it->second.launches += 1;
        it->second.total_ms += ms;
        it->second.leaves += t.leaves;
        hipEventDestroy(t.start);
        hipEventDestroy(t.stop);
    }
    c->timers.clear();
    *count = (int)order.size();
    for (int i = 0; i < (int)order.size() && i < cap && stats; ++i) stats[i] = agg[order[i]];
    return VQHIP_OK;
}

int vqhip_debug_fetch(vqhip_codec* c, const char* name, int64_t n, float* out)
{
    if (!c || !name || !out || n < 1) return VQHIP_ERR_INVALID;
    auto it = c->act.find(name);
    if (it == c->act.end()) return fail(c, VQHIP_ERR_INVALID, std::string("debug_fetch: unknown activation '") + name + "'");
    const int C = c->act_shape[name].first, NP = c->act_shape[name].second;
    if (std::strcmp(name, "xr") == 0) return fail(c, VQHIP_ERR_INVALID, "debug_fetch: 'xr' is the first conv's row layout [tile][64 rows][32 leaves][12], not a [tile][pos][32] activation; fetch 'xt'");
    if ((C != 1 && C < 4) || n > std::max(c->ws_tiles, c->ft_tiles) * 32) return fail(c, VQHIP_ERR_INVALID, "debug_fetch: not a tile activation or n too large");
    for (const ActSpec& a : kActs)   // compact (inference) layout: large activations share three regions and overwrite each other
        if (!c->ws_full && a.region != -1 && std::strcmp(a.name, name) == 0)
            return fail(c, VQHIP_ERR_INVALID, std::string("debug_fetch: '") + name + "' is not kept in the compact inference workspace; call vqhip_debug_enable(1) before the pass");
    if (!it->second) return fail(c, VQHIP_ERR_INVALID, std::string("debug_fetch: '") + name + "' is not allocated");
    if (C == 1) {  // [tile][NP][32]
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipDeviceSynchronize());
        const int64_t tl = (n + 31) / 32;
        std::vector<float> raw1((size_t)tl * 32 * NP);
        HIPCHK(c, hipMemcpy(raw1.data(), it->second, raw1.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int64_t l = 0; l < n; ++l)
            for (int p = 0; p < NP; ++p) out[(size_t)l * NP + p] = raw1[((size_t)(l / 32) * NP + p) * 32 + (l % 32)];
        return VQHIP_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    const int64_t tiles = (n + 31) / 32;
    std::vector<float> raw((size_t)tiles * 32 * C * NP);
    HIPCHK(c, hipMemcpy(raw.data(), it->second, raw.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int64_t l = 0; l < n; ++l)
        for (int ch = 0; ch < C; ++ch)
            for (int p = 0; p < NP; ++p)
                out[((size_t)l * C + ch) * NP + p] = raw[((((size_t)(l / 32) * NP + p) * (C / 4) + ch / 4) * 32 + (l % 32)) * 4 + ch % 4];
    return VQHIP_OK;
}

int vqhip_selftest_mfma(vqhip_codec* c, int64_t* mismatches)
{
    if (!c || !mismatches) return VQHIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const int ks = 24;
    std::vector<float> h((size_t)(32 * 2 * ks) * 2 + (size_t)(16 * 4 * ks) * 2);
    uint32_t x = 12345u;
    for (auto& v : h) {
        x = x * 1664525u + 1013904223u;
        v = ((int)(x >> 8) - (1 << 23)) * (1.0f / (1 << 22)) * (1.0f + (float)(x & 7));
    }
    float* d = nullptr;
    unsigned long long* dm = nullptr;
    HIPCHK(c, hipMalloc(&d, h.size() * sizeof(float)));
    HIPCHK(c, hipMalloc(&dm, 2 * sizeof(unsigned long long)));
    HIPCHK(c, hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(dm, 0, 2 * sizeof(unsigned long long)));
    const float* a32 = d;
    const float* b32 = a32 + 32 * 2 * ks;
    const float* a16 = b32 + 32 * 2 * ks;
    const float* b16 = a16 + 16 * 4 * ks;
    hipLaunchKernelGGL(mfma_probe_k, dim3(1), dim3(64), 0, c->stream, a32, b32, a16, b16, ks, dm);
    HIPCHK(c, hipGetLastError());
    unsigned long long hm[2] = {0, 0};
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(hm, dm, sizeof(hm), hipMemcpyDeviceToHost));
    hipFree(d);
    hipFree(dm);
    mismatches[0] = (int64_t)hm[0];
    mismatches[1] = (int64_t)hm[1];
    return VQHIP_OK;
}

}  // extern "C"

#include "vq_train_full.inc"
#include "vq_vec3.inc"
#include "vq_vec3_bf16.inc"
#include "vq_vec3_bounded.inc"
#include "vq_bounded.inc"
#include "vq_residual.inc"
#include "vq_vec3_residual.inc"
#include "vq_file.inc"
#include "vq_rate.inc"
#include "vq_vec3_rate.inc"
#include "vq_vec3_mask.inc"
#include "vq_vec3_active.inc"
#include "vq_vec3_file.inc"
#include "vq_vec3_budget.inc"
#include "vq_vec3_train.inc"
#include "vq_vec3_fulltrain.inc"
