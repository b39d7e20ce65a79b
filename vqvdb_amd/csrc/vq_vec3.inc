// vq_vec3.inc — the Vec3 model handle (vqhip_vec3_*; include/vqvdb_hip.h, DESIGN.md §11).  Part of vq_runtime.hip's
// translation unit: it reuses the weight-pack parser (parse_pack / need) and nothing else of the scalar handle.

#include "vq_vec3.h"
#include "vq_vec3_train.h"

struct vqhip_vec3_codec {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int k_codes = 0, k_pad = 0;
    std::map<std::string, float*> w;   // device weights / fragments
    int64_t chunk = 16384;
    bool chunk_fitted = false;
    DevBuf<float> ws;                  // V3_LEAF_FLOATS per leaf; v3_ws lays it out for the leaves it holds
    DevBuf<float> io_leaves;           // host entry points: [chunk][512][3]
    DevBuf<uint16_t> io_idx;           // [chunk][64]
    bool debug = false;
    // bf16-operand inference mode (vq_vec3_bf16.inc): VQHIP_VEC3_PRECISION_*; the bf16 fragment tables exist once bf_ready
    int precision = 0;
    bool bf_ready = false;
    // codebook training (vq_vec3_train.inc): set by vqhip_vec3_train_begin
    bool training = false;
    DevBuf<float> tr_cs;               // cluster_size [K]
    DevBuf<float> tr_avg;              // embed_avg [K][64]
    DevBuf<unsigned char> tr_ws;       // training workspace, laid out for tr_leaves leaves (v3t_layout)
    int64_t tr_leaves = 0;
    // full training (vq_vec3_fulltrain.inc): set by vqhip_vec3_fulltrain_begin; P, M, V live in w ("ft.P", "ft.M", "ft.V")
    bool ft_on = false;
    float *ft_P = nullptr, *ft_M = nullptr, *ft_V = nullptr;
    DevBuf<float> ft_ws;               // activations, gradients and partials, laid out for ft_leaves leaves (v3f_layout)
    int64_t ft_leaves = 0;
    // error-bounded round trip (vq_vec3_bounded.inc)
    DevBuf<int64_t> bd_scan;           // selection: per-block counts / offsets
    DevBuf<float> bd_err;              // host entry point: leaf errors [m][2]
    DevBuf<int64_t> bd_ids;            // host entry point: outlier ids [m], then their count
    // quantised residuals (vq_vec3_residual.inc), host pair: one chunk's reconstruction, leaf errors, codes, offsets, payload
    DevBuf<float> rs_recon;            // [m][512][3]
    DevBuf<float> rs_err;              // [m][2]
    DevBuf<uint16_t> rs_code;          // [m]
    DevBuf<int64_t> rs_off;            // [m + 1]
    DevBuf<uint8_t> rs_payload;        // m * 6144 bytes
    // size sweep (vq_vec3_rate.inc), host calls: the histogram [64][51]
    DevBuf<int64_t> rate_hist;
    // active-voxel masks (vq_vec3_mask.inc), host calls: one chunk's masks [m][8]
    DevBuf<uint64_t> mk_mask;
    // compact records (vq_vec3_active.inc), host sweep: the payload bytes of every rung [64]
    DevBuf<int64_t> ac_bytes;
    // leaf-pointer and file calls (vq_vec3_file.inc): pinned staging of one batch's leaves [m][512][3]
    PinBuf<float> fl_stage;
    struct Dbg {
        DevBuf<float> p;
        int64_t n = 0;
        int floats = 0;                // per leaf
    };
    std::map<std::string, Dbg> dbg;
};

namespace {

thread_local std::string g_v3_create_error = "";

int v3_fail(vqhip_vec3_codec* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    else g_v3_create_error = msg;
    return code;
}

// per-leaf workspace, floats: R8 (two 64-channel 8^3 tensors; the decoder's up_conv output), P and Q (128-channel 4^3),
// Z (64-channel latent / gathered codes), gate (128), GroupNorm statistics (8 x {mean, rstd})
constexpr int64_t V3_R8 = 2 * 64 * 512, V3_P = 128 * 64, V3_Z = 64 * 64, V3_GATE = 128, V3_STATS = 16;
constexpr int64_t V3_LEAF_FLOATS = V3_R8 + 2 * V3_P + V3_Z + V3_GATE + V3_STATS;
constexpr int64_t V3_IO_BYTES = 1536 * 4 + 64 * 2;
// largest chunk: 131 072 leaves are 45 GB of workspace.  The elementwise kernels (gn_relu_k, gather_k) loop over their
// elements with a grid of at most V3_EW_BLOCKS workgroups, so no launch comes near the 2^32 work-item limit.
constexpr int64_t V3_MAX_CHUNK = 131072;
constexpr int64_t V3_EW_BLOCKS = 1 << 16;
unsigned v3_ew_grid(int64_t elements) { return (unsigned)std::min(V3_EW_BLOCKS, (elements + 255) / 256); }

struct V3Ws {
    float *a8, *b8, *u, *p, *q, *z, *gate, *stats;
};
V3Ws v3_ws(const vqhip_vec3_codec* c)
{
    const int64_t L = (int64_t)c->ws.capacity() / V3_LEAF_FLOATS;
    V3Ws r;
    r.a8 = c->ws;
    r.b8 = r.a8 + L * 64 * 512;
    r.u = r.a8;   // decoder: [256][64] per leaf inside R8
    r.p = c->ws + L * V3_R8;
    r.q = r.p + L * V3_P;
    r.z = r.q + L * V3_P;
    r.gate = r.z + L * V3_Z;
    r.stats = r.gate + L * V3_GATE;
    return r;
}

// [ctile][tap][cin/2][lane] = W[32 ctile + (lane&31)][2 cp + (lane>>5)][tap]; input channels >= cin_real are zero
std::vector<float> v3_frag(const float* W, int cout, int cin_real, int cin_pad, int kt)
{
    const int cp_n = cin_pad / 2;
    std::vector<float> f((size_t)cout * cin_pad * kt);
    for (int ct = 0; ct < cout / 32; ++ct)
        for (int t = 0; t < kt; ++t)
            for (int cp = 0; cp < cp_n; ++cp)
                for (int l = 0; l < 64; ++l) {
                    const int co = 32 * ct + (l & 31), ci = 2 * cp + (l >> 5);
                    f[(((size_t)ct * kt + t) * cp_n + cp) * 64 + l] = ci < cin_real ? W[((size_t)co * cin_real + ci) * kt + t] : 0.0f;
                }
    return f;
}

int v3_upload(vqhip_vec3_codec* c, const std::string& name, const float* p, size_t count)
{
    float* d = nullptr;
    HIPCHK(c, hipMalloc(&d, count * sizeof(float)));
    c->w[name] = d;
    HIPCHK(c, hipMemcpy(d, p, count * sizeof(float), hipMemcpyHostToDevice));
    return VQHIP_OK;
}

struct V3Spec {
    std::string name;
    std::vector<uint32_t> dims;
};

// every inference tensor of VQVAE(3, 64, K).state_dict() (python/VQVAE_v2.py EncoderVec3 / DecoderVec3), K checked apart
std::vector<V3Spec> v3_specs()
{
    std::vector<V3Spec> s;
    auto conv = [&](const std::string& p, uint32_t co, uint32_t ci, uint32_t k) {
        s.push_back({p + ".weight", {co, ci, k, k, k}});
        s.push_back({p + ".bias", {co}});
    };
    auto gn = [&](const std::string& p, uint32_t ch) {
        s.push_back({p + ".weight", {ch}});
        s.push_back({p + ".bias", {ch}});
    };
    auto rb = [&](const std::string& p, uint32_t ch) {
        gn(p + ".gn1", ch);
        conv(p + ".conv1", ch, ch, 3);
        gn(p + ".gn2", ch);
        conv(p + ".conv2", ch, ch, 3);
    };
    conv("encoder.pre.0", 64, 3, 3);
    gn("encoder.pre.1", 64);
    rb("encoder.pre.3", 64);
    conv("encoder.down1", 128, 64, 3);
    rb("encoder.res_stack.0", 128);
    rb("encoder.res_stack.1", 128);
    s.push_back({"encoder.attn.fc.0.weight", {32, 128}});
    s.push_back({"encoder.attn.fc.2.weight", {128, 32}});
    conv("encoder.proj", 64, 128, 1);
    conv("decoder.stem.0", 128, 64, 3);
    gn("decoder.stem.1", 128);
    rb("decoder.res_stack.0", 128);
    rb("decoder.res_stack.1", 128);
    s.push_back({"decoder.attn.fc.0.weight", {32, 128}});
    s.push_back({"decoder.attn.fc.2.weight", {128, 32}});
    conv("decoder.up_conv", 256, 128, 3);
    conv("decoder.final", 3, 32, 3);
    return s;
}

// names and shapes of every tensor (host only: runs before any device is touched); K = rows of quantizer.embedding
bool v3_validate(const std::map<std::string, PackTensor>& pk, std::string& err)
{
    if (pk.count("encoder.down.weight") || (pk.count("encoder.pre.0.weight") && pk.at("encoder.pre.0.weight").dims.size() == 5 &&
                                            pk.at("encoder.pre.0.weight").dims[1] == 1)) {
        err = "weight pack: not a Vec3 model pack (this is the scalar VQVAE(1, ...) model; load it with vqhip_create)";
        return false;
    }
    auto e = pk.find("quantizer.embedding");
    if (e == pk.end()) err = "weight pack: missing tensor 'quantizer.embedding'";
    else if (e->second.dims.size() != 2) err = "weight pack: tensor 'quantizer.embedding' has unexpected shape (expected [K][64])";
    else if (e->second.dims[1] != 64) err = "weight pack: embedding_dim is " + std::to_string(e->second.dims[1]) + ", the Vec3 model needs 64";
    else if (e->second.dims[0] < 1 || e->second.dims[0] > 65536)
        err = "weight pack: num_codes is " + std::to_string(e->second.dims[0]) + ", must be in [1, 65536] (16-bit indices)";
    if (!err.empty()) return false;
    for (const V3Spec& sp : v3_specs()) {
        auto it = pk.find(sp.name);
        if (it == pk.end()) err = "weight pack: missing tensor '" + sp.name + "'";
        else if (it->second.dims != sp.dims) err = "weight pack: tensor '" + sp.name + "' has unexpected shape";
        if (!err.empty()) return false;
    }
    return true;
}

int v3_load(vqhip_vec3_codec* c, const std::map<std::string, PackTensor>& pk)
{
    auto e = pk.find("quantizer.embedding");
    std::map<std::string, const float*> t;
    for (const V3Spec& sp : v3_specs()) t[sp.name] = pk.at(sp.name).data;

    int rc = VQHIP_OK;
    auto frag = [&](const std::string& dev, const std::string& p, int cout, int cin, int cin_pad, int kt) {
        if (rc) return;
        const std::vector<float> f = v3_frag(t[p + ".weight"], cout, cin, cin_pad, kt);
        rc = v3_upload(c, dev + ".wf", f.data(), f.size());
        if (!rc) rc = v3_upload(c, dev + ".b", t[p + ".bias"], cout);
    };
    auto raw = [&](const std::string& dev, const std::string& p, size_t n) {
        if (!rc) rc = v3_upload(c, dev, t[p], n);
    };
    auto rb = [&](const std::string& dev, const std::string& p, int ch) {
        raw(dev + ".g1", p + ".gn1.weight", ch);
        raw(dev + ".b1", p + ".gn1.bias", ch);
        frag(dev + ".c1", p + ".conv1", ch, ch, ch, 27);
        raw(dev + ".g2", p + ".gn2.weight", ch);
        raw(dev + ".b2", p + ".gn2.bias", ch);
        frag(dev + ".c2", p + ".conv2", ch, ch, ch, 27);
    };
    frag("e.pre", "encoder.pre.0", 64, 3, 4, 27);
    raw("e.pre.g", "encoder.pre.1.weight", 64);
    raw("e.pre.bt", "encoder.pre.1.bias", 64);
    rb("e.rb64", "encoder.pre.3", 64);
    frag("e.down", "encoder.down1", 128, 64, 64, 27);
    rb("e.rb0", "encoder.res_stack.0", 128);
    rb("e.rb1", "encoder.res_stack.1", 128);
    raw("e.fc1", "encoder.attn.fc.0.weight", 32 * 128);
    raw("e.fc2", "encoder.attn.fc.2.weight", 128 * 32);
    frag("e.proj", "encoder.proj", 64, 128, 128, 1);
    frag("d.stem", "decoder.stem.0", 128, 64, 64, 27);
    raw("d.stem.g", "decoder.stem.1.weight", 128);
    raw("d.stem.bt", "decoder.stem.1.bias", 128);
    rb("d.rb0", "decoder.res_stack.0", 128);
    rb("d.rb1", "decoder.res_stack.1", 128);
    raw("d.fc1", "decoder.attn.fc.0.weight", 32 * 128);
    raw("d.fc2", "decoder.attn.fc.2.weight", 128 * 32);
    frag("d.up", "decoder.up_conv", 256, 128, 128, 27);
    raw("d.final.w", "decoder.final.weight", 3 * 32 * 27);
    raw("d.final.b", "decoder.final.bias", 3);
    if (rc) return rc;

    // codebook: raw rows (decoder gather), MFMA fragments padded to 128-code blocks, |e|^2 (fp32, dimension order; padding +inf)
    const float* E = e->second.data;
    c->k_codes = (int)e->second.dims[0];
    c->k_pad = (c->k_codes + v3::VQ_BLOCK_CODES - 1) / v3::VQ_BLOCK_CODES * v3::VQ_BLOCK_CODES;
    std::vector<float> ef((size_t)c->k_pad * 64, 0.0f), ee(c->k_pad, INFINITY);
    for (int code = 0; code < c->k_codes; ++code) {
        float s = 0.0f;
        for (int d = 0; d < 64; ++d) {
            const float v = E[(size_t)code * 64 + d];
            s = s + v * v;
            ef[(((size_t)(code / 32) * 32 + d / 2) * 64) + (d & 1) * 32 + (code & 31)] = v;
        }
        ee[code] = s;
    }
    if ((rc = v3_upload(c, "cb", E, (size_t)c->k_codes * 64))) return rc;
    if ((rc = v3_upload(c, "cb.f", ef.data(), ef.size()))) return rc;
    return v3_upload(c, "cb.ee", ee.data(), ee.size());
}

template <typename K>
int v3_set_lds(vqhip_vec3_codec* c, K kernel, size_t bytes)
{
    if (bytes > 64 * 1024) HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return VQHIP_OK;
}

// ---- kernel instantiations --------------------------------------------------------------------------------------------
//                                  CIN COUT SI SO KS ST PD LPB MT NT INMODE        OUTMODE
constexpr auto v3_pre = v3::conv_k<4, 64, 8, 8, 3, 1, 1, 1, 2, 2, v3::IN_LEAF3, v3::OUT_BIAS>;        // 3->64 (channel 3 zero)
constexpr auto v3_r64a = v3::conv_k<64, 64, 8, 8, 3, 1, 1, 1, 2, 2, v3::IN_GNRELU, v3::OUT_BIAS>;     // ResBlock(64) conv1
constexpr auto v3_r64b = v3::conv_k<64, 64, 8, 8, 3, 1, 1, 1, 2, 2, v3::IN_GNRELU, v3::OUT_RESID>;    // ResBlock(64) conv2
constexpr auto v3_down = v3::conv_k<64, 128, 8, 4, 3, 2, 1, 1, 1, 1, v3::IN_PLAIN, v3::OUT_BIAS>;     // k3 s2 p1
constexpr auto v3_r128a = v3::conv_k<128, 128, 4, 4, 3, 1, 1, 2, 1, 2, v3::IN_GNRELU, v3::OUT_BIAS>;
constexpr auto v3_r128b = v3::conv_k<128, 128, 4, 4, 3, 1, 1, 2, 1, 2, v3::IN_GNRELU, v3::OUT_RESID>;
constexpr auto v3_proj = v3::conv_k<128, 64, 4, 4, 1, 1, 0, 2, 1, 1, v3::IN_GATE, v3::OUT_BIAS>;
constexpr auto v3_stem = v3::conv_k<64, 128, 4, 4, 3, 1, 1, 2, 1, 2, v3::IN_PLAIN, v3::OUT_BIAS>;
constexpr auto v3_up = v3::conv_k<128, 256, 4, 4, 3, 1, 1, 2, 2, 2, v3::IN_GATE, v3::OUT_BIAS>;

template <int CIN, int COUT, int SI, int SO, int LPB, int MT, int NT>
struct V3Launch {
    static constexpr int threads = LPB * v3::ConvShape<CIN, COUT, SO, MT, NT>::WPL * 64;
    static constexpr size_t lds = (size_t)LPB * CIN * SI * SI * SI * sizeof(float);
};
using L_pre = V3Launch<4, 64, 8, 8, 1, 2, 2>;
using L_r64 = V3Launch<64, 64, 8, 8, 1, 2, 2>;
using L_down = V3Launch<64, 128, 8, 4, 1, 1, 1>;
using L_r128 = V3Launch<128, 128, 4, 4, 2, 1, 2>;
using L_proj = V3Launch<128, 64, 4, 4, 2, 1, 1>;
using L_stem = V3Launch<64, 128, 4, 4, 2, 1, 2>;
using L_up = V3Launch<128, 256, 4, 4, 2, 2, 2>;
constexpr size_t V3_LDS_FINAL = 32 * 512 * sizeof(float);

int v3_init_attrs(vqhip_vec3_codec* c)
{
    int rc = v3_set_lds(c, v3_pre, L_pre::lds);
    if (!rc) rc = v3_set_lds(c, v3_r64a, L_r64::lds);
    if (!rc) rc = v3_set_lds(c, v3_r64b, L_r64::lds);
    if (!rc) rc = v3_set_lds(c, v3_down, L_down::lds);
    if (!rc) rc = v3_set_lds(c, v3_r128a, L_r128::lds);
    if (!rc) rc = v3_set_lds(c, v3_r128b, L_r128::lds);
    if (!rc) rc = v3_set_lds(c, v3_proj, L_proj::lds);
    if (!rc) rc = v3_set_lds(c, v3_stem, L_stem::lds);
    if (!rc) rc = v3_set_lds(c, v3_up, L_up::lds);
    if (!rc) rc = v3_set_lds(c, v3::final_k, V3_LDS_FINAL);
    return rc;
}

int v3_ensure_ws(vqhip_vec3_codec* c, int64_t m)
{
    const int rc = ensure(c, c->ws, (size_t)m * V3_LEAF_FLOATS, [&](hipError_t) { return "vec3: cannot allocate the workspace of " + std::to_string(m) + " leaves"; });
    if (rc) c->chunk_fitted = false;   // re-fit the chunk to the free memory at the next call
    return rc;
}

size_t v3t_ws_bytes(int64_t leaves, int k_codes);   // vq_vec3_train.inc: training workspace of a chunk (0 for 0 leaves)
size_t v3f_ws_bytes(int64_t leaves);                // vq_vec3_fulltrain.inc: full-training workspace of a chunk (0 for 0 leaves)

// halve the chunk until workspace + I/O slots (+ the training workspaces once training has begun) fit into 80 % of the free device memory (never below 1024 leaves)
void v3_fit_chunk(vqhip_vec3_codec* c)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;
    free_b += c->ws.bytes() + c->io_leaves.bytes() + c->io_idx.bytes() + c->tr_ws.bytes() + c->ft_ws.bytes();   // what this handle holds can be re-used
    auto need = [&](int64_t m) {
        return (size_t)m * (V3_LEAF_FLOATS * sizeof(float) + V3_IO_BYTES) + (c->training ? v3t_ws_bytes(m, c->k_codes) : 0) +
               (c->ft_on ? v3f_ws_bytes(m) : 0);
    };
    while (c->chunk > 1024 && need(c->chunk) > free_b / 5 * 4)
        c->chunk = (c->chunk / 2 + 31) / 32 * 32;
    c->chunk_fitted = true;
}

// debug mode: copy a chunk's activation [m][floats] to the named buffer
int v3_keep(vqhip_vec3_codec* c, const char* name, const float* src, int floats, int64_t m, hipStream_t s)
{
    if (!c->debug) return VQHIP_OK;
    auto& d = c->dbg[name];
    if (int rc = ensure(c, d.p, (size_t)m * floats, "a debug activation")) return rc;
    d.floats = floats;
    d.n = m;
    HIPCHK(c, hipMemcpyAsync(d.p, src, (size_t)m * floats * sizeof(float), hipMemcpyDeviceToDevice, s));
    return VQHIP_OK;
}

int v3_launch_check(vqhip_vec3_codec* c, const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return v3_fail(c, VQHIP_ERR_DEVICE, std::string("launch ") + what + ": " + hipGetErrorString(e));
    return VQHIP_OK;
}

template <typename K, typename L>
void v3_conv(K kernel, L, hipStream_t s, int64_t m, v3::ConvArgs a, int lpb)
{
    a.n = m;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((m + lpb - 1) / lpb)), dim3(L::threads), L::lds, s, a);
}

v3::ConvArgs v3_args(const float* in, const float* wf, const float* bias, float* out)
{
    v3::ConvArgs a{};
    a.in = in, a.wf = wf, a.bias = bias, a.out = out, a.res = out;
    return a;
}

// ResidualBlock(128) in place on x (y = x + 0.1 conv2(relu(gn2(conv1(relu(gn1(x))))))), h = scratch
int v3_rb128(vqhip_vec3_codec* c, const std::string& p, float* x, float* h, float* stats, int64_t m, hipStream_t s)
{
    const unsigned nb = (unsigned)m;
    hipLaunchKernelGGL((v3::gn_stats_k<128, 64>), dim3(nb), dim3(256), 0, s, x, stats, m);
    v3::ConvArgs a = v3_args(x, c->w[p + ".c1.wf"], c->w[p + ".c1.b"], h);
    a.stats = stats, a.gamma = c->w[p + ".g1"], a.beta = c->w[p + ".b1"];
    v3_conv(v3_r128a, L_r128{}, s, m, a, 2);
    hipLaunchKernelGGL((v3::gn_stats_k<128, 64>), dim3(nb), dim3(256), 0, s, h, stats, m);
    a = v3_args(h, c->w[p + ".c2.wf"], c->w[p + ".c2.b"], x);
    a.stats = stats, a.gamma = c->w[p + ".g2"], a.beta = c->w[p + ".b2"], a.res = x;
    v3_conv(v3_r128b, L_r128{}, s, m, a, 2);
    return v3_launch_check(c, p.c_str());
}

int v3_encode_chunk(vqhip_vec3_codec* c, const float* leaves, int64_t m, uint16_t* idx, hipStream_t s)
{
    if (int rc = v3_ensure_ws(c, m)) return rc;
    const V3Ws W = v3_ws(c);
    auto& w = c->w;
    const unsigned nb = (unsigned)m;
    int rc = VQHIP_OK;
    // encoder.pre: conv 3->64, GroupNorm(8,64) + ReLU (materialised: the residual of the block), ResidualBlock(64)
    v3_conv(v3_pre, L_pre{}, s, m, v3_args(leaves, w["e.pre.wf"], w["e.pre.b"], W.a8), 1);
    if ((rc = v3_launch_check(c, "vec3 encoder.pre.0")) || (rc = v3_keep(c, "encoder.pre.0", W.a8, 64 * 512, m, s))) return rc;
    hipLaunchKernelGGL((v3::gn_stats_k<64, 512>), dim3(nb), dim3(256), 0, s, W.a8, W.stats, m);
    hipLaunchKernelGGL((v3::gn_relu_k<64, 512>), dim3(v3_ew_grid(m * 64 * 512)), dim3(256), 0, s, W.a8, W.stats, w["e.pre.g"],
                       w["e.pre.bt"], m);
    if ((rc = v3_launch_check(c, "vec3 encoder.pre.1")) || (rc = v3_keep(c, "encoder.pre.2", W.a8, 64 * 512, m, s))) return rc;
    hipLaunchKernelGGL((v3::gn_stats_k<64, 512>), dim3(nb), dim3(256), 0, s, W.a8, W.stats, m);
    v3::ConvArgs a = v3_args(W.a8, w["e.rb64.c1.wf"], w["e.rb64.c1.b"], W.b8);
    a.stats = W.stats, a.gamma = w["e.rb64.g1"], a.beta = w["e.rb64.b1"];
    v3_conv(v3_r64a, L_r64{}, s, m, a, 1);
    hipLaunchKernelGGL((v3::gn_stats_k<64, 512>), dim3(nb), dim3(256), 0, s, W.b8, W.stats, m);
    a = v3_args(W.b8, w["e.rb64.c2.wf"], w["e.rb64.c2.b"], W.a8);
    a.stats = W.stats, a.gamma = w["e.rb64.g2"], a.beta = w["e.rb64.b2"], a.res = W.a8;
    v3_conv(v3_r64b, L_r64{}, s, m, a, 1);
    if ((rc = v3_launch_check(c, "vec3 encoder.pre.3")) || (rc = v3_keep(c, "encoder.pre", W.a8, 64 * 512, m, s))) return rc;
    // down1 -> 128 x 4^3, two ResidualBlock(128), ChannelAttention gates, proj 128->64 on the gated input
    v3_conv(v3_down, L_down{}, s, m, v3_args(W.a8, w["e.down.wf"], w["e.down.b"], W.p), 1);
    if ((rc = v3_launch_check(c, "vec3 encoder.down1")) || (rc = v3_keep(c, "encoder.down1", W.p, 128 * 64, m, s))) return rc;
    if ((rc = v3_rb128(c, "e.rb0", W.p, W.q, W.stats, m, s)) || (rc = v3_keep(c, "encoder.res_stack.0", W.p, 128 * 64, m, s))) return rc;
    if ((rc = v3_rb128(c, "e.rb1", W.p, W.q, W.stats, m, s)) || (rc = v3_keep(c, "encoder.res_stack.1", W.p, 128 * 64, m, s))) return rc;
    hipLaunchKernelGGL(v3::se_k, dim3(nb), dim3(128), 0, s, W.p, w["e.fc1"], w["e.fc2"], W.gate, m);
    a = v3_args(W.p, w["e.proj.wf"], w["e.proj.b"], W.z);
    a.gate = W.gate;
    v3_conv(v3_proj, L_proj{}, s, m, a, 2);
    if ((rc = v3_launch_check(c, "vec3 encoder.proj")) || (rc = v3_keep(c, "encoder.proj", W.z, 64 * 64, m, s))) return rc;
    hipLaunchKernelGGL(v3::vq_k, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, W.z, w["cb.f"], w["cb.ee"], c->k_pad, idx, m);
    return v3_launch_check(c, "vec3 quantizer");
}

// the decoder from decoder.stem to decoder.up_conv, reading its input [m][64][64] from W.z (workspace of at least m leaves);
// leaves W.u for the tail (final_k, or final_err_k of vq_vec3_bounded.inc)
int v3_decode_body(vqhip_vec3_codec* c, int64_t m, hipStream_t s)
{
    const V3Ws W = v3_ws(c);
    auto& w = c->w;
    const unsigned nb = (unsigned)m;
    int rc = VQHIP_OK;
    v3_conv(v3_stem, L_stem{}, s, m, v3_args(W.z, w["d.stem.wf"], w["d.stem.b"], W.p), 2);
    if ((rc = v3_launch_check(c, "vec3 decoder.stem.0")) || (rc = v3_keep(c, "decoder.stem.0", W.p, 128 * 64, m, s))) return rc;
    hipLaunchKernelGGL((v3::gn_stats_k<128, 64>), dim3(nb), dim3(256), 0, s, W.p, W.stats, m);
    hipLaunchKernelGGL((v3::gn_relu_k<128, 64>), dim3(v3_ew_grid(m * 128 * 64)), dim3(256), 0, s, W.p, W.stats, w["d.stem.g"],
                       w["d.stem.bt"], m);
    if ((rc = v3_launch_check(c, "vec3 decoder.stem")) || (rc = v3_keep(c, "decoder.stem", W.p, 128 * 64, m, s))) return rc;
    if ((rc = v3_rb128(c, "d.rb0", W.p, W.q, W.stats, m, s)) || (rc = v3_keep(c, "decoder.res_stack.0", W.p, 128 * 64, m, s))) return rc;
    if ((rc = v3_rb128(c, "d.rb1", W.p, W.q, W.stats, m, s)) || (rc = v3_keep(c, "decoder.res_stack.1", W.p, 128 * 64, m, s))) return rc;
    hipLaunchKernelGGL(v3::se_k, dim3(nb), dim3(128), 0, s, W.p, w["d.fc1"], w["d.fc2"], W.gate, m);
    v3::ConvArgs a = v3_args(W.p, w["d.up.wf"], w["d.up.b"], W.u);
    a.gate = W.gate;
    v3_conv(v3_up, L_up{}, s, m, a, 2);
    if ((rc = v3_launch_check(c, "vec3 decoder.up_conv"))) return rc;
    return v3_keep(c, "decoder.up_conv", W.u, 256 * 64, m, s);
}

// the decoder from decoder.stem on
int v3_decode_from_z(vqhip_vec3_codec* c, int64_t m, float* out, hipStream_t s)
{
    if (int rc = v3_decode_body(c, m, s)) return rc;
    hipLaunchKernelGGL(v3::final_k, dim3((unsigned)m), dim3(512), V3_LDS_FINAL, s, v3_ws(c).u, c->w["d.final.w"], c->w["d.final.b"], out, m);
    return v3_launch_check(c, "vec3 decoder.final");
}

int v3_decode_chunk(vqhip_vec3_codec* c, const uint16_t* idx, int64_t m, float* out, hipStream_t s)
{
    if (int rc = v3_ensure_ws(c, m)) return rc;
    hipLaunchKernelGGL(v3::gather_k, dim3(v3_ew_grid(m * 4096)), dim3(256), 0, s, idx, c->w["cb"], c->k_codes, v3_ws(c).z, m);
    return v3_decode_from_z(c, m, out, s);
}

// vq_vec3_bf16.inc: the same chunks with bf16 convolution operands
int v3b_encode_chunk(vqhip_vec3_codec* c, const float* leaves, int64_t m, uint16_t* idx, hipStream_t s);
int v3b_decode_chunk(vqhip_vec3_codec* c, const uint16_t* idx, int64_t m, float* out, hipStream_t s);
int v3b_decode_body(vqhip_vec3_codec* c, const uint16_t* idx, int64_t m, hipStream_t s);   // gather to decoder.up_conv

// the public entry points follow the handle's precision mode (training calls v3_encode_chunk / v3_decode_from_z: always fp32)
int v3_encode_mode(vqhip_vec3_codec* c, const float* leaves, int64_t m, uint16_t* idx, hipStream_t s)
{
    return c->precision ? v3b_encode_chunk(c, leaves, m, idx, s) : v3_encode_chunk(c, leaves, m, idx, s);
}

int v3_decode_mode(vqhip_vec3_codec* c, const uint16_t* idx, int64_t m, float* out, hipStream_t s)
{
    return c->precision ? v3b_decode_chunk(c, idx, m, out, s) : v3_decode_chunk(c, idx, m, out, s);
}

int v3_ensure_io(vqhip_vec3_codec* c, int64_t m)
{
    auto nomem = [&](hipError_t) { return "vec3: cannot allocate the I/O buffers of " + std::to_string(m) + " leaves"; };
    if (int rc = ensure(c, c->io_leaves, (size_t)m * 1536, nomem)) return rc;
    return ensure(c, c->io_idx, (size_t)m * 64, nomem);
}

int v3_prepare(vqhip_vec3_codec* c)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->chunk_fitted) v3_fit_chunk(c);
    return VQHIP_OK;
}

// one chunk of the host entry points (m <= c->chunk, after v3_prepare): host leaves -> host indices and back, in the handle's mode
int v3_encode_host_chunk(vqhip_vec3_codec* c, const float* leaves, int64_t m, uint16_t* indices)
{
    if (int rc = v3_ensure_io(c, m)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->io_leaves, leaves, (size_t)m * 1536 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (int rc = v3_encode_mode(c, c->io_leaves, m, c->io_idx, c->stream)) return rc;
    HIPCHK(c, hipMemcpyAsync(indices, c->io_idx, (size_t)m * 64 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VQHIP_OK;
}

int v3_decode_host_chunk(vqhip_vec3_codec* c, const uint16_t* indices, int64_t m, float* leaves)
{
    if (int rc = v3_ensure_io(c, m)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->io_idx, indices, (size_t)m * 64 * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    if (int rc = v3_decode_mode(c, c->io_idx, m, c->io_leaves, c->stream)) return rc;
    HIPCHK(c, hipMemcpyAsync(leaves, c->io_leaves, (size_t)m * 1536 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VQHIP_OK;
}

// the decoder gathers codebook rows by index: every one of n leaves' indices is below K, or nothing is launched.  first_leaf: the
// position of indices[0] in the caller's array, for the message
int v3_check_indices(vqhip_vec3_codec* c, const uint16_t* indices, int64_t n, int64_t first_leaf)
{
    for (int64_t i = 0; i < n * 64; ++i)
        if (indices[i] >= c->k_codes)
            return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decode: index " + std::to_string(indices[i]) + " at leaf " + std::to_string(first_leaf + i / 64) +
                                                     ", position " + std::to_string(i % 64) + " is out of range (num_codes " + std::to_string(c->k_codes) + ")");
    return VQHIP_OK;
}

}  // namespace

extern "C" {

const char* vqhip_vec3_last_error(const vqhip_vec3_codec* c) { return c ? c->err.c_str() : g_v3_create_error.c_str(); }

int vqhip_vec3_create(const char* pack_path, const void* pack_bytes, size_t pack_size, int device_id, vqhip_vec3_codec** out)
{
    if (!out) return v3_fail(nullptr, VQHIP_ERR_INVALID, "vqhip_vec3_create: out is NULL");
    *out = nullptr;
    std::vector<unsigned char> file;
    const unsigned char* p = static_cast<const unsigned char*>(pack_bytes);
    size_t n = pack_size;
    if (pack_path) {
        std::ifstream f(pack_path, std::ios::binary);
        if (!f) return v3_fail(nullptr, VQHIP_ERR_MODEL, std::string("Model file not found at path: ") + pack_path);
        file.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
        p = file.data();
        n = file.size();
    }
    if (!p || !n) return v3_fail(nullptr, VQHIP_ERR_MODEL, "vqhip_vec3_create: no weight pack given");
    std::map<std::string, PackTensor> pk;
    std::string err;
    if (!parse_pack(p, n, pk, err) || !v3_validate(pk, err)) return v3_fail(nullptr, VQHIP_ERR_MODEL, err);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return v3_fail(nullptr, VQHIP_ERR_DEVICE, std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0"));
    if (device_id < 0 || device_id >= ndev) return v3_fail(nullptr, VQHIP_ERR_INVALID, "vqhip_vec3_create: device_id out of range");
    vqhip_vec3_codec* c = new vqhip_vec3_codec();
    c->device = device_id;
    auto bail = [&](int rc) {
        g_v3_create_error = c->err;
        vqhip_vec3_destroy(c);
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
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        c->err = "hipStreamCreate failed";
        return bail(VQHIP_ERR_DEVICE);
    }
    int rc = v3_load(c, pk);
    if (!rc) rc = v3_init_attrs(c);
    if (rc) return bail(rc);
    *out = c;
    return VQHIP_OK;
}

void vqhip_vec3_destroy(vqhip_vec3_codec* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (auto& kv : c->w) hipFree(kv.second);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;   // the buffers go in the struct's destructor, with the device still current
}

int vqhip_vec3_model_info(const vqhip_vec3_codec* c, int64_t* num_codes, int64_t* embedding_dim, int64_t latent[3])
{
    if (!c) return VQHIP_ERR_INVALID;
    if (num_codes) *num_codes = c->k_codes;
    if (embedding_dim) *embedding_dim = 64;
    if (latent) latent[0] = latent[1] = latent[2] = 4;
    return VQHIP_OK;
}

int vqhip_vec3_set_chunk_leaves(vqhip_vec3_codec* c, int64_t chunk)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (chunk < 1 || chunk > V3_MAX_CHUNK)
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 chunk_leaves must be in [1, " + std::to_string(V3_MAX_CHUNK) + "]");
    c->chunk = chunk;
    c->chunk_fitted = false;
    return VQHIP_OK;
}

int64_t vqhip_vec3_chunk_leaves(const vqhip_vec3_codec* c) { return c ? c->chunk : -1; }

int vqhip_vec3_encode_device(vqhip_vec3_codec* c, const float* d_leaves, int64_t n, uint16_t* d_idx, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 encode: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (!d_leaves || !d_idx) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 encode: null pointer");
    if (int rc = v3_prepare(c)) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    for (int64_t o = 0; o < n; o += c->chunk)
        if (int rc = v3_encode_mode(c, d_leaves + o * 1536, std::min(c->chunk, n - o), d_idx + o * 64, s)) return rc;
    return VQHIP_OK;
}

int vqhip_vec3_decode_device(vqhip_vec3_codec* c, const uint16_t* d_idx, int64_t n, float* d_out, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decode: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (!d_idx || !d_out) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decode: null pointer");
    if (int rc = v3_prepare(c)) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    for (int64_t o = 0; o < n; o += c->chunk)
        if (int rc = v3_decode_mode(c, d_idx + o * 64, std::min(c->chunk, n - o), d_out + o * 1536, s)) return rc;
    return VQHIP_OK;
}

int vqhip_vec3_encode(vqhip_vec3_codec* c, const float* leaves, int64_t n, uint16_t* indices)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 encode: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (!leaves || !indices) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 encode: null pointer");
    if (int rc = v3_prepare(c)) return rc;
    for (int64_t o = 0; o < n; o += c->chunk)
        if (int rc = v3_encode_host_chunk(c, leaves + o * 1536, std::min(c->chunk, n - o), indices + o * 64)) return rc;
    return VQHIP_OK;
}

int vqhip_vec3_decode(vqhip_vec3_codec* c, const uint16_t* indices, int64_t n, float* leaves)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decode: n_leaves < 0");
    if (n == 0) return VQHIP_OK;
    if (!leaves || !indices) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 decode: null pointer");
    if (int rc = v3_check_indices(c, indices, n, 0)) return rc;
    if (int rc = v3_prepare(c)) return rc;
    for (int64_t o = 0; o < n; o += c->chunk)
        if (int rc = v3_decode_host_chunk(c, indices + o * 64, std::min(c->chunk, n - o), leaves + o * 1536)) return rc;
    return VQHIP_OK;
}

int vqhip_vec3_debug_enable(vqhip_vec3_codec* c, int on)
{
    if (!c) return VQHIP_ERR_INVALID;
    c->debug = on != 0;
    return VQHIP_OK;
}

int vqhip_vec3_debug_fetch(vqhip_vec3_codec* c, const char* name, int64_t n, float* out)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!name || !out) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 debug_fetch: null pointer");
    auto it = c->dbg.find(name);
    if (it == c->dbg.end() || !it->second.p)
        return v3_fail(c, VQHIP_ERR_INVALID, std::string("vec3 debug_fetch: '") + name + "' was not kept; call vqhip_vec3_debug_enable(1) before the pass");
    if (n < 0 || n > it->second.n)
        return v3_fail(c, VQHIP_ERR_INVALID, std::string("vec3 debug_fetch: the last chunk holds ") + std::to_string(it->second.n) + " leaves");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(out, it->second.p, (size_t)n * it->second.floats * sizeof(float), hipMemcpyDeviceToHost));
    return VQHIP_OK;
}

}  // extern "C"
