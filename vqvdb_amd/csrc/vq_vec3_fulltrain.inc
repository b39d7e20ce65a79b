// vq_vec3_fulltrain.inc — the full training step of the Vec3 model on the Vec3 handle (vqhip_vec3_fulltrain_*;
// include/vqvdb_hip_vec3_fulltrain.h, DESIGN.md §13).  Part of vq_runtime.hip's translation unit, after vq_vec3.inc and
// vq_vec3_train.inc: the forward runs the inference kernels with every activation the backward reads in a buffer of its
// own, the quantizer statistics are stage 1's, and the backward is vq_vec3_fulltrain.h plus conv_k on dgrad fragments.
//
// State: the flat parameter vector P (the 60 tensors of model.parameters(), PyTorch layouts, 5 124 067 floats) and the AdamW
// moments M, V.  P is the source of truth while training; every apply rebuilds the handle's weight tables from it.

#include "vq_vec3_fulltrain.h"
#include "../../include/vqvdb_hip_vec3_fulltrain.h"

namespace {

constexpr int64_t V3F_PARAMS = 5124067, V3F_DECODER_OFFSET = 2235712;
constexpr int V3F_GROUP = 16;                         // leaves per weight-gradient workgroup (and per bias partial)
constexpr int64_t V3F_MAX_WPARAMS = 256 * 128 * 27;   // largest conv weight (decoder.up_conv)

// per-leaf floats of the activation / gradient workspace
constexpr int64_t V3F_T8 = 64 * 512, V3F_T4 = 128 * 64, V3F_U = 256 * 64;
enum { F8_Y0, F8_A0, F8_T, F8_A1, F8_G0, F8_G1, F8_G2, F8_N };
enum { F4_P0, F4_T0, F4_P1, F4_T1, F4_P2, F4_S0, F4_D0, F4_DT0, F4_D1, F4_DT1, F4_D2, F4_N };
enum { ST_Y0, ST_A0, ST_T, ST_P0, ST_T0, ST_P1, ST_T1, ST_S0, ST_D0, ST_DT0, ST_D1, ST_DT1, ST_N };
constexpr int64_t V3F_LEAF_FLOATS = F8_N * V3F_T8 + F4_N * V3F_T4 + 2 * 4096 /*Z, Q*/ + 4 * V3F_U /*U, 3 gradients*/ + 2 * 1536 /*R, dpre*/ +
                                    ST_N * 16 + 2 * 128 /*gates*/ + 32 /*indices*/;

struct V3FWs {
    float* f8[F8_N];
    float* f4[F4_N];
    float *z, *q, *u, *g4[3], *r, *dpre, *st[ST_N], *egate, *dgate;
    uint16_t* idx;
    float* part;
};

int64_t v3f_part_floats(int64_t leaves)
{
    const int64_t groups = (leaves + V3F_GROUP - 1) / V3F_GROUP;
    return std::max(groups * V3F_MAX_WPARAMS, leaves * 8192);
}

V3FWs v3f_layout(float* base, int64_t L)
{
    V3FWs w{};
    float* p = base;
    auto take = [&](int64_t per_leaf) {
        float* r = p;
        p += L * per_leaf;
        return r;
    };
    for (int i = 0; i < F8_N; ++i) w.f8[i] = take(V3F_T8);
    for (int i = 0; i < F4_N; ++i) w.f4[i] = take(V3F_T4);
    w.z = take(4096), w.q = take(4096), w.u = take(V3F_U);
    for (int i = 0; i < 3; ++i) w.g4[i] = take(V3F_U);
    w.r = take(1536), w.dpre = take(1536);
    for (int i = 0; i < ST_N; ++i) w.st[i] = take(16);
    w.egate = take(128), w.dgate = take(128);
    w.idx = reinterpret_cast<uint16_t*>(take(32));
    w.part = p;
    return w;
}

size_t v3f_ws_bytes(int64_t leaves) { return leaves > 0 ? (size_t)(leaves * V3F_LEAF_FLOATS + v3f_part_floats(leaves)) * sizeof(float) : 0; }

// offsets of the 60 tensors in the flat vector (v3_specs order = model.parameters() order), by state_dict name
struct V3FTensor {
    int64_t off, size;
};
const std::map<std::string, V3FTensor>& v3f_tensors()
{
    static const std::map<std::string, V3FTensor> t = [] {
        std::map<std::string, V3FTensor> m;
        int64_t off = 0;
        for (const V3Spec& sp : v3_specs()) {
            int64_t s = 1;
            for (uint32_t d : sp.dims) s *= d;
            m[sp.name] = {off, s};
            off += s;
        }
        return m;
    }();
    return t;
}
int64_t v3f_off(const std::string& name) { return v3f_tensors().at(name).off; }

// the handle's device tables of every conv: (device prefix, state_dict prefix, cout, cin, cin_pad, kt, dgrad scale or 0 = none)
struct V3FConv {
    const char* dev;
    std::string sd;
    int cout, cin, cin_pad, kt;
    float dscale;
};
std::vector<V3FConv> v3f_convs()
{
    std::vector<V3FConv> v = {{"e.pre", "encoder.pre.0", 64, 3, 4, 27, 0.0f}, {"e.down", "encoder.down1", 128, 64, 64, 27, 0.0f},
                              {"e.proj", "encoder.proj", 64, 128, 128, 1, 1.0f},  {"d.stem", "decoder.stem.0", 128, 64, 64, 27, 1.0f},
                              {"d.up", "decoder.up_conv", 256, 128, 128, 27, 1.0f}};
    auto rb = [&](const char* d1, const char* d2, const std::string& p, int ch) {
        v.push_back({d1, p + ".conv1", ch, ch, ch, 27, 1.0f});
        v.push_back({d2, p + ".conv2", ch, ch, ch, 27, 0.1f});   // the residual scale of ResidualBlock, folded into dgrad
    };
    rb("e.rb64.c1", "e.rb64.c2", "encoder.pre.3", 64);
    rb("e.rb0.c1", "e.rb0.c2", "encoder.res_stack.0", 128);
    rb("e.rb1.c1", "e.rb1.c2", "encoder.res_stack.1", 128);
    rb("d.rb0.c1", "d.rb0.c2", "decoder.res_stack.0", 128);
    rb("d.rb1.c1", "d.rb1.c2", "decoder.res_stack.1", 128);
    return v;
}
// raw (unpermuted) device copies: (device name, state_dict name)
std::vector<std::pair<std::string, std::string>> v3f_raws()
{
    std::vector<std::pair<std::string, std::string>> v = {
        {"e.pre.g", "encoder.pre.1.weight"}, {"e.pre.bt", "encoder.pre.1.bias"}, {"e.fc1", "encoder.attn.fc.0.weight"},
        {"e.fc2", "encoder.attn.fc.2.weight"}, {"d.stem.g", "decoder.stem.1.weight"}, {"d.stem.bt", "decoder.stem.1.bias"},
        {"d.fc1", "decoder.attn.fc.0.weight"}, {"d.fc2", "decoder.attn.fc.2.weight"}, {"d.final.w", "decoder.final.weight"},
        {"d.final.b", "decoder.final.bias"}};
    auto rb = [&](const std::string& d, const std::string& p) {
        v.push_back({d + ".g1", p + ".gn1.weight"});
        v.push_back({d + ".b1", p + ".gn1.bias"});
        v.push_back({d + ".g2", p + ".gn2.weight"});
        v.push_back({d + ".b2", p + ".gn2.bias"});
    };
    rb("e.rb64", "encoder.pre.3");
    rb("e.rb0", "encoder.res_stack.0");
    rb("e.rb1", "encoder.res_stack.1");
    rb("d.rb0", "decoder.res_stack.0");
    rb("d.rb1", "decoder.res_stack.1");
    return v;
}

// ---- kernel instantiations: data gradients of the stride-1 convs on conv_k (input = the output gradient) ----------------
//                                       CIN COUT SI SO KS ST PD LPB MT NT INMODE        OUTMODE
constexpr auto v3f_dg_r64 = v3::conv_k<64, 64, 8, 8, 3, 1, 1, 1, 2, 2, v3::IN_PLAIN, v3::OUT_BIAS>;
constexpr auto v3f_dg_r128 = v3::conv_k<128, 128, 4, 4, 3, 1, 1, 2, 1, 2, v3::IN_PLAIN, v3::OUT_BIAS>;
constexpr auto v3f_dg_up = v3::conv_k<256, 128, 4, 4, 3, 1, 1, 1, 1, 2, v3::IN_PLAIN, v3::OUT_BIAS>;
constexpr auto v3f_dg_stem = v3::conv_k<128, 64, 4, 4, 3, 1, 1, 2, 1, 2, v3::IN_PLAIN, v3::OUT_BIAS>;
constexpr auto v3f_dg_proj = v3::conv_k<64, 128, 4, 4, 1, 1, 0, 2, 1, 2, v3::IN_PLAIN, v3::OUT_BIAS>;
using LF_up = V3Launch<256, 128, 4, 4, 1, 1, 2>;
using LF_stem = V3Launch<128, 64, 4, 4, 2, 1, 2>;
using LF_proj = V3Launch<64, 128, 4, 4, 2, 1, 2>;
// weight gradients:                      CIN COUT SI SO KS ST PD INMODE
constexpr auto v3f_wg_pre = v3f::wgrad_k<3, 64, 8, 8, 3, 1, 1, v3::IN_LEAF3>;
constexpr auto v3f_wg_r64 = v3f::wgrad_k<64, 64, 8, 8, 3, 1, 1, v3::IN_GNRELU>;
constexpr auto v3f_wg_down = v3f::wgrad_k<64, 128, 8, 4, 3, 2, 1, v3::IN_PLAIN>;
constexpr auto v3f_wg_r128 = v3f::wgrad_k<128, 128, 4, 4, 3, 1, 1, v3::IN_GNRELU>;
constexpr auto v3f_wg_proj = v3f::wgrad_k<128, 64, 4, 4, 1, 1, 0, v3::IN_GATE>;
constexpr auto v3f_wg_stem = v3f::wgrad_k<64, 128, 4, 4, 3, 1, 1, v3::IN_PLAIN>;
constexpr auto v3f_wg_up = v3f::wgrad_k<128, 256, 4, 4, 3, 1, 1, v3::IN_GATE>;
constexpr auto v3f_wg_final = v3f::wgrad_k<32, 3, 8, 8, 3, 1, 1, v3f::IN_SHUF>;

int v3f_init_attrs(vqhip_vec3_codec* c)
{
    int rc = v3_set_lds(c, v3f_dg_r64, L_r64::lds);
    if (!rc) rc = v3_set_lds(c, v3f_dg_r128, L_r128::lds);
    if (!rc) rc = v3_set_lds(c, v3f_dg_up, LF_up::lds);
    if (!rc) rc = v3_set_lds(c, v3f_dg_stem, LF_stem::lds);
    if (!rc) rc = v3_set_lds(c, v3f_dg_proj, LF_proj::lds);
    if (!rc) rc = v3_set_lds(c, v3f_wg_pre, v3f::wgrad_lds<8, 8>());
    if (!rc) rc = v3_set_lds(c, v3f_wg_r64, v3f::wgrad_lds<8, 8>());
    if (!rc) rc = v3_set_lds(c, v3f_wg_down, v3f::wgrad_lds<8, 4>());
    if (!rc) rc = v3_set_lds(c, v3f_wg_r128, v3f::wgrad_lds<4, 4>());
    if (!rc) rc = v3_set_lds(c, v3f_wg_proj, v3f::wgrad_lds<4, 4>());
    if (!rc) rc = v3_set_lds(c, v3f_wg_stem, v3f::wgrad_lds<4, 4>());
    if (!rc) rc = v3_set_lds(c, v3f_wg_up, v3f::wgrad_lds<4, 4>());
    if (!rc) rc = v3_set_lds(c, v3f_wg_final, v3f::wgrad_lds<8, 8>());
    return rc;
}

int v3f_require(vqhip_vec3_codec* c, const char* what)
{
    if (!c->ft_on) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": call vqhip_vec3_fulltrain_begin first");
    return VQHIP_OK;
}

int v3f_ensure_ws(vqhip_vec3_codec* c, int64_t m)
{
    if (m <= c->ft_leaves) return VQHIP_OK;
    if (int rc = ensure(c, c->ft_ws, v3f_ws_bytes(m) / sizeof(float), [&](hipError_t) { return "vec3 full training: cannot allocate the workspace of " + std::to_string(m) + " leaves"; })) {
        if (!c->ft_ws) c->ft_leaves = 0;   // (a failed synchronise leaves the old block and its layout)
        c->chunk_fitted = false;
        return rc;
    }
    c->ft_leaves = m;
    return VQHIP_OK;
}

// every weight-derived device table from P: forward fragments and biases, GroupNorm / fc / final copies, dgrad fragments,
// down1's transposed table.  All are permutations of P (the dgrad fragments of a conv2 are scaled by 0.1).
int v3f_rebuild(vqhip_vec3_codec* c, hipStream_t s)
{
    auto& w = c->w;
    const float* P = c->ft_P;
    for (const V3FConv& k : v3f_convs()) {
        const int64_t wo = v3f_off(k.sd + ".weight"), bo = v3f_off(k.sd + ".bias");
        const std::string d = k.dev;
        hipLaunchKernelGGL(v3f::frag_k, dim3(512), dim3(256), 0, s, P + wo, k.cout, k.cin, k.cin_pad, k.kt, w[d + ".wf"]);
        HIPCHK(c, hipMemcpyAsync(w[d + ".b"], P + bo, (size_t)k.cout * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (k.dscale != 0.0f) hipLaunchKernelGGL(v3f::dfrag_k, dim3(512), dim3(256), 0, s, P + wo, k.cout, k.cin, k.kt, k.dscale, w[d + ".df"]);
    }
    hipLaunchKernelGGL(v3f::downT_k, dim3(256), dim3(256), 0, s, P + v3f_off("encoder.down1.weight"), w["e.down.wt"]);
    for (const auto& r : v3f_raws()) {
        const V3FTensor& t = v3f_tensors().at(r.second);
        HIPCHK(c, hipMemcpyAsync(w[r.first], P + t.off, (size_t)t.size * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    if (c->bf_ready)   // bf16 inference mode: its fragments follow the fp32 ones just rebuilt
        if (int rc = v3b_refrag(c, s)) return rc;
    return v3_launch_check(c, "vec3 full training: weight tables");
}

// P from the handle's current tables (host inverse of v3_frag; the raw tensors are copies)
int v3f_params_from_tables(vqhip_vec3_codec* c, std::vector<float>& P)
{
    P.assign(V3F_PARAMS, 0.0f);
    for (const V3FConv& k : v3f_convs()) {
        const int64_t wo = v3f_off(k.sd + ".weight"), bo = v3f_off(k.sd + ".bias");
        std::vector<float> f((size_t)k.cout * k.cin_pad * k.kt);
        HIPCHK(c, hipMemcpy(f.data(), c->w[std::string(k.dev) + ".wf"], f.size() * sizeof(float), hipMemcpyDeviceToHost));
        const int cp_n = k.cin_pad / 2;
        for (int ct = 0; ct < k.cout / 32; ++ct)
            for (int t = 0; t < k.kt; ++t)
                for (int cp = 0; cp < cp_n; ++cp)
                    for (int l = 0; l < 64; ++l) {
                        const int co = 32 * ct + (l & 31), ci = 2 * cp + (l >> 5);
                        if (ci < k.cin) P[wo + ((size_t)co * k.cin + ci) * k.kt + t] = f[(((size_t)ct * k.kt + t) * cp_n + cp) * 64 + l];
                    }
        HIPCHK(c, hipMemcpy(P.data() + bo, c->w[std::string(k.dev) + ".b"], (size_t)k.cout * sizeof(float), hipMemcpyDeviceToHost));
    }
    for (const auto& r : v3f_raws()) {
        const V3FTensor& t = v3f_tensors().at(r.second);
        HIPCHK(c, hipMemcpy(P.data() + t.off, c->w[r.first], (size_t)t.size * sizeof(float), hipMemcpyDeviceToHost));
    }
    return VQHIP_OK;
}

int v3f_alloc(vqhip_vec3_codec* c, const std::string& name, size_t floats)
{
    if (c->w.count(name)) return VQHIP_OK;
    float* d = nullptr;
    if (hipMalloc(&d, floats * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return v3_fail(c, VQHIP_ERR_NOMEM, "vec3 fulltrain_begin: cannot allocate " + name);
    }
    c->w[name] = d;
    return VQHIP_OK;
}

// ---- launch helpers -----------------------------------------------------------------------------------------------------
unsigned v3f_groups(int64_t m) { return (unsigned)((m + V3F_GROUP - 1) / V3F_GROUP); }

void v3f_reduce(hipStream_t s, const float* part, int64_t groups, int64_t stride, int64_t count, float* out)
{
    const unsigned blocks = (unsigned)std::min<int64_t>(4096, (count + 255) / 256);
    hipLaunchKernelGGL(v3f::reduce_k, dim3(blocks), dim3(256), 0, s, part, groups, stride, count, out);
}

// weight gradient of a conv (kernel K with CIN / COUT / KT as given) into grads + off, then its bias gradient into the next C
template <int CIN, int COUT, int KT, typename K>
void v3f_wgrad(K kernel, size_t lds, hipStream_t s, int64_t m, v3f::WgradArgs a, float* grads, int64_t off, int npo)
{
    a.n = m, a.group = V3F_GROUP;
    const unsigned groups = v3f_groups(m);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(((CIN + 31) / 32) * ((COUT + 31) / 32)), groups), dim3(v3f::WG_THREADS), lds, s, a);
    const int64_t np = (int64_t)COUT * CIN * KT;
    v3f_reduce(s, a.part, groups, np, np, grads + off);
    hipLaunchKernelGGL(v3f::bias_part_k, dim3(groups), dim3(256), 0, s, a.dy, COUT, npo, m, V3F_GROUP, a.dy_scale, a.part);
    v3f_reduce(s, a.part, groups, COUT, COUT, grads + off + np);
}

v3f::WgradArgs v3f_wargs(const float* dy, const float* in, float* part)
{
    v3f::WgradArgs a{};
    a.dy = dy, a.in = in, a.part = part, a.dy_scale = 1.0f;
    return a;
}

// ResidualBlock forward into separate buffers: t = conv1(relu(gn1(x))), y = x + 0.1 conv2(relu(gn2(t)))
template <typename KA, typename KB, typename L>
void v3f_rb_fwd(vqhip_vec3_codec* c, KA ka, KB kb, L lt, int lpb, const std::string& p, int ch, int np, const float* x, float* st_x, float* t,
                float* st_t, float* y, int64_t m, hipStream_t s)
{
    const unsigned nb = (unsigned)m;
    if (ch == 64) hipLaunchKernelGGL((v3::gn_stats_k<64, 512>), dim3(nb), dim3(256), 0, s, x, st_x, m);
    else hipLaunchKernelGGL((v3::gn_stats_k<128, 64>), dim3(nb), dim3(256), 0, s, x, st_x, m);
    v3::ConvArgs a = v3_args(x, c->w[p + ".c1.wf"], c->w[p + ".c1.b"], t);
    a.stats = st_x, a.gamma = c->w[p + ".g1"], a.beta = c->w[p + ".b1"];
    v3_conv(ka, lt, s, m, a, lpb);
    if (ch == 64) hipLaunchKernelGGL((v3::gn_stats_k<64, 512>), dim3(nb), dim3(256), 0, s, t, st_t, m);
    else hipLaunchKernelGGL((v3::gn_stats_k<128, 64>), dim3(nb), dim3(256), 0, s, t, st_t, m);
    a = v3_args(t, c->w[p + ".c2.wf"], c->w[p + ".c2.b"], y);
    a.stats = st_t, a.gamma = c->w[p + ".g2"], a.beta = c->w[p + ".b2"], a.res = x;
    v3_conv(kb, lt, s, m, a, lpb);
    (void)np;
}

// ResidualBlock backward.  dy: gradient of the block output, replaced by the gradient of its input x; t1, t2: scratch.
template <int C, int NP, typename KW, typename KD, typename L>
void v3f_rb_bwd(vqhip_vec3_codec* c, KW kw, KD kd, L lt, int lpb, const std::string& p, const std::string& sd, const float* x, const float* st_x,
                const float* t, const float* st_t, float* dy, float* t1, float* t2, float* part, float* grads, int64_t m, hipStream_t s)
{
    auto& w = c->w;
    constexpr int S = NP == 512 ? 8 : 4;
    const size_t lds = v3f::wgrad_lds<S, S>();
    const unsigned nb = (unsigned)m;
    // conv2: weight gradient from 0.1 dy on relu(gn2(t)), data gradient through the 0.1-scaled dgrad fragments
    v3f::WgradArgs a = v3f_wargs(dy, t, part);
    a.stats = st_t, a.gamma = w[p + ".g2"], a.beta = w[p + ".b2"], a.dy_scale = 0.1f;
    v3f_wgrad<C, C, 27>(kw, lds, s, m, a, grads, v3f_off(sd + ".conv2.weight"), NP);
    v3_conv(kd, lt, s, m, v3_args(dy, w[p + ".c2.df"], w["ft.zero"], t1), lpb);
    hipLaunchKernelGGL((v3f::gn_bwd_k<C, NP>), dim3(nb), dim3(256), 0, s, t, st_t, w[p + ".g2"], w[p + ".b2"], t1, nullptr, t2, part, m);
    v3f_reduce(s, part, m, 2 * C, 2 * C, grads + v3f_off(sd + ".gn2.weight"));
    // conv1 on relu(gn1(x))
    a = v3f_wargs(t2, x, part);
    a.stats = st_x, a.gamma = w[p + ".g1"], a.beta = w[p + ".b1"];
    v3f_wgrad<C, C, 27>(kw, lds, s, m, a, grads, v3f_off(sd + ".conv1.weight"), NP);
    v3_conv(kd, lt, s, m, v3_args(t2, w[p + ".c1.df"], w["ft.zero"], t1), lpb);
    hipLaunchKernelGGL((v3f::gn_bwd_k<C, NP>), dim3(nb), dim3(256), 0, s, x, st_x, w[p + ".g1"], w[p + ".b1"], t1, dy, dy, part, m);
    v3f_reduce(s, part, m, 2 * C, 2 * C, grads + v3f_off(sd + ".gn1.weight"));
}

// training-mode forward of m leaves (m <= ft_leaves, > 0): every activation the backward reads, indices, reconstruction
int v3f_forward(vqhip_vec3_codec* c, const float* leaves, int64_t m, hipStream_t s, V3FWs& F)
{
    auto& w = c->w;
    F = v3f_layout(c->ft_ws, c->ft_leaves);
    const unsigned nb = (unsigned)m;
    int rc = VQHIP_OK;
    float** A = F.f8;
    float** B = F.f4;
    // encoder.pre: conv 3->64, GroupNorm + ReLU, ResidualBlock(64)
    v3_conv(v3_pre, L_pre{}, s, m, v3_args(leaves, w["e.pre.wf"], w["e.pre.b"], A[F8_Y0]), 1);
    if ((rc = v3_launch_check(c, "vec3 ft encoder.pre.0")) || (rc = v3_keep(c, "encoder.pre.0", A[F8_Y0], 64 * 512, m, s))) return rc;
    hipLaunchKernelGGL((v3::gn_stats_k<64, 512>), dim3(nb), dim3(256), 0, s, A[F8_Y0], F.st[ST_Y0], m);
    HIPCHK(c, hipMemcpyAsync(A[F8_A0], A[F8_Y0], (size_t)m * V3F_T8 * sizeof(float), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL((v3::gn_relu_k<64, 512>), dim3(v3_ew_grid(m * 64 * 512)), dim3(256), 0, s, A[F8_A0], F.st[ST_Y0], w["e.pre.g"],
                       w["e.pre.bt"], m);
    if ((rc = v3_launch_check(c, "vec3 ft encoder.pre.1")) || (rc = v3_keep(c, "encoder.pre.2", A[F8_A0], 64 * 512, m, s))) return rc;
    v3f_rb_fwd(c, v3_r64a, v3_r64b, L_r64{}, 1, "e.rb64", 64, 512, A[F8_A0], F.st[ST_A0], A[F8_T], F.st[ST_T], A[F8_A1], m, s);
    if ((rc = v3_launch_check(c, "vec3 ft encoder.pre.3")) || (rc = v3_keep(c, "encoder.pre", A[F8_A1], 64 * 512, m, s))) return rc;
    v3_conv(v3_down, L_down{}, s, m, v3_args(A[F8_A1], w["e.down.wf"], w["e.down.b"], B[F4_P0]), 1);
    if ((rc = v3_launch_check(c, "vec3 ft encoder.down1")) || (rc = v3_keep(c, "encoder.down1", B[F4_P0], 128 * 64, m, s))) return rc;
    v3f_rb_fwd(c, v3_r128a, v3_r128b, L_r128{}, 2, "e.rb0", 128, 64, B[F4_P0], F.st[ST_P0], B[F4_T0], F.st[ST_T0], B[F4_P1], m, s);
    if ((rc = v3_launch_check(c, "vec3 ft e.rb0")) || (rc = v3_keep(c, "encoder.res_stack.0", B[F4_P1], 128 * 64, m, s))) return rc;
    v3f_rb_fwd(c, v3_r128a, v3_r128b, L_r128{}, 2, "e.rb1", 128, 64, B[F4_P1], F.st[ST_P1], B[F4_T1], F.st[ST_T1], B[F4_P2], m, s);
    if ((rc = v3_launch_check(c, "vec3 ft e.rb1")) || (rc = v3_keep(c, "encoder.res_stack.1", B[F4_P2], 128 * 64, m, s))) return rc;
    hipLaunchKernelGGL(v3::se_k, dim3(nb), dim3(128), 0, s, B[F4_P2], w["e.fc1"], w["e.fc2"], F.egate, m);
    v3::ConvArgs a = v3_args(B[F4_P2], w["e.proj.wf"], w["e.proj.b"], F.z);
    a.gate = F.egate;
    v3_conv(v3_proj, L_proj{}, s, m, a, 2);
    if ((rc = v3_launch_check(c, "vec3 ft encoder.proj")) || (rc = v3_keep(c, "encoder.proj", F.z, 64 * 64, m, s))) return rc;
    hipLaunchKernelGGL(v3::vq_k, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, F.z, w["cb.f"], w["cb.ee"], c->k_pad, F.idx, m);
    // decoder on the straight-through value z + (e - z), the codebook before this step's update
    HIPCHK(c, hipMemcpyAsync(F.q, F.z, (size_t)m * 4096 * sizeof(float), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(v3t::straight_k, dim3(v3_ew_grid(m * 4096)), dim3(256), 0, s, F.q, F.idx, w["cb"], m);
    v3_conv(v3_stem, L_stem{}, s, m, v3_args(F.q, w["d.stem.wf"], w["d.stem.b"], B[F4_S0]), 2);
    if ((rc = v3_launch_check(c, "vec3 ft decoder.stem.0")) || (rc = v3_keep(c, "decoder.stem.0", B[F4_S0], 128 * 64, m, s))) return rc;
    hipLaunchKernelGGL((v3::gn_stats_k<128, 64>), dim3(nb), dim3(256), 0, s, B[F4_S0], F.st[ST_S0], m);
    HIPCHK(c, hipMemcpyAsync(B[F4_D0], B[F4_S0], (size_t)m * V3F_T4 * sizeof(float), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL((v3::gn_relu_k<128, 64>), dim3(v3_ew_grid(m * 128 * 64)), dim3(256), 0, s, B[F4_D0], F.st[ST_S0], w["d.stem.g"],
                       w["d.stem.bt"], m);
    if ((rc = v3_launch_check(c, "vec3 ft decoder.stem")) || (rc = v3_keep(c, "decoder.stem", B[F4_D0], 128 * 64, m, s))) return rc;
    v3f_rb_fwd(c, v3_r128a, v3_r128b, L_r128{}, 2, "d.rb0", 128, 64, B[F4_D0], F.st[ST_D0], B[F4_DT0], F.st[ST_DT0], B[F4_D1], m, s);
    if ((rc = v3_launch_check(c, "vec3 ft d.rb0")) || (rc = v3_keep(c, "decoder.res_stack.0", B[F4_D1], 128 * 64, m, s))) return rc;
    v3f_rb_fwd(c, v3_r128a, v3_r128b, L_r128{}, 2, "d.rb1", 128, 64, B[F4_D1], F.st[ST_D1], B[F4_DT1], F.st[ST_DT1], B[F4_D2], m, s);
    if ((rc = v3_launch_check(c, "vec3 ft d.rb1")) || (rc = v3_keep(c, "decoder.res_stack.1", B[F4_D2], 128 * 64, m, s))) return rc;
    hipLaunchKernelGGL(v3::se_k, dim3(nb), dim3(128), 0, s, B[F4_D2], w["d.fc1"], w["d.fc2"], F.dgate, m);
    a = v3_args(B[F4_D2], w["d.up.wf"], w["d.up.b"], F.u);
    a.gate = F.dgate;
    v3_conv(v3_up, L_up{}, s, m, a, 2);
    if ((rc = v3_launch_check(c, "vec3 ft decoder.up_conv")) || (rc = v3_keep(c, "decoder.up_conv", F.u, 256 * 64, m, s))) return rc;
    hipLaunchKernelGGL(v3::final_k, dim3(nb), dim3(512), V3_LDS_FINAL, s, F.u, w["d.final.w"], w["d.final.b"], F.r, m);
    return v3_launch_check(c, "vec3 ft decoder.final");
}

// backward of m leaves after v3f_forward: grads [V3F_PARAMS] (local sums of the global-batch mean's gradient)
int v3f_backward(vqhip_vec3_codec* c, const float* leaves, int64_t m, int64_t n_global, float* grads, const V3FWs& F, hipStream_t s)
{
    auto& w = c->w;
    const unsigned nb = (unsigned)m;
    float* const* A = F.f8;
    float* const* B = F.f4;
    float* const* G = F.g4;
    float* part = F.part;
    const float inv_count = (float)(1.0 / ((double)n_global * 1536.0));
    // loss -> final: dpre, final's weight / bias gradients, du [256][64] into G[0]
    hipLaunchKernelGGL(v3f::loss_final_bwd_k, dim3(nb), dim3(512), 0, s, F.r, leaves, w["d.final.w"], inv_count, F.dpre, G[0], m);
    v3f_wgrad<32, 3, 27>(v3f_wg_final, v3f::wgrad_lds<8, 8>(), s, m, v3f_wargs(F.dpre, F.u, part), grads, v3f_off("decoder.final.weight"), 512);
    // up_conv on the gated decoder features
    v3f::WgradArgs a = v3f_wargs(G[0], B[F4_D2], part);
    a.gate = F.dgate;
    v3f_wgrad<128, 256, 27>(v3f_wg_up, v3f::wgrad_lds<4, 4>(), s, m, a, grads, v3f_off("decoder.up_conv.weight"), 64);
    v3_conv(v3f_dg_up, LF_up{}, s, m, v3_args(G[0], w["d.up.df"], w["ft.zero"], G[1]), 1);
    hipLaunchKernelGGL(v3f::se_bwd_k, dim3(nb), dim3(128), 0, s, B[F4_D2], w["d.fc1"], w["d.fc2"], G[1], G[2], part, m);
    v3f_reduce(s, part, m, 8192, 8192, grads + v3f_off("decoder.attn.fc.0.weight"));
    if (int rc = v3_launch_check(c, "vec3 ft backward: decoder tail")) return rc;
    v3f_rb_bwd<128, 64>(c, v3f_wg_r128, v3f_dg_r128, L_r128{}, 2, "d.rb1", "decoder.res_stack.1", B[F4_D1], F.st[ST_D1], B[F4_DT1], F.st[ST_DT1], G[2],
                        G[0], G[1], part, grads, m, s);
    v3f_rb_bwd<128, 64>(c, v3f_wg_r128, v3f_dg_r128, L_r128{}, 2, "d.rb0", "decoder.res_stack.0", B[F4_D0], F.st[ST_D0], B[F4_DT0], F.st[ST_DT0], G[2],
                        G[0], G[1], part, grads, m, s);
    hipLaunchKernelGGL((v3f::gn_bwd_k<128, 64>), dim3(nb), dim3(256), 0, s, B[F4_S0], F.st[ST_S0], w["d.stem.g"], w["d.stem.bt"], G[2], nullptr, G[0],
                       part, m);
    v3f_reduce(s, part, m, 256, 256, grads + v3f_off("decoder.stem.1.weight"));
    v3f_wgrad<64, 128, 27>(v3f_wg_stem, v3f::wgrad_lds<4, 4>(), s, m, v3f_wargs(G[0], F.q, part), grads, v3f_off("decoder.stem.0.weight"), 64);
    v3_conv(v3f_dg_stem, LF_stem{}, s, m, v3_args(G[0], w["d.stem.df"], w["ft.zero"], G[1]), 2);
    if (int rc = v3_launch_check(c, "vec3 ft backward: decoder")) return rc;
    // quantizer: straight-through plus the commitment term 0.25 mean((z - e)^2) over n_global * 4096 values
    const float coef = (float)(0.25 * 2.0 / ((double)n_global * 4096.0));
    hipLaunchKernelGGL(v3f::dz_k, dim3(v3_ew_grid(m * 4096)), dim3(256), 0, s, G[1], F.z, F.idx, w["cb"], coef, G[2], m);
    // encoder.proj on the gated features, ChannelAttention, the two ResidualBlock(128)
    a = v3f_wargs(G[2], B[F4_P2], part);
    a.gate = F.egate;
    v3f_wgrad<128, 64, 1>(v3f_wg_proj, v3f::wgrad_lds<4, 4>(), s, m, a, grads, v3f_off("encoder.proj.weight"), 64);
    v3_conv(v3f_dg_proj, LF_proj{}, s, m, v3_args(G[2], w["e.proj.df"], w["ft.zero"], G[0]), 2);
    hipLaunchKernelGGL(v3f::se_bwd_k, dim3(nb), dim3(128), 0, s, B[F4_P2], w["e.fc1"], w["e.fc2"], G[0], G[1], part, m);
    v3f_reduce(s, part, m, 8192, 8192, grads + v3f_off("encoder.attn.fc.0.weight"));
    v3f_rb_bwd<128, 64>(c, v3f_wg_r128, v3f_dg_r128, L_r128{}, 2, "e.rb1", "encoder.res_stack.1", B[F4_P1], F.st[ST_P1], B[F4_T1], F.st[ST_T1], G[1],
                        G[0], G[2], part, grads, m, s);
    v3f_rb_bwd<128, 64>(c, v3f_wg_r128, v3f_dg_r128, L_r128{}, 2, "e.rb0", "encoder.res_stack.0", B[F4_P0], F.st[ST_P0], B[F4_T0], F.st[ST_T0], G[1],
                        G[0], G[2], part, grads, m, s);
    if (int rc = v3_launch_check(c, "vec3 ft backward: encoder 4^3")) return rc;
    // down1 (k3 s2 p1), ResidualBlock(64), GroupNorm of encoder.pre, encoder.pre.0 (no data gradient)
    v3f_wgrad<64, 128, 27>(v3f_wg_down, v3f::wgrad_lds<8, 4>(), s, m, v3f_wargs(G[1], A[F8_A1], part), grads, v3f_off("encoder.down1.weight"), 64);
    hipLaunchKernelGGL(v3f::down_dgrad_k, dim3(nb), dim3(512), 0, s, G[1], w["e.down.wt"], A[F8_G0], m);
    v3f_rb_bwd<64, 512>(c, v3f_wg_r64, v3f_dg_r64, L_r64{}, 1, "e.rb64", "encoder.pre.3", A[F8_A0], F.st[ST_A0], A[F8_T], F.st[ST_T], A[F8_G0],
                        A[F8_G1], A[F8_G2], part, grads, m, s);
    hipLaunchKernelGGL((v3f::gn_bwd_k<64, 512>), dim3(nb), dim3(256), 0, s, A[F8_Y0], F.st[ST_Y0], w["e.pre.g"], w["e.pre.bt"], A[F8_G0], nullptr,
                       A[F8_G1], part, m);
    v3f_reduce(s, part, m, 128, 128, grads + v3f_off("encoder.pre.1.weight"));
    v3f_wgrad<3, 64, 27>(v3f_wg_pre, v3f::wgrad_lds<8, 8>(), s, m, v3f_wargs(A[F8_G1], leaves, part), grads, v3f_off("encoder.pre.0.weight"), 512);
    return v3_launch_check(c, "vec3 ft backward: encoder 8^3");
}

int v3f_check_batch(vqhip_vec3_codec* c, const char* what, const float* leaves, int64_t n)
{
    if (int rc = v3f_require(c, what)) return rc;
    if (n < 0) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": n_leaves < 0");
    if (n > 0 && !leaves) return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": leaves_dev is NULL");
    if (n > c->chunk)
        return v3_fail(c, VQHIP_ERR_INVALID, std::string(what) + ": " + std::to_string(n) + " leaves exceed the chunk of " + std::to_string(c->chunk) +
                                                 " (vqhip_vec3_chunk_leaves)");
    return VQHIP_OK;
}

}  // namespace

extern "C" {

int64_t vqhip_vec3_fulltrain_param_count(const vqhip_vec3_codec* c) { return c ? V3F_PARAMS : -1; }

int64_t vqhip_vec3_fulltrain_decoder_offset(const vqhip_vec3_codec* c) { return c ? V3F_DECODER_OFFSET : -1; }

int64_t vqhip_vec3_fulltrain_aux_floats(const vqhip_vec3_codec* c) { return c ? (int64_t)66 * c->k_codes + 4 : -1; }

int vqhip_vec3_fulltrain_begin(vqhip_vec3_codec* c)
{
    if (!c) return VQHIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (!c->training)
        if (int rc = vqhip_vec3_train_begin(c, nullptr, nullptr)) return rc;
    int rc = VQHIP_OK;
    for (const V3FConv& k : v3f_convs())
        if (!rc && k.dscale != 0.0f) rc = v3f_alloc(c, std::string(k.dev) + ".df", (size_t)k.cout * k.cin * k.kt);
    if (!rc) rc = v3f_alloc(c, "e.down.wt", (size_t)128 * 64 * 27);
    if (!rc) rc = v3f_alloc(c, "ft.zero", 256);
    if (!rc) rc = v3f_alloc(c, "ft.P", V3F_PARAMS);
    if (!rc) rc = v3f_alloc(c, "ft.M", V3F_PARAMS);
    if (!rc) rc = v3f_alloc(c, "ft.V", V3F_PARAMS);
    if (!rc) rc = v3f_init_attrs(c);
    if (rc) return rc;
    c->ft_P = c->w["ft.P"], c->ft_M = c->w["ft.M"], c->ft_V = c->w["ft.V"];
    std::vector<float> P;
    if ((rc = v3f_params_from_tables(c, P))) return rc;
    HIPCHK(c, hipMemcpy(c->ft_P, P.data(), (size_t)V3F_PARAMS * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(c->ft_M, 0, (size_t)V3F_PARAMS * sizeof(float)));
    HIPCHK(c, hipMemset(c->ft_V, 0, (size_t)V3F_PARAMS * sizeof(float)));
    HIPCHK(c, hipMemset(c->w["ft.zero"], 0, 256 * sizeof(float)));
    if ((rc = v3f_rebuild(c, c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ft_on = true;
    c->chunk_fitted = false;   // the next call fits the chunk to all three workspaces
    return VQHIP_OK;
}

int vqhip_vec3_fulltrain_forward_device(vqhip_vec3_codec* c, const float* leaves_dev, int64_t n, uint16_t* indices_dev, float* recon_dev,
                                        void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3f_require(c, "vec3 fulltrain_forward")) return rc;
    if (int rc = v3_prepare(c)) return rc;
    if (int rc = v3f_check_batch(c, "vec3 fulltrain_forward", leaves_dev, n)) return rc;
    if (n == 0) return VQHIP_OK;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (int rc = v3f_ensure_ws(c, n)) return rc;
    V3FWs F;
    if (int rc = v3f_forward(c, leaves_dev, n, s, F)) return rc;
    if (indices_dev) HIPCHK(c, hipMemcpyAsync(indices_dev, F.idx, (size_t)n * 64 * sizeof(uint16_t), hipMemcpyDeviceToDevice, s));
    if (recon_dev) HIPCHK(c, hipMemcpyAsync(recon_dev, F.r, (size_t)n * 1536 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return VQHIP_OK;
}

int vqhip_vec3_fulltrain_fwdbwd_device(vqhip_vec3_codec* c, const float* leaves_dev, int64_t n, int64_t n_global, float* grads_dev, float* aux_dev,
                                       float* latent_dev, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3f_require(c, "vec3 fulltrain_fwdbwd")) return rc;
    if (int rc = v3_prepare(c)) return rc;
    if (int rc = v3f_check_batch(c, "vec3 fulltrain_fwdbwd", leaves_dev, n)) return rc;
    if (n_global < n || n_global < 1) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 fulltrain_fwdbwd: n_global must be >= n and >= 1");
    if (!grads_dev) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 fulltrain_fwdbwd: grads_dev is NULL");
    if (!aux_dev) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 fulltrain_fwdbwd: aux_dev is NULL");
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const int64_t naux = vqhip_vec3_fulltrain_aux_floats(c);
    if (n == 0) {
        HIPCHK(c, hipMemsetAsync(grads_dev, 0, (size_t)V3F_PARAMS * sizeof(float), s));
        HIPCHK(c, hipMemsetAsync(aux_dev, 0, (size_t)naux * sizeof(float), s));
        return VQHIP_OK;
    }
    if (int rc = v3_ensure_ws(c, n)) return rc;
    if (int rc = v3t_ensure_ws(c, n)) return rc;
    if (int rc = v3f_ensure_ws(c, n)) return rc;
    const V3TWs T = v3t_layout(c->tr_ws, c->tr_leaves, c->k_codes);
    V3FWs F;
    if (int rc = v3f_forward(c, leaves_dev, n, s, F)) return rc;
    // aux: stage-1 statistics of this batch against the codebook before the update, then the reconstruction sums
    float* flat = latent_dev ? latent_dev : T.flat;
    hipLaunchKernelGGL(v3t::flat_k, dim3((unsigned)n), dim3(256), 0, s, F.z, flat, n);
    if (int rc = v3t_stats(c, T, flat, F.idx, n * 64, aux_dev, s)) return rc;
    hipLaunchKernelGGL(recon_loss_partials_k, dim3(RL_BLOCKS), dim3(256), 0, s, leaves_dev, F.r, n * 1536, T.rl);
    hipLaunchKernelGGL(recon_loss_reduce_k, dim3(1), dim3(1), 0, s, T.rl, n * 1536, aux_dev + 66 * (int64_t)c->k_codes + 1);
    if (int rc = v3_launch_check(c, "vec3 ft loss sums")) return rc;
    return v3f_backward(c, leaves_dev, n, n_global, grads_dev, F, s);
}

int vqhip_vec3_fulltrain_apply_device(vqhip_vec3_codec* c, const float* grads_dev, const float* aux_dev, float lr, int64_t step, float beta1,
                                      float beta2, float adam_eps, float weight_decay, float ema_decay, float ema_eps, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3f_require(c, "vec3 fulltrain_apply")) return rc;
    if (!grads_dev) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 fulltrain_apply: grads_dev is NULL");
    if (step < 1) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 fulltrain_apply: step must be >= 1");
    if (!(lr >= 0.0f) || !(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(adam_eps > 0.0f) || !(weight_decay >= 0.0f))
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 fulltrain_apply: lr, betas, eps or weight_decay out of range");
    if (aux_dev && (!(ema_decay >= 0.0f && ema_decay <= 1.0f) || !(ema_eps > 0.0f)))
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 fulltrain_apply: ema decay must be in [0, 1] and ema eps > 0");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const float bc1 = (float)(1.0 - std::pow((double)beta1, (double)step)), bc2s = (float)std::sqrt(1.0 - std::pow((double)beta2, (double)step));
    hipLaunchKernelGGL(adamw_k, dim3(1024), dim3(256), 0, s, c->ft_P, grads_dev, c->ft_M, c->ft_V, V3F_PARAMS, lr, beta1, beta2, adam_eps, weight_decay,
                       bc1, bc2s);
    if (int rc = v3_launch_check(c, "vec3 ft AdamW")) return rc;
    if (aux_dev) {
        const float alpha = (float)(1.0 - (double)ema_decay);
        hipLaunchKernelGGL(v3t::ema_update_k, dim3((c->k_codes + 3) / 4), dim3(256), 0, s, aux_dev, c->k_codes, ema_decay, alpha, ema_eps, c->tr_cs,
                           c->tr_avg, c->w["cb"]);
        if (int rc = v3_launch_check(c, "vec3 ft EMA update")) return rc;
        if (int rc = v3t_rebuild_tables(c, s)) return rc;
    }
    return v3f_rebuild(c, s);
}

int vqhip_vec3_fulltrain_get_params(vqhip_vec3_codec* c, float* params)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3f_require(c, "vec3 fulltrain_get_params")) return rc;
    if (!params) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 fulltrain_get_params: params is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(params, c->ft_P, (size_t)V3F_PARAMS * sizeof(float), hipMemcpyDeviceToHost));
    return VQHIP_OK;
}

int vqhip_vec3_fulltrain_set_params(vqhip_vec3_codec* c, const float* params)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3f_require(c, "vec3 fulltrain_set_params")) return rc;
    if (!params) return v3_fail(c, VQHIP_ERR_INVALID, "vec3 fulltrain_set_params: params is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(c->ft_P, params, (size_t)V3F_PARAMS * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = v3f_rebuild(c, c->stream)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VQHIP_OK;
}

int vqhip_vec3_fulltrain_get_opt_state(vqhip_vec3_codec* c, float* exp_avg, float* exp_avg_sq)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3f_require(c, "vec3 fulltrain_get_opt_state")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (exp_avg) HIPCHK(c, hipMemcpy(exp_avg, c->ft_M, (size_t)V3F_PARAMS * sizeof(float), hipMemcpyDeviceToHost));
    if (exp_avg_sq) HIPCHK(c, hipMemcpy(exp_avg_sq, c->ft_V, (size_t)V3F_PARAMS * sizeof(float), hipMemcpyDeviceToHost));
    return VQHIP_OK;
}

int vqhip_vec3_fulltrain_set_opt_state(vqhip_vec3_codec* c, const float* exp_avg, const float* exp_avg_sq)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (int rc = v3f_require(c, "vec3 fulltrain_set_opt_state")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (exp_avg) HIPCHK(c, hipMemcpy(c->ft_M, exp_avg, (size_t)V3F_PARAMS * sizeof(float), hipMemcpyHostToDevice));
    if (exp_avg_sq) HIPCHK(c, hipMemcpy(c->ft_V, exp_avg_sq, (size_t)V3F_PARAMS * sizeof(float), hipMemcpyHostToDevice));
    return VQHIP_OK;
}

}  // extern "C"
