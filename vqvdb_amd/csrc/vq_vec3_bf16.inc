// vq_vec3_bf16.inc — runtime of the Vec3 handle's bf16-operand inference mode (include/vqvdb_hip_vec3_precision.h,
// DESIGN.md §14).  Part of vq_runtime.hip's translation unit, after vq_vec3.inc.  The bf16 weight fragments live beside the
// fp32 ones (c->w["<conv>.wb"]), are built on the device from them at the first switch to bf16, and are rebuilt wherever full
// training rebuilds the fp32 tables (v3f_rebuild).  Everything that is not a convolution launches the fp32 path's kernels.

#include "vq_vec3_bf16.h"
#include "../../include/vqvdb_hip_vec3_precision.h"

namespace {

struct V3BConv {
    const char* dev;
    int cout, cin_src, kt, pair;   // cin_src: input channels of the fp32 fragments (4 for encoder.pre.0)
};
const V3BConv V3B_CONVS[] = {
    {"e.pre", 64, 4, 27, 1},       {"e.rb64.c1", 64, 64, 27, 0},  {"e.rb64.c2", 64, 64, 27, 0},  {"e.down", 128, 64, 27, 0},
    {"e.rb0.c1", 128, 128, 27, 0}, {"e.rb0.c2", 128, 128, 27, 0}, {"e.rb1.c1", 128, 128, 27, 0}, {"e.rb1.c2", 128, 128, 27, 0},
    {"e.proj", 64, 128, 1, 0},     {"d.stem", 128, 64, 27, 0},    {"d.rb0.c1", 128, 128, 27, 0}, {"d.rb0.c2", 128, 128, 27, 0},
    {"d.rb1.c1", 128, 128, 27, 0}, {"d.rb1.c2", 128, 128, 27, 0}, {"d.up", 256, 128, 27, 0},
};
size_t v3b_frag_bytes(const V3BConv& k)
{
    const size_t ntq = k.pair ? (k.kt + 1) / 2 : k.kt, kc = k.pair ? 1 : k.cin_src / 16;
    return (size_t)(k.cout / 32) * ntq * kc * 64 * 16;
}

// ---- kernel instantiations --------------------------------------------------------------------------------------------
//                                    CIN CINP COUT SI SO KS ST PD LPB MT NT INMODE        OUTMODE
constexpr auto v3b_pre = v3b::conv_k<3, 8, 64, 8, 8, 3, 1, 1, 1, 2, 2, v3::IN_LEAF3, v3::OUT_BIAS>;
constexpr auto v3b_r64a = v3b::conv_k<64, 64, 64, 8, 8, 3, 1, 1, 1, 2, 2, v3::IN_GNRELU, v3::OUT_BIAS>;
constexpr auto v3b_r64b = v3b::conv_k<64, 64, 64, 8, 8, 3, 1, 1, 1, 2, 2, v3::IN_GNRELU, v3::OUT_RESID>;
constexpr auto v3b_down = v3b::conv_k<64, 64, 128, 8, 4, 3, 2, 1, 1, 1, 1, v3::IN_PLAIN, v3::OUT_BIAS>;
constexpr auto v3b_r128a = v3b::conv_k<128, 128, 128, 4, 4, 3, 1, 1, 4, 1, 4, v3::IN_GNRELU, v3::OUT_BIAS>;
constexpr auto v3b_r128b = v3b::conv_k<128, 128, 128, 4, 4, 3, 1, 1, 4, 1, 4, v3::IN_GNRELU, v3::OUT_RESID>;
constexpr auto v3b_proj = v3b::conv_k<128, 128, 64, 4, 4, 1, 1, 0, 4, 1, 2, v3::IN_GATE, v3::OUT_BIAS>;
constexpr auto v3b_stem = v3b::conv_k<64, 64, 128, 4, 4, 3, 1, 1, 4, 1, 4, v3::IN_PLAIN, v3::OUT_BIAS>;
constexpr auto v3b_up = v3b::conv_k<128, 128, 256, 4, 4, 3, 1, 1, 4, 2, 2, v3::IN_GATE, v3::OUT_BIAS>;

template <int CINP, int COUT, int SI, int SO, int LPB_, int MT, int NT>
struct V3BLaunch {
    static constexpr int LPB = LPB_;
    static constexpr int threads = v3b::Shape<COUT, SO, LPB, MT, NT>::THREADS;
    static constexpr size_t lds = (size_t)(LPB * SI * SI * SI + 1) * CINP * 2;   // the leaves and the row of zeros
};
using LB_pre = V3BLaunch<8, 64, 8, 8, 1, 2, 2>;
using LB_r64 = V3BLaunch<64, 64, 8, 8, 1, 2, 2>;
using LB_down = V3BLaunch<64, 128, 8, 4, 1, 1, 1>;
using LB_r128 = V3BLaunch<128, 128, 4, 4, 4, 1, 4>;
using LB_proj = V3BLaunch<128, 64, 4, 4, 4, 1, 2>;
using LB_stem = V3BLaunch<64, 128, 4, 4, 4, 1, 4>;
using LB_up = V3BLaunch<128, 256, 4, 4, 4, 2, 2>;

int v3b_init_attrs(vqhip_vec3_codec* c)
{
    int rc = v3_set_lds(c, v3b_pre, LB_pre::lds);
    if (!rc) rc = v3_set_lds(c, v3b_r64a, LB_r64::lds);
    if (!rc) rc = v3_set_lds(c, v3b_r64b, LB_r64::lds);
    if (!rc) rc = v3_set_lds(c, v3b_down, LB_down::lds);
    if (!rc) rc = v3_set_lds(c, v3b_r128a, LB_r128::lds);
    if (!rc) rc = v3_set_lds(c, v3b_r128b, LB_r128::lds);
    if (!rc) rc = v3_set_lds(c, v3b_proj, LB_proj::lds);
    if (!rc) rc = v3_set_lds(c, v3b_stem, LB_stem::lds);
    if (!rc) rc = v3_set_lds(c, v3b_up, LB_up::lds);
    return rc;
}

// rebuild every bf16 fragment table from the fp32 fragments of the same conv (stream-ordered after whatever wrote those)
int v3b_refrag(vqhip_vec3_codec* c, hipStream_t s)
{
    for (const V3BConv& k : V3B_CONVS) {
        const unsigned blocks = (unsigned)((v3b_frag_bytes(k) / 16 + 255) / 256);
        hipLaunchKernelGGL(v3b::frag_bf16_k, dim3(blocks), dim3(256), 0, s, c->w[std::string(k.dev) + ".wf"], k.cout, k.cin_src, k.kt, k.pair,
                           reinterpret_cast<uint16_t*>(c->w[std::string(k.dev) + ".wb"]));
    }
    return v3_launch_check(c, "vec3 bf16 weight fragments");
}

// first switch to bf16: allocate the tables (10.2 MB), raise the LDS limits, build the fragments
int v3b_ensure(vqhip_vec3_codec* c)
{
    if (c->bf_ready) return VQHIP_OK;
    for (const V3BConv& k : V3B_CONVS) {
        const std::string name = std::string(k.dev) + ".wb";
        if (c->w.count(name)) continue;
        void* d = nullptr;
        HIPCHK(c, hipMalloc(&d, v3b_frag_bytes(k)));
        c->w[name] = static_cast<float*>(d);   // freed with the other tables by vqhip_vec3_destroy
    }
    if (int rc = v3b_init_attrs(c)) return rc;
    if (int rc = v3b_refrag(c, c->stream)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->bf_ready = true;
    return VQHIP_OK;
}

template <typename K, typename L>
void v3b_conv(K kernel, L, hipStream_t s, int64_t m, v3::ConvArgs a)
{
    a.n = m;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((m + L::LPB - 1) / L::LPB)), dim3(L::threads), L::lds, s, a);
}

int v3b_rb128(vqhip_vec3_codec* c, const std::string& p, float* x, float* h, float* stats, int64_t m, hipStream_t s)
{
    const unsigned nb = (unsigned)m;
    hipLaunchKernelGGL((v3::gn_stats_k<128, 64>), dim3(nb), dim3(256), 0, s, x, stats, m);
    v3::ConvArgs a = v3_args(x, c->w[p + ".c1.wb"], c->w[p + ".c1.b"], h);
    a.stats = stats, a.gamma = c->w[p + ".g1"], a.beta = c->w[p + ".b1"];
    v3b_conv(v3b_r128a, LB_r128{}, s, m, a);
    hipLaunchKernelGGL((v3::gn_stats_k<128, 64>), dim3(nb), dim3(256), 0, s, h, stats, m);
    a = v3_args(h, c->w[p + ".c2.wb"], c->w[p + ".c2.b"], x);
    a.stats = stats, a.gamma = c->w[p + ".g2"], a.beta = c->w[p + ".b2"], a.res = x;
    v3b_conv(v3b_r128b, LB_r128{}, s, m, a);
    return v3_launch_check(c, p.c_str());
}

// v3_encode_chunk with the bf16 convolutions; the same launches, debug names and helper kernels otherwise
int v3b_encode_chunk(vqhip_vec3_codec* c, const float* leaves, int64_t m, uint16_t* idx, hipStream_t s)
{
    if (int rc = v3_ensure_ws(c, m)) return rc;
    const V3Ws W = v3_ws(c);
    auto& w = c->w;
    const unsigned nb = (unsigned)m;
    int rc = VQHIP_OK;
    v3b_conv(v3b_pre, LB_pre{}, s, m, v3_args(leaves, w["e.pre.wb"], w["e.pre.b"], W.a8));
    if ((rc = v3_launch_check(c, "vec3 bf16 encoder.pre.0")) || (rc = v3_keep(c, "encoder.pre.0", W.a8, 64 * 512, m, s))) return rc;
    hipLaunchKernelGGL((v3::gn_stats_k<64, 512>), dim3(nb), dim3(256), 0, s, W.a8, W.stats, m);
    hipLaunchKernelGGL((v3::gn_relu_k<64, 512>), dim3(v3_ew_grid(m * 64 * 512)), dim3(256), 0, s, W.a8, W.stats, w["e.pre.g"],
                       w["e.pre.bt"], m);
    if ((rc = v3_launch_check(c, "vec3 bf16 encoder.pre.1")) || (rc = v3_keep(c, "encoder.pre.2", W.a8, 64 * 512, m, s))) return rc;
    hipLaunchKernelGGL((v3::gn_stats_k<64, 512>), dim3(nb), dim3(256), 0, s, W.a8, W.stats, m);
    v3::ConvArgs a = v3_args(W.a8, w["e.rb64.c1.wb"], w["e.rb64.c1.b"], W.b8);
    a.stats = W.stats, a.gamma = w["e.rb64.g1"], a.beta = w["e.rb64.b1"];
    v3b_conv(v3b_r64a, LB_r64{}, s, m, a);
    hipLaunchKernelGGL((v3::gn_stats_k<64, 512>), dim3(nb), dim3(256), 0, s, W.b8, W.stats, m);
    a = v3_args(W.b8, w["e.rb64.c2.wb"], w["e.rb64.c2.b"], W.a8);
    a.stats = W.stats, a.gamma = w["e.rb64.g2"], a.beta = w["e.rb64.b2"], a.res = W.a8;
    v3b_conv(v3b_r64b, LB_r64{}, s, m, a);
    if ((rc = v3_launch_check(c, "vec3 bf16 encoder.pre.3")) || (rc = v3_keep(c, "encoder.pre", W.a8, 64 * 512, m, s))) return rc;
    v3b_conv(v3b_down, LB_down{}, s, m, v3_args(W.a8, w["e.down.wb"], w["e.down.b"], W.p));
    if ((rc = v3_launch_check(c, "vec3 bf16 encoder.down1")) || (rc = v3_keep(c, "encoder.down1", W.p, 128 * 64, m, s))) return rc;
    if ((rc = v3b_rb128(c, "e.rb0", W.p, W.q, W.stats, m, s)) || (rc = v3_keep(c, "encoder.res_stack.0", W.p, 128 * 64, m, s))) return rc;
    if ((rc = v3b_rb128(c, "e.rb1", W.p, W.q, W.stats, m, s)) || (rc = v3_keep(c, "encoder.res_stack.1", W.p, 128 * 64, m, s))) return rc;
    hipLaunchKernelGGL(v3::se_k, dim3(nb), dim3(128), 0, s, W.p, w["e.fc1"], w["e.fc2"], W.gate, m);
    a = v3_args(W.p, w["e.proj.wb"], w["e.proj.b"], W.z);
    a.gate = W.gate;
    v3b_conv(v3b_proj, LB_proj{}, s, m, a);
    if ((rc = v3_launch_check(c, "vec3 bf16 encoder.proj")) || (rc = v3_keep(c, "encoder.proj", W.z, 64 * 64, m, s))) return rc;
    hipLaunchKernelGGL(v3::vq_k, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, W.z, w["cb.f"], w["cb.ee"], c->k_pad, idx, m);
    return v3_launch_check(c, "vec3 quantizer");
}

// gather to decoder.up_conv with the bf16 convolutions; leaves W.u for the tail
int v3b_decode_body(vqhip_vec3_codec* c, const uint16_t* idx, int64_t m, hipStream_t s)
{
    const V3Ws W = v3_ws(c);
    auto& w = c->w;
    const unsigned nb = (unsigned)m;
    int rc = VQHIP_OK;
    hipLaunchKernelGGL(v3::gather_k, dim3(v3_ew_grid(m * 4096)), dim3(256), 0, s, idx, w["cb"], c->k_codes, W.z, m);
    v3b_conv(v3b_stem, LB_stem{}, s, m, v3_args(W.z, w["d.stem.wb"], w["d.stem.b"], W.p));
    if ((rc = v3_launch_check(c, "vec3 bf16 decoder.stem.0")) || (rc = v3_keep(c, "decoder.stem.0", W.p, 128 * 64, m, s))) return rc;
    hipLaunchKernelGGL((v3::gn_stats_k<128, 64>), dim3(nb), dim3(256), 0, s, W.p, W.stats, m);
    hipLaunchKernelGGL((v3::gn_relu_k<128, 64>), dim3(v3_ew_grid(m * 128 * 64)), dim3(256), 0, s, W.p, W.stats, w["d.stem.g"],
                       w["d.stem.bt"], m);
    if ((rc = v3_launch_check(c, "vec3 bf16 decoder.stem")) || (rc = v3_keep(c, "decoder.stem", W.p, 128 * 64, m, s))) return rc;
    if ((rc = v3b_rb128(c, "d.rb0", W.p, W.q, W.stats, m, s)) || (rc = v3_keep(c, "decoder.res_stack.0", W.p, 128 * 64, m, s))) return rc;
    if ((rc = v3b_rb128(c, "d.rb1", W.p, W.q, W.stats, m, s)) || (rc = v3_keep(c, "decoder.res_stack.1", W.p, 128 * 64, m, s))) return rc;
    hipLaunchKernelGGL(v3::se_k, dim3(nb), dim3(128), 0, s, W.p, w["d.fc1"], w["d.fc2"], W.gate, m);
    v3::ConvArgs a = v3_args(W.p, w["d.up.wb"], w["d.up.b"], W.u);
    a.gate = W.gate;
    v3b_conv(v3b_up, LB_up{}, s, m, a);
    if ((rc = v3_launch_check(c, "vec3 bf16 decoder.up_conv"))) return rc;
    return v3_keep(c, "decoder.up_conv", W.u, 256 * 64, m, s);
}

int v3b_decode_chunk(vqhip_vec3_codec* c, const uint16_t* idx, int64_t m, float* out, hipStream_t s)
{
    if (int rc = v3_ensure_ws(c, m)) return rc;
    if (int rc = v3b_decode_body(c, idx, m, s)) return rc;
    hipLaunchKernelGGL(v3::final_k, dim3((unsigned)m), dim3(512), V3_LDS_FINAL, s, v3_ws(c).u, c->w["d.final.w"], c->w["d.final.b"], out, m);
    return v3_launch_check(c, "vec3 decoder.final");
}

}  // namespace

extern "C" {

int vqhip_vec3_set_precision(vqhip_vec3_codec* c, int mode)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (mode != VQHIP_VEC3_PRECISION_FP32 && mode != VQHIP_VEC3_PRECISION_BF16)
        return v3_fail(c, VQHIP_ERR_INVALID, "vec3 set_precision: mode " + std::to_string(mode) + " is neither VQHIP_VEC3_PRECISION_FP32 (0) nor VQHIP_VEC3_PRECISION_BF16 (1)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (mode == VQHIP_VEC3_PRECISION_BF16)
        if (int rc = v3b_ensure(c)) return rc;
    c->precision = mode;
    return VQHIP_OK;
}

int vqhip_vec3_get_precision(const vqhip_vec3_codec* c, int* mode)
{
    if (!c || !mode) return VQHIP_ERR_INVALID;
    *mode = c->precision;
    return VQHIP_OK;
}

}  // extern "C"
