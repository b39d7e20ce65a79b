// vq_train_full.inc — host side of the full training step (SURVEY.md §8 f-2, stage 2), included at the end of vq_runtime.hip.
//
// State: a flat fp32 parameter vector P (the 44 trainable tensors in the reference's parameter order, 995 905 values), AdamW
// moments M and V, and the EMA codebook state of vqhip_train_begin.  Every weight-derived table the kernels read (MFMA
// fragments of the forward and of the data-gradient convolutions) is rebuilt ON THE DEVICE from P after each optimizer step.
// One step on a rank:   forward (all activations kept) -> loss -> backward into a flat gradient vector G (+ the VQ statistics)
//                       [host: all-reduce G and the statistics over RCCL]  -> AdamW on P, EMA on the codebook, refragment.

namespace {

const ActSpec kTrainActs[] = {
    // forward tensors the inference workspace does not hold
    {"t_z", 128, 64},    {"t_q", 128, 64},   {"t_upA", 128, 64}, {"t_upB", 128, 64}, {"t_ps", 32, 512}, {"t_pre", 1, 512}, {"t_recon", 1, 512},
    {"t_egate", 0, 32},  {"t_dgate", 0, 64},
    // saved statistics (encoder: written by the forward's fused statistics; decoder: recomputed in the contract's order from the stored activations)
    {"ts_gn0.mean", 0, 4},   {"ts_gn0.rstd", 0, 4},   {"ts_r16g1.mean", 0, 8}, {"ts_r16g1.rstd", 0, 8}, {"ts_r16g2.mean", 0, 8}, {"ts_r16g2.rstd", 0, 8},
    {"ts_r32g1.mean", 0, 8}, {"ts_r32g1.rstd", 0, 8}, {"ts_r32g2.mean", 0, 8}, {"ts_r32g2.rstd", 0, 8}, {"ts_ecsum", 0, 32},
    {"ts_dgn.mean", 0, 8},   {"ts_dgn.rstd", 0, 8},   {"ts_r64g1.mean", 0, 8}, {"ts_r64g1.rstd", 0, 8}, {"ts_r64g2.mean", 0, 8}, {"ts_r64g2.rstd", 0, 8},
    {"ts_dcsum", 0, 64},
    // gradients
    {"g_pre", 1, 512},   {"g_pre4", 1, 512},  {"g_ps", 32, 512},  {"g_upA", 128, 64}, {"g_upB", 128, 64}, {"g64a", 64, 64}, {"g64b", 64, 64}, {"g64c", 64, 64}, {"g64d", 64, 64}, {"g_q", 128, 64},
    {"g32a", 32, 64},    {"g32b", 32, 64},   {"g32c", 32, 64},   {"g32d", 32, 64},  {"g16a", 16, 512}, {"g16b", 16, 512}, {"g16c", 16, 512}, {"g16d", 16, 512},
    {"gs_1", 0, 64},     {"gs_2", 0, 64},    // GroupNorm-backward partial sums per (position range <= 8, group, leaf)
    {"gs_c1", 0, 8},     {"gs_c2", 0, 8},    // ... combined over the ranges
};

int ensure_train_workspace(vqhip_codec* c, int64_t n_leaves)
{
    const int64_t tiles = (n_leaves + 31) / 32;
    if (tiles <= c->ft_tiles) return VQHIP_OK;
    auto bytes = [&](const ActSpec& a) { return (((a.C ? (size_t)a.C * a.NP : (size_t)a.NP) * sizeof(float) * 32 * tiles) + 255) / 256 * 256; };
    size_t total = 0;
    for (const ActSpec& a : kTrainActs) total += bytes(a);
    if (int rc = ensure(c, c->ft_ws, total, [](hipError_t e) { return std::string("training workspace hipMalloc failed: ") + hipGetErrorString(e); })) {
        if (!c->ft_ws) c->ft_tiles = 0;   // (a failed synchronise leaves the old block and its layout)
        return rc;
    }
    size_t off = 0;
    for (const ActSpec& a : kTrainActs) {
        c->act[a.name] = reinterpret_cast<float*>(c->ft_ws + off);
        c->act_shape[a.name] = {a.C, a.NP};
        off += bytes(a);
    }
    c->ft_tiles = tiles;
    return VQHIP_OK;
}

float* param(vqhip_codec* c, const char* name) { return c->ft_P + c->p_off.at(name).first; }

// device buffers of weight-derived tables; created on first use with the right size
int table(vqhip_codec* c, const char* name, size_t floats, float** out)
{
    auto it = c->dw.find(name);
    if (it == c->dw.end()) {
        float* d = nullptr;
        HIPCHK(c, hipMalloc(&d, floats * sizeof(float)));
        c->dw[name] = d;
        *out = d;
    } else {
        *out = it->second;
    }
    return VQHIP_OK;
}

// Rebuild every table that derives from P (forward fragments shared with the inference kernels, training-only forward
// fragments, data-gradient fragments).  The folded decoder tail / stem table / folded VQ search of the inference path are
// refreshed lazily (tables_stale) from a host copy, see vqhip_fulltrain_commit.
int refrag_all(vqhip_codec* c, hipStream_t s)
{
    int rc;
    float* d;
    c->bf_stale = true;   // the bf16 decode mode packs its fragments from "r64c1.w16" / "r64c2.w16" again at its next call (ensure_dec_bf16_frags)
    c->bf_enc_stale = true;   // ... and the bf16 encode mode its own from "r16c1.w" / "r16c2.w" (ensure_enc_bf16_frags)
    // The job list is built once (the tables are allocated on the first pass and never move, the parameters live in ft_P) and kept on the
    // device; every later call is ONE launch of refrag_multi_k.
    if (c->ft_refrag_jobs && c->ft_refrag_P != c->ft_P) {   // the cached table bakes in addresses inside the parameter block: rebuild if that moved
        HIPCHK(c, hipDeviceSynchronize());
        c->ft_refrag_jobs.reset();
        c->ft_refrag_n = c->ft_refrag_wgs = 0;
    }
    if (c->ft_refrag_jobs) {
        hipLaunchKernelGGL(refrag_multi_k, dim3(c->ft_refrag_wgs), dim3(256), 0, s, (const RefragJob*)c->ft_refrag_jobs.get(), c->ft_refrag_n);
        HIPCHK(c, hipGetLastError());
        return VQHIP_OK;
    }
    std::vector<RefragJob> jobs;
    int wgs = 0;
    auto job = [&](int kind, const float* src, float* dst, int total, float scale, int a = 0, int b = 0, int cc = 0, int dd = 0, int e = 0, int f = 0) {
        jobs.push_back(RefragJob{src, dst, kind, a, b, cc, dd, e, f, scale, total, wgs});
        wgs += (total + 255) / 256;
    };
#define T(name, n) \
    if ((rc = table(c, name, n, &d))) return rc;
#define F32(dst, src, COUT, CIN, KT, IC, row0, tr, scale)                                                                       \
    T(dst, (size_t)(KT) * ((CIN) / 8) * ((COUT) / 32) * 256)                                                                     \
    job(1, param(c, src), d, (int)((KT) * ((CIN) / 8) * ((COUT) / 32) * 256), scale, COUT, CIN, KT, IC, row0, tr);
#define DF(dst, src, COUT, row0) T(dst, COUT) job(5, param(c, src), d, COUT, 1.0f, row0);
#define CP(dst, src)                              \
    T(dst, (size_t)c->p_off.at(src).second)       \
    job(0, param(c, src), d, (int)c->p_off.at(src).second, 1.0f);
#define R16(dst, src, tr, scale) T(dst, 27 * 256) job(2, param(c, src), d, 27 * 256, scale, 27, tr);
#define R16G(dst, src, COUT, CIN, KT, tr, scale) T(dst, (size_t)(KT) * ((CIN) / 16) * ((COUT) / 16) * 256) job(3, param(c, src), d, (KT) * ((CIN) / 16) * ((COUT) / 16) * 256, scale, COUT, CIN, KT, tr);
    // ---- forward tables (names of load_weights) ----
    T("e0.w", 9 * 64) job(4, param(c, "encoder.pre.0.weight"), d, 9 * 64, 1.0f);
    CP("e0.b", "encoder.pre.0.bias") CP("eg0.w", "encoder.pre.1.weight") CP("eg0.b", "encoder.pre.1.bias")
    CP("r16g1.w", "encoder.pre.3.gn1.weight") CP("r16g1.b", "encoder.pre.3.gn1.bias") CP("r16c1.b", "encoder.pre.3.conv1.bias")
    CP("r16g2.w", "encoder.pre.3.gn2.weight") CP("r16g2.b", "encoder.pre.3.gn2.bias") CP("r16c2.b", "encoder.pre.3.conv2.bias")
    R16("r16c1.w", "encoder.pre.3.conv1.weight", 0, 1.0f)
    R16("r16c2.w", "encoder.pre.3.conv2.weight", 0, 1.0f)
    F32("ed.w", "encoder.down.weight", 32, 16, 64, 16, 0, 0, 1.0f) DF("ed.b", "encoder.down.bias", 32, 0)
    CP("r32g1.w", "encoder.res_stack.0.gn1.weight") CP("r32g1.b", "encoder.res_stack.0.gn1.bias")
    CP("r32g2.w", "encoder.res_stack.0.gn2.weight") CP("r32g2.b", "encoder.res_stack.0.gn2.bias")
    F32("r32c1.w", "encoder.res_stack.0.conv1.weight", 32, 32, 27, 32, 0, 0, 1.0f) DF("r32c1.b", "encoder.res_stack.0.conv1.bias", 32, 0)
    F32("r32c2.w", "encoder.res_stack.0.conv2.weight", 32, 32, 27, 32, 0, 0, 1.0f) DF("r32c2.b", "encoder.res_stack.0.conv2.bias", 32, 0)
    CP("efc0", "encoder.attn.fc.0.weight") CP("efc2", "encoder.attn.fc.2.weight")
    F32("tr.wproj", "encoder.proj.weight", 128, 32, 1, 32, 0, 0, 1.0f) DF("tr.bproj", "encoder.proj.bias", 128, 0)
    CP("ds.w", "decoder.stem.0.weight") CP("ds.b", "decoder.stem.0.bias") CP("dg0.w", "decoder.stem.1.weight") CP("dg0.b", "decoder.stem.1.bias")
    CP("r64g1.w", "decoder.res_stack.0.gn1.weight") CP("r64g1.b", "decoder.res_stack.0.gn1.bias")
    CP("r64g2.w", "decoder.res_stack.0.gn2.weight") CP("r64g2.b", "decoder.res_stack.0.gn2.bias")
    F32("r64c1.w", "decoder.res_stack.0.conv1.weight", 64, 64, 27, 64, 0, 0, 1.0f) DF("r64c1.b", "decoder.res_stack.0.conv1.bias", 64, 0)
    F32("r64c2.w", "decoder.res_stack.0.conv2.weight", 64, 64, 27, 64, 0, 0, 1.0f) DF("r64c2.b", "decoder.res_stack.0.conv2.bias", 64, 0)
    R16G("r64c1.w16", "decoder.res_stack.0.conv1.weight", 64, 64, 27, 0, 1.0f)
    R16G("r64c2.w16", "decoder.res_stack.0.conv2.weight", 64, 64, 27, 0, 1.0f)
    R16G("r32c1.w16", "encoder.res_stack.0.conv1.weight", 32, 32, 27, 0, 1.0f)
    R16G("r32c2.w16", "encoder.res_stack.0.conv2.weight", 32, 32, 27, 0, 1.0f)
    R16G("ed.w16", "encoder.down.weight", 32, 16, 64, 0, 1.0f)
    CP("r32c1.braw", "encoder.res_stack.0.conv1.bias") CP("r32c2.braw", "encoder.res_stack.0.conv2.bias") CP("ed.braw", "encoder.down.bias")
    CP("r64c1.braw", "decoder.res_stack.0.conv1.bias") CP("r64c2.braw", "decoder.res_stack.0.conv2.bias")
    CP("dfc0", "decoder.attn.fc.0.weight") CP("dfc2", "decoder.attn.fc.2.weight")
    // ---- training-only forward tables: real stem conv, unfolded tail ----
    F32("ft.stem.w", "decoder.stem.0.weight", 64, 128, 27, 128, 0, 0, 1.0f) DF("ft.stem.b", "decoder.stem.0.bias", 64, 0)
    F32("ft.upA.w", "decoder.up_conv.weight", 128, 64, 27, 64, 0, 0, 1.0f) DF("ft.upA.b", "decoder.up_conv.bias", 128, 0)
    F32("ft.upB.w", "decoder.up_conv.weight", 128, 64, 27, 64, 128, 0, 1.0f) DF("ft.upB.b", "decoder.up_conv.bias", 128, 128)
    // ---- data-gradient tables (transposed, taps flipped; the 0.1 residual scale of conv2 is folded in) ----
    F32("bt.upA.w", "decoder.up_conv.weight", 64, 128, 27, 64, 0, 1, 1.0f)
    F32("bt.upB.w", "decoder.up_conv.weight", 64, 128, 27, 64, 128, 1, 1.0f)
    R16G("bt.r64c2.w16", "decoder.res_stack.0.conv2.weight", 64, 64, 27, 1, 0.1f)
    R16G("bt.r64c1.w16", "decoder.res_stack.0.conv1.weight", 64, 64, 27, 1, 1.0f)
    F32("bt.stem.w", "decoder.stem.0.weight", 128, 64, 27, 128, 0, 1, 1.0f)
    F32("bt.proj.w", "encoder.proj.weight", 32, 128, 1, 32, 0, 1, 1.0f)
    R16G("bt.r32c2.w16", "encoder.res_stack.0.conv2.weight", 32, 32, 27, 1, 0.1f)
    R16G("bt.r32c1.w16", "encoder.res_stack.0.conv1.weight", 32, 32, 27, 1, 1.0f)
    R16("bt.r16c2.w", "encoder.pre.3.conv2.weight", 1, 0.1f)
    R16("bt.r16c1.w", "encoder.pre.3.conv1.weight", 1, 1.0f)
    T("bt.down.w", 64 * 2 * 256) job(6, param(c, "encoder.down.weight"), d, 64 * 2 * 256, 1.0f);
    T("bt.zero128", 128) job(7, c->ft_P, d, 128, 0.0f);
#undef T
#undef F32
#undef DF
#undef CP
#undef R16
#undef R16G
    // the list is published (pointer, count, grid) only once it is on the device: a failure on the way leaves the handle without one,
    // and the next step builds it again
    DevBuf<unsigned char> djobs;
    if ((rc = ensure(c, djobs, jobs.size() * sizeof(RefragJob), "the refrag job list"))) return rc;
    hipError_t je = hipMemcpyAsync(djobs, jobs.data(), jobs.size() * sizeof(RefragJob), hipMemcpyHostToDevice, s);
    if (je == hipSuccess) je = hipStreamSynchronize(s);   // (jobs is a local)
    if (je != hipSuccess) return fail(c, VQHIP_ERR_DEVICE, std::string("refrag job list upload: ") + hipGetErrorString(je));
    c->ft_refrag_jobs = std::move(djobs);
    c->ft_refrag_n = (int)jobs.size(), c->ft_refrag_wgs = wgs, c->ft_refrag_P = c->ft_P;
    hipLaunchKernelGGL(refrag_multi_k, dim3(wgs), dim3(256), 0, s, (const RefragJob*)c->ft_refrag_jobs.get(), c->ft_refrag_n);
    HIPCHK(c, hipGetLastError());
    return VQHIP_OK;
}

// the training forward / data-gradient convolutions of the decoder (configurations: vq_kernels.h; 2-tile workgroups, no fused statistics)
constexpr auto kTrainDecConvs = conv_kernels(TrainDecConvs{});

// folded tail: device tables + static schedules (created once)
int ensure_tail_tables(vqhip_codec* c)
{
    if (c->dw.count("w.tail")) return VQHIP_OK;
    float* d = nullptr;
    int rc;
    if ((rc = table(c, "ft.tail.w", (size_t)224 * 8192, &d))) return rc;
    if ((rc = table(c, "ft.tailT.w", (size_t)224 * 8192, &d))) return rc;
    if ((rc = table(c, "ft.tail.b", 512, &d))) return rc;
    if ((rc = table(c, "ft.tail.G", (size_t)2 * 27 * 8 * 27 * 64, &d))) return rc;     // doubles
    if ((rc = table(c, "ft.tail.dG", (size_t)2 * 27 * 8 * 27 * 64, &d))) return rc;
    if ((rc = table(c, "ft.tail.Bg", 2 * 216, &d))) return rc;
    if ((rc = table(c, "ft.tail.dBg", 2 * 216, &d))) return rc;
    if ((rc = table(c, "ft.tail.dWc", (size_t)224 * 128 * 64, &d))) return rc;
    if ((rc = table(c, "ft.tail.dbc", 512, &d))) return rc;
    // data-gradient schedule: output = input position p (64), "taps" = the slabs d whose receptive field holds p; x = slab (the conv's
    // input position), y = forward step = transposed-fragment index of (d, p)
    std::vector<int> st;
    for (int p = 0; p < 64; ++p) {
        const size_t first = st.size();
        for (int d = 0; d < 4; ++d) {
            if (p < tail_step_p0(d) || p >= tail_step_p0(d) + tail_step_count(d)) continue;
            st.insert(st.end(), {d, tail_step_base(d) + p - tail_step_p0(d), p, 1 << 8});
        }
        st[first + 3] |= 1;
        st[st.size() - 1] |= 2;
    }
    if ((rc = upload_steps(c, "steps.tailT", st))) return rc;
    // weight-gradient pairs: "tap" q = forward step (d, p): one (input position p, output "position" = slab d) pair each
    std::vector<int> pairs, start;
    for (int d = 0; d < 4; ++d)
        for (int k = 0; k < tail_step_count(d); ++k) {
            start.push_back((int)pairs.size() / 2);
            pairs.push_back(tail_step_p0(d) + k);
            pairs.push_back(d);
        }
    start.push_back((int)pairs.size() / 2);
    while (pairs.size() % 4) pairs.push_back(0);
    while (start.size() % 4) start.push_back(start.back());
    if ((rc = upload_i(c, "w.tail", pairs))) return rc;
    if ((rc = upload_i(c, "w.tail.start", start))) return rc;
    return VQHIP_OK;
}

// "`to` may not pass this point before `from` got here": one event of the per-step pool (c->ft_ev, rewound by the step's entry point)
int stream_link(vqhip_codec* c, hipStream_t from, hipStream_t to)
{
    if (from == to) return VQHIP_OK;
    if (c->ft_ev_next == c->ft_ev.size()) {
        hipEvent_t e = nullptr;
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->ft_ev.push_back(e);
    }
    hipEvent_t e = c->ft_ev[c->ft_ev_next++];
    HIPCHK(c, hipEventRecord(e, from));
    HIPCHK(c, hipStreamWaitEvent(to, e, 0));
    return VQHIP_OK;
}
// the second stream of the training step (weight / bias gradients, statistics, the tail fold), or `s` itself when it is switched off
int side_stream(vqhip_codec* c, hipStream_t s, hipStream_t& ws)
{
    ws = s;
    if (!c->train_side_stream) return VQHIP_OK;
    if (!c->ft_side) {
        // VQHIP_TRAIN_SIDE_PRIO=high|low: the weight-gradient stream's queue priority against the data-gradient stream (the caller's)
        int lo = 0, hi = 0;
        if (c->train_side_prio && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi)
            HIPCHK(c, hipStreamCreateWithPriority(&c->ft_side, hipStreamNonBlocking, c->train_side_prio > 0 ? hi : lo));
        else HIPCHK(c, hipStreamCreateWithFlags(&c->ft_side, hipStreamNonBlocking));
    }
    ws = c->ft_side;
    if (c->train_red_stream && !c->ft_red) {
        // Two reduction streams, chosen per step by the batch (Bwd::rs).  Streams of one priority share a small pool of hardware queues: a
        // plain third stream landed on the weight-gradient stream's queue, where its 40 launches lengthened that queue by 0.45 ms at 2048
        // leaves per rank (profiles/r06_train_step_timeline_2048_three_streams_one_queue.txt: 4.50 ms against 4.28 without it) — while at
        // 8192 leaves exactly that arrangement is the fastest (13.25 ms against 13.67).  A stream of ANOTHER priority gets a queue of its
        // own: 4.13-4.16 ms at 2048 leaves (…_own_queue.txt), but 15.5 ms at 8192.  So: own queue (high priority: the launches are a few
        // microseconds each) for small batches, the shared queue for large ones.  VQHIP_TRAIN_RED_PRIO=own|normal forces one of them.
        // VQHIP_TRAIN_RED_QUEUE=mask (default): a stream created with a CU mask owns its HSA queue (the mask is a queue property) — a full mask
        // gives a dedicated queue at NORMAL priority; =prio: a high-priority stream (round 6's first attempt: a dedicated queue too, but
        // erratic — 4.87 ms against 2.70 at 1024 leaves per rank, 9.4 against 7.2 at 4096, equal at 2048)
        int lo = 0, hi = 0;
        if (!c->train_red_queue_mask && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi) {
            HIPCHK(c, hipStreamCreateWithPriority(&c->ft_red, hipStreamNonBlocking, hi));
        } else {
            std::vector<uint32_t> mask((size_t)(c->n_cus_device + 31) / 32, 0xffffffffu);   // the device's own count: VQHIP_CUS masks nothing off
            if (c->n_cus_device % 32) mask.back() = (1u << (c->n_cus_device % 32)) - 1u;
            if (hipExtStreamCreateWithCUMask(&c->ft_red, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
                (void)hipGetLastError();
                HIPCHK(c, hipStreamCreateWithFlags(&c->ft_red, hipStreamNonBlocking));
            }
        }
        HIPCHK(c, hipStreamCreateWithFlags(&c->ft_red_shared, hipStreamNonBlocking));
    }
    return VQHIP_OK;
}

// fragments of the folded tail from the live parameters
int fulltrain_fold_tail(vqhip_codec* c, Launcher& L, hipStream_t s)
{
    int rc = ensure_tail_tables(c);
    if (rc) return rc;
    auto& w = c->dw;
    double* G = reinterpret_cast<double*>(w["ft.tail.G"]);
    double* Bg = reinterpret_cast<double*>(w["ft.tail.Bg"]);
    L.run_on(s, "ft_tail_fold", [&] {
        hipLaunchKernelGGL(tail_fold_g_k, dim3((27 * 8 * 27 * 64 + 255) / 256), dim3(256), 0, s, param(c, "decoder.up_conv.weight"), param(c, "decoder.up_conv.bias"),
                           param(c, "decoder.final.weight"), G, Bg);
        hipLaunchKernelGGL(tail_fold_frags_k, dim3((2 * 224 * 8192 + 512 + 255) / 256), dim3(256), 0, s, G, Bg, param(c, "decoder.final.bias"), w["ft.tail.w"],
                           w["ft.tailT.w"], w["ft.tail.b"]);
    });
    return L.rc;
}

// training-mode forward; keeps every activation.  Returns with recon / pre / up / ... in the workspaces.
int fulltrain_forward(vqhip_codec* c, const float* d_leaves, int64_t n, hipStream_t s, float* d_aux = nullptr, bool* ema_done = nullptr)
{
    int rc = ensure_train_workspace(c, n);
    if (rc) return rc;
    if ((rc = ensure(c, c->tr_z, (size_t)n * 64 * 128, "the training latents"))) return rc;
    if ((rc = ensure(c, c->tr_idx, (size_t)n * 64, "the training indices"))) return rc;
    if ((rc = ensure_workspace(c, n))) return rc;
    // The folded tail depends on the parameters only: it is rebuilt on the second stream while the encoder runs (0.08 ms off the chain).
    c->ft_ev_next = 0;   // (a step starts here: rewind the event pool)
    hipStream_t ws = s;
    if ((rc = side_stream(c, s, ws))) return rc;
    hipEvent_t fold_done = nullptr;
    if (c->train_folded_tail && ws != s) {
        Launcher Ls{c, s, n};
        if ((rc = stream_link(c, s, ws)) || (rc = fulltrain_fold_tail(c, Ls, ws))) return rc;
        // (its own event: the chain waits for the fold only, not for what follows it on the side stream)
        if (c->ft_ev_next == c->ft_ev.size()) {
            hipEvent_t e = nullptr;
            HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            c->ft_ev.push_back(e);
        }
        fold_done = c->ft_ev[c->ft_ev_next++];
        HIPCHK(c, hipEventRecord(fold_done, ws));
    }
    // encoder + latent (flat rows, and the L4 layout in t_z) + assignment against the live codebook
    if ((rc = encode_chunk(c, d_leaves, n, c->tr_idx, s, c->tr_z, VQHIP_PRECISION_FP32, c->act["t_z"]))) return rc;
    const int nt = (int)((n + 31) / 32);
    auto& a = c->act;
    auto& w = c->dw;
    Launcher L{c, s, n};
    if (ema_done) *ema_done = false;
    c->ft_egate_early = false;
    if (ws != s && c->train_ema_early) {
        // ... and the encoder attention's gates for the backward pass (the projection's weight gradient, on that stream too): 12 us here,
        // 127 us between the contended kernels of the data-gradient chain
        if ((rc = stream_link(c, s, ws))) return rc;
        L.run_on(ws, "bt_egate", [&] { hipLaunchKernelGGL(se_gate_k<32>, dim3(nt), dim3(64), 0, ws, a["ts_ecsum"], w["efc0"], w["efc2"], a["t_egate"]); });
        c->ft_egate_early = true;
    }
    if (d_aux && ws != s && c->train_ema_early) {
        // Round 6: the codebook statistics of this batch need the latent rows and the assignment only — they start here on the side stream,
        // which is idle until the backward pass, instead of at the head of the weight-gradient queue (0.2 ms of its 2.8 ms at 2048 leaves)
        const int64_t rows = n * 64;
        const int n_seg = (int)((rows + VQ_SEG_ROWS - 1) / VQ_SEG_ROWS);
        if ((rc = ensure(c, c->tr_part, ema_scratch_bytes(n_seg), "the codebook statistics partials"))) return rc;
        L.run_on(ws, "ft_vq_stats", [&] { launch_vq_ema(c, ws, c->tr_z, c->tr_idx, rows, n_seg, d_aux); });
        if (ema_done) *ema_done = true;
    }
    // (the statistics of the encoder's GroupNorms / attention the backward pass needs were written by the forward kernels themselves
    // into ts_gn0 / ts_r16g1 / ts_r16g2 / ts_r32g1 / ts_r32g2 / ts_ecsum: enc_stats_of() in vq_runtime.hip)
    const int g2 = (nt + 1) / 2;
    const int4* k3 = (const int4*)w["steps.k3s1_4"];
    const int nk3 = c->nsteps["steps.k3s1_4"];
    const int* g64 = reinterpret_cast<const int*>(w["steps.k3s1_4.grp"]);   // position-split launches (64 output positions)
    const int ps64 = split_factor(g2, 1, 32, 1024);
    const int g4 = (nt + 3) / 4, ps128 = split_factor(g4, 1, 32, 512);
    const int gh = (2 * nt + 7) / 8, psr = split_factor(gh, 1, 16, 512);   // conv_rows16_k: 8 half tiles per workgroup, 16 output rows
    const int4* r3 = (const int4*)w["steps.rows_k3_4"];
    const int* gr16 = reinterpret_cast<const int*>(w["steps.rows_k3_4.grp"]);
    L.run("ft_gather_q", [&] { hipLaunchKernelGGL(gather_codes_k, dim3(std::min(nt * 256, 65536)), dim3(256), 0, s, c->tr_idx, w["cb"], a["t_q"], n, nt); });
    if (c->train_stem_lut) {
        // the stem only ever sees the 256 codebook rows: (tap, code) table from the live weights and codebook (a 57 M-MAC GEMM on the
        // matrix pipe), then table look-ups like inference (stem_lut_k) — instead of 8.2 M MAC per leaf; t_q above still feeds the
        // backward pass (weight gradient, straight-through)
        float* lut = nullptr;
        if (int rc = table(c, "ft.stem.lut", (size_t)27 * 256 * 64, &lut)) return rc;
        L.run("ft_stem_lut", [&] { hipLaunchKernelGGL(build_stem_lut_mfma_k, dim3(27 * 16), dim3(64), 0, s, w["ft.stem.w"], w["cb"], lut); });
        L.run("ft_stem", [&] {
            hipLaunchKernelGGL(stem_lut_k, dim3(2 * nt, split_factor(2 * nt, 2, 16, 2048)), dim3(256), 0, s, c->tr_idx, lut, param(c, "decoder.stem.0.bias"), a["d_ystem"],
                               (float*)nullptr, (float*)nullptr, k3, nk3, n, nt, g64, (double*)nullptr, (double*)nullptr);
        });
    } else {
        ConvArgs A{};
        A.in = a["t_q"], A.out = a["d_ystem"], A.wfrag = w["ft.stem.w"], A.bias_frag = w["ft.stem.b"], A.n_tiles = nt, A.n_steps = nk3, A.n_taps = 27, A.grp_start = g64;
        L.run("ft_stem", [&] { launch_mfma32<TrainStem>(s, A, k3, nt, ps128); });
    }
    L.run("ft_stats_ystem", [&] { hipLaunchKernelGGL((gn_stats_seq_k<64, 64, 8>), dim3(nt), dim3(512), 0, s, a["d_ystem"], a["ts_dgn.mean"], a["ts_dgn.rstd"]); });
    L.run("ft_gn_relu_d2", [&] {
        hipLaunchKernelGGL((ew_gn_relu_k<64, 64, 8>), dim3(nt, 8), dim3(256), 0, s, a["d_ystem"], a["d_d2"], a["ts_dgn.mean"], a["ts_dgn.rstd"], w["dg0.w"], w["dg0.b"]);
    });
    L.run("ft_stats_d2", [&] { hipLaunchKernelGGL((gn_stats_seq_k<64, 64, 8>), dim3(nt), dim3(512), 0, s, a["d_d2"], a["ts_r64g1.mean"], a["ts_r64g1.rstd"]); });
    {
        ConvArgs A{};
        A.in = a["d_d2"], A.out = a["d_y4"], A.wfrag = w["r64c1.w16"], A.bias_frag = w["r64c1.braw"];
        A.in_mean = a["ts_r64g1.mean"], A.in_rstd = a["ts_r64g1.rstd"], A.in_gamma = w["r64g1.w"], A.in_beta = w["r64g1.b"], A.n_tiles = nt;
        A.n_steps = c->nsteps["steps.rows_k3_4"], A.n_taps = 27, A.grp_start = gr16;
        const bool q4r = c->train_r64_quarters && gh * psr * 4 <= 1024;   // up to 2048 leaves
        L.run("ft_res64_conv1", [&] {
            if (q4r) launch_rows<TrainR64C1Split4Res>(s, A, r3, nt, psr);
            else launch_rows<TrainR64C1>(s, A, r3, nt, psr);
        });
        L.run("ft_stats_y4", [&] { hipLaunchKernelGGL((gn_stats_seq_k<64, 64, 8>), dim3(nt), dim3(512), 0, s, a["d_y4"], a["ts_r64g2.mean"], a["ts_r64g2.rstd"]); });
        A.in = a["d_y4"], A.out = a["d_x6"], A.wfrag = w["r64c2.w16"], A.bias_frag = w["r64c2.braw"], A.skip = a["d_d2"];
        A.in_mean = a["ts_r64g2.mean"], A.in_rstd = a["ts_r64g2.rstd"], A.in_gamma = w["r64g2.w"], A.in_beta = w["r64g2.b"];
        L.run("ft_res64_conv2", [&] {
            if (q4r) launch_rows<TrainR64C2Split4Res>(s, A, r3, nt, psr);
            else launch_rows<TrainR64C2>(s, A, r3, nt, psr);
        });
        L.run("ft_csum_x6", [&] { hipLaunchKernelGGL((csum_seq_k<64, 64>), dim3(nt), dim3(512), 0, s, a["d_x6"], a["ts_dcsum"]); });
    }
    if (c->train_folded_tail) {
        // the tail as ONE linear operator, like inference: fragments rebuilt from the live parameters (fp64 fold on the device), then the
        // small-batch tail kernel writing the reconstruction in the tile layout (vq_train_tail.h)
        if (ws == s) rc = fulltrain_fold_tail(c, L, s);
        else if (hipStreamWaitEvent(s, fold_done, 0) != hipSuccess) rc = fail(c, VQHIP_ERR_DEVICE, "training forward: waiting for the tail fold failed");
        if (rc) return rc;
        L.run("ft_dgate", [&] { hipLaunchKernelGGL(se_gate_k<64>, dim3(nt), dim3(64), 0, s, a["ts_dcsum"], w["dfc0"], w["dfc2"], a["t_dgate"]); });
        ConvArgs A{};
        A.in = a["d_x6"], A.out = a["t_recon"], A.wfrag = w["ft.tail.w"], A.bias_frag = w["ft.tail.b"], A.se_gate = a["t_dgate"];
        A.n_tiles = nt, A.n_leaves = n;
        L.run("ft_tail", [&] { hipLaunchKernelGGL(tail_small_k<true>, dim3(nt, 4), dim3(256), 0, s, A); });
        return L.rc;
    }
    {
        ConvArgs A{};
        A.in = a["d_x6"], A.se_csum = a["ts_dcsum"], A.se_fc0 = w["dfc0"], A.se_fc2 = w["dfc2"], A.n_tiles = nt, A.n_steps = nk3, A.n_taps = 27, A.grp_start = g64;
        A.out = a["t_upA"], A.wfrag = w["ft.upA.w"], A.bias_frag = w["ft.upA.b"];
        L.run("ft_up_conv_a", [&] { launch_mfma32<TrainUp>(s, A, k3, nt, ps128); });
        A.out = a["t_upB"], A.wfrag = w["ft.upB.w"], A.bias_frag = w["ft.upB.b"];
        L.run("ft_up_conv_b", [&] { launch_mfma32<TrainUp>(s, A, k3, nt, ps128); });
    }
    L.run("ft_final", [&] {
        hipLaunchKernelGGL(pixshuf_k<false>, dim3(std::min(nt * 512, 65536)), dim3(256), 0, s, a["t_upA"], a["t_upB"], a["t_ps"], nt);
        hipLaunchKernelGGL(final_fwd_k, dim3(nt, 64), dim3(256), 0, s, a["t_ps"], param(c, "decoder.final.weight"), param(c, "decoder.final.bias"), a["t_pre"],
                           a["t_recon"]);
    });
    return L.rc;
}

// (input position, output position) pairs of every tap of a convolution geometry, sorted by tap (wgrad32_k schedule)
void wsteps_conv(int SI, int SO, int KS, int STRIDE, int PAD, std::vector<int>& pairs, std::vector<int>& start)
{
    pairs.clear(), start.clear();
    for (int kd = 0; kd < KS; ++kd)
        for (int kh = 0; kh < KS; ++kh)
            for (int kw = 0; kw < KS; ++kw) {
                start.push_back((int)pairs.size() / 2);
                for (int od = 0; od < SO; ++od)
                    for (int oh = 0; oh < SO; ++oh)
                        for (int ow = 0; ow < SO; ++ow) {
                            const int id = od * STRIDE - PAD + kd, ih = oh * STRIDE - PAD + kh, iw = ow * STRIDE - PAD + kw;
                            if (id < 0 || id >= SI || ih < 0 || ih >= SI || iw < 0 || iw >= SI) continue;
                            pairs.push_back((id * SI + ih) * SI + iw);
                            pairs.push_back((od * SO + oh) * SO + ow);
                        }
            }
    start.push_back((int)pairs.size() / 2);
}

int upload_wsteps(vqhip_codec* c, const char* name, int SI, int SO, int KS, int STRIDE, int PAD)
{
    if (c->dw.count(name)) return VQHIP_OK;
    std::vector<int> pairs, start;
    wsteps_conv(SI, SO, KS, STRIDE, PAD, pairs, start);
    while (pairs.size() % 4) pairs.push_back(0);
    while (start.size() % 4) start.push_back(start.back());
    int rc = upload_i(c, name, pairs);
    if (rc) return rc;
    return upload_i(c, (std::string(name) + ".start").c_str(), start);
}

// scratch for partial gradients: [wgrad partials | channel partials A | channel partials B | small partials]
struct PartBufs {
    float *wg, *chA, *chB, *small;
    float *sideCh, *sideSmall;   // the side stream's own channel / small partials (bias gradients, first conv)
    float *redCh, *gnParts;      // the reduction stream's bias partials; one (dgamma, dbeta) partial pair per GroupNorm layer of the step
    float* defParts;             // deferred reductions: every bias layer's own partial block
};
constexpr int DEF_PART_CHANNELS = 3 * 128 + 3 * 64 + 3 * 32 + 3 * 16 + 64;   // the bias sums of a step (unfolded tail: two up_conv halves), + slack
constexpr int GN_PART_CHANNELS = 3 * 64 + 2 * 32 + 3 * 16;   // the eight GroupNorm backward passes of a step
constexpr int WG_GROUPS = 32;
constexpr size_t WG_MAX = (size_t)27 * 128 * 64;  // largest KT*COUT*CIN among the layers (up_conv half)

int ensure_parts(vqhip_codec* c, int nt, PartBufs& pb)
{
    const size_t wg = (size_t)WG_GROUPS * WG_MAX, ch = (size_t)nt * 128 * 32, sm = (size_t)nt * 4096;   // (first conv: 8 planes x 432 per tile)
    const size_t gnp = (size_t)nt * 32 * 2 * GN_PART_CHANNELS;
    const size_t dfp = (size_t)nt * 32 * DEF_PART_CHANNELS;
    const size_t need = (wg + 4 * ch + 2 * sm + gnp + dfp) * sizeof(float);
    if (int rc = ensure(c, c->ft_part, need, "the partial-gradient scratch")) return rc;
    pb.wg = reinterpret_cast<float*>(c->ft_part.get());
    pb.chA = pb.wg + wg;
    pb.chB = pb.chA + ch;
    pb.small = pb.chB + ch;
    pb.sideCh = pb.small + sm;
    pb.sideSmall = pb.sideCh + ch;
    pb.redCh = pb.sideSmall + sm;
    pb.gnParts = pb.redCh + ch;
    pb.defParts = pb.gnParts + gnp;
    return VQHIP_OK;
}

// helpers of the backward pass ---------------------------------------------------------------------------------
struct Bwd {
    vqhip_codec* c;
    Launcher& L;
    hipStream_t s;
    int nt;
    float* G;       // flat gradient vector (device)
    PartBufs pb;
    // Weight and bias gradients leave the data-gradient chain: they run on a second stream (ws) beside it.  fork() = "ws may start what was
    // enqueued on s so far", join() = "s waits for everything on ws".  Nothing on s overwrites a buffer the side stream still reads: the
    // backward pass keeps such buffers (g64d / g32d / g16d exist for that) until the join at the end of the step.  One stream: ws == s.
    hipStream_t ws = nullptr;
    hipEvent_t next_event()
    {
        if (c->ft_ev_next == c->ft_ev.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            c->ft_ev.push_back(e);
        }
        return c->ft_ev[c->ft_ev_next++];
    }
    void link(hipStream_t from, hipStream_t to)
    {
        if (from == to || L.rc != VQHIP_OK) return;
        hipEvent_t e = next_event();
        if (!e || hipEventRecord(e, from) != hipSuccess || hipStreamWaitEvent(to, e, 0) != hipSuccess) {
            c->err = "training side stream: event record / wait failed";
            L.rc = VQHIP_ERR_DEVICE;
        }
    }
    // Round 6: a third stream (rs) takes the small reductions NOTHING on the data-gradient chain waits for — bias sums (csum_seq_k +
    // chan_reduce_k), the channel reductions of the GroupNorm-affine gradients (gn_bwd_finish_k) and of the attention weights
    // (parts_reduce_k): 40 launches, 0.5 ms of the chain's 2.9 ms at 2048 leaves per rank (profiles/r06_train_step_timeline_2048.txt, where
    // they sat between a layer's dY and its data-gradient conv).  fork() orders BOTH streams after the chain with one event; launches for
    // rs that follow a chain kernel directly are parked in `pending` and leave at the next fork / join, so the chain gets no extra events.
    // Round 6, final form: DEFERRED reductions.  The 40 small launches are not launched at all where they arise: a bias sum, a channel
    // reduction or a parts reduction becomes a JOB (vq_grad_kernels.h: CsumJobs / RedJobs), and join() — or the decoder-done point of the
    // RCCL overlap — puts two multi-job launches on the chain's stream behind its last kernel.  Everything they read stays alive until
    // then (the backward pass keeps every dY for the weight-gradient stream anyway; every layer has its own partial blocks).  Same
    // arithmetic per job as csum_seq_k / chan_reduce_k / parts_reduce_k: gradients bit-identical to every other arrangement.  No third
    // stream, hence no dependence on which hardware queue a stream happens to get (the third-stream form, VQHIP_TRAIN_BIAS=third, runs
    // 4.1 or 4.5 ms at 2048 leaves per rank and 2.7 or 4.9 ms at 1024 depending on that: profiles/r06_train_step_ab_reduction_stream.txt).
    CsumJobs cj{};
    RedJobs rj{};
    int cblocks = 0, rblocks = 0;
    size_t def_part_off = 0;
    bool deferred() const { return c->train_red_deferred; }
    void red_job(int kind, const float* part, int n_parts, int n, float* dst, float scale)
    {
        if (rj.n >= RED_MAX_JOBS) flush_deferred();
        rj.j[rj.n++] = RedJob{part, dst, kind, n_parts, n, rblocks, scale};
        rblocks += kind == 0 ? n : (n + 63) / 64;
    }
    void flush_deferred()
    {
        if (!cj.n && !rj.n) return;
        const CsumJobs cjl = cj;
        const RedJobs rjl = rj;
        const int cb = cblocks, rb = rblocks;
        L.run("bt_reductions", [&] {
            if (cjl.n) hipLaunchKernelGGL(csum_multi_k, dim3(cb), dim3(128), 0, s, cjl);
            if (rjl.n) hipLaunchKernelGGL(reduce_multi_k, dim3(rb), dim3(256), 0, s, rjl);
        });
        cj.n = rj.n = 0, cblocks = rblocks = 0;
    }
    hipStream_t rs = nullptr;
    std::vector<std::function<void()>> pending;
    size_t gn_part_off = 0;
    int64_t fork_mark = -1;
    bool third() const { return rs && rs != s; }
    void fork()   // (the other streams are in order: one event covers every launch that follows until the main stream has moved on)
    {
        if (L.on_main == fork_mark) return;
        fork_mark = L.on_main;
        if (L.rc != VQHIP_OK) return;
        if (ws != s || third()) {
            hipEvent_t e = next_event();
            bool ok = e && hipEventRecord(e, s) == hipSuccess;
            if (ok && ws != s) ok = hipStreamWaitEvent(ws, e, 0) == hipSuccess;
            if (ok && third()) ok = hipStreamWaitEvent(rs, e, 0) == hipSuccess;
            if (!ok) {
                c->err = "training side streams: event record / wait failed";
                L.rc = VQHIP_ERR_DEVICE;
                return;
            }
        }
        flush();
    }
    void flush()
    {
        for (auto& f : pending) f();
        pending.clear();
    }
    // a launch group for the reduction stream that reads what the chain's LAST kernel wrote
    template <typename F>
    void after_chain(const char* lname, F&& f)
    {
        if (!third()) {
            L.run(lname, f);
            return;
        }
        std::string name(lname);
        pending.push_back([this, name, f] { L.run_on(rs, name.c_str(), f); });
    }
    void join()
    {
        flush_deferred();
        fork_mark = -1;
        fork();   // (parked reductions leave; both streams are ordered after the chain's end)
        link(ws, s);
        if (third()) link(rs, s);
    }
    float* g(const char* name) { return G + c->p_off.at(name).first; }
    int groups() const { return std::min(nt, WG_GROUPS); }
    int tiles_per_group() const { return (nt + groups() - 1) / groups(); }

    // weight gradient of a leaf-tile conv into G[wname] rows [row0, row0+COUT)
    template <int CIN, int COUT, int NPI, int NPO, int INMODE, int GIN>
    void wgrad(const char* lname, const float* dy, const float* x, const char* geom, int KT, const char* wname, int row0, int IC, float scale,
               const float* mean = nullptr, const float* rstd = nullptr, const float* gamma = nullptr, const float* beta = nullptr, const float* gate = nullptr)
    {
        WgradArgs A{};
        A.dy = dy, A.x = x, A.mean = mean, A.rstd = rstd, A.gamma = gamma, A.beta = beta, A.gate = gate;
        fork();
        if constexpr (NPI == 64 && NPO == 64 && CIN % 32 == 0 && COUT % 32 == 0) {
            // k3 p1 at 4^3: rolling-window kernel, equal slices of the (class, tile, row pair) order (wgrad_rows4_k).  Slices: one workgroup per
            // CU for the eight-wave layers, two for the four-wave ones, four for the 32 -> 32 layers (16 x 16 quadrants) (measured, tools/ablate/wgrad_ablate.hip); never more than macro steps.
            if (KT == 27 && c->train_wgrad_rows) {
                constexpr int NT4 = rows4_threads<CIN, COUT>();
                // (train_wgrad_cu_pct < 100: fewer slices than CUs, so that the data-gradient chain's kernels — whose LDS does not fit beside a
                // weight-gradient workgroup on one CU — always find free CUs)
                const int Q = (int)std::min<int64_t>((int64_t)100 * nt, std::max<int64_t>(1, c->n_cus * c->train_wgrad_cu_pct / 100) * (NT4 >= 512 ? 1 : CIN == 32 && COUT == 32 ? 4 : 2));
                static_assert((size_t)(512 + 8) * 3 * COUT * CIN <= (size_t)WG_GROUPS * WG_MAX || NT4 >= 512, "partial buffer");
                static_assert((size_t)(256 + 8) * 3 * COUT * CIN <= (size_t)WG_GROUPS * WG_MAX, "partial buffer");
                if ((size_t)(Q + 8) * 3 * COUT * CIN <= (size_t)WG_GROUPS * WG_MAX) {
                    A.part = pb.wg, A.n_tiles = nt, A.KT = 27;
                    float* dst4 = g(wname);
                    float* part4 = pb.wg;
                    const int ntl = nt;
                    L.run_on(ws, lname, [&] {
                        hipLaunchKernelGGL((wgrad_rows4_k<CIN, COUT, INMODE, GIN>), dim3(Q), dim3(NT4), 0, ws, A);
                        hipLaunchKernelGGL(wgrad_rows4_reduce_k, dim3(std::min(4096, 27 * COUT * CIN / 64)), dim3(256), 0, ws, part4, Q, ntl, COUT, CIN, dst4, row0, IC, scale);
                    });
                    return;
                }
                // (not silently: the pair-per-step kernel below is 15-30 % slower on these layers)
                static std::atomic<bool> told{false};
                if (!told.exchange(true))
                    fprintf(stderr, "vqvdb_hip: weight gradient %s: %d slices do not fit the partial buffer on this device (%d CUs), using the pair-per-step kernel\n",
                            lname, Q, c->n_cus);
            }
        }
        A.wsteps = reinterpret_cast<const int2*>(c->dw[geom]);
        A.tap_start = reinterpret_cast<const int*>(c->dw[std::string(geom) + ".start"]);
        A.part = pb.wg, A.n_tiles = nt, A.tiles_per_group = tiles_per_group(), A.KT = KT;
        const int ng = (nt + A.tiles_per_group - 1) / A.tiles_per_group;
        constexpr int NT = CIN == 16 ? 64 : ((COUT + 31) / 32) * ((CIN + 31) / 32) * 64;
        // split every tap's pair list into chunks while the partial buffer allows it and the launch is short of ~4096 waves
        int chunks = 1;
        while (chunks < 16 && (size_t)ng * (2 * chunks) * KT * COUT * CIN <= (size_t)WG_GROUPS * WG_MAX && (int64_t)KT * ng * chunks * (NT / 64) < 4096) chunks *= 2;
        float* dst = g(wname);
        float* part = pb.wg;
        L.run_on(ws, lname, [&] {
            hipLaunchKernelGGL((wgrad32_k<CIN, COUT, NPI, NPO, INMODE, GIN>), dim3(KT, ng, chunks), dim3(NT), 0, ws, A);
            hipLaunchKernelGGL(wgrad_reduce_k, dim3(std::min(4096, (KT * COUT * CIN + 63) / 64)), dim3(256), 0, ws, part, ng * chunks, KT, COUT, CIN, dst, row0, IC, scale);
        });
    }
    // 16 -> 16 k3 layers at 8^3: row-reuse kernel (X' = relu(GroupNorm(8,16)(x)))
    void wgrad16(const char* lname, const float* dy, const float* x, const char* wname, float scale, const float* mean, const float* rstd,
                 const float* gamma, const float* beta)
    {
        WgradArgs A{};
        A.dy = dy, A.x = x, A.mean = mean, A.rstd = rstd, A.gamma = gamma, A.beta = beta;
        A.part = pb.wg, A.n_tiles = nt, A.tiles_per_group = tiles_per_group(), A.KT = 27;
        const int ng = (nt + A.tiles_per_group - 1) / A.tiles_per_group;
        int chunks = 1;
        while (chunks < 16 && (int64_t)9 * ng * chunks < 2048) chunks *= 2;
        float* dst = g(wname);
        float* part = pb.wg;
        fork();
        if (c->train_wgrad_rows) {
            // a plane (tile, od, kd) per step of a workgroup, all nine (kh, kw) taps from one pass over the rows (wgrad16_planes_k);
            // P planes per workgroup so that the launch has at most ~1500 workgroups
            const int P = std::max(1, (nt + 63) / 64), gx = (8 * nt + P - 1) / P;
            const int ntl = nt;
            L.run_on(ws, lname, [&] {
                hipLaunchKernelGGL(wgrad16_planes_k, dim3(gx, 3), dim3(512), 0, ws, A, P);
                hipLaunchKernelGGL(wgrad16_planes_reduce_k, dim3(27 * 256 / 64), dim3(256), 0, ws, part, gx, ntl, P, dst, scale);
            });
            return;
        }
        L.run_on(ws, lname, [&] {
            hipLaunchKernelGGL(wgrad16_rows_k, dim3(9, ng, chunks), dim3(192), 0, ws, A, chunks);
            hipLaunchKernelGGL(wgrad_reduce_k, dim3(27 * 256 / 64), dim3(256), 0, ws, part, ng * chunks, 27, 16, 16, dst, 0, 16, scale);
        });
    }
    // per-channel sum over leaves and positions of an L4 gradient (bias gradients) into dst[0..C)
    template <int C, int NP>
    void bias_grad(const char* lname, const float* dy, float* dst, float scale)
    {
        // on the data-gradient stream by default (round 4): since the one-pass GroupNorm backward that stream waits for the weight-gradient
        // stream at the end of the step, so the bias sums (0.27 ms of small launches at 2048 leaves) ride in its slack
        static_assert((C == 64 && NP == 64) || (C == 128 && NP == 64) || (C == 32 && NP == 64) || (C == 16 && NP == 512), "csum_multi_k dispatches these shapes");
        if (deferred()) {
            if (cj.n >= RED_MAX_CSUM || def_part_off + (size_t)nt * C * 32 > (size_t)nt * 32 * DEF_PART_CHANNELS) flush_deferred(), def_part_off = 0;
            float* part = pb.defParts + def_part_off;
            def_part_off += (size_t)nt * C * 32;
            cj.j[cj.n++] = CsumJob{dy, part, C, NP, cblocks};
            cblocks += nt * (C / 16);
            red_job(0, part, nt, C, dst, scale);
            return;
        }
        hipStream_t bs = third() ? rs : c->train_bias_main ? s : ws;
        float* part = bs == s ? pb.chA : bs == ws ? pb.sideCh : pb.redCh;
        const int n = nt;
        if (bs != s) fork();
        L.run_on(bs, lname, [&] {
            hipLaunchKernelGGL((csum_seq_k<C, NP>), dim3(n), dim3(64 * C / 8), 0, bs, dy, part);
            hipLaunchKernelGGL(chan_reduce_k, dim3(C), dim3(256), 0, bs, part, n, C, dst, scale);
        });
    }
    // GroupNorm+ReLU backward: dx = d(relu(gn(x)))/dx applied to da (+ add); dgamma/dbeta into G
    template <int C, int NP, int CPG>
    void gn_bwd(const char* lname, const float* x, const float* da, const char* stats, const char* gname, const char* bname, const float* add, float* dx)
    {
        auto& a = c->act;
        const float *mean = a[std::string(stats) + ".mean"], *rstd = a[std::string(stats) + ".rstd"];
        const float *gamma = c->ft_P + c->p_off.at(gname).first, *beta = c->ft_P + c->p_off.at(bname).first;
        float *s1 = a["gs_1"], *s2 = a["gs_2"], *c1 = a["gs_c1"], *c2 = a["gs_c2"], *pa = pb.chA, *pbb = pb.chB, *dg = g(gname), *db = g(bname);
        const int n = nt;
        // position ranges per tile while the launch is short of ~2048 waves (partial buffers hold up to 8 ranges of 16 channels)
        int sp = 1;
        while (sp < 8 && sp * 2 * C <= 128 && NP / (sp * 2) >= 16 && (int64_t)n * sp * (C / 8) < 2048) sp *= 2;
        if (c->train_gn_fused) {
            // one pass: a workgroup owns whole groups of a tile, x and da are read once (gn_bwd_fused_k); then the channel reduction of
            // the dgamma / dbeta partials (gn_bwd_finish_k's second half: no combine blocks)
            constexpr int QW = C == 64 ? 2 : 1, LW = C == 16 ? 16 : 32, NT = C == 64 ? 512 : (C == 32 ? 256 : 1024);
            if (deferred() || third()) {
                // the channel reduction of dgamma / dbeta leaves the chain: this layer's own partial pair (the chain's next GroupNorm must not overwrite it)
                float* qa = pb.gnParts + gn_part_off;
                float* qb = qa + (size_t)n * C * 32;
                gn_part_off += (size_t)2 * n * C * 32;
                if (gn_part_off > (size_t)n * 32 * 2 * GN_PART_CHANNELS) {
                    c->err = "GroupNorm backward: more layers than partial buffers";
                    L.rc = VQHIP_ERR_INVALID;
                    return;
                }
                L.run(lname, [&] { hipLaunchKernelGGL((gn_bwd_fused_k<C, NP, CPG, QW, LW, NT>), dim3(n, 8), dim3(NT), 0, s, x, da, mean, rstd, gamma, beta, add, dx, qa, qb); });
                if (deferred()) {
                    red_job(0, qa, n, C, dg, 1.0f);
                    red_job(0, qb, n, C, db, 1.0f);
                    return;
                }
                hipStream_t r = rs;
                after_chain((std::string(lname) + "_affine").c_str(),
                            [=] { hipLaunchKernelGGL(gn_bwd_finish_k, dim3(2 * C), dim3(256), 0, r, s1, s2, 1, 0, n, c1, c2, qa, qb, C, dg, db); });
                return;
            }
            L.run(lname, [&] {
                hipLaunchKernelGGL((gn_bwd_fused_k<C, NP, CPG, QW, LW, NT>), dim3(n, 8), dim3(NT), 0, s, x, da, mean, rstd, gamma, beta, add, dx, pa, pbb);
                hipLaunchKernelGGL(gn_bwd_finish_k, dim3(2 * C), dim3(256), 0, s, s1, s2, 1, 0, n, c1, c2, pa, pbb, C, dg, db);
            });
            return;
        }
        L.run(lname, [&] {
            hipLaunchKernelGGL((gn_bwd_sums_k<C, NP, CPG>), dim3(n, sp), dim3(64 * C / 8), 0, s, x, da, mean, rstd, gamma, beta, s1, s2, pa, pbb);
            constexpr int per_tile = (C / CPG) * 32;
            hipLaunchKernelGGL(gn_bwd_finish_k, dim3((n * per_tile + 255) / 256 + 2 * C), dim3(256), 0, s, s1, s2, sp, per_tile, n, c1, c2, pa, pbb, C, dg, db);
            hipLaunchKernelGGL((gn_bwd_apply_k<C, NP, CPG>), dim3(n, 8), dim3(256), 0, s, x, da, mean, rstd, gamma, beta, c1, c2, 1, add, dx);
        });
    }
};

// backward of the decoder: from d(loss)/d(pre) down to d(loss)/d(q) (left in "g_q"), decoder gradients into G
int fulltrain_backward_decoder(Bwd& B, int64_t n, float c_mse, float c_l1)
{
    vqhip_codec* c = B.c;
    auto& a = c->act;
    auto& w = c->dw;
    Launcher& L = B.L;
    hipStream_t s = B.s;
    const int nt = B.nt, g2 = (nt + 1) / 2;
    const int4* k3 = (const int4*)w["steps.k3s1_4"];
    const int nk3 = c->nsteps["steps.k3s1_4"];
    const int* g64 = reinterpret_cast<const int*>(w["steps.k3s1_4.grp"]);   // position-split launches (64 output positions)
    const int ps64 = split_factor(g2, 1, 32, 1024);
    const int g4 = (nt + 3) / 4, ps128 = split_factor(g4, 1, 32, 512);
    const int gh = (2 * nt + 7) / 8, psr = split_factor(gh, 1, 16, 512);   // conv_rows16_k: 8 half tiles per workgroup, 16 output rows
    const int4* r3 = (const int4*)w["steps.rows_k3_4"];
    const int* gr16 = reinterpret_cast<const int*>(w["steps.rows_k3_4.grp"]);
    if (c->train_folded_tail) {
        // dpre in both layouts; then everything about the tail goes through the folded operator (vq_train_tail.h)
        L.run("bt_loss_grad", [&] {
            hipLaunchKernelGGL(loss_grad_k, dim3(std::min(nt * 64, 4096)), dim3(256), 0, s, a["xt"], a["t_recon"], a["g_pre"], c_mse, c_l1, n, nt, a["g_pre4"]);
        });
        {   // data gradient wrt the gated input x' = gate * x6: g64a = Wc^T dpre
            ConvArgs A{};
            A.in = a["g_pre4"], A.out = a["g64a"], A.wfrag = w["ft.tailT.w"], A.bias_frag = w["bt.zero128"], A.n_tiles = nt;
            A.n_steps = c->nsteps["steps.tailT"], A.n_taps = 224, A.grp_start = reinterpret_cast<const int*>(w["steps.tailT.grp"]);
            L.run("bt_tail_dgrad", [&] { launch_mfma32<DgradTail>(s, A, w["steps.tailT"], nt, ps128); });
        }
        {   // gradient of the folded weights (K = leaves), then the chain rule back to up_conv / final
            WgradArgs A{};
            A.dy = a["g_pre4"], A.x = a["d_x6"], A.gate = a["t_dgate"];
            A.wsteps = reinterpret_cast<const int2*>(w["w.tail"]), A.tap_start = reinterpret_cast<const int*>(w["w.tail.start"]);
            A.part = B.pb.wg, A.n_tiles = nt, A.KT = 224;
            const int max_groups = (int)std::max<size_t>(1, (size_t)WG_GROUPS * WG_MAX / ((size_t)224 * 128 * 64));   // what the partial buffer holds
            A.tiles_per_group = (nt + max_groups - 1) / max_groups;
            const int ng = (nt + A.tiles_per_group - 1) / A.tiles_per_group;
            float* dWc = w["ft.tail.dWc"];
            float* dbc = w["ft.tail.dbc"];
            double* dG = reinterpret_cast<double*>(w["ft.tail.dG"]);
            double* dBg = reinterpret_cast<double*>(w["ft.tail.dBg"]);
            hipStream_t ws = B.ws;
            B.fork();
            L.run_on(ws, "bt_tail_wgrad", [&] {
                hipLaunchKernelGGL((wgrad32_k<64, 128, 64, 4, 2, 0>), dim3(224, ng, 1), dim3(512), 0, ws, A);
                hipLaunchKernelGGL(wgrad_reduce_k, dim3(4096), dim3(256), 0, ws, B.pb.wg, ng, 224, 128, 64, dWc, 0, 64, 1.0f);
            });
            L.run_on(ws, "bt_tail_chain", [&] {
                hipLaunchKernelGGL(tail_dbc_k, dim3(512), dim3(256), 0, ws, a["g_pre"], nt, dbc);
                hipLaunchKernelGGL(tail_chain_dbg_k, dim3(1), dim3(256), 0, ws, dbc, dBg);
                hipLaunchKernelGGL(tail_chain_dg_k, dim3((27 * 8 * 27 * 64 + 255) / 256), dim3(256), 0, ws, dWc, dG);
                hipLaunchKernelGGL(tail_chain_wu_k, dim3((256 * 64 * 27 + 255) / 256), dim3(256), 0, ws, dG, dBg, param(c, "decoder.final.weight"),
                                   B.g("decoder.up_conv.weight"), B.g("decoder.up_conv.bias"));
                hipLaunchKernelGGL(tail_chain_wf_k, dim3(865), dim3(256), 0, ws, dG, dBg, param(c, "decoder.up_conv.weight"), param(c, "decoder.up_conv.bias"), dbc,
                                   B.g("decoder.final.weight"), B.g("decoder.final.bias"));
            });
        }
    } else {
        L.run("bt_loss_grad", [&] { hipLaunchKernelGGL(loss_grad_k, dim3(std::min(nt * 64, 4096)), dim3(256), 0, s, a["xt"], a["t_recon"], a["g_pre"], c_mse, c_l1, n, nt); });
        L.run("bt_final_wgrad", [&] {
            const int fs = nt <= 256 ? 8 : 1;   // position ranges per tile
            hipLaunchKernelGGL(final_wgrad_k, dim3(nt, fs), dim3(512), 0, s, a["g_pre"], a["t_ps"], B.pb.wg);
            hipLaunchKernelGGL(parts_reduce_k, dim3((865 + 63) / 64), dim3(256), 0, s, B.pb.wg, nt * fs, 865, B.g("decoder.final.weight"), 1.0f);
        });
        L.run("bt_final_dgrad", [&] {
            hipLaunchKernelGGL(final_bwd_data_k, dim3(nt, 64), dim3(256), 0, s, a["g_pre"], param(c, "decoder.final.weight"), a["g_ps"]);
            hipLaunchKernelGGL(pixshuf_k<true>, dim3(std::min(nt * 512, 65536)), dim3(256), 0, s, a["g_upA"], a["g_upB"], a["g_ps"], nt);
        });
        // up_conv: gates of the attention, weight / bias gradients of both halves, data gradient (two partial results, summed by se_bwd_k)
        L.run("bt_dgate", [&] { hipLaunchKernelGGL(se_gate_k<64>, dim3(nt), dim3(64), 0, s, a["ts_dcsum"], w["dfc0"], w["dfc2"], a["t_dgate"]); });
        B.wgrad<64, 128, 64, 64, 2, 0>("bt_up_wgrad_a", a["g_upA"], a["d_x6"], "w.k3_4", 27, "decoder.up_conv.weight", 0, 64, 1.0f, nullptr, nullptr, nullptr, nullptr, a["t_dgate"]);
        B.wgrad<64, 128, 64, 64, 2, 0>("bt_up_wgrad_b", a["g_upB"], a["d_x6"], "w.k3_4", 27, "decoder.up_conv.weight", 128, 64, 1.0f, nullptr, nullptr, nullptr, nullptr, a["t_dgate"]);
        B.bias_grad<128, 64>("bt_up_bias_a", a["g_upA"], B.g("decoder.up_conv.bias"), 1.0f);
        B.bias_grad<128, 64>("bt_up_bias_b", a["g_upB"], B.g("decoder.up_conv.bias") + 128, 1.0f);
        {
            ConvArgs A{};
            A.bias_frag = w["bt.zero128"], A.n_tiles = nt, A.n_steps = nk3, A.n_taps = 27, A.grp_start = g64;
            A.in = a["g_upA"], A.out = a["g64a"], A.wfrag = w["bt.upA.w"];
            L.run("bt_up_dgrad_a", [&] { launch_mfma32<TrainStem>(s, A, k3, nt, ps128); });
            A.in = a["g_upB"], A.out = a["g64b"], A.wfrag = w["bt.upB.w"];
            L.run("bt_up_dgrad_b", [&] { launch_mfma32<TrainStem>(s, A, k3, nt, ps128); });
        }
    }
    {
        float* p0 = B.pb.small;
        float* p2 = B.pb.small + (size_t)nt * 1024;
        float *g0 = B.g("decoder.attn.fc.0.weight"), *g2w = B.g("decoder.attn.fc.2.weight");
        const int ntl = nt;
        L.run("bt_dattn", [&] {
            hipLaunchKernelGGL((se_bwd_k<64, 64>), dim3(nt), dim3(512), 0, s, a["d_x6"], a["g64a"], c->train_folded_tail ? (const float*)nullptr : a["g64b"], a["ts_dcsum"], w["dfc0"],
                               w["dfc2"], a["g64c"], p0, p2);
        });
        hipStream_t r = B.third() ? B.rs : s;
        if (B.deferred()) B.red_job(1, p0, ntl, 1024, g0, 1.0f), B.red_job(1, p2, ntl, 1024, g2w, 1.0f);
        else B.after_chain("bt_dattn_weights", [=] {
            hipLaunchKernelGGL(parts_reduce_k, dim3(16), dim3(256), 0, r, p0, ntl, 1024, g0, 1.0f);
            hipLaunchKernelGGL(parts_reduce_k, dim3(16), dim3(256), 0, r, p2, ntl, 1024, g2w, 1.0f);
        });
    }
    // ResidualBlock(64): x6 = d2 + 0.1 conv2(relu(gn2(y4))), y4 = conv1(relu(gn1(d2)))
    B.wgrad<64, 64, 64, 64, 1, 8>("bt_r64c2_wgrad", a["g64c"], a["d_y4"], "w.k3_4", 27, "decoder.res_stack.0.conv2.weight", 0, 64, 0.1f, a["ts_r64g2.mean"],
                                   a["ts_r64g2.rstd"], param(c, "decoder.res_stack.0.gn2.weight"), param(c, "decoder.res_stack.0.gn2.bias"));
    B.bias_grad<64, 64>("bt_r64c2_bias", a["g64c"], B.g("decoder.res_stack.0.conv2.bias"), 0.1f);
    {
        ConvArgs A{};
        A.bias_frag = w["bt.zero128"], A.n_tiles = nt, A.n_steps = c->nsteps["steps.rows_k3_4"], A.n_taps = 27, A.grp_start = gr16;
        A.in = a["g64c"], A.out = a["g64a"], A.wfrag = w["bt.r64c2.w16"];
        L.run("bt_r64c2_dgrad", [&] {
            if (c->train_r64_quarters && c->train_dgrad_small_lds && gh * psr * 4 <= 1024) launch_rows<DgradR64Split4>(s, A, r3, nt, psr);
            else if (c->train_r64_quarters && gh * psr * 4 <= 1024) launch_rows<DgradR64Split4Res>(s, A, r3, nt, psr);
            else launch_rows<DgradR64>(s, A, r3, nt, psr);
        });
    }
    B.gn_bwd<64, 64, 8>("bt_r64gn2", a["d_y4"], a["g64a"], "ts_r64g2", "decoder.res_stack.0.gn2.weight", "decoder.res_stack.0.gn2.bias", nullptr, a["g64b"]);
    B.wgrad<64, 64, 64, 64, 1, 8>("bt_r64c1_wgrad", a["g64b"], a["d_d2"], "w.k3_4", 27, "decoder.res_stack.0.conv1.weight", 0, 64, 1.0f, a["ts_r64g1.mean"],
                                   a["ts_r64g1.rstd"], param(c, "decoder.res_stack.0.gn1.weight"), param(c, "decoder.res_stack.0.gn1.bias"));
    B.bias_grad<64, 64>("bt_r64c1_bias", a["g64b"], B.g("decoder.res_stack.0.conv1.bias"), 1.0f);
    {
        ConvArgs A{};
        A.bias_frag = w["bt.zero128"], A.n_tiles = nt, A.n_steps = c->nsteps["steps.rows_k3_4"], A.n_taps = 27, A.grp_start = gr16;
        A.in = a["g64b"], A.out = a["g64a"], A.wfrag = w["bt.r64c1.w16"];
        L.run("bt_r64c1_dgrad", [&] {
            if (c->train_r64_quarters && c->train_dgrad_small_lds && gh * psr * 4 <= 1024) launch_rows<DgradR64Split4>(s, A, r3, nt, psr);
            else if (c->train_r64_quarters && gh * psr * 4 <= 1024) launch_rows<DgradR64Split4Res>(s, A, r3, nt, psr);
            else launch_rows<DgradR64>(s, A, r3, nt, psr);
        });
    }
    // (into g64d: the side stream may still be reading g64b for conv1's weight gradient)
    B.gn_bwd<64, 64, 8>("bt_r64gn1", a["d_d2"], a["g64a"], "ts_r64g1", "decoder.res_stack.0.gn1.weight", "decoder.res_stack.0.gn1.bias", a["g64c"], a["g64d"]);
    // stem: d2 = relu(gn(ys)), ys = conv(q)
    B.gn_bwd<64, 64, 8>("bt_dgn", a["d_ystem"], a["g64d"], "ts_dgn", "decoder.stem.1.weight", "decoder.stem.1.bias", nullptr, a["g64a"]);
    B.wgrad<128, 64, 64, 64, 0, 0>("bt_stem_wgrad", a["g64a"], a["t_q"], "w.k3_4", 27, "decoder.stem.0.weight", 0, 128, 1.0f);
    B.bias_grad<64, 64>("bt_stem_bias", a["g64a"], B.g("decoder.stem.0.bias"), 1.0f);
    {
        ConvArgs A{};
        A.bias_frag = w["bt.zero128"], A.n_tiles = nt, A.n_steps = nk3, A.n_taps = 27, A.grp_start = g64;
        A.in = a["g64a"], A.out = a["g_q"], A.wfrag = w["bt.stem.w"];
        L.run("bt_stem_dgrad", [&] { launch_mfma32<DgradStem>(s, A, k3, nt, ps128); });
    }
    return L.rc;
}

constexpr auto kTrainEncConvs = conv_kernels(TrainEncConvs{});   // ... and of the encoder: proj^T, res32 conv^T

// backward of the quantizer's straight-through path and of the encoder: consumes d(loss)/d(q) in "g_q"
int fulltrain_backward_encoder(Bwd& B, int64_t n, float c_commit)
{
    vqhip_codec* c = B.c;
    auto& a = c->act;
    auto& w = c->dw;
    Launcher& L = B.L;
    hipStream_t s = B.s;
    const int nt = B.nt, g2 = (nt + 1) / 2;
    L.run("bt_straight_through", [&] { hipLaunchKernelGGL(st_grad_k, dim3(std::min(nt * 256, 65536)), dim3(256), 0, s, a["g_q"], a["t_z"], a["t_q"], a["g_q"], c_commit, n, nt); });
    // proj (1x1x1, 32 -> 128) on the gated activations
    if (!c->ft_egate_early) L.run("bt_egate", [&] { hipLaunchKernelGGL(se_gate_k<32>, dim3(nt), dim3(64), 0, s, a["ts_ecsum"], w["efc0"], w["efc2"], a["t_egate"]); });
    B.wgrad<32, 128, 64, 64, 2, 0>("bt_proj_wgrad", a["g_q"], a["e_x11"], "w.k1_4", 1, "encoder.proj.weight", 0, 32, 1.0f, nullptr, nullptr, nullptr, nullptr, a["t_egate"]);
    B.bias_grad<128, 64>("bt_proj_bias", a["g_q"], B.g("encoder.proj.bias"), 1.0f);
    {
        ConvArgs A{};
        A.bias_frag = w["bt.zero128"], A.n_tiles = nt, A.n_steps = c->nsteps["steps.k1_4"], A.n_taps = 1;
        A.grp_start = reinterpret_cast<const int*>(w["steps.k1_4.grp"]);
        A.in = a["g_q"], A.out = a["g32a"], A.wfrag = w["bt.proj.w"];
        L.run("bt_proj_dgrad", [&] { launch_mfma32<DgradProj>(s, A, w["steps.k1_4"], nt, split_factor(g2, 1, 16, 1024)); });
    }
    {
        // (its own region of the small partials: the decoder's attention reduction may still be pending on the reduction stream)
        float* p0 = B.pb.small + (size_t)nt * 2048;
        float* p2 = p0 + (size_t)nt * 256;
        float *g0 = B.g("encoder.attn.fc.0.weight"), *g2w = B.g("encoder.attn.fc.2.weight");
        const int ntl = nt;
        L.run("bt_eattn", [&] {
            hipLaunchKernelGGL((se_bwd_k<32, 64>), dim3(nt), dim3(256), 0, s, a["e_x11"], a["g32a"], (const float*)nullptr, a["ts_ecsum"], w["efc0"], w["efc2"], a["g32b"], p0, p2);
        });
        hipStream_t r = B.third() ? B.rs : s;
        if (B.deferred()) B.red_job(1, p0, ntl, 256, g0, 1.0f), B.red_job(1, p2, ntl, 256, g2w, 1.0f);
        else B.after_chain("bt_eattn_weights", [=] {
            hipLaunchKernelGGL(parts_reduce_k, dim3(4), dim3(256), 0, r, p0, ntl, 256, g0, 1.0f);
            hipLaunchKernelGGL(parts_reduce_k, dim3(4), dim3(256), 0, r, p2, ntl, 256, g2w, 1.0f);
        });
    }
    // ResidualBlock(32)
    const int4* r3 = (const int4*)w["steps.rows_k3_4"];
    const int nr3 = c->nsteps["steps.rows_k3_4"];
    const int gh32 = (2 * nt + 7) / 8;
    B.wgrad<32, 32, 64, 64, 1, 8>("bt_r32c2_wgrad", a["g32b"], a["e_y9"], "w.k3_4", 27, "encoder.res_stack.0.conv2.weight", 0, 32, 0.1f, a["ts_r32g2.mean"],
                                   a["ts_r32g2.rstd"], param(c, "encoder.res_stack.0.gn2.weight"), param(c, "encoder.res_stack.0.gn2.bias"));
    B.bias_grad<32, 64>("bt_r32c2_bias", a["g32b"], B.g("encoder.res_stack.0.conv2.bias"), 0.1f);
    {
        ConvArgs A{};
        A.bias_frag = w["bt.zero128"], A.n_tiles = nt, A.n_steps = nr3, A.n_taps = 27, A.grp_start = reinterpret_cast<const int*>(w["steps.rows_k3_4.grp"]);
        A.in = a["g32b"], A.out = a["g32a"], A.wfrag = w["bt.r32c2.w16"];
        L.run("bt_r32c2_dgrad", [&] {
            const int ps32 = split_factor(gh32, 1, 16, 512);
            if (c->train_dgrad_small_lds && gh32 * ps32 * 2 <= 1024) launch_rows<DgradR32Split2>(s, A, r3, nt, ps32);
            else launch_rows<DgradR32>(s, A, r3, nt, ps32);
        });
    }
    B.gn_bwd<32, 64, 4>("bt_r32gn2", a["e_y9"], a["g32a"], "ts_r32g2", "encoder.res_stack.0.gn2.weight", "encoder.res_stack.0.gn2.bias", nullptr, a["g32c"]);
    B.wgrad<32, 32, 64, 64, 1, 8>("bt_r32c1_wgrad", a["g32c"], a["e_x7"], "w.k3_4", 27, "encoder.res_stack.0.conv1.weight", 0, 32, 1.0f, a["ts_r32g1.mean"],
                                   a["ts_r32g1.rstd"], param(c, "encoder.res_stack.0.gn1.weight"), param(c, "encoder.res_stack.0.gn1.bias"));
    B.bias_grad<32, 64>("bt_r32c1_bias", a["g32c"], B.g("encoder.res_stack.0.conv1.bias"), 1.0f);
    {
        ConvArgs A{};
        A.bias_frag = w["bt.zero128"], A.n_tiles = nt, A.n_steps = nr3, A.n_taps = 27, A.grp_start = reinterpret_cast<const int*>(w["steps.rows_k3_4.grp"]);
        A.in = a["g32c"], A.out = a["g32a"], A.wfrag = w["bt.r32c1.w16"];
        L.run("bt_r32c1_dgrad", [&] {
            const int ps32 = split_factor(gh32, 1, 16, 512);
            if (c->train_dgrad_small_lds && gh32 * ps32 * 2 <= 1024) launch_rows<DgradR32Split2>(s, A, r3, nt, ps32);
            else launch_rows<DgradR32>(s, A, r3, nt, ps32);
        });
    }
    // (into g32d: the side stream may still be reading g32c for conv1's weight gradient)
    B.gn_bwd<32, 64, 4>("bt_r32gn1", a["e_x7"], a["g32a"], "ts_r32g1", "encoder.res_stack.0.gn1.weight", "encoder.res_stack.0.gn1.bias", a["g32b"], a["g32d"]);
    // down (k4 s2): g32d = d(loss)/d(x7)
    B.wgrad<16, 32, 512, 64, 0, 0>("bt_down_wgrad", a["g32d"], a["e_a6"], "w.k4s2", 64, "encoder.down.weight", 0, 16, 1.0f);
    B.bias_grad<32, 64>("bt_down_bias", a["g32d"], B.g("encoder.down.bias"), 1.0f);
    L.run("bt_down_dgrad", [&] { hipLaunchKernelGGL(deconv_down_k, dim3((2 * nt + 3) / 4, split_factor((2 * nt + 3) / 4, 1, 16, 1024)), dim3(256), 0, s, a["g32d"], w["bt.down.w"], a["g16a"], nt); });
    // ResidualBlock(16): g16a = d(loss)/d(a6)
    const int4* rg = (const int4*)w["steps.rowgroups8_4"];
    const int nrg = c->nsteps["steps.rowgroups8_4"];
    B.wgrad16("bt_r16c2_wgrad", a["g16a"], a["e_y4"], "encoder.pre.3.conv2.weight", 0.1f, a["ts_r16g2.mean"], a["ts_r16g2.rstd"],
              param(c, "encoder.pre.3.gn2.weight"), param(c, "encoder.pre.3.gn2.bias"));
    B.bias_grad<16, 512>("bt_r16c2_bias", a["g16a"], B.g("encoder.pre.3.conv2.bias"), 0.1f);
    {
        ConvArgs A{};
        A.bias_frag = w["bt.zero128"], A.n_tiles = nt, A.n_steps = nrg, A.grp_start = reinterpret_cast<const int*>(w["steps.rowgroups8_4.grp"]);
        A.in = a["g16a"], A.out = a["g16b"], A.wfrag = w["bt.r16c2.w"];
        L.run("bt_r16c2_dgrad", [&] { hipLaunchKernelGGL((conv8_c16_k<4, false, false, true>), dim3((2 * nt + 3) / 4, split_factor((2 * nt + 3) / 4, 1, 16, 1024)), dim3(256), 0, s, A, rg); });
    }
    B.gn_bwd<16, 512, 2>("bt_r16gn2", a["e_y4"], a["g16b"], "ts_r16g2", "encoder.pre.3.gn2.weight", "encoder.pre.3.gn2.bias", nullptr, a["g16c"]);
    B.wgrad16("bt_r16c1_wgrad", a["g16c"], a["e_a1"], "encoder.pre.3.conv1.weight", 1.0f, a["ts_r16g1.mean"], a["ts_r16g1.rstd"],
              param(c, "encoder.pre.3.gn1.weight"), param(c, "encoder.pre.3.gn1.bias"));
    B.bias_grad<16, 512>("bt_r16c1_bias", a["g16c"], B.g("encoder.pre.3.conv1.bias"), 1.0f);
    {
        ConvArgs A{};
        A.bias_frag = w["bt.zero128"], A.n_tiles = nt, A.n_steps = nrg, A.grp_start = reinterpret_cast<const int*>(w["steps.rowgroups8_4.grp"]);
        A.in = a["g16c"], A.out = a["g16b"], A.wfrag = w["bt.r16c1.w"];
        L.run("bt_r16c1_dgrad", [&] { hipLaunchKernelGGL((conv8_c16_k<4, false, false, true>), dim3((2 * nt + 3) / 4, split_factor((2 * nt + 3) / 4, 1, 16, 1024)), dim3(256), 0, s, A, rg); });
    }
    // (into g16d: the side stream may still be reading g16c for conv1's weight gradient)
    B.gn_bwd<16, 512, 2>("bt_r16gn1", a["e_a1"], a["g16b"], "ts_r16g1", "encoder.pre.3.gn1.weight", "encoder.pre.3.gn1.bias", a["g16a"], a["g16d"]);
    // a1 = relu(gn0(y1)), y1 = conv0(x): g16d = d(loss)/d(a1)
    B.gn_bwd<16, 512, 4>("bt_gn0", a["e_y1"], a["g16d"], "ts_gn0", "encoder.pre.1.weight", "encoder.pre.1.bias", nullptr, a["g16b"]);
    {
        hipStream_t ws = B.ws;
        float* small = B.pb.sideSmall;   // (never pb.small: the attention partials of this step wait there for the deferred reductions)
        B.fork();
        L.run_on(ws, "bt_conv0_wgrad", [&] {
            hipLaunchKernelGGL(wgrad_first_k, dim3(nt, 8), dim3(576), 0, ws, a["g16b"], a["xt"], small);
            hipLaunchKernelGGL(parts_reduce_k, dim3((432 + 63) / 64), dim3(256), 0, ws, small, nt * 8, 432, B.g("encoder.pre.0.weight"), 1.0f);
        });
    }
    B.bias_grad<16, 512>("bt_conv0_bias", a["g16b"], B.g("encoder.pre.0.bias"), 1.0f);
    B.join();   // every gradient is complete once the caller's stream gets past this point
    return L.rc;
}

}  // namespace

extern "C" {

int vqhip_fulltrain_begin(vqhip_codec* c)
{
    if (!c) return VQHIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = c->training ? VQHIP_OK : vqhip_train_begin(c, nullptr, nullptr);
    if (rc) return rc;
    const size_t np = c->h_params.size();
    if ((rc = ensure(c, c->ft_P, np, "the training parameters"))) return rc;
    if ((rc = ensure(c, c->ft_M, np, "the first AdamW moments"))) return rc;
    if ((rc = ensure(c, c->ft_V, np, "the second AdamW moments"))) return rc;
    HIPCHK(c, hipMemcpy(c->ft_P, c->h_params.data(), np * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(c->ft_M, 0, np * sizeof(float)));
    HIPCHK(c, hipMemset(c->ft_V, 0, np * sizeof(float)));
    if ((rc = refrag_all(c, c->stream))) return rc;
    if (!c->dw.count("steps.k1_4") && (rc = upload_steps(c, "steps.k1_4", steps_conv(4, 4, 1, 1, 0, 1)))) return rc;
    if ((rc = set_lds(c, kTrainDecConvs)) || (rc = set_lds(c, kTrainEncConvs))) return rc;
    if ((rc = upload_wsteps(c, "w.k3_4", 4, 4, 3, 1, 1))) return rc;
    if ((rc = upload_wsteps(c, "w.k3_8", 8, 8, 3, 1, 1))) return rc;
    if ((rc = upload_wsteps(c, "w.k4s2", 8, 4, 4, 2, 1))) return rc;
    if ((rc = upload_wsteps(c, "w.k1_4", 4, 4, 1, 1, 0))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->full_training = true;
    return VQHIP_OK;
}

int64_t vqhip_fulltrain_param_count(const vqhip_codec* c) { return c ? (int64_t)c->h_params.size() : 0; }

int vqhip_fulltrain_set_folded_tail(vqhip_codec* c, int on)
{
    if (!c) return VQHIP_ERR_INVALID;
    c->train_folded_tail = on != 0;
    return VQHIP_OK;
}

// test hook: training-mode forward only (activations stay in the workspaces for vqhip_debug_fetch)
int vqhip_fulltrain_forward_device(vqhip_codec* c, const float* d_leaves, int64_t n, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!c->full_training) return fail(c, VQHIP_ERR_INVALID, "fulltrain_forward: call vqhip_fulltrain_begin first");
    if (!d_leaves || n < 1 || n > c->chunk) return fail(c, VQHIP_ERR_INVALID, "fulltrain_forward: null pointer or n_leaves outside [1, chunk]");
    HIPCHK(c, hipSetDevice(c->device));
    return fulltrain_forward(c, d_leaves, n, stream ? (hipStream_t)stream : c->stream);
}

// forward + backward of this rank's batch.  grads_dev: flat gradient vector; aux_dev (may be NULL): the VQ statistics of
// vqhip_train_vq_stats_device followed by { sum (recon-x)^2, sum |recon-x|, voxels } of this rank.
int vqhip_fulltrain_fwdbwd_device(vqhip_codec* c, const float* d_leaves, int64_t n, int64_t n_global, float* d_grads, float* d_aux, void* stream)
{
    return vqhip_fulltrain_fwdbwd_overlap_device(c, d_leaves, n, n_global, d_grads, d_aux, stream, nullptr, nullptr);
}

// ... with a hook between the two halves of the backward pass: `decoder_done(user)` is called on the calling thread right after the
// decoder's backward kernels have been ENQUEUED (nothing is synchronised).  At that point of the stream the decoder's slice of the
// gradient vector — everything from vqhip_fulltrain_decoder_offset() on — is final, so a data-parallel caller records an event there
// and all-reduces that slice on another stream while the encoder half of the backward pass runs (vqvdb_amd/full_training.py).
int vqhip_fulltrain_fwdbwd_overlap_device(vqhip_codec* c, const float* d_leaves, int64_t n, int64_t n_global, float* d_grads, float* d_aux, void* stream,
                                          vqhip_phase_fn decoder_done, void* user)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!c->full_training) return fail(c, VQHIP_ERR_INVALID, "fulltrain_fwdbwd: call vqhip_fulltrain_begin first");
    if (!d_leaves || !d_grads || n < 1 || n > c->chunk || n_global < n) return fail(c, VQHIP_ERR_INVALID, "fulltrain_fwdbwd: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    bool ema_done = false;
    int rc = fulltrain_forward(c, d_leaves, n, s, d_aux, &ema_done);
    if (rc) return rc;
    const int nt = (int)((n + 31) / 32);
    Launcher L{c, s, n};
    Bwd B{c, L, s, nt, d_grads, {}};
    if ((rc = ensure_parts(c, nt, B.pb))) return rc;
    if ((rc = side_stream(c, s, B.ws))) return rc;
    B.rs = s;
    if (B.ws != s && c->train_red_stream && !c->train_red_deferred && c->ft_red) {
        const bool own = c->train_red_prio ? c->train_red_prio > 0 : n <= c->train_red_own_leaves;
        B.rs = own ? c->ft_red : c->ft_red_shared;
    }
    HIPCHK(c, hipMemsetAsync(d_grads, 0, c->h_params.size() * sizeof(float), s));
    if (d_aux) {
        // codebook statistics of this batch (same kernels as stage 1) and the reconstruction-loss sums
        const int64_t rows = n * 64;
        const int n_seg = (int)((rows + VQ_SEG_ROWS - 1) / VQ_SEG_ROWS);
        if (int rc = ensure(c, c->tr_part, ema_scratch_bytes(n_seg), "the codebook statistics partials")) return rc;
        if (int rc = ensure(c, c->tr_loss_part, (size_t)RL_BLOCKS * 2, "the loss partials")) return rc;
        // (second stream: nothing in the backward pass needs them; Bwd::join at the end of the step covers them)
        hipStream_t ws = B.ws;
        B.fork();
        L.run_on(ws, ema_done ? "ft_loss_sums" : "ft_vq_stats", [&] {
            if (!ema_done) launch_vq_ema(c, ws, c->tr_z, c->tr_idx, rows, n_seg, d_aux);
            hipLaunchKernelGGL(loss_sums_k, dim3(RL_BLOCKS), dim3(256), 0, ws, c->act["xt"], c->act["t_recon"], n, nt, c->tr_loss_part);
            hipLaunchKernelGGL(recon_loss_reduce_k, dim3(1), dim3(1), 0, ws, c->tr_loss_part, n * 512, d_aux + VQ_STATS_FLOATS);
        });
    }
    // An error exit after work has been put on the side stream must not return while that stream may still write grads_dev / aux_dev or
    // read the workspaces (the regular exit orders the caller's stream after it with Bwd::join): wait for it, then report.
    auto bail = [&](int code) {
        if (B.ws && B.ws != s) (void)hipStreamSynchronize(B.ws);
        if (B.third()) (void)hipStreamSynchronize(B.rs);
        return code;
    };
    const double nvox = (double)n_global * 512.0;
    if ((rc = fulltrain_backward_decoder(B, n, (float)(1.6 / nvox), (float)(0.2 / nvox)))) return bail(rc);
    // the caller ships the decoder's gradients now: from the second stream (vqhip_fulltrain_ready_stream), which is first ordered after the
    // decoder's kernels of this stream (GroupNorm-affine and attention gradients are written here) — the chain itself does not wait
    if (decoder_done) {
        B.flush_deferred();   // the decoder's bias / affine / attention-weight gradients: complete on the chain's stream from here
        B.fork_mark = -1, B.fork();
        if (B.third()) B.link(B.rs, B.ws);   // the decoder's bias / affine / attention-weight gradients come from the reduction stream
    }
    if (decoder_done && decoder_done(user) != 0) return bail(fail(c, VQHIP_ERR_INVALID, "fulltrain_fwdbwd: the decoder_done callback failed"));
    rc = fulltrain_backward_encoder(B, n, (float)(2.0 * 0.25 / ((double)n_global * 64.0 * 128.0)));
    return rc ? bail(rc) : VQHIP_OK;
}

// the stream on which the decoder's gradients are complete at the decoder_done callback (NULL: the caller's own stream)
void* vqhip_fulltrain_ready_stream(const vqhip_codec* c) { return c && c->train_side_stream ? (void*)c->ft_side : nullptr; }

// first element of the decoder's parameters in the flat vector (the reference's parameter order: encoder, then decoder)
int64_t vqhip_fulltrain_decoder_offset(const vqhip_codec* c)
{
    if (!c) return -1;
    auto it = c->p_off.find("decoder.stem.0.weight");
    return it == c->p_off.end() ? -1 : it->second.first;
}

// Optimizer step from the (all-reduced) gradients and statistics: AdamW on the parameters (python/training.py:104), EMA on the
// codebook (VQVAE_v2.py:133-144), then every device table that derives from them is rebuilt.  step counts from 1.
int vqhip_fulltrain_apply_device(vqhip_codec* c, const float* d_grads, const float* d_aux, float lr, int64_t step, float beta1, float beta2, float adam_eps,
                                 float weight_decay, float ema_decay, float ema_eps, void* stream)
{
    if (!c) return VQHIP_ERR_INVALID;
    if (!c->full_training) return fail(c, VQHIP_ERR_INVALID, "fulltrain_apply: call vqhip_fulltrain_begin first");
    if (!d_grads || step < 1 || !(lr >= 0.0f)) return fail(c, VQHIP_ERR_INVALID, "fulltrain_apply: null gradients, step < 1 or negative learning rate");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const int64_t np = (int64_t)c->h_params.size();
    const float bc1 = (float)(1.0 - std::pow((double)beta1, (double)step)), bc2s = (float)std::sqrt(1.0 - std::pow((double)beta2, (double)step));
    Launcher L{c, s, 0};
    L.run("ft_adamw", [&] { hipLaunchKernelGGL(adamw_k, dim3(1024), dim3(256), 0, s, c->ft_P, d_grads, c->ft_M, c->ft_V, np, lr, beta1, beta2, adam_eps, weight_decay, bc1, bc2s); });
    if (d_aux) {
        const float alpha = (float)(1.0 - (double)ema_decay);
        L.run("ft_vq_ema_update", [&] {
            hipLaunchKernelGGL(vq_ema_update_k, dim3(256), dim3(128), 0, s, d_aux, ema_decay, alpha, ema_eps, c->dw["tr.cs"], c->dw["tr.avg"], c->dw["cb"]);
        });
    }
    if (L.rc) return L.rc;
    int rc = refrag_all(c, s);
    c->tables_stale = true, c->weights_stale = true;
    return rc;
}

int vqhip_fulltrain_get_params(vqhip_codec* c, float* params)
{
    if (!c || !params) return VQHIP_ERR_INVALID;
    if (!c->full_training) return fail(c, VQHIP_ERR_INVALID, "fulltrain_get_params: call vqhip_fulltrain_begin first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(params, c->ft_P, c->h_params.size() * sizeof(float), hipMemcpyDeviceToHost));
    return VQHIP_OK;
}

int vqhip_fulltrain_set_params(vqhip_codec* c, const float* params)
{
    if (!c || !params) return VQHIP_ERR_INVALID;
    if (!c->full_training) return fail(c, VQHIP_ERR_INVALID, "fulltrain_set_params: call vqhip_fulltrain_begin first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(c->ft_P, params, c->h_params.size() * sizeof(float), hipMemcpyHostToDevice));
    int rc = refrag_all(c, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tables_stale = true, c->weights_stale = true;
    return rc;
}

// AdamW moments (exp_avg | exp_avg_sq, each param_count floats, the flat parameter order) for checkpoints: a resumed run
// continues the optimizer exactly like the reference's checkpoint does (training.py:216-226); the step count / schedule
// position lives on the host (vqvdb_amd/full_training.py).
int vqhip_fulltrain_get_opt_state(vqhip_codec* c, float* exp_avg, float* exp_avg_sq)
{
    if (!c || !exp_avg || !exp_avg_sq) return VQHIP_ERR_INVALID;
    if (!c->full_training) return fail(c, VQHIP_ERR_INVALID, "fulltrain_get_opt_state: call vqhip_fulltrain_begin first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(exp_avg, c->ft_M, c->h_params.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(exp_avg_sq, c->ft_V, c->h_params.size() * sizeof(float), hipMemcpyDeviceToHost));
    return VQHIP_OK;
}

int vqhip_fulltrain_set_opt_state(vqhip_codec* c, const float* exp_avg, const float* exp_avg_sq)
{
    if (!c || !exp_avg || !exp_avg_sq) return VQHIP_ERR_INVALID;
    if (!c->full_training) return fail(c, VQHIP_ERR_INVALID, "fulltrain_set_opt_state: call vqhip_fulltrain_begin first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(c->ft_M, exp_avg, c->h_params.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->ft_V, exp_avg_sq, c->h_params.size() * sizeof(float), hipMemcpyHostToDevice));
    return VQHIP_OK;
}

}  // extern "C"
