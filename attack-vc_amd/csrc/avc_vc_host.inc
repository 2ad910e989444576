// libavc host side of the voice-conversion path (included at the end of avc_api.hip):
// ContentEncoder + Decoder weights, the e2e / feedback attack loops and inference.
//
//   e2e iteration (attack_utils.py:39-46):
//     se_fwd_fused(adv) -> se_head_v(fwd) -> dense(cond) -> dec_fwd_fused(+ loss, d/d out)
//     -> dec_bwd_fused -> dense^T(d/d emb) -> se_head_v(bwd from d/d emb) -> se_bwd_fused(+Adam)
//   fb iteration (attack_utils.py:121-128): the same, with the decoder output fed through a
//   second SpeakerEncoder pass (fwd, loss vs tgt/org embeddings, bwd to d/d out) in between.
// The ContentEncoder output mu = CE(vc_src) is constant over the attack: computed once.

namespace {

struct VcWs {
    int B = 0, T = 0, Ts = 0;            // attacked (SpeakerEncoder) length T, source length Ts
    int Tce = 0, Tn = 0;                 // Ts -> ContentEncoder length Tce -> Decoder output Tn
    std::vector<int> Tl_ce, Tl_dec, Tl_se2;
    DevBuf src, mu, emb, cond, gcond, gemb, stash, invstd, out, tgt_out, org_out, gout, gdec, pooled2, gpooled2;
    DevBuf lsig;                          // ContentEncoder.forward's log_sigma (std_layer), on demand
    DevBuf hact;                          // fused head: SE(adv)'s dense activations [B][2nd][C] (mode 0 -> 3)
    DevPtr<unsigned long long> masks2;
    bool ce_long = false, dec_long = false, se2_long = false;   // long engine for these lengths
    LongScratch lz;                       // their scratch (max(Ts, Tn) frames) + SE2's ballot masks
    int stash_per_utt = 0;
    std::vector<int> stash_off;
    size_t S = 0, O = 0;                  // floats of the source array (B x 80 x Ts) and of an output-sized one
                                          // (B x 80 x Tn), or their packed sums
    // ragged batch (avc_*_attack_ragged / avc_inference_ragged): utterance b has its own source length, every
    // array is packed blocks, every component runs on the long engine (scratch sized for the longest)
    bool ragged = false;
    DevPtr<RagUtt> rag_ce, rag_se2;       // ContentEncoder (Ts_b, source / mu offsets), SE over the decoder output (Tn_b)
    DevPtr<DecUtt> rag_dec;
    double fl_ce = 0, fl_se2 = 0, fl_dec[2] = {0, 0};   // algorithmic FLOPs over the batch (dec: fwd, bwd)
    int ws_gen = -1;                      // SpeakerEncoder workspace generation the plans point into
    struct Plans {                        // rebuilt whenever the SpeakerEncoder workspace is re-planned (renew)
        Plan ce, ce_std, dec_pre, se2_pre;
        Plan it[2][2];                    // [e2e | fb][PREC]
        GraphExec graph[2][2];
    } pl;                                 // last: destroyed before the buffers its launches point into
};

}  // namespace

struct VcState {
    avc_vc_cfg cfg{};
    avc_se_cfg ce{};                      // the ContentEncoder as an encoder config
    std::vector<int> ce_bank_k;
    FusedW cew[2];                        // ContentEncoder A operands (+ mean_layer)
    FusedW cew_std[2];                    // the same with std_layer in mean_layer's place (log_sigma)
    DecW dw[2];                           // Decoder A operands
    DevBuf aff, affT, aff_b;              // conv_affine stacked [2n*256][128], its transpose, bias
    std::deque<DevBuf> own;               // biases
    // spectral norm (cfg.dec_sn): weight_orig of every layer [h][w], its u / v, sigma, and the chunks
    // of every packed copy (per precision) that sn_scale rewrites as weight_orig / sigma
    std::vector<SnLayer> sn_layers;
    std::vector<SnChunk> sn_chunks[2];
    DevBuf sn_raw, sn_uv, sn_sigma, sn_layer_dev, sn_chunk_dev[2], sn_train;   // sn_train: 1 int (SnArgs.train)
    size_t sn_uv_count = 0;
    // workspaces by VcKey {B, T, Ts, ce_long, dec_long, lens, src_lens}, most recently used first; each one's plans
    // point into the SpeakerEncoder workspace whose gen they record (ws_gen)
    LruCache<VcKey, VcWs> wss;
    VcWs* cur = nullptr;
};

// (callers have the device current and the stream drained)
static void vc_free(avc_ctx* ctx) {
    if (!ctx->vc) return;
    ctx->n_vc_evictions += ctx->vc->wss.evictions;
    delete ctx->vc;
    ctx->vc = nullptr;
}
static long vc_evictions(avc_ctx* ctx) { return ctx->vc ? ctx->vc->wss.evictions : 0; }

static avc_se_cfg ce_as_encoder(const avc_vc_cfg& v) {
    avc_se_cfg c{};
    c.c_in = v.ce_c_in;
    c.c_h = v.ce_c_h;
    c.c_out = v.ce_c_out;
    c.kernel_size = v.ce_kernel_size;
    c.bank_size = v.ce_bank_size;
    c.bank_scale = v.ce_bank_scale;
    c.c_bank = v.ce_c_bank;
    c.n_conv_blocks = v.ce_n_conv_blocks;
    c.n_dense_blocks = 0;
    for (int l = 0; l < AVC_MAX_BLOCKS; ++l) c.subsample[l] = v.ce_subsample[l];
    c.act = v.ce_act;
    return c;
}

static size_t vc_weight_count(const avc_vc_cfg& v) {
    size_t n = 0;
    for (int k = v.ce_bank_scale; v.ce_bank_scale > 0 && k <= v.ce_bank_size; k += v.ce_bank_scale)
        n += (size_t)v.ce_c_bank * v.ce_c_in * k + v.ce_c_bank;
    const int nbk = v.ce_bank_scale > 0 ? v.ce_bank_size / v.ce_bank_scale : 0;
    n += (size_t)v.ce_c_h * (v.ce_c_bank * nbk + v.ce_c_in) + v.ce_c_h;
    n += 2 * (size_t)v.ce_n_conv_blocks * ((size_t)v.ce_c_h * v.ce_c_h * v.ce_kernel_size + v.ce_c_h);
    n += 2 * ((size_t)v.ce_c_out * v.ce_c_h + v.ce_c_out);   // mean_layer, std_layer
    const size_t H = v.dec_c_h;
    n += H * v.dec_c_in + H;
    for (int l = 0; l < v.dec_n_conv_blocks; ++l) n += H * H * v.dec_kernel_size + H;
    for (int l = 0; l < v.dec_n_conv_blocks; ++l)
        n += H * v.dec_upsample[l] * H * v.dec_kernel_size + H * v.dec_upsample[l];
    n += 2 * (size_t)v.dec_n_conv_blocks * (2 * H * v.dec_c_cond + 2 * H);
    n += (size_t)v.dec_c_out * H + v.dec_c_out;
    return n;
}

extern "C" size_t avc_vc_weight_count(const avc_vc_cfg* cfg) { return cfg ? vc_weight_count(*cfg) : 0; }

static int vc_cfg_check(const avc_vc_cfg& v) {
    if (v.ce_n_conv_blocks < 0 || v.ce_n_conv_blocks > AVC_MAX_BLOCKS || v.dec_n_conv_blocks < 1 ||
        v.dec_n_conv_blocks > AVC_MAX_BLOCKS)
        return fail("avc_attach_vc: block counts out of range");
    if (!fused_cfg_ok(ce_as_encoder(v)))
        return fail("avc_attach_vc: the ContentEncoder needs c_in=80, c_h=c_bank=c_out=128, bank_scale=1, "
                    "bank_size<=8, odd kernel_size<=5, 1..8 conv blocks with subsample 1|2");
    if (v.ce_act != 0 && v.ce_act != 1) return fail("avc_attach_vc: ce_act must be 0 or 1");
    if (v.dec_c_in != FZ_C || v.dec_c_cond != FZ_C || v.dec_c_h != FZ_C || v.dec_c_out != DZ_COUT)
        return fail("avc_attach_vc: the Decoder needs c_in = c_cond = c_h = 128 and c_out = 80");
    if (v.dec_kernel_size % 2 == 0 || v.dec_kernel_size > 5)
        return fail("avc_attach_vc: the Decoder needs an odd kernel_size <= 5");
    if (v.dec_n_conv_blocks > DZ_MAXBLK) return fail("avc_attach_vc: at most %d Decoder blocks", DZ_MAXBLK);
    for (int l = 0; l < v.dec_n_conv_blocks; ++l)
        if (v.dec_upsample[l] != 1 && v.dec_upsample[l] != 2)
            return fail("avc_attach_vc: Decoder upsample must be 1 or 2 (block %d: %d)", l, v.dec_upsample[l]);
    if (v.dec_act != 0 && v.dec_act != 1) return fail("avc_attach_vc: dec_act must be 0 or 1");
    return 0;
}

extern "C" int avc_attach_vc(avc_ctx* ctx, const avc_vc_cfg* cfgp, const float* w, size_t n_weights) {
    if (!ctx || !cfgp || !w) return fail("avc_attach_vc: null argument");
    const avc_vc_cfg& v = *cfgp;
    if (vc_cfg_check(v)) return 1;
    if (!ctx->fused_ok) return fail("avc_attach_vc: the SpeakerEncoder of this context is not fused-capable");
    if (n_weights != vc_weight_count(v))
        return fail("avc_attach_vc: got %zu weights, config needs %zu", n_weights, vc_weight_count(v));
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    vc_free(ctx);
    VcState* S = new VcState();
    ctx->vc = S;
    S->wss.tag = "vc";
    S->wss.trace = debug_ws();
    S->cfg = v;
    S->ce = ce_as_encoder(v);
    const avc_se_cfg& ce = S->ce;
    for (int k = ce.bank_scale; k <= ce.bank_size; k += ce.bank_scale) S->ce_bank_k.push_back(k);
    const int nb = (int)S->ce_bank_k.size(), C = FZ_C, ks = ce.kernel_size;
    int rc = 0;
    auto dev = [&](const float* h, size_t n) -> const float* {
        S->own.emplace_back();
        rc |= upload(S->own.back(), std::vector<float>(h, h + n));
        return S->own.back().p;
    };

    // ---- ContentEncoder (state_dict order, models.py:157-180)
    const float* p = w;
    std::vector<HostConv> bank(nb), c1(ce.n_conv_blocks), c2(ce.n_conv_blocks);
    FzBias fb;
    for (int i = 0; i < nb; ++i) {
        bank[i] = {ce.c_bank, ce.c_in, S->ce_bank_k[i], p, nullptr};
        p += (size_t)ce.c_bank * ce.c_in * S->ce_bank_k[i];
        bank[i].b = p;
        fb.bank.push_back(dev(p, ce.c_bank));
        p += ce.c_bank;
    }
    const int cat = ce.c_bank * nb + ce.c_in;
    HostConv inc{ce.c_h, cat, 1, p, nullptr};
    p += (size_t)ce.c_h * cat;
    inc.b = p;
    fb.in = dev(p, ce.c_h);
    p += ce.c_h;
    for (auto* vec : {&c1, &c2})
        for (int l = 0; l < ce.n_conv_blocks; ++l) {
            (*vec)[l] = {C, C, ks, p, nullptr};
            p += (size_t)C * C * ks;
            (*vec)[l].b = p;
            (vec == &c1 ? fb.c1 : fb.c2).push_back(dev(p, C));
            p += C;
        }
    const float* meanW = p;
    p += (size_t)ce.c_out * C;
    const float* meanB = dev(p, ce.c_out);
    p += ce.c_out;
    // std_layer: log_sigma, unused by inference() (models.py:472-489); ContentEncoder.forward
    // returns it (models.py:208-210)
    const float* stdW = p;
    p += (size_t)ce.c_out * C;
    const float* stdB = dev(p, ce.c_out);
    p += ce.c_out;
    if (!rc) rc |= pack_fused(ctx, S->cew, bank, inc, c1, c2, fb);
    for (int prec = 0; prec < 2 && !rc; ++prec) {
        rc |= fz_pack(ctx, prec, C, C, [&](int m, int k) { return meanW[(size_t)m * C + k]; }, S->cew[prec].mean_w);
        S->cew[prec].b_mean = meanB;
        S->cew_std[prec] = S->cew[prec];
        rc |= fz_pack(ctx, prec, C, C, [&](int m, int k) { return stdW[(size_t)m * C + k]; }, S->cew_std[prec].mean_w);
        S->cew_std[prec].b_mean = stdB;
    }

    // ---- Decoder (models.py:380-399)
    const int nd = v.dec_n_conv_blocks, kd = v.dec_kernel_size;
    // spectral norm: layer ids in module order (in, first_conv[l], second_conv[l], conv_affine[q], out),
    // their weight_orig matrices and u / v offsets
    const bool sn = v.dec_sn != 0;
    std::vector<float> sn_raw;
    auto sn_layer = [&](const float* W, int h, int wd) {
        if (!sn) return;
        SnLayer L{h, wd, (int64_t)sn_raw.size(), (int64_t)S->sn_uv_count, (int64_t)S->sn_uv_count + h};
        sn_raw.insert(sn_raw.end(), W, W + (size_t)h * wd);
        S->sn_uv_count += (size_t)h + wd;
        S->sn_layers.push_back(L);
    };
    auto sn_chunks = [&](int prec, const void* dst, const float* src, size_t n, int layer, bool bf16) {
        for (size_t e = 0; e < n; e += SN_CHUNK)
            S->sn_chunks[prec].push_back(SnChunk{(char*)const_cast<void*>(dst) + e * (bf16 ? 2 : 4), src + e,
                                                 (int32_t)std::min<size_t>(SN_CHUNK, n - e), layer, bf16 ? 1 : 0, 0});
    };
    const int L_IN = 0, L_C1 = 1, L_C2 = 1 + nd, L_AFF = 1 + 2 * nd, L_OUT = 1 + 4 * nd;
    (void)L_IN;
    const float* inW = p;
    p += (size_t)C * C;
    const float* inB = dev(p, C);
    p += C;
    sn_layer(inW, C, C);
    std::vector<const float*> w1(nd), w2(nd);
    std::vector<const float*> b1(nd);
    std::vector<std::array<const float*, 2>> b2(nd);
    for (int l = 0; l < nd; ++l) {
        w1[l] = p;
        sn_layer(p, C, C * kd);
        p += (size_t)C * C * kd;
        b1[l] = dev(p, C);
        p += C;
    }
    for (int l = 0; l < nd; ++l) {
        const int up = v.dec_upsample[l];
        w2[l] = p;
        sn_layer(p, up * C, C * kd);
        p += (size_t)up * C * C * kd;
        for (int s = 0; s < up; ++s) {   // half s: bias of channels up*c + s
            std::vector<float> h(C);
            for (int c = 0; c < C; ++c) h[c] = p[up * c + s];
            b2[l][s] = dev(h.data(), C);
        }
        if (up == 1) b2[l][1] = b2[l][0];
        p += (size_t)up * C;
    }
    {   // conv_affine_layers: [2nd][256][128] stacked row-major, its transpose, bias
        const int M = 2 * nd * 2 * C;
        std::vector<float> A((size_t)M * C), At((size_t)C * M), bb(M);
        for (int q = 0; q < 2 * nd; ++q) {
            sn_layer(p, 2 * C, C);
            for (int r = 0; r < 2 * C; ++r)
                for (int k = 0; k < C; ++k) {
                    const float x = p[(size_t)r * C + k];
                    A[(size_t)(q * 2 * C + r) * C + k] = x;
                    At[(size_t)k * M + q * 2 * C + r] = x;
                }
            p += (size_t)2 * C * C;
            for (int r = 0; r < 2 * C; ++r) bb[q * 2 * C + r] = p[r];
            p += 2 * C;
        }
        rc |= upload(S->aff, A);
        rc |= upload(S->affT, At);
        rc |= upload(S->aff_b, bb);
        if (sn && !rc) {   // pristine copies of both layouts; chunks per layer (rows of A, columns of At)
            S->own.emplace_back();
            rc |= upload(S->own.back(), A);
            const float* sa = S->own.back().p;
            S->own.emplace_back();
            rc |= upload(S->own.back(), At);
            const float* st = S->own.back().p;
            for (int prec = 0; prec < 2; ++prec)
                for (int q = 0; q < 2 * nd; ++q) {
                    const size_t o = (size_t)q * 2 * C * C;
                    sn_chunks(prec, S->aff.p + o, sa + o, (size_t)2 * C * C, L_AFF + q, false);
                    for (int k = 0; k < C; ++k) {
                        const size_t ot = (size_t)k * M + (size_t)q * 2 * C;
                        sn_chunks(prec, S->affT.p + ot, st + ot, (size_t)2 * C, L_AFF + q, false);
                    }
                }
        }
    }
    const float* outW = p;
    sn_layer(outW, DZ_COUT, C);
    p += (size_t)DZ_COUT * C;
    const float* outB = dev(p, DZ_COUT);
    p += DZ_COUT;
    if ((size_t)(p - w) != n_weights) rc |= fail("avc_attach_vc: internal weight walk mismatch");
    for (int prec = 0; prec < 2 && !rc; ++prec) {
        DecW& D = S->dw[prec];
        // one packed copy of layer `layer`; with spectral norm also its fp32 twin and rescale chunks
        auto pk = [&](int M, int K, auto get, const void*& dst, int layer) {
            const float* shadow = nullptr;
            size_t n = 0;
            const int r = fz_pack(ctx, prec, M, K, get, dst, sn ? &shadow : nullptr, &n);
            if (!r && sn) sn_chunks(prec, dst, shadow, n, layer, prec == PREC_BF16);
            return r;
        };
        rc |= pk(C, C, [&](int m, int k) { return inW[(size_t)m * C + k]; }, D.in, L_IN);
        rc |= pk(DZ_COUT, C, [&](int m, int k) { return outW[(size_t)m * C + k]; }, D.out, L_OUT);
        rc |= pk(C, DZ_COUT, [&](int m, int k) { return outW[(size_t)k * C + m]; }, D.outT, L_OUT);
        for (int l = 0; l < nd; ++l) {
            const float* W1 = w1[l];
            const float* W2 = w2[l];
            const int up = v.dec_upsample[l];
            // forward: A[co][j*128 + ci] = W[co][ci][j];  dgrad: A[ci][j*128 + co] = W[co][ci][j]
            rc |= pk(C, kd * C, [&](int m, int k) { return W1[((size_t)m * C + k % C) * kd + k / C]; }, D.c1[l], L_C1 + l);
            rc |= pk(C, kd * C, [&](int m, int k) { return W1[((size_t)(k % C) * C + m) * kd + k / C]; }, D.c1T[l],
                     L_C1 + l);
            for (int s = 0; s < up; ++s) {
                rc |= pk(C, kd * C, [&](int m, int k) { return W2[((size_t)(up * m + s) * C + k % C) * kd + k / C]; },
                         D.c2[l][s], L_C2 + l);
                rc |= pk(C, kd * C, [&](int m, int k) { return W2[((size_t)(up * (k % C) + s) * C + m) * kd + k / C]; },
                         D.c2T[l][s], L_C2 + l);
            }
            if (up == 1) {
                D.c2[l][1] = D.c2[l][0];
                D.c2T[l][1] = D.c2T[l][0];
            }
            D.b_c1[l] = b1[l];
            D.b_c2[l][0] = b2[l][0];
            D.b_c2[l][1] = b2[l][1];
        }
        D.b_in = inB;
        D.b_out = outB;
    }
    if (sn && !rc) {
        std::vector<float> uv0(S->sn_uv_count, 0.f);   // set by avc_set_sn_state before use
        rc |= upload(S->sn_raw, sn_raw);
        rc |= upload(S->sn_uv, uv0);
        rc |= upload(S->sn_sigma, std::vector<float>(S->sn_layers.size(), 1.f));
        rc |= upload_pod(S->sn_train, std::vector<int>{1});   // train mode until avc_set_sn_train says otherwise
        rc |= upload_pod(S->sn_layer_dev, S->sn_layers);
        for (int prec = 0; prec < 2; ++prec) rc |= upload_pod(S->sn_chunk_dev[prec], S->sn_chunks[prec]);
        for (const SnLayer& L : S->sn_layers)
            if (L.h > SN_MAXDIM || L.w > SN_MAXDIM) rc |= fail("avc_attach_vc: spectral-norm layer %dx%d too large", L.h, L.w);
    }
    if (!rc) {
        const std::pair<const void*, int> fns[] = {
            {(const void*)dec_fwd_fused<PREC_F32, 0>, dz_lds_fwd(PREC_F32, 128, 5)},
            {(const void*)dec_fwd_fused<PREC_F32, 8>, dz_lds_fwd(PREC_F32, 128, 5)},
            {(const void*)dec_fwd_fused<PREC_BF16, 0>, dz_lds_fwd(PREC_BF16, 128, 5)},
            {(const void*)dec_fwd_fused<PREC_BF16, 8>, dz_lds_fwd(PREC_BF16, 128, 5)},
            {(const void*)dec_bwd_fused<PREC_F32, 0>, dz_lds_bwd(PREC_F32, 128)},
            {(const void*)dec_bwd_fused<PREC_F32, 8>, dz_lds_bwd(PREC_F32, 128)},
            {(const void*)dec_bwd_fused<PREC_BF16, 0>, dz_lds_bwd(PREC_BF16, 128)},
            {(const void*)dec_bwd_fused<PREC_BF16, 8>, dz_lds_bwd(PREC_BF16, 128)},
        };
        for (auto& fn : fns) {
            const hipError_t e = hipFuncSetAttribute(fn.first, hipFuncAttributeMaxDynamicSharedMemorySize, fn.second);
            if (e != hipSuccess) {
                rc |= fail("avc_attach_vc: %s", hipGetErrorString(e));
                break;
            }
        }
    }
    if (rc) {
        vc_free(ctx);
        return 1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------
// lengths, launches and plans
// ---------------------------------------------------------------------------------
// encoder block lengths for T input frames (ceil-mode pooling; torch's reflect pad < length)
static int enc_lengths(const avc_se_cfg& c, const std::vector<int>& bank_k, int T, std::vector<int>& Tl) {
    Tl.assign(1, T);
    int maxpad = 0;
    for (int k : bank_k) {
        int a, b;
        pads_of(k, a, b);
        maxpad = std::max(maxpad, std::max(a, b));
    }
    if (T <= maxpad) return fail("T=%d too short for the conv bank reflect padding (%d)", T, maxpad);
    int kpl, kpr;
    pads_of(c.kernel_size, kpl, kpr);
    for (int l = 0; l < c.n_conv_blocks; ++l) {
        if (Tl.back() <= std::max(kpl, kpr))
            return fail("T=%d too short: conv block %d input has %d frames", T, l, Tl.back());
        Tl.push_back(cdiv(Tl.back(), c.subsample[l]));
    }
    return 0;
}

static int dec_lengths(const avc_vc_cfg& v, int T0, std::vector<int>& Tl) {
    Tl.assign(1, T0);
    for (int l = 0; l < v.dec_n_conv_blocks; ++l) {
        if (Tl.back() <= v.dec_kernel_size / 2)
            return fail("Decoder block %d input has %d frames (reflect pad %d)", l, Tl.back(), v.dec_kernel_size / 2);
        Tl.push_back(Tl.back() * v.dec_upsample[l]);
    }
    return 0;
}

static int vc_out_frames(avc_ctx* ctx, int T, int* Tn) {
    if (!ctx->vc) return fail("no ContentEncoder/Decoder attached (avc_attach_vc)");
    std::vector<int> a, b;
    if (enc_lengths(ctx->vc->ce, ctx->vc->ce_bank_k, T, a) || dec_lengths(ctx->vc->cfg, a.back(), b)) return 1;
    *Tn = b.back();
    return 0;
}

extern "C" size_t avc_sn_state_count(avc_ctx* ctx) {
    return ctx && ctx->vc && ctx->vc->cfg.dec_sn ? ctx->vc->sn_uv_count : 0;
}

static int sn_state_io(avc_ctx* ctx, float* host, size_t n, bool set) {
    const char* nm = set ? "avc_set_sn_state" : "avc_get_sn_state";
    if (!ctx || !host) return fail("%s: null argument", nm);
    if (!ctx->vc || !ctx->vc->cfg.dec_sn) return fail("%s: the attached Decoder has no spectral norm", nm);
    if (n != ctx->vc->sn_uv_count) return fail("%s: got %zu floats, the Decoder's u / v hold %zu", nm, n, ctx->vc->sn_uv_count);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (set) HIPCHK(hipMemcpy(ctx->vc->sn_uv.p, host, n * sizeof(float), hipMemcpyHostToDevice));
    else HIPCHK(hipMemcpy(host, ctx->vc->sn_uv.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int avc_set_sn_state(avc_ctx* ctx, const float* uv, size_t n) {
    return sn_state_io(ctx, const_cast<float*>(uv), n, true);
}
extern "C" int avc_get_sn_state(avc_ctx* ctx, float* uv, size_t n) { return sn_state_io(ctx, uv, n, false); }

// The same state as a DEVICE buffer, copied on the caller's stream (no host round trip, no synchronisation):
// set = 1 loads uv into the Decoder's u / v, set = 0 stores them into uv.
extern "C" int avc_sn_state_dev(avc_ctx* ctx, float* uv, size_t n, int set, void* stream) {
    const char* nm = "avc_sn_state_dev";
    if (!ctx || !uv) return fail("%s: null argument", nm);
    if (!ctx->vc || !ctx->vc->cfg.dec_sn) return fail("%s: the attached Decoder has no spectral norm", nm);
    if (n != ctx->vc->sn_uv_count) return fail("%s: got %zu floats, the Decoder's u / v hold %zu", nm, n, ctx->vc->sn_uv_count);
    hipStream_t us = (hipStream_t)stream;
    if (begin_call(ctx, us)) return 1;
    if (set) HIPCHK(hipMemcpyAsync(ctx->vc->sn_uv.p, uv, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    else HIPCHK(hipMemcpyAsync(uv, ctx->vc->sn_uv.p, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return end_call(ctx, us);
}

// torch's spectral_norm hook in train mode (1: one power iteration per forward, u / v updated) or eval
// mode (0: sigma from the stored u / v, nothing updated), as the Decoder module's .training says
extern "C" int avc_set_sn_train(avc_ctx* ctx, int train, void* stream) {
    if (!ctx) return fail("avc_set_sn_train: null context");
    if (!ctx->vc || !ctx->vc->cfg.dec_sn) return fail("avc_set_sn_train: the attached Decoder has no spectral norm");
    hipStream_t us = (hipStream_t)stream;
    if (begin_call(ctx, us)) return 1;
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctx->vc->sn_train.p), train ? 1 : 0, 1, ctx->stream));
    return end_call(ctx, us);
}

extern "C" int avc_vc_out_frames(avc_ctx* ctx, int T) {
    int Tn = -1;
    if (!ctx || vc_out_frames(ctx, T, &Tn)) return -1;
    return Tn;
}

static int dec_shape(const avc_vc_cfg& v, int T0) {
    bool std_cfg = T0 == 16 && v.dec_n_conv_blocks == 6 && v.dec_kernel_size == 5 && v.dec_act == 0;
    for (int l = 0; std_cfg && l < 6; ++l)
        if (v.dec_upsample[l] != ((l & 1) ? 1 : 2)) std_cfg = false;
    return (std_cfg && !env_is("AVC_FUSED_STD", '0')) ? 0 : 8;
}

static FusedArgs enc_args(const avc_se_cfg& c, int nb, int B, const std::vector<int>& Tl, const FusedW& w) {
    FusedArgs A{};
    A.B = B;
    A.T = Tl[0];
    A.nb = nb;
    A.ks = c.kernel_size;
    A.nblk = c.n_conv_blocks;
    A.act = c.act;
    for (int l = 0; l < c.n_conv_blocks; ++l) A.sub[l] = c.subsample[l];
    for (int l = 0; l <= c.n_conv_blocks; ++l) A.Tl[l] = Tl[l];
    A.w = w;
    return A;
}

// one encoder pass: the fused kernel, or the long kernel with scratch `lz` (non-null)
static Launch enc_launch(int kind, int prec, const FusedArgs& A, int shape, int ks, double flop, const char* what,
                         const LongArgs* lz = nullptr) {
    Launch L;
    L.kind = kind;
    L.prec = prec;
    L.grid = dim3(A.B);
    L.block = dim3(256);
    L.shmem = kind == L_FZ_FWD ? fz_lds_fwd(prec, A.T, ks)
                               : fz_lds_bwd_launch(prec, shape == 16 ? 128 : A.T, shape, A.mask_words);   // (SH = 16: 128-frame layout)
    L.fz = A;
    L.fz_shape = shape;
    L.flop = flop;
    L.name = std::string(kind == L_FZ_FWD ? "se_fwd_fused" : "se_bwd_fused") + (prec == PREC_F32 ? "<f32>" : "<bf16>");
    if (lz) {
        L.kind = kind == L_FZ_FWD ? L_LZ_FWD : L_LZ_BWD;
        L.shmem = LZ_SHMEM;
        L.lz = *lz;
        L.name = std::string(kind == L_FZ_FWD ? "lz_se_fwd" : "lz_se_bwd") + (prec == PREC_F32 ? "<f32>" : "<bf16>");
    }
    (void)what;

    return L;
}

static Launch head_launch(avc_ctx* ctx, int B, int TN, int mode, const float* pooled, float* g_pooled, float* emb_out,
                          const float* tgt, const float* org, float* losses, const int* step, const float* scal,
                          int loss_len, int prec) {
    const avc_se_cfg& c = ctx->cfg;
    Launch L;
    L.kind = L_HEAD_V;
    L.grid = dim3(cdiv(B, 2));
    L.block = dim3(512);
    const int S = std::max(c.c_h, c.c_out);
    L.shmem = (size_t)(2 * c.n_dense_blocks + 5) * S * 2 * sizeof(float) +
              (size_t)(2 * c.n_dense_blocks * c.c_h + c.c_out + 4 * c.c_out + 2) * sizeof(float);
    HeadArgs& A = L.head;
    L.prec = prec;
    A.Wr = ctx->head_Wr.p;
    A.WrT = ctx->head_WrT.p;
    A.Wr16 = reinterpret_cast<const uint16_t*>(ctx->head_Wr16.p);
    A.WrT16 = reinterpret_cast<const uint16_t*>(ctx->head_WrT16.p);
    A.pooled_in = pooled;
    A.g_pooled = g_pooled;
    A.Wp = ctx->head_Wp.p;
    A.WpT = ctx->head_WpT.p;
    A.bias = ctx->head_bias.p;
    A.emb_out = emb_out;
    A.tgt = tgt;
    A.org = org;
    A.losses = losses;
    A.step = step;
    A.B = B;
    A.C = c.c_h;
    A.TN = TN;
    A.D = c.c_out;
    A.n_dense = c.n_dense_blocks;
    A.act = c.act;
    A.mode = mode;
    A.scal = scal;
    A.loss_len = loss_len;
    const double dense = 2.0 * c.c_h * c.c_h * 2 * c.n_dense_blocks + 2.0 * c.c_out * c.c_h;
    L.flop = dense * B * (mode == 0 ? 1 : 2);
    L.name = "se_head_v";
    return L;
}

static Launch dense_launch(const float* A, const float* X, const float* bias, float* Y, int M, int K, int B,
                           const char* name, int kslices = 1) {
    Launch L;
    L.kind = L_DENSE;
    // LDS-staged MFMA tiles (64 rows x 16 utterances) when a K slice fits DZ_KC = 128 floats,
    // register-fed MFMA tiles (64 x 32) for wider slices, the VALU kernel when K or the slice is
    // not a multiple of 4 (16-byte loads).  The two MFMA kernels give every output the same bits.
    const int kc = cdiv(K, kslices);
    const int variant = (K % 4 || kc % 4) ? DZ_VALU : kc <= 128 ? DZ_LDS : DZ_MFMA;
    L.grid = dim3(cdiv(M, 64), cdiv(B, variant == DZ_LDS ? 16 : 32), kslices);
    L.block = dim3(256);
    L.shmem = variant == DZ_LDS ? (64 + 16) * (128 + 4) * 4 : 0;
    L.dn = DenseArgs{A, X, bias, Y, M, K, B, kc, variant};
    L.flop = 2.0 * M * K * B;
    L.name = name;
    return L;
}

// spectral norm (sn=True): the power iteration and the rescale of precision `prec`'s packed copies,
// ahead of a Decoder forward (nothing when the Decoder has no spectral norm)
static void sn_launches(avc_ctx* ctx, int prec, Plan& pl) {
    VcState* S = ctx->vc;
    if (!S->cfg.dec_sn || S->sn_layers.empty()) return;
    SnArgs a{reinterpret_cast<const SnLayer*>(S->sn_layer_dev.p), S->sn_raw.p, S->sn_uv.p, S->sn_sigma.p,
             reinterpret_cast<const SnChunk*>(S->sn_chunk_dev[prec].p), reinterpret_cast<const int*>(S->sn_train.p)};
    Launch P;
    P.kind = L_SN_POWER;
    P.grid = dim3((unsigned)S->sn_layers.size());
    P.block = dim3(256);
    P.sn = a;
    P.name = "sn_power";
    pl.launches.push_back(P);
    Launch Q = P;
    Q.kind = L_SN_SCALE;
    Q.grid = dim3((unsigned)S->sn_chunks[prec].size());
    Q.name = "sn_scale";
    pl.launches.push_back(Q);
}

// Decoder MACs per utterance: forward (in_conv, blocks, out_conv); backward (out_conv^T,
// every block's conv2^T and all conv1^T but the first)
static double dec_mac(const avc_vc_cfg& v, const std::vector<int>& Tl, bool bwd) {
    const double C = FZ_C, k = v.dec_kernel_size;
    const int n = v.dec_n_conv_blocks;
    double mac = (double)DZ_COUT * C * Tl[n];
    if (!bwd) mac += C * C * Tl[0];
    for (int l = 0; l < n; ++l) {
        if (!bwd || l > 0) mac += C * C * k * Tl[l];
        mac += C * C * k * v.dec_upsample[l] * Tl[l];
    }
    return mac;
}

static Launch dec_launch(avc_ctx* ctx, int kind, int prec, int B, const std::vector<int>& Tl, bool stash) {
    VcState* S = ctx->vc;
    const avc_vc_cfg& v = S->cfg;
    VcWs& w = *S->cur;
    Launch L;
    L.kind = kind;
    L.prec = prec;
    L.grid = dim3(B);
    L.block = dim3(256);
    const int Tn = Tl.back();
    L.shmem = kind == L_DZ_FWD ? dz_lds_fwd(prec, Tn, v.dec_kernel_size) : dz_lds_bwd(prec, Tn);
    L.fz_shape = dec_shape(v, Tl[0]);
    if (w.dec_long) {
        L.kind = kind == L_DZ_FWD ? L_LZD_FWD : L_LZD_BWD;
        L.shmem = LZ_SHMEM;
        L.lz = w.lz.a;
    }
    DecArgs& A = L.dz;
    A.B = B;
    A.ks = v.dec_kernel_size;
    A.nblk = v.dec_n_conv_blocks;
    A.act = v.dec_act;
    for (int l = 0; l < A.nblk; ++l) A.up[l] = v.dec_upsample[l];
    for (int l = 0; l <= A.nblk; ++l) A.Tl[l] = Tl[l];
    for (int q = 0; q < 2 * A.nblk; ++q) A.stash_off[q] = w.stash_off[q];
    A.stash_per_utt = stash ? w.stash_per_utt : 0;
    A.mu = w.mu.p;
    A.cond = w.cond.p;
    A.out = w.out.p;
    A.stash = w.stash.p;
    A.invstd = w.invstd.p;
    A.g_cond = w.gcond.p;
    A.rag = w.rag_dec.get();
    A.w = S->dw[prec];
    L.flop = w.ragged ? w.fl_dec[kind == L_DZ_BWD] : 2.0 * dec_mac(v, Tl, kind == L_DZ_BWD) * B;
    L.name = std::string(kind == L_DZ_FWD ? "dec_fwd_fused" : "dec_bwd_fused") + (prec == PREC_F32 ? "<f32>" : "<bf16>");
    if (w.dec_long) L.name = std::string(kind == L_DZ_FWD ? "lz_dec_fwd" : "lz_dec_bwd") + (prec == PREC_F32 ? "<f32>" : "<bf16>");
    return L;
}

// a VC workspace whose build or plan failed part-way: forget it (its owners free what it holds); returns 1
static int drop_vc_cur(avc_ctx* ctx) {
    (void)hipStreamSynchronize(ctx->stream);
    ctx->vc->wss.erase(ctx->vc->cur);
    ctx->vc->cur = nullptr;
    return 1;
}

// the lengths and buffers of a new VC workspace for key `k` over the SpeakerEncoder workspace `ws`
static int build_vc_ws(avc_ctx* ctx, VcWs& w, const VcKey& k, const Workspace& ws) {
    VcState* S = ctx->vc;
    const avc_se_cfg& c = ctx->cfg;
    const avc_vc_cfg& v = S->cfg;
    if (enc_lengths(S->ce, S->ce_bank_k, k.Ts, w.Tl_ce) || dec_lengths(v, w.Tl_ce.back(), w.Tl_dec)) return 1;
    w.Tce = w.Tl_ce.back();
    w.Tn = w.Tl_dec.back();
    if (enc_lengths(c, ctx->bank_k, w.Tn, w.Tl_se2)) return 1;
    w.B = k.B;
    w.T = k.T;
    w.Ts = k.Ts;
    w.S = (size_t)k.B * FZ_CIN * k.Ts;
    w.O = (size_t)k.B * DZ_COUT * w.Tn;
    const int nd = v.dec_n_conv_blocks;
    // long engine for lengths past the fused engine's 128 frames (or when forced: then all three)
    w.ce_long = k.ce_long;
    w.dec_long = k.dec_long;
    w.se2_long = (k.ce_long && k.Ts <= 128) || w.Tn > 128;
    w.stash_off.assign(2 * DZ_MAXBLK, 0);
    int off = 0;
    for (int l = 0; l < nd; ++l) {
        // fused: [half][fragment] per layer; long: the fragment-layout stream of the layer's frames
        const int nfq = cdiv(w.Tl_dec[l], 16), nfo = cdiv(w.Tl_dec[l + 1], 16);
        w.stash_off[2 * l] = off;
        off += 2048 * nfq;
        w.stash_off[2 * l + 1] = off;
        off += 2048 * (w.dec_long ? nfo : nfq * v.dec_upsample[l]);
    }
    w.stash_per_utt = off;
    const size_t Bz = k.B;
    int rc = 0;
    rc |= dalloc(w.src, Bz * FZ_CIN * k.Ts);
    rc |= dalloc(w.mu, Bz * FZ_C * w.Tce);
    rc |= dalloc(w.lsig, Bz * FZ_C * w.Tce);
    for (DevBuf* b : {&w.emb, &w.pooled2, &w.gpooled2}) rc |= dalloc(*b, Bz * FZ_C);
    rc |= dalloc(w.gemb, Bz * FZ_C * 4 * nd);   // split-K slices of d loss / d emb
    rc |= dalloc(w.hact, Bz * 2 * c.n_dense_blocks * FZ_C);
    rc |= dalloc(w.cond, Bz * 2 * nd * 2 * FZ_C);
    rc |= dalloc(w.gcond, Bz * 2 * nd * 2 * FZ_C);
    rc |= dalloc(w.stash, Bz * (size_t)w.stash_per_utt);
    rc |= dalloc(w.invstd, Bz * 2 * nd * FZ_C);
    for (DevBuf* b : {&w.out, &w.tgt_out, &w.org_out, &w.gout, &w.gdec}) rc |= dalloc(*b, Bz * DZ_COUT * w.Tn);
    if (rc || dmalloc(w.masks2, Bz * ws.mask_words * sizeof(unsigned long long))) return 1;
    return (w.ce_long || w.dec_long || w.se2_long) &&
           alloc_long(w.lz, k.B, std::max(k.Ts, w.Tn), (int)ctx->bank_k.size() + 1 + 2 * c.n_conv_blocks);
}

// A source utterance's lengths through the ContentEncoder, the Decoder and the SpeakerEncoder over the
// decoder output; `b` names the utterance in the message of one that is too short
static int ragged_src_lengths(avc_ctx* ctx, int b, int Ts, std::vector<int>& tce, std::vector<int>& tdec,
                              std::vector<int>& tse2) {
    VcState* S = ctx->vc;
    if (Ts <= 0 || enc_lengths(S->ce, S->ce_bank_k, Ts, tce) || dec_lengths(S->cfg, tce.back(), tdec) ||
        enc_lengths(ctx->cfg, ctx->bank_k, tdec.back(), tse2))
        return fail("ragged batch: source utterance %d has %d frames, too short for the reflect padding of the "
                    "ContentEncoder / Decoder / SpeakerEncoder", b, Ts);
    return 0;
}

// the lengths, tables and buffers of a new ragged VC workspace for key `k` (k.lens / k.src_lens) over the ragged
// SpeakerEncoder workspace `ws`: buffers sized by sums of lengths, scratch for the longest utterance
static int build_vc_ws_ragged(avc_ctx* ctx, VcWs& w, const VcKey& k, const Workspace& ws) {
    VcState* S = ctx->vc;
    const avc_se_cfg& c = ctx->cfg;
    const avc_vc_cfg& v = S->cfg;
    const int B = k.B, nd = v.dec_n_conv_blocks;
    w.B = B;
    w.T = k.T;
    w.Ts = k.Ts;
    w.ragged = w.ce_long = w.dec_long = w.se2_long = true;
    // the plans' uniform fields (ignored by the kernels next to a table) describe the longest utterance
    const int longest = (int)(std::max_element(k.src_lens.begin(), k.src_lens.end()) - k.src_lens.begin());
    if (ragged_src_lengths(ctx, longest, k.Ts, w.Tl_ce, w.Tl_dec, w.Tl_se2)) return 1;
    w.Tce = w.Tl_ce.back();
    w.Tn = w.Tl_dec.back();
    w.stash_off.assign(2 * DZ_MAXBLK, 0);   // (the long Decoder derives a layer's offset from the utterance's T0)
    std::vector<RagUtt> rce(B), rse2(B);
    std::vector<DecUtt> rdec(B);
    std::vector<int> tce, tdec, tse2;
    size_t mu = 0, stash = 0;
    for (int b = 0; b < B; ++b) {
        if (ragged_src_lengths(ctx, b, k.src_lens[b], tce, tdec, tse2)) return 1;
        const int Tn = tdec.back();
        rce[b] = RagUtt{k.src_lens[b], 0, (int64_t)w.S, (int64_t)mu};
        rse2[b] = RagUtt{Tn, 0, (int64_t)w.O, 0};
        // the gradient scale of the output MSE over this utterance's 80 x Tn elements: the arithmetic of a
        // single-utterance call (vc_attack's g_out)
        rdec[b] = DecUtt{tce.back(), (float)(2.0 / (1.0 * DZ_COUT * Tn)), (int64_t)mu, (int64_t)w.O, (int64_t)stash};
        w.S += (size_t)FZ_CIN * k.src_lens[b];
        w.O += (size_t)DZ_COUT * Tn;
        mu += (size_t)FZ_C * tce.back();
        // stash block: the fragment-layout stream of every InstanceNorm layer's frames (avc_long.hip lz_dec_so)
        size_t st = 0;
        for (int l = 0; l < nd; ++l) st += 2048 * (size_t)(cdiv(tdec[l], 16) + cdiv(tdec[l + 1], 16));
        stash += st;
        w.stash_per_utt = std::max(w.stash_per_utt, (int)st);   // (the longest's: non-zero = "stash" in dec_launch)
        w.fl_ce += fz_fwd_flop(S->ce, tce, S->ce_bank_k);
        w.fl_se2 += fz_fwd_flop(c, tse2, ctx->bank_k);
        for (int bw = 0; bw < 2; ++bw) w.fl_dec[bw] += 2.0 * dec_mac(v, tdec, bw != 0);
    }
    if (dmalloc(w.rag_ce, B * sizeof(RagUtt)) || dmalloc(w.rag_se2, B * sizeof(RagUtt)) ||
        dmalloc(w.rag_dec, B * sizeof(DecUtt)))
        return 1;
    HIPCHK(hipMemcpy(w.rag_ce.get(), rce.data(), B * sizeof(RagUtt), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(w.rag_se2.get(), rse2.data(), B * sizeof(RagUtt), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(w.rag_dec.get(), rdec.data(), B * sizeof(DecUtt), hipMemcpyHostToDevice));
    const size_t Bz = B;
    int rc = 0;
    rc |= dalloc(w.src, w.S);
    rc |= dalloc(w.mu, mu);
    rc |= dalloc(w.lsig, mu);
    for (DevBuf* b : {&w.emb, &w.pooled2, &w.gpooled2}) rc |= dalloc(*b, Bz * FZ_C);
    rc |= dalloc(w.gemb, Bz * FZ_C * 4 * nd);
    rc |= dalloc(w.hact, Bz * 2 * c.n_dense_blocks * FZ_C);
    rc |= dalloc(w.cond, Bz * 2 * nd * 2 * FZ_C);
    rc |= dalloc(w.gcond, Bz * 2 * nd * 2 * FZ_C);
    rc |= dalloc(w.stash, stash);
    rc |= dalloc(w.invstd, Bz * 2 * nd * FZ_C);
    for (DevBuf* b : {&w.out, &w.tgt_out, &w.org_out, &w.gout, &w.gdec}) rc |= dalloc(*b, w.O);
    if (rc || dmalloc(w.masks2, Bz * ws.mask_words * sizeof(unsigned long long))) return 1;
    return alloc_long(w.lz, B, std::max(k.Ts, w.Tn), (int)ctx->bank_k.size() + 1 + 2 * c.n_conv_blocks);
}

static int plan_vc_ws(avc_ctx* ctx, VcWs& w, Workspace& ws);
static int ensure_vc_key(avc_ctx* ctx, const VcKey& k);

// The VC workspace of a call (ctx->vc->cur) over the SpeakerEncoder workspace of (B, T): resolve the
// key, look it up, build a new entry or re-plan one whose SpeakerEncoder workspace was re-planned, plan.
static int ensure_vc_ws(avc_ctx* ctx, int B, int T, int Ts, int n_iters) {
    VcState* S = ctx->vc;
    if (!S) return fail("no ContentEncoder/Decoder attached (avc_attach_vc)");
    if (ensure_ws(ctx, B, T, n_iters)) return 1;
    Workspace& ws = *ctx->cur;
    if (!ws.fused) return fail("the e2e / fb path runs on the fused engine only (T <= 128, engine not LAYERED)");
    // the engine of each component is part of the key (avc_set_engine may force the long one)
    std::vector<int> tce, tdec;
    if (enc_lengths(S->ce, S->ce_bank_k, Ts, tce) || dec_lengths(S->cfg, tce.back(), tdec)) return 1;
    const int Tmax = std::max(Ts, tdec.back());
    const bool force = engine_for(ctx, Tmax) == AVC_ENGINE_LONG && Tmax <= 128;
    return ensure_vc_key(ctx, VcKey{B, T, Ts, force || Ts > 128, force || tdec.back() > 128, {}, {}});
}

// A ragged batch: utterance b attacks lens[b] frames with a source of src_lens[b] frames.  The SpeakerEncoder
// workspace under it is the ragged one of `lens` on the long engine, whatever the lengths: every component of
// the ragged VC path runs on the long engine, one launch per pass over the whole batch.
static int ensure_vc_ws_ragged(avc_ctx* ctx, const std::vector<int>& lens, const std::vector<int>& src_lens,
                               int n_iters) {
    VcState* S = ctx->vc;
    if (!S) return fail("no ContentEncoder/Decoder attached (avc_attach_vc)");
    if (ctx->engine == AVC_ENGINE_LAYERED)
        return fail("ragged e2e / fb / inference batches run on the long engine: not under AVC_ENGINE_LAYERED");
    const int B = (int)lens.size();
    if (B <= 0 || src_lens.size() != lens.size()) return fail("ragged batch: %zu source lengths for B=%d", src_lens.size(), B);
    std::vector<int> a, b, c;   // the key's lengths are valid before anything is built or evicted for it
    for (int u = 0; u < B; ++u)
        if (ragged_src_lengths(ctx, u, src_lens[u], a, b, c)) return 1;
    if (ensure_ws(ctx, B, 0, n_iters, &lens, true)) return 1;
    return ensure_vc_key(ctx, VcKey{B, *std::max_element(lens.begin(), lens.end()),
                                    *std::max_element(src_lens.begin(), src_lens.end()), true, true, lens, src_lens});
}

// look the key up over the SpeakerEncoder workspace of the call (ctx->cur), build / re-plan / plan
static int ensure_vc_key(avc_ctx* ctx, const VcKey& k) {
    VcState* S = ctx->vc;
    Workspace& ws = *ctx->cur;
    S->cur = S->wss.find(k);
    if (S->cur && S->cur->ws_gen == ws.gen) {
        ++ctx->n_ws_hits;               // served by the cached workspace as it was (include/avc.h "hits")
        return 0;
    }
    const bool fresh = !S->cur;
    auto quiesce = [&] { return hipStreamSynchronize(ctx->stream) != hipSuccess; };
    if (fresh) {
        S->wss.cap = ctx->wss.cap;
        S->cur = S->wss.insert(k, env_int("AVC_WS_CACHE", S->wss.cap), quiesce);
        if (!S->cur) return fail("hipStreamSynchronize failed before a workspace eviction");
    }
    ++(fresh ? ctx->n_ws_builds : ctx->n_ws_replans);   // (replan: the SpeakerEncoder workspace under it was)
    if (quiesce()) {
        fail("hipStreamSynchronize failed");
        return drop_vc_cur(ctx);
    }
    if ((fresh && (k.src_lens.empty() ? build_vc_ws(ctx, *S->cur, k, ws) : build_vc_ws_ragged(ctx, *S->cur, k, ws))) ||
        plan_vc_ws(ctx, *S->cur, ws))
        return drop_vc_cur(ctx);
    return 0;
}

// every plan of `w`, pointing into `ws` as it is now
static int plan_vc_ws(avc_ctx* ctx, VcWs& w, Workspace& ws) {
    VcState* S = ctx->vc;
    const avc_se_cfg& c = ctx->cfg;
    const avc_vc_cfg& v = S->cfg;
    const int B = w.B, T = w.T, Ts = w.Ts;
    renew(w.pl);
    const int nbS = ctx->nb, nbC = (int)S->ce_bank_k.size();
    const int nd = v.dec_n_conv_blocks, M = 2 * nd * 2 * FZ_C;
    // (a ragged workspace: the sums over its utterances; every encoder pass takes its table of lengths)
    const double se_fl = w.ragged ? ws.flop_fwd : fz_fwd_flop(c, ws.Tl, ctx->bank_k) * B;
    const double se2_fl = w.ragged ? w.fl_se2 : fz_fwd_flop(c, w.Tl_se2, ctx->bank_k) * B;
    const int shS = enc_shape(c, nbS, T), shS2 = enc_shape(c, nbS, w.Tn);
    const int TNs = ws.Tl.back(), TNs2 = w.Tl_se2.back();

    {   // ContentEncoder (fp32, once per attack): mu = CE(src)
        FusedArgs A = enc_args(S->ce, nbC, B, w.Tl_ce, S->cew[PREC_F32]);
        A.x = w.src.p;
        A.ce_mode = 1;
        A.mu_out = w.mu.p;
        A.rag = w.rag_ce.get();
        w.pl.ce.launches.push_back(enc_launch(L_FZ_FWD, PREC_F32, A, enc_shape(S->ce, nbC, Ts), S->ce.kernel_size,
                                           w.ragged ? w.fl_ce : fz_fwd_flop(S->ce, w.Tl_ce, S->ce_bank_k) * B, "ce",
                                           w.ce_long ? &w.lz.a : nullptr));
        w.pl.ce.launches.back().name = w.ce_long ? "lz_ce_fwd<f32>" : "ce_fwd_fused<f32>";
        // log_sigma = std_layer(h_N): the same pass with std_layer as the final 1x1 (on demand)
        A.w = S->cew_std[PREC_F32];
        A.mu_out = w.lsig.p;
        w.pl.ce_std.launches.push_back(w.pl.ce.launches.back());
        w.pl.ce_std.launches.back().fz = A;
    }
    // Decoder(mu, emb = ws.emb_fwd) -> w.out (fp32, precomputations / inference)
    sn_launches(ctx, PREC_F32, w.pl.dec_pre);
    w.pl.dec_pre.launches.push_back(dense_launch(S->aff.p, ws.emb_fwd.p, S->aff_b.p, w.cond.p, M, FZ_C, B, "dense_affine"));
    w.pl.dec_pre.launches.push_back(dec_launch(ctx, L_DZ_FWD, PREC_F32, B, w.Tl_dec, false));
    {   // SpeakerEncoder(w.out) -> ws.emb_fwd (fp32; fb's org embedding)
        FusedArgs A = enc_args(c, nbS, B, w.Tl_se2, ctx->fzw[PREC_F32]);
        A.x = w.out.p;
        A.pooled = w.pooled2.p;
        A.masks = w.masks2.get();
        A.mask_words = ws.mask_words;
        A.rag = w.rag_se2.get();
        w.pl.se2_pre.launches.push_back(enc_launch(L_FZ_FWD, PREC_F32, A, shS2, c.kernel_size, se2_fl, "se2",
                                                w.se2_long ? &w.lz.a : nullptr));
        w.pl.se2_pre.launches.push_back(head_launch(ctx, B, TNs2, 0, w.pooled2.p, nullptr, ws.emb_fwd.p, nullptr, nullptr,
                                                 nullptr, ws.step.get(), ws.scal.p, ws.iters_cap, PREC_F32));
    }
    // bf16, config.yaml shape: the head chains run inside the encoder kernels (se_head_fused
    // modes 0 / 1 / 3) instead of three se_head_v launches; AVC_FUSE_HEAD=0 keeps the launches
    const bool head_ok = ctx->head_Wr16.p && c.c_h == FZ_C && c.c_out == FZ_C && c.n_dense_blocks == 6 &&
                         !env_is("AVC_FUSE_HEAD", '0');
    const size_t head_lds = (size_t)(4 * c.n_dense_blocks + 8) * FZ_C * sizeof(float);
    for (int kind = 0; kind < 2; ++kind)
        for (int prec = 0; prec < 2; ++prec) {
            Plan& pl = w.pl.it[kind][prec];
            const bool fh1 = prec == PREC_BF16 && head_ok && !ws.lz && (shS == 0 || shS == 16);    // SE(adv) fwd / bwd
            const bool fh2 = prec == PREC_BF16 && head_ok && !w.se2_long && (shS2 == 0 || shS2 == 16);   // fb: SE(dec)
            {   // SE(adv): masks + time-mean; advances the step counter
                FusedArgs A = enc_args(c, nbS, B, ws.Tl, ctx->fzw[prec]);
                A.x = ws.adv.p;
                A.pooled = ws.pooled.p;
                A.masks = ws.masks.get();
                A.mask_words = ws.mask_words;
                A.write_masks = 1;
                A.tick = ws.step.get();
                A.rag = ws.rag.get();
                Launch F = enc_launch(L_FZ_FWD, prec, A, shS, c.kernel_size, se_fl, "se", ws.lz ? &ws.lzs.a : nullptr);
                Launch H = head_launch(ctx, B, TNs, 0, ws.pooled.p, nullptr, w.emb.p, nullptr, nullptr, nullptr,
                                       ws.step.get(), ws.scal.p, ws.iters_cap, prec);
                if (fh1) {   // embedding + dense activations from the forward's tail
                    F.fz.fuse_head = 2;
                    F.fz.head = H.head;
                    F.fz.head.act_out = w.hact.p;
                    F.shmem = std::max(F.shmem, head_lds);
                    F.flop += H.flop;
                    pl.launches.push_back(F);
                } else {
                    pl.launches.push_back(F);
                    pl.launches.push_back(H);
                }
            }
            sn_launches(ctx, prec, pl);   // one power iteration per Decoder forward (sn=True)
            pl.launches.push_back(dense_launch(S->aff.p, w.emb.p, S->aff_b.p, w.cond.p, M, FZ_C, B, "dense_affine"));
            Launch df = dec_launch(ctx, L_DZ_FWD, prec, B, w.Tl_dec, true);
            Launch db = dec_launch(ctx, L_DZ_BWD, prec, B, w.Tl_dec, true);
            if (kind == 0) {   // e2e: output loss and its gradient inside the decoder forward
                df.dz.tgt_out = w.tgt_out.p;
                df.dz.org_out = w.org_out.p;
                df.dz.g_out = w.gout.p;
                df.dz.losses = ws.losses.p;
                df.dz.step = ws.step.get();
                df.dz.scal = ws.scal.p;
                df.dz.loss_len = ws.iters_cap;
                if (!w.dec_long) df.dz.out = nullptr;   // nothing reads the output in an e2e iteration
                db.dz.g_in = w.gout.p;
                pl.launches.push_back(df);
            } else {   // fb: SE(dec) -> loss vs the fb embeddings -> d loss / d dec
                pl.launches.push_back(df);
                FusedArgs A = enc_args(c, nbS, B, w.Tl_se2, ctx->fzw[prec]);
                A.x = w.out.p;
                A.pooled = w.pooled2.p;
                A.masks = w.masks2.get();
                A.mask_words = ws.mask_words;
                A.write_masks = 1;
                A.rag = w.rag_se2.get();
                Launch F2 = enc_launch(L_FZ_FWD, prec, A, shS2, c.kernel_size, se2_fl, "se2",
                                       w.se2_long ? &w.lz.a : nullptr);
                Launch H2 = head_launch(ctx, B, TNs2, 1, w.pooled2.p, w.gpooled2.p, w.emb.p, ws.tgt.p, ws.org.p,
                                        ws.losses.p, ws.step.get(), ws.scal.p, ws.iters_cap, prec);
                if (fh2) {   // the emb-loss chain in SE(dec)'s tail; the loss row is written by its bwd
                    F2.fz.fuse_head = 1;
                    F2.fz.head = H2.head;
                    F2.fz.loss_cur = ws.loss_cur.p;
                    F2.shmem = std::max(F2.shmem, head_lds);
                    F2.flop += H2.flop;
                    pl.launches.push_back(F2);
                } else {
                    pl.launches.push_back(F2);
                    pl.launches.push_back(H2);
                }
                FusedArgs G = A;
                G.write_masks = 0;
                G.g_pooled = w.gpooled2.p;
                G.step = ws.step.get();
                G.scal = ws.scal.p;
                G.table_len = ws.iters_cap;
                G.gx_out = w.gdec.p;
                if (fh2) {
                    G.loss_cur = ws.loss_cur.p;
                    G.losses = ws.losses.p;
                    G.loss_len = ws.iters_cap;
                }
                pl.launches.push_back(enc_launch(L_FZ_BWD, prec, G, shS2, c.kernel_size, se2_fl, "se2",
                                                 w.se2_long ? &w.lz.a : nullptr));
                db.dz.g_in = w.gdec.p;
            }
            pl.launches.push_back(db);
            // d loss / d emb = sum over the 2n AdaIN layers q of W_q^T g_cond_q: two K slices
            // per layer (4n x B/32 x 2 workgroups), the slices summed by the head in order
            pl.launches.push_back(dense_launch(S->affT.p, w.gcond.p, nullptr, w.gemb.p, FZ_C, M, B, "dense_affine_T",
                                               4 * nd));
            Launch H3 = head_launch(ctx, B, TNs, 3, ws.pooled.p, ws.gpooled.p, w.emb.p, w.gemb.p, w.gemb.p, nullptr,
                                    ws.step.get(), ws.scal.p, ws.iters_cap, prec);
            H3.head.tgt_parts = 4 * nd;
            if (!fh1) pl.launches.push_back(H3);
            if (plan_fused_backward(ctx, ws, pl, prec)) return 1;
            if (fh1) {   // d loss / d emb -> g_pooled at the start of SE(adv)'s backward
                Launch& Bk = pl.launches.back();
                Bk.fz.fuse_head = 3;
                Bk.fz.head = H3.head;
                Bk.fz.head.act_in = w.hact.p;
                Bk.shmem = std::max(Bk.shmem, head_lds);
                Bk.flop += H3.flop / 2;
            }
        }
    w.ws_gen = ws.gen;
    return 0;
}

// Decoder(ContentEncoder(src).mu, emb): emb [B][c_out] given (emb_dev) or SE(tgt) at Ts frames.
// src_lens (ragged batch, emb_dev only): src / out are packed blocks of src_lens[b] / Tn(src_lens[b]) frames.
static int inference_impl(avc_ctx* ctx, const float* src, int Ts, const float* tgt, const float* emb_dev, int B,
                          float* out, void* stream, const std::vector<int>* src_lens = nullptr) {
    if (!ctx || !src || !(tgt || emb_dev) || !out) return fail("avc_inference: null argument");
    hipStream_t us = (hipStream_t)stream;
    if (src_lens ? ensure_vc_ws_ragged(ctx, *src_lens, *src_lens, 1) : ensure_vc_ws(ctx, B, Ts, Ts, 1)) return 1;
    if (begin_call(ctx, us)) return 1;
    VcWs& w = *ctx->vc->cur;
    Workspace& ws = *ctx->cur;
    if (d2d(ctx, w.src.p, src, w.S) || run_plan(ctx, w.pl.ce, false)) return 1;
    if (tgt) {
        if (se_embed(ctx, tgt)) return 1;
    } else if (d2d(ctx, ws.emb_fwd.p, emb_dev, (size_t)B * ctx->cfg.c_out)) {
        return 1;
    }
    if (run_plan(ctx, w.pl.dec_pre, false)) return 1;
    if (d2d(ctx, out, w.out.p, w.O)) return 1;
    return end_call(ctx, us);
}

extern "C" int avc_inference(avc_ctx* ctx, const float* src, const float* tgt, int B, int T, float* out, void* stream) {
    if (!tgt) return fail("avc_inference: null argument");
    return inference_impl(ctx, src, T, tgt, nullptr, B, out, stream);
}

extern "C" int avc_inference_emb(avc_ctx* ctx, const float* src, int B, int T_src, const float* emb, float* out,
                                 void* stream) {
    if (!emb) return fail("avc_inference_emb: null argument");
    return inference_impl(ctx, src, T_src, nullptr, emb, B, out, stream);
}

// A ragged batch: src is packed [80][src_lengths[b]] blocks in batch order (host array of lengths), emb
// [B][c_out], out packed [80][Tn(src_lengths[b])] blocks.  One launch per component over every length.
extern "C" int avc_inference_ragged(avc_ctx* ctx, const float* src, const int* src_lengths, int B, const float* emb,
                                    float* out, void* stream) {
    if (!ctx || !src_lengths || !emb) return fail("avc_inference_ragged: null argument");
    if (B <= 0) return fail("avc_inference_ragged: batch size must be positive (got %d)", B);
    const std::vector<int> sl(src_lengths, src_lengths + B);
    return inference_impl(ctx, src, 0, nullptr, emb, B, out, stream, &sl);
}

// e2e / fb attack; vc_src has Ts frames, vc_tgt / ptb0 T frames; the target embedding is
// SE(adv_tgt) at T frames (adv_tgt given) or the caller's tgt_emb [B][c_out].
// lens / src_lens (ragged batch, tgt_emb only): every array is packed blocks of the utterances' own lengths.
static int vc_attack(avc_ctx* ctx, int kind, const float* vc_src, int Ts, const float* vc_tgt, const float* adv_tgt,
                     const float* tgt_emb, const float* ptb0, int B, int T, float eps, int n_iters, float* out_adv,
                     const avc_attack_opts* opts, void* stream, const std::vector<int>* lens = nullptr,
                     const std::vector<int>* src_lens = nullptr) {
    const char* nm = kind == 0 ? "avc_e2e_attack" : "avc_fb_attack";
    if (!ctx || !vc_src || !vc_tgt || !(adv_tgt || tgt_emb) || !ptb0 || !out_adv) return fail("%s: null argument", nm);
    if (n_iters < 0) return fail("n_iters must be >= 0");
    avc_attack_opts o;
    if (attack_opts(opts, &o)) return 1;
    hipStream_t us = (hipStream_t)stream;
    if (lens ? ensure_vc_ws_ragged(ctx, *lens, *src_lens, n_iters) : ensure_vc_ws(ctx, B, T, Ts, n_iters)) return 1;
    Workspace& ws = *ctx->cur;
    VcWs& w = *ctx->vc->cur;
    const int prec = o.precision == AVC_PREC_BF16 ? PREC_BF16 : PREC_F32;
    if (begin_call(ctx, us)) return 1;
    const avc_se_cfg& c = ctx->cfg;
    const bool mean = o.reduction == AVC_REDUCE_MEAN;
    const float g_emb = (float)(2.0 / ((mean ? (double)B : 1.0) * c.c_out));
    // (a ragged batch: every utterance's own 2 / (80 Tn_b), in the Decoder's table)
    const float g_out = (float)(2.0 / ((mean ? (double)B : 1.0) * DZ_COUT * w.Tn));
    if (stage_attack_consts(ctx, n_iters, eps, g_emb, g_out, o)) return 1;

    if (d2d(ctx, ws.vc.p, vc_tgt, ws.X) || d2d(ctx, w.src.p, vc_src, w.S)) return 1;
    if (run_plan(ctx, w.pl.ce, false)) return 1;                                  // mu = CE(vc_src)
    const size_t O = w.O, Eb = (size_t)B * c.c_out;
    if (kind == 0) {
        // org_out = inference(vc_src, vc_tgt), tgt_out = inference(vc_src, adv_tgt)  (attack_utils.py:35-37)
        if (se_embed(ctx, vc_tgt) || run_plan(ctx, w.pl.dec_pre, false) || d2d(ctx, w.org_out.p, w.out.p, O)) return 1;
        if (adv_tgt ? se_embed(ctx, adv_tgt) : d2d(ctx, ws.emb_fwd.p, tgt_emb, Eb)) return 1;
        if (run_plan(ctx, w.pl.dec_pre, false) || d2d(ctx, w.tgt_out.p, w.out.p, O)) return 1;
    } else {
        // org_emb = SE(inference(vc_src, vc_tgt)), tgt_emb = SE(adv_tgt)  (attack_utils.py:117-119)
        if (se_embed(ctx, vc_tgt) || run_plan(ctx, w.pl.dec_pre, false) || run_plan(ctx, w.pl.se2_pre, false) ||
            d2d(ctx, ws.org.p, ws.emb_fwd.p, Eb))
            return 1;
        if (adv_tgt ? (se_embed(ctx, adv_tgt) || d2d(ctx, ws.tgt.p, ws.emb_fwd.p, Eb)) : d2d(ctx, ws.tgt.p, tgt_emb, Eb))
            return 1;
    }
    if (attack_begin(ctx, ptb0, eps, o)) return 1;
    if (run_iterations(ctx, w.pl.it[kind][prec], w.pl.graph[kind][prec], n_iters, o.use_graph != 0)) return 1;
    return attack_end(ctx, n_iters, out_adv, o, us);
}

extern "C" int avc_e2e_attack(avc_ctx* ctx, const float* vc_src, const float* vc_tgt, const float* adv_tgt,
                              const float* ptb0, int B, int T, float eps, int n_iters, float* out_adv,
                              const avc_attack_opts* opts, void* stream) {
    if (!adv_tgt) return fail("avc_e2e_attack: null argument");
    return vc_attack(ctx, 0, vc_src, T, vc_tgt, adv_tgt, nullptr, ptb0, B, T, eps, n_iters, out_adv, opts, stream);
}

extern "C" int avc_fb_attack(avc_ctx* ctx, const float* vc_src, const float* vc_tgt, const float* adv_tgt,
                             const float* ptb0, int B, int T, float eps, int n_iters, float* out_adv,
                             const avc_attack_opts* opts, void* stream) {
    if (!adv_tgt) return fail("avc_fb_attack: null argument");
    return vc_attack(ctx, 1, vc_src, T, vc_tgt, adv_tgt, nullptr, ptb0, B, T, eps, n_iters, out_adv, opts, stream);
}

extern "C" int avc_e2e_attack_emb(avc_ctx* ctx, const float* vc_src, int T_src, const float* vc_tgt,
                                  const float* tgt_emb, const float* ptb0, int B, int T, float eps, int n_iters,
                                  float* out_adv, const avc_attack_opts* opts, void* stream) {
    if (!tgt_emb) return fail("avc_e2e_attack_emb: null argument");
    return vc_attack(ctx, 0, vc_src, T_src, vc_tgt, nullptr, tgt_emb, ptb0, B, T, eps, n_iters, out_adv, opts, stream);
}

extern "C" int avc_fb_attack_emb(avc_ctx* ctx, const float* vc_src, int T_src, const float* vc_tgt,
                                 const float* tgt_emb, const float* ptb0, int B, int T, float eps, int n_iters,
                                 float* out_adv, const avc_attack_opts* opts, void* stream) {
    if (!tgt_emb) return fail("avc_fb_attack_emb: null argument");
    return vc_attack(ctx, 1, vc_src, T_src, vc_tgt, nullptr, tgt_emb, ptb0, B, T, eps, n_iters, out_adv, opts, stream);
}

// Ragged batches: utterance b has src_lengths[b] source and lengths[b] attacked frames (host arrays); vc_src is
// packed [80][src_lengths[b]] blocks, vc_tgt / ptb0 / out_adv (and opts->grad0) packed [80][lengths[b]] blocks in
// batch order, tgt_emb [B][c_out] = SE(adv_tgt_b) at adv_tgt_b's own length.  Every pass of every component is
// one launch over the whole batch on the long engine.
static int vc_attack_ragged(avc_ctx* ctx, int kind, const float* vc_src, const int* src_lengths, const float* vc_tgt,
                            const int* lengths, int B, const float* tgt_emb, const float* ptb0, float eps, int n_iters,
                            float* out_adv, const avc_attack_opts* opts, void* stream) {
    const char* nm = kind == 0 ? "avc_e2e_attack_ragged" : "avc_fb_attack_ragged";
    if (!ctx || !src_lengths || !lengths || !tgt_emb) return fail("%s: null argument", nm);
    if (B <= 0) return fail("%s: batch size must be positive (got %d)", nm, B);
    if (opts && opts->reduction != AVC_REDUCE_INDEPENDENT)
        return fail("%s: only independent per-utterance attacks (reduction 0)", nm);
    const std::vector<int> lens(lengths, lengths + B), sl(src_lengths, src_lengths + B);
    return vc_attack(ctx, kind, vc_src, 0, vc_tgt, nullptr, tgt_emb, ptb0, B, 0, eps, n_iters, out_adv, opts, stream,
                     &lens, &sl);
}

extern "C" int avc_e2e_attack_ragged(avc_ctx* ctx, const float* vc_src, const int* src_lengths, const float* vc_tgt,
                                     const int* lengths, int B, const float* tgt_emb, const float* ptb0, float eps,
                                     int n_iters, float* out_adv, const avc_attack_opts* opts, void* stream) {
    return vc_attack_ragged(ctx, 0, vc_src, src_lengths, vc_tgt, lengths, B, tgt_emb, ptb0, eps, n_iters, out_adv, opts,
                            stream);
}

extern "C" int avc_fb_attack_ragged(avc_ctx* ctx, const float* vc_src, const int* src_lengths, const float* vc_tgt,
                                    const int* lengths, int B, const float* tgt_emb, const float* ptb0, float eps,
                                    int n_iters, float* out_adv, const avc_attack_opts* opts, void* stream) {
    return vc_attack_ragged(ctx, 1, vc_src, src_lengths, vc_tgt, lengths, B, tgt_emb, ptb0, eps, n_iters, out_adv, opts,
                            stream);
}

// ContentEncoder.forward (models.py:181-210): (mu, log_sigma) [B][c_out][Tce] of x [B][80][T], fp32
extern "C" int avc_content_encoder(avc_ctx* ctx, const float* x, int B, int T, float* mu, float* log_sigma,
                                   void* stream) {
    if (!ctx || !x || !(mu || log_sigma)) return fail("avc_content_encoder: null argument");
    hipStream_t us = (hipStream_t)stream;
    if (ensure_vc_ws(ctx, B, T, T, 1)) return 1;
    if (begin_call(ctx, us)) return 1;
    VcWs& w = *ctx->vc->cur;
    const size_t O = (size_t)B * FZ_C * w.Tce;
    if (d2d(ctx, w.src.p, x, (size_t)B * FZ_CIN * T)) return 1;
    if (mu && (run_plan(ctx, w.pl.ce, false) || d2d(ctx, mu, w.mu.p, O))) return 1;
    if (log_sigma && (run_plan(ctx, w.pl.ce_std, false) || d2d(ctx, log_sigma, w.lsig.p, O))) return 1;
    return end_call(ctx, us);
}

extern "C" int avc_content_frames(avc_ctx* ctx, int T) {
    if (!ctx || !ctx->vc) {
        fail("no ContentEncoder/Decoder attached (avc_attach_vc)");
        return -1;
    }
    std::vector<int> a;
    if (enc_lengths(ctx->vc->ce, ctx->vc->ce_bank_k, T, a)) return -1;
    return a.back();
}

// Decoder.forward (models.py:403-435): out [B][80][Tn] = Decoder(z [B][c_h][Tz], cond [B][c_cond]), fp32.
// Runs the inference plan of a source length that the ContentEncoder maps onto Tz frames.
extern "C" int avc_decoder(avc_ctx* ctx, const float* z, int B, int Tz, const float* cond, float* out, void* stream) {
    if (!ctx || !z || !cond || !out) return fail("avc_decoder: null argument");
    if (!ctx->vc) return fail("no ContentEncoder/Decoder attached (avc_attach_vc)");
    long Ts = Tz;
    for (int l = 0; l < ctx->vc->ce.n_conv_blocks; ++l) Ts *= ctx->vc->ce.subsample[l];
    if (Tz <= 0 || Ts > (1 << 20)) return fail("avc_decoder: bad input length %d", Tz);
    hipStream_t us = (hipStream_t)stream;
    if (ensure_vc_ws(ctx, B, (int)Ts, (int)Ts, 1)) return 1;
    VcWs& w = *ctx->vc->cur;
    if (w.Tce != Tz) return fail("avc_decoder: internal length mapping %ld -> %d (want %d)", Ts, w.Tce, Tz);
    if (begin_call(ctx, us)) return 1;
    Workspace& ws = *ctx->cur;
    if (d2d(ctx, w.mu.p, z, (size_t)B * FZ_C * Tz) || d2d(ctx, ws.emb_fwd.p, cond, (size_t)B * ctx->vc->cfg.dec_c_cond))
        return 1;
    if (run_plan(ctx, w.pl.dec_pre, false)) return 1;
    if (d2d(ctx, out, w.out.p, (size_t)B * DZ_COUT * w.Tn)) return 1;
    return end_call(ctx, us);
}
