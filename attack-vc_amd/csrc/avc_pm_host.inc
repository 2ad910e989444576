// libavc host side of the VSMask PredictiveModel forward (included at the end of
// avc_api.hip): weight packing (BatchNorm folded into the convolutions, transposed
// convolutions split by output parity class), workspace, one launch per layer.

struct avc_pm {
    int device = 0;
    struct Layer {
        int Cin, Cout, sh, sw, mode, act;
        float slope;
        int woff[4];
        DevBuf w, b;
        bool mfma = false;            // Cin, Cout multiples of 16: pm_mfma (NHWC) in the network forward
        int wmoff[4] = {0, 0, 0, 0};
        DevBuf wm;                    // A in pm_mfma's fragment order
    };
    std::vector<Layer> layers;
    std::vector<DevBuf> act;          // per layer output (grow-only)
    DevBuf part;                      // split-K partial sums (grow-only)
    DevBuf vwin, vy;                  // VSMask: gathered windows, predictor outputs (grow-only)
    size_t cap_B = 0;
    int cap_H = 0, cap_W = 0;
};

namespace {
// predictive_model.py:66-83
const int PM_DOWN[7][4] = {{1, 32, 1, 2}, {32, 64, 2, 2}, {64, 128, 2, 2}, {128, 256, 2, 2},
                           {256, 256, 2, 2}, {256, 512, 2, 2}, {512, 512, 2, 2}};
const int PM_UP[5][2] = {{512, 256}, {256, 128}, {128, 64}, {64, 32}, {32, 1}};
}  // namespace

static size_t pm_weight_count() {
    size_t n = 0;
    for (auto& d : PM_DOWN) n += (size_t)d[1] * d[0] * 9 + d[1] + 4 * (size_t)d[1] + 1;   // conv, BN x4, PReLU
    for (auto& u : PM_UP) n += (size_t)u[0] * u[1] * 9 + u[1];
    return n;
}

extern "C" size_t avc_pm_weight_count(void) { return pm_weight_count(); }

// output size of the network for an H x W window; 0 if a reflect pad would exceed its input
static int pm_shapes(int H, int W, std::vector<std::array<int, 2>>& hw) {
    hw.assign(1, {H, W});
    for (auto& d : PM_DOWN) {
        const int h = hw.back()[0], w = hw.back()[1];
        if (h < 2 || w < 2) return fail("PredictiveModel: a %dx%d input to ReflectionPad2d(1) is too small", h, w);
        hw.push_back({(h + 2 - 3) / d[2] + 1, (w + 2 - 3) / d[3] + 1});
    }
    for (int i = 0; i < 5; ++i) hw.push_back({2 * (hw.back()[0] - 1) + 3, 2 * (hw.back()[1] - 1) + 3});
    return 0;
}

extern "C" int avc_pm_out_shape(int H, int W, int* Ho, int* Wo) {
    std::vector<std::array<int, 2>> hw;
    if (pm_shapes(H, W, hw)) return 1;
    if (Ho) *Ho = hw.back()[0];
    if (Wo) *Wo = hw.back()[1];
    return 0;
}

// A of one layer in pm_mfma's fragment order: class c's rows [Cout][K = (tap, ci)] given by get(c, co,
// tap, ci); value (m tile mt, K chunk kc, lane l, step s) = A[16 mt + (l & 15)][16 kc + 4 (l >> 4) + s]
template <typename G>
static int pm_pack_mfma(avc_pm::Layer& L, G get) {
    std::vector<float> A;
    const int nmt = (L.Cout + 15) / 16, ccpt = L.Cin / 16;
    for (int cls = 0; cls < (L.mode == 1 ? 4 : 1); ++cls) {
        const int py = cls >> 1, px = cls & 1;
        const int ntaps = L.mode == 1 ? (py == 0 ? 2 : 1) * (px == 0 ? 2 : 1) : 9;
        const int nchunk = ntaps * ccpt;
        L.wmoff[cls] = (int)A.size();
        for (int mt = 0; mt < nmt; ++mt)
            for (int kc = 0; kc < nchunk; ++kc)
                for (int l = 0; l < 64; ++l)
                    for (int st = 0; st < 4; ++st) {
                        const int co = 16 * mt + (l & 15), k = 16 * kc + 4 * (l >> 4) + st;
                        const int tap = k / L.Cin, ci = k - tap * L.Cin;
                        A.push_back(co < L.Cout ? get(cls, co, tap, ci) : 0.f);
                    }
    }
    L.mfma = true;
    return upload(L.wm, A);
}

extern "C" int avc_pm_create(int device, const float* w, size_t n, avc_pm** out) {
    if (!w || !out) return fail("avc_pm_create: null argument");
    if (n != pm_weight_count()) return fail("avc_pm_create: got %zu weights, PredictiveModel needs %zu", n, pm_weight_count());
    HIPCHK(hipSetDevice(device));
    avc_pm* pm = new avc_pm();
    pm->device = device;
    const float* p = w;
    int rc = 0;
    for (auto& d : PM_DOWN) {   // down_blocks.i.conv: 1 = Conv2d, 2 = BatchNorm2d, 3 = PReLU
        const int ci = d[0], co = d[1];
        const float* W = p;
        p += (size_t)co * ci * 9;
        const float* cb = p;
        p += co;
        const float *g = p, *be = p + co, *mu = p + 2 * co, *var = p + 3 * co;
        p += 4 * co;
        const float slope = *p++;
        avc_pm::Layer L{ci, co, d[2], d[3], 0, 0, slope, {0, 0, 0, 0}, {}, {}};
        std::vector<float> A((size_t)co * ci * 9), bias(co);
        for (int o = 0; o < co; ++o) {
            // BatchNorm2d eval (eps 1e-5): (conv + b - mean) * gamma / sqrt(var + eps) + beta
            const double s = (double)g[o] / std::sqrt((double)var[o] + 1e-5);
            for (size_t k = 0; k < (size_t)ci * 9; ++k) A[(size_t)o * ci * 9 + k] = (float)(W[(size_t)o * ci * 9 + k] * s);
            bias[o] = (float)(((double)cb[o] - mu[o]) * s + be[o]);
        }
        rc |= upload(L.w, A);
        rc |= upload(L.b, bias);
        if (ci % 16 == 0 && co % 16 == 0)   // A[co][(tap = 3 ky + kx, ci)] = folded W[co][ci][ky][kx]
            rc |= pm_pack_mfma(L, [&](int, int o, int tap, int i) { return A[((size_t)o * ci + i) * 9 + tap]; });
        pm->layers.push_back(std::move(L));
    }
    for (int u = 0; u < 5; ++u) {   // up_blocks.i.conv_transpose.0: ConvTranspose2d W [Cin][Cout][3][3]
        const int ci = PM_UP[u][0], co = PM_UP[u][1];
        const float* W = p;
        p += (size_t)ci * co * 9;
        const float* cb = p;
        p += co;
        avc_pm::Layer L{ci, co, 2, 2, 1, u == 4 ? 2 : 1, 0.f, {0, 0, 0, 0}, {}, {}};
        std::vector<float> A;
        for (int cls = 0; cls < 4; ++cls) {
            const int py = cls >> 1, px = cls & 1;
            const int nty = py == 0 ? 2 : 1, ntx = px == 0 ? 2 : 1;
            L.woff[cls] = (int)A.size();
            for (int o = 0; o < co; ++o)
                for (int i = 0; i < ci; ++i)
                    for (int a = 0; a < nty; ++a)
                        for (int bb = 0; bb < ntx; ++bb) {
                            const int ky = py == 0 ? 2 * a : 1, kx = px == 0 ? 2 * bb : 1;
                            A.push_back(W[(((size_t)i * co + o) * 3 + ky) * 3 + kx]);
                        }
        }
        rc |= upload(L.w, A);
        rc |= upload(L.b, std::vector<float>(cb, cb + co));
        if (ci % 16 == 0 && co % 16 == 0)   // class (py, px), tap (a, bb): W[ci][co][ky][kx]
            rc |= pm_pack_mfma(L, [&](int cls, int o, int tap, int i) {
                const int py = cls >> 1, px = cls & 1, ntx = px == 0 ? 2 : 1;
                const int a = tap / ntx, bb = tap - a * ntx;
                const int ky = py == 0 ? 2 * a : 1, kx = px == 0 ? 2 * bb : 1;
                return W[(((size_t)i * co + o) * 3 + ky) * 3 + kx];
            });
        pm->layers.push_back(std::move(L));
    }
    if ((size_t)(p - w) != n) rc |= fail("avc_pm_create: internal weight walk mismatch");
    if (rc) {
        avc_pm_destroy(pm);
        return 1;
    }
    *out = pm;
    return 0;
}

extern "C" void avc_pm_destroy(avc_pm* pm) {
    if (!pm) return;
    hipSetDevice(pm->device);
    delete pm;   // its buffers free themselves
}

// one layer: y = layer(x) over B windows of Hin x Win (the layer's input); layouts NCHW / NHWC as
// flagged (pm_mfma: NHWC both); mfma picks the matrix-core kernel for an eligible layer
static int pm_layer(avc_pm* pm, int l, const float* x, int B, int Hin, int Win, float* y, int in_nhwc,
                    int out_nhwc, bool mfma, hipStream_t s, int act_override = -1) {
    const avc_pm::Layer& L = pm->layers[l];
    PmConvArgs P{};
    P.x = x;
    P.w = L.w.p;
    P.wm = L.wm.p;
    P.bias = L.b.p;
    P.y = y;
    P.B = B;
    P.Cin = L.Cin;
    P.Hin = Hin;
    P.Win = Win;
    P.Cout = L.Cout;
    P.Ho = L.mode == 1 ? 2 * (Hin - 1) + 3 : (Hin + 2 - 3) / L.sh + 1;
    P.Wo = L.mode == 1 ? 2 * (Win - 1) + 3 : (Win + 2 - 3) / L.sw + 1;
    P.sh = L.sh;
    P.sw = L.sw;
    P.mode = L.mode;
    P.act = act_override >= 0 ? act_override : L.act;
    P.slope = L.slope;
    P.in_nhwc = in_nhwc;
    P.out_nhwc = out_nhwc;
    for (int c = 0; c < 4; ++c) {
        P.woff[c] = L.woff[c];
        P.wmoff[c] = L.wmoff[c];
    }
    mfma = mfma && L.mfma && in_nhwc && out_nhwc;
    const int ncls = L.mode == 1 ? 4 : 1;
    // columns of the largest output class (mode 1: class (0, 0)), per window and in all
    const long N1 = L.mode == 1 ? (long)((P.Ho + 1) / 2) * ((P.Wo + 1) / 2) : (long)P.Ho * P.Wo;
    const long N = (long)B * N1;
    // deterministic split-K for the layers whose output tiles leave the chip idle.  Chosen from the
    // window geometry only, never from B, so a window's summation order (and result) is the same
    // in any batch: pm_conv -- ~256 workgroups at B = 1, >= 8 K chunks of 16 per slice; pm_mfma --
    // >= 256 workgroups at a reference batch of 128 windows, >= 8 K chunks per slice
    const int MT = L.Cout >= 64 && !env_is("AVC_PM_MT", '2') ? 4 : 2;
    // N tiles of 16 output pixels per wave (MT = 4 layers): the workgroup covers 64 * NT pixels
    // (A/B, B = 256, MT = 4 layers: NT = 1 310k windows/s, 2 292k, 4 251k -- the smaller tiles balance
    // the CUs and leave registers for 5 waves per SIMD; the MT = 2 layer: NT = 2 50 us, NT = 1 54 us)
    const int nt_env = env_int("AVC_PM_NT", 0);
    const int NT = nt_env == 1 || nt_env == 2 || (nt_env == 4 && MT == 4) ? nt_env : (MT == 4 ? 1 : 2);
    const long wgs = mfma ? ((128 * N1 + 127) / 128) * ((L.Cout + 16 * MT - 1) / (16 * MT)) * ncls
                          : ((N1 + 63) / 64) * ((L.Cout + 63) / 64) * ncls;
    const int kchunks = mfma ? L.Cin / 16 * (L.mode == 1 ? 4 : 9) : (L.Cin * (L.mode == 1 ? 4 : 9) + 15) / 16;
    int ksplit = 1;
    // (the pm_mfma target, workgroups at the reference batch; A/B at B = 256: 64 -> 286k windows/s,
    // 128 -> 308k, 256 -> 310k, 512 -> 296k)
    const long ks_target = env_int("AVC_PM_KSWG", 256);
    if (mfma)
        while (wgs * ksplit < ks_target && kchunks >= 16 * ksplit) ksplit *= 2;
    else
        while (wgs * ksplit * 2 <= 256 && kchunks >= 8 * ksplit) ksplit *= 2;
    const size_t per = (size_t)B * L.Cout * P.Ho * P.Wo;
    // the edge layers on their own kernels (pm_conv's per-output arithmetic, bitwise): Cin = 1 into
    // NHWC, and Cout = 1 (its K slices summed in-thread in pm_reduce's order).  AVC_PM_EDGE=0: pm_conv
    const bool edge = !env_is("AVC_PM_EDGE", '0');
    if (edge && !mfma && L.mode == 0 && L.Cin == 1 && L.Cout == 32 && out_nhwc && ksplit == 1) {
        hipLaunchKernelGGL(pm_cin1<32>, dim3((unsigned)((B * (long)P.Ho * P.Wo + 255) / 256)), dim3(256), 0, s, P);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (edge && !mfma && L.mode == 1 && L.Cout == 1 && in_nhwc && L.Cin == 32) {
        P.ksplit = ksplit;
        // ksplit 2 on CI = 32 splits every class at ci = 16: the half-channel kernel (same bits)
        const bool halves = ksplit == 2 && !env_is("AVC_PM_COUT1H", '0');
        if (halves) hipLaunchKernelGGL(pm_cout1h<32>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, P);
        else hipLaunchKernelGGL(pm_cout1<32>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, P);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (ksplit > 1) {
        if (dalloc(pm->part, per * ksplit)) return 1;
        P.ksplit = ksplit;
        P.part = pm->part.p;
    }
    if (mfma) {
        const dim3 g((unsigned)((N + 64 * NT - 1) / (64 * NT)), (unsigned)((L.Cout + 16 * MT - 1) / (16 * MT)),
                     ncls * ksplit);
        const int m0 = L.mode == 0;
        if (MT == 2 && NT == 1) {
            if (m0) hipLaunchKernelGGL((pm_mfma<2, 0, 1>), g, dim3(256), 0, s, P);
            else hipLaunchKernelGGL((pm_mfma<2, 1, 1>), g, dim3(256), 0, s, P);
        } else if (MT == 2) {
            if (m0) hipLaunchKernelGGL((pm_mfma<2, 0, 2>), g, dim3(256), 0, s, P);
            else hipLaunchKernelGGL((pm_mfma<2, 1, 2>), g, dim3(256), 0, s, P);
        } else if (NT == 1) {
            if (m0) hipLaunchKernelGGL((pm_mfma<4, 0, 1>), g, dim3(256), 0, s, P);
            else hipLaunchKernelGGL((pm_mfma<4, 1, 1>), g, dim3(256), 0, s, P);
        } else if (NT == 4) {
            if (m0) hipLaunchKernelGGL((pm_mfma<4, 0, 4>), g, dim3(256), 0, s, P);
            else hipLaunchKernelGGL((pm_mfma<4, 1, 4>), g, dim3(256), 0, s, P);
        } else {
            if (m0) hipLaunchKernelGGL((pm_mfma<4, 0, 2>), g, dim3(256), 0, s, P);
            else hipLaunchKernelGGL((pm_mfma<4, 1, 2>), g, dim3(256), 0, s, P);
        }
    } else {
        hipLaunchKernelGGL(pm_conv, dim3((unsigned)((N + 63) / 64), (unsigned)((L.Cout + 63) / 64), ncls * ksplit),
                           dim3(256), 0, s, P);
    }
    HIPCHK(hipGetLastError());
    if (ksplit > 1) {
        hipLaunchKernelGGL(pm_reduce, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, s, P);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

extern "C" int avc_pm_forward(avc_pm* pm, const float* x, int B, int H, int W, float* y, void* stream) {
    if (!pm || !x || !y) return fail("avc_pm_forward: null argument");
    if (B <= 0) return fail("avc_pm_forward: batch size must be positive (got %d)", B);
    std::vector<std::array<int, 2>> hw;
    if (pm_shapes(H, W, hw)) return 1;
    HIPCHK(hipSetDevice(pm->device));
    const int nl = (int)pm->layers.size();
    pm->act.resize(nl);
    for (int l = 0; l + 1 < nl; ++l)
        if (dalloc(pm->act[l], (size_t)B * pm->layers[l].Cout * hw[l + 1][0] * hw[l + 1][1])) return 1;
    hipStream_t s = (hipStream_t)stream;
    // NHWC between layers (the matrix-core layers' layout); the network's own input and output
    // have one channel, so NCHW == NHWC there.  AVC_PM_MFMA=0: every layer on pm_conv (A/B runs).
    const bool mfma = !env_is("AVC_PM_MFMA", '0');
    const float* in = x;
    for (int l = 0; l < nl; ++l) {
        float* out = l + 1 < nl ? pm->act[l].p : y;
        if (pm_layer(pm, l, in, B, hw[l][0], hw[l][1], out, 1, 1, mfma, s)) return 1;
        in = out;
    }
    return 0;
}

// one block of the network on its own (DownSamplingBlock / UpSamplingBlock.forward,
// models/predictive_model.py:28-29, 50-51): NCHW in / out, pm_conv
extern "C" int avc_pm_block_shape(avc_pm* pm, int layer, int H, int W, int* C, int* Ho, int* Wo, int* Cin) {
    if (!pm || layer < 0 || layer >= (int)pm->layers.size()) return fail("avc_pm_block_shape: bad layer %d", layer);
    const avc_pm::Layer& L = pm->layers[layer];
    if (L.mode == 0 && (H < 2 || W < 2)) return fail("PredictiveModel: a %dx%d input to ReflectionPad2d(1) is too small", H, W);
    if (H < 1 || W < 1) return fail("PredictiveModel: empty %dx%d input", H, W);
    if (C) *C = L.Cout;
    if (Cin) *Cin = L.Cin;
    if (Ho) *Ho = L.mode == 1 ? 2 * (H - 1) + 3 : (H + 2 - 3) / L.sh + 1;
    if (Wo) *Wo = L.mode == 1 ? 2 * (W - 1) + 3 : (W + 2 - 3) / L.sw + 1;
    return 0;
}

extern "C" int avc_pm_block_forward(avc_pm* pm, int layer, const float* x, int B, int Cin, int H, int W, float* y,
                                    void* stream) {
    if (!pm || !x || !y) return fail("avc_pm_block_forward: null argument");
    if (B <= 0) return fail("avc_pm_block_forward: batch size must be positive (got %d)", B);
    int cin = 0;
    if (avc_pm_block_shape(pm, layer, H, W, nullptr, nullptr, nullptr, &cin)) return 1;
    if (Cin != cin)
        return fail("PredictiveModel block %d: expected input[B, %d, H, W], got %d channels", layer, cin, Cin);
    HIPCHK(hipSetDevice(pm->device));
    // the last block's tanh belongs to PredictiveModel.forward (predictive_model.py:106-107)
    const int act = pm->layers[layer].act == 2 ? 1 : pm->layers[layer].act;
    return pm_layer(pm, layer, x, B, H, W, y, 0, 0, false, (hipStream_t)stream, act);
}

// ---- VSMask protect loop (vsmask.py:160-213, utils/audio.py:77-116) ----------------------

// windows of the reference loop: range(0, T - W, S)
static int vsm_windows(int T, int W, int S) { return T > W ? (T - W + S - 1) / S : 0; }

extern "C" int avc_vsmask_windows(int T, int window_size, int future_step, int* n_windows) {
    if (window_size <= 0 || future_step <= 0)
        return fail("VSMask: window_size (%d) and future_step (%d) must be positive", window_size, future_step);
    if (T < 0) return fail("VSMask: negative frame count %d", T);
    if (n_windows) *n_windows = vsm_windows(T, window_size, future_step);
    return 0;
}

static int vsm_launch(VsmArgs& A, bool gather, hipStream_t s) {
    const size_t n = gather ? (size_t)A.B * A.nw * A.F * A.W : (size_t)A.B * A.F * A.T;
    if (n == 0) return 0;
    const unsigned g = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
    if (gather) hipLaunchKernelGGL(vsm_gather, dim3(g), dim3(256), 0, s, A);
    else hipLaunchKernelGGL(vsm_combine, dim3(g), dim3(256), 0, s, A);
    HIPCHK(hipGetLastError());
    return 0;
}

static void vsm_bands(VsmArgs& A) {
    A.low_end = (int)(A.F * 0.3);      // utils/audio.py:97-98, Python int() of the double product
    A.high_start = (int)(A.F * 0.7);
}

extern "C" int avc_vsmask_protect(avc_pm* pm, const float* mel, int B, int F, int T, const float* header, int Th,
                                  int window_size, int future_step, float eps1, float eps2, float eps3, float* out,
                                  void* stream) {
    if (!pm || !mel || !out) return fail("avc_vsmask_protect: null argument");
    if (B <= 0 || F <= 0 || T <= 0) return fail("avc_vsmask_protect: bad mel shape [%d, 1, %d, %d]", B, F, T);
    if (header && Th <= 0) return fail("avc_vsmask_protect: header length must be positive (got %d)", Th);
    if (mel == out) return fail("avc_vsmask_protect: out must not alias mel");
    int nw = 0;
    if (avc_vsmask_windows(T, window_size, future_step, &nw)) return 1;
    HIPCHK(hipSetDevice(pm->device));
    hipStream_t s = (hipStream_t)stream;
    VsmArgs A{};
    A.mel = mel;
    A.header = header;
    A.out = out;
    A.B = B;
    A.F = F;
    A.T = T;
    A.Th = header ? Th : 0;
    A.W = window_size;
    A.S = future_step;
    A.nw = nw;
    A.eps1 = eps1;
    A.eps2 = eps2;
    A.eps3 = eps3;
    vsm_bands(A);
    if (nw > 0) {
        int Ho = 0, Wo = 0;
        if (avc_pm_out_shape(F, window_size, &Ho, &Wo)) return 1;
        A.Ho = Ho;
        A.Wo = Wo;
        A.rows = std::min(F, Ho);      // the predictor's 95 rows cropped to the mel's 80 (SURVEY 2 note A)
        const size_t nwin = (size_t)B * nw;
        if (dalloc(pm->vwin, nwin * F * window_size) || dalloc(pm->vy, nwin * Ho * Wo)) return 1;
        A.win = pm->vwin.p;
        A.y = pm->vy.p;
        if (vsm_launch(A, true, s)) return 1;
        if (avc_pm_forward(pm, pm->vwin.p, (int)nwin, F, window_size, pm->vy.p, stream)) return 1;
    }
    return vsm_launch(A, false, s);
}

extern "C" int avc_vsmask_band_clamp(int device, const float* x, int B, int F, int T, float eps1, float eps2,
                                     float eps3, float* out, void* stream) {
    if (!x || !out) return fail("avc_vsmask_band_clamp: null argument");
    if (B <= 0 || F <= 0 || T <= 0) return fail("avc_vsmask_band_clamp: bad shape [%d, %d, %d]", B, F, T);
    HIPCHK(hipSetDevice(device));
    VsmArgs A{};
    A.mel = x;
    A.out = out;
    A.B = B;
    A.F = F;
    A.T = T;
    A.eps1 = eps1;
    A.eps2 = eps2;
    A.eps3 = eps3;
    A.mode = 2;
    vsm_bands(A);
    return vsm_launch(A, false, (hipStream_t)stream);
}

extern "C" int avc_vsmask_apply_header(int device, const float* mel, int B, int F, int T, const float* header, int Th,
                                       float* out, void* stream) {
    if (!mel || !header || !out) return fail("avc_vsmask_apply_header: null argument");
    if (B <= 0 || F <= 0 || T <= 0 || Th <= 0)
        return fail("avc_vsmask_apply_header: bad shapes mel [%d, 1, %d, %d], header length %d", B, F, T, Th);
    HIPCHK(hipSetDevice(device));
    VsmArgs A{};
    A.mel = mel;
    A.header = header;
    A.out = out;
    A.B = B;
    A.F = F;
    A.T = T;
    A.Th = Th;
    A.mode = 1;
    vsm_bands(A);
    return vsm_launch(A, false, (hipStream_t)stream);
}
