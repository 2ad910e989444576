// libavc host side of the mel front / back end (included at the end of avc_api.hip):
// filter bank, window and twiddle tables, workspace, the launch sequences of
// file2mel / mel2wav / griffin_lim (data_utils.py:16-197).

namespace avc {
template <int LOGN>
__global__ void dsp_wav2mel(DspArgs A);
__global__ void dsp_mel2mag(DspArgs A);
__global__ void dsp_transpose(DspArgs A);
template <int LOGN>
__global__ void dsp_gl_frames(DspArgs A);
__global__ void dsp_ola(DspArgs A);
__global__ void dsp_ola4(DspArgs A);
__global__ void dsp_wss(DspArgs A);
__global__ void dsp_deemph(DspArgs A);
}  // namespace avc

static constexpr int DSP_THREADS_H = 256;   // = DSP_THREADS of avc_dsp.hip (dsp_mel2mag: DSP_MT = 8 frames per workgroup)

// the FFT kernels are instantiated per log2 n_fft (4 .. 12)
typedef void (*DspKernel)(avc::DspArgs);
static DspKernel dsp_kernel(bool gl, int logN) {
#define AVC_DSP_K(LG) \
    case LG: return gl ? (DspKernel)avc::dsp_gl_frames<LG> : (DspKernel)avc::dsp_wav2mel<LG>;
    switch (logN) {
        AVC_DSP_K(4) AVC_DSP_K(5) AVC_DSP_K(6) AVC_DSP_K(7) AVC_DSP_K(8)
        AVC_DSP_K(9) AVC_DSP_K(10) AVC_DSP_K(11) AVC_DSP_K(12)
    }
#undef AVC_DSP_K
    return nullptr;
}

struct avc_dsp {
    int device = 0;
    avc_dsp_cfg cfg{};
    int N = 0, logN = 0, F = 0;
    DevBuf window, twiddle, mel_basis, mel_range, inv_mel;
    DevBuf spect, frames, y, wss;     // workspace (grow-only)
    DevBuf tprev;                     // flavor 1: Griffin-Lim momentum state [B][Tf][F] complex
    // avc_dsp_set_profiling: per-kernel HIP events (launch count, device ms)
    bool prof = false;
    std::map<std::string, std::pair<long, double>> prof_k;
};

// launch through `fn`, bracketed by HIP events on stream s while profiling
template <class Fn>
static int dsp_launch(avc_dsp* d, const char* name, hipStream_t s, Fn fn) {
    if (!d->prof) {
        fn();
        return 0;
    }
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, s));
    fn();
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    auto& k = d->prof_k[name];
    k.first += 1;
    k.second += ms;
    return 0;
}

namespace {
// librosa 0.8 hz_to_mel / mel_to_hz, htk=False (Slaney): linear below 1 kHz, log above
double dsp_hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp,
                 logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double dsp_mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp,
                 logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

int dsp_check(const avc_dsp_cfg* c, int& logN) {
    if (!c) return fail("avc_dsp: null config");
    const int N = c->n_fft;
    if (N < 16 || N > 4096 || (N & (N - 1))) return fail("avc_dsp: n_fft must be a power of two in [16, 4096], got %d", N);
    logN = 0;
    while ((1 << logN) < N) ++logN;
    if (c->win_length < 1 || c->win_length > N) return fail("avc_dsp: win_length %d must be in [1, n_fft]", c->win_length);
    if (c->hop_length < 1) return fail("avc_dsp: hop_length must be positive");
    if (c->n_mels < 1 || c->n_mels > 1024) return fail("avc_dsp: n_mels must be in [1, 1024]");
    if (c->sample_rate < 1) return fail("avc_dsp: sample_rate must be positive");
    if (c->pad_mode != 0 && c->pad_mode != 1) return fail("avc_dsp: pad_mode must be 0 (reflect) or 1 (constant)");
    if (c->flavor != 0 && c->flavor != 1) return fail("avc_dsp: flavor must be 0 (data_utils) or 1 (utils/audio.py)");
    if (c->flavor == 1) {
        if (c->preemph != 0.f) return fail("avc_dsp: the torchaudio flavor has no pre-emphasis (preemph must be 0)");
        return 0;
    }
    if (!(c->max_db != 0.f)) return fail("avc_dsp: max_db must be non-zero");
    return 0;
}

void dsp_mel_basis(const avc_dsp_cfg& c, std::vector<float>& W);
void dsp_inv_mel(const avc_dsp_cfg& c, const std::vector<float>& W, std::vector<float>& inv);

// torchaudio.functional.melscale_fbanks(n_freqs, 0, sample_rate // 2, n_mels, sample_rate, norm=None,
// mel_scale="htk") as MelSpectrogram builds it, transposed to [n_mels][F] (fb^T); float64 then
// float32 (torchaudio evaluates the same formulas in float32: parity unpinned, torchaudio absent)
void dsp_mel_basis_htk(const avc_dsp_cfg& c, std::vector<float>& W) {
    const int F = c.n_fft / 2 + 1, nm = c.n_mels;
    const double fmax = (double)(c.sample_rate / 2);
    auto h2m = [](double f) { return 2595.0 * std::log10(1.0 + f / 700.0); };
    auto m2h = [](double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); };
    std::vector<double> fp(nm + 2);
    const double mmax = h2m(fmax);
    for (int i = 0; i < nm + 2; ++i) fp[i] = m2h(mmax * i / (nm + 1));
    W.assign((size_t)nm * F, 0.f);
    for (int m = 0; m < nm; ++m)
        for (int f = 0; f < F; ++f) {
            const double fr = fmax * f / (F - 1);
            const double down = (fr - fp[m]) / (fp[m + 1] - fp[m]), up = (fp[m + 2] - fr) / (fp[m + 2] - fp[m + 1]);
            W[(size_t)m * F + f] = (float)std::max(0.0, std::min(down, up));
        }
}

// InverseMelScale's solve (torch.linalg.lstsq of fb^T X = mel, full row rank: the minimum-norm
// solution) as one matrix: pinv(W) = W^T (W W^T)^-1, [F][n_mels], by a float64 Cholesky of W W^T
int dsp_pinv(const avc_dsp_cfg& c, const std::vector<float>& W, std::vector<float>& inv) {
    const int F = c.n_fft / 2 + 1, nm = c.n_mels;
    std::vector<double> G((size_t)nm * nm), Lc((size_t)nm * nm, 0.0);
    for (int i = 0; i < nm; ++i)
        for (int j = 0; j < nm; ++j) {
            double p = 0.0;
            for (int f = 0; f < F; ++f) p += (double)W[(size_t)i * F + f] * W[(size_t)j * F + f];
            G[(size_t)i * nm + j] = p;
        }
    for (int j = 0; j < nm; ++j) {
        double d = G[(size_t)j * nm + j];
        for (int k = 0; k < j; ++k) d -= Lc[(size_t)j * nm + k] * Lc[(size_t)j * nm + k];
        if (!(d > 1e-12 * std::max(1.0, G[(size_t)j * nm + j])))
            return fail("avc_dsp: the mel filter bank is rank deficient (filter %d); no least-squares inverse", j);
        Lc[(size_t)j * nm + j] = std::sqrt(d);
        for (int i = j + 1; i < nm; ++i) {
            double s = G[(size_t)i * nm + j];
            for (int k = 0; k < j; ++k) s -= Lc[(size_t)i * nm + k] * Lc[(size_t)j * nm + k];
            Lc[(size_t)i * nm + j] = s / Lc[(size_t)j * nm + j];
        }
    }
    // (W W^T)^-1 column by column, then inv = W^T (W W^T)^-1
    std::vector<double> Gi((size_t)nm * nm), y(nm);
    for (int col = 0; col < nm; ++col) {
        for (int i = 0; i < nm; ++i) {
            double s = i == col ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) s -= Lc[(size_t)i * nm + k] * y[k];
            y[i] = s / Lc[(size_t)i * nm + i];
        }
        for (int i = nm - 1; i >= 0; --i) {
            double s = y[i];
            for (int k = i + 1; k < nm; ++k) s -= Lc[(size_t)k * nm + i] * Gi[(size_t)k * nm + col];
            Gi[(size_t)i * nm + col] = s / Lc[(size_t)i * nm + i];
        }
    }
    inv.assign((size_t)F * nm, 0.f);
    for (int f = 0; f < F; ++f)
        for (int m = 0; m < nm; ++m) {
            double s = 0.0;
            for (int j = 0; j < nm; ++j) s += (double)W[(size_t)j * F + f] * Gi[(size_t)j * nm + m];
            inv[(size_t)f * nm + m] = (float)s;
        }
    return 0;
}

// the context's filter bank [n_mels][F] and its inverse [F][n_mels] for either flavor
int dsp_tables(const avc_dsp_cfg& c, std::vector<float>& W, std::vector<float>& inv) {
    if (c.flavor == 1) {
        dsp_mel_basis_htk(c, W);
        return dsp_pinv(c, W, inv);
    }
    dsp_mel_basis(c, W);
    dsp_inv_mel(c, W, inv);
    return 0;
}

// librosa.filters.mel(sr, n_fft, n_mels) (fmin 0, fmax sr/2, htk=False, norm='slaney');
// float32 like librosa
void dsp_mel_basis(const avc_dsp_cfg& c, std::vector<float>& W) {
    const int F = c.n_fft / 2 + 1, nm = c.n_mels;
    std::vector<double> fft(F), mel_f(nm + 2);
    for (int f = 0; f < F; ++f) fft[f] = (double)f * (c.sample_rate / 2.0) / (F - 1);
    const double lo = dsp_hz_to_mel(0.0), hi = dsp_hz_to_mel(c.sample_rate / 2.0);
    for (int i = 0; i < nm + 2; ++i) mel_f[i] = dsp_mel_to_hz(lo + (hi - lo) * i / (nm + 1));
    W.assign((size_t)nm * F, 0.f);
    for (int i = 0; i < nm; ++i) {
        const double d0 = mel_f[i + 1] - mel_f[i], d1 = mel_f[i + 2] - mel_f[i + 1];
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int f = 0; f < F; ++f) {
            const double lower = -(mel_f[i] - fft[f]) / d0, upper = (mel_f[i + 2] - fft[f]) / d1;
            // float32 store, then the in-place float64 enorm scale rounded back (numpy semantics)
            W[(size_t)i * F + f] = (float)((double)(float)std::max(0.0, std::min(lower, upper)) * enorm);
        }
    }
}

// inv_mel_matrix (data_utils.py:16-32): M^T diag(d), d_j = 1 / sum_i (M M^T)_ij (|.| > 1e-8)
void dsp_inv_mel(const avc_dsp_cfg& c, const std::vector<float>& W, std::vector<float>& inv) {
    const int F = c.n_fft / 2 + 1, nm = c.n_mels;
    std::vector<double> d(nm, 0.0);
    for (int i = 0; i < nm; ++i)
        for (int j = 0; j < nm; ++j) {
            double p = 0.0;
            for (int f = 0; f < F; ++f) p += (double)W[(size_t)i * F + f] * W[(size_t)j * F + f];
            d[j] += p;
        }
    for (int j = 0; j < nm; ++j) d[j] = std::fabs(d[j]) > 1e-8 ? 1.0 / d[j] : d[j];
    inv.assign((size_t)F * nm, 0.f);
    for (int f = 0; f < F; ++f)
        for (int m = 0; m < nm; ++m) inv[(size_t)f * nm + m] = (float)(W[(size_t)m * F + f] * d[m]);
}

DspArgs dsp_args(const avc_dsp* d, int B, int Tf) {
    DspArgs A{};
    A.B = B;
    A.N = d->N;
    A.logN = d->logN;
    A.F = d->F;
    A.hop = d->cfg.hop_length;
    A.Tf = Tf;
    A.n_mels = d->cfg.n_mels;
    A.pad_mode = d->cfg.pad_mode;
    A.preemph = d->cfg.preemph;
    A.ref_db = d->cfg.ref_db;
    A.max_db = d->cfg.max_db;
    A.window = d->window.p;
    A.twiddle = d->twiddle.p;
    A.mel_basis = d->mel_basis.p;
    A.mel_range = reinterpret_cast<const int32_t*>(d->mel_range.p);
    A.inv_mel = d->inv_mel.p;
    A.flavor = d->cfg.flavor;
    return A;
}

// LDS of dsp_gl_frames: the padded complex buffer and the padded twiddle table
size_t dsp_frame_lds(int N) { return (size_t)dsp_zlen(N) * 8 + (size_t)dsp_twlen(N) * 8; }

// Griffin-Lim from d->spect ([B][Tf][F]) to wav [B][hop*(Tf-1)], de-emphasised if deemph
int dsp_run_gl(avc_dsp* d, int B, int Tf, int n_iter, float* wav, bool deemph, hipStream_t s,
               float momentum = 0.f, const float* angles0 = nullptr) {
    const int Ly = d->cfg.hop_length * (Tf - 1);
    if (dalloc(d->frames, (size_t)B * Tf * d->N) || dalloc(d->y, (size_t)B * std::max(Ly, 1)) ||
        dalloc(d->wss, (size_t)std::max(Ly, 4)))
        return 1;
    if (d->cfg.flavor == 1 && dalloc(d->tprev, (size_t)B * Tf * d->F * 2)) return 1;
    DspArgs A = dsp_args(d, B, Tf);
    A.momentum = momentum;
    A.angles0 = angles0;
    A.tprev = d->cfg.flavor == 1 ? d->tprev.p : nullptr;
    A.spect = d->spect.p;
    A.frames = d->frames.p;
    A.y = deemph ? d->y.p : wav;
    A.wss = d->wss.p;
    A.x = nullptr;
    A.L = Ly;
    A.Ly = Ly;
    A.wav = wav;
    const dim3 gf((Tf + 1) / 2, B), go((Ly + DSP_THREADS_H - 1) / DSP_THREADS_H, B);
    const dim3 go4((Ly + 4 * DSP_THREADS_H - 1) / (4 * DSP_THREADS_H), B);
    // four samples per thread: 16-byte frame loads need hop % 4 == 0 (n_fft / 2 is) and an aligned y
    const bool ola4 = d->cfg.hop_length % 4 == 0 && ((uintptr_t)A.y & 15) == 0;
    A.vec4 = ola4 ? 1 : 0;
    const size_t lds = dsp_frame_lds(d->N);
    int rc = 0;
    if (ola4 && Ly > 0)
        rc |= dsp_launch(d, "dsp_wss", s, [&] {
            hipLaunchKernelGGL(avc::dsp_wss, dim3((Ly + DSP_THREADS_H - 1) / DSP_THREADS_H), dim3(DSP_THREADS_H), 0, s, A);
        });
    auto frames = [&](const char* nm) {
        rc |= dsp_launch(d, nm, s, [&] { hipLaunchKernelGGL(dsp_kernel(true, d->logN), gf, dim3(DSP_THREADS_H), lds, s, A); });
    };
    auto ola = [&] {
        if (Ly <= 0) return;
        if (ola4)
            rc |= dsp_launch(d, "dsp_ola", s, [&] { hipLaunchKernelGGL(avc::dsp_ola4, go4, dim3(DSP_THREADS_H), 0, s, A); });
        else
            rc |= dsp_launch(d, "dsp_ola", s, [&] { hipLaunchKernelGGL(avc::dsp_ola, go, dim3(DSP_THREADS_H), 0, s, A); });
    };
    A.init = 1;
    frames("dsp_gl_frames<init>");
    A.init = 0;
    for (int it = 0; it < n_iter; ++it) {
        ola();
        frames("dsp_gl_frames");
    }
    ola();
    if (Ly > 0 && deemph)
        rc |= dsp_launch(d, "dsp_deemph", s, [&] { hipLaunchKernelGGL(avc::dsp_deemph, dim3(B), dim3(1024), 0, s, A); });
    HIPCHK(hipGetLastError());
    return rc;
}
}  // namespace

extern "C" int avc_dsp_frames(const avc_dsp_cfg* cfg, int n_samples) {
    int logN;
    if (dsp_check(cfg, logN)) return -1;
    if (n_samples < 1) return fail("avc_dsp_frames: need at least one sample"), -1;
    return 1 + n_samples / cfg->hop_length;
}

extern "C" int avc_dsp_mel_basis(const avc_dsp_cfg* cfg, float* mel_basis, float* inv_mel) {
    int logN;
    if (dsp_check(cfg, logN)) return 1;
    std::vector<float> W, inv;
    if (dsp_tables(*cfg, W, inv)) return 1;
    if (mel_basis) std::copy(W.begin(), W.end(), mel_basis);
    if (inv_mel) std::copy(inv.begin(), inv.end(), inv_mel);
    return 0;
}

extern "C" int avc_dsp_create(int device, const avc_dsp_cfg* cfg, avc_dsp** out) {
    if (!out) return fail("avc_dsp_create: null output");
    int logN;
    if (dsp_check(cfg, logN)) return 1;
    HIPCHK(hipSetDevice(device));
    avc_dsp* d = new avc_dsp();
    d->device = device;
    d->cfg = *cfg;
    d->N = cfg->n_fft;
    d->logN = logN;
    d->F = cfg->n_fft / 2 + 1;
    const int N = d->N, F = d->F, nm = cfg->n_mels, win = cfg->win_length;
    // periodic Hann(win_length) (scipy get_window fftbins=True) centered in n_fft
    std::vector<float> w(N, 0.f), tw(N), W, inv;
    const int lpad = (N - win) / 2;
    for (int n = 0; n < win; ++n) w[lpad + n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / win));
    for (int k = 0; k < N / 2; ++k) {
        tw[2 * k] = (float)std::cos(2.0 * M_PI * k / N);
        tw[2 * k + 1] = (float)-std::sin(2.0 * M_PI * k / N);
    }
    if (dsp_tables(*cfg, W, inv)) {
        delete d;
        return 1;
    }
    std::vector<float> range(2 * nm);
    for (int m = 0; m < nm; ++m) {
        int lo = F, hi = 0;
        for (int f = 0; f < F; ++f)
            if (W[(size_t)m * F + f] != 0.f) {
                lo = std::min(lo, f);
                hi = f + 1;
            }
        if (hi == 0) lo = 0;
        int32_t r[2] = {lo, hi};
        std::memcpy(&range[2 * m], r, sizeof r);
    }
    int rc = 0;
    rc |= upload(d->window, w);
    rc |= upload(d->twiddle, tw);
    rc |= upload(d->mel_basis, W);
    std::vector<float> invT((size_t)nm * F);   // device copy transposed [n_mels][F]
    for (int f = 0; f < F; ++f)
        for (int m = 0; m < nm; ++m) invT[(size_t)m * F + f] = inv[(size_t)f * nm + m];
    rc |= upload(d->inv_mel, invT);
    rc |= upload(d->mel_range, range);
    if (!rc) {
        const size_t lds = dsp_frame_lds(N), lds_mel = lds + (size_t)2 * F * 4;
        if (lds_mel > 64 * 1024)
            HIPCHK(hipFuncSetAttribute((const void*)dsp_kernel(false, logN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_mel));
        if (lds > 64 * 1024)
            HIPCHK(hipFuncSetAttribute((const void*)dsp_kernel(true, logN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    if (rc) {
        avc_dsp_destroy(d);
        return 1;
    }
    *out = d;
    return 0;
}

extern "C" void avc_dsp_destroy(avc_dsp* d) {
    if (!d) return;
    delete d;   // its buffers free themselves
}

extern "C" int avc_dsp_wav2mel(avc_dsp* d, const float* wav, int B, int L, const float* mean, const float* std_,
                               int transpose, float* mel, void* stream) {
    if (!d || !wav || !mel) return fail("avc_dsp_wav2mel: null argument");
    if (B < 1 || L < 1) return fail("avc_dsp_wav2mel: need B >= 1 utterances of L >= 1 samples");
    if ((mean == nullptr) != (std_ == nullptr)) return fail("avc_dsp_wav2mel: give both mean and std, or neither");
    if (d->cfg.flavor == 1 && mean) return fail("avc_dsp_wav2mel: the torchaudio flavor takes no mean / std");
    HIPCHK(hipSetDevice(d->device));
    const int Tf = 1 + L / d->cfg.hop_length;
    DspArgs A = dsp_args(d, B, Tf);
    A.x = wav;
    A.L = L;
    A.mean = mean;
    A.std = std_;
    A.transpose = transpose ? 1 : 0;
    A.mel_out = mel;
    // (sized from dsp_zlen: the old (N + N/32) complex entries undercounted the padded buffer by
    // up to 1.5 KB, covered only by the allocation granularity)
    const size_t lds = dsp_frame_lds(d->N) + (size_t)2 * d->F * 4;
    if (dsp_launch(d, "dsp_wav2mel", (hipStream_t)stream, [&] {
            hipLaunchKernelGGL(dsp_kernel(false, d->logN), dim3((Tf + 1) / 2, B), dim3(DSP_THREADS_H), lds, (hipStream_t)stream, A);
        }))
        return 1;
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int avc_dsp_mel2wav(avc_dsp* d, const float* mel, int B, int Tf, int transpose, const float* mean,
                               const float* std_, int n_iter, float* wav, void* stream) {
    if (!d || !mel || !wav) return fail("avc_dsp_mel2wav: null argument");
    if (B < 1 || Tf < 2) return fail("avc_dsp_mel2wav: need B >= 1 utterances of Tf >= 2 frames");
    if (n_iter < 0) return fail("avc_dsp_mel2wav: n_iter must be >= 0");
    if ((mean == nullptr) != (std_ == nullptr)) return fail("avc_dsp_mel2wav: give both mean and std, or neither");
    if (d->cfg.flavor != 0) return fail("avc_dsp_mel2wav: a torchaudio-flavor context inverts with avc_dsp_ta_mel2wav");
    HIPCHK(hipSetDevice(d->device));
    if (dalloc(d->spect, (size_t)B * Tf * d->F)) return 1;
    DspArgs A = dsp_args(d, B, Tf);
    A.mel_in = mel;
    A.mean = mean;
    A.std = std_;
    A.transpose = transpose ? 1 : 0;
    A.spect_out = d->spect.p;
    if (dsp_launch(d, "dsp_mel2mag", (hipStream_t)stream, [&] {
            hipLaunchKernelGGL(avc::dsp_mel2mag, dim3((Tf + 7) / 8, B), dim3(DSP_THREADS_H), (size_t)8 * d->cfg.n_mels * 4,
                               (hipStream_t)stream, A);
        }))
        return 1;
    HIPCHK(hipGetLastError());
    return dsp_run_gl(d, B, Tf, n_iter, wav, true, (hipStream_t)stream);
}

extern "C" int avc_dsp_griffin_lim(avc_dsp* d, const float* spect, int B, int Tf, int n_iter, float* wav,
                                   void* stream) {
    if (!d || !spect || !wav) return fail("avc_dsp_griffin_lim: null argument");
    if (B < 1 || Tf < 2) return fail("avc_dsp_griffin_lim: need B >= 1 spectrograms of Tf >= 2 frames");
    if (n_iter < 0) return fail("avc_dsp_griffin_lim: n_iter must be >= 0");
    if (d->cfg.flavor != 0) return fail("avc_dsp_griffin_lim: a torchaudio-flavor context inverts with avc_dsp_ta_mel2wav");
    HIPCHK(hipSetDevice(d->device));
    if (dalloc(d->spect, (size_t)B * Tf * d->F)) return 1;
    DspArgs A = dsp_args(d, B, Tf);
    A.spect = spect;
    A.spect_out = d->spect.p;
    hipLaunchKernelGGL(avc::dsp_transpose, dim3((d->F + DSP_THREADS_H - 1) / DSP_THREADS_H, Tf, B),
                       dim3(DSP_THREADS_H), 0, (hipStream_t)stream, A);
    HIPCHK(hipGetLastError());
    return dsp_run_gl(d, B, Tf, n_iter, wav, false, (hipStream_t)stream);
}

extern "C" int avc_dsp_ta_mel2wav(avc_dsp* d, const float* mel, int B, int Tf, int n_iter, float momentum,
                                  const float* angles0, float* wav, void* stream) {
    if (!d || !mel || !wav) return fail("avc_dsp_ta_mel2wav: null argument");
    if (d->cfg.flavor != 1) return fail("avc_dsp_ta_mel2wav: needs a flavor-1 (utils/audio.py) context");
    if (B < 1 || Tf < 2) return fail("avc_dsp_ta_mel2wav: need B >= 1 mels of Tf >= 2 frames");
    if (n_iter < 0) return fail("avc_dsp_ta_mel2wav: n_iter must be >= 0");
    if (!(momentum >= 0.f && momentum < 1.f)) return fail("avc_dsp_ta_mel2wav: momentum must be in [0, 1)");
    HIPCHK(hipSetDevice(d->device));
    if (dalloc(d->spect, (size_t)B * Tf * d->F)) return 1;
    DspArgs A = dsp_args(d, B, Tf);
    A.mel_in = mel;
    A.transpose = 1;
    A.spect_out = d->spect.p;
    if (dsp_launch(d, "dsp_mel2mag", (hipStream_t)stream, [&] {
            hipLaunchKernelGGL(avc::dsp_mel2mag, dim3((Tf + 7) / 8, B), dim3(DSP_THREADS_H), (size_t)8 * d->cfg.n_mels * 4,
                               (hipStream_t)stream, A);
        }))
        return 1;
    HIPCHK(hipGetLastError());
    return dsp_run_gl(d, B, Tf, n_iter, wav, false, (hipStream_t)stream, momentum, angles0);
}

extern "C" int avc_dsp_set_profiling(avc_dsp* d, int enable) {
    if (!d) return fail("avc_dsp_set_profiling: null dsp");
    d->prof = enable != 0;
    d->prof_k.clear();
    return 0;
}

extern "C" int avc_dsp_profile_count(avc_dsp* d) { return d ? (int)d->prof_k.size() : 0; }

extern "C" int avc_dsp_profile_kernel(avc_dsp* d, int i, char* name, int name_len, long* launches, double* total_ms) {
    if (!d || i < 0 || i >= (int)d->prof_k.size()) return fail("avc_dsp_profile_kernel: bad index");
    auto it = d->prof_k.begin();
    std::advance(it, i);
    if (name && name_len > 0) {
        strncpy(name, it->first.c_str(), name_len - 1);
        name[name_len - 1] = 0;
    }
    if (launches) *launches = it->second.first;
    if (total_ms) *total_ms = it->second.second;
    return 0;
}
