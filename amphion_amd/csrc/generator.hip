// The amp_gen handle: descriptor checks, weight loading and weight-norm folding, workspace, profiling ring and the staged forward
// (conv_pre, per stage ConvTranspose + resblocks + MRF, conv_post) on the convs and fused forms of conv_host.hip.
#include <math.h>
#include <stdio.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "amp_host.h"

using namespace amp;

// ------------------------------------------------------------------------------------------------
// generator handle
// ------------------------------------------------------------------------------------------------
struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; }
};

struct ResBlock {
    int k = 0;
    std::vector<int> dil;
    std::vector<std::unique_ptr<amp_conv>> c1, c2;  // type 2 uses c1 only
    std::vector<ActParams> acts;
};

struct amp_gen {
    amp_gen_desc d{};
    std::map<std::string, std::vector<int64_t>> expected;  // key -> shape
    std::map<std::string, HostTensor> w;
    bool finalized = false;
    int hop = 1;
    std::vector<int> ch;  // channels after each stage
    std::unique_ptr<amp_conv> conv_pre, cond;
    std::vector<std::unique_ptr<amp_conv>> ups;
    std::vector<ResBlock> rbs;
    ActParams act_post;
    float* post_w_dev = nullptr;
    float* post_b_dev = nullptr;
    int post_cin = 0;
    std::vector<float*> dev_allocs;
    // profiling: a ring of event sets, one per forward, so that a caller can time EVERY forward of a region
    // without synchronising in between (bench.py reads them after its closing fence)
    struct ProfSlot {
        hipEvent_t ev_begin = nullptr, ev_end = nullptr;
        std::vector<hipEvent_t> ev_mrf;  // begin/end per (batch group, stage)
        std::vector<hipEvent_t> ev_rb;   // per (batch group, stage): n_kernels + 1 marks around the resblocks
        std::vector<std::string> rb_kernels;   // per (stage, resblock): the distinct kernels its launches ran, " | "-joined (first batch group)
        int ev_groups = 0;
        bool valid = false;
    };
    std::vector<ProfSlot> prof;          // empty = profiling off
    size_t prof_count = 0;               // forwards recorded so far
    RangeGuard guard;                    // this handle's f16 operand-range word (allocated by finalize on its device)
    // concurrent resblocks (small launches): n_kernels - 1 side streams, per stage one fork event and n_kernels - 1 join events
    std::vector<hipStream_t> side;
    std::vector<hipEvent_t> ev_side;
    // One launch sequence of this handle at a time: the side streams, their fork / join events, the profiling ring and the
    // range-guard word are per HANDLE, so two host threads (or two caller streams) enqueueing forwards of the same generator take turns
    // on the HOST -- each sequence's event records and waits are then issued as a unit (a wait binds to the record that precedes it in
    // issue order) and the device-side order per side stream is the issue order.  The forwards still overlap on the device.
    std::mutex launch_mu;
    ~amp_gen() {
        guard_free(guard);
        for (auto s_ : side) (void)hipStreamDestroy(s_);
        for (auto e : ev_side) (void)hipEventDestroy(e);
        for (float* p : dev_allocs) (void)hipFree(p);
        for (auto& p : prof) {
            if (p.ev_begin) (void)hipEventDestroy(p.ev_begin);
            if (p.ev_end) (void)hipEventDestroy(p.ev_end);
            for (auto e : p.ev_mrf) (void)hipEventDestroy(e);
            for (auto e : p.ev_rb) (void)hipEventDestroy(e);
        }
    }
};

static void expect_conv(amp_gen* g, const std::string& p, int cout, int cin, int k, bool transposed, bool wn, bool bias) {
    const int64_t d0 = transposed ? cin : cout, d1 = transposed ? cout : cin;
    if (bias) g->expected[p + ".bias"] = {cout};
    // both the weight-normed and the folded form are accepted
    (void)wn;
    g->expected[p + ".weight_g"] = {d0, 1, 1};
    g->expected[p + ".weight_v"] = {d0, d1, k};
    g->expected[p + ".weight"] = {d0, d1, k};
}

static void expect_act(amp_gen* g, const std::string& p, int c) {
    g->expected[p + ".act.alpha"] = {c};
    if (g->d.activation == AMP_ACT_SNAKEBETA) g->expected[p + ".act.beta"] = {c};
    g->expected[p + ".upsample.filter"] = {1, 1, 12};
    g->expected[p + ".downsample.lowpass.filter"] = {1, 1, 12};
}

static std::string ups_key(const amp_gen* g, int i) {
    // BigVGAN nests each upsampler in a 1-element ModuleList (bigvgan.py:261-276)
    return g->d.arch == AMP_ARCH_BIGVGAN ? "ups." + std::to_string(i) + ".0" : "ups." + std::to_string(i);
}

extern "C" {

int amp_gen_create(const amp_gen_desc* desc, amp_gen** out) {
    if (!desc || !out) { set_error("amp_gen_create: null argument"); return AMP_ERR_INVALID; }
    const amp_gen_desc& d = *desc;
    if (d.arch < AMP_ARCH_HIFIGAN || d.arch > AMP_ARCH_HIFIGAN_VITS) { set_error("amp_gen_create: unknown arch %d", d.arch); return AMP_ERR_INVALID; }
    if (d.n_in <= 0 || d.upsample_initial_channel <= 0 || d.n_stages <= 0 || d.n_stages > AMP_MAX_STAGES ||
        d.n_kernels <= 0 || d.n_kernels > AMP_MAX_KERNELS || (d.resblock_type != 1 && d.resblock_type != 2)) {
        set_error("amp_gen_create: bad descriptor (n_in=%d C0=%d stages=%d kernels=%d resblock=%d)", d.n_in,
                  d.upsample_initial_channel, d.n_stages, d.n_kernels, d.resblock_type);
        return AMP_ERR_INVALID;
    }
    if (d.arch == AMP_ARCH_BIGVGAN && d.activation != AMP_ACT_SNAKE && d.activation != AMP_ACT_SNAKEBETA) {
        // bigvgan.py:132-135 raises NotImplementedError for anything else
        set_error("activation incorrectly specified. check the config file and look for 'activation'.");
        return AMP_ERR_UNSUPPORTED;
    }
    if ((d.upsample_initial_channel >> d.n_stages) <= 0) { set_error("amp_gen_create: upsample_initial_channel too small"); return AMP_ERR_INVALID; }
    auto g = std::make_unique<amp_gen>();
    g->d = d;
    if (d.arch != AMP_ARCH_BIGVGAN) g->d.activation = AMP_ACT_LRELU;
    const bool vits = d.arch == AMP_ARCH_HIFIGAN_VITS;
    int c0 = d.upsample_initial_channel;
    expect_conv(g.get(), "conv_pre", c0, d.n_in, 7, false, !vits, true);
    g->hop = 1;
    int ch = c0;
    for (int i = 0; i < d.n_stages; ++i) {
        const int u = d.upsample_rates[i], k = d.upsample_kernel_sizes[i];
        if (u <= 0 || k < u) { set_error("amp_gen_create: stage %d rate=%d kernel=%d", i, u, k); return AMP_ERR_INVALID; }
        if ((k - u) % 2 != 0) { set_error("amp_gen_create: stage %d: kernel-rate must be even (output length = rate*T)", i); return AMP_ERR_UNSUPPORTED; }
        const int cin = c0 >> i, cout = c0 >> (i + 1);
        expect_conv(g.get(), ups_key(g.get(), i), cout, cin, k, true, true, true);
        g->hop *= u;
        ch = cout;
        g->ch.push_back(cout);
        for (int j = 0; j < d.n_kernels; ++j) {
            const int rk = d.resblock_kernel_sizes[j], nd = d.n_dilations[j];
            if (rk <= 0 || (rk & 1) == 0 || nd <= 0 || nd > AMP_MAX_DILATIONS) { set_error("amp_gen_create: resblock %d kernel=%d dilations=%d", j, rk, nd); return AMP_ERR_INVALID; }
            const std::string pre = "resblocks." + std::to_string(i * d.n_kernels + j);
            for (int p = 0; p < nd; ++p) {
                if (d.resblock_type == 1) {
                    expect_conv(g.get(), pre + ".convs1." + std::to_string(p), cout, cout, rk, false, true, true);
                    expect_conv(g.get(), pre + ".convs2." + std::to_string(p), cout, cout, rk, false, true, true);
                } else {
                    expect_conv(g.get(), pre + ".convs." + std::to_string(p), cout, cout, rk, false, true, true);
                }
            }
            if (d.arch == AMP_ARCH_BIGVGAN) {
                const int nact = d.resblock_type == 1 ? 2 * nd : nd;
                for (int m = 0; m < nact; ++m) expect_act(g.get(), pre + ".activations." + std::to_string(m), cout);
            }
        }
    }
    if (d.arch == AMP_ARCH_BIGVGAN) expect_act(g.get(), "activation_post", ch);
    expect_conv(g.get(), "conv_post", 1, ch, 7, false, !vits, !vits);
    if (vits && d.gin_channels > 0) expect_conv(g.get(), "cond", c0, d.gin_channels, 1, false, false, true);
    *out = g.release();
    return AMP_OK;
}

int amp_gen_set_weight(amp_gen* g, const char* ref_key, const float* data_host, const int64_t* shape, int ndim) {
    if (!g || !ref_key || !data_host || (!shape && ndim > 0)) { set_error("amp_gen_set_weight: null argument"); return AMP_ERR_INVALID; }
    if (g->finalized) { set_error("amp_gen_set_weight: handle already finalized"); return AMP_ERR_STATE; }
    std::string key(ref_key);
    if (key.rfind("module.", 0) == 0) key = key.substr(7);  // from_multi_gpu checkpoints, vocoder_inference.py:312-327
    auto it = g->expected.find(key);
    if (it == g->expected.end()) { set_error("amp_gen_set_weight: unexpected key '%s'", ref_key); return AMP_ERR_INVALID; }
    HostTensor t;
    t.shape.assign(shape, shape + ndim);
    if (t.shape != it->second) {
        std::string got, want;
        for (auto s : t.shape) got += std::to_string(s) + ",";
        for (auto s : it->second) want += std::to_string(s) + ",";
        set_error("amp_gen_set_weight: '%s' has shape (%s) expected (%s)", ref_key, got.c_str(), want.c_str());
        return AMP_ERR_INVALID;
    }
    // `data_host` may also be a DEVICE pointer (a parameter that already lives on the GPU): copied back here, once,
    // instead of through a host tensor the caller would have to materialise first
    hipPointerAttribute_t attr{};
    const bool on_device = hipPointerGetAttributes(&attr, data_host) == hipSuccess && attr.type == hipMemoryTypeDevice;
    if (!on_device) (void)hipGetLastError();          // a plain host pointer is not an error
    if (on_device) {
        t.data.resize(t.numel());
        AMP_HIP(hipMemcpy(t.data.data(), data_host, t.numel() * sizeof(float), hipMemcpyDeviceToHost));
    } else {
        t.data.assign(data_host, data_host + t.numel());
    }
    g->w[key] = std::move(t);
    return AMP_OK;
}

}  // extern "C"

// fold weight-norm (or take the folded weight) for `prefix`; returns false when tensors are missing
static bool get_folded(amp_gen* g, const std::string& p, std::vector<float>* wout, const float** bias, bool need_bias) {
    auto itw = g->w.find(p + ".weight");
    if (itw != g->w.end()) {
        *wout = itw->second.data;
    } else {
        auto ig = g->w.find(p + ".weight_g"), iv = g->w.find(p + ".weight_v");
        if (ig == g->w.end() || iv == g->w.end()) { set_error("amp_gen_finalize: missing weight for '%s'", p.c_str()); return false; }
        const HostTensor& V = iv->second;
        const size_t d0 = (size_t)V.shape[0], inner = V.numel() / d0;
        wout->resize(V.numel());
        for (size_t r = 0; r < d0; ++r) {
            // torch.norm_except_dim: fp32 2-norm over all dims but 0, w = v * (g / norm)
            double ss = 0.0;
            for (size_t i = 0; i < inner; ++i) { const double v = V.data[r * inner + i]; ss += v * v; }
            const float nrm = (float)sqrt(ss);
            const float sc = ig->second.data[r] / nrm;
            for (size_t i = 0; i < inner; ++i) (*wout)[r * inner + i] = V.data[r * inner + i] * sc;
        }
    }
    *bias = nullptr;
    auto ib = g->w.find(p + ".bias");
    if (ib != g->w.end()) *bias = ib->second.data.data();
    else if (need_bias) { set_error("amp_gen_finalize: missing '%s.bias'", p.c_str()); return false; }
    return true;
}

static int upload(amp_gen* g, const float* src, size_t n, float** dst) {
    AMP_RC(device_upload(src, n * sizeof(float), (void**)dst));
    g->dev_allocs.push_back(*dst);
    return AMP_OK;
}

static int build_act(amp_gen* g, const std::string& p, int c, ActParams* out) {
    auto ia = g->w.find(p + ".act.alpha");
    if (ia == g->w.end()) { set_error("amp_gen_finalize: missing '%s.act.alpha'", p.c_str()); return AMP_ERR_MISSING_WEIGHT; }
    const std::vector<float>* beta = nullptr;
    if (g->d.activation == AMP_ACT_SNAKEBETA) {
        auto ib = g->w.find(p + ".act.beta");
        if (ib == g->w.end()) { set_error("amp_gen_finalize: missing '%s.act.beta'", p.c_str()); return AMP_ERR_MISSING_WEIGHT; }
        beta = &ib->second.data;
    }
    auto iu = g->w.find(p + ".upsample.filter"), idn = g->w.find(p + ".downsample.lowpass.filter");
    if (iu == g->w.end() || idn == g->w.end()) { set_error("amp_gen_finalize: missing anti-aliasing filter buffers of '%s'", p.c_str()); return AMP_ERR_MISSING_WEIGHT; }
    std::vector<float> a(c), ib(c);
    for (int i = 0; i < c; ++i) {
        float al = ia->second.data[i];
        float be = beta ? (*beta)[i] : al;
        if (g->d.snake_logscale) { al = expf(al); be = expf(be); }  // snake.py:57-58,116-118
        a[i] = al;
        ib[i] = 1.0f / (be + 0.000000001f);                          // snake.py:59,119
    }
    int rc;
    if ((rc = upload(g, a.data(), c, &out->a_dev)) != AMP_OK) return rc;
    if ((rc = upload(g, ib.data(), c, &out->invb_dev)) != AMP_OK) return rc;
    if ((rc = upload(g, iu->second.data.data(), 12, &out->fu_dev)) != AMP_OK) return rc;
    if ((rc = upload(g, idn->second.data.data(), 12, &out->fd_dev)) != AMP_OK) return rc;
    float fu2[12];
    for (int i = 0; i < 12; ++i) fu2[i] = 2.f * iu->second.data[i];
    if ((rc = upload(g, fu2, 12, &out->fu2_dev)) != AMP_OK) return rc;
    return AMP_OK;
}

static int make_conv(amp_gen* g, const std::string& p, bool transposed, int cin, int cout, int k, int stride, int dil,
                     int pad, bool need_bias, std::unique_ptr<amp_conv>* out) {
    std::vector<float> w;
    const float* bias = nullptr;
    if (!get_folded(g, p, &w, &bias, need_bias)) return AMP_ERR_MISSING_WEIGHT;
    auto c = std::make_unique<amp_conv>();
    c->transposed = transposed; c->cin = cin; c->cout = cout; c->k = k; c->stride = stride; c->dilation = dil; c->padding = pad;
    int rc = conv_build(c.get(), w.data(), bias);
    if (rc != AMP_OK) return rc;
    *out = std::move(c);
    return AMP_OK;
}

extern "C" {

int amp_gen_finalize(amp_gen* g) {
    if (!g) { set_error("amp_gen_finalize: null handle"); return AMP_ERR_INVALID; }
    if (g->finalized) return AMP_OK;
    if (amp_device_count() <= 0) { set_error("amp_gen_finalize: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    const amp_gen_desc& d = g->d;
    const bool vits = d.arch == AMP_ARCH_HIFIGAN_VITS;
    const int c0 = d.upsample_initial_channel;
    int rc;
    if ((rc = make_conv(g, "conv_pre", false, d.n_in, c0, 7, 1, 1, 3, true, &g->conv_pre)) != AMP_OK) return rc;
    if (vits && d.gin_channels > 0)
        if ((rc = make_conv(g, "cond", false, d.gin_channels, c0, 1, 1, 1, 0, true, &g->cond)) != AMP_OK) return rc;
    int ch = c0;
    for (int i = 0; i < d.n_stages; ++i) {
        const int u = d.upsample_rates[i], k = d.upsample_kernel_sizes[i];
        const int cin = c0 >> i, cout = c0 >> (i + 1);
        std::unique_ptr<amp_conv> up;
        if ((rc = make_conv(g, ups_key(g, i), true, cin, cout, k, u, 1, (k - u) / 2, true, &up)) != AMP_OK) return rc;
        g->ups.push_back(std::move(up));
        ch = cout;
        for (int j = 0; j < d.n_kernels; ++j) {
            ResBlock rb;
            rb.k = d.resblock_kernel_sizes[j];
            const std::string pre = "resblocks." + std::to_string(i * d.n_kernels + j);
            for (int p = 0; p < d.n_dilations[j]; ++p) {
                const int dl = d.resblock_dilation_sizes[j][p];
                rb.dil.push_back(dl);
                std::unique_ptr<amp_conv> a, b;
                const int pad1 = (rb.k * dl - dl) / 2;  // get_padding, gan_utils.py:12-13
                if (d.resblock_type == 1) {
                    if ((rc = make_conv(g, pre + ".convs1." + std::to_string(p), false, cout, cout, rb.k, 1, dl, pad1, true, &a)) != AMP_OK) return rc;
                    if ((rc = make_conv(g, pre + ".convs2." + std::to_string(p), false, cout, cout, rb.k, 1, 1, (rb.k - 1) / 2, true, &b)) != AMP_OK) return rc;
                    rb.c1.push_back(std::move(a));
                    rb.c2.push_back(std::move(b));
                } else {
                    if ((rc = make_conv(g, pre + ".convs." + std::to_string(p), false, cout, cout, rb.k, 1, dl, pad1, true, &a)) != AMP_OK) return rc;
                    rb.c1.push_back(std::move(a));
                }
            }
            if (d.arch == AMP_ARCH_BIGVGAN) {
                const int nact = d.resblock_type == 1 ? 2 * d.n_dilations[j] : d.n_dilations[j];
                rb.acts.resize(nact);
                for (int m = 0; m < nact; ++m)
                    if ((rc = build_act(g, pre + ".activations." + std::to_string(m), cout, &rb.acts[m])) != AMP_OK) return rc;
            }
            g->rbs.push_back(std::move(rb));
        }
    }
    if (d.arch == AMP_ARCH_BIGVGAN)
        if ((rc = build_act(g, "activation_post", ch, &g->act_post)) != AMP_OK) return rc;
    {
        std::vector<float> w;
        const float* bias = nullptr;
        if (!get_folded(g, "conv_post", &w, &bias, !vits)) return AMP_ERR_MISSING_WEIGHT;
        g->post_cin = ch;
        if ((rc = upload(g, w.data(), w.size(), &g->post_w_dev)) != AMP_OK) return rc;
        if (bias) if ((rc = upload(g, bias, 1, &g->post_b_dev)) != AMP_OK) return rc;
    }
    if (!guard_init(g->guard)) { set_error("amp_gen_finalize: cannot allocate the range-guard word"); return AMP_ERR_HIP; }
    g->w.clear();  // host copies no longer needed
    g->finalized = true;
    return AMP_OK;
}

int amp_gen_hop(const amp_gen* g) { return g ? g->hop : 0; }

static size_t gen_buf_elems(const amp_gen* g, int B, int T) {
    size_t mx = (size_t)B * g->d.upsample_initial_channel * T;
    int t = T;
    for (int i = 0; i < g->d.n_stages; ++i) {
        t *= g->d.upsample_rates[i];
        const size_t e = (size_t)B * g->ch[i] * t;
        if (e > mx) mx = e;
    }
    return (mx + 63) & ~(size_t)63;
}

// scratch tensors of a forward: X, XS, U, R, TMP (+ ACT for BigVGAN).
static int gen_num_bufs(const amp_gen* g) { return g->d.arch == AMP_ARCH_BIGVGAN ? 6 : 5; }

// Concurrent resblocks.  The n_kernels resblocks of a stage read the same U and are independent until the MRF mean; run one after
// the other each of them is a chain of 1-9 dependent launches, and for a single utterance no launch fills the chip (a 3-s utterance:
// 50-300 workgroups per launch on 256 CUs, 52 launches back to back = 1.06 ms that a hipGraph replay does not shorten -- the chain
// is serialised on the GPU, not by the host).  In this mode resblocks 1 .. n - 1 run on streams of their own with their own R / TMP
// (/ ACT) buffers and the first one stays on the caller's stream; only the LAST launch of each resblock -- the one that accumulates
// into XS -- is ordered after the last launch of resblock j - 1 (an event) and keeps its sequential `=` / `+=` / `(y + v) / n` mode,
// so every sum is formed by the same kernel in the same
// order and the bits do not change (tests/test_gpu_resblock.py).  (A post-hoc mean of separately stored results would not do: the
// conv kernels add y into the accumulator BEFORE the products.)  Policy (amp_set_resblock_streams(-1) / AMP_RB_STREAMS unset): only
// while B * T <= kRbStreamsMaxFrames mel frames; at full batches every launch fills the chip and the same idea measured 28.1 vs
// 28.1 ms (round 2, BigVGAN, profiles/r2_i_bigvgan_streams.txt).  Works under stream capture (fork / join by events) once the side
// streams exist: they are created by the first eager forward or by amp_gen_prepare_streams(), never inside a capture.
constexpr long long kRbHorizontalMaxFrames = 1024;   // profiles/r4_streams_horizontal_sweep.txt: 0.81 / 0.90 / 0.91 against 0.84 / 0.94 / 0.95 on streams at 256 / 512 / 1 024 frames, equal at 2 048, behind at 4 096
constexpr long long kRbStreamsMaxFrames = 4096;   // tools/streams_sweep.py, profiles/r4_streams_sweep.txt: 0.87-0.97 of the sequential time up to here, 1.00 beyond
static int gen_side_bufs(const amp_gen* g) { return (g->d.n_kernels - 1) * (g->d.arch == AMP_ARCH_BIGVGAN ? 4 : 3); }   // R, TMP, XS (+ ACT) per extra resblock
static bool gen_streams_wanted(const amp_gen* g, int B, int T) {
    if (g->d.n_kernels < 2) return false;
    const int m = cfg().rb_streams;
    return m == 1 || (m < 0 && (long long)B * T <= kRbStreamsMaxFrames);
}

// Optional depth-first batch grouping: a group of items runs through the WHOLE generator before the
// next one starts, with a working set (the scratch tensors of its largest stage) bounded by
// amp_set_group_mb().  It bounds the workspace (168 MB instead of 2.7 GB at config 2) but
// is OFF by default (0 = whole batch per layer): sized to the 256 MiB Infinity Cache it was measured
// SLOWER on MI355X (36.2 ms ungrouped vs 45.6 / 49.9 / 62.4 ms at 200 / 144 / 104 MB groups,
// profiles/r1_exp_group.txt) -- the small grids under-fill 256 CUs and the cache brings no bandwidth win.
static size_t group_target_bytes() { return cfg().group_bytes; }

static int gen_group_items(const amp_gen* g, int B, int T) {
    const size_t target = group_target_bytes();
    if (target == 0) return B;
    // live tensors of a stage: U, R, TMP, XS (+ ACT) -- X is dead once the stage's ConvTranspose has run
    const size_t per_item = gen_buf_elems(g, 1, T) * sizeof(float) * (size_t)(gen_num_bufs(g) - 1);
    size_t n = target / (per_item ? per_item : 1);
    if (n < 1) n = 1;
    return n < (size_t)B ? (int)n : B;
}

size_t amp_gen_workspace_bytes(const amp_gen* g, int B, int T) {
    if (!g || B <= 0 || T <= 0) return 0;
    const int G = gen_group_items(g, B, T);
    const int nb = gen_num_bufs(g) + ((G == B && gen_streams_wanted(g, B, T)) ? gen_side_bufs(g) : 0);
    return gen_buf_elems(g, G, T) * sizeof(float) * nb + (size_t)G * g->d.upsample_initial_channel * sizeof(float) + 256;
}

int amp_gen_set_profiling(amp_gen* g, int slots) {
    if (!g || slots < 0 || slots > 4096) { set_error("amp_gen_set_profiling: bad argument"); return AMP_ERR_INVALID; }
    for (auto& p : g->prof) {
        if (p.ev_begin) (void)hipEventDestroy(p.ev_begin);
        if (p.ev_end) (void)hipEventDestroy(p.ev_end);
        for (auto e : p.ev_mrf) (void)hipEventDestroy(e);
        for (auto e : p.ev_rb) (void)hipEventDestroy(e);
    }
    g->prof.clear();
    g->prof.resize((size_t)slots);
    g->prof_count = 0;
    for (auto& p : g->prof) {
        AMP_HIP(hipEventCreate(&p.ev_begin));
        AMP_HIP(hipEventCreate(&p.ev_end));
    }
    return AMP_OK;
}

int amp_gen_timing_ms(amp_gen* g, int back, int which, float* ms_out) {
    if (!g || !ms_out) { set_error("amp_gen_timing_ms: null argument"); return AMP_ERR_INVALID; }
    if (g->prof.empty() || back < 0 || (size_t)back >= g->prof.size() || (size_t)back >= g->prof_count) {
        set_error("amp_gen_timing_ms: no profiled forward %d back (slots=%zu, recorded=%zu)", back, g->prof.size(), g->prof_count);
        return AMP_ERR_STATE;
    }
    const amp_gen::ProfSlot& p = g->prof[(g->prof_count - 1 - (size_t)back) % g->prof.size()];
    if (!p.valid) { set_error("amp_gen_timing_ms: slot not recorded"); return AMP_ERR_STATE; }
    AMP_HIP(hipEventSynchronize(p.ev_end));
    if (which == 0) {
        AMP_HIP(hipEventElapsedTime(ms_out, p.ev_begin, p.ev_end));
    } else if (which >= 1 && which < 2 + g->d.n_stages) {
        // sum over the batch groups (and, for which == 1, over the stages)
        float tot = 0.f;
        for (int gi = 0; gi < p.ev_groups; ++gi)
            for (int i = 0; i < g->d.n_stages; ++i) {
                if (which >= 2 && i != which - 2) continue;
                float ms = 0.f;
                const size_t e = 2 * ((size_t)g->d.n_stages * gi + i);
                AMP_HIP(hipEventElapsedTime(&ms, p.ev_mrf[e], p.ev_mrf[e + 1]));
                tot += ms;
            }
        *ms_out = tot;
    } else if (which >= 100 && which < 100 + 16 * g->d.n_stages && (which - 100) % 16 < g->d.n_kernels) {
        // one resblock: 100 + 16 * stage + j, summed over the batch groups
        const int i = (which - 100) / 16, j = (which - 100) % 16, nk = g->d.n_kernels;
        float tot = 0.f;
        for (int gi = 0; gi < p.ev_groups; ++gi) {
            float ms = 0.f;
            const size_t e = (size_t)g->d.n_stages * (nk + 1) * gi + (size_t)i * (nk + 1) + j;
            AMP_HIP(hipEventElapsedTime(&ms, p.ev_rb[e], p.ev_rb[e + 1]));
            tot += ms;
        }
        *ms_out = tot;
    } else {
        set_error("amp_gen_timing_ms: which=%d", which);
        return AMP_ERR_INVALID;
    }
    return AMP_OK;
}

int amp_gen_last_timing_ms(amp_gen* g, int which, float* ms_out) { return amp_gen_timing_ms(g, 0, which, ms_out); }

int amp_gen_kernel_name(amp_gen* g, int back, int which, char* buf, size_t n) {
    if (!g || !buf || n == 0) { set_error("amp_gen_kernel_name: null argument"); return AMP_ERR_INVALID; }
    if (g->prof.empty() || back < 0 || (size_t)back >= g->prof.size() || (size_t)back >= g->prof_count) {
        set_error("amp_gen_kernel_name: no profiled forward %d back (slots=%zu, recorded=%zu)", back, g->prof.size(), g->prof_count);
        return AMP_ERR_STATE;
    }
    const amp_gen::ProfSlot& p = g->prof[(g->prof_count - 1 - (size_t)back) % g->prof.size()];
    const int i = (which - 100) / 16, j = (which - 100) % 16;
    if (which < 100 || i >= g->d.n_stages || j >= g->d.n_kernels || (size_t)(i * g->d.n_kernels + j) >= p.rb_kernels.size()) {
        set_error("amp_gen_kernel_name: which=%d", which);
        return AMP_ERR_INVALID;
    }
    snprintf(buf, n, "%s", p.rb_kernels[(size_t)i * g->d.n_kernels + j].c_str());
    return AMP_OK;
}

constexpr float kLreluSlope = 0.1f;  // LRELU_SLOPE hifigan.py:14

// One stage of gen_forward_group after its ConvTranspose: what every step of it reads.
struct Stage {
    amp_gen* g;
    int i;                    // stage index
    int B, t, C, lm;          // items, columns, channels, samples per mel frame (ragged batches: valid length = lens[b] * lm)
    const int* lens;
    hipStream_t st;
    bool conc;                // resblocks 1 .. n_kernels - 1 on g->side streams, with buffers of their own (gen_forward_group)
    const float* U;           // upsampled stage tensor (input of every resblock)
    float* XS;                // MRF accumulator: the stage's output
    float *R, *TMP, *ACT;     // running x inside a resblock, xt between the two convs of a pair, activation output (BigVGAN only)
    float* SIDE;              // concurrent mode: R, TMP, XS (+ ACT) of resblocks 1 .. n_kernels - 1, side_per buffers of be floats each
    int side_per;
    size_t be;
    const ResBlock& rb(int j) const { return g->rbs[(size_t)i * g->d.n_kernels + j]; }
};

// The pairs of a type-1 block as the pointer arrays rb_* / ampb_* take; n = 0 when the block has more pairs than either kernel covers
constexpr int kMaxFusedPairs = AMP_AMPB_MAX_STEPS / 2 > AMP_RB_MAX_PAIRS ? AMP_AMPB_MAX_STEPS / 2 : AMP_RB_MAX_PAIRS;
struct RbPtrs {
    const amp_conv *c1[kMaxFusedPairs], *c2[kMaxFusedPairs];
    int n = 0;
    explicit RbPtrs(const ResBlock& rb) {
        if (rb.c1.size() > (size_t)kMaxFusedPairs || rb.c2.size() != rb.c1.size()) return;
        n = (int)rb.c1.size();
        for (int p = 0; p < n; ++p) { c1[p] = rb.c1[p].get(); c2[p] = rb.c2[p].get(); }
    }
};

// MRF mode of resblock j's accumulating launch in the chain of nk resblocks: XS = v, XS += v, ..., XS = (XS + v) / nk
static int accumulate_mode(int j, int nk) { return j == 0 ? 0 : (j == nk - 1 ? 2 : 1); }

// Resblock j's buffers: its own ones behind the regular buffers when `own` (concurrent mode) and j > 0, else the regular ones
struct RbBufs { float *R, *TMP, *XS, *ACT; };
static RbBufs rb_bufs(const Stage& s, int j, bool own) {
    if (!own || j == 0) return {s.R, s.TMP, s.XS, s.ACT};
    float* SB = s.SIDE + (size_t)(j - 1) * s.side_per * s.be;
    return {SB, SB + s.be, SB + 2 * s.be, s.ACT ? SB + 3 * s.be : nullptr};
}

// XS = ((XS + XS_1) + XS_2 ...) / nk: the MRF mean of resblocks that stored their results separately (in their own XS).  evs: the
// concurrent mode's events, `st` waits for every side resblock's evs[1 + j] first; null: nothing to wait for.
static int launch_stage_mrf_sum(const Stage& s, const hipEvent_t* evs) {
    const int nk = s.g->d.n_kernels;
    MrfSumArgs ma{};
    ma.y = s.XS; ma.n = nk - 1; ma.div = (float)nk; ma.count = (size_t)s.B * s.C * s.t;
    for (int j = 1; j < nk; ++j) {
        if (evs) AMP_HIP(hipStreamWaitEvent(s.st, evs[1 + j], 0));
        ma.p[j - 1] = rb_bufs(s, j, true).XS;
    }
    AMP_HIP(launch_mrf_sum(ma, s.st));
    return AMP_OK;
}

// The horizontal stage forms (try_stage_pair3, try_stage_small3) take a stage of three ResBlock1 whose kernels are 11, 7 and 3 in any order:
// slot_of[0 / 1 / 2] = the resblock with k = 11 / 7 / 3.  false when the stage is not of that shape.
static bool horizontal_slots(const Stage& s, int slot_of[3]) {
    slot_of[0] = slot_of[1] = slot_of[2] = -1;
    for (int j = 0; j < 3; ++j) {
        const int k = s.rb(j).c1[0]->k;
        const int sl = k == 11 ? 0 : k == 7 ? 1 : k == 3 ? 2 : -1;
        if (sl < 0 || slot_of[sl] >= 0) return false;
        slot_of[sl] = j;
    }
    return true;
}

// Horizontal form (pair3_f16x3.hip): where the stage's three resblocks run as per-tile fused pairs, pair p of all three shares ONE launch --
// nd launches + the MRF mean instead of 3 nd launches on three streams with their fork / join events.  Every launch is planned first:
// *ran = false, nothing launched, when one of the pairs is not a per-tile fused pair.
static int try_stage_pair3(const Stage& s, const int slot_of[3], bool* ran) {
    *ran = false;
    const int nk = s.g->d.n_kernels;
    const size_t nd = s.rb(0).dil.size();
    std::vector<Pair3Args> plan(nd);
    for (int sl = 0; sl < 3; ++sl) {
        const int j = slot_of[sl];
        const ResBlock& rb = s.rb(j);
        if (rb.dil.size() != nd) return AMP_OK;
        const RbBufs b = rb_bufs(s, j, true);
        const float* cur = s.U;
        for (size_t p = 0; p < nd; ++p) {
            float* dst = p + 1 == nd ? b.XS : (cur == b.R ? b.TMP : b.R);
            if (!pair_tile_args(rb.c1[p].get(), rb.c2[p].get(), cur, s.B, s.t, kLreluSlope, dst, 0, (float)nk, s.lens, s.lm, &plan[p].a[sl]))
                return AMP_OK;
            plan[p].n[sl] = s.B * plan[p].a[sl].tiles_per_item;
            cur = dst;
        }
    }
    for (const Pair3Args& p : plan) AMP_HIP(launch_pair3(p, s.st));
    AMP_RC(launch_stage_mrf_sum(s, nullptr));
    *ran = true;
    return AMP_OK;
}

// The same for a stage of UNFUSED whole-K convs (the C = 256 stage of a single utterance): c1 of a dilation, then c2, of all three
// resblocks in one launch each (conv_small3_f16x3.hip); only the three convs that accumulate into XS stay separate launches, in resblock
// order with their `=` / `+=` / `(y + v) / n` modes (they add y BEFORE the products: no post-hoc mean).  Every launch is planned first
// (conv_run with plan_small launches nothing): *ran = false, nothing launched, when one of them is not a whole-K conv.
static int try_stage_small3(const Stage& s, const int slot_of[3], bool* ran) {
    *ran = false;
    const int nk = s.g->d.n_kernels;
    for (int j = 0; j < 3; ++j)
        if (pair_supported(s.rb(j).c1[0].get(), s.rb(j).c2[0].get())) return AMP_OK;
    const size_t nd = s.rb(0).dil.size();
    struct Step { ConvSmall3Args p; int ni[3]; };
    std::vector<Step> steps;                        // c1(d_0), c2, c1(d_1), c2, ..., c1(d_last)
    const float* cur[3] = {s.U, s.U, s.U};
    RbBufs b[3];
    for (int j = 0; j < 3; ++j) b[j] = rb_bufs(s, j, true);
    auto plan3 = [&](bool second, size_t p) -> bool {    // one merged launch: c1[p] (second = false) or c2[p] of the three resblocks
        Step sp{};
        for (int sl = 0; sl < 3; ++sl) {
            const int j = slot_of[sl];
            const amp_conv* c = second ? s.rb(j).c2[p].get() : s.rb(j).c1[p].get();
            const int rc = second ? conv_run(c, b[j].TMP, s.B, s.t, 1.f, cur[j], 1.f, b[j].R, 0, 1.f, s.st, 0, s.lens, s.lm, &sp.p.a[sl], &sp.ni[sl])
                                  : conv_run(c, cur[j], s.B, s.t, kLreluSlope, nullptr, kLreluSlope, b[j].TMP, 0, 1.f, s.st, 0, s.lens, s.lm, &sp.p.a[sl], &sp.ni[sl]);
            if (rc != AMP_OK) return false;
            sp.p.nx[sl] = s.B * sp.p.a[sl].tiles_per_item;
            sp.p.ny[sl] = (sp.p.a[sl].M + 127) / 128;
        }
        if (sp.ni[1] != 1 || sp.ni[2] != 1) return false;
        steps.push_back(sp);
        return true;
    };
    bool ok = true;
    for (size_t p = 0; ok && p < nd; ++p) {
        for (int j = 0; j < 3 && ok; ++j) ok = s.rb(j).dil.size() == nd;
        ok = ok && plan3(false, p);
        if (ok && p + 1 < nd) {
            ok = plan3(true, p);
            for (int j = 0; j < 3; ++j) cur[j] = b[j].R;
        }
    }
    // the accumulating convs must be whole-K launches too
    for (int j = 0; ok && j < 3; ++j) {
        ConvArgs unused_a; int unused_ni;
        ok = conv_run(s.rb(j).c2[nd - 1].get(), b[j].TMP, s.B, s.t, 1.f, cur[j], 1.f, s.XS, accumulate_mode(j, nk), (float)nk, s.st, 0, s.lens,
                      s.lm, &unused_a, &unused_ni) == AMP_OK;
    }
    if (!ok) return AMP_OK;
    for (const Step& sp : steps) AMP_HIP(launch_conv_small3(sp.p, sp.ni, s.st));
    for (int j = 0; j < 3; ++j)
        AMP_RC(conv_run(s.rb(j).c2[nd - 1].get(), b[j].TMP, s.B, s.t, 1.f, cur[j], 1.f, s.XS, accumulate_mode(j, nk), (float)nk, s.st, 0, s.lens, s.lm));
    *ran = true;
    return AMP_OK;
}

// Called right before a resblock's launch that writes XS: in a concurrent chain that launch reads what resblock j - 1 accumulated there and
// first waits for it (`wait` = evs[j]; null otherwise).
static int wait_before_last(hipEvent_t wait, hipStream_t sj) {
    if (wait) AMP_HIP(hipStreamWaitEvent(sj, wait, 0));
    return AMP_OK;
}

// ResBlock1 (HiFi-GAN), U -> b.XS on sj with the MRF mode mode_last: the whole resblock in one to three launches, else pair by pair (a fused
// pair, or its two convs)
static int run_resblock1(const Stage& s, const ResBlock& rb, const RbBufs& b, int mode_last, hipEvent_t wait, hipStream_t sj) {
    const int B = s.B, t = s.t;
    const float nk = (float)s.g->d.n_kernels;
    const int nd = (int)rb.dil.size();
    RbPtrs q(rb);
    if (q.n && rb_supported(q.c1, q.c2, nd, B, t)) {
        // the whole resblock in one launch: U -> XS (x and the residual never leave the CU in between) -- or in two
        // or three: the launches of rb_plan(), x ping-ponging R <-> TMP in between as on the pair path below
        const RbPlan pl = rb_plan(q.c1, nd, B, t, s.lens != nullptr);
        const float* cur = s.U;
        int first = 0;
        for (int l = 0; l + 1 < pl.n; first += pl.count[l++]) {
            float* dst = cur == b.R ? b.TMP : b.R;
            AMP_RC(rb_run(q.c1, q.c2, nd, cur, B, t, kLreluSlope, dst, 0, 1.f, sj, s.lens, s.lm, first, pl.count[l]));
            cur = dst;
        }
        AMP_RC(wait_before_last(wait, sj));
        return rb_run(q.c1, q.c2, nd, cur, B, t, kLreluSlope, b.XS, mode_last, nk, sj, s.lens, s.lm, first, -1);
    }
    const float* cur = s.U;
    for (int p = 0; p < nd; ++p) {
        const bool last = p == nd - 1;
        const amp_conv *c1 = rb.c1[p].get(), *c2 = rb.c2[p].get();
        if (pair_supported(c1, c2)) {
            // the whole pair in one kernel; the output ping-pongs R <-> TMP (never in place: other tiles still read the input's halo)
            float* dst = last ? b.XS : (cur == b.R ? b.TMP : b.R);
            if (last) AMP_RC(wait_before_last(wait, sj));
            AMP_RC(pair_run(c1, c2, cur, B, t, kLreluSlope, dst, last ? mode_last : 0, nk, sj, s.lens, s.lm));
            cur = dst;
            continue;
        }
        // xt = lrelu(c1(lrelu(x))) ; x = c2(xt) + x        hifigan.py:93-100
        if (cur == b.TMP) {  // previous pair was fused into TMP: keep the unfused ping-pong legal
            AMP_HIP(hipMemcpyAsync(b.R, b.TMP, (size_t)B * s.C * t * sizeof(float), hipMemcpyDeviceToDevice, sj));
            cur = b.R;
        }
        AMP_RC(conv_run(c1, cur, B, t, kLreluSlope, nullptr, kLreluSlope, b.TMP, 0, 1.f, sj, 0, s.lens, s.lm));
        if (!last) { AMP_RC(conv_run(c2, b.TMP, B, t, 1.f, cur, 1.f, b.R, 0, 1.f, sj, 0, s.lens, s.lm)); cur = b.R; }
        else { AMP_RC(wait_before_last(wait, sj)); AMP_RC(conv_run(c2, b.TMP, B, t, 1.f, cur, 1.f, b.XS, mode_last, nk, sj, 0, s.lens, s.lm)); }
    }
    return AMP_OK;
}

// AMPBlock1 (BigVGAN), U -> b.XS: the whole block in one launch, else per pair act1d, c1, act1d, c2 + residual
static int run_ampblock1(const Stage& s, const ResBlock& rb, const RbBufs& b, int mode_last, hipEvent_t wait, hipStream_t sj) {
    const int B = s.B, t = s.t, nd = (int)rb.dil.size();
    const float nk = (float)s.g->d.n_kernels;
    RbPtrs q(rb);
    if (q.n && ampb_supported(q.c1, q.c2, nd, rb.acts.data(), rb.acts.size(), B, t)) {
        // the whole AMPBlock in one launch: U -> XS (bigvgan.py:137-146)
        AMP_RC(wait_before_last(wait, sj));
        return ampb_run(q.c1, q.c2, nd, rb.acts.data(), s.U, B, t, b.XS, mode_last, nk, sj, s.lens, s.lm);
    }
    const float* cur = s.U;   // U, then R: never TMP (no fused pairs here)
    for (int p = 0; p < nd; ++p) {
        // xt = c2(a2(c1(a1(x)))) ; x = xt + x              bigvgan.py:137-146
        const ActParams& a1 = rb.acts[2 * p];
        const ActParams& a2 = rb.acts[2 * p + 1];
        AMP_HIP(launch_act1d(cur, b.ACT, B, s.C, t, a1.a_dev, a1.invb_dev, a1.fu_dev, a1.fd_dev, s.lens, s.lm, sj, next_rev(s.lens)));
        AMP_RC(conv_run(rb.c1[p].get(), b.ACT, B, t, 1.f, nullptr, 1.f, b.TMP, 0, 1.f, sj, 0, s.lens, s.lm));
        AMP_HIP(launch_act1d(b.TMP, b.ACT, B, s.C, t, a2.a_dev, a2.invb_dev, a2.fu_dev, a2.fd_dev, s.lens, s.lm, sj, next_rev(s.lens)));
        if (p < nd - 1) { AMP_RC(conv_run(rb.c2[p].get(), b.ACT, B, t, 1.f, cur, 1.f, b.R, 0, 1.f, sj, 0, s.lens, s.lm)); cur = b.R; }
        else { AMP_RC(wait_before_last(wait, sj)); AMP_RC(conv_run(rb.c2[p].get(), b.ACT, B, t, 1.f, cur, 1.f, b.XS, mode_last, nk, sj, 0, s.lens, s.lm)); }
    }
    return AMP_OK;
}

// ResBlock2 / AMPBlock2, U -> b.XS: x = c(act(x)) + x per dilation          hifigan.py:140-145, bigvgan.py:218-224
static int run_resblock2(const Stage& s, const ResBlock& rb, const RbBufs& b, int mode_last, hipEvent_t wait, hipStream_t sj) {
    const bool big = s.g->d.arch == AMP_ARCH_BIGVGAN;
    const int B = s.B, t = s.t, nd = (int)rb.dil.size();
    const float* cur = s.U;
    for (int p = 0; p < nd; ++p) {
        const float* in = cur;
        float sl = kLreluSlope;
        if (big) {
            const ActParams& a1 = rb.acts[p];
            AMP_HIP(launch_act1d(cur, b.ACT, B, s.C, t, a1.a_dev, a1.invb_dev, a1.fu_dev, a1.fd_dev, s.lens, s.lm, sj, next_rev(s.lens)));
            in = b.ACT;
            sl = 1.f;
        }
        if (p < nd - 1) {
            // the conv reads a halo of `in`; never write the tensor it is reading
            float* dst = (in == cur && cur == b.R) ? b.TMP : b.R;
            AMP_RC(conv_run(rb.c1[p].get(), in, B, t, sl, cur, 1.f, dst, 0, 1.f, sj, 0, s.lens, s.lm));
            cur = dst;
        } else {
            AMP_RC(wait_before_last(wait, sj));
            AMP_RC(conv_run(rb.c1[p].get(), in, B, t, sl, cur, 1.f, b.XS, mode_last, (float)s.g->d.n_kernels, sj, 0, s.lens, s.lm));
        }
    }
    return AMP_OK;
}

// A stage whose resblocks ALL end in a fused pair / whole-resblock kernel (HiFi-GAN, C <= 128) needs no chain in the concurrent mode: those
// kernels add the accumulated y to their finished, rounded result, so each resblock stores its own result (mode 0) and one small launch
// forms ((XS0 + XS1) + XS2) / n afterwards -- the same bits with one join instead of two chained cross-queue waits (~12 us each).
static bool stage_sums_separately(const Stage& s) {
    const amp_gen_desc& d = s.g->d;
    if (!s.conc || d.resblock_type != 1 || d.arch == AMP_ARCH_BIGVGAN || d.n_kernels - 1 > AMP_MRF_MAX_PARTS) return false;
    for (int j = 0; j < d.n_kernels; ++j) {
        const ResBlock& rb = s.rb(j);
        const size_t last = rb.dil.size() - 1;
        RbPtrs q(rb);
        if (!(q.n && rb_supported(q.c1, q.c2, q.n, s.B, s.t)) && !pair_supported(rb.c1[last].get(), rb.c2[last].get())) return false;
    }
    return true;
}

// profiled forward: every launch of one resblock logs its kernel's name (note_kernel, amp_internal.h)
struct KernelLogScope {
    explicit KernelLogScope(std::string* p) { tl_kernel_log = p; if (p) p->clear(); }
    ~KernelLogScope() { tl_kernel_log = nullptr; }
};

// The stage's resblocks U -> XS, one after the other on `st` -- or, concurrent mode, resblock 0 on `st` and resblocks 1 .. nk - 1 on the side
// streams: evs[0] fork, evs[1 + j] = resblock j's accumulating launch done; the launch that accumulates resblock j >= 1 waits for evs[j] and
// `st` joins on evs[nk] (a chain), or `st` waits for them all and forms the MRF mean itself (stage_sums_separately).  (Measured the other way
// round too -- the widest resblock on `st`, the others on the side streams: the same 0.81-0.83 ms as a graph replay, but 1.08 instead of
// 0.90-0.95 ms eager, where the host issues the critical stream's launches last.)  ev_rb / rb_names: the profiled forward's per-resblock
// events and kernel names.
static int run_stage_resblocks(const Stage& s, hipEvent_t* ev_rb, std::vector<std::string>* rb_names) {
    amp_gen* g = s.g;
    const int nk = g->d.n_kernels;
    const size_t ev0 = (size_t)s.i * (nk + 1);
    hipEvent_t* evs = s.conc ? &g->ev_side[ev0] : nullptr;
    const bool sum_stage = stage_sums_separately(s);
    if (s.conc) {
        AMP_HIP(hipEventRecord(evs[0], s.st));
        for (int j = 1; j < nk; ++j) AMP_HIP(hipStreamWaitEvent(g->side[j - 1], evs[0], 0));
    }
    for (int j = 0; j < nk; ++j) {
        const hipStream_t sj = (s.conc && j > 0) ? g->side[j - 1] : s.st;
        RbBufs b = rb_bufs(s, j, s.conc);
        if (!sum_stage) b.XS = s.XS;                                             // a chain: every resblock accumulates into XS
        const hipEvent_t wait = (s.conc && !sum_stage && j > 0) ? evs[j] : nullptr;
        const int mode_last = sum_stage ? 0 : accumulate_mode(j, nk);
        if (ev_rb) AMP_HIP(hipEventRecord(ev_rb[ev0 + j], sj));
        {
            KernelLogScope log_scope(rb_names ? &(*rb_names)[(size_t)s.i * nk + j] : nullptr);
            const ResBlock& rb = s.rb(j);
            if (g->d.resblock_type != 1) AMP_RC(run_resblock2(s, rb, b, mode_last, wait, sj));
            else if (g->d.arch == AMP_ARCH_BIGVGAN) AMP_RC(run_ampblock1(s, rb, b, mode_last, wait, sj));
            else AMP_RC(run_resblock1(s, rb, b, mode_last, wait, sj));
        }
        if (s.conc) AMP_HIP(hipEventRecord(evs[1 + j], sj));
    }
    if (s.conc && !sum_stage) AMP_HIP(hipStreamWaitEvent(s.st, evs[nk], 0));   // join: the last resblock's accumulating launch follows all the others
    if (sum_stage) AMP_RC(launch_stage_mrf_sum(s, evs));
    if (ev_rb) AMP_HIP(hipEventRecord(ev_rb[ev0 + nk], s.st));
    return AMP_OK;
}

// One group of `B` items through the whole generator (buffers sized for `be` elements each).
static int gen_forward_group(amp_gen* g, const float* mel_dev, const float* cond_dev, const int* lens, int B, int T,
                             float* wav_dev, float* base, size_t be, hipStream_t st,
                             hipEvent_t* ev_mrf /* 2 per stage, or null */, hipEvent_t* ev_rb /* (n_kernels+1) per stage */,
                             std::vector<std::string>* rb_names = nullptr /* per (stage, resblock), or null */,
                             bool conc = false /* resblocks of a stage on g->side streams (the buffers behind the regular ones exist) */) {
    const amp_gen_desc& d = g->d;
    const bool big = d.arch == AMP_ARCH_BIGVGAN;
    float* X = base;            // stage input / MRF accumulator (ping-pong with XS)
    float* XS = base + be;
    float* U = base + 2 * be;   // upsampled stage tensor (input of every resblock)
    Stage s{};
    s.g = g; s.B = B; s.lens = lens; s.st = st; s.conc = conc; s.U = U;
    s.R = base + 3 * be;
    s.TMP = base + 4 * be;
    s.ACT = big ? base + 5 * be : nullptr;
    s.SIDE = base + (size_t)gen_num_bufs(g) * be;
    s.side_per = big ? 4 : 3;
    s.be = be;
    float* CB = base + (size_t)(gen_num_bufs(g) + (conc ? gen_side_bufs(g) : 0)) * be;  // cond(g): [B, C0]

    AMP_RC(conv_run(g->conv_pre.get(), mel_dev, B, T, 1.f, nullptr, 1.f, X, 0, 1.f, st, 0, lens, 1));
    if (cond_dev) {  // x = x + self.cond(g), hifigan.py:426-427 (g has length 1 -> per-channel bias)
        AMP_RC(conv_run(g->cond.get(), cond_dev, B, 1, 1.f, nullptr, 1.f, CB, 0, 1.f, st));
        AMP_HIP(launch_add_channel_bias(X, CB, B, d.upsample_initial_channel, T, st));
    }
    // the horizontal stage forms: concurrent mode, at most kRbHorizontalMaxFrames mel frames, three ResBlock1 per stage
    const bool horizontal = conc && (long long)B * T <= kRbHorizontalMaxFrames && d.resblock_type == 1 && !big && d.n_kernels == 3;
    int t = T;
    int lm = 1;  // samples per mel frame at the current stage
    for (int i = 0; i < d.n_stages; ++i) {
        // HiFiGAN: leaky_relu(0.1) before the transposed conv (hifigan.py:206); BigVGAN: none (bigvgan.py:316-318)
        AMP_RC(conv_run(g->ups[i].get(), X, B, t, big ? 1.f : kLreluSlope, nullptr, 1.f, U, 0, 1.f, st, 0, lens, lm));
        t *= d.upsample_rates[i];
        lm *= d.upsample_rates[i];
        if (ev_mrf) AMP_HIP(hipEventRecord(ev_mrf[2 * i], st));
        s.i = i; s.t = t; s.C = g->ch[i]; s.lm = lm; s.XS = XS;
        bool ran = false;
        int slot_of[3];
        if (horizontal && horizontal_slots(s, slot_of)) {
            AMP_RC(try_stage_pair3(s, slot_of, &ran));
            if (!ran) AMP_RC(try_stage_small3(s, slot_of, &ran));
        }
        if (!ran) AMP_RC(run_stage_resblocks(s, ev_rb, rb_names));
        if (ev_mrf) AMP_HIP(hipEventRecord(ev_mrf[2 * i + 1], st));
        float* tmp = X; X = XS; XS = tmp;  // x = xs / num_kernels
    }
    if (big) {
        AMP_HIP(launch_act1d(X, s.ACT, B, g->post_cin, t, g->act_post.a_dev, g->act_post.invb_dev, g->act_post.fu_dev, g->act_post.fd_dev, lens, lm, st, next_rev(lens)));
        AMP_HIP(launch_conv_post(s.ACT, g->post_w_dev, g->post_b_dev, wav_dev, B, g->post_cin, t, 7, 1.f, 1, lens, lm, st));
    } else {
        // F.leaky_relu(x) with the DEFAULT slope 0.01 (hifigan.py:215,439), conv_post, tanh
        AMP_HIP(launch_conv_post(X, g->post_w_dev, g->post_b_dev, wav_dev, B, g->post_cin, t, 7, 0.01f, 1, lens, lm, st));
    }
    return AMP_OK;
}

// The side streams and fork / join events of the concurrent-resblock mode; false when they do not exist and cannot be created now
// (`st` is being captured: hipStreamCreate is not a capturable call -- the forward then runs the sequential chain, same bits).
static bool gen_ensure_side(amp_gen* g, hipStream_t st) {
    const size_t ns = (size_t)g->d.n_kernels - 1, ne = (size_t)g->d.n_stages * (g->d.n_kernels + 1);
    if (g->side.size() == ns && g->ev_side.size() == ne) return true;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return false; }
    while (g->side.size() < ns) {
        hipStream_t s_ = nullptr;
        if (hipStreamCreateWithFlags(&s_, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return false; }
        g->side.push_back(s_);
    }
    while (g->ev_side.size() < ne) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
        g->ev_side.push_back(e);
    }
    return true;
}

int amp_gen_prepare_streams(amp_gen* g) {
    if (!g || !g->finalized) { set_error("amp_gen_prepare_streams: null or unfinalized handle"); return AMP_ERR_STATE; }
    if (g->d.n_kernels < 2) return AMP_OK;
    if (!gen_ensure_side(g, nullptr)) { set_error("amp_gen_prepare_streams: could not create the side streams"); return AMP_ERR_HIP; }
    return AMP_OK;
}

int amp_gen_forward(amp_gen* g, const float* mel_dev, const float* cond_dev, int B, int T, float* wav_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream_) {
    return amp_gen_forward_ragged(g, mel_dev, cond_dev, nullptr, B, T, wav_dev, workspace_dev, workspace_bytes, stream_);
}

int amp_gen_forward_ragged(amp_gen* g, const float* mel_dev, const float* cond_dev, const int32_t* lens_dev, int B, int T,
                           float* wav_dev, void* workspace_dev, size_t workspace_bytes, void* stream_) {
    if (!g || !mel_dev || !wav_dev || !workspace_dev) { set_error("amp_gen_forward: null argument"); return AMP_ERR_INVALID; }
    if (!g->finalized) { set_error("amp_gen_forward: call amp_gen_finalize first"); return AMP_ERR_STATE; }
    if (B <= 0 || T <= 0) { set_error("amp_gen_forward: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    if (workspace_bytes < amp_gen_workspace_bytes(g, B, T)) { set_error("amp_gen_forward: workspace too small (%zu < %zu)", workspace_bytes, amp_gen_workspace_bytes(g, B, T)); return AMP_ERR_INVALID; }
    if (cond_dev && !g->cond) { set_error("amp_gen_forward: cond given but gin_channels == 0"); return AMP_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream_;
    std::lock_guard<std::mutex> launch_lock(g->launch_mu);
    AMP_RC(range_poll(&g->guard, st)); // a previous forward of this handle left the f16 operand range: say so now
    RangeFlagScope flag_scope(g->guard.dev);
    const amp_gen_desc& d = g->d;
    const int G = gen_group_items(g, B, T);
    const int ngroups = (B + G - 1) / G;
    const size_t be = gen_buf_elems(g, G, T);
    const size_t L = (size_t)T * g->hop;
    amp_gen::ProfSlot* ps = g->prof.empty() ? nullptr : &g->prof[g->prof_count % g->prof.size()];
    // concurrent resblocks: small launches, the whole batch in one group, not while the per-resblock events are being recorded (they
    // time one resblock after the other on `st`)
    const bool conc = ngroups == 1 && !ps && gen_streams_wanted(g, B, T) && gen_ensure_side(g, st);
    if (ps) {
        const size_t need = 2 * (size_t)d.n_stages * ngroups;
        while (ps->ev_mrf.size() < need) {
            hipEvent_t e;
            AMP_HIP(hipEventCreate(&e));
            ps->ev_mrf.push_back(e);
        }
        const size_t need_rb = (size_t)d.n_stages * (d.n_kernels + 1) * ngroups;
        while (ps->ev_rb.size() < need_rb) {
            hipEvent_t e;
            AMP_HIP(hipEventCreate(&e));
            ps->ev_rb.push_back(e);
        }
        ps->ev_groups = ngroups;
        ps->rb_kernels.assign((size_t)d.n_stages * d.n_kernels, std::string());
        AMP_HIP(hipEventRecord(ps->ev_begin, st));
    }
    for (int gi = 0; gi < ngroups; ++gi) {
        const int b0 = gi * G;
        const int Bg = (B - b0) < G ? (B - b0) : G;
        AMP_RC(gen_forward_group(g, mel_dev + (size_t)b0 * d.n_in * T,
                                 cond_dev ? cond_dev + (size_t)b0 * d.gin_channels : nullptr,
                                 lens_dev ? lens_dev + b0 : nullptr, Bg, T,
                                 wav_dev + (size_t)b0 * L, (float*)workspace_dev, be, st,
                                 ps ? ps->ev_mrf.data() + 2 * (size_t)d.n_stages * gi : nullptr,
                                 ps ? ps->ev_rb.data() + (size_t)d.n_stages * (d.n_kernels + 1) * gi : nullptr,
                                 (ps && gi == 0) ? &ps->rb_kernels : nullptr, conc));
    }
    if (ps) { AMP_HIP(hipEventRecord(ps->ev_end, st)); ps->valid = true; ++g->prof_count; }
    AMP_RC(range_publish(&g->guard, st));
    return AMP_OK;
}

int amp_gen_range_check(amp_gen* g, void* stream_) {
    if (!g) { set_error("amp_gen_range_check: null handle"); return AMP_ERR_INVALID; }
    return range_check_sync(&g->guard, (hipStream_t)stream_, "amp_gen_range_check");
}

void amp_gen_destroy(amp_gen* g) { delete g; }

}  // extern "C"
