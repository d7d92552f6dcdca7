// capi_hooks.cpp — the test, profiling and microbenchmark hooks of include/llmi.h: whole
// steps under a profiler or tracer, the test options and taps, and the kernel-level
// entry points that launch one kernel without a model.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/llmi.h"
#include "capi_internal.h"

using namespace llmi;

namespace {
// (the device allocations of one hook call: a local DevPool's get(), dev_mem.h)
// launch_pf_quant's outputs for tpad token rows (llmi_pf_gemm's sizes), zeroed: the padded
// rows are read
struct QuantScratch {
    void* aq = nullptr;
    int16_t* abs = nullptr;
    float* ad = nullptr;
    void* abf = nullptr;
    QuantScratch(DevPool& P, size_t tpad, size_t cols) {
        aq = P.get<void>(tpad * cols * 2);
        abf = P.get<void>(tpad * (cols / 256) * 64);
        abs = P.get<int16_t>(tpad * (cols / 16) * 2);
        ad = P.get<float>(tpad * (cols / 32) * 4);
    }
};
// the stream, event pair and graph exec of one hook call, destroyed on every way out
struct HipObjs {
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipGraphExec_t ex = nullptr;
    hipError_t events() {
        const hipError_t e = e0 ? hipSuccess : hipEventCreate(&e0);
        return e != hipSuccess || e1 ? e : hipEventCreate(&e1);
    }
    ~HipObjs() {
        if (ex) (void)hipGraphExecDestroy(ex);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (s) (void)hipStreamDestroy(s);
    }
};
// microseconds of what `launch` puts on the null stream, between two events
template <class F>
hipError_t time_launch(HipObjs& h, F launch, double& us) {
    hipError_t e = h.events();
    if (e != hipSuccess) return e;
    (void)hipEventRecord(h.e0, nullptr);
    e = launch();
    (void)hipEventRecord(h.e1, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(h.e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, h.e0, h.e1);
    us = (double)ms * 1e3;
    return e;
}
// microseconds per launch of h.ex (per_replay launches each) on h.s: one warm replay (code,
// TLB), then n timed ones; < 0 on error
double replay_us(HipObjs& h, int n, int per_replay) {
    if (h.events() != hipSuccess) return -1.0;
    (void)hipGraphLaunch(h.ex, h.s);
    (void)hipEventRecord(h.e0, h.s);
    for (int r = 0; r < n; ++r) (void)hipGraphLaunch(h.ex, h.s);
    (void)hipEventRecord(h.e1, h.s);
    float ms = 0.f;
    if (hipEventSynchronize(h.e1) != hipSuccess || hipEventElapsedTime(&ms, h.e0, h.e1) != hipSuccess) return -1.0;
    return (double)ms * 1e3 / ((double)n * per_replay);
}
bool head_shape_ok(int n_head, int n_head_kv, int head_dim) {
    return n_head > 0 && n_head_kv > 0 && n_head % n_head_kv == 0 && (head_dim == 64 || head_dim == 128);
}
bool weight_type_ok(int t) { return t == T_Q4_K || t == T_Q5_K || t == T_Q6_K || t == T_Q8_0; }
int hook_grid_cap() {  // the matvec grid cap a context of the current device launches with
    int dev = 0;
    (void)hipGetDevice(&dev);
    return mv_grid_cap(dev);
}
// the StepStates of n steps at positions n_kv[t] - 1 (step sequence number seq), on the device
StepState* dev_states(DevPool& P, const int* n_kv, int n, unsigned seq) {
    std::vector<StepState> hs((size_t)n);
    for (int t = 0; t < n; ++t) {
        hs[(size_t)t].pos = n_kv[t] - 1;
        hs[(size_t)t].pos_next = n_kv[t];
        hs[(size_t)t].seq = seq;
    }
    StepState* st = P.get<StepState>((size_t)n * sizeof(StepState), false);
    if (st) P.err = hipMemcpy(st, hs.data(), (size_t)n * sizeof(StepState), hipMemcpyHostToDevice);
    return P.err == hipSuccess ? st : nullptr;
}
}  // namespace

extern "C" {

int32_t llmi_profile_kernels(struct llama_context* ctx, llama_token first, int32_t pos0, int32_t n_steps, double* us,
                             double* bytes, int32_t* launches) {
    API_TRY
    if (!ctx || n_steps <= 0 || !us || !bytes || !launches) { set_err("llmi_profile_kernels: bad arguments"); return -1; }
    Context& c = ctx->c;
    if (first < 0 || first >= c.m->hp.n_vocab || pos0 < 0 || pos0 >= c.n_ctx) {
        set_err("llmi_profile_kernels: token/position out of range");
        return -1;
    }
    (void)hipSetDevice(c.m->device);
    // In situ: n_steps whole decode steps at position pos0 (the decode graph's exact
    // kernels, grids and arguments, in their order), launched one by one with EVERY
    // kernel armed with an event pair that the runtime records when it starts and ends
    // (hipExtLaunchKernelGGL): each kernel's execution time in its real place in the
    // step (caches as its predecessor leaves them), without launch gaps.  One warm step
    // first.  No tokens are consumed: the state is reset to (first, pos0) afterwards.
    const int kv_bound = kv_bucket_bound(pos0 + 1, c.n_ctx);
    std::string err;
    int rc = 0;
    {
        Prof warm;
        if (launch_state_set(c.st, first, pos0, c.stream) != hipSuccess) { set_err("state set failed"); return -3; }
        c.prof = &warm;
        bool ok = step_enqueue(c, kv_bound, err);
        Prof pk;
        pk.timed = true;
        for (int r = 0; ok && r < n_steps; ++r) {
            if (launch_state_set(c.st, first, pos0, c.stream) != hipSuccess) { ok = false; break; }
            c.prof = &pk;
            ok = step_enqueue(c, kv_bound, err);
        }
        c.prof = nullptr;
        if (!ok || hipStreamSynchronize(c.stream) != hipSuccess) {
            set_err("llmi_profile_kernels: " + (err.empty() ? std::string("launch failed") : err));
            rc = -4;
        }
        for (int k = 0; rc == 0 && k < K_NCLASS; ++k) {
            int used = 0;
            const double t = pk.elapsed_us(k, &used);
            const int n = std::max(1, pk.launches[k]);
            us[k] = used ? t / (double)used : 0.0;
            bytes[k] = (pk.bytes[k] + pk.per_kv[k] * (double)(pos0 + 1)) / n;
            launches[k] = pk.launches[k] / n_steps;
        }
    }
    if (launch_state_set(c.st, first, pos0, c.stream) != hipSuccess || hipStreamSynchronize(c.stream) != hipSuccess) {
        if (rc == 0) { set_err("llmi_profile_kernels: state reset failed"); rc = -4; }
    }
    c.n_past = pos0;
    return rc;
    API_CATCH(-5)
}


int32_t llmi_engine_trace(struct llama_context* ctx, llama_token first, int32_t pos0, int32_t layer, uint64_t* out,
                          int64_t n_out) {
    API_TRY
    if (!ctx || !out) { set_err("llmi_engine_trace: bad arguments"); return -1; }
    Context& c = ctx->c;
    if (first < 0 || first >= c.m->hp.n_vocab || pos0 < 0 || pos0 >= c.n_ctx || layer < 0 || layer >= c.m->hp.n_layer) {
        set_err("llmi_engine_trace: token/position/layer out of range");
        return -1;
    }
    (void)hipSetDevice(c.m->device);
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.m->device);
    const size_t n = (size_t)cus * 16 * 32;
    if ((size_t)n_out < n) { set_err("llmi_engine_trace: out holds fewer than CUs x 512 stamps"); return -1; }
    // one eager warm step, then one traced step at (first, pos0); the state is reset after
    const int kv_bound = kv_bucket_bound(pos0 + 1, c.n_ctx);
    std::string err;
    int rc = 0;
    if (!c.le_trace && c.pool.alloc(c.le_trace, n * 8) != hipSuccess) { set_err("llmi_engine_trace: hipMalloc"); return -3; }
    (void)hipMemsetAsync(c.le_trace, 0, n * 8, c.stream);
    bool ok = launch_state_set(c.st, first, pos0, c.stream) == hipSuccess && step_enqueue(c, kv_bound, err);
    c.le_trace_layer = layer;
    ok = ok && launch_state_set(c.st, first, pos0, c.stream) == hipSuccess && step_enqueue(c, kv_bound, err);
    c.le_trace_layer = -1;
    if (!ok || hipMemcpyAsync(out, c.le_trace, n * 8, hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
        hipStreamSynchronize(c.stream) != hipSuccess) {
        set_err("llmi_engine_trace: " + (err.empty() ? std::string("launch failed") : err));
        rc = -4;
    }
    if (launch_state_set(c.st, first, pos0, c.stream) != hipSuccess || hipStreamSynchronize(c.stream) != hipSuccess)
        if (rc == 0) { set_err("llmi_engine_trace: state reset failed"); rc = -4; }
    c.n_past = pos0;
    return rc == 0 ? cus : rc;
    API_CATCH(-5)
}

double llmi_le_stream_bench(const void* src, int64_t bytes, int32_t mode, int32_t iters, int32_t nt) {
    return le_stream_bench(src, (size_t)bytes, mode, iters, nt);
}

// numerics of this thread's kernel-level entry points (llmi_test_option "numerics")
static thread_local int t_hook_numerics = 0;

int32_t llmi_test_option(const char* name, int32_t value) {
    if (!name) return -1;
    int* opt = nullptr;
    if (!strcmp(name, "numerics")) {
        const int old = t_hook_numerics;
        if (value >= 0 && value <= (NUMERICS_X86 | NUMERICS_FA)) t_hook_numerics = value;
        else if (value >= 0) { set_err("llmi_test_option: numerics must be 0..3"); return -1; }
        return old;
    }
    if (!strcmp(name, "mv_unit_split")) {  // -1 auto (LLMI_MV_SPLIT), 0 off, 1 every launch that can, 2 / 3: kernels.hip
        const int old = g_mv_unit_split;
        if (value < -1 || value > 3) { set_err("llmi_test_option: mv_unit_split must be -1..3"); return -2; }
        g_mv_unit_split = value;
        return old;
    }
    if (!strcmp(name, "kv_cp_unroll")) {  // k_kv_seq_cp's items per thread: 0 auto (by the copy's size), 1, 4
        const int old = g_kv_cp_unroll;
        if (value >= 0 && value != 0 && value != 1 && value != 4) { set_err("llmi_test_option: kv_cp_unroll must be 0, 1 or 4"); return -2; }
        if (value >= 0) g_kv_cp_unroll = value;
        return old;
    }
    if (!strcmp(name, "pf_attn_simple")) opt = &g_pf_attn_simple;
    else if (!strcmp(name, "mv_split_nt")) opt = &g_mv_split_nt;  // 0 auto (LLMI_MV_SPLIT_NT), 256, 512
    else if (!strcmp(name, "pf_fa_noalloc")) opt = &g_pf_fa_noalloc;
    else if (!strcmp(name, "pf_attn_fa")) opt = &g_pf_attn_fa;
    else if (!strcmp(name, "pf_gemm_ng")) opt = &g_pf_gemm_ng;
    else if (!strcmp(name, "pf_qkv_merge")) opt = &g_pf_qkv_merge;
    else if (!strcmp(name, "pf_xcd_map")) opt = &g_pf_xcd_map;
    else if (!strcmp(name, "pf_quant_bpc")) opt = &g_pf_quant_bpc;
    else if (!strcmp(name, "pf_quant_split_below")) opt = &g_pf_quant_split_below;
    else if (!strcmp(name, "pf_fa_cfg")) opt = &g_pf_fa_cfg;
    else if (!strcmp(name, "pf_max_kv")) opt = &g_pf_max_kv;
    else if (!strcmp(name, "xspin_limit")) opt = &g_xspin_limit;
    else if (!strcmp(name, "xtag_skew")) opt = &g_xtag_skew;
    else if (!strcmp(name, "engine")) opt = &g_le_on;      // layer engine on/off (contexts made after)
    else if (!strcmp(name, "le_spin")) opt = &g_le_spin;   // layer engine's bounded-wait polls
    if (!opt) { set_err("llmi_test_option: unknown option"); return -1; }
    const int old = *opt;
    if (value >= 0) *opt = value;
    return old;
}

int32_t llmi_debug_tap(struct llama_context* ctx, int32_t which, float* out) {
    if (!ctx || !out) { set_err("llmi_debug_tap: bad arguments"); return -1; }
    Context& c = ctx->c;
    const HParams& hp = c.m->hp;
    (void)hipSetDevice(c.m->device);
    if (which == 7 || which == 8) {  // last layer's K ([HK][n_ctx][D]) or V ([HK][D][n_ctx]) cache, raw f16
        const size_t kvl = (size_t)hp.n_head_kv * c.n_ctx * hp.head_dim;
        const uint16_t* base = (which == 7 ? c.kc : c.vc) + (size_t)(hp.n_layer - 1) * kvl;
        hipError_t e = hipMemcpyAsync(out, base, kvl * 2, hipMemcpyDeviceToHost, c.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
        if (e != hipSuccess) { set_err(hip_err(e)); return -2; }
        return 0;
    }
    if (which >= 11 && which <= 15) {  // batched-step buffers, kMaxBatch rows each
        const float* b = which == 11 ? c.bx : which == 12 ? c.bq : which == 13 ? c.batt : which == 14 ? c.bh : c.blogits;
        const size_t per = which == 11 ? hp.n_embd : which == 14 ? hp.n_ff : which == 15 ? hp.n_vocab
                                                                                     : (size_t)hp.n_head * hp.head_dim;
        if (!b) { set_err("llmi_debug_tap: no batched step ran"); return -1; }
        hipError_t e = hipMemcpy(out, b, per * kMaxBatch * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { set_err(hip_err(e)); return -2; }
        return 0;
    }
    if (which == 0) {  // the last step's embedding row (get_rows), recomputed by k_embed's dequant
        DevPool P;
        float* tmp = P.get<float>((size_t)hp.n_embd * 4, false);
        if (!tmp) { set_err("out of device memory"); return -2; }
        EmbArgs ea;
        ea.w = seg_of(*c.m, c.m->tok_embd, 0);
        ea.cols = hp.n_embd;
        ea.vocab = hp.n_vocab;
        hipError_t e = launch_embed_row(ea, c.st, tmp, c.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, (size_t)hp.n_embd * 4, hipMemcpyDeviceToHost, c.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
        if (e != hipSuccess) { set_err(hip_err(e)); return -2; }
        return 0;
    }
    const float* src = which == 1 ? c.x : which == 2 ? c.q : which == 3 ? c.att : which == 4 ? c.h : nullptr;
    const size_t n = which == 1 ? hp.n_embd : which == 4 ? hp.n_ff : (size_t)hp.n_head * hp.head_dim;
    if (!src) { set_err("llmi_debug_tap: unknown tap"); return -1; }
    (void)hipSetDevice(c.m->device);
    hipError_t e = hipMemcpyAsync(out, src, n * 4, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) { set_err(hip_err(e)); return -2; }
    return 0;
}

// ---------------- kernel-level entry points (tests / microbenchmarks) ----------------
static Seg seg_at(int32_t type, const void* w, int64_t rows, int64_t cols) {
    DevMat dm;
    dm.type = type;
    dm.rows = rows;
    dm.cols = cols;
    plan_planes(dm, 0);
    Seg s;
    s.a = (const uint8_t*)w + dm.off_a;
    s.h = (const uint8_t*)w + dm.off_h;
    s.s = (const uint8_t*)w + dm.off_s;
    s.d = (const uint8_t*)w + dm.off_d;
    s.type = type;
    s.rows = (int)rows;
    s.row0 = 0;
    s.rgs = dm.rgs;
    s.x86 = (t_hook_numerics & NUMERICS_X86) != 0;
    return s;
}

int64_t llmi_device_layout_bytes(int32_t type, int64_t rows, int64_t cols) {
    if (!type_supported(type) || cols % block_elems(type)) return -1;
    if (rows > 0 && cols > 0 && !planes_fit_u32(type, rows, cols)) {
        set_err(std::string("llmi_device_layout_bytes: ") + kPlaneLimitMsg);
        return -1;
    }
    DevMat dm;
    dm.type = type; dm.rows = rows; dm.cols = cols;
    return (int64_t)plan_planes(dm, 0);
}

int32_t llmi_repack(int32_t type, const void* raw, void* w, int64_t rows, int64_t cols) {
    if (!type_supported(type) || cols % block_elems(type)) { set_err("bad type/shape"); return -1; }
    if (rows > 0 && cols > 0 && !planes_fit_u32(type, rows, cols)) {
        set_err(std::string("llmi_repack: ") + kPlaneLimitMsg);
        return -1;
    }
    DevMat dm;
    dm.type = type; dm.rows = rows; dm.cols = cols;
    plan_planes(dm, 0);
    hipError_t e;
    if (needs_repack(type)) {
        e = launch_repack(type, raw, (uint8_t*)w + dm.off_a, (uint8_t*)w + dm.off_h, (uint8_t*)w + dm.off_s,
                          (uint8_t*)w + dm.off_d, rows * (cols / block_elems(type)), cols, dm.rgs,
                          (t_hook_numerics & NUMERICS_X86) != 0, nullptr);
    } else {
        e = hipMemcpy(w, raw, dm.bytes, hipMemcpyDeviceToDevice);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_err(hip_err(e)); return -2; }
    return 0;
}

int32_t llmi_matvec(int32_t type, const void* w, int64_t rows, int64_t cols, const float* x, const float* nw, float eps,
                    float* y, int32_t mode) {
    if (!weight_type_ok(type) || cols % 256 || rows <= 0) {
        set_err("llmi_matvec: unsupported type/shape");
        return -1;
    }
    MVArgs a;
    a.seg[0] = seg_at(type, w, rows, cols);
    a.nseg = 1;
    a.cols = (int)cols;
    a.npairs = (int)((rows + 1) / 2);
    a.x = x; a.nw = nw; a.eps = eps; a.y = y;
    a.num = t_hook_numerics & NUMERICS_X86;
    hipError_t e = launch_matvec(a, mode == 1 ? EPI_ADD : EPI_STORE, hook_grid_cap(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_err(hip_err(e)); return -2; }
    return 0;
}

int32_t llmi_pf_gemm(int32_t type, const void* w, int64_t rows, int64_t cols, const float* x, const float* nw, float eps,
                     int32_t n_tok, float* y, double* usec) {
    if (!pf_gemm_ok(type, (int)rows, (int)cols) || n_tok <= 0) { set_err("llmi_pf_gemm: unsupported type/shape"); return -1; }
    API_TRY
    const int x86 = (t_hook_numerics & NUMERICS_X86) != 0;
    DevPool P;
    QuantScratch q(P, (size_t)(n_tok + 63) / 64 * 64, (size_t)cols);
    hipError_t e = P.err;
    if (e == hipSuccess) e = launch_pf_quant(x, (int)cols, nw, eps, (int)cols, act_kind(type), n_tok, q.aq, q.abs, q.ad, q.abf, nullptr, x86);
    PfGemm g;
    g.w = seg_at(type, w, rows, cols); g.rows = (int)rows; g.cols = (int)cols; g.T = n_tok;
    g.aq = q.aq; g.abs = q.abs; g.ad = q.ad; g.abf = q.abf; g.y = y; g.ldy = (int)rows;
    HipObjs h;
    auto launch = [&] { return launch_pf_gemm(g, EPI_STORE, nullptr); };
    if (e == hipSuccess) e = usec ? time_launch(h, launch, *usec) : launch();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_err(hip_err(e)); return -2; }
    return 0;
    API_CATCH(-5)
}

int32_t llmi_bmv(int32_t type, const void* w, int64_t rows, int64_t cols, const float* x, const float* nw, float eps,
                 int32_t nt, float* y, int32_t kernel) {
    if (!weight_type_ok(type) || rows <= 0 || rows > INT32_MAX ||
        cols <= 0 || cols > INT32_MAX || cols % 256 || nt < 1 || nt > kMaxBatch || kernel < 0 || kernel > 1 || !w || !x ||
        !y) {
        set_err("llmi_bmv: bad arguments");
        return -1;
    }
    API_TRY
    MVArgs a;
    a.seg[0] = seg_at(type, w, rows, cols);
    a.nseg = 1;
    a.cols = (int)cols;
    a.npairs = (int)((rows + 1) / 2);
    a.nw = nw; a.eps = eps;
    a.x_stride = (int)cols; a.y_stride = (int)rows;
    a.num = t_hook_numerics & NUMERICS_X86;
    // never a silent fall-back to k_mvn (host check, before any device call)
    if (kernel == 1 && !bmm_ok(a, EPI_STORE)) {
        set_err("llmi_bmv: the matrix-core kernels do not take these arguments (type, rows % 16, numerics, LLMI_BMM*)");
        return -1;
    }
    // k_mvn pads nt to 1, 2, 4 or 8 tokens and reads and writes the padded rows: both
    // sides go through kMaxBatch-row buffers of the hook's own, the x rows past nt zero
    const size_t xb = (size_t)cols * 4, yb = (size_t)rows * 4;
    DevPool P;
    float* xp = P.get<float>(kMaxBatch * xb);
    float* yp = P.get<float>(kMaxBatch * yb);
    hipError_t e = P.err;
    if (e == hipSuccess) e = hipMemcpy(xp, x, (size_t)nt * xb, hipMemcpyDeviceToDevice);
    a.x = xp; a.y = yp;
    if (e == hipSuccess && kernel == 0) {
        e = launch_mvn(a, EPI_STORE, nt, hook_grid_cap(), nullptr);
    } else if (e == hipSuccess) {  // the scratch of llmi_pf_gemm (a superset of the batched step's 32 rows)
        QuantScratch q(P, 64, (size_t)cols);
        e = P.err;
        if (e == hipSuccess) e = launch_pf_quant(xp, (int)cols, nw, eps, (int)cols, 0, nt, q.aq, q.abs, q.ad, q.abf, nullptr, a.num ? 1 : 0);
        if (e == hipSuccess) e = launch_bmm(a, EPI_STORE, nt, q.aq, q.abf, q.ad, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(y, yp, (size_t)nt * yb, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { set_err(std::string("llmi_bmv: ") + hip_err(e)); return -2; }
    return 0;
    API_CATCH(-5)
}

int32_t llmi_mv_epilogue(const struct llmi_epilogue_args* A) {
    auto bad = [](const char* what) {
        set_err(std::string("llmi_mv_epilogue: ") + what);
        return -1;
    };
    if (!A) return bad("null arguments");
    const int kernel = A->kernel, epi = A->epi, nt = A->nt;
    if (kernel < 0 || kernel > 4) return bad("kernel outside 0..4");
    if (epi != EPI_QKV && epi != EPI_SWIGLU && epi != EPI_LOGITS) return bad("epi is none of QKV, SWIGLU, LOGITS");
    if (kernel == 3 && epi == EPI_LOGITS) return bad("the prefill GEMM has no LOGITS epilogue");
    if (kernel == 4 && epi != EPI_QKV) return bad("kernel 4 (launch_bmm_qkv2) takes QKV only");
    const int nw = epi == EPI_QKV ? 3 : epi == EPI_SWIGLU ? 2 : 1;
    for (int i = 0; i < nw; ++i) {
        const int t = A->type[i];
        if (!weight_type_ok(t)) return bad("unknown weight type");
        if (!A->w_dev[i]) return bad("null weight");
        if (A->rows[i] <= 0 || A->rows[i] > INT32_MAX) return bad("rows out of range");
    }
    if (A->cols <= 0 || A->cols > INT32_MAX || A->cols % 256) return bad("cols must be a positive multiple of 256");
    if (!A->x_dev || !A->norm_w_dev) return bad("null x / norm weight (the RMSNorm is always fused)");
    if (kernel == 0 ? nt != 1 : kernel == 3 ? (nt < 1 || nt > (1 << 20)) : (nt < 1 || nt > kMaxBatch))
        return bad("nt out of range (kernel 0: 1, kernels 1 / 2 / 4: 1..8, kernel 3: > 0)");
    const int cols = (int)A->cols, D = A->head_dim, n_ctx = A->n_ctx;
    const int r0 = (int)A->rows[0];
    if (epi == EPI_QKV) {
        if (D <= 0 || D % 2 || n_ctx <= 0) return bad("head_dim must be positive and even, n_ctx positive");
        if (A->n_rot < 0 || A->n_rot % 2 || A->n_rot > D) return bad("n_rot must be even and at most head_dim");
        for (int i = 0; i < 3; ++i)
            if (A->rows[i] % D) return bad("rows must be multiples of head_dim");
        if (A->rows[1] != A->rows[2]) return bad("k and v must have the same rows");
        if (!A->rope_dev || !A->pos || !A->q_dev || !A->kc_dev || !A->vc_dev) return bad("null rope / pos / q / kc / vc");
        if (kernel == 3) {
            if (A->pos[0] < 0 || (int64_t)A->pos[0] + nt > n_ctx) return bad("pos0 + T > n_ctx");
        } else {
            for (int t = 0; t < nt; ++t)
                if (A->pos[t] < 0 || A->pos[t] >= n_ctx) return bad("position outside 0..n_ctx-1");
        }
    } else {
        if (!A->y_dev) return bad("null y");
        if (epi == EPI_SWIGLU && A->rows[0] != A->rows[1]) return bad("gate and up must have the same rows");
        if (epi == EPI_LOGITS) {
            if (!A->pos || !A->token_out || !A->pos_next_out) return bad("null pos / token_out / pos_next_out");
            for (int t = 0; t < nt; ++t)
                if (A->pos[t] < 0 || A->pos[t] == INT32_MAX) return bad("position out of range");
        }
    }
    API_TRY
    const int num = t_hook_numerics & NUMERICS_X86;
    Seg seg[3];
    for (int i = 0, row0 = 0; i < nw; ++i) {
        seg[i] = seg_at(A->type[i], A->w_dev[i], A->rows[i], cols);
        seg[i].row0 = epi == EPI_QKV ? row0 : 0;
        row0 += (int)A->rows[i];
    }
    const int nq = r0, nk = epi == EPI_QKV ? (int)A->rows[1] : 0;
    const int ldy = r0;  // floats per row of the f32 output (q, h or the logits)
    // the launches' descriptors (kernels 0 / 1 / 2 / 4), grouped as the engine groups them
    MVArgs base;
    base.cols = cols; base.nw = A->norm_w_dev; base.eps = A->eps; base.num = num;
    if (epi == EPI_QKV) {
        base.rope = A->rope_dev; base.head_dim = D; base.n_rot = A->n_rot; base.n_ctx = n_ctx; base.nq = nq; base.nk = nk;
    }
    MVArgs grp[3];
    int ng = 1, first[3] = {0, 0, 0};
    if (epi == EPI_QKV) {
        const Seg qkv[3] = {seg[0], seg[1], seg[2]};
        ng = qkv_launch_groups(qkv, kernel == 0, base, grp, first);
    } else {
        grp[0] = base;
        grp[0].nseg = nw;
        for (int i = 0; i < nw; ++i) grp[0].seg[i] = seg[i];
        grp[0].npairs = epi == EPI_SWIGLU ? r0 : (r0 + 1) / 2;
    }
    // never another kernel than the one asked for: what it does not take is refused here,
    // on the host, before any device call
    auto one_type = [](const MVArgs& a) {
        for (int i = 1; i < a.nseg; ++i)
            if (a.seg[i].type != a.seg[0].type) return false;
        return true;
    };
    if (kernel == 0 || kernel == 1) {
        for (int g = 0; g < ng; ++g) {
            MVArgs probe = grp[g];
            for (int i = 1; i < probe.nseg; ++i)
                if (act_kind(probe.seg[i].type) != act_kind(probe.seg[0].type))
                    return bad("launch_matvec / launch_mvn take segments of one activation kind");
            if (kernel == 1 && !one_type(probe)) return bad("launch_mvn takes segments of one type");
            if (!mv_geometry(probe, epi)) return bad("the segments cannot be cut into row tasks");
        }
    } else if (kernel == 2 || kernel == 4) {
        if (kernel == 4 && ng != 2) return bad("kernel 4 (launch_bmm_qkv2) takes a QKV of two type groups");
        for (int g = 0; g < ng; ++g)
            if (!bmm_ok(grp[g], epi))
                return bad("the matrix-core kernels do not take these arguments (type, rows % 16, numerics, LLMI_BMM*)");
    } else {
        for (int i = 0; i < nw; ++i)
            if (!pf_gemm_ok(A->type[i], (int)A->rows[i], cols)) return bad("launch_pf_gemm does not take this type / shape");
        if (epi == EPI_SWIGLU && act_kind(A->type[0]) != act_kind(A->type[1]))
            return bad("prefill: ffn_gate / ffn_up of different activation kinds");
    }

    DevPool P;
    const int mb = hook_grid_cap();
    const size_t kvl = epi == EPI_QKV ? (size_t)(nk / D) * n_ctx * D : 0;  // elements of one cache
    // one StepState per token slot + the dummy one of the padded slots
    const int nslot = kernel == 0 || kernel == 3 ? 1 : nt;
    std::vector<StepState> hs((size_t)nslot + 1);
    for (int t = 0; t < nslot; ++t) {
        StepState& s = hs[(size_t)t];
        memset(&s, 0, sizeof(s));
        s.pos = s.pos_next = A->pos && kernel != 3 ? A->pos[t] : 0;
        s.seq = 1;
    }
    memset(&hs[(size_t)nslot], 0, sizeof(StepState));
    StepState* st = P.get<StepState>(hs.size() * sizeof(StepState));
    hipError_t e = P.err;
    if (e == hipSuccess) e = hipMemcpy(st, hs.data(), hs.size() * sizeof(StepState), hipMemcpyHostToDevice);
    const char* refused = nullptr;
    if (kernel == 0) {
        for (int g = 0; g < ng && e == hipSuccess; ++g) {
            MVArgs& a = grp[g];
            a.x = A->x_dev; a.st = st;
            if (epi == EPI_QKV) { a.y = A->q_dev; a.kc = A->kc_dev; a.vc = A->vc_dev; }
            else a.y = A->y_dev;
            if (epi == EPI_LOGITS) a.argmax = &st->key[0][0];
            e = launch_matvec(a, epi, mb, nullptr);
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
    } else if (kernel == 3) {
        const int T = nt, x86 = num ? 1 : 0;
        const size_t tpad = (size_t)(T + 63) / 64 * 64;
        QuantScratch q(P, tpad, (size_t)cols);
        e = P.err;
        PfGemm g;
        g.T = T; g.cols = cols; g.aq = q.aq; g.abs = q.abs; g.ad = q.ad; g.abf = q.abf;
        if (epi == EPI_QKV) {
            // prefill_enqueue's q / k / v launches (pf_qkv_launches)
            g.kc = A->kc_dev; g.vc = A->vc_dev; g.rope = A->rope_dev;
            g.pos0 = A->pos[0]; g.head_dim = D; g.n_rot = A->n_rot; g.n_ctx = n_ctx;
            g.y = A->q_dev; g.ldy = nq;
            PfGemm qg[3];
            int qkind[3];
            const int nqg = pf_qkv_launches(seg, g_pf_qkv_merge != 0, g, qg, qkind);
            for (int i = 0; i < nqg && e == hipSuccess; ++i) {
                if (qkind[i] >= 0)
                    e = launch_pf_quant(A->x_dev, cols, A->norm_w_dev, A->eps, cols, qkind[i], T, q.aq, q.abs, q.ad, q.abf,
                                        nullptr, x86);
                if (e == hipSuccess) e = launch_pf_gemm(qg[i], EPI_QKV, nullptr);
            }
        } else {  // gate into y, then y = silu(y) * up
            if (e == hipSuccess)
                e = launch_pf_quant(A->x_dev, cols, A->norm_w_dev, A->eps, cols, act_kind(A->type[0]), T, q.aq, q.abs, q.ad,
                                    q.abf, nullptr, x86);
            g.w = seg[0]; g.w2 = seg[1]; g.rows = r0; g.y = A->y_dev; g.ldy = ldy;
            if (e == hipSuccess) e = launch_pf_gemm(g, EPI_STORE, nullptr);
            g.w = seg[1];
            if (e == hipSuccess) e = launch_pf_gemm(g, EPI_SWIGLU_UP, nullptr);
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
    } else {
        // the batched step's buffers: kMaxBatch rows of x and of the f32 output (k_mvn reads
        // and writes the padded rows), nt + 1 caches (the last one the padded slots'), the
        // slot -> position / sequence maps
        const size_t xb = (size_t)cols * 4, yb = (size_t)ldy * 4;
        float* xp = P.get<float>(kMaxBatch * xb);
        float* yp = P.get<float>(kMaxBatch * yb);
        float* yout = epi == EPI_QKV ? A->q_dev : A->y_dev;
        uint16_t *kcp = nullptr, *vcp = nullptr;
        if (epi == EPI_QKV) {
            kcp = P.get<uint16_t>((size_t)(nt + 1) * kvl * 2);
            vcp = P.get<uint16_t>((size_t)(nt + 1) * kvl * 2);
        }
        int hmap[2 * kMaxBatch];  // [0, 8): positions, [8, 16): sequences
        for (int t = 0; t < kMaxBatch; ++t) {
            hmap[t] = t < nt && A->pos ? A->pos[t] : 0;
            hmap[kMaxBatch + t] = t < nt ? t : nt;
        }
        int* dmap = P.get<int>(sizeof(hmap));
        e = e == hipSuccess ? P.err : e;
        if (e == hipSuccess) e = hipMemcpy(dmap, hmap, sizeof(hmap), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(xp, A->x_dev, (size_t)nt * xb, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(yp, yout, (size_t)nt * yb, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && kcp) e = hipMemcpy(kcp, A->kc_dev, (size_t)nt * kvl * 2, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && vcp) e = hipMemcpy(vcp, A->vc_dev, (size_t)nt * kvl * 2, hipMemcpyDeviceToDevice);
        for (int g = 0; g < ng; ++g) {
            MVArgs& a = grp[g];
            a.x = xp; a.x_stride = cols; a.y = yp; a.y_stride = ldy; a.st = st;
            a.tpos = dmap; a.tseq = dmap + kMaxBatch; a.kv_stride = kvl; a.kc = kcp; a.vc = vcp;
        }
        if (kernel == 1) {
            for (int g = 0; g < ng && e == hipSuccess; ++g) e = launch_mvn(grp[g], epi, nt, mb, nullptr);
        } else {
            QuantScratch q(P, 64, (size_t)cols);
            if (e == hipSuccess) e = P.err;
            if (e == hipSuccess)
                e = launch_pf_quant(xp, cols, A->norm_w_dev, A->eps, cols, 0, nt, q.aq, q.abs, q.ad, q.abf, nullptr, num ? 1 : 0);
            if (kernel == 2) {
                for (int g = 0; g < ng && e == hipSuccess; ++g) e = launch_bmm(grp[g], epi, nt, q.aq, q.abf, q.ad, nullptr);
            } else if (e == hipSuccess) {
                e = launch_bmm_qkv2(grp[0], grp[1], nt, q.aq, q.abf, q.ad, nullptr);
                if (e == hipErrorNotSupported) {
                    refused = "launch_bmm_qkv2 does not take this pair of types (or LLMI_BMM2 / LLMI_BMM_DMA is 0)";
                    e = hipSuccess;
                }
            }
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess && !refused) e = hipMemcpy(yout, yp, (size_t)nt * yb, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && !refused && kcp) e = hipMemcpy(A->kc_dev, kcp, (size_t)nt * kvl * 2, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && !refused && vcp) e = hipMemcpy(A->vc_dev, vcp, (size_t)nt * kvl * 2, hipMemcpyDeviceToDevice);
    }
    if (refused) return bad(refused);
    if (e == hipSuccess && epi == EPI_LOGITS) {
        e = hipMemcpy(hs.data(), st, hs.size() * sizeof(StepState), hipMemcpyDeviceToHost);
        for (int t = 0; t < nt && e == hipSuccess; ++t) {
            A->token_out[t] = key_token(hs[(size_t)t].key[A->pos[t] & 1]);
            A->pos_next_out[t] = hs[(size_t)t].pos_next;
        }
    }
    if (e != hipSuccess) { set_err(std::string("llmi_mv_epilogue: ") + hip_err(e)); return -2; }
    return 0;
    API_CATCH(-5)
}

static_assert(sizeof(llmi_step_state) == sizeof(StepState) && offsetof(llmi_step_state, key) == offsetof(StepState, key) &&
                  offsetof(llmi_step_state, seq) == offsetof(StepState, seq),
              "llmi_step_state mirrors StepState");

int32_t llmi_step_entry(const struct llmi_step_entry_args* A) {
    auto bad = [](const char* what) {
        set_err(std::string("llmi_step_entry: ") + what);
        return -1;
    };
    if (!A) return bad("null arguments");
    const int kernel = A->kernel, nt = A->nt, n_seq = A->n_seq, n_ctx = A->n_ctx;
    if (kernel < 0 || kernel > 3) return bad("kernel outside 0..3");
    if (!weight_type_ok(A->type)) return bad("unknown weight type");
    if (!A->w_dev) return bad("null weight");
    if (A->cols <= 0 || A->cols > INT32_MAX || A->cols % 256) return bad("cols must be a positive multiple of 256");
    if (A->vocab <= 0 || A->vocab > INT32_MAX) return bad("vocab out of range");
    if (!planes_fit_u32(A->type, A->vocab, A->cols)) return bad(kPlaneLimitMsg);
    if (kernel == 1 ? (nt < 1 || nt > kMaxBatch) : kernel == 2 ? (nt < 1 || nt > 65535) : nt != 1)
        return bad("nt out of range (kernels 0 / 3: 1, kernel 1: 1..8, kernel 2: 1..65535)");
    if (kernel == 1 ? (n_seq < nt || n_seq > 64) : n_seq != 1) return bad("n_seq out of range (kernel 1: nt..64, else 1)");
    if (n_ctx <= 0 || n_ctx > (1 << 20)) return bad("n_ctx outside 1..2^20");
    if (kernel == 1) {
        if (!A->tseq || !A->tpos) return bad("null tseq / tpos");
        for (int s = 0; s < nt; ++s) {
            if (A->tseq[s] < 0 || A->tseq[s] >= n_seq) return bad("tseq outside 0..n_seq-1");
            for (int r = 0; r < s; ++r)
                if (A->tseq[r] == A->tseq[s]) return bad("tseq names a sequence twice");
        }
    }
    if (kernel == 2) {
        if (!A->tokens) return bad("null tokens");
        if (A->pos0 < 0 || A->pos0 > INT32_MAX - nt) return bad("pos0 out of range");
    } else if (!A->states) {
        return bad("null states");
    }
    if (kernel != 3 && !A->hist) return bad("null hist");
    if (!A->x_out || !A->guard_bad) return bad("null x_out / guard_bad");
    API_TRY
    const int cols = (int)A->cols, vocab = (int)A->vocab;
    const size_t slots = kernel == 1 ? (size_t)kMaxBatch : kernel == 2 ? (size_t)nt : 1;
    constexpr size_t G = 1024;  // guard words before and after each buffer
    DevPool P;
    // a device buffer of `words` 32-bit words between two guards, everything the sentinel but
    // the `init` words copied in
    struct Guarded {
        uint32_t* dev = nullptr;
        size_t words = 0;
        std::vector<uint32_t> host;
        uint32_t* body() { return dev + G; }
    };
    auto make = [&](Guarded& g, size_t words, const void* init) {
        g.words = words;
        g.host.assign(words + 2 * G, LLMI_STEP_SENTINEL);
        if (init) memcpy(g.host.data() + G, init, words * 4);
        g.dev = P.get<uint32_t>(g.host.size() * 4, false);
        if (g.dev) P.err = hipMemcpy(g.dev, g.host.data(), g.host.size() * 4, hipMemcpyHostToDevice);
    };
    // back to the host: the body into `out`, the guards counted
    auto fetch = [&](Guarded& g, void* out, int32_t& nbad) -> hipError_t {
        nbad = 0;
        if (!g.dev) return hipSuccess;
        const hipError_t e = hipMemcpy(g.host.data(), g.dev, g.host.size() * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        for (size_t i = 0; i < G; ++i)
            nbad += (g.host[i] != LLMI_STEP_SENTINEL) + (g.host[G + g.words + i] != LLMI_STEP_SENTINEL);
        if (out) memcpy(out, g.host.data() + G, g.words * 4);
        return hipSuccess;
    };
    Guarded gx, gh, gs;
    make(gx, slots * (size_t)cols, nullptr);
    if (kernel != 3) make(gh, (size_t)n_seq * n_ctx, A->hist);
    if (kernel != 2) make(gs, (size_t)n_seq * sizeof(StepState) / 4, A->states);
    int hmap[2 * kMaxBatch] = {};  // [0, 8): tpos, [8, 16): tseq
    int* dmap = nullptr;
    int32_t* dtok = nullptr;
    if (kernel == 1) {
        for (int s = 0; s < kMaxBatch; ++s) hmap[s] = A->tpos[s];
        for (int s = 0; s < nt; ++s) hmap[kMaxBatch + s] = A->tseq[s];
        dmap = P.get<int>(sizeof(hmap), false);
        if (dmap) P.err = hipMemcpy(dmap, hmap, sizeof(hmap), hipMemcpyHostToDevice);
    } else if (kernel == 2) {
        dtok = P.get<int32_t>((size_t)nt * 4, false);
        if (dtok) P.err = hipMemcpy(dtok, A->tokens, (size_t)nt * 4, hipMemcpyHostToDevice);
    }
    hipError_t e = P.err;
    const Seg w = seg_at(A->type, A->w_dev, vocab, cols);
    if (e == hipSuccess && (kernel == 0 || kernel == 3)) {
        EmbArgs ea;
        ea.w = w; ea.cols = cols; ea.vocab = vocab; ea.n_ctx = n_ctx;
        ea.x = (float*)gx.body();
        ea.st = (StepState*)gs.body();
        ea.hist = kernel == 0 ? (int32_t*)gh.body() : nullptr;
        e = kernel == 0 ? launch_embed(ea, nullptr) : launch_embed_row(ea, ea.st, ea.x, nullptr);
    } else if (e == hipSuccess && kernel == 1) {
        BEmbArgs ba;
        ba.w = w; ba.cols = cols; ba.vocab = vocab; ba.n_ctx = n_ctx; ba.nt = nt;
        ba.x = (float*)gx.body();
        ba.st = (StepState*)gs.body();
        ba.hist = (int32_t*)gh.body();
        ba.tseq = dmap + kMaxBatch;
        ba.tpos = dmap;
        e = launch_bembed(ba, nullptr);
    } else if (e == hipSuccess) {
        e = launch_pf_embed(w, cols, vocab, dtok, (float*)gx.body(), nt, (int32_t*)gh.body(), A->pos0, n_ctx, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = fetch(gx, A->x_out, A->guard_bad[0]);
    if (e == hipSuccess) e = fetch(gh, A->hist, A->guard_bad[1]);
    if (e == hipSuccess) e = fetch(gs, A->states, A->guard_bad[2]);
    if (e == hipSuccess && kernel == 1) {
        e = hipMemcpy(hmap, dmap, sizeof(hmap), hipMemcpyDeviceToHost);
        for (int s = 0; s < kMaxBatch && e == hipSuccess; ++s) A->tpos[s] = hmap[s];
    }
    if (e != hipSuccess) { set_err(std::string("llmi_step_entry: ") + hip_err(e)); return -2; }
    return 0;
    API_CATCH(-5)
}

int32_t llmi_quantize_act(int32_t type, int64_t cols, const float* x, const float* nw, float eps, void* out) {
    if (cols % 256) { set_err("cols must be a multiple of 256"); return -1; }
    MVArgs a;
    a.cols = (int)cols; a.x = x; a.nw = nw; a.eps = eps;
    a.num = t_hook_numerics & NUMERICS_X86;
    hipError_t e = launch_quant_dump(a, act_kind(type), out, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_err(hip_err(e)); return -2; }
    return 0;
}

double llmi_bench_matvec_ex(int32_t type, const void* w, int32_t n_mats, int64_t rows, int64_t cols, const float* x, float* y,
                            int32_t reps, int32_t mode) {
    const int64_t lb = llmi_device_layout_bytes(type, rows, cols);
    if (lb <= 0 || n_mats <= 0 || reps <= 0) { set_err("bad arguments"); return -1.0; }
    const size_t stride = align_up((size_t)lb, 4096);
    API_TRY
    const int mb = hook_grid_cap();
    // mode bit 5: gate+up SwiGLU launch (rows = both halves; RMSNorm on), bit 6: residual-add
    // epilogue (ffn_down / attn_output)
    const bool swiglu = mode & 32, add = mode & 64;
    const bool norm = (mode & 1) || swiglu, logits = mode & 2, img = mode & 8;
    DevPool P;
    float* nw = norm ? P.get<float>((size_t)cols * 4, false) : nullptr;
    StepState* st = logits ? P.get<StepState>(sizeof(StepState)) : nullptr;
    // mode bit 3: timing with a pre-quantized activation image (zeros)
    const uint8_t* xq = img ? P.get<uint8_t>((size_t)(cols / 256) * 304) : nullptr;
    if (P.err != hipSuccess) { set_err("out of device memory"); return -1.0; }
    if (norm) {
        std::vector<float> ones((size_t)cols, 1.0f);
        (void)hipMemcpy(nw, ones.data(), (size_t)cols * 4, hipMemcpyHostToDevice);
    }
    MVArgs a;
    a.nseg = 1; a.cols = (int)cols; a.npairs = (int)((rows + 1) / 2); a.x = x; a.y = y; a.xq = xq;
    a.nw = nw; a.eps = 1e-5f; a.xfirst = (mode & 4) ? 1 : (mode & 256) ? -1 : 0;  // mode bit 2: weights after x, bit 8: never
    if (mode & 16) {  // mode bit 4 (experiment builds): alternating priority, blocks past the CU count in the other phase
        int dev = 0;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&a.prio_alt, hipDeviceAttributeMultiprocessorCount, dev);
    }
    if (logits) { a.st = st; a.argmax = &st->key[0][0]; }
    const int epi = logits ? EPI_LOGITS : swiglu ? EPI_SWIGLU : add ? EPI_ADD : EPI_STORE;
    const size_t half = swiglu ? (size_t)llmi_device_layout_bytes(type, rows / 2, cols) : 0;
    // one graph of n_mats launches (one per weight copy), replayed: no host launch cost
    HipObjs h;
    (void)hipStreamCreateWithFlags(&h.s, hipStreamNonBlocking);
    // mode bit 7: every launch reads copy 0 (its weights L2/MALL-hot from the launch before)
    const size_t wstride = (mode & 128) ? 0 : stride;
    std::string err;
    h.ex = capture_graph(h.s, [&](std::string&) {
        bool ok = true;
        for (int k = 0; ok && k < n_mats; ++k) {
            if (swiglu) {
                a.nseg = 2;
                a.seg[0] = seg_at(type, (const uint8_t*)w + wstride * k, rows / 2, cols);
                a.seg[1] = seg_at(type, (const uint8_t*)w + wstride * k + half, rows / 2, cols);
            } else {
                a.seg[0] = seg_at(type, (const uint8_t*)w + wstride * k, rows, cols);
            }
            ok = launch_matvec(a, epi, mb, h.s) == hipSuccess;
        }
        return ok;
    }, err);
    if (!h.ex) { set_err("llmi_bench_matvec: capture/launch failed"); return -1.0; }
    return replay_us(h, std::max(1, reps / n_mats), n_mats);
    API_CATCH(-1.0)
}

double llmi_bench_matvec(int32_t type, const void* w, int32_t n_mats, int64_t rows, int64_t cols, const float* x, float* y,
                         int32_t reps) {
    return llmi_bench_matvec_ex(type, w, n_mats, rows, cols, x, y, reps, 0);
}

double llmi_bench_stream(const void* dev, int32_t n_bufs, uint64_t stride, uint64_t bytes, int32_t reps, int32_t blocks) {
    API_TRY
    DevPool P;
    unsigned* out = P.get<unsigned>(16, false);
    if (!out) return -1.0;
    for (int k = 0; k < n_bufs; ++k) (void)launch_stream_read((const uint8_t*)dev + stride * k, bytes, out, blocks, nullptr);
    HipObjs h;
    double us = 0.0;
    const hipError_t e = time_launch(h, [&] {
        for (int r = 0; r < reps; ++r) (void)launch_stream_read((const uint8_t*)dev + stride * (r % n_bufs), bytes, out, blocks, nullptr);
        return hipSuccess;
    }, us);
    return e == hipSuccess ? us / reps : -1.0;
    API_CATCH(-1.0)
}

}  // extern "C"

// Attention microbenchmark (kernel level, no model): n_layers distinct KV caches of
// n_ctx = round256(n_kv) positions (>= 512 MB in total, so replays stream them from HBM
// like a decode step does), one launch per layer captured into a graph, `reps` graph
// replays timed between two events.  Returns microseconds per launch (incl. the
// dependent-launch gap), < 0 on error.  mode: attention path (0 auto, 1 fused, 2 split, 3 two-kernel).
int32_t llmi_attention(int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t n_kv, int32_t n_ctx, const float* q,
                       const uint16_t* kc, const uint16_t* vc, float* out, int32_t mode) {
    if (!head_shape_ok(n_head, n_head_kv, head_dim) || n_kv <= 0 || n_ctx < n_kv || n_ctx % 256 || !q || !kc || !vc || !out) {
        set_err("llmi_attention: bad arguments");
        return -1;
    }
    API_TRY
    DevPool P;
    float* scores = P.get<float>(attn_scratch_floats(n_head, n_ctx) * 4);
    StepState* st = dev_states(P, &n_kv, 1, 1);
    if (P.err != hipSuccess) { set_err("llmi_attention: out of device memory"); return -2; }
    AttnArgs a;
    a.q = q; a.kc = kc; a.vc = vc; a.out = out; a.st = st; a.n_ctx = n_ctx;
    a.scale = 1.0f / sqrtf((float)head_dim);
    attn_bind_scratch(a, scores, n_head, n_ctx);
    a.num = t_hook_numerics & NUMERICS_X86;
    a.fa = (t_hook_numerics & NUMERICS_FA) ? 1 : 0;
    hipError_t e = launch_attention(a, n_head, n_head_kv, head_dim, kv_bucket_bound(n_kv, n_ctx), nullptr, mode);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_err(std::string("llmi_attention: ") + hip_err(e)); return -3; }
    return 0;
    API_CATCH(-5)
}

// k_kv_seq_cp alone over the caller's device memory (llama_kv_self_seq_cp's launch).  Every
// refusal comes before the first device call, so a machine without a GPU can ask for them.
int32_t llmi_kv_seq_copy(int32_t n_planes, int32_t head_dim, int32_t n_ctx, int32_t p0, int32_t p1, const uint16_t* kc_src,
                         const uint16_t* vc_src, const int32_t* hist_src, uint16_t* kc_dst, uint16_t* vc_dst,
                         int32_t* hist_dst, double* usec) {
    API_TRY
    const std::string who = "llmi_kv_seq_copy: ";
    const struct { const char* field; const void* p; } ptrs[] = {{"kc_src", kc_src}, {"vc_src", vc_src}, {"hist_src", hist_src},
                                                                {"kc_dst", kc_dst}, {"vc_dst", vc_dst}, {"hist_dst", hist_dst}};
    for (const auto& f : ptrs)
        if (!f.p) { set_err(who + f.field + " is a null pointer"); return -1; }
    if (n_planes <= 0) { set_err(who + "n_planes must be positive"); return -1; }
    if (head_dim <= 0 || head_dim % 8) { set_err(who + "head_dim must be a positive multiple of 8"); return -1; }
    if (n_ctx <= 0 || n_ctx % 256) { set_err(who + "n_ctx must be a positive multiple of 256"); return -1; }
    if (p0 < 0 || p0 >= p1) { set_err(who + "p0 outside 0 <= p0 < p1"); return -1; }
    if (p1 > n_ctx) { set_err(who + "p1 beyond n_ctx"); return -1; }
    KvCopyArgs a;
    a.kc_src = kc_src; a.vc_src = vc_src; a.hist_src = hist_src;
    a.kc_dst = kc_dst; a.vc_dst = vc_dst; a.hist_dst = hist_dst;
    a.n_planes = n_planes; a.head_dim = head_dim; a.n_ctx = n_ctx; a.p0 = p0; a.p1 = p1;
    if (!kv_seq_cp_ok(a)) { set_err(who + "n_planes * head_dim too large"); return -1; }
    const int cap = hook_grid_cap();
    if (cap <= 0) { set_err(who + "device query failed"); return -2; }
    HipObjs h;
    auto launch = [&] { return launch_kv_seq_cp(a, cap, nullptr); };
    hipError_t e = usec ? time_launch(h, launch, *usec) : launch();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_err(who + hip_err(e)); return -3; }
    return 0;
    API_CATCH(-5)
}

// k_embd_rows / k_embd_mean alone over the caller's device memory (the launch llama_decode
// makes per prefill chunk and decode step in embeddings mode).  Every refusal comes before
// the first device call, so a machine without a GPU can ask for them.
int32_t llmi_embd_pool(const float* x_dev, int64_t ldx, int32_t n_tok, int32_t n_embd, const float* norm_w_dev, float eps,
                       int32_t pooling, int32_t n_total, int32_t t0, double* acc_dev, float* out_dev, double* usec) {
    API_TRY
    const std::string who = "llmi_embd_pool: ";
    EmbdPoolArgs a;
    a.x = x_dev; a.ldx = ldx; a.n_tok = n_tok; a.n_embd = n_embd; a.w = norm_w_dev; a.eps = eps;
    a.pooling = pooling; a.n_total = n_total; a.t0 = t0; a.acc = acc_dev; a.out = out_dev;
    std::string why;
    if (!embd_pool_ok(a, why)) { set_err(who + why); return -1; }
    DevPool P;
    if (pooling == POOLING_MEAN) {
        a.scale = P.get<float>((size_t)n_tok * sizeof(float));
        if (!a.scale) { set_err(who + hip_err(P.err)); return -2; }
    }
    HipObjs h;
    auto launch = [&] { return launch_embd_pool(a, nullptr); };
    hipError_t e = usec ? time_launch(h, launch, *usec) : launch();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_err(who + hip_err(e)); return -3; }
    return 0;
    API_CATCH(-5)
}

// The decode attention path launch_attention takes for this shape, KV bound and mode (host
// only: no device call, so a test can ask on a machine without a GPU).
int32_t llmi_attn_path(int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t kv_bound, int32_t mode) {
    if (!head_shape_ok(n_head, n_head_kv, head_dim) || kv_bound <= 0 || mode < 0 || mode > 7) {
        set_err("llmi_attn_path: bad arguments");
        return -1;
    }
    return attn_path(n_head, n_head_kv, kv_bound, head_dim, mode);
}

// The form launch_attention takes in x86 numerics (host only): k_a86_h's pass class, or 0.
int32_t llmi_attn_x86_form(int32_t kv_bound, int32_t mode) {
    if (kv_bound <= 0 || mode < 0 || mode > 7) { set_err("llmi_attn_x86_form: bad arguments"); return -1; }
    return attn_x86_form(kv_bound, mode);
}

// One batched-step attention (bstep_enqueue's launch_battention) of nt slots: slot t is one
// sequence with its own caches, query, output, StepState (pos = n_kv[t] - 1) and scratch,
// laid out as the batched step lays them out; the KV bound is the batch's (its longest slot).
int32_t llmi_battention(int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t nt, const int32_t* n_kv, int32_t n_ctx,
                        const float* q, const uint16_t* kc, const uint16_t* vc, float* out) {
    if (!head_shape_ok(n_head, n_head_kv, head_dim) || nt < 1 || nt > kMaxBatch || !n_kv || n_ctx <= 0 || n_ctx % 256 || !q ||
        !kc || !vc || !out) {
        set_err("llmi_battention: bad arguments");
        return -1;
    }
    int max_kv = 0;
    for (int t = 0; t < nt; ++t) {
        if (n_kv[t] <= 0 || n_kv[t] > n_ctx) { set_err("llmi_battention: n_kv outside 1..n_ctx"); return -1; }
        max_kv = std::max(max_kv, n_kv[t]);
    }
    API_TRY
    const size_t scr = attn_scratch_floats(n_head, n_ctx);
    const size_t QD = (size_t)n_head * head_dim, kvl = (size_t)n_head_kv * n_ctx * head_dim;
    DevPool P;
    float* scores = P.get<float>((size_t)nt * scr * 4);
    StepState* st = dev_states(P, n_kv, nt, 1);
    if (P.err != hipSuccess) { set_err("llmi_battention: out of device memory"); return -2; }
    BAttnArgs ba;
    for (int t = 0; t < nt; ++t) {
        AttnArgs& at = ba.a[t];
        at.q = q + (size_t)t * QD; at.kc = kc + (size_t)t * kvl; at.vc = vc + (size_t)t * kvl;
        // (bstep_enqueue binds without the exchange path's granules: no batched path reads them)
        attn_bind_scratch(at, scores + (size_t)t * scr, n_head, n_ctx);
        at.out = out + (size_t)t * QD; at.st = st + t; at.n_ctx = n_ctx;
        at.scale = 1.0f / sqrtf((float)head_dim);
        at.num = t_hook_numerics & NUMERICS_X86;
        at.fa = (t_hook_numerics & NUMERICS_FA) ? 1 : 0;
    }
    hipError_t e = launch_battention(ba, nt, n_head, n_head_kv, head_dim, kv_bucket_bound(max_kv, n_ctx), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_err(std::string("llmi_battention: ") + hip_err(e)); return -3; }
    return 0;
    API_CATCH(-5)
}

// The three llmi_pf_attention* hooks after their own argument checks: one timed
// launch_pf_attn over T rows at pos0.. (`at` brings the numerics and, for path 0, the score
// scratch); microseconds, -3 on a launch error
static double pf_attention_run(const char* name, PfAttn at, int n_head, int n_head_kv, int head_dim, int T, int pos0,
                               int n_ctx, const float* q, const uint16_t* kc, const uint16_t* vc, float* out, int path = -1) {
    at.q = q; at.out = out; at.ldq = n_head * head_dim; at.kc = kc; at.vc = vc;
    at.n_ctx = n_ctx; at.pos0 = pos0; at.gqa = n_head / n_head_kv; at.max_kv = pos0 + T;
    at.scale = 1.0f / sqrtf((float)head_dim);
    HipObjs h;
    double us = 0.0;
    hipError_t e = time_launch(h, [&] { return launch_pf_attn(at, n_head, head_dim, T, nullptr, path); }, us);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_err(std::string(name) + ": " + hip_err(e)); return -3; }
    return us;
}
// the arguments the three hooks check alike
static bool pf_attention_args_ok(int n_head, int n_head_kv, int head_dim, int T, int pos0, int n_ctx, const void* q,
                                 const void* kc, const void* vc, const void* out) {
    return head_shape_ok(n_head, n_head_kv, head_dim) && T > 0 && pos0 >= 0 && n_ctx % 256 == 0 && pos0 + T <= n_ctx && q &&
           kc && vc && out;
}

double llmi_pf_attention(int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t T, int32_t pos0, int32_t n_ctx,
                         const float* q, const uint16_t* kc, const uint16_t* vc, float* out, int32_t mode,
                         int64_t scratch_bytes) {
    // mode 0 runs to n_ctx, the rule prefill_max_kv applies when k_pf_fa's scratch exists
    // (pf_attention_args_ok); the LDS kernels' score rows end at kPfAttnMaxKV
    if (!pf_attention_args_ok(n_head, n_head_kv, head_dim, T, pos0, n_ctx, q, kc, vc, out) || mode < 0 || mode > 2 ||
        (mode != 0 && pos0 + T > kPfAttnMaxKV)) {
        set_err("llmi_pf_attention: bad arguments");
        return -1;
    }
    API_TRY
    PfAttn at;
    DevPool P;
    if (mode == 0) {
        size_t bytes = pf_fa_scratch_bytes(n_head, n_head_kv, head_dim, std::max(T, 512), n_ctx);
        if (!bytes) { set_err("llmi_pf_attention: no tiled kernel for this head shape"); return -1; }
        if (scratch_bytes > 0) bytes = (size_t)scratch_bytes;
        at.wsc = P.get<float>(bytes, false);
        if (!at.wsc) { set_err("llmi_pf_attention: out of device memory"); return -2; }
        at.wsc_bytes = bytes;
    }
    return pf_attention_run("llmi_pf_attention", at, n_head, n_head_kv, head_dim, T, pos0, n_ctx, q, kc, vc, out, mode);
    API_CATCH(-5)
}

// The kernel launch_pf_attn takes in an LDS mode at max_kv score positions (the ladder's
// ceilings come from each kernel's static LDS: a device query, cached).
int32_t llmi_pf_attn_path(int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t max_kv, int32_t mode) {
    if (!head_shape_ok(n_head, n_head_kv, head_dim) || max_kv <= 0 || mode < 1 || mode > 2) {
        set_err("llmi_pf_attn_path: bad arguments");
        return -2;
    }
    API_TRY
    return pf_attn_path(n_head, n_head_kv, head_dim, max_kv, mode);
    API_CATCH(-5)
}

double llmi_pf_attention_fa(int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t T, int32_t pos0, int32_t n_ctx,
                            const float* q, const uint16_t* kc, const uint16_t* vc, float* out) {
    if (!pf_attention_args_ok(n_head, n_head_kv, head_dim, T, pos0, n_ctx, q, kc, vc, out) || n_head / n_head_kv > 32 ||
        pos0 + T > kFaMaxKV) {
        set_err("llmi_pf_attention_fa: bad arguments");
        return -1;
    }
    API_TRY
    PfAttn at;
    at.num = t_hook_numerics & NUMERICS_X86;
    at.fa = 1;
    return pf_attention_run("llmi_pf_attention_fa", at, n_head, n_head_kv, head_dim, T, pos0, n_ctx, q, kc, vc, out);
    API_CATCH(-5)
}

// The x86 association's prefill kernel alone (k_pf_a86): PfAttn::num set, so launch_pf_attn
// goes to launch_pf_attn_x86 and to nothing else; what that refuses (a KV length past
// pf_attn_x86_max_kv, a head shape without an instantiation) is an error here.
double llmi_pf_attention_x86(int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t T, int32_t pos0, int32_t n_ctx,
                             const float* q, const uint16_t* kc, const uint16_t* vc, float* out) {
    if (!pf_attention_args_ok(n_head, n_head_kv, head_dim, T, pos0, n_ctx, q, kc, vc, out) || pos0 + T > kPfAttnMaxKV) {
        set_err("llmi_pf_attention_x86: bad arguments");
        return -1;
    }
    API_TRY
    PfAttn at;
    at.num = NUMERICS_X86;
    return pf_attention_run("llmi_pf_attention_x86", at, n_head, n_head_kv, head_dim, T, pos0, n_ctx, q, kc, vc, out);
    API_CATCH(-5)
}

// The longest KV k_pf_a86 takes for this head shape (host only: no device call).
int32_t llmi_pf_attn_x86_max_kv(int32_t n_head, int32_t n_head_kv, int32_t head_dim) {
    if (!head_shape_ok(n_head, n_head_kv, head_dim)) {
        set_err("llmi_pf_attn_x86_max_kv: bad arguments");
        return -1;
    }
    return pf_attn_x86_max_kv(n_head, n_head_kv, head_dim);
}

double llmi_bench_attention(int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t n_kv, int32_t mode, int32_t reps,
                            uint64_t* trace_dev) {
    if (!head_shape_ok(n_head, n_head_kv, head_dim) || n_kv <= 0 || reps <= 0) {
        set_err("llmi_bench_attention: bad arguments");
        return -1.0;
    }
    API_TRY
    const int kv_bound = kv_bucket_bound(n_kv, INT32_MAX), n_ctx = kv_bound;
    const size_t kv_layer = (size_t)n_head_kv * n_ctx * head_dim;  // elements per layer, K or V
    const int nl = (int)std::max<size_t>(2, (size_t)(512u << 20) / (kv_layer * 4) + 1);
    DevPool P;
    uint16_t* kc = P.get<uint16_t>(kv_layer * nl * 2, false);
    uint16_t* vc = P.get<uint16_t>(kv_layer * nl * 2, false);
    float* q = P.get<float>((size_t)n_head * head_dim * 4);
    float* scores = P.get<float>(attn_scratch_floats(n_head, n_ctx) * 4);
    float* out = P.get<float>((size_t)n_head * head_dim * 4, false);
    StepState* st = dev_states(P, &n_kv, 1, 0);
    if (P.err != hipSuccess) { set_err("llmi_bench_attention: out of device memory"); return -1.0; }
    (void)hipMemset(kc, 0x3c, kv_layer * nl * 2);  // f16 0x3c3c ~ 1.06
    (void)hipMemset(vc, 0x3c, kv_layer * nl * 2);
    HipObjs h;
    (void)hipStreamCreateWithFlags(&h.s, hipStreamNonBlocking);
    const hipStream_t s = h.s;
    AttnArgs a;
    a.q = q; a.out = out; a.st = st; a.n_ctx = n_ctx; a.scale = 1.0f / sqrtf((float)head_dim);
    a.num = t_hook_numerics & NUMERICS_X86;
    attn_bind_scratch(a, scores, n_head, n_ctx);
    if (trace_dev) {  // one traced eager launch on a cold layer (LLMI_EXP_TRACE builds)
        for (int l = 0; l + 1 < nl; ++l) {
            a.kc = kc + (size_t)l * kv_layer;
            a.vc = vc + (size_t)l * kv_layer;
            a.layer = l % 255;
            (void)launch_attention(a, n_head, n_head_kv, head_dim, kv_bound, s, mode);
        }
        a.kc = kc + (size_t)(nl - 1) * kv_layer;
        a.vc = vc + (size_t)(nl - 1) * kv_layer;
        a.layer = (nl - 1) % 255;
        a.trace = (unsigned long long*)trace_dev;
        const bool okt = launch_attention(a, n_head, n_head_kv, head_dim, kv_bound, s, mode) == hipSuccess &&
                         hipStreamSynchronize(s) == hipSuccess;
        return okt ? 0.0 : -1.0;
    }
    std::string err;
    h.ex = capture_graph(s, [&](std::string&) {
        // a new step sequence number per replay: k_attn_x's hand-off tags never repeat
        bool ok = launch_state_tick(st, s) == hipSuccess;
        for (int l = 0; ok && l < nl; ++l) {
            a.kc = kc + (size_t)l * kv_layer;
            a.vc = vc + (size_t)l * kv_layer;
            a.layer = l % 255;
            ok = launch_attention(a, n_head, n_head_kv, head_dim, kv_bound, s, mode) == hipSuccess;
        }
        return ok;
    }, err);
    if (!h.ex) { set_err("llmi_bench_attention: capture/launch failed"); return -1.0; }
    return replay_us(h, reps, nl);
    API_CATCH(-1.0)
}

static_assert(LLMI_SAMPLE_MAX_TOP_K == kSampleMaxTopK && LLMI_SAMPLE_MAX_LAST_N == kSampleMaxLastN, "llmi.h limits");

// k_sample alone over crafted rows.  The rows' key slots start as a logits launch leaves
// them (the raw row's argmax key, here in slot 5), so a greedy row reads back its argmax
// and a sampled row shows that the kernel cleared the other slots.
int32_t llmi_sample_logits(const float* logits, int32_t n_rows, int32_t V, const int32_t* hist, int32_t n_hist,
                           const struct llmi_sampler_params* params, const double* uniforms, int32_t* token_out,
                           int32_t* cand_out, int32_t* n_cand_out, float* penalized_out, double* us_out) {
    const std::string who = "llmi_sample_logits: ";
    if (!logits || !params || !uniforms || !token_out || !cand_out || !n_cand_out || (n_hist > 0 && !hist)) {
        set_err(who + "bad arguments (null pointer)");
        return -1;
    }
    if (n_rows <= 0 || n_rows > kMaxBatch) { set_err(who + "bad arguments (n_rows 1..8)"); return -1; }
    if (V <= 0 || n_hist < 0) { set_err(who + "bad arguments (V, n_hist)"); return -1; }
    std::vector<SampleRec> recs((size_t)n_rows);
    for (int r = 0; r < n_rows; ++r) {
        const llmi_sampler_params& p = params[r];
        std::string why;
        if (!sample_rec_make(p.temperature, p.top_k, p.top_p, p.min_p, p.repeat_penalty, p.repeat_last_n, p.presence_penalty,
                             p.frequency_penalty, recs[(size_t)r], why)) {
            set_err(who + "params[" + std::to_string(r) + "]: " + why + " (the device sampler's limits)");
            return -1;
        }
    }
    API_TRY
    DevPool P;
    const size_t nv = (size_t)n_rows * V, nh = (size_t)n_rows * n_hist;
    float* d_lg = P.get<float>(nv * 4, false);
    int32_t* d_hist = P.get<int32_t>(nh * 4);
    double* d_uni = P.get<double>((size_t)n_rows * 8, false);
    SampleRec* d_rec = P.get<SampleRec>((size_t)n_rows * sizeof(SampleRec), false);
    int32_t* d_cand = P.get<int32_t>((size_t)n_rows * kSampleMaxTopK * 4);
    int32_t* d_nc = P.get<int32_t>((size_t)n_rows * 4);
    StepState* d_st = P.get<StepState>((size_t)n_rows * sizeof(StepState), false);
    if (P.err != hipSuccess) { set_err(who + "out of device memory"); return -2; }
    std::vector<StepState> hs((size_t)n_rows);
    const int pos = n_hist - 1;
    for (int r = 0; r < n_rows; ++r) {
        StepState& s = hs[(size_t)r];
        memset(&s, 0, sizeof s);
        s.pos = pos;
        s.pos_next = pos + 1;
        unsigned long long best = 0;
        for (int i = 0; i < V; ++i) {  // argmax_key (mv_device.h) on the host
            float v = logits[(size_t)r * V + i];
            if (v == 0.f) v = 0.f;
            uint32_t u;
            memcpy(&u, &v, 4);
            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
            const unsigned long long k = ((unsigned long long)u << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
            best = k > best ? k : best;
        }
        s.key[pos & 1][5] = best;
        recs[(size_t)r].uni = d_uni + r;
        recs[(size_t)r].pos0 = pos;
        recs[(size_t)r].n_uni = 1;
    }
    hipError_t e = hipMemcpy(d_lg, logits, nv * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && nh) e = hipMemcpy(d_hist, hist, nh * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_uni, uniforms, (size_t)n_rows * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_rec, recs.data(), (size_t)n_rows * sizeof(SampleRec), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_st, hs.data(), (size_t)n_rows * sizeof(StepState), hipMemcpyHostToDevice);
    SampleArgs a;
    a.logits = d_lg; a.V = V; a.st = d_st; a.hist = d_hist; a.hist_stride = (size_t)n_hist; a.rec = d_rec;
    a.cand = d_cand; a.n_cand = d_nc;
    HipObjs h;
    double us = 0.0;
    if (e == hipSuccess) e = time_launch(h, [&] { return launch_sample(a, n_rows, nullptr); }, us);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<float> rows(penalized_out ? nv : 0);
    if (e == hipSuccess) e = hipMemcpy(hs.data(), d_st, (size_t)n_rows * sizeof(StepState), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(cand_out, d_cand, (size_t)n_rows * kSampleMaxTopK * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(n_cand_out, d_nc, (size_t)n_rows * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && penalized_out) e = hipMemcpy(rows.data(), d_lg, nv * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { set_err(who + hip_err(e)); return -3; }
    for (int r = 0; r < n_rows; ++r) {
        token_out[r] = key_token(hs[(size_t)r].key[pos & 1]);
        for (int j = 0; penalized_out && j < n_hist; ++j) {
            const int32_t tok = hist[(size_t)r * n_hist + j];
            penalized_out[(size_t)r * n_hist + j] = tok >= 0 && tok < V ? rows[(size_t)r * V + tok] : 0.f;
        }
    }
    if (us_out) *us_out = us;
    return 0;
    API_CATCH(-5)
}

// The tail of a step with log-probabilities over crafted rows: k_logprob, k_sample,
// k_logprob_pick in step order.  Key slots as llmi_sample_logits sets them.
int32_t llmi_logprob_rows(const float* logits, int32_t n_rows, int32_t V, const int32_t* hist, int32_t n_hist,
                          const struct llmi_sampler_params* params, const double* uniforms, const int32_t* n_top,
                          int32_t* token_out, double* tok_logprob_out, double* lse_out, int32_t* top_id_out,
                          double* top_logprob_out, float* rows_out, double* us_out) {
    const std::string who = "llmi_logprob_rows: ";
    if (!logits || !params || !uniforms || !n_top || !token_out || !tok_logprob_out || !lse_out || !top_id_out ||
        !top_logprob_out || (n_hist > 0 && !hist)) {
        set_err(who + "bad arguments (null pointer)");
        return -1;
    }
    if (n_rows <= 0 || n_rows > kMaxBatch) { set_err(who + "bad arguments (n_rows 1..8)"); return -1; }
    if (V <= 0 || n_hist < 0) { set_err(who + "bad arguments (V, n_hist)"); return -1; }
    std::vector<SampleRec> recs((size_t)n_rows);
    for (int r = 0; r < n_rows; ++r) {
        const llmi_sampler_params& p = params[r];
        std::string why;
        if (!sample_rec_make(p.temperature, p.top_k, p.top_p, p.min_p, p.repeat_penalty, p.repeat_last_n, p.presence_penalty,
                             p.frequency_penalty, recs[(size_t)r], why)) {
            set_err(who + "params[" + std::to_string(r) + "]: " + why + " (the device sampler's limits)");
            return -1;
        }
        if (n_top[r] < -1 || n_top[r] > kLogprobMaxTop) {
            set_err(who + "n_top[" + std::to_string(r) + "] outside -1.." + std::to_string(kLogprobMaxTop));
            return -1;
        }
    }
    API_TRY
    DevPool P;
    const size_t nv = (size_t)n_rows * V, nh = (size_t)n_rows * n_hist, nr = (size_t)n_rows;
    float* d_lg = P.get<float>(nv * 4, false);
    int32_t* d_hist = P.get<int32_t>(nh * 4);
    double* d_uni = P.get<double>(nr * 8, false);
    SampleRec* d_rec = P.get<SampleRec>(nr * sizeof(SampleRec), false);
    LogprobRec* d_lrec = P.get<LogprobRec>(nr * sizeof(LogprobRec), false);
    StepState* d_st = P.get<StepState>(nr * sizeof(StepState), false);
    double* d_lse = P.get<double>(nr * 8);
    double* d_tok = P.get<double>(nr * 8);
    double* d_top = P.get<double>(nr * kLogprobMaxTop * 8);
    int32_t* d_top_id = P.get<int32_t>(nr * kLogprobMaxTop * 4);
    int32_t* d_wtok = P.get<int32_t>(nr * kSampleMaxLastN * 4);
    float* d_wraw = P.get<float>(nr * kSampleMaxLastN * 4);
    if (P.err != hipSuccess) { set_err(who + "out of device memory"); return -2; }
    std::vector<StepState> hs(nr);
    std::vector<LogprobRec> lrecs(nr);
    const int pos = n_hist - 1;
    for (int r = 0; r < n_rows; ++r) {
        StepState& s = hs[(size_t)r];
        memset(&s, 0, sizeof s);
        s.pos = pos;
        s.pos_next = pos + 1;
        unsigned long long best = 0;
        for (int i = 0; i < V; ++i) {  // argmax_key (mv_device.h) on the host
            float v = logits[(size_t)r * V + i];
            if (v == 0.f) v = 0.f;
            uint32_t u;
            memcpy(&u, &v, 4);
            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
            const unsigned long long k = ((unsigned long long)u << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
            best = k > best ? k : best;
        }
        s.key[pos & 1][5] = best;
        recs[(size_t)r].uni = d_uni + r;
        recs[(size_t)r].pos0 = pos;
        recs[(size_t)r].n_uni = 1;
        LogprobRec& l = lrecs[(size_t)r];
        l.n_top = n_top[r]; l.pos0 = pos; l.n_step = 1;
        l.lse = d_lse + r; l.tok_lp = d_tok + r;
        l.top_lp = d_top + (size_t)r * kLogprobMaxTop; l.top_id = d_top_id + (size_t)r * kLogprobMaxTop;
        l.win_tok = d_wtok + (size_t)r * kSampleMaxLastN; l.win_raw = d_wraw + (size_t)r * kSampleMaxLastN;
    }
    hipError_t e = hipMemcpy(d_lg, logits, nv * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && nh) e = hipMemcpy(d_hist, hist, nh * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_uni, uniforms, nr * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_rec, recs.data(), nr * sizeof(SampleRec), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_lrec, lrecs.data(), nr * sizeof(LogprobRec), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_st, hs.data(), nr * sizeof(StepState), hipMemcpyHostToDevice);
    SampleArgs a;
    a.logits = d_lg; a.V = V; a.st = d_st; a.hist = d_hist; a.hist_stride = (size_t)n_hist; a.rec = d_rec;
    LogprobArgs la;
    la.logits = d_lg; la.V = V; la.st = d_st; la.hist = d_hist; la.hist_stride = (size_t)n_hist; la.rec = d_rec;
    la.lrec = d_lrec;
    HipObjs h;
    double us[3] = {0.0, 0.0, 0.0};
    if (e == hipSuccess) e = time_launch(h, [&] { return launch_logprob(la, n_rows, nullptr); }, us[0]);
    if (e == hipSuccess) e = time_launch(h, [&] { return launch_sample(a, n_rows, nullptr); }, us[1]);
    if (e == hipSuccess) e = time_launch(h, [&] { return launch_logprob_pick(la, n_rows, nullptr); }, us[2]);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<double> lse(nr), tok(nr), top(nr * kLogprobMaxTop);
    std::vector<int32_t> top_id(nr * kLogprobMaxTop);
    if (e == hipSuccess) e = hipMemcpy(hs.data(), d_st, nr * sizeof(StepState), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(lse.data(), d_lse, nr * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(tok.data(), d_tok, nr * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(top.data(), d_top, nr * kLogprobMaxTop * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(top_id.data(), d_top_id, nr * kLogprobMaxTop * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && rows_out) e = hipMemcpy(rows_out, d_lg, nv * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { set_err(who + hip_err(e)); return -3; }
    for (int r = 0; r < n_rows; ++r) {
        token_out[r] = key_token(hs[(size_t)r].key[pos & 1]);
        if (n_top[r] < 0) continue;
        lse_out[r] = lse[(size_t)r];
        tok_logprob_out[r] = tok[(size_t)r];
        for (int i = 0; i < kLogprobMaxTop; ++i) {
            top_id_out[r * kLogprobMaxTop + i] = top_id[(size_t)r * kLogprobMaxTop + i];
            top_logprob_out[r * kLogprobMaxTop + i] = top[(size_t)r * kLogprobMaxTop + i];
        }
    }
    if (us_out) for (int i = 0; i < 3; ++i) us_out[i] = us[i];
    return 0;
    API_CATCH(-5)
}

// Experiment hook (LLMI_EXP_TRACE builds): one STORE matvec launch with per-wave
// s_memrealtime stamps {entry, after prologue, first pair done, exit, HW_ID, XCC<<32|pairs}
// written to trace_dev[grid*waves*6]; returns the grid size, < 0 on error.
int32_t llmi_trace_matvec(int32_t type, const void* w, int64_t rows, int64_t cols, const float* x, float* y, int32_t mode,
                          uint64_t* trace_dev) {
    API_TRY
    const int mb = hook_grid_cap();
    MVArgs a;
    a.nseg = 1; a.cols = (int)cols; a.npairs = (int)((rows + 1) / 2); a.x = x; a.y = y;
    a.seg[0] = seg_at(type, w, rows, cols);
    a.trace = (unsigned long long*)trace_dev;
    if (mode & 256) a.xfirst = -1;  // mode bit 8: weights issued before the activation arrives
    DevPool P;
    if (mode & 8) a.xq = P.get<uint8_t>((size_t)(cols / 256) * 304);  // mode bit 3: pre-quantized activation image (zeros)
    const bool ok = launch_matvec(a, EPI_STORE, mb, nullptr) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        set_err("llmi_trace_matvec: launch failed");
        return -1;
    }
    return std::min(mb, (a.npairs + kMVWaves - 1) / kMVWaves);
    API_CATCH(-1)
}
