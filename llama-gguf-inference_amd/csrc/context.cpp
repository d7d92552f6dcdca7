// context.cpp — the decode context: KV cache (upstream's f16 cache),
// scratch and RoPE table, the kernel-class profiler, the sampler and logprob records of a
// generate call, and the embeddings pooling.  Every block is allocated through c.pool.
#include "engine_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace llmi {

std::string hip_err(hipError_t e) { return std::string(hipGetErrorString(e)); }

int wg_per_cu() {  // read per call (context creation): tests vary it within a process
    const char* e = getenv("LLMI_WG_PER_CU");
    const int n = e ? atoi(e) : 0;
    return n > 0 ? n : 2;
}

int mv_grid_cap(int device) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return 0;
    return std::max(64, cus * wg_per_cu());
}

hipGraphExec_t capture_graph(hipStream_t s, const std::function<bool(std::string&)>& enqueue, std::string& err) {
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { err = "hipStreamBeginCapture: " + hip_err(e); return nullptr; }
    std::string e2;
    const bool ok = enqueue(e2);
    hipGraph_t g = nullptr;
    hipGraphExec_t ex = nullptr;
    e = hipStreamEndCapture(s, &g);
    if (!ok) err = "capture: " + e2;
    else if (e != hipSuccess) err = "hipStreamEndCapture: " + hip_err(e);
    else if ((e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0)) != hipSuccess) {
        err = "hipGraphInstantiate: " + hip_err(e);
        ex = nullptr;
    }
    if (g) (void)hipGraphDestroy(g);
    return ex;
}

Context::~Context() {
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (m) (void)hipSetDevice(device);
    graphs.destroy();
    pool.free_all();  // here, not in the member's destructor: that runs after the caller's device is restored
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
    (void)hipSetDevice(cur);
}

bool context_init(Model* m, int n_ctx, bool use_graphs, int n_seq, Context& c, std::string& err) {
    const HParams& hp = m->hp;
    c.m = m;
    c.device = m->device;
    c.n_ctx = n_ctx > 0 ? n_ctx : std::min(hp.n_ctx_train > 0 ? hp.n_ctx_train : 4096, 4096);
    // padded like upstream llama.cpp's KV cache (multiple of 256): the attention kernels
    // read V rows in 16-B (8-position) pieces and K in 64-position tiles
    c.n_ctx = (c.n_ctx + 255) / 256 * 256;
    {
        const char* e = getenv("LLMI_ATTN_MODE");
        set_attn_mode(e ? atoi(e) : 0);
    }
    c.use_graphs = use_graphs;
    HIPC(hipSetDevice(m->device));
    if (!(c.max_blocks = mv_grid_cap(m->device))) { err = "device query failed"; return false; }
    HIPC(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    HIPC(hipEventCreate(&c.ev0));
    HIPC(hipEventCreate(&c.ev1));
    const size_t E = (size_t)hp.n_embd, QD = (size_t)hp.n_head * hp.head_dim;
    const size_t kv_elems = (size_t)hp.n_layer * hp.n_head_kv * (size_t)c.n_ctx * hp.head_dim;
    HIPC(c.pool.alloc(c.x, E * 4));
    HIPC(c.pool.alloc(c.q, QD * 4));
    HIPC(c.pool.alloc(c.att, QD * 4));
    HIPC(c.pool.alloc(c.h, (size_t)hp.n_ff * 4));
    HIPC(c.pool.alloc(c.logits, (size_t)hp.n_vocab * 4));
    HIPC(c.pool.alloc(c.scores, attn_scratch_floats(hp.n_head, c.n_ctx) * 4));
    {
        AttnArgs a;
        attn_bind_scratch(a, c.scores, hp.n_head, c.n_ctx);
        c.fault_dev = a.fault;
    }
    HIPC(c.pool.alloc_pinned(c.fault_host, 16));
    HIPC(c.pool.alloc(c.le_cnt, le_counter_bytes(hp.n_layer)));
    *c.fault_host = 0;
    if (n_seq < 1 || n_seq > 64) { err = "n_seq_max must be in [1, 64]"; return false; }
    c.n_seq = n_seq;
    c.kv_seq_elems = kv_elems;
    const int nalloc = n_seq > 1 ? n_seq + 1 : 1;  // + the dummy sequence of padded batch slots
    HIPC(c.pool.alloc(c.kc0, kv_elems * 2 * nalloc));
    HIPC(c.pool.alloc(c.vc0, kv_elems * 2 * nalloc));
    HIPC(c.pool.alloc(c.st0, sizeof(StepState) * nalloc));
    HIPC(c.pool.alloc(c.hist0, (size_t)c.n_ctx * 4 * nalloc));
    c.seq_past.assign((size_t)n_seq, 0);
    c.kc = c.kc0; c.vc = c.vc0; c.st = c.st0; c.hist = c.hist0; c.cur_seq = 0;
    // RoPE table [pos][n_rot/2][cos,sin]: ggml_rope_cache_init's iterative theta, computed
    // on the host with libm cosf/sinf exactly as the CPU path does
    const int half = hp.n_rot / 2;
    std::vector<float> tab((size_t)c.n_ctx * half * 2);
    const float theta_scale = powf(hp.rope_base, -2.0f / (float)hp.n_rot);
    for (int p = 0; p < c.n_ctx; ++p) {
        float theta = (float)p;
        for (int i = 0; i < half; ++i) {
            const float ff = m->has_rope_freqs ? m->rope_freq_host[(size_t)i] : 1.0f;
            const float th = 1.0f * (theta / ff);
            tab[((size_t)p * half + i) * 2 + 0] = cosf(th) * 1.0f;
            tab[((size_t)p * half + i) * 2 + 1] = sinf(th) * 1.0f;
            theta *= theta_scale;
        }
    }
    HIPC(c.pool.alloc(c.rope, tab.size() * 4));
    HIPC(hipMemcpy(c.rope, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    context_clear(c);
    HIPC(hipStreamSynchronize(c.stream));
    return true;
}

void context_select_seq(Context& c, int s) {
    if (s < 0 || s >= std::max(1, c.n_seq + (c.n_seq > 1 ? 1 : 0))) return;
    if (s != c.cur_seq && c.cur_seq < (int)c.seq_past.size()) c.seq_past[(size_t)c.cur_seq] = c.n_past;
    c.cur_seq = s;
    c.kc = c.kc0 + (size_t)s * c.kv_seq_elems;
    c.vc = c.vc0 + (size_t)s * c.kv_seq_elems;
    c.st = c.st0 + s;
    c.hist = c.hist0 + (size_t)s * c.n_ctx;
    if (s < (int)c.seq_past.size()) c.n_past = c.seq_past[(size_t)s];
}

// a sequence's state before its first step: no token fed from the host
static StepState fresh_step_state() {
    StepState s{};
    s.token_in = -1;
    s.token_in_pos = -1;
    return s;
}

void context_clear_seq(Context& c, int s) {
    (void)hipSetDevice(c.device);
    (void)hipMemsetAsync(c.kc0 + (size_t)s * c.kv_seq_elems, 0, c.kv_seq_elems * 2, c.stream);
    (void)hipMemsetAsync(c.vc0 + (size_t)s * c.kv_seq_elems, 0, c.kv_seq_elems * 2, c.stream);
    (void)hipMemsetAsync(c.hist0 + (size_t)s * c.n_ctx, 0, (size_t)c.n_ctx * 4, c.stream);
    const StepState s0 = fresh_step_state();
    (void)hipMemcpyAsync(c.st0 + s, &s0, sizeof s0, hipMemcpyHostToDevice, c.stream);
    (void)hipStreamSynchronize(c.stream);
    if (s < (int)c.seq_past.size()) c.seq_past[(size_t)s] = 0;
    if (s == c.cur_seq) c.n_past = 0;
}

void context_clear(Context& c) {
    const HParams& hp = c.m->hp;
    const int nalloc = c.n_seq > 1 ? c.n_seq + 1 : 1;
    const size_t kv_elems = (size_t)hp.n_layer * hp.n_head_kv * (size_t)c.n_ctx * hp.head_dim * nalloc;
    (void)hipSetDevice(c.m->device);
    (void)hipMemsetAsync(c.kc0, 0, kv_elems * 2, c.stream);
    (void)hipMemsetAsync(c.vc0, 0, kv_elems * 2, c.stream);
    (void)hipMemsetAsync(c.hist0, 0, (size_t)c.n_ctx * 4 * nalloc, c.stream);
    const StepState s0 = fresh_step_state();
    for (int s = 0; s < nalloc; ++s) (void)hipMemcpyAsync(c.st0 + s, &s0, sizeof s0, hipMemcpyHostToDevice, c.stream);
    std::fill(c.seq_past.begin(), c.seq_past.end(), 0);
    // attention scratch incl. k_attn_x's granules: the step sequence restarts at 0 below,
    // so no granule of an earlier sequence may keep a tag the new one will use
    (void)hipMemsetAsync(c.scores, 0, attn_scratch_floats(hp.n_head, c.n_ctx) * 4, c.stream);
    (void)hipStreamSynchronize(c.stream);
    c.n_past = 0;
}

void context_fault_readback(Context& c) {
    (void)hipMemcpyAsync(c.fault_host, c.fault_dev, 4, hipMemcpyDeviceToHost, c.stream);
}

bool context_fault_ok(Context& c, std::string& err) {
    if (*c.fault_host == 0) return true;
    err = "an in-kernel bounded wait gave up (device fault word " + std::to_string(*c.fault_host) +
          ": bit 0 attention hand-off, 0x100.. layer engine ring / edge / barrier / ring space); this call's "
          "outputs are invalid";
    *c.fault_host = 0;
    (void)hipMemsetAsync(c.fault_dev, 0, 4, c.stream);
    (void)hipStreamSynchronize(c.stream);
    return false;
}

bool Prof::arm(int k) {
    if (!timed) return true;
    while (ev.size() < 2 * (used + 1)) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return false;
        ev.push_back(e);
    }
    if (ev_cls.size() < used + 1) ev_cls.resize(used + 1);
    ev_cls[used] = k;
    set_launch_events(ev[2 * used], ev[2 * used + 1]);
    ++used;
    return true;
}
void Prof::disarm() { set_launch_events(nullptr, nullptr); }
double Prof::elapsed_us(int k, int* n) const {
    double t = 0;
    int cnt = 0;
    for (size_t i = 0; i < used; ++i) {
        if (ev_cls[i] != k) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) == hipSuccess) { t += ms * 1e3; ++cnt; }
    }
    if (n) *n = cnt;
    return t;
}
Prof::~Prof() {
    disarm();
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
}

bool sample_prepare(Context& c, int n, const SampleRec* recs, const int* pos0, const double* uniforms, int n_gen,
                    std::string& err) {
    if (!c.srec) HIPC(c.pool.alloc(c.srec, sizeof(SampleRec) * kMaxBatch));
    // the records carry the buffer's address: no graph holds it
    HIPC(c.pool.grow({{&c.suni, sizeof(double) * kMaxBatch}}, c.suni_cap, n_gen, std::max(64, n_gen), c.stream));
    c.srec_host.assign((size_t)kMaxBatch, SampleRec());
    c.suni_host.assign(uniforms, uniforms + (size_t)n * n_gen);
    for (int k = 0; k < n; ++k) {
        SampleRec& r = c.srec_host[(size_t)k];
        r = recs[k];
        r.uni = c.suni + (size_t)k * n_gen;
        r.pos0 = pos0[k];
        r.n_uni = n_gen;
    }
    HIPC(hipMemcpyAsync(c.suni, c.suni_host.data(), sizeof(double) * n * n_gen, hipMemcpyHostToDevice, c.stream));
    HIPC(hipMemcpyAsync(c.srec, c.srec_host.data(), sizeof(SampleRec) * kMaxBatch, hipMemcpyHostToDevice, c.stream));
    return true;
}

bool logprob_prepare(Context& c, int n, const int32_t* n_top, const int* pos0, int n_gen, std::string& err) {
    if (!c.lrec) {
        HIPC(c.pool.alloc(c.lrec, sizeof(LogprobRec) * kMaxBatch));
        HIPC(c.pool.alloc(c.lp_win_tok, sizeof(int32_t) * kMaxBatch * kSampleMaxLastN));
        HIPC(c.pool.alloc(c.lp_win_raw, sizeof(float) * kMaxBatch * kSampleMaxLastN));
    }
    // the records carry the rings' addresses: no graph holds them
    HIPC(c.pool.grow({{&c.lp_lse, sizeof(double) * kMaxBatch},
                      {&c.lp_tok, sizeof(double) * kMaxBatch},
                      {&c.lp_top, sizeof(double) * kMaxBatch * kLogprobMaxTop},
                      {&c.lp_top_id, sizeof(int32_t) * kMaxBatch * kLogprobMaxTop}},
                     c.lp_cap, n_gen, std::max(64, n_gen), c.stream));
    c.lrec_host.assign((size_t)kMaxBatch, LogprobRec());
    for (int k = 0; k < n; ++k) {
        LogprobRec& r = c.lrec_host[(size_t)k];
        const size_t at = (size_t)k * c.lp_cap;
        r.n_top = n_top[k];
        r.pos0 = pos0[k];
        r.n_step = n_gen;
        r.lse = c.lp_lse + at;
        r.tok_lp = c.lp_tok + at;
        r.top_lp = c.lp_top + at * kLogprobMaxTop;
        r.top_id = c.lp_top_id + at * kLogprobMaxTop;
        r.win_tok = c.lp_win_tok + (size_t)k * kSampleMaxLastN;
        r.win_raw = c.lp_win_raw + (size_t)k * kSampleMaxLastN;
    }
    HIPC(hipMemcpyAsync(c.lrec, c.lrec_host.data(), sizeof(LogprobRec) * kMaxBatch, hipMemcpyHostToDevice, c.stream));
    return true;
}

void logprob_readback(Context& c, int k, int n_gen, double* tok_lp, int32_t* top_id, double* top_lp) {
    const size_t at = (size_t)k * c.lp_cap, n = (size_t)n_gen;
    (void)hipMemcpyAsync(tok_lp, c.lp_tok + at, n * 8, hipMemcpyDeviceToHost, c.stream);
    (void)hipMemcpyAsync(top_id, c.lp_top_id + at * kLogprobMaxTop, n * kLogprobMaxTop * 4, hipMemcpyDeviceToHost, c.stream);
    (void)hipMemcpyAsync(top_lp, c.lp_top + at * kLogprobMaxTop, n * kLogprobMaxTop * 8, hipMemcpyDeviceToHost, c.stream);
}

// ---------------------------------------------------------------------------------
// Embeddings (embd.hip): result_norm + pooling of the sequence llama_decode is running.
// ---------------------------------------------------------------------------------
bool embd_alloc(Context& c, int rows, std::string& err) {
    const size_t E = (size_t)c.m->hp.n_embd;
    if (!c.embd_acc) HIPC(c.pool.alloc(c.embd_acc, E * sizeof(double)));
    if (!c.embd_scale) HIPC(c.pool.alloc(c.embd_scale, (size_t)kEmbdMaxChunk * sizeof(float)));
    HIPC(c.pool.grow({{&c.embd_out, E * sizeof(float)}}, c.embd_cap, rows, rows));
    return true;
}

void embd_begin(Context& c, int n_total, float* dst) {
    c.embd_total = n_total;
    c.embd_done = 0;
    c.embd_dst = dst;
}

bool embd_pool_enqueue(Context& c, const float* x, int64_t ldx, int n_tok, std::string& err) {
    const HParams& hp = c.m->hp;
    for (int b0 = 0; b0 < n_tok; b0 += kEmbdMaxChunk) {
        EmbdPoolArgs a;
        a.x = x + (size_t)b0 * ldx; a.ldx = ldx; a.n_tok = std::min(kEmbdMaxChunk, n_tok - b0); a.n_embd = hp.n_embd;
        a.w = (const float*)(c.m->arena + c.m->out_norm.off_a); a.eps = hp.eps;
        a.pooling = c.pooling; a.n_total = c.embd_total; a.t0 = c.embd_done;
        a.acc = c.embd_acc; a.scale = c.embd_scale;
        a.out = c.pooling == POOLING_NONE ? c.embd_dst + (size_t)c.embd_done * hp.n_embd : c.embd_dst;
        std::string why;
        if (!embd_pool_ok(a, why)) { err = "embeddings: " + why; return false; }
        const hipError_t e = launch_embd_pool(a, c.stream);
        if (e != hipSuccess) { err = "launch_embd_pool: " + hip_err(e); return false; }
        c.embd_done += a.n_tok;
    }
    return true;
}

}  // namespace llmi
