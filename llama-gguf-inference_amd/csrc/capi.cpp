// capi.cpp — extern "C" drop-in surface (include/llmi.h).  Each function restates
// the upstream llama.h entry point of the same name; no C++ exception
// crosses this boundary, errors go to the thread-local llmi_last_error().
// (The vocab / tokenizer entry points: capi_host.cpp; the replica fan-out:
// capi_fanout.cpp; the test and microbenchmark hooks: capi_hooks.cpp.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/llmi.h"
#include "capi_internal.h"

using namespace llmi;

namespace {
bool ensure_outs(llama_context* ctx, int n) {
    DevPool& pool = ctx->c.pool;  // the context's: freed with it, inside its device scope
    const size_t V = (size_t)ctx->c.m->hp.n_vocab;
    if (pool.grow({{&ctx->outs, V * 4}}, ctx->outs_cap, n, n) != hipSuccess) { set_err("hipMalloc logits outputs"); return false; }
    if (pool.grow({{&ctx->keys_pinned, 8 * kArgSlots, true}}, ctx->keys_cap, n, n) != hipSuccess) {
        set_err("hipHostMalloc");
        return false;
    }
    return true;
}

int seq_past_of(const Context& c, int s) { return s == c.cur_seq ? c.n_past : c.seq_past[(size_t)s]; }
void set_seq_past(Context& c, int s, int v) {
    if (s == c.cur_seq) c.n_past = v;
    else c.seq_past[(size_t)s] = v;
}

// where llmi_generate_logprobs_batch wants its results: n_top per sequence (-1: nothing for it)
struct LogprobOut {
    const int32_t* n_top;
    double* tok_lp;   // [n][n_gen]
    int32_t* top_id;  // [n][n_gen][kLogprobMaxTop]
    double* top_lp;
};
void logprob_readback_seq(Context& c, const LogprobOut& lp, int k, int n_gen) {
    if (lp.n_top[k] < 0) return;  // its entries stay as the caller left them
    const size_t at = (size_t)k * n_gen;
    logprob_readback(c, k, n_gen, lp.tok_lp + at, lp.top_id + at * kLogprobMaxTop, lp.top_lp + at * kLogprobMaxTop);
}

// the end of a generate call, its read-backs enqueued: the sync, the fault check and the
// call's time and bytes; 0, or the call's error code with the error set
int32_t generate_finish(Context& c, const std::string& who, double bytes) {
    context_fault_readback(c);
    hipError_t e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) { set_err(who + hip_err(e)); return -4; }
    std::string err;
    if (!context_fault_ok(c, err)) { set_err(who + err); return -6; }
    float ms = 0.f;
    hipEventElapsedTime(&ms, c.ev0, c.ev1);
    c.last_us = ms * 1e3;
    c.last_bytes = bytes;
    c.n_outputs = 0;
    return 0;
}

// llmi_generate_greedy's body; sampled: the steps end with k_sample (the caller has uploaded
// the records and uniforms, sample_prepare); lp: and with the logprob kernels around it
// (logprob_prepare), slot 0's results read back with the tokens
int32_t generate_one(const char* name, llama_context* ctx, llama_token first, int32_t pos0, int32_t n_gen, llama_token* out,
                     bool sampled, const LogprobOut* lp = nullptr) {
    const std::string who = std::string(name) + ": ";
    if (!ctx || !out || n_gen <= 0) { set_err(who + "bad arguments"); return -1; }
    Context& c = ctx->c;
    const HParams& hp = c.m->hp;
    if (first < 0 || first >= hp.n_vocab) { set_err(who + "token out of range"); return -1; }
    if (pos0 < 0 || pos0 + n_gen > c.n_ctx) { set_err(who + "exceeds n_ctx"); return 1; }
    (void)hipSetDevice(c.m->device);
    (void)hipGetLastError();
    std::string err;
    double bytes = 0;
    if (launch_state_set(c.st, first, pos0, c.stream) != hipSuccess) { set_err("state set failed"); return -3; }
    hipEventRecord(c.ev0, c.stream);
    for (int k = 0; k < n_gen; ++k) {
        if (!step_run(c, pos0 + k, err, lp ? STEP_LOGPROBS : sampled ? STEP_SAMPLED : STEP_GREEDY)) {
            if (sampled) (void)hipStreamSynchronize(c.stream);  // sample_prepare's copies read the context's host vectors
            set_err(who + err);
            return -3;
        }
        bytes += bytes_per_token(*c.m, pos0 + k + 1);
    }
    hipEventRecord(c.ev1, c.stream);
    std::vector<int32_t> h((size_t)n_gen);
    unsigned long long keys[kArgSlots];
    if (n_gen > 1)
        (void)hipMemcpyAsync(h.data(), c.hist + pos0 + 1, (size_t)(n_gen - 1) * 4, hipMemcpyDeviceToHost, c.stream);
    (void)hipMemcpyAsync(keys, &c.st->key[(pos0 + n_gen - 1) & 1][0], sizeof(keys), hipMemcpyDeviceToHost, c.stream);
    if (lp) logprob_readback_seq(c, *lp, 0, n_gen);
    if (const int32_t rc = generate_finish(c, who, bytes)) return rc;
    for (int k = 0; k + 1 < n_gen; ++k) out[k] = h[(size_t)k];
    out[n_gen - 1] = (llama_token)key_token(keys);
    c.n_past = pos0 + n_gen;
    return n_gen;
}

// llmi_generate_greedy_batch's body; recs (n records) and uniforms (n x n_gen) non-null: the
// sampled call, every step ending with k_sample; lp non-null as well: the call with logprobs
int32_t generate_batch(const char* name, llama_context* ctx, int32_t n, const int32_t* seqs, const llama_token* first,
                       const int32_t* pos0, int32_t n_gen, llama_token* out, const SampleRec* recs, const double* uniforms,
                       const LogprobOut* lp = nullptr) {
    const std::string who = std::string(name) + ": ";
    const bool sampled = recs != nullptr;
    if (!ctx || n <= 0 || n > kMaxBatch || !seqs || !first || !pos0 || !out || n_gen <= 0) {
        set_err(who + "bad arguments (1..8 sequences)");
        return -1;
    }
    Context& c = ctx->c;
    const HParams& hp = c.m->hp;
    for (int k = 0; k < n; ++k) {
        if (seqs[k] < 0 || seqs[k] >= c.n_seq) { set_err(who + "seq out of range (n_seq_max)"); return -1; }
        for (int j = 0; j < k; ++j)
            if (seqs[j] == seqs[k]) { set_err(who + "repeated sequence"); return -1; }
        if (first[k] < 0 || first[k] >= hp.n_vocab) { set_err(who + "token out of range"); return -1; }
        if (pos0[k] < 0 || pos0[k] + n_gen > c.n_ctx) { set_err(who + "exceeds n_ctx"); return 1; }
    }
    (void)hipSetDevice(c.m->device);
    (void)hipGetLastError();
    std::string err;
    if (sampled && !sample_prepare(c, n, recs, pos0, uniforms, n_gen, err)) { set_err(who + err); return -3; }
    if (lp && !logprob_prepare(c, n, lp->n_top, pos0, n_gen, err)) {
        (void)hipStreamSynchronize(c.stream);
        set_err(who + err);
        return -3;
    }
    if (n == 1) {  // one sequence: the single-sequence step (k_matvec path, its own graphs)
        context_select_seq(c, seqs[0]);
        return generate_one(name, ctx, first[0], pos0[0], n_gen, out, sampled, lp);
    }
    double bytes = 0;
    for (int k = 0; k < n; ++k)
        if (launch_state_set(c.st0 + seqs[k], first[k], pos0[k], c.stream) != hipSuccess) {
            if (sampled) (void)hipStreamSynchronize(c.stream);
            set_err("state set failed");
            return -3;
        }
    hipEventRecord(c.ev0, c.stream);
    for (int j = 0; j < n_gen; ++j) {
        int max_pos = 0;
        for (int k = 0; k < n; ++k) {
            max_pos = std::max(max_pos, pos0[k] + j);
            bytes += bytes_per_token(*c.m, pos0[k] + j + 1) / n;
        }
        if (!bstep_run(c, n, seqs, max_pos, err, lp ? STEP_LOGPROBS : sampled ? STEP_SAMPLED : STEP_GREEDY)) {
            // (a model without a batched step ends here; the caller may call again at once, and
            // sample_prepare's pending copies still read the context's host vectors)
            if (sampled) (void)hipStreamSynchronize(c.stream);
            set_err(who + err);
            return -3;
        }
    }
    hipEventRecord(c.ev1, c.stream);
    std::vector<int32_t> h((size_t)n * n_gen);
    std::vector<unsigned long long> keys((size_t)n * kArgSlots);
    for (int k = 0; k < n; ++k) {
        const int32_t* hist = c.hist0 + (size_t)seqs[k] * c.n_ctx;
        if (n_gen > 1)
            (void)hipMemcpyAsync(h.data() + (size_t)k * n_gen, hist + pos0[k] + 1, (size_t)(n_gen - 1) * 4, hipMemcpyDeviceToHost,
                                 c.stream);
        (void)hipMemcpyAsync(keys.data() + (size_t)k * kArgSlots, &c.st0[seqs[k]].key[(pos0[k] + n_gen - 1) & 1][0],
                             8 * kArgSlots, hipMemcpyDeviceToHost, c.stream);
        if (lp) logprob_readback_seq(c, *lp, k, n_gen);
    }
    if (const int32_t rc = generate_finish(c, who, bytes)) return rc;
    for (int k = 0; k < n; ++k) {
        for (int j = 0; j + 1 < n_gen; ++j) out[(size_t)k * n_gen + j] = h[(size_t)k * n_gen + j];
        out[(size_t)k * n_gen + n_gen - 1] = (llama_token)key_token(keys.data() + (size_t)k * kArgSlots);
        set_seq_past(c, seqs[k], pos0[k] + n_gen);
    }
    return n_gen;
}
}  // namespace

extern "C" {

int32_t llmi_model_numerics(const struct llama_model* model) {
    return model ? model->m.numerics | (model->m.fa ? NUMERICS_FA : 0) : -1;
}

void llama_backend_init(void) { (void)hipInit(0); }
void llama_backend_free(void) {}

struct llama_model_params llama_model_default_params(void) {
    struct llama_model_params p;
    p.n_gpu_layers = 999;
    p.main_gpu = 0;
    p.vocab_only = false;
    p.use_mmap = true;
    p.no_upload = false;
    p.numerics = LLMI_NUMERICS_GENERIC;
    return p;
}

struct llama_context_params llama_context_default_params(void) {
    struct llama_context_params p;
    p.n_ctx = 4096;
    p.n_batch = 2048;
    p.n_ubatch = 512;
    p.n_seq_max = 1;
    p.n_threads = 0;
    p.use_graphs = true;
    return p;
}

int32_t llmi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

struct llama_model* llama_model_load_from_file(const char* path, struct llama_model_params params) {
    API_TRY
    if (!path) { set_err("null path"); return nullptr; }
    if (params.n_gpu_layers == 0 && !params.vocab_only) {
        set_err("n_gpu_layers=0 requests the CPU path; llmi is GPU-only (the NGL=0 path is the reference's "
                "llama.cpp CPU server, Dockerfile.cpu:84-89)");
        return nullptr;
    }
    if (!params.vocab_only) {
        const int n = llmi_device_count();
        if (n <= 0) { set_err("no HIP device visible"); return nullptr; }
        if (params.main_gpu < 0 || params.main_gpu >= n) { set_err("main_gpu out of range"); return nullptr; }
    }
    std::string err;
    llama_model* m = make_model([&](Model& M) {
        return model_load(path, params.main_gpu, params.vocab_only, params.no_upload, M, err, nullptr, params.numerics);
    });
    if (!m) set_err(err);
    return m;
    API_CATCH(nullptr)
}

void llama_model_free(struct llama_model* model) { delete model; }

struct llama_context* llama_init_from_model(struct llama_model* model, struct llama_context_params params) {
    API_TRY
    if (!model || !model->m.arena) { set_err("model has no device weights"); return nullptr; }
    auto* ctx = new llama_context();
    ctx->owner = model;
    std::string err;
    if (!context_init(&model->m, (int)params.n_ctx, params.use_graphs, (int)std::max<uint32_t>(1u, params.n_seq_max), ctx->c, err)) {
        set_err(err);
        delete ctx;
        return nullptr;
    }
    // upstream's default pooling: the model's own (GGUF <arch>.pooling_type) if it is one llmi runs
    const int mp = model->m.hp.pooling_type;
    ctx->c.pooling = mp >= POOLING_NONE && mp <= POOLING_LAST ? mp : POOLING_NONE;
    return ctx;
    API_CATCH(nullptr)
}

void llama_free(struct llama_context* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->c.device);  // never reads the model: it may be freed already
    delete ctx;  // outs and keys_pinned are the context pool's
}

struct llama_batch llama_batch_get_one(llama_token* tokens, int32_t n_tokens) {
    struct llama_batch b;
    std::memset(&b, 0, sizeof b);
    b.n_tokens = n_tokens;
    b.token = tokens;
    return b;
}

struct llama_batch llama_batch_init(int32_t n_tokens, int32_t embd, int32_t n_seq_max) {
    struct llama_batch b;
    std::memset(&b, 0, sizeof b);
    if (n_tokens <= 0) return b;
    if (embd) b.embd = (float*)calloc((size_t)n_tokens * embd, sizeof(float));
    else b.token = (llama_token*)calloc((size_t)n_tokens, sizeof(llama_token));
    b.pos = (llama_pos*)calloc((size_t)n_tokens, sizeof(llama_pos));
    b.n_seq_id = (int32_t*)calloc((size_t)n_tokens, sizeof(int32_t));
    b.seq_id = (llama_seq_id**)calloc((size_t)n_tokens + 1, sizeof(llama_seq_id*));
    for (int i = 0; i < n_tokens; ++i) b.seq_id[i] = (llama_seq_id*)calloc((size_t)std::max(1, n_seq_max), sizeof(llama_seq_id));
    b.logits = (int8_t*)calloc((size_t)n_tokens, 1);
    return b;
}

void llama_batch_free(struct llama_batch b) {
    free(b.token);
    free(b.embd);
    free(b.pos);
    free(b.n_seq_id);
    if (b.seq_id) {
        for (int i = 0; b.seq_id[i]; ++i) free(b.seq_id[i]);
        free(b.seq_id);
    }
    free(b.logits);
}

// shortest prompt run taken by the batched prefill path (shorter runs: decode steps)
static constexpr int kPrefillMin = 2;

static void copy_out(llama_context* ctx, int r, const float* logits_dev, const StepState* st, int pos) {
    Context& c = ctx->c;
    const size_t V = (size_t)c.m->hp.n_vocab;
    (void)hipMemcpyAsync(ctx->outs + (size_t)r * V * 4, logits_dev, V * 4, hipMemcpyDeviceToDevice, c.stream);
    (void)hipMemcpyAsync(ctx->keys_pinned + (size_t)r * kArgSlots, &st->key[pos & 1][0], 8 * kArgSlots, hipMemcpyDeviceToHost,
                         c.stream);
}

// One sequence's tokens (batch indices idx, positions pos) through the single-sequence
// path: the batched prefill of the leading run of consecutive, logit-less tokens (leaving
// at least the last token to a decode step), then decode steps.
// LLMI_NO_PREFILL=1 runs every token as a decode step (and so does a flash-attention
// numerics model without LLMI_FA_PREFILL=1: prefill_supported).
// embd_dst non-null (embeddings mode): the sequence's final hidden states are pooled as they
// appear, each prefill chunk inside prefill_enqueue and each decode step here.
static bool run_seq(llama_context* ctx, const llama_batch& batch, int seq, const std::vector<int>& idx,
                    const std::vector<int>& pos, const std::vector<int>& rows, double& bytes, std::string& err,
                    float* embd_dst = nullptr) {
    Context& c = ctx->c;
    context_select_seq(c, seq);
    const int n = (int)idx.size();
    if (embd_dst) embd_begin(c, n, embd_dst);
    int i0 = 0;
    const char* no_pf_env = getenv("LLMI_NO_PREFILL");
    const bool no_pf = no_pf_env && atoi(no_pf_env) != 0;
    const int p0 = pos[0];
    int run = 0;
    while (run < n - 1 && rows[(size_t)idx[(size_t)run]] < 0 && pos[(size_t)run] == p0 + run) ++run;
    // a run reaching past prefill_max_kv() positions (the LDS-resident attention kernels'
    // limit where the tiled one does not apply) goes through decode steps from there on
    if (!no_pf && run >= kPrefillMin && prefill_supported(*c.m)) {
        const int pf_lim = prefill_max_kv(c);
        if (p0 + run > pf_lim) run = std::max(0, pf_lim - p0);
    }
    if (!no_pf && run >= kPrefillMin && prefill_supported(*c.m)) {
        std::vector<int32_t> toks((size_t)run);
        for (int i = 0; i < run; ++i) toks[(size_t)i] = batch.token[idx[(size_t)i]];
        if (!prefill_enqueue(c, toks.data(), run, p0, err)) return false;
        c.pf_tokens += run;
        for (int i = 0; i < run; ++i) bytes += bytes_per_token(*c.m, p0 + i + 1);
        i0 = run;
    }
    for (int i = i0; i < n; ++i) {
        const int p = pos[(size_t)i];
        if (launch_state_set(c.st, batch.token[idx[(size_t)i]], p, c.stream) != hipSuccess || !step_run(c, p, err)) {
            if (err.empty()) err = "launch failed";
            return false;
        }
        bytes += bytes_per_token(*c.m, p + 1);
        const int r = rows[(size_t)idx[(size_t)i]];
        if (r >= 0) copy_out(ctx, r, c.logits, c.st, p);
        if (embd_dst && !embd_pool_enqueue(c, c.x, c.m->hp.n_embd, 1, err)) return false;
    }
    return true;
}

int32_t llama_decode(struct llama_context* ctx, struct llama_batch batch) {
    API_TRY
    if (!ctx) { set_err("null context"); return -1; }
    Context& c = ctx->c;
    const HParams& hp = c.m->hp;
    if (batch.n_tokens <= 0 || !batch.token) { set_err("llama_decode: empty batch or no tokens"); return -1; }
    if (batch.embd) { set_err("llama_decode: embedding input is not supported"); return -1; }
    const int n = batch.n_tokens;
    std::vector<int> rows((size_t)n, -1);
    int n_out = 0;
    for (int i = 0; i < n; ++i)
        if (batch.logits ? batch.logits[i] != 0 : i == n - 1) rows[(size_t)i] = n_out++;
    // tokens by sequence (llama_batch.seq_id[i][0]; no seq_id: sequence 0), in batch order
    std::vector<std::vector<int>> by_seq((size_t)c.n_seq), pos_of((size_t)c.n_seq);
    for (int i = 0; i < n; ++i) {
        const int tok = batch.token[i];
        if (tok < 0 || tok >= hp.n_vocab) { set_err("llama_decode: token id out of range"); return -1; }
        int s = 0;
        if (batch.seq_id && batch.n_seq_id) {
            if (batch.n_seq_id[i] > 1) { set_err("llama_decode: a token shared by several sequences is not supported"); return -1; }
            if (batch.n_seq_id[i] == 1) s = batch.seq_id[i][0];
        }
        if (s < 0 || s >= c.n_seq) { set_err("llama_decode: seq_id out of range (n_seq_max)"); return -1; }
        const int pos = batch.pos ? batch.pos[i] : seq_past_of(c, s) + (int)by_seq[(size_t)s].size();
        if (pos < 0) { set_err("llama_decode: negative position"); return -1; }
        if (pos >= c.n_ctx) { set_err("llama_decode: no KV slot (position >= n_ctx)"); return 1; }
        by_seq[(size_t)s].push_back(i);
        pos_of[(size_t)s].push_back(pos);
    }
    if (hipSetDevice(c.m->device) != hipSuccess) { set_err("hipSetDevice"); return -2; }
    (void)hipGetLastError();  // launch wrappers report hipGetLastError: drop an unrelated stale one
    if (n_out > 0 && !ensure_outs(ctx, n_out)) return -2;
    c.out_rows = rows;
    c.n_outputs = n_out;
    ctx->host_valid.assign((size_t)n_out, 0);
    c.logits_host.resize((size_t)std::max(1, n_out) * hp.n_vocab);
    std::string err;
    double bytes = 0;
    // embeddings mode (llama_set_embeddings): every sequence goes through run_seq, which pools
    // its hidden states; pooling NONE keeps a row per token, sequence by sequence
    const bool embd = c.embd_on;
    const size_t E = (size_t)hp.n_embd;
    ctx->embd_call = -2;
    struct EmbdDone {  // no sequence is being pooled once the call returns, however it returns
        Context& c;
        ~EmbdDone() { c.embd_total = 0; }
    } embd_done{c};
    if (embd && !embd_alloc(c, c.pooling == POOLING_NONE ? n : c.n_seq, err)) { set_err("llama_decode: " + err); return -2; }
    hipEventRecord(c.ev0, c.stream);
    // sequences with one token each advance together through batched steps (batch.hip,
    // up to kMaxBatch per step); the others run one sequence at a time
    std::vector<int> singles;
    for (int s = 0; s < c.n_seq; ++s)
        if (by_seq[(size_t)s].size() == 1) singles.push_back(s);
    if (singles.size() < 2 || embd) singles.clear();
    for (size_t g = 0; g < singles.size(); g += kMaxBatch) {
        const int nt = (int)std::min<size_t>(kMaxBatch, singles.size() - g);
        const int* seqs = singles.data() + g;
        int max_pos = 0;
        for (int k = 0; k < nt; ++k) {
            const int s = seqs[k], p = pos_of[(size_t)s][0];
            max_pos = std::max(max_pos, p);
            if (launch_state_set(c.st0 + s, batch.token[by_seq[(size_t)s][0]], p, c.stream) != hipSuccess) {
                set_err("llama_decode: state set failed");
                return -3;
            }
        }
        if (!bstep_run(c, nt, seqs, max_pos, err)) {
            // not batchable here (context beyond the batched attention's LDS bound, mixed
            // gate/up types): these sequences take the single-sequence path below
            err.clear();
            singles.resize(g);
            break;
        }
        for (int k = 0; k < nt; ++k) {
            const int s = seqs[k], p = pos_of[(size_t)s][0];
            bytes += bytes_per_token(*c.m, p + 1) / nt;  // weights once for the group, KV per sequence
            const int r = rows[(size_t)by_seq[(size_t)s][0]];
            if (r >= 0) copy_out(ctx, r, c.blogits + (size_t)k * hp.n_vocab, c.st0 + s, p);
        }
    }
    size_t embd_row = 0;  // pooling NONE: the first row of the sequence's tokens
    for (int s = 0; s < c.n_seq; ++s) {
        if (by_seq[(size_t)s].empty() || std::find(singles.begin(), singles.end(), s) != singles.end()) continue;
        float* dst = !embd ? nullptr : c.embd_out + (c.pooling == POOLING_NONE ? embd_row : (size_t)s) * E;
        if (!run_seq(ctx, batch, s, by_seq[(size_t)s], pos_of[(size_t)s], rows, bytes, err, dst)) {
            set_err("llama_decode: " + err);
            return -3;
        }
        embd_row += by_seq[(size_t)s].size();
    }
    hipEventRecord(c.ev1, c.stream);
    if (embd) {
        if (c.pooling == POOLING_NONE) {
            ctx->embd_stage.resize((size_t)n * E);
            (void)hipMemcpyAsync(ctx->embd_stage.data(), c.embd_out, (size_t)n * E * 4, hipMemcpyDeviceToHost, c.stream);
        } else {
            ctx->embd_host.resize((size_t)c.n_seq * E);
            for (int s = 0; s < c.n_seq; ++s)
                if (!by_seq[(size_t)s].empty())
                    (void)hipMemcpyAsync(ctx->embd_host.data() + (size_t)s * E, c.embd_out + (size_t)s * E, E * 4,
                                         hipMemcpyDeviceToHost, c.stream);
        }
    }
    context_fault_readback(c);
    hipError_t e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) { set_err("llama_decode: " + hip_err(e)); return -4; }
    if (!context_fault_ok(c, err)) { set_err("llama_decode: " + err); return -6; }
    float ms = 0.f;
    hipEventElapsedTime(&ms, c.ev0, c.ev1);
    c.last_us = ms * 1e3;
    c.last_bytes = bytes;
    if (embd && c.pooling == POOLING_NONE) {  // the staged rows, sequence by sequence, into batch order
        ctx->embd_host.resize((size_t)n * E);
        size_t r = 0;
        for (int s = 0; s < c.n_seq; ++s)
            for (int i : by_seq[(size_t)s])
                std::memcpy(ctx->embd_host.data() + (size_t)i * E, ctx->embd_stage.data() + (r++) * E, E * 4);
        ctx->embd_rows = n;
        ctx->embd_call = POOLING_NONE;
    } else if (embd) {
        ctx->embd_seq_ok.assign((size_t)c.n_seq, 0);
        for (int s = 0; s < c.n_seq; ++s) ctx->embd_seq_ok[(size_t)s] = !by_seq[(size_t)s].empty();
        ctx->embd_call = c.pooling;
    }
    for (int s = 0; s < c.n_seq; ++s) {
        if (by_seq[(size_t)s].empty()) continue;
        int last = seq_past_of(c, s) - 1;
        for (int p : pos_of[(size_t)s]) last = std::max(last, p);
        set_seq_past(c, s, last + 1);
    }
    return 0;
    API_CATCH(-5)
}

int llama_eval(struct llama_context* ctx, llama_token* tokens, int32_t n_tokens, int32_t n_past) {
    if (!ctx || !tokens || n_tokens <= 0) { set_err("llama_eval: bad arguments"); return 1; }
    std::vector<llama_pos> pos((size_t)n_tokens);
    for (int i = 0; i < n_tokens; ++i) pos[(size_t)i] = n_past + i;
    struct llama_batch b = llama_batch_get_one(tokens, n_tokens);
    b.pos = pos.data();
    return llama_decode(ctx, b) == 0 ? 0 : 1;
}

static int out_row(llama_context* ctx, int32_t i) {
    Context& c = ctx->c;
    if (c.n_outputs <= 0) return -1;
    if (i < 0) return c.n_outputs - 1;
    if (i >= (int)c.out_rows.size()) return -1;
    return c.out_rows[(size_t)i];
}

float* llama_get_logits_ith(struct llama_context* ctx, int32_t i) {
    API_TRY
    if (!ctx) return nullptr;
    const int r = out_row(ctx, i);
    if (r < 0) { set_err("llama_get_logits_ith: no logits for this batch index"); return nullptr; }
    Context& c = ctx->c;
    const size_t V = (size_t)c.m->hp.n_vocab;
    if (!ctx->host_valid[(size_t)r]) {
        (void)hipSetDevice(c.m->device);
        if (hipMemcpy(c.logits_host.data() + (size_t)r * V, ctx->outs + (size_t)r * V * 4, V * 4,
                      hipMemcpyDeviceToHost) != hipSuccess) {
            set_err("logits copy failed");
            return nullptr;
        }
        ctx->host_valid[(size_t)r] = 1;
    }
    return c.logits_host.data() + (size_t)r * V;
    API_CATCH(nullptr)
}

float* llama_get_logits(struct llama_context* ctx) {
    if (!ctx || ctx->c.n_outputs <= 0) { set_err("llama_get_logits: no outputs"); return nullptr; }
    for (int r = 0; r < ctx->c.n_outputs; ++r) {
        // materialise every output row
        int idx = -1;
        for (size_t k = 0; k < ctx->c.out_rows.size(); ++k)
            if (ctx->c.out_rows[k] == r) idx = (int)k;
        if (idx >= 0 && !llama_get_logits_ith(ctx, idx)) return nullptr;
    }
    return ctx->c.logits_host.data();
}

llama_token llmi_greedy_ith(struct llama_context* ctx, int32_t i) {
    if (!ctx) return -1;
    const int r = out_row(ctx, i);
    if (r < 0) { set_err("llmi_greedy_ith: no logits for this batch index"); return -1; }
    return (llama_token)key_token(ctx->keys_pinned + (size_t)r * kArgSlots);
}

int32_t llmi_generate_greedy(struct llama_context* ctx, llama_token first, int32_t pos0, int32_t n_gen, llama_token* out) {
    API_TRY
    return generate_one("llmi_generate_greedy", ctx, first, pos0, n_gen, out, false);
    API_CATCH(-5)
}

int32_t llmi_generate_greedy_batch(struct llama_context* ctx, int32_t n, const int32_t* seqs, const llama_token* first,
                                   const int32_t* pos0, int32_t n_gen, llama_token* out) {
    API_TRY
    return generate_batch("llmi_generate_greedy_batch", ctx, n, seqs, first, pos0, n_gen, out, nullptr, nullptr);
    API_CATCH(-5)
}

int32_t llmi_generate_sampled_batch(struct llama_context* ctx, int32_t n, const int32_t* seqs, const llama_token* first,
                                    const int32_t* pos0, int32_t n_gen, const struct llmi_sampler_params* params,
                                    const double* uniforms, llama_token* out) {
    API_TRY
    const char* name = "llmi_generate_sampled_batch";
    // what needs no context first: refusals name their field before any device work
    if (n <= 0 || n > kMaxBatch || !seqs || !first || !pos0 || !out || n_gen <= 0 || !params || !uniforms) {
        set_err(std::string(name) + ": bad arguments (1..8 sequences, no null pointers)");
        return -1;
    }
    for (int k = 0; k < n; ++k)
        for (int j = 0; j < k; ++j)
            if (seqs[j] == seqs[k]) { set_err(std::string(name) + ": repeated sequence"); return -1; }
    std::vector<SampleRec> recs((size_t)n);
    for (int k = 0; k < n; ++k) {
        const llmi_sampler_params& p = params[k];
        std::string why;
        if (!sample_rec_make(p.temperature, p.top_k, p.top_p, p.min_p, p.repeat_penalty, p.repeat_last_n, p.presence_penalty,
                             p.frequency_penalty, recs[(size_t)k], why)) {
            set_err(std::string(name) + ": params[" + std::to_string(k) + "]: " + why + " (the device sampler's limits)");
            return -1;
        }
    }
    if (!ctx) { set_err(std::string(name) + ": bad arguments (null context)"); return -1; }
    return generate_batch(name, ctx, n, seqs, first, pos0, n_gen, out, recs.data(), uniforms);
    API_CATCH(-5)
}

static_assert(LLMI_LOGPROBS_MAX_TOP == kLogprobMaxTop, "llmi.h limits");

int32_t llmi_generate_logprobs_batch(struct llama_context* ctx, int32_t n, const int32_t* seqs, const llama_token* first,
                                     const int32_t* pos0, int32_t n_gen, const struct llmi_sampler_params* params,
                                     const double* uniforms, const int32_t* n_top, llama_token* out, double* tok_logprob,
                                     int32_t* top_id, double* top_logprob) {
    API_TRY
    const std::string name = "llmi_generate_logprobs_batch";
    // what needs no context first: refusals name their field before any device work
    if (n <= 0 || n > kMaxBatch || n_gen <= 0) { set_err(name + ": bad arguments (1..8 sequences, n_gen >= 1)"); return -1; }
    const struct { const char* field; const void* p; } ptrs[] = {
        {"seqs", seqs}, {"first", first}, {"pos0", pos0}, {"params", params}, {"uniforms", uniforms}, {"n_top", n_top},
        {"out", out}, {"tok_logprob", tok_logprob}, {"top_id", top_id}, {"top_logprob", top_logprob}};
    for (const auto& f : ptrs)
        if (!f.p) { set_err(name + ": " + f.field + " is a null pointer"); return -1; }
    for (int k = 0; k < n; ++k)
        for (int j = 0; j < k; ++j)
            if (seqs[j] == seqs[k]) { set_err(name + ": seqs: repeated sequence"); return -1; }
    std::vector<SampleRec> recs((size_t)n);
    for (int k = 0; k < n; ++k) {
        const llmi_sampler_params& p = params[k];
        std::string why;
        if (!sample_rec_make(p.temperature, p.top_k, p.top_p, p.min_p, p.repeat_penalty, p.repeat_last_n, p.presence_penalty,
                             p.frequency_penalty, recs[(size_t)k], why)) {
            set_err(name + ": params[" + std::to_string(k) + "]: " + why + " (the device sampler's limits)");
            return -1;
        }
        if (n_top[k] < -1 || n_top[k] > kLogprobMaxTop) {
            set_err(name + ": n_top[" + std::to_string(k) + "] " + std::to_string(n_top[k]) + " outside -1.." +
                    std::to_string(kLogprobMaxTop));
            return -1;
        }
    }
    if (!ctx) { set_err(name + ": ctx is a null pointer"); return -1; }
    const LogprobOut lp = {n_top, tok_logprob, top_id, top_logprob};
    return generate_batch(name.c_str(), ctx, n, seqs, first, pos0, n_gen, out, recs.data(), uniforms, &lp);
    API_CATCH(-5)
}

bool llama_kv_self_seq_rm(struct llama_context* ctx, llama_seq_id seq_id, llama_pos p0, llama_pos p1) {
    if (!ctx) return false;
    Context& c = ctx->c;
    if (seq_id >= c.n_seq) return false;
    if (p1 >= 0) { set_err("llama_kv_self_seq_rm: only tail removal [p0, inf) is supported"); return false; }
    const int lo = seq_id < 0 ? 0 : seq_id, hi = seq_id < 0 ? c.n_seq : seq_id + 1;
    (void)hipSetDevice(c.device);
    for (int s = lo; s < hi; ++s) {
        if (p0 <= 0) {
            context_clear_seq(c, s);
        } else {
            // positions >= p0 are rewritten before any step attends to them (a step at
            // position p reads KV rows [0, p]): truncation is a bookkeeping change
            set_seq_past(c, s, std::min(seq_past_of(c, s), (int)p0));
        }
    }
    return true;
}

bool llama_kv_self_seq_cp(struct llama_context* ctx, llama_seq_id seq_src, llama_seq_id seq_dst, llama_pos p0, llama_pos p1) {
    API_TRY
    const std::string who = "llama_kv_self_seq_cp: ";
    if (!ctx) { set_err(who + "ctx is a null pointer"); return false; }
    Context& c = ctx->c;
    if (seq_src < 0 || seq_src >= c.n_seq) { set_err(who + "seq_src out of range (n_seq_max)"); return false; }
    if (seq_dst < 0 || seq_dst >= c.n_seq) { set_err(who + "seq_dst out of range (n_seq_max)"); return false; }
    if (seq_src == seq_dst) { set_err(who + "seq_src and seq_dst are the same sequence"); return false; }
    const int past_src = seq_past_of(c, seq_src), past_dst = seq_past_of(c, seq_dst);
    if (p0 < 0) p0 = 0;
    if (p1 < 0) p1 = past_src;
    if (p1 > past_src) { set_err(who + "p1 beyond seq_src's past"); return false; }
    if (p0 > past_dst) { set_err(who + "p0 beyond seq_dst's past (would leave a hole)"); return false; }
    if (p1 > 0 && p0 >= p1) { set_err(who + "p0 >= p1: an empty range"); return false; }
    if (p1 <= 0) {  // nothing to copy: seq_dst keeps its own [0, p0)
        set_seq_past(c, seq_dst, p0);
        return true;
    }
    const HParams& hp = c.m->hp;
    KvCopyArgs a;
    a.kc_src = c.kc0 + (size_t)seq_src * c.kv_seq_elems;
    a.vc_src = c.vc0 + (size_t)seq_src * c.kv_seq_elems;
    a.hist_src = c.hist0 + (size_t)seq_src * c.n_ctx;
    a.kc_dst = c.kc0 + (size_t)seq_dst * c.kv_seq_elems;
    a.vc_dst = c.vc0 + (size_t)seq_dst * c.kv_seq_elems;
    a.hist_dst = c.hist0 + (size_t)seq_dst * c.n_ctx;
    a.n_planes = hp.n_layer * hp.n_head_kv;
    a.head_dim = hp.head_dim;
    a.n_ctx = c.n_ctx;
    a.p0 = p0;
    a.p1 = p1;
    if (!kv_seq_cp_ok(a)) { set_err(who + "unsupported cache shape"); return false; }
    (void)hipSetDevice(c.device);
    (void)hipGetLastError();
    hipError_t e = launch_kv_seq_cp(a, c.max_blocks, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e != hipSuccess) { set_err(who + hip_err(e)); return false; }
    // seq_dst's StepState stays: the next call sets token and position from the host
    set_seq_past(c, seq_dst, p1);
    return true;
    API_CATCH(false)
}

int32_t llmi_seq_pos_max(const struct llama_context* ctx, llama_seq_id seq_id) {
    if (!ctx || seq_id < 0 || seq_id >= ctx->c.n_seq) return -1;
    return seq_past_of(ctx->c, seq_id) - 1;
}

void llmi_last_step_stats(struct llama_context* ctx, double* bytes, double* usec) {
    if (!ctx) return;
    if (bytes) *bytes = ctx->c.last_bytes;
    if (usec) *usec = ctx->c.last_us;
}

double llmi_model_upload_s(const struct llama_model* model) { return model ? model->m.upload_s : -1.0; }

int32_t llmi_prefill_supported(const struct llama_model* model) {
    return model && prefill_supported(model->m) ? 1 : 0;
}

int64_t llmi_prefill_token_count(const struct llama_context* ctx) { return ctx ? ctx->c.pf_tokens : 0; }

double llmi_bytes_per_token(const struct llama_model* model, int32_t n_kv) {
    return model ? bytes_per_token(model->m, n_kv) : 0.0;
}

const struct llama_vocab* llama_model_get_vocab(const struct llama_model* model) {
    return model ? &model->vocab : nullptr;
}
int32_t llama_model_n_embd(const struct llama_model* m) { return m ? m->m.hp.n_embd : 0; }
int32_t llama_model_n_layer(const struct llama_model* m) { return m ? m->m.hp.n_layer : 0; }
int32_t llama_model_n_head(const struct llama_model* m) { return m ? m->m.hp.n_head : 0; }
int32_t llama_model_n_head_kv(const struct llama_model* m) { return m ? m->m.hp.n_head_kv : 0; }
int32_t llama_model_n_ctx_train(const struct llama_model* m) { return m ? m->m.hp.n_ctx_train : 0; }
uint64_t llama_model_size(const struct llama_model* m) { return m ? (uint64_t)model_tensor_bytes(m->m) : 0; }
int32_t llama_model_desc(const struct llama_model* m, char* buf, size_t n) {
    if (!m) return -1;
    return snprintf(buf, n, "%s", m->m.desc.c_str());
}
uint32_t llama_n_ctx(const struct llama_context* ctx) { return ctx ? (uint32_t)ctx->c.n_ctx : 0; }
void llama_kv_self_clear(struct llama_context* ctx) {
    if (ctx) context_clear(ctx->c);
}

}  // extern "C"
