// model.cpp — GGUF model -> HBM arena: the loader, the arena plan, the chunked upload and
// the replica fan-out's schedule.
//
// Replaces upstream libllama's llama_model_loader.
#include "engine_internal.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>

namespace llmi {

Model::~Model() {
    if (arena && owns_arena) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(device);
        (void)hipFree(arena);
        (void)hipSetDevice(cur);
    }
}

namespace {

bool map_mat(const GgufFile& f, const std::string& name, DevMat& m, std::string& err, bool required = true) {
    const GgufTensor* t = f.tensor(name);
    if (!t) {
        if (required) err = "missing tensor " + name;
        return false;
    }
    m.type = t->type;
    m.cols = t->ne[0];
    m.rows = t->ne[1] * t->ne[2] * t->ne[3];
    return true;
}

}  // namespace

size_t model_tensor_bytes(const Model& m) {
    size_t b = m.tok_embd.bytes + m.out_norm.bytes + (m.output.off_a == m.tok_embd.off_a ? 0 : m.output.bytes);
    for (const Layer& L : m.layers)
        b += L.attn_norm.bytes + L.wq.bytes + L.wk.bytes + L.wv.bytes + L.wo.bytes + L.ffn_norm.bytes + L.wg.bytes +
             L.wu.bytes + L.wd.bytes;
    return b;
}

double bytes_per_token(const Model& m, int n_kv) {
    const HParams& hp = m.hp;
    double b = (double)m.output.bytes + (double)m.out_norm.bytes + (double)m.tok_embd.bytes / hp.n_vocab;
    for (const Layer& L : m.layers)
        b += (double)(L.attn_norm.bytes + L.wq.bytes + L.wk.bytes + L.wv.bytes + L.wo.bytes + L.ffn_norm.bytes +
                      L.wg.bytes + L.wu.bytes + L.wd.bytes);
    const double kv_row = 2.0 * hp.n_head_kv * hp.head_dim * 2.0;  // K+V f16 per layer per position
    b += hp.n_layer * kv_row * (double)n_kv;                       // KV read
    b += hp.n_layer * kv_row;                                      // KV write of the new token
    return b;
}

// end of a matrix's planes in the arena (plan_planes)
static size_t region_end(const DevMat& m) {
    const size_t nblk = (size_t)m.rows * (size_t)(m.cols / block_elems(m.type));
    switch (m.type) {
        case T_Q4_K: case T_Q5_K: return m.off_s + nblk * 16;
        case T_Q6_K: case T_Q8_0: return m.off_d + nblk * 2;
        default: return m.off_a + m.bytes;
    }
}

size_t fanout_plan(size_t arena_bytes, size_t chunk, const std::vector<size_t>& prefix_ends, std::vector<int>& ready) {
    ready.clear();
    if (chunk == 0 || arena_bytes == 0) return 0;
    const size_t n = (arena_bytes + chunk - 1) / chunk;
    size_t e = 0;
    for (size_t k = 0; k < n; ++k) {
        const size_t end = std::min((k + 1) * chunk, arena_bytes);
        while (e < prefix_ends.size() && prefix_ends[e] < end) ++e;
        ready.push_back(e < prefix_ends.size() ? (int)e : (int)prefix_ends.size() - 1);
    }
    return n;
}

bool model_load(const std::string& path, int device, bool vocab_only, bool no_upload, Model& M, std::string& err,
                const UploadHook* hook, int numerics) {
    M.path = path;
    M.device = device;
    if (numerics < 0 || numerics > (NUMERICS_X86 | NUMERICS_FA)) { err = "unknown numerics " + std::to_string(numerics); return false; }
    M.numerics = numerics & NUMERICS_X86;
    M.fa = (numerics & NUMERICS_FA) ? 1 : 0;
    M.file = std::make_shared<GgufFile>();
    GgufFile& f = *M.file;
    if (!f.open(path, err)) return false;
    const std::string arch = f.str("general.architecture", "");
    if (arch != "llama") { err = "unsupported architecture '" + arch + "' (llmi decodes the llama family)"; return false; }
    HParams& hp = M.hp;
    hp.n_embd = (int)f.num("llama.embedding_length", 0);
    hp.n_layer = (int)f.num("llama.block_count", 0);
    hp.n_head = (int)f.num("llama.attention.head_count", 0);
    hp.n_head_kv = (int)f.num("llama.attention.head_count_kv", hp.n_head);
    hp.n_ff = (int)f.num("llama.feed_forward_length", 0);
    hp.n_ctx_train = (int)f.num("llama.context_length", 4096);
    hp.eps = (float)f.num("llama.attention.layer_norm_rms_epsilon", 1e-5);
    hp.rope_base = (float)f.num("llama.rope.freq_base", 10000.0);
    hp.file_type = (int)f.num("general.file_type", 0);
    hp.pooling_type = (int)f.num("llama.pooling_type", -1);
    if (hp.n_embd <= 0 || hp.n_layer <= 0 || hp.n_head <= 0 || hp.n_head_kv <= 0) {
        err = "missing llama.* hyperparameters";
        return false;
    }
    hp.head_dim = hp.n_embd / hp.n_head;
    hp.n_rot = (int)f.num("llama.rope.dimension_count", hp.head_dim);
    if (const GgufKV* tk = f.kv("tokenizer.ggml.tokens")) M.vocab = tk->arr_str;
    M.bos = (int)f.num("tokenizer.ggml.bos_token_id", -1);
    M.eos = (int)f.num("tokenizer.ggml.eos_token_id", -1);
    if (!map_mat(f, "token_embd.weight", M.tok_embd, err)) return false;
    if (!map_mat(f, "output_norm.weight", M.out_norm, err)) return false;
    bool tied = !map_mat(f, "output.weight", M.output, err, false);
    hp.n_vocab = (int)M.tok_embd.rows;
    if (M.vocab.empty()) {
        M.vocab.resize((size_t)hp.n_vocab);
    }
    M.tok = Tokenizer::from_gguf(f, hp.n_vocab);
    M.layers.resize((size_t)hp.n_layer);
    for (int l = 0; l < hp.n_layer; ++l) {
        Layer& L = M.layers[(size_t)l];
        const std::string p = "blk." + std::to_string(l) + ".";
        if (!map_mat(f, p + "attn_norm.weight", L.attn_norm, err) || !map_mat(f, p + "attn_q.weight", L.wq, err) ||
            !map_mat(f, p + "attn_k.weight", L.wk, err) || !map_mat(f, p + "attn_v.weight", L.wv, err) ||
            !map_mat(f, p + "attn_output.weight", L.wo, err) || !map_mat(f, p + "ffn_norm.weight", L.ffn_norm, err) ||
            !map_mat(f, p + "ffn_gate.weight", L.wg, err) || !map_mat(f, p + "ffn_up.weight", L.wu, err) ||
            !map_mat(f, p + "ffn_down.weight", L.wd, err))
            return false;
    }
    if (hp.n_ff <= 0) hp.n_ff = (int)M.layers[0].wg.rows;
    // shape checks: everything the kernels assume
    const int E = hp.n_embd, D = hp.head_dim, nq = hp.n_head * D, nk = hp.n_head_kv * D;
    if (D != 64 && D != 128) { err = "head_dim " + std::to_string(D) + " unsupported (64 or 128)"; return false; }
    const int gqa = hp.n_head / hp.n_head_kv;
    if (hp.n_head % hp.n_head_kv || (gqa != 1 && gqa != 2 && gqa != 4 && gqa != 8)) {
        err = "GQA ratio unsupported";
        return false;
    }
    if (hp.n_rot <= 0 || hp.n_rot > D || hp.n_rot % 2) { err = "bad rope.dimension_count"; return false; }
    // scaled RoPE (linear, YaRN) is not implemented: refuse it, never decode it unscaled
    const std::string rs_type = f.str("llama.rope.scaling.type", "none");
    if (rs_type != "none") { err = "llama.rope.scaling.type '" + rs_type + "' not supported (RoPE is unscaled)"; return false; }
    if (f.num("llama.rope.scaling.factor", 1.0) != 1.0) {
        err = "llama.rope.scaling.factor other than 1 not supported (RoPE is unscaled)";
        return false;
    }
    if (E % 256 || hp.n_ff % 256) { err = "n_embd and n_ff must be multiples of 256"; return false; }
    auto chk = [&](const DevMat& m, int64_t rows, int64_t cols, const char* nm, bool quant) {
        if (m.rows != rows || m.cols != cols) { err = std::string(nm) + ": unexpected shape"; return false; }
        if (quant && !(m.type == T_Q4_K || m.type == T_Q5_K || m.type == T_Q6_K || m.type == T_Q8_0)) {
            err = std::string(nm) + ": weight type " + type_name(m.type) + " not supported on the decode path";
            return false;
        }
        if (!quant && m.type != T_F32) { err = std::string(nm) + ": norm weight must be f32"; return false; }
        if (quant && !planes_fit_u32(m.type, rows, cols)) { err = std::string(nm) + ": " + kPlaneLimitMsg; return false; }
        return true;
    };
    if (!chk(M.out_norm, 1, E, "output_norm", false)) return false;
    if (!chk(M.tok_embd, hp.n_vocab, E, "token_embd", true)) return false;
    if (!tied && !chk(M.output, hp.n_vocab, E, "output", true)) return false;
    for (const Layer& L : M.layers) {
        if (!chk(L.attn_norm, 1, E, "attn_norm", false) || !chk(L.ffn_norm, 1, E, "ffn_norm", false) ||
            !chk(L.wq, nq, E, "attn_q", true) || !chk(L.wk, nk, E, "attn_k", true) || !chk(L.wv, nk, E, "attn_v", true) ||
            !chk(L.wo, E, nq, "attn_output", true) || !chk(L.wg, hp.n_ff, E, "ffn_gate", true) ||
            !chk(L.wu, hp.n_ff, E, "ffn_up", true) || !chk(L.wd, E, hp.n_ff, "ffn_down", true))
            return false;
        if (act_kind(L.wg.type) != act_kind(L.wu.type)) { err = "ffn_gate/ffn_up mix Q8_0 with K-quants"; return false; }
    }
    if (const GgufTensor* rf = f.tensor("rope_freqs.weight")) {
        if (rf->type != T_F32 || rf->ne[0] * 2 < hp.n_rot) { err = "bad rope_freqs.weight"; return false; }
        M.rope_freq_host.assign((const float*)rf->data, (const float*)rf->data + rf->ne[0]);
        M.has_rope_freqs = true;
    }
    // ---- arena plan ----
    size_t off = 0;
    auto plan = [&](DevMat& m) { off = plan_planes(m, off); };
    plan(M.tok_embd);
    plan(M.out_norm);
    if (tied) M.output = M.tok_embd;
    else plan(M.output);
    for (Layer& L : M.layers) {
        plan(L.attn_norm); plan(L.wq); plan(L.wk); plan(L.wv); plan(L.wo);
        plan(L.ffn_norm); plan(L.wg); plan(L.wu); plan(L.wd);
    }
    M.arena_bytes = align_up(off, 4096);
    char desc[256];
    snprintf(desc, sizeof desc, "llama %dL E%d H%d/%d FF%d V%d ftype %d (%.2f GB)", hp.n_layer, E, hp.n_head,
             hp.n_head_kv, hp.n_ff, hp.n_vocab, hp.file_type, (double)model_tensor_bytes(M) / 1e9);
    M.desc = desc;
    if (vocab_only) return true;
    HIPC(hipSetDevice(device));
    HIPC(hipMalloc(&M.arena, M.arena_bytes));
    M.owns_arena = true;
    if (no_upload) return true;
    return model_upload(M, err, hook);
}

// The chunked H2D + on-device repack of every tensor into the planned arena (the model's
// GGUF stays mapped in M.file).  `hook` (replica fan-out) sees the arena prefix grow.
bool model_upload(Model& M, std::string& err, const UploadHook* hook) {
    if (!M.file || !M.arena) { err = "model_upload: no layout"; return false; }
    GgufFile& f = *M.file;
    const HParams& hp = M.hp;
    const bool tied = f.tensor("output.weight") == nullptr;
    if (hipSetDevice(M.device) != hipSuccess) { err = "hipSetDevice"; return false; }
    (void)hipGetLastError();  // launch_repack reports hipGetLastError: start from a clean slate
    // ---- upload: H2D + on-device repack of the unaligned block types ----
    struct Item { const GgufTensor* t; DevMat* m; };
    std::vector<Item> items;
    auto add = [&](const std::string& name, DevMat* m) { items.push_back({f.tensor(name), m}); };
    add("token_embd.weight", &M.tok_embd);
    add("output_norm.weight", &M.out_norm);
    if (!tied) add("output.weight", &M.output);
    for (int l = 0; l < hp.n_layer; ++l) {
        Layer& L = M.layers[(size_t)l];
        const std::string p = "blk." + std::to_string(l) + ".";
        add(p + "attn_norm.weight", &L.attn_norm); add(p + "attn_q.weight", &L.wq); add(p + "attn_k.weight", &L.wk);
        add(p + "attn_v.weight", &L.wv); add(p + "attn_output.weight", &L.wo); add(p + "ffn_norm.weight", &L.ffn_norm);
        add(p + "ffn_gate.weight", &L.wg); add(p + "ffn_up.weight", &L.wu); add(p + "ffn_down.weight", &L.wd);
    }
    // Chunked, double-buffered upload: host threads copy a chunk of whole rows from the
    // mmap into a pinned buffer (page faults of a cold file taken in parallel) while the
    // previous chunk's DMA and on-device repack run on the upload stream.
    constexpr size_t kChunk = 64u << 20;
    uint8_t* pin[2] = {nullptr, nullptr};
    uint8_t* dstage[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    hipStream_t us = nullptr;
    bool ok = true;
    DevPool stage;  // pin and dstage
    auto cleanup = [&]() {
        if (us) (void)hipStreamSynchronize(us);
        stage.free_all();
        for (int k = 0; k < 2; ++k)
            if (ev[k]) (void)hipEventDestroy(ev[k]);
        if (us) (void)hipStreamDestroy(us);
    };
    hipError_t e = hipStreamCreateWithFlags(&us, hipStreamNonBlocking);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        e = stage.alloc_pinned(pin[k], kChunk);
        if (e == hipSuccess) e = stage.alloc(dstage[k], kChunk);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        err = "upload buffers: " + hip_err(e);
        cleanup();
        return false;
    }
    const unsigned nthr = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    auto host_copy = [&](uint8_t* dst, const uint8_t* src, size_t n) {
        if (n < (4u << 20) || nthr == 1) { memcpy(dst, src, n); return; }
        std::vector<std::thread> th;
        const size_t per = (n + nthr - 1) / nthr;
        for (unsigned t = 0; t < nthr; ++t) {
            const size_t o = t * per;
            if (o >= n) break;
            th.emplace_back([=] { memcpy(dst + o, src + o, std::min(per, n - o)); });
        }
        for (auto& x : th) x.join();
    };
    int slot = 0;
    auto next_slot = [&]() -> hipError_t {
        if (used[slot]) {
            hipError_t e2 = hipEventSynchronize(ev[slot]);
            if (e2 != hipSuccess) return e2;
        }
        return hipSuccess;
    };
    const auto t_up = std::chrono::steady_clock::now();
    for (const Item& it : items) {
        const DevMat& m = *it.m;
        const uint8_t* src = (const uint8_t*)it.t->data;
        e = hipSuccess;
        if (needs_repack(m.type)) {
            const int64_t bpr = m.cols / block_elems(m.type);  // blocks per row
            const size_t row_raw = (size_t)bpr * block_bytes(m.type);
            // chunks of whole row groups (common.h): a multiple of 64 rows
            const int64_t rows_per = std::max<int64_t>(64, (int64_t)(kChunk / row_raw) / 64 * 64);
            const size_t pa = m.type == T_Q8_0 ? 32 : 128, ph = m.type == T_Q5_K ? 32 : m.type == T_Q6_K ? 64 : 0,
                         ps = m.type == T_Q8_0 ? 0 : 16, pd = (m.type == T_Q6_K || m.type == T_Q8_0) ? 2 : 0;
            for (int64_t r0 = 0; r0 < m.rows && e == hipSuccess; r0 += rows_per) {
                const int64_t nr = std::min(rows_per, m.rows - r0);
                const size_t n = (size_t)nr * row_raw;
                const size_t b0 = (size_t)r0 * bpr;
                e = next_slot();
                if (e != hipSuccess) break;
                host_copy(pin[slot], src + (size_t)r0 * row_raw, n);
                e = hipMemcpyAsync(dstage[slot], pin[slot], n, hipMemcpyHostToDevice, us);
                if (e == hipSuccess)
                    e = launch_repack(m.type, dstage[slot], M.arena + m.off_a + b0 * pa, M.arena + m.off_h + b0 * ph,
                                      M.arena + m.off_s + b0 * ps, M.arena + m.off_d + b0 * pd, nr * bpr, m.cols, m.rgs,
                                      M.numerics == NUMERICS_X86, us);
                if (e == hipSuccess) e = hipEventRecord(ev[slot], us);
                used[slot] = true;
                slot ^= 1;
            }
        } else {
            for (size_t o = 0; o < it.t->nbytes && e == hipSuccess; o += kChunk) {
                const size_t n = std::min(kChunk, it.t->nbytes - o);
                e = next_slot();
                if (e != hipSuccess) break;
                host_copy(pin[slot], src + o, n);
                e = hipMemcpyAsync(M.arena + m.off_a + o, pin[slot], n, hipMemcpyHostToDevice, us);
                if (e == hipSuccess) e = hipEventRecord(ev[slot], us);
                used[slot] = true;
                slot ^= 1;
            }
        }
        if (e != hipSuccess) { err = "upload of " + it.t->name + ": " + hip_err(e); ok = false; break; }
        if (hook) {
            const size_t end = &it == &items.back() ? M.arena_bytes : region_end(m);
            if (!(*hook)(end, us)) { err = "upload: fan-out failed"; ok = false; break; }
        }
    }
    if (ok) {
        e = hipStreamSynchronize(us);
        if (e != hipSuccess) { err = "upload: " + hip_err(e); ok = false; }
    }
    M.upload_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_up).count();
    cleanup();
    return ok;
}

bool model_clone_layout(const Model& src, int device, Model& dst, std::string& err) {
    dst.device = device;
    dst.numerics = src.numerics;
    dst.fa = src.fa;
    dst.path = src.path;
    dst.desc = src.desc;
    dst.file = src.file;
    dst.hp = src.hp;
    dst.tok_embd = src.tok_embd; dst.out_norm = src.out_norm; dst.output = src.output;
    dst.layers = src.layers;
    dst.vocab = src.vocab; dst.tok = src.tok; dst.bos = src.bos; dst.eos = src.eos;
    dst.rope_freq_host = src.rope_freq_host; dst.has_rope_freqs = src.has_rope_freqs;
    dst.arena_bytes = src.arena_bytes;
    HIPC(hipSetDevice(device));
    HIPC(hipMalloc(&dst.arena, dst.arena_bytes));
    dst.owns_arena = true;
    return true;
}

Seg seg_of(const Model& m, const DevMat& d, int row0) {
    Seg s;
    s.a = m.arena + d.off_a;
    s.h = m.arena + d.off_h;
    s.s = m.arena + d.off_s;
    s.d = m.arena + d.off_d;
    s.type = d.type;
    s.rows = (int)d.rows;
    s.row0 = row0;
    s.rgs = d.rgs;
    s.x86 = m.numerics == NUMERICS_X86;
    return s;
}

}  // namespace llmi
