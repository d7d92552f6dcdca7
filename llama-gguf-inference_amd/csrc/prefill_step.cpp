// prefill_step.cpp — the batched prefill's scratch and its per-ubatch launch schedule.
#include "engine_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace llmi {

// ---------------------------------------------------------------------------------
// Batched prefill: the prompt's tokens go through every layer as
// one launch per op over all of them (prefill.hip): embed -> per layer [norm+quant,
// q/k/v GEMMs (RoPE, KV write), causal attention, quant, attn_output GEMM (+residual),
// norm+quant, gate/up GEMM (SwiGLU), quant, down GEMM (+residual)].  Results equal T
// decode steps bit for bit (both follow ggml's generic order); the caller runs
// the prompt's last token as an ordinary decode step for its logits.
// ---------------------------------------------------------------------------------
bool prefill_supported(const Model& m) {
    const HParams& hp = m.hp;
    // flash-attention numerics: prompts as decode steps unless LLMI_FA_PREFILL=1 (read on
    // every call) opts in to k_pf_attn_fa (pfattnfa.hip, <= 32 heads per KV head)
    if (m.fa) {
        const char* e = getenv("LLMI_FA_PREFILL");
        if (!e || atoi(e) == 0) return false;
        if (hp.n_head_kv <= 0 || hp.n_head % hp.n_head_kv || hp.n_head / hp.n_head_kv > 32) return false;
    }
    if (hp.head_dim != 128 && hp.head_dim != 64) return false;
    if (hp.n_rot % 2 || hp.n_rot > hp.head_dim) return false;
    for (const Layer& L : m.layers) {
        const DevMat* ms[] = {&L.wq, &L.wk, &L.wv, &L.wo, &L.wg, &L.wu, &L.wd};
        for (const DevMat* d : ms) {
            if (!pf_gemm_ok(d->type, (int)d->rows, (int)d->cols)) return false;
        }
        if (act_kind(L.wg.type) != act_kind(L.wu.type)) return false;
    }
    return true;
}

static bool prefill_alloc(Context& c, std::string& err) {
    if (c.pf_cap) return true;
    const HParams& hp = c.m->hp;
    // ubatch (llama.cpp's default n_ubatch 512; LLMI_PF_UBATCH, a multiple of 64 up to
    // 4096, for A/B), a multiple of 64 (k_pf_gemm's token groups)
    int cap = 512;
    if (const char* e = getenv("LLMI_PF_UBATCH")) {
        const int v = atoi(e);
        if (v >= 64 && v <= 4096 && v % 64 == 0) cap = v;
    }
    const size_t E = hp.n_embd, QD = (size_t)hp.n_head * hp.head_dim, F = hp.n_ff;
    const size_t maxc = std::max({E, QD, F});
    HIPC(c.pool.alloc(c.pf_tok, cap * 4));
    HIPC(c.pool.alloc(c.pf_x, cap * E * 4));
    HIPC(c.pool.alloc(c.pf_q, cap * QD * 4));
    HIPC(c.pool.alloc(c.pf_att, cap * QD * 4));
    HIPC(c.pool.alloc(c.pf_h, cap * F * 4));
    HIPC(c.pool.alloc(c.pf_aq, cap * maxc * 2));
    HIPC(c.pool.alloc(c.pf_abs, cap * (maxc / 16) * 2));
    HIPC(c.pool.alloc(c.pf_ad, cap * (maxc / 32) * 4));
    HIPC(c.pool.alloc(c.pf_abf, cap * (maxc / 256) * 64));
    // padded token rows of the activation buffers are read (never stored): keep them finite
    HIPC(hipMemsetAsync(c.pf_aq, 0, cap * maxc * 2, c.stream));
    HIPC(hipMemsetAsync(c.pf_abs, 0, cap * (maxc / 16) * 2, c.stream));
    HIPC(hipMemsetAsync(c.pf_ad, 0, cap * (maxc / 32) * 4, c.stream));
    HIPC(hipMemsetAsync(c.pf_abf, 0, cap * (maxc / 256) * 64, c.stream));
    // the tiled attention's score rows (<= kPfFaScratchCap, launches chunked to fit); a
    // failed allocation leaves the LDS kernels in charge
    const size_t wsc = pf_fa_scratch_bytes(hp.n_head, hp.n_head_kv, hp.head_dim, cap, c.n_ctx);
    if (wsc && !g_pf_fa_noalloc && c.pool.alloc(c.pf_wsc, wsc) == hipSuccess) c.pf_wsc_bytes = wsc;
    else { c.pf_wsc = nullptr; (void)hipGetLastError(); }
    c.pf_cap = cap;
    return true;
}

int prefill_max_kv(Context& c) {
    const HParams& hp = c.m->hp;
    const int lim = pf_max_kv();
    if (c.m->fa) return std::min(c.n_ctx, kFaMaxKV);  // k_pf_attn_fa streams the keys: no score space
    if (c.m->numerics == NUMERICS_X86)  // k_pf_a86 keeps the G heads' scores in LDS
        return std::min(lim, pf_attn_x86_max_kv(hp.n_head, hp.n_head_kv, hp.head_dim));
    // the whole context only where the tiled kernel can run: its score scratch must exist
    // (allocated here, before the limit is chosen; a failed allocation leaves the LDS
    // kernels' limit)
    std::string err;
    if (lim == kPfAttnMaxKV && g_pf_attn_fa && !g_pf_attn_simple && prefill_alloc(c, err) && c.pf_wsc)
        return c.n_ctx;
    return lim;
}

bool prefill_enqueue(Context& c, const int32_t* tokens, int n, int pos0, std::string& err) {
    const Model& m = *c.m;
    const HParams& hp = m.hp;
    if (!prefill_supported(m)) { err = "prefill: model shapes not supported by the batched path"; return false; }
    if (pos0 < 0 || pos0 + n > c.n_ctx) { err = "prefill: positions out of the context"; return false; }
    if (!prefill_alloc(c, err)) return false;
    const int E = hp.n_embd, D = hp.head_dim, nq = hp.n_head * D, F = hp.n_ff;
    const size_t kv_layer = (size_t)hp.n_head_kv * c.n_ctx * D;
    const int x86 = m.numerics == NUMERICS_X86;
    for (int b0 = 0; b0 < n; b0 += c.pf_cap) {
        const int T = std::min(c.pf_cap, n - b0), p0 = pos0 + b0;
        HIPC(hipMemcpyAsync(c.pf_tok, tokens + b0, (size_t)T * 4, hipMemcpyHostToDevice, c.stream));
        HIPC(launch_pf_embed(seg_of(m, m.tok_embd, 0), E, hp.n_vocab, c.pf_tok, c.pf_x, T, c.hist, p0, c.n_ctx, c.stream));
        for (int l = 0; l < hp.n_layer; ++l) {
            const Layer& L = m.layers[(size_t)l];
            PfGemm g;
            g.T = T; g.aq = c.pf_aq; g.abs = c.pf_abs; g.ad = c.pf_ad; g.abf = c.pf_abf;
            g.kc = c.kc + l * kv_layer; g.vc = c.vc + l * kv_layer; g.rope = c.rope;
            g.pos0 = p0; g.head_dim = D; g.n_rot = hp.n_rot; g.n_ctx = c.n_ctx;
            // q, k, v (each quantized for its own activation kind; pf_qkv_launches)
            g.cols = E; g.y = c.pf_q; g.ldy = nq;
            const Seg qkv[3] = {seg_of(m, L.wq, 0), seg_of(m, L.wk, 0), seg_of(m, L.wv, 0)};
            PfGemm qg[3];
            int qkind[3];
            const int nqg = pf_qkv_launches(qkv, g_pf_qkv_merge != 0, g, qg, qkind);
            for (int i = 0; i < nqg; ++i) {
                if (qkind[i] >= 0)
                    HIPC(launch_pf_quant(c.pf_x, E, (const float*)(m.arena + L.attn_norm.off_a), hp.eps, E, qkind[i], T,
                                        c.pf_aq, c.pf_abs, c.pf_ad, c.pf_abf, c.stream, x86));
                HIPC(launch_pf_gemm(qg[i], EPI_QKV, c.stream));
            }
            PfAttn at;
            at.q = c.pf_q; at.out = c.pf_att; at.ldq = nq; at.kc = g.kc; at.vc = g.vc;
            at.n_ctx = c.n_ctx; at.pos0 = p0; at.gqa = hp.n_head / hp.n_head_kv; at.max_kv = p0 + T;
            at.scale = 1.0f / sqrtf((float)D);
            at.wsc = c.pf_wsc; at.wsc_bytes = c.pf_wsc_bytes;
            at.num = x86;
            at.fa = m.fa;
            HIPC(launch_pf_attn(at, hp.n_head, D, T, c.stream));
            // attn_output + residual
            HIPC(launch_pf_quant(c.pf_att, nq, nullptr, 0.f, nq, act_kind(L.wo.type), T, c.pf_aq, c.pf_abs, c.pf_ad, c.pf_abf, c.stream, x86));
            g.w = seg_of(m, L.wo, 0); g.rows = (int)L.wo.rows; g.cols = nq; g.y = c.pf_x; g.ldy = E;
            HIPC(launch_pf_gemm(g, EPI_ADD, c.stream));
            // gate/up + SwiGLU
            HIPC(launch_pf_quant(c.pf_x, E, (const float*)(m.arena + L.ffn_norm.off_a), hp.eps, E, act_kind(L.wg.type), T,
                                c.pf_aq, c.pf_abs, c.pf_ad, c.pf_abf, c.stream, x86));
            g.w = seg_of(m, L.wg, 0); g.w2 = seg_of(m, L.wu, 0); g.rows = (int)L.wg.rows; g.cols = E; g.y = c.pf_h; g.ldy = F;
            {  // gate into h, then h = silu(h) * up (two launches: a fused gate+up launch
               // spills past 256 VGPRs and measured slower: Mistral 2048 TTFT 229 vs 225
               // ms, 8B 180 vs 165, profiles/r04/prefill/swiglu_fused_vs_two.txt)
                if (act_kind(L.wu.type) != act_kind(L.wg.type)) {
                    err = "prefill: ffn_gate/ffn_up of different activation kinds";
                    return false;
                }
                HIPC(launch_pf_gemm(g, EPI_STORE, c.stream));
                g.w = seg_of(m, L.wu, 0);
                HIPC(launch_pf_gemm(g, EPI_SWIGLU_UP, c.stream));
            }
            // down + residual
            HIPC(launch_pf_quant(c.pf_h, F, nullptr, 0.f, F, act_kind(L.wd.type), T, c.pf_aq, c.pf_abs, c.pf_ad, c.pf_abf, c.stream, x86));
            g.w = seg_of(m, L.wd, 0); g.rows = (int)L.wd.rows; g.cols = F; g.y = c.pf_x; g.ldy = E;
            HIPC(launch_pf_gemm(g, EPI_ADD, c.stream));
        }
        // embeddings: the chunk's final hidden states, before the next chunk overwrites them
        if (c.embd_total > 0 && !embd_pool_enqueue(c, c.pf_x, E, T, err)) return false;
    }
    return true;
}

}  // namespace llmi
