// decode_step.cpp — the per-step kernel schedule of one sequence and of a batch of them.
//
// Replaces upstream's llm_build_llama graph for one token.  One
// decode step is 2 + 6*n_layer kernel launches, captured once per 256-position KV bucket
// into a HIP graph and replayed; the next token is fed back on the device (argmax key ->
// k_embed), so greedy generation needs no host round trip.
#include "engine_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace llmi {

#if defined(LLMI_EXPERIMENTS)
// LLMI_EXP_XQ (step_enqueue): a zero q8 image, allocated before any capture
static const int exp_xq = [] {
    const char* e = getenv("LLMI_EXP_XQ");
    return e ? atoi(e) : 0;
}();
static uint8_t* g_exp_img = nullptr;
static bool exp_prepare(const Model& m) {
    if (!exp_xq || g_exp_img) return true;
    const size_t nb = (size_t)(std::max<int64_t>(m.hp.n_ff, m.hp.n_vocab > 0 ? m.hp.n_embd * 2 : 0) / 256 + 1) * 304;
    return hipMalloc(&g_exp_img, nb) == hipSuccess && hipMemset(g_exp_img, 0, nb) == hipSuccess &&
           hipDeviceSynchronize() == hipSuccess;
}
#endif

// How a step ends after its logits launch, over the nt rows at `logits` (states st, histories
// hist; the batched step: slot s is sequence tseq[s], histories hist_stride apart).
static bool enqueue_step_tail(Context& c, int tail, float* logits, StepState* st, const int32_t* hist, int nt,
                              const int* tseq, size_t hist_stride, std::string& err) {
    LogprobArgs la;
    la.logits = logits; la.V = c.m->hp.n_vocab; la.st = st; la.hist = hist; la.hist_stride = hist_stride;
    la.tseq = tseq; la.rec = c.srec; la.lrec = c.lrec;
    // the raw rows' logsumexp and alternatives, before the sampler rewrites them
    if (tail == STEP_LOGPROBS) HIPC_AS("launch_logprob", launch_logprob(la, nt, c.stream));
    if (tail != STEP_GREEDY) {  // the sampler chain over the step's logits, one launch for every slot: the key slots
                                // then hold the sampled token (a slot whose record says greedy keeps its argmax keys)
        SampleArgs sa;
        sa.logits = logits; sa.V = la.V; sa.st = st; sa.hist = hist; sa.hist_stride = hist_stride;
        sa.tseq = tseq; sa.rec = c.srec;
        HIPC_AS("launch_sample", launch_sample(sa, nt, c.stream));
    }
    // the chosen tokens' log-probabilities
    if (tail == STEP_LOGPROBS) HIPC_AS("launch_logprob_pick", launch_logprob_pick(la, nt, c.stream));
    return true;
}

bool step_enqueue(Context& c, int kv_bound, std::string& err, int tail) {
    const Model& m = *c.m;
    const HParams& hp = m.hp;
    const int E = hp.n_embd, D = hp.head_dim, nq = hp.n_head * D, nk = hp.n_head_kv * D;
    const size_t kv_layer = (size_t)hp.n_head_kv * c.n_ctx * D;
    EmbArgs ea;
    ea.w = seg_of(m, m.tok_embd, 0);
    ea.cols = E; ea.vocab = hp.n_vocab; ea.x = c.x; ea.st = c.st; ea.hist = c.hist; ea.n_ctx = c.n_ctx;
    Prof* P = c.prof;
    const double kvpos = (double)hp.n_head_kv * D * 2.0;  // bytes of K (or V) per layer per position
#if defined(LLMI_EXPERIMENTS)
    // experiment builds only (make EXTRA=-DLLMI_EXPERIMENTS; results garbage, never in
    // the product library): LLMI_EXP_SKIP = bitmask of kernel classes left out of the
    // step, LLMI_EXP_XFIRST = multi-round launches also wait for x before the weights
    static const int exp_skip = [] {
        const char* e = getenv("LLMI_EXP_SKIP");
        return e ? atoi(e) : 0;
    }();
    static const int exp_xfirst = [] {
        const char* e = getenv("LLMI_EXP_XFIRST");
        return e ? atoi(e) : 0;
    }();
    // LLMI_EXP_XQ = bitmask (1 QKV, 2 attn_output, 4 gate+up, 8 down, 16 output) of launches
    // fed a zero q8 image instead of their prologue: the upper bound of a free image
    if (exp_xq && !g_exp_img) { err = "exp_img not allocated"; return false; }
    auto xq_for = [&](int bit) -> const uint8_t* { return (exp_xq >> bit & 1) ? g_exp_img : nullptr; };
#else
    constexpr int exp_skip = 0, exp_xfirst = 0;
    auto xq_for = [](int) -> const uint8_t* { return nullptr; };
#endif
    auto want = [P](int k) { return !(exp_skip >> k & 1) && (!P || P->want(k)); };
    // a filtered launch, armed with an event pair when the profiler asks for timing
#define LLMI_RUN(K, EXPR)                                  \
    do {                                                   \
        if (want(K)) {                                     \
            if (P && !P->arm(K)) {                         \
                err = "hipEventCreate failed";             \
                return false;                              \
            }                                              \
            const hipError_t r_ = (EXPR);                  \
            if (P) Prof::disarm();                         \
            HIPC_AS(#EXPR, r_);                            \
        }                                                  \
    } while (0)
    // layer engine (leng.hip): one persistent launch per layer for attn_output, gate/up,
    // down and the next layer's QKV when the shapes qualify (LLMI_ENGINE=0: separate
    // launches); its edge counters are zeroed once per step
    const bool use_le = le_wanted() && c.le_cnt && !exp_skip && !exp_xfirst && !xq_for(0) && !xq_for(1) && !xq_for(2) &&
                        !xq_for(3);
    if (use_le && hipMemsetAsync(c.le_cnt, 0, le_counter_bytes(hp.n_layer), c.stream) != hipSuccess) {
        err = "hipMemsetAsync(le_cnt) failed";
        return false;
    }
    LLMI_RUN(K_EMBED, launch_embed(ea, c.stream));
    if (P) P->add(K_EMBED, (double)m.tok_embd.bytes / hp.n_vocab + E * 4.0);
    const int num = m.numerics;
    // QKV + RoPE + KV write of layer l, grouped by activation kind: n launches' args
    auto qkv_groups = [&](int l, MVArgs (&out)[3], double (&bytes)[3]) -> int {
        const Layer& L = m.layers[(size_t)l];
        MVArgs a; a.xfirst = exp_xfirst >> 0 & 1; a.num = num; a.xq = xq_for(0);
        a.cols = E; a.x = c.x; a.nw = (const float*)(m.arena + L.attn_norm.off_a); a.eps = hp.eps; a.y = c.q;
        a.kc = c.kc + l * kv_layer; a.vc = c.vc + l * kv_layer; a.rope = c.rope; a.st = c.st;
        a.head_dim = D; a.n_rot = hp.n_rot; a.n_ctx = c.n_ctx; a.nq = nq; a.nk = nk;
        const Seg qkv[3] = {seg_of(m, L.wq, 0), seg_of(m, L.wk, nq), seg_of(m, L.wv, nq + nk)};
        int first[3];
        const int n = qkv_launch_groups(qkv, true, a, out, first);
        for (int g = 0; g < n; ++g) {
            double b = 8.0 * E;
            for (int k = first[g]; k < first[g] + out[g].nseg; ++k) {
                const DevMat& dm = k == 0 ? L.wq : k == 1 ? L.wk : L.wv;
                b += (double)dm.bytes + (k == 0 ? 4.0 * nq : 2.0 * nk);
            }
            bytes[g] = b;
        }
        return n;
    };
    bool qkv_done = false;  // layer l's QKV already ran inside layer l-1's engine launch
    for (int l = 0; l < hp.n_layer; ++l) {
        const Layer& L = m.layers[(size_t)l];
        if (!qkv_done) {
            MVArgs qg[3];
            double qb[3];
            const int nqg = qkv_groups(l, qg, qb);
            for (int i = 0; i < nqg; ++i) {
                LLMI_RUN(K_QKV, launch_matvec(qg[i], EPI_QKV, c.max_blocks, c.stream));
                if (P) P->add(K_QKV, qb[i]);
            }
        }
        qkv_done = false;
        // --- attention ---
        AttnArgs at;
        at.q = c.q; at.kc = c.kc + l * kv_layer; at.vc = c.vc + l * kv_layer; at.out = c.att; at.st = c.st;
        attn_bind_scratch(at, c.scores, hp.n_head, c.n_ctx);  // at.fault = c.fault_dev
        at.n_ctx = c.n_ctx; at.scale = 1.0f / sqrtf((float)D);
        at.layer = l;
        at.num = num;
        at.fa = m.fa;
        LLMI_RUN(K_ATTN, launch_attention(at, hp.n_head, hp.n_head_kv, D, kv_bound, c.stream));
        if (P) P->add(K_ATTN, 8.0 * nq, 2.0 * kvpos);
        // --- output projection + residual ---
        MVArgs o; o.xfirst = exp_xfirst >> 1 & 1; o.num = num; o.xq = xq_for(1);
        o.seg[0] = seg_of(m, L.wo, 0); o.nseg = 1; o.cols = nq; o.x = c.att; o.y = c.x; o.npairs = (E + 1) / 2;
        const double o_bytes = (double)L.wo.bytes + 4.0 * nq + 8.0 * E;
        // --- gate/up + SwiGLU ---
        MVArgs gu; gu.xfirst = exp_xfirst >> 2 & 1; gu.num = num; gu.xq = xq_for(2);
        gu.seg[0] = seg_of(m, L.wg, 0); gu.seg[1] = seg_of(m, L.wu, 0); gu.nseg = 2;
        gu.cols = E; gu.x = c.x; gu.nw = (const float*)(m.arena + L.ffn_norm.off_a); gu.eps = hp.eps;
        gu.y = c.h; gu.npairs = hp.n_ff;
        const double gu_bytes = (double)(L.wg.bytes + L.wu.bytes) + 8.0 * E + 4.0 * hp.n_ff;
        // --- down + residual ---
        MVArgs dn; dn.xfirst = exp_xfirst >> 3 & 1; dn.num = num; dn.xq = xq_for(3);
        dn.seg[0] = seg_of(m, L.wd, 0); dn.nseg = 1; dn.cols = hp.n_ff; dn.x = c.h; dn.y = c.x; dn.npairs = (E + 1) / 2;
        const double dn_bytes = (double)L.wd.bytes + 4.0 * hp.n_ff + 8.0 * E;
        bool engine_ran = false;
        if (use_le && want(K_LAYER)) {
            LeArgs la;
            la.op[0] = o; la.op[1] = gu; la.op[2] = dn; la.nops = 3;
            double lb = o_bytes + gu_bytes + dn_bytes;
            if (l + 1 < hp.n_layer) {
                MVArgs qn[3];
                double qb[3];
                if (qkv_groups(l + 1, qn, qb) == 1) { la.op[3] = qn[0]; la.nops = 4; lb += qb[0]; }
            }
            la.cnt = c.le_cnt + (size_t)l * kLeOps * 16;
            la.cnt_stride = le_counter_stride(hp.n_layer);
            la.fault = c.fault_dev;
            if (l == c.le_trace_layer) la.trace = c.le_trace;
            const hipError_t ep = layer_engine_prepare(la);
            if (ep == hipSuccess) {
                LLMI_RUN(K_LAYER, launch_layer_engine(la, c.stream));
                if (P) P->add(K_LAYER, lb);
                engine_ran = true;
                qkv_done = la.nops == 4;
            } else if (ep != hipErrorNotSupported) {
                err = "layer_engine_prepare: " + hip_err(ep);
                return false;
            }
        }
        if (!engine_ran) {
            LLMI_RUN(K_ATTN_OUT, launch_matvec(o, EPI_ADD, c.max_blocks, c.stream));
            if (P) P->add(K_ATTN_OUT, o_bytes);
            LLMI_RUN(K_FFN_GATE_UP, launch_matvec(gu, EPI_SWIGLU, c.max_blocks, c.stream));
            if (P) P->add(K_FFN_GATE_UP, gu_bytes);
            LLMI_RUN(K_FFN_DOWN, launch_matvec(dn, EPI_ADD, c.max_blocks, c.stream));
            if (P) P->add(K_FFN_DOWN, dn_bytes);
        }
    }
    MVArgs lo;
    lo.num = m.numerics; lo.xq = xq_for(4);
    lo.seg[0] = seg_of(m, m.output, 0); lo.nseg = 1; lo.cols = E; lo.x = c.x;
    lo.nw = (const float*)(m.arena + m.out_norm.off_a); lo.eps = hp.eps; lo.y = c.logits;
    lo.npairs = (hp.n_vocab + 1) / 2; lo.argmax = &c.st->key[0][0]; lo.st = c.st;
    LLMI_RUN(K_OUTPUT, launch_matvec(lo, EPI_LOGITS, c.max_blocks, c.stream));
    if (P) P->add(K_OUTPUT, (double)m.output.bytes + 8.0 * E + 4.0 * hp.n_vocab);
#undef LLMI_RUN
    return enqueue_step_tail(c, tail, c.logits, c.st, c.hist, 1, nullptr, 0, err);
}

bool step_run(Context& c, int pos, std::string& err, int tail) {
#if defined(LLMI_EXPERIMENTS)
    if (!exp_prepare(*c.m)) { err = "exp_img"; return false; }
#endif
    const int kv_bound = kv_bucket_bound(pos + 1, c.n_ctx);
    if (!c.use_graphs) return step_enqueue(c, kv_bound, err, tail);
    const int bucket = pos / 256;
    const int gkey = bucket * 256 + c.cur_seq;
    hipGraphExec_t ex = c.graphs.find_or_capture(
        tail, gkey, c.stream, [&](std::string& e) { return step_enqueue(c, kv_bound, e, tail); }, err);
    if (!ex) return false;
    HIPC_AS("hipGraphLaunch(it->second, c.stream)", hipGraphLaunch(ex, c.stream));
    return true;
}

// ---------------------------------------------------------------------------------
// Batched decode (batch.hip): nt sequences advance one token per
// step; every launch streams its weights once for all of them.  Per step: k_bembed, then
// per layer QKV (k_mvn, segments grouped by weight type), the split attention over a
// third grid dimension of slots, attn_output, gate/up, down; the output head (k_mvn
// LOGITS) leaves each sequence's argmax in its own StepState slots.
// ---------------------------------------------------------------------------------
static bool balloc(Context& c, std::string& err) {
    if (c.bx) return true;
    const HParams& hp = c.m->hp;
    const size_t B = kMaxBatch, E = hp.n_embd, QD = (size_t)hp.n_head * hp.head_dim, F = hp.n_ff, V = hp.n_vocab;
    HIPC(c.pool.alloc(c.bx, B * E * 4));
    HIPC(c.pool.alloc(c.bq, B * QD * 4));
    HIPC(c.pool.alloc(c.batt, B * QD * 4));
    HIPC(c.pool.alloc(c.bh, B * F * 4));
    HIPC(c.pool.alloc(c.blogits, B * V * 4));
    HIPC(c.pool.alloc(c.bscores, B * attn_scratch_floats(hp.n_head, c.n_ctx) * 4));
    HIPC(c.pool.alloc(c.btpos, B * 4));
    HIPC(c.pool.alloc(c.btseq, B * 4));
    const size_t maxc = std::max({(size_t)E, QD, F});
    HIPC(c.pool.alloc(c.baq, 32 * maxc * 2));
    HIPC(c.pool.alloc(c.babs, B * (maxc / 16) * 2));
    HIPC(c.pool.alloc(c.bad, B * (maxc / 32) * 4));
    HIPC(hipMemsetAsync(c.baq, 0, 32 * maxc * 2, c.stream));
    HIPC(c.pool.alloc(c.babf, 32 * (maxc / 256) * 64));
    HIPC(hipMemsetAsync(c.babf, 0, 32 * (maxc / 256) * 64, c.stream));
    // padded slots read these rows: finite (zeros); their positions 0.  On the context
    // stream (a null-stream memset is not ordered with it: it could land after the slot
    // map upload that follows and point every slot at sequence 0)
    HIPC(hipMemsetAsync(c.bx, 0, B * E * 4, c.stream));
    HIPC(hipMemsetAsync(c.batt, 0, B * QD * 4, c.stream));
    HIPC(hipMemsetAsync(c.bh, 0, B * F * 4, c.stream));
    HIPC(hipMemsetAsync(c.btpos, 0, B * 4, c.stream));
    HIPC(hipMemsetAsync(c.btseq, 0, B * 4, c.stream));
    HIPC(hipStreamSynchronize(c.stream));
    return true;
}

static bool bstep_enqueue(Context& c, int nt, const int* seqs, int kv_bound, std::string& err, int tail) {
    const Model& m = *c.m;
    const HParams& hp = m.hp;
    const int E = hp.n_embd, D = hp.head_dim, QD = hp.n_head * D, nk = hp.n_head_kv * D, F = hp.n_ff, V = hp.n_vocab;
    const size_t kv_layer = (size_t)hp.n_head_kv * c.n_ctx * D;
    BEmbArgs ea;
    ea.w = seg_of(m, m.tok_embd, 0); ea.cols = E; ea.vocab = V; ea.n_ctx = c.n_ctx; ea.nt = nt;
    ea.x = c.bx; ea.st = c.st0; ea.hist = c.hist0; ea.tseq = c.btseq; ea.tpos = c.btpos;
    HIPC(launch_bembed(ea, c.stream));
    MVArgs base;
    base.tpos = c.btpos; base.tseq = c.btseq; base.kv_stride = c.kv_seq_elems; base.st = c.st0;
    base.num = m.numerics;
    const bool x86 = m.numerics == NUMERICS_X86;
    // one matvec of the step: k_bmd / k_bmm (matrix cores; x86 numerics: k_bmd's x86 fold)
    // after quantizing the nt inputs, where its segments qualify, else k_mvn (x86: its x86
    // form); `quantized` skips the quantization for a launch that reads the same input as
    // the previous one
    bool qkv_quant = false;
    auto bmv = [&](const MVArgs& a, int epi, bool& quantized) -> hipError_t {
        if (nt < bmm_min_tokens() || !bmm_ok(a, epi)) return launch_mvn(a, epi, nt, c.max_blocks, c.stream);
        if (!quantized) {
            const hipError_t e = launch_pf_quant(a.x, a.x_stride, a.nw, a.eps, a.cols, 0, nt, c.baq, c.babs, c.bad, c.babf,
                                                 c.stream, x86 ? 1 : 0);
            if (e != hipSuccess) return e;
            quantized = true;
        }
        return launch_bmm(a, epi, nt, c.baq, c.babf, c.bad, c.stream);
    };
    for (int l = 0; l < hp.n_layer; ++l) {
        const Layer& L = m.layers[(size_t)l];
        qkv_quant = false;
        // QKV + RoPE + f16 KV write: one launch per run of same-type segments, or both type
        // groups in one k_bmd2 launch (launch_bmm_qkv2) on the matrix cores
        const Seg qkv[3] = {seg_of(m, L.wq, 0), seg_of(m, L.wk, QD), seg_of(m, L.wv, QD + nk)};
        MVArgs grp[3];
        int first[3];
        MVArgs a = base;
        a.cols = E; a.x = c.bx; a.x_stride = E; a.nw = (const float*)(m.arena + L.attn_norm.off_a); a.eps = hp.eps;
        a.y = c.bq; a.y_stride = QD; a.kc = c.kc0 + l * kv_layer; a.vc = c.vc0 + l * kv_layer; a.rope = c.rope;
        a.head_dim = D; a.n_rot = hp.n_rot; a.n_ctx = c.n_ctx; a.nq = QD; a.nk = nk;
        const int ng = qkv_launch_groups(qkv, false, a, grp, first);
        bool done = false;
        if (ng == 2 && nt >= bmm_min_tokens() && bmm_ok(grp[0], EPI_QKV) && bmm_ok(grp[1], EPI_QKV)) {
            HIPC(launch_pf_quant(c.bx, E, grp[0].nw, hp.eps, E, 0, nt, c.baq, c.babs, c.bad, c.babf, c.stream, x86 ? 1 : 0));
            qkv_quant = true;
            const hipError_t e2 = launch_bmm_qkv2(grp[0], grp[1], nt, c.baq, c.babf, c.bad, c.stream);
            if (e2 != hipErrorNotSupported) {
                HIPC(e2);
                done = true;
            }
        }
        if (!done)
            for (int gi = 0; gi < ng; ++gi) HIPC(bmv(grp[gi], EPI_QKV, qkv_quant));
        BAttnArgs ba;
        const size_t scr = attn_scratch_floats(hp.n_head, c.n_ctx);
        for (int s = 0; s < nt; ++s) {
            AttnArgs& at = ba.a[s];
            const size_t sq = (size_t)seqs[s] * c.kv_seq_elems;
            at.q = c.bq + (size_t)s * QD; at.kc = c.kc0 + sq + l * kv_layer; at.vc = c.vc0 + sq + l * kv_layer;
            attn_bind_scratch(at, c.bscores + (size_t)s * scr, hp.n_head, c.n_ctx, false);
            at.out = c.batt + (size_t)s * QD; at.st = c.st0 + seqs[s]; at.n_ctx = c.n_ctx;
            at.scale = 1.0f / sqrtf((float)D); at.layer = l;
            at.num = m.numerics;
            at.fa = m.fa;
        }
        // every slot in one launch (generic, x86 and flash-attention kernels alike)
        HIPC(launch_battention(ba, nt, hp.n_head, hp.n_head_kv, D, kv_bound, c.stream));
        MVArgs o = base;
        o.seg[0] = seg_of(m, L.wo, 0); o.nseg = 1; o.cols = QD; o.x = c.batt; o.x_stride = QD; o.y = c.bx; o.y_stride = E;
        o.npairs = (E + 1) / 2;
        { bool q = false; HIPC(bmv(o, EPI_ADD, q)); }
        MVArgs gu = base;
        gu.seg[0] = seg_of(m, L.wg, 0); gu.seg[1] = seg_of(m, L.wu, 0); gu.nseg = 2; gu.cols = E; gu.x = c.bx; gu.x_stride = E;
        gu.nw = (const float*)(m.arena + L.ffn_norm.off_a); gu.eps = hp.eps; gu.y = c.bh; gu.y_stride = F; gu.npairs = F;
        { bool q = false; HIPC(bmv(gu, EPI_SWIGLU, q)); }
        MVArgs dn = base;
        dn.seg[0] = seg_of(m, L.wd, 0); dn.nseg = 1; dn.cols = F; dn.x = c.bh; dn.x_stride = F; dn.y = c.bx; dn.y_stride = E;
        dn.npairs = (E + 1) / 2;
        { bool q = false; HIPC(bmv(dn, EPI_ADD, q)); }
    }
    MVArgs lo = base;
    lo.seg[0] = seg_of(m, m.output, 0); lo.nseg = 1; lo.cols = E; lo.x = c.bx; lo.x_stride = E;
    lo.nw = (const float*)(m.arena + m.out_norm.off_a); lo.eps = hp.eps; lo.y = c.blogits; lo.y_stride = V;
    lo.npairs = (V + 1) / 2;
    { bool q = false; HIPC(bmv(lo, EPI_LOGITS, q)); }
    return enqueue_step_tail(c, tail, c.blogits, c.st0, c.hist0, nt, c.btseq, (size_t)c.n_ctx, err);
}

// the batched step in this model's numerics: every numerics and weight type (generic and
// x86 K-quant rows on the matrix cores from 3 tokens, the rest through k_mvn; x86 Q8_0
// rows with 4 working waves per workgroup, batch.hip mvn_work_waves).  A layer whose
// ffn_gate and ffn_up differ in type has no batched step in any numerics (bstep_run's
// error; llama_decode then steps such sequences one at a time)
bool bstep_run(Context& c, int nt, const int* seqs, int max_pos, std::string& err, int tail) {
    const HParams& hp = c.m->hp;
    if (nt < 1 || nt > kMaxBatch || c.n_seq < 2) { err = "batched step: 1..8 slots of a context with n_seq_max >= 2"; return false; }
    for (const Layer& L : c.m->layers)
        if (L.wg.type != L.wu.type) { err = "batched step: ffn_gate / ffn_up of different types"; return false; }
    if (!balloc(c, err)) return false;
    const int bucket = max_pos / 256;
    const int kv_bound = kv_bucket_bound(max_pos + 1, c.n_ctx);
    if (hp.n_head / hp.n_head_kv > 8 && (size_t)(hp.n_head / hp.n_head_kv) * kv_bound * 4 > kSplitAttnMaxLds) {
        err = "batched step: context too long for GQA groups of more than 8 heads";
        return false;
    }
    // slot -> sequence map (padded slots -> the dummy sequence n_seq)
    std::vector<int> map((size_t)kMaxBatch, c.n_seq);
    for (int s = 0; s < nt; ++s) map[(size_t)s] = seqs[s];
    if (map != c.btseq_host) {
        HIPC(hipMemcpyAsync(c.btseq, map.data(), kMaxBatch * 4, hipMemcpyHostToDevice, c.stream));
        HIPC(hipStreamSynchronize(c.stream));
        c.btseq_host = map;
    }
    if (!c.use_graphs) return bstep_enqueue(c, nt, seqs, kv_bound, err, tail);
    std::string key = std::to_string(bucket) + ":" + std::to_string(nt);
    for (int s = 0; s < nt; ++s) key += "," + std::to_string(seqs[s]);
    hipGraphExec_t ex = c.graphs.find_or_capture(
        tail, key, c.stream, [&](std::string& e) { return bstep_enqueue(c, nt, seqs, kv_bound, e, tail); }, err);
    if (!ex) return false;
    HIPC_AS("hipGraphLaunch(it->second, c.stream)", hipGraphLaunch(ex, c.stream));
    return true;
}

}  // namespace llmi
