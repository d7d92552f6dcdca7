// capi_embd.cpp — the embeddings surface of include/llmi.h: upstream's llama_set_embeddings,
// llama_pooling_type and llama_get_embeddings*, and llmi's setter for what upstream keeps in
// the context params.  llama_decode (capi.cpp) fills what the getters hand out.
#include <string>

#include "../../include/llmi.h"
#include "capi_internal.h"

using namespace llmi;

namespace {
// the context's embeddings of the last llama_decode, or null with the error set
llama_context* embd_ready(const char* who, llama_context* ctx, bool want_none) {
    const std::string name = std::string(who) + ": ";
    if (!ctx) { set_err(name + "ctx is a null pointer"); return nullptr; }
    const Context& c = ctx->c;
    if (!c.embd_on) { set_err(name + "embeddings are off (llama_set_embeddings)"); return nullptr; }
    if (want_none && c.pooling != POOLING_NONE) {
        set_err(name + "the context pools its embeddings (pooling type " + std::to_string(c.pooling) +
                "): llama_get_embeddings_seq has them");
        return nullptr;
    }
    if (!want_none && c.pooling == POOLING_NONE) {
        set_err(name + "pooling type is none: llama_get_embeddings_ith has the token rows");
        return nullptr;
    }
    if (ctx->embd_call != c.pooling) { set_err(name + "the last llama_decode produced no such embeddings"); return nullptr; }
    return ctx;
}
}  // namespace

extern "C" {

void llama_set_embeddings(struct llama_context* ctx, bool embeddings) {
    if (!ctx) { set_err("llama_set_embeddings: ctx is a null pointer"); return; }
    ctx->c.embd_on = embeddings;
    if (!embeddings) ctx->embd_call = -2;
}

int32_t llmi_set_pooling_type(struct llama_context* ctx, int32_t type) {
    const std::string who = "llmi_set_pooling_type: ";
    // (the value first: a refusal of it needs no context)
    if (type == POOLING_RANK) { set_err(who + "type 4 (rank) is not supported"); return -1; }
    if (type < POOLING_NONE || type > POOLING_LAST) {
        set_err(who + "type " + std::to_string(type) + " is not a pooling type (0 none, 1 mean, 2 cls, 3 last)");
        return -1;
    }
    if (!ctx) { set_err(who + "ctx is a null pointer"); return -1; }
    if (type != ctx->c.pooling) ctx->embd_call = -2;  // the last call's results are of another kind
    ctx->c.pooling = type;
    return 0;
}

int32_t llama_pooling_type(const struct llama_context* ctx) {
    if (!ctx) { set_err("llama_pooling_type: ctx is a null pointer"); return POOLING_UNSPECIFIED; }
    return ctx->c.pooling;
}

int32_t llmi_model_pooling_type(const struct llama_model* model) {
    if (!model) { set_err("llmi_model_pooling_type: model is a null pointer"); return -1; }
    return model->m.hp.pooling_type;
}

float* llama_get_embeddings_seq(struct llama_context* ctx, llama_seq_id seq_id) {
    API_TRY
    if (!embd_ready("llama_get_embeddings_seq", ctx, false)) return nullptr;
    if (seq_id < 0 || seq_id >= ctx->c.n_seq || !ctx->embd_seq_ok[(size_t)seq_id]) {
        set_err("llama_get_embeddings_seq: seq_id " + std::to_string(seq_id) + " had no token in the last llama_decode");
        return nullptr;
    }
    return ctx->embd_host.data() + (size_t)seq_id * ctx->c.m->hp.n_embd;
    API_CATCH(nullptr)
}

float* llama_get_embeddings_ith(struct llama_context* ctx, int32_t i) {
    API_TRY
    if (!embd_ready("llama_get_embeddings_ith", ctx, true)) return nullptr;
    if (i < 0) i = i == -1 ? ctx->embd_rows - 1 : ctx->embd_rows;
    if (i >= ctx->embd_rows) { set_err("llama_get_embeddings_ith: i outside the last batch"); return nullptr; }
    return ctx->embd_host.data() + (size_t)i * ctx->c.m->hp.n_embd;
    API_CATCH(nullptr)
}

float* llama_get_embeddings(struct llama_context* ctx) {
    if (!embd_ready("llama_get_embeddings", ctx, true)) return nullptr;
    return ctx->embd_host.data();
}

}  // extern "C"
