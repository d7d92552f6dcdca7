// capi_internal.h — the handle types behind include/llmi.h, shared by capi.cpp,
// capi_fanout.cpp and capi_hooks.cpp.
#pragma once

#include <memory>
#include <vector>

#include "capi_vocab.h"
#include "engine.h"

struct llama_model {
    llmi::Model m;
    llama_vocab vocab;              // llama_model_get_vocab: lives exactly as long as the model
};
struct llama_context {
    llmi::Context c;
    llama_model* owner;
    uint8_t* outs = nullptr;        // device copies of flagged logits rows [cap][n_vocab]
    int outs_cap = 0;
    std::vector<char> host_valid;   // per output row: logits_host filled
    unsigned long long* keys_pinned = nullptr;  // per output row argmax key (pinned host)
    int keys_cap = 0;
    // the embeddings of the last llama_decode (capi_embd.cpp's getters), host memory
    int embd_call = -2;             // that call's pooling type; -2: it produced no embeddings
    int embd_rows = 0;              // pooling NONE: the call's tokens
    std::vector<float> embd_host;   // NONE: [embd_rows][n_embd] in batch order; else [n_seq][n_embd]
    std::vector<float> embd_stage;  // NONE: the rows as the device wrote them, sequence by sequence
    std::vector<char> embd_seq_ok;  // pooled: the sequence had tokens in the call
};

namespace llmi {
// A llama_model whose Model `load` fills (model_load / model_clone_layout; false: failed),
// its vocab handle bound to the loaded tokenizer.  Null when load fails.
template <class Load>
llama_model* make_model(Load load) {
    auto m = std::make_unique<llama_model>();
    if (!load(m->m)) return nullptr;
    m->vocab.tok = m->m.tok.get();
    m->vocab.n_vocab = m->m.hp.n_vocab;
    return m.release();
}
}  // namespace llmi
