// capi_host.cpp — the host-only part of the C ABI (include/llmi.h): the thread-local
// llmi_last_error(), the vocab / tokenizer entry points and the synthetic GGUF writer.
// No HIP, RCCL or engine header: this unit also builds with the plain host compiler
// (make hostcheck runs it under the address and undefined-behaviour sanitizers).
#include <climits>
#include <cstdint>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "../../include/llmi.h"
#include "capi_vocab.h"
#include "gguf.h"

using namespace llmi;

namespace {
thread_local std::string g_err;
}
void llmi::set_err(const std::string& e) { g_err = e; }

extern "C" {

const char* llmi_last_error(void) { return g_err.c_str(); }

int32_t llama_vocab_n_tokens(const struct llama_vocab* v) { return v ? v->n_vocab : 0; }
llama_token llama_vocab_bos(const struct llama_vocab* v) { return v ? v->tok->bos : -1; }
llama_token llama_vocab_eos(const struct llama_vocab* v) { return v ? v->tok->eos : -1; }
const char* llama_vocab_get_text(const struct llama_vocab* v, llama_token t) {
    if (!v || t < 0 || t >= (int)v->tok->tokens.size()) return nullptr;
    return v->tok->tokens[(size_t)t].c_str();
}
bool llama_vocab_get_add_bos(const struct llama_vocab* v) { return v && v->tok->add_bos; }

// upstream llama_tokenize: the count, or -(count) when n_tokens_max is too small
int32_t llama_tokenize(const struct llama_vocab* v, const char* text, int32_t text_len, llama_token* tokens,
                       int32_t n_tokens_max, bool add_special, bool parse_special) {
    if (!v || (!text && text_len > 0) || text_len < 0) {
        set_err("llama_tokenize: bad arguments");
        return INT32_MIN;
    }
    try {
        const std::vector<int32_t> ids = v->tok->tokenize(std::string(text ? text : "", (size_t)text_len), add_special,
                                                          parse_special);
        if ((int64_t)ids.size() > (int64_t)INT32_MAX) {
            set_err("llama_tokenize: too many tokens");
            return INT32_MIN;
        }
        const int32_t n = (int32_t)ids.size();
        if (n > n_tokens_max) return -n;
        for (int32_t i = 0; i < n; ++i) tokens[i] = ids[(size_t)i];
        return n;
    } catch (const std::exception& e) {
        set_err(std::string("llama_tokenize: ") + e.what());
        return INT32_MIN;
    }
}

// upstream llama_token_to_piece: bytes written (no NUL), or -(bytes needed); up to
// lstrip leading spaces are skipped; special renders CONTROL tokens as their text
int32_t llama_token_to_piece(const struct llama_vocab* v, llama_token token, char* buf, int32_t length, int32_t lstrip,
                             bool special) {
    if (!v) return 0;
    API_TRY
    std::string p = v->tok->piece(token, special);
    size_t k = 0;
    while (lstrip > 0 && k < p.size() && p[k] == ' ') {
        ++k;
        --lstrip;
    }
    const int32_t n = (int32_t)(p.size() - k);
    if (n > length) return -n;
    if (n > 0) memcpy(buf, p.data() + k, (size_t)n);
    return n;
    API_CATCH(INT32_MIN)
}

// upstream llama_detokenize: the pieces concatenated; remove_special drops a leading BOS
// (when the vocabulary adds one) and a trailing EOS (when it adds one: add_eos_token);
// unparse_special renders CONTROL text.
// Bytes written, or -(bytes needed).
int32_t llama_detokenize(const struct llama_vocab* v, const llama_token* tokens, int32_t n_tokens, char* text,
                         int32_t text_len_max, bool remove_special, bool unparse_special) {
    if (!v || n_tokens < 0 || (!tokens && n_tokens > 0)) return INT32_MIN;
    API_TRY
    int32_t b = 0, e = n_tokens;
    if (remove_special && e > b && v->tok->add_bos && tokens[b] == v->tok->bos) ++b;
    if (remove_special && e > b && v->tok->add_eos && tokens[e - 1] == v->tok->eos) --e;
    std::string out;
    for (int32_t i = b; i < e; ++i) out += v->tok->piece(tokens[i], unparse_special);
    if ((int64_t)out.size() > (int64_t)text_len_max) return -(int32_t)out.size();
    if (!out.empty()) memcpy(text, out.data(), out.size());
    return (int32_t)out.size();
    API_CATCH(INT32_MIN)
}

// a tokenizer-only handle from a GGUF's metadata (no tensors needed)
struct llama_vocab* llmi_vocab_load_from_file(const char* path) {
    API_TRY
    GgufFile f;
    std::string err;
    if (!path || !f.open(path, err)) {
        set_err(err.empty() ? "llmi_vocab_load_from_file: no path" : err);
        return nullptr;
    }
    const GgufTensor* te = f.tensor("token_embd.weight");
    auto v = std::make_unique<llama_vocab>();
    v->owned = Tokenizer::from_gguf(f, te ? (int)te->ne[1] : 0);
    v->tok = v->owned.get();
    v->n_vocab = (int32_t)v->tok->tokens.size();
    return v.release();
    API_CATCH(nullptr)
}
void llmi_vocab_free(struct llama_vocab* v) {
    if (v && v->owned) delete v;
}

int64_t llmi_synth_write_gguf(const char* path, const char* preset, uint64_t seed, int32_t n_layer, int32_t n_vocab,
                              int32_t n_threads) {
    API_TRY
    if (!path || !preset) { set_err("null argument"); return -1; }
    std::string err;
    int64_t r = synth_write_gguf(path, preset, seed, n_layer, n_vocab, n_threads, err);
    if (r < 0) set_err(err);
    return r;
    API_CATCH(-1)
}

}  // extern "C"
