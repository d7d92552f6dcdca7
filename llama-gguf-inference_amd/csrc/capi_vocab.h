// capi_vocab.h — what the host-only part of the C ABI (capi_host.cpp) shares with the
// device-side units: the vocab handle, the error slot, the exception fence.  No HIP here.
#pragma once

#include <cstdint>
#include <memory>
#include <new>
#include <string>

#include "tokenizer.h"

// Self-contained: a model's handle is a member of its llama_model (valid on any thread
// until llama_model_free), a file handle (llmi_vocab_load_from_file) owns its tokenizer.
struct llama_vocab {
    const llmi::Tokenizer* tok = nullptr;
    int32_t n_vocab = 0;                       // llama_vocab_n_tokens
    std::unique_ptr<llmi::Tokenizer> owned;    // file handles only
};

namespace llmi {
void set_err(const std::string& e);  // this thread's llmi_last_error() (capi_host.cpp)
}

#define API_TRY try {
#define API_CATCH(ret)                                   \
    }                                                    \
    catch (const std::bad_alloc&) {                      \
        set_err("out of host memory");                   \
        return ret;                                      \
    }                                                    \
    catch (...) {                                        \
        set_err("internal error");                       \
        return ret;                                      \
    }
