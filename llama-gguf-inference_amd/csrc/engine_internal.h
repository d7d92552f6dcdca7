// engine_internal.h — shared by the engine units (model.cpp, context.cpp, decode_step.cpp,
// prefill_step.cpp) only.
#pragma once

#include "engine.h"

// In a function returning bool with a std::string& err: a failed HIP call leaves
// "<what>: <error>" in err and returns false.  HIPC names the call by its own text.
#define HIPC_AS(what, expr)                                                \
    do {                                                                   \
        hipError_t e_ = (expr);                                            \
        if (e_ != hipSuccess) {                                            \
            err = std::string(what) + ": " + hip_err(e_);                  \
            return false;                                                  \
        }                                                                  \
    } while (0)
#define HIPC(expr) HIPC_AS(#expr, expr)
