// logprob.hip — token log-probabilities on the device (gfx950): llmi/sampling.py's
// token_logprobs over a step's raw logits row, next to the sampler (sample.hip).
//
//   k_logprob       one workgroup of kSmpThreads per slot, after the logits launch and BEFORE
//                   k_sample; it writes nothing into the row or the key slots.
//     window        the slot's penalty window (its SampleRec's, the tokens k_sample is about
//                   to rewrite) and the raw logits of its tokens go to a per-slot scratch.
//     pass 1        the row maximum (as an argmax_key) and, for rows longer than kSmpCand, the
//                   first histogram of the radix select, in one walk of the row; the select's
//                   further passes narrow the key prefix (sample_device.h).
//     pass 2        S = sum exp((double)x - (double)m) in FP64, one partial per thread, and
//                   the gather of the keys at or above the prefix, in one walk.
//     sort, output  the bitonic sort leaves the keys in the host's lexsort order; lse = m +
//                   log(S); alternative t < n_top: id and (double)logit - lse from its key,
//                   the rest id -1 and -inf.  Never log(p): a token more than 745 below the
//                   maximum keeps a finite value.
//   k_logprob_pick  one wave per slot, after k_sample (or after k_logprob in a step without
//                   sampled slots): the step's token by key_token's rule, its raw logit from
//                   the saved window if k_sample penalized it, else from the row;
//                   tok_logprob = raw - lse.
#include "kernels.h"
#include "sample_device.h"
#include "launch_util.h"

#include <cmath>

#include <hip/hip_runtime.h>

namespace llmi {

namespace {

struct LpLds {
    SelLds sel;
    unsigned long long red[kSmpWaves];
    double dred[kSmpWaves];
    unsigned long long best;
    double lse;
};

}  // namespace

__global__ __launch_bounds__(kSmpThreads) void k_logprob(LogprobArgs a) {
    const int slot = blockIdx.x;
    const LogprobRec R = a.lrec[slot];
    if (R.n_top < 0) return;
    __shared__ LpLds L;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int seq = a.tseq ? a.tseq[slot] : slot;
    const StepState* st = a.st + seq;
    const int32_t* hist = a.hist + (size_t)seq * a.hist_stride;
    const float* lg = a.logits + (size_t)slot * a.V;
    const int V = a.V, pos = st->pos;
    const int idx = pos - R.pos0;
    if (idx < 0 || idx >= R.n_step) return;

    // ---- the penalty window's raw logits, before k_sample rewrites them ----
    if (t < kSampleMaxLastN) {
        const SampleRec* sr = a.rec + slot;
        const int n = sr->mode != SAMPLE_GREEDY && sr->penalized ? min(sr->repeat_last_n, pos + 1) : 0;
        int tok = -1;
        float raw = 0.f;
        if (t < n) {
            tok = hist[pos + 1 - n + t];
            if (tok >= 0 && tok < V) raw = lg[tok];
            else tok = -1;
        }
        R.win_tok[t] = tok;
        R.win_raw[t] = raw;
    }

    // ---- pass 1: the maximum, with the select's first histogram ----
    const int k = min(R.n_top, V);
    unsigned long long best = 0, prefix = 0;
    const auto fold_max = [&](float v, int i) {
        const unsigned long long key = argmax_key(v, i);
        best = key > best ? key : best;
    };
    if (k > 0 && V > kSmpCand) prefix = select_prefix(L.sel, lg, V, k, fold_max);
    else for_row(lg, V, fold_max);
    best = wave_max_u64(best);
    if (lane == 0) L.red[wave] = best;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kSmpWaves; ++w) best = L.red[w] > best ? L.red[w] : best;
        L.best = best;
    }
    __syncthreads();
    const double m = (double)key_value(L.best);

    // ---- pass 2: the FP64 sum, with the gather ----
    double part = 0.0;
    const auto fold_sum = [&](float v, int) { part += exp((double)v - m); };
    if (k > 0) gather_sort(L.sel, lg, V, prefix, fold_sum);
    else for_row(lg, V, fold_sum);
    part = wave_sum_f64(part);
    if (lane == 0) L.dred[wave] = part;
    __syncthreads();
    if (t == 0) {
        double S = 0.0;
        for (int w = 0; w < kSmpWaves; ++w) S += L.dred[w];
        L.lse = m + log(S);
        R.lse[idx] = L.lse;
    }
    __syncthreads();
    if (t < kLogprobMaxTop) {
        int32_t id = -1;
        double lp = -INFINITY;
        if (t < k) {
            const unsigned long long key = L.sel.key[t];
            id = (int32_t)key_id(key);
            lp = (double)key_value(key) - L.lse;
        }
        R.top_id[(size_t)idx * kLogprobMaxTop + t] = id;
        R.top_lp[(size_t)idx * kLogprobMaxTop + t] = lp;
    }
}

__global__ __launch_bounds__(64) void k_logprob_pick(LogprobArgs a) {
    const int slot = blockIdx.x;
    const LogprobRec R = a.lrec[slot];
    if (R.n_top < 0) return;
    const int lane = threadIdx.x;
    const int seq = a.tseq ? a.tseq[slot] : slot;
    const StepState* st = a.st + seq;
    const float* lg = a.logits + (size_t)slot * a.V;
    const int pos = st->pos;
    const int idx = pos - R.pos0;
    if (idx < 0 || idx >= R.n_step) return;
    static_assert(kArgSlots == 64, "one lane per key slot");
    const unsigned long long key = wave_max_u64(st->key[pos & 1][lane]);
    const uint32_t tok = key_id(key);
    double lp = -INFINITY;  // (a token outside the row: no step leaves one)
    if (tok < (uint32_t)a.V) {
        float raw = lg[tok];
        for (int j0 = 0; j0 < kSampleMaxLastN; j0 += 64) {
            const unsigned long long hit = __ballot(R.win_tok[j0 + lane] == (int32_t)tok);
            if (hit) {  // every occurrence saved the same raw value
                raw = R.win_raw[j0 + __ffsll((long long)hit) - 1];
                break;
            }
        }
        lp = (double)raw - R.lse[idx];
    }
    if (lane == 0) R.tok_lp[idx] = lp;
}

static bool logprob_args_ok(const LogprobArgs& a, int slots) {
    return slots >= 1 && slots <= kMaxBatch && a.V >= 1 && a.logits && a.st && a.rec && a.lrec && a.hist;
}

hipError_t launch_logprob(const LogprobArgs& a, int slots, hipStream_t s) {
    if (!logprob_args_ok(a, slots)) return hipErrorInvalidValue;
    launch_k(k_logprob, dim3(slots), dim3(kSmpThreads), 0, s, true, true, a);
    return hipGetLastError();
}

hipError_t launch_logprob_pick(const LogprobArgs& a, int slots, hipStream_t s) {
    if (!logprob_args_ok(a, slots)) return hipErrorInvalidValue;
    launch_k(k_logprob_pick, dim3(slots), dim3(64), 0, s, true, true, a);
    return hipGetLastError();
}

}  // namespace llmi
