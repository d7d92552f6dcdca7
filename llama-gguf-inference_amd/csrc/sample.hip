// sample.hip — the sampler chain on the device (gfx950): k_sample restates
// llmi/sampling.py's sample_with_uniform over a step's logits row,
//
//     penalties -> top_k -> top_p -> min_p -> temperature -> dist
//
// and leaves the chosen token in the step's argmax key slots, so the next step's k_embed /
// k_bembed and the host's key_token read it exactly as they read a greedy argmax.  One
// workgroup of kSmpThreads serves one slot; nothing waits on another workgroup, and no
// result depends on the grid.
//
//   penalties  the last min(repeat_last_n, pos + 1) tokens of hist[0 .. pos] go to LDS; the
//              first occurrence of every distinct in-range token rewrites its logit: f32
//              v <= 0 ? v * rp : v / rp, then (float)(((double)v - c * fp) - pp), numpy's
//              types line by line.  The row is LEFT PENALIZED (the next step's logits launch
//              rewrites it whole, and no llama_get_logits* row is exposed after a generate
//              call).
//   top_k      by the 64-bit argmax_key (logit descending, lower id first on ties; distinct,
//              so the selection is exact).  Rows of up to kSmpCand entries are taken whole.
//              Longer rows: a radix select on the key, 8 bits a pass from the top, narrows a
//              key prefix until the elements at or above it fit kSmpCand; those are gathered
//              into LDS.  A bitonic sort there leaves them in the host's lexsort order, and
//              the first k are the candidates.  (Logits share their leading bits: a pass keeps
//              four copies of each bin, by lane, so that equal digits collide less in LDS.)
//   top_p, min_p, temperature, dist
//              on the <= kSampleMaxTopK sorted candidates in FP64, one thread per candidate:
//              softmax as exp(x - max) / sum, prefix sums by a Hillis-Steele scan.  (The
//              host sums pairwise and scans in sequence: the roundings differ in the last
//              bits, which the decision margins of the tests bound.)
//   output     slot 0 of st->key[pos & 1] = the chosen candidate's key, slots 1 .. 63 = 0.
#include "kernels.h"
#include "sample_device.h"
#include "launch_util.h"

#include <cmath>

#include <hip/hip_runtime.h>

namespace llmi {

bool sample_rec_make(double temperature, int top_k, double top_p, double min_p, double repeat_penalty, int repeat_last_n,
                     double presence_penalty, double frequency_penalty, SampleRec& r, std::string& why) {
    const struct { const char* name; double v; } fin[] = {
        {"temperature", temperature}, {"top_p", top_p}, {"min_p", min_p}, {"repeat_penalty", repeat_penalty},
        {"presence_penalty", presence_penalty}, {"frequency_penalty", frequency_penalty}};
    for (const auto& f : fin)
        if (!std::isfinite(f.v)) { why = std::string(f.name) + " is not finite"; return false; }
    if (top_k < 1 || top_k > kSampleMaxTopK) {
        why = "top_k " + std::to_string(top_k) + " outside 1.." + std::to_string(kSampleMaxTopK);
        return false;
    }
    if (repeat_last_n < 0 || repeat_last_n > kSampleMaxLastN) {
        why = "repeat_last_n " + std::to_string(repeat_last_n) + " outside 0.." + std::to_string(kSampleMaxLastN);
        return false;
    }
    r = SampleRec();
    r.temperature = temperature; r.top_p = top_p; r.min_p = min_p; r.repeat_penalty = repeat_penalty;
    r.presence_penalty = presence_penalty; r.frequency_penalty = frequency_penalty;
    r.top_k = top_k; r.repeat_last_n = repeat_last_n;
    r.penalized = repeat_penalty != 1.0 || presence_penalty != 0.0 || frequency_penalty != 0.0;
    r.mode = (temperature <= 0.0 || top_k == 1) && !r.penalized ? SAMPLE_GREEDY
             : temperature <= 0.0                               ? SAMPLE_ARGMAX
                                                                : SAMPLE_DIST;
    return true;
}

namespace {

struct SmpLds {
    SelLds sel;                        // the select's bins and the gathered keys, sorted descending
    unsigned long long red[kSmpWaves];
    double x[kSampleMaxTopK];          // candidate logits (/ temperature in the last softmax)
    double s[2][kSampleMaxTopK];       // scan ping-pong; s[cur][i] = inclusive prefix sum
    double dred[kSmpWaves];
    int32_t win[kSampleMaxLastN];
    int idx;
};

// softmax of L.x[0 .. n) (sorted descending: the max is x[0]) and its inclusive prefix sums
// L.s[ret][0 .. n); returns the scan buffer.  Every thread calls it; `total` = the sum.
__device__ int softmax_scan(SmpLds& L, int n, double& pr_self, double& total) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double e = t < n ? exp(L.x[t] - L.x[0]) : 0.0;
    const double ws = wave_sum_f64(e);
    __syncthreads();
    if (lane == 0) L.dred[wave] = ws;
    __syncthreads();
    double sum = 0.0;
    for (int w = 0; w < (kSampleMaxTopK + 63) / 64; ++w) sum += L.dred[w];
    const double pr = e / sum;
    pr_self = pr;
    int cur = 0;
    if (t < kSampleMaxTopK) L.s[0][t] = pr;
    __syncthreads();
    for (int o = 1; o < kSampleMaxTopK; o <<= 1) {
        if (t < kSampleMaxTopK) L.s[cur ^ 1][t] = t >= o ? L.s[cur][t - o] + L.s[cur][t] : L.s[cur][t];
        cur ^= 1;
        __syncthreads();
    }
    total = L.s[cur][n - 1];
    return cur;
}

// smallest t in [0, n) whose thread passes hit, else n (block-wide; L.idx)
__device__ int first_hit(SmpLds& L, int n, bool hit) {
    __syncthreads();
    if (threadIdx.x == 0) L.idx = n;
    __syncthreads();
    if ((int)threadIdx.x < n && hit) atomicMin(&L.idx, (int)threadIdx.x);
    __syncthreads();
    return L.idx;
}

}  // namespace

__global__ __launch_bounds__(kSmpThreads) void k_sample(SampleArgs a) {
    const int slot = blockIdx.x;
    const SampleRec R = a.rec[slot];
    if (R.mode == SAMPLE_GREEDY) return;
    __shared__ SmpLds L;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int seq = a.tseq ? a.tseq[slot] : slot;
    StepState* st = a.st + seq;
    const int32_t* hist = a.hist + (size_t)seq * a.hist_stride;
    float* lg = a.logits + (size_t)slot * a.V;
    const int V = a.V, pos = st->pos;

    // ---- penalties ----
    if (R.penalized) {
        const int n = min(R.repeat_last_n, pos + 1);
        if (t < n) L.win[t] = hist[pos + 1 - n + t];
        __syncthreads();
        if (t < n) {
            const int tok = L.win[t];
            bool first = tok >= 0 && tok < V;
            int c = 0;
            for (int j = 0; j < n; ++j) {
                const bool eq = L.win[j] == tok;
                c += eq;
                first = first && !(eq && j < t);
            }
            if (first) {
                const float v = lg[tok];
                const float v32 = v <= 0.f ? v * (float)R.repeat_penalty : v / (float)R.repeat_penalty;
                lg[tok] = (float)(((double)v32 - (double)c * R.frequency_penalty) - R.presence_penalty);
            }
        }
        __syncthreads();  // the penalized row is read below by every thread
    }

    unsigned long long chosen = 0;
    int n_final = 1;
    if (R.mode == SAMPLE_ARGMAX) {
        unsigned long long best = 0;
        for_row(lg, V, [&](float v, int i) {
            const unsigned long long k = argmax_key(v, i);
            best = k > best ? k : best;
        });
        best = wave_max_u64(best);
        if (lane == 0) L.red[wave] = best;
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < kSmpWaves; ++w) best = L.red[w] > best ? L.red[w] : best;
            L.sel.key[0] = best;
        }
        __syncthreads();
        chosen = L.sel.key[0];
    } else {
        // ---- top_k: the elements whose key is >= a prefix, at most kSmpCand of them, into LDS ----
        const int k = min(R.top_k, V);
        const auto nothing = [](float, int) {};
        const unsigned long long prefix = V > kSmpCand ? select_prefix(L.sel, lg, V, k, nothing) : 0ull;
        gather_sort(L.sel, lg, V, prefix, nothing);
        // ---- top_p, min_p, temperature, dist on the first k, FP64 ----
        int n = k;
        if (t < kSampleMaxTopK) {
            double x = 0.0;
            const uint32_t id = 0xffffffffu - (uint32_t)(L.sel.key[t] & 0xffffffffull);
            if (t < n && id < (uint32_t)V) x = (double)lg[id];
            L.x[t] = x;
        }
        __syncthreads();
        double pr, total;
        if (R.top_p < 1.0) {
            const int cur = softmax_scan(L, n, pr, total);
            const int at = first_hit(L, n, t < n && L.s[cur][t] >= R.top_p);
            n = max(1, min(at + 1, n));
        }
        if (R.min_p > 0.0 && n > 1) {
            softmax_scan(L, n, pr, total);
            __syncthreads();
            if (t == 0) L.s[0][0] = pr;
            __syncthreads();
            const double thr = R.min_p * L.s[0][0];
            // the candidates are sorted, so the kept ones are a prefix; candidate 0 always stays
            n = first_hit(L, n, t > 0 && !(pr >= thr));
        }
        __syncthreads();
        if (t < n) L.x[t] = L.x[t] / R.temperature;
        __syncthreads();
        const int cur = softmax_scan(L, n, pr, total);
        const int idx = pos - R.pos0;
        const double u = idx >= 0 && idx < R.n_uni ? R.uni[idx] : 0.0;
        const int pick = first_hit(L, n, t < n && L.s[cur][t] / total > u);
        chosen = L.sel.key[min(pick, n - 1)];
        n_final = n;
    }
    if (a.cand) {
        if (t < n_final)
            a.cand[(size_t)slot * kSampleMaxTopK + t] =
                (int32_t)(0xffffffffu - (uint32_t)((R.mode == SAMPLE_ARGMAX ? chosen : L.sel.key[t]) & 0xffffffffull));
        if (t == 0) a.n_cand[slot] = n_final;
    }
    if (t < kArgSlots) st->key[pos & 1][t] = t == 0 ? chosen : 0ull;
}

hipError_t launch_sample(const SampleArgs& a, int slots, hipStream_t s) {
    if (slots < 1 || slots > kMaxBatch || a.V < 1 || !a.logits || !a.st || !a.rec) return hipErrorInvalidValue;
    launch_k(k_sample, dim3(slots), dim3(kSmpThreads), 0, s, true, true, a);
    return hipGetLastError();
}

}  // namespace llmi
