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
#include "mv_device.h"
#include "launch_util.h"

#include <cmath>

#include <hip/hip_runtime.h>

namespace llmi {

constexpr int kSmpThreads = 1024;
constexpr int kSmpWaves = kSmpThreads / 64;
constexpr int kSmpUnroll = 4;    // 16-byte row loads a thread has in flight before it uses the first
constexpr int kSmpCand = 1024;  // keys gathered into LDS for the sort (>= kSampleMaxTopK, a power of two)
static_assert(kSmpCand >= kSampleMaxTopK && (kSmpCand & (kSmpCand - 1)) == 0, "sort space");
static_assert(kSmpThreads == 4 * 256, "one thread per radix bin copy");
static_assert(kSmpCand <= kSmpThreads && kSampleMaxLastN <= kSmpThreads && kSampleMaxTopK <= kSmpThreads, "one thread each");

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
    unsigned long long key[kSmpCand];  // gathered keys, sorted descending
    unsigned long long red[kSmpWaves];
    double x[kSampleMaxTopK];          // candidate logits (/ temperature in the last softmax)
    double s[2][kSampleMaxTopK];       // scan ping-pong; s[cur][i] = inclusive prefix sum
    double dred[kSmpWaves];
    int32_t win[kSampleMaxLastN];
    unsigned bins[4 * 256];            // radix bins, four copies each (lane & 3): equal digits collide less
    unsigned hist[2][256];             // their sums, suffix-scan ping-pong
    unsigned long long prefix;
    unsigned need, n_ge, n_key;
    int idx;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// f(value, index) for every element of the row, each by one thread of the workgroup.  The
// body of the row goes in 16-byte loads, kSmpUnroll of them in flight per thread before the
// first is used (a row starts wherever slot * V puts it: the elements before the first
// 16-byte boundary and after the last whole quad go singly).
template <class F>
__device__ __forceinline__ void for_row(const float* lg, int V, F f) {
    const int t = threadIdx.x;
    const int head = min(V, (int)(((16u - (unsigned)((uintptr_t)lg & 15u)) & 15u) >> 2));
    const int n4 = (V - head) >> 2;
    const float4* q = (const float4*)(lg + head);
    if (t < head) f(lg[t], t);
    for (int i0 = 0; i0 < n4; i0 += kSmpUnroll * kSmpThreads) {
        float4 v[kSmpUnroll];
#pragma unroll
        for (int j = 0; j < kSmpUnroll; ++j) {
            const int i = i0 + j * kSmpThreads + t;
            if (i < n4) v[j] = q[i];
        }
#pragma unroll
        for (int j = 0; j < kSmpUnroll; ++j) {
            const int i = i0 + j * kSmpThreads + t;
            if (i < n4) {
                const int e = head + 4 * i;
                f(v[j].x, e); f(v[j].y, e + 1); f(v[j].z, e + 2); f(v[j].w, e + 3);
            }
        }
    }
    const int e = head + 4 * n4 + t;
    if (e < V) f(lg[e], e);
}

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
            L.key[0] = best;
        }
        __syncthreads();
        chosen = L.key[0];
    } else {
        // ---- top_k: the elements whose key is >= a prefix, at most kSmpCand of them, into LDS ----
        const int k = min(R.top_k, V);
        unsigned long long prefix = 0;
        if (V > kSmpCand) {
            unsigned need = (unsigned)k;  // candidates still to take from the elements matching the prefix
            for (int shift = 56; shift >= 0; shift -= 8) {
                L.bins[t] = 0;
                __syncthreads();
                for_row(lg, V, [&](float v, int i) {
                    const unsigned long long key = argmax_key(v, i);
                    if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8)))
                        atomicAdd(&L.bins[(((unsigned)(key >> shift) & 255u) << 2) | (unsigned)(lane & 3)], 1u);
                });
                __syncthreads();
                if (t < 256) L.hist[0][t] = L.bins[4 * t] + L.bins[4 * t + 1] + L.bins[4 * t + 2] + L.bins[4 * t + 3];
                __syncthreads();
                // suffix sums: hist[cur][b] = elements in bins >= b
                int cur = 0;
                for (int o = 1; o < 256; o <<= 1) {
                    if (t < 256) L.hist[cur ^ 1][t] = L.hist[cur][t] + (t + o < 256 ? L.hist[cur][t + o] : 0u);
                    cur ^= 1;
                    __syncthreads();
                }
                if (t < 256) {
                    const unsigned ge = L.hist[cur][t], gt = t < 255 ? L.hist[cur][t + 1] : 0u;
                    if (gt < need && need <= ge) {  // exactly one bin: the k-th largest key lies in it
                        L.prefix = prefix | ((unsigned long long)t << shift);
                        L.need = need - gt;
                        L.n_ge = (unsigned)k - need + ge;  // elements with key >= the new prefix
                    }
                }
                __syncthreads();
                prefix = L.prefix;
                need = L.need;
                const unsigned n_ge = L.n_ge;
                __syncthreads();
                if (n_ge <= (unsigned)kSmpCand) break;  // at the last pass need == 1 and n_ge == k
            }
        }
        if (t == 0) L.n_key = 0;
        if (t < kSmpCand) L.key[t] = 0;
        __syncthreads();
        for_row(lg, V, [&](float v, int i) {
            const unsigned long long key = argmax_key(v, i);
            if (key >= prefix) {
                const unsigned at = atomicAdd(&L.n_key, 1u);
                if (at < (unsigned)kSmpCand) L.key[at] = key;
            }
        });
        __syncthreads();
        const int n_key = min((int)L.n_key, kSmpCand);
        int n_sort = 64;
        while (n_sort < n_key) n_sort <<= 1;
        // bitonic sort, descending (the unused tail holds 0, below every key of a real logit)
        for (int kk = 2; kk <= n_sort; kk <<= 1) {
            for (int j = kk >> 1; j > 0; j >>= 1) {
                const int p = t ^ j;
                if (t < n_sort && p > t) {
                    const unsigned long long x = L.key[t], y = L.key[p];
                    const bool desc = (t & kk) == 0;
                    if (desc ? x < y : x > y) { L.key[t] = y; L.key[p] = x; }
                }
                __syncthreads();
            }
        }
        // ---- top_p, min_p, temperature, dist on the first k, FP64 ----
        int n = k;
        if (t < kSampleMaxTopK) {
            double x = 0.0;
            const uint32_t id = 0xffffffffu - (uint32_t)(L.key[t] & 0xffffffffull);
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
        chosen = L.key[min(pick, n - 1)];
        n_final = n;
    }
    if (a.cand) {
        if (t < n_final)
            a.cand[(size_t)slot * kSampleMaxTopK + t] =
                (int32_t)(0xffffffffu - (uint32_t)((R.mode == SAMPLE_ARGMAX ? chosen : L.key[t]) & 0xffffffffull));
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
