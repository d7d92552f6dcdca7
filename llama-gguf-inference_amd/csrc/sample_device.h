// sample_device.h — what k_sample (sample.hip) and k_logprob (logprob.hip) share: the row
// walk in 16-byte loads, the radix select on the 64-bit argmax_key, the gather of the
// selected keys into LDS and the bitonic sort that leaves them in the host's lexsort order
// (logit descending, lower id first on ties).  One workgroup of kSmpThreads serves one row.
#pragma once
#include "kernels.h"
#include "mv_device.h"

#include <hip/hip_runtime.h>

namespace llmi {

constexpr int kSmpThreads = 1024;
constexpr int kSmpWaves = kSmpThreads / 64;
constexpr int kSmpUnroll = 4;    // 16-byte row loads a thread has in flight before it uses the first
constexpr int kSmpCand = 1024;  // keys gathered into LDS for the sort (>= kSampleMaxTopK, a power of two)
static_assert(kSmpCand >= kSampleMaxTopK && (kSmpCand & (kSmpCand - 1)) == 0, "sort space");
static_assert(kSmpThreads == 4 * 256, "one thread per radix bin copy");
static_assert(kSmpCand <= kSmpThreads && kSampleMaxLastN <= kSmpThreads && kSampleMaxTopK <= kSmpThreads, "one thread each");
static_assert(kLogprobMaxTop <= kSmpCand, "the alternatives come out of the same sort");

// the select's LDS: a member of each kernel's own shared struct
struct SelLds {
    unsigned long long key[kSmpCand];  // gathered keys, sorted descending
    unsigned bins[4 * 256];            // radix bins, four copies each (lane & 3): equal digits collide less
    unsigned hist[2][256];             // their sums, suffix-scan ping-pong
    unsigned long long prefix;
    unsigned need, n_ge, n_key;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the logit an argmax_key was made of (-0 comes back as +0)
__device__ __forceinline__ float key_value(unsigned long long key) {
    const uint32_t u = (uint32_t)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ uint32_t key_id(unsigned long long key) { return 0xffffffffu - (uint32_t)(key & 0xffffffffull); }

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

// Radix select on the key, 8 bits a pass from the top: narrows a key prefix until the
// elements at or above it (the k largest among them, 1 <= k <= V) fit kSmpCand, and returns
// it.  For rows longer than kSmpCand (a shorter row is gathered whole, prefix 0).  The first
// pass also calls first(value, index) for every element: a caller's own fold over the row
// rides on it.  Every thread calls this; ends on a barrier.
template <class G>
__device__ __forceinline__ unsigned long long select_prefix(SelLds& S, const float* lg, int V, int k, G first) {
    const int t = threadIdx.x, lane = t & 63;
    unsigned long long prefix = 0;
    unsigned need = (unsigned)k;  // candidates still to take from the elements matching the prefix
    for (int shift = 56; shift >= 0; shift -= 8) {
        S.bins[t] = 0;
        __syncthreads();
        for_row(lg, V, [&](float v, int i) {
            const unsigned long long key = argmax_key(v, i);
            if (shift == 56) first(v, i);
            if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8)))
                atomicAdd(&S.bins[(((unsigned)(key >> shift) & 255u) << 2) | (unsigned)(lane & 3)], 1u);
        });
        __syncthreads();
        if (t < 256) S.hist[0][t] = S.bins[4 * t] + S.bins[4 * t + 1] + S.bins[4 * t + 2] + S.bins[4 * t + 3];
        __syncthreads();
        // suffix sums: hist[cur][b] = elements in bins >= b
        int cur = 0;
        for (int o = 1; o < 256; o <<= 1) {
            if (t < 256) S.hist[cur ^ 1][t] = S.hist[cur][t] + (t + o < 256 ? S.hist[cur][t + o] : 0u);
            cur ^= 1;
            __syncthreads();
        }
        if (t < 256) {
            const unsigned ge = S.hist[cur][t], gt = t < 255 ? S.hist[cur][t + 1] : 0u;
            if (gt < need && need <= ge) {  // exactly one bin: the k-th largest key lies in it
                S.prefix = prefix | ((unsigned long long)t << shift);
                S.need = need - gt;
                S.n_ge = (unsigned)k - need + ge;  // elements with key >= the new prefix
            }
        }
        __syncthreads();
        prefix = S.prefix;
        need = S.need;
        const unsigned n_ge = S.n_ge;
        __syncthreads();
        if (n_ge <= (unsigned)kSmpCand) break;  // at the last pass need == 1 and n_ge == k
    }
    return prefix;
}

// The elements whose key is >= prefix (at most kSmpCand of them) into S.key, then a bitonic
// sort, descending: S.key[0 .. n) in the host's lexsort order, the unused tail 0 (below every
// key of a real logit).  The gathering pass also calls each(value, index) for every element
// of the row.  Returns n; every thread calls this; ends on a barrier.
template <class G>
__device__ __forceinline__ int gather_sort(SelLds& S, const float* lg, int V, unsigned long long prefix, G each) {
    const int t = threadIdx.x;
    if (t == 0) S.n_key = 0;
    if (t < kSmpCand) S.key[t] = 0;
    __syncthreads();
    for_row(lg, V, [&](float v, int i) {
        const unsigned long long key = argmax_key(v, i);
        each(v, i);
        if (key >= prefix) {
            const unsigned at = atomicAdd(&S.n_key, 1u);
            if (at < (unsigned)kSmpCand) S.key[at] = key;
        }
    });
    __syncthreads();
    const int n_key = min((int)S.n_key, kSmpCand);
    int n_sort = 64;
    while (n_sort < n_key) n_sort <<= 1;
    for (int kk = 2; kk <= n_sort; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            const int p = t ^ j;
            if (t < n_sort && p > t) {
                const unsigned long long x = S.key[t], y = S.key[p];
                const bool desc = (t & kk) == 0;
                if (desc ? x < y : x > y) { S.key[t] = y; S.key[p] = x; }
            }
            __syncthreads();
        }
    }
    return n_key;
}

}  // namespace llmi
