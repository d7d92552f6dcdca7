// attnfa_stream.hip — flash-attention numerics decode attention, streamed: the bits of
// k_attn_fa (attnfa.hip, whose header states the recurrence and why taking it apart is
// exact) with a fixed LDS footprint, so the KV length has no limit but the cache's.
//
// One workgroup per query head (per slot in the batched form) walks the keys in tiles of
// kFaStreamTile positions.  Its waves have two roles, and each role works on another tile:
//   consumers (the first D / 64 waves): lane d runs dim d's recurrence over tile i,
//       y = f16(f32(y) * ms), y = f16(f32(y) + v * vs) (X86: one fma), S = S * ms + vs,
//       from the (ms, vs) pairs of LDS buffer i & 1.  ms is 1 wherever the running maximum
//       does not move and scaling by 1 changes nothing, so a group of 8 positions whose ms
//       are all 1 skips the scale step (two of the chain's five conversions).  V (transposed)
//       arrives 64 positions ahead of use in 16-byte loads, the next tile's first 64
//       requested before the barrier.
//   producers (kFaStreamTile / 64 waves, one lane per position):
//       stage A, tile i + 2: the score in the model's association, the exclusive prefix
//           max inside the wave, and the wave's max into cmax[i & 1];
//       stage B, tile i + 1: prev = max(carried M, the waves before, the lanes before);
//           new max -> ms = expf(prev - s), vs = 1; else ms = 1, vs = expf(s - prev)
//           (strict >, so a tie takes the else branch), into buffer (i + 1) & 1.
//       A lane keeps its score in a register from A to B.  The carried maximum M is the
//       max of every cmax seen so far, kept per lane (a prefix max: exact in any order).
// One __syncthreads() per tile and two to fill the pipeline, the trip count from n_kv alone
// (uniform in the workgroup): no flags, no waits, nothing between workgroups.  Positions at or
// past n_kv are never scored, never read from LDS and never multiplied (stale cache entries
// may be NaN); a 16-byte V load is issued only if its first position is live.
#include "kernels.h"
#include "launch_util.h"
#include "mv_device.h"

namespace llmi {

namespace {

constexpr int kTK = kFaStreamTile;
constexpr int kPW = kTK / 64;  // producer waves
static_assert(kTK % 64 == 0, "a producer wave owns 64 positions, a V prefetch covers 64");

// phase 1 of attn_fa_body: one position's score
template <int D, int X86>
__device__ __forceinline__ float fa_s_score(const uint16_t* kr, const float* qs, float scale) {
    float s;
    if constexpr (X86) {
        float acc[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) acc[i] = 0.f;
#pragma unroll
        for (int d0 = 0; d0 < D; d0 += 8) {
            const u32x4 kv = *(const u32x4*)(kr + d0);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = d0 + j;
                acc[i & 31] = __builtin_fmaf(h2f((uint16_t)(kv[j >> 1] >> (16 * (j & 1)))), qs[i], acc[i & 31]);
            }
        }
        float c[8];
#pragma unroll
        for (int l = 0; l < 8; ++l) c[l] = (acc[l] + acc[16 + l]) + (acc[8 + l] + acc[24 + l]);
        const float t0 = c[0] + c[4], t1 = c[1] + c[5], t2 = c[2] + c[6], t3 = c[3] + c[7];
        s = (float)(double)((t0 + t1) + (t2 + t3));
    } else {
        double sum = 0.0;
#pragma unroll
        for (int d0 = 0; d0 < D; d0 += 8) {
            const u32x4 kv = *(const u32x4*)(kr + d0);
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += (double)(h2f((uint16_t)(kv[j >> 1] >> (16 * (j & 1)))) * qs[d0 + j]);
        }
        s = (float)sum;
    }
    s = s * scale;
    return s + 0.0f;  // + slope * mask (0 for every position the query sees)
}

// 8 positions of dim d's recurrence from their (ms, vs) pairs; `live` of them exist.  SCALE
// false: every ms is 1, and f16(f32(y) * 1) = y, S * 1 = S.
template <int X86, bool SCALE>
__device__ __forceinline__ void fa_s_steps(uint16_t& y, float& S, const u32x4 v8, const float4 (&f)[4], int live) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k < live) {
            const float ms = (k & 1) ? f[k >> 1].z : f[k >> 1].x, vs = (k & 1) ? f[k >> 1].w : f[k >> 1].y;
            const float v = h2f((uint16_t)(v8[k >> 1] >> (16 * (k & 1))));
            if constexpr (SCALE) y = f2h(h2f(y) * ms);
            if constexpr (X86) {
                y = f2h(__builtin_fmaf(v, vs, h2f(y)));
                S = SCALE ? __builtin_fmaf(S, ms, vs) : S + vs;
            } else {
                y = f2h(h2f(y) + v * vs);
                S = SCALE ? S * ms + vs : S + vs;
            }
        }
    }
}

template <int D, int X86>
__device__ __forceinline__ void attn_fa_s_body(const AttnArgs& a, int G) {
    constexpr int CW = D / 64;  // consumer waves
    __shared__ __attribute__((aligned(16))) float fac[2][kTK * 2];  // (ms, vs) per position, two tiles
    __shared__ float qs[D];
    __shared__ float cmax[2][kPW];
    const int h = blockIdx.x, g = h / G, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_kv = min(a.st->pos + 1, a.n_ctx);
    const int nt = (n_kv + kTK - 1) / kTK;
    for (int d = tid; d < D; d += 64 * (CW + kPW)) qs[d] = h2f(f2h(a.q[(size_t)h * D + d]));
    // producer state: this lane's score of the tile after next and the max of the lanes
    // before it in the wave (stage A), the max of every tile already turned into factors
    const int pw = wave - CW, p = pw * 64 + lane;
    const uint16_t* kb = a.kc + (size_t)g * a.n_ctx * D;
    float s = -INFINITY, e = -INFINITY, M = -INFINITY;
    // consumer state: dim `tid`'s accumulator, the sum, the 64 positions in hand
    const uint16_t* vr = a.vc + ((size_t)g * D + (tid < D ? tid : 0)) * a.n_ctx;
    uint16_t y = 0;
    float S = 0.0f;
    u32x4 cur[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        cur[j] = u32x4{0, 0, 0, 0};
        if (wave < CW && 8 * j < n_kv) cur[j] = *(const u32x4*)(vr + 8 * j);
    }
    __syncthreads();
    for (int it = -2; it < nt; ++it) {
        if (wave >= CW) {
            if (it + 1 >= 0 && it + 1 < nt) {  // stage B of tile it + 1
                const float* cm = cmax[(it + 1) & 1];
                float prev = fmaxf(M, e);
#pragma unroll
                for (int j = 0; j < kPW; ++j) {
                    const float c = cm[j];
                    if (j < pw) prev = fmaxf(prev, c);
                    M = fmaxf(M, c);
                }
                if ((it + 1) * kTK + p < n_kv) {
                    float ms = 1.0f, vs = 1.0f;
                    if (s > prev) ms = llmi_expf_glibc(prev - s, 1);
                    else vs = llmi_expf_glibc(s - prev, 1);
                    *(float2*)&fac[(it + 1) & 1][2 * p] = make_float2(ms, vs);
                }
            }
            if (it + 2 < nt) {  // stage A of tile it + 2
                const int t = (it + 2) * kTK + p;
                s = t < n_kv ? fa_s_score<D, X86>(kb + (size_t)t * D, qs, a.scale) : -INFINITY;
                float inc = s;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const float up = __shfl_up(inc, o, 64);
                    if (lane >= o) inc = fmaxf(inc, up);
                }
                e = __shfl_up(inc, 1, 64);
                if (lane == 0) e = -INFINITY;
                if (lane == 63) cmax[it & 1][pw] = inc;
            }
        } else if (it >= 0) {
            const float* f = fac[it & 1];
            const int t0 = it * kTK, nl = min(kTK, n_kv - t0);  // live positions of this tile
            for (int sb = 0; sb * 64 < nl; ++sb) {
                u32x4 nxt[8];
                const int tn = t0 + (sb + 1) * 64;  // the 64 positions after these (the next tile's first, too)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    nxt[j] = u32x4{0, 0, 0, 0};
                    if (tn + 8 * j < n_kv) nxt[j] = *(const u32x4*)(vr + tn + 8 * j);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int b = sb * 64 + 8 * j;
                    if (b < nl) {
                        float4 f4[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) f4[k] = *(const float4*)(f + 2 * b + 4 * k);
                        const int live = nl - b;
                        bool moved = false;  // a stale pair is whatever the tile before last left: at worst the scale step runs
#pragma unroll
                        for (int k = 0; k < 4; ++k) moved = moved || f4[k].x != 1.0f || f4[k].z != 1.0f;
                        if (__builtin_amdgcn_readfirstlane((int)moved)) fa_s_steps<X86, true>(y, S, cur[j], f4, live);
                        else fa_s_steps<X86, false>(y, S, cur[j], f4, live);
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) cur[j] = nxt[j];
            }
        }
        __syncthreads();
    }
    if (tid < D) {
        const float S_inv = S == 0.0f ? 0.0f : 1.0f / S;
        a.out[(size_t)h * D + tid] = h2f(y) * S_inv;
    }
}

template <int D, int X86>
__global__ __launch_bounds__(D + kTK) void k_attn_fa_s(AttnArgs a, int G) { attn_fa_s_body<D, X86>(a, G); }
// batched decode: batch slot = blockIdx.y (its own sequence's caches, q, output, position)
template <int D, int X86>
__global__ __launch_bounds__(D + kTK) void k_battn_fa_s(BAttnArgs b, int G) { attn_fa_s_body<D, X86>(b.a[blockIdx.y], G); }

}  // namespace

int g_fa_stream = 2;  // launch_attention_fa's kernel (kernels.h)

// the callers (attnfa.hip) have checked the head counts and the context
hipError_t launch_attention_fa_s(const AttnArgs& a, int n_head, int n_head_kv, int head_dim, hipStream_t s) {
    const int G = n_head / n_head_kv;
    const bool ok = pick([&](auto D, auto X) {
        launch_k(k_attn_fa_s<D, X>, dim3(n_head), dim3(D + kTK), 0, s, true, true, a, G);
    }, OfD{head_dim}, Of<0, 1>{a.num ? 1 : 0});
    return ok ? hipGetLastError() : hipErrorNotSupported;
}

hipError_t launch_battention_fa_s(const BAttnArgs& b, int nt, int n_head, int n_head_kv, int head_dim, hipStream_t s) {
    const int G = n_head / n_head_kv;
    const bool ok = pick([&](auto D, auto X) {
        launch_k(k_battn_fa_s<D, X>, dim3(n_head, nt), dim3(D + kTK), 0, s, true, true, b, G);
    }, OfD{head_dim}, Of<0, 1>{b.a[0].num ? 1 : 0});
    return ok ? hipGetLastError() : hipErrorNotSupported;
}

}  // namespace llmi
