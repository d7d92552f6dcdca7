// attn.hip — decode attention over the f16 KV cache in ggml's generic (non-flash) order,
// the default numerics (the other two: attn86.hip, attnfa.hip): the kernels, the path
// selection of the single-sequence and the batched step, and the single-sequence launch.
// The batched launch is battn.hip; bodies that both run are in attn_device.h.
// Seven paths, bit-identical to each other and to the oracle (tests/test_gpu_attention.py):
//   1 k_attn_fused                one workgroup per head, scores in LDS
//   2 k_attn_scores8 -> k_attn_pv16   split: (group, 32-position tile), then (group, 16 dims)
//   3 k_attn_scores -> k_attn_pv  two kernels at any length
//   4 k_attn_x                    one launch, scores handed over through tagged granules
//   5 k_attn_r                    one launch, every load issued at entry, up to 512 positions
//   6 k_attn_d                    5 with the PV split over dim slices, up to 1024 positions
//   7 k_attl_*                    long contexts: four launches over position tiles
// The batched step (battn.hip) runs paths 2, 6 and 7.
#include "kernels.h"
#include "attn_device.h"
#include "launch_util.h"

#include <cstdlib>

namespace llmi {

// ----------------------------------------------------------------------------------
// Attention, ggml non-flash path:
//   kq[t] = sum_d f16(q_d) * K[t][d]        (ggml_vec_dot_f16, exact products, double sum)
//   w[t]  = kq[t] * (1/sqrt(D)); M = max w; e = exp(w-M); S = sum (double) e
//   p[t]  = f16(e * (float)(1/S));  out[d] = sum_t V[t][d] * p[t]    (double sum)
// scores: grid (HK, ceil(kv_bound/64)); workgroup = one kv head x 64 positions, its
//         K tile staged through LDS (rows padded by 16 B: conflict-free ds_read_b128).
// pv:     grid (HK, D/16); workgroup = one kv head x 16 dims for all GQA heads, reading
//         the transposed V cache [HK][D][n_ctx] with coalesced 128-B rows.
// ----------------------------------------------------------------------------------
template <int D, int G>
__global__ __launch_bounds__(256) void k_attn_scores(AttnArgs a) {
    const int g = blockIdx.x, chunk = blockIdx.y;
    const int n_kv = a.st->pos + 1;
    const int t0 = chunk * 64;
    if (t0 >= n_kv) return;
    const int nt = min(64, n_kv - t0);
    __shared__ float qs[G][D];
    __shared__ __attribute__((aligned(16))) uint16_t ks[64][D + 8];
    for (int i = threadIdx.x; i < G * D; i += 256) qs[i / D][i % D] = h2f(f2h(a.q[(size_t)g * G * D + i]));
    constexpr int PPR = D * 2 / 16;  // 16-B pieces per K row
    const uint16_t* kb = a.kc + ((size_t)g * a.n_ctx + t0) * D;
    for (int i = threadIdx.x; i < nt * PPR; i += 256) {
        const int r = i / PPR, pc = i % PPR;
        *(u32x4*)&ks[r][pc * 8] = *(const u32x4*)(kb + (size_t)r * D + pc * 8);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < nt) {
        for (int hh = wave; hh < G; hh += 4) {
            double acc = 0.0;
#pragma unroll 4
            for (int d = 0; d < D; d += 8) {
                const u32x4 kv = *(const u32x4*)&ks[lane][d];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc += (double)(h2f(kv[j]) * qs[hh][d + 2 * j]);
                    acc += (double)(h2f(kv[j] >> 16) * qs[hh][d + 2 * j + 1]);
                }
            }
            a.scores[(size_t)(g * G + hh) * a.n_ctx + t0 + lane] = (float)acc * a.scale;
        }
    }
}

template <int D, int G>
__global__ __launch_bounds__(256) void k_attn_pv(AttnArgs a) {
    const int g = blockIdx.x, dc = blockIdx.y;
    const int n_kv = a.st->pos + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ float sM[G], sInv[G];
    __shared__ float sp[G][256];
    __shared__ double red[4];
    __shared__ float redf[4];
    for (int hh = 0; hh < G; ++hh) {
        const float* w = a.scores + (size_t)(g * G + hh) * a.n_ctx;
        float mx = -INFINITY;
        for (int t = tid; t < n_kv; t += 256) mx = fmaxf(mx, w[t]);
        mx = wave_max(mx);
        if (lane == 0) redf[wave] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
        double s = 0.0;
        for (int t = tid; t < n_kv; t += 256) s += (double)llmi_expf(w[t] - mx);
        s = wave_sum_d(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        if (tid == 0) {
            sM[hh] = mx;
            sInv[hh] = (float)(1.0 / ((red[0] + red[1]) + (red[2] + red[3])));
        }
        __syncthreads();
    }
    const int d0 = dc * 16 + wave * 4;
    double acc[G][4];
#pragma unroll
    for (int hh = 0; hh < G; ++hh)
#pragma unroll
        for (int dd = 0; dd < 4; ++dd) acc[hh][dd] = 0.0;
    const uint16_t* vb = a.vc + ((size_t)g * D + d0) * a.n_ctx;
    for (int tc = 0; tc < n_kv; tc += 256) {
        __syncthreads();
        const int t = tc + tid;
#pragma unroll
        for (int hh = 0; hh < G; ++hh) {
            float p = 0.f;
            if (t < n_kv) {
                const float e = llmi_expf(a.scores[(size_t)(g * G + hh) * a.n_ctx + t] - sM[hh]);
                p = h2f(f2h(e * sInv[hh]));
            }
            sp[hh][tid] = p;
        }
        __syncthreads();
        const int nt = min(256, n_kv - tc);
        for (int j = lane; j < nt; j += 64) {
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
                const float v = h2f(vb[(size_t)dd * a.n_ctx + tc + j]);
#pragma unroll
                for (int hh = 0; hh < G; ++hh) acc[hh][dd] += (double)(v * sp[hh][j]);
            }
        }
    }
#pragma unroll
    for (int hh = 0; hh < G; ++hh)
#pragma unroll
        for (int dd = 0; dd < 4; ++dd) {
            const double s = wave_sum_d(acc[hh][dd]);
            if (lane == 0) a.out[(size_t)(g * G + hh) * D + d0 + dd] = (float)s;
        }
}

// Split attention, phase 1: grid (HK, kv_bound/64), 256 threads; thread (t, qd) dots
// quarter qd of K row t with the G f16-rounded query heads of its group (G independent
// double chains of D/4), then a 4-lane butterfly; K rows are read straight from HBM,
// 4 lanes x (D/2) B per row.  Rows < kv_bound are always inside the cache, so the K
// loads are issued before the position is known (no dependent-load chain).
template <int D, int G>
__global__ __launch_bounds__(256) void k_attn_scores4(AttnArgs a) {
    LLMI_ATT_STAMP(0, 0)
    const int g = blockIdx.x, t0 = blockIdx.y * 64;
    const int tid = threadIdx.x;
    constexpr int DQ = D / 4;
    const int t = t0 + (tid >> 2), qd = tid & 3;
    const uint16_t* kr = a.kc + ((size_t)g * a.n_ctx + t) * D + qd * DQ;
    u32x4 kv[DQ / 8];
#pragma unroll
    for (int i = 0; i < DQ / 8; ++i) kv[i] = *(const u32x4*)(kr + 8 * i);
    __shared__ __attribute__((aligned(16))) float qs[G][D];
    for (int i = tid; i < G * D; i += 256) qs[i / D][i % D] = h2f(f2h(a.q[(size_t)g * G * D + i]));
    const int n_kv = a.st->pos + 1;
    __syncthreads();
    LLMI_ATT_STAMP(0, 1)
    if (t0 >= n_kv) return;
#if defined(LLMI_EXP_TRACE)
    asm volatile("" ::"v"(kv[0].x));
    LLMI_ATT_STAMP(0, 2)
#endif
    double acc[G];
#pragma unroll
    for (int hh = 0; hh < G; ++hh) acc[hh] = 0.0;
#pragma unroll
    for (int i = 0; i < DQ / 8; ++i) {
        const int d = qd * DQ + 8 * i;
        float k[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            k[2 * j] = h2f((uint16_t)kv[i][j]);
            k[2 * j + 1] = h2f((uint16_t)(kv[i][j] >> 16));
        }
#pragma unroll
        for (int hh = 0; hh < G; ++hh) {
            const float4 qa = *(const float4*)&qs[hh][d], qb = *(const float4*)&qs[hh][d + 4];
            acc[hh] += (double)(k[0] * qa.x); acc[hh] += (double)(k[1] * qa.y);
            acc[hh] += (double)(k[2] * qa.z); acc[hh] += (double)(k[3] * qa.w);
            acc[hh] += (double)(k[4] * qb.x); acc[hh] += (double)(k[5] * qb.y);
            acc[hh] += (double)(k[6] * qb.z); acc[hh] += (double)(k[7] * qb.w);
        }
    }
#pragma unroll
    for (int hh = 0; hh < G; ++hh) {
        acc[hh] += xor_partner_d<1>(acc[hh]);
        acc[hh] += xor_partner_d<2>(acc[hh]);
        if (t < n_kv && qd == (hh & 3)) a.scores[(size_t)(g * G + hh) * a.n_ctx + t] = (float)acc[hh] * a.scale;
    }
    LLMI_ATT_STAMP(0, 3)
}

// Split attention, phase 2: grid (HK, D/8), 256 threads.  Every workgroup recomputes
// the softmax of its G heads from the scores (one wave per head: max, e = expf(s - max)
// kept in LDS, double sum, p = f16(e / sum) exactly as the fused kernel), then
// accumulates 8 output dims: 32 lanes per dim, 8 positions (16 B of the transposed V
// row) per lane and step, 4 steps of loads in flight, G double accumulators, 32-lane
// butterfly.  Score and first V loads are issued before the position is known.
template <int D, int G>
__global__ __launch_bounds__(256) void k_attn_pv_split(AttnArgs a, int kvb) {
    LLMI_ATT_STAMP(1, 0)
    extern __shared__ __attribute__((aligned(16))) float spv[];  // [G][kvb]
    const int g = blockIdx.x, dc = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = dc * 8 + (tid >> 5), sl = tid & 31;
    const uint16_t* vr = a.vc + ((size_t)g * D + d) * a.n_ctx;
    u32x4 vv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) vv[u] = *(const u32x4*)(vr + min(8 * sl + 256 * u, kvb - 8));
    // 1. stage the G score rows (all kv_bound positions; those past n_kv are never used)
    const int n4 = kvb >> 2;
#pragma unroll
    for (int hh = 0; hh < G; ++hh) {
        const float4* src = (const float4*)(a.scores + (size_t)(g * G + hh) * a.n_ctx);
        float4* dst = (float4*)(spv + hh * kvb);
        for (int j0 = tid; j0 < n4; j0 += 1024) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = src[min(j0 + 256 * u, n4 - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (j0 + 256 * u < n4) dst[j0 + 256 * u] = v[u];
        }
    }
    const int n_kv = a.st->pos + 1;
    __syncthreads();
    LLMI_ATT_STAMP(1, 1)
    // 2. softmax, one wave per head; p = 0 past n_kv (up to the next multiple of 8)
    for (int hh = wave; hh < G; hh += 4) {
        float* sp = spv + hh * kvb;
        float mx = -INFINITY;
        for (int t = lane; t < n_kv; t += 64) mx = fmaxf(mx, sp[t]);
        mx = wave_max(mx);
        double sum = 0.0;
        for (int t = lane; t < n_kv; t += 64) {
            const float e = llmi_expf(sp[t] - mx);
            sp[t] = e;
            sum += (double)e;
        }
        sum = wave_sum_d(sum);
        const float inv = (float)(1.0 / sum);
        for (int t = lane; t < n_kv; t += 64) sp[t] = h2f(f2h(sp[t] * inv));
        for (int t = n_kv + lane; t < ((n_kv + 7) & ~7); t += 64) sp[t] = 0.f;
    }
    __syncthreads();
    LLMI_ATT_STAMP(1, 2)
    // 3. PV (V past n_kv may be anything: masked to 0 so 0 * NaN never happens)
    double acc[G];
#pragma unroll
    for (int hh = 0; hh < G; ++hh) acc[hh] = 0.0;
    for (int t0 = 8 * sl;;) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int tb = t0 + 256 * u;
            if (tb < n_kv) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float f = h2f((uint16_t)(vv[u][j >> 1] >> (16 * (j & 1))));
                    v[j] = tb + j < n_kv ? f : 0.f;
                }
#pragma unroll
                for (int hh = 0; hh < G; ++hh) {
                    const float4 pa = *(const float4*)&spv[hh * kvb + tb], pb = *(const float4*)&spv[hh * kvb + tb + 4];
                    acc[hh] += (double)(v[0] * pa.x); acc[hh] += (double)(v[1] * pa.y);
                    acc[hh] += (double)(v[2] * pa.z); acc[hh] += (double)(v[3] * pa.w);
                    acc[hh] += (double)(v[4] * pb.x); acc[hh] += (double)(v[5] * pb.y);
                    acc[hh] += (double)(v[6] * pb.z); acc[hh] += (double)(v[7] * pb.w);
                }
            }
        }
        t0 += 1024;
        if (t0 >= n_kv) break;
#pragma unroll
        for (int u = 0; u < 4; ++u) vv[u] = *(const u32x4*)(vr + min(t0 + 256 * u, kvb - 8));
    }
#pragma unroll
    for (int hh = 0; hh < G; ++hh) {
        double v = acc[hh];
        v += xor_partner_d<1>(v);
        v += xor_partner_d<2>(v);
        v += xor_partner_d<4>(v);
        v += xor_partner_d<8>(v);
        v += xor_partner_d<16>(v);
        if (sl == 0) a.out[(size_t)(g * G + hh) * D + d] = (float)v;
    }
    LLMI_ATT_STAMP(1, 3)
}

// Split attention v2 (bodies in attn_device.h, shared with k_battn_scores8 / k_battn_pv16)
template <int D, int G>
__global__ __launch_bounds__(256) void k_attn_scores8(AttnArgs a) { attn_scores8_body<D, G>(a); }
template <int D, int G>
__global__ __launch_bounds__(512) void k_attn_pv16(AttnArgs a, int kvb) { attn_pv16_body<D, G>(a, kvb); }

// One-launch exchange attention for short contexts (kv_bound <= kXAttnMaxKV): grid
// (HK, D/16), 512 threads.  Workgroup (g, j) computes the scores of position tile j
// (64*NP positions; 8 lanes x D/8 dims per position, exact f16 products in double as
// k_attn_scores8) and publishes them as 8-byte {tag, score} granules (one relaxed
// agent-scope store each: the data is the flag, no fence; MI355X_MICROARCH.md
// "R2 granules").  Every workgroup of the group then sweeps all G x n_kv granules of
// its group until their tags match this step's (tag = step seq * 256 + layer + 1, read
// from device state at run time, so graph replays never see a previous step's
// granules), and runs k_attn_pv16's softmax and PV for its 16 output dims.  One
// launch and one hand-off replace the scores -> PV kernel boundary; K and V loads are
// issued before the position is known.  Every spin is bounded: a timed-out wait writes
// NaN outputs and sets *a.fault instead of hanging the GPU.
constexpr int kXSpinLimit = 1 << 22;
typedef unsigned long long __attribute__((address_space(1))) gu64;
template <int D, int G, int NP>
__global__ __launch_bounds__(512) void k_attn_x(AttnArgs a, int kvb) {
    LLMI_ATT_STAMP(0, 0)
    extern __shared__ __attribute__((aligned(16))) float spx[];  // [G][kvb] probabilities
    __shared__ __attribute__((aligned(16))) double qs[G][D];
    __shared__ float redm[8];
    __shared__ double reds[8];
    __shared__ int s_fault;
    constexpr int WPH = 8 / G;             // waves per head (softmax)
    constexpr int DQ = D / 8;              // dims per lane in the scores
    constexpr int NS = kXAttnMaxKV / (WPH * 64);  // max positions per lane in the softmax
    const int g = blockIdx.x, j = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // 1. step state and q first (they gate everything), then this tile's K rows (NP
    // passes of 64 positions), then this workgroup's V window: loads complete in issue
    // order, so nothing early waits behind the K/V stream
    const int pos = a.st->pos;
    const uint32_t seq = a.st->seq;
    float qv[(G * D + 511) / 512];
#pragma unroll
    for (int k = 0; k < (G * D + 511) / 512; ++k) qv[k] = a.q[(size_t)g * G * D + min(tid + 512 * k, G * D - 1)];
    const int qd = tid & 7;
    const int tile0 = j * 64 * NP;
    u32x4 kv[NP][DQ / 8];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int t = min(tile0 + p * 64 + (tid >> 3), kvb - 1);
        const uint16_t* kr = a.kc + ((size_t)g * a.n_ctx + t) * D + qd * DQ;
#pragma unroll
        for (int i = 0; i < DQ / 8; ++i) kv[p][i] = __builtin_nontemporal_load((const u32x4*)(kr + 8 * i));
    }
    const int d = j * 16 + (tid >> 5), sl = tid & 31;
    const uint16_t* vr = a.vc + ((size_t)g * D + d) * a.n_ctx;
    constexpr int NV = 8;  // 8-B V loads in flight per lane: a 1024-position window
    u32x2 vv[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) vv[k] = __builtin_nontemporal_load((const u32x2*)(vr + min(4 * sl + 128 * k, kvb - 4)));
#pragma unroll
    for (int k = 0; k < (G * D + 511) / 512; ++k)
        if (tid + 512 * k < G * D) qs[(tid + 512 * k) / D][(tid + 512 * k) % D] = (double)h2f(f2h(qv[k]));
    if (tid == 0) s_fault = 0;
    const int n_kv = pos + 1;
    const uint32_t tag = seq * 256u + (uint32_t)a.layer + 1u;
    const uint32_t want = tag + (uint32_t)a.tag_skew;  // test option: 1 = a hand-off that never completes
    __syncthreads();
    LLMI_ATT_STAMP(0, 1)
    // 2. scores of the tile -> granules
    gu64* gr = (gu64*)a.gran + (size_t)g * G * kXAttnMaxKV;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int t = tile0 + p * 64 + (tid >> 3);
        if (tile0 + p * 64 >= n_kv) break;  // uniform
        double acc[G];
#pragma unroll
        for (int hh = 0; hh < G; ++hh) acc[hh] = 0.0;
#pragma unroll
        for (int i = 0; i < DQ / 8; ++i) {
            const int d0 = qd * DQ + 8 * i;
            double k[8];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                k[2 * jj] = (double)h2f((uint16_t)kv[p][i][jj]);
                k[2 * jj + 1] = (double)h2f((uint16_t)(kv[p][i][jj] >> 16));
            }
#pragma unroll
            for (int hh = 0; hh < G; ++hh)
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) acc[hh] = __builtin_fma(k[jj], qs[hh][d0 + jj], acc[hh]);
        }
#pragma unroll
        for (int hh = 0; hh < G; ++hh) {
            acc[hh] += xor_partner_d<1>(acc[hh]);
            acc[hh] += xor_partner_d<2>(acc[hh]);
            acc[hh] += xor_partner_d<4>(acc[hh]);
            if (t < n_kv && qd == (hh & 7)) {
                const float sc = (float)acc[hh] * a.scale;
                __hip_atomic_store(gr + (size_t)hh * kXAttnMaxKV + t,
                                   ((unsigned long long)tag << 32) | __float_as_uint(sc), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    LLMI_ATT_STAMP(0, 2)
    // 3. sweep: lane (head hh, wave wi of the head) owns positions wi*64 + lane + k*WPH*64,
    // the softmax's own mapping, so the scores stay in registers.  All of a lane's
    // granule loads are issued together; only stragglers are re-read (bounded spin).
    const int hh = wave / WPH, wi = wave % WPH;
    const gu64* gh = gr + (size_t)hh * kXAttnMaxKV;
    float sv[NS];
    {
        unsigned long long x[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int t = wi * 64 + lane + k * WPH * 64;
            x[k] = t < n_kv ? __hip_atomic_load(gh + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                            : ((unsigned long long)tag << 32);
        }
        for (int spins = 0;; ++spins) {
            bool ok = true;
#pragma unroll
            for (int k = 0; k < NS; ++k) ok &= (uint32_t)(x[k] >> 32) == want;
            if (__all(ok)) break;
            if (spins >= a.spin_limit) {
                s_fault = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int t = wi * 64 + lane + k * WPH * 64;
                if ((uint32_t)(x[k] >> 32) != want && t < n_kv)
                    x[k] = __hip_atomic_load(gh + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) sv[k] = __uint_as_float((uint32_t)x[k]);
    }
    LLMI_ATT_STAMP(0, 3)
    // 4. softmax as k_attn_pv16: row max (exact in any order), e = expf(s - max) with a
    // double sum (waves combined in fixed order), p = f16(e / sum) into LDS
    {
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < NS; ++k)
            if (wi * 64 + lane + k * WPH * 64 < n_kv) m = fmaxf(m, sv[k]);
        m = wave_max(m);
        if (lane == 0) redm[wave] = m;
    }
    __syncthreads();
    float mx = redm[hh * WPH];
#pragma unroll
    for (int i = 1; i < WPH; ++i) mx = fmaxf(mx, redm[hh * WPH + i]);
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < NS; ++k)
        if (wi * 64 + lane + k * WPH * 64 < n_kv) {
            sv[k] = llmi_expf(sv[k] - mx);
            sum += (double)sv[k];
        }
    sum = wave_sum_d(sum);
    if (lane == 0) reds[wave] = sum;
    __syncthreads();
    double tot = reds[hh * WPH];
#pragma unroll
    for (int i = 1; i < WPH; ++i) tot += reds[hh * WPH + i];
    const float inv = (float)(1.0 / tot);
    float* sp = spx + hh * kvb;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int t = wi * 64 + lane + k * WPH * 64;
        if (t < n_kv) sp[t] = h2f(f2h(sv[k] * inv));
        else if (t < ((n_kv + 3) & ~3)) sp[t] = 0.f;
    }
    __syncthreads();
    LLMI_ATT_STAMP(1, 0)
    // 5. PV for dims [16j, 16j+16): as k_attn_pv16
    double acc[G];
#pragma unroll
    for (int h = 0; h < G; ++h) acc[h] = 0.0;
    for (int t0 = 4 * sl;;) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int tb = t0 + 128 * k;
            if (tb < n_kv) {
                double v[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const float f = h2f((uint16_t)((jj < 2 ? vv[k].x : vv[k].y) >> (16 * (jj & 1))));
                    v[jj] = tb + jj < n_kv ? (double)f : 0.0;
                }
#pragma unroll
                for (int h = 0; h < G; ++h) {
                    const float4 p = *(const float4*)(spx + h * kvb + tb);
                    acc[h] = __builtin_fma(v[0], (double)p.x, acc[h]);
                    acc[h] = __builtin_fma(v[1], (double)p.y, acc[h]);
                    acc[h] = __builtin_fma(v[2], (double)p.z, acc[h]);
                    acc[h] = __builtin_fma(v[3], (double)p.w, acc[h]);
                }
            }
        }
        t0 += 128 * NV;
        if (t0 >= n_kv) break;
#pragma unroll
        for (int k = 0; k < NV; ++k) vv[k] = __builtin_nontemporal_load((const u32x2*)(vr + min(t0 + 128 * k, kvb - 4)));
    }
    LLMI_ATT_STAMP(1, 1)
    const bool fault = s_fault != 0;
#pragma unroll
    for (int h = 0; h < G; ++h) {
        double v = acc[h];
        v += xor_partner_d<1>(v);
        v += xor_partner_d<2>(v);
        v += xor_partner_d<4>(v);
        v += xor_partner_d<8>(v);
        v += xor_partner_d<16>(v);
        if (sl == 0) a.out[(size_t)(g * G + h) * D + d] = fault ? __uint_as_float(0x7fc00000u) : (float)v;
    }
    if (fault && tid == 0) atomicOr(a.fault, 1u);
}

// Fused single-launch attention for KV lengths that fit in LDS (kv_bound <= 8192):
// one 1024-thread workgroup per query head; scores, softmax statistics and the
// f16-rounded probabilities stay in LDS, so the only global traffic is one K and one V
// read per head (the G heads of a KV group are dealt to one XCD: blockIdx % HK = group,
// so 3 of 4 K/V reads hit that XCD's L2).  Same numerics as the two-kernel path above.
template <int D>
__global__ __launch_bounds__(1024) void k_attn_fused(AttnArgs a, int G, int HK) {
    LLMI_ATT_STAMP(0, 0)
    extern __shared__ __attribute__((aligned(16))) float sp_lds[];
    __shared__ float qs[D];
    __shared__ double redd[16];
    __shared__ float redf[16];
    const int b = blockIdx.x;
    const int g = b % HK, h = g * G + b / HK;
    const int n_kv = a.st->pos + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < D) qs[tid] = h2f(f2h(a.q[(size_t)h * D + tid]));
    __syncthreads();
    // scores: one position per thread, K row read straight from HBM/L2 (16 x 16 B)
    const uint16_t* kb = a.kc + (size_t)g * a.n_ctx * D;
    float mx = -INFINITY;
    for (int t = tid; t < n_kv; t += 1024) {
        const uint16_t* kr = kb + (size_t)t * D;
        double acc = 0.0;
#pragma unroll 4
        for (int d = 0; d < D; d += 8) {
            const u32x4 kv = *(const u32x4*)(kr + d);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc += (double)(h2f(kv[j]) * qs[d + 2 * j]);
                acc += (double)(h2f(kv[j] >> 16) * qs[d + 2 * j + 1]);
            }
        }
        const float w = (float)acc * a.scale;
        sp_lds[t] = w;
        mx = fmaxf(mx, w);
    }
    LLMI_ATT_STAMP(0, 1)
    mx = wave_max(mx);
    if (lane == 0) redf[wave] = mx;
    __syncthreads();
    mx = redf[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, redf[w]);
    double s = 0.0;
    for (int t = tid; t < n_kv; t += 1024) s += (double)llmi_expf(sp_lds[t] - mx);
    s = wave_sum_d(s);
    if (lane == 0) redd[wave] = s;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += redd[w];
    const float inv = (float)(1.0 / tot);
    for (int t = tid; t < n_kv; t += 1024) sp_lds[t] = h2f(f2h(llmi_expf(sp_lds[t] - mx) * inv));
    __syncthreads();
    LLMI_ATT_STAMP(0, 2)
    // PV over the transposed V cache: SL threads per output dim, 8 positions (16 B) each
    constexpr int SL = 1024 / D;
    const int d = tid / SL, sl = tid % SL;
    const uint16_t* vr = a.vc + ((size_t)g * D + d) * a.n_ctx;
    double acc = 0.0;
    for (int t0 = 8 * sl; t0 < n_kv; t0 += 32 * SL) {  // 4 loads in flight, addresses clamped into the row
        u32x4 vv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vv[u] = *(const u32x4*)(vr + min(t0 + 8 * SL * u, a.n_ctx - 8));
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = t0 + 8 * SL * u + 2 * j;
                if (t < n_kv) acc += (double)(h2f(vv[u][j]) * sp_lds[t]);
                if (t + 1 < n_kv) acc += (double)(h2f(vv[u][j] >> 16) * sp_lds[t + 1]);
            }
    }
    acc += xor_partner_d<1>(acc);
    acc += xor_partner_d<2>(acc);
    acc += xor_partner_d<4>(acc);
    if constexpr (SL >= 16) acc += xor_partner_d<8>(acc);
    static_assert(SL == 8 || SL == 16, "head_dim 64 or 128");
    if (sl == 0) a.out[(size_t)h * D + d] = (float)acc;
    LLMI_ATT_STAMP(0, 3)
}

// Register-prefetched one-launch attention for short contexts (kv_bound <= 64*P <= 512):
// one 512-thread workgroup per query head.  Every global load of the launch — the step
// position, the head's q slice, all kv_bound K rows and the V window — is issued at
// entry (addresses clamped into the bucket, never gated on the position), so one memory
// latency covers the launch; the rest is the dependent compute chain:
//   scores  8 lanes x D/8 dims per position (exact f16 products summed in double, 3-step
//           butterfly), P passes of 64 positions; scores to LDS, row max per wave
//   softmax e = expf(s - max), double sum over the workgroup (fixed order), p =
//           f16(e * (float)(1/sum)) in LDS as f32 — the formulas of k_attn_fused
//   PV      512/D lanes per output dim, double fma of exact f16 products, butterfly.
// Same numerics as the other paths (the double sums are exact in practice; the paths
// are checked bit-identical against each other and the oracle).
template <int D, int P>
__global__ __launch_bounds__(512) void k_attn_r(AttnArgs a, int G, int kvb) {
    constexpr int DQ = D / 8;          // score dims per lane
    constexpr int SLV = 512 / D;       // PV lanes per output dim (4 or 8)
    constexpr int NVL = 64 * P / (8 * SLV);  // 16-B V loads per lane (8 positions each)
    __shared__ __attribute__((aligned(16))) float sp[64 * P + 8];
    __shared__ float redm[8];
    __shared__ double reds[8];
    LLMI_ATT_STAMP(0, 0)
    const int h = blockIdx.x, g = h / G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qd = tid & 7, pp = tid >> 3;
    // 1. every load up front: position, q slice, K rows of all passes, V window
    const int pos = a.st->pos;
    float4 qv[DQ / 4];
#pragma unroll
    for (int i = 0; i < DQ / 4; ++i) qv[i] = *(const float4*)(a.q + (size_t)h * D + qd * DQ + 4 * i);
    u32x4 kv[P][DQ / 8];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int t = min(64 * p + pp, kvb - 1);
        const uint16_t* kr = a.kc + ((size_t)g * a.n_ctx + t) * D + qd * DQ;
#pragma unroll
        for (int i = 0; i < DQ / 8; ++i) kv[p][i] = __builtin_nontemporal_load((const u32x4*)(kr + 8 * i));
    }
    const int d = tid / SLV, sl = tid % SLV;
    const uint16_t* vr = a.vc + ((size_t)g * D + d) * a.n_ctx;
    u32x4 vv[NVL];
#pragma unroll
    for (int u = 0; u < NVL; ++u) vv[u] = __builtin_nontemporal_load((const u32x4*)(vr + min(8 * sl + 8 * SLV * u, kvb - 8)));
    const int n_kv = pos + 1;
    // 2. scores (q rounded to f16 as upstream's KQ mul_mat does; f16 x f16 products exact)
    double q[DQ];
#pragma unroll
    for (int i = 0; i < DQ / 4; ++i) {
        q[4 * i + 0] = (double)h2f(f2h(qv[i].x)); q[4 * i + 1] = (double)h2f(f2h(qv[i].y));
        q[4 * i + 2] = (double)h2f(f2h(qv[i].z)); q[4 * i + 3] = (double)h2f(f2h(qv[i].w));
    }
    float m = -INFINITY;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < DQ / 8; ++i)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                acc = __builtin_fma((double)h2f((uint16_t)kv[p][i][jj]), q[8 * i + 2 * jj], acc);
                acc = __builtin_fma((double)h2f((uint16_t)(kv[p][i][jj] >> 16)), q[8 * i + 2 * jj + 1], acc);
            }
        acc += xor_partner_d<1>(acc);
        acc += xor_partner_d<2>(acc);
        acc += xor_partner_d<4>(acc);
        const int t = 64 * p + pp;
        const float sc = (float)acc * a.scale;
        if (qd == 0) sp[t] = sc;
        if (t < n_kv) m = fmaxf(m, sc);
    }
    LLMI_ATT_STAMP(0, 1)
    m = wave_max(m);
    if (lane == 0) redm[wave] = m;
    __syncthreads();
    float mx = redm[0];
#pragma unroll
    for (int w = 1; w < 8; ++w) mx = fmaxf(mx, redm[w]);
    // 3. softmax: thread t owns position t (64*P <= 512 positions)
    float e = 0.f;
    double s = 0.0;
    if (tid < n_kv && tid < 64 * P) {
        e = llmi_expf(sp[tid] - mx);
        s = (double)e;
    }
    s = wave_sum_d(s);
    if (lane == 0) reds[wave] = s;
    __syncthreads();
    double tot = reds[0];
#pragma unroll
    for (int w = 1; w < 8; ++w) tot += reds[w];
    const float inv = (float)(1.0 / tot);
    if (tid < 64 * P) sp[tid] = tid < n_kv ? h2f(f2h(e * inv)) : 0.f;
    __syncthreads();
    LLMI_ATT_STAMP(0, 2)
    // 4. PV: lane sl covers positions 8*sl + 8*SLV*u + j; two double chains
    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
    for (int u = 0; u < NVL; ++u) {
        const int tb = 8 * sl + 8 * SLV * u;
        if (tb < n_kv) {
            const float4 p0 = *(const float4*)(sp + tb), p1 = *(const float4*)(sp + tb + 4);
            const float pr[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float f = h2f((uint16_t)(vv[u][j >> 1] >> (16 * (j & 1))));
                const double v = tb + j < n_kv ? (double)f : 0.0;
                if (j & 1) acc1 = __builtin_fma(v, (double)pr[j], acc1);
                else acc0 = __builtin_fma(v, (double)pr[j], acc0);
            }
        }
    }
    double acc = acc0 + acc1;
    acc += xor_partner_d<1>(acc);
    acc += xor_partner_d<2>(acc);
    if constexpr (SLV == 8) acc += xor_partner_d<4>(acc);
    if (sl == 0) a.out[(size_t)h * D + d] = (float)acc;
    LLMI_ATT_STAMP(0, 3)
}

// Long-context attention (path 7): bodies in attn_device.h (shared with k_battl_*)
template <int D, int G, int NP>
__global__ __launch_bounds__(256) void k_attl_scores(AttnArgs a) { attl_scores_body<D, G, NP>(a); }
__global__ __launch_bounds__(256) void k_attl_exp(AttnArgs a, int n_head, int kvb) { attl_exp_body(a, n_head, kvb); }
template <int D, int G>
__global__ __launch_bounds__(512) void k_attl_pv(AttnArgs a, int n_head, int kvb) { attl_pv_body<D, G>(a, n_head, kvb); }
template <int D>
__global__ __launch_bounds__(D) void k_attl_sum(AttnArgs a, int n_head) { attl_sum_body<D>(a, n_head); }

// Dim-split one-launch attention (path 6): body in attn_device.h (shared with k_battn_d)
// What the entry needs arrives as plain scalars and pointers, which are preloaded into
// SGPRs (14 dwords: 5 pointers, n_ctx, geo = G | HK << 8 | pf << 24, kvb, scale)
template <int D, int P, int S>
__global__ __launch_bounds__(512) void k_attn_d(const float* q, const uint16_t* kc, const uint16_t* vc, const StepState* st,
                                                float* out, int n_ctx, int geo, int kvb, float scale,
                                                unsigned long long* trace) {
    const int pf = geo >> 24;
    attn_d_body<D, P, S>(AttnDArgs{q, kc, vc, st, out, n_ctx, scale, trace}, geo & 255, (geo >> 8) & 0xffff, kvb, pf & 1,
                         (pf >> 1) & 1);
}

// ---- Selection: which path, and each path's P / S / NP / tile counts, for the single-
// sequence and the batched step (battn.hip).  Plain host functions, no launch in them. ----
// Test options (llmi_test_option; never read from the environment)
int g_xspin_limit = kXSpinLimit;  // k_attn_x bounded-wait polls before it faults
int g_xtag_skew = 0;              // k_attn_x consumers expect tag + skew (1: never matches)

// dim slices of k_attn_d: about 256 workgroups (one per CU), 2..8, at least 8 dims each
static int g_attn_s = 0;  // LLMI_ATTN_S (A/B only): force 2, 4 or 8 slices
// k_attn_d reads the position before its K/V loads and skips those past it (default;
// LLMI_ATTN_PF=0 loads the whole KV bucket, A/B only): ties at bucket ends, up to 1.4 us
// faster mid-bucket (profiles/r02/attn_dim_split.md)
static int g_attn_pf = 3;
int attn_d_slices(int n_head, int head_dim) {
    const int s = g_attn_s ? g_attn_s : n_head >= 128 ? 2 : n_head >= 64 ? 4 : 8;
    return head_dim / s >= 8 ? s : head_dim / 8;
}

static int g_attn_mode = 0;  // 0 auto, 1..7 one path (kernels.h attn_path; LLMI_ATTN_MODE at model load)
void set_attn_mode(int mode) {
    g_attn_mode = mode;
    const char* e = getenv("LLMI_ATTN_S");
    const int v = e ? atoi(e) : 0;
    g_attn_s = (v == 2 || v == 4 || v == 8) ? v : 0;
    const char* f = getenv("LLMI_ATTN_PF");
    g_attn_pf = f ? atoi(f) : 1;
    const char* r = getenv("LLMI_ATTN_ROT");  // rotated K pass order (bit 1 of the word; default on)
    if (!r || atoi(r)) g_attn_pf |= 2;
}
int attn_path(int n_head, int n_head_kv, int kv_bound, int head_dim, int mode) {
    const int g = n_head / n_head_kv;
    const int m = mode < 0 ? g_attn_mode : mode;
    const bool split_ok = (size_t)g * kv_bound * 4 <= kSplitAttnMaxLds;
    const bool fused_ok = kv_bound <= kFusedAttnMaxKV;
    if (m == 4 && g <= 8 && kv_bound <= kXAttnMaxKV) return 4;
    if (m == 5 && kv_bound <= kRegAttnMaxKV) return 5;
    if (m == 6 && kv_bound <= kDimAttnMaxKV) return 6;
    if (m == 7 && g <= 8) return 7;
    if (m == 1 && fused_ok) return 1;
    if (m == 2 && split_ok) return 2;
    if (m == 3) return 3;
    // auto, from the crossovers measured by tools/attnbench.py (graph-free launches, us;
    // profiles/r01/attn_modes.md):
    //   G=4, D=128 (8B, Mistral): fused <= 256 (8.1 vs 8.4 exchange), exchange <= 512,
    //                             split beyond (640: 10.8 vs 12.9 exchange)
    //   G=8, D=128 (70B): fused <= 640 (128: 8.1 vs 16.3 exchange), split beyond
    //   G=8, D=64 (TinyLlama): fused <= 2048 (128: 6.2 vs 9.7; 1280: 15.9 vs 20.9)
    //   G=8, D=64: register-prefetched k_attn_r <= 256 (5.5-5.9 vs 6.2-6.7 fused); for
    //              D=128 it loses to fused (one CU pulls 64 KB+ per head: per-CU bandwidth)
    //   k_attn_d (dim-split, scores recomputed per slice, round 2) beats all of the above
    //   up to 1024 positions on every shape (tools/attnbench.py, profiles/r02/attn_dim_split.md):
    //   G=4 D=128 128: 5.2 vs 8.1 fused, 512: 7.0 vs 10.0 exchange, 1024: 10.8 vs 12.7 split
    //   long-context four-launch path 7 (profiles/r02/attn_long.md): G=4 D=128 beyond 2048
    //   (4096: 25.4 vs 31.2 split, 16384: 62 vs 628 two-kernel), G=8 beyond 1024
    if (m == 0) {
        if (g <= 8 && kv_bound <= kDimAttnMaxKV && attn_d_slices(n_head, head_dim) >= 2) return 6;
        if (g == 8 && kv_bound > 1024) return 7;
        if (g <= 4 && kv_bound > 2048) return 7;
        if (g == 8 && head_dim == 64 && kv_bound <= 256) return 5;
        if (g == 8 && fused_ok && kv_bound <= (head_dim == 64 ? 2048 : 640)) return 1;
        if (g == 4 && fused_ok && kv_bound <= 256) return 1;
        if (g == 4 && split_ok && kv_bound > 512) return 2;
        if (g <= 8 && kv_bound <= kXAttnMaxKV) return 4;
    }
    return split_ok ? 2 : fused_ok ? 1 : 3;
}

// batched dim slices: the single-sequence choice (about 256 workgroups) is H * S * slots
// workgroups here, each re-reading its head's K rows; up to 512 positions 2 slices for
// <= 4 slots and 1 beyond (8B, ~200 positions, 2/4/8 slots: 721/960/1878 tok/s split or 8
// slices -> 731/992/1945 with 2, 727/987/1963 with 1, profiles/r05/batch/battn_slices.txt);
// LLMI_BATTN_S (A/B) forces 1, 2, 4 or 8
int battn_slices(int n_head, int head_dim, int kv_bound, int nt) {
    if (const char* es = getenv("LLMI_BATTN_S")) {
        const int v = atoi(es);
        if ((v == 1 || v == 2 || v == 4 || v == 8) && head_dim / v >= 8) return v;
    }
    if (kv_bound <= 512 && nt >= 2) return nt > 4 ? 1 : 2;
    return attn_d_slices(n_head, head_dim);
}
// batched path: dim split up to 1024 positions for up to 3 slots (8B bench: 2 slots 940 vs
// 897 tok/s split, 4: 1335 vs 1341, 8: 1746 vs 1823 with 8 dim slices — at 8 slots its
// redundant K reads cost more than the split path's second launch), and for any slot count
// up to 512 positions with 1-2 slices (battn_slices), split while its LDS fits up to 2048
// (G <= 4) / 1024 positions, long-context beyond; LLMI_BATTN_MODE (A/B only) forces 2
// split, 6 dim split or 7 long-context
int battn_path(int g, int n_head, int head_dim, int kv_bound, int nt) {
    const char* e = getenv("LLMI_BATTN_MODE");
    const int forced = e ? atoi(e) : 0;
    const bool split_ok = (size_t)g * kv_bound * 4 <= kSplitAttnMaxLds;
    const bool dim_ok = g <= 8 && kv_bound <= kDimAttnMaxKV && attn_d_slices(n_head, head_dim) >= 2;
    if (forced == 2 && split_ok) return 2;
    if (forced == 6 && dim_ok) return 6;
    if (forced == 7 && g <= 8) return 7;
    if (dim_ok && (nt <= 3 || kv_bound <= 512)) return 6;
    if (split_ok && (g <= 4 ? kv_bound <= 2048 : kv_bound <= 1024)) return 2;
    if (dim_ok) return 6;
    return g <= 8 ? 7 : (split_ok ? 2 : 0);
}

// paths 5 and 6 (kernels.h; k_attn_r: cap 8, k_attn_d and k_battn_d: cap 16)
int attn_passes(int kv_bound, int cap) {
    const int p = kv_bound <= 64 ? 1 : kv_bound <= 128 ? 2 : kv_bound <= 256 ? 4 : kv_bound <= 512 ? 8 : kv_bound <= 768 ? 12 : 16;
    return p < cap ? p : cap;
}

// path 4: K tile passes for a KV bound (tiles of 64*NP positions cover kv_bound with D/16
// workgroups per group); 0 = not applicable.  D = 128 has 8 workgroups per group, so
// kXAttnMaxKV positions need at most 2 passes: NP = 4 exists for D = 64 only.
static_assert(kXAttnMaxKV <= 2 * (128 / 16) * 64 && kXAttnMaxKV <= 4 * (64 / 16) * 64, "k_attn_x passes");
static int attn_x_np(int head_dim, int kv_bound) {
    const int nw = head_dim / 16;
    const int np = (kv_bound + nw * 64 - 1) / (nw * 64);
    if (kv_bound > kXAttnMaxKV) return 0;
    return np <= 1 ? 1 : np <= 2 ? 2 : np <= 4 ? 4 : 0;
}

// path 7 (kernels.h)
LongGeo attn_long_geo(int kv_bound) {
    const int np = kv_bound > 4096 ? 4 : 1;
    return {(kv_bound + kLongTile - 1) / kLongTile, np, (kv_bound + 32 * np - 1) / (32 * np)};
}

// Single-sequence launch.  Every launch goes through launch_k: `first` / `last` mark the
// op's first and last kernel for the launch-event hook.
hipError_t launch_attention(const AttnArgs& a0, int n_head, int n_head_kv, int head_dim, int kv_bound, hipStream_t s,
                            int mode) {
    if (n_head_kv <= 0 || n_head % n_head_kv) return hipErrorInvalidValue;
    if (a0.fa) return launch_attention_fa(a0, n_head, n_head_kv, head_dim, kv_bound, s);
    if (a0.num) return launch_attention_x86(a0, n_head, n_head_kv, head_dim, kv_bound, s, mode < 0 ? g_attn_mode : mode);
    AttnArgs a = a0;
    a.spin_limit = g_xspin_limit;
    a.tag_skew = g_xtag_skew;
    const int g = n_head / n_head_kv, hk = n_head_kv;
    int path = attn_path(n_head, n_head_kv, kv_bound, head_dim, mode);
    if (path == 4 && (!a.gran || !a.fault || a.layer < 0 || a.layer > 254))
        path = attn_path(n_head, n_head_kv, kXAttnMaxKV + 256, head_dim, mode);
    const OfD d{head_dim};
    const OfG gq{g};
    const size_t lds_g = (size_t)g * kv_bound * 4;  // the group's probabilities (paths 2 and 4)
    const LongGeo lg = attn_long_geo(kv_bound);     // path 7
    const dim3 heads(n_head);
    bool ok;
    switch (path) {
        case 1:
            ok = pick([&](auto D) { launch_k(k_attn_fused<D>, heads, dim3(1024), (size_t)kv_bound * 4, s, true, true, a, g, hk); }, d);
            break;
        case 2:
            ok = pick([&](auto D, auto G) {
                launch_k(k_attn_scores8<D, G>, dim3(hk, (kv_bound + 31) / 32), dim3(256), 0, s, true, false, a);
                launch_k(k_attn_pv16<D, G>, dim3(hk, D / 16), dim3(512), lds_g, s, false, true, a, kv_bound);
            }, d, gq);
            break;
        case 4:
            ok = pick([&](auto D, auto G, auto NP) {
                if constexpr (D == 64 || NP < 4)  // attn_x_np
                    launch_k(k_attn_x<D, G, NP>, dim3(hk, D / 16), dim3(512), lds_g, s, true, true, a, kv_bound);
            }, d, gq, Of<1, 2, 4>{attn_x_np(head_dim, kv_bound)});
            break;
        case 5:
            ok = pick([&](auto D, auto P) { launch_k(k_attn_r<D, P>, heads, dim3(512), 0, s, true, true, a, g, kv_bound); },
                      d, Of<1, 2, 4, 8>{attn_passes(kv_bound, 8)});
            break;
        case 6:
            ok = pick([&](auto D, auto P, auto S) {
                launch_k(k_attn_d<D, P, S>, dim3(n_head * S), dim3(512), 0, s, true, true, a.q, a.kc, a.vc, a.st, a.out,
                         a.n_ctx, g | hk << 8 | g_attn_pf << 24, kv_bound, a.scale, a.trace);
            }, d, Of<1, 2, 4, 8, 12, 16>{attn_passes(kv_bound, 16)}, Of<2, 4, 8>{attn_d_slices(n_head, head_dim)});
            break;
        case 7:
            ok = pick([&](auto D, auto G, auto NP) {
                launch_k(k_attl_scores<D, G, NP>, dim3(hk, lg.nscores), dim3(256), 0, s, true, false, a);
                launch_k(k_attl_exp, dim3(n_head, lg.ntile), dim3(256), 0, s, false, false, a, n_head, kv_bound);
                launch_k(k_attl_pv<D, G>, dim3(hk, lg.ntile), dim3(512), 0, s, false, false, a, n_head, kv_bound);
                launch_k(k_attl_sum<D>, heads, dim3(D), 0, s, false, true, a, n_head);
            }, d, gq, Of<1, 4>{lg.np});
            break;
        default:  // 3
            ok = pick([&](auto D, auto G) {
                launch_k(k_attn_scores<D, G>, dim3(hk, (kv_bound + 63) / 64), dim3(256), 0, s, true, false, a);
                launch_k(k_attn_pv<D, G>, dim3(hk, D / 16), dim3(256), 0, s, false, true, a);
            }, d, gq);
    }
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace llmi

