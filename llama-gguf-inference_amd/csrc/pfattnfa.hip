// pfattnfa.hip — batched-prefill attention in the flash-attention numerics (opt-in,
// LLMI_FA_PREFILL=1): T query rows at positions pos0.. run upstream's
// one_chunk recurrence (attnfa.hip header, oracle/ggml_oracle.c attn_head_fa) against the
// f16 caches, every row seeing positions 0 .. pos0 + i, bit-identical to T decode steps
// of k_attn_fa.  Rows and heads are independent; only the position loop of one (row,
// head, dim) is sequential, so the kernel streams over the keys flash-style:
//
//   workgroup  one KV head x a tile of TQ = 32 / G query rows x its G heads = up to 32
//              (row, head) PAIRS, 512 threads (two waves per SIMD: with one, every LDS wait of
//              the score loop was exposed); the latest rows (longest loops) launch first
//   key tile   64 positions: K [64][D] and V [D][64] staged in LDS once for all pairs
//              (the next tile's global loads are in flight during the recurrence)
//   (a) scores wave w owns pairs 4w .. 4w + 3, lane = key: the decode kernel's dot
//              (generic: one double chain per pair, the 4 pairs interleaved; x86: the 32
//              fp32 fma chains and the fixed tree, K row in registers), * scale, + 0
//   (b) factors the running max is a prefix max: a 64-lane scan seeded with the pair's
//              carried M (kept in lane p of its wave); then (ms, vs) of all 64 positions at
//              once into LDS, and a 64-bit mask of the positions that raised the maximum
//   (c) recurrence  thread = dim d of D / 16 pairs (8 or 4 independent chains that hide
//              the convert / mul / convert / add latency; each V value is loaded and
//              converted once).  ms = 1 wherever no new maximum appears, and scaling by 1
//              is exact, so positions without one in any of the thread's pairs (a
//              wave-uniform test of the masks, 4 positions at a time) skip the rescale; S runs
//              beside y.
//   causal     positions past a pair's pos0 + i are skipped, never multiplied by zero
//              (stale cache entries may be NaN): they score -inf in the scan, and in the
//              tiles that cross the diagonal every chain keeps its old value by select.
//   state      M per pair (phase a/b waves), S per pair and y per (pair, dim) (phase c)
// No KV-length limit of its own (launch_pf_attn_fa takes up to kFaMaxKV like the decode
// kernel, whose results it must equal).
#include "kernels.h"
#include "launch_util.h"
#include "mv_device.h"

namespace llmi {

namespace {

constexpr int kPfaPairs = 32;   // (row, head) pairs of a workgroup
constexpr int kPfaKT = 64;      // positions of a key tile
constexpr int kPfaThreads = 512;  // 8 waves, 2 per SIMD: the other wave runs while one waits for LDS
constexpr int kPfaPW = kPfaPairs / (kPfaThreads / 64);   // pairs of a wave in phases a and b

template <int D>
struct PfaLds {
    static constexpr int KROW = D * 2 + 16;   // bytes: 16-B pad, row-per-lane ds_read_b128 conflict-free
    static constexpr int VROW = kPfaKT * 2 + 16;
    static constexpr size_t K = 0;
    static constexpr size_t V = K + (size_t)kPfaKT * KROW;
    static constexpr size_t Q = V + (size_t)D * VROW;
    static constexpr size_t MS = Q + (size_t)kPfaPairs * D * 4;
    static constexpr size_t VS = MS + (size_t)kPfaPairs * kPfaKT * 4;
    static constexpr size_t NM = VS + (size_t)kPfaPairs * kPfaKT * 4;
    static constexpr size_t LIM = NM + (size_t)kPfaPairs * 8;
    static constexpr size_t TAB = LIM + (size_t)kPfaPairs * 4;   // llmi_exp2f_tab, 32 x 8 B
    static constexpr size_t BYTES = TAB + 32 * 8;
};

// the next key tile's K and V pieces of this thread (16 B each)
template <int D>
struct PfaStage {
    u32x4 k[D * 8 / kPfaThreads], v[D * 8 / kPfaThreads];
};
template <int D>
__device__ __forceinline__ void pfa_stage_load(PfaStage<D>& r, const uint16_t* kb, const uint16_t* vb, int n_ctx, int kt,
                                               int tmax) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < D * 8 / kPfaThreads; ++i) {
        const int ci = tid + kPfaThreads * i;
        // K: row ci / (D / 8), 8 dims from (ci % (D / 8)) * 8; rows past the last visible
        // position (never used) are clamped into the cache
        const int row = min(kt * kPfaKT + ci / (D / 8), tmax);
        r.k[i] = *(const u32x4*)(kb + (size_t)row * D + (ci % (D / 8)) * 8);
        // V: dim ci / 8, positions 8 (ci % 8) .. + 7 of the tile (n_ctx is a multiple of 8)
        const int t0 = min(kt * kPfaKT + (ci % 8) * 8, tmax & ~7);
        r.v[i] = *(const u32x4*)(vb + (size_t)(ci / 8) * n_ctx + t0);
    }
}
template <int D>
__device__ __forceinline__ void pfa_stage_store(const PfaStage<D>& r, uint8_t* lds) {
    using L = PfaLds<D>;
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < D * 8 / kPfaThreads; ++i) {
        const int ci = tid + kPfaThreads * i;
        *(u32x4*)(lds + L::K + (size_t)(ci / (D / 8)) * L::KROW + (ci % (D / 8)) * 16) = r.k[i];
        *(u32x4*)(lds + L::V + (size_t)(ci / 8) * L::VROW + (ci % 8) * 16) = r.v[i];
    }
}

// one position of one chain.  RESCALE: the position may carry ms != 1; MASK: `live`
// (wave-uniform) selects between the step and the old state
template <int X86, bool RESCALE, bool MASK>
__device__ __forceinline__ void pfa_step(float& y, float& S, float v, float ms, float vs, bool live) {
    float yn = y, Sn;
    if constexpr (RESCALE) yn = h2f(f2h(yn * ms));
    if constexpr (X86) {
        yn = h2f(f2h(__builtin_fmaf(v, vs, yn)));
        if constexpr (RESCALE) Sn = __builtin_fmaf(S, ms, vs);
        else Sn = S + vs;
    } else {
        yn = h2f(f2h(yn + v * vs));
        if constexpr (RESCALE) Sn = S * ms + vs;
        else Sn = S + vs;
    }
    if constexpr (MASK) {
        y = live ? yn : y;
        S = live ? Sn : S;
    } else {
        y = yn;
        S = Sn;
    }
}

// (b) of one pair: this lane's score s of position t -> the pair's factors of the tile.
// The running max is a prefix max: a 64-lane scan seeded with the carried M (lane ip of
// the wave holds it in Mreg); positions past the pair's last one (lim) score -inf -- they
// follow every live position, so no prefix that is used contains them.
__device__ __forceinline__ void pfa_factors(float s, float scale, int t, int lim, int ip, int p, float& Mreg, float* msv,
                                            float* vsv, uint32_t* nmv, const uint64_t* tab) {
    const int lane = threadIdx.x & 63;
    s = s * scale;
    s = s + 0.0f;  // + slope * mask (0 for every position the query sees)
    const bool live = t <= lim;
    if (!live) s = -INFINITY;
    float incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(incl, o);
        if (lane >= o) incl = fmaxf(incl, up);
    }
    float excl = __shfl_up(incl, 1);
    if (lane == 0) excl = -INFINITY;
    const float Mp = __shfl(Mreg, ip);
    const float prev = fmaxf(Mp, excl);
    const float tot = __shfl(incl, 63);
    if (lane == ip) Mreg = fmaxf(Mp, tot);
    // new maximum: ms = expf(Mold - s), vs = 1; else ms = 1, vs = expf(s - M) -- one call
    const bool up = s > prev;
    const float e = llmi_expf_glibc_tab(up ? prev - s : s - prev, 1, tab);
    const float ms = up ? e : 1.0f, vs = up ? 1.0f : e;
    msv[p * kPfaKT + lane] = ms;
    vsv[p * kPfaKT + lane] = vs;
    const unsigned long long nm = __ballot(up && live);
    if (lane == 0) {
        nmv[2 * p] = (uint32_t)nm;
        nmv[2 * p + 1] = (uint32_t)(nm >> 32);
    }
}

template <int D, int X86>
__global__ __launch_bounds__(kPfaThreads) void k_pf_attn_fa(PfAttn a, int T) {
    using L = PfaLds<D>;
    constexpr int PPG = kPfaPairs * D / kPfaThreads;  // pairs of a phase-c thread (kPfaThreads / D groups of them)
    constexpr int PW = kPfaPW;
    extern __shared__ __attribute__((aligned(16))) uint8_t pfa_lds[];
    uint8_t* lds = pfa_lds;
    float* qs = (float*)(lds + L::Q);
    float* msv = (float*)(lds + L::MS);
    float* vsv = (float*)(lds + L::VS);
    uint32_t* nmv = (uint32_t*)(lds + L::NM);
    int* limv = (int*)(lds + L::LIM);   // last position of each pair
    uint64_t* tab = (uint64_t*)(lds + L::TAB);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = a.gqa, TQ = kPfaPairs / G;
    const int g = blockIdx.x;
    const int row0 = ((int)gridDim.y - 1 - (int)blockIdx.y) * TQ;    // latest rows first
    const int tmax = a.pos0 + min(row0 + TQ, T) - 1;                 // last position any pair sees
    const int nt = tmax / kPfaKT + 1;
    const uint16_t* kb = a.kc + (size_t)g * a.n_ctx * D;
    const uint16_t* vb = a.vc + (size_t)g * D * a.n_ctx;
    // pair p: row min(p / G, TQ - 1) of the tile (clamped into the T rows), head p % G of
    // the group; pairs past TQ * G or T repeat a live one and are not stored
    auto pair_row = [&](int p) { return min(row0 + min(p / G, TQ - 1), T - 1); };

    PfaStage<D> st;
    pfa_stage_load<D>(st, kb, vb, a.n_ctx, 0, tmax);
    for (int i = tid; i < kPfaPairs * D; i += kPfaThreads) {
        const int p = i / D, d = i % D;
        qs[i] = h2f(f2h(a.q[(size_t)pair_row(p) * a.ldq + (size_t)(g * G + p % G) * D + d]));
    }
    // phase-c state: dim dd of pairs pg0 .. pg0 + PPG - 1
    const int dd = tid % D, pg0 = (tid / D) * PPG;
    float y[PPG], S[PPG];
#pragma unroll
    for (int i = 0; i < PPG; ++i) y[i] = S[i] = 0.f;
    if (tid < kPfaPairs) limv[tid] = a.pos0 + pair_row(tid);
    if (tid >= 64 && tid < 96) tab[tid - 64] = llmi_exp2f_tab((uint32_t)tid - 64);
    // phase-a/b state: lane l < PW of wave w carries M of pair PW w + l
    float Mreg = -INFINITY;

    for (int kt = 0; kt < nt; ++kt) {
        __syncthreads();  // the tile before is done with K, V and the factors
        pfa_stage_store<D>(st, lds);
        __syncthreads();
        if (kt + 1 < nt) pfa_stage_load<D>(st, kb, vb, a.n_ctx, kt + 1, tmax);
        // ---- (a) scores of this lane's key for the wave's 8 pairs, (b) their factors
        const uint8_t* krow = lds + L::K + (size_t)lane * L::KROW;
        if constexpr (X86) {
            uint32_t kr[D / 2];
#pragma unroll
            for (int c = 0; c < D / 8; ++c) {
                const u32x4 kv = *(const u32x4*)(krow + 16 * c);
                kr[4 * c] = kv[0]; kr[4 * c + 1] = kv[1]; kr[4 * c + 2] = kv[2]; kr[4 * c + 3] = kv[3];
            }
#pragma unroll 1
            for (int ip = 0; ip < PW; ++ip) {
                const float* qp = qs + (size_t)(PW * wave + ip) * D;
                // keep the row packed: converted out of this loop it would take D f32 registers
                // (the fmas read the f16 halves directly, v_fma_mix_f32)
#pragma unroll
                for (int c = 0; c < D / 2; ++c) __asm__ volatile("" : "+v"(kr[c]));
                float acc[32];
#pragma unroll
                for (int i = 0; i < 32; ++i) acc[i] = 0.f;
#pragma unroll
                for (int d0 = 0; d0 < D; d0 += 4) {
                    const float4 q4 = *(const float4*)(qp + d0);
                    const float qv[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = d0 + j;
                        acc[i & 31] = __builtin_fmaf(h2f(kr[i >> 1] >> (16 * (i & 1))), qv[j], acc[i & 31]);
                    }
                }
                float c[8];
#pragma unroll
                for (int l = 0; l < 8; ++l) c[l] = (acc[l] + acc[16 + l]) + (acc[8 + l] + acc[24 + l]);
                const float t0 = c[0] + c[4], t1 = c[1] + c[5], t2 = c[2] + c[6], t3 = c[3] + c[7];
                pfa_factors((float)(double)((t0 + t1) + (t2 + t3)), a.scale, kt * kPfaKT + lane, limv[PW * wave + ip], ip,
                            PW * wave + ip, Mreg, msv, vsv, nmv, tab);
            }
        } else {
            double sum[PW];
#pragma unroll
            for (int ip = 0; ip < PW; ++ip) sum[ip] = 0.0;
#pragma unroll 1
            for (int d0 = 0; d0 < D; d0 += 8) {
                const u32x4 kv = *(const u32x4*)(krow + 2 * d0);
                float kf[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) kf[j] = h2f(kv[j >> 1] >> (16 * (j & 1)));
#pragma unroll
                for (int ip = 0; ip < PW; ++ip) {
                    const float* qp = qs + (size_t)(PW * wave + ip) * D + d0;
                    const float4 qa = *(const float4*)qp, qb = *(const float4*)(qp + 4);
                    const float qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
                    for (int j = 0; j < 8; ++j) sum[ip] += (double)(kf[j] * qv[j]);
                }
            }
#pragma unroll 1
            for (int ip = 0; ip < PW; ++ip) {  // rolled: one copy of the factors' code (and of expf's constants)
                double sp = sum[0];
#pragma unroll
                for (int k = 1; k < PW; ++k) sp = ip == k ? sum[k] : sp;
                pfa_factors((float)sp, a.scale, kt * kPfaKT + lane, limv[PW * wave + ip], ip, PW * wave + ip, Mreg, msv, vsv, nmv,
                            tab);
            }
        }
        __syncthreads();
        // ---- (c) the recurrence of dim dd over the tile's positions
        uint32_t any_lo = 0, any_hi = 0;
#pragma unroll
        for (int i = 0; i < PPG; ++i) {
            any_lo |= nmv[2 * (pg0 + i)];
            any_hi |= nmv[2 * (pg0 + i) + 1];
        }
        const unsigned long long any = ((unsigned long long)(uint32_t)uniform((int)any_hi) << 32) | (uint32_t)uniform((int)any_lo);
        const bool diag = kt * kPfaKT + kPfaKT - 1 > a.pos0 + row0;  // some pair's last position is inside the tile
        const int nlive = min(kPfaKT, tmax - kt * kPfaKT + 1);       // positions of the tile any pair sees
        const uint8_t* vrow = lds + L::V + (size_t)dd * L::VROW;
        // 4 positions at a time; the next 4 positions' V and vs are read before this step's
        // chains run (one wave per SIMD: nothing else hides the LDS latency)
        const int n4 = (nlive + 3) / 4;
        u32x2 vn = *(const u32x2*)vrow;
        float4 vsn[PPG];
#pragma unroll
        for (int i = 0; i < PPG; ++i) vsn[i] = *(const float4*)(vsv + (pg0 + i) * kPfaKT);
#pragma unroll 1
        for (int t4 = 0; t4 < n4; ++t4) {
            const u32x2 vv = vn;
            float vs4[PPG][4];
#pragma unroll
            for (int i = 0; i < PPG; ++i) { vs4[i][0] = vsn[i].x; vs4[i][1] = vsn[i].y; vs4[i][2] = vsn[i].z; vs4[i][3] = vsn[i].w; }
            const int tn = min(t4 + 1, kPfaKT / 4 - 1);
            vn = *(const u32x2*)(vrow + 8 * tn);
#pragma unroll
            for (int i = 0; i < PPG; ++i) vsn[i] = *(const float4*)(vsv + (pg0 + i) * kPfaKT + 4 * tn);
            float vf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) vf[j] = h2f(vv[j >> 1] >> (16 * (j & 1)));
            if (!diag && ((any >> (4 * t4)) & 15) == 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < PPG; ++i) pfa_step<X86, false, false>(y[i], S[i], vf[j], 1.0f, vs4[i][j], true);
            } else {
                const int tb = kt * kPfaKT + 4 * t4;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float msj[PPG];
#pragma unroll
                    for (int i = 0; i < PPG; ++i) msj[i] = msv[(pg0 + i) * kPfaKT + 4 * t4 + j];
                    if (!diag) {
#pragma unroll
                        for (int i = 0; i < PPG; ++i) pfa_step<X86, true, false>(y[i], S[i], vf[j], msj[i], vs4[i][j], true);
                    } else {
#pragma unroll
                        for (int i = 0; i < PPG; ++i)
                            pfa_step<X86, true, true>(y[i], S[i], vf[j], msj[i], vs4[i][j], tb + j <= uniform(limv[pg0 + i]));
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < PPG; ++i) {
        const int p = pg0 + i, row = row0 + p / G;
        if (p < TQ * G && row < T) {
            const float S_inv = S[i] == 0.0f ? 0.0f : 1.0f / S[i];
            a.out[(size_t)row * a.ldq + (size_t)(g * G + p % G) * D + dd] = y[i] * S_inv;
        }
    }
}

}  // namespace

hipError_t launch_pf_attn_fa(const PfAttn& a, int n_head, int head_dim, int T, hipStream_t s) {
    const int G = a.gqa;
    if (T <= 0 || G <= 0 || G > kPfaPairs || n_head % G || a.pos0 < 0 || a.pos0 + T > a.n_ctx || a.pos0 + T > kFaMaxKV ||
        a.n_ctx % 8)
        return hipErrorNotSupported;
    const int TQ = kPfaPairs / G;
    const dim3 grid(n_head / G, (T + TQ - 1) / TQ);
#define LLMI_PFA(D_, X_)                                                                                        \
    if (head_dim == D_ && (a.num ? 1 : 0) == X_) {                                                              \
        launch_k(k_pf_attn_fa<D_, X_>, grid, dim3(kPfaThreads), PfaLds<D_>::BYTES, s, true, true, a, T);        \
        return hipGetLastError();                                                                               \
    }
    LLMI_PFA(128, 0) LLMI_PFA(128, 1) LLMI_PFA(64, 0) LLMI_PFA(64, 1)
#undef LLMI_PFA
    return hipErrorNotSupported;
}

}  // namespace llmi
