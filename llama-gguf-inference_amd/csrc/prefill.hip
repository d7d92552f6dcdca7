// prefill.hip — batched prompt prefill on gfx950 MFMA.
// It shares mv_device.h's and pf_device.h's device helpers (unit-major weight planes, the
// activation quantizer, fp16 conversions, DPP lanes).
//
// A prompt of T tokens runs through the same llm_build_llama graph as T decode steps,
// but every linear layer is ONE launch over all T tokens, so each weight byte is read
// T/32 times instead of T times, and the integer dot products run on the matrix cores:
//
//   k_pf_embed   get_rows for T tokens (dequant_elem, as k_embed)
//   k_pf_quant   [RMSNorm] + quantize_row_q8_K_ref / _q8_0_ref of T rows (the matvec
//                prologue, bit-exact), written as f16 MFMA fragments (below) with the
//                block d and the bsum pairs
//   k_pf_gemm    Y[t][row] in ggml's generic order (mv_device.h), the integer sums from
//                v_mfma_f32_16x16x32_f16 (next paragraph), the fp32 chains on the VALU
//   k_pf_fa      causal attention of T query tokens with ggml's non-flash numerics, tiled
//                on the FP64 matrix cores (k_pf_attn_g / k_pf_attn: the LDS-resident paths
//                for head shapes it does not take)
// The last prompt token then runs as an ordinary decode step (logits, argmax feedback).
//
// Exact integer sums on an f16 MFMA.  ggml's generic K-quant dot needs, per 256-block,
// aux32[l] = sum over the block's elements e = l (mod 8) of scale(e) * q(e) * a(e).  The
// K dimension of one MFMA is that residue class (32 elements: 4 per 32-element
// sub-block for Q4_K/Q5_K, 2 per 16-element sub-block for Q6_K), A = the q8 activations
// as f16 (|a| <= 127, exact), B = q(e) * scale(e) as f16 — exact for Q4_K (<= 15*63) and
// Q5_K (<= 31*63 < 2048); Q6_K's (q-32)*sc (up to 4096) is split as sc = 16*sh + sl into
// two MFMAs (|(q-32)*sl| <= 480, |(q-32)*sh| <= 256).  Every product and every partial
// sum is an integer below 2^24, so the f32 accumulation is exact in any order and the
// accumulator equals (float)aux32[l] (Q6_K: 16*acc_h + acc_l, exact as well).  Q8_0: K
// = one 32-block, B = the int8 weights, the accumulator = sumi.  The VALU then runs the
// generic fp32 chains: sums[l] += (d_w*d_a)*aux, sumf -= (dmin_w*d_a)*sumi (sumi from the
// bsum pairs by v_dot2), Q8_0 sumf += sumi*(d_w*d_a), and sumf += sums[0..7] at the end —
// so prefill logits and KV rows equal T decode steps and the oracle bit for bit.
//
// Fragment order of a K-quant block (element e = 64 g + 32 h + l + 8 i of the block):
// MFMA k = 8 g + 4 h + i for residue l, i.e. lane group g = chunk g of the block, which
// is the weight layout's residue-order chunk (common.h): dword l%4 of part 2g + l/4 of the
// unit holds exactly the 8 weights of residue l of chunk g (low nibbles h = 0, high h = 1).
#include "kernels.h"
#include "launch_util.h"
#include "mv_device.h"
#include "pf_device.h"

#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>

namespace llmi {

constexpr int kPfRows = 64;         // weight rows per workgroup (16 per wave)
constexpr int kPfStage = 16384;      // bytes of f16 activation fragments per stage (256 K x 32 tokens)


// ---------------------------------------------------------------------------------
// k_pf_quant: grid (T, chunks); the matvec prologue of row t into LDS (a chunk of bpc
// 256-element blocks per workgroup when the row is split: every chunk's workgroup takes the
// row's RMSNorm scale the same way, then quantizes its own blocks), then out as
//   aq: f16 MFMA fragments [T/32][stage][32 entries][32 tokens][8 f16], a stage = 256
//       elements (K-quants: one block, entry = 4 l + g; Q8_0: eight 32-blocks, entry =
//       4 block + g, natural element order)
//   abs: K-quants: bsum pairs [T][blocks][8] int16 (bs[2j] + bs[2j+1])
//   abf: K-quants, optional: the bsum pairs as the A fragments of k_pf_gemm's sumi MFMA
//        [T/32][stage][4 g][32 tokens][8 f16] = (lo, hi) of pairs 2g, 2g + 1 and four
//        zeros, pair = 64 hi + lo with lo in [0, 63] (both exact in f16)
//   ad:  the activation block d [T][blocks] (q8_K: per 256; q8_0: per 32, f16-rounded)
// ---------------------------------------------------------------------------------
template <int ACT, bool NORM, int X86 = 0>
__global__ __launch_bounds__(kMVThreads) void k_pf_quant(MVArgs A, int ldx, uint8_t* aq, int16_t* abs, float* ad,
                                                         uint8_t* abf, int bpc) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const Lds L = carve(smem, ACT, A.cols);
    const int t = blockIdx.x, cols = A.cols, nstage = cols >> 8;
    const int b0 = blockIdx.y * bpc, b1 = min(nstage, b0 + bpc);  // this workgroup's 256-element blocks
    A.x += (size_t)t * ldx;
    if (b0 == 0 && b1 == nstage) {
        mv_prologue<ACT, NORM, X86>(A, L);
    } else {
        ProRegs<NORM, 1> R;
        if constexpr (NORM) mv_prologue_issue<NORM, 1>(A, R);
        const float scale = mv_norm_scale<NORM, 1>(A, L, R);
        for (int sb = 16 * b0 + (int)threadIdx.x; sb < 16 * b1; sb += kMVThreads) {  // 16-lane groups = one block
            float v[16], w[16];
            load_sub<NORM, 1>(A, R, 1, sb, v, w);
            if constexpr (NORM) {
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = (v[j] * scale) * w[j];
            }
            quant_sub<ACT, X86>(L, cols, sb, v);
        }
    }
    __syncthreads();
    // (X86: the record's byte order is the weights' x86 one, so the same entry reads give
    // x86 lane l of chunk g)
    for (int f = 32 * b0 + (int)threadIdx.x; f < b1 * 32; f += kMVThreads) {
        const int stage = f >> 5, entry = f & 31;
        const uint8_t* rec = L.act + (size_t)stage * kRec;
        const uint8_t* lo;
        if constexpr (ACT == 0) {  // residue l = entry / 4 of chunk g = entry % 4: LO / HI bytes 4(l%4) .. +3 of part 2g + l/4
            const int l = entry >> 2, g = entry & 3;
            lo = rec + 32 * (2 * g + (l >> 2)) + 4 * (l & 3);
        } else {  // 32-block entry / 4 of the unit, elements 8 g .. 8 g + 7 (natural order)
            lo = rec + 32 * (entry >> 2) + 8 * (entry & 3);
        }
        const uint32_t wl = *(const uint32_t*)lo, wh = *(const uint32_t*)(lo + (ACT == 0 ? 16 : 4));
        h8 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = (_Float16)(float)(int8_t)(wl >> (8 * j));
            v[4 + j] = (_Float16)(float)(int8_t)(wh >> (8 * j));
        }
        *(h8*)(aq + pf_aq_off(t, stage, entry, nstage)) = v;
    }
    if constexpr (ACT == 0) {
        for (int i = 8 * b0 + (int)threadIdx.x; i < 8 * b1; i += kMVThreads) {
            const int16_t* bs = (const int16_t*)(L.act + (size_t)(i >> 3) * kRec + kRecBs) + 2 * (i & 7);
            abs[(size_t)t * (cols >> 5) + i] = (int16_t)(bs[0] + bs[1]);
        }
        if (abf)
            for (int f = 4 * b0 + (int)threadIdx.x; f < 4 * b1; f += kMVThreads) {
                const int16_t* bs = (const int16_t*)(L.act + (size_t)(f >> 2) * kRec + kRecBs) + 4 * (f & 3);
                h8 v;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int pr = bs[2 * k] + bs[2 * k + 1];
                    v[2 * k] = (_Float16)(float)(pr & 63);
                    v[2 * k + 1] = (_Float16)(float)(pr >> 6);
                    v[4 + 2 * k] = (_Float16)0.f;
                    v[5 + 2 * k] = (_Float16)0.f;
                }
                *(h8*)(abf + pf_abf_off(t, f >> 2, f & 3, nstage)) = v;
            }
        for (int b = b0 + (int)threadIdx.x; b < b1; b += kMVThreads)
            ad[(size_t)t * (cols / 256) + b] = *(const float*)(L.act + (size_t)b * kRec + kRecD);
    } else {
        for (int b = 8 * b0 + (int)threadIdx.x; b < 8 * b1; b += kMVThreads)
            ad[(size_t)t * (cols / 32) + b] = *(const float*)(L.act + (size_t)(b >> 3) * kRec + kRecBs + 4 * (b & 7));
    }
}

// ---------------------------------------------------------------------------------
// k_pf_embed: grid (ceil(cols/256), T): X[t] = token_embd row of toks[t]; hist[pos0+t]
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pf_embed(Seg w, int cols, int vocab, const int32_t* toks, float* X, int T,
                                                  int32_t* hist, int pos0, int n_ctx) {
    const int t = blockIdx.y;
    int tok = toks[t];
    if (tok < 0 || tok >= vocab) tok = 0;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < cols) X[(size_t)t * cols + e] = dequant_elem(w, tok, e, cols);
    if (blockIdx.x == 0 && threadIdx.x == 0 && pos0 + t < n_ctx) hist[pos0 + t] = tok;
}

// ---------------------------------------------------------------------------------
// k_pf_gemm: grid (rows / 64, Tpad / (32 NG)), 256 threads.  Wave w owns weight rows
// [64 bx + 16 w, +16) for the workgroup's 32 NG tokens (2 NG 16-token tiles), so every
// B fragment it builds (q * scale of 16 rows, one residue) feeds 2 NG MFMAs.  Per stage
// (256 elements of K) the activation fragments of the NG token groups (NG x 16 KB), the
// block d and the bsum pairs go global -> LDS by LDS-DMA (global_load_lds, no VGPRs),
// issued one stage ahead into the other half of a double buffer; the weights of the next
// stage load into registers at the same time; ONE barrier per stage (its vmcnt(0) retires
// both, and it orders every wave's reads of a buffer before that buffer is restaged).
// SWIGLU runs gate then up as one stream of 2 x nstage steps.  Per residue l the wave
// builds B = q * scale as f16 (lane: row lane & 15, chunk lane >> 4), runs one MFMA per
// token tile and folds the accumulator into the row's chains with packed f32 math
// (v_pk_mul_f32 / v_pk_add_f32: two tokens per instruction, each its own IEEE mul and
// add, so the generic order is kept).  C/D: lane holds row lane & 15 for tokens
// 4 (lane >> 4) + i of each tile.
// ---------------------------------------------------------------------------------
typedef float f2v __attribute__((ext_vector_type(2)));
// two-token f32 ops of the chains: packed v_pk_*_f32 (LLMI_PK=1) or two scalar ops (build
// with -fno-slp-vectorize so they stay scalar); each element is its own IEEE op either way
#ifndef LLMI_PK
#define LLMI_PK 1
#endif
__device__ __forceinline__ f2v mul2(f2v a, f2v b) {
    if constexpr (LLMI_PK) return a * b;
    else return f2v{a[0] * b[0], a[1] * b[1]};
}
__device__ __forceinline__ f2v add2(f2v a, f2v b) {
    if constexpr (LLMI_PK) return a + b;
    else return f2v{a[0] + b[0], a[1] + b[1]};
}
__device__ __forceinline__ f2v sub2(f2v a, f2v b) {
    if constexpr (LLMI_PK) return a - b;
    else return f2v{a[0] - b[0], a[1] - b[1]};
}
__device__ __forceinline__ f2v fma2(f2v a, f2v b, f2v c) {
    if constexpr (LLMI_PK) return __builtin_elementwise_fma(a, b, c);
    else return f2v{__builtin_fmaf(a[0], b[0], c[0]), __builtin_fmaf(a[1], b[1], c[1])};
}
typedef __attribute__((address_space(3))) void* lds_vp;
typedef __attribute__((address_space(1))) void* glb_vp;
template <int NG>
struct PfBuf {
    static constexpr size_t A = (size_t)NG * kPfStage;     // [NG][32 entries][32 tokens][16 B] (the global layout)
    static constexpr size_t DA = (size_t)NG * 32 * 8 * 4;  // d: K-quants [32 NG] floats, Q8_0 [32 NG][8]
    static constexpr size_t BF = (size_t)NG * 2048;        // K-quants: [NG][4 g][32 tokens][16 B] sumi A fragments
    static constexpr size_t BYTES = A + DA + BF;
};
// stage `stage` of the token groups at tok0 into LDS buffer `buf` (LDS-DMA: destination
// = wave-uniform base + 16 B (4 B) per lane)
template <int ACT, int NG>
__device__ __forceinline__ void pf_stage_dma(const PfGemm& g, int tok0, int stage, uint8_t* buf) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nstage = g.cols >> 8;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const uint8_t* src = (const uint8_t*)g.aq + pf_aq_off(tok0 + 32 * j, stage, 0, nstage);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int kb = 4 * wave + k;  // 1 KB piece of the group's 16 KB
            __builtin_amdgcn_global_load_lds((glb_vp)(src + kb * 1024 + lane * 16), (lds_vp)(buf + j * kPfStage + kb * 1024),
                                             16, 0, 0);
        }
    }
    uint8_t* da = buf + PfBuf<NG>::A;
    if constexpr (ACT == 0) {
        if (wave == 1 && lane < 32 * NG)  // token lane: d of the stage's block
            __builtin_amdgcn_global_load_lds((glb_vp)(g.ad + (size_t)(tok0 + lane) * nstage + stage), (lds_vp)da, 4, 0, 0);
        if (wave >= 2)  // the groups' 2 KB of sumi fragments: 1 KB per wave-instruction
#pragma unroll
            for (int j = 0; j < NG; ++j)
                __builtin_amdgcn_global_load_lds(
                    (glb_vp)((const uint8_t*)g.abf + pf_abf_off(tok0 + 32 * j, stage, 0, nstage) + (wave - 2) * 1024 + lane * 16),
                    (lds_vp)(buf + PfBuf<NG>::A + PfBuf<NG>::DA + j * 2048 + (wave - 2) * 1024), 16, 0, 0);
    } else {  // lane: token 32 j + lane / 2, blocks 4 (lane & 1) .. +3 of the stage
        if (wave == 1)
#pragma unroll
            for (int j = 0; j < NG; ++j)
                __builtin_amdgcn_global_load_lds(
                    (glb_vp)(g.ad + (size_t)(tok0 + 32 * j + (lane >> 1)) * (g.cols >> 5) + 8 * stage + 4 * (lane & 1)),
                    (lds_vp)(da + j * 1024), 16, 0, 0);
    }
}

// X86 = 1: the x86 association (mv_device.h "x86 numerics"): per lane l the chain
// acc[l] = fma(d_a * d_w, (float)sumi[l], acc[l]), Q4_K's four min lanes (one sumi MFMA per
// lane group: group g's K slice is exactly prod[g]) / Q5_K's one fma min chain, result
// hsum_float_8(acc) [+ min lanes]; Q8_0: per 32-block, lane l's 4 elements by one MFMA each
// (eight per block and token tile instead of one: the weights of the other lanes zeroed)
template <int T, int EPI, int NG, int X86 = 0>
// two workgroups per CU (<= 256 registers) where that costs no spills in the step loop
__global__ __launch_bounds__(256, T == T_Q8_0 ? 1 : 2) void k_pf_gemm(PfGemm g) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int ACT = T == T_Q8_0 ? 1 : 0, NTL = 2 * NG, NP = 2 * NTL;  // NP token pairs per lane
    constexpr size_t BUF = PfBuf<NG>::BYTES;
    // tile of this workgroup: XCD-aware when g.xcd_map (workgroup w runs on XCD w % 8; XCD
    // k takes tiles [k n/8, (k+1) n/8) in order, token groups fastest, so the token groups
    // of a row block run back to back on one XCD and share its L2 copy of the weights)
    // (g.xcd_map = SY > 1: the token groups in chunks of SY, each chunk row block by row
    // block, so an XCD's L2 holds SY groups' activations while the weights stream past)
    int bx = blockIdx.x, by = blockIdx.y;
    if (g.xcd_map) {
        const int n = gridDim.x * gridDim.y, w = blockIdx.y * gridDim.x + blockIdx.x;
        const int t = (w & 7) * (n >> 3) + (w >> 3);
        const int sy = g.xcd_map, per = (int)gridDim.x * sy, c = t / per, rem = t - c * per;
        bx = rem / sy;
        by = c * sy + (rem - bx * sy);
    }
    const int tok0 = by * 32 * NG;
    const int wave = uniform((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int row0 = bx * kPfRows + wave * 16;
    const int nstage = g.cols >> 8;
    const bool wave_on = row0 < g.rows;  // uniform per wave (rows % 16 == 0)
    const int grp = lane >> 4, tq = 4 * grp;
    constexpr int NW = EPI == EPI_SWIGLU ? 2 : 1;  // weight matrices (SWIGLU: gate, up)
    // QKV: the workgroup's part and its rows within that part (merged launches, g.r1 > 0)
    int part = g.part, lrow0 = row0;
    if constexpr (EPI == EPI_QKV) {
        const int wg_row = bx * kPfRows;
        if (g.r1 > 0 && wg_row >= g.r1) {
            if (wg_row < g.r2) {
                part += 1;
                lrow0 -= g.r1;
            } else {
                part += 2;
                lrow0 -= g.r2;
            }
        }
    }
    const int row = lrow0 + (lane & 15);
#if defined(LLMI_EXPERIMENTS)
    const int wrow = (g.exp & 1) ? lrow0 : row;  // experiment: the wave's weights from one row (hot, coalesced)
#else
    const int wrow = row;
#endif
    RowPtr rp[NW];
    if constexpr (EPI == EPI_QKV) {
        const int lr = wave_on ? wrow : 0;
        if (part == g.part) rp[0] = row_ptr<T>(g.w, lr, g.cols);
        else if (part == g.part + 1) rp[0] = row_ptr<T>(g.wk, lr, g.cols);
        else rp[0] = row_ptr<T>(g.wv, lr, g.cols);
    } else {
#pragma unroll
        for (int wi = 0; wi < NW; ++wi) rp[wi] = row_ptr<T>(wi ? g.w2 : g.w, wave_on ? wrow : 0, g.cols);
    }
    const int nsteps = NW * nstage;
    pf_stage_dma<ACT, NG>(g, tok0, 0, smem);
    PfW<T> wcur = pf_w_load<T>(rp[0], 0, nstage);
    f2v res[NW][NP];
    // chains, token pair p = 2 tile + h: tokens 4 grp + 2h, +1 of the tile
    // (X86: sums = the 8 lane chains, sumf = Q5_K's summs, accm = Q4_K's min lanes)
    f2v sums[8][NP], sumf[NP];
    constexpr int NM = (X86 && T == T_Q4_K) ? 4 : 1;
    [[maybe_unused]] f2v accm[NM][NP];
    __syncthreads();
    for (int step = 0; step < nsteps; ++step) {
        const int wi = step >= nstage ? 1 : 0, st = step - wi * nstage;
        if (st == 0) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                sumf[p] = f2v{0.f, 0.f};
#pragma unroll
                for (int l = 0; l < 8; ++l) sums[l][p] = f2v{0.f, 0.f};
                if constexpr (X86 && T == T_Q4_K) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) accm[k][p] = f2v{0.f, 0.f};
                }
            }
        }
        const uint8_t* B = smem + (step & 1) * BUF;
        const float* Lda = (const float*)(B + PfBuf<NG>::A);
        const uint8_t* Lbf = B + PfBuf<NG>::A + PfBuf<NG>::DA;
        // next step: its activations by LDS-DMA, its weights into registers (the last step
        // re-reads itself: unconditional loads keep the weight struct out of scratch)
        const int nx = step + 1 < nsteps ? step + 1 : step, wn = nx >= nstage ? 1 : 0, stn = nx - wn * nstage;
        if (step + 1 < nsteps) pf_stage_dma<ACT, NG>(g, tok0, stn, smem + ((step + 1) & 1) * BUF);
        PfW<T> wnxt = pf_w_load<T>(rp[wn], stn, nstage);
        if (wave_on) {
            auto afrag = [&](int l, int tl) -> h8 {
                return *(const h8*)(B + (tl >> 1) * kPfStage + ((size_t)(4 * l + grp) * 32 + 16 * (tl & 1) + (lane & 15)) * 16);
            };
            if constexpr (T == T_Q8_0 && X86) {
                // x86 lane j of a 32-block = its elements 4j..4j+3 = half j % 2 of lane group
                // j / 2's fragment: one MFMA per lane with the other weights zeroed gives
                // sumi[j] exactly; acc[j] = fma(d_w * d_a, (float)sumi[j], acc[j]) in block order
#pragma unroll
                for (int l = 0; l < 8; ++l) {  // 32-block 8 st + l
                    h8 bf;
                    pf_build_b<T>(wcur, l, h2{}, h2{}, h2{}, h2{}, nullptr, nullptr, &bf);
                    const float dw = h2f(wcur.dd[l >> 1] >> (16 * (l & 1)));
#pragma unroll
                    for (int tl = 0; tl < NTL; ++tl) {
                        const h8 af = afrag(l, tl);
                        f2v d[2];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int t0 = 16 * tl + tq + 2 * h;
                            d[h] = mul2(f2v{dw, dw}, f2v{Lda[t0 * 8 + l], Lda[(t0 + 1) * 8 + l]});
                        }
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const bool mine = grp == (j >> 1);
                            h8 bj;
#pragma unroll
                            for (int e = 0; e < 8; ++e) bj[e] = (mine && (e >> 2) == (j & 1)) ? bf[e] : (_Float16)0.f;
                            const f4 acc = mfma16(af, bj, f4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                            for (int h = 0; h < 2; ++h)
                                sums[j][2 * tl + h] = fma2(d[h], f2v{acc[2 * h], acc[2 * h + 1]}, sums[j][2 * tl + h]);
                        }
                    }
                }
            } else if constexpr (T == T_Q8_0) {
#pragma unroll
                for (int l = 0; l < 8; ++l) {  // 32-block 8 st + l
                    h8 bf;
                    pf_build_b<T>(wcur, l, h2{}, h2{}, h2{}, h2{}, nullptr, nullptr, &bf);
                    const float dw = h2f(wcur.dd[l >> 1] >> (16 * (l & 1)));
#pragma unroll
                    for (int tl = 0; tl < NTL; ++tl) {
                        const f4 acc = mfma16(afrag(l, tl), bf, f4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int t0 = 16 * tl + tq + 2 * h;
                            const f2v da = f2v{Lda[t0 * 8 + l], Lda[(t0 + 1) * 8 + l]};
                            const f2v a2 = f2v{acc[2 * h], acc[2 * h + 1]};
                            sumf[2 * tl + h] = add2(sumf[2 * tl + h], mul2(a2, mul2(f2v{dw, dw}, da)));
                        }
                    }
                }
            } else {
                h2 slo{}, shi{}, slo_o{}, shi_o{};
                h2 s6[8], s6o[8];
                float dw, dmw = 0.f;
                h8 bm{};  // sumi B fragment: (min, 64 min) of sub-blocks 2 grp, 2 grp + 1
                if constexpr (T == T_Q4_K || T == T_Q5_K) {
                    int sc0, m0, sc1, m1;
                    scale_min(2 * grp, wcur.hdr.y, wcur.hdr.z, wcur.hdr.w, sc0, m0);
                    scale_min(2 * grp + 1, wcur.hdr.y, wcur.hdr.z, wcur.hdr.w, sc1, m1);
                    slo = h2{(_Float16)(float)sc0, (_Float16)(float)sc0};
                    shi = h2{(_Float16)(float)sc1, (_Float16)(float)sc1};
                    slo_o = slo * h2{(_Float16)1024.f, (_Float16)1024.f};
                    shi_o = shi * h2{(_Float16)1024.f, (_Float16)1024.f};
                    dw = h2f(wcur.hdr.x);
                    dmw = h2f(wcur.hdr.x >> 16);
                    bm[0] = (_Float16)(float)m0;
                    bm[1] = (_Float16)(float)(64 * m0);
                    bm[2] = (_Float16)(float)m1;
                    bm[3] = (_Float16)(float)(64 * m1);
                } else {  // Q6_K: sc = 16 sh + sl per sub-block 4 grp + k
                    dw = h2f(wcur.d);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int sc = (int)(int8_t)(wcur.sc >> (8 * k));
                        const int sh = sc >> 4, sl = sc & 15;  // floor division: sc = 16 sh + sl
                        const _Float16 fl = (_Float16)(float)sl, fh = (_Float16)(float)sh;
                        s6[2 * k] = h2{fl, fl};
                        s6[2 * k + 1] = h2{fh, fh};
                        s6o[2 * k] = s6[2 * k] * h2{(_Float16)1056.f, (_Float16)1056.f};
                        s6o[2 * k + 1] = s6[2 * k + 1] * h2{(_Float16)1056.f, (_Float16)1056.f};
                    }
                }
                f2v d[NP];  // d_w * d_a per token pair
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const int t0 = 16 * (p >> 1) + tq + 2 * (p & 1);
                    d[p] = mul2(f2v{dw, dw}, f2v{Lda[t0], Lda[t0 + 1]});
                }
#pragma unroll
                for (int l = 0; l < 8; ++l) {
                    h8 bf[2];
                    pf_build_b<T, X86>(wcur, l, slo, shi, slo_o, shi_o, s6, s6o, bf);
#pragma unroll
                    for (int tl = 0; tl < NTL; ++tl) {
                        const h8 af = afrag(l, tl);
                        f4 acc = mfma16(af, bf[0], f4{0.f, 0.f, 0.f, 0.f});
                        if constexpr (T == T_Q6_K) {
                            const f4 acc_h = mfma16(af, bf[1], f4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                            for (int h = 0; h < 2; ++h) {  // acc_h * 16 + acc: exact (< 2^24), so one fma
                                const f2v v = fma2(f2v{acc_h[2 * h], acc_h[2 * h + 1]}, f2v{16.f, 16.f},
                                                                        f2v{acc[2 * h], acc[2 * h + 1]});
                                acc[2 * h] = v[0];
                                acc[2 * h + 1] = v[1];
                            }
                        }
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            if constexpr (X86)
                                sums[l][2 * tl + h] = fma2(d[2 * tl + h], f2v{acc[2 * h], acc[2 * h + 1]}, sums[l][2 * tl + h]);
                            else
                                sums[l][2 * tl + h] = add2(sums[l][2 * tl + h], mul2(d[2 * tl + h], f2v{acc[2 * h], acc[2 * h + 1]}));
                        }
                    }
                }
                if constexpr (X86 && T == T_Q4_K) {  // acc_m[k] = fma(-d_a * dmin_w, (float)prod[k], acc_m[k]), prod[k] = lane group k's slice
#pragma unroll
                    for (int tl = 0; tl < NTL; ++tl) {
                        const h8 af = *(const h8*)(Lbf + (tl >> 1) * 2048 + ((size_t)grp * 32 + 16 * (tl & 1) + (lane & 15)) * 16);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const f4 si = mfma16(af, grp == k ? bm : h8{}, f4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                const int t0 = 16 * tl + tq + 2 * h;
                                const f2v dm = mul2(f2v{-Lda[t0], -Lda[t0 + 1]}, f2v{dmw, dmw});
                                accm[k][2 * tl + h] = fma2(dm, f2v{si[2 * h], si[2 * h + 1]}, accm[k][2 * tl + h]);
                            }
                        }
                    }
                } else if constexpr (X86 && T == T_Q5_K) {  // summs = fma(-d_a * dmin_w, (float)sumi, summs)
#pragma unroll
                    for (int tl = 0; tl < NTL; ++tl) {
                        const h8 af = *(const h8*)(Lbf + (tl >> 1) * 2048 + ((size_t)grp * 32 + 16 * (tl & 1) + (lane & 15)) * 16);
                        const f4 si = mfma16(af, bm, f4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int t0 = 16 * tl + tq + 2 * h;
                            const f2v dm = mul2(f2v{-Lda[t0], -Lda[t0 + 1]}, f2v{dmw, dmw});
                            sumf[2 * tl + h] = fma2(dm, f2v{si[2 * h], si[2 * h + 1]}, sumf[2 * tl + h]);
                        }
                    }
                } else if constexpr (T != T_Q6_K) {  // sumf -= (dmin * d_a) * sumi; sumi = mins . bsum pairs on the MFMA (exact)
#pragma unroll
                    for (int tl = 0; tl < NTL; ++tl) {
                        const h8 af = *(const h8*)(Lbf + (tl >> 1) * 2048 + ((size_t)grp * 32 + 16 * (tl & 1) + (lane & 15)) * 16);
                        const f4 si = mfma16(af, bm, f4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                        for (int h = 0; h < 2; ++h) {  // dmin_w * d_a (d_a read again: fewer live registers)
                            const int t0 = 16 * tl + tq + 2 * h;
                            const f2v dm = mul2(f2v{dmw, dmw}, f2v{Lda[t0], Lda[t0 + 1]});
                            sumf[2 * tl + h] = sub2(sumf[2 * tl + h], mul2(dm, f2v{si[2 * h], si[2 * h + 1]}));
                        }
                    }
                }
            }
        }
        if (st == nstage - 1) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                f2v v = sumf[p];
                if constexpr (X86) {  // hsum_float_8(acc) [+ min lanes (Q4_K) / summs (Q5_K)]
                    const f2v t0 = add2(sums[0][p], sums[4][p]), t1 = add2(sums[1][p], sums[5][p]);
                    const f2v t2 = add2(sums[2][p], sums[6][p]), t3 = add2(sums[3][p], sums[7][p]);
                    v = add2(add2(t0, t2), add2(t1, t3));
                    if constexpr (T == T_Q4_K) v = add2(v, add2(add2(accm[0][p], accm[2][p]), add2(accm[1][p], accm[3][p])));
                    if constexpr (T == T_Q5_K) v = add2(v, sumf[p]);
                } else if constexpr (T != T_Q8_0) {
#pragma unroll
                    for (int l = 0; l < 8; ++l) v = add2(v, sums[l][p]);
                }
                res[wi][p] = v;
            }
        }
        __syncthreads();  // vmcnt(0): the next step's DMA and weights landed; every wave is done with this buffer
        wcur = wnxt;
    }
    if (!wave_on) return;
    float v[2 * NP];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            v[2 * p + h] = res[0][p][h];
            if constexpr (EPI == EPI_SWIGLU)
                v[2 * p + h] = (X86 ? x86_silu(res[0][p][h]) : llmi_silu(res[0][p][h])) * res[NW - 1][p][h];
        }
    if constexpr (EPI == EPI_QKV) {
        const int hd = g.head_dim, hh = row / hd, dd = row - hh * hd;
#pragma unroll
        for (int k = 0; k < 2 * NP; ++k) {
            const int t = tok0 + 16 * (k >> 2) + tq + (k & 3);
            const float pv = xor_partner<1>(v[k]);  // the RoPE partner row (d ^ 1): lane ^ 1
            if (t >= g.T) continue;
            const int pos = g.pos0 + t;
            float o = v[k];
            if (part < 2 && dd < g.n_rot) {
                const float2 cs = *(const float2*)(g.rope + ((size_t)pos * (g.n_rot / 2) + dd / 2) * 2);
                const float va = (dd & 1) ? pv : v[k], vb = (dd & 1) ? v[k] : pv;
                o = (dd & 1) ? va * cs.y + vb * cs.x : va * cs.x - vb * cs.y;
            }
            if (part == 0) g.y[(size_t)t * g.ldy + row] = o;
            else if (part == 1) g.kc[((size_t)hh * g.n_ctx + pos) * hd + dd] = f2h(o);
            else g.vc[((size_t)hh * hd + dd) * g.n_ctx + pos] = f2h(o);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2 * NP; ++k) {
            const int t = tok0 + 16 * (k >> 2) + tq + (k & 3);
            if (t >= g.T) continue;
            float* y = g.y + (size_t)t * g.ldy + row;
            if constexpr (EPI == EPI_ADD) *y = *y + v[k];
            else if constexpr (EPI == EPI_SWIGLU_UP) *y = (X86 ? x86_silu(*y) : llmi_silu(*y)) * v[k];
            else *y = v[k];
        }
    }
}

// ---------------------------------------------------------------------------------
// k_pf_attn: grid (H, T), 256 threads.  Query token t at position pos0+t attends to
// positions 0..pos0+t of the f16 cache with or_decode's formulas: q rounded to f16;
// kq = (float) sequential double sum of exact f16 products; w = kq * scale; e =
// llmi_expf(w - max); S = double sum; p = f16(e * (float)(1/S)); out = double sum of
// exact f16 products.  Scores live in LDS (n_kv <= kPfAttnMaxKV).
// ---------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void k_pf_attn(PfAttn a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* w = (float*)smem;                       // [n_kv]
    double* red = (double*)(smem + (((size_t)a.max_kv * 4 + 16 + 7) & ~(size_t)7));  // [8], 8-B aligned
    __shared__ uint16_t qh[D];
    const int h = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int g = h / a.gqa, pos = a.pos0 + t, n_kv = pos + 1;
    if (tid < D) qh[tid] = f2h(a.q[(size_t)t * a.ldq + h * D + tid]);
    __syncthreads();
    const uint16_t* K = a.kc + (size_t)g * a.n_ctx * D;
    float mx = -INFINITY;
    for (int p = tid; p < n_kv; p += 256) {
        const uint16_t* kr = K + (size_t)p * D;
        double s = 0.0;
#pragma unroll 4
        for (int d0 = 0; d0 < D; d0 += 8) {
            const u32x4 kv = *(const u32x4*)(kr + d0);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float kf = h2f(kv[j >> 1] >> (16 * (j & 1)));
                s += (double)(kf * h2f(qh[d0 + j]));
            }
        }
        const float wv = (float)s * a.scale;
        w[p] = wv;
        mx = fmaxf(mx, wv);
    }
    // block max
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = (double)mx;
    __syncthreads();
    mx = fmaxf(fmaxf((float)red[0], (float)red[1]), fmaxf((float)red[2], (float)red[3]));
    __syncthreads();
    double sum = 0.0;
    for (int p = tid; p < n_kv; p += 256) {
        const float e = llmi_expf(w[p] - mx);
        w[p] = e;
        sum += (double)e;
    }
    sum = wave_sum_d(sum);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    sum = (red[0] + red[1]) + (red[2] + red[3]);
    const float inv = (float)(1.0 / sum);
    for (int p = tid; p < n_kv; p += 256) w[p] = h2f(f2h(w[p] * inv));
    __syncthreads();
    // PV: thread = (dim d, quarter qq of the positions); V row d is contiguous over positions
    const uint16_t* V = a.vc + (size_t)g * D * a.n_ctx;
    constexpr int PER = 256 / D;  // position splits per dim
    const int d = tid % D, part = tid / D;
    double acc = 0.0;
    if (part < PER) {
        const uint16_t* vr = V + (size_t)d * a.n_ctx;
        for (int p = part; p < n_kv; p += PER) acc += (double)(h2f(vr[p]) * w[p]);
    }
    __syncthreads();
    double* pr = (double*)smem;  // reuse the score space: [PER][D]
    if (part < PER) pr[part * D + d] = acc;
    __syncthreads();
    if (tid < D) {
        double s = pr[tid];
#pragma unroll
        for (int k = 1; k < PER; ++k) s += pr[k * D + tid];
        a.out[(size_t)t * a.ldq + h * D + tid] = (float)s;
    }
}

// k_pf_attn_g: grid (HK, T), 256 threads: the G query heads of one KV group for one
// query token, all scores in LDS (G * n_kv * 4 B).  Scores as k_attn_scores8 (8 lanes
// per position, D/8 dims each, fma in double on exact f16 products, xor 1,2,4), every K
// row read once for the G heads with coalesced 256-B rows; softmax per head (double sum);
// PV: thread = (dim, position half), V rows read as 16-B pieces for all G heads at once.
template <int D, int G>
__global__ __launch_bounds__(256) void k_pf_attn_g(PfAttn a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* w = (float*)smem;  // [G][ldw]
    const int ldw = (a.max_kv + 3) & ~3;
    __shared__ __attribute__((aligned(16))) double qs[G][D];
    __shared__ double red[4][G];
    const int g = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pos = a.pos0 + t, n_kv = pos + 1;
    for (int i = tid; i < G * D; i += 256)
        qs[i / D][i % D] = (double)h2f(f2h(a.q[(size_t)t * a.ldq + (size_t)g * G * D + i]));
    __syncthreads();
    constexpr int DQ = D / 8;
    const int qd = tid & 7;
    // G may be a divisor of the model's GQA group (sub-groups of G heads when the whole
    // group's scores do not fit in LDS): workgroup g serves heads g*G.. of KV group kvg
    const int kvg = (g * G) / a.gqa;
    const uint16_t* K = a.kc + (size_t)kvg * a.n_ctx * D;
    float mx[G];
#pragma unroll
    for (int hh = 0; hh < G; ++hh) mx[hh] = -INFINITY;
    for (int t0 = 0; t0 < n_kv; t0 += 32) {
        const int p = t0 + (tid >> 3);
        const int pc = p < n_kv ? p : n_kv - 1;
        const uint16_t* kr = K + (size_t)pc * D + qd * DQ;
        double acc[G];
#pragma unroll
        for (int hh = 0; hh < G; ++hh) acc[hh] = 0.0;
#pragma unroll
        for (int i = 0; i < DQ / 8; ++i) {
            const u32x4 kv = *(const u32x4*)(kr + 8 * i);
            const int d = qd * DQ + 8 * i;
            double k[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                k[2 * j] = (double)h2f((uint16_t)kv[j]);
                k[2 * j + 1] = (double)h2f((uint16_t)(kv[j] >> 16));
            }
#pragma unroll
            for (int hh = 0; hh < G; ++hh)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[hh] = __builtin_fma(k[j], qs[hh][d + j], acc[hh]);
        }
#pragma unroll
        for (int hh = 0; hh < G; ++hh) {
            acc[hh] += xor_partner_d<1>(acc[hh]);
            acc[hh] += xor_partner_d<2>(acc[hh]);
            acc[hh] += xor_partner_d<4>(acc[hh]);
            const float sc = (float)acc[hh] * a.scale;
            if (p < n_kv) {
                if (qd == (hh & 7)) w[hh * ldw + p] = sc;
                mx[hh] = fmaxf(mx[hh], sc);
            }
        }
    }
    // softmax per head: max, e = expf(s - max), double sum, p = f16(e * (float)(1/S))
#pragma unroll
    for (int hh = 0; hh < G; ++hh) {
        const float m = wave_max(mx[hh]);
        if (lane == 0) red[wave][hh] = (double)m;
    }
    __syncthreads();
    float gm[G];
#pragma unroll
    for (int hh = 0; hh < G; ++hh)
        gm[hh] = fmaxf(fmaxf((float)red[0][hh], (float)red[1][hh]), fmaxf((float)red[2][hh], (float)red[3][hh]));
    __syncthreads();
#pragma unroll
    for (int hh = 0; hh < G; ++hh) {
        double s = 0.0;
        for (int p = tid; p < n_kv; p += 256) {
            const float e = llmi_expf(w[hh * ldw + p] - gm[hh]);
            w[hh * ldw + p] = e;
            s += (double)e;
        }
        s = wave_sum_d(s);
        if (lane == 0) red[wave][hh] = s;
    }
    __syncthreads();
#pragma unroll
    for (int hh = 0; hh < G; ++hh) {
        const float inv = (float)(1.0 / ((red[0][hh] + red[1][hh]) + (red[2][hh] + red[3][hh])));
        for (int p = tid; p < n_kv; p += 256) w[hh * ldw + p] = h2f(f2h(w[hh * ldw + p] * inv));
    }
    __syncthreads();
    // PV
    constexpr int PER = 256 / D;  // position splits per dim (2 for D=128, 4 for D=64)
    const int d = tid % D, part = tid / D;
    const uint16_t* vr = a.vc + ((size_t)kvg * D + d) * a.n_ctx;
    double o[G];
#pragma unroll
    for (int hh = 0; hh < G; ++hh) o[hh] = 0.0;
    for (int p0 = 8 * part; p0 < n_kv; p0 += 8 * PER) {
        const u32x4 vv = *(const u32x4*)(vr + p0);  // n_ctx is a multiple of 256: in bounds
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (p0 + j < n_kv) {
                const double v = (double)h2f((uint16_t)(vv[j >> 1] >> (16 * (j & 1))));
#pragma unroll
                for (int hh = 0; hh < G; ++hh) o[hh] = __builtin_fma(v, (double)w[hh * ldw + p0 + j], o[hh]);
            }
        }
    }
    __syncthreads();
    double* pr = (double*)smem;  // [PER][G][D], reusing the score space
#pragma unroll
    for (int hh = 0; hh < G; ++hh) pr[(part * G + hh) * D + d] = o[hh];
    __syncthreads();
    for (int i = tid; i < G * D; i += 256) {
        const int hh = i / D, dd = i % D;
        double s = pr[hh * D + dd];
#pragma unroll
        for (int k = 1; k < PER; ++k) s += pr[(k * G + hh) * D + dd];
        a.out[(size_t)t * a.ldq + (size_t)(g * G + hh) * D + dd] = (float)s;
    }
}
template <int D, int G>
static size_t pf_attn_g_lds(int max_kv) {
    const size_t sc = (size_t)G * ((max_kv + 3) & ~3) * 4, pv = (size_t)(256 / D) * G * D * sizeof(double);
    return sc > pv ? sc : pv;
}

// ---------------------------------------------------------------------------------
// k_pf_fa: the tiled prefill attention on the FP64 matrix cores (v_mfma_f64_16x16x4_f64:
// 16 rows x 16 columns x 4 k per instruction, chained through its accumulator).  grid =
// query tiles x KV groups, linear id b -> group b % hk, tile b / hk (the tiles of one
// group land on one XCD and share its L2), 256 threads.  The workgroup's 64 ROWS are
// TQ = 64 / G query tokens x the G heads of its KV group (row r: token r / G, head
// g G + r % G); wave w owns rows 16 w .. 16 w + 15.  K and V pass through LDS in tiles of
// 64 positions, prefetched into registers one tile ahead, so every K / V tile is read
// once for 64 rows (k_pf_attn_g above reads it once per query token).  or_decode's
// numerics (oracle/ggml_oracle.c attn_head), term by term:
//   pass 1  kq = double sum over d = 0, 1, .. D-1 of the exact products f16(q) * K:
//           k-step s of the MFMA takes dims 4 s .. 4 s + 3 and chains the accumulator,
//           i.e. the oracle's sequential order; w = (float)kq * scale goes to a global
//           scratch row; the row max over the live positions;
//   pass 2  S = double sum of e = llmi_expf(w - max) (a lane tree: absorbed, as on every
//           attention path);
//   pass 3  p = f16(e * (float)(1 / S)) into LDS (rows private to the wave), out =
//           double sum over the positions in order of the exact products v * p (MFMA k =
//           positions 4 s .. 4 s + 3 of the tile).
// Positions past a row's own token never enter max or S and get p = 0 (an exact +-0
// term after the live ones); V past the tile's last live position is staged as 0, so no
// stale cache value meets a p.  A lane reads back only scratch it wrote itself (same
// addresses, program order): no fence between the passes.
// ---------------------------------------------------------------------------------
typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ d4 mfma64(double a, double b, d4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
constexpr int kFaRows = 64, kFaKeys = 64;
constexpr int kFaLdv = kFaKeys + 2;  // V tile row (one dim) / p tile row (one query row) in doubles: 528 B,
                                     // so 16 rows x 4 positions of a fragment hit 32 distinct bank pairs
// LDS of k_pf_fa (dynamic): pass 1 holds the K tile [64 keys][D + 2] as doubles, pass 3
// the V tile [D][kFaLdv] and the p tile [R][kFaLdv] in the same space
template <int D, int R>
constexpr size_t pf_fa_lds() {
    const size_t k = (size_t)kFaKeys * (D + 2), vp = (size_t)(D + R) * kFaLdv;
    return (k > vp ? k : vp) * sizeof(double);
}

// The f64 MFMA and the VALU do not run side by side on a SIMD (tools/mfma64_probe.hip:
// a VALU wave beside MFMA waves makes no progress until they stop), so the kernel's time
// is its MFMA cycles PLUS its VALU cycles: K and V are widened to double once, when a
// tile is staged into LDS (not once per fragment use), and p is stored as double.
// llmi_expf (include/llmi_math.h) with its final 2^n scaling as one v_ldexp_f32: the
// correctly rounded p * 2^n in every range the original's scaling covers (normal n; the
// overflowing n = 128, doubled first there; subnormal results for n < -126, scaled in
// two exact-then-rounding steps there) -- the same bits with fewer VALU operations, which
// matters here because k_pf_fa's VALU and f64 MFMA time add up
__device__ __forceinline__ float pf_expf(float x) {
    if (x != x) return x;
    if (x > 88.72283935546875f) return __builtin_inff();
    if (x < -103.97208404541015625f) return 0.0f;
    const float t = x * 1.44269502162933349609375f;
    float nf = t + 12582912.f;
    nf = nf - 12582912.f;
    const int n = (int)nf;
    float r = x - nf * 0.693359375f;
    r = r - nf * -2.12194440e-4f;
    float p = 1.98412698e-4f;
    p = p * r + 1.38888889e-3f;
    p = p * r + 8.33333333e-3f;
    p = p * r + 4.16666667e-2f;
    p = p * r + 1.66666667e-1f;
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    return __builtin_ldexpf(p, n);
}

template <int D, int G, int RB, int WV, bool PE>
__global__ __launch_bounds__(64 * RB * WV) void k_pf_fa(PfAttn a, int T, int hk, int tile0, int ldw) {
    // RB 16-row blocks per workgroup (R = 16 RB rows: TQ = R / G tokens), WV waves per
    // block: pass 1 splits the tile's 4 key blocks between them, pass 3 the D / 16 dim
    // blocks.  PE: pass 2 stores e over w and pass 3 reads it back instead of taking the
    // exp again.
    constexpr int R = 16 * RB, NT = 64 * RB * WV, TQ = R / G, LDK = D + 2, NP = D * 8 / NT;  // NP: 8-element pieces per thread of a K / V tile
    constexpr int KB = 4 / WV, DB = D / 16 / WV;
    static_assert(TQ >= 1 && NP >= 1 && (D * 8) % NT == 0, "k_pf_fa shape");
    extern __shared__ __attribute__((aligned(16))) double fa_lds[];
    double* kd = fa_lds;                   // pass 1: [64][LDK]
    double* vd = fa_lds;                   // pass 3: [D][kFaLdv]
    double* pd = fa_lds + D * kFaLdv;      // pass 3: [R][kFaLdv]
    __shared__ float mxs[WV][R];
    __shared__ double sms[WV][R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
    const int rb = wave % RB, hf = wave / RB;  // row block, key / dim part
    const int b = blockIdx.x, g = b % hk, tq0 = (tile0 + b / hk) * TQ;
    const int tlast = min(tq0 + TQ, T) - 1;
    const int n_kv_max = a.pos0 + tlast + 1, nkt = (n_kv_max + kFaKeys - 1) / kFaKeys;
    float* ws = a.wsc + (size_t)b * R * ldw;
    const uint16_t* K = a.kc + (size_t)g * a.n_ctx * D;
    const uint16_t* V = a.vc + (size_t)g * D * a.n_ctx;
    // this lane's accumulator rows 16 rb + lk + 4 i and their live lengths (padding rows
    // past T repeat the last token's)
    int nkv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) nkv[i] = a.pos0 + min(tq0 + (16 * rb + lk + 4 * i) / G, tlast) + 1;
    double qa[D / 4];  // A fragments: row 16 rb + lr, dim 4 s + lk
    {
        const int r = 16 * rb + lr, t = tq0 + r / G;
        const float* qr = a.q + (size_t)min(t, T - 1) * a.ldq + (size_t)(g * G + r % G) * D + lk;
#pragma unroll
        for (int s = 0; s < D / 4; ++s) qa[s] = t < T ? (double)h2f(f2h(qr[4 * s])) : 0.0;
    }
    // scratch entry of this lane: row 16 rb + lk + 4 i, key kt 64 + (hf KB + kb) 16 + lr
    float* wrow = ws + (size_t)(16 * rb + lk) * ldw + (hf * KB) * 16 + lr;
    auto wsp = [&](int kt, int kb, int i) -> float* { return wrow + (size_t)(4 * i) * ldw + kt * kFaKeys + kb * 16; };
    // 8 f16 -> 8 doubles at dst (16-B aligned)
    auto widen8 = [](double* dst, u32x4 v) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            *(d2*)(dst + 2 * e) = d2{(double)h2f(v[e] & 0xffffu), (double)h2f(v[e] >> 16)};
    };

    // ---- pass 1: scores and row max
    u32x4 kr[NP];
    auto k_load = [&](int kt) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int i = tid + NT * j, key = i / (D / 8), c = i % (D / 8);
            kr[j] = *(const u32x4*)(K + (size_t)(kt * kFaKeys + key) * D + c * 8);
        }
    };
    auto k_store = [&]() {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int i = tid + NT * j, key = i / (D / 8), c = i % (D / 8);
            widen8(kd + key * LDK + c * 8, kr[j]);
        }
    };
    float mx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) mx[i] = -INFINITY;
    k_load(0);
    k_store();
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) k_load(kt + 1);
        d4 acc[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) acc[kb] = d4{0.0, 0.0, 0.0, 0.0};
        const double* kp = kd + (hf * KB * 16 + lr) * LDK + lk;  // B fragment: key (hf KB + kb) 16 + lr, dim 4 s + lk
#pragma unroll
        for (int s = 0; s < D / 4; ++s) {
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) acc[kb] = mfma64(qa[s], kp[kb * 16 * LDK + 4 * s], acc[kb]);
        }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            const int key = kt * kFaKeys + (hf * KB + kb) * 16 + lr;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float wv = (float)acc[kb][i] * a.scale;
                *wsp(kt, kb, i) = wv;
                if (key < nkv[i]) mx[i] = fmaxf(mx[i], wv);
            }
        }
        __syncthreads();
        if (kt + 1 < nkt) k_store();
        __syncthreads();
    }

    // ---- pass 2: row max and sum over the 16 lanes of each row group (and the WV waves)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mx[i] = fmaxf(mx[i], xor_partner<1>(mx[i]));
        mx[i] = fmaxf(mx[i], xor_partner<2>(mx[i]));
        mx[i] = fmaxf(mx[i], xor_partner<4>(mx[i]));
        mx[i] = fmaxf(mx[i], xor_partner<8>(mx[i]));
    }
    if constexpr (WV > 1) {
        if (lr == 0)
#pragma unroll
            for (int i = 0; i < 4; ++i) mxs[hf][16 * rb + lk + 4 * i] = mx[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float m = mxs[0][16 * rb + lk + 4 * i];
#pragma unroll
            for (int h = 1; h < WV; ++h) m = fmaxf(m, mxs[h][16 * rb + lk + 4 * i]);
            mx[i] = m;
        }
    }
    double sm[4] = {0.0, 0.0, 0.0, 0.0};
    // software-pipelined over batches of B2 tiles: the next batch's score loads are
    // issued before this batch's e stores, so waiting for them never waits for the
    // stores (one in-order vmcnt counts both)
    constexpr int B2 = KB >= 4 ? 1 : 4 / KB;
    float wb[2][B2][KB * 4];
    auto p2_load = [&](int kt0, float (&w)[B2][KB * 4]) {
#pragma unroll
        for (int b = 0; b < B2; ++b)
            if (kt0 + b < nkt)
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                    for (int i = 0; i < 4; ++i) w[b][kb * 4 + i] = *wsp(kt0 + b, kb, i);
    };
    auto p2_step = [&](int kt0, const float (&w)[B2][KB * 4]) {
#pragma unroll
        for (int b = 0; b < B2; ++b) {
            const int kt = kt0 + b;
            if (kt < nkt)
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) {
                    const int key = kt * kFaKeys + (hf * KB + kb) * 16 + lr;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (key < nkv[i]) {
                            const float e = pf_expf(w[b][kb * 4 + i] - mx[i]);
                            sm[i] += (double)e;
                            if constexpr (PE) *wsp(kt, kb, i) = e;
                        }
                }
        }
    };
    p2_load(0, wb[0]);
    for (int kt0 = 0; kt0 < nkt; kt0 += 2 * B2) {
        p2_load(kt0 + B2, wb[1]);
        p2_step(kt0, wb[0]);
        p2_load(kt0 + 2 * B2, wb[0]);
        p2_step(kt0 + B2, wb[1]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sm[i] += xor_partner_d<1>(sm[i]);
        sm[i] += xor_partner_d<2>(sm[i]);
        sm[i] += xor_partner_d<4>(sm[i]);
        sm[i] += xor_partner_d<8>(sm[i]);
    }
    if constexpr (WV > 1) {
        if (lr == 0)
#pragma unroll
            for (int i = 0; i < 4; ++i) sms[hf][16 * rb + lk + 4 * i] = sm[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double t = sms[0][16 * rb + lk + 4 * i];
#pragma unroll
            for (int h = 1; h < WV; ++h) t += sms[h][16 * rb + lk + 4 * i];
            sm[i] = t;
        }
    }
    float inv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) inv[i] = (float)(1.0 / sm[i]);

    // ---- pass 3: p and PV (pass 1's last barrier freed the K tile's space)
    u32x4 vr[NP];
    float wr[KB * 4];
    auto v_load = [&](int kt) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int i = tid + NT * j, d = i / 8, c = i % 8, p0 = kt * kFaKeys + c * 8;
            u32x4 v = *(const u32x4*)(V + (size_t)d * a.n_ctx + p0);
            if (p0 + 8 > n_kv_max) {
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    const uint32_t lo = p0 + e < n_kv_max ? 0xffffu : 0u, hi = p0 + e + 1 < n_kv_max ? 0xffff0000u : 0u;
                    v[e >> 1] &= lo | hi;
                }
            }
            vr[j] = v;
        }
    };
    auto v_store = [&]() {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int i = tid + NT * j, d = i / 8, c = i % 8;
            widen8(vd + d * kFaLdv + c * 8, vr[j]);
        }
    };
    auto w_load = [&](int kt, float* w) {
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int i = 0; i < 4; ++i) w[kb * 4 + i] = *wsp(kt, kb, i);
    };
    d4 o[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) o[db] = d4{0.0, 0.0, 0.0, 0.0};
    v_load(0);
    v_store();
    w_load(0, wr);
    for (int kt = 0; kt < nkt; ++kt) {
        float wn[KB * 4];
        if (kt + 1 < nkt) {
            v_load(kt + 1);
            w_load(kt + 1, wn);
        }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            const int kk = (hf * KB + kb) * 16 + lr, key = kt * kFaKeys + kk;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e = PE ? wr[kb * 4 + i] : pf_expf(wr[kb * 4 + i] - mx[i]);
                const float p = key < nkv[i] ? h2f(f2h(e * inv[i])) : 0.f;
                pd[(16 * rb + lk + 4 * i) * kFaLdv + kk] = (double)p;
            }
        }
        __syncthreads();
        const double* pp = pd + (16 * rb + lr) * kFaLdv + lk;          // A fragment: row 16 rb + lr, position 4 s + lk
        const double* vp = vd + (hf * DB * 16 + lr) * kFaLdv + lk;     // B fragment: position 4 s + lk, dim (hf DB + db) 16 + lr
#pragma unroll
        for (int s = 0; s < kFaKeys / 4; ++s) {
            const double pa = pp[4 * s];
#pragma unroll
            for (int db = 0; db < DB; ++db) o[db] = mfma64(pa, vp[db * 16 * kFaLdv + 4 * s], o[db]);
        }
        __syncthreads();
        if (kt + 1 < nkt) {
            v_store();
#pragma unroll
            for (int e = 0; e < KB * 4; ++e) wr[e] = wn[e];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = 16 * rb + lk + 4 * i, t = tq0 + r / G;
        if (t < T) {
            float* orow = a.out + (size_t)t * a.ldq + (size_t)(g * G + r % G) * D + hf * DB * 16 + lr;
#pragma unroll
            for (int db = 0; db < DB; ++db) orow[db * 16] = (float)o[db][i];
        }
    }
}

static bool pf_fa_shape(int n_head, int n_head_kv, int head_dim) {
    if (n_head <= 0 || n_head_kv <= 0 || n_head % n_head_kv) return false;
    const int G = n_head / n_head_kv;
    return (head_dim == 128 || head_dim == 64) && (G == 1 || G == 2 || G == 4 || G == 8);
}
size_t pf_fa_scratch_bytes(int n_head, int n_head_kv, int head_dim, int T, int n_ctx) {
    if (!pf_fa_shape(n_head, n_head_kv, head_dim) || T <= 0 || n_ctx <= 0) return 0;
    const int TQ = kFaRows / (n_head / n_head_kv);
    const size_t ntile = (size_t)(T + TQ - 1) / TQ, ldw = (size_t)(n_ctx + kFaKeys - 1) / kFaKeys * kFaKeys;
    const size_t tile = (size_t)n_head_kv * kFaRows * ldw * 4;
    return std::max(tile, std::min(ntile * tile, kPfFaScratchCap));
}
template <int D, int G, int RB, int WV, bool PE>
static void pf_fa_chunks(const PfAttn& a, int n_head, int T, hipStream_t s) {
    constexpr int R = 16 * RB, TQ = R / G;
    if constexpr (D * 8 < 64 * RB * WV || TQ < 1) {  // a K / V tile has fewer 16-B pieces than threads
        pf_fa_chunks<D, G, 4, 2, false>(a, n_head, T, s);
        return;
    }
    const int hk = n_head / G, ntile = (T + TQ - 1) / TQ;
    const int ldw = (a.pos0 + T + kFaKeys - 1) / kFaKeys * kFaKeys;
    const int chunk = (int)std::min<size_t>((size_t)ntile, a.wsc_bytes / ((size_t)hk * R * ldw * 4));
    for (int t0 = 0; t0 < ntile; t0 += chunk) {
        const int nt = std::min(chunk, ntile - t0);
        if constexpr (D * 8 >= 64 * RB * WV && TQ >= 1)
            launch_k(k_pf_fa<D, G, RB, WV, PE>, dim3(nt * hk), dim3(64 * RB * WV), pf_fa_lds<D, R>(), s, true, true, a, T,
                     hk, t0, ldw);
    }
}
// g_pf_fa_cfg: decimal digits RB WV PE (default 440: 64-row workgroups, four waves per
// row block, pass 3 takes the exp again; head_dim 64 takes 420); every configuration
// gives the same bits.  Measured (tools/pfattn_bench.py, 8B heads, T = 512 at pos0
// 15872, pass 2 software-pipelined): 440 45.7 FP64 TFLOP/s, 441 42.4, 420 40.9, 421
// 40.9, 410 33.2, 241 31.8, 221 29.8 (K / V / p as doubles in LDS; 2-row-block
// workgroups fit one per CU; storing e costs more than recomputing it)
template <int D, int G>
static hipError_t pf_fa_launch(const PfAttn& a, int n_head, int T, hipStream_t s) {
    const int hk = n_head / G, ldw = (a.pos0 + T + kFaKeys - 1) / kFaKeys * kFaKeys;
    if (a.wsc_bytes < (size_t)hk * kFaRows * ldw * 4) return hipErrorNotSupported;
    switch (g_pf_fa_cfg) {
        case 410: pf_fa_chunks<D, G, 4, 1, false>(a, n_head, T, s); break;
        case 420: pf_fa_chunks<D, G, 4, 2, false>(a, n_head, T, s); break;
        case 421: pf_fa_chunks<D, G, 4, 2, true>(a, n_head, T, s); break;
        case 220: pf_fa_chunks<D, G, 2, 2, false>(a, n_head, T, s); break;
        case 221: pf_fa_chunks<D, G, 2, 2, true>(a, n_head, T, s); break;
        case 241: pf_fa_chunks<D, G, 2, 4, true>(a, n_head, T, s); break;
        case 441: pf_fa_chunks<D, G, 4, 4, true>(a, n_head, T, s); break;
        default: pf_fa_chunks<D, G, 4, 4, false>(a, n_head, T, s);
    }
    return hipGetLastError();
}
// hipErrorNotSupported: no tiled kernel for this shape (the caller takes the LDS kernels)
static hipError_t pf_fa_dispatch(const PfAttn& a, int n_head, int head_dim, int T, hipStream_t s) {
    if (!a.wsc || a.pos0 + T > a.n_ctx || a.gqa <= 0 || n_head % a.gqa ||
        !pf_fa_shape(n_head, n_head / a.gqa, head_dim))
        return hipErrorNotSupported;
    const int G = a.gqa;
    if (head_dim == 128) {
        if (G == 4) return pf_fa_launch<128, 4>(a, n_head, T, s);
        if (G == 8) return pf_fa_launch<128, 8>(a, n_head, T, s);
        if (G == 2) return pf_fa_launch<128, 2>(a, n_head, T, s);
        return pf_fa_launch<128, 1>(a, n_head, T, s);
    }
    if (G == 4) return pf_fa_launch<64, 4>(a, n_head, T, s);
    if (G == 8) return pf_fa_launch<64, 8>(a, n_head, T, s);
    if (G == 2) return pf_fa_launch<64, 2>(a, n_head, T, s);
    return pf_fa_launch<64, 1>(a, n_head, T, s);
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
size_t pf_quant_lds(int act, int cols) { return mv_lds_bytes(act, cols); }

hipError_t launch_pf_quant(const float* x, int ldx, const float* nw, float eps, int cols, int act, int T, void* aqv,
                           int16_t* abs, float* ad, void* abf, hipStream_t s, int x86) {
    uint8_t* aq = (uint8_t*)aqv;
    MVArgs A;
    A.x = x; A.nw = nw; A.eps = eps; A.cols = cols;
    const size_t lds = mv_lds_bytes(act, cols);
    // few rows (batched decode): split each row over workgroups of g_pf_quant_bpc blocks
    const int nstage = cols >> 8;
    const int bpc = (T < g_pf_quant_split_below && g_pf_quant_bpc > 0) ? std::min(g_pf_quant_bpc, nstage) : nstage;
    const dim3 grid(T, (nstage + bpc - 1) / bpc);
    if (x86) {  // the x86 q8 quantization (round-half-even q8_0, x86 record order for q8_K)
        if (act == 0) {
            if (nw) launch_k(k_pf_quant<0, true, 1>, grid, dim3(kMVThreads), lds, s, true, true, A, ldx, aq, abs, ad, (uint8_t*)abf, bpc);
            else launch_k(k_pf_quant<0, false, 1>, grid, dim3(kMVThreads), lds, s, true, true, A, ldx, aq, abs, ad, (uint8_t*)abf, bpc);
        } else {
            if (nw) launch_k(k_pf_quant<1, true, 1>, grid, dim3(kMVThreads), lds, s, true, true, A, ldx, aq, abs, ad, (uint8_t*)abf, bpc);
            else launch_k(k_pf_quant<1, false, 1>, grid, dim3(kMVThreads), lds, s, true, true, A, ldx, aq, abs, ad, (uint8_t*)abf, bpc);
        }
        return hipGetLastError();
    }
    if (act == 0) {
        if (nw) launch_k(k_pf_quant<0, true>, grid, dim3(kMVThreads), lds, s, true, true, A, ldx, aq, abs, ad, (uint8_t*)abf, bpc);
        else launch_k(k_pf_quant<0, false>, grid, dim3(kMVThreads), lds, s, true, true, A, ldx, aq, abs, ad, (uint8_t*)abf, bpc);
    } else {
        if (nw) launch_k(k_pf_quant<1, true>, grid, dim3(kMVThreads), lds, s, true, true, A, ldx, aq, abs, ad, (uint8_t*)abf, bpc);
        else launch_k(k_pf_quant<1, false>, grid, dim3(kMVThreads), lds, s, true, true, A, ldx, aq, abs, ad, (uint8_t*)abf, bpc);
    }
    return hipGetLastError();
}

hipError_t launch_pf_embed(const Seg& w, int cols, int vocab, const int32_t* toks, float* X, int T, int32_t* hist,
                           int pos0, int n_ctx, hipStream_t s) {
    launch_k(k_pf_embed, dim3((cols + 255) / 256, T), dim3(256), 0, s, true, true, w, cols, vocab, toks, X, T, hist, pos0,
             n_ctx);
    return hipGetLastError();
}

// k_pf_gemm's tile order: 0 = launch order; SY = token-group chunk of the XCD-aware order
// (g_pf_xcd_map: 1 = all groups of a row block together, k > 1 = chunks of k groups)
static int pf_xcd_sy(dim3 grid) {
    if (!g_pf_xcd_map || (grid.x * grid.y) % 8 != 0) return 0;
    const int sy = g_pf_xcd_map == 1 ? (int)grid.y : g_pf_xcd_map;
    return (int)grid.y % sy == 0 ? sy : (int)grid.y;
}
template <int T, int EPI>
static hipError_t pf_gemm_launch(const PfGemm& g0, hipStream_t s) {
#if defined(LLMI_EXPERIMENTS)
    PfGemm g = g0;
    g.exp = getenv("LLMI_PF_EXP") ? atoi(getenv("LLMI_PF_EXP")) : 0;
#else
    const PfGemm& g = g0;
#endif
    if (g.w.x86) {  // x86 numerics: 32-token workgroups (the 8-12 chains per row: register room)
        const dim3 grid((g.rows + kPfRows - 1) / kPfRows, (g.T + 31) / 32);
        PfGemm gx = g;
        gx.xcd_map = pf_xcd_sy(grid);
        launch_k(k_pf_gemm<T, EPI, 1, 1>, grid, dim3(256), 2 * PfBuf<1>::BYTES, s, true, true, gx);
        return hipGetLastError();
    }
    // 64 tokens per workgroup (NG = 2) while that still gives every CU a workgroup (at
    // fewer, 32-token workgroups: twice the grid); activation rows are padded to a
    // multiple of 64 (prefill_alloc's 512-token buffers, llmi_pf_gemm's own)
    const int wg64 = (g.rows + kPfRows - 1) / kPfRows * ((g.T + 63) / 64);
    if (g_pf_gemm_ng == 2 && g.T > 32 && wg64 >= cu_count()) {
        const dim3 grid((g.rows + kPfRows - 1) / kPfRows, (g.T + 63) / 64);
        PfGemm gx = g;
        gx.xcd_map = pf_xcd_sy(grid);
        launch_k(k_pf_gemm<T, EPI, 2>, grid, dim3(256), 2 * PfBuf<2>::BYTES, s, true, true, gx);
    } else {
        const dim3 grid((g.rows + kPfRows - 1) / kPfRows, (g.T + 31) / 32);
        PfGemm gx = g;
        gx.xcd_map = pf_xcd_sy(grid);
        launch_k(k_pf_gemm<T, EPI, 1>, grid, dim3(256), 2 * PfBuf<1>::BYTES, s, true, true, gx);
    }
    return hipGetLastError();
}
template <int T>
static hipError_t pf_gemm_epi(const PfGemm& g, int epi, hipStream_t s) {
    switch (epi) {
        case EPI_STORE: return pf_gemm_launch<T, EPI_STORE>(g, s);
        case EPI_ADD: return pf_gemm_launch<T, EPI_ADD>(g, s);
        case EPI_QKV: return pf_gemm_launch<T, EPI_QKV>(g, s);
        case EPI_SWIGLU_UP: return pf_gemm_launch<T, EPI_SWIGLU_UP>(g, s);
        default: return hipErrorInvalidValue;
    }
}
bool pf_gemm_ok(int type, int rows, int cols) {
    if (rows % 16 || rows <= 0 || cols % 256 || cols <= 0) return false;
    return type == T_Q4_K || type == T_Q5_K || type == T_Q6_K || type == T_Q8_0;
}
hipError_t launch_pf_gemm(const PfGemm& g, int epi, hipStream_t s) {
    if (!pf_gemm_ok(g.w.type, g.rows, g.cols) || g.T <= 0) return hipErrorInvalidValue;
    switch (g.w.type) {
        case T_Q4_K: return pf_gemm_epi<T_Q4_K>(g, epi, s);
        case T_Q5_K: return pf_gemm_epi<T_Q5_K>(g, epi, s);
        case T_Q6_K: return pf_gemm_epi<T_Q6_K>(g, epi, s);
        case T_Q8_0: return pf_gemm_epi<T_Q8_0>(g, epi, s);
        default: return hipErrorInvalidValue;
    }
}

// static LDS of a kernel (hipFuncGetAttributes, cached): a launch whose dynamic + static
// LDS passes the CU's 160 KiB aborts the queue (HSA_STATUS_ERROR_INVALID_ALLOCATION)
static size_t static_lds(const void* k) {
    static std::mutex mu;
    static std::map<const void*, size_t> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(k);
    if (it != cache.end()) return it->second;
    hipFuncAttributes at{};
    const size_t v = hipFuncGetAttributes(&at, k) == hipSuccess ? at.sharedSizeBytes : (size_t)16 * 1024;
    cache[k] = v;
    return v;
}
constexpr size_t kLdsPerCU = 160 * 1024;
template <int D, int G>
static bool pf_attn_g_fits(int max_kv) {
    return pf_attn_g_lds<D, G>(max_kv) + static_lds((const void*)k_pf_attn_g<D, G>) <= kLdsPerCU;
}

template <int D, int G>
static hipError_t pf_attn_g_launch(const PfAttn& a, int n_head, int T, hipStream_t s) {
    const size_t lds = pf_attn_g_lds<D, G>(a.max_kv);
    auto k = k_pf_attn_g<D, G>;  // > 64 KiB dynamic LDS needs no attribute (see launch_pf_attn)
    launch_k(k, dim3(n_head / G, T), dim3(256), lds, s, true, true, a);
    return hipGetLastError();
}

// size of k_pf_attn's dynamic LDS: the scores of one head, the reduction slots, the PV partials
static size_t pf_attn_lds(int max_kv) {
    const size_t lds = (((size_t)max_kv * 4 + 16 + 7) & ~(size_t)7) + 8 * sizeof(double), pv = (size_t)256 * sizeof(double);
    return lds < pv ? pv : lds;
}

// What launch_pf_attn launches for an LDS path (1: grouped, then one head per workgroup; 2:
// one head per workgroup) at max_kv score positions: 8, 4 or 2 = k_pf_attn_g<D, that many
// heads> (the whole GQA group, or a sub-group of it), 1 = k_pf_attn, -1 = refused
int pf_attn_path(int n_head, int n_head_kv, int head_dim, int max_kv, int path) {
    if ((head_dim != 128 && head_dim != 64) || n_head <= 0 || n_head_kv <= 0 || n_head % n_head_kv || max_kv <= 0) return -1;
    const int gqa = n_head / n_head_kv;
    auto fits = [&](int G) {
        if (head_dim == 128) return G == 8 ? pf_attn_g_fits<128, 8>(max_kv) : G == 4 ? pf_attn_g_fits<128, 4>(max_kv) : pf_attn_g_fits<128, 2>(max_kv);
        return G == 8 ? pf_attn_g_fits<64, 8>(max_kv) : G == 4 ? pf_attn_g_fits<64, 4>(max_kv) : pf_attn_g_fits<64, 2>(max_kv);
    };
    // grouped kernel while the G heads' scores fit in LDS (8B, G = 4: 10 Ki positions)
    if (path != 2) {
        if ((gqa == 8 || gqa == 4 || gqa == 2) && fits(gqa)) return gqa;
        // the whole group's scores do not fit: sub-groups of 4 or 2 heads (K and V read
        // gqa / 4 or gqa / 2 times instead of gqa times by the one-head kernel below)
        if (gqa == 8 && fits(4)) return 4;
        if (gqa % 2 == 0 && gqa > 2 && fits(2)) return 2;
    }
    if (max_kv > kPfAttnMaxKV) return -1;
    auto k = head_dim == 128 ? k_pf_attn<128> : k_pf_attn<64>;
    if (pf_attn_lds(max_kv) + static_lds((const void*)k) > kLdsPerCU) return -1;
    return 1;
}

hipError_t launch_pf_attn(const PfAttn& a, int n_head, int head_dim, int T, hipStream_t s, int path) {
    if (head_dim != 128 && head_dim != 64) return hipErrorInvalidValue;
    if (a.fa) return launch_pf_attn_fa(a, n_head, head_dim, T, s);
    if (a.num) return launch_pf_attn_x86(a, n_head, n_head / a.gqa, head_dim, T, s);
    if (path < 0) path = g_pf_attn_simple ? 2 : g_pf_attn_fa ? -1 : 1;
    if (path == 0) return pf_fa_dispatch(a, n_head, head_dim, T, s);
    // the tiled FP64-MFMA kernel wherever the head shape and the scratch allow
    if (path < 0) {
        const hipError_t e = pf_fa_dispatch(a, n_head, head_dim, T, s);
        if (e != hipErrorNotSupported) return e;
    }
    if (a.gqa <= 0 || n_head % a.gqa || a.pos0 + T > a.max_kv) return hipErrorInvalidValue;
    // gfx950 launches take up to 160 KiB of dynamic LDS as is (the split decode attention
    // uses 128 KiB); hipFuncSetAttribute(MaxDynamicSharedMemorySize) is refused here with
    // "invalid argument", which failed every 8B prompt reaching past 4 Ki positions
    const bool d128 = head_dim == 128;
    switch (pf_attn_path(n_head, n_head / a.gqa, head_dim, a.max_kv, path == 2 ? 2 : 1)) {
        case 8: return d128 ? pf_attn_g_launch<128, 8>(a, n_head, T, s) : pf_attn_g_launch<64, 8>(a, n_head, T, s);
        case 4: return d128 ? pf_attn_g_launch<128, 4>(a, n_head, T, s) : pf_attn_g_launch<64, 4>(a, n_head, T, s);
        case 2: return d128 ? pf_attn_g_launch<128, 2>(a, n_head, T, s) : pf_attn_g_launch<64, 2>(a, n_head, T, s);
        case 1: break;
        default: return hipErrorInvalidValue;
    }
    auto k = d128 ? k_pf_attn<128> : k_pf_attn<64>;
    launch_k(k, dim3(n_head, T), dim3(256), pf_attn_lds(a.max_kv), s, true, true, a);
    return hipGetLastError();
}

}  // namespace llmi
