// kernels.hip — gfx950 (CDNA4, wave64) kernels of the GGUF K-quant decode step.
//
// The hot path of SURVEY.md §8(a): per token, every linear layer is a quantized
// matrix-vector product that streams the whole weight matrix from HBM once (rows
// a6-a9, ~100% of the bytes), wrapped by the small fused ops a5 (activation
// quantization), a10-a15.  Design:
//
//   k_matvec  one launch per fused weight group (QKV, O, gate+up, down, output head).
//     prologue  every workgroup re-derives the quantized activation in LDS from the
//               f32 input (L2/MALL-resident, 16-57 KB): optional RMSNorm (double sum, as
//               ggml_compute_forward_rms_norm) then quantize_row_q8_K_ref /
//               quantize_row_q8_0_ref, bit-exactly.  This replaces a separate
//               norm+quantize launch (a 1.2-1.9 us dependent-kernel boundary on MI355X).
//     body      a wave owns a PAIR of rows; lane L owns pieces L, L+64, ... of both rows
//               (a piece = 32 weights, common.h): 16-B loads that cover 1 KiB of
//               consecutive bytes per wave instruction, integer v_dot4c_i32_i8 against
//               the LDS activation (stored in the same piece order: conflict-free
//               ds_read_b128), exact int32 per-piece sums combined in fp32 as
//               ggml_vec_dot_*_q8_K does (d_w*d_a*isum - dmin_w*d_a*imin), then a
//               64-lane butterfly.  The next piece's weights are in flight while the
//               current one is reduced, and a wave's first piece is issued before the
//               prologue so HBM latency overlaps it.
//     epilogue  store / residual add / RoPE + f16 KV write / SwiGLU / logits + argmax.
//   (decode attention: attn.hip, attn86.hip, attnfa.hip)
//   k_embed    token selection (host token or previous argmax) + get_rows dequant.
//   k_repack_* one-time load-time layout transforms (common.h).
#include "kernels.h"
#include "mv_device.h"
#include "launch_util.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <hip/hip_runtime.h>

namespace llmi {

// Launch-event hook (llmi_profile_kernels): while armed, the timed launches record
// `start` when the first kernel of the op begins and `stop` when the last one ends
// (hipExtLaunchKernelGGL), i.e. kernel execution time without dependent-launch gaps.
static thread_local hipEvent_t t_ev_start = nullptr, t_ev_stop = nullptr;
void set_launch_events(hipEvent_t start, hipEvent_t stop) {
    t_ev_start = start;
    t_ev_stop = stop;
}
hipEvent_t launch_event(bool stop) { return stop ? t_ev_stop : t_ev_start; }

// LDS of a matvec workgroup: the activation image, the prologue's reduction slots, then
// one fold buffer (mv_device.h kFoldFloats) per wave
size_t mv_lds_bytes(int act, int cols) { return fold_off(act, cols, kMVWaves) + (size_t)kMVWaves * kFoldFloats * 4; }

// The prologue's quantized activation written out in ggml block form (test hook).
template <int ACT, int X86>
__global__ __launch_bounds__(kMVThreads) void k_quant_dump(MVArgs A, uint8_t* out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const Lds L = carve(smem, ACT, A.cols);
    if (A.nw) mv_prologue<ACT, true, X86>(A, L);
    else mv_prologue<ACT, false, X86>(A, L);
    __syncthreads();
    const int cols = A.cols;
    for (int e = threadIdx.x; e < cols; e += blockDim.x) {
        const uint8_t* rec = L.act + (size_t)(e >> 8) * kRec;
        const int t = e & 255;
        if (ACT == 0) {  // residue order: element 64c + 32h + l + 8i at part 2c + l/4, half h, byte 4 (l % 4) + i
                         // (x86: element 64c + 32h + 4l + i)
            const int c = t >> 6, h = (t >> 5) & 1, l = X86 ? (t & 31) >> 2 : t & 7, i = X86 ? t & 3 : (t & 31) >> 3;
            out[(size_t)(e >> 8) * 292 + 4 + t] = rec[32 * (2 * c + (l >> 2)) + 16 * h + 4 * (l & 3) + i];
        } else {
            out[(size_t)(e >> 5) * 34 + 2 + (e & 31)] = rec[t];
        }
    }
    if (ACT == 0) {
        for (int b = threadIdx.x; b < cols / 256; b += blockDim.x)
            *(float*)(out + (size_t)b * 292) = *(const float*)(L.act + (size_t)b * kRec + kRecD);
        for (int sb = threadIdx.x; sb < cols / 16; sb += blockDim.x)
            *(int16_t*)(out + (size_t)(sb >> 4) * 292 + 260 + 2 * (sb & 15)) =
                *(const int16_t*)(L.act + (size_t)(sb >> 4) * kRec + kRecBs + 2 * (sb & 15));
    } else {
        for (int b = threadIdx.x; b < cols / 32; b += blockDim.x)
            *(uint16_t*)(out + (size_t)b * 34) = f2h(*(const float*)(L.act + (size_t)(b >> 3) * kRec + kRecBs + 4 * (b & 7)));
    }
}

// ----------------------------------------------------------------------------------
// Step entry: choose the token, advance pos, dequantize its embedding row
// (upstream ggml_get_rows + dequantize_row_*; bit-exact).
// Reads the piece-planar device layout (common.h).
// ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_embed(EmbArgs a) {
    StepState* st = a.st;
    const int pos = st->pos_next;
    __shared__ int s_tok;
    if (threadIdx.x < 64) {  // wave 0: max over the previous step's argmax slots
        static_assert(kArgSlots == 64, "one slot per lane");
        const unsigned long long k = wave_max_u64(st->key[(pos + 1) & 1][threadIdx.x]);
        if (threadIdx.x == 0) {
            int tok = st->token_in_pos == pos ? st->token_in : (int)(0xffffffffu - (uint32_t)(k & 0xffffffffull));
            if (tok < 0 || tok >= a.vocab) tok = 0;
            s_tok = tok;
        }
    }
    __syncthreads();
    const int tok = s_tok;
    if (blockIdx.x == 0) {
        if (threadIdx.x < kArgSlots) st->key[pos & 1][threadIdx.x] = 0;
        if (threadIdx.x == 0) {
            st->pos = pos;
            st->token = tok;
            st->seq = st->seq + 1u;  // tags of this step's in-launch hand-offs (k_attn_x)
            if (pos >= 0 && pos < a.n_ctx) a.hist[pos] = tok;
        }
    }
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < a.cols) a.x[e] = dequant_elem(a.w, tok, e, a.cols);
}

// get_rows of the last step's token (st->token, set by k_embed) with k_embed's dequant:
// the per-op check of SURVEY.md §8a row a10 (llmi_debug_tap 0)
__global__ __launch_bounds__(256) void k_embed_row(Seg w, int cols, int vocab, const StepState* st, float* out) {
    int tok = st->token;
    if (tok < 0 || tok >= vocab) tok = 0;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < cols) out[e] = dequant_elem(w, tok, e, cols);
}
hipError_t launch_embed_row(const EmbArgs& a, const StepState* st, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_embed_row, dim3((a.cols + 255) / 256), dim3(256), 0, s, a.w, a.cols, a.vocab, st, out);
    return hipGetLastError();
}

__global__ void k_state_tick(StepState* st) { st->seq = st->seq + 1u; }

hipError_t launch_state_tick(StepState* st, hipStream_t s) {
    hipLaunchKernelGGL(k_state_tick, dim3(1), dim3(1), 0, s, st);
    return hipGetLastError();
}

__global__ void k_state_set(StepState* st, int token_in, int pos_next) {
    st->token_in = token_in;
    st->token_in_pos = pos_next;
    st->pos_next = pos_next;
}

// ----------------------------------------------------------------------------------
// Load-time repack of GGUF blocks into the unit-major layout (common.h).
// One thread per (block, chunk c in 0..3); nbr = blocks (units) per row.
// ----------------------------------------------------------------------------------
// x86 = 1: the x86-numerics byte order (common.h): part 2c + k = native bytes, i.e. byte
// 4m + i of part 2c + k holds chunk elements t = 16k + 4m + i (low nibble) and 32 + t
__global__ void k_repack_kq(int type, const uint8_t* raw, uint8_t* A, uint8_t* H, uint8_t* S, uint8_t* Dp, int64_t nblk,
                            int nbr, int rgs, int x86) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t b = gid >> 2;
    const int c = (int)(gid & 3);
    if (b >= nblk) return;
    const int64_t row = b / nbr, u = b % nbr, U = nbr;
    // piece (row, part p, unit u) at A + piece_off(row, p, u, U, 8, rgs) (common.h ROW GROUPS)
    auto apiece = [&](int p) { return A + piece_off((uint32_t)row, (uint32_t)p, (uint32_t)u, (uint32_t)U, 8, rgs); };
    // residue order: byte 4m + i of part 2c + k holds chunk elements t = l + 8i (low
    // nibble) and 32 + t (high nibble), l = 4k + m
    if (type == T_Q4_K || type == T_Q5_K) {
        const int bb = type == T_Q4_K ? 144 : 176;
        const uint8_t* x = raw + b * bb;
        const uint8_t* qs = x + (type == T_Q4_K ? 16 : 48);
        // chunk element of (l = 4k + m, byte i): residue order l + 8i, x86 order 4l + i
        auto el = [&](int l, int i) { return x86 ? 4 * l + i : l + 8 * i; };
        for (int k = 0; k < 2; ++k)
            for (int m = 0; m < 4; ++m)
                for (int i = 0; i < 4; ++i) apiece(2 * c + k)[4 * m + i] = qs[32 * c + el(4 * k + m, i)];
        if (c == 0)
            for (int i = 0; i < 16; ++i) S[b * 16 + i] = x[i];
        if (type == T_Q5_K) {  // byte i, bit l of the lo word: qh[el(l, i)] bit 2c; hi word: bit 2c+1
            const uint8_t* qh = x + 16;
            uint8_t* h = H + piece_off((uint32_t)row, (uint32_t)(c >> 1), (uint32_t)u, (uint32_t)U, 2, rgs) + 8 * (c & 1);
            for (int i = 0; i < 4; ++i) {
                uint8_t lo = 0, hi = 0;
                for (int l = 0; l < 8; ++l) {
                    lo |= (uint8_t)(((qh[el(l, i)] >> (2 * c)) & 1) << l);
                    hi |= (uint8_t)(((qh[el(l, i)] >> (2 * c + 1)) & 1) << l);
                }
                h[i] = lo;
                h[4 + i] = hi;
            }
        }
    } else {  // Q6_K
        const uint8_t* x = raw + b * 210;
        const uint8_t* ql = x;
        const uint8_t* qh = x + 128;
        auto u6 = [&](int w) -> int {  // 6-bit unsigned value of weight w of the block
            const int n = w >> 7, rr = w & 127, quad = rr >> 5, l = rr & 31;
            const uint8_t qlb = ql[64 * n + l + 32 * (quad & 1)];
            const int lo = (quad >> 1) ? (qlb >> 4) : (qlb & 0xF);
            const int hi = (qh[32 * n + l] >> (2 * quad)) & 3;
            return lo | (hi << 4);
        };
        auto el = [&](int l, int i) { return x86 ? 4 * l + i : l + 8 * i; };
        for (int k = 0; k < 2; ++k)
            for (int m = 0; m < 4; ++m)
                for (int i = 0; i < 4; ++i) {
                    const int t = el(4 * k + m, i);
                    apiece(2 * c + k)[4 * m + i] =
                        (uint8_t)((u6(64 * c + t) & 15) | ((u6(64 * c + 32 + t) & 15) << 4));
                }
        // H part c, dword g = 2*hi + k: byte i bits [2m, 2m+1] = (high 2 bits of chunk
        // element 32*hi + el(4k + m, i)) XOR 2, which v_perm turns into the high part of q - 32
        uint8_t* h = H + piece_off((uint32_t)row, (uint32_t)c, (uint32_t)u, (uint32_t)U, 4, rgs);
        for (int g = 0; g < 4; ++g)
            for (int i = 0; i < 4; ++i) {
                uint8_t v = 0;
                for (int m = 0; m < 4; ++m)
                    v |= (uint8_t)(((u6(64 * c + 32 * (g >> 1) + el(4 * (g & 1) + m, i)) >> 4) ^ 2) << (2 * m));
                h[4 * g + i] = v;
            }
        for (int i = 0; i < 4; ++i) S[b * 16 + 4 * c + i] = x[192 + 4 * c + i];
        if (c == 0) { Dp[b * 2] = x[208]; Dp[b * 2 + 1] = x[209]; }
    }
}

// Q8_0: one thread per 32-block; unit u = 8 blocks, block b of the unit in parts 2b, 2b+1
__global__ void k_repack_q80(const uint8_t* raw, uint8_t* A, uint8_t* Dp, int64_t nblk, int nb_row, int rgs) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nblk) return;
    const int64_t row = g / nb_row, bi = g % nb_row, U = nb_row / 8, u = bi >> 3, b = bi & 7;
    const uint8_t* x = raw + g * 34;
    for (int h = 0; h < 2; ++h)
        for (int i = 0; i < 16; ++i)
            A[piece_off((uint32_t)row, (uint32_t)(2 * b + h), (uint32_t)u, (uint32_t)U, 16, rgs) + i] = x[2 + 16 * h + i];
    Dp[(row * U + u) * 16 + 2 * b] = x[0];
    Dp[(row * U + u) * 16 + 2 * b + 1] = x[1];
}

// Streaming-read reference (achievable HBM rate for a perfectly coalesced 16-B/lane
// read of the same bytes): each thread sums dwords of grid-strided 16-B pieces.
__global__ __launch_bounds__(256) void k_stream_read(const u32x4* p, size_t n16, unsigned* out) {
    unsigned acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
        const u32x4 v = ldw((const uint8_t*)(p + i));
        acc += v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x12345678u) out[0] = acc;  // keep the loads alive
}

hipError_t launch_stream_read(const void* p, size_t bytes, unsigned* out, int blocks, hipStream_t s) {
    hipLaunchKernelGGL(k_stream_read, dim3(blocks), dim3(256), 0, s, (const u32x4*)p, bytes / 16, out);
    return hipGetLastError();
}

// Arena hash (replica check): H = sum over 8-byte words i (mod 2^64) of
// mix64(word_i ^ (i * phi)), mix64 = splitmix64's finalizer; the last partial word is
// zero-padded.  A sum of per-position terms is independent of the order the grid visits
// the words in, so every replica of the same bytes gets the same value on any device
// (tests/test_fanout_check.py restates it in numpy).
__device__ __forceinline__ unsigned long long hash_mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__global__ __launch_bounds__(256) void k_arena_hash(const uint8_t* p, size_t bytes, unsigned long long* out) {
    const size_t nw = bytes >> 3, n16 = bytes >> 4;
    unsigned long long acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
        const u32x4 v = ldw(p + i * 16);
        const unsigned long long w0 = ((unsigned long long)v.y << 32) | v.x, w1 = ((unsigned long long)v.w << 32) | v.z;
        acc += hash_mix64(w0 ^ ((2 * i) * 0x9E3779B97F4A7C15ull));
        acc += hash_mix64(w1 ^ ((2 * i + 1) * 0x9E3779B97F4A7C15ull));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the word past the last 16-B piece, and the tail
        for (size_t i = 2 * n16; i * 8 < bytes; ++i) {
            unsigned long long w = 0;
            for (size_t b = 0; b < 8 && i * 8 + b < bytes; ++b) w |= (unsigned long long)p[i * 8 + b] << (8 * b);
            acc += hash_mix64(w ^ (i * 0x9E3779B97F4A7C15ull));
        }
    }
    (void)nw;
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}

hipError_t launch_arena_hash(const void* p, size_t bytes, unsigned long long* out, hipStream_t s) {
    hipError_t e = hipMemsetAsync(out, 0, 8, s);
    if (e != hipSuccess) return e;
    const size_t n16 = bytes >> 4;
    const int blocks = (int)std::max<size_t>(1, std::min<size_t>(4096, (n16 + 255) / 256));
    hipLaunchKernelGGL(k_arena_hash, dim3(blocks), dim3(256), 0, s, (const uint8_t*)p, bytes, out);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------
// launchers
// ----------------------------------------------------------------------------------
// QKV whose segments form two contiguous type groups split at a task boundary: both groups
// pipelined (k_matvec's T2 path).  Returns hipErrorNotSupported when not applicable.
template <bool NORM, int X86>
static hipError_t mv_dispatch_qkv2(const MVArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    if (a.nseg < 2 || grid.x < 2) return hipErrorNotSupported;
    int t1 = a.seg[0].type, t2 = -1, split_row = -1;
    for (int i = 1; i < a.nseg; ++i) {
        if (a.seg[i].type == (t2 < 0 ? t1 : t2)) continue;
        if (t2 >= 0) return hipErrorNotSupported;  // a third group
        t2 = a.seg[i].type;
        split_row = a.seg[i].row0 - a.seg[0].row0;
    }
    if (t2 < 0 || split_row % a.rpt || a.cols > 16 * kMVThreads) return hipErrorNotSupported;
    const int sp = split_row / a.rpt;
#define LLMI_QKV2(A_, B_)                                                                            \
    if (t1 == A_ && t2 == B_) return mv_qkv2_launch<NORM, A_, B_, X86>(a, sp, grid, lds, s);
    if constexpr (NORM) {
        LLMI_QKV2(T_Q4_K, T_Q6_K) LLMI_QKV2(T_Q4_K, T_Q5_K) LLMI_QKV2(T_Q5_K, T_Q6_K)
    }
#undef LLMI_QKV2
    return hipErrorNotSupported;
}

template <bool NORM, int X86>
static hipError_t mv_dispatch_type(const MVArgs& a, int epi, dim3 grid, size_t lds, hipStream_t s) {
    static const bool qkv2 = !getenv("LLMI_NO_QKV2");  // A/B switch for measurements
    if (epi == EPI_QKV && qkv2) {
        const hipError_t e = mv_dispatch_qkv2<NORM, X86>(a, grid, lds, s);
        if (e != hipErrorNotSupported) return e;
    }
    // primary (pipelined) type = the type owning the most rows of the launch
    int best = a.seg[0].type, best_rows = 0;
    for (int i = 0; i < a.nseg; ++i) {
        int rows = 0;
        for (int k = 0; k < a.nseg; ++k)
            if (a.seg[k].type == a.seg[i].type) rows += a.seg[k].rows;
        if (rows > best_rows) { best_rows = rows; best = a.seg[i].type; }
    }
    switch (best) {
        case T_Q4_K: return mv_dispatch_epi<0, NORM, T_Q4_K, X86>(a, epi, grid, lds, s);
        case T_Q5_K: return mv_dispatch_epi<0, NORM, T_Q5_K, X86>(a, epi, grid, lds, s);
        case T_Q6_K: return mv_dispatch_epi<0, NORM, T_Q6_K, X86>(a, epi, grid, lds, s);
        case T_Q8_0: return mv_dispatch_epi<1, NORM, T_Q8_0, X86>(a, epi, grid, lds, s);
        default: return hipErrorInvalidValue;
    }
}

// Row-task geometry (mv_device.h "Row tasks"): Lr lanes per row = U rounded up to a
// multiple of 4, at most 64 (QKV: 32, so that a task holds RoPE pairs); R = 64 / Lr
// rounded down to a power of two, halved until every segment starts on a task boundary.
// With us = 2 lanes per unit (mv_device.h "Split units") the same holds for the units: at
// most 32 (QKV: 16) units per sub-item, Lr = twice that, R = 64 / Lr: a 4096-column row is
// 32 lanes, two rows per task, twice the tasks.
static void mv_geo_lanes(const MVArgs& a, int epi, int us, int& lr, int& R) {
    const int U = a.cols >> 8, lmax = (epi == EPI_QKV ? 32 : 64) / us;
    static const int lr_cap = [] {  // A/B knob: cap on units per row (more rows per task)
        const char* e = getenv("LLMI_MV_LR");
        return e ? atoi(e) : 64;
    }();
    int lu = (std::min(std::min(U, lmax), lr_cap) + 3) & ~3;
    lu = std::min(std::max(lu, 4), lmax);
    lr = lu * us;
    R = 1;
    while (2 * R * lr <= 64) R *= 2;
    auto aligned = [&](int r) {
        for (int i = 1; i < a.nseg; ++i)
            if ((a.seg[i].row0 - a.seg[0].row0) % r) return false;
        return true;
    };
    if (epi != EPI_SWIGLU)
        while (R > 1 && !aligned(R)) R >>= 1;
}
bool mv_geometry(MVArgs& a, int epi) {
    if (a.nseg < 1 || a.cols < 256 || a.cols % 256 || (a.us != 1 && a.us != 2)) return false;
    int lr, R;
    mv_geo_lanes(a, epi, a.us, lr, R);
    if (epi == EPI_QKV && R < 2) return false;
    if (a.us2) {  // the second type group's own geometry
        if (a.us2 != 1 && a.us2 != 2) return false;
        mv_geo_lanes(a, epi, a.us2, a.lr2, a.rpt2);
        if (epi == EPI_QKV && a.rpt2 < 2) return false;
    }
    int rows;
    if (epi == EPI_SWIGLU) {
        if (a.nseg != 2 || a.seg[0].rows != a.seg[1].rows) return false;
        rows = a.seg[0].rows;
    } else {
        rows = a.seg[a.nseg - 1].row0 + a.seg[a.nseg - 1].rows - a.seg[0].row0;
    }
    a.lr = lr;
    a.rpt = R;
    a.ntasks = (rows + R - 1) / R;
    return a.ntasks > 0;
}

// LLMI_MV_FW (A/B): 1 = each wave issues its second sub-item's weights only after its
// first sub-item's have landed, so the launch's first chip-wide round of requests is one
// sub-item per wave instead of two (every result is unchanged)
static int mv_fw() {
    static const int v = [] {
        const char* e = getenv("LLMI_MV_FW");
        return e ? atoi(e) : 0;
    }();
    return v;
}

// Split units (mv_device.h "Split units"): which launches run with two lanes per unit.
// LLMI_MV_SPLIT = auto (default) | 0 | 1 | 2 | 3, or the test option mv_unit_split (-1 auto):
//   1  every launch that can: K-quant STORE / ADD / QKV launches of Q4_K or Q6_K alone, and
//      both groups of a Q4_K + Q6_K QKV launch
//   2  only the Q6_K group of a Q4_K + Q6_K QKV launch (the slower group: 2.4 x the
//      instructions of a Q4_K wave, dispatched last)
//   3  2, and the single-type launches that are single-round today (unsplit tasks <= the
//      waves the grid holds: attn_output, an all-Q4_K QKV; not ffn_down)
//   auto = 3: every class's own kernel time came down (profiles/mv_split).
// LLMI_MV_SPLIT_NT = 256 (default) | 512 (test option mv_split_nt): the workgroup of a split
// launch; two 4-wave workgroups per CU measured faster than one of 8 waves on the all-Q4_K QKV
// (8.24 vs 9.17 us) and the same on the other two classes.
// Like every launch knob neither changes a result.
int g_mv_unit_split = -1;
int g_mv_split_nt = 0;
static int mv_split_mode() {
    static const int env = [] {
        const char* e = getenv("LLMI_MV_SPLIT");
        return e && strcmp(e, "auto") ? atoi(e) : -1;
    }();
    const int m = g_mv_unit_split >= 0 ? g_mv_unit_split : env;
    return m < 0 || m > 3 ? 3 : m;
}
static int mv_split_nt() {
    static const int env = [] {
        const char* e = getenv("LLMI_MV_SPLIT_NT");
        return e ? atoi(e) : 0;
    }();
    const int v = g_mv_split_nt ? g_mv_split_nt : env;
    return v == 256 || v == 512 ? v : 256;
}
// Sets a.us / a.us2 for the launch; returns 0 (no split), 1 (single type), 2 (two groups)
static int mv_split_plan(MVArgs& a, int epi, int max_blocks) {
    static const bool qkv2 = !getenv("LLMI_NO_QKV2");
    const int mode = mv_split_mode();
    if (mode == 0 || !(epi == EPI_STORE || epi == EPI_ADD || epi == EPI_QKV)) return 0;
    if (epi == EPI_QKV && !a.nw) return 0;
    int t1 = a.seg[0].type, t2 = -1;
    for (int i = 1; i < a.nseg; ++i) {
        if (a.seg[i].type == (t2 < 0 ? t1 : t2)) continue;
        if (t2 >= 0) return 0;  // a third group
        t2 = a.seg[i].type;
    }
    const int waves = max_blocks * kMVWaves;  // what the grid of 4-wave workgroups holds
    MVArgs g = a;
    if (t2 < 0) {
        if ((t1 != T_Q4_K && t1 != T_Q6_K) || mode == 2) return 0;
        if (!mv_geometry(g, epi)) return 0;
        if (mode == 3 && g.ntasks > waves) return 0;  // (unsplit: not single-round today)
        g.us = 2;
        if (!mv_geometry(g, epi)) return 0;
        a.us = 2;
        return 1;
    }
    if (epi != EPI_QKV || !qkv2 || t1 != T_Q4_K || t2 != T_Q6_K || a.cols > 16 * kMVThreads) return 0;
    a.us = mode == 1 ? 2 : 1;
    a.us2 = 2;
    return 2;
}

hipError_t launch_matvec(const MVArgs& a0, int epi, int max_blocks, hipStream_t s) {
    if (a0.nseg < 1 || a0.cols <= 0 || a0.cols % 256) return hipErrorInvalidValue;
    MVArgs a = a0;
    a.fw = mv_fw();
    a.us = 1;
    a.us2 = 0;
    const int split = act_kind(a.seg[0].type) == 0 ? mv_split_plan(a, epi, max_blocks) : 0;
    if (!mv_geometry(a, epi)) return hipErrorInvalidValue;
    if (split) {
        for (int i = 0; i < a.nseg; ++i)
            if (act_kind(a.seg[i].type) != 0 || (a.seg[i].x86 != 0) != (a.num != 0)) return hipErrorInvalidValue;
        const int nt = mv_split_nt();
        if (split == 1) {
            const int t = a.seg[0].type;
#define LLMI_SPLIT1(N_, T_, X_) return mv_split_launch<N_, T_, X_>(a, epi, nt, s)
            if (a.nw) {
                if (t == T_Q4_K) { if (a.num) LLMI_SPLIT1(true, T_Q4_K, 1); else LLMI_SPLIT1(true, T_Q4_K, 0); }
                else { if (a.num) LLMI_SPLIT1(true, T_Q6_K, 1); else LLMI_SPLIT1(true, T_Q6_K, 0); }
            } else {
                if (t == T_Q4_K) { if (a.num) LLMI_SPLIT1(false, T_Q4_K, 1); else LLMI_SPLIT1(false, T_Q4_K, 0); }
                else { if (a.num) LLMI_SPLIT1(false, T_Q6_K, 1); else LLMI_SPLIT1(false, T_Q6_K, 0); }
            }
#undef LLMI_SPLIT1
        }
        // two groups: the Q6_K rows start at the first Q6_K segment (a task boundary of both geometries)
        int split_row = 0;
        for (int i = a.nseg - 1; i >= 1; --i)
            if (a.seg[i].type == T_Q6_K) split_row = a.seg[i].row0 - a.seg[0].row0;
        const int rows = a.seg[a.nseg - 1].row0 + a.seg[a.nseg - 1].rows - a.seg[0].row0;
        if (split_row <= 0 || split_row % a.rpt || split_row % a.rpt2) return hipErrorInvalidValue;
        a.split_tasks = split_row / a.rpt;
        a.t2beg = split_row / a.rpt2;
        a.t2end = (rows + a.rpt2 - 1) / a.rpt2;
        if (a.us == 2) return a.num ? mv_split_qkv2_launch<1, 2>(a, nt, s) : mv_split_qkv2_launch<0, 2>(a, nt, s);
        return a.num ? mv_split_qkv2_launch<1, 1>(a, nt, s) : mv_split_qkv2_launch<0, 1>(a, nt, s);
    }
    const int act = act_kind(a.seg[0].type);
    for (int i = 1; i < a.nseg; ++i)
        if (act_kind(a.seg[i].type) != act) return hipErrorInvalidValue;
    const size_t lds = mv_lds_bytes(act, a.cols);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    int blocks = (a.ntasks + kMVWaves - 1) / kMVWaves;
    if (blocks > max_blocks) blocks = max_blocks;
#if defined(LLMI_EXPERIMENTS)
    static const int exp_blocks = [] {  // experiment builds: fixed grid for launch sweeps
        const char* e = getenv("LLMI_MV_BLOCKS");
        return e ? atoi(e) : 0;
    }();
    if (exp_blocks > 0 && exp_blocks < blocks) blocks = exp_blocks;
#endif
    const dim3 grid(blocks);
    // the weights' byte order must be the numerics' (common.h: x86 planes for x86 numerics)
    for (int i = 0; i < a.nseg; ++i)
        if ((a.seg[i].x86 != 0) != (a.num != 0)) return hipErrorInvalidValue;
    if (a.num) return a.nw ? mv_dispatch_type<true, 1>(a, epi, grid, lds, s) : mv_dispatch_type<false, 1>(a, epi, grid, lds, s);
    return a.nw ? mv_dispatch_type<true, 0>(a, epi, grid, lds, s) : mv_dispatch_type<false, 0>(a, epi, grid, lds, s);
}

hipError_t launch_quant_dump(const MVArgs& a, int act, void* out, hipStream_t s) {
    if (a.cols <= 0 || a.cols % 256) return hipErrorInvalidValue;
    const size_t lds = mv_lds_bytes(act, a.cols);
    if (a.num) {
        if (act == 0) hipLaunchKernelGGL((k_quant_dump<0, 1>), dim3(1), dim3(kMVThreads), lds, s, a, (uint8_t*)out);
        else hipLaunchKernelGGL((k_quant_dump<1, 1>), dim3(1), dim3(kMVThreads), lds, s, a, (uint8_t*)out);
    } else {
        if (act == 0) hipLaunchKernelGGL((k_quant_dump<0, 0>), dim3(1), dim3(kMVThreads), lds, s, a, (uint8_t*)out);
        else hipLaunchKernelGGL((k_quant_dump<1, 0>), dim3(1), dim3(kMVThreads), lds, s, a, (uint8_t*)out);
    }
    return hipGetLastError();
}

// Test options (llmi_test_option; never read from the environment): paths that give
// bit-identical results, or limits lowered so a test reaches a fallback / fault path.
int g_pf_attn_simple = 0;               // batched-prefill attention: one head per workgroup
int g_pf_fa_noalloc = 0;               // prefill: never allocate k_pf_fa's score scratch (its failure path)
#ifndef LLMI_PF_QUANT_BPC
#define LLMI_PF_QUANT_BPC 2
#endif
// k_pf_quant: 256-element blocks per workgroup when rows are split (0: never); LLMI_PF_QUANT_BPC (A/B)
int g_pf_quant_bpc = getenv("LLMI_PF_QUANT_BPC") ? atoi(getenv("LLMI_PF_QUANT_BPC")) : LLMI_PF_QUANT_BPC;
int g_pf_quant_split_below = 64;  // ... i.e. below this many rows (batched decode)
#ifndef LLMI_PF_XCD_MAP
#define LLMI_PF_XCD_MAP 1
#endif
int g_pf_xcd_map = LLMI_PF_XCD_MAP;  // k_pf_gemm: XCD-aware tile order
int g_pf_qkv_merge = 1;            // prefill: consecutive same-type q/k/v parts in one GEMM launch
int g_pf_gemm_ng = 2;                   // k_pf_gemm 32-token groups per workgroup (1 or 2)
int g_pf_fa_cfg = 440;                  // k_pf_fa configuration (prefill.hip pf_fa_launch)
int g_pf_attn_fa = 1;                   // batched-prefill attention: tiled FP64-MFMA kernel when it applies
int g_pf_max_kv = kPfAttnMaxKV;         // longest KV the batched-prefill attention takes
int pf_max_kv() { return g_pf_max_kv; }

hipError_t launch_embed(const EmbArgs& a, hipStream_t s) {
    launch_k(k_embed, dim3((a.cols + 255) / 256), dim3(256), 0, s, true, true, a);
    return hipGetLastError();
}

hipError_t launch_state_set(StepState* st, int token_in, int pos_next, hipStream_t s) {
    hipLaunchKernelGGL(k_state_set, dim3(1), dim3(1), 0, s, st, token_in, pos_next);
    return hipGetLastError();
}

hipError_t launch_repack(int type, const void* raw, uint8_t* a, uint8_t* h, uint8_t* sp, uint8_t* d, int64_t nblk,
                         int64_t cols, int rgs, int x86, hipStream_t s) {
    if (nblk <= 0) return hipSuccess;
    if (cols % 256) return hipErrorInvalidValue;
    if (type == T_Q4_K || type == T_Q5_K || type == T_Q6_K) {
        const int64_t thr = nblk * 4;
        hipLaunchKernelGGL(k_repack_kq, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, s, type, (const uint8_t*)raw, a,
                           h, sp, d, nblk, (int)(cols / 256), rgs, x86);
    } else if (type == T_Q8_0) {
        hipLaunchKernelGGL(k_repack_q80, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, s, (const uint8_t*)raw, a, d,
                           nblk, (int)(cols / 32), rgs);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace llmi
