// kvshift.hip — context shift on the device (gfx950): one sequence's cached positions
// [n_keep + d, n_past) slide down by d = n_discard in place, and the K rows are re-rotated for
// their new positions, in one launch over every layer and KV head (llmi_kv_self_seq_shift).
//
//   k_kv_shift   the tail p in [n_keep + d, n_past) of
//     K     [planes][n_ctx][head_dim] f16: row p -> row p - d.  Its first n_rot dims are rotated
//           by -d positions: with the QKV epilogue's pairing (dims 2i, 2i + 1) and (c, s) = row d
//           of its table, x0' = f16(x0*c + x1*s), x1' = f16(x1*c - x0*s) in f32 (no contraction,
//           x widened from f16): theta(-d) = -theta(d).  The dims from n_rot up move bit for bit.
//     V     [planes * head_dim][n_ctx] f16 (transposed): in every row the elements of the tail
//           move down by d elements, bit for bit.
//     hist  [n_ctx] int32: hist[p - d] = hist[p].
//   The rows [n_past - d, n_past) are left as they are: stale, and beyond the sequence's new past.
//
//   Strips.  The move is in place, and source and destination overlap whenever the tail is
//   longer than d, so the work is cut into strips that share no byte: a K strip is one plane's
//   kSliceK columns of 16 bytes (128 bytes of every row), a V strip one row, and the history is
//   one more.  A workgroup owns a K strip, or kRowsV V rows side by side, or the history; it
//   takes such items with the grid's stride (the grid is sized from the CU count), and no item
//   reads or writes what another touches: nothing relies on the order of workgroups.
//
//   Chunks.  A workgroup walks its strip in ascending chunks of kChunk = 256 positions.  Per
//   chunk every thread first loads its pieces, then the workgroup meets at a barrier, then
//   everyone rotates and stores.  Why that is safe: a chunk's stores go to [s - d, e - d) where
//   it read [s, e).  They can overlap only what this chunk or an earlier one has read (all of
//   it below e, and read before the barrier), never what a later chunk will read (from e up),
//   because dst = src - d and d >= 1: a chunk's writes end below the next chunk's reads.
//
//   K moves whole 16-byte pieces: thread t has column t % kSliceK of the slice and rows t /
//   kSliceK + 32 u of the chunk (u < kUnrollK), so its 4 pairs' (c, s) are loaded once per strip.
//   V's shift is 2-byte granular: for d % 8 != 0 source and destination differ in 16-byte
//   alignment.  A V chunk is cut by the DESTINATION's 16-byte windows (32 per row and chunk):
//   the threads load the 33 aligned source pieces those need into LDS (one aligned uint4 each;
//   through LDS because window j needs the pieces j + d / 8 and j + d / 8 + 1, the second of
//   which is the next lane's), and after the barrier each takes its two pieces back, funnels
//   them by (d % 8) * 2 bytes in registers (v_alignbyte) and stores one aligned uint4.  Only the
//   first and last window of a row's range can be partial; they are stored half by half so that
//   nothing below n_keep or from n_past - d up is written.  The stores of a chunk lie in windows
//   [j, j + 32), the next chunk's loads from window j + 32 + d / 8 up: the argument above, in
//   windows.
#include "kernels.h"
#include "launch_util.h"

#include <algorithm>

#include <hip/hip_runtime.h>

namespace llmi {

namespace {

constexpr int kShThreads = 256;
constexpr int kChunk = kKvShiftChunk;  // positions per chunk
constexpr int kSliceK = 8;             // 16-byte columns per K strip
constexpr int kUnrollK = kChunk / (kShThreads / kSliceK);  // a thread's rows per chunk: 8
constexpr int kWinV = kChunk / 8;                          // destination windows per V row and chunk: 32
constexpr int kRowsV = 32;                                 // V rows per workgroup
constexpr int kUnrollV = kRowsV * kWinV / kShThreads;      // a thread's windows per chunk: 4
// workgroups per matvec grid-cap slot, as k_kv_seq_cp: 8 per CU at the default cap of 2 per CU
constexpr int kShGridMul = 4;

__device__ __forceinline__ float sh_h2f(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(h & 0xffffu)); }
// f32 -> f16 as a rounding of its own (the empty asm keeps the compiler from folding the f32
// sum into a mixed-precision instruction that rounds once: mv_device.h's f2h)
__device__ __forceinline__ uint32_t sh_f2h(float f) {
    __asm__("" : "+v"(f));
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
}

// one (x0, x1) pair of a K row, packed as the cache holds it, rotated by -d positions
__device__ __forceinline__ uint32_t unrope(uint32_t w, float2 cs) {
    const float x0 = sh_h2f(w), x1 = sh_h2f(w >> 16);
    return sh_f2h(x0 * cs.x + x1 * cs.y) | (sh_f2h(x1 * cs.x - x0 * cs.y) << 16);
}

// K strip `strip` = (plane, slice): rows [a, n_past) -> [a - d, n_past - d), a = n_keep + d
__device__ __forceinline__ void shift_k(const KvShiftArgs& A, unsigned strip) {
    const unsigned t = threadIdx.x, col = t % kSliceK, r0 = t / kSliceK;
    const unsigned slices = (unsigned)A.head_dim / (8 * kSliceK);
    const unsigned plane = strip / slices, slice = strip - plane * slices;
    const unsigned dim0 = (slice * kSliceK + col) * 8;  // the piece's first dim
    // the pairs' (cos, sin) at position d; a pair from n_rot up is not rotated
    float2 cs[4];
    bool rot[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        rot[k] = (int)dim0 + 2 * k < A.n_rot;
        cs[k] = rot[k] ? *(const float2*)(A.rope + ((size_t)A.n_discard * (A.n_rot / 2) + dim0 / 2 + k) * 2) : float2{1.f, 0.f};
    }
    const size_t pieces = (size_t)(A.head_dim / 8);
    uint4* base = (uint4*)A.kc + (size_t)plane * A.n_ctx * pieces + slice * kSliceK + col;
    const int a = A.n_keep + A.n_discard;
    for (int s = a; s < A.n_past; s += kChunk) {
        uint4 v[kUnrollK];
        // (a row past the tail is clamped onto its last row and not stored: every load is
        // unconditional, so the kUnrollK of them are issued back to back)
#pragma unroll
        for (int u = 0; u < kUnrollK; ++u) v[u] = base[(size_t)min(s + (int)r0 + 32 * u, A.n_past - 1) * pieces];
        __syncthreads();  // the chunk is read by everyone before anyone writes into it
#pragma unroll
        for (int u = 0; u < kUnrollK; ++u) {
            const int p = s + (int)r0 + 32 * u;
            if (p >= A.n_past) continue;
            uint4 o = v[u];
            if (rot[0]) o.x = unrope(o.x, cs[0]);
            if (rot[1]) o.y = unrope(o.y, cs[1]);
            if (rot[2]) o.z = unrope(o.z, cs[2]);
            if (rot[3]) o.w = unrope(o.w, cs[3]);
            base[(size_t)(p - A.n_discard) * pieces] = o;
        }
    }
}

// dwords WO .. WO + 3 of the 32 bytes (lo, hi), taken `bb` bytes (0 or 2) further up
template <int WO>
__device__ __forceinline__ uint4 funnel_at(uint4 lo, uint4 hi, unsigned bb) {
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint4 o;
    o.x = __builtin_amdgcn_alignbyte(w[WO + 1], w[WO + 0], bb);
    o.y = __builtin_amdgcn_alignbyte(w[WO + 2], w[WO + 1], bb);
    o.z = __builtin_amdgcn_alignbyte(w[WO + 3], w[WO + 2], bb);
    o.w = __builtin_amdgcn_alignbyte(w[WO + 4], w[WO + 3], bb);
    return o;
}
// the 16 bytes that start `sh` f16 elements (0..7, uniform) into (lo, hi)
__device__ __forceinline__ uint4 funnel(uint4 lo, uint4 hi, unsigned sh) {
    const unsigned bb = (sh & 1u) * 2u;
    switch (sh >> 1) {
    case 0: return funnel_at<0>(lo, hi, bb);
    case 1: return funnel_at<1>(lo, hi, bb);
    case 2: return funnel_at<2>(lo, hi, bb);
    default: return funnel_at<3>(lo, hi, bb);
    }
}

// V rows [group * kRowsV, + kRowsV): elements [a, n_past) of each -> [n_keep, n_past - d)
__device__ __forceinline__ void shift_v(const KvShiftArgs& A, unsigned group, uint4 (*lds)[kWinV + 1]) {
    const unsigned t = threadIdx.x, wi = t % kWinV, r0 = t / kWinV;  // r0 < 8: rows r0 + 8 u
    const int end = A.n_past - A.n_discard;                          // the destination range is [n_keep, end)
    const int j0 = A.n_keep >> 3, j1 = (end + 7) >> 3;               // its windows [j0, j1)
    const int dq = A.n_discard >> 3, last = (A.n_ctx >> 3) - 1;      // source piece of window j: j + dq (and the next)
    const unsigned sh = (unsigned)A.n_discard & 7u;
    uint16_t* rows = A.vc + (size_t)group * kRowsV * A.n_ctx;
    for (int jc = j0; jc < j1; jc += kWinV) {
        // the chunk's source pieces jc + dq .. jc + dq + kWinV of every row -> LDS (a piece past
        // the row's end is clamped onto its last: nothing of it is used, end + d <= n_ctx)
#pragma unroll
        for (int u = 0; u < kUnrollV; ++u) {
            const unsigned r = r0 + 8 * u;
            lds[r][wi] = *(const uint4*)(rows + (size_t)r * A.n_ctx + (size_t)min(jc + dq + (int)wi, last) * 8);
        }
        if (t < kRowsV) lds[t][kWinV] = *(const uint4*)(rows + (size_t)t * A.n_ctx + (size_t)min(jc + dq + kWinV, last) * 8);
        __syncthreads();  // the chunk is read by everyone (the data is in LDS) before anyone writes into it
        uint4 o[kUnrollV];
#pragma unroll
        for (int u = 0; u < kUnrollV; ++u) o[u] = funnel(lds[r0 + 8 * u][wi], lds[r0 + 8 * u][wi + 1], sh);
        __syncthreads();  // LDS is free for the next chunk
        const int j = jc + (int)wi, lo = j * 8;
        if (j >= j1) continue;
#pragma unroll
        for (int u = 0; u < kUnrollV; ++u) {
            uint16_t* dst = rows + (size_t)(r0 + 8 * u) * A.n_ctx + lo;
            if (lo >= A.n_keep && lo + 8 <= end) {
                *(uint4*)dst = o[u];
            } else {  // the ragged first or last window of the row's range, half by half
                const uint32_t w[4] = {o[u].x, o[u].y, o[u].z, o[u].w};
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (lo + e >= A.n_keep && lo + e < end) dst[e] = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
            }
        }
    }
}

// hist: one strip, one position per thread and chunk
__device__ __forceinline__ void shift_hist(const KvShiftArgs& A) {
    for (int s = A.n_keep + A.n_discard; s < A.n_past; s += kChunk) {
        const int p = s + (int)threadIdx.x;
        const int32_t v = A.hist[min(p, A.n_past - 1)];
        __syncthreads();
        if (p < A.n_past) A.hist[p - A.n_discard] = v;
    }
}

}  // namespace

__global__ __launch_bounds__(kShThreads) void k_kv_shift(KvShiftArgs A) {
    __shared__ uint4 lds[kRowsV][kWinV + 1];
    const unsigned nk = (unsigned)A.n_planes * ((unsigned)A.head_dim / (8 * kSliceK));
    const unsigned nv = (unsigned)A.n_planes * (unsigned)A.head_dim / kRowsV;
    // (item and every trip count below are uniform over the workgroup: the barriers are met by all)
    for (unsigned item = blockIdx.x; item < nk + nv + 1; item += gridDim.x) {
        if (item < nk) shift_k(A, item);
        else if (item < nk + nv) shift_v(A, item - nk, lds);
        else shift_hist(A);
    }
}

hipError_t kv_shift_check(const KvShiftArgs& a) {
    if ((a.head_dim != 64 && a.head_dim != 128) || a.n_ctx % 8 != 0 || a.n_rot % 2 != 0 || a.n_rot > a.head_dim)
        return hipErrorNotSupported;
    const bool ok = a.kc && a.vc && a.hist && a.rope && a.n_planes > 0 && a.n_ctx > 0 && a.n_rot >= 0 && a.n_keep >= 0 &&
                    a.n_discard >= 1 && a.n_past <= a.n_ctx && a.n_keep <= a.n_past - a.n_discard &&
                    (long long)a.n_planes * a.head_dim <= 0x7fffffffLL && (uintptr_t)a.kc % 16 == 0 && (uintptr_t)a.vc % 16 == 0 &&
                    (uintptr_t)a.rope % 8 == 0;
    return ok ? hipSuccess : hipErrorInvalidValue;
}

hipError_t launch_kv_shift(const KvShiftArgs& a, int max_blocks, hipStream_t stream) {
    if (max_blocks <= 0) return hipErrorInvalidValue;
    if (const hipError_t e = kv_shift_check(a)) return e;
    if (a.n_keep + a.n_discard == a.n_past) return hipSuccess;  // an empty tail: the shift is a truncation
    const unsigned long long items = (unsigned long long)a.n_planes * (a.head_dim / (8 * kSliceK)) +
                                     (unsigned long long)a.n_planes * a.head_dim / kRowsV + 1;
    const dim3 grid((unsigned)std::min(items, (unsigned long long)max_blocks * kShGridMul)), block(kShThreads);
    launch_k(k_kv_shift, grid, block, 0, stream, true, true, a);
    return hipGetLastError();
}

}  // namespace llmi
