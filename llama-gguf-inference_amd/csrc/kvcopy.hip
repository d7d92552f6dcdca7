// kvcopy.hip — llama_kv_self_seq_cp on the device (gfx950): positions [p0, p1) of one
// sequence's K cache, V cache and token history into another sequence's, in one launch.
//
//   k_kv_seq_cp   three strided 2-D copies in one grid; every item is 16 bytes but the history's:
//     K     [planes][n_ctx][head_dim] f16: per plane one run of (p1 - p0) * head_dim / 8 uint4,
//           16-byte aligned at both ends (head_dim is a multiple of 8).
//     V     [planes * head_dim][n_ctx] f16 (transposed): per row the 8-position windows that
//           [p0, p1) touches.  A window inside the range is one uint4; the first and the last
//           may be partial: loaded whole, stored half by half, so nothing outside [p0, p1)
//           is written.
//     hist  [n_ctx] int32: one row of p1 - p0 words.
//   Each copy is cut into tiles of kCpThreads x U items (U = 4, or 1 for a copy too short to
//   fill the grid with such tiles: launch_kv_seq_cp).  2^shift lanes lie side by side along a
//   row (the smallest power of two covering the row's items, at most the workgroup), the
//   workgroup's other lanes on the rows below; a thread's U items lie along the row where it
//   is long enough, else on further rows, so a short range still fills its tiles.  A
//   workgroup walks tiles with the grid's stride; a thread's U loads come before its first
//   store, 16 KiB per workgroup in flight at U = 4.  The grid is sized from the CU count
//   (launch_kv_seq_cp's max_blocks), not from the range.  The copy is exact: 16 bits for 16
//   bits, no conversion.
#include "kernels.h"
#include "launch_util.h"

#include <algorithm>

#include <hip/hip_runtime.h>

namespace llmi {

namespace {

constexpr int kCpThreads = 256;
// items per thread and tile (the kernel's template argument U, a power of two): 4 for a copy
// that fills the grid, 1 for a shorter one, which then has four times the workgroups
constexpr int kCpUnroll = 4;
// workgroups per matvec grid-cap slot: the cap is 2 per CU by default, so 8 workgroups (8 waves
// per SIMD, the kernel's 40 VGPRs allow them) of 16 KiB of loads each per CU: a pure stream hides
// its HBM misses by what it keeps in flight
#ifndef LLMI_KVCP_GRID_MUL
#define LLMI_KVCP_GRID_MUL 4
#endif
constexpr int kCpGridMul = LLMI_KVCP_GRID_MUL;

// One thread's U items of a tile: 2^ushift of them side by side along the row (lpr
// lanes apart), the others on the rows `rstep` below.  The loads of an item past the copy's
// edge are clamped onto its last row / item and not stored: every load is unconditional, so
// the U of them are issued back to back.
template <int U>
struct CpItems {
    unsigned row0, rstep, i0, lpr, ushift, rows, width;
    __device__ __forceinline__ unsigned row(int u) const { return row0 + ((unsigned)u >> ushift) * rstep; }
    __device__ __forceinline__ unsigned item(int u) const { return i0 + ((unsigned)u & ((1u << ushift) - 1u)) * lpr; }
    __device__ __forceinline__ bool live(int u) const { return row(u) < rows && item(u) < width; }
    __device__ __forceinline__ unsigned row_c(int u) const { return min(row(u), rows - 1u); }
    __device__ __forceinline__ unsigned item_c(int u) const { return min(item(u), width - 1u); }
};

// K: a row is a plane, its items the uint4 of the plane's run
template <int U>
__device__ __forceinline__ void cp_k(const KvCopyArgs& a, const CpItems<U>& t) {
    const size_t per_pos = (size_t)(a.head_dim >> 3), plane = (size_t)a.n_ctx * per_pos, at = (size_t)a.p0 * per_pos;
    const uint4* src = (const uint4*)a.kc_src + at;
    uint4* dst = (uint4*)a.kc_dst + at;
    uint4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = src[t.row_c(u) * plane + t.item_c(u)];
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (t.live(u)) dst[t.row(u) * plane + t.item(u)] = v[u];
}

// V: a row is one (plane, dim) row of n_ctx positions, item i its 8-position window (p0 / 8 +
// i).  The whole window is loaded (it lies inside src's row); what of it lies outside
// [p0, p1) is not stored.
template <int U>
__device__ __forceinline__ void cp_v(const KvCopyArgs& a, const CpItems<U>& t) {
    const unsigned w0 = (unsigned)a.p0 >> 3;
    uint4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
        v[u] = *(const uint4*)(a.vc_src + (size_t)t.row_c(u) * a.n_ctx + (size_t)(w0 + t.item_c(u)) * 8);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (!t.live(u)) continue;
        const int lo = (int)(w0 + t.item(u)) * 8;
        uint16_t* dst = a.vc_dst + (size_t)t.row(u) * a.n_ctx;
        if (lo >= a.p0 && lo + 8 <= a.p1) {
            *(uint4*)(dst + lo) = v[u];
        } else {  // the unaligned head or tail of the row's range, half by half
            const unsigned w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (lo + j >= a.p0 && lo + j < a.p1) dst[lo + j] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
        }
    }
}

// hist: one row of int32
template <int U>
__device__ __forceinline__ void cp_hist(const KvCopyArgs& a, const CpItems<U>& t) {
    const int32_t* src = a.hist_src + a.p0;
    int32_t* dst = a.hist_dst + a.p0;
    int32_t v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = src[t.item_c(u)];
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (t.live(u)) dst[t.item(u)] = v[u];
}

// rows x width items as tiles: 2^shift lanes along a row, and of a thread's `unroll` items as
// many along the row as the row has use for (2^ushift), the others down the rows
KvCopySec cp_section(unsigned rows, unsigned width, int unroll) {
    KvCopySec s;
    s.rows = rows;
    s.width = width;
    s.shift = 0;
    while ((1u << s.shift) < width && (1u << s.shift) < (unsigned)kCpThreads) ++s.shift;
    s.ushift = 0;
    while ((1u << s.ushift) < (unsigned)unroll && ((1u << s.shift) << s.ushift) < width) ++s.ushift;
    const unsigned per_tile_w = (1u << s.shift) << s.ushift;
    const unsigned per_tile_r = ((unsigned)kCpThreads >> s.shift) * ((unsigned)unroll >> s.ushift);
    s.tiles_w = (width + per_tile_w - 1) / per_tile_w;
    s.tiles = (unsigned long long)s.tiles_w * ((rows + per_tile_r - 1) / per_tile_r);  // (checked by the launcher)
    return s;
}

}  // namespace

template <int U>
__global__ __launch_bounds__(kCpThreads) void k_kv_seq_cp(KvCopyArgs a) {
    const unsigned t = threadIdx.x;
    const unsigned total = (unsigned)(a.sec[0].tiles + a.sec[1].tiles + a.sec[2].tiles);  // < 2^31: launch_kv_seq_cp
    for (unsigned tile = blockIdx.x; tile < total; tile += gridDim.x) {
        unsigned k = tile;
        int s = 0;
        if (k >= a.sec[0].tiles) {
            k -= (unsigned)a.sec[0].tiles;
            s = 1;
            if (k >= a.sec[1].tiles) {
                k -= (unsigned)a.sec[1].tiles;
                s = 2;
            }
        }
        const KvCopySec S = a.sec[s];
        // (uniform over the workgroup: one division per tile, not per item)
        const unsigned rg = k / S.tiles_w, wg = k - rg * S.tiles_w;
        CpItems<U> it;
        it.lpr = 1u << S.shift;
        it.ushift = S.ushift;
        it.rstep = (unsigned)kCpThreads >> S.shift;
        it.row0 = rg * (it.rstep * ((unsigned)U >> S.ushift)) + (t >> S.shift);
        it.i0 = wg * (it.lpr << S.ushift) + (t & (it.lpr - 1));
        it.rows = S.rows;
        it.width = S.width;
        if (s == 0) cp_k(a, it);
        else if (s == 1) cp_v(a, it);
        else cp_hist(a, it);
    }
}

bool kv_seq_cp_ok(const KvCopyArgs& a) {
    return a.kc_src && a.vc_src && a.hist_src && a.kc_dst && a.vc_dst && a.hist_dst && a.n_planes > 0 && a.head_dim > 0 &&
           a.head_dim % 8 == 0 && a.n_ctx > 0 && a.n_ctx % 256 == 0 && a.p0 >= 0 && a.p0 < a.p1 && a.p1 <= a.n_ctx &&
           (long long)a.n_planes * a.head_dim <= 0x7fffffffLL;
}

int g_kv_cp_unroll = 0;  // test option: k_kv_seq_cp's items per thread (0 auto, 1, 4)

hipError_t launch_kv_seq_cp(const KvCopyArgs& args, int max_blocks, hipStream_t stream) {
    if (!kv_seq_cp_ok(args) || max_blocks <= 0) return hipErrorInvalidValue;
    KvCopyArgs a = args;
    const unsigned n = (unsigned)(a.p1 - a.p0);
    const unsigned long long cap = (unsigned long long)max_blocks * kCpGridMul;
    unsigned long long total = 0;
    int unroll = g_kv_cp_unroll == 1 || g_kv_cp_unroll == kCpUnroll ? g_kv_cp_unroll : kCpUnroll;
    for (;; unroll = 1) {
        a.sec[0] = cp_section((unsigned)a.n_planes, n * (unsigned)(a.head_dim >> 3), unroll);
        a.sec[1] = cp_section((unsigned)a.n_planes * (unsigned)a.head_dim, (unsigned)((a.p1 + 7) >> 3) - (unsigned)(a.p0 >> 3),
                              unroll);
        a.sec[2] = cp_section(1u, n, unroll);
        total = a.sec[0].tiles + a.sec[1].tiles + a.sec[2].tiles;
        // a copy that does not fill the grid once is bound by latency, not by bandwidth: it
        // runs faster as four times the workgroups of one item per thread
        if (unroll == 1 || g_kv_cp_unroll != 0 || total >= cap) break;
    }
    if (total > 0x7fffffffULL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::min(total, cap)), block(kCpThreads);
    if (unroll == 1) launch_k(k_kv_seq_cp<1>, grid, block, 0, stream, true, true, a);
    else launch_k(k_kv_seq_cp<kCpUnroll>, grid, block, 0, stream, true, true, a);
    return hipGetLastError();
}

}  // namespace llmi
