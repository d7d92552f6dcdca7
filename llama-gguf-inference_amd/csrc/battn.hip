// battn.hip — the batched step's attention in the generic numerics: the bodies of paths 2, 6
// and 7 (attn_device.h) with the batch slot as the last grid dimension, each slot reading
// its own sequence's KV cache, and their launch; the choices are attn.hip's selectors.  A
// unit of its own so that attn_d_body<D, P, S> has one caller per unit: with k_attn_d
// beside it the compiler schedules the entry of 36 k_battn_d instances differently.
#include "kernels.h"
#include "attn_device.h"
#include "launch_util.h"

namespace llmi {

template <int D, int G>
__global__ __launch_bounds__(256) void k_battn_scores8(BAttnArgs b) {
    const AttnArgs a = b.a[blockIdx.z];
    attn_scores8_body<D, G>(a);
}
template <int D, int G>
__global__ __launch_bounds__(512) void k_battn_pv16(BAttnArgs b, int kvb) {
    const AttnArgs a = b.a[blockIdx.z];
    attn_pv16_body<D, G>(a, kvb);
}
template <int D, int P, int S>
__global__ __launch_bounds__(512) void k_battn_d(BAttnArgs b, int G, int HK, int kvb) {
    attn_d_body<D, P, S>(attn_d_args(b.a[blockIdx.y]), G, HK, kvb, 1, 1);
}
template <int D, int G, int NP>
__global__ __launch_bounds__(256) void k_battl_scores(BAttnArgs b) { attl_scores_body<D, G, NP>(b.a[blockIdx.z]); }
__global__ __launch_bounds__(256) void k_battl_exp(BAttnArgs b, int n_head, int kvb) { attl_exp_body(b.a[blockIdx.z], n_head, kvb); }
template <int D, int G>
__global__ __launch_bounds__(512) void k_battl_pv(BAttnArgs b, int n_head, int kvb) { attl_pv_body<D, G>(b.a[blockIdx.z], n_head, kvb); }
template <int D>
__global__ __launch_bounds__(D) void k_battl_sum(BAttnArgs b, int n_head) { attl_sum_body<D>(b.a[blockIdx.z], n_head); }

// the nt slots in one grid (plain launches: the batched step is not timed per op)
hipError_t launch_battention(const BAttnArgs& b, int nt, int n_head, int n_head_kv, int head_dim, int kv_bound,
                             hipStream_t s) {
    if (nt < 1 || nt > kMaxBatch || n_head_kv <= 0 || n_head % n_head_kv) return hipErrorInvalidValue;
    // the model's numerics (every slot's): flash attention, x86 association, else generic
    if (b.a[0].fa) return launch_battention_fa(b, nt, n_head, n_head_kv, head_dim, kv_bound, s);
    if (b.a[0].num) return launch_battention_x86(b, nt, n_head, n_head_kv, head_dim, kv_bound, s);
    const int g = n_head / n_head_kv, hk = n_head_kv;
    const OfD d{head_dim};
    const OfG gq{g};
    const LongGeo lg = attn_long_geo(kv_bound);  // path 7
    bool ok = false;
    switch (battn_path(g, n_head, head_dim, kv_bound, nt)) {
        case 2:
            ok = pick([&](auto D, auto G) {
                hipLaunchKernelGGL((k_battn_scores8<D, G>), dim3(hk, (kv_bound + 31) / 32, nt), dim3(256), 0, s, b);
                hipLaunchKernelGGL((k_battn_pv16<D, G>), dim3(hk, D / 16, nt), dim3(512), (size_t)g * kv_bound * 4, s, b, kv_bound);
            }, d, gq);
            break;
        case 6:
            ok = pick([&](auto D, auto P, auto S) {
                hipLaunchKernelGGL((k_battn_d<D, P, S>), dim3(n_head * S, nt), dim3(512), 0, s, b, g, hk, kv_bound);
            }, d, Of<1, 2, 4, 8, 12, 16>{attn_passes(kv_bound, 16)}, Of<1, 2, 4, 8>{battn_slices(n_head, head_dim, kv_bound, nt)});
            break;
        case 7:
            ok = pick([&](auto D, auto G, auto NP) {
                hipLaunchKernelGGL((k_battl_scores<D, G, NP>), dim3(hk, lg.nscores, nt), dim3(256), 0, s, b);
                hipLaunchKernelGGL(k_battl_exp, dim3(n_head, lg.ntile, nt), dim3(256), 0, s, b, n_head, kv_bound);
                hipLaunchKernelGGL((k_battl_pv<D, G>), dim3(hk, lg.ntile, nt), dim3(512), 0, s, b, n_head, kv_bound);
                hipLaunchKernelGGL((k_battl_sum<D>), dim3(n_head, 1, nt), dim3(D), 0, s, b, n_head);
            }, d, gq, Of<1, 4>{lg.np});
            break;
    }
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace llmi

