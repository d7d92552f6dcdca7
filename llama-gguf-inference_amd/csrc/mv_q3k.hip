// mv_q3k.hip — the single-token matvec instantiations for T_Q3_K weights (mv_kernels.h):
// generic numerics only (upstream's x86 association of Q3_K is another order; model.cpp refuses
// such a load), every epilogue, and the two-group QKV launches of Q3_K_M files (q / k in Q3_K,
// attn_v in Q4_K or Q5_K).
#include "mv_kernels.h"

namespace llmi {
template hipError_t mv_dispatch_epi<0, true, T_Q3_K, 0>(const MVArgs&, int, dim3, size_t, hipStream_t);
template hipError_t mv_dispatch_epi<0, false, T_Q3_K, 0>(const MVArgs&, int, dim3, size_t, hipStream_t);
template hipError_t mv_qkv2_launch<true, T_Q3_K, T_Q4_K, 0>(const MVArgs&, int, dim3, size_t, hipStream_t);
template hipError_t mv_qkv2_launch<true, T_Q3_K, T_Q5_K, 0>(const MVArgs&, int, dim3, size_t, hipStream_t);
}  // namespace llmi
