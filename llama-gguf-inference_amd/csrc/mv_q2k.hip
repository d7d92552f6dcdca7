// mv_q2k.hip — the single-token matvec instantiations for T_Q2_K weights (mv_kernels.h):
// generic numerics only (model.cpp refuses such a load in x86 numerics), every epilogue, and
// the two-group QKV launches of Q2_K files (q / k in Q2_K, attn_v in Q3_K or Q4_K).
#include "mv_kernels.h"

namespace llmi {
template hipError_t mv_dispatch_epi<0, true, T_Q2_K, 0>(const MVArgs&, int, dim3, size_t, hipStream_t);
template hipError_t mv_dispatch_epi<0, false, T_Q2_K, 0>(const MVArgs&, int, dim3, size_t, hipStream_t);
template hipError_t mv_qkv2_launch<true, T_Q2_K, T_Q3_K, 0>(const MVArgs&, int, dim3, size_t, hipStream_t);
template hipError_t mv_qkv2_launch<true, T_Q2_K, T_Q4_K, 0>(const MVArgs&, int, dim3, size_t, hipStream_t);
}  // namespace llmi
