// mv_split.hip — the split-unit instantiations of the single-token matvec (k_matvec_split,
// mv_kernels.h): Q4_K and Q6_K, epilogues STORE / ADD / QKV, 256- and 512-thread workgroups,
// and the Q4_K + Q6_K QKV launch with its Q6_K group split (and its Q4_K group or not).
// mv_split_x86.hip includes this file with LLMI_MV_X86 = 1 (the x86-numerics instantiations)
#ifndef LLMI_MV_X86
#define LLMI_MV_X86 0
#endif
#include "mv_kernels.h"
namespace llmi {
template hipError_t mv_split_launch<true, T_Q4_K, LLMI_MV_X86>(const MVArgs&, int, int, hipStream_t);
template hipError_t mv_split_launch<false, T_Q4_K, LLMI_MV_X86>(const MVArgs&, int, int, hipStream_t);
template hipError_t mv_split_launch<true, T_Q6_K, LLMI_MV_X86>(const MVArgs&, int, int, hipStream_t);
template hipError_t mv_split_launch<false, T_Q6_K, LLMI_MV_X86>(const MVArgs&, int, int, hipStream_t);
template hipError_t mv_split_qkv2_launch<LLMI_MV_X86, 1>(const MVArgs&, int, hipStream_t);
template hipError_t mv_split_qkv2_launch<LLMI_MV_X86, 2>(const MVArgs&, int, hipStream_t);
}  // namespace llmi
