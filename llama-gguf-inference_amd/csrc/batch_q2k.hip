// batch_q2k.hip — the batched-decode kernels of batch.hip for T_Q2_K weights (generic
// numerics only): k_mvn for 1, 2, 4 and 8 tokens, k_bmm, k_bmd and the QKV pairs of k_bmd2
// that Q2_K files need (q / k in Q2_K, attn_v in Q3_K or Q4_K), every epilogue, behind
// mvn_q2k / bmm_q2k / bmm2_q2k.  A separate translation unit so the builds compile in parallel.
#define LLMI_BATCH_Q2K 1
#include "batch.hip"
