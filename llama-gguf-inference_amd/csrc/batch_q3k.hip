// batch_q3k.hip — the batched-decode kernels of batch.hip for T_Q3_K weights (generic
// numerics only): k_mvn for 1, 2, 4 and 8 tokens, k_bmm, k_bmd and the Q3_K_M QKV pairs of
// k_bmd2 (q / k in Q3_K, attn_v in Q4_K or Q5_K), every epilogue, behind mvn_q3k / bmm_q3k /
// bmm2_q3k.  A separate translation unit so the two builds compile in parallel.
#define LLMI_BATCH_Q3K 1
#include "batch.hip"
