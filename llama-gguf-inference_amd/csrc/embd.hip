// embd.hip — embeddings on the device (gfx950): the tail of the graph behind
// llama_get_embeddings_*: result_norm of the final hidden states and their pooling.
//
//   k_embd_rows  one workgroup of kMVThreads per token row of an [n_tok][ldx] f32 buffer.
//                The row's RMSNorm scale exactly as the logits launch's fused prologue
//                computes it (mv_norm_scale, mv_device.h): thread t sums (double)(x*x) over
//                the 16-element sub-blocks t, t + kMVThreads, ... in order, block_sum_d joins
//                the threads, scale = 1/sqrtf((float)(sum/n) + eps).  It writes the normed
//                row y = (x*scale)*w (NONE / CLS / LAST: the launcher points it at the rows
//                that are wanted) and / or scale[t] (MEAN).
//   k_embd_mean  one thread per column e over the chunk's tokens in order: upstream's
//                mul_mat(transpose(embd), inp_mean) in ggml's generic ggml_vec_dot_f32,
//                acc[e] += (double)(y[t][e] * inv) with the product in f32 and the sum in
//                FP64.  The accumulator lives in device memory and is carried from chunk to
//                chunk, so the result does not depend on where a prompt is cut; the
//                sequence's last chunk also stores out[e] = (float)acc[e].  Lanes read
//                consecutive e (coalesced); the loads of kEmbdUnroll tokens are independent
//                and issued together, only the FP64 adds are serial.
#include "kernels.h"
#include "mv_device.h"
#include "launch_util.h"

#include <hip/hip_runtime.h>

namespace llmi {

namespace {
constexpr int kEmbdMeanThreads = 64;  // one wave: n_embd / 64 workgroups spread the columns over the CUs
constexpr int kEmbdUnroll = 16;
}  // namespace

__global__ __launch_bounds__(kMVThreads) void k_embd_rows(const float* x, long long ldx, int cols, const float* w, float eps,
                                                          float* out, long long ldo, float* scale_out) {
    __shared__ double red[kMVWaves];
    const int tid = threadIdx.x, nsub = cols / 16;
    const float* xr = x + (size_t)blockIdx.x * ldx;
    double s = 0.0;
    for (int sb = tid; sb < nsub; sb += kMVThreads) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 v = *(const float4*)(xr + sb * 16 + 4 * k);
            s += (double)(v.x * v.x);
            s += (double)(v.y * v.y);
            s += (double)(v.z * v.z);
            s += (double)(v.w * v.w);
        }
    }
    s = block_sum_d<kMVWaves>(s, red);
    const float mean = (float)(s / (double)cols);
    const float scale = 1.0f / sqrtf(mean + eps);
    if (scale_out && tid == 0) scale_out[blockIdx.x] = scale;
    if (out) {
        float* o = out + (size_t)blockIdx.x * ldo;
        for (int i = tid * 4; i < cols; i += kMVThreads * 4) {
            const float4 v = *(const float4*)(xr + i), g = *(const float4*)(w + i);
            float4 y;
            y.x = (v.x * scale) * g.x;
            y.y = (v.y * scale) * g.y;
            y.z = (v.z * scale) * g.z;
            y.w = (v.w * scale) * g.w;
            *(float4*)(o + i) = y;
        }
    }
}

__global__ __launch_bounds__(kEmbdMeanThreads) void k_embd_mean(const float* x, long long ldx, int n_tok, int cols, const float* w,
                                                                const float* scale, float inv, int first, int last, double* acc,
                                                                float* out) {
    const int e = blockIdx.x * kEmbdMeanThreads + threadIdx.x;
    if (e >= cols) return;
    const float g = w[e];
    double a = first ? 0.0 : acc[e];
    const float* xe = x + e;
    int t = 0;
    for (; t + kEmbdUnroll <= n_tok; t += kEmbdUnroll) {
        float v[kEmbdUnroll], sc[kEmbdUnroll];
#pragma unroll
        for (int k = 0; k < kEmbdUnroll; ++k) {
            v[k] = xe[(size_t)(t + k) * ldx];
            sc[k] = scale[t + k];
        }
#pragma unroll
        for (int k = 0; k < kEmbdUnroll; ++k) a += (double)(((v[k] * sc[k]) * g) * inv);
    }
    for (; t < n_tok; ++t) a += (double)(((xe[(size_t)t * ldx] * scale[t]) * g) * inv);
    acc[e] = a;
    if (last) out[e] = (float)a;
}

bool embd_pool_ok(const EmbdPoolArgs& a, std::string& why) {
    if (!a.x) { why = "x_dev is a null pointer"; return false; }
    if (!a.w) { why = "norm_w_dev is a null pointer"; return false; }
    if (!a.out) { why = "out_dev is a null pointer"; return false; }
    if (a.pooling < POOLING_NONE || a.pooling > POOLING_LAST) { why = "pooling outside 0..3 (none, mean, cls, last)"; return false; }
    if (a.pooling == POOLING_MEAN && !a.acc) { why = "acc_dev is a null pointer (mean pooling)"; return false; }
    if (a.n_embd <= 0 || a.n_embd % 256) { why = "n_embd must be a positive multiple of 256"; return false; }
    if (a.ldx < a.n_embd) { why = "ldx smaller than n_embd"; return false; }
    if (a.n_tok <= 0) { why = "n_tok must be positive"; return false; }
    if (a.t0 < 0) { why = "t0 is negative"; return false; }
    if ((long long)a.t0 + a.n_tok > a.n_total) { why = "t0 + n_tok beyond n_total"; return false; }
    return true;
}

hipError_t launch_embd_pool(const EmbdPoolArgs& a, hipStream_t s) {
    std::string why;
    if (!embd_pool_ok(a, why) || (a.pooling == POOLING_MEAN && !a.scale)) return hipErrorInvalidValue;
    const int E = a.n_embd;
    const bool first = a.t0 == 0, last = a.t0 + a.n_tok == a.n_total;
    switch (a.pooling) {
    case POOLING_NONE:
        launch_k(k_embd_rows, dim3(a.n_tok), dim3(kMVThreads), 0, s, true, true, a.x, (long long)a.ldx, E, a.w, a.eps, a.out,
                 (long long)E, (float*)nullptr);
        break;
    case POOLING_CLS:
        if (first)
            launch_k(k_embd_rows, dim3(1), dim3(kMVThreads), 0, s, true, true, a.x, (long long)a.ldx, E, a.w, a.eps, a.out,
                     (long long)E, (float*)nullptr);
        break;
    case POOLING_LAST:
        if (last)
            launch_k(k_embd_rows, dim3(1), dim3(kMVThreads), 0, s, true, true, a.x + (size_t)(a.n_tok - 1) * a.ldx,
                     (long long)a.ldx, E, a.w, a.eps, a.out, (long long)E, (float*)nullptr);
        break;
    default:  // POOLING_MEAN
        launch_k(k_embd_rows, dim3(a.n_tok), dim3(kMVThreads), 0, s, true, false, a.x, (long long)a.ldx, E, a.w, a.eps,
                 (float*)nullptr, (long long)0, a.scale);
        launch_k(k_embd_mean, dim3(E / kEmbdMeanThreads), dim3(kEmbdMeanThreads), 0, s, false, true, a.x, (long long)a.ldx,
                 a.n_tok, E, a.w, (const float*)a.scale, 1.0f / (float)a.n_total, first ? 1 : 0, last ? 1 : 0, a.acc, a.out);
        break;
    }
    return hipGetLastError();
}

}  // namespace llmi
