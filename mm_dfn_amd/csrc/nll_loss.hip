// K12: NLLLoss forward / backward as one launch each (torch.nn.NLLLoss(weight, ignore_index, reduction), what the reference's
// training script builds for --loss NLLLoss [--class_weight], run_train_erc.py:509).
//   loss = sum_{i : t_i != ignore} w[t_i] * (-log_prob[i, t_i])  /  sum_{i : t_i != ignore} w[t_i]        ('mean'; 'sum': no division)
//   d loss / d log_prob[i, c] = (c == t_i) * (-w[t_i]) * scale,   scale = 1 / sum of the weights ('mean') or 1 ('sum')
// Modelled on the *_ignore launches of focal_loss.hip: ONE workgroup walks the rows with a fixed row -> thread assignment and
// reduces in a fixed tree (bit-reproducible, no atomics); the denominator is taken on the device, so a captured step serves
// batches with different numbers of rows that count.  Both sums are kept in float64 (one workgroup, a handful of rows per
// thread): the loss is the correctly rounded quotient of the exact products.
// Edge rules (as FocalLoss): every row ignored -> loss 0, scale 0 (torch: NaN); a label outside [0, C) that is not ignore_index
// -> NaN loss and a NaN gradient row (torch raises; a kernel cannot without a host sync).
#include "mmdfn_internal.h"
#include "../../include/mmdfn_hip.h"

namespace {

constexpr int NLL_NT = 1024;

__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(NLL_NT) void nll_loss_fwd_kernel(const float* __restrict__ logp, const int64_t* __restrict__ target,
                                                              const float* __restrict__ weight, float* __restrict__ loss,
                                                              float* __restrict__ coef, float* __restrict__ scale_out, int64_t N,
                                                              int C, int mean, int64_t ignore_index) {
    __shared__ double part[NLL_NT / 64];
    __shared__ double wpart[NLL_NT / 64];
    __shared__ int cpart[NLL_NT / 64];
    double acc = 0.0, wsum = 0.0;
    int cnt = 0;
    for (int64_t i = threadIdx.x; i < N; i += NLL_NT) {
        int64_t t = target[i];
        if (t == ignore_index) {
            coef[i] = 0.f;
            continue;
        }
        const bool bad = t < 0 || t >= C;
        t = bad ? 0 : t;
        const float lp = bad ? __builtin_nanf("") : logp[i * C + t];
        float w = weight != nullptr ? weight[t] : 1.f;
        if (bad) w = __builtin_nanf("");
        coef[i] = -w;
        acc += (double)w * (double)(-lp);
        wsum += (double)w;
        ++cnt;
    }
    acc = wave_sum_f64(acc);
    wsum = wave_sum_f64(wsum);
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6] = acc;
        wpart[threadIdx.x >> 6] = wsum;
        cpart[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0, ws = 0.0;
        int n = 0;
#pragma unroll
        for (int w = 0; w < NLL_NT / 64; ++w) {
            s += part[w];
            ws += wpart[w];
            n += cpart[w];
        }
        if (n == 0) {                       // every row ignored: 0 with zero gradients
            loss[0] = 0.f;
            scale_out[0] = mean ? 0.f : 1.f;
        } else if (mean) {                  // (all weights that count zero: 0 / 0 = NaN, as torch)
            loss[0] = (float)(s / ws);
            scale_out[0] = (float)(1.0 / ws);
        } else {
            loss[0] = (float)s;
            scale_out[0] = 1.f;
        }
    }
}

__global__ __launch_bounds__(256) void nll_loss_bwd_kernel(const float* __restrict__ coef, const int64_t* __restrict__ target,
                                                           const float* __restrict__ dloss, const float* __restrict__ scale,
                                                           float* __restrict__ dlogp, int64_t N, int C, int64_t ignore_index) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (idx >= N * C) return;
    const int64_t i = idx / C;
    const int c = (int)(idx - i * C);
    const int64_t t = target[i];
    float v = 0.f;
    if (t != ignore_index && (c == t || t < 0 || t >= C)) v = coef[i] * scale[0] * dloss[0];     // bad label: coef is NaN
    dlogp[idx] = v;
}

}  // namespace

extern "C" int mmdfn_nll_loss_threads(void) { return NLL_NT; }

extern "C" int mmdfn_nll_loss_fwd(const float* logp, const int64_t* target, const float* weight, float* loss, float* coef,
                                  float* scale_out, int64_t N, int C, int mean, int64_t ignore_index, void* stream) {
    if (N <= 0 || C <= 0 || logp == nullptr || target == nullptr || loss == nullptr || coef == nullptr || scale_out == nullptr)
        return -1;
    hipLaunchKernelGGL(nll_loss_fwd_kernel, dim3(1), dim3(NLL_NT), 0, (hipStream_t)stream, logp, target, weight, loss, coef,
                       scale_out, N, C, mean, ignore_index);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_nll_loss_bwd(const float* coef, const int64_t* target, const float* dloss, const float* scale, float* dlogp,
                                  int64_t N, int C, int64_t ignore_index, void* stream) {
    if (N <= 0 || C <= 0 || coef == nullptr || target == nullptr || dloss == nullptr || scale == nullptr || dlogp == nullptr)
        return -1;
    const int64_t total = N * C;
    hipLaunchKernelGGL(nll_loss_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, coef,
                       target, dloss, scale, dlogp, N, C, ignore_index);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

// K15: MaskedNLLLoss (reference loss.py:38-58), the objective of the recurrent baselines (run_train_erc.py:92-146):
//   loss = sum_i m_i w[t_i] (-pred[i, t_i])  /  sum_i m_i w[t_i]          (w = 1 without a weight table; m: the 0 / 1 utterance mask)
//   d loss / d pred[i, c] = (c == t_i) (-m_i w[t_i]) / sum_i m_i w[t_i]
// The K12 launch shape: ONE workgroup, fixed row -> thread assignment, both sums in float64 through a fixed tree, the denominator
// taken on the device.  Edge rules as K12: no row with a non-zero mask -> loss 0, scale 0 (the reference: 0 / 0 = NaN); a label
// outside [0, C) on a row that counts -> NaN loss and a NaN gradient row.  Rows whose mask is 0 never read their label's column.
namespace {

__global__ __launch_bounds__(NLL_NT) void masked_nll_fwd_kernel(const float* __restrict__ pred, const int64_t* __restrict__ target,
                                                                const float* __restrict__ mask, const float* __restrict__ weight,
                                                                float* __restrict__ loss, float* __restrict__ coef,
                                                                float* __restrict__ scale_out, int64_t N, int C) {
    __shared__ double part[NLL_NT / 64];
    __shared__ double wpart[NLL_NT / 64];
    __shared__ int cpart[NLL_NT / 64];
    double acc = 0.0, wsum = 0.0;
    int cnt = 0;
    for (int64_t i = threadIdx.x; i < N; i += NLL_NT) {
        const float m = mask[i];
        if (m == 0.f) {
            coef[i] = 0.f;
            continue;
        }
        int64_t t = target[i];
        const bool bad = t < 0 || t >= C;
        t = bad ? 0 : t;
        const float lp = bad ? __builtin_nanf("") : pred[i * C + t];
        float w = weight != nullptr ? weight[t] : 1.f;
        if (bad) w = __builtin_nanf("");
        const float mw = m * w;
        coef[i] = -mw;
        acc += (double)mw * (double)(-lp);
        wsum += (double)mw;
        ++cnt;
    }
    acc = wave_sum_f64(acc);
    wsum = wave_sum_f64(wsum);
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6] = acc;
        wpart[threadIdx.x >> 6] = wsum;
        cpart[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0, ws = 0.0;
        int n = 0;
#pragma unroll
        for (int w = 0; w < NLL_NT / 64; ++w) {
            s += part[w];
            ws += wpart[w];
            n += cpart[w];
        }
        if (n == 0) {                       // every row masked: 0 with zero gradients
            loss[0] = 0.f;
            scale_out[0] = 0.f;
        } else {                            // (all weights that count zero: 0 / 0 = NaN, as the reference)
            loss[0] = (float)(s / ws);
            scale_out[0] = (float)(1.0 / ws);
        }
    }
}

__global__ __launch_bounds__(256) void masked_nll_bwd_kernel(const float* __restrict__ coef, const int64_t* __restrict__ target,
                                                             const float* __restrict__ mask, const float* __restrict__ dloss,
                                                             const float* __restrict__ scale, float* __restrict__ dpred,
                                                             int64_t N, int C) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (idx >= N * C) return;
    const int64_t i = idx / C;
    const int c = (int)(idx - i * C);
    float v = 0.f;
    if (mask[i] != 0.f) {
        const int64_t t = target[i];
        if (c == t || t < 0 || t >= C) v = coef[i] * scale[0] * dloss[0];     // bad label: coef is NaN
    }
    dpred[idx] = v;
}

}  // namespace

extern "C" int mmdfn_masked_nll_fwd(const float* pred, const int64_t* target, const float* mask, const float* weight, float* loss,
                                    float* coef, float* scale_out, int64_t N, int C, void* stream) {
    if (N <= 0 || C <= 0 || pred == nullptr || target == nullptr || mask == nullptr || loss == nullptr || coef == nullptr ||
        scale_out == nullptr)
        return -1;
    hipLaunchKernelGGL(masked_nll_fwd_kernel, dim3(1), dim3(NLL_NT), 0, (hipStream_t)stream, pred, target, mask, weight, loss,
                       coef, scale_out, N, C);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_masked_nll_bwd(const float* coef, const int64_t* target, const float* mask, const float* dloss,
                                    const float* scale, float* dpred, int64_t N, int C, void* stream) {
    if (N <= 0 || C <= 0 || coef == nullptr || target == nullptr || mask == nullptr || dloss == nullptr || scale == nullptr ||
        dpred == nullptr)
        return -1;
    const int64_t total = N * C;
    hipLaunchKernelGGL(masked_nll_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, coef,
                       target, mask, dloss, scale, dpred, N, C);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
