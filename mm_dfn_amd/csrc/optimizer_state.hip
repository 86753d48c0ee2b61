// FlatAdam on DEVICE-RESIDENT step state (ABI 22): the step count, the bias corrections, lr / weight decay, the global gradient
// norm, its clipping factor and the skip decision live in a 64-byte block of device memory (mmdfn_adam_state), so no launch below
// takes an argument that changes from step to step -- the three of them can be nodes of a captured training step
// (graphs.CapturedStep(optimizer=...)), and clipping / skipping cost no host synchronisation.
//   mmdfn_grad_sumsq      sum g^2 in double, one partial per workgroup (fixed order, no atomics: bit-reproducible)
//   mmdfn_adam_prepare    one workgroup: norm, clip factor, skip decision, ++step and the bias corrections of the new step
//   mmdfn_adam_step_state the arithmetic of optimizer.hip's adam_step_kernel on what the block holds
// Update semantics: optimizer.hip (torch.optim.Adam with L2 folded into the gradient); the clip factor is
// torch.nn.utils.clip_grad_norm_'s min(1, max_norm / (norm + 1e-6)).
#include "mmdfn_internal.h"
#include "../../include/mmdfn_hip.h"

static_assert(sizeof(mmdfn_adam_state) == 64, "mmdfn_adam_state_bytes(): what callers allocate");

namespace {

constexpr int SUMSQ_THREADS = 256;
constexpr int SUMSQ_MAX_BLOCKS = 1024;

// sum over the wave in a fixed butterfly order (every lane gets it)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(SUMSQ_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n,
                                                                   double* __restrict__ partials) {
    __shared__ double wave_part[SUMSQ_THREADS / 64];
    const int64_t n4 = n / 4;
    double acc = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 x = reinterpret_cast<const float4*>(g)[i];
        // (products in double: the square of a float is exact there and cannot overflow)
        acc += (double)x.x * (double)x.x;
        acc += (double)x.y * (double)x.y;
        acc += (double)x.z * (double)x.z;
        acc += (double)x.w * (double)x.w;
    }
    // tail (n not a multiple of 4): the first lanes of workgroup 0
    const int64_t t = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t < n) acc += (double)g[t] * (double)g[t];
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

__global__ __launch_bounds__(SUMSQ_THREADS) void adam_prepare_kernel(mmdfn_adam_state* __restrict__ st,
                                                                     const double* __restrict__ partials, int nparts,
                                                                     float beta1, float beta2) {
    __shared__ double part[SUMSQ_MAX_BLOCKS];
    if (partials != nullptr)
        for (int i = threadIdx.x; i < nparts; i += blockDim.x) part[i] = partials[i];
    __syncthreads();
    if (threadIdx.x != 0 || !st->enabled) return;
    // one vector lane from here on: the partials in index order, then plain stores into the block
    float grad_norm = 0.0f, scale = 1.0f;
    int skip = 0;
    if (partials != nullptr) {
        double sum = 0.0;
        for (int i = 0; i < nparts; ++i) sum += part[i];
        grad_norm = (float)sqrt(sum);
        const float max_norm = st->max_norm;
        if (max_norm > 0.0f) scale = fminf(1.0f, max_norm / (grad_norm + 1e-6f));
        skip = st->skip_nonfinite && !isfinite(sum);
    }
    st->grad_norm = grad_norm;
    st->scale = scale;
    st->last_skipped = skip;
    if (skip) {
        st->skipped = st->skipped + 1;
        return;
    }
    const int step = st->step + 1;
    st->step = step;
    // bias corrections in double, rounded once (optimizer.hip: a float beta2^t next to 1 costs ~100 u on the update at steps 2..5)
    st->bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    st->bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
}

__global__ void adam_step_state_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                       float* __restrict__ v, int64_t n, const mmdfn_adam_state* __restrict__ st, float beta1,
                                       float beta2, float eps) {
    if (!st->enabled || st->last_skipped) return;          // (uniform: every lane reads the same words)
    const float wd = st->weight_decay, bc2_sqrt = st->bc2_sqrt, scale = st->scale;
    const float step_size = st->lr / st->bc1;
    const bool clip = scale < 1.0f;
    const int64_t n4 = n / 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 mv = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
#define ADAM1(F)                                                       \
    {                                                                  \
        const float gc = clip ? scale * gv.F : gv.F;                   \
        const float gg = gc + wd * pv.F;                               \
        mv.F = beta1 * mv.F + (1.0f - beta1) * gg;                     \
        vv.F = beta2 * vv.F + (1.0f - beta2) * gg * gg;                \
        pv.F -= step_size * mv.F / (sqrtf(vv.F) / bc2_sqrt + eps);     \
    }
        ADAM1(x) ADAM1(y) ADAM1(z) ADAM1(w)
#undef ADAM1
        reinterpret_cast<float4*>(p)[i] = pv;
        reinterpret_cast<float4*>(m)[i] = mv;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    // tail (n not a multiple of 4)
    const int64_t t = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t < n) {
        const float gc = clip ? scale * g[t] : g[t];
        const float gg = gc + wd * p[t];
        const float mm = beta1 * m[t] + (1.0f - beta1) * gg;
        const float vv = beta2 * v[t] + (1.0f - beta2) * gg * gg;
        m[t] = mm;
        v[t] = vv;
        p[t] -= step_size * mm / (sqrtf(vv) / bc2_sqrt + eps);
    }
}

// non-null and 16-byte aligned: the state block, and every buffer the kernels read as float4
inline bool aligned16(const void* q) { return q != nullptr && (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
inline bool state_ok(const void* st) { return aligned16(st); }

}  // namespace

extern "C" int64_t mmdfn_adam_state_bytes(void) { return (int64_t)sizeof(mmdfn_adam_state); }

extern "C" int mmdfn_grad_sumsq(const float* g, int64_t n, double* partials, int nparts_cap, int* nparts, void* stream) {
    if (n <= 0 || !aligned16(g) || partials == nullptr || nparts == nullptr || nparts_cap < 1) return -1;
    int64_t blocks = (n / 4 + SUMSQ_THREADS - 1) / SUMSQ_THREADS;
    if (blocks > SUMSQ_MAX_BLOCKS) blocks = SUMSQ_MAX_BLOCKS;
    if (blocks > nparts_cap) blocks = nparts_cap;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(SUMSQ_THREADS), 0, (hipStream_t)stream, g, n, partials);
    MMDFN_CHECK_LAUNCH();
    *nparts = (int)blocks;
    return 0;
}

extern "C" int mmdfn_adam_prepare(mmdfn_adam_state* st, const double* partials, int nparts, float beta1, float beta2,
                                  void* stream) {
    if (!state_ok(st)) return -1;
    if (partials != nullptr && (nparts < 1 || nparts > SUMSQ_MAX_BLOCKS)) return -1;
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(SUMSQ_THREADS), 0, (hipStream_t)stream, st, partials, nparts, beta1,
                       beta2);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_adam_step_state(float* p, const float* g, float* m, float* v, int64_t n, const mmdfn_adam_state* st,
                                     float beta1, float beta2, float eps, void* stream) {
    if (n <= 0 || !aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v) || !state_ok(st)) return -1;
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(adam_step_state_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, st,
                       beta1, beta2, eps);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
