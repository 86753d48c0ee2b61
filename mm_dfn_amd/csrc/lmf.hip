// Low-rank multimodal fusion (LMF, reference model_fusion.py:214-310): the rank-weighted product over the three modalities, one
// launch each way.  The dense products of the module -- the three subnets and [1, h_m] . factor_m -- run on the few-row grouped
// MFMA kernel (linear_small.hip) and the weight-gradient kernels (gemm_tn.hip); what is left is pointwise over (row, column)
// with a row reduction for d fusion_weights:
//
//   P_m,r = h_m . factor_m[r, 1:, :]   (written by the grouped linear kernel into column block (m R + r) of P)
//   fwd:  P_m,r += factor_m[r, 0, :]   (the constant 1 of [1, h_m], kept in P for the backward pass)
//         out = sum_r w_r P_a,r (.) P_v,r (.) P_t,r + bias
//   bwd:  dP_a,r = g w_r P_v,r (.) P_t,r   (and its two rotations)
//         T_r   = sum_o g (.) P_a,r (.) P_v,r (.) P_t,r       (row partial of d fusion_weights)
//   D = [dP (3 R O columns) | g (O) | T (R)] row by row: one column-sum launch of D then yields d factor_m[r, 0, :],
//   d fusion_bias and d fusion_weights together; d factor_m[r, 1:, :] = h_m^T dP_m,r and dh_m = sum_r dP_m,r factor_m[r, 1:, :]^T
//   are grouped gemm_tn / linear launches on the column blocks of D.
#include "mmdfn_internal.h"
#include "../../include/mmdfn_hip.h"

namespace {

constexpr int LMF_RMAX = 8;

// grid-stride over rows, one workgroup per row; columns o = threadIdx.x + 256 k
__global__ __launch_bounds__(256) void lmf_fwd_kernel(float* __restrict__ P, const float* __restrict__ fa,
                                                      const float* __restrict__ fv, const float* __restrict__ ft, int64_t sa,
                                                      int64_t sv, int64_t st, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ out, int64_t N, int O,
                                                      int R, int ldp, int ldo) {
    for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
        float* pr = P + n * ldp;
        for (int o = threadIdx.x; o < O; o += blockDim.x) {
            float acc = bias[o];
            for (int r = 0; r < R; ++r) {
                const float pa = pr[(0 * R + r) * O + o] + fa[r * sa + o];
                const float pv = pr[(1 * R + r) * O + o] + fv[r * sv + o];
                const float pt = pr[(2 * R + r) * O + o] + ft[r * st + o];
                pr[(0 * R + r) * O + o] = pa;
                pr[(1 * R + r) * O + o] = pv;
                pr[(2 * R + r) * O + o] = pt;
                acc += w[r] * (pa * pv * pt);
            }
            out[n * ldo + o] = acc;
        }
    }
}

__global__ __launch_bounds__(256) void lmf_bwd_kernel(const float* __restrict__ g, const float* __restrict__ P,
                                                      const float* __restrict__ w, float* __restrict__ D, int64_t N, int O, int R,
                                                      int ldg, int ldp, int ldd) {
    __shared__ float red[4][LMF_RMAX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
        const float* pr = P + n * ldp;
        float* dr = D + n * ldd;
        float T[LMF_RMAX];
#pragma unroll
        for (int r = 0; r < LMF_RMAX; ++r) T[r] = 0.f;
        for (int o = threadIdx.x; o < O; o += blockDim.x) {
            const float gv = g[n * ldg + o];
#pragma unroll
            for (int r = 0; r < LMF_RMAX; ++r) {
                if (r < R) {
                    const float pa = pr[(0 * R + r) * O + o], pv = pr[(1 * R + r) * O + o], pt = pr[(2 * R + r) * O + o];
                    const float q = gv * w[r];
                    dr[(0 * R + r) * O + o] = q * (pv * pt);
                    dr[(1 * R + r) * O + o] = q * (pa * pt);
                    dr[(2 * R + r) * O + o] = q * (pa * pv);
                    T[r] += gv * (pa * pv * pt);
                }
            }
            dr[3 * R * O + o] = gv;
        }
#pragma unroll
        for (int r = 0; r < LMF_RMAX; ++r) {
            const float s = wave_sum(T[r]);
            if (lane == 0) red[wv][r] = s;
        }
        __syncthreads();
        if (threadIdx.x < R)
            dr[3 * R * O + O + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        for (int c = 3 * R * O + O + R + threadIdx.x; c < ldd; c += blockDim.x) dr[c] = 0.f;      // (row padding: summed too)
        __syncthreads();                                     // red[] is rewritten by the next row
    }
}

unsigned lmf_grid(int64_t N) { return (unsigned)(N < 4096 ? N : 4096); }

}  // namespace

extern "C" int mmdfn_lmf_bwd_width(int O, int R) { return ((3 * R * O + O + R) + 3) & ~3; }

extern "C" int mmdfn_lmf_fwd(float* P, const float* factor_a, const float* factor_v, const float* factor_t, int64_t rank_stride_a,
                             int64_t rank_stride_v, int64_t rank_stride_t, const float* w, const float* bias, float* out,
                             int64_t N, int O, int R, int ldp, int ldo, void* stream) {
    if (N <= 0 || O < 1 || R < 1 || R > LMF_RMAX || ldp < 3 * R * O || ldo < O) return -1;
    hipLaunchKernelGGL(lmf_fwd_kernel, dim3(lmf_grid(N)), dim3(256), 0, (hipStream_t)stream, P, factor_a, factor_v, factor_t,
                       rank_stride_a, rank_stride_v, rank_stride_t, w, bias, out, N, O, R, ldp, ldo);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_lmf_bwd(const float* g, const float* P, const float* w, float* D, int64_t N, int O, int R, int ldg, int ldp,
                             int ldd, void* stream) {
    if (N <= 0 || O < 1 || R < 1 || R > LMF_RMAX || ldg < O || ldp < 3 * R * O || ldd < mmdfn_lmf_bwd_width(O, R)) return -1;
    hipLaunchKernelGGL(lmf_bwd_kernel, dim3(lmf_grid(N)), dim3(256), 0, (hipStream_t)stream, g, P, w, D, N, O, R, ldg, ldp, ldd);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
