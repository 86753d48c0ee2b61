// K14: all-pairs masked matching attention over a dialogue (MatchingAttention(att_type='general2'), model.py:66-76,84), every
// query row of a dialogue in one launch instead of the reference's Python loop of L x (bmm, tanh, softmax, renormalise, bmm).
//   z[t,b,s]     = <X[t,b,:], M[s,b,:]>
//   e[t,b,s]     = (mask[b,s] != 0) exp(tanh(z))            tanh bounds the exponent to [-1, 1]: no max subtraction
//   alpha[t,b,s] = e / sum_s' e[t,b,s']                     (a dialogue whose mask row is all zero: alpha = 0, pool = 0)
//   pool[t,b,:]  = sum_s alpha[t,b,s] M[s,b,:]
// backward for G = d pool (alpha is an output that is not differentiated through):
//   dP = <G[t,b,:], M[s,b,:]>,  r[t,b] = sum_s alpha dP,  dz = alpha (dP - r) (1 - tanh(z)^2)
//   dX[t,b,:] = sum_s dz[t,b,s] M[s,b,:]
//   dM[s,b,:] = sum_t dz[t,b,s] X[t,b,:] + sum_t alpha[t,b,s] G[t,b,:]
//
// Work decomposition.  match_att_rows_kernel<MODE>: one workgroup of 4 waves per (dialogue, tile of 16 query rows).
//   phase 1  the waves split the key tiles (16 keys each): a wave holds the 16 x D query tile as MFMA A fragments in registers
//            (loaded once), reads the key tile's rows of M from global as B fragments and forms the 16 x 16 scores with
//            v_mfma_f32_16x16x4_f32 (exact fp32 products, two accumulators); exp(tanh(z)) goes to the 16 x L score tile in LDS,
//            tanh(z) to `aux` for the backward pass.  A key tile whose 16 mask values are all zero is skipped (its scores are 0).
//   phase 2  16 threads per query row sum the row in a fixed order (strided partial sums, then a 16-lane DPP tree) and normalise.
//   phase 3  the waves split the D range (tiles of 16 columns, up to 4 per wave): pool = alpha M with alpha read from LDS as the
//            A operand and M from global as the B operand.
// MODE 1 is the backward pass's first launch on the same skeleton: the query operand is G, phase 1 leaves dP, phase 2 forms dz
// (written to the workspace for the second launch), phase 3 gives dX = dz M.
// match_att_keys_kernel: one workgroup per (dialogue, tile of 16 keys); dM = dz^T X + alpha^T G as ONE MFMA chain over the query
// rows in ascending order per output element -- a fixed order, no atomics: the same inputs give the same bits on every run.
// The contraction index of every MFMA is spread over the lanes so that a lane's four k values are adjacent in memory (one
// 16-byte load of X / M / the LDS tile per four MFMAs); both operands use the same assignment, which is all the sum needs.
#include "mmdfn_internal.h"
#include "../../include/mmdfn_hip.h"

namespace {

constexpr int MA_NT = 256;                 // 4 waves
constexpr int MA_MAXD = 256;
constexpr int MA_NJ = MA_MAXD / 16;        // 16-wide steps of the feature contraction
constexpr int MA_MAXL = 1008;              // the 16 x L score tile (+ padding, + the live flags) stays below 64 KB of LDS

__host__ __device__ __forceinline__ int ma_lp(int L) { return ((L + 15) & ~15) + 4; }

__device__ __forceinline__ f32x4 ma_mfma4(const float4 a, const float4 b, f32x4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
    return c;
}

// MODE 0 (forward):  Q = X, out = pool, alpha / aux written.
// MODE 1 (backward): Q = G, out = dX,  alpha / aux read, dz written.
template <int MODE>
__global__ __launch_bounds__(MA_NT) void match_att_rows_kernel(const float* __restrict__ Q, const float* __restrict__ M,
                                                               const float* __restrict__ mask, float* __restrict__ out,
                                                               float* alpha, float* aux, float* __restrict__ dz, int Tq, int L,
                                                               int B, int D) {
    extern __shared__ float ma_smem[];
    const int Lp = ma_lp(L), nkt = (L + 15) >> 4, nj = (D + 15) >> 4;
    float* Es = ma_smem;                                          // [16][Lp]
    int* live = reinterpret_cast<int*>(ma_smem + 16 * Lp);        // [nkt]: the key tile has a key that counts
    const int b = blockIdx.y, t0 = blockIdx.x * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;

    // ---- phase 1: scores.  A[row r = query][k = g], B[k = g][col r = key]; step (j, i) contracts d = 16 j + 4 g + i
    float4 qf[MA_NJ];
    {
        const int t = t0 + r;
        const float* qrow = Q + ((size_t)t * B + b) * D;
#pragma unroll
        for (int j = 0; j < MA_NJ; ++j) {
            const int d = 16 * j + 4 * g;
            qf[j] = (t < Tq && d < D) ? ld4(qrow + d) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    // the wave's next key tile is requested before the current one is contracted (one tile in flight: the tiles of a wave are
    // otherwise a chain of load, wait, 4 nj MFMAs)
    auto tile_keep = [&](int kt) {
        const int s = 16 * kt + r;
        return s < L && mask[(size_t)b * L + s] != 0.f;
    };
    auto tile_load = [&](int kt, float4 (&mf)[MA_NJ]) {
        const int s = 16 * kt + r;
        const float* mrow = M + ((size_t)s * B + b) * D;
#pragma unroll
        for (int j = 0; j < MA_NJ; ++j) {
            const int d = 16 * j + 4 * g;
            mf[j] = (s < L && d < D) ? ld4(mrow + d) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    float4 mnext[MA_NJ];
#pragma unroll
    for (int j = 0; j < MA_NJ; ++j) mnext[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    bool keep_next = false, any_next = false;
    if (wave < nkt) {
        keep_next = tile_keep(wave);
        any_next = __ballot(keep_next) != 0;                      // (wave-uniform)
        if (any_next) tile_load(wave, mnext);
    }
    for (int kt = wave; kt < nkt; kt += MA_NT / 64) {
        const int s = 16 * kt + r;
        const bool keep = keep_next, any = any_next;
        if (lane == 0) live[kt] = any ? 1 : 0;
        float4 mf[MA_NJ];
#pragma unroll
        for (int j = 0; j < MA_NJ; ++j) mf[j] = mnext[j];
        const int kn = kt + MA_NT / 64;
        if (kn < nkt) {
            keep_next = tile_keep(kn);
            any_next = __ballot(keep_next) != 0;
            if (any_next) tile_load(kn, mnext);
        }
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        if (any) {
#pragma unroll
            for (int j = 0; j < MA_NJ; j += 2) {
                if (j < nj) acc0 = ma_mfma4(qf[j], mf[j], acc0);
                if (j + 1 < nj) acc1 = ma_mfma4(qf[j + 1], mf[j + 1], acc1);
            }
        }
        // C/D: register i holds row 4 g + i (query), column r (key)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int tr = 4 * g + i, t = t0 + tr;
            const float v = acc0[i] + acc1[i];
            float e;
            if (MODE == 0) {
                const float th = tanhf(v);
                e = keep ? expf(th) : 0.f;
                if (t < Tq && s < L) aux[((size_t)t * B + b) * L + s] = keep ? th : 0.f;
            } else {
                e = keep ? v : 0.f;
            }
            Es[tr * Lp + s] = e;                                   // (s < 16 nkt <= Lp - 4; columns past L hold 0)
        }
    }
    __syncthreads();

    // ---- phase 2: 16 threads per query row, fixed order
    {
        const int tr = threadIdx.x >> 4, sub = threadIdx.x & 15, t = t0 + tr;
        const bool tv = t < Tq;
        const size_t row = tv ? ((size_t)t * B + b) * L : 0;
        float* er = Es + tr * Lp;
        if (MODE == 0) {
            float part = 0.f;
            for (int s = sub; s < L; s += 16) part += er[s];
            const float tot = row_sum16(part);
            for (int s = sub; s < L; s += 16) {
                const float a = tot > 0.f ? er[s] / tot : 0.f;
                er[s] = a;
                if (tv) alpha[row + s] = a;
            }
        } else {
            float part = 0.f;
            for (int s = sub; s < L; s += 16) part += (tv ? alpha[row + s] : 0.f) * er[s];
            const float rr = row_sum16(part);
            for (int s = sub; s < L; s += 16) {
                const float a = tv ? alpha[row + s] : 0.f;
                const float th = tv ? aux[row + s] : 0.f;
                const float v = a * (er[s] - rr) * (1.f - th * th);
                er[s] = v;
                if (tv) dz[row + s] = v;
            }
        }
    }
    __syncthreads();

    // ---- phase 3: out = Es M.  A[row r = query][k = g] = Es[r][16 kt + 4 g + kk], B[k = g][col r] = M[16 kt + 4 g + kk][d0 + r]
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // (the next live key tile's rows of M are requested before the current tile's MFMAs, as in phase 1)
    auto rows_load = [&](int kt, float4 (&bv)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ct = wave + 4 * i, d = 16 * ct + r;
            bv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ct < nj) {                                        // (wave-uniform)
                float* bp = reinterpret_cast<float*>(&bv[i]);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int s = 16 * kt + 4 * g + kk;
                    bp[kk] = (s < L && d < D) ? M[((size_t)s * B + b) * D + d] : 0.f;
                }
            }
        }
    };
    float4 bnext[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bnext[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live[0]) rows_load(0, bnext);
    for (int kt = 0; kt < nkt; ++kt) {
        float4 bcur[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bcur[i] = bnext[i];
        if (kt + 1 < nkt && live[kt + 1]) rows_load(kt + 1, bnext);
        if (!live[kt]) continue;                                  // (workgroup-uniform)
        const float4 av = *reinterpret_cast<const float4*>(Es + r * Lp + 16 * kt + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (wave + 4 * i < nj) acc[i] = ma_mfma4(av, bcur[i], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ct = wave + 4 * i, d = 16 * ct + r;
        if (ct < nj && d < D) {
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int t = t0 + 4 * g + ii;
                if (t < Tq) out[((size_t)t * B + b) * D + d] = acc[i][ii];
            }
        }
    }
}

// dM[s,b,:] = sum_t dz[t,b,s] X[t,b,:] + alpha[t,b,s] G[t,b,:].  A[row r = key][k = g] = dz / alpha [t = tt + 4 g + kk][s0 + r],
// B[k = g][col r] = X / G [t][d0 + r]; the waves split the D range as in phase 3 above.
__global__ __launch_bounds__(MA_NT) void match_att_keys_kernel(const float* __restrict__ dz, const float* __restrict__ alpha,
                                                               const float* __restrict__ X, const float* __restrict__ G,
                                                               const float* __restrict__ mask, float* __restrict__ dM, int Tq,
                                                               int L, int B, int D) {
    const int b = blockIdx.y, s0 = blockIdx.x * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int nj = (D + 15) >> 4;
    const int s = s0 + r;
    const bool keep = s < L && mask[(size_t)b * L + s] != 0.f;
    const bool any = __ballot(keep) != 0;                         // (the same in every wave: all read the same 16 keys)
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (any) {
        // operands of the 16 query rows from tt on: [0] dz, [1] alpha (A), [2 + i] X, [6 + i] G of column tile i (B); the next
        // block is requested before the current one's MFMAs
        auto block_load = [&](int tt, float4 (&op)[10]) {
            float* pz = reinterpret_cast<float*>(&op[0]);
            float* pa = reinterpret_cast<float*>(&op[1]);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int t = tt + 4 * g + kk;
                const bool ok = t < Tq && s < L;
                const size_t off = ok ? ((size_t)t * B + b) * L + s : 0;
                pz[kk] = ok ? dz[off] : 0.f;
                pa[kk] = ok ? alpha[off] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ct = wave + 4 * i, d = 16 * ct + r;
                op[2 + i] = make_float4(0.f, 0.f, 0.f, 0.f);
                op[6 + i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ct < nj) {
                    float* px = reinterpret_cast<float*>(&op[2 + i]);
                    float* pg = reinterpret_cast<float*>(&op[6 + i]);
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        const int t = tt + 4 * g + kk;
                        const bool ok = t < Tq && d < D;
                        const size_t off = ok ? ((size_t)t * B + b) * D + d : 0;
                        px[kk] = ok ? X[off] : 0.f;
                        pg[kk] = ok ? G[off] : 0.f;
                    }
                }
            }
        };
        float4 onext[10];
        block_load(0, onext);
        for (int tt = 0; tt < Tq; tt += 16) {
            float4 ocur[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) ocur[k] = onext[k];
            if (tt + 16 < Tq) block_load(tt + 16, onext);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (wave + 4 * i < nj) {
                    acc[i] = ma_mfma4(ocur[0], ocur[2 + i], acc[i]);
                    acc[i] = ma_mfma4(ocur[1], ocur[6 + i], acc[i]);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ct = wave + 4 * i, d = 16 * ct + r;
        if (ct < nj && d < D) {
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int sk = s0 + 4 * g + ii;
                if (sk < L) dM[((size_t)sk * B + b) * D + d] = acc[i][ii];
            }
        }
    }
}

bool ma_shape_ok(int Tq, int L, int B, int D) {
    return Tq >= 1 && L >= 1 && L <= MA_MAXL && B >= 1 && B <= 65535 && D >= 4 && D <= MA_MAXD && D % 4 == 0;
}

size_t ma_lds_bytes(int L) { return ((size_t)16 * ma_lp(L) + (size_t)((L + 15) >> 4)) * sizeof(float); }

}  // namespace

extern "C" int mmdfn_match_att_max_width(void) { return MA_MAXD; }
extern "C" int mmdfn_match_att_max_len(void) { return MA_MAXL; }

extern "C" int64_t mmdfn_match_att_workspace(int Tq, int L, int B, int D) {
    if (!ma_shape_ok(Tq, L, B, D)) return -1;
    return (int64_t)Tq * B * L;
}

extern "C" int mmdfn_match_att_fwd(const float* X, const float* M, const float* mask, float* pool, float* alpha, float* aux,
                                   int Tq, int L, int B, int D, void* stream) {
    if (!ma_shape_ok(Tq, L, B, D) || X == nullptr || M == nullptr || mask == nullptr || pool == nullptr || alpha == nullptr ||
        aux == nullptr)
        return -1;
    hipLaunchKernelGGL(match_att_rows_kernel<0>, dim3((unsigned)((Tq + 15) / 16), (unsigned)B), dim3(MA_NT), ma_lds_bytes(L),
                       (hipStream_t)stream, X, M, mask, pool, alpha, aux, (float*)nullptr, Tq, L, B, D);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_match_att_bwd(const float* dpool, const float* X, const float* M, const float* mask, const float* alpha,
                                   const float* aux, float* dX, float* dM, float* ws, int Tq, int L, int B, int D,
                                   void* stream) {
    if (!ma_shape_ok(Tq, L, B, D) || dpool == nullptr || X == nullptr || M == nullptr || mask == nullptr || alpha == nullptr ||
        aux == nullptr || dX == nullptr || dM == nullptr || ws == nullptr)
        return -1;
    hipLaunchKernelGGL(match_att_rows_kernel<1>, dim3((unsigned)((Tq + 15) / 16), (unsigned)B), dim3(MA_NT), ma_lds_bytes(L),
                       (hipStream_t)stream, dpool, M, mask, dX, const_cast<float*>(alpha), const_cast<float*>(aux), ws, Tq, L, B,
                       D);
    MMDFN_CHECK_LAUNCH();
    hipLaunchKernelGGL(match_att_keys_kernel, dim3((unsigned)((L + 15) / 16), (unsigned)B), dim3(MA_NT), 0, (hipStream_t)stream,
                       (const float*)ws, alpha, X, dpool, mask, dM, Tq, L, B, D);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
