// Tensor fusion (TFN, reference model_fusion.py:123-211): the three products against post_fusion_layer_1's (O, K) weight, K =
// A1 V1 T1 (A1 = Ha + 1, ...: 101^3 = 1 030 301 by default), on a GENERATED operand.  The fused tensor
//
//   Z[n, (i V1 + j) T1 + k] = [1, h_a][n, i] [1, h_v][n, j] [1, h_t][n, k]          Zd = Z (.) keep * scale   (dropout)
//
// is rank 1 per row, so every kernel rebuilds its fragments of Zd in registers from the three [1, h] rows, the keep flag of
// tfn_keep.h and the scale; nothing of size N K (Z, the mask, dZ: 7.25 GB each at N = 1 760) is ever stored.  All products are
// exact f32 (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain), sums across workgroups go through slab buffers reduced in a fixed
// order (no floating-point atomics: two runs give the same bits).
//
//   fwd    pre[n, o]  = sum_K Zd[n, K] W1[o, K]      workgroup = 64 rows x one K slab x all O columns; the W1 slab is streamed
//                                                     once through LDS in 32-wide steps; slabs summed (+ bias, ReLU) by a
//                                                     second launch
//   wgrad  dW1[o, K]  = sum_n dpre[n, o] Zd[n, K]    workgroup = 128 consecutive K x all O, loops over all rows (dpre through
//                                                     LDS, 32 rows a step); every output is written exactly once
//   dgrad  G[n, K]    = sum_o dpre[n, o] W1[o, K]    workgroup = 64 rows x a slab of (i, j) pairs; G stays in the accumulators
//          dh_t[n, k] = sum_{i,j} Gd a1[i] v1[j]      (tiles of 32 consecutive k of ONE (i, j) pair), is masked and scaled and
//          dh_v[n, j] = sum_{i,k} Gd a1[i] t1[k]      folded into per-workgroup LDS accumulators whose every entry has one owner
//          dh_a[n, i] = sum_{j,k} Gd v1[j] t1[k]      lane; slab partials summed by a second launch (the 1 slots get nothing)
//
// Lane maps of the 16x16x4 f32 MFMA (lane l): A[l & 15][l >> 4], B[l >> 4][l & 15], C/D column l & 15, row 4 (l >> 4) + reg.
#include "mmdfn_internal.h"
#include "tfn_keep.h"
#include "../../include/mmdfn_hip.h"

namespace {

constexpr int TFN_ROWS = 64;         // rows of a forward / input-gradient workgroup (16 per wave)
constexpr int TFN_BK = 32;           // K step of the staged W1 tile
constexpr int TFN_LDW_F = 36;        // LDS row pitch of the tile, forward (lanes read 8 consecutive k: 16-byte aligned rows)
constexpr int TFN_LDW_D = 48;        // ... input gradient (lanes read single floats, 4 tile rows a request: no bank shared)
constexpr int TFN_WG_K = 128;        // K columns of a weight-gradient workgroup (32 per wave)
constexpr int TFN_WG_ROWS = 32;      // rows per step of the weight-gradient loop
constexpr int TFN_MAX_LDS = 152 * 1024;

struct TfnArgs {
    const float* ha; const float* hv; const float* ht;      // (N, Ha) / (N, Hv) / (N, Ht), row strides ld*
    int ldha, ldhv, ldht;
    int64_t N;
    int A1, V1, T1, O;
    int64_t K;                                               // A1 V1 T1 (< 2^31)
    tfnk::Keep keep;
};

// [1, h][n, idx]
__device__ __forceinline__ float one_h(const float* __restrict__ h, int ld, int64_t n, int idx) {
    return idx == 0 ? 1.f : h[n * ld + (idx - 1)];
}

// A 16 OT x 32 tile of W1 (rows o, columns kbase .. kbase + 31; columns at or past kvalid and rows at or past O are zero)
// through registers: 2 OT floats per thread of 256.
template <int OT>
__device__ __forceinline__ void tile_load(float (&pre)[2 * OT], const float* __restrict__ W1, int64_t ldw, int O, int64_t kbase,
                                          int kvalid) {
    const int col = threadIdx.x & 31, row0 = threadIdx.x >> 5;
#pragma unroll
    for (int u = 0; u < 2 * OT; ++u) {
        const int row = row0 + 8 * u;
        pre[u] = (row < O && col < kvalid) ? W1[(int64_t)row * ldw + kbase + col] : 0.f;
    }
}
template <int OT, int LDW>
__device__ __forceinline__ void tile_store(const float (&pre)[2 * OT], float* __restrict__ sW) {
    const int col = threadIdx.x & 31, row0 = threadIdx.x >> 5;
#pragma unroll
    for (int u = 0; u < 2 * OT; ++u) sW[(row0 + 8 * u) * LDW + col] = pre[u];
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
// grid (row blocks, K slabs); part: [slab][N][O]
template <int OT>
__global__ __launch_bounds__(256) void tfn_fwd_kernel(const TfnArgs a, const float* __restrict__ W1, int64_t ldw,
                                                      float* __restrict__ part, int64_t slab_len) {
    extern __shared__ float smem[];
    float* sW = smem;                                   // [16 OT][TFN_LDW_F]
    float* sA = sW + 16 * OT * TFN_LDW_F;               // [64][A1]  rows of [1, h_a]
    float* sV = sA + TFN_ROWS * a.A1;
    float* sT = sV + TFN_ROWS * a.V1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, kq = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * TFN_ROWS;
    const int64_t ks = (int64_t)blockIdx.y * slab_len;
    const int64_t ke = ks + slab_len < a.K ? ks + slab_len : a.K;
    for (int idx = tid; idx < TFN_ROWS * a.A1; idx += 256) {
        const int r = idx / a.A1, i = idx - r * a.A1;
        sA[idx] = row0 + r < a.N ? one_h(a.ha, a.ldha, row0 + r, i) : 0.f;
    }
    for (int idx = tid; idx < TFN_ROWS * a.V1; idx += 256) {
        const int r = idx / a.V1, i = idx - r * a.V1;
        sV[idx] = row0 + r < a.N ? one_h(a.hv, a.ldhv, row0 + r, i) : 0.f;
    }
    for (int idx = tid; idx < TFN_ROWS * a.T1; idx += 256) {
        const int r = idx / a.T1, i = idx - r * a.T1;
        sT[idx] = row0 + r < a.N ? one_h(a.ht, a.ldht, row0 + r, i) : 0.f;
    }
    const bool drop = a.keep.used != nullptr;
    const unsigned long long seed = drop ? a.keep.used[0] : 0ull, offset = drop ? a.keep.used[1] : 0ull;
    const int64_t gpr = tfnk::groups_per_row(a.K);
    const int r = 16 * wave + c;                         // the lane's row (A operand)
    const int64_t n = row0 + r;
    const float* ra = sA + r * a.A1;
    const float* rv = sV + r * a.V1;
    const float* rt = sT + r * a.T1;
    f32x4 acc[OT];
#pragma unroll
    for (int ct = 0; ct < OT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    float pre[2 * OT];
    {
        const int64_t left = a.K - ks;
        tile_load<OT>(pre, W1, ldw, a.O, ks, left < TFN_BK ? (int)left : TFN_BK);
    }
    for (int64_t k0 = ks; k0 < ke; k0 += TFN_BK) {
        tile_store<OT, TFN_LDW_F>(pre, sW);
        __syncthreads();
        if (k0 + TFN_BK < ke) {
            const int64_t left = a.K - (k0 + TFN_BK);
            tile_load<OT>(pre, W1, ldw, a.O, k0 + TFN_BK, left < TFN_BK ? (int)left : TFN_BK);
        }
        // the lane's 8 consecutive elements of Zd: k = k0 + 8 kq + e (one keep group)
        const int64_t kb = k0 + 8 * kq;
        float z[8];
        {
            const uint32_t q = (uint32_t)kb / (uint32_t)a.T1;
            int kk = (int)((uint32_t)kb - q * (uint32_t)a.T1);
            int i = (int)(q / (uint32_t)a.V1);
            int j = (int)(q - (uint32_t)i * (uint32_t)a.V1);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool ok = kb + e < a.K;
                z[e] = ok ? (ra[ok ? i : 0] * rv[ok ? j : 0]) * rt[ok ? kk : 0] : 0.f;
                if (++kk == a.T1) {
                    kk = 0;
                    if (++j == a.V1) { j = 0; ++i; }
                }
            }
        }
        if (drop && kb < a.K && n < a.N) {
            const uint4 d = tfnk::draw8(seed, offset, n, gpr, kb >> 3);
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] *= tfnk::draw16(d, e) < a.keep.threshold ? a.keep.scale : 0.f;
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f32x4 b[OT];
#pragma unroll
            for (int ct = 0; ct < OT; ++ct)
                b[ct] = *reinterpret_cast<const f32x4*>(sW + (16 * ct + c) * TFN_LDW_F + 8 * kq + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int ct = 0; ct < OT; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(z[4 * half + e], b[ct][e], acc[ct], 0, 0, 0);
        }
        __syncthreads();
    }
    float* dst = part + (int64_t)blockIdx.y * a.N * a.O;
#pragma unroll
    for (int ct = 0; ct < OT; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t nn = row0 + 16 * wave + 4 * kq + g;
            const int o = 16 * ct + c;
            if (nn < a.N && o < a.O) dst[nn * a.O + o] = acc[ct][g];
        }
}

// out[n, o] = act(bias[o] + sum over slabs)
__global__ __launch_bounds__(256) void tfn_fwd_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                             float* __restrict__ out, int64_t NO, int O, int slabs, int relu) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < NO; e += (int64_t)gridDim.x * 256) {
        float s = part[e];
        for (int sl = 1; sl < slabs; ++sl) s += part[(int64_t)sl * NO + e];
        s += bias[e % O];
        out[e] = (relu && s < 0.f) ? 0.f : s;
    }
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------------
// grid (ceil(K / 128)); wave w owns K columns kw = 128 block + 32 w .. + 31 (two 16-column tiles) and all O rows
template <int OT>
__global__ __launch_bounds__(256) void tfn_wgrad_kernel(const TfnArgs a, const float* __restrict__ dpre, float* __restrict__ dW1) {
    constexpr int LDD = ((16 * OT + 47) / 64) * 64 + 16;      // pitch = 16 mod 64: the 4 rows of an A request share no bank
    __shared__ float sD[TFN_WG_ROWS * LDD];                    // dpre rows n0 .. n0 + 31, columns o (zero past O / N)
    __shared__ uint4 sF[4][2][64];                             // per wave: the draws of 32 rows x 4 keep groups
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, nq = lane >> 4;
    const int64_t kw = (int64_t)blockIdx.x * TFN_WG_K + 32 * wave;
    const bool drop = a.keep.used != nullptr;
    const unsigned long long seed = drop ? a.keep.used[0] : 0ull, offset = drop ? a.keep.used[1] : 0ull;
    const int64_t gpr = tfnk::groups_per_row(a.K);
    int ii[2], jj[2], kk[2];
    bool kok[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int64_t k = kw + 16 * t + c;
        kok[t] = k < a.K;
        const uint32_t ku = kok[t] ? (uint32_t)k : 0u;
        const uint32_t q = ku / (uint32_t)a.T1;
        kk[t] = (int)(ku - q * (uint32_t)a.T1);
        ii[t] = (int)(q / (uint32_t)a.V1);
        jj[t] = (int)(q - (uint32_t)ii[t] * (uint32_t)a.V1);
    }
    f32x4 acc[2][OT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int rt = 0; rt < OT; ++rt) acc[t][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float pre[2 * OT];
    auto load = [&](int64_t n0) {
#pragma unroll
        for (int u = 0; u < 2 * OT; ++u) {
            const int idx = tid + 256 * u, row = idx / (16 * OT), col = idx - row * (16 * OT);
            pre[u] = (n0 + row < a.N && col < a.O) ? dpre[(n0 + row) * a.O + col] : 0.f;
        }
    };
    load(0);
    for (int64_t n0 = 0; n0 < a.N; n0 += TFN_WG_ROWS) {
#pragma unroll
        for (int u = 0; u < 2 * OT; ++u) {
            const int idx = tid + 256 * u, row = idx / (16 * OT), col = idx - row * (16 * OT);
            sD[row * LDD + col] = pre[u];
        }
        if (drop) {
            // lane -> (row lane >> 2 of a half of 16 rows, keep group lane & 3 of the wave's 32 columns)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t nn = n0 + 16 * h + (lane >> 2), g = (kw >> 3) + (lane & 3);
                sF[wave][h][lane] = (nn < a.N && g < gpr) ? tfnk::draw8(seed, offset, nn, gpr, g) : make_uint4(0u, 0u, 0u, 0u);
            }
        }
        __syncthreads();
        if (n0 + TFN_WG_ROWS < a.N) load(n0 + TFN_WG_ROWS);
        // the three factors of Z for rows n0 + 4 s + nq: those of step s + 1 are requested before the products of step s
        float nxt[2][3];
        auto fetch = [&](int s) {
            const int64_t nn = n0 + 4 * s + nq;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const bool ok = nn < a.N && kok[t];
                nxt[t][0] = ok ? one_h(a.ha, a.ldha, nn, ii[t]) : 0.f;
                nxt[t][1] = ok ? one_h(a.hv, a.ldhv, nn, jj[t]) : 0.f;
                nxt[t][2] = ok ? one_h(a.ht, a.ldht, nn, kk[t]) : 0.f;
            }
        };
        fetch(0);
#pragma unroll 1
        for (int s = 0; s < TFN_WG_ROWS / 4; ++s) {      // (not unrolled: 152 accumulators + the prefetch leave no room)
            const int ri = 4 * s + nq;
            const int64_t nn = n0 + ri;
            float z[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) z[t] = (nxt[t][0] * nxt[t][1]) * nxt[t][2];
            if (s + 1 < TFN_WG_ROWS / 4) fetch(s + 1);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (nn < a.N && kok[t]) {
                    if (drop) {
                        const unsigned short* f = reinterpret_cast<const unsigned short*>(&sF[wave][ri >> 4][(ri & 15) * 4 + 2 * t + (c >> 3)]);
                        z[t] *= (uint32_t)f[c & 7] < a.keep.threshold ? a.keep.scale : 0.f;
                    }
                }
            }
#pragma unroll
            for (int rt = 0; rt < OT; ++rt) {
                const float av = sD[ri * LDD + 16 * rt + c];
                acc[0][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, z[0], acc[0][rt], 0, 0, 0);
                acc[1][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, z[1], acc[1][rt], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int64_t k = kw + 16 * t + c;
        if (k >= a.K) continue;
#pragma unroll
        for (int rt = 0; rt < OT; ++rt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int o = 16 * rt + 4 * nq + g;
                if (o < a.O) dW1[(int64_t)o * a.K + k] = acc[t][rt][g];
            }
    }
}

// ---- input gradients -------------------------------------------------------------------------------------------------------
// grid (row blocks, slabs of (i, j) pairs); dpart: [slab][N][A1 + V1 + T1].  dy masked by y1 > 0 when relu; the workgroups of
// slab 0 also write that dpre (N, O) for the weight gradient and the bias gradient.
template <int OT>
__global__ __launch_bounds__(256) void tfn_dgrad_kernel(const TfnArgs a, const float* __restrict__ dy, const float* __restrict__ y1,
                                                        int relu, const float* __restrict__ W1, int64_t ldw,
                                                        float* __restrict__ dpre_out, float* __restrict__ dpart, int pairs_per_slab) {
    extern __shared__ float smem[];
    // (all of it dynamic: static LDS next to the raised dynamic limit of mmdfn_allow_big_lds would pass the CU's 160 KB)
    uint4 (*sF)[80] = reinterpret_cast<uint4 (*)[80]>(smem);      // [4][80] per wave: the draws of 16 rows x 5 keep groups of a step
    float* sW = smem + 4 * 80 * 4;                      // [16 OT][TFN_LDW_D]
    float* accA = sW + 16 * OT * TFN_LDW_D;             // [64][A1] / [64][V1] / [64][T1]: every entry has ONE owner lane
    float* accV = accA + TFN_ROWS * a.A1;
    float* accT = accV + TFN_ROWS * a.V1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, nq = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * TFN_ROWS;
    const int H3 = a.A1 + a.V1 + a.T1;
    for (int idx = tid; idx < TFN_ROWS * H3; idx += 256) accA[idx] = 0.f;
    const bool drop = a.keep.used != nullptr;
    const unsigned long long seed = drop ? a.keep.used[0] : 0ull, offset = drop ? a.keep.used[1] : 0ull;
    const int64_t gpr = tfnk::groups_per_row(a.K);
    // A operand: dpre[n = row0 + 16 wave + c][o = 4 s + nq], held for the whole slab
    float af[4 * OT];
    {
        const int64_t n = row0 + 16 * wave + c;
#pragma unroll
        for (int s = 0; s < 4 * OT; ++s) {
            const int o = 4 * s + nq;
            float v = 0.f;
            if (n < a.N && o < a.O) {
                v = dy[n * a.O + o];
                if (relu && !(y1[n * a.O + o] > 0.f)) v = 0.f;
                if (blockIdx.y == 0) dpre_out[n * a.O + o] = v;
            }
            af[s] = v;
        }
    }
    const int Q = a.A1 * a.V1;
    const int q0 = blockIdx.y * pairs_per_slab;
    const int q1 = q0 + pairs_per_slab < Q ? q0 + pairs_per_slab : Q;
    const int NC = (a.T1 + TFN_BK - 1) / TFN_BK;
    float pre[2 * OT];
    {
        const int left = a.T1;
        tile_load<OT>(pre, W1, ldw, a.O, (int64_t)q0 * a.T1, left < TFN_BK ? left : TFN_BK);
    }
    int q = q0, ch = 0;
    int i = q0 / a.V1, j = q0 - i * a.V1;
    while (q < q1) {
        const int64_t kb = (int64_t)q * a.T1 + TFN_BK * ch;      // first k of the step
        const int64_t g0 = kb >> 3;
        tile_store<OT, TFN_LDW_D>(pre, sW);
        if (drop) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int id = lane + 64 * h;
                if (id < 80) {
                    const int fr = id / 5, sl = id - 5 * fr;
                    const int64_t nn = row0 + 16 * wave + fr;
                    sF[wave][id] = (nn < a.N && g0 + sl < gpr) ? tfnk::draw8(seed, offset, nn, gpr, g0 + sl) : make_uint4(0u, 0u, 0u, 0u);
                }
            }
        }
        __syncthreads();
        // next step: (q, ch + 1) or (q + 1, 0)
        int qn = q, chn = ch + 1;
        if (chn == NC) { chn = 0; ++qn; }
        if (qn < q1) {
            const int left = a.T1 - TFN_BK * chn;
            tile_load<OT>(pre, W1, ldw, a.O, (int64_t)qn * a.T1 + TFN_BK * chn, left < TFN_BK ? left : TFN_BK);
        }
        const bool two = TFN_BK * ch + 16 < a.T1;               // the second 16-column tile holds columns of this pair
        // the h values the fold below needs, requested before the products so that their latency hides behind them
        float av[4], vv[4], tv[2][4];
        int rl[4];
        bool rok[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            rl[g] = 16 * wave + 4 * nq + g;
            const int64_t nn = row0 + rl[g];
            rok[g] = nn < a.N;
            av[g] = rok[g] ? one_h(a.ha, a.ldha, nn, i) : 0.f;
            vv[g] = rok[g] ? one_h(a.hv, a.ldhv, nn, j) : 0.f;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int kk = TFN_BK * ch + 16 * t + c;
                tv[t][g] = (rok[g] && kk < a.T1) ? one_h(a.ht, a.ldht, nn, kk) : 0.f;
            }
        }
        f32x4 g0acc = f32x4{0.f, 0.f, 0.f, 0.f}, g1acc = f32x4{0.f, 0.f, 0.f, 0.f};
        if (two) {
#pragma unroll
            for (int s = 0; s < 4 * OT; ++s) {
                const float* bp = sW + (4 * s + nq) * TFN_LDW_D + c;
                g0acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s], bp[0], g0acc, 0, 0, 0);
                g1acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s], bp[16], g1acc, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int s = 0; s < 4 * OT; ++s)
                g0acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s], sW[(4 * s + nq) * TFN_LDW_D + c], g0acc, 0, 0, 0);
        }
        // fold the 16 x 32 tile of G (lane: rows 4 nq + reg of the wave's 16, columns c and 16 + c) into the accumulators
        {
            float ssum[4] = {0.f, 0.f, 0.f, 0.f};
            float x[2][4], old[2][4];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int kk = TFN_BK * ch + 16 * t + c;
                const bool okk = kk < a.T1;
                const int64_t k = (int64_t)q * a.T1 + kk;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float xv = 0.f;
                    if (okk && rok[g]) {
                        xv = t == 0 ? g0acc[g] : g1acc[g];
                        if (drop) {
                            const unsigned short* f = reinterpret_cast<const unsigned short*>(&sF[wave][(4 * nq + g) * 5 + (int)((k >> 3) - g0)]);
                            xv *= (uint32_t)f[k & 7] < a.keep.threshold ? a.keep.scale : 0.f;
                        }
                    }
                    x[t][g] = xv;
                    ssum[g] += xv * tv[t][g];
                    old[t][g] = okk ? accT[rl[g] * a.T1 + kk] : 0.f;
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int kk = TFN_BK * ch + 16 * t + c;
                if (kk < a.T1) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) accT[rl[g] * a.T1 + kk] = old[t][g] + x[t][g] * (av[g] * vv[g]);
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) ssum[g] = row_sum16(ssum[g]);
            if (c == 0) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    accV[rl[g] * a.V1 + j] += ssum[g] * av[g];
                    accA[rl[g] * a.A1 + i] += ssum[g] * vv[g];
                }
            }
        }
        __syncthreads();
        q = qn;
        ch = chn;
        if (ch == 0 && ++j == a.V1) { j = 0; ++i; }
    }
    float* dst = dpart + (int64_t)blockIdx.y * a.N * H3;
    for (int idx = tid; idx < TFN_ROWS * H3; idx += 256) {
        // accA | accV | accT are consecutive: entry (r, col) of block m
        int r, col;
        if (idx < TFN_ROWS * a.A1) { r = idx / a.A1; col = idx - r * a.A1; }
        else if (idx < TFN_ROWS * (a.A1 + a.V1)) { const int e = idx - TFN_ROWS * a.A1; r = e / a.V1; col = a.A1 + (e - r * a.V1); }
        else { const int e = idx - TFN_ROWS * (a.A1 + a.V1); r = e / a.T1; col = a.A1 + a.V1 + (e - r * a.T1); }
        if (row0 + r < a.N) dst[(row0 + r) * H3 + col] = accA[idx];
    }
}

// dh_m[n, i - 1] = sum over slabs of dpart[slab][n][block m, i], i >= 1
__global__ __launch_bounds__(256) void tfn_dgrad_reduce_kernel(const float* __restrict__ dpart, float* __restrict__ dha,
                                                               float* __restrict__ dhv, float* __restrict__ dht, int64_t N,
                                                               int A1, int V1, int T1, int slabs) {
    const int H3 = A1 + V1 + T1;
    const int64_t NH = N * H3;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < NH; e += (int64_t)gridDim.x * 256) {
        const int64_t n = e / H3;
        const int col = (int)(e - n * H3);
        float* out;
        if (col < A1) {
            if (col == 0) continue;
            out = dha + n * (A1 - 1) + (col - 1);
        } else if (col < A1 + V1) {
            if (col == A1) continue;
            out = dhv + n * (V1 - 1) + (col - A1 - 1);
        } else {
            if (col == A1 + V1) continue;
            out = dht + n * (T1 - 1) + (col - A1 - V1 - 1);
        }
        float s = dpart[e];
        for (int sl = 1; sl < slabs; ++sl) s += dpart[(int64_t)sl * NH + e];
        *out = s;
    }
}

// ---- generator state and the debug export -----------------------------------------------------------------------------------
__global__ void tfn_state_kernel(unsigned long long* __restrict__ state, unsigned long long* __restrict__ used,
                                 unsigned long long counters) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const unsigned long long off = state[1];
        used[0] = state[0];
        used[1] = off;
        state[1] = off + counters;
    }
}

__global__ __launch_bounds__(256) void tfn_keep_flags_kernel(const tfnk::Keep keep, float* __restrict__ out, int64_t K, int64_t row0,
                                                             int64_t rows) {
    const int64_t gpr = tfnk::groups_per_row(K);
    const unsigned long long seed = keep.used[0], offset = keep.used[1];
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < rows * gpr; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / gpr, g = e - r * gpr;
        const uint4 d = tfnk::draw8(seed, offset, row0 + r, gpr, g);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (8 * g + j < K) out[r * K + 8 * g + j] = tfnk::draw16(d, j) < keep.threshold ? 1.f : 0.f;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
int tfn_ot(int O) { return O < 1 ? 0 : O <= 64 ? 4 : O <= 304 ? 19 : 0; }

bool tfn_shape(int64_t N, int Ha, int Hv, int Ht, int O, TfnArgs& a) {
    if (N < 1 || N > (int64_t)1 << 40 || Ha < 1 || Hv < 1 || Ht < 1 || Ha > 4096 || Hv > 4096 || Ht > 4096 || !tfn_ot(O)) return false;
    const int64_t K = (int64_t)(Ha + 1) * (Hv + 1) * (Ht + 1);
    if (K >= ((int64_t)1 << 31) - 256) return false;
    const int64_t rows_bytes = (int64_t)TFN_ROWS * (Ha + Hv + Ht + 3) * 4;
    if (4 * 80 * 16 + 16 * tfn_ot(O) * TFN_LDW_D * 4 + rows_bytes > TFN_MAX_LDS) return false;      // (the input-gradient kernel's: the larger)
    a.N = N; a.A1 = Ha + 1; a.V1 = Hv + 1; a.T1 = Ht + 1; a.O = O; a.K = K;
    return true;
}

// K slabs of the forward launch: about two workgroups per CU in all, whole 32-wide steps
void tfn_fwd_slabs(const TfnArgs& a, int& slabs, int64_t& slab_len) {
    const int64_t rb = (a.N + TFN_ROWS - 1) / TFN_ROWS, steps = (a.K + TFN_BK - 1) / TFN_BK;
    int64_t s = 2 * MMDFN_CUS / rb;          // (rounded DOWN: one workgroup per CU, a third round for a few stragglers costs half again)
    if (s > 256) s = 256;
    if (s > steps) s = steps;
    if (s < 1) s = 1;
    slab_len = (steps + s - 1) / s * TFN_BK;
    slabs = (int)((a.K + slab_len - 1) / slab_len);
}

// slabs of (i, j) pairs of the input-gradient launch
void tfn_dgrad_slabs(const TfnArgs& a, int& slabs, int& pairs) {
    const int64_t rb = (a.N + TFN_ROWS - 1) / TFN_ROWS, Q = (int64_t)a.A1 * a.V1;
    int64_t s = 2 * MMDFN_CUS / rb;
    if (s > 256) s = 256;
    if (s > Q) s = Q;
    if (s < 1) s = 1;
    pairs = (int)((Q + s - 1) / s);
    slabs = (int)((Q + pairs - 1) / pairs);
}

bool tfn_keep(tfnk::Keep& k, const void* used, float keep, float scale) {
    k.used = reinterpret_cast<const unsigned long long*>(used);
    if (!(keep >= 0.f) || keep > 1.f) return false;
    k.threshold = keep >= 1.f ? 65536u : (uint32_t)((double)keep * 65536.0 + 0.5);
    k.scale = scale;
    return true;
}

bool tfn_rows(TfnArgs& a, const float* ha, const float* hv, const float* ht, int ldha, int ldhv, int ldht) {
    if (!ha || !hv || !ht || ldha < a.A1 - 1 || ldhv < a.V1 - 1 || ldht < a.T1 - 1) return false;
    a.ha = ha; a.hv = hv; a.ht = ht; a.ldha = ldha; a.ldhv = ldhv; a.ldht = ldht;
    return true;
}

unsigned tfn_flat_grid(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > 8 * MMDFN_CUS ? 8 * MMDFN_CUS : g);
}

}  // namespace

extern "C" int64_t mmdfn_tfn_workspace(int64_t N, int Ha, int Hv, int Ht, int O, int which) {
    TfnArgs a;
    if (!tfn_shape(N, Ha, Hv, Ht, O, a)) return -1;
    if (which == 0) {
        int slabs; int64_t len;
        tfn_fwd_slabs(a, slabs, len);
        return (int64_t)slabs * N * O;
    }
    if (which == 1) {
        int slabs, pairs;
        tfn_dgrad_slabs(a, slabs, pairs);
        return (int64_t)slabs * N * (a.A1 + a.V1 + a.T1);
    }
    return -1;
}

extern "C" int mmdfn_tfn_fwd(const float* ha, const float* hv, const float* ht, int ldha, int ldhv, int ldht, const float* W1,
                             int64_t ldw, const float* b1, void* state, void* used, int64_t counters, float keep, float scale,
                             float* out, float* workspace, int64_t N, int Ha, int Hv, int Ht, int O, int relu, void* stream) {
    TfnArgs a;
    if (!tfn_shape(N, Ha, Hv, Ht, O, a) || !tfn_rows(a, ha, hv, ht, ldha, ldhv, ldht) || !W1 || !b1 || !out || !workspace
        || ldw < a.K || (state != nullptr && (used == nullptr || counters < N * tfnk::groups_per_row(a.K))))
        return -1;
    if (!tfn_keep(a.keep, state != nullptr ? used : nullptr, keep, scale)) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (state != nullptr) {
        hipLaunchKernelGGL(tfn_state_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<unsigned long long*>(state),
                           reinterpret_cast<unsigned long long*>(used), (unsigned long long)counters);
        MMDFN_CHECK_LAUNCH();
    }
    int slabs; int64_t slab_len;
    tfn_fwd_slabs(a, slabs, slab_len);
    const int OT = tfn_ot(O);
    const size_t lds = (size_t)(16 * OT * TFN_LDW_F + TFN_ROWS * (a.A1 + a.V1 + a.T1)) * sizeof(float);
    const dim3 grid((unsigned)((N + TFN_ROWS - 1) / TFN_ROWS), (unsigned)slabs);
    if (OT == 4) {
        if (int e = mmdfn_allow_big_lds(tfn_fwd_kernel<4>)) return e;
        hipLaunchKernelGGL(tfn_fwd_kernel<4>, grid, dim3(256), lds, s, a, W1, ldw, workspace, slab_len);
    } else {
        if (int e = mmdfn_allow_big_lds(tfn_fwd_kernel<19>)) return e;
        hipLaunchKernelGGL(tfn_fwd_kernel<19>, grid, dim3(256), lds, s, a, W1, ldw, workspace, slab_len);
    }
    MMDFN_CHECK_LAUNCH();
    hipLaunchKernelGGL(tfn_fwd_reduce_kernel, dim3(tfn_flat_grid(N * O)), dim3(256), 0, s, workspace, b1, out, N * O, O, slabs,
                       relu);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_tfn_bwd_input(const float* dy, const float* y1, int relu, const float* W1, int64_t ldw, const float* ha,
                                   const float* hv, const float* ht, int ldha, int ldhv, int ldht, void* used, float keep,
                                   float scale, float* dpre, float* dha, float* dhv, float* dht, float* workspace, int64_t N,
                                   int Ha, int Hv, int Ht, int O, void* stream) {
    TfnArgs a;
    if (!tfn_shape(N, Ha, Hv, Ht, O, a) || !tfn_rows(a, ha, hv, ht, ldha, ldhv, ldht) || !dy || !W1 || !dpre || !dha || !dhv
        || !dht || !workspace || ldw < a.K || (relu && !y1))
        return -1;
    if (!tfn_keep(a.keep, used, keep, scale)) return -1;
    hipStream_t s = (hipStream_t)stream;
    int slabs, pairs;
    tfn_dgrad_slabs(a, slabs, pairs);
    const int OT = tfn_ot(O);
    const size_t lds = (size_t)(4 * 80 * 4 + 16 * OT * TFN_LDW_D + TFN_ROWS * (a.A1 + a.V1 + a.T1)) * sizeof(float);
    const dim3 grid((unsigned)((N + TFN_ROWS - 1) / TFN_ROWS), (unsigned)slabs);
    if (OT == 4) {
        if (int e = mmdfn_allow_big_lds(tfn_dgrad_kernel<4>)) return e;
        hipLaunchKernelGGL(tfn_dgrad_kernel<4>, grid, dim3(256), lds, s, a, dy, y1, relu, W1, ldw, dpre, workspace, pairs);
    } else {
        if (int e = mmdfn_allow_big_lds(tfn_dgrad_kernel<19>)) return e;
        hipLaunchKernelGGL(tfn_dgrad_kernel<19>, grid, dim3(256), lds, s, a, dy, y1, relu, W1, ldw, dpre, workspace, pairs);
    }
    MMDFN_CHECK_LAUNCH();
    hipLaunchKernelGGL(tfn_dgrad_reduce_kernel, dim3(tfn_flat_grid(N * (a.A1 + a.V1 + a.T1))), dim3(256), 0, s, workspace, dha, dhv,
                       dht, N, a.A1, a.V1, a.T1, slabs);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_tfn_bwd_weight(const float* dpre, const float* ha, const float* hv, const float* ht, int ldha, int ldhv,
                                    int ldht, void* used, float keep, float scale, float* dW1, int64_t N, int Ha, int Hv, int Ht,
                                    int O, void* stream) {
    TfnArgs a;
    if (!tfn_shape(N, Ha, Hv, Ht, O, a) || !tfn_rows(a, ha, hv, ht, ldha, ldhv, ldht) || !dpre || !dW1) return -1;
    if (!tfn_keep(a.keep, used, keep, scale)) return -1;
    const dim3 grid((unsigned)((a.K + TFN_WG_K - 1) / TFN_WG_K));
    if (tfn_ot(O) == 4)
        hipLaunchKernelGGL(tfn_wgrad_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a, dpre, dW1);
    else
        hipLaunchKernelGGL(tfn_wgrad_kernel<19>, grid, dim3(256), 0, (hipStream_t)stream, a, dpre, dW1);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_tfn_keep_flags(void* used, float keep, float* out, int64_t N, int64_t K, int64_t row0, int64_t rows,
                                    void* stream) {
    tfnk::Keep k;
    if (!used || !out || N < 1 || K < 1 || row0 < 0 || rows < 1 || row0 + rows > N || !tfn_keep(k, used, keep, 0.f)) return -1;
    hipLaunchKernelGGL(tfn_keep_flags_kernel, dim3(tfn_flat_grid(rows * tfnk::groups_per_row(K))), dim3(256), 0,
                       (hipStream_t)stream, k, out, K, row0, rows);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
