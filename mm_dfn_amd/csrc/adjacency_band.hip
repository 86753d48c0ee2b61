// K5b: the sparse dialogue graphs of GCNII / GCNII_lyc with new_graph=True, forward only.
//
// Replaces message_passing_relation_graph (a context window, reference model_GCN.py:381-409 / :556-584) and
// message_passing_directed_speaker (per-speaker chains, :348-379 / :523-554): per-edge Python loops that fill a dense
// (N x N) fp32 matrix and normalise it with two dense N^3 products.  Both graphs are unimodal (M = 1), block-diagonal over
// dialogues and symmetric, and ONE predicate covers both: every row carries a key (chain, rank), and rows p != q of one
// dialogue are joined iff their chains are equal and |rank_p - rank_q| <= width.
//
//     S[p,q] = 1 - acos(clamp(cos(x_p, x_q), -1, 1)) / pi   on an edge   (cos = 0 when either norm is 0; no 0.99999 shrink)
//     S[p,p] = 1,   S = 0 elsewhere,   A_hat = D^-1/2 S D^-1/2,  D = row sums of S  (>= 1: rdeg is always finite)
//
// The reference takes every weight through math.acos on a Python float: the graph is a constant for autograd, so there is
// no backward.  The result is stored in the block-tile layout of include/mmdfn_hip.h as DENSE L x ld tiles -- entries off the
// band and the pad columns are written as exact 0.0f, every consumer (propagate, the fused stack, the strip launches) takes
// them unchanged -- but dot products are formed for the pairs of the predicate only: O(N width D) work, no Gram matrix.
//
//   band_raw    -> one wave per tile row: the row's keys against the dialogue's (a ballot per 64 columns), one D-term dot
//                  product + the neighbour's squared norm per set bit, raw S row and its degree
//   band_scale  -> T[p,q] = (r_p S[p,q]) r_q with r = degree^-1/2 taken from the degrees; writes rdeg
#include "mmdfn_internal.h"
#include "../../include/mmdfn_hip.h"

namespace {

// key layout (include/mmdfn_hip.h): rank in the low 24 bits, chain above them
__device__ __forceinline__ bool band_edge(int kp, int kq, int width) {
    const int dr = (kp & 0xFFFFFF) - (kq & 0xFFFFFF);
    return (kp >> 24) == (kq >> 24) && dr <= width && -dr <= width;
}

// explicit fmaf, one accumulator per lane, elements in index order: x_p.x_q and x_q.x_p are the same bits, and so is a
// row's squared norm whether it is taken as "own" or as "neighbour" -- S comes out bitwise symmetric
__device__ __forceinline__ float fma4(float4 a, float4 b, float s) {
    s = fmaf(a.x, b.x, s);
    s = fmaf(a.y, b.y, s);
    s = fmaf(a.z, b.z, s);
    return fmaf(a.w, b.w, s);
}

// NCH > 0: the row's own features live in NCH float4 registers per lane (D <= 256 NCH); NCH = 0: any D, re-read per pair
template <int NCH>
__global__ __launch_bounds__(256) void band_raw_kernel(const float* __restrict__ feats, const int32_t* __restrict__ keys,
                                                       float* __restrict__ deg, float* __restrict__ tiles,
                                                       const int32_t* __restrict__ dia_len,
                                                       const int32_t* __restrict__ row_start,
                                                       const int64_t* __restrict__ tile_base, int D, int max_len,
                                                       int width) {
    const int rowblocks = (max_len + 3) / 4;
    const int i = blockIdx.x / rowblocks;
    const int p = (blockIdx.x % rowblocks) * 4 + (threadIdx.x >> 6);
    const int L = dia_len[i];
    if (p >= L) return;
    const int lane = threadIdx.x & 63;
    const int ld = (L + 3) & ~3;
    const int rs = row_start[i];
    const float* xp = feats + (int64_t)(rs + p) * D;
    float* t = tiles + tile_base[i] + (int64_t)p * ld;
    const int kp = keys[rs + p];

    float4 own[NCH > 0 ? NCH : 1];
    float pp = 0.f;
    if (NCH > 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int k = (lane + 64 * c) * 4;
            own[c] = k < D ? ld4(xp + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            pp = fma4(own[c], own[c], pp);
        }
    } else {
        for (int k = lane * 4; k < D; k += 256) {
            const float4 a = ld4(xp + k);
            pp = fma4(a, a, pp);
        }
    }
    const float np = sqrtf(wave_sum(pp));

    float rowsum = 0.f;
    for (int q0 = 0; q0 < ld; q0 += 64) {
        const int q = q0 + lane;
        const bool edge = q < L && q != p && band_edge(kp, keys[rs + (q < L ? q : 0)], width);
        unsigned long long todo = __ballot(edge);
        float val = q == p ? 1.0f : 0.0f;             // the diagonal is torch.eye's 1, not a dot product
        while (todo) {                                // (wave-uniform: one neighbour per turn)
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const float* xq = feats + (int64_t)(rs + q0 + j) * D;
            float pq = 0.f, qq = 0.f;
            if (NCH > 0) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int k = (lane + 64 * c) * 4;
                    const float4 b = k < D ? ld4(xq + k) : make_float4(0.f, 0.f, 0.f, 0.f);
                    pq = fma4(own[c], b, pq);
                    qq = fma4(b, b, qq);
                }
            } else {
                for (int k = lane * 4; k < D; k += 256) {
                    const float4 a = ld4(xp + k), b = ld4(xq + k);
                    pq = fma4(a, b, pq);
                    qq = fma4(b, b, qq);
                }
            }
            pq = wave_sum(pq);
            const float nq = sqrtf(wave_sum(qq));
            const float den = np * nq;
            float c = den == 0.f ? 0.f : pq / den;    // cossim: `if b == 0: return 0` -- never an x / 0 unit row
            c = fminf(fmaxf(c, -1.0f), 1.0f);         // atom_calculate_edge_weight
            const float w = 1.0f - acosf(c) / MMDFN_PI_F;
            if (lane == j) val = w;
        }
        rowsum += val;
        if (q < ld) t[q] = val;                       // off the band and in the pad columns: exact zeros
    }
    rowsum = wave_sum(rowsum);
    if (lane == 0) deg[rs + p] = rowsum;
}

// T[p,q] = (r_p S[p,q]) r_q, r = deg^-1/2  -- one wave per tile row; lane 0 leaves r_p in rdeg
__global__ __launch_bounds__(256) void band_scale_kernel(float* __restrict__ tiles, const float* __restrict__ deg,
                                                         float* __restrict__ rdeg, const int32_t* __restrict__ dia_len,
                                                         const int32_t* __restrict__ row_start,
                                                         const int64_t* __restrict__ tile_base, int max_len) {
    const int rowblocks = (max_len + 3) / 4;
    const int i = blockIdx.x / rowblocks;
    const int p = (blockIdx.x % rowblocks) * 4 + (threadIdx.x >> 6);
    const int L = dia_len[i];
    if (p >= L) return;
    const int lane = threadIdx.x & 63;
    const int ld = (L + 3) & ~3;
    const int rs = row_start[i];
    float* t = tiles + tile_base[i] + (int64_t)p * ld;
    const float rp = powf(deg[rs + p], -0.5f);
    for (int q = lane; q < L; q += 64) {
        const float s = t[q];
        if (s != 0.f) t[q] = (rp * s) * powf(deg[rs + q], -0.5f);
    }
    if (lane == 0) rdeg[rs + p] = rp;
}

}  // namespace

extern "C" int mmdfn_adj_build_band(const float* feats, const int32_t* keys, float* deg, float* rdeg, float* tiles,
                                    const int32_t* dia_len, const int32_t* row_start, const int64_t* tile_base, int B, int M,
                                    int N, int D, int max_len, int width, void* stream) {
    if (B <= 0 || M != 1 || N <= 0 || D <= 0 || (D & 3) || max_len <= 0 || width < 0) return -1;
    if (!feats || !keys || !deg || !rdeg || !tiles || !dia_len || !row_start || !tile_base) return -1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)B * (unsigned)((max_len + 3) / 4)), block(256);
#define BAND_RAW(NCH) hipLaunchKernelGGL(band_raw_kernel<NCH>, grid, block, 0, s, feats, keys, deg, tiles, dia_len, row_start, tile_base, D, max_len, width)
    if (D <= 256) BAND_RAW(1);
    else if (D <= 512) BAND_RAW(2);
    else BAND_RAW(0);
#undef BAND_RAW
    MMDFN_CHECK_LAUNCH();
    hipLaunchKernelGGL(band_scale_kernel, grid, block, 0, s, tiles, deg, rdeg, dia_len, row_start, tile_base, max_len);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
