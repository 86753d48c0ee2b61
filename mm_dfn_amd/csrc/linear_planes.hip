// K1p: dense projections  Y = act(X W^T + b) (+ Y)  against a weight that arrives as bf16 PIECE PLANES.
//
// Replaces nn.Linear / F.linear for the hoisted GRU input contractions of both recurrent encoders and their input gradients
// (reference model.py:866,868,1082,1132: `nn.GRU` input products of `lstm_l` / `rnn_parties`; run_train_erc.py:512 is where the
// weights change) at the row counts of the BASELINE configs (1 760 .. 19 008 rows, K = 200 / 600, N = 600 / 200).
//
// Why another form.  The 128 x 128-tile kernels (linear_split.hip) cut BOTH operands in every workgroup, run 7 chunks of a
// software pipeline whose prologue and epilogue weigh as much as the chunks, and put 275 workgroups on 256 CUs: 33 us for a
// product whose matrix time is 4 us ("weak" 7).  A weight changes once per optimizer step, so its three bf16
// pieces are cut ONCE per step (mmdfn_cut_weight_planes, one grouped launch for all registered weights) and stored in MFMA
// B-fragment order; here
//   * a workgroup = 64 rows x 128 columns, wave = 64 rows x ONE 32-column tile (two 32 x 32 accumulators): 2 090 wave tasks of
//     168 MFMAs at 7 040 x 200 -> 600, four workgroups resident per CU (24 KB of LDS, < 128 VGPRs), so the chip fills evenly and
//     the phases of different workgroups overlap;
//   * B fragments (the weight pieces) go L2 -> registers with ONE coalesced 1 KB load per piece and k-step, one phase ahead:
//     no cutting, no LDS, no barrier on the B side;
//   * A (the X rows) is cut once per workgroup -- 1/4 per wave -- into LDS in A-fragment order (16 bytes per lane, conflict
//     free), two k-steps (32 k) per phase, double-buffered, one barrier per phase.
// Arithmetic: the six piece products of bf16_pieces.h.
// Plane layout: planes_common.h; the main loop: planes_pipeline.h (shared with the GCN stack's plane kernels, gcn_planes.hip).
#include "planes_common.h"
#include "../../include/mmdfn_hip.h"

namespace {

constexpr int PL_MAXW = 16;        // weights per cut launch

struct CutTable {
    const float* w1[PL_MAXW];      // first block of the stored matrix
    const float* w2[PL_MAXW];      // second block (null: one block)
    u32x4* planes[PL_MAXW];
    int n1[PL_MAXW], ld[PL_MAXW];
    int N[PL_MAXW], K[PL_MAXW];    // of the B operand: N output columns, K contraction
    int mode[PL_MAXW];             // see mmdfn_cut_weight_planes
    int prefix[PL_MAXW + 1];       // fragment-lane tasks (NT * KS * 64) before weight i
    int n;
};

// element B[n][k] of weight i (0 outside N x K)
__device__ __forceinline__ float cut_element(const CutTable& T, int i, int n, int k) {
    const int N = T.N[i], K = T.K[i], ld = T.ld[i], n1 = T.n1[i];
    if (n >= N || k >= K) return 0.f;
    int row, col;
    const float* base;
    switch (T.mode[i]) {
        case 0:                    // B[n][k] = stored[n][k], stored rows split at n1
            row = n; col = k;
            base = row < n1 ? T.w1[i] : T.w2[i];
            if (row >= n1) row -= n1;
            break;
        case 1:                    // B[n][k] = stored[k][n], stored rows split at n1
            row = k; col = n;
            base = row < n1 ? T.w1[i] : T.w2[i];
            if (row >= n1) row -= n1;
            break;
        case 2:                    // B[n][k] = w1[k][n] (n < n1) | w2[k][n - n1]: two matrices side by side, transposed
            row = k; col = n;
            base = col < n1 ? T.w1[i] : T.w2[i];
            if (col >= n1) col -= n1;
            break;
        default: {                 // 3: as 2 with the contraction index gate-interleaved: k = 4 u + g  <->  stored row g (K / 4) + u
            const int H = K >> 2;
            row = (k & 3) * H + (k >> 2); col = n;
            base = col < n1 ? T.w1[i] : T.w2[i];
            if (col >= n1) col -= n1;
            break;
        }
    }
    return base[(int64_t)row * ld + col];
}

// one thread = one fragment lane (ct, ks, lane): 8 elements in, 3 x 16 bytes out
__global__ __launch_bounds__(256) void cut_planes_kernel(CutTable T) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= T.prefix[T.n]) return;
    int i = 0;
    while (i + 1 < T.n && g >= T.prefix[i + 1]) ++i;
    const int t = g - T.prefix[i];
    const int N = T.N[i], K = T.K[i], ld = T.ld[i], n1 = T.n1[i];
    const int KS = (K + 15) >> 4;
    const int lane = t & 63;
    const int f = t >> 6;                      // ct * KS + ks
    const int ct = f / KS, ks = f - ct * KS;
    const int n = 32 * ct + (lane & 31);
    const int k0 = 16 * ks + 8 * (lane >> 5);
    float x[8];
    if (T.mode[i] == 0 && n < N && k0 + 8 <= K && (ld & 3) == 0) {
        // eight consecutive k of one stored row: two 16-byte loads (rows are 16-byte aligned: checked by the launcher)
        const float* rp = (n < n1) ? T.w1[i] + (int64_t)n * ld + k0 : T.w2[i] + (int64_t)(n - n1) * ld + k0;
        const float4 a = *reinterpret_cast<const float4*>(rp), b = *reinterpret_cast<const float4*>(rp + 4);
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = cut_element(T, i, n, k0 + j);      // (transposed modes: lanes walk a stored row)
    }
    u32x4 p1, p2, p3;
    cut8_pairs(x, BF16_HI, p1, p2, p3);
    u32x4* dst = T.planes[i] + (int64_t)f * 3 * 64 + lane;
    dst[0] = p1;
    dst[64] = p2;
    dst[128] = p3;
}

// Party-ordered store (PARTY instances of the body below): the problem's rows are the utterances (t, b) of speaker-encoded modality
// m, row t B + b; instead of Y the result row goes to S[rank(t, b, p), (m B + b) P + p, :] for every speaker p flagged in
// qmask[t, b, :] -- the layout the party GRU reads (encoder_glue.hip, party_gather_kernel, whose launch this replaces) -- where
// rank(t, b, p) = the number of t' < t with qmask[t', b, p] != 0.
struct PlParty {
    const float* qmask;            // (L, B, P)
    float* S;                      // (L, Mn B P, N)
    int B, P, Mn, m;
};
constexpr int PL_MAXP = 16;        // speakers per dialogue the party-ordered store covers (ranks of a row block: 64 x 16 ints of LDS)

// RH = row halves per wave: 2 -> wave = 64 rows x one 32-column tile, workgroup = 64 x 128 (many column tiles: the forward
// products, N = 600); 1 -> wave = 32 rows x one tile, workgroup = 64 x 64 (few column tiles: the input gradients, N = 200 --
// twice the workgroups, half the MFMA chain per wave).  A = the X rows: every wave cuts ONE (row half, k-step) task per phase.
// one workgroup's share of Y = act(X B^T + bias) (+ Y); `bid`: the workgroup's number inside ITS problem's block range
// INMASK: the X rows pass through a dropout first -- xmask (R x K keep flags, contiguous) is fetched with the x values and the
// staging step cuts (x * keep) * xscale, the expression of mask_scale_kernel; the workgroups of column block 0 also write the
// dropped rows to xdrop (R x K, contiguous; may be null): the layer's weight gradients contract them.
// PARTY: see PlParty; rk: 64 x PL_MAXP ints of LDS.  Every workgroup derives the ranks of its own 64 rows: the flags of all
// utterances up to its last row are staged as bytes in As (before the main loop uses it), then one thread per (row, speaker)
// counts the earlier flags of that speaker.
template <int RH, bool INMASK = false, bool PARTY = false>
__device__ __forceinline__ void linear_planes_body(
    u32x4* As, const float* __restrict__ X, const u32x4* __restrict__ planes, const float* __restrict__ bias,
    const float* __restrict__ bias2, int n1, float* __restrict__ Y, int R, int K, int N, int ldx, int ldy, int act,
    int accumulate, int nrb, int ncb, int bid, const float* __restrict__ mask = nullptr, float mscale = 1.0f,
    const float* __restrict__ xmask = nullptr, float* __restrict__ xdrop = nullptr, float xscale = 1.0f,
    int* rk = nullptr, const PlParty pt = PlParty{nullptr, nullptr, 1, 1, 1, 0}) {
    constexpr int TPW = 4 / (3 - RH);                   // column tiles per workgroup: RH = 2 -> 4, RH = 1 -> 2
    constexpr int NACC = (RH == 2) ? 1 : 2;
    int rb, cb;
    if (!pl_decode(nrb, ncb, rb, cb, bid)) return;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const int KS = (K + 15) >> 4;
    const int NPH = (KS + PL_STG - 1) / PL_STG;
    const int NT = (N + 31) >> 5;
    const int ct = TPW * cb + (RH == 2 ? w : (w >> 1));
    const int myh = (RH == 2) ? 0 : (w & 1);
    const bool has_tile = ct < NT;                       // (a wave without a tile multiplies tile 0 and stores nothing)
    const int r0 = rb * PL_BM;

    if constexpr (PARTY) {
        unsigned char* fl = reinterpret_cast<unsigned char*>(As);      // (the launcher checked L B P <= the bytes of As)
        const int BP = pt.B * pt.P;
        const int rlast = (r0 + PL_BM - 1 < R) ? r0 + PL_BM - 1 : R - 1;
        const int nflag = (rlast / pt.B + 1) * BP;
        for (int e = tid; e < nflag; e += 256) fl[e] = pt.qmask[e] != 0.f ? 1 : 0;
        __syncthreads();
        for (int task = tid; task < PL_BM * pt.P; task += 256) {
            const int j = task / pt.P, p = task - j * pt.P;
            const int r = r0 + j;
            int k = -1;
            if (r < R) {
                const int t = r / pt.B, b = r - t * pt.B;
                const unsigned char* f = fl + b * pt.P + p;
                int c = 0;
                for (int tt = 0; tt < t; ++tt) c += f[tt * BP];
                k = f[t * BP] ? c : -1;
            }
            rk[task] = k;
        }
        __syncthreads();                                               // (As is free for the main loop; rk stays)
    }

    f32x16 acc[RH][NACC];
#pragma unroll
    for (int h = 0; h < RH; ++h)
#pragma unroll
        for (int c = 0; c < NACC; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[h][c][r] = 0.f;

    const u32x4* bsrc = planes + ((int64_t)(has_tile ? ct : 0) * KS) * 3 * 64 + lane;
    f32x4 raw[2][2];                                     // [phase parity][float4 of the 8 k values]
    // staging task of this wave in every phase: row half w & 1, k-step w >> 1; lane -> (row of the half, k group)
    const int shf = w & 1, sksl = w >> 1;
    const int srow = r0 + 32 * shf + (lane & 31);
    const float* xrow = X + (int64_t)(srow < R ? srow : R - 1) * ldx;
    const int skofs = 16 * sksl + 8 * (lane >> 5);       // k of this lane's first value inside the phase
    f32x4 mraw[INMASK ? 2 : 1][2];                       // the keep flags of raw[][]
    const float* mrow = INMASK ? xmask + (int64_t)(srow < R ? srow : R - 1) * K : nullptr;
    float* drow = (INMASK && xdrop && cb == 0 && srow < R) ? xdrop + (int64_t)srow * K : nullptr;

#define PL_ISSUE_X(PAR, PH)                                                                                 \
    do {                                                                                                    \
        const int k0_ = 16 * PL_STG * (PH) + skofs;                                                         \
        raw[PAR][0] = *reinterpret_cast<const f32x4*>(xrow + (k0_ < K ? k0_ : 0));                          \
        raw[PAR][1] = *reinterpret_cast<const f32x4*>(xrow + (k0_ + 4 < K ? k0_ + 4 : 0));                  \
        if constexpr (INMASK) {                                                                             \
            mraw[PAR][0] = *reinterpret_cast<const f32x4*>(mrow + (k0_ < K ? k0_ : 0));                     \
            mraw[PAR][1] = *reinterpret_cast<const f32x4*>(mrow + (k0_ + 4 < K ? k0_ + 4 : 0));             \
        }                                                                                                   \
    } while (0)
#define PL_PARK(PAR, PH, BUF)                                                                               \
    do {                                                                                                    \
        const int k0_ = 16 * PL_STG * (PH) + skofs;                                                         \
        const bool ok0_ = k0_ < K, ok1_ = k0_ + 4 < K;       /* (K % 4 == 0: a float4 below K is inside the row) */ \
        float x_[8] = {ok0_ ? raw[PAR][0].x : 0.f, ok0_ ? raw[PAR][0].y : 0.f, ok0_ ? raw[PAR][0].z : 0.f, ok0_ ? raw[PAR][0].w : 0.f, \
                       ok1_ ? raw[PAR][1].x : 0.f, ok1_ ? raw[PAR][1].y : 0.f, ok1_ ? raw[PAR][1].z : 0.f, ok1_ ? raw[PAR][1].w : 0.f}; \
        if constexpr (INMASK) {                                                                             \
            _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) {                                              \
                x_[j_] = ok0_ ? x_[j_] * mraw[PAR][0][j_] * xscale : 0.f;                                   \
                x_[4 + j_] = ok1_ ? x_[4 + j_] * mraw[PAR][1][j_] * xscale : 0.f;                           \
            }                                                                                               \
            if (drow) {                                                                                     \
                if (ok0_) *reinterpret_cast<f32x4*>(drow + k0_) = f32x4{x_[0], x_[1], x_[2], x_[3]};        \
                if (ok1_) *reinterpret_cast<f32x4*>(drow + k0_ + 4) = f32x4{x_[4], x_[5], x_[6], x_[7]};    \
            }                                                                                               \
        }                                                                                                   \
        u32x4 p1_, p2_, p3_;                                                                                \
        cut8_pairs(x_, BF16_HI, p1_, p2_, p3_);                                                             \
        u32x4* dst_ = &As[(BUF) * (PL_LDS / 2) + ((sksl * 3) * 2 + shf) * 64 + lane];                       \
        dst_[0] = p1_;                                                                                      \
        dst_[2 * 64] = p2_;                                                                                 \
        dst_[4 * 64] = p3_;                                                                                 \
    } while (0)
#include "planes_pipeline.h"
#undef PL_PARK
#undef PL_ISSUE_X

    if (!has_tile) return;
    // ---- epilogue straight from the accumulators: C layout col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int col = 32 * ct + (lane & 31);
    if (col >= N) return;
    float bv = 0.f;
    if (col < n1) { if (bias) bv = bias[col]; }
    else if (bias2) bv = bias2[col - n1];
    if constexpr (PARTY) {
        // row (t, b) goes to every flagged speaker's party row; proj + bias is the one fp32 add of gather(proj) + bias
        const int64_t cols = (int64_t)pt.Mn * pt.B * pt.P;
#pragma unroll
        for (int h = 0; h < RH; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = 32 * (RH == 2 ? h : myh) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int row = r0 + j;
                if (row < R) {
                    const int b = row % pt.B;
                    const float v = (NACC == 2 ? acc[h][0][r] + acc[h][NACC - 1][r] : acc[h][0][r]) + bv;
                    float* sp = pt.S + (((int64_t)pt.m * pt.B + b) * pt.P) * N + col;
                    for (int p = 0; p < pt.P; ++p) {
                        const int k = rk[j * pt.P + p];
                        if (k >= 0) sp[((int64_t)k * cols + p) * N] = v;
                    }
                }
            }
        return;
    }
    // keep flags of a folded dropout: requested for all the rows first (a load inside the store loop waits a round trip per row)
    float mv[RH][16];
#pragma unroll
    for (int h = 0; h < RH; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = r0 + 32 * (RH == 2 ? h : myh) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            mv[h][r] = 1.0f;
            if (mask) mv[h][r] = mask[(int64_t)(row < R ? row : R - 1) * N + col] * mscale;
        }
#pragma unroll
    for (int h = 0; h < RH; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = r0 + 32 * (RH == 2 ? h : myh) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (row < R) {
                float* yp = Y + (int64_t)row * ldy + col;
                float v = (NACC == 2 ? acc[h][0][r] + acc[h][NACC - 1][r] : acc[h][0][r]) + bv;
                if (act == 1) v = v > 0.f ? v : 0.f;
                v *= mv[h][r];
                if (accumulate) v += *yp;
                *yp = v;
            }
        }
}

template <int RH>
__global__ __launch_bounds__(256, 4) void linear_planes_kernel(
    const float* __restrict__ X, const u32x4* __restrict__ planes, const float* __restrict__ bias,
    const float* __restrict__ bias2, int n1, float* __restrict__ Y, int R, int K, int N, int ldx, int ldy, int act,
    int accumulate, int nrb, int ncb) {
    __shared__ u32x4 As[PL_LDS];
    linear_planes_body<RH>(As, X, planes, bias, bias2, n1, Y, R, K, N, ldx, ldy, act, accumulate, nrb, ncb, (int)blockIdx.x);
}

// Several independent projections in ONE launch (the context and the party encoder's input contractions of a GRU layer, their
// input gradients): problem p owns the blocks [blk0[p], blk0[p + 1]) and keeps the tile form it would take alone.
constexpr int PL_MAXG = 4;
struct PlGroup {
    const float* X[PL_MAXG];
    const u32x4* planes[PL_MAXG];
    const float* bias[PL_MAXG];
    const float* bias2[PL_MAXG];
    float* Y[PL_MAXG];
    const float* mask[PL_MAXG];
    const float* xmask[PL_MAXG];   // keep flags of a dropout on the X rows (null: none), the dropped rows' copy (may be null)
    float* xdrop[PL_MAXG];
    int party[PL_MAXG];            // modality index of a problem with the party-ordered store (-1: none)
    // party-ordered store: behind the problems' blocks, B P fill_ny blocks write `rank` and the bias into the padding rows of S
    const float* qmask;
    float* S;
    int32_t* rank;
    int L, B, P, Mn, fill_ny, fill_i;      // fill_i: a party problem (bias, bias2, n1, N of the fill rows)
    int n1[PL_MAXG], R[PL_MAXG], K[PL_MAXG], N[PL_MAXG], ldx[PL_MAXG], ldy[PL_MAXG], nrb[PL_MAXG], ncb[PL_MAXG], rh[PL_MAXG];
    int blk0[PL_MAXG + 1];
    int n;
};

// fill block fb = (b P + p) + B P y of a launch with party problems: the ballot / popcount scan over qmask[:, b, p] gives the ranks
// (written by the y = 0 blocks) and the party's count; rows k >= count of S[k, (m, b, p), :] in the block's row range receive the
// bias (0 + bias: the bits party_gather_kernel writes there).  They are rows no projection workgroup writes.
__device__ __forceinline__ void party_fill_body(int* sh, const PlGroup& G, int fb) {
    const int L = G.L, B = G.B, P = G.P, Mn = G.Mn;
    const int BP = B * P;
    const int y = fb / BP, bp = fb - y * BP;
    const int b = bp / P, p = bp - b * P;
    const int tid = threadIdx.x;
    if (tid < 64) {
        int base = 0;
        for (int t0 = 0; t0 < L; t0 += 64) {
            const int t = t0 + tid;
            const bool f = (t < L) && (G.qmask[((int64_t)t * B + b) * P + p] != 0.f);
            const unsigned long long bal = __ballot(f);
            const int pre = __popcll(bal & ((1ull << tid) - 1ull));
            if (t < L && y == 0) G.rank[((int64_t)t * B + b) * P + p] = f ? base + pre : -1;
            base += __popcll(bal);
        }
        if (tid == 0) sh[0] = base;
    }
    __syncthreads();
    const int cnt = sh[0];
    const int i = G.fill_i;
    const int N = G.N[i], n1 = G.n1[i];
    const float* bias = G.bias[i];
    const float* bias2 = G.bias2[i];
    const int N4 = N >> 2;
    const int64_t cols = (int64_t)Mn * BP;
    const int kper = (L + G.fill_ny - 1) / G.fill_ny;
    const int k_lo = y * kper;
    const int k_hi = (k_lo + kper < L) ? k_lo + kper : L;
    const int k0 = cnt > k_lo ? cnt : k_lo;
    if (k0 >= k_hi) return;
    for (int j = tid; j < Mn * N4; j += 256) {
        const int m = j / N4;
        const int col = 4 * (j - m * N4);
        float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < n1) { if (bias) bb = make_float4(bias[col], bias[col + 1], bias[col + 2], bias[col + 3]); }
        else if (bias2) bb = make_float4(bias2[col - n1], bias2[col - n1 + 1], bias2[col - n1 + 2], bias2[col - n1 + 3]);
        const float4 v = make_float4(0.f + bb.x, 0.f + bb.y, 0.f + bb.z, 0.f + bb.w);
        float* sm = G.S + (((int64_t)m * B + b) * P + p) * N + col;
        for (int k = k0; k < k_hi; ++k) *reinterpret_cast<float4*>(sm + (int64_t)k * cols * N) = v;
    }
}

__global__ __launch_bounds__(256, 4) void linear_planes_group_kernel(PlGroup G, int act, int accumulate, float mscale, float xscale) {
    __shared__ u32x4 As[PL_LDS];
    __shared__ int rk[PL_BM * PL_MAXP];
    if ((int)blockIdx.x >= G.blk0[G.n]) {                  // (only a launch with party problems has such blocks)
        party_fill_body(rk, G, (int)blockIdx.x - G.blk0[G.n]);
        return;
    }
    int p = 0;
    while (p + 1 < G.n && (int)blockIdx.x >= G.blk0[p + 1]) ++p;
    const int bid = (int)blockIdx.x - G.blk0[p];
#define PL_GROUP_BODY(RH_, IN_, PT_, ...)                                                                                 \
    linear_planes_body<RH_, IN_, PT_>(As, G.X[p], G.planes[p], G.bias[p], G.bias2[p], G.n1[p], G.Y[p], G.R[p], G.K[p], G.N[p], \
                                      G.ldx[p], G.ldy[p], act, accumulate, G.nrb[p], G.ncb[p], bid, G.mask[p], mscale,   \
                                      G.xmask[p], G.xdrop[p], xscale, ##__VA_ARGS__)
    // (a problem without an option runs the plain instance: the tile form and the bits of its own launch)
    if (G.party[p] >= 0) {
        const PlParty pt{G.qmask, G.S, G.B, G.P, G.Mn, G.party[p]};
        if (G.rh[p] == 2) PL_GROUP_BODY(2, false, true, rk, pt);
        else PL_GROUP_BODY(1, false, true, rk, pt);
    } else if (G.xmask[p]) {
        if (G.rh[p] == 2) PL_GROUP_BODY(2, true, false);
        else PL_GROUP_BODY(1, true, false);
    } else {
        if (G.rh[p] == 2) PL_GROUP_BODY(2, false, false);
        else PL_GROUP_BODY(1, false, false);
    }
#undef PL_GROUP_BODY
}

// tile form of one problem: few column tiles (an input gradient, N = 200) or few rows -> 64 x 64 workgroups, so that the launch
// has workgroups for every CU
inline void pl_form(int R, int N, int* nrb, int* ncb, int* rh) {
    *nrb = (R + PL_BM - 1) / PL_BM;
    const int NT = (N + 31) / 32;
    const bool narrow = (int64_t)*nrb * ((NT + 3) / 4) < 400;
    *ncb = narrow ? (NT + 1) / 2 : (NT + 3) / 4;
    *rh = narrow ? 1 : 2;
}

}  // namespace

extern "C" {

int64_t mmdfn_weight_planes_workspace(int N, int K) {
    if (N <= 0 || K <= 0) return -1;
    const int64_t NT = (N + 31) / 32, KS = (K + 15) / 16;
    return NT * KS * 3 * 64 * 16;                 // bytes
}

int mmdfn_cut_weight_planes(int n, const float* const* w1, const float* const* w2, const int* n1, const int* ld,
                            const int* N, const int* K, const int* mode, void* const* planes, void* stream) {
    if (n <= 0 || n > PL_MAXW) return -1;
    CutTable T;
    T.n = n;
    T.prefix[0] = 0;
    for (int i = 0; i < n; ++i) {
        if (!w1[i] || !planes[i] || N[i] <= 0 || K[i] <= 0 || mode[i] < 0 || mode[i] > 3) return -1;
        if ((reinterpret_cast<uintptr_t>(planes[i]) & 15) != 0) return -1;
        if ((ld[i] & 3) == 0 && ((reinterpret_cast<uintptr_t>(w1[i]) & 15) || (w2[i] && (reinterpret_cast<uintptr_t>(w2[i]) & 15))))
            return -1;                             // (16-byte rows are fetched with 16-byte loads)
        // the index that is split at n1: stored rows (modes 0, 1) or output columns (modes 2, 3)
        const int split_extent = mode[i] == 0 ? N[i] : mode[i] == 1 ? K[i] : N[i];
        if (n1[i] < split_extent && !w2[i]) return -1;
        if (mode[i] == 3 && (K[i] & 3)) return -1;
        T.w1[i] = w1[i];
        T.w2[i] = w2[i];
        T.planes[i] = reinterpret_cast<u32x4*>(planes[i]);
        T.n1[i] = n1[i];
        T.ld[i] = ld[i];
        T.N[i] = N[i];
        T.K[i] = K[i];
        T.mode[i] = mode[i];
        const int64_t tasks = (int64_t)((N[i] + 31) / 32) * ((K[i] + 15) / 16) * 64;
        if (T.prefix[i] + tasks > (1ll << 30)) return -1;
        T.prefix[i + 1] = T.prefix[i] + (int)tasks;
    }
    hipLaunchKernelGGL(cut_planes_kernel, dim3((T.prefix[n] + 255) / 256), dim3(256), 0, (hipStream_t)stream, T);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

int mmdfn_linear_planes(const float* X, const void* planes, const float* bias, const float* bias2, int n1, float* Y, int R,
                        int K, int N, int ldx, int ldy, int act, int accumulate, void* stream) {
    if (R <= 0) return 0;
    if (!X || !planes || !Y || K < 4 || (K & 3) || N <= 0 || (ldx & 3) || ldx < K || ldy < N) return -1;
    if ((reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(planes) & 15)) return -1;
    int nrb, ncb, rh;
    pl_form(R, N, &nrb, &ncb, &rh);
    const bool narrow = rh == 1;
    const int64_t grid = pl_grid(nrb, ncb);
    if (grid > (1ll << 30)) return -1;
    if (narrow)
        hipLaunchKernelGGL(linear_planes_kernel<1>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, X,
                           reinterpret_cast<const u32x4*>(planes), bias, bias2, n1, Y, R, K, N, ldx, ldy, act, accumulate, nrb, ncb);
    else
        hipLaunchKernelGGL(linear_planes_kernel<2>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, X,
                           reinterpret_cast<const u32x4*>(planes), bias, bias2, n1, Y, R, K, N, ldx, ldy, act, accumulate, nrb, ncb);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

int mmdfn_linear_planes_group_in(int n, const float* const* X, const void* const* planes, const float* const* bias,
                                 const float* const* bias2, const int* n1, float* const* Y, const int* R, const int* K,
                                 const int* N, const int* ldx, const int* ldy, int act, int accumulate,
                                 const float* const* mask, float mask_scale, const float* const* xmask,
                                 float* const* xdrop, float xscale, void* stream) {
    return mmdfn_linear_planes_group_party(n, X, planes, bias, bias2, n1, Y, R, K, N, ldx, ldy, act, accumulate, mask, mask_scale,
                                           xmask, xdrop, xscale, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, stream);
}

int mmdfn_linear_planes_group_party(int n, const float* const* X, const void* const* planes, const float* const* bias,
                                    const float* const* bias2, const int* n1, float* const* Y, const int* R, const int* K,
                                    const int* N, const int* ldx, const int* ldy, int act, int accumulate,
                                    const float* const* mask, float mask_scale, const float* const* xmask,
                                    float* const* xdrop, float xscale, const int* party, const float* qmask, float* S,
                                    int32_t* rank, int L, int B, int P, int Mn, void* stream) {
    const bool has_party = party != nullptr;
    if (has_party) {
        // shapes the party-ordered store covers (-2: the caller projects in utterance order and runs mmdfn_party_gather)
        if (!qmask || !S || !rank || L <= 0 || B <= 0 || P <= 0 || Mn <= 0 || Mn > PL_MAXG) return -1;
        if (L > 2048 || P > PL_MAXP || (int64_t)L * B * P > (int64_t)PL_LDS * 16) return -2;
        if (act != 0 || accumulate != 0) return -1;
    }
    if (n <= 0 || n > PL_MAXG) return -1;
    PlGroup G;
    G.n = 0;
    G.blk0[0] = 0;
    for (int i = 0; i < n; ++i) {
        if (R[i] <= 0) continue;                   // (an empty problem takes no blocks)
        const int pm = has_party ? party[i] : -1;
        if (pm >= 0) {
            if (pm >= Mn || R[i] != L * B || (N[i] & 3) || (n1[i] & 3) || (mask && mask[i]) || (xmask && xmask[i])) return -1;
            if (G.n > 0 && G.party[0] >= 0 && (N[i] != G.N[0] || n1[i] != G.n1[0])) return -1;   // (party problems come first)
            if (G.n > 0 && G.party[G.n - 1] < 0) return -1;
        }
        if (!X[i] || !planes[i] || (!Y[i] && pm < 0) || K[i] < 4 || (K[i] & 3) || N[i] <= 0 || (ldx[i] & 3) || ldx[i] < K[i] || (ldy[i] < N[i] && pm < 0))
            return -1;
        if ((reinterpret_cast<uintptr_t>(X[i]) & 15) || (reinterpret_cast<uintptr_t>(planes[i]) & 15)) return -1;
        const int p = G.n++;
        G.party[p] = pm;
        G.X[p] = X[i];
        G.planes[p] = reinterpret_cast<const u32x4*>(planes[i]);
        G.bias[p] = bias ? bias[i] : nullptr;
        G.bias2[p] = bias2 ? bias2[i] : nullptr;
        G.Y[p] = Y[i];
        G.mask[p] = mask ? mask[i] : nullptr;
        G.xmask[p] = xmask ? xmask[i] : nullptr;
        G.xdrop[p] = (xdrop && G.xmask[p]) ? xdrop[i] : nullptr;
        if ((reinterpret_cast<uintptr_t>(G.xmask[p]) & 15) || (reinterpret_cast<uintptr_t>(G.xdrop[p]) & 15)) return -1;
        G.n1[p] = n1[i]; G.R[p] = R[i]; G.K[p] = K[i]; G.N[p] = N[i]; G.ldx[p] = ldx[i]; G.ldy[p] = ldy[i];
        pl_form(R[i], N[i], &G.nrb[p], &G.ncb[p], &G.rh[p]);
        const int64_t blocks = pl_grid(G.nrb[p], G.ncb[p]);
        if (G.blk0[p] + blocks > (1ll << 30)) return -1;
        G.blk0[p + 1] = G.blk0[p] + (int)blocks;
    }
    if (G.n == 0) return 0;
    for (int p = G.n; p < PL_MAXG; ++p) {
        G.X[p] = nullptr; G.planes[p] = nullptr; G.bias[p] = G.bias2[p] = nullptr; G.Y[p] = nullptr; G.mask[p] = nullptr;
        G.xmask[p] = nullptr; G.xdrop[p] = nullptr; G.party[p] = -1;
        G.n1[p] = G.R[p] = G.K[p] = G.N[p] = G.ldx[p] = G.ldy[p] = G.nrb[p] = G.ncb[p] = G.rh[p] = 0;
        G.blk0[p + 1] = G.blk0[G.n];
    }
    G.qmask = nullptr; G.S = nullptr; G.rank = nullptr;
    G.L = G.B = G.P = G.Mn = G.fill_ny = G.fill_i = 0;
    int64_t grid = G.blk0[G.n];
    if (has_party && G.party[0] >= 0) {
        int np = 0;
        while (np < G.n && G.party[np] >= 0) ++np;
        if (np != Mn) return -1;                   // every modality's rows of S are written by this launch
        for (int a = 0; a < np; ++a)
            for (int c = a + 1; c < np; ++c)
                if (G.party[a] == G.party[c]) return -1;
        G.qmask = qmask; G.S = S; G.rank = rank;
        G.L = L; G.B = B; G.P = P; G.Mn = Mn; G.fill_i = 0;
        int ny = 1024 / (B * P);                   // the fill blocks' row ranges (as mmdfn_party_gather's)
        if (ny > (L + 7) / 8) ny = (L + 7) / 8;
        if (ny < 1) ny = 1;
        G.fill_ny = ny;
        grid += (int64_t)B * P * ny;
        if (grid > (1ll << 30)) return -1;
    } else if (has_party) {
        return -1;
    }
    hipLaunchKernelGGL(linear_planes_group_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, G, act,
                       accumulate, mask_scale, xscale);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

int mmdfn_linear_planes_group(int n, const float* const* X, const void* const* planes, const float* const* bias,
                              const float* const* bias2, const int* n1, float* const* Y, const int* R, const int* K,
                              const int* N, const int* ldx, const int* ldy, int act, int accumulate,
                              const float* const* mask, float mask_scale, void* stream) {
    return mmdfn_linear_planes_group_in(n, X, planes, bias, bias2, n1, Y, R, K, N, ldx, ldy, act, accumulate, mask, mask_scale,
                                        nullptr, nullptr, 1.0f, stream);
}

}  // extern "C"
