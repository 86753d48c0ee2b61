// K18  fused embedding -> Conv1d (n_k kernel sizes) -> ReLU -> max over time, the text front end of the reference's
// CNNFeatureExtractor (model.py:1410-1443), forward and backward.  DESIGN 4ac.
//
// Forward (cnn_pool_fwd_kernel).  One workgroup (4 waves) owns CNN_RG = 1 utterance row and walks its words in tiles of CNN_TW
// = 32 window starts.  Per tile the TW + max K - 1 embedding rows are gathered from the table by token id (clamped into [0, V)),
// cut into the three bf16 pieces of bf16_pieces.h and staged in LDS -- the only copy of the embedded text that ever exists.  The
// convolution of size K is the sum over its K taps of (positions x D) . (D x F) products against the SAME staged rows shifted by
// the tap, so the A operand of v_mfma_f32_16x16x32_bf16 for tap k is read at row (position + k): lane l holds
// A[row l & 15][c = 8 (l >> 4) + 0..7].  The B operand (all taps of all sizes, (D) x (sum K_i F)) is cut ONCE PER LAUNCH into
// fragment planes by cnn_cut_kernel and streamed from L2, one coalesced 16 bytes per lane and piece:
//   planes[(poff_i + ((k ndc + dc) nft + ft) 3 + piece) 64 + lane] = piece of W_i[f = 16 ft + (lane & 15)][c = 32 dc + 8 (lane >> 4) + 0..7][k]
// (zero for f >= F or c >= D; ndc = ceil(D / 32), nft = ceil(F / 16)).  A wave owns the (size, filter tile) pairs = its number
// mod 4 and keeps two accumulators (the two 16-position halves of the tile) per pair; the epilogue adds the bias, applies the
// ReLU and folds the tile into the running (max, lowest argmax) of its columns in LDS.  Nothing of size rows W D or rows W F is
// written to global memory.
//
// Backward.  The gradient is sparse: one window per (row, size, filter) with a positive maximum.
//   cnn_wgrad_kernel       dW_i[f, c, k] = sum_r g E[tok[r, t* + k], c],  db_i[f] = sum_r g: one workgroup per (f, k, i), a lane
//                          per (row slice, c): contiguous row slices summed in ascending order, then the slices in order.
//   cnn_table_keys_kernel  key of entry (r, column, k) = the token the window's tap k touched (V for a dead entry); the caller
//                          sorts the keys (stable), which orders every token's entries by (r, column, k);
//   cnn_table_bounds_kernel  the segment of every token in the sorted keys;
//   cnn_table_bwd_kernel   one workgroup per token:
//                          dEmb[v, c] = sum over its segment, in sorted order, of g W_i[f, c, k].  No float atomics: two runs give
//                          the same bits.  Tokens without entries get zeros (the kernel writes the whole gradient).
// Every loop is bounded by a dimension; no workgroup waits for another.
#include "bf16_pieces.h"
#include "../../include/mmdfn_hip.h"

namespace {

constexpr int CNN_TW = 32;          // window starts per tile
constexpr int CNN_RG = 1;           // utterance rows per workgroup
constexpr int CNN_NT = 256;         // threads of the forward workgroup
constexpr int CNN_MAXSIZES = 4;
constexpr int CNN_MAXK = 8;
constexpr int CNN_MAXF = 64;
constexpr int CNN_MAXD = 304;
constexpr int CNN_MAXW = 512;
constexpr int CNN_MAXCOLS = CNN_MAXSIZES * CNN_MAXF;

struct CnnSizes {
    const float* w[CNN_MAXSIZES];
    const float* b[CNN_MAXSIZES];
    float* dw[CNN_MAXSIZES];
    float* db[CNN_MAXSIZES];
    int K[CNN_MAXSIZES];
    int poff[CNN_MAXSIZES + 1];     // first fragment group (of 3 x 64 u32x4) of a size's planes; [n] = their total
    int n, maxk, mink;
};

__host__ __device__ inline int cnn_ndc(int D) { return (D + 31) / 32; }
__host__ __device__ inline int cnn_nft(int F) { return (F + 15) / 16; }
// dwords per staged row of one piece: D padded to 32, two bf16 per dword, + 4 so that the 16 rows of a ds_read_b128 fragment
// read start in 16 different 4-bank groups
__host__ __device__ inline int cnn_row_dwords(int D) { return cnn_ndc(D) * 16 + 4; }

__device__ __forceinline__ int64_t cnn_clamp_id(int64_t id, int V) { return id < 0 ? 0 : (id >= V ? (int64_t)V - 1 : id); }

bool cnn_fill(CnnSizes& S, const float* const* w, const float* const* b, float* const* dw, float* const* db, int D, int F,
              int n_k, const int32_t* ks) {
    S = CnnSizes();
    if (n_k < 1 || n_k > CNN_MAXSIZES || ks == nullptr) return false;
    if (D < 4 || D > CNN_MAXD || D % 4 || F < 1 || F > CNN_MAXF) return false;
    S.n = n_k;
    S.mink = CNN_MAXK;
    int off = 0;
    for (int i = 0; i < n_k; ++i) {
        if (ks[i] < 1 || ks[i] > CNN_MAXK) return false;
        S.K[i] = ks[i];
        S.maxk = ks[i] > S.maxk ? ks[i] : S.maxk;
        S.mink = ks[i] < S.mink ? ks[i] : S.mink;
        S.poff[i] = off;
        off += ks[i] * cnn_ndc(D) * cnn_nft(F);
        if (w) { if (w[i] == nullptr) return false; S.w[i] = w[i]; }
        if (b) { if (b[i] == nullptr) return false; S.b[i] = b[i]; }
        if (dw) { if (dw[i] == nullptr) return false; S.dw[i] = dw[i]; }
        if (db) { if (db[i] == nullptr) return false; S.db[i] = db[i]; }
    }
    for (int i = n_k; i <= CNN_MAXSIZES; ++i) S.poff[i] = off;
    return true;
}

// ---- the weight cut: one thread per (fragment group, lane) -----------------------------------------------------------------
__global__ void cnn_cut_kernel(CnnSizes S, u32x4* __restrict__ planes, int D, int F) {
    const int ndc = cnn_ndc(D), nft = cnn_nft(F);
    const int gidx = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (gidx >= S.poff[S.n]) return;
    int i = 0;
#pragma unroll
    for (int j = 1; j < CNN_MAXSIZES; ++j)
        if (j < S.n && gidx >= S.poff[j]) i = j;
    const int K = S.K[i];
    int rem = gidx - S.poff[i];
    const int ft = rem % nft; rem /= nft;
    const int dc = rem % ndc;
    const int k = rem / ndc;
    const int f = 16 * ft + (lane & 15), c0 = 32 * dc + 8 * (lane >> 4);
    const float* w = S.w[i];
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (f < F && c0 + e < D) ? w[((int64_t)f * D + c0 + e) * K + k] : 0.f;
    u32x4 p1, p2, p3;
    cut8(v, BF16_HI, p1, p2, p3);
    u32x4* dst = planes + (int64_t)gidx * 3 * 64 + lane;
    dst[0] = p1; dst[64] = p2; dst[128] = p3;
}

// ---- forward -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CNN_NT) void cnn_pool_fwd_kernel(const int64_t* __restrict__ tokens, const float* __restrict__ table,
                                                              CnnSizes S, const float* __restrict__ row_mask,
                                                              const u32x4* __restrict__ planes, float* __restrict__ pooled,
                                                              int32_t* __restrict__ argmax, int W, int V, int D, int F) {
    extern __shared__ uint32_t smem[];                  // [piece][staged row][row dwords]
    __shared__ float runmax[CNN_MAXCOLS];
    __shared__ int runarg[CNN_MAXCOLS];
    __shared__ int64_t toks[CNN_TW + CNN_MAXK];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int NC = S.n * F;
    if (row_mask[r] == 0.f) {                           // (uniform over the workgroup) a masked row: zeros, no window
        for (int c = tid; c < NC; c += CNN_NT) { pooled[r * NC + c] = 0.f; argmax[r * NC + c] = -1; }
        return;
    }
    for (int c = tid; c < CNN_MAXCOLS; c += CNN_NT) { runmax[c] = 0.f; runarg[c] = -1; }
    const int ndc = cnn_ndc(D), nft = cnn_nft(F), rowdw = cnn_row_dwords(D);
    const int nrows = CNN_TW + S.maxk - 1;              // staged rows of a tile: its window starts + the halo
    const int piece_stride = nrows * rowdw;
    const int ntask = S.n * nft;
    const int q4 = ndc * 8;                             // float4 groups of a padded row
    for (int t0 = 0; t0 + S.mink <= W; t0 += CNN_TW) {      // tiles in which a window of the smallest size still starts
        __syncthreads();                                // the previous tile's fragment reads are done; runmax init is visible
        if (tid < nrows) {
            const int pos = t0 + tid;
            toks[tid] = pos < W ? cnn_clamp_id(tokens[r * W + pos], V) : -1;
        }
        __syncthreads();
        for (int idx = tid; idx < nrows * q4; idx += CNN_NT) {
            const int j = idx / q4, c4 = idx - j * q4;
            const int64_t tok = toks[j];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (tok >= 0 && 4 * c4 < D) v = ld4(table + tok * D + 4 * c4);
            u32x2 p1, p2, p3;
            cut4(v.x, v.y, v.z, v.w, BF16_HI, p1, p2, p3);
            uint32_t* dst = smem + j * rowdw + 2 * c4;
            *reinterpret_cast<u32x2*>(dst) = p1;
            *reinterpret_cast<u32x2*>(dst + piece_stride) = p2;
            *reinterpret_cast<u32x2*>(dst + 2 * piece_stride) = p3;
        }
        __syncthreads();
        for (int task = wave; task < ntask; task += CNN_NT / 64) {
            const int i = task / nft, ft = task - i * nft;
            const int K = S.K[i];
            if (t0 + K > W) continue;                   // no window of this size starts in the tile
            f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            const u32x4* bp = planes + ((int64_t)S.poff[i] + ft) * 3 * 64 + lane;
            // steps = (tap k, channel chunk dc), k-major as the planes are laid out; the B fragments of step s + 1 are requested
            // before the MFMAs of step s (two workgroups of 77 KB fit a CU: two waves per SIMD do not hide an L2 round trip)
            const int nsteps = K * ndc;
            const int64_t bstep = (int64_t)nft * 3 * 64;
            u32x4 b[3] = {bp[0], bp[64], bp[128]};
            int k = 0, dc = 0;
            for (int st = 0; st < nsteps; ++st) {
                const u32x4* bq = bp + (st + 1 < nsteps ? st + 1 : st) * bstep;
                const u32x4 bn[3] = {bq[0], bq[64], bq[128]};
                const uint32_t* arow = smem + ((lane & 15) + k) * rowdw + 4 * (lane >> 4) + 16 * dc;
#pragma unroll
                for (int ms = 0; ms < 2; ++ms) {
                    const uint32_t* ap = arow + ms * 16 * rowdw;
                    const u32x4 a[3] = {*reinterpret_cast<const u32x4*>(ap), *reinterpret_cast<const u32x4*>(ap + piece_stride),
                                        *reinterpret_cast<const u32x4*>(ap + 2 * piece_stride)};
                    acc[ms] = six(a, b, acc[ms]);
                }
                b[0] = bn[0]; b[1] = bn[1]; b[2] = bn[2];
                if (++dc == ndc) { dc = 0; ++k; }
            }
            // epilogue: C element j of half ms is position t0 + 16 ms + 4 (lane >> 4) + j, filter 16 ft + (lane & 15)
            const int f = 16 * ft + (lane & 15);
            const float bias = f < F ? S.b[i][f] : 0.f;
            float best = 0.f;
            int bt = -1;
#pragma unroll
            for (int ms = 0; ms < 2; ++ms)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int t = t0 + 16 * ms + 4 * (lane >> 4) + j;
                    const float v = acc[ms][j] + bias;
                    if (t + K <= W && v > best) { best = v; bt = t; }      // ascending t, strict: the lowest t of a tie stays
                }
#pragma unroll
            for (int off = 16; off < 64; off <<= 1) {
                const float ob = __shfl_xor(best, off);
                const int ot = __shfl_xor(bt, off);
                if (ot >= 0 && (ob > best || (ob == best && ot < bt))) { best = ob; bt = ot; }
            }
            if (lane < 16 && f < F && bt >= 0 && best > runmax[i * F + f]) {   // earlier tiles hold lower t: strict again
                runmax[i * F + f] = best;
                runarg[i * F + f] = bt;
            }
        }
    }
    __syncthreads();
    for (int c = tid; c < NC; c += CNN_NT) { pooled[r * NC + c] = runmax[c]; argmax[r * NC + c] = runarg[c]; }
}

// ---- weight and bias gradients -----------------------------------------------------------------------------------------------
// CNN_WG_NT threads = nsl row slices x cw channel lanes (cw = D rounded up to whole waves): slice s sums its contiguous share of
// the rows in ascending order, four rows' dependent loads (argmax -> token -> table row) in flight at a time; the slices meet in
// LDS in ascending order.
constexpr int CNN_WG_NT = 1024;
__global__ __launch_bounds__(CNN_WG_NT) void cnn_wgrad_kernel(const float* __restrict__ dp, const int32_t* __restrict__ argmax,
                                                              const int64_t* __restrict__ tokens, const float* __restrict__ table,
                                                              CnnSizes S, int64_t rows, int W, int V, int D, int F) {
    __shared__ float part[CNN_WG_NT];
    __shared__ float bpart[CNN_WG_NT / 64];
    const int f = blockIdx.x, k = blockIdx.y, i = blockIdx.z;
    const int K = S.K[i];
    if (k >= K) return;                                 // (uniform over the workgroup)
    const int cw = 64 * ((D + 63) / 64), nsl = CNN_WG_NT / cw;
    const int sl = threadIdx.x / cw, c = threadIdx.x - sl * cw;
    const int NC = S.n * F, col = i * F + f;
    float acc = 0.f, bacc = 0.f;
    if (sl < nsl) {
        const int64_t chunk = (rows + nsl - 1) / nsl;
        const int64_t r0 = sl * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
        for (int64_t r = r0; r < r1; r += 4) {
            int t[4];
            float g[4];
            int64_t tok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = r + u < r1 ? argmax[(r + u) * NC + col] : -1;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (t[u] < 0 || t[u] + K > W) { t[u] = -1; g[u] = 0.f; tok[u] = 0; continue; }
                g[u] = dp[(r + u) * NC + col];
                tok[u] = cnn_clamp_id(tokens[(r + u) * W + t[u] + k], V);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (t[u] < 0) continue;                 // (uniform over the wave: a wave lies inside one slice)
                if (c < D) acc = fmaf(g[u], table[tok[u] * D + c], acc);
                bacc += g[u];
            }
        }
    }
    part[threadIdx.x] = acc;
    if (sl < nsl && c == 0) bpart[sl] = bacc;
    __syncthreads();
    if (sl == 0 && c < D) {
        float sum = part[c];
        for (int q = 1; q < nsl; ++q) sum += part[q * cw + c];
        S.dw[i][((int64_t)f * D + c) * K + k] = sum;
    }
    if (threadIdx.x == 0 && k == 0) {
        float sum = bpart[0];
        for (int q = 1; q < nsl; ++q) sum += bpart[q];
        S.db[i][f] = sum;
    }
}

// ---- table gradient ----------------------------------------------------------------------------------------------------------
__global__ void cnn_table_keys_kernel(const int32_t* __restrict__ argmax, const int64_t* __restrict__ tokens,
                                      int32_t* __restrict__ keys, CnnSizes S, int64_t n, int W, int V, int F) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int NC = S.n * F;
    const int k = (int)(e % S.maxk);
    const int64_t rc = e / S.maxk;
    const int col = (int)(rc % NC);
    const int64_t r = rc / NC;
    const int K = S.K[col / F];
    const int t = argmax[rc];
    int32_t key = V;
    if (k < K && t >= 0 && t + K <= W) key = (int32_t)cnn_clamp_id(tokens[r * W + t + k], V);
    keys[e] = key;
}

// bounds[v] = the first sorted position whose key is >= v, v = 0 .. V (token v's segment is [bounds[v], bounds[v + 1])): position s
// writes the entries (key[s - 1], key[s]], position n (key V) the rest, so every entry has exactly one writer.
__global__ void cnn_table_bounds_kernel(const int32_t* __restrict__ sorted_keys, int64_t* __restrict__ bounds, int64_t n, int V) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n) return;
    int key = V, prev = -1;
    if (s < n) { key = sorted_keys[s]; key = key < V ? key : V; }
    if (s > 0) { prev = sorted_keys[s - 1]; prev = prev < V ? prev : V; }
    for (int v = prev + 1; v <= key; ++v) bounds[v] = s;        // (at most V + 1 entries)
}

__global__ void cnn_table_bwd_kernel(const float* __restrict__ dp, const int64_t* __restrict__ bounds,
                                     const int64_t* __restrict__ order, CnnSizes S, float* __restrict__ dtable, int D, int F) {
    const int v = blockIdx.x, c = threadIdx.x;
    const int NC = S.n * F;
    const int64_t lo = bounds[v], hi = bounds[v + 1];
    float acc = 0.f;
    for (int64_t s = lo; s < hi; s += 4) {              // four entries' dependent loads in flight; summed in sorted order
        float g[4];
        const float* wp[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t e = order[s + u < hi ? s + u : hi - 1];
            const int k = (int)(e % S.maxk);
            const int64_t rc = e / S.maxk;
            const int col = (int)(rc % NC);
            const int i = col / F, f = col - i * F;
            g[u] = dp[rc];
            wp[u] = S.w[i] + ((int64_t)f * D + (c < D ? c : 0)) * S.K[i] + k;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (s + u < hi) acc = fmaf(g[u], *wp[u], acc);
    }
    if (c < D) dtable[(int64_t)v * D + c] = acc;
}

bool cnn_shape_ok(int64_t rows, int W, int V, const CnnSizes& S) {
    return rows >= 1 && rows <= 0x7fffffff && V >= 1 && W >= S.maxk && W <= CNN_MAXW;
}

}  // namespace

extern "C" int mmdfn_cnn_tile_words(void) { return CNN_TW; }
extern "C" int mmdfn_cnn_rows_per_group(void) { return CNN_RG; }

extern "C" int64_t mmdfn_cnn_planes_bytes(int D, int F, int n_k, const int32_t* ksizes) {
    CnnSizes S;
    if (!cnn_fill(S, nullptr, nullptr, nullptr, nullptr, D, F, n_k, ksizes)) return -1;
    return (int64_t)S.poff[S.n] * 3 * 64 * 16;
}

extern "C" int mmdfn_cnn_pool_fwd(const int64_t* tokens, const float* table, const float* const* conv_w,
                                  const float* const* conv_b, const float* row_mask, void* planes, float* pooled,
                                  int32_t* argmax, int64_t rows, int W, int V, int D, int F, int n_k, const int32_t* ksizes,
                                  void* stream) {
    CnnSizes S;
    if (tokens == nullptr || table == nullptr || conv_w == nullptr || conv_b == nullptr || row_mask == nullptr ||
        planes == nullptr || pooled == nullptr || argmax == nullptr)
        return -1;
    if (!cnn_fill(S, conv_w, conv_b, nullptr, nullptr, D, F, n_k, ksizes) || !cnn_shape_ok(rows, W, V, S)) return -1;
    const int groups = S.poff[S.n];
    hipLaunchKernelGGL(cnn_cut_kernel, dim3((groups + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, (u32x4*)planes, D, F);
    MMDFN_CHECK_LAUNCH();
    const size_t lds = (size_t)3 * (CNN_TW + S.maxk - 1) * cnn_row_dwords(D) * sizeof(uint32_t);
    if (lds > 48 * 1024) {
        const int rc = mmdfn_allow_big_lds(cnn_pool_fwd_kernel);
        if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(cnn_pool_fwd_kernel, dim3((unsigned)rows), dim3(CNN_NT), lds, (hipStream_t)stream, tokens, table, S,
                       row_mask, (const u32x4*)planes, pooled, argmax, W, V, D, F);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_cnn_pool_bwd(const float* d_pooled, const int32_t* argmax, const int64_t* tokens, const float* table,
                                  float* const* d_w, float* const* d_b, int64_t rows, int W, int V, int D, int F, int n_k,
                                  const int32_t* ksizes, void* stream) {
    CnnSizes S;
    if (d_pooled == nullptr || argmax == nullptr || tokens == nullptr || table == nullptr || d_w == nullptr || d_b == nullptr)
        return -1;
    if (!cnn_fill(S, nullptr, nullptr, d_w, d_b, D, F, n_k, ksizes) || !cnn_shape_ok(rows, W, V, S)) return -1;
    hipLaunchKernelGGL(cnn_wgrad_kernel, dim3(F, S.maxk, n_k), dim3(CNN_WG_NT), 0, (hipStream_t)stream, d_pooled, argmax, tokens,
                       table, S, rows, W, V, D, F);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t mmdfn_cnn_table_entries(int64_t rows, int F, int n_k, const int32_t* ksizes) {
    CnnSizes S;
    if (rows < 1 || !cnn_fill(S, nullptr, nullptr, nullptr, nullptr, 4, F, n_k, ksizes)) return -1;
    return rows * n_k * F * S.maxk;
}

extern "C" int mmdfn_cnn_table_keys(const int32_t* argmax, const int64_t* tokens, int32_t* keys, int64_t rows, int W, int V,
                                    int F, int n_k, const int32_t* ksizes, void* stream) {
    CnnSizes S;
    if (argmax == nullptr || tokens == nullptr || keys == nullptr) return -1;
    if (!cnn_fill(S, nullptr, nullptr, nullptr, nullptr, 4, F, n_k, ksizes) || !cnn_shape_ok(rows, W, V, S)) return -1;
    const int64_t n = rows * n_k * F * S.maxk;
    if ((n + 255) / 256 > 0x7fffffff) return -1;
    hipLaunchKernelGGL(cnn_table_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, argmax,
                       tokens, keys, S, n, W, V, F);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_cnn_table_bwd(const float* d_pooled, const int32_t* sorted_keys, const int64_t* order,
                                   const float* const* conv_w, int64_t* bounds, float* d_table, int64_t rows, int V, int D, int F,
                                   int n_k, const int32_t* ksizes, void* stream) {
    CnnSizes S;
    if (d_pooled == nullptr || sorted_keys == nullptr || order == nullptr || conv_w == nullptr || bounds == nullptr ||
        d_table == nullptr)
        return -1;
    if (rows < 1 || V < 1 || !cnn_fill(S, conv_w, nullptr, nullptr, nullptr, D, F, n_k, ksizes)) return -1;
    const int64_t n = rows * n_k * F * S.maxk;
    if ((n + 256) / 256 > 0x7fffffff) return -1;
    hipLaunchKernelGGL(cnn_table_bounds_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, (hipStream_t)stream, sorted_keys,
                       bounds, n, V);
    MMDFN_CHECK_LAUNCH();
    hipLaunchKernelGGL(cnn_table_bwd_kernel, dim3((unsigned)V), dim3(64 * ((D + 63) / 64)), 0, (hipStream_t)stream, d_pooled,
                       bounds, order, S, d_table, D, F);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
