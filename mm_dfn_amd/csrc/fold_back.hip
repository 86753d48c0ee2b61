// Fold-back of the encoder input projections.  X_m = u_m W_m^T + b_m feeds a GRU's first-layer input contraction
// gi = X_m W_ih^T with nothing in between, so the weight gradients of BOTH layers follow from the small products
//   M = dG^T u_m  (n x D)   and   c = colsum(dG)  (n)
// that the end-of-backward weight-gradient batch leaves (dG: the contraction's pre-activation gradient, n of its columns = one
// direction half of W_ih):
//   dW_ih (n x H) (+)= M W_m^T + c b_m^T          kind A: row-local in M, contraction over D (+ 1 for the bias column)
//   dW_m  (H x D) (+)= W_ih^T M                   kind B: contraction over the n rows of M
//   db_m  (H)     (+)= W_ih^T c                   (kind B's column D)
// One TERM is one (direction half, modality) pair; terms that share an output are summed in term order inside the workgroup
// (kind A) or slab by slab in term order by the last workgroup of the tile (kind B): no float atomics, bit-reproducible.
// Accumulation: 32 consecutive products of a chain are summed by fp32 FMAs, the sums of 32 are accumulated in float64, kind B's
// partial slabs are float64, and the result is rounded to float ONCE, behind the optional existing gradient.  (All-float64
// chains measured 39 us for the cfg2 launch: four v_cvt_f64_f32 per four FMAs; the error of a 32-chain is at most 32 x 2^-24 of
// its absolute sum, that of M itself -- a 1 760-row bf16-piece contraction -- is larger.)
// One launch: 32 x 32 output tiles, 256 threads; the four waves split a round's chains, every lane holds 4 x 4 outputs, and the
// waves' partial tiles are summed through LDS in wave order.  Operands are staged in LDS in rounds of <= 128 k (37 KB of LDS, four
// workgroups per CU).  A kind-A workgroup runs all terms of its tile; a kind-B workgroup runs ONE term of its tile (all its rows,
// round by round) and writes a float64 slab; the tile's last-arriving workgroup (an integer ticket per tile, left at zero for the
// next launch) sums the slabs in term order.  (Slabs per 104-row chunk -- three times as many, three batches of slab loads in the
// last arriver -- measured 19.8 us for the kind-B half of the cfg2 launch, 11.5 us of it behind the contraction.)
#include "mmdfn_internal.h"
#include "../../include/mmdfn_hip.h"

namespace {

constexpr int FB_MAXTERM = 16;
constexpr int FB_MAXOUT = 32;
constexpr int FB_T = 32;            // output tile edge
constexpr int FB_LD = FB_T + 4;     // LDS row stride (floats): 16-byte aligned rows for the 4-wide operand reads
constexpr int FB_KMAX = 128;        // k per staging round (a multiple of FB_CH)
constexpr int FB_CH = 32;           // products per fp32 chain
constexpr int FB_NT = 256;

struct FbTerm {
    const float* M;
    const float* c;
    const float* wih;
    const float* wm;
    const float* bm;
    int n, D;
};

struct FbOut {
    float* out;
    float* out2;        // kind B: db_m (column D of the tile grid) or null
    unsigned mask;      // terms that contribute, in term order
    int kind;           // 0 = A (dW_ih), 1 = B (dW_m, db_m)
    int rows, cols;     // kind A: n x H; kind B: H x (D + 1 with db_m)
    int acc;
    int tiles_x, tiles, units;
    int blk0;           // first workgroup
    int slab0;          // first partial slab (kind B with units > 1)
    int cnt0;           // first ticket
};

struct FbArgs {
    int blk0[FB_MAXOUT];        // o[q].blk0 (INT_MAX behind the last output) side by side: a workgroup finds its output with
                                // wide scalar loads instead of a chain of dependent ones
    FbTerm t[FB_MAXTERM];
    FbOut o[FB_MAXOUT];
    int nout, H;
    double* slabs;
    int* tickets;
};


__global__ __launch_bounds__(FB_NT) void fold_back_kernel(const FbArgs P) {
    // ONE LDS object: [A rows | B rows] of a staging round, then the four waves' partial tiles (float64), then the reducer flag
    constexpr int LDS_FLOATS = 2 * FB_KMAX * FB_LD > 8 * FB_T * FB_T ? 2 * FB_KMAX * FB_LD : 8 * FB_T * FB_T;
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS + 4];
    float* As = lds;
    float* Bs = lds + FB_KMAX * FB_LD;
    double* red = reinterpret_cast<double*>(lds);
    int* flag = reinterpret_cast<int*>(lds + LDS_FLOATS);
    const int tid = threadIdx.x, wave = tid >> 6, lx = tid & 7, ly = (tid >> 3) & 7;
    const int H = P.H;
    int oi = 0;
#pragma unroll
    for (int q = 1; q < FB_MAXOUT; ++q)
        if ((int)blockIdx.x >= P.blk0[q]) oi = q;
    const FbOut& O = P.o[oi];
    const int local = (int)blockIdx.x - O.blk0;
    const int tile = local / O.units, unit = local - tile * O.units;
    const int i0 = (tile / O.tiles_x) * FB_T, j0 = (tile % O.tiles_x) * FB_T;
    // every wave holds the whole 32 x 32 tile, 4 x 4 outputs per lane (rows 4 ly .., columns 4 lx ..), over ITS chains of FB_CH
    // products: chain q of a round belongs to wave q % 4
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;

    auto contract = [&](const int klen) {
        // (the staging step zero-fills the rows up to the next multiple of FB_CH)
        for (int k0 = wave * FB_CH; k0 < klen; k0 += 4 * FB_CH) {
            float s[4][4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) s[a][b] = 0.f;
#pragma unroll
            for (int k = k0; k < k0 + FB_CH; ++k) {
                const float4 x = *reinterpret_cast<const float4*>(As + k * FB_LD + 4 * ly);
                const float4 y = *reinterpret_cast<const float4*>(Bs + k * FB_LD + 4 * lx);
                // (two-wide FMAs: v_pk_fma_f32, half the issue slots of sixteen scalar ones)
                typedef float f2 __attribute__((ext_vector_type(2)));
                const float xs[4] = {x.x, x.y, x.z, x.w};
                const f2 y01 = {y.x, y.y}, y23 = {y.z, y.w};
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const f2 xa = {xs[a], xs[a]};
                    f2 s01 = {s[a][0], s[a][1]}, s23 = {s[a][2], s[a][3]};
                    s01 = __builtin_elementwise_fma(xa, y01, s01);
                    s23 = __builtin_elementwise_fma(xa, y23, s23);
                    s[a][0] = s01.x; s[a][1] = s01.y; s[a][2] = s23.x; s[a][3] = s23.y;
                }
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] += (double)s[a][b];
        }
    };

    int D = 0;
    if (O.kind == 0) {
        for (int t = 0; t < FB_MAXTERM; ++t) {
            if (!((O.mask >> t) & 1u)) continue;
            const FbTerm T = P.t[t];
            const float* __restrict__ Mp = T.M;
            const float* __restrict__ cp = T.c;
            const float* __restrict__ wmp = T.wm;
            const float* __restrict__ bmp = T.bm;
            const int K = T.D + (bmp != nullptr ? 1 : 0), rows = O.rows;
            D = T.D;
            for (int k0 = 0; k0 < K; k0 += FB_KMAX) {
                const int klen = min(FB_KMAX, K - k0);
                const int kb = bmp != nullptr ? D - k0 : -1;       // the bias row's place in this round (if inside it)
                __syncthreads();                                   // the previous round's reads are done
                // thread -> rows (tid / 32) + 8 x, k = (tid % 32) + 32 y: every load of the round is issued before the first
                // LDS store (a loop that waits per element costs one global round trip per element)
                constexpr int NX = FB_T / 8, NY = (FB_KMAX + 31) / 32;
                static_assert(FB_KMAX % FB_CH == 0, "zero-filled tail rows stay inside the LDS rows");
                float av[NX][NY], bv[NX][NY];
#pragma unroll
                for (int x = 0; x < NX; ++x)
#pragma unroll
                    for (int y = 0; y < NY; ++y) {
                        const int r = (tid >> 5) + 8 * x, k = (tid & 31) + 32 * y, kk = k0 + k;
                        const int gi = i0 + r, gj = j0 + r;
                        // branch-free: every lane loads from a clamped, valid address and masks the value (loads under
                        // divergent branches are waited for one by one); the bias row k = D is staged apart, below
                        const size_t ci = (size_t)min(gi, rows - 1), cj = (size_t)min(gj, H - 1);
                        const int kc = min(kk, D - 1);
                        const float a = Mp[ci * D + kc], b = wmp[cj * D + kc];
                        // (a product, not a select: a select lets the compiler put the load back under the condition.  A
                        // non-finite value at a clamped address belongs to the same row of the same operand, whose outputs
                        // it reaches anyway)
                        av[x][y] = a * ((kk < D && gi < rows) ? 1.f : 0.f);
                        bv[x][y] = b * ((kk < D && gj < H) ? 1.f : 0.f);
                    }
#pragma unroll
                for (int x = 0; x < NX; ++x)
#pragma unroll
                    for (int y = 0; y < NY; ++y) {
                        const int r = (tid >> 5) + 8 * x, k = (tid & 31) + 32 * y;
                        if (k < ((klen + FB_CH - 1) & ~(FB_CH - 1)) && k != kb) {
                            As[k * FB_LD + r] = av[x][y];
                            Bs[k * FB_LD + r] = bv[x][y];
                        }
                    }
                if (kb >= 0 && kb < klen && tid < FB_T) {          // (wave-uniform) the row c b_m^T contracts over
                    As[kb * FB_LD + tid] = i0 + tid < rows ? cp[i0 + tid] : 0.f;
                    Bs[kb * FB_LD + tid] = j0 + tid < H ? bmp[j0 + tid] : 0.f;
                }
                __syncthreads();
                contract(klen);
            }
        }
    } else {
        // kind B: unit u = the u-th term of the output; its rows in rounds of FB_KMAX.  (All terms of a tile in ONE workgroup,
        // with no exchange between workgroups, measured 39 us: 56 workgroups carry the launch's 36 M multiply-adds.)
        int t = 0;
#pragma unroll
        for (int q = FB_MAXTERM - 1; q >= 0; --q)
            if (((O.mask >> q) & 1u) && __builtin_popcount(O.mask & ((1u << q) - 1u)) == unit) t = q;
        {
        const FbTerm T = P.t[t];
        const float* __restrict__ Mp = T.M;
        const float* __restrict__ cp = T.c;
        const float* __restrict__ wihp = T.wih;
        const bool csum = O.out2 != nullptr;
        const int nrows = T.n;
        D = T.D;
        for (int r0 = 0; r0 < nrows; r0 += FB_KMAX) {
            const int klen = min(FB_KMAX, nrows - r0);
            __syncthreads();                                       // the previous round's reads are done
            // thread -> column tid % 32 of rows (tid / 32) + 8 y: all loads first (clamped addresses, values masked by a product
            // as in kind A), then the LDS stores
            constexpr int NY = FB_KMAX / 8;
            float av[NY], bv[NY];
            const int r = tid & 31, gi = i0 + r, gj = j0 + r;
#pragma unroll
            for (int y = 0; y < NY; ++y) {
                const int k = (tid >> 5) + 8 * y;
                const size_t row = (size_t)min(r0 + k, nrows - 1);
                const float a = wihp[row * H + min(gi, H - 1)], b = Mp[row * D + min(gj, D - 1)];
                av[y] = a * ((k < klen && gi < H) ? 1.f : 0.f);
                bv[y] = b * ((k < klen && gj < D) ? 1.f : 0.f);
            }
#pragma unroll
            for (int y = 0; y < NY; ++y) {
                const int k = (tid >> 5) + 8 * y;
                if (k < ((klen + FB_CH - 1) & ~(FB_CH - 1))) {
                    As[k * FB_LD + r] = av[y];
                    if (!(csum && gj == D)) Bs[k * FB_LD + r] = bv[y];
                }
            }
            if (csum && D >= j0 && D < j0 + FB_T && tid < ((klen + FB_CH - 1) & ~(FB_CH - 1)))  // the column of c (-> db_m)
                Bs[tid * FB_LD + D - j0] = tid < klen ? cp[r0 + tid] : 0.f;
            __syncthreads();
            contract(klen);
        }
        }
    }

    // the four waves' partial tiles meet in LDS; thread -> row tid / 8, columns 4 (tid % 8) .., summed in wave order
    __syncthreads();                                               // the last round's reads are done
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) red[wave * (FB_T * FB_T) + (4 * ly + a) * FB_T + 4 * lx + b] = acc[a][b];
    __syncthreads();
    const int row = tid >> 3, c0 = 4 * (tid & 7);
    double v[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        v[b] = red[row * FB_T + c0 + b];
#pragma unroll
        for (int w = 1; w < 4; ++w) v[b] += red[w * (FB_T * FB_T) + row * FB_T + c0 + b];
    }

    if (O.kind == 0) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (i0 + row < O.rows && j0 + c0 + b < O.cols) {
                float* dst = O.out + (size_t)(i0 + row) * H + j0 + c0 + b;
                *dst = (float)(O.acc ? (double)*dst + v[b] : v[b]);
            }
        return;
    }
    if (O.units > 1) {
        double* mine = P.slabs + ((size_t)O.slab0 + (size_t)tile * O.units + unit) * (FB_T * FB_T);
#pragma unroll
        for (int b = 0; b < 4; ++b)
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(mine + row * FB_T + c0 + b),
                               (unsigned long long)__double_as_longlong(v[b]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // publish the slab, draw a ticket; the last arriver of the tile sums every slab in unit order.  The slab words are
        // agent-scope (write-through) stores and are read back by agent-scope loads: no cache writeback or invalidate -- a
        // release fence per workgroup writes the whole L2 back and made this launch 29 us.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            int* ticket = P.tickets + O.cnt0 + tile;
            const int drawn = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = drawn == O.units - 1;
            if (last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // zero again for the next launch
            *flag = last;
        }
        __syncthreads();
        if (!*flag) return;
        const double* base = P.slabs + ((size_t)O.slab0 + (size_t)tile * O.units) * (FB_T * FB_T);
#pragma unroll
        for (int b = 0; b < 4; ++b) v[b] = 0.0;
        for (int u0 = 0; u0 < O.units; u0 += 4) {          // four slabs' loads in flight, summed in unit order
            double part[4][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double* s = base + (size_t)(u0 + q) * (FB_T * FB_T);
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    part[q][b] = u0 + q < O.units
                        ? __longlong_as_double((long long)__hip_atomic_load(
                              reinterpret_cast<const unsigned long long*>(s + row * FB_T + c0 + b), __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT))
                        : 0.0;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (u0 + q < O.units) v[b] += part[q][b];
        }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int gr = i0 + row, gc = j0 + c0 + b;
        if (gr >= H || gc >= O.cols) continue;
        float* dst = gc < D ? O.out + (size_t)gr * D + gc : O.out2 + gr;
        *dst = (float)(O.acc ? (double)*dst + v[b] : v[b]);
    }
}

// the launch plan of one call: outputs by pointer identity, kind B first (its tiles end with the slab sum).  0 or -1 / -2.
int fb_plan(FbArgs& P, int nterm, const float* const* M, const float* const* c, const float* const* wih, const float* const* wm,
            const float* const* bm, float* const* dwih, float* const* dwm, float* const* dbm, const int* n, const int* D, int H,
            const int* acc_wih, const int* acc_wm, int& blocks, int64_t& slabs, int& tickets) {
    if (nterm < 1 || nterm > FB_MAXTERM || H < 4 || (H & 3)) return -2;
    for (int t = 0; t < nterm; ++t)
        if (n[t] < 1 || D[t] < 4 || (D[t] & 3)) return -2;
    P.nout = 0;
    P.H = H;
    for (int pass = 1; pass >= 0; --pass)
        for (int t = 0; t < nterm; ++t) {
            float* target = pass ? (dwm ? dwm[t] : nullptr) : (dwih ? dwih[t] : nullptr);
            if (target == nullptr) continue;
            int q = 0;
            for (; q < P.nout; ++q)
                if (P.o[q].out == target) break;
            if (q == P.nout) {
                if (P.nout == FB_MAXOUT) return -2;
                FbOut& O = P.o[P.nout++];
                O.out = target;
                O.out2 = pass && dbm ? dbm[t] : nullptr;
                O.mask = 0u;
                O.kind = pass;
                O.rows = pass ? H : n[t];
                O.cols = pass ? D[t] + (O.out2 ? 1 : 0) : H;
                O.acc = (pass ? acc_wm[t] : acc_wih[t]) ? 1 : 0;
                O.units = 0;
            }
            FbOut& O = P.o[q];
            const int first = __builtin_ctz(O.mask | (1u << t));
            // terms of one output agree on its shape (and, kind B, on the projection they came through)
            if (O.kind != pass) return -2;
            if (pass ? (D[first] != D[t] || (dbm ? dbm[t] : nullptr) != O.out2) : n[first] != n[t]) return -2;
            O.mask |= 1u << t;
            O.units += pass ? 1 : 0;
        }
    if (P.nout == 0) return -2;
    blocks = 0;
    slabs = 0;
    tickets = 0;
    int64_t nblk = 0;
    for (int q = 0; q < P.nout; ++q) {
        FbOut& O = P.o[q];
        if (O.kind == 0) O.units = 1;
        O.tiles_x = (O.cols + FB_T - 1) / FB_T;
        O.tiles = O.tiles_x * ((O.rows + FB_T - 1) / FB_T);
        O.blk0 = (int)nblk;
        O.slab0 = (int)slabs;
        O.cnt0 = tickets;
        nblk += (int64_t)O.tiles * O.units;
        if (O.units > 1) {
            slabs += (int64_t)O.tiles * O.units;
            tickets += O.tiles;
        }
        if (nblk > (1 << 20) || slabs > (1 << 20)) return -2;
    }
    blocks = (int)nblk;
    for (int q = 0; q < FB_MAXOUT; ++q) P.blk0[q] = q < P.nout ? P.o[q].blk0 : 0x7fffffff;
    for (int t = 0; t < nterm; ++t) {
        const bool a = dwih && dwih[t], b = dwm && dwm[t];
        if (M == nullptr || M[t] == nullptr) return -1;
        if (a && (wm == nullptr || wm[t] == nullptr)) return -1;
        if (b && (wih == nullptr || wih[t] == nullptr)) return -1;
        const float* bias = bm ? bm[t] : nullptr;
        const bool need_c = (a && bias) || (b && dbm && dbm[t]);
        if (need_c && (c == nullptr || c[t] == nullptr)) return -1;
        P.t[t] = FbTerm{M[t], c ? c[t] : nullptr, wih ? wih[t] : nullptr, wm ? wm[t] : nullptr, bias, n[t], D[t]};
    }
    return 0;
}

}  // namespace

extern "C" int mmdfn_fold_back_tickets(void) { return FB_MAXOUT * 64; }

extern "C" int64_t mmdfn_fold_back_workspace(int nterm, float* const* dwm, const int* n, const int* D, int H) {
    if (nterm < 1 || nterm > FB_MAXTERM || n == nullptr || D == nullptr || H < 4 || (H & 3)) return -2;
    // per distinct dW_m: tiles x slabs (an upper bound that does not look at the bias column: one more tile column)
    int64_t total = 0;
    for (int t = 0; t < nterm; ++t) {
        if (n[t] < 1 || D[t] < 4 || (D[t] & 3)) return -2;
        if (dwm == nullptr || dwm[t] == nullptr) continue;
        const int64_t tiles = (int64_t)((D[t] + 1 + FB_T - 1) / FB_T) * ((H + FB_T - 1) / FB_T);
        total += tiles;
    }
    return total * (FB_T * FB_T) * 2;       // floats (the slabs are float64)
}

extern "C" int mmdfn_fold_back(int nterm, const float* const* M, const float* const* c, const float* const* wih,
                               const float* const* wm, const float* const* bm, float* const* dwih, float* const* dwm,
                               float* const* dbm, const int* n, const int* D, int H, const int* acc_wih, const int* acc_wm,
                               float* workspace, int32_t* tickets, void* stream) {
    if (n == nullptr || D == nullptr || acc_wih == nullptr || acc_wm == nullptr) return -1;
    FbArgs P;
    int blocks = 0, ntick = 0;
    int64_t slabs = 0;
    const int rc = fb_plan(P, nterm, M, c, wih, wm, bm, dwih, dwm, dbm, n, D, H, acc_wih, acc_wm, blocks, slabs, ntick);
    if (rc != 0) return rc;
    if (ntick > mmdfn_fold_back_tickets()) return -2;
    if (slabs > 0 && (workspace == nullptr || tickets == nullptr)) return -1;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return -2;
    P.slabs = reinterpret_cast<double*>(workspace);
    P.tickets = tickets;
    hipLaunchKernelGGL(fold_back_kernel, dim3((unsigned)blocks), dim3(FB_NT), 0, (hipStream_t)stream, P);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
