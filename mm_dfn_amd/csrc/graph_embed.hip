// K11: speaker / modality embeddings of the graph input, one launch each way.
//
// Replaces the per-dialogue qmask slices, the argmax, the nn.Embedding lookup and the in-place adds in front of the adjacency
// build (MM_GCN.forward, reference model_mm.py:78-93) on the (M, N, D) modality-major stack:
//   s_n   = first maximum of qmask[flat_idx[n], :]           (torch.argmax on the loaders' one-hot rows; an all-zero row: 0)
//   Y[l]  = (X[l] + speaker[s_n]) + modal[2]                  (the reference's order of the two in-place adds)
//   Y[m]  = X[m] + modal[row(m)]                              (a -> 0, v -> 1)
// Plain fp32 adds: bit-equal to the torch path.  The speaker index is read from device memory through flat_idx (the pad-strip
// index t * B + b of every stripped row), so a captured step whose index arrays are rewritten serves other dialogue lengths;
// the grids depend on (M, N, D) only.
// Backward: dX is dY itself (no launch).  The table gradients
//   d speaker[s]   = sum_{n : s_n = s} dY[l, n, :]           d modal[row(m)] = sum_n dY[m, n, :]
// come from ONE launch without float atomics and without a workspace: a workgroup owns a 64-byte column strip of one modality
// for all N rows; GE_ROWS row groups walk the rows in a fixed order, each thread adds into LDS sums of its own (one per speaker)
// and a register (the modality sum), and the row groups' sums are added in group order.  Bit-reproducible.
#include "mmdfn_internal.h"
#include "../../include/mmdfn_hip.h"

namespace {

constexpr int GE_NT = 256;
constexpr int GE_MAX_M = 3;              // subsets of 'avl' (model_mm.py:97-106)
constexpr int GE_STRIP = 16;             // floats of a backward workgroup's column strip (64 bytes: four 16-byte lanes)
constexpr int GE_LANES = GE_STRIP / 4;
constexpr int GE_ROWS = GE_NT / GE_LANES;  // row groups of a backward workgroup: thread (g, lane) takes rows g, g + GE_ROWS, ...
// (S + 1) sums x GE_ROWS row groups x 64 bytes of LDS: 64 KB at S = 15
constexpr int GE_MAX_S = 15;

struct GeSlots {
    int row[GE_MAX_M];                   // row of slot m in the modality table
};

// (selects, not an indexed read of the by-value argument)
__device__ __forceinline__ int ge_row(const GeSlots& sl, int m) { return m == 0 ? sl.row[0] : (m == 1 ? sl.row[1] : sl.row[2]); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

__global__ __launch_bounds__(GE_NT) void graph_embed_fwd_kernel(const float* __restrict__ X, const float* __restrict__ qmask,
                                                                const int64_t* __restrict__ flat_idx,
                                                                const float* __restrict__ spk_tab,
                                                                const float* __restrict__ mod_tab, float* __restrict__ Y,
                                                                int32_t* __restrict__ spk, GeSlots slots, int l_slot, int M, int N,
                                                                int D4, int P, int64_t LB) {
    const int64_t idx = blockIdx.x * (int64_t)GE_NT + threadIdx.x;          // one 16-byte lane of the stack
    if (idx >= (int64_t)M * N * D4) return;
    const int64_t r = idx / D4;
    const int c4 = (int)(idx - r * D4);
    const int m = (int)(r / N);
    const int n = (int)(r - (int64_t)m * N);
    float4 x = ld4(X + idx * 4);
    if (spk_tab != nullptr && m == l_slot) {
        const int64_t fi = flat_idx[n];
        int s = 0;
        if (fi >= 0 && fi < LB) {                      // (an index outside the grid reads nothing: speaker 0)
            const float* q = qmask + fi * P;
            float best = q[0];
            for (int p = 1; p < P; ++p) {
                const float v = q[p];
                if (v > best || (v != v && best == best)) {      // first maximum; a NaN counts as the maximum (torch.argmax)
                    best = v;
                    s = p;
                }
            }
        }
        if (c4 == 0) spk[n] = s;
        x = add4(x, ld4(spk_tab + ((int64_t)s * D4 + c4) * 4));
    }
    if (mod_tab != nullptr) x = add4(x, ld4(mod_tab + ((int64_t)ge_row(slots, m) * D4 + c4) * 4));
    st4(Y + idx * 4, x);
}

__global__ __launch_bounds__(GE_NT) void graph_embed_bwd_kernel(const float* __restrict__ dY, const int32_t* __restrict__ spk,
                                                                float* __restrict__ dspk, float* __restrict__ dmod, GeSlots slots,
                                                                int l_slot, int M, int N, int D, int S) {
    extern __shared__ float4 ge_acc[];               // [nacc + 1][GE_ROWS][GE_LANES] float4
    const int nstrip = (D + GE_STRIP - 1) / GE_STRIP;
    const int m = blockIdx.x / nstrip;
    const int strip = blockIdx.x - m * nstrip;
    const bool speak = dspk != nullptr && m == l_slot;
    if (!speak && dmod == nullptr) return;           // (the whole workgroup: nothing to sum for this modality)
    const int nacc = speak ? S : 0;
    const int lane = threadIdx.x & (GE_LANES - 1);
    const int g = threadIdx.x / GE_LANES;
    const int col = strip * GE_STRIP + lane * 4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < nacc; ++s) ge_acc[(s * GE_ROWS + g) * GE_LANES + lane] = zero;
    float4 msum = zero;
    if (col < D) {                                   // (D % 4 == 0: a lane is inside the row or outside it)
        const float* src = dY + (int64_t)m * N * D + col;
        for (int n = g; n < N; n += GE_ROWS) {
            const float4 v = ld4(src + (int64_t)n * D);
            msum = add4(msum, v);
            if (speak) {
                const int s = spk[n];
                if (s >= 0 && s < S) {
                    float4* a = &ge_acc[(s * GE_ROWS + g) * GE_LANES + lane];      // this thread's own sum: no race
                    *a = add4(*a, v);
                }
            }
        }
    }
    ge_acc[(nacc * GE_ROWS + g) * GE_LANES + lane] = msum;
    __syncthreads();
    // the row groups' sums, added in group order: (nacc + 1) * GE_STRIP <= GE_NT outputs, one thread each
    const float* acc = reinterpret_cast<const float*>(ge_acc);
    const int t = threadIdx.x;
    const int s = t / GE_STRIP;
    const int c = strip * GE_STRIP + (t & (GE_STRIP - 1));
    if (s <= nacc && c < D) {
        float sum = 0.f;
        for (int k = 0; k < GE_ROWS; ++k) sum += acc[(s * GE_ROWS + k) * GE_STRIP + (t & (GE_STRIP - 1))];
        if (s < nacc)
            dspk[(int64_t)s * D + c] = sum;
        else if (dmod != nullptr)
            dmod[(int64_t)ge_row(slots, m) * D + c] = sum;
    }
    // rows of absent modalities are exact zeros: written by slot 0's workgroups, strip by strip
    if (m == 0 && dmod != nullptr && t < GE_STRIP && strip * GE_STRIP + t < D) {
        for (int row = 0; row < 3; ++row) {
            const bool present = slots.row[0] == row || slots.row[1] == row || slots.row[2] == row;      // (unused slots hold -1)
            if (!present) dmod[(int64_t)row * D + strip * GE_STRIP + t] = 0.f;
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// modality-table rows of the M slots: distinct, inside the table, 'l' (row 2) in slot l_slot and nowhere else
bool ge_slots(GeSlots& sl, const int32_t* modal_rows, int l_slot, int M) {
    if (M < 1 || M > GE_MAX_M || modal_rows == nullptr || l_slot < -1 || l_slot >= M) return false;
    for (int m = 0; m < GE_MAX_M; ++m) sl.row[m] = -1;
    for (int m = 0; m < M; ++m) {
        const int r = modal_rows[m];
        if (r < 0 || r > 2 || (r == 2) != (m == l_slot)) return false;
        for (int k = 0; k < m; ++k)
            if (sl.row[k] == r) return false;
        sl.row[m] = r;
    }
    return true;
}

}  // namespace

extern "C" int mmdfn_graph_embed_rows(void) { return GE_ROWS; }
extern "C" int mmdfn_graph_embed_threads(void) { return GE_NT; }
extern "C" int mmdfn_graph_embed_max_speakers(void) { return GE_MAX_S; }

extern "C" int mmdfn_graph_embed_fwd(const float* X, const float* qmask, const int64_t* flat_idx, const float* speaker,
                                     const float* modal, const int32_t* modal_rows, int l_slot, float* Y, int32_t* spk, int M,
                                     int N, int D, int P, int S, int64_t LB, void* stream) {
    GeSlots sl;
    if (X == nullptr || Y == nullptr || N <= 0 || D <= 0 || !ge_slots(sl, modal_rows, l_slot, M)) return -1;
    if (l_slot < 0) speaker = nullptr;               // no 'l': the speaker embedding has nothing to be added to
    if (speaker != nullptr && (qmask == nullptr || flat_idx == nullptr || spk == nullptr || P <= 0 || S <= 0 || LB <= 0 || P > S))
        return -1;
    if (D % 4 != 0 || !aligned16(X) || !aligned16(Y) || !aligned16(speaker) || !aligned16(modal)) return -2;
    if (speaker != nullptr && S > GE_MAX_S) return -2;           // (the backward launch's LDS sums)
    const int64_t total = (int64_t)M * N * (D / 4);
    const int64_t blocks = (total + GE_NT - 1) / GE_NT;
    if (blocks > 0x7fffffff) return -1;
    hipLaunchKernelGGL(graph_embed_fwd_kernel, dim3((unsigned)blocks), dim3(GE_NT), 0, (hipStream_t)stream, X, qmask, flat_idx,
                       speaker, modal, Y, spk, sl, l_slot, M, N, D / 4, P, LB);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_graph_embed_bwd(const float* dY, const int32_t* spk, float* dspeaker, float* dmodal,
                                     const int32_t* modal_rows, int l_slot, int M, int N, int D, int S, void* stream) {
    GeSlots sl;
    if (dY == nullptr || N <= 0 || D <= 0 || !ge_slots(sl, modal_rows, l_slot, M)) return -1;
    if (l_slot < 0) dspeaker = nullptr;
    if (dspeaker != nullptr && (spk == nullptr || S <= 0)) return -1;
    if (dspeaker == nullptr && dmodal == nullptr) return -1;
    if (D % 4 != 0 || !aligned16(dY)) return -2;
    if (dspeaker != nullptr && S > GE_MAX_S) return -2;
    const int nstrip = (D + GE_STRIP - 1) / GE_STRIP;
    const size_t lds = (size_t)((dspeaker != nullptr ? S : 0) + 1) * GE_ROWS * GE_LANES * sizeof(float4);
    hipLaunchKernelGGL(graph_embed_bwd_kernel, dim3((unsigned)(M * nstrip)), dim3(GE_NT), lds, (hipStream_t)stream, dY, spk,
                       dspeaker, dmodal, sl, l_slot, M, N, D, S);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
