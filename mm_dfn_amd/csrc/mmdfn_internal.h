// Internal helpers shared by the gfx950 kernels of libmmdfn_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define MMDFN_CHECK_LAUNCH()                         \
    do {                                             \
        hipError_t e__ = hipGetLastError();          \
        if (e__ != hipSuccess) return (int)e__;      \
    } while (0)

// sim(c) = 1 - acos(0.99999 c) / pi          (model_mm.py:149-150, 166-167)
#define MMDFN_COS_SHRINK 0.99999f
#define MMDFN_PI_F 3.14159265358979323846f

// compute units of the target (gfx950 / MI355X): what the GRU launches' rider sizing counts idle CUs against
constexpr int MMDFN_CUS = 256;

__device__ __forceinline__ float mmdfn_sim(float c) {
    return 1.0f - acosf(c * MMDFN_COS_SHRINK) / MMDFN_PI_F;
}
// d sim / d c = a / (pi sqrt(1 - (a c)^2))
__device__ __forceinline__ float mmdfn_dsim(float c) {
    float ac = c * MMDFN_COS_SHRINK;
    return MMDFN_COS_SHRINK / (MMDFN_PI_F * sqrtf(1.0f - ac * ac));
}

// Graph kinds of the adjacency build (mmdfn_adj_build_kind), a compile-time parameter of its kernels:
//   0  angular similarity  sim(c) = 1 - acos(0.99999 c) / pi, cross-modal entries sim(cos) * modal_weight
//      (MM_GCN.create_big_adj, model_mm.py:122-180)
//   1  arccos distance     sim(c) = acos(0.99999 c), cross-modal entries the constant the modal_weight slot carries
//      (MM_GCN2.create_big_adj, model_mm.py:241-296; GCNII_lyc.message_passing_wo_speaker, model_GCN.py:490-511)
//      The diagonal of a tile is cos(x, x) = 1 by definition: kind 1 takes it as that constant (entry acos(0.99999), no
//      gradient through it) instead of the rounded sum u.u -- acos is at its steepest there (|d acos| = 224 at 0.99999), so
//      the last-bit noise of a float32 dot product would otherwise be the whole error of the graph (3e-5 against 2e-7).
constexpr int MMDFN_ADJ_KINDS = 2;
template <int KIND>
__device__ __forceinline__ float mmdfn_sim_k(float c) {
    if (KIND == 0) return mmdfn_sim(c);
    return acosf(c * MMDFN_COS_SHRINK);
}
// kind 1: d acos(a c) / d c = -a / sqrt((1 - a c)(1 + a c)).  The factored radicand keeps its relative accuracy where a c is
// within 1e-5 of 1 (the diagonal of the Gram matrix, c = 1 +- a few ulp): 1 - a c is exact there, 1 - (a c)^2 would round the
// square first; it stays positive as long as c < 1 / a = 1 + 1e-5.
template <int KIND>
__device__ __forceinline__ float mmdfn_dsim_k(float c) {
    if (KIND == 0) return mmdfn_dsim(c);
    const float ac = c * MMDFN_COS_SHRINK;
    return -MMDFN_COS_SHRINK / sqrtf((1.0f - ac) * (1.0f + ac));
}

// index of the unordered modality pair (m < n) in lexicographic order
__host__ __device__ __forceinline__ int mmdfn_pair_index(int m, int n, int M) {
    return m * (2 * M - m - 1) / 2 + (n - m - 1);
}

// Reductions on the DPP path (hipcc turns __shfl_xor into ds_bpermute_b32: an LDS round trip per step).  After the two quad
// steps every quad holds its sum in all four lanes, so the mirror steps are exchanges between equal halves: all 16 lanes of a
// row end with the same bits.
template <int CTRL>
__device__ __forceinline__ float mmdfn_dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// sum over each row of 16 lanes (every lane of the row gets it)
__device__ __forceinline__ float row_sum16(float v) {
    v += mmdfn_dpp_mov<0xB1>(v);          // quad_perm [1,0,3,2]
    v += mmdfn_dpp_mov<0x4E>(v);          // quad_perm [2,3,0,1]
    v += mmdfn_dpp_mov<0x141>(v);         // row_half_mirror
    v += mmdfn_dpp_mov<0x140>(v);         // row_mirror
    return v;
}
__device__ __forceinline__ float lane_value(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
// sum over the whole wave (every lane gets it): four row sums met through scalar registers in a fixed order
__device__ __forceinline__ float wave_sum(float v) {
    v = row_sum16(v);
    return (lane_value(v, 0) + lane_value(v, 16)) + (lane_value(v, 32) + lane_value(v, 48));
}
// sum over the 32 lanes of each half of the wave (lanes 0-31 get the lower half's sum, 32-63 the upper's)
__device__ __forceinline__ float half_sum32(float v) {
    v = row_sum16(v);
    const float lo = lane_value(v, 0) + lane_value(v, 16);
    const float hi = lane_value(v, 32) + lane_value(v, 48);
    return (threadIdx.x & 32) ? hi : lo;
}

// Gate non-linearities on the hardware transcendental units (v_exp_f32 / v_rcp_f32, ~1 ulp each): the accurate libm expf /
// tanhf are ~600 cycles of dependent scalar code per timestep on the serial critical path of the GRU recurrence
// (tools/ubench/step_latency.hip), and the LSTM cell of the GCN stack evaluates six per element -- more issue slots than the
// contraction next to it.  Absolute error < 3e-7, far inside the 1e-5 parity budget of the encoders and the stack (logits 1e-4).
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }
// the libm form, for the pointwise kernels off the critical path (gcn_pointwise.hip, fusion.hip)
__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// more than 64 KB of dynamic LDS per workgroup needs the attribute raised once per kernel (gfx950: 160 KB per CU)
template <class Kern>
inline int mmdfn_allow_big_lds(Kern kern) {
    static thread_local const void* done[48] = {nullptr};      // (one table per kernel SIGNATURE: kernels of one type share it)
    const void* key = reinterpret_cast<const void*>(kern);
    for (int i = 0; i < 48; ++i)
        if (done[i] == key) return 0;
    // (a little below the 160 KB of a CU: kernels may also hold a few hundred bytes of static LDS)
    hipError_t e = hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
    if (e != hipSuccess) {
        (void)hipGetLastError();      // do not leave the error for the next launch check to find
        return (int)e;
    }
    for (int i = 0; i < 48; ++i)
        if (done[i] == nullptr) { done[i] = key; break; }
    return 0;
}

// launchers implemented in propagate.hip / tile_dot.hip, used by adjacency.hip
int mmdfn_launch_propagate(const float* tiles, const float* cross, const float* H, float* out,
                           const int32_t* dia_len, const int32_t* row_start, const int64_t* tile_base,
                           int B, int M, int N, int d, int ldh, int ldo, int max_len, int transpose, hipStream_t s);

// one-workgroup-per-(dialogue, modality) form of the adjacency build for short dialogues (adjacency_small.hip); -2 = not covered
int mmdfn_launch_adj_small_fwd(const float* feats, float* unit, float* norm, float* cosg, float* cdot, float* rdeg,
                               float* tiles, float* cross, const int32_t* dia_len, const int32_t* row_start,
                               const int64_t* tile_base, int B, int M, int N, int D, int max_len, float modal_weight,
                               int kind, hipStream_t s);
int mmdfn_launch_adj_small_bwd(const float* dtiles, const float* dcross, const float* unit, const float* norm,
                               const float* cosg, const float* cdot, const float* rdeg, const float* tiles,
                               const float* cross, const float* addend, float* dfeats, const int32_t* dia_len,
                               const int32_t* row_start, const int64_t* tile_base, int B, int M, int N, int D, int max_len,
                               float modal_weight, int kind, hipStream_t s);

// bf16-piece variant of the forward product for large launches (propagate_split.hip); -2 = shape not covered
int mmdfn_launch_propagate_split(const float* tiles, const float* cross, const float* H, float* out,
                                 const int32_t* dia_len, const int32_t* row_start, const int64_t* tile_base,
                                 int B, int M, int N, int d, int ldh, int ldo, int max_len, hipStream_t s);

// bf16-piece variant of the dense projection for many-row launches (linear_split.hip); -2 = shape not covered
int mmdfn_launch_linear_split(const float* X, const float* W, const float* W2, int N1, const float* bias,
                              const float* bias2, float* Y, int R, int K, int N, int ldx, int ldy, int act, int accumulate,
                              hipStream_t s);

// bf16-piece form of the GCN stack's LSTM cell for many-row launches (lstm_gate_split.hip); -2 = shape not covered
int mmdfn_launch_lstm_gate_fwd_split(const float* q, const float* h, const float* c, const float* Wih, const float* Whh,
                                     const float* bsum, const float* bsum2, float* gates, float* h_out, float* c_out, int R,
                                     int H, int ldh, const void* planes, hipStream_t s);
// piece planes of the cell's weights for the form above (cut once per step; `planes` = null: every workgroup cuts its own)
int64_t mmdfn_lstm_gate_planes_floats(int H);
int mmdfn_launch_lstm_gate_cut(const float* Wih, const float* Whh, void* planes, int H, hipStream_t s);

int mmdfn_launch_tile_dot_split(const float* X, const float* Y, float* out_tiles, const int32_t* dia_len,
                                const int32_t* row_start, const int64_t* tile_base, int B, int M, int N, int K, int ldx,
                                int ldy, int max_len, int accumulate, hipStream_t s);

// EPI 0: dtiles (+)= X.Y^T ; EPI 1: cosine Gram + raw similarity + row degree ; EPI 2: EPI 1 with the arccos kind's sim
int mmdfn_launch_tile_dot(const float* X, const float* Y, float* out_tiles, float* out_aux, float* deg,
                          const int32_t* dia_len, const int32_t* row_start, const int64_t* tile_base,
                          int B, int M, int N, int K, int ldx, int ldy, int max_len, int epi, int accumulate, hipStream_t s);

// bf16-piece form of the weight-gradient batch (gemm_tn_split.hip): the segment table of one launch.  A workgroup owns a
// MMDFN_TNS_TM x MMDFN_TNS_TN output tile of segment p over the rows [split * rows_per_split, ...) of its split; tiles =
// row tiles x nblocks (column blocks).  part / colpart: the slab stacks of gemm_tn.hip's batch ([split][M][N], [split][M]).
// Block index -> (split, tile) inside a segment's range of 8 ceil(splits / 8) tiles blocks: XCD = block % 8 takes the splits
// = its number (mod 8), all tiles of a split back to back -- the workgroups that read the same operand rows run on one XCD
// at the same time and share them through its L2 (blocks of splits past the last one exit at once).
#define MMDFN_TNS_BK 32
#define MMDFN_TNS_TM 128
#define MMDFN_TNS_TN 112
template <int CAP>
struct TnSegTable {
    const float* A[CAP];
    const float* B[CAP];
    float* part[CAP];
    float* colpart[CAP];
    int R[CAP], lda[CAP], ldb[CAP], bshift[CAP];
    int rows_per_split[CAP], splits[CAP], tiles[CAP], nblocks[CAP];
    int M[CAP], N[CAP];
    int wide[CAP];          // != 0: 128 x (2 MMDFN_TNS_TN) tiles, nblocks counts 224-column blocks (gemm_tn_split.hip)
    int wg_prefix[CAP + 1];
    int n;
};
// the first min(CD, CS) slots of s (and its n) as a table of another capacity; the rest of d is zero
template <int CD, int CS>
inline void mmdfn_seg_copy(TnSegTable<CD>& d, const TnSegTable<CS>& s) {
    constexpr int m = CD < CS ? CD : CS;
    auto cp = [](auto& dst, const auto& src, int cnt) { for (int k = 0; k < cnt; ++k) dst[k] = src[k]; };
    d = TnSegTable<CD>();
    cp(d.A, s.A, m); cp(d.B, s.B, m); cp(d.part, s.part, m); cp(d.colpart, s.colpart, m);
    cp(d.R, s.R, m); cp(d.lda, s.lda, m); cp(d.ldb, s.ldb, m); cp(d.bshift, s.bshift, m);
    cp(d.rows_per_split, s.rows_per_split, m); cp(d.splits, s.splits, m); cp(d.tiles, s.tiles, m); cp(d.nblocks, s.nblocks, m);
    cp(d.M, s.M, m); cp(d.N, s.N, m); cp(d.wide, s.wide, m); cp(d.wg_prefix, s.wg_prefix, m + 1);
    d.n = s.n;
}
// (the two capacities are named types, not aliases: the kernels that take them by value keep their symbols)
constexpr int MMDFN_TNS_MAXSEG = 40;
struct TnSplitSegs : TnSegTable<MMDFN_TNS_MAXSEG> {};
int mmdfn_launch_gemm_tn_split(const TnSplitSegs& sq, hipStream_t s);

// Riders of the GRU recurrence launches (gru.hip, gru_mfma.hip): work STAGED in a caller-owned MmdfnRiders context instead of
// launched -- a weight-gradient batch (mmdfn_wgrad_riders_stage, gemm_tn.hip) or a dropout-flag draw (mmdfn_keep_flags_stage,
// encoder_glue.hip).  A GRU backward / forward launch given the context runs what it holds as extra workgroups on the CUs the
// recurrence leaves idle; mmdfn_riders_launched then files the batch's slab reduction.  What a launch did not take is launched
// the ordinary way by mmdfn_wgrad_riders_flush / mmdfn_keep_flags_flush.
constexpr int MMDFN_RIDER_MAXSEG = 16;
struct TnRiderSegs : TnSegTable<MMDFN_RIDER_MAXSEG> {};      // what a recurrence launch carries (mmdfn_seg_copy of a batch's table)
static_assert(sizeof(TnSplitSegs) == 3208 && sizeof(TnRiderSegs) == 1288, "kernel-argument layouts of the segment tables");

constexpr int TN_MAXOUT = 40;      // outputs of one weight-gradient batch's reduction launch (gemm_tn.hip)
namespace kfb {
struct FlagJob {            // one dropout keep-flag draw (keep_flags_body.h)
    float* out;
    int64_t n8, n4;
    uint32_t threshold;
    int all;
    unsigned long long* state;
};
}  // namespace kfb

// One output of a weight-gradient batch's slab reduction: `splits` slabs summed into C / colsum / colsum2 (gemm_tn.hip).
struct DeferredOut {
    const float* part; const float* colpart; float* C; float* colsum; float* colsum2;
    int M, N, ldc, splits, accumulate;
};
// A batch staged for a GRU backward launch: its tile table and the outputs of its slab reduction.
struct RiderPlan {
    bool valid;
    TnSplitSegs tq;
    DeferredOut outs[TN_MAXOUT];
    int nout;
};
// The rider context (mmdfn_riders_bytes): host memory owned by the caller, all-zero bytes = empty.
struct MmdfnRiders {
    RiderPlan rider;
    DeferredOut deferred[TN_MAXOUT];      // slab reductions of batches that rode, waiting for the next reduction launch
    int ndeferred;
    kfb::FlagJob flag_job;
    bool flag_job_valid;
};
static_assert(sizeof(MmdfnRiders) == 8400, "mmdfn_riders_bytes(): what callers allocate");
int mmdfn_riders_launched(MmdfnRiders* riders, hipStream_t s);

// How the plain (unsegmented) recurrence launch of these groups runs: the MFMA form (16 sequences per workgroup) or R sequences
// per workgroup, `slices` workgroups per direction, and the CUs it leaves idle for riders (0: it takes none).  The launches and
// the query entry points all read it.
struct GruForm {
    bool mfma;
    int R, slices, idle_cus;
};
GruForm mmdfn_gru_form(int ngroups, const int* rows);

// MFMA form of the GRU recurrence for launches with very many sequences (gru_mfma.hip): 16 sequences per workgroup, the
// recurrent products on bf16 pieces.  Same operands and layouts as mmdfn_gru_seq_fwd / _bwd; -2 = not covered.
int mmdfn_launch_gru_fwd_mfma(const GruForm& f, int ngroups, const float* const* gi, const float* const* w_hh,
                              const float* const* b_hh, float* const* y, float* const* gates, const int* rows, const int* T,
                              MmdfnRiders* riders, hipStream_t s);
int mmdfn_launch_gru_bwd_mfma(const GruForm& f, int ngroups, const float* const* dy, const float* const* y,
                              const float* const* gates, const float* const* w_hh, float* const* dgi, float* const* dgh,
                              const int* rows, const int* T, MmdfnRiders* riders, hipStream_t s);

// Host fillers of the recurrence launches' group tables (gru.hip FwdGroups / BwdGroups, gru_mfma.hip MfFwd / MfBwd: kernel
// arguments passed by value, the same leading fields in both files).  A filler value-initialises the table, copies the ngroups
// live slots and lays the groups' workgroup slices end to end, per_wg sequences per workgroup: slice0[g] = first slice of group
// g, slice0[ngroups ..] = their total (per_wg = 0: a segmented launch, whose workgroups are chains -- every slice0 stays 0).
// false = a group without rows or steps.  What only one table has (abl, seg, ytab, dhinit, kout) is set by the caller.
template <class Tab>
inline bool mmdfn_gru_fill(Tab& G, int ngroups, const float* const* w_hh, const int* rows, const int* T, int per_wg) {
    constexpr int maxg = sizeof(G.rows) / sizeof(G.rows[0]);
    G = Tab();
    G.n = ngroups;
    int sl = 0;
    for (int g = 0; g < ngroups; ++g) {
        if (rows[g] <= 0 || T[g] <= 0) return false;
        G.w_hh[2 * g] = w_hh[2 * g]; G.w_hh[2 * g + 1] = w_hh[2 * g + 1];
        G.rows[g] = rows[g]; G.T[g] = T[g]; G.slice0[g] = sl;
        if (per_wg > 0) sl += (rows[g] + per_wg - 1) / per_wg;
    }
    for (int g = ngroups; g <= maxg; ++g) G.slice0[g] = sl;
    return true;
}
template <class Tab>
inline bool mmdfn_gru_fill_fwd(Tab& G, int ngroups, const float* const* gi, const float* const* w_hh, const float* const* b_hh,
                               float* const* y, float* const* gates, const int* rows, const int* T, int per_wg) {
    if (!mmdfn_gru_fill(G, ngroups, w_hh, rows, T, per_wg)) return false;
    for (int g = 0; g < ngroups; ++g) {
        G.gi[g] = gi[g]; G.y[g] = y[g]; G.gates[g] = gates[g];
        G.b_hh[2 * g] = b_hh[2 * g]; G.b_hh[2 * g + 1] = b_hh[2 * g + 1];
    }
    return true;
}
template <class Tab>
inline bool mmdfn_gru_fill_bwd(Tab& G, int ngroups, const float* const* dy, const float* const* y, const float* const* gates,
                               const float* const* w_hh, float* const* dgi, float* const* dgh, const int* rows, const int* T,
                               int per_wg) {
    if (!mmdfn_gru_fill(G, ngroups, w_hh, rows, T, per_wg)) return false;
    for (int g = 0; g < ngroups; ++g) {
        G.dy[g] = dy[g]; G.y[g] = y[g]; G.gates[g] = gates[g]; G.dgi[g] = dgi[g]; G.dgh[g] = dgh[g];
    }
    return true;
}
