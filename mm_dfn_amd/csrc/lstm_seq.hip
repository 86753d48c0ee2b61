// K16: fused LSTM recurrence (forward and backward through time) of the recurrent baseline ``LSTMModel``
// (reference model.py:320-356: nn.LSTM(D_m, 100, num_layers=2, bidirectional=True), run step by step through ATen / MIOpen).
//
// Split of one LSTM layer, as for the GRU (gru.hip):
//   * the input contraction  GI = X W_ih^T + b_ih  for all timesteps and both directions is one dense launch outside this
//     file (ops.linear2);
//   * this file is the serial part: one PERSISTENT workgroup per (sequence, direction), blockIdx.y = direction, so there is
//     no inter-workgroup synchronisation and no launch per step.  W_hh (4H x H fp32 = 160 KB per direction) lives in
//     REGISTERS, sliced over the workgroup: the lane pair (2u, 2u+1) keeps the i / f / g / o rows of hidden unit u, each
//     lane one half of the contraction index (4 x 52 floats); h_{t-1} is broadcast from a double-buffered LDS row; the two
//     partial sums meet with one DPP exchange and every lane applies the gate math: ONE barrier per timestep.  The cell
//     state c stays in a register of the owning pair.
//
// Gate order i, f, g, o (torch):  a = W_hh h + b_hh + gi;  i, f, o = sig(.);  g = tanh(.);  c' = f c + i g;  h' = o tanh(c').
//
// Global memory traffic of the time loop is BLOCKED, as in gru.hip's gru_seq_fwd_kernel: gfx950 retires vector memory
// operations in order and vmcnt counts stores as well as loads, so a per-step wait for the next step's operands would also
// wait for the previous step's result stores.  The operands of LSTM_TB consecutive timesteps are copied global -> registers
// one block ahead (coalesced 16-byte loads by all 256 threads), dropped into LDS at the block boundary, and a block's results
// are collected in LDS and written out with coalesced 16-byte stores that nobody waits for before the next block boundary.
// Inside a block the recurrence touches LDS only.  All waits are the compiler's (no hand-counted vmcnt / lgkmcnt).
//
// Deliberately absent (LSTMModel runs 2B chains, 32-64 at the reference's batch sizes, against 256 CUs): an MFMA many-sequence
// form, valid-length segmented launches, weight-gradient / flag riders, several modules per launch.
#include "mmdfn_internal.h"
#include "../../include/mmdfn_hip.h"

namespace {

constexpr int LH = 100;          // hidden size (the reference's D_e)
constexpr int LNT = 256;
constexpr int LSTM_TB = 8;       // timesteps per staged block
constexpr int LK0 = 52;          // forward: split point of the contraction index (16-byte aligned halves [0, 52) / [52, 100))
constexpr int LKW = 52;          // forward: weights held per gate per lane (second half: 48 used, 4 zeros)
constexpr int LJ0 = 200;         // backward: split point of the 4H gate rows
constexpr int LJW = 200;         // backward: weights held per lane

typedef float l32x2 __attribute__((ext_vector_type(2)));

// a use of a freshly loaded register BEFORE the time loop: keeps the compiler from sinking the loop-invariant weight loads
// (and their vmcnt waits) into the step loop
__device__ __forceinline__ void lstm_pin(float& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void lstm_pin(l32x2& v) {
    float a = v[0], b = v[1];
    asm volatile("" : "+v"(a), "+v"(b));
    v[0] = a;
    v[1] = b;
}

// Gate non-linearities.  The GRU kernels' forms on the hardware exp / rcp units (mmdfn_internal.h: sigmoidf_, tanhf_) are
// accurate to a few u ABSOLUTELY; 1 - 2 / (1 + e^2x) loses the relative accuracy of a small tanh to the cancellation, and at
// the model's initialisation (|W| <= 0.1) most of g and tanh(c) is small.  Those errors reach the weight gradients' small
// entries, which Adam amplifies (profiles/lstm_model.md), so K16 uses libm's tanhf (relative accuracy) and a sigmoid on
// libm's expf with a true division, in the forward pass and for the backward pass's recomputed tanh(c).
__device__ __forceinline__ float lstm_sigmoid(float x) { return sigmoid_exact(x); }
__device__ __forceinline__ float lstm_tanh(float x) { return tanhf(x); }

// exchange with the other lane of the pair (lane ^ 1): DPP quad_perm [1,0,3,2]
__device__ __forceinline__ float lstm_pair_swap(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
}

// gi (T, rows, 8H);  y (T, rows, 2H);  state (T, rows, 2, 5, H): i f g o c
__global__ __launch_bounds__(LNT) void lstm_seq_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ w_f,
                                                            const float* __restrict__ w_r, const float* __restrict__ b_f,
                                                            const float* __restrict__ b_r, float* __restrict__ y,
                                                            float* __restrict__ state, const int rows, const int T) {
    constexpr int TB = LSTM_TB;
    constexpr int IN4 = 4 * LH / 4;                 // float4 per step of staged input  (gi: i f g o)
    constexpr int OUT4 = 6 * LH / 4;                // float4 per step of staged output (y | i f g o c)
    constexpr int NIN = (TB * IN4 + LNT - 1) / LNT;
    __shared__ __attribute__((aligned(16))) float hs[2][LH + 4];
    __shared__ __attribute__((aligned(16))) float in_s[2][TB][4 * LH];
    __shared__ __attribute__((aligned(16))) float out_s[TB][6 * LH];

    const int tid = threadIdx.x;
    const int u = tid >> 1;
    const int half = tid & 1;
    const bool active = u < LH;
    const int uu = active ? u : LH - 1;
    const int kbase = half ? LK0 : 0;
    const int klen = half ? LH - LK0 : LK0;
    const int dir = blockIdx.y;
    const int row = blockIdx.x;
    const float* __restrict__ w_hh = dir ? w_r : w_f;
    const float* __restrict__ b_hh = dir ? b_r : b_f;

    // weights as packed pairs (v_pk_fma_f32: two FMAs per issue slot)
    l32x2 wi[LKW / 2], wf[LKW / 2], wg[LKW / 2], wo[LKW / 2];
#pragma unroll
    for (int k = 0; k < LKW; ++k) {
        const bool ok = k < klen;
        const int kk = kbase + (ok ? k : 0);
        wi[k >> 1][k & 1] = ok ? w_hh[(int64_t)(0 * LH + uu) * LH + kk] : 0.f;
        wf[k >> 1][k & 1] = ok ? w_hh[(int64_t)(1 * LH + uu) * LH + kk] : 0.f;
        wg[k >> 1][k & 1] = ok ? w_hh[(int64_t)(2 * LH + uu) * LH + kk] : 0.f;
        wo[k >> 1][k & 1] = ok ? w_hh[(int64_t)(3 * LH + uu) * LH + kk] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < LKW / 2; ++k) {
        lstm_pin(wi[k]);
        lstm_pin(wf[k]);
        lstm_pin(wg[k]);
        lstm_pin(wo[k]);
    }
    float bi = b_hh[uu], bf = b_hh[LH + uu], bg = b_hh[2 * LH + uu], bo = b_hh[3 * LH + uu];
    lstm_pin(bi);
    lstm_pin(bf);
    lstm_pin(bg);
    lstm_pin(bo);

    const bool mine = active && half == 0;
    const int nblocks = (T + TB - 1) / TB;
    float4 stage[NIN];
    auto load_block = [&](int b) {            // global -> registers (slots past the sequence are never consumed)
#pragma unroll
        for (int e = 0; e < NIN; ++e) {
            const int idx = tid + e * LNT;
            const int sl = idx / IN4;
            const int c4 = idx - sl * IN4;
            const int sidx = b * TB + sl;
            stage[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (sl < TB && sidx < T) {
                const int t = dir ? T - 1 - sidx : sidx;
                stage[e] = *reinterpret_cast<const float4*>(gi + ((int64_t)t * rows + row) * (8 * LH) + dir * 4 * LH + 4 * c4);
            }
        }
    };
    auto stash_block = [&](int buf) {          // registers -> LDS
#pragma unroll
        for (int e = 0; e < NIN; ++e) {
            const int idx = tid + e * LNT;
            if (idx < TB * IN4) *reinterpret_cast<float4*>(&in_s[buf][0][0] + 4 * idx) = stage[e];
        }
    };
    auto flush_block = [&](int b) {            // LDS -> global
        for (int idx = tid; idx < TB * OUT4; idx += LNT) {
            const int sl = idx / OUT4;
            const int c4 = idx - sl * OUT4;
            const int sidx = b * TB + sl;
            if (sidx >= T) continue;
            const int t = dir ? T - 1 - sidx : sidx;
            const float4 v = *reinterpret_cast<const float4*>(&out_s[sl][4 * c4]);
            const int64_t o = (int64_t)t * rows + row;
            if (c4 < LH / 4)
                *reinterpret_cast<float4*>(y + o * (2 * LH) + dir * LH + 4 * c4) = v;
            else      // (saved for the backward pass only)
                __builtin_nontemporal_store(__builtin_bit_cast(f32x4, v),
                                            reinterpret_cast<f32x4*>(state + (o * 2 + dir) * (5 * LH) + 4 * (c4 - LH / 4)));
        }
    };

    for (int i = tid; i < 2 * (LH + 4); i += LNT) (&hs[0][0])[i] = 0.f;
    load_block(0);
    stash_block(0);
    if (nblocks > 1) load_block(1);
    __syncthreads();

    float cprev = 0.f;
    int step = 0;
    for (int b = 0; b < nblocks; ++b) {
        const int buf = b & 1;
        for (int sl = 0; sl < TB && step < T; ++sl, ++step) {
            const int cur = step & 1;
            const float* gp = &in_s[buf][sl][uu];
            const float gi_i = gp[0], gi_f = gp[LH], gi_g = gp[2 * LH], gi_o = gp[3 * LH];
            l32x2 ai0 = {0.f, 0.f}, af0 = {0.f, 0.f}, ag0 = {0.f, 0.f}, ao0 = {0.f, 0.f};
            l32x2 ai1 = {0.f, 0.f}, af1 = {0.f, 0.f}, ag1 = {0.f, 0.f}, ao1 = {0.f, 0.f};
            const float4* hv = reinterpret_cast<const float4*>(&hs[cur][kbase]);
#pragma unroll
            for (int k4 = 0; k4 < LKW / 4; ++k4) {
                // the second half has 12 real float4 (48 floats); its 13th reads the 4 zero pad floats against zero weights
                const float4 h4 = hv[k4];
                const l32x2 ha = {h4.x, h4.y}, hb = {h4.z, h4.w};
                ai0 = __builtin_elementwise_fma(wi[2 * k4], ha, ai0);
                af0 = __builtin_elementwise_fma(wf[2 * k4], ha, af0);
                ag0 = __builtin_elementwise_fma(wg[2 * k4], ha, ag0);
                ao0 = __builtin_elementwise_fma(wo[2 * k4], ha, ao0);
                ai1 = __builtin_elementwise_fma(wi[2 * k4 + 1], hb, ai1);
                af1 = __builtin_elementwise_fma(wf[2 * k4 + 1], hb, af1);
                ag1 = __builtin_elementwise_fma(wg[2 * k4 + 1], hb, ag1);
                ao1 = __builtin_elementwise_fma(wo[2 * k4 + 1], hb, ao1);
            }
            float ai = (ai0.x + ai0.y) + (ai1.x + ai1.y);
            float af = (af0.x + af0.y) + (af1.x + af1.y);
            float ag = (ag0.x + ag0.y) + (ag1.x + ag1.y);
            float ao = (ao0.x + ao0.y) + (ao1.x + ao1.y);
            ai += lstm_pair_swap(ai);
            af += lstm_pair_swap(af);
            ag += lstm_pair_swap(ag);
            ao += lstm_pair_swap(ao);
            // (every lane does the gate math: both lanes of a pair hold the same sums)
            const float ii = lstm_sigmoid((ai + bi) + gi_i);
            const float ff = lstm_sigmoid((af + bf) + gi_f);
            const float gg = lstm_tanh((ag + bg) + gi_g);
            const float oo = lstm_sigmoid((ao + bo) + gi_o);
            const float cc = ff * cprev + ii * gg;
            const float hh = oo * lstm_tanh(cc);
            cprev = cc;
            if (mine) {
                hs[cur ^ 1][u] = hh;
                float* op = &out_s[sl][u];
                op[0] = hh;
                op[LH] = ii;
                op[2 * LH] = ff;
                op[3 * LH] = gg;
                op[4 * LH] = oo;
                op[5 * LH] = cc;
            }
            __syncthreads();
        }
        // block boundary: the next block's operands (loaded a block ago) drop into LDS, this block's results leave, and the
        // loads of block b+2 are issued
        if (b + 1 < nblocks) stash_block(buf ^ 1);
        flush_block(b);
        if (b + 2 < nblocks) load_block(b + 2);
        __syncthreads();
    }
}

// Backward through time.  dh_prev[u] = dy_prev[u] + sum_j dgate[j] W_hh[j][u]: lane (u, half) keeps W_hh[j][u] for j in its
// half of the 4H gate rows ([0, 200) / [200, 400)); dgate of the step processed just before is broadcast from LDS.
// dy (T, rows, 2H);  y unused by the recurrence itself (the caller contracts it with dgate);  dgate (T, rows, 8H)
__global__ __launch_bounds__(LNT) void lstm_seq_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ state,
                                                            const float* __restrict__ w_f, const float* __restrict__ w_r,
                                                            float* __restrict__ dgate, const int rows, const int T) {
    constexpr int TB = LSTM_TB;
    constexpr int IN4 = 7 * LH / 4;     // staged per step: dy (H) | i f g o c (5 H) | c_prev (H)
    constexpr int OUT4 = 4 * LH / 4;    // dgate: di df dg do
    constexpr int NIN = (TB * IN4 + LNT - 1) / LNT;
    __shared__ __attribute__((aligned(16))) float dgs[2][4 * LH];
    __shared__ __attribute__((aligned(16))) float in_s[2][TB][7 * LH];
    __shared__ __attribute__((aligned(16))) float out_s[TB][4 * LH];

    const int tid = threadIdx.x;
    const int u = tid >> 1;
    const int half = tid & 1;
    const bool active = u < LH;
    const int uu = active ? u : LH - 1;
    const int jbase = half ? LJ0 : 0;
    const int dir = blockIdx.y;
    const int row = blockIdx.x;
    const float* __restrict__ w_hh = dir ? w_r : w_f;

    l32x2 w[LJW / 2];
#pragma unroll
    for (int j = 0; j < LJW; ++j) w[j >> 1][j & 1] = w_hh[(int64_t)(jbase + j) * LH + uu];
#pragma unroll
    for (int j = 0; j < LJW / 2; ++j) lstm_pin(w[j]);

    const bool mine = active && half == 0;
    // step index s runs in the REVERSE of the forward order: t(s) = dir ? s : T-1-s
    const int nblocks = (T + TB - 1) / TB;
    float4 stage[NIN];
    auto load_block = [&](int b) {
#pragma unroll
        for (int e = 0; e < NIN; ++e) {
            const int idx = tid + e * LNT;
            const int sl = idx / IN4;
            const int c4 = idx - sl * IN4;
            const int sidx = b * TB + sl;
            stage[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (sl < TB && sidx < T) {
                const int t = dir ? sidx : T - 1 - sidx;
                const int64_t o = (int64_t)t * rows + row;
                if (c4 < LH / 4) {
                    stage[e] = *reinterpret_cast<const float4*>(dy + o * (2 * LH) + dir * LH + 4 * c4);
                } else if (c4 < 6 * LH / 4) {
                    stage[e] = *reinterpret_cast<const float4*>(state + (o * 2 + dir) * (5 * LH) + 4 * (c4 - LH / 4));
                } else {
                    const int tp = dir ? t + 1 : t - 1;   // the step that produced c_prev in the forward pass (none: c = 0)
                    if (tp >= 0 && tp < T)
                        stage[e] = *reinterpret_cast<const float4*>(state + (((int64_t)tp * rows + row) * 2 + dir) * (5 * LH) +
                                                                    4 * LH + 4 * (c4 - 6 * LH / 4));
                }
            }
        }
    };
    auto stash_block = [&](int buf) {
#pragma unroll
        for (int e = 0; e < NIN; ++e) {
            const int idx = tid + e * LNT;
            if (idx < TB * IN4) *reinterpret_cast<float4*>(&in_s[buf][0][0] + 4 * idx) = stage[e];
        }
    };
    auto flush_block = [&](int b) {
        for (int idx = tid; idx < TB * OUT4; idx += LNT) {
            const int sl = idx / OUT4;
            const int c4 = idx - sl * OUT4;
            const int sidx = b * TB + sl;
            if (sidx >= T) continue;
            const int t = dir ? sidx : T - 1 - sidx;
            const float4 v = *reinterpret_cast<const float4*>(&out_s[sl][4 * c4]);
            *reinterpret_cast<float4*>(dgate + ((int64_t)t * rows + row) * (8 * LH) + dir * 4 * LH + 4 * c4) = v;
        }
    };

    for (int i = tid; i < 2 * 4 * LH; i += LNT) (&dgs[0][0])[i] = 0.f;
    load_block(0);
    stash_block(0);
    if (nblocks > 1) load_block(1);
    __syncthreads();

    float dc_carry = 0.f;
    int step = 0;
    for (int b = 0; b < nblocks; ++b) {
        const int buf = b & 1;
        for (int sl = 0; sl < TB && step < T; ++sl, ++step) {
            const int cur = step & 1;
            // recurrent contribution of the step processed just before (its dgate sits in dgs[cur ^ 1]; zeros at the first)
            l32x2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f}, a2 = {0.f, 0.f}, a3 = {0.f, 0.f};
            const float4* dv = reinterpret_cast<const float4*>(&dgs[cur ^ 1][jbase]);
#pragma unroll
            for (int j8 = 0; j8 < LJW / 8; ++j8) {
                const float4 d4 = dv[2 * j8], e4 = dv[2 * j8 + 1];
                const l32x2 da = {d4.x, d4.y}, db = {d4.z, d4.w}, dc2 = {e4.x, e4.y}, dd = {e4.z, e4.w};
                a0 = __builtin_elementwise_fma(w[4 * j8 + 0], da, a0);
                a1 = __builtin_elementwise_fma(w[4 * j8 + 1], db, a1);
                a2 = __builtin_elementwise_fma(w[4 * j8 + 2], dc2, a2);
                a3 = __builtin_elementwise_fma(w[4 * j8 + 3], dd, a3);
            }
            float rec = ((a0.x + a0.y) + (a1.x + a1.y)) + ((a2.x + a2.y) + (a3.x + a3.y));
            rec += lstm_pair_swap(rec);
            if (mine) {
                const float* ip = &in_s[buf][sl][u];
                const float dh = ip[0] + rec;
                const float ii = ip[LH], ff = ip[2 * LH], gg = ip[3 * LH], oo = ip[4 * LH], cc = ip[5 * LH], cp = ip[6 * LH];
                const float tc = lstm_tanh(cc);
                const float d_o = dh * tc * oo * (1.0f - oo);
                const float dc = dc_carry + dh * oo * (1.0f - tc * tc);
                const float d_i = dc * gg * ii * (1.0f - ii);
                const float d_f = dc * cp * ff * (1.0f - ff);
                const float d_g = dc * ii * (1.0f - gg * gg);
                dc_carry = dc * ff;
                float* op = &out_s[sl][u];
                op[0] = d_i;
                op[LH] = d_f;
                op[2 * LH] = d_g;
                op[3 * LH] = d_o;
                float* dp = &dgs[cur][u];
                dp[0] = d_i;
                dp[LH] = d_f;
                dp[2 * LH] = d_g;
                dp[3 * LH] = d_o;
            }
            __syncthreads();
        }
        if (b + 1 < nblocks) stash_block(buf ^ 1);
        flush_block(b);
        if (b + 2 < nblocks) load_block(b + 2);
        __syncthreads();
    }
}

}  // namespace

extern "C" int mmdfn_lstm_seq_block_steps(void) { return LSTM_TB; }

extern "C" int mmdfn_lstm_seq_fwd(const float* gi, const float* const* w_hh, const float* const* b_hh, float* y, float* state,
                                  int rows, int T, int H, void* stream) {
    if (H != LH || rows <= 0 || T <= 0) return -1;
    if (gi == nullptr || w_hh == nullptr || b_hh == nullptr || y == nullptr || state == nullptr) return -1;
    if (w_hh[0] == nullptr || w_hh[1] == nullptr || b_hh[0] == nullptr || b_hh[1] == nullptr) return -1;
    hipLaunchKernelGGL(lstm_seq_fwd_kernel, dim3(rows, 2), dim3(LNT), 0, (hipStream_t)stream, gi, w_hh[0], w_hh[1], b_hh[0],
                       b_hh[1], y, state, rows, T);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_lstm_seq_bwd(const float* dy, const float* y, const float* state, const float* const* w_hh, float* dgate,
                                  int rows, int T, int H, void* stream) {
    if (H != LH || rows <= 0 || T <= 0) return -1;
    if (dy == nullptr || y == nullptr || state == nullptr || w_hh == nullptr || dgate == nullptr) return -1;
    if (w_hh[0] == nullptr || w_hh[1] == nullptr) return -1;
    hipLaunchKernelGGL(lstm_seq_bwd_kernel, dim3(rows, 2), dim3(LNT), 0, (hipStream_t)stream, dy, state, w_hh[0], w_hh[1], dgate,
                       rows, T);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
