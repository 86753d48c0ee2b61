// K17: fused DialogueRNN recurrence (forward and backward through time) of the recurrent baseline ``DialogRNNModel``
// (reference model.py:168-278, 359-417: a Python loop over timesteps with three chained nn.GRUCell, an attention over the
// growing history of global states and a per-dialogue party select, run once per direction).
//
// Per chain (dialogue b, direction) and chain step s, with speaker = argmax qmask, m = qmask[speaker] (0 or 1):
//   g_s    = keep_g * GRU_g([U, q[speaker]], g_{s-1})          the DROPPED g_s is carried and joins the history
//   c_s    = sum_{j<s} alpha_sj g_j     alpha_s = softmax_j <x_s, g_j>    x_s = W_att U ('general') or w ('simple');  c_0 = 0
//   qs     = keep_q * GRU_p([U, c_s], q[speaker])
//   q[speaker] = m qs + (1 - m) q[speaker]
//   e_s    = keep_e * GRU_e(q[speaker], e_{s-1})                the dropped e_s is carried
// The U-dependent halves of the g / p input contractions (+ b_ih) and W_att U do not depend on the state: they arrive as
// projected rows ``pu`` (one dense launch outside this file).
//
// Mapping.  The state-side matrices of a step are 345 000 floats (1.38 MB): they fit neither the registers (512 KB) nor the LDS
// (160 KB) of a CU, so they are STREAMED from L2 on every step, and a workgroup can serve R (= DR) chains against one pass over
// them: every weight value fetched is used R times, the state vectors are broadcast from LDS.  Grid (ceil(B / R), 2),
// blockIdx.y = direction; a workgroup owns its chains for the whole sequence and is the only reader and writer of their rows,
// so __syncthreads() is the only ordering there is: no workgroup waits for another, no atomics, no spin loops; every loop is
// bounded by T, P or a dimension.  A chain of the reverse direction runs t = len-1 .. 0 and stops at its length.
//   forward : lane j of the workgroup owns gate row j (450 / 300 rows) and reads the k-major weight IMAGE (coalesced);
//   backward: lane (gate block, k) owns input column k for one gate block and reads the matrices as nn.GRUCell stores
//             them (row j, column k: coalesced over k); the three partial sums meet in LDS in a fixed order.
// A chain's arithmetic does not depend on its slot in the workgroup or on its neighbours; all reductions have a fixed order.
// Gate non-linearities are libm's (tanhf, expf with a true division) as in K16 (lstm_seq.hip), for the reason given there.
//
// Deliberately absent: the e cell as a recurrence of its own behind a batched input projection, a captured-graph step,
// the listener cell (listener_state=True), attention types other than 'simple' / 'general', MFMA forms.
#include "mmdfn_internal.h"
#include "../../include/mmdfn_hip.h"

namespace {

constexpr int DR = 1;            // chains per workgroup (R), chosen by measurement: profiles/dialog_rnn_model.md
constexpr int DNT = 512;
constexpr int DG = 150;          // D_g = D_p
constexpr int DE = 100;          // D_e
constexpr int DW = 152;          // row width of the saved planes (DG padded to a multiple of 4)
constexpr int G3 = 3 * DG;       // gate rows of the g / p cells
constexpr int E3 = 3 * DE;       // gate rows of the e cell
constexpr int GW = 452;          // row width of the gate-gradient planes (G3 padded to a multiple of 4)
constexpr int NPL = 17;          // saved planes per direction
constexpr int NDG = 6;           // gate-gradient planes per direction
constexpr int PMAX = 16;
constexpr int TMAX = 1008;
// planes
enum { P_RG, P_ZG, P_NG, P_HNG, P_G, P_RP, P_ZP, P_NP, P_HNP, P_Q0, P_Q1, P_C, P_RE, P_ZE, P_NE, P_HNE, P_E };
// forward weight image (floats)
constexpr int OFF_GQ = 0;                    // (150, 450)  W_ih_g[:, D_m:]^T
constexpr int OFF_GH = OFF_GQ + DG * G3;     // (150, 450)  W_hh_g^T
constexpr int OFF_PC = OFF_GH + DG * G3;     // (150, 450)  W_ih_p[:, D_m:]^T
constexpr int OFF_PH = OFF_PC + DG * G3;     // (150, 450)  W_hh_p^T
constexpr int OFF_EI = OFF_PH + DG * G3;     // (150, 300)  W_ih_e^T
constexpr int OFF_EH = OFF_EI + DG * E3;     // (100, 300)  W_hh_e^T
constexpr int OFF_BG = OFF_EH + DE * E3;     // b_hh_g (450)
constexpr int OFF_BP = OFF_BG + G3;          // b_hh_p (450)
constexpr int OFF_BEI = OFF_BP + G3;         // b_ih_e (300)
constexpr int OFF_BEH = OFF_BEI + E3;        // b_hh_e (300)
constexpr int OFF_W = OFF_BEH + E3;          // SimpleAttention.scalar.weight (150, + 2 zeros)
constexpr int IMG = OFF_W + DW;

__device__ __forceinline__ float drnn_sigmoid(float x) { return sigmoid_exact(x); }
__device__ __forceinline__ float drnn_tanh(float x) { return tanhf(x); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

struct DrnnFwd {
    const float* pu[2];
    const float* img[2];
    const int* speaker;
    const float* upd;
    const int* lengths;
    const float* keep_g[2];
    const float* keep_q[2];
    const float* keep_e[2];
    float scale;
    float* e_out;
    float* alpha;
    float* state;
    int B, T, P, npu, att;
};

struct DrnnBwd {
    const float* de_out;
    const float* pu[2];
    const float* img[2];
    const float* w[2][6];       // gq gh pc ph ei eh as the modules store them (row j, column k), with row strides ld[]
    int ld[6];
    const int* speaker;
    const float* upd;
    const int* lengths;
    const float* keep_g[2];
    const float* keep_q[2];
    const float* keep_e[2];
    float scale;
    const float* alpha;
    const float* state;
    float* dgate;
    float* dpu[2];
    float* dghist;
    float* dw_part;
    int B, T, P, npu, att;
};

extern __shared__ __attribute__((aligned(16))) float drnn_lds[];

__device__ __forceinline__ int64_t plane_row(int dir, int plane, int s, int b, int T, int B) {
    return ((((int64_t)dir * NPL + plane) * T + s) * B + b) * DW;
}
__device__ __forceinline__ int64_t dgate_row(int dir, int plane, int s, int b, int T, int B) {
    return ((((int64_t)dir * NDG + plane) * T + s) * B + b) * GW;
}

// per-step bookkeeping of the workgroup's chains
struct ChainMeta {
    int len[DR], t[DR], spk[DR];
    float m[DR];
};

__device__ __forceinline__ int chain_len(const int* lengths, int b, int B, int T, int dir) {
    if (b >= B) return 0;
    if (!dir) return T;
    const int l = lengths[b];
    return l < 0 ? 0 : (l > T ? T : l);
}

// y_i[r][j] = sum_k Wi[k][j] xi[r][k],  y_h[r][j] = sum_k Wh[k][j] xh[r][k]  for the gate row j of this lane (k-major images).
// The step is bound by the latency of the weight stream, not its volume: DRNN_UNROLL requests per stream are in flight at once.
#define DRNN_UNROLL 10      /* divides 150 and 100 */
template <int NJ>
__device__ __forceinline__ void contract1(const float* __restrict__ w, const int kn, const float* x, const int j, float (&acc)[DR]) {
#pragma unroll
    for (int r = 0; r < DR; ++r) acc[r] = 0.f;
#pragma unroll 1
    for (int k0 = 0; k0 < kn; k0 += DRNN_UNROLL) {
        float wv[DRNN_UNROLL];
#pragma unroll
        for (int i = 0; i < DRNN_UNROLL; ++i) wv[i] = w[(k0 + i) * NJ + j];
#pragma unroll
        for (int i = 0; i < DRNN_UNROLL; ++i)
#pragma unroll
            for (int r = 0; r < DR; ++r) acc[r] = fmaf(wv[i], x[r * DW + k0 + i], acc[r]);
    }
}
template <int NJ>
__device__ __forceinline__ void contract2(const float* __restrict__ wi, const int ki, const float* xi, const float* __restrict__ wh,
                                          const int kh, const float* xh, const int j, float (&ai)[DR], float (&ah)[DR]) {
    if (ki != kh) {
        contract1<NJ>(wi, ki, xi, j, ai);
        contract1<NJ>(wh, kh, xh, j, ah);
        return;
    }
#pragma unroll
    for (int r = 0; r < DR; ++r) ai[r] = ah[r] = 0.f;
#pragma unroll 1
    for (int k0 = 0; k0 < ki; k0 += DRNN_UNROLL) {       // both streams in one loop: twice the requests in flight
        float wa[DRNN_UNROLL], wb[DRNN_UNROLL];
#pragma unroll
        for (int i = 0; i < DRNN_UNROLL; ++i) {
            wa[i] = wi[(k0 + i) * NJ + j];
            wb[i] = wh[(k0 + i) * NJ + j];
        }
#pragma unroll
        for (int i = 0; i < DRNN_UNROLL; ++i)
#pragma unroll
            for (int r = 0; r < DR; ++r) {
                ai[r] = fmaf(wa[i], xi[r * DW + k0 + i], ai[r]);
                ah[r] = fmaf(wb[i], xh[r * DW + k0 + i], ah[r]);
            }
    }
}

__global__ __launch_bounds__(DNT) void drnn_seq_fwd_kernel(const DrnnFwd a) {
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * DR;
    const int B = a.B, T = a.T, P = a.P;
    const int Tp = (T + 3) & ~3;
    float* q_s = drnn_lds;                 // [R][P][DW] party states
    float* g_s = q_s + DR * P * DW;        // [R][DW] carried g
    float* e_s = g_s + DR * DW;            // [R][DW] carried e
    float* c_s = e_s + DR * DW;
    float* x_s = c_s + DR * DW;            // score vector
    float* q0_s = x_s + DR * DW;
    float* q1_s = q0_s + DR * DW;
    float* pi_s = q1_s + DR * DW;          // [R][GW] input-side pre-activations
    float* ph_s = pi_s + DR * GW;          // [R][GW] hidden-side pre-activations
    float* sc_s = ph_s + DR * GW;          // [R][Tp] scores, then alpha
    __shared__ ChainMeta cm;

    const float* __restrict__ img = a.img[dir];
    const float* __restrict__ pu = a.pu[dir];
    const float* kg = a.keep_g[dir];
    const float* kq = a.keep_q[dir];
    const float* ke = a.keep_e[dir];
    const float* gplane = a.state + plane_row(dir, P_G, 0, 0, T, B);      // history: rows (j, b)

    for (int i = tid; i < DR * P * DW + 2 * DR * DW; i += DNT) q_s[i] = 0.f;       // q, g, e
    int nsteps = 0;
    if (tid < DR) cm.len[tid] = chain_len(a.lengths, b0 + tid, B, T, dir);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < DR; ++r) nsteps = max(nsteps, cm.len[r]);

    for (int s = 0; s < nsteps; ++s) {
        if (tid < DR) {
            const int r = tid;
            const int len = cm.len[r];
            int t = 0, spk = 0;
            float m = 0.f;
            if (s < len) {
                t = dir ? len - 1 - s : s;
                spk = a.speaker[(int64_t)t * B + b0 + r];
                spk = spk < 0 ? 0 : (spk >= P ? P - 1 : spk);
                m = a.upd[(int64_t)t * B + b0 + r];
            }
            cm.t[r] = t;
            cm.spk[r] = spk;
            cm.m[r] = m;
        }
        __syncthreads();
        for (int i = tid; i < DR * DW; i += DNT) {
            const int r = i / DW, d = i - r * DW;
            float x = 0.f;
            if (d < DG && s < cm.len[r])
                x = a.att ? pu[((int64_t)cm.t[r] * B + b0 + r) * a.npu + 2 * G3 + d] : img[OFF_W + d];
            x_s[i] = x;
            q0_s[i] = q_s[(r * P + cm.spk[r]) * DW + d];
        }
        __syncthreads();
        // ---- g cell contraction, scores over the history
        if (tid < G3) {
            float ai[DR], ah[DR];
            contract2<G3>(img + OFF_GQ, DG, q0_s, img + OFF_GH, DG, g_s, tid, ai, ah);
            const float bh = img[OFF_BG + tid];
#pragma unroll
            for (int r = 0; r < DR; ++r) {
                float in = 0.f;
                if (s < cm.len[r]) in = pu[((int64_t)cm.t[r] * B + b0 + r) * a.npu + tid];
                pi_s[r * GW + tid] = ai[r] + in;
                ph_s[r * GW + tid] = ah[r] + bh;
            }
        }
        for (int pr = wave; pr < DR * s; pr += DNT / 64) {
            const int r = pr % DR, j = pr / DR;
            if (s >= cm.len[r]) continue;
            const float* gj = gplane + ((int64_t)j * B + b0 + r) * DW;
            float v = 0.f;
            for (int d = lane; d < DG; d += 64) v = fmaf(x_s[r * DW + d], gj[d], v);
            v = wave_sum(v);
            if (lane == 0) sc_s[r * Tp + j] = v;
        }
        __syncthreads();
        // ---- g gates; softmax of the scores (max subtracted: they are unbounded)
        for (int i = tid; i < DR * DG; i += DNT) {
            const int r = i / DG, u = i - r * DG;
            if (s >= cm.len[r]) continue;
            const float* pi = pi_s + r * GW;
            const float* ph = ph_s + r * GW;
            const float rr = drnn_sigmoid(pi[u] + ph[u]);
            const float zz = drnn_sigmoid(pi[DG + u] + ph[DG + u]);
            const float hn = ph[2 * DG + u];
            const float nn = drnn_tanh(pi[2 * DG + u] + rr * hn);
            float gn = (1.0f - zz) * nn + zz * g_s[r * DW + u];
            if (kg) gn *= kg[((int64_t)s * B + b0 + r) * DG + u] * a.scale;
            g_s[r * DW + u] = gn;
            float* st = a.state + plane_row(dir, 0, s, b0 + r, T, B) + u;
            const int64_t ps = (int64_t)T * B * DW;
            st[P_RG * ps] = rr;
            st[P_ZG * ps] = zz;
            st[P_NG * ps] = nn;
            st[P_HNG * ps] = hn;
            st[P_G * ps] = gn;
        }
        if (wave < DR && s > 0 && s < cm.len[wave]) {
            const int r = wave;
            float* sc = sc_s + r * Tp;
            float mx = -INFINITY;
            for (int j = lane; j < s; j += 64) mx = fmaxf(mx, sc[j]);
            mx = wave_max(mx);
            float sum = 0.f;
            for (int j = lane; j < s; j += 64) {
                const float ex = expf(sc[j] - mx);
                sc[j] = ex;
                sum += ex;
            }
            sum = wave_sum(sum);
            float* al = a.alpha + (((int64_t)dir * T + s) * B + b0 + r) * T;
            for (int j = lane; j < s; j += 64) {
                const float v = sc[j] / sum;
                sc[j] = v;
                al[j] = v;
            }
        }
        __syncthreads();
        // ---- pool (history excludes g_s: rows j < s, written in earlier steps)
        for (int i = tid; i < DR * DG; i += DNT) {
            const int r = i / DG, d = i - r * DG;
            if (s >= cm.len[r]) continue;
            float c = 0.f;
            const float* gj = gplane + (int64_t)(b0 + r) * DW + d;
            const float* al = sc_s + r * Tp;
            for (int j = 0; j < s; ++j) c = fmaf(al[j], gj[(int64_t)j * B * DW], c);
            c_s[r * DW + d] = c;
            a.state[plane_row(dir, P_C, s, b0 + r, T, B) + d] = c;
        }
        __syncthreads();
        // ---- p cell
        if (tid < G3) {
            float ai[DR], ah[DR];
            contract2<G3>(img + OFF_PC, DG, c_s, img + OFF_PH, DG, q0_s, tid, ai, ah);
            const float bh = img[OFF_BP + tid];
#pragma unroll
            for (int r = 0; r < DR; ++r) {
                float in = 0.f;
                if (s < cm.len[r]) in = pu[((int64_t)cm.t[r] * B + b0 + r) * a.npu + G3 + tid];
                pi_s[r * GW + tid] = ai[r] + in;
                ph_s[r * GW + tid] = ah[r] + bh;
            }
        }
        __syncthreads();
        for (int i = tid; i < DR * DG; i += DNT) {
            const int r = i / DG, u = i - r * DG;
            if (s >= cm.len[r]) continue;
            const float* pi = pi_s + r * GW;
            const float* ph = ph_s + r * GW;
            const float rr = drnn_sigmoid(pi[u] + ph[u]);
            const float zz = drnn_sigmoid(pi[DG + u] + ph[DG + u]);
            const float hn = ph[2 * DG + u];
            const float nn = drnn_tanh(pi[2 * DG + u] + rr * hn);
            const float q0 = q0_s[r * DW + u];
            float qs = (1.0f - zz) * nn + zz * q0;
            if (kq) qs *= kq[((int64_t)s * B + b0 + r) * DG + u] * a.scale;
            const float m = cm.m[r];
            const float q1 = m * qs + (1.0f - m) * q0;
            q1_s[r * DW + u] = q1;
            q_s[(r * P + cm.spk[r]) * DW + u] = q1;
            float* st = a.state + plane_row(dir, 0, s, b0 + r, T, B) + u;
            const int64_t ps = (int64_t)T * B * DW;
            st[P_RP * ps] = rr;
            st[P_ZP * ps] = zz;
            st[P_NP * ps] = nn;
            st[P_HNP * ps] = hn;
            st[P_Q0 * ps] = q0;
            st[P_Q1 * ps] = q1;
        }
        __syncthreads();
        // ---- e cell
        if (tid < E3) {
            float ai[DR], ah[DR];
            contract2<E3>(img + OFF_EI, DG, q1_s, img + OFF_EH, DE, e_s, tid, ai, ah);
            const float bi = img[OFF_BEI + tid], bh = img[OFF_BEH + tid];
#pragma unroll
            for (int r = 0; r < DR; ++r) {
                pi_s[r * GW + tid] = ai[r] + bi;
                ph_s[r * GW + tid] = ah[r] + bh;
            }
        }
        __syncthreads();
        for (int i = tid; i < DR * DE; i += DNT) {
            const int r = i / DE, u = i - r * DE;
            if (s >= cm.len[r]) continue;
            const float* pi = pi_s + r * GW;
            const float* ph = ph_s + r * GW;
            const float rr = drnn_sigmoid(pi[u] + ph[u]);
            const float zz = drnn_sigmoid(pi[DE + u] + ph[DE + u]);
            const float hn = ph[2 * DE + u];
            const float nn = drnn_tanh(pi[2 * DE + u] + rr * hn);
            float en = (1.0f - zz) * nn + zz * e_s[r * DW + u];
            if (ke) en *= ke[((int64_t)s * B + b0 + r) * DE + u] * a.scale;
            e_s[r * DW + u] = en;
            float* st = a.state + plane_row(dir, 0, s, b0 + r, T, B) + u;
            const int64_t ps = (int64_t)T * B * DW;
            st[P_RE * ps] = rr;
            st[P_ZE * ps] = zz;
            st[P_NE * ps] = nn;
            st[P_HNE * ps] = hn;
            st[P_E * ps] = en;
            a.e_out[(((int64_t)dir * T + cm.t[r]) * B + b0 + r) * DE + u] = en;
        }
        __syncthreads();
    }
}

// GRU cell backward at one unit: dh (gradient of the cell's output) -> gate-gradient entries and the direct part of dh_prev
struct GateGrad {
    float dr, dz, dni, dnh, dh_direct;
};
__device__ __forceinline__ GateGrad gru_gate_grad(float dh, float r, float z, float n, float hn, float hprev) {
    GateGrad o;
    const float dnp = dh * (1.0f - z) * (1.0f - n * n);
    o.dz = dh * (hprev - n) * z * (1.0f - z);
    o.dr = dnp * hn * r * (1.0f - r);
    o.dni = dnp;
    o.dnh = dnp * r;
    o.dh_direct = dh * z;
    return o;
}

// part[blk][r][k] = sum_{j in gate block blk} d[r][blk * NB + j] W[(blk * NB + j) * ld + k]
template <int NB>
__device__ __forceinline__ void contract_t(const float* __restrict__ w, const int ld, const float* d_s, float* part_s, const int blk,
                                           const int k) {
    float acc[DR];
#pragma unroll
    for (int r = 0; r < DR; ++r) acc[r] = 0.f;
    const float* wp = w + (int64_t)blk * NB * ld + k;
    const float* dp = d_s + blk * NB;
#pragma unroll 1
    for (int j0 = 0; j0 < NB; j0 += DRNN_UNROLL) {
        float wv[DRNN_UNROLL];
#pragma unroll
        for (int i = 0; i < DRNN_UNROLL; ++i) wv[i] = wp[(int64_t)(j0 + i) * ld];
#pragma unroll
        for (int i = 0; i < DRNN_UNROLL; ++i)
#pragma unroll
            for (int r = 0; r < DR; ++r) acc[r] = fmaf(wv[i], dp[r * GW + j0 + i], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < DR; ++r) part_s[(blk * DR + r) * DW + k] = acc[r];
}

__global__ __launch_bounds__(DNT) void drnn_seq_bwd_kernel(const DrnnBwd a) {
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * DR;
    const int B = a.B, T = a.T, P = a.P;
    const int Tp = (T + 3) & ~3;
    float* dq_s = drnn_lds;                 // [R][P][DW] carried party-state gradients
    float* dg_s = dq_s + DR * P * DW;       // [R][DW] carried dg (hidden side of the next step's g cell)
    float* de_s = dg_s + DR * DW;           // [R][DW] carried de
    float* dwa_s = de_s + DR * DW;          // [R][DW] 'simple': running dw of the chain
    float* dq0_s = dwa_s + DR * DW;
    float* dc_s = dq0_s + DR * DW;
    float* x_s = dc_s + DR * DW;
    float* pa_s = x_s + DR * DW;            // [3][R][DW] partial sums per gate block
    float* pb_s = pa_s + 3 * DR * DW;       // [3][R][DW]
    float* di_s = pb_s + 3 * DR * DW;       // [R][GW] input-side gate gradients
    float* dh_s = di_s + DR * GW;           // [R][GW] hidden-side gate gradients
    float* al_s = dh_s + DR * GW;           // [R][Tp] alpha
    float* da_s = al_s + DR * Tp;           // [R][Tp] dalpha, then dscore
    __shared__ ChainMeta cm;

    const float* __restrict__ pu = a.pu[dir];
    const float* __restrict__ img = a.img[dir];
    const float* kg = a.keep_g[dir];
    const float* kq = a.keep_q[dir];
    const float* ke = a.keep_e[dir];
    float* dpu = a.dpu[dir];
    const int64_t ps = (int64_t)T * B * DW;     // plane stride
    const int64_t gs = (int64_t)T * B * GW;     // gate-gradient plane stride
    const float* gplane = a.state + plane_row(dir, P_G, 0, 0, T, B);
    float* dgh = a.dghist + (int64_t)dir * T * B * DW;

    for (int i = tid; i < DR * P * DW + 3 * DR * DW; i += DNT) dq_s[i] = 0.f;      // dq, dg, de, dw
    int nsteps = 0;
    if (tid < DR) cm.len[tid] = chain_len(a.lengths, b0 + tid, B, T, dir);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < DR; ++r) nsteps = max(nsteps, cm.len[r]);

    for (int s = nsteps - 1; s >= 0; --s) {
        if (tid < DR) {
            const int r = tid;
            const int len = cm.len[r];
            int t = 0, spk = 0;
            float m = 0.f;
            if (s < len) {
                t = dir ? len - 1 - s : s;
                spk = a.speaker[(int64_t)t * B + b0 + r];
                spk = spk < 0 ? 0 : (spk >= P ? P - 1 : spk);
                m = a.upd[(int64_t)t * B + b0 + r];
            }
            cm.t[r] = t;
            cm.spk[r] = spk;
            cm.m[r] = m;
        }
        __syncthreads();
        // ---- e cell gates
        for (int i = tid; i < DR * DE; i += DNT) {
            const int r = i / DE, u = i - r * DE;
            float* di = di_s + r * GW;
            float* dh = dh_s + r * GW;
            if (s >= cm.len[r]) {
                di[u] = di[DE + u] = di[2 * DE + u] = 0.f;
                dh[u] = dh[DE + u] = dh[2 * DE + u] = 0.f;
                continue;
            }
            const int b = b0 + r;
            float d = a.de_out[(((int64_t)dir * T + cm.t[r]) * B + b) * DE + u] + de_s[r * DW + u];
            if (ke) d *= ke[((int64_t)s * B + b) * DE + u] * a.scale;
            const float* st = a.state + plane_row(dir, 0, s, b, T, B) + u;
            const float hp = s > 0 ? a.state[plane_row(dir, P_E, s - 1, b, T, B) + u] : 0.f;
            const GateGrad g = gru_gate_grad(d, st[P_RE * ps], st[P_ZE * ps], st[P_NE * ps], st[P_HNE * ps], hp);
            di[u] = g.dr;
            di[DE + u] = g.dz;
            di[2 * DE + u] = g.dni;
            dh[u] = g.dr;
            dh[DE + u] = g.dz;
            dh[2 * DE + u] = g.dnh;
            float* o = a.dgate + dgate_row(dir, 4, s, b, T, B) + u;
            o[0] = g.dr;
            o[DE] = g.dz;
            o[2 * DE] = g.dni;
            o[gs] = g.dr;
            o[gs + DE] = g.dz;
            o[gs + 2 * DE] = g.dnh;
            de_s[r * DW + u] = g.dh_direct;
        }
        __syncthreads();
        if (tid < 3 * DG) contract_t<DE>(a.w[dir][4], a.ld[4], di_s, pa_s, tid / DG, tid % DG);
        if (tid < 3 * DE) contract_t<DE>(a.w[dir][5], a.ld[5], dh_s, pb_s, tid / DE, tid % DE);
        __syncthreads();
        // ---- p cell gates
        for (int i = tid; i < DR * DG; i += DNT) {
            const int r = i / DG, u = i - r * DG;
            float* di = di_s + r * GW;
            float* dh = dh_s + r * GW;
            if (s >= cm.len[r]) {
                di[u] = di[DG + u] = di[2 * DG + u] = 0.f;
                dh[u] = dh[DG + u] = dh[2 * DG + u] = 0.f;
                continue;
            }
            const int b = b0 + r;
            const int o3 = r * DW + u;
            if (u < DE) de_s[o3] += (pb_s[o3] + pb_s[DR * DW + o3]) + pb_s[2 * DR * DW + o3];
            const float dq1 = ((pa_s[o3] + pa_s[DR * DW + o3]) + pa_s[2 * DR * DW + o3]) + dq_s[(r * P + cm.spk[r]) * DW + u];
            const float m = cm.m[r];
            float dqs = m * dq1;
            if (kq) dqs *= kq[((int64_t)s * B + b) * DG + u] * a.scale;
            const float* st = a.state + plane_row(dir, 0, s, b, T, B) + u;
            const GateGrad g = gru_gate_grad(dqs, st[P_RP * ps], st[P_ZP * ps], st[P_NP * ps], st[P_HNP * ps], st[P_Q0 * ps]);
            di[u] = g.dr;
            di[DG + u] = g.dz;
            di[2 * DG + u] = g.dni;
            dh[u] = g.dr;
            dh[DG + u] = g.dz;
            dh[2 * DG + u] = g.dnh;
            float* o = a.dgate + dgate_row(dir, 2, s, b, T, B) + u;
            o[0] = g.dr;
            o[DG] = g.dz;
            o[2 * DG] = g.dni;
            o[gs] = g.dr;
            o[gs + DG] = g.dz;
            o[gs + 2 * DG] = g.dnh;
            float* dp = dpu + ((int64_t)cm.t[r] * B + b) * a.npu + G3 + u;
            dp[0] = g.dr;
            dp[DG] = g.dz;
            dp[2 * DG] = g.dni;
            dq0_s[o3] = (1.0f - m) * dq1 + g.dh_direct;
        }
        __syncthreads();
        if (tid < 3 * DG) {
            contract_t<DG>(a.w[dir][2], a.ld[2], di_s, pa_s, tid / DG, tid % DG);     // -> dc
            contract_t<DG>(a.w[dir][3], a.ld[3], dh_s, pb_s, tid / DG, tid % DG);     // -> dq0
        }
        __syncthreads();
        for (int i = tid; i < DR * DW; i += DNT) {
            const int r = i / DW, d = i - r * DW;
            float x = 0.f, dc = 0.f;
            if (d < DG && s < cm.len[r]) {
                x = a.att ? pu[((int64_t)cm.t[r] * B + b0 + r) * a.npu + 2 * G3 + d] : img[OFF_W + d];
                dc = (pa_s[i] + pa_s[DR * DW + i]) + pa_s[2 * DR * DW + i];
                dq0_s[i] += (pb_s[i] + pb_s[DR * DW + i]) + pb_s[2 * DR * DW + i];
            }
            x_s[i] = x;
            dc_s[i] = dc;
        }
        __syncthreads();
        // ---- attention of step s: c = sum_j alpha_j g_j over j < s
        for (int pr = wave; pr < DR * s; pr += DNT / 64) {
            const int r = pr % DR, j = pr / DR;
            if (s >= cm.len[r]) continue;
            const float* gj = gplane + ((int64_t)j * B + b0 + r) * DW;
            float v = 0.f;
            for (int d = lane; d < DG; d += 64) v = fmaf(dc_s[r * DW + d], gj[d], v);
            v = wave_sum(v);
            if (lane == 0) {
                da_s[r * Tp + j] = v;
                al_s[r * Tp + j] = a.alpha[(((int64_t)dir * T + s) * B + b0 + r) * T + j];
            }
        }
        __syncthreads();
        if (wave < DR && s > 0 && s < cm.len[wave]) {
            const int r = wave;
            float dot = 0.f;
            for (int j = lane; j < s; j += 64) dot = fmaf(al_s[r * Tp + j], da_s[r * Tp + j], dot);
            dot = wave_sum(dot);
            for (int j = lane; j < s; j += 64) da_s[r * Tp + j] = al_s[r * Tp + j] * (da_s[r * Tp + j] - dot);
        }
        __syncthreads();
        for (int i = tid; i < DR * DG; i += DNT) {
            const int r = i / DG, d = i - r * DG;
            if (s >= cm.len[r] || s == 0) continue;
            const int b = b0 + r;
            const float dc = dc_s[r * DW + d], x = x_s[r * DW + d];
            float dx = 0.f;
            for (int j = 0; j < s; ++j) {
                const int64_t o = ((int64_t)j * B + b) * DW + d;
                const float ds = da_s[r * Tp + j];
                dx = fmaf(ds, gplane[o], dx);
                dgh[o] += al_s[r * Tp + j] * dc + ds * x;
            }
            if (a.att)
                dpu[((int64_t)cm.t[r] * B + b) * a.npu + 2 * G3 + d] = dx;
            else
                dwa_s[r * DW + d] += dx;
        }
        __syncthreads();
        // ---- g cell gates
        for (int i = tid; i < DR * DG; i += DNT) {
            const int r = i / DG, u = i - r * DG;
            float* di = di_s + r * GW;
            float* dh = dh_s + r * GW;
            if (s >= cm.len[r]) {
                di[u] = di[DG + u] = di[2 * DG + u] = 0.f;
                dh[u] = dh[DG + u] = dh[2 * DG + u] = 0.f;
                continue;
            }
            const int b = b0 + r;
            float d = dg_s[r * DW + u] + dgh[((int64_t)s * B + b) * DW + u];
            if (kg) d *= kg[((int64_t)s * B + b) * DG + u] * a.scale;
            const float* st = a.state + plane_row(dir, 0, s, b, T, B) + u;
            const float hp = s > 0 ? gplane[((int64_t)(s - 1) * B + b) * DW + u] : 0.f;
            const GateGrad g = gru_gate_grad(d, st[P_RG * ps], st[P_ZG * ps], st[P_NG * ps], st[P_HNG * ps], hp);
            di[u] = g.dr;
            di[DG + u] = g.dz;
            di[2 * DG + u] = g.dni;
            dh[u] = g.dr;
            dh[DG + u] = g.dz;
            dh[2 * DG + u] = g.dnh;
            float* o = a.dgate + dgate_row(dir, 0, s, b, T, B) + u;
            o[0] = g.dr;
            o[DG] = g.dz;
            o[2 * DG] = g.dni;
            o[gs] = g.dr;
            o[gs + DG] = g.dz;
            o[gs + 2 * DG] = g.dnh;
            float* dp = dpu + ((int64_t)cm.t[r] * B + b) * a.npu + u;
            dp[0] = g.dr;
            dp[DG] = g.dz;
            dp[2 * DG] = g.dni;
            dg_s[r * DW + u] = g.dh_direct;
        }
        __syncthreads();
        if (tid < 3 * DG) {
            contract_t<DG>(a.w[dir][0], a.ld[0], di_s, pa_s, tid / DG, tid % DG);     // -> dq0
            contract_t<DG>(a.w[dir][1], a.ld[1], dh_s, pb_s, tid / DG, tid % DG);     // -> dg
        }
        __syncthreads();
        for (int i = tid; i < DR * DG; i += DNT) {
            const int r = i / DG, d = i - r * DG;
            if (s >= cm.len[r]) continue;
            const int o3 = r * DW + d;
            dq_s[(r * P + cm.spk[r]) * DW + d] = dq0_s[o3] + ((pa_s[o3] + pa_s[DR * DW + o3]) + pa_s[2 * DR * DW + o3]);
            dg_s[o3] += (pb_s[o3] + pb_s[DR * DW + o3]) + pb_s[2 * DR * DW + o3];
        }
        __syncthreads();
    }
    if (a.dw_part != nullptr)
        for (int i = tid; i < DR * DW; i += DNT) {
            const int r = i / DW, d = i - r * DW;
            if (b0 + r < B) a.dw_part[((int64_t)dir * B + b0 + r) * DW + d] = dwa_s[i];
        }
}

bool drnn_served(int B, int T, int P, int Dg, int Dp, int De, int npu, int att) {
    return B > 0 && T > 0 && T <= TMAX && P > 0 && P <= PMAX && Dg == DG && Dp == DG && De == DE && (att == 0 || att == 1) &&
           npu == 2 * G3 + (att ? DG : 0);
}

}  // namespace

extern "C" int mmdfn_drnn_chains_per_group(void) { return DR; }

extern "C" int64_t mmdfn_drnn_image_floats(void) { return IMG; }

extern "C" int mmdfn_drnn_seq_fwd(const float* const* pu, const float* const* img, const int32_t* speaker, const float* upd,
                                  const int32_t* lengths, const float* const* keep_g, const float* const* keep_q,
                                  const float* const* keep_e, float keep_scale, float* e_out, float* alpha, float* state, int B,
                                  int T, int P, int Dg, int Dp, int De, int npu, int att, int ndir, void* stream) {
    if (!drnn_served(B, T, P, Dg, Dp, De, npu, att) || ndir < 1 || ndir > 2) return -1;
    if (pu == nullptr || img == nullptr || speaker == nullptr || upd == nullptr || lengths == nullptr || e_out == nullptr ||
        alpha == nullptr || state == nullptr)
        return -1;
    for (int d = 0; d < ndir; ++d)
        if (pu[d] == nullptr || img[d] == nullptr) return -1;
    DrnnFwd a;
    for (int i = 0; i < 2; ++i) {
        const int d = i < ndir ? i : 0;       // (the arrays hold ndir entries)
        a.pu[i] = pu[d];
        a.img[i] = img[d];
        a.keep_g[i] = keep_g ? keep_g[d] : nullptr;
        a.keep_q[i] = keep_q ? keep_q[d] : nullptr;
        a.keep_e[i] = keep_e ? keep_e[d] : nullptr;
    }
    a.speaker = speaker;
    a.upd = upd;
    a.lengths = lengths;
    a.scale = keep_scale;
    a.e_out = e_out;
    a.alpha = alpha;
    a.state = state;
    a.B = B;
    a.T = T;
    a.P = P;
    a.npu = npu;
    a.att = att;
    const int Tp = (T + 3) & ~3;
    const size_t lds = sizeof(float) * ((size_t)DR * P * DW + 6 * DR * DW + 2 * DR * GW + (size_t)DR * Tp);
    const int rc = mmdfn_allow_big_lds(drnn_seq_fwd_kernel);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(drnn_seq_fwd_kernel, dim3((B + DR - 1) / DR, ndir), dim3(DNT), lds, (hipStream_t)stream, a);
    MMDFN_CHECK_LAUNCH();
    return 0;
}

extern "C" int mmdfn_drnn_seq_bwd(const float* de_out, const float* const* pu, const float* const* img, const float* const* w,
                                  const int32_t* ld, const int32_t* speaker, const float* upd, const int32_t* lengths,
                                  const float* const* keep_g, const float* const* keep_q, const float* const* keep_e,
                                  float keep_scale, const float* alpha, const float* state, float* dgate, float* const* dpu,
                                  float* dghist, float* dw_part, int B, int T, int P, int Dg, int Dp, int De, int npu, int att,
                                  int ndir, void* stream) {
    if (!drnn_served(B, T, P, Dg, Dp, De, npu, att) || ndir < 1 || ndir > 2) return -1;
    if (de_out == nullptr || pu == nullptr || img == nullptr || w == nullptr || ld == nullptr || speaker == nullptr ||
        upd == nullptr || lengths == nullptr || alpha == nullptr || state == nullptr || dgate == nullptr || dpu == nullptr ||
        dghist == nullptr || (att == 0 && dw_part == nullptr))
        return -1;
    for (int d = 0; d < ndir; ++d)
        if (pu[d] == nullptr || img[d] == nullptr || dpu[d] == nullptr) return -1;
    static const int min_ld[6] = {DG, DG, DG, DG, DG, DE};
    for (int i = 0; i < 6 * ndir; ++i)
        if (w[i] == nullptr) return -1;
    for (int i = 0; i < 6; ++i)
        if (ld[i] < min_ld[i]) return -1;
    DrnnBwd a;
    for (int k = 0; k < 2; ++k) {
        const int d = k < ndir ? k : 0;       // (the arrays hold ndir entries)
        a.pu[k] = pu[d];
        a.img[k] = img[d];
        a.dpu[k] = dpu[d];
        a.keep_g[k] = keep_g ? keep_g[d] : nullptr;
        a.keep_q[k] = keep_q ? keep_q[d] : nullptr;
        a.keep_e[k] = keep_e ? keep_e[d] : nullptr;
        for (int i = 0; i < 6; ++i) a.w[k][i] = w[d * 6 + i];
    }
    for (int i = 0; i < 6; ++i) a.ld[i] = ld[i];
    a.de_out = de_out;
    a.speaker = speaker;
    a.upd = upd;
    a.lengths = lengths;
    a.scale = keep_scale;
    a.alpha = alpha;
    a.state = state;
    a.dgate = dgate;
    a.dghist = dghist;
    a.dw_part = att ? nullptr : dw_part;
    a.B = B;
    a.T = T;
    a.P = P;
    a.npu = npu;
    a.att = att;
    const int Tp = (T + 3) & ~3;
    const size_t lds = sizeof(float) * ((size_t)DR * P * DW + 6 * DR * DW + 6 * DR * DW + 2 * DR * GW + 2 * (size_t)DR * Tp);
    const int rc = mmdfn_allow_big_lds(drnn_seq_bwd_kernel);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(drnn_seq_bwd_kernel, dim3((B + DR - 1) / DR, ndir), dim3(DNT), lds, (hipStream_t)stream, a);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
