/*
 * mmdfn_hip.h -- C ABI of libmmdfn_hip.so: the MI355X (gfx950) kernels behind
 * the MM-DFN graph dynamic-fusion hot path.
 *
 * The reference (zerohd4869/MM-DFN) has no FFI layer: its "operators" are
 * torch ops called from nn.Module.forward.  Each entry point below replaces
 * the reference call site cited next to it; the Python host side
 * (the mm_dfn_amd Python package) binds them with ctypes and keeps the reference's
 * nn.Module signatures (see INTEGRATION.md for the stub a maintainer adds).
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (the PyTorch
 *     caching allocator); kernels never allocate or free.  The one exception
 *     is `riders`, a HOST rider context (see mmdfn_riders_bytes);
 *   - fp32 row-major contiguous data, int32 / int64 index arrays;
 *   - asynchronous enqueue on `stream` (a hipStream_t passed as void*), no
 *     internal synchronisation, no global state, re-entrant;
 *   - return value 0 = success, otherwise a hipError_t (or -1 for an invalid
 *     argument); nothing throws across the ABI.
 *
 * Dialogue layout shared by the graph kernels ("block-tile adjacency"):
 *   B dialogues of lengths dia_len[i]; row_start[i] = sum_{j<i} dia_len[j]
 *   (B+1 entries, row_start[B] = N).  M modalities.  Node (m, r) of the
 *   multimodal dialogue graph is row m*N + r of every (M*N, d) feature matrix
 *   (the reference's cat([a, v, l], 0) order, model_mm.py:98).
 *   The normalised adjacency is never materialised densely; it is stored as
 *     tiles : for dialogue i, modality m a dia_len[i] x dia_len[i] fp32 tile,
 *             row-major with leading dimension ld_i = round_up(dia_len[i], 4),
 *             at float offset tile_base[i] + m * dia_len[i] * ld_i
 *             (tile_base: B+1 int64 entries, multiples of 4); pad columns are 0;
 *     cross : for each unordered modality pair (m<n), in lexicographic order,
 *             N fp32 values: entry r is A[(m,r),(n,r)] = A[(n,r),(m,r)].
 */
#ifndef MMDFN_HIP_H
#define MMDFN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Rider context: HOST memory of mmdfn_riders_bytes() bytes, owned by the caller; all-zero bytes = empty.  Work staged in it
 * (mmdfn_wgrad_riders_stage, mmdfn_keep_flags_stage) is taken only by a launch given the same context; the library never
 * allocates, frees or keeps a pointer to it beyond a call.  NULL wherever a `riders` argument is taken = no riders: nothing is
 * staged, a GRU launch takes nothing, a weight-gradient batch merges nothing. */
int64_t mmdfn_riders_bytes(void);

/* Library / device sanity: returns the ABI version (currently 23: 22 + the graph kind of the adjacency build mmdfn_adj_build_kind,
 * mmdfn_adj_build_bwd_kind, and -- an addition that moves no existing symbol, so 23 also carries it -- the key-band builder of the
 * sparse graphs mmdfn_adj_build_band; 22 = 21 + FlatAdam on device-resident step state mmdfn_adam_state_bytes, mmdfn_grad_sumsq,
 * mmdfn_adam_prepare, mmdfn_adam_step_state; 21 = 20 + the TFN tensor-fusion kernels mmdfn_tfn_{workspace,fwd,bwd_input,bwd_weight,keep_flags};
 * 20 = 19 + mmdfn_linear_planes_group_in (input dropout in the
 * plane projection's staging step), mmdfn_linear_planes_group_party (party-ordered store) and mmdfn_linear_group_seg2 (two K segments per few-row problem); 19 = 18 + the head without its ReLU mmdfn_head_{fwd,bwd,bwd_partial}_act
 * and the LMF fusion kernels mmdfn_lmf_{fwd,bwd,bwd_width}; 18 = 17 with the rider hand-off made explicit -- the rider context
 * `riders` (mmdfn_riders_bytes) is an argument of mmdfn_wgrad_riders_{stage,staged,flush,drain}, mmdfn_keep_flags_{stage,flush},
 * mmdfn_gru_seq_{fwd,bwd} and mmdfn_gemm_tn_batch / _ext; 17 = 16 + the GRU backward launch's weight-gradient riders mmdfn_wgrad_riders_{stage,staged,flush,drain}, mmdfn_gru_seq_bwd_idle_cus, mmdfn_gru_seq_bwd_step_ns, and the dropout-flag draw as a rider of the GRU forward launch mmdfn_keep_flags_{stage,flush}, mmdfn_gru_seq_fwd_takes_flags; 16 = 15 + mmdfn_linear_planes_group, mmdfn_party_gather_bwd_colsum, mmdfn_party_combine_bwd_dst, mmdfn_prop_layer_fwd; 15 = 14 + mmdfn_weight_planes_workspace, mmdfn_cut_weight_planes, mmdfn_linear_planes; 14 = 13 + mmdfn_lstm_gate_{planes_workspace,cut_weights,fwd_pre,takes_planes}; 13 = 12 + mmdfn_gemm_tn_batch_ext, mmdfn_head_bwd_partial / _groups, mmdfn_colsum_partial; 12 = 11 + the segmented GRU recurrence mmdfn_gru_seq_{fwd,bwd}_seg, mmdfn_gru_tab_reduce, the strided forms mmdfn_lstm_gate_fwd_ld, mmdfn_gcnii_layer_bwd_ld, mmdfn_focal_loss_{fwd,bwd}_ignore and mmdfn_focal_loss_fwd_grad). */
int mmdfn_abi_version(void);

/* ---------------------------------------------------------------------------
 * K6  scatter-propagate  out = A_hat . H        (replaces torch.spmm(adj, input),
 *                                                model_GCN.py:178)
 *   out[(m,r),:] = sum_q tile_{i,m}[r,q] * H[(m,q),:] + sum_{n!=m} cross_{mn}[r] * H[(n,r),:]
 *   transpose != 0 uses tile^T (for dH = A^T . dO when tiles are not symmetric).
 *   H, out: M*N rows of d fp32 with row strides ldh / ldo floats (>= d, multiples of 4, so a
 *   column slice of a wider matrix can be read or written in place); d % 4 == 0.
 *   max_len = max_i dia_len[i].
 * ------------------------------------------------------------------------- */
int mmdfn_propagate(const float* tiles, const float* cross, const float* H, float* out,
                    const int32_t* dia_len, const int32_t* row_start, const int64_t* tile_base,
                    int B, int M, int N, int d, int ldh, int ldo, int max_len, int transpose,
                    void* stream);

/* ---------------------------------------------------------------------------
 * K6 backward w.r.t. the adjacency, restricted to the stored pattern
 * (autograd of model_GCN.py:178 w.r.t. adj; the reference gets a dense
 * (MN x MN) gradient from SpmmBackward):
 *   dtiles_{i,m}[p,q] (+)= X[(m,p),:] . Y[(m,q),:]
 *   dcross_{mn}[r]    (+)= X[(m,r),:].Y[(n,r),:] + X[(n,r),:].Y[(m,r),:]
 *   with X = dOut, Y = H (row strides ldx / ldy floats).  accumulate != 0 adds into dtiles/dcross.
 *   Any d % 4 == 0 (wide d runs on the bf16-piece kernel); the adjacency build below needs D <= 512.
 * ------------------------------------------------------------------------- */
int mmdfn_tile_outer(const float* X, const float* Y, float* dtiles, float* dcross,
                     const int32_t* dia_len, const int32_t* row_start, const int64_t* tile_base,
                     int B, int M, int N, int d, int ldx, int ldy, int max_len, int accumulate,
                     void* stream);

/* ---------------------------------------------------------------------------
 * K5  adjacency build (replaces MM_GCN.create_big_adj, model_mm.py:122-180)
 *   feats  : (M, N, D) fp32 (modality-major stack of the encoder outputs)
 *   unit   : (M, N, D) out, x / ||x||              (saved for backward)
 *   norm   : (M, N)    out, ||x||
 *   cosg   : tile-shaped out, raw cosine Gram G    (saved for backward)
 *   cdot   : (npairs, N) out, raw cross cosines    (saved for backward)
 *   rdeg   : (M, N)    out, degree^-1/2
 *   tiles, cross : the normalised adjacency (layout above)
 *   sim(c) = 1 - acos(0.99999 c)/pi ; cross entries are scaled by modal_weight.
 * ------------------------------------------------------------------------- */
int mmdfn_adj_build(const float* feats, float* unit, float* norm, float* cosg, float* cdot,
                    float* rdeg, float* tiles, float* cross,
                    const int32_t* dia_len, const int32_t* row_start, const int64_t* tile_base,
                    int B, int M, int N, int D, int max_len, float modal_weight, void* stream);

/* Backward of mmdfn_adj_build: given dtiles / dcross (gradients of the stored
 * entries) produce dfeats (M, N, D).  `wsym` (tile-shaped), `etile`
 * (tile-shaped), `ecross` (npairs, N), `ddeg` (M, N) and `dunit` (M, N, D) are
 * caller-provided scratch.  * addend (mmdfn_adj_build_bwd, may be NULL): (M, N, D) gradient reaching the same features on another path (they are
 *   also the input of the GCN stack); dfeats = adjacency gradient + addend, so no separate accumulation launch runs.
 */
int mmdfn_adj_build_bwd(const float* dtiles, const float* dcross,
                        const float* unit, const float* norm, const float* cosg, const float* cdot,
                        const float* rdeg, const float* tiles, const float* cross,
                        float* wsym, float* etile, float* ecross, float* ddeg, float* dunit,
                        float* dfeats, const float* addend,
                        const int32_t* dia_len, const int32_t* row_start, const int64_t* tile_base,
                        int B, int M, int N, int D, int max_len, float modal_weight, void* stream);

/* ---------------------------------------------------------------------------
 * K5 with the graph kind as an argument (ABI 23).  Same operands, layouts and scratch as mmdfn_adj_build /
 * mmdfn_adj_build_bwd; forward and backward of one tensor set take the same kind.
 *   kind 0 : the angular-similarity graph above -- mmdfn_adj_build / _bwd are these calls with kind 0.
 *   kind 1 : the arccos-distance graph of the MMGCN baseline (MM_GCN2.create_big_adj, model_mm.py:241-296) and of
 *            GCNII_lyc without an adjacency (message_passing_wo_speaker, model_GCN.py:490-511, the M = 1 case):
 *              within a modality   A[(m,p),(m,q)] = acos(0.99999 cos(x_mp, x_mq))   (radians, diagonal included:
 *                                  cos(x, x) is taken as the constant 1 there, cosg holds 1, no gradient flows through it)
 *              between modalities  A[(m,r),(n,r)] = c, a constant: the `modal_weight` slot carries c
 *              (MM_GCN2 passes 0.99999); degree = row sum, A_hat = D^-1/2 A D^-1/2 as for kind 0.
 *            cdot is written as zeros (no cross cosine is formed).  Backward: the constant entries reach the
 *            features through the degrees only, so dcross contributes to d(degree) and ecross is written as zeros.
 *   any other kind returns -1.
 * ------------------------------------------------------------------------- */
int mmdfn_adj_build_kind(const float* feats, float* unit, float* norm, float* cosg, float* cdot,
                         float* rdeg, float* tiles, float* cross,
                         const int32_t* dia_len, const int32_t* row_start, const int64_t* tile_base,
                         int B, int M, int N, int D, int max_len, float modal_weight, int kind, void* stream);

int mmdfn_adj_build_bwd_kind(const float* dtiles, const float* dcross,
                             const float* unit, const float* norm, const float* cosg, const float* cdot,
                             const float* rdeg, const float* tiles, const float* cross,
                             float* wsym, float* etile, float* ecross, float* ddeg, float* dunit,
                             float* dfeats, const float* addend,
                             const int32_t* dia_len, const int32_t* row_start, const int64_t* tile_base,
                             int B, int M, int N, int D, int max_len, float modal_weight, int kind, void* stream);

/* ---------------------------------------------------------------------------
 * K5b  the sparse unimodal graphs of GCNII / GCNII_lyc with new_graph=True (csrc/adjacency_band.hip): the context window
 * of message_passing_relation_graph (model_GCN.py:381-409, :556-584) and the speaker chains of
 * message_passing_directed_speaker (model_GCN.py:348-379, :523-554).  Forward only: the reference takes every edge weight
 * through math.acos on a Python float, so the graph is a constant for autograd.
 *   feats : (N, D) fp32, D % 4 == 0;  M must be 1
 *   keys  : (N) int32, one per row: rank in the low 24 bits, chain in the bits above (key = chain << 24 | rank, both >= 0).
 *           Rows p != q of ONE dialogue are joined iff chain_p == chain_q and |rank_p - rank_q| <= width.
 *             window graph   : chain 0, rank = position in the dialogue, width 20 (the union of the reference's
 *                              [k - 10, k + 10] cliques)
 *             speaker chains : chain 0 where qmask[i][j][0] == 1, chain 1 otherwise; rank = index inside the chain; width 1
 *   on an edge  S[p,q] = 1 - acos(c) / pi,  c = x_p.x_q / (||x_p|| ||x_q||) clamped to [-1, 1], taken as 0 when either norm is
 *               0 (weight 0.5; no x / 0 is formed); there is no 0.99999 shrink
 *   S[p,p] = 1 (a constant, not a dot product), S = 0 elsewhere;  degree = row sum of S (>= 1)
 *   deg   : (N) scratch, the degrees;  rdeg : (N) out, degree^-1/2 (always finite)
 *   tiles : out, (r_p S[p,q]) r_q in the block-tile layout above as DENSE dia_len[i] x ld_i tiles: entries that are no
 *           edge and the pad columns are written as exact 0.0f.  Dot products are formed for the pairs of the predicate
 *           only: O(N width D) work.  There are no cross diagonals (M = 1).
 *   Returns -1 before any launch for width < 0, M != 1, D % 4 != 0, non-positive sizes or a null pointer.
 * ------------------------------------------------------------------------- */
int mmdfn_adj_build_band(const float* feats, const int32_t* keys, float* deg, float* rdeg, float* tiles,
                         const int32_t* dia_len, const int32_t* row_start, const int64_t* tile_base,
                         int B, int M, int N, int D, int max_len, int width, void* stream);

/* ---------------------------------------------------------------------------
 * K2  fused GRU recurrence (replaces the time loop inside nn.GRU for ``lstm_l``
 * and ``rnn_parties``: model.py:866,868, called at :1082,1112,1132,1145).
 * One layer, both directions, `ngroups` independent GRUs in one launch
 * (host arrays of device pointers, one entry per group; ngroups <= 4):
 *   gi[g]    : (T, rows, 2, 3H)  X W_ih^T + b_ih for both directions (dir-major columns)
 *   w_hh[2g + dir] : (3H, H), b_hh[2g + dir] : (3H)  per direction, exactly as nn.GRU stores
 *              weight_hh_l*[_reverse] / bias_hh_l*[_reverse] (arrays of 2*ngroups pointers); gate order r, z, n
 *   y[g]     : (T, rows, 2H) out; direction 1 runs t = T-1 .. 0; zero initial state
 *   gates[g] : (T, rows, 2, 4, H) out: r, z, n and W_hn h + b_hn (saved for backward)
 * H must be 100 (the reference hard-codes D_e = 100).
 * ------------------------------------------------------------------------- */
int mmdfn_gru_seq_fwd(int ngroups, const float* const* gi, const float* const* w_hh,
                      const float* const* b_hh, float* const* y, float* const* gates,
                      const int* rows, const int* T, int H, void* riders, void* stream);

/* Backward through time of the same recurrence: given dy[g] (T, rows, 2H) writes
 *   dgi[g], dgh[g] : (T, rows, 2, 3H)  gradients of the input-side / hidden-side gate
 *   pre-activations (they differ only in the n gate: dgh_n = dgi_n * r).
 * Weight gradients are dense contractions of these done by the caller. */
int mmdfn_gru_seq_bwd(int ngroups, const float* const* dy, const float* const* y,
                      const float* const* gates, const float* const* w_hh,
                      float* const* dgi, float* const* dgh,
                      const int* rows, const int* T, int H, void* riders, void* stream);

/* Valid-length ("segmented") form of the same recurrence for the speaker-party batch (model.py:1076-1087: per dialogue b and
 * speaker p the reference fills rows [:k_bp] of a zero (L, H) buffer, runs the party GRU over all L steps and scatters rows
 * [:k_bp] back).  Exact work removal, see csrc/gru.hip "Valid-length truncation".  Per group g (host arrays, one entry per group):
 *   rank[g]  : the gather's (T, BP) int32 rank array (>= 0 where speaker p talks) or NULL (every row runs all T steps);
 *              rows[g] must be a multiple of BP[g] (one (B, P) block per gathered modality), P[g] <= 16, P[g] * T[g] <= 2048
 *   tdir[g]  : -1, or the direction that stops at / starts from the valid length: its P sequences per (modality, dialogue)
 *              run back to back in one workgroup.  Rows with k = 0 are skipped in BOTH directions.
 *   ytab[g]  : NULL, or (tdir[g] must be 1) the (T, 1, 2H) outputs of the all-padding sequence (gi = b_ih at every step, run
 *              through mmdfn_gru_seq_fwd as a one-row group): a truncated reverse row starts at t = k - 1 from ytab[k] and
 *              its outputs at t >= k are copies of ytab[t]; with NULL a truncated row starts from 0 and y[t >= k] = 0.
 * Positions never visited hold ytab copies / zeros in y and are NOT written in gates.
 * Backward: dgi / dgh are zero at the positions never visited; with dhinit[g] (rows, H) and kout[g] (rows) int32 given
 * (tdir[g] == 1) the gradient wrt every truncated row's start state and its step count are written, and
 * mmdfn_gru_tab_reduce sums what reaches the all-padding sequence:
 *   dyt[t][dir half] = sum_{rows: k <= t} dy[t][row] + sum_{rows: k == t >= 1} dhinit[row]   (the other half zero),
 * the dy of that one-row group's own mmdfn_gru_seq_bwd. */
int mmdfn_gru_seq_fwd_seg(int ngroups, const float* const* gi, const float* const* w_hh,
                          const float* const* b_hh, float* const* y, float* const* gates,
                          const int* rows, const int* T, int H, const int32_t* const* rank, const int* P,
                          const int* BP, const int* tdir, const float* const* ytab, void* stream);
int mmdfn_gru_seq_bwd_seg(int ngroups, const float* const* dy, const float* const* y,
                          const float* const* gates, const float* const* w_hh,
                          float* const* dgi, float* const* dgh, const int* rows, const int* T, int H,
                          const int32_t* const* rank, const int* P, const int* BP, const int* tdir,
                          float* const* dhinit, int32_t* const* kout, void* stream);
int mmdfn_gru_tab_reduce(const float* dy, const int32_t* kout, const float* dhinit, float* dyt, int rows, int T,
                         int H, int dir, void* stream);

/* ---------------------------------------------------------------------------
 * K8  LSTM-cell gate math of the "reasoning" / dynamic-fusion module (replaces the pointwise part
 * of nn.LSTM with seq_len 1, model_GCN.py:433,466; gate order i, f, g, o):
 *   G (R, 4H) = x W_ih^T + b_ih + h W_hh^T + b_hh   (dense contractions done by the caller)
 *   c = sig(f) c_prev + sig(i) tanh(g) ;  h = sig(o) tanh(c).   c_prev may be NULL (zero state).
 * Backward: dG (R, 4H), dc_prev (R, H) from dh, dc_next (either may be NULL = zero).
 * ------------------------------------------------------------------------- */
int mmdfn_lstm_pointwise_fwd(const float* G, const float* c_prev, float* h_out, float* c_out,
                             int64_t R, int H, void* stream);
int mmdfn_lstm_pointwise_bwd(const float* G, const float* c_prev, const float* c_new,
                             const float* dh, const float* dc_next, float* dG, float* dc_prev,
                             int64_t R, int H, void* stream);

/* ---------------------------------------------------------------------------
 * K7  GCNII update (replaces model_GCN.py:179-186 variant branch + :469-472):
 *   S2 (R, 2d) = [A.x | h0],  P (R, d) = S2 . W  (contraction done by the caller)
 *   out = relu(theta P + (1-theta)((1-alpha) A.x + alpha h0)) * mask + q
 *   mask (dropout keep-mask already scaled by 1/(1-p)) and q may be NULL.
 * Backward: dP (R, d) and dS2 (R, 2d) from dout (dq = dout is the caller's).
 * ------------------------------------------------------------------------- */
int mmdfn_gcnii_combine_fwd(const float* P, const float* S2, const float* q, const float* mask,
                            float* out, float theta, float alpha, int64_t R, int d, void* stream);
int mmdfn_gcnii_combine_bwd(const float* P, const float* S2, const float* mask, const float* dout,
                            float* dP, float* dS2, float theta, float alpha, int64_t R, int d,
                            void* stream);

/* ---------------------------------------------------------------------------
 * K3 / K4  speaker-party gather / scatter + pad strip (replaces the per-(dialogue, speaker) Python
 * slice-assign loops model.py:1076-1087 (x3 modalities) and simple_batch_graphify model.py:553-565).
 *   X[m]   : Mn host-array entries, each a device (L, B, H) fp32 projection (Mn <= 4)
 *   qmask  : (L, B, P) fp32 speaker flags (non-zero = speaker p utters t in dialogue b)
 *   S      : (L, Mn*B*P, H) out: column ((m*B+b)*P+p) holds speaker p's utterances of dialogue b
 *            compacted to the front in time order, zero rows behind (the party-GRU input)
 *   bias   : NULL, or H floats added to EVERY row of S.  With it the gather can run after a bias-free projection
 *            (gather(X) W^T + b == gather(X W^T) + b, padding rows = b): the input contraction of the first party-GRU
 *            layer then runs over the L*B real utterances instead of the L*P*B mostly-zero party rows
 *   rank   : (L, B, P) int32 out: position of utterance t inside its party sequence, -1 otherwise
 * combine: out[m][n][:] = base[m][t,b,:] + weights[m] * E[rank[t,b,p*], ((m*B+b)*P+p*), :]
 *   with flat_idx[n] = t*B + b (dialogue-major order), p* = LAST flagged speaker (the reference
 *   scatters speaker by speaker), E = party-GRU output or NULL; out: (Mn, N, H).  E holds ONE column block per
 *   modality whose weight is non-zero, in modality order: (L, nact*B*P, H), column ((slot(m)*B+b)*P+p) with
 *   slot(m) = #{m' < m : weights[m'] != 0}.  (The reference also encodes the zero-weight modality and multiplies the
 *   result by 0, model.py:1121; that block is never needed.)
 *   `weights` is a HOST array of Mn floats (speaker_weights, model.py:816).
 * Backward entries: dX / dbase are Mn host-array entries of device (L, B, H) buffers;
 *   combine_bwd expects dbase and dE pre-zeroed (it writes only the rows that exist).
 *   gather_bwd: `addend` (NULL, or Mn entries each NULL or an (L, B, H) buffer) is added to dX -- the gradient that
 *   reaches X_m as the base of the combine stage, so that no separate accumulation launch is needed.
 * ------------------------------------------------------------------------- */
int mmdfn_party_gather(int Mn, const float* const* X, const float* qmask, const float* bias, float* S,
                       int32_t* rank, int L, int B, int P, int H, void* stream);
int mmdfn_party_gather_bwd(int Mn, const float* dS, const int32_t* rank, float* const* dX,
                           const float* const* addend, int L, int B, int P, int H, void* stream);
/* ABI 16: mmdfn_party_gather_bwd and mmdfn_colsum_partial of the SAME dS (viewed as (L Mn B P) x H; the party GRU's bias
 * gradient, model.py:1082) in one launch; returns the number of [H] slabs written to `workspace` (mmdfn_colsum_workspace(H)
 * floats) for mmdfn_gemm_tn_batch_ext to sum, negative = rejected. */
int mmdfn_party_gather_bwd_colsum(int Mn, const float* dS, const int32_t* rank, float* const* dX,
                                  const float* const* addend, int L, int B, int P, int H, float* workspace, void* stream);

/* Column sums out[c] = sum_r A[r][c] of an (R, H) matrix (row stride lda; H, lda % 4 == 0, 16-byte aligned), bit-reproducible
 * (slab partial sums + a small final launch): the bias gradient of gate pre-activations gathered after a bias-free
 * projection (replaces the autograd `sum` of the broadcast bias add, model.py:1082).
 * workspace: mmdfn_colsum_workspace(H) floats. */
/* Dropout keep flags (replaces the generator launch behind F.dropout / nn.Dropout / nn.GRU(dropout=p), model.py:866,868,1328,
 * model_GCN.py:453-470): out[i] = 1.0f with probability `keep`, else 0.0f, n % 4 == 0, 16-byte aligned; Philox4x32-10 keyed by
 * state[0] (seed) at counter state[1] + i / 8 (16 random bits per flag: the rate is exact to 2^-16).  `state`: three 64-bit words
 * in DEVICE memory (seed, offset, 0); the launch adds ceil(n / 8) rounded up to a multiple of 64 to the offset itself, so replays of a captured graph draw fresh flags. */
int mmdfn_keep_flags(float* out, int64_t n, float keep, void* state, void* stream);
/* The same draw as a RIDER of the first GRU layer's forward recurrence launch.  mmdfn_keep_flags_stage takes the arguments of
 * mmdfn_keep_flags and stages the draw in `riders` instead of launching it (a second staged draw, or riders = NULL: launched at
 * once); a mmdfn_gru_seq_fwd launch given the same context, of the kind mmdfn_gru_seq_fwd_takes_flags answers 1 for (fewer
 * workgroups than CUs), runs the draw as extra workgroups on the CUs the recurrence leaves idle -- the same flags bit for bit
 * (which counter yields which flag depends on neither the grid nor the block size); mmdfn_keep_flags_flush launches a draw that
 * is still staged.  The flags must not be read
 * before the launch that carries them (their first consumer in the reference is the dropout behind that GRU layer,
 * model.py:866). */
int mmdfn_keep_flags_stage(float* out, int64_t n, float keep, void* state, void* riders, void* stream);
int mmdfn_keep_flags_flush(void* riders, void* stream);
int mmdfn_gru_seq_fwd_takes_flags(int ngroups, const int* rows);
int64_t mmdfn_colsum_workspace(int H);
int mmdfn_colsum(const float* A, int64_t R, int H, int lda, float* out, float* workspace, void* stream);
/* The first launch of mmdfn_colsum alone (ABI 13): returns the number (> 0) of [H] slabs left in `workspace` for
 * mmdfn_gemm_tn_batch_ext to sum (ext_N = 0, ext_M = H), negative = rejected. */
int mmdfn_colsum_partial(const float* A, int64_t R, int H, int lda, float* workspace, void* stream);
int mmdfn_party_combine(int Mn, const float* const* base, const float* E, const int32_t* rank,
                        const int64_t* flat_idx, float* out, const float* weights,
                        int L, int B, int P, int N, int H, void* stream);
int mmdfn_party_combine_bwd(int Mn, const float* dout, const int32_t* rank, const int64_t* flat_idx,
                            float* const* dbase, float* dE, const float* weights,
                            int L, int B, int P, int N, int H, void* stream);
/* ABI 16: the same gradients written destination by destination -- dbase / dE need NOT be zeroed by the caller (its fill was a
 * launch of its own).  inv: (L * B) int64, the row of (t, b) in the stripped order or -1 (the inverse of flat_idx).
 * Returns -2 when the shape is not covered (L > 2048): use mmdfn_party_combine_bwd on pre-zeroed buffers. */
int mmdfn_party_combine_bwd_dst(int Mn, const float* dout, const int32_t* rank, const int64_t* inv, float* const* dbase,
                                float* dE, const float* weights, int L, int B, int P, int N, int H, void* stream);


/* ---------------------------------------------------------------------------
 * Dropout as a multiply by precomputed keep flags, several tensors per launch (the inter-layer dropout of
 * nn.GRU(num_layers=2, dropout=p) for the context and the party encoder, model.py:866,868, one launch each way):
 *   out[g][i] = x[g][i] * mask[g][i] * scale,  i < n[g]   (n[g] % 4 == 0, 16-byte aligned buffers, ngroups <= 4).
 * The backward pass is the same call on the incoming gradients.  x, mask, out: HOST arrays of device pointers.
 * ------------------------------------------------------------------------- */
int mmdfn_mask_scale(int ngroups, const float* const* x, const float* const* mask, float* const* out,
                     const int64_t* n, float scale, void* stream);

/* ---------------------------------------------------------------------------
 * K1  dense projection, fp32 in / fp32 out (replaces nn.Linear / F.linear / torch.mm on the hot path:
 * model.py:1065,1094,1129; the hoisted nn.GRU input contraction; model_GCN.py:454,466,186):
 *   Y[r, n] = act( sum_k X[r, k] W[n, k] + bias[n] ) (+ Y[r, n] if accumulate)
 *   X: R rows of K floats, row stride ldx; W: (N, K) contiguous (nn.Linear layout); bias: N or NULL;
 *   Y: R rows of N floats, row stride ldy.  act: 0 = identity, 1 = ReLU.  K % 4 == 0, ldx % 4 == 0.
 *   With both, the activation comes after the addend: Y = act(X W^T + bias + Y) (mmdfn_linear_group* likewise).
 * Arithmetic: exact-f32 MFMA (v_mfma_f32_16x16x4_f32); launches with >= 256 output tiles of 128 x 128 run on the
 * bf16 matrix path with every fp32 operand cut exactly into three bf16 pieces and six piece products per MAC
 * (fp32-level error, < 2e-6 relative to max|Y| on the tested shapes; the same scheme serves K6 / K6' on dialogues
 * of >= 128 utterances).
 * ------------------------------------------------------------------------- */
int mmdfn_linear(const float* X, const float* W, const float* bias, float* Y, int R, int K, int N,
                 int ldx, int ldy, int act, int accumulate, void* stream);
/* The same projection with the weight rows given as TWO blocks: output columns [0, N1) use W (N1, K) / bias,
 * columns [N1, N) use W2 (N - N1, K) / bias2.  A bidirectional nn.GRU layer keeps one weight_ih / bias_ih
 * parameter per direction (model.py:866,868); the hoisted input contraction of both directions runs as one
 * launch on the parameters themselves, without a concatenated copy per step.  N1 == N: W2 / bias2 unused. */
int mmdfn_linear2(const float* X, const float* W, const float* W2, int N1, const float* bias, const float* bias2,
                  float* Y, int R, int K, int N, int ldx, int ldy, int act, int accumulate, void* stream);

/* ---------------------------------------------------------------------------
 * K1p  the same projection against a weight that arrives as bf16 PIECE PLANES (linear_planes.hip; ABI 15).
 * Replaces the `nn.GRU` input products of `lstm_l` / `rnn_parties` (reference model.py:866,868,1082,1132) and their input
 * gradients at the row counts of the BASELINE configs.  A weight changes once per optimizer step
 * (run_train_erc.py:512), so its three exact bf16 pieces are cut once per step -- one grouped launch for up to 16 weights --
 * into MFMA B-fragment order, and the projection kernel cuts only its own X rows.
 *
 * mmdfn_weight_planes_workspace: bytes of the plane buffer of a B operand with N output columns and K contraction
 *   (ceil(N/32) x ceil(K/16) x 3 pieces x 1 KB; zero-filled outside N x K by the cut).
 * mmdfn_cut_weight_planes: weight i is given as up to two fp32 matrices w1[i] / w2[i] of row stride ld[i] (w2 may be null) and a
 *   mode[i] that says how the B operand (N[i] output columns, K[i] contraction) is read from them:
 *     0  B[n][k] = stored[n][k], the stored rows split at n1[i] (rows [0, n1) in w1, the rest in w2): a forward product against
 *        the two directions' own parameters;
 *     1  B[n][k] = stored[k][n], the stored rows (= k) split at n1[i]: the input gradient dX = dY . W on the same parameters
 *        (and y = x W for a weight stored (K, N): GraphConvolution.weight, model_GCN.py:172);
 *     2  B[n][k] = w1[k][n] for n < n1[i], w2[k][n - n1] beyond: two (K, .) matrices side by side, transposed;
 *     3  as 2 with the contraction index gate-interleaved, k = 4 u + g  <->  stored row g (K / 4) + u ([W_ih | W_hh] of an LSTM
 *        cell, K = 4H; used by the stack-kernel experiment under tools/gcn_planes/).
 *   planes[i]: 16-byte aligned, mmdfn_weight_planes_workspace(N[i], K[i]) bytes.
 * mmdfn_linear_planes:  Y = act(X B^T + bias) (+ Y);  X: R rows of K floats (row stride ldx, 16-byte aligned rows, K % 4 == 0),
 *   bias / bias2 split at n1 as in mmdfn_linear2 (either may be null), Y: R x N (row stride ldy), act: 0 identity, 1 ReLU.
 *   Arithmetic: six bf16 piece products per MAC, fp32 accumulation -- fp32-level error, as mmdfn_linear's many-row form.
 * mmdfn_linear_planes_group (ABI 16): n <= 4 such products in ONE launch (problem i: X[i], planes[i], ... as above; bias / bias2
 *   may be null arrays; R[i] == 0 skips a problem) -- the hoisted input contractions of the context and the party GRU of one
 *   layer (model.py:866-868, 1082, 1132) and their input gradients, which do not depend on each other.  Every problem keeps the
 *   tile form it takes alone, so its results are the bits of its own mmdfn_linear_planes launch.  mask (may be null, entries may
 *   be null): R[i] x N[i] keep flags (0 / 1, contiguous); Y_i is multiplied by mask_i * mask_scale after the activation -- the
 *   backward of the dropout between the GRU layers (nn.GRU(dropout=), model.py:866) folded into the input gradient's epilogue.
 * ------------------------------------------------------------------------- */
int64_t mmdfn_weight_planes_workspace(int N, int K);
int mmdfn_cut_weight_planes(int n, const float* const* w1, const float* const* w2, const int* n1, const int* ld,
                            const int* N, const int* K, const int* mode, void* const* planes, void* stream);
int mmdfn_linear_planes(const float* X, const void* planes, const float* bias, const float* bias2, int n1, float* Y, int R,
                        int K, int N, int ldx, int ldy, int act, int accumulate, void* stream);
int mmdfn_linear_planes_group(int n, const float* const* X, const void* const* planes, const float* const* bias,
                              const float* const* bias2, const int* n1, float* const* Y, const int* R, const int* K,
                              const int* N, const int* ldx, const int* ldy, int act, int accumulate,
                              const float* const* mask, float mask_scale, void* stream);
/* ABI 20: the same with an optional dropout on the INPUT rows of a problem: xmask (may be null, entries may be null): R[i] x K[i]
 * keep flags (0 / 1, contiguous, 16-byte aligned); problem i contracts (X_i * xmask_i) * xscale, formed where the launch stages
 * its X rows (the forward of nn.GRU's inter-layer dropout, model.py:866, inside the second layer's input contraction), and
 * writes those rows to xdrop[i] (R[i] x K[i] contiguous, may be null) for the layer's weight gradients.  A problem without
 * xmask is mmdfn_linear_planes_group's, bit for bit. */
int mmdfn_linear_planes_group_in(int n, const float* const* X, const void* const* planes, const float* const* bias,
                                 const float* const* bias2, const int* n1, float* const* Y, const int* R, const int* K,
                                 const int* N, const int* ldx, const int* ldy, int act, int accumulate,
                                 const float* const* mask, float mask_scale, const float* const* xmask,
                                 float* const* xdrop, float xscale, void* stream);
/* ABI 20: the same with the PARTY-ORDERED STORE (replaces the mmdfn_party_gather launch behind the first party-GRU layer's input
 * contraction, model.py:1070-1090): party (may be null: none) names, per problem, the speaker-encoded modality m whose utterance
 * rows (t, b) = row t B + b the problem projects (R[i] == L B), or -1.  A party problem stores row (t, b) of X [W1; W2]^T +
 * [b1; b2] to S[rank(t, b, p), (m B + b) P + p, :] for every speaker p flagged in qmask[t, b, :] (qmask: (L, B, P) floats;
 * S: (L, Mn B P, N); Y[i] unused, may be null); extra workgroups of the launch write rank (L, B, P) int32 (-1: not flagged) and
 * the bias into the padding rows k >= count(b, p) of S.  S and rank are bit for bit what mmdfn_party_gather makes of the
 * bias-free projection.  The party problems come first, one per modality 0 .. Mn-1, with equal N / n1 (multiples of 4); act ==
 * 0, accumulate == 0.  Returns -2 for a shape the store does not cover (L > 2048, P > 16, L B P > 24 576). */
int mmdfn_linear_planes_group_party(int n, const float* const* X, const void* const* planes, const float* const* bias,
                                    const float* const* bias2, const int* n1, float* const* Y, const int* R, const int* K,
                                    const int* N, const int* ldx, const int* ldy, int act, int accumulate,
                                    const float* const* mask, float mask_scale, const float* const* xmask,
                                    float* const* xdrop, float xscale, const int* party, const float* qmask, float* S,
                                    int32_t* rank, int L, int B, int P, int Mn, void* stream);

/* A GROUP of few-row projections in one launch (linear_small.hip; n <= 8 problems, K <= 768, K % 4 == 0):
 *   Y_p = act(X_p W_p^T + b_p) (+ Y_p)      X_p: R_p rows of K_p floats (stride ldx), Y_p: R_p x N_p (stride ldy)
 *   kmajor[p] == 0: W_p is (N, K) with k-contiguous rows (row stride ldw), given as two row blocks W / W2 split at
 *                   N1 (N1 == N: one block), biases likewise;
 *   kmajor[p] != 0: W_p is (K, N) with n-contiguous rows (row stride ldw): the input gradient dX = dY . Wcat of a dense
 *                   layer reads the stacked weight as stored.
 * Replaces the modality projections model.py:1065,1094,1129, the hoisted GRU input contractions model.py:1082,1132
 * and their autograd input gradients at BASELINE cfg2-cfg4 row counts.  mmdfn_linear_group_supported: 1 if covered. */
int mmdfn_linear_group_supported(int R, int K, int N);
int mmdfn_linear_group(int n, const float* const* X, const float* const* W, const float* const* W2, const int* N1,
                       const float* const* bias, const float* const* bias2, float* const* Y, const int* R,
                       const int* K, const int* N, const int* ldx, const int* ldw, const int* ldy,
                       const int* kmajor, const int* accumulate, int act, void* stream);
/* The same with an out-of-place addend: problem p computes Y_p = act(X_p W_p (+ b)) + Z_p for Z[p] != NULL (Z_p: R_p rows of
 * N_p floats, row stride ldz[p]; read only -- an autograd node adds onto an incoming gradient without writing into a tensor
 * it does not own), and behaves like mmdfn_linear_group for Z[p] == NULL (Z == NULL: for every problem). */
int mmdfn_linear_group_addend(int n, const float* const* X, const float* const* W, const float* const* W2, const int* N1,
                              const float* const* bias, const float* const* bias2, float* const* Y, const float* const* Z,
                              const int* ldz, const int* R, const int* K, const int* N, const int* ldx, const int* ldw,
                              const int* ldy, const int* kmajor, const int* accumulate, int act, void* stream);
/* ABI 20: the same with an optional SECOND K segment per problem: Y_p = X_p . W_p + X2_p . Wk2_p (+ Z_p) for X2[p] != NULL
 * (kmajor[p] != 0 only; X2_p: R_p rows of K2[p] floats, row stride ldx2[p]; Wk2_p: (K2, N) with n-contiguous rows of stride
 * ldw2[p]; 16-byte aligned, K2 % 4 == 0).  One workgroup contracts both operand pairs, each padded to whole 64-wide chunks: the
 * input gradient that reaches the same rows through two projections (the party and the context GRU's first-layer input
 * contractions of the text rows, model.py:1082,1132) is one launch and one accumulation chain.  X2 == NULL or X2[p] == NULL:
 * the problem is mmdfn_linear_group_addend's, bit for bit.  Returns -2 when a second segment is asked for and the operands do
 * not take the LDS-staged form (unaligned): the caller runs two launches. */
int mmdfn_linear_group_seg2(int n, const float* const* X, const float* const* W, const float* const* W2, const int* N1,
                            const float* const* bias, const float* const* bias2, float* const* Y, const float* const* Z,
                            const int* ldz, const int* R, const int* K, const int* N, const int* ldx, const int* ldw,
                            const int* ldy, const int* kmajor, const int* accumulate, const float* const* X2,
                            const float* const* Wk2, const int* K2, const int* ldx2, const int* ldw2, int act, void* stream);

/* ---------------------------------------------------------------------------
 * Secondary fusion modules (fusion.hip); their dense projections go through mmdfn_linear_group.
 *   MFN, reference model_fusion.py:62-120, per timestep and batch row:
 *     softmax_scale: att = softmax(z, dim=1) (saved), out = att * c          (:96-97; z, c, att, out: R x W)
 *     mfn_mem      : mem' = sigmoid(v1) mem + sigmoid(v2) tanh(u)            (:98-102; n elements; saved: 3 n floats)
 *   MMGatedAttention 'general', reference model.py:761-781, per modality pair (m, n) and row:
 *     gated_pair   : z = sigmoid(w . [x_m | x_n | x_m * x_n] + b) (w: 3 D floats, saved in zs),
 *                    out = z tanh(p_m) + (1 - z) tanh(p_n)   (x: R x D, p / out: R x C);
 *                    backward also writes dpre[r] = d loss / d (gate pre-activation)
 *     rowscale_colsum: out[0:3D] = sum_r s[r] [x_m | x_n | x_m * x_n][r], out[3D] = sum_r s[r]   (gate weight / bias gradient)
 * ------------------------------------------------------------------------- */
int mmdfn_softmax_scale_fwd(const float* z, const float* c, float* att, float* out, int R, int W, void* stream);
int mmdfn_softmax_scale_bwd(const float* att, const float* c, const float* dout, float* dz, float* dc, int R, int W,
                            void* stream);
int mmdfn_mfn_mem_fwd(const float* u, const float* v1, const float* v2, const float* mem, float* out, float* saved,
                      int64_t n, void* stream);
int mmdfn_mfn_mem_bwd(const float* saved, const float* mem, const float* dout, float* du, float* dv1, float* dv2,
                      float* dmem, int64_t n, void* stream);
int mmdfn_gated_pair_fwd(const float* xm, const float* xn, const float* w, const float* b, const float* pm,
                         const float* pn, float* out, float* zs, int R, int D, int C, void* stream);
int mmdfn_gated_pair_bwd(const float* xm, const float* xn, const float* w, const float* pm, const float* pn,
                         const float* zs, const float* dout, float* dxm, float* dxn, float* dpm, float* dpn,
                         float* dpre, int R, int D, int C, void* stream);
int mmdfn_rowscale_colsum(const float* s, const float* xm, const float* xn, float* out, int R, int D, void* stream);

/* ---------------------------------------------------------------------------
 * Weight-gradient contraction (autograd of the dense layers on the path: dW = dY^T X, db = sum_r dY):
 *   C[m, n] = sum_r A[r, m] B[r, n]      A: R rows of M floats (stride lda), B: R rows of N floats (ldb)
 *   colsum[m] = sum_r A[r, m]            (optional, NULL to skip)
 * Split over r across workgroups; `workspace` must hold splits*(M*N + M) floats
 * (splits from mmdfn_gemm_tn_splits).  M, N, lda, ldb multiples of 4.  C: M rows, stride ldc.
 * ------------------------------------------------------------------------- */
int mmdfn_gemm_tn_splits(int R, int M, int N);
int mmdfn_gemm_tn(const float* A, const float* B, float* C, float* colsum, float* workspace,
                  int R, int M, int N, int lda, int ldb, int ldc, int splits, void* stream);

/* ---------------------------------------------------------------------------
 * The same contraction for up to 8 independent problems in ONE launch pair, with an optional row shift on B:
 *   C_p[m, n] = sum_r A_p[r, m] * B_p[r + bshift_p, n]     (rows of B_p outside [0, R_p) count as zero)
 *   colsum_p[m] = sum_r A_p[r, m]                           (colsum may be NULL, or an array with NULL entries)
 * Replaces the recurrent-weight gradients of nn.GRU on the path (autograd of model.py:866,868: for every GRU,
 * layer and direction dW_hh = sum_t dgh_t (x) h_{t-1}, db_hh = sum_t dgh_t): h_{t-1} is the output sequence
 * shifted by one time step (bshift = -rows_per_step forward, +rows_per_step reverse), and with the shift inside
 * the kernel A spans every row so its column sums are the full bias gradient.  A, B, C, colsum, R .. bshift are
 * HOST arrays of length n (device pointers / ints).  workspace: mmdfn_gemm_tn_grouped_workspace(n, R, M, N) floats.
 * ------------------------------------------------------------------------- */
int64_t mmdfn_gemm_tn_grouped_workspace(int n, const int* R, const int* M, const int* N);
int mmdfn_gemm_tn_grouped(int n, const float* const* A, const float* const* B, float* const* C, float* const* colsum,
                          const int* R, const int* M, const int* N, const int* lda, const int* ldb, const int* ldc,
                          const int* bshift, float* workspace, void* stream);

/* ---------------------------------------------------------------------------
 * Fused stages of the GCNII "dynamic fusion" stack (GCNII_lyc.forward model_GCN.py:444-488, GraphConvolution.forward
 * :176-189): each is ONE launch whose dense contraction runs as exact-f32 MFMA with the pointwise work in its
 * prologue / epilogue (csrc/gcn_stack.hip).  R rows (= M * N graph nodes), H = hidden width (<= 100, multiple of 4),
 * F = input width (<= 256, multiple of 4); every mask is a float keep-mask (0 / 1) multiplied by mscale = 1/(1-p) where
 * it is used, NULL = ones.
 *
 * input stage (model_GCN.py:453-456):  xd = x (.) mx (row stride ldxd);  h0 = relu(xd W0^T + b0);  cur0 = h0 (.) m0
 *   bwd:  dpre = (dcur0 (.) m0 + dh0) (.) [h0 > 0]  (operand of dW0 / db0);  dx = (dpre W0 + dxd) (.) mx,
 *         dxd = gradient reaching xd directly (row stride lddxd) or NULL.
 * gate (K8, model_GCN.py:463-467, nn.LSTM seq_len 1, gate order i f g o, W_ih / W_hh (4H, H), bias = bsum + bsum2
 *   (b_ih, b_hh; bsum2 may be NULL):
 *   fwd:  (h_out, c_out) = LSTMCell(q, (h, c));  h = c = NULL is the zero state;  gates (R, 4H) = gate ACTIVATIONS.
 *   bwd:  dh' = dh_a + dh_b (either NULL), dc_next (NULL = 0) -> dG (R, 4H) pre-activation gradients (operand of
 *         dW_ih, dW_hh, db), dc_prev, dq = dG W_ih + dres (row stride lddres, NULL = 0), dh_prev = dG W_hh;  has_h = 0: the incoming
 *         state was zero, dc_prev / dh_prev are not produced.
 * layer (K7, model_GCN.py:178-186,469-472, W (2H, H) as stored by GraphConvolution):
 *   fwd:  pre = theta [hi | h0] W + (1-theta)((1-alpha) hi + alpha h0);  out = relu(pre) (.) m + q (row stride ldo, q
 *         NULL = 0);  gmask = m (.) [pre > 0].
 *   bwd:  dP = theta dout (.) gmask (operand of dW = [hi | h0]^T dP; dout row stride lddo);
 *         dhi = dP W[:H]^T + (1-theta)(1-alpha) gg,  dh0 (+)= dP W[H:]^T + (1-theta) alpha gg,  gg = dout (.) gmask;
 *         acc_h0 != 0 accumulates into dh0 (h0 feeds every layer).
 * ------------------------------------------------------------------------- */
int mmdfn_gcn_input_fwd(const float* x, const float* mx, const float* W0, const float* b0, const float* m0, float* xd,
                        float* h0, float* cur0, int R, int F, int H, int ldxd, float mscale, void* stream);
int mmdfn_gcn_input_bwd(const float* dcur0, const float* m0, const float* dh0, const float* h0, const float* W0,
                        const float* dxd, const float* mx, float* dpre, float* dx, int R, int F, int H, int lddxd,
                        float mscale, void* stream);
int mmdfn_lstm_gate_fwd(const float* q, const float* h, const float* c, const float* Wih, const float* Whh,
                        const float* bsum, const float* bsum2, float* gates, float* h_out, float* c_out, int R, int H,
                        void* stream);
/* the same with a row stride ldh (floats, >= H, % 4 == 0) on BOTH h and h_out: the layers' hidden states live as column blocks of
 * one (R, nl H) buffer, which is then the Y operand of ONE mmdfn_tile_outer(d = nl H) for the whole stack (model_GCN.py:461-472
 * shares `adj` across the layers: dA = sum_l dhi_l zin_l^T is one contraction of width nl H) */
int mmdfn_lstm_gate_fwd_ld(const float* q, const float* h, const float* c, const float* Wih, const float* Whh,
                           const float* bsum, const float* bsum2, float* gates, float* h_out, float* c_out, int R, int H,
                           int ldh, void* stream);
/* The cell's weights as bf16 piece planes for the many-row form of the forward launch (ABI 14).  The LSTM cell of the reasoning
 * module is shared by all layers of a stack and constant inside a step (model_GCN.py:466), so a caller whose launches take the
 * many-row form (mmdfn_lstm_gate_takes_planes(R, H) != 0) cuts it ONCE per forward pass -- mmdfn_lstm_gate_cut_weights into
 * mmdfn_lstm_gate_planes_workspace(H) floats -- and hands the planes to every layer's mmdfn_lstm_gate_fwd_pre (same operands
 * as mmdfn_lstm_gate_fwd_ld; planes = NULL, h = NULL or a launch of another form: identical to mmdfn_lstm_gate_fwd_ld). */
int64_t mmdfn_lstm_gate_planes_workspace(int H);
int mmdfn_lstm_gate_cut_weights(const float* Wih, const float* Whh, float* planes, int H, void* stream);
int mmdfn_lstm_gate_takes_planes(int R, int H);
int mmdfn_lstm_gate_fwd_pre(const float* q, const float* h, const float* c, const float* Wih, const float* Whh,
                            const float* bsum, const float* bsum2, float* gates, float* h_out, float* c_out, int R, int H,
                            int ldh, const float* planes, void* stream);
int mmdfn_lstm_gate_bwd(const float* gates, const float* c_prev, const float* c_new, const float* dh_a, const float* dh_b,
                        const float* dc_next, const float* Wih, const float* Whh, const float* dres, float* dG,
                        float* dc_prev, float* dq, float* dh_prev, int R, int H, int has_h, int lddres, void* stream);
int mmdfn_gcnii_layer_fwd(const float* hi, const float* h0, const float* W, const float* q, const float* m, float* out,
                          float* gmask, float theta, float alpha, int R, int H, int ldo, float mscale, void* stream);

/* ABI 16: K6 + K7 forward of one layer in ONE launch for short dialogues (L <= 128, M <= 3, H <= 100, H % 4 == 0, at most 4 096
 * (dialogue, modality, 32-row strip) workgroups):  hi = A_hat . z (written out: the backward pass contracts against it; z rows
 * have stride ldz), then mmdfn_gcnii_layer_fwd's update of the same rows.  Same operands as mmdfn_propagate (block-tile
 * adjacency, layout arrays) and mmdfn_gcnii_layer_fwd (h0, W, q, m: row stride H; out: row stride ldo; gmask).  Returns -2 when
 * the shape is not covered: the caller runs the two launches.  (csrc/gcn_small.hip; model_GCN.py:178-189) */
int mmdfn_prop_layer_fwd(const float* tiles, const float* cross, const float* zin, int ldz, const int32_t* dia_len,
                         const int32_t* row_start, const int64_t* tile_base, int B, int M, int N, int max_len,
                         const float* h0, const float* W, const float* q, const float* m, float* hi, float* out,
                         float* gmask, float theta, float alpha, int H, int ldo, float mscale, void* stream);
int mmdfn_gcnii_layer_bwd(const float* dout, const float* gmask, const float* W, float* dP, float* dhi, float* dh0,
                          float theta, float alpha, int R, int H, int lddo, int acc_h0, void* stream);
/* the same with a row stride lddhi on dhi (the X operand of the stack's single mmdfn_tile_outer, see mmdfn_lstm_gate_fwd_ld) */
int mmdfn_gcnii_layer_bwd_ld(const float* dout, const float* gmask, const float* W, float* dP, float* dhi, float* dh0,
                             float theta, float alpha, int R, int H, int lddo, int acc_h0, int lddhi, void* stream);

/* Weight FRAGMENT IMAGES of the stack kernels (ABI 23, additive; csrc/stack_images.hip, csrc/stack_image_map.h).  Every
 * workgroup of the launches above re-derives the same slice of a parameter (registers -> padded LDS rows) before its first
 * MFMA.  The slice depends on the weights alone, so the caller may cut it ONCE per optimizer step into the order the
 * consumer waves read it: float4 ((cb * ntiles + t) * nk + kc) * 64 + lane of an image is what lane `lane` of the wave that
 * holds tile t of column block cb reads for K-chunk kc -- exact fp32 values of the parameter, or 0.0 where the LDS copy holds
 * padding.  kind: 0 input fwd (W0), 1 input bwd (W0), 2 layer bwd (the (2H, H) weight), 3 gate fwd ([W_ih | W_hh]; has_h = 0:
 * W_ih alone, the layer without a previous state), 4 gate bwd (W_ih column blocks, then W_hh's when has_h != 0).  F is read by
 * kinds 0 / 1 only.
 *   mmdfn_stack_images_workspace: bytes of one image (-1: shape not covered).
 *   mmdfn_stack_image_source: host-side, no GPU work: the source of float j of image position (cb, t, kc, lane) -- returns 0
 *     (the image holds 0.0), 1 (element (*row, *col) of the first matrix: W0 / W / W_ih) or 2 (of the second: W_hh); -1 on
 *     arguments outside the image.  The cut kernel evaluates the same function.
 *   mmdfn_cut_stack_images: n <= 16 images in ONE launch; parameters contiguous; w2 is W_hh for kinds 3 / 4 with has_h != 0
 *     (else ignored, may be null); image[i]: 16-byte aligned, mmdfn_stack_images_workspace(...) bytes.
 *   mmdfn_*_img: the launch without the suffix reading its weight slice from `image` (no slice in LDS: ~35 KB per workgroup
 *     instead of ~120; the fragments are held in registers).  Results are bit-identical.  image = NULL: the entry without the
 *     suffix.  Returns -2 (nothing launched) for shapes the image form does not cover (16 384 rows or more, F > 208): the caller takes
 *     the entry without the suffix. */
int64_t mmdfn_stack_images_workspace(int kind, int H, int F, int has_h);
int mmdfn_stack_image_source(int kind, int H, int F, int has_h, int cb, int t, int kc, int lane, int j, int* row, int* col);
int mmdfn_cut_stack_images(int n, const int* kind, const float* const* w1, const float* const* w2, const int* H, const int* F,
                           const int* has_h, float* const* image, void* stream);
int mmdfn_gcn_input_fwd_img(const float* x, const float* mx, const float* W0, const float* b0, const float* m0, float* xd,
                            float* h0, float* cur0, int R, int F, int H, int ldxd, float mscale, const float* image,
                            void* stream);
int mmdfn_gcn_input_bwd_img(const float* dcur0, const float* m0, const float* dh0, const float* h0, const float* W0,
                            const float* dxd, const float* mx, float* dpre, float* dx, int R, int F, int H, int lddxd,
                            float mscale, const float* image, void* stream);
int mmdfn_gcnii_layer_bwd_ld_img(const float* dout, const float* gmask, const float* W, float* dP, float* dhi, float* dh0,
                                 float theta, float alpha, int R, int H, int lddo, int acc_h0, int lddhi, const float* image,
                                 void* stream);
int mmdfn_lstm_gate_fwd_pre_img(const float* q, const float* h, const float* c, const float* Wih, const float* Whh,
                                const float* bsum, const float* bsum2, float* gates, float* h_out, float* c_out, int R, int H,
                                int ldh, const float* planes, const float* image, void* stream);
int mmdfn_lstm_gate_bwd_img(const float* gates, const float* c_prev, const float* c_new, const float* dh_a, const float* dh_b,
                            const float* dc_next, const float* Wih, const float* Whh, const float* dres, float* dG,
                            float* dc_prev, float* dq, float* dh_prev, int R, int H, int has_h, int lddres,
                            const float* image, void* stream);

/* ---------------------------------------------------------------------------
 * Batch form: EVERY weight-gradient contraction of a training step in one launch pair (they feed nothing but the
 * optimizer, so the host queues them during backward and issues them at its end; run_train_erc.py:208 autograd).
 *   segment s (0 <= s < nseg):  A_s (R_s rows, stride lda_s), B_s (R_s rows, stride ldb_s), row shift bshift_s on B,
 *                               contributes  sum_r A_s[r, :]^T B_s[r + bshift_s, :]  to output out[s];
 *   output o (0 <= o < nout):   C_o (M_o x N_o, stride ldc_o) (+)= sum of its segments; colsum_o / colsum2_o (M_o
 *                               floats or NULL; two destinations because b_ih and b_hh of the LSTM gate share one
 *                               gradient) (+)= column sums of the segments' A;  accumulate_o != 0 adds to the
 *                               existing contents.  Segments of one output are extra splits of one slab stack: the
 *                               layer-shared LSTM gate (model_GCN.py:466) gets one segment per GCN layer and no
 *                               gradient-accumulation kernel.
 * nseg, nout <= 40.  All arrays are HOST arrays.  workspace: mmdfn_gemm_tn_batch_workspace(...) floats.
 * Kernel form per batch (an implementation choice, results do not depend on it beyond fp32 summation order): 64 x 64 / 64 x 112
 * output tiles with the rows split over workgroups, or -- when the batch holds enough long segments (>= 8192 rows, a multiple
 * of 16, 64-128 or 336-448 output rows, 64-112 columns, no shift) -- one workgroup per whole-output slab for those.
 * ------------------------------------------------------------------------- */
int64_t mmdfn_gemm_tn_batch_workspace(int nseg, const int* R, const int* out, int nout, const int* M, const int* N);
int mmdfn_gemm_tn_batch(int nseg, const float* const* A, const float* const* B, const int* R, const int* lda,
                        const int* ldb, const int* bshift, const int* out, int nout, float* const* C,
                        float* const* colsum, float* const* colsum2, const int* M, const int* N, const int* ldc,
                        const int* accumulate, float* workspace, void* riders, void* stream);
/* The same batch whose reduction launch ALSO sums `next` slab stacks written by other kernels (ABI 13): stack e holds
 * ext_splits[e] slabs of ext_M[e] x ext_N[e] floats (ext_part[e], summed into ext_C[e] of row stride ext_ldc[e]; ext_N[e] = 0:
 * none) and / or of ext_M[e] floats (ext_colpart[e], summed into ext_colsum[e]; NULL: none), in slab order (bit-reproducible);
 * ext_accumulate[e] != 0 adds to the destination.  Producers: mmdfn_head_bwd_partial (the classifier's dW / db, reference
 * model.py:1337), mmdfn_colsum_partial (the bias gradient of the project-then-gather node, model.py:1082).  nseg = nout = 0 with
 * next > 0 runs the reduction alone; nout + next <= 40. */
int mmdfn_gemm_tn_batch_ext(int nseg, const float* const* A, const float* const* B, const int* R, const int* lda,
                            const int* ldb, const int* bshift, const int* out, int nout, float* const* C,
                            float* const* colsum, float* const* colsum2, const int* M, const int* N, const int* ldc,
                            const int* accumulate, float* workspace, int next, const float* const* ext_part,
                            const float* const* ext_colpart, float* const* ext_C, float* const* ext_colsum, const int* ext_M,
                            const int* ext_N, const int* ext_ldc, const int* ext_splits, const int* ext_accumulate,
                            void* riders, void* stream);

/* Weight-gradient RIDERS of the GRU backward recurrence launch (ABI 17; the `riders` context: 18).  The backward recurrence of
 * nn.GRU (reference model.py:866-868: autograd of the context / party GRUs) keeps one CU per sequence busy for ~T x 0.65 us and leaves the other
 * CUs idle (IEMOCAP batch of 16: 160 of 256).  mmdfn_wgrad_riders_stage takes the arguments of mmdfn_gemm_tn_batch, plans the
 * batch and allocates its slabs exactly as that call would, but -- when the batch runs on the bf16-piece form, has at most 16
 * segments and nothing is staged in `riders` yet -- stages it there instead of launching it: a mmdfn_gru_seq_bwd call given the
 * same context, on a launch with idle CUs (mmdfn_gru_seq_bwd_idle_cus), runs the batch's tiles as extra workgroups of the
 * recurrence launch (never on a CU that holds a recurrence: the launch's LDS request keeps every CU to one workgroup); the slab
 * reduction follows later (mmdfn_wgrad_riders_drain).  A batch that cannot ride is launched by the stage call itself.
 * mmdfn_wgrad_riders_staged: 1 while a batch waits in the context; mmdfn_wgrad_riders_flush launches a waiting batch the
 * ordinary way (call it where no GRU backward launch will follow).  The operands and the workspace must stay valid until the
 * launch that consumes them has been issued on `stream` (the same stream for all three calls).  Results are those of
 * mmdfn_gemm_tn_batch bit for bit (same tiles, same slab order). */
int mmdfn_wgrad_riders_stage(int nseg, const float* const* A, const float* const* B, const int* R, const int* lda,
                             const int* ldb, const int* bshift, const int* out, int nout, float* const* C,
                             float* const* colsum, float* const* colsum2, const int* M, const int* N, const int* ldc,
                             const int* accumulate, float* workspace, void* riders, void* stream);
int mmdfn_wgrad_riders_staged(void* riders);
/* CUs the mmdfn_gru_seq_bwd launch of these groups leaves idle if it is of the kind that takes riders, else 0: stage a batch
 * only when this is > 0, and size it for that many CUs over the recurrence's ~0.65 us x T. */
int mmdfn_gru_seq_bwd_idle_cus(int ngroups, const int* rows);
int mmdfn_gru_seq_bwd_step_ns(int ngroups, const int* rows);    /* ns per recurrence step of that launch (650 / 2300: the two forms) */
int mmdfn_wgrad_riders_flush(void* riders, void* stream);
/* The slab reduction of a batch that rode (or that mmdfn_wgrad_riders_flush launched) is not a launch of its own either: it waits
 * in the context and joins the reduction launch of the next mmdfn_gemm_tn_batch / _ext call given that context (unless that call
 * writes one of the same gradients: then it goes first, alone).
 * mmdfn_wgrad_riders_drain(riders, stream, 0) reduces what is still waiting -- call it once at the end of the backward pass, behind the
 * last batch; the slabs (the staged batches' workspaces) must stay valid until then.  discard != 0 forgets staged and waiting
 * work instead (after a backward pass that raised). */
int mmdfn_wgrad_riders_drain(void* riders, void* stream, int discard);

/* ---------------------------------------------------------------------------
 * Fused Adam step over flat fp32 buffers (replaces torch.optim.Adam(lr, weight_decay=l2).step(),
 * run_train_erc.py:512,212): L2 folded into the gradient, bias-corrected, `step` = 1, 2, ...
 * p, m, v updated in place; n elements (16-byte aligned buffers).
 * ------------------------------------------------------------------------- */
int mmdfn_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int step, void* stream);

/* ABI 22: the same update on DEVICE-RESIDENT step state (csrc/optimizer_state.hip).  mmdfn_adam_step takes the step count from the
 * host, so a captured launch of it would repeat step 1 for ever; here the count, the bias corrections, lr / weight decay, the
 * global gradient norm, its clipping factor and the skip decision live in a caller-owned block of DEVICE memory
 * (mmdfn_adam_state_bytes() = 64 bytes, 16-byte aligned) and no launch takes an argument that changes from step to step: the
 * three launches below can be nodes of a captured training step.  The host writes step / enabled / skip_nonfinite / lr /
 * weight_decay / max_norm (ordinary stream-ordered copies); the kernels write the rest. */
typedef struct mmdfn_adam_state {
  int32_t step;            /* steps applied so far */
  int32_t enabled;         /* 0: every kernel below leaves p, m, v and step untouched */
  int32_t skip_nonfinite;
  int32_t skipped;         /* running count of skipped steps */
  int32_t last_skipped;    /* 1 if the latest call was skipped */
  float lr, weight_decay, max_norm;     /* max_norm <= 0: no clipping */
  float grad_norm, scale;               /* outputs of the latest call */
  float bc1, bc2_sqrt;
  int32_t reserved[4];
} mmdfn_adam_state;
/* Every entry point below returns -1 and launches nothing on n <= 0, a null pointer, or a state block / float buffer (g, p, m,
 * v: read as 16-byte vectors) that is not 16-byte aligned. */
int64_t mmdfn_adam_state_bytes(void);
/* sum of g[i]^2 over n floats (16-byte aligned), accumulated in double: one partial per workgroup in partials[0 .. *nparts)
 * (*nparts = min(ceil(n / 4 / 256), 1024, nparts_cap) >= 1, written to HOST memory by the call itself); lanes, waves and
 * workgroups are reduced in a fixed order and without atomics, so the same data gives the same bits. */
int mmdfn_grad_sumsq(const float* g, int64_t n, double* partials, int nparts_cap, int* nparts, void* stream);
/* One workgroup, in front of mmdfn_adam_step_state.  With st->enabled == 0 it writes nothing.  Otherwise: the partials summed
 * in index order (partials == NULL: the norm is not wanted -- grad_norm = 0, scale = 1, never skipped; else 1 <= nparts <= 1024);
 * grad_norm = (float)sqrt(sum); scale = max_norm > 0 ? min(1, max_norm / (grad_norm + 1e-6f)) : 1 (torch's clip_grad_norm_);
 * last_skipped = skip_nonfinite && !isfinite(sum).  A skipped step counts in `skipped`; any other does ++step and leaves the
 * new step's bias corrections bc1 = 1 - beta1^step, bc2_sqrt = sqrt(1 - beta2^step) (computed in double, rounded once). */
int mmdfn_adam_prepare(mmdfn_adam_state* st, const double* partials, int nparts, float beta1, float beta2, void* stream);
/* mmdfn_adam_step's arithmetic with lr, weight_decay, bc1 and bc2_sqrt read from *st and g replaced by scale * g when scale < 1;
 * returns at once when !enabled || last_skipped (p, m, v untouched: non-finite gradients never reach them).  The same grid. */
int mmdfn_adam_step_state(float* p, const float* g, float* m, float* v, int64_t n, const mmdfn_adam_state* st, float beta1,
                          float beta2, float eps, void* stream);

/* ---------------------------------------------------------------------------
 * K9  classifier head (reference model.py:1328-1337: dropout_ -> ReLU -> smax_fc -> log_softmax) as one launch each way:
 *   z = relu(F (.) mask * mscale);  logp = log_softmax(z W^T + b)       F: N rows of Wd floats (row stride ldf),
 *   mask: (N, Wd) 0 / 1 keep flags or NULL, W: (C, Wd) nn.Linear layout, C <= 8 classes, Wd % 4 == 0.
 *   bwd: dF (row stride lddf), dW (C, Wd), db (C) from dlogp; workspace: mmdfn_head_bwd_workspace(Wd, C) floats;
 *   dW / db are reduced in a fixed order (bit-reproducible).
 *   split = 0: F / dF are plain (N, Wd) matrices.  split = Wm > 0 (Wm % 4 == 0, Wd % Wm == 0): F / dF are Wd / Wm
 *   consecutive (N, Wm) matrices of row stride ldf / lddf, read as their column-wise concatenation -- the (M, N, Wm)
 *   output of the graph stack used as cat([F[0], .., F[M-1]], -1) (model_mm.py:113-117) without materialising it.
 * ------------------------------------------------------------------------- */
int mmdfn_head_fwd(const float* F, const float* mask, const float* W, const float* bias, float* logp, int64_t N, int Wd,
                   int C, int ldf, int split, float mscale, void* stream);
int64_t mmdfn_head_bwd_workspace(int Wd, int C);
int mmdfn_head_bwd(const float* dlogp, const float* logp, const float* F, const float* mask, const float* W, float* dF,
                   float* dW, float* db, float* workspace, int64_t N, int Wd, int C, int ldf, int lddf, int split,
                   float mscale, void* stream);
/* mmdfn_head_bwd without its slab reduction (ABI 13): dF is complete, `workspace` holds mmdfn_head_bwd_groups() slabs of dW
 * ([groups][C][Wd]) followed by as many of db ([groups][C]) for mmdfn_gemm_tn_batch_ext. */
int mmdfn_head_bwd_groups(void);
int mmdfn_head_bwd_partial(const float* dlogp, const float* logp, const float* F, const float* mask, const float* W, float* dF,
                           float* workspace, int64_t N, int Wd, int C, int ldf, int lddf, int split, float mscale,
                           void* stream);
/* The same three launches with the ReLU made optional (ABI 19): relu != 0 is mmdfn_head_fwd / _bwd / _bwd_partial, relu == 0 is
 * z = F (.) mask * mscale and dF = (g W) (.) mask * mscale -- the head of the graph-free model (reference model.py:1403-1404:
 * dropout_ -> smax_fc -> log_softmax). */
int mmdfn_head_fwd_act(const float* F, const float* mask, const float* W, const float* bias, float* logp, int64_t N, int Wd,
                       int C, int ldf, int split, float mscale, int relu, void* stream);
int mmdfn_head_bwd_act(const float* dlogp, const float* logp, const float* F, const float* mask, const float* W, float* dF,
                       float* dW, float* db, float* workspace, int64_t N, int Wd, int C, int ldf, int lddf, int split,
                       float mscale, int relu, void* stream);
int mmdfn_head_bwd_partial_act(const float* dlogp, const float* logp, const float* F, const float* mask, const float* W,
                               float* dF, float* workspace, int64_t N, int Wd, int C, int ldf, int lddf, int split, float mscale,
                               int relu, void* stream);

/* ---------------------------------------------------------------------------
 * LMF  low-rank multimodal fusion (reference model_fusion.py:214-310), the pointwise part of each direction (csrc/lmf.hip);
 * the products [1, h_m] . factor_m run on the grouped linear / gemm_tn kernels.  O = output_dim, R = rank <= 8, modalities
 * in the order a, v, t.
 *   fwd: P (N rows, stride ldp >= 3 R O) holds P_m,r = h_m . factor_m[r, 1:, :] in column block m R + r; the kernel adds the
 *        constant row factor_m[r, 0, :] (at factor_m + r * rank_stride_m) in place and writes
 *        out = sum_r w[r] P_a,r (.) P_v,r (.) P_t,r + bias   (N, O), row stride ldo.
 *   bwd: from g = d out (row stride ldg) and the P of the forward, D (row stride ldd >= mmdfn_lmf_bwd_width(O, R)) gets
 *        [dP (3 R O) | g (O) | T (R) | zeros]: dP_m,r = g w_r times the other two modalities' P_.,r, T_r = sum_o g P_a,r P_v,r P_t,r;
 *        the column sums of D are d factor_m[r, 0, :], d bias and d w.
 * ------------------------------------------------------------------------- */
int mmdfn_lmf_bwd_width(int O, int R);
int mmdfn_lmf_fwd(float* P, const float* factor_a, const float* factor_v, const float* factor_t, int64_t rank_stride_a,
                  int64_t rank_stride_v, int64_t rank_stride_t, const float* w, const float* bias, float* out, int64_t N, int O,
                  int R, int ldp, int ldo, void* stream);
int mmdfn_lmf_bwd(const float* g, const float* P, const float* w, float* D, int64_t N, int O, int R, int ldg, int ldp, int ldd,
                  void* stream);

/* ---------------------------------------------------------------------------
 * TFN  tensor fusion (reference model_fusion.py:169-211) after its subnets, ABI 21 (csrc/tensor_fusion.hip):
 *   Z[n, (i V1 + j) T1 + k] = [1, h_a][n, i] [1, h_v][n, j] [1, h_t][n, k]      (A1 = Ha + 1, ..., K = A1 V1 T1)
 *   out = act(dropout(Z) W1^T + b1),  W1 (O, K) with row stride ldw, O <= 304, act = ReLU when relu != 0.
 * Z, its dropout mask and dZ are never stored: every kernel regenerates its fragments of dropout(Z) from the h rows ((N, H_m),
 * row strides ldh*) and the keep flag of element (n, k), a pure function of the generator state the forward call used
 * (csrc/tfn_keep.h: Philox counter offset + n ceil(K / 8) + k / 8, 16-bit draw k % 8 against keep * 65536).  Exact f32 products,
 * fixed-order slab sums: the same inputs and state give the same bits.
 *   mmdfn_tfn_workspace  floats of `workspace` for mmdfn_tfn_fwd (which = 0: K slabs of (N, O)) and mmdfn_tfn_bwd_input
 *                        (which = 1: pair slabs of (N, A1 + V1 + T1)); -1: widths the kernels do not take.
 *   mmdfn_tfn_fwd        state != NULL (dropout on): the keep-flag generator state of the device ((seed, offset, ...), int64);
 *                        the call copies (seed, offset) to `used` (2 int64, kept for the backward calls) and advances the
 *                        offset by `counters` (>= N ceil(K / 8)); keep = 1 - p, scale = 1 / keep (0 for keep = 0).
 *                        state == NULL: no dropout (used / counters / keep / scale ignored).
 *   mmdfn_tfn_bwd_input  dpre = dy (.) (y1 > 0) (relu != 0; y1 = the forward's out) or dy, written to dpre (N, O);
 *                        dh_m (N, H_m) contiguous = the gradients of the three h; used == NULL: no dropout.
 *   mmdfn_tfn_bwd_weight dW1 (O, K) contiguous = dpre^T dropout(Z), every element written once.
 *   mmdfn_tfn_keep_flags test / debug: out (rows, K) = the 0 / 1 keep flags of rows row0 .. row0 + rows - 1 of an N-row call.
 * ------------------------------------------------------------------------- */
int64_t mmdfn_tfn_workspace(int64_t N, int Ha, int Hv, int Ht, int O, int which);
int mmdfn_tfn_fwd(const float* ha, const float* hv, const float* ht, int ldha, int ldhv, int ldht, const float* W1, int64_t ldw,
                  const float* b1, void* state, void* used, int64_t counters, float keep, float scale, float* out,
                  float* workspace, int64_t N, int Ha, int Hv, int Ht, int O, int relu, void* stream);
int mmdfn_tfn_bwd_input(const float* dy, const float* y1, int relu, const float* W1, int64_t ldw, const float* ha,
                        const float* hv, const float* ht, int ldha, int ldhv, int ldht, void* used, float keep, float scale,
                        float* dpre, float* dha, float* dhv, float* dht, float* workspace, int64_t N, int Ha, int Hv, int Ht,
                        int O, void* stream);
int mmdfn_tfn_bwd_weight(const float* dpre, const float* ha, const float* hv, const float* ht, int ldha, int ldhv, int ldht,
                         void* used, float keep, float scale, float* dW1, int64_t N, int Ha, int Hv, int Ht, int O,
                         void* stream);
int mmdfn_tfn_keep_flags(void* used, float keep, float* out, int64_t N, int64_t K, int64_t row0, int64_t rows, void* stream);

/* ---------------------------------------------------------------------------
 * K10  FocalLoss (reference loss.py:14-34) as one launch each way:
 *   loss = reduce_i( -(1 - pt_i)^gamma * alpha[t_i] * log_prob[i, t_i] ),  pt_i = exp(log_prob[i, t_i]) held constant
 *   (the reference detaches it), reduce = mean if size_average else sum; alpha (C) may be NULL.
 *   fwd writes loss[0] and coef[i] = -(1 - pt_i)^gamma * alpha[t_i] * (1/N or 1); the sum is reduced in a fixed order
 *   (bit-reproducible).  bwd: dlogp[i, c] = (c == t_i) * coef[i] * dloss[0]   (all N*C entries written).
 *   log_prob: (N, C) contiguous fp32; target: N int64.
 * ------------------------------------------------------------------------- */
int mmdfn_focal_loss_fwd(const float* logp, const int64_t* target, const float* alpha, float* loss, float* coef,
                         int64_t N, int C, float gamma, int size_average, void* stream);
/* the same, additionally writing dlogp_unit (N, C) = d loss / d log_prob for an upstream gradient of exactly 1 (NULL: not
 * wanted): loss.backward() then needs no launch for the loss (mmdfn_focal_loss_bwd remains for other upstream gradients) */
int mmdfn_focal_loss_fwd_grad(const float* logp, const int64_t* target, const float* alpha, float* loss, float* coef,
                              float* dlogp_unit, int64_t N, int C, float gamma, int size_average, void* stream);
int mmdfn_focal_loss_bwd(const float* coef, const int64_t* target, const float* dloss, float* dlogp, int64_t N, int C,
                         void* stream);
/* the same with rows to leave out (target == ignore_index: no loss, zero gradient row; the mean divides by the rows that
 * count, on the device).  An extension of the reference's FocalLoss (loss.py has no ignore_index): train.StepGraphCache pads
 * a batch to its size bucket with a dummy dialogue labelled ignore_index, so one captured step serves batches with different
 * numbers of utterances.  scale_out: 1 float (1 / count, or 1 without size_average), handed to the backward. */
int mmdfn_focal_loss_fwd_ignore(const float* logp, const int64_t* target, const float* alpha, float* loss, float* coef,
                                float* scale_out, int64_t N, int C, float gamma, int size_average, int64_t ignore_index,
                                void* stream);
int mmdfn_focal_loss_bwd_ignore(const float* coef, const int64_t* target, const float* dloss, const float* scale,
                                float* dlogp, int64_t N, int C, int64_t ignore_index, void* stream);

/* ---------------------------------------------------------------------------
 * K11  speaker / modality embeddings of the graph input (MM_GCN.forward,
 *      model_mm.py:78-93) on the (M, N, D) modality-major stack, M <= 3
 * ---------------------------------------------------------------------------
 * modal_rows: HOST array of M ints, the row of every slot in the (3, D) modality table (a 0, v 1, l 2); l_slot: the slot of
 * 'l', -1 when absent (row 2 must sit in that slot and nowhere else).  speaker (S, D) / modal (3, D): NULL = not added.
 *   s_n = first maximum of qmask[flat_idx[n], 0..P)   (qmask: (LB, P) fp32, flat_idx: (N,) int64 pad-strip rows t * B + b; an
 *         index outside [0, LB) gives speaker 0), written to spk[n] (int32) when the speaker part runs (speaker and 'l' present)
 *   Y[l_slot] = (X[l_slot] + speaker[s_n]) + modal[2],   Y[m] = X[m] + modal[modal_rows[m]]     (plain fp32 adds)
 * Returns -1 on bad arguments (P > S among them), -2 having launched nothing when D % 4 != 0, a pointer is not 16-byte aligned
 * or S > mmdfn_graph_embed_max_speakers() (callers take another path).  One launch, grid from (M, N, D) only.
 * Backward (dX is dY itself): dspeaker[s] = sum_{n: spk[n] = s} dY[l_slot, n, :]  (all S rows written; no utterance: 0),
 * dmodal[modal_rows[m]] = sum_n dY[m, n, :]  (all 3 rows written; absent modalities: 0); either may be NULL.  One launch, no
 * atomics, no workspace, fixed summation order: rows n = g, g + R, g + 2R, ... per row group g < R = mmdfn_graph_embed_rows(),
 * then the groups in order.  Same -1 / -2 rules.  mmdfn_graph_embed_threads(): 16-byte lanes per forward workgroup. */
int mmdfn_graph_embed_rows(void);
int mmdfn_graph_embed_threads(void);
int mmdfn_graph_embed_max_speakers(void);
int mmdfn_graph_embed_fwd(const float* X, const float* qmask, const int64_t* flat_idx, const float* speaker, const float* modal,
                          const int32_t* modal_rows, int l_slot, float* Y, int32_t* spk, int M, int N, int D, int P, int S,
                          int64_t LB, void* stream);
int mmdfn_graph_embed_bwd(const float* dY, const int32_t* spk, float* dspeaker, float* dmodal, const int32_t* modal_rows,
                          int l_slot, int M, int N, int D, int S, void* stream);

/* ---------------------------------------------------------------------------
 * K12  NLLLoss (torch.nn.NLLLoss(weight, ignore_index, reduction 'mean' / 'sum'), run_train_erc.py:509)
 * ---------------------------------------------------------------------------
 * loss = sum_{t_i != ignore} w[t_i] (-logp[i, t_i]) / sum_{t_i != ignore} w[t_i]   (mean != 0; mean == 0: no division; weight
 * NULL: 1).  One workgroup of mmdfn_nll_loss_threads() threads, fixed-order reduction in float64.  coef[i] = -w[t_i] (0 for
 * an ignored row), scale_out[0] = 1 / sum of the weights (1 without mean).  Every row ignored: loss 0, zero gradients (torch:
 * NaN); a label outside [0, C) that is not ignore_index: NaN loss, NaN gradient row.  weight must hold C entries.
 * Backward: dlogp[i, c] = (c == t_i) coef[i] scale[0] dloss[0]. */
int mmdfn_nll_loss_threads(void);
int mmdfn_nll_loss_fwd(const float* logp, const int64_t* target, const float* weight, float* loss, float* coef,
                       float* scale_out, int64_t N, int C, int mean, int64_t ignore_index, void* stream);
int mmdfn_nll_loss_bwd(const float* coef, const int64_t* target, const float* dloss, const float* scale, float* dlogp,
                       int64_t N, int C, int64_t ignore_index, void* stream);

/* ---------------------------------------------------------------------------
 * Fold-back of the encoder input projections (ABI 23, additive; csrc/fold_back.hip)
 * ---------------------------------------------------------------------------
 * X_m = u_m W_m^T + b_m feeds a GRU's first-layer input contraction with nothing in between, so both layers' weight gradients
 * follow from M = dG^T u_m (n x D) and c = colsum(dG) (n), which the weight-gradient batch leaves.  One TERM = one (direction
 * half of W_ih, modality) pair; per term
 *   dwih (n x H)  (+)= M wm^T + c bm^T        (wm: H x D, bm: H or NULL)
 *   dwm  (H x D)  (+)= wih^T M                (wih: n x H)
 *   dbm  (H)      (+)= wih^T c
 * Terms that name the same dwih (same n) or the same dwm / dbm (same D) are summed in term order (fp32 chains of 32 products,
 * their sums in float64) and rounded once behind the existing gradient (acc_wih[t] / acc_wm[t] != 0: accumulate, else write; taken from an output's first term).
 * dwih[t] / dwm[t] / dbm[t] may be NULL (that product is not wanted).  1 <= nterm <= 16; D, H multiples of 4 (n: any), at most 32
 * distinct outputs: otherwise -2; a missing operand -1.  No float atomics: bit-reproducible.
 * workspace: mmdfn_fold_back_workspace(...) floats, 8-byte aligned; tickets: mmdfn_fold_back_tickets() int32, ZERO before the
 * first launch that uses them -- every launch leaves them zero again (they may be shared by launches of one stream). */
int mmdfn_fold_back_tickets(void);
int64_t mmdfn_fold_back_workspace(int nterm, float* const* dwm, const int* n, const int* D, int H);
int mmdfn_fold_back(int nterm, const float* const* M, const float* const* c, const float* const* wih,
                    const float* const* wm, const float* const* bm, float* const* dwih, float* const* dwm,
                    float* const* dbm, const int* n, const int* D, int H, const int* acc_wih, const int* acc_wm,
                    float* workspace, int32_t* tickets, void* stream);

/* ---------------------------------------------------------------------------
 * K13  Pass metrics accumulated on the device (ABI 23, additive; csrc/pass_stats.hip)
 * ---------------------------------------------------------------------------
 * One launch per step: ONE workgroup of mmdfn_pass_stats_threads() threads, fixed row -> thread assignment, counts through an
 * LDS histogram of C x C integer counters (C <= mmdfn_pass_stats_max_classes()), added to the caller's accumulator with plain
 * loads and stores -- launches that share an accumulator must be serialised on one stream.  Bit-reproducible; no scratch, no
 * workspace.  logp: (N, C) contiguous fp32; target: N int64; loss: 1 fp32 or NULL; all in device memory, as is the accumulator:
 *   pred      N int64          pred[i] = lowest index among the maxima of row i (torch.argmax); a row that holds a NaN predicts
 *                              the index of its first NaN.  Written for EVERY row on EVERY launch, armed or not.
 *   counts    C * C int64      counts[label * C + pred]
 *   meta      8 int64          [0] armed  [1] rows  [2] batches  [3] bad_labels  [4] nan_rows  [5..7] reserved (never touched)
 *   loss_sum  1 double
 *   loss_hist slots fp32       the first `slots` batch losses of the pass, in launch order
 * meta[armed] == 0: the launch writes pred and NOTHING else (warm-up and pre-capture launches of a captured step).
 * Otherwise, for every row with target != ignore_index: 0 <= target < C -> counts[target * C + pred] += 1, meta[rows] += 1; any
 * other label -> meta[bad_labels] += 1 and no cell; a NaN row among them -> meta[nan_rows] += 1 (ignored rows are counted
 * nowhere).  Then once per launch: k = meta[batches]; loss_sum[0] += (double)loss[0]; if k < slots: loss_hist[k] = loss[0];
 * meta[batches] = k + 1  (loss NULL: the batch is counted, the two loss updates are skipped).  The kernel never writes
 * meta[armed]: the host does, with an ordinary fill, between launches.
 * Returns -1 before any launch for N <= 0, C <= 0, C > max_classes, slots < 0, a null logp / target / pred / counts / meta /
 * loss_sum, or a null loss_hist with slots > 0. */
int mmdfn_pass_stats_threads(void);
int mmdfn_pass_stats_max_classes(void);
int mmdfn_pass_stats_accumulate(const float* logp, const int64_t* target, const float* loss, int64_t* pred, int64_t* counts,
                                int64_t* meta, double* loss_sum, float* loss_hist, int64_t N, int C, int64_t ignore_index,
                                int slots, void* stream);

/* ---------------------------------------------------------------------------
 * K14  Matching attention over a dialogue (ABI 23, additive; csrc/matching_attention.hip)
 * ---------------------------------------------------------------------------
 * MatchingAttention(att_type='general2') (model.py:66-76,84) for every query row at once.  X (Tq, B, D) queries, M (L, B, D)
 * memory, mask (B, L) fp32 ("non-zero keeps"), all contiguous fp32 in device memory, rows 16-byte aligned:
 *   z = <X[t,b,:], M[s,b,:]>,  e = (mask[b,s] != 0) exp(tanh z),  alpha[t,b,s] = e / sum_s e,  pool[t,b,:] = sum_s alpha M[s,b,:]
 * Outputs: pool (Tq, B, D), alpha (Tq, B, L), aux (Tq, B, L) = tanh z (0 where the mask is), which the backward pass reads.
 * A dialogue whose mask row is all zero: pool, alpha and every gradient of it are 0 (the reference: 0 / 0 = NaN).
 * Backward for dpool (alpha is not differentiated through), ws: mmdfn_match_att_workspace(...) floats (it receives dz):
 *   dP = <dpool[t,b,:], M[s,b,:]>,  r = sum_s alpha dP,  dz = alpha (dP - r)(1 - aux^2)
 *   dX[t,b,:] = sum_s dz M[s,b,:]      dM[s,b,:] = sum_t dz X[t,b,:] + sum_t alpha dpool[t,b,:]
 * Exact fp32 products (v_mfma_f32_16x16x4_f32), every reduction in a fixed order, no atomics: bit-reproducible.  One launch
 * forward, two backward.  Served: D % 4 == 0, 4 <= D <= mmdfn_match_att_max_width(), 1 <= L <= mmdfn_match_att_max_len(),
 * Tq >= 1, 1 <= B <= 65535; anything else (or a null operand) returns -1 before any launch (the workspace query too). */
int mmdfn_match_att_max_width(void);
int mmdfn_match_att_max_len(void);
int64_t mmdfn_match_att_workspace(int Tq, int L, int B, int D);
int mmdfn_match_att_fwd(const float* X, const float* M, const float* mask, float* pool, float* alpha, float* aux, int Tq,
                        int L, int B, int D, void* stream);
int mmdfn_match_att_bwd(const float* dpool, const float* X, const float* M, const float* mask, const float* alpha,
                        const float* aux, float* dX, float* dM, float* ws, int Tq, int L, int B, int D, void* stream);

/* ---------------------------------------------------------------------------
 * K15  MaskedNLLLoss (ABI 23, additive; csrc/nll_loss.hip beside K12; reference loss.py:38-58)
 * ---------------------------------------------------------------------------
 * loss = sum_i m_i w[t_i] (-pred[i, t_i]) / sum_i m_i w[t_i]   (weight NULL: w = 1).  pred (N, C) fp32, target N int64, mask N
 * fp32 (the (B, L) utterance mask, rows in pred's order).  One workgroup of mmdfn_nll_loss_threads() threads, fixed-order
 * reduction in float64, the denominator on the device.  coef[i] = -m_i w[t_i], scale_out[0] = 1 / denominator.  No row with a
 * non-zero mask: loss 0, scale 0, zero gradients (the reference: NaN); a label outside [0, C) on a row that counts: NaN loss,
 * NaN gradient row; rows whose mask is 0 do not read their label.  weight must hold C entries.
 * Backward: dpred[i, c] = (c == t_i) coef[i] scale[0] dloss[0]; rows whose mask is 0 are written as exact zeros. */
int mmdfn_masked_nll_fwd(const float* pred, const int64_t* target, const float* mask, const float* weight, float* loss,
                         float* coef, float* scale_out, int64_t N, int C, void* stream);
int mmdfn_masked_nll_bwd(const float* coef, const int64_t* target, const float* mask, const float* dloss, const float* scale,
                         float* dpred, int64_t N, int C, void* stream);

/* ---------------------------------------------------------------------------
 * K16  fused LSTM recurrence (ABI 23, additive; csrc/lstm_seq.hip; the time loop inside the reference's
 * LSTMModel.lstm = nn.LSTM(D_m, 100, num_layers=2, bidirectional=True), model.py:320-356)
 * ---------------------------------------------------------------------------
 * One layer, both directions, one launch each way; one persistent workgroup per (sequence, direction).  Contiguous fp32 in
 * device memory; w_hh / b_hh are HOST arrays of two device pointers (forward, reverse):
 *   gi      : (T, rows, 8H)  X W_ih^T + b_ih, direction-major: forward [i f g o], then reverse [i f g o] (torch gate order)
 *   w_hh[d] : (4H, H), b_hh[d] : (4H)  exactly as nn.LSTM stores weight_hh_l*[_reverse] / bias_hh_l*[_reverse]
 *   y       : (T, rows, 2H) out, forward and reverse outputs side by side; direction 1 runs t = T-1 .. 0
 *   state   : (T, rows, 2, 5, H) out: i, f, g, o, c_t -- what the backward pass needs and nothing more (tanh(c_t) is
 *             recomputed; c_{t-1} is the previous (forward) / next (reverse) row block's c)
 *   dgate   : (T, rows, 8H) out, the gradient of the four pre-activations in gi's layout.  It is the gradient of both the
 *             input-side and the hidden-side pre-activations (so db_hh = db_ih); weight gradients are the caller's contractions.
 * Both directions start from h = c = 0; (h_n, c_n) is not an output.
 *   forward step :  a = W_hh h + b_hh + gi;  i, f, o = sig(.);  g = tanh(.);  c' = f c + i g;  h' = o tanh(c')
 *   backward step (per direction, in the reverse of its processing order):
 *     tc = tanh(c');  do = dh tc o (1-o);  dc = dc_carry + dh o (1 - tc^2);  di = dc g i (1-i);  df = dc c_prev f (1-f);
 *     dg = dc i (1 - g^2);  dc_carry = dc f;  dh_prev = dy_prev + dgate W_hh
 * The backward pass reads dy, state and w_hh (y is part of the signature for the caller's dW_hh contraction; it must be valid).
 * Both entry points return -1 before any HIP call for H != 100, rows <= 0, T <= 0 or any null pointer (the two entries of
 * w_hh / b_hh included).  mmdfn_lstm_seq_block_steps(): timesteps per staged block of operands (launch edges for tests). */
int mmdfn_lstm_seq_block_steps(void);
int mmdfn_lstm_seq_fwd(const float* gi, const float* const* w_hh, const float* const* b_hh, float* y, float* state,
                       int rows, int T, int H, void* stream);
int mmdfn_lstm_seq_bwd(const float* dy, const float* y, const float* state, const float* const* w_hh, float* dgate,
                       int rows, int T, int H, void* stream);

/* ---------------------------------------------------------------------------
 * K17  fused DialogueRNN recurrence (ABI 23, additive; csrc/dialogue_rnn.hip; the time loop of the reference's
 * DialogueRNN / DialogueRNNCell, model.py:168-278, both directions of DialogRNNModel, model.py:359-417, in one launch)
 * ---------------------------------------------------------------------------
 * Grid (ceil(B / R), ndir), ndir = 1 (a DialogueRNN on its own: direction 0 only; the arrays below then hold one direction and
 * the buffers keep their leading 2) or 2, R = mmdfn_drnn_chains_per_group(): a workgroup owns R chains of one direction for the whole sequence
 * and streams the state-side weights once per step for all of them.  Direction 1 runs each dialogue reversed within its own
 * length (t = len-1 .. 0) and stops there; direction 0 runs all T steps.  "Chain-step order" below: row s of a chain is its
 * s-th processed step (time s for direction 0, time len-1-s for direction 1).  Contiguous fp32 / int32 device memory; pu, img,
 * keep_*, w, dpu are HOST arrays of device pointers, [direction] (w: [direction][6]).
 *   pu[d]    : (T, B, npu) in TIME order, npu = 900 ('simple', att = 0) or 1050 ('general', att = 1):
 *              [U W_ih_g[:, :D_m]^T + b_ih_g (450) | U W_ih_p[:, :D_m]^T + b_ih_p (450) | U W_att^T (150)]
 *   img[d]   : mmdfn_drnn_image_floats() floats, the forward weight image, k-major (transposed) matrices then vectors:
 *              W_ih_g[:, D_m:]^T (150,450) | W_hh_g^T (150,450) | W_ih_p[:, D_m:]^T (150,450) | W_hh_p^T (150,450) |
 *              W_ih_e^T (150,300) | W_hh_e^T (100,300) | b_hh_g (450) | b_hh_p (450) | b_ih_e (300) | b_hh_e (300) |
 *              SimpleAttention.scalar.weight (150) + 2 zeros
 *   w[d][i]  : backward: the same six matrices as nn.GRUCell stores them (gate row j, column k), row strides ld[i]
 *              (W_ih_g[:, D_m:] is the pointer weight_ih + D_m with ld = D_m + 150)
 *   speaker  : (T, B) int32 argmax of qmask (clamped to [0, P));  upd : (T, B) qmask at the speaker (0 or 1);  lengths : (B)
 *   keep_*   : NULL (no dropout), or per direction NULL / 0-1 flags in chain-step order: g, q (T, B, 150), e (T, B, 100);
 *              kept values are multiplied by keep_scale
 *   e_out    : (2, T, B, 100) in TIME order;  alpha : (2, T, B, T) chain-step order, row s holds alpha_sj for j < s
 *   state    : (2, 17, T, B, 152) chain-step order, planes r z n hn of the g cell, g (dropped, carried), r z n hn of the p
 *              cell, q_{s-1}[speaker], q_s[speaker], c, r z n hn of the e cell, e (dropped, carried); columns past the width
 *              (150 / 100) are padding
 *   dgate    : (2, 6, T, B, 452) chain-step order: dgi_g dgh_g dgi_p dgh_p dgi_e dgh_e (gradients of the input-side and the
 *              hidden-side pre-activations: they differ in the n block);  dpu[d] : (T, B, npu) TIME order
 *   dghist   : (2, T, B, 152) workspace (the history gradient);  dw_part : (2, B, 152) per-chain dw of 'simple' (att = 0)
 * e_out, alpha, state, dgate, dpu, dghist must be ZERO on entry: the kernels write only the steps below a chain's length and
 * the columns below a plane's width.  Both entry points return -1 before any HIP call for a null pointer or an unserved size
 * (served: Dg = Dp = 150, De = 100, 1 <= P <= 16, 1 <= T <= 1008, B >= 1, npu as above, att 0 / 1, ndir 1 / 2, ld[i] >= the
 * width). */
int mmdfn_drnn_chains_per_group(void);
int64_t mmdfn_drnn_image_floats(void);
int mmdfn_drnn_seq_fwd(const float* const* pu, const float* const* img, const int32_t* speaker, const float* upd,
                       const int32_t* lengths, const float* const* keep_g, const float* const* keep_q,
                       const float* const* keep_e, float keep_scale, float* e_out, float* alpha, float* state, int B, int T,
                       int P, int Dg, int Dp, int De, int npu, int att, int ndir, void* stream);
int mmdfn_drnn_seq_bwd(const float* de_out, const float* const* pu, const float* const* img, const float* const* w,
                       const int32_t* ld, const int32_t* speaker, const float* upd, const int32_t* lengths,
                       const float* const* keep_g, const float* const* keep_q, const float* const* keep_e, float keep_scale,
                       const float* alpha, const float* state, float* dgate, float* const* dpu, float* dghist, float* dw_part,
                       int B, int T, int P, int Dg, int Dp, int De, int npu, int att, int ndir, void* stream);

/* ---------------------------------------------------------------------------
 * K18  fused embedding -> Conv1d -> ReLU -> max over time (ABI 23, additive; csrc/cnn_features.hip; the pooled
 * block of the reference's CNNFeatureExtractor, model.py:1410-1443)
 * ---------------------------------------------------------------------------
 * Contiguous device memory; conv_w / conv_b / d_w / d_b are HOST arrays of n_k device pointers, ksizes a HOST array of n_k sizes:
 *   tokens     : (rows, W) int64 token ids.  The caller validates them; the kernels clamp an id into [0, V) before every read.
 *   table      : (V, D) fp32, the embedding table
 *   conv_w[i]  : (F, D, K_i) fp32, conv_b[i] : (F), exactly as nn.Conv1d stores them
 *   row_mask   : (rows) fp32; a row whose mask is 0 is skipped: pooled 0, argmax -1
 *   planes     : workspace of mmdfn_cnn_planes_bytes(D, F, n_k, ksizes) bytes: the bf16 piece fragments of every tap, cut by
 *                the forward launch itself (nothing to keep fresh between steps)
 *   pooled     : (rows, n_k F) out, column i F + f = max_t relu(b_i[f] + sum_{k, c} W_i[f, c, k] E[tok[r, t + k], c]), 0 <= t <= W - K_i
 *   argmax     : (rows, n_k F) int32 out, the LOWEST t attaining the maximum; -1 where the maximum is <= 0 (no gradient)
 * mmdfn_cnn_pool_bwd writes (does not accumulate) d_w[i] (F, D, K_i) and d_b[i] (F) from d_pooled (rows, n_k F) and the saved
 * argmax, rows summed in ascending order.  The table gradient is a family of its own, launched only for a trainable table:
 *   mmdfn_cnn_table_entries = rows n_k F max K, the number of (row, column, tap) entries;
 *   mmdfn_cnn_table_keys writes keys (entries) int32: the token entry (r, column, k) touched, V for a dead one (k >= K_i or
 *     argmax -1);  the caller sorts them STABLY (sorted_keys, order = the int64 permutation);
 *   mmdfn_cnn_table_bwd writes all of d_table (V, D): token v's entries summed in sorted order, zeros for a token without any
 *     (bounds: a workspace of V + 1 int64, the tokens' segments in the sorted keys, written by a launch of its own).
 * No float atomics anywhere: the same inputs give the same bits.  Every entry point returns -1 before any HIP call for a null
 * pointer or an unserved size (served: D % 4 == 0 in 4..304, F in 1..64, n_k in 1..4, K_i in 1..8, max K <= W <= 512,
 * rows >= 1, V >= 1); the size queries return -1 likewise.  mmdfn_cnn_tile_words(): window starts per staged tile;
 * mmdfn_cnn_rows_per_group(): utterance rows per workgroup (launch edges for tests). */
int mmdfn_cnn_tile_words(void);
int mmdfn_cnn_rows_per_group(void);
int64_t mmdfn_cnn_planes_bytes(int D, int F, int n_k, const int32_t* ksizes);
int mmdfn_cnn_pool_fwd(const int64_t* tokens, const float* table, const float* const* conv_w, const float* const* conv_b,
                       const float* row_mask, void* planes, float* pooled, int32_t* argmax, int64_t rows, int W, int V, int D,
                       int F, int n_k, const int32_t* ksizes, void* stream);
int mmdfn_cnn_pool_bwd(const float* d_pooled, const int32_t* argmax, const int64_t* tokens, const float* table,
                       float* const* d_w, float* const* d_b, int64_t rows, int W, int V, int D, int F, int n_k,
                       const int32_t* ksizes, void* stream);
int64_t mmdfn_cnn_table_entries(int64_t rows, int F, int n_k, const int32_t* ksizes);
int mmdfn_cnn_table_keys(const int32_t* argmax, const int64_t* tokens, int32_t* keys, int64_t rows, int W, int V, int F,
                         int n_k, const int32_t* ksizes, void* stream);
int mmdfn_cnn_table_bwd(const float* d_pooled, const int32_t* sorted_keys, const int64_t* order, const float* const* conv_w,
                        int64_t* bounds, float* d_table, int64_t rows, int V, int D, int F, int n_k, const int32_t* ksizes,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMDFN_HIP_H */
