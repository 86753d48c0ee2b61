// Weight FRAGMENT IMAGES of the GCN stack kernels (gcn_stack.hip): where every float of an image comes from.
//
// A stack kernel contracts 16-row blocks of activations against a slice of a parameter that it parks in LDS as k-contiguous
// rows sW[n][k] (zero-padded to whole 16-wide chunks, missing rows zero).  Consumer lane l of a wave that holds tile t reads,
// for K-chunk kc, the 16 bytes at sW[16 t + frag_row(l & 15)][16 kc + 4 frag_unit(l >> 4) .. + 3].  The image of a slice
// stores exactly that float4 at index ((cb * ntiles + t) * nk + kc) * 64 + l (cb = column block of the launch), so a wave
// fetches a fragment with one coalesced 1 KB request and no workgroup has to re-derive the slice.  The slice depends on the
// weights alone: images are cut once per optimizer step (stack_images.hip), not once per workgroup.
#pragma once

enum StackImageKind {
    SI_INPUT_FWD = 0,    // W0 (H, F) as stored:            sW[n][k] = W0[n][k],  n < H, k < F
    SI_INPUT_BWD = 1,    // W0 (H, F) transposed:           sW[n][k] = W0[k][n],  n < F, k < H
    SI_LAYER_BWD = 2,    // GraphConvolution W (2H, H):     sW[n][k] = W[n][k],   n < 2H, k < H
    SI_GATE_FWD = 3,     // [W_ih | W_hh] (4H, H each), column block = 32 units x 4 gates: sW[gate * 32 + ul][k]
    SI_GATE_BWD = 4,     // W_ih / W_hh (4H, H) transposed, column block = 64 columns of one of them: sW[n][k] = W[k][n0 + n]
    SI_KINDS = 5
};

constexpr int SI_UB = 32;     // hidden units per column block of the gate forward (gcn_stack.hip UB)
constexpr int SI_CBW = 64;    // output columns per column block of the gate backward (gcn_stack.hip CBW)

struct StackImageShape {
    int ntiles;   // 16-row tiles of a column block's slice
    int nk;       // 16-wide K chunks
    int ncb;      // column blocks
};

__host__ __device__ inline int si_frag_row(int i) { return i < 4 ? 2 * i : (i < 12 ? 2 * (i - 4) + 1 : 2 * (i - 12) + 8); }
__host__ __device__ inline int si_frag_unit(int g) { return ((g & 1) << 1) | (g >> 1); }

__host__ __device__ inline bool stack_image_shape(int kind, int H, int F, int has_h, StackImageShape& s) {
    if (H < 4 || (H & 3) || H > 100) return false;
    switch (kind) {
        case SI_INPUT_FWD:
        case SI_INPUT_BWD:
            if (F < 4 || (F & 3) || F > 256) return false;
            s.ntiles = ((kind == SI_INPUT_FWD ? H : F) + 15) >> 4;
            s.nk = ((kind == SI_INPUT_FWD ? F : H) + 15) >> 4;
            s.ncb = 1;
            return true;
        case SI_LAYER_BWD:
            s.ntiles = (2 * H + 15) >> 4; s.nk = (H + 15) >> 4; s.ncb = 1;
            return true;
        case SI_GATE_FWD:
            s.ntiles = 4 * SI_UB / 16; s.nk = ((has_h ? 2 * H : H) + 15) >> 4; s.ncb = (H + SI_UB - 1) / SI_UB;
            return true;
        case SI_GATE_BWD:
            s.ntiles = SI_CBW / 16; s.nk = (4 * H + 15) >> 4; s.ncb = (has_h ? 2 : 1) * ((H + SI_CBW - 1) / SI_CBW);
            return true;
        default:
            return false;
    }
}

// Source of float j of the float4 at (column block cb, tile t, chunk kc, lane l): 0 = the image holds 0.0 there, 1 = element
// (row, col) of the first matrix (W0 / W / W_ih), 2 = element (row, col) of the second matrix (W_hh).  The shape must be valid.
__host__ __device__ inline int stack_image_src(int kind, int H, int F, int has_h, int cb, int t, int kc, int l, int j, int& row,
                                               int& col) {
    const int n = 16 * t + si_frag_row(l & 15);
    const int k = 16 * kc + 4 * si_frag_unit(l >> 4) + j;
    row = col = 0;
    switch (kind) {
        case SI_INPUT_FWD:
            if (n >= H || k >= F) return 0;
            row = n; col = k;
            return 1;
        case SI_INPUT_BWD:
            if (n >= F || k >= H) return 0;
            row = k; col = n;
            return 1;
        case SI_LAYER_BWD:
            if (n >= 2 * H || k >= H) return 0;
            row = n; col = k;
            return 1;
        case SI_GATE_FWD: {
            const int gate = n / SI_UB, ul = n - gate * SI_UB, u0 = cb * SI_UB;
            if (u0 + ul >= H || k >= (has_h ? 2 * H : H)) return 0;
            row = gate * H + u0 + ul;
            col = k < H ? k : k - H;
            return k < H ? 1 : 2;
        }
        default: {          // SI_GATE_BWD
            const int nb = (H + SI_CBW - 1) / SI_CBW;
            const int n0 = (cb >= nb ? cb - nb : cb) * SI_CBW;
            if (n >= SI_CBW || n0 + n >= H || k >= 4 * H) return 0;
            row = k; col = n0 + n;
            return cb >= nb ? 2 : 1;
        }
    }
}
