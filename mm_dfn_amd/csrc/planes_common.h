// Shared declarations of the kernels that multiply against bf16 PIECE PLANES (linear_planes.hip, gcn_planes.hip).
//
// Plane layout of a B operand "B[n][k]" (n < N output columns, k < K contraction):  KS = ceil(K / 16) k-steps, NT = ceil(N / 32)
// column tiles;  planes[((ct * KS + ks) * 3 + piece) * 64 + lane] = 8 bf16 (16 bytes) = piece `piece` of
// B[32 ct + (lane & 31)][16 ks + 8 (lane >> 5) + 0..7], zero outside N x K: exactly the B operand of v_mfma_f32_32x32x16_bf16.
#pragma once
#include "bf16_pieces.h"

namespace {

constexpr int PL_BM = 64;          // rows per workgroup
constexpr int PL_STG = 2;          // k-steps per phase (32 k): 2 buffers x 2 x 3 pieces x 2 row halves x 1 KB = 24 KB of LDS
constexpr int PL_LDS = 2 * PL_STG * 3 * 2 * 64;     // u32x4 elements of the A-fragment double buffer

// workgroup decode shared by the launches: grid = 8 ceil(row blocks / 8) ncb; blockIdx % 8 (the XCD) owns the row blocks = its
// number (mod 8) and runs the ncb column blocks of a row block back to back, so the A rows of a row block are fetched into ONE L2
__device__ __forceinline__ bool pl_decode(int nrb, int ncb, int& rb, int& cb, int bid) {
    const int yq = bid >> 3;
    rb = (yq / ncb) * 8 + (bid & 7);
    cb = yq % ncb;
    return rb < nrb;
}
inline int64_t pl_grid(int nrb, int ncb) { return (int64_t)((nrb + 7) / 8) * 8 * ncb; }

}  // namespace
