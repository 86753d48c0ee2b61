// Dropout of the TFN fusion tensor (tensor_fusion.hip): the keep flag of element (n, k) of Z is never stored -- it is a pure
// function of (seed, offset, n, k), so the forward product, both backward products and the debug export regenerate it.
//
//   counter(n, k) = offset + n * ceil(K / 8) + (k >> 3)          (one Philox4x32-10 call = 128 bits = the 8 flags of a group of
//   keep(n, k)    = 16-bit draw (k & 7) of that call < threshold  8 consecutive k of one row: thresholds as keep_flags_body.h)
//
// Rows are padded to whole groups, so a call never serves two rows and the map depends on no grid, tile or slab choice; one
// call of the operator consumes the counters offset .. offset + N ceil(K / 8) of the package's generator stream (ops_flags).
#pragma once
#include "keep_flags_body.h"

namespace tfnk {

struct Keep {
    const unsigned long long* used;      // (seed, offset) the forward call took from the generator state; null: no dropout
    uint32_t threshold;                  // keep * 65536 (65536: everything kept)
    float scale;                         // 1 / keep (0 when nothing is kept)
};

__host__ __device__ __forceinline__ int64_t groups_per_row(int64_t K) { return (K + 7) >> 3; }

// THE generator: the 8 draws of group g (k = 8 g .. 8 g + 7) of row n
__device__ __forceinline__ uint4 draw8(unsigned long long seed, unsigned long long offset, int64_t n, int64_t gpr, int64_t g) {
    const unsigned long long c = offset + (unsigned long long)(n * gpr + g);
    return kfb::philox4x32_10(make_uint4((uint32_t)c, (uint32_t)(c >> 32), 0u, 0u),
                              make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}

// draw j (= k & 7) of a group: the order of keep_flags_body.h (x low, x high, y low, ...)
__device__ __forceinline__ uint32_t draw16(const uint4& r, int j) {
    const uint32_t lo = (j & 4) ? r.z : r.x, hi = (j & 4) ? r.w : r.y;
    const uint32_t d = (j & 2) ? hi : lo;
    return (j & 1) ? (d >> 16) : (d & 0xFFFFu);
}

}  // namespace tfnk
