// Cut kernel of the GCN stack's weight fragment images (stack_image_map.h): one grouped launch writes up to 16 images, one
// thread per output float4.  A float of an image is bit-for-bit a float of the parameter or 0.0; the map from image position
// to parameter element is the host-callable stack_image_src(), which mmdfn_stack_image_source exposes to the tests.
#include "mmdfn_internal.h"
#include "../../include/mmdfn_hip.h"
#include "stack_image_map.h"

namespace {

constexpr int SI_MAXW = 16;        // images per cut launch

struct StackCutTable {
    const float* w1[SI_MAXW];
    const float* w2[SI_MAXW];      // W_hh of the gate kinds (null otherwise / without a previous state)
    float4* image[SI_MAXW];
    int kind[SI_MAXW], H[SI_MAXW], F[SI_MAXW], has_h[SI_MAXW], ld[SI_MAXW];
    int ntiles[SI_MAXW], nk[SI_MAXW];
    int prefix[SI_MAXW + 1];       // float4 slots before image i
    int n;
};

__global__ __launch_bounds__(256) void cut_stack_images_kernel(StackCutTable T) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= T.prefix[T.n]) return;
    int i = 0;
    while (i + 1 < T.n && g >= T.prefix[i + 1]) ++i;
    const int s = g - T.prefix[i];
    const int l = s & 63, f = s >> 6;               // f = (cb * ntiles + t) * nk + kc
    const int kc = f % T.nk[i], ct = f / T.nk[i];
    const int t = ct % T.ntiles[i], cb = ct / T.ntiles[i];
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int row, col;
        const int src = stack_image_src(T.kind[i], T.H[i], T.F[i], T.has_h[i], cb, t, kc, l, j, row, col);
        v[j] = src == 0 ? 0.f : (src == 1 ? T.w1[i] : T.w2[i])[(int64_t)row * T.ld[i] + col];
    }
    T.image[i][s] = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace

extern "C" int64_t mmdfn_stack_images_workspace(int kind, int H, int F, int has_h) {
    StackImageShape s;
    if (!stack_image_shape(kind, H, F, has_h, s)) return -1;
    return (int64_t)s.ncb * s.ntiles * s.nk * 64 * (int64_t)sizeof(float4);
}

extern "C" int mmdfn_stack_image_source(int kind, int H, int F, int has_h, int cb, int t, int kc, int lane, int j, int* row,
                                        int* col) {
    StackImageShape s;
    if (!stack_image_shape(kind, H, F, has_h, s) || !row || !col) return -1;
    if (cb < 0 || cb >= s.ncb || t < 0 || t >= s.ntiles || kc < 0 || kc >= s.nk || lane < 0 || lane >= 64 || j < 0 || j >= 4)
        return -1;
    return stack_image_src(kind, H, F, has_h, cb, t, kc, lane, j, *row, *col);
}

extern "C" int mmdfn_cut_stack_images(int n, const int* kind, const float* const* w1, const float* const* w2, const int* H,
                                      const int* F, const int* has_h, float* const* image, void* stream) {
    if (n <= 0 || n > SI_MAXW || !kind || !w1 || !w2 || !H || !F || !has_h || !image) return -1;
    StackCutTable T = {};
    T.n = n;
    T.prefix[0] = 0;
    for (int i = 0; i < n; ++i) {
        StackImageShape s;
        if (!stack_image_shape(kind[i], H[i], F[i], has_h[i], s) || !w1[i] || !image[i]) return -1;
        const bool gate = kind[i] == SI_GATE_FWD || kind[i] == SI_GATE_BWD;
        if (gate && has_h[i] && !w2[i]) return -1;
        if (((uintptr_t)image[i] & 15) != 0) return -1;
        T.w1[i] = w1[i]; T.w2[i] = w2[i]; T.image[i] = reinterpret_cast<float4*>(image[i]);
        T.kind[i] = kind[i]; T.H[i] = H[i]; T.F[i] = F[i]; T.has_h[i] = has_h[i];
        T.ld[i] = (kind[i] == SI_INPUT_FWD || kind[i] == SI_INPUT_BWD) ? F[i] : H[i];      // contiguous parameters
        T.ntiles[i] = s.ntiles; T.nk[i] = s.nk;
        T.prefix[i + 1] = T.prefix[i] + s.ncb * s.ntiles * s.nk * 64;
    }
    hipLaunchKernelGGL(cut_stack_images_kernel, dim3((T.prefix[n] + 255) / 256), dim3(256), 0, (hipStream_t)stream, T);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
