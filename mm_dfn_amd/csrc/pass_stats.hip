// K13: the pass loop's bookkeeping as one launch of the step (train.PassStats).  Per row of the (N, C) log-probabilities the
// prediction (torch.argmax's rule: lowest index among the maxima, a NaN row predicts its first NaN), and -- when the block's
// armed word is set -- the C x C confusion matrix, the row / bad-label / NaN-row counts, the sum of the batch losses in float64
// and the batch count, accumulated in device memory across the launches of a pass and read back once.
// Modelled on nll_loss.hip: ONE workgroup, fixed row -> thread assignment.  The counts go through an LDS histogram of C x C
// 64-bit counters (integer adds commute: the result does not depend on the order the waves run in, so the launch is
// bit-reproducible); the workgroup then adds the histogram to the global accumulator with ordinary loads and stores -- launches
// on one stream are serialised, so nothing else touches the block meanwhile and no global atomics are needed.
// Every index is bounded before use: a label reaches the histogram only when 0 <= t < C, pred < C by construction.
#include "mmdfn_internal.h"
#include "../../include/mmdfn_hip.h"

namespace {

constexpr int PS_NT = 1024;
constexpr int PS_MAXC = 64;          // 64 x 64 counters of 8 bytes = 32 KB of LDS
// words of meta (int64): the layout include/mmdfn_hip.h documents
constexpr int PS_ARMED = 0, PS_ROWS = 1, PS_BATCHES = 2, PS_BAD = 3, PS_NAN = 4;

__global__ __launch_bounds__(PS_NT) void pass_stats_kernel(const float* __restrict__ logp, const int64_t* __restrict__ target,
                                                           const float* __restrict__ loss, int64_t* __restrict__ pred,
                                                           int64_t* __restrict__ counts, int64_t* meta,
                                                           double* __restrict__ loss_sum, float* __restrict__ loss_hist,
                                                           int64_t N, int C, int64_t ignore_index, int slots) {
    __shared__ unsigned long long hist[PS_MAXC * PS_MAXC];
    __shared__ unsigned long long tally[3];          // rows that count, bad labels, NaN rows
    const bool armed = meta[PS_ARMED] != 0;          // (the same word for every thread: the branches below are uniform)
    const int cells = C * C;
    if (armed) {
        for (int k = threadIdx.x; k < cells; k += PS_NT) hist[k] = 0ull;
        if (threadIdx.x < 3) tally[threadIdx.x] = 0ull;
        __syncthreads();
    }
    for (int64_t i = threadIdx.x; i < N; i += PS_NT) {
        const float* row = logp + i * C;
        int best = 0;
        float bv = row[0];
        bool nan = bv != bv;
        for (int c = 1; c < C && !nan; ++c) {
            const float v = row[c];
            if (v != v) {
                best = c;
                nan = true;
            } else if (v > bv) {          // strict: the lowest index among equal maxima stays
                best = c;
                bv = v;
            }
        }
        pred[i] = best;
        if (!armed) continue;
        const int64_t t = target[i];
        if (t == ignore_index) continue;
        if (nan) atomicAdd(&tally[2], 1ull);
        if (t < 0 || t >= C) {
            atomicAdd(&tally[1], 1ull);
        } else {
            atomicAdd(&hist[(int)t * C + best], 1ull);
            atomicAdd(&tally[0], 1ull);
        }
    }
    if (!armed) return;
    __syncthreads();
    for (int k = threadIdx.x; k < cells; k += PS_NT) {
        const unsigned long long h = hist[k];
        if (h != 0ull) counts[k] += (int64_t)h;
    }
    if (threadIdx.x == 0) {
        meta[PS_ROWS] += (int64_t)tally[0];
        meta[PS_BAD] += (int64_t)tally[1];
        meta[PS_NAN] += (int64_t)tally[2];
        const int64_t k = meta[PS_BATCHES];
        if (loss != nullptr) {
            const float l = loss[0];
            loss_sum[0] += (double)l;
            if (k < slots) loss_hist[k] = l;
        }
        meta[PS_BATCHES] = k + 1;
    }
}

}  // namespace

extern "C" int mmdfn_pass_stats_threads(void) { return PS_NT; }
extern "C" int mmdfn_pass_stats_max_classes(void) { return PS_MAXC; }

extern "C" int mmdfn_pass_stats_accumulate(const float* logp, const int64_t* target, const float* loss, int64_t* pred,
                                           int64_t* counts, int64_t* meta, double* loss_sum, float* loss_hist, int64_t N, int C,
                                           int64_t ignore_index, int slots, void* stream) {
    if (N <= 0 || C <= 0 || C > PS_MAXC || slots < 0 || logp == nullptr || target == nullptr || pred == nullptr ||
        counts == nullptr || meta == nullptr || loss_sum == nullptr || (slots > 0 && loss_hist == nullptr))
        return -1;
    hipLaunchKernelGGL(pass_stats_kernel, dim3(1), dim3(PS_NT), 0, (hipStream_t)stream, logp, target, loss, pred, counts, meta,
                       loss_sum, loss_hist, N, C, ignore_index, slots);
    MMDFN_CHECK_LAUNCH();
    return 0;
}
