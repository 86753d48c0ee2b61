// Host-side argument handling of the K11 / K12 entry points under AddressSanitizer: every call below returns -1 or -2 before
// anything is launched (NULL or never-dereferenced device pointers), so the program needs no GPU.
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address -I include tools/graph_embed_args_check.cpp \
//         mm_dfn_amd/csrc/graph_embed.hip mm_dfn_amd/csrc/nll_loss.hip -o graph_embed_args_check && ./graph_embed_args_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mmdfn_hip.h"

static int failures = 0;
static void expect(const char* what, int got, int want) {
    if (got != want) {
        std::printf("FAIL %s: got %d, want %d\n", what, got, want);
        ++failures;
    }
}

int main() {
    float* aligned = reinterpret_cast<float*>(uintptr_t(0x1000));       // never dereferenced: the calls return first
    float* skew = reinterpret_cast<float*>(uintptr_t(0x1004));
    int32_t* spk = reinterpret_cast<int32_t*>(uintptr_t(0x2000));
    const int64_t* idx = reinterpret_cast<const int64_t*>(uintptr_t(0x3000));
    // the slot table is read on the host: exactly M entries, on the heap so that a read past them is seen
    auto rows = [](std::initializer_list<int32_t> v) { return std::vector<int32_t>(v); };
    auto fwd = [&](const float* X, const float* sp, const float* mo, const std::vector<int32_t>& r, int l, float* Y, int M, int D,
                   int P, int S) {
        return mmdfn_graph_embed_fwd(X, aligned, idx, sp, mo, r.empty() ? nullptr : r.data(), l, Y, spk, M, 5, D, P, S, 40, nullptr);
    };
    expect("null X", fwd(nullptr, aligned, aligned, rows({0, 1, 2}), 2, aligned, 3, 8, 2, 2), -1);
    expect("null rows", fwd(aligned, aligned, aligned, rows({}), 2, aligned, 3, 8, 2, 2), -1);
    expect("M = 0", fwd(aligned, aligned, aligned, rows({0}), -1, aligned, 0, 8, 2, 2), -1);
    expect("M = 4", fwd(aligned, aligned, aligned, rows({0, 1, 2, 2}), 2, aligned, 4, 8, 2, 2), -1);
    expect("row 3", fwd(aligned, aligned, aligned, rows({0, 3}), -1, aligned, 2, 8, 2, 2), -1);
    expect("duplicate row", fwd(aligned, aligned, aligned, rows({1, 1}), -1, aligned, 2, 8, 2, 2), -1);
    expect("l in the wrong slot", fwd(aligned, aligned, aligned, rows({0, 2}), 0, aligned, 2, 8, 2, 2), -1);
    expect("l_slot past M", fwd(aligned, aligned, aligned, rows({0, 2}), 2, aligned, 2, 8, 2, 2), -1);
    expect("P > S", fwd(aligned, aligned, aligned, rows({0, 1, 2}), 2, aligned, 3, 8, 3, 2), -1);
    expect("D = 6", fwd(aligned, aligned, aligned, rows({0, 1, 2}), 2, aligned, 3, 6, 2, 2), -2);
    expect("X off the grid", fwd(skew, aligned, aligned, rows({0, 1, 2}), 2, aligned, 3, 8, 2, 2), -2);
    expect("Y off the grid", fwd(aligned, aligned, aligned, rows({0, 1, 2}), 2, skew, 3, 8, 2, 2), -2);
    expect("speaker table off the grid", fwd(aligned, skew, aligned, rows({0, 2}), 1, aligned, 2, 8, 2, 2), -2);
    expect("modal table off the grid", fwd(aligned, nullptr, skew, rows({0, 1}), -1, aligned, 2, 8, 2, 2), -2);
    expect("too many speakers", fwd(aligned, aligned, aligned, rows({0, 1, 2}), 2, aligned, 3, 8, 2,
                                    mmdfn_graph_embed_max_speakers() + 1), -2);
    auto bwd = [&](const float* dY, float* ds, float* dm, const std::vector<int32_t>& r, int l, int M, int D, int S) {
        return mmdfn_graph_embed_bwd(dY, spk, ds, dm, r.empty() ? nullptr : r.data(), l, M, 5, D, S, nullptr);
    };
    expect("bwd null dY", bwd(nullptr, aligned, aligned, rows({0, 1, 2}), 2, 3, 8, 2), -1);
    expect("bwd nothing to compute", bwd(aligned, nullptr, nullptr, rows({0, 1, 2}), 2, 3, 8, 2), -1);
    expect("bwd speaker table without l and no modal table", bwd(aligned, aligned, nullptr, rows({0, 1}), -1, 2, 8, 2), -1);
    expect("bwd bad rows", bwd(aligned, aligned, aligned, rows({2, 0}), 1, 2, 8, 2), -1);
    expect("bwd D = 6", bwd(aligned, aligned, aligned, rows({0, 1, 2}), 2, 3, 6, 2), -2);
    expect("bwd dY off the grid", bwd(skew, aligned, aligned, rows({0, 1, 2}), 2, 3, 8, 2), -2);
    expect("bwd too many speakers", bwd(aligned, aligned, aligned, rows({0, 1, 2}), 2, 3, 8, 16), -2);
    expect("nll null logp", mmdfn_nll_loss_fwd(nullptr, idx, nullptr, aligned, aligned, aligned, 4, 6, 1, -100, nullptr), -1);
    expect("nll N = 0", mmdfn_nll_loss_fwd(aligned, idx, nullptr, aligned, aligned, aligned, 0, 6, 1, -100, nullptr), -1);
    expect("nll bwd null scale", mmdfn_nll_loss_bwd(aligned, idx, aligned, nullptr, aligned, 4, 6, -100, nullptr), -1);
    std::printf(failures ? "%d failures\n" : "all argument checks answered as documented\n", failures);
    return failures ? 1 : 0;
}
