// Checker-side build of the 3D evaluation arithmetic (differentiable-blocksworld_amd/csrc/nn_math.h, the header nn_search.hip compiles) for
// the host; tests/test_eval3d_host.py compares it with numpy, torch and the reference's golden DTU lattice without a GPU.  Test
// infrastructure only.
#include "../differentiable-blocksworld_amd/csrc/nn_math.h"

using namespace dbw;

extern "C" {

void host_nn_dist2(const float *x, const float *y, long long n, float *d2) {
    for (long long i = 0; i < n; ++i) d2[i] = nn_dist2(x[i * 3], x[i * 3 + 1], x[i * 3 + 2], y[i * 3], y[i * 3 + 1], y[i * 3 + 2]);
}

void host_lattice_counts(const double *tri, long long F, long long *counts) {
    for (long long f = 0; f < F; ++f) counts[f] = lattice_count(tri + f * 9);
}

// points of all faces back to back (offsets = exclusive scan of counts)
void host_lattice_points(const double *tri, long long F, const long long *counts, const long long *offsets, double *out) {
    for (long long f = 0; f < F; ++f) lattice_emit(tri + f * 9, out + offsets[f] * 3, counts[f]);
}
}
