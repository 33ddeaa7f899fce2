// The launch of the exact nearest-neighbour search (nn_search.hip) for the callers inside the library: dbw_nn_points and the gradient ICP
// (icp_align.hip), which reads the 64-bit keys (dist2 bits << 32 | idx, dbw::nn_key) directly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The number of y ranges a search of these sizes runs with: `splits` itself where positive (clamped to P2), chosen from the sizes and the
// chip where 0.  Negative (DBW_ERR_INVALID, text set under the name `caller`, the entry point's) when the grid would be too large.  No launch.
int dbw_nn_search_plan(const char *caller, int N, int P1, int P2, int splits);

// keys[n * P1 + i] = the key of x[n, i]'s nearest neighbour among y[n, :]; splits from dbw_nn_search_plan.  keys: N * P1 uint64.
int dbw_nn_search_launch(const float *x, const float *y, const int64_t *x_lengths, const int64_t *y_lengths, int N, int P1, int P2,
                         int splits, void *keys, hipStream_t st);
