// What the three image terms of the loss share (ssim_term.hip, masked_loss.hip, exposure_loss.hip): the fixed-order fp64 sum of a
// workgroup of 256 threads, the one-workgroup launch that adds the workgroups' partials, and a lane's 16-byte or element loads and stores
// of the layers' planes.  No atomics anywhere: the bits of a value do not depend on the schedule.
#pragma once
#include "dbw_common.h"

namespace dbw {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_WAVES = LOSS_THREADS / DBW_WAVE;

// NS sums of the workgroup: the wave through fixed-order butterflies (32 .. 1), the waves in wave order from red[0]; thread k < NS leaves
// with sum k, every other thread with 0.  Its barrier lies between the callers' work before it and after it.
template <int NS>
__device__ __forceinline__ double block_sums(double (&s)[NS], double (*red)[NS]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_xor(s[k], off, DBW_WAVE);
    }
    if ((tid & (DBW_WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) red[tid / DBW_WAVE][k] = s[k];
    }
    __syncthreads();
    double t = 0.0;
    if (tid < NS) {
        t = red[0][tid];
        for (int w = 1; w < LOSS_WAVES; ++w) t += red[w][tid];
    }
    return t;
}

// One sum, on a scalar: the same operations in the same order, the result in thread 0.  (ssim_term_kernel needs this form: one value sent
// through the array form reaches the optimiser as memory until the k loops are unrolled, and the kernel's column pass is then packed
// into other instructions: profiles/ssim_term.md.)
__device__ __forceinline__ double block_sum(double s, double (*red)[1]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, DBW_WAVE);
    if ((tid & (DBW_WAVE - 1)) == 0) red[tid / DBW_WAVE][0] = s;
    __syncthreads();
    double t = 0.0;
    if (tid == 0) {
        t = red[0][0];
        for (int w = 1; w < LOSS_WAVES; ++w) t += red[w][0];
    }
    return t;
}

// value[0] = (the partials added in a fixed order) * mul / div, 0 where div is not positive: thread t adds t, t + 256, ... in index order,
// the 256 sums go through block_sums.  (mul = 1 and div = 1 are exact: a caller with one factor passes 1 for the other.)
static __global__ void __launch_bounds__(LOSS_THREADS) partials_finish_kernel(const double *__restrict__ partial, long long count, double mul,
                                                                              double div, double *__restrict__ value) {
    __shared__ double red[LOSS_WAVES][1];
    double s[1] = {0.0};
    for (long long i = threadIdx.x; i < count; i += LOSS_THREADS) s[0] += partial[i];
    const double t = block_sums<1>(s, red);
    if (threadIdx.x == 0) value[0] = div > 0.0 ? (t * mul) / div : 0.0;
}

static inline int partials_finish(const double *partial, long long count, double mul, double div, double *value, hipStream_t s) {
    hipLaunchKernelGGL(partials_finish_kernel, dim3(1), dim3(LOSS_THREADS), 0, s, partial, count, mul, div, value);
    return dbw_check_launch("partials_finish_kernel");
}

// ---- a lane's PX = 4 (one 16-byte access) or 1 adjacent pixels of a plane --------------------------------------------------------------------
template <int PX>
__device__ __forceinline__ void load_px(const float *p, float v[PX]) {
    if constexpr (PX == 4) {
        const float4 t = *(const float4 *)p;
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}

template <int PX>
__device__ __forceinline__ void store_px(float *p, const float v[PX]) {
    if constexpr (PX == 4) *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

// what the composite kernels read of pixel p of image n -- fg, env (N,4,plane), img, grad_rec (N,3,plane), msk (N,1,plane): fg and env rgb,
// the target, grad_rec (zeros without one), alpha, the mask (ones without one)
template <int PX>
__device__ __forceinline__ void load_layers_px(const float *fg, const float *env, const float *img, const float *grad_rec, const float *msk,
                                               bool has_extra, bool has_mask, long long n, long long p, long long plane, float fc[3][PX],
                                               float ec[3][PX], float tc[3][PX], float xc[3][PX], float al[PX], float mk[PX]) {
    const float *f = fg + n * 4 * plane + p, *e = env + n * 4 * plane + p, *t = img + n * 3 * plane + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        load_px<PX>(f + c * plane, fc[c]);
        load_px<PX>(e + c * plane, ec[c]);
        load_px<PX>(t + c * plane, tc[c]);
#pragma unroll
        for (int k = 0; k < PX; ++k) xc[c][k] = 0.f;
        if (has_extra) load_px<PX>(grad_rec + n * 3 * plane + c * plane + p, xc[c]);
    }
    load_px<PX>(f + 3 * plane, al);
#pragma unroll
    for (int k = 0; k < PX; ++k) mk[k] = 1.f;
    if (has_mask) load_px<PX>(msk + n * plane + p, mk);
}

// the eight gradient planes of pixel p of image n: grad_fg, grad_env (N,4,plane)
template <int PX>
__device__ __forceinline__ void store_layer_grads_px(float *gfg, float *genv, long long n, long long p, long long plane, const float gf[4][PX],
                                                     const float ge[4][PX]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        store_px<PX>(gfg + n * 4 * plane + c * plane + p, gf[c]);
        store_px<PX>(genv + n * 4 * plane + c * plane + p, ge[c]);
    }
}

}  // namespace dbw
