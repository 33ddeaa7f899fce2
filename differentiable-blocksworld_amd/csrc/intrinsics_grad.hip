// Intrinsics refinement (include/dbw_lens.h): the gradient of a render with respect to the shared pinhole matrix K, and the
// 4-vector (a_x, a_y, c_x, c_y) that refines its focal lengths and principal point.  The arithmetic is intrinsics_math.h (host + device).
//
// intrinsics_grad_kernel has the shape of pose_grad_kernel (pose_grad.hip), which stays as it is: one workgroup per (view, chunk of 256
// clipped-face slots), one lane per slot, twelve accumulators per lane (rows 0, 1 and 3 of K), lanes summed in registers (wave_sum_dpp),
// the four waves through LDS in wave order, ONE 12-float partial per workgroup.  Slots >= num_faces[b] are never read; a lane whose nine
// gradient components are all zero skips the projection.  intrinsics_finish_kernel adds ALL partials, view-major then chunk, in fp64 on
// twelve lanes and writes the sixteen floats of grad_K (row 2: zero).  No float atomics: the order of every sum is fixed and two calls give
// the same bits.
//
// intrinsics_apply_kernel / intrinsics_chain_kernel: sixteen floats of work on one lane of one wave.
#include "dbw_common.h"
#include "intrinsics_math.h"
#include "../../include/dbw_lens.h"

using namespace dbw;

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / DBW_WAVE;

__global__ __launch_bounds__(NT) void intrinsics_grad_kernel(
    const float *__restrict__ verts, const int *__restrict__ faces, const float *__restrict__ R, const float *__restrict__ T,
    const float *__restrict__ Kmat, int F, float eps, float zc, int persp, const int *__restrict__ num_faces, const int *__restrict__ c2o,
    const int *__restrict__ code, const float *__restrict__ cw, const float *__restrict__ gfvc, float *__restrict__ partial) {
    __shared__ float s_part[WAVES][12];
    const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j = chunk * NT + tid;
    bool act = j < num_faces[b] && j < 2 * F;          // (the forward counted num_faces[b] <= 2F; the view's 2F slots bound the read anyway)
    const long long o = (long long)b * 2 * F + (act ? j : 0);
    float g[9];
    if (act) {
        bool any = false;
#pragma unroll
        for (int i = 0; i < 9; ++i) { g[i] = gfvc[o * 9 + i]; any |= (g[i] != 0.f); }
        act = any;
    }
    float acc[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (act) {
        Cam cam;
        load_cam(R, T, Kmat, b, cam);
        const int f = c2o[o], cd = code[o];
        slot_k_grad(verts, faces[f * 3], faces[f * 3 + 1], faces[f * 3 + 2], cam, eps, zc, persp, cd, cw[o * 2], cw[o * 2 + 1], g, acc);
    }
#pragma unroll
    for (int c = 0; c < 12; ++c) {
        const float s = wave_sum_dpp(acc[c]);          // inactive lanes hold zeros
        if (lane == 0) s_part[wv][c] = s;
    }
    __syncthreads();
    if (tid < 12) {
        float s = s_part[0][tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += s_part[w][tid];
        partial[((long long)b * gridDim.x + chunk) * 12 + tid] = s;
    }
}

// one wave: lanes 0..11 own the accumulators (rows 0, 1, 3 of K), lanes 12..15 row 2
__global__ __launch_bounds__(DBW_WAVE) void intrinsics_finish_kernel(const float *__restrict__ partial, long long n_partials, float *__restrict__ gK,
                                                                     int accumulate) {
    const int c = threadIdx.x;
    if (c >= 16) return;
    if (c >= 12) {                                     // row 2: never read by the projection
        if (!accumulate) gK[8 + (c - 12)] = 0.f;
        return;
    }
    double s = 0.0;
    // 64 independent loads in flight per lane ahead of the dependent fp64 adds: the chain of adds, not the memory latency, is what is left
#pragma unroll 64
    for (long long k = 0; k < n_partials; ++k) s += (double)partial[k * 12 + c];          // view-major, then chunk: the order of the workspace
    float *dst = gK + (c < 8 ? c : c + 4);
    *dst = accumulate ? (float)((double)*dst + s) : (float)s;
}

__global__ __launch_bounds__(DBW_WAVE) void intrinsics_apply_kernel(const float *__restrict__ K0, const float *__restrict__ theta,
                                                                    float *__restrict__ K1) {
    if (threadIdx.x != 0) return;
    float k0[16], th[4], k1[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) k0[i] = K0[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) th[i] = theta[i];
    intrinsics_apply(k0, th, k1);
#pragma unroll
    for (int i = 0; i < 16; ++i) K1[i] = k1[i];
}

__global__ __launch_bounds__(DBW_WAVE) void intrinsics_chain_kernel(const float *__restrict__ K0, const float *__restrict__ theta,
                                                                    const float *__restrict__ gK, float *__restrict__ gtheta) {
    if (threadIdx.x != 0) return;
    float k0[16], th[4], gk[16], gt[4];
#pragma unroll
    for (int i = 0; i < 16; ++i) { k0[i] = K0[i]; gk[i] = gK[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) th[i] = theta[i];
    intrinsics_chain(k0, th, gk, gt);
#pragma unroll
    for (int i = 0; i < 4; ++i) gtheta[i] = gt[i];
}

int k_chunks(int F) { return (int)((2LL * F + NT - 1) / NT); }

}  // namespace

extern "C" size_t dbw_lens_intrinsics_grad_workspace_bytes(int B, int F) {
    if (B <= 0 || F <= 0) return 0;
    return (size_t)B * (size_t)k_chunks(F) * 12 * sizeof(float);
}

extern "C" int dbw_lens_intrinsics_grad(const float *verts_world, const int32_t *faces, const float *R, const float *T, const float *Kmat, int B,
                                        int V, int F, float eps, float z_clip, int perspective_correct, const int32_t *num_faces,
                                        const int32_t *c2o, const int32_t *clip_code, const float *clip_w, const float *grad_face_verts_c,
                                        void *workspace, size_t workspace_bytes, float *grad_K, int accumulate, dbw_stream_t stream) {
    DBW_REQUIRE(verts_world && faces && R && T && Kmat && num_faces && c2o && clip_code && clip_w && grad_face_verts_c && grad_K, "null pointer");
    DBW_REQUIRE(B >= 0 && V > 0 && F > 0, "bad size");
    DBW_REQUIRE((long long)B * 2 * F < 0x7fffffffLL && B <= 65535, "B*2F overflows int32 face indices, or more than 65535 views");
    if (B == 0) return DBW_OK;
    DBW_REQUIRE(workspace && workspace_bytes >= dbw_lens_intrinsics_grad_workspace_bytes(B, F), "workspace missing or too small");
    DBW_REQUIRE(((uintptr_t)workspace & 3) == 0, "workspace not aligned to 4 bytes");
    const int nchunks = k_chunks(F);
    hipLaunchKernelGGL(intrinsics_grad_kernel, dim3((unsigned)nchunks, (unsigned)B), dim3(NT), 0, (hipStream_t)stream, verts_world, faces, R, T, Kmat, F,
                       eps, z_clip, perspective_correct, num_faces, c2o, clip_code, clip_w, grad_face_verts_c, (float *)workspace);
    const int rc = dbw_check_launch("intrinsics_grad_kernel");
    if (rc != DBW_OK) return rc;
    hipLaunchKernelGGL(intrinsics_finish_kernel, dim3(1), dim3(DBW_WAVE), 0, (hipStream_t)stream, (const float *)workspace, (long long)B * nchunks, grad_K,
                       accumulate);
    return dbw_check_launch("intrinsics_finish_kernel");
}

extern "C" int dbw_lens_intrinsics_apply(const float *K0, const float *theta, float *K_out, dbw_stream_t stream) {
    DBW_REQUIRE(K0 && theta && K_out, "null pointer");
    hipLaunchKernelGGL(intrinsics_apply_kernel, dim3(1), dim3(DBW_WAVE), 0, (hipStream_t)stream, K0, theta, K_out);
    return dbw_check_launch("intrinsics_apply_kernel");
}

extern "C" int dbw_lens_intrinsics_chain(const float *K0, const float *theta, const float *grad_K, float *grad_theta, dbw_stream_t stream) {
    DBW_REQUIRE(K0 && theta && grad_K && grad_theta, "null pointer");
    hipLaunchKernelGGL(intrinsics_chain_kernel, dim3(1), dim3(DBW_WAVE), 0, (hipStream_t)stream, K0, theta, grad_K, grad_theta);
    return dbw_check_launch("intrinsics_chain_kernel");
}
