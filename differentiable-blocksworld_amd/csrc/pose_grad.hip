// Camera pose refinement (include/dbw_lens.h): the gradient of a render with respect to each view's R and T, and the
// per-view 6-vector that refines a pose.  The arithmetic is pose_math.h (host + device).
//
// pose_grad_kernel: project_clip_bwd_kernel sums the gradient of the clipped faces over the VIEWS into the vertices; this one sums it
// over the FACES into each view's camera.  One workgroup per (view, chunk of 256 clipped-face slots), one lane per slot: a lane does the
// per-slot work of the vertex backward (the same case analysis, the same projections) and keeps 12 accumulators, 9 for g_R and 3 for
// g_T.  Lanes are summed in registers (wave_sum_dpp), the four waves through LDS in wave order, and the workgroup leaves ONE 12-float
// partial in the workspace.  pose_finish_kernel adds a view's partials in chunk order, in fp64.  No float atomics anywhere: the order of
// every sum is fixed and two calls give the same bits.  Slots >= num_faces[b] are never read.
//
// pose_apply_kernel / pose_chain_kernel: a lane per view -- a few hundred bytes of work.  The ids of a batch are distinct (the host
// checks), so the chain writes its rows of grad_delta without atomics.
#include "dbw_common.h"
#include "pose_math.h"
#include "../../include/dbw_lens.h"

using namespace dbw;

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / DBW_WAVE;
constexpr int FIN_LANES = 16;          // lanes of a view's group in pose_finish_kernel (12 of them work)

__global__ __launch_bounds__(NT) void pose_grad_kernel(
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
        slot_cam_grad(verts, faces[f * 3], faces[f * 3 + 1], faces[f * 3 + 2], cam, eps, zc, persp, cd, cw[o * 2], cw[o * 2 + 1], g, acc);
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

__global__ __launch_bounds__(NT) void pose_finish_kernel(const float *__restrict__ partial, int B, int nchunks, float *__restrict__ gR,
                                                         float *__restrict__ gT, int accumulate) {
    const int t = blockIdx.x * NT + threadIdx.x, b = t / FIN_LANES, c = t % FIN_LANES;
    if (b >= B || c >= 12) return;
    double s = 0.0;
    for (int k = 0; k < nchunks; ++k) s += (double)partial[((long long)b * nchunks + k) * 12 + c];
    float *dst = c < 9 ? gR + b * 9 + c : gT + b * 3 + (c - 9);
    *dst = accumulate ? (float)((double)*dst + s) : (float)s;
}

__global__ __launch_bounds__(NT) void pose_apply_kernel(const float *__restrict__ R0, const float *__restrict__ T0, const float *__restrict__ delta,
                                                        const int *__restrict__ ids, int B, int V, float *__restrict__ R1, float *__restrict__ T1) {
    const int b = blockIdx.x * NT + threadIdx.x;
    if (b >= B) return;
    const int v = ids[b];
    float r0[9], t0[3], d[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, r1[9], t1[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) r0[i] = R0[b * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t0[i] = T0[b * 3 + i];
    if (v >= 0 && v < V) {                              // (an id outside the table refines nothing and touches nothing)
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = delta[(long long)v * 6 + i];
    }
    pose_apply(r0, t0, d, r1, t1);
#pragma unroll
    for (int i = 0; i < 9; ++i) R1[b * 9 + i] = r1[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) T1[b * 3 + i] = t1[i];
}

__global__ __launch_bounds__(NT) void pose_chain_kernel(const float *__restrict__ R0, const float *__restrict__ T0, const float *__restrict__ delta,
                                                        const int *__restrict__ ids, int B, int V, const float *__restrict__ gR,
                                                        const float *__restrict__ gT, float *__restrict__ gdelta) {
    const int b = blockIdx.x * NT + threadIdx.x;
    if (b >= B) return;
    const int v = ids[b];
    if (v < 0 || v >= V) return;
    float r0[9], t0[3], d[6], gr[9], gt[3], gd[6];
#pragma unroll
    for (int i = 0; i < 9; ++i) { r0[i] = R0[b * 9 + i]; gr[i] = gR[b * 9 + i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) { t0[i] = T0[b * 3 + i]; gt[i] = gT[b * 3 + i]; }
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = delta[(long long)v * 6 + i];
    pose_chain(r0, t0, d, gr, gt, gd);
#pragma unroll
    for (int i = 0; i < 6; ++i) gdelta[(long long)v * 6 + i] = gd[i];
}

int pose_chunks(int F) { return (int)((2LL * F + NT - 1) / NT); }

}  // namespace

extern "C" size_t dbw_lens_pose_grad_workspace_bytes(int B, int F) {
    if (B <= 0 || F <= 0) return 0;
    return (size_t)B * (size_t)pose_chunks(F) * 12 * sizeof(float);
}

extern "C" int dbw_lens_pose_grad(const float *verts_world, const int32_t *faces, const float *R, const float *T, const float *Kmat, int B, int V,
                                  int F, float eps, float z_clip, int perspective_correct, const int32_t *num_faces, const int32_t *c2o,
                                  const int32_t *clip_code, const float *clip_w, const float *grad_face_verts_c, void *workspace,
                                  size_t workspace_bytes, float *grad_R, float *grad_T, int accumulate, dbw_stream_t stream) {
    DBW_REQUIRE(verts_world && faces && R && T && Kmat && num_faces && c2o && clip_code && clip_w && grad_face_verts_c && grad_R && grad_T,
                "null pointer");
    DBW_REQUIRE(B >= 0 && V > 0 && F > 0, "bad size");
    DBW_REQUIRE((long long)B * 2 * F < 0x7fffffffLL && B <= 65535, "B*2F overflows int32 face indices, or more than 65535 views");
    if (B == 0) return DBW_OK;
    DBW_REQUIRE(workspace && workspace_bytes >= dbw_lens_pose_grad_workspace_bytes(B, F), "workspace missing or too small");
    DBW_REQUIRE(((uintptr_t)workspace & 3) == 0, "workspace not aligned to 4 bytes");
    const int nchunks = pose_chunks(F);
    hipLaunchKernelGGL(pose_grad_kernel, dim3((unsigned)nchunks, (unsigned)B), dim3(NT), 0, (hipStream_t)stream, verts_world, faces, R, T, Kmat, F, eps,
                       z_clip, perspective_correct, num_faces, c2o, clip_code, clip_w, grad_face_verts_c, (float *)workspace);
    int rc = dbw_check_launch("pose_grad_kernel");
    if (rc != DBW_OK) return rc;
    hipLaunchKernelGGL(pose_finish_kernel, dim3((unsigned)((B * FIN_LANES + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, (const float *)workspace, B,
                       nchunks, grad_R, grad_T, accumulate);
    return dbw_check_launch("pose_finish_kernel");
}

extern "C" int dbw_lens_pose_apply(const float *R0, const float *T0, const float *delta, const int32_t *ids, int B, int V, float *R_out, float *T_out,
                                   dbw_stream_t stream) {
    DBW_REQUIRE(R0 && T0 && delta && ids && R_out && T_out, "null pointer");
    DBW_REQUIRE(B >= 0 && V > 0, "bad size");
    if (B == 0) return DBW_OK;
    hipLaunchKernelGGL(pose_apply_kernel, dim3((unsigned)((B + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, R0, T0, delta, ids, B, V, R_out, T_out);
    return dbw_check_launch("pose_apply_kernel");
}

extern "C" int dbw_lens_pose_chain(const float *R0, const float *T0, const float *delta, const int32_t *ids, int B, int V, const float *grad_R,
                                   const float *grad_T, float *grad_delta, dbw_stream_t stream) {
    DBW_REQUIRE(R0 && T0 && delta && ids && grad_R && grad_T && grad_delta, "null pointer");
    DBW_REQUIRE(B >= 0 && V > 0, "bad size");
    if (B == 0) return DBW_OK;
    hipLaunchKernelGGL(pose_chain_kernel, dim3((unsigned)((B + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, R0, T0, delta, ids, B, V, grad_R, grad_T,
                       grad_delta);
    return dbw_check_launch("pose_chain_kernel");
}
