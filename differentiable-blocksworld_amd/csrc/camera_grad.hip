// Camera-side gradients of a render (include/dbw_lens.h): with respect to each view's R and T (pose refinement) and to the
// shared pinhole matrix K (intrinsics refinement), and the small vectors that refine them -- a 6-vector per view for a pose, (a_x, a_y, c_x,
// c_y) for K.  The arithmetic is camera_math.h, pose_math.h and intrinsics_math.h (host + device).
//
// camera_partials_kernel<Sink>: project_clip_bwd_kernel sums the gradient of the clipped faces over the VIEWS into the vertices; this one
// sums it over the FACES into twelve accumulators of the view's camera -- 9 for g_R and 3 for g_T (CamGradSink), or rows 0, 1 and 3 of g_K
// (KGradSink).  One workgroup per (view, chunk of 256 clipped-face slots), one lane per slot: a lane walks its slot through
// camera_math.h::clip_slot_walk (the case analysis and the projections of the vertex backward) into the sink.  Lanes are summed in registers
// (wave_sum_dpp), the four waves through LDS in wave order, and the workgroup leaves ONE 12-float partial in the workspace.  Slots >=
// num_faces[b] are never read; a lane whose nine gradient components are all zero skips the projection.
//
// The two finish kernels add the partials in fp64, each in the order its call documents: pose_finish_kernel a view's partials in chunk order
// (a lane per view and component), intrinsics_finish_kernel ALL partials, view-major then chunk, on twelve lanes, writing the sixteen floats
// of grad_K (row 2: zero).  No float atomics anywhere: the order of every sum is fixed and two calls give the same bits.
//
// pose_apply_kernel / pose_chain_kernel: a lane per view -- a few hundred bytes of work.  The ids of a batch are distinct (the host
// checks), so the chain writes its rows of grad_delta without atomics.  intrinsics_apply_kernel / intrinsics_chain_kernel: sixteen floats
// of work on one lane of one wave.
#include "dbw_common.h"
#include "pose_math.h"
#include "intrinsics_math.h"
#include "../../include/dbw_lens.h"

using namespace dbw;

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / DBW_WAVE;
constexpr int FIN_LANES = 16;          // lanes of a view's group in pose_finish_kernel (12 of them work)

template <class Sink>
__global__ __launch_bounds__(NT) void camera_partials_kernel(
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
        clip_slot_walk(verts, faces[f * 3], faces[f * 3 + 1], faces[f * 3 + 2], cam, eps, zc, persp, cd, cw + o * 2, g, Sink{verts, cam, eps, acc});
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

int slot_chunks(int F) { return (int)((2LL * F + NT - 1) / NT); }

size_t partials_bytes(int B, int F) {
    if (B <= 0 || F <= 0) return 0;
    return (size_t)B * (size_t)slot_chunks(F) * 12 * sizeof(float);
}

// What dbw_lens_pose_grad and dbw_lens_intrinsics_grad share: the argument checks (reported under the name `fn` of the call) and the
// partials launch.  `outputs` = the call's output pointers are all there.  *nchunks = 0: nothing to do (B == 0, no launch).  Otherwise the
// workspace holds B * *nchunks partials, view-major.
template <class Sink>
int launch_camera_partials(const char *fn, const float *verts_world, const int32_t *faces, const float *R, const float *T, const float *Kmat, int B, int V,
                           int F, float eps, float z_clip, int perspective_correct, const int32_t *num_faces, const int32_t *c2o,
                           const int32_t *clip_code, const float *clip_w, const float *grad_face_verts_c, void *workspace, size_t workspace_bytes,
                           bool outputs, hipStream_t stream, int *nchunks) {
#define CAM_REQUIRE(cond, msg)                      \
    do {                                            \
        if (!(cond)) {                              \
            dbw_set_error("%s: %s", fn, msg);       \
            return DBW_ERR_INVALID;                 \
        }                                           \
    } while (0)
    *nchunks = 0;
    CAM_REQUIRE(verts_world && faces && R && T && Kmat && num_faces && c2o && clip_code && clip_w && grad_face_verts_c && outputs, "null pointer");
    CAM_REQUIRE(B >= 0 && V > 0 && F > 0, "bad size");
    CAM_REQUIRE((long long)B * 2 * F < 0x7fffffffLL && B <= 65535, "B*2F overflows int32 face indices, or more than 65535 views");
    if (B == 0) return DBW_OK;
    CAM_REQUIRE(workspace && workspace_bytes >= partials_bytes(B, F), "workspace missing or too small");
    CAM_REQUIRE(((uintptr_t)workspace & 3) == 0, "workspace not aligned to 4 bytes");
#undef CAM_REQUIRE
    *nchunks = slot_chunks(F);
    hipLaunchKernelGGL(camera_partials_kernel<Sink>, dim3((unsigned)*nchunks, (unsigned)B), dim3(NT), 0, stream, verts_world, faces, R, T, Kmat, F, eps,
                       z_clip, perspective_correct, num_faces, c2o, clip_code, clip_w, grad_face_verts_c, (float *)workspace);
    return dbw_check_launch("camera_partials_kernel");
}

}  // namespace

extern "C" size_t dbw_lens_pose_grad_workspace_bytes(int B, int F) { return partials_bytes(B, F); }
extern "C" size_t dbw_lens_intrinsics_grad_workspace_bytes(int B, int F) { return partials_bytes(B, F); }

extern "C" int dbw_lens_pose_grad(const float *verts_world, const int32_t *faces, const float *R, const float *T, const float *Kmat, int B, int V,
                                  int F, float eps, float z_clip, int perspective_correct, const int32_t *num_faces, const int32_t *c2o,
                                  const int32_t *clip_code, const float *clip_w, const float *grad_face_verts_c, void *workspace,
                                  size_t workspace_bytes, float *grad_R, float *grad_T, int accumulate, dbw_stream_t stream) {
    int nchunks;
    const int rc = launch_camera_partials<CamGradSink>(__func__, verts_world, faces, R, T, Kmat, B, V, F, eps, z_clip, perspective_correct, num_faces,
                                                       c2o, clip_code, clip_w, grad_face_verts_c, workspace, workspace_bytes, grad_R && grad_T,
                                                       (hipStream_t)stream, &nchunks);
    if (rc != DBW_OK || nchunks == 0) return rc;
    hipLaunchKernelGGL(pose_finish_kernel, dim3((unsigned)((B * FIN_LANES + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, (const float *)workspace, B,
                       nchunks, grad_R, grad_T, accumulate);
    return dbw_check_launch("pose_finish_kernel");
}

extern "C" int dbw_lens_intrinsics_grad(const float *verts_world, const int32_t *faces, const float *R, const float *T, const float *Kmat, int B,
                                        int V, int F, float eps, float z_clip, int perspective_correct, const int32_t *num_faces,
                                        const int32_t *c2o, const int32_t *clip_code, const float *clip_w, const float *grad_face_verts_c,
                                        void *workspace, size_t workspace_bytes, float *grad_K, int accumulate, dbw_stream_t stream) {
    int nchunks;
    const int rc = launch_camera_partials<KGradSink>(__func__, verts_world, faces, R, T, Kmat, B, V, F, eps, z_clip, perspective_correct,
                                                     num_faces, c2o, clip_code, clip_w, grad_face_verts_c, workspace, workspace_bytes, grad_K != nullptr,
                                                     (hipStream_t)stream, &nchunks);
    if (rc != DBW_OK || nchunks == 0) return rc;
    hipLaunchKernelGGL(intrinsics_finish_kernel, dim3(1), dim3(DBW_WAVE), 0, (hipStream_t)stream, (const float *)workspace, (long long)B * nchunks, grad_K,
                       accumulate);
    return dbw_check_launch("intrinsics_finish_kernel");
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
