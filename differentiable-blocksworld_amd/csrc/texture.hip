// Texture-side kernels: sigmoid + decimation (dbw.py:273-278,288-293,306,331-334), TV regulariser with gradient
// (dbw.py:378-387, loss.py:46) and the fused decoupled composite + MSE forward/backward (dbw.py:223,366-367).
// All are streaming, HBM-bound passes over O(10 MB) per optimisation step (not per view).
#include "dbw_common.h"
#include "loss_math.h"
#include "texture_body.h"
#include "step_kernels.h"
#include "../../include/dbw_hip.h"

#include <string.h>
#include <algorithm>

using namespace dbw;

namespace {

constexpr int NT = 256;

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ float block_sum(float v, float *s_red) {  // NT threads, returns the total in every thread
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) s_red[wv] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < NT / DBW_WAVE; ++w) t += s_red[w];
    return t;
}

__global__ __launch_bounds__(256) void texture_prep_fwd_kernel(const float *__restrict__ tex, int n, int h, int w, int d,
                                                               float *__restrict__ maps, float *__restrict__ sig) {
    texture_prep_fwd_body(tex, n, h, w, d, maps, sig, blockIdx.x, gridDim.x);
}

// several texture sets in ONE launch (blockIdx.y = set): the three maps of a scene (blocks, sky, ground) differ in shape, and one
// 5 us launch each is all they cost
constexpr int MAX_SETS = 4;
struct TextureSets { dbw_texture_set s[MAX_SETS]; };

__global__ __launch_bounds__(256) void texture_prep_fwd_sets_kernel(const TextureSets S) {
    const dbw_texture_set &t = S.s[blockIdx.y];
    texture_prep_fwd_body(t.texture, t.n, t.h, t.w, t.decim, t.maps, t.sig, blockIdx.x, gridDim.x);
}

__global__ void texture_prep_bwd_kernel(const float *__restrict__ tex, int n, int h, int w, int d,
                                        const float *__restrict__ gmaps, const float *__restrict__ gsig,
                                        float *__restrict__ gtex) {
    texture_prep_bwd_body(tex, n, h, w, d, gmaps, gsig, gtex, blockIdx.x, gridDim.x);
}

__global__ void texture_prep_bwd_sets_kernel(const TextureSets S) {
    const dbw_texture_set &t = S.s[blockIdx.y];
    texture_prep_bwd_body(t.texture, t.n, t.h, t.w, t.decim, t.grad_maps, t.grad_sig, t.grad_texture, blockIdx.x, gridDim.x);
}

// one thread per texel (its three channels); blockIdx.y = row (map * h + y): no integer division anywhere
__device__ __forceinline__ void tv_l2sq_body(const float *__restrict__ m, int n, int h, int w, int wrap,
                                             float scale, float *__restrict__ loss, float *__restrict__ gm, float *s_red) {
    const float sx = 1.f / ((float)h * (float)(w - 1 + (wrap ? 1 : 0)));
    const float sy = 1.f / ((float)(h - 1) * (float)w);
    float part = 0.f;
    for (int row = blockIdx.y; row < n * h; row += gridDim.y) {
        const int y = row % h;
        const float *r = m + (long long)row * w * 3;
        for (int x = blockIdx.x * NT + threadIdx.x; x < w; x += gridDim.x * NT) {
            float g3[3];
            part += tv_l2sq_texel(r, x, y, w, h, wrap, sx, sy, g3);
            if (gm) {
#pragma unroll
                for (int c = 0; c < 3; ++c) gm[((long long)row * w + x) * 3 + c] = scale * g3[c];
            }
        }
    }
    const float tot = block_sum(part, s_red);
    if (threadIdx.x == 0 && tot != 0.f) unsafeAtomicAdd(loss, scale * tot);
}

__global__ __launch_bounds__(NT) void tv_l2sq_kernel(const float *__restrict__ m, int n, int h, int w, int wrap,
                                                     float scale, float *__restrict__ loss, float *__restrict__ gm) {
    __shared__ float s_red[NT / DBW_WAVE];
    tv_l2sq_body(m, n, h, w, wrap, scale, loss, gm, s_red);
}

__global__ __launch_bounds__(NT) void tv_l2sq_sets_kernel(const TextureSets S, float *__restrict__ loss) {
    __shared__ float s_red[NT / DBW_WAVE];
    const dbw_texture_set &t = S.s[blockIdx.z];
    tv_l2sq_body(t.sig, t.n, t.h, t.w, t.wrap_x, t.tv_scale, loss, t.grad_sig_out, s_red);
}

// 1024-thread blocks: the loss is one atomic per block on a single address (~9 ns each when they queue up), so the same number of
// threads in 4x fewer blocks shortens the tail of the forward (loss-only) launch
constexpr int CNT = 1024;
__global__ __launch_bounds__(CNT) void composite_mse_kernel(const float *__restrict__ fg, const float *__restrict__ env,
                                                           const float *__restrict__ img, int N, long long plane,
                                                           float scale, const float *__restrict__ scale_dev, float *__restrict__ rec,
                                                           float *__restrict__ loss, float *__restrict__ gfg,
                                                           float *__restrict__ genv) {
    __shared__ float s_red[CNT / DBW_WAVE];
    const long long total = (long long)N * plane;
    float part = 0.f;
    const float loss_scale = scale;
    if (scale_dev) scale *= scale_dev[0];
    for (long long i0 = (long long)blockIdx.x * CNT; i0 < total; i0 += (long long)gridDim.x * CNT) {
        const long long i = i0 + threadIdx.x;
        if (i < total) {
            const long long n = i / plane, p = i % plane;
            const float *f = fg + n * 4 * plane + p, *e = env + n * 4 * plane + p;
            const float *t = img ? img + n * 3 * plane + p : nullptr;
            const float mask = f[3 * plane];
            const float fc3[3] = {f[0], f[plane], f[2 * plane]}, ec3[3] = {e[0], e[plane], e[2 * plane]};
            const float t3[3] = {t ? t[0] : 0.f, t ? t[plane] : 0.f, t ? t[2 * plane] : 0.f};
            float rec3[3], gf3[3], ge3[3], gmask = 0.f;
            part += composite_mse_pixel(fc3, mask, ec3, t3, t != nullptr, 2.f * scale, rec3, gf3, ge3, gmask);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (rec) rec[n * 3 * plane + c * plane + p] = rec3[c];
                if (gfg) { gfg[n * 4 * plane + c * plane + p] = gf3[c]; genv[n * 4 * plane + c * plane + p] = ge3[c]; }
            }
            if (gfg) { gfg[n * 4 * plane + 3 * plane + p] = gmask; genv[n * 4 * plane + 3 * plane + p] = 0.f; }
        }
    }
    part = wave_sum(part);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0 && loss) {
        float tot = 0.f;
        for (int w = 0; w < CNT / DBW_WAVE; ++w) tot += s_red[w];
        unsafeAtomicAdd(loss, tot * loss_scale);
    }
}

__global__ void adam_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                            float *__restrict__ v, long long n, float step_size, float beta1, float beta2, float eps,
                            float bc2_sqrt) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        adam_update(p[i], g[i], m[i], v[i], step_size, beta1, beta2, eps, bc2_sqrt);
    }
}

struct AdamGroups { long long end[MAX_SETS]; float step_size[MAX_SETS]; };

// parameter groups that differ in learning rate only (optimizer.py:6-18: textures vs everything else), contiguous in one flat buffer
// zero_buf: scratch the NEXT step expects zero-initialised (the per-step zero arena): cleared here, at the end of a step, so that the
// next step does not open with a fill launch in front of its first kernel
__global__ void adam_groups_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                                   long long n, const AdamGroups G, float beta1, float beta2, float eps, float bc2_sqrt,
                                   uint4 *__restrict__ zero_buf, long long zero_vec, const float *__restrict__ skip_flag) {
    // (skip_flag: a training step whose cross-stream wait gave up -- its gradients may be incomplete -- moves nothing; the flag lies
    // outside zero_buf and nobody writes it while this launch runs)
    if (skip_flag && *skip_flag != 0.f) n = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float step_size = G.step_size[0];
#pragma unroll
        for (int k = 1; k < MAX_SETS; ++k) step_size = i >= G.end[k - 1] ? G.step_size[k] : step_size;
        adam_update(p[i], g[i], m[i], v[i], step_size, beta1, beta2, eps, bc2_sqrt);
    }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < zero_vec; i += (long long)gridDim.x * blockDim.x)
        zero_buf[i] = make_uint4(0u, 0u, 0u, 0u);
}

__device__ __forceinline__ float group_step_size(const AdamGroups &G, long long i) {
    float step_size = G.step_size[0];
#pragma unroll
    for (int k = 1; k < MAX_SETS; ++k) step_size = i >= G.end[k - 1] ? G.step_size[k] : step_size;
    return step_size;
}

// The training step's last launch (step_kernels.h: AdamTailArgs): the backward of the texture preparation of up to two sets whose texture and
// gradient lie in the flat buffers, Adam on both lr groups with those gradients from registers, the run's void latch and the zero-arena clear.
// The prepared maps' gradients lie in the arena (the hole): they are cleared by the lanes that read them, never by the arena loop.  The
// grid is split by the amount of work: the first `nenv` workgroups run the texture sets, the others Adam on the remaining elements (a
// compacted index that steps over the sets' ranges), so that neither half waits for the other's stragglers.
struct AdamTex { const float *tex; const float *gsig; float *gmaps; int n, h, w, d; long long off; };
struct AdamTailK {
    float *p, *g, *m, *v; long long n; AdamGroups G; float beta1, beta2, eps, bc2_sqrt;
    uint4 *zero_buf; long long zero_vec, hole_lo, hole_hi;
    AdamTex t[2]; int ntex, clear_maps, nenv;
    long long skip_lo[2], skip_len[2];       // the sets' ranges in ascending order (unused: lo = n, len = 0)
    const float *void_raised; float *void_flag;
};

// the backward of one set's texture preparation -- the same arithmetic as texture_prep_bwd_body, element by element -- and Adam on its
// elements, by threads etid of neth
__device__ __forceinline__ void adam_tex_set(const AdamTailK &A, const AdamTex &t, bool skip, long long etid, long long neth) {
    if (t.d <= 1) {
        const long long total = (long long)t.n * t.h * t.w * 3;
        for (long long i = etid; i < total; i += neth) {
            float oms;          // 1 - s
            const float s = tex_sigmoid(t.tex[i], oms);
            float g = t.gmaps[i];
            if (A.clear_maps) t.gmaps[i] = 0.f;
            if (t.gsig) g += t.gsig[i];
            const float gt = g * s * oms;
            const long long o = t.off + i;
            A.g[o] = gt;
            if (!skip) adam_update(A.p[o], gt, A.m[o], A.v[o], group_step_size(A.G, o), A.beta1, A.beta2, A.eps, A.bc2_sqrt);
        }
        return;
    }
    // decimated: one wave per cell -- every lane reads the cell's three gradients, lanes 0..2 clear the one they read behind their uses of
    // it, so no wave clears a cell another one still reads
    const float inv = 1.f / (float)(t.d * t.d);
    const int ch_ = t.h / t.d, cw_ = t.w / t.d, lane = threadIdx.x & 63;
    const long long cells = (long long)t.n * ch_ * cw_;
    for (long long c = etid >> 6; c < cells; c += neth >> 6) {
        const int m = (int)(c / ((long long)ch_ * cw_));
        const int r = (int)(c % ((long long)ch_ * cw_));
        const int cy = r / cw_, cx = r % cw_;
        const float gc[3] = {t.gmaps[c * 3], t.gmaps[c * 3 + 1], t.gmaps[c * 3 + 2]};
        for (int q = lane; q < t.d * t.d; q += 64) {
            const long long e = (((long long)m * t.h + cy * t.d + q / t.d) * t.w + cx * t.d + q % t.d) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const long long i = e + ch;
                float oms;          // 1 - s
                const float s = tex_sigmoid(t.tex[i], oms);
                float g = gc[ch] * inv;
                if (t.gsig) g += t.gsig[i];
                const float gt = g * s * oms;
                const long long o = t.off + i;
                A.g[o] = gt;
                if (!skip) adam_update(A.p[o], gt, A.m[o], A.v[o], group_step_size(A.G, o), A.beta1, A.beta2, A.eps, A.bc2_sqrt);
            }
        }
        if (A.clear_maps && lane < 3) t.gmaps[c * 3 + lane] = 0.f;       // (program order: behind this lane's uses of gc)
    }
}

__global__ __launch_bounds__(NT) void adam_groups_tex_kernel(const AdamTailK A) {
    const bool skip = *A.void_raised != 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0 && A.void_flag) *A.void_flag = *A.void_raised;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
    const long long neth = (long long)A.nenv * blockDim.x;
    if (tid < neth) {
        for (int k = 0; k < A.ntex; ++k) adam_tex_set(A, A.t[k], skip, tid, neth);
    } else if (!skip) {
        const long long rest = A.n - A.skip_len[0] - A.skip_len[1];
        for (long long j = tid - neth; j < rest; j += nth - neth) {
            long long i = j;
            if (i >= A.skip_lo[0]) i += A.skip_len[0];
            if (i >= A.skip_lo[1]) i += A.skip_len[1];
            adam_update(A.p[i], A.g[i], A.m[i], A.v[i], group_step_size(A.G, i), A.beta1, A.beta2, A.eps, A.bc2_sqrt);
        }
    }
    for (long long i = tid; i < A.zero_vec; i += nth)
        if (i < A.hole_lo || i >= A.hole_hi) A.zero_buf[i] = make_uint4(0u, 0u, 0u, 0u);
}

inline unsigned grid_for(long long work) {
    long long b = (work + NT - 1) / NT;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;   // 256 CUs x 8 resident blocks, grid-stride beyond that
    return (unsigned)b;
}

}  // namespace

extern "C" int dbw_texture_prep_fwd(const float *texture, int n, int h, int w, int decim, float *maps_out,
                                    float *sig_out, dbw_stream_t stream) {
    DBW_REQUIRE(texture && maps_out, "null pointer");
    DBW_REQUIRE(n > 0 && h > 0 && w > 0 && decim >= 1, "bad size");
    DBW_REQUIRE(decim == 1 || sig_out, "sig_out is required when decimating");
    DBW_REQUIRE(decim == 1 || (h % decim == 0 && w % decim == 0), "map size must be a multiple of the decimation factor");
    const long long work = decim > 1 ? (long long)n * (h / decim) * (w / decim) * 64 : (long long)n * h * w * 3;
    hipLaunchKernelGGL(texture_prep_fwd_kernel, dim3(grid_for(work)), dim3(NT), 0, (hipStream_t)stream, texture, n, h,
                       w, decim, maps_out, sig_out);
    return dbw_check_launch("texture_prep_fwd_kernel");
}

extern "C" int dbw_texture_prep_bwd(const float *texture, int n, int h, int w, int decim, const float *grad_maps,
                                    const float *grad_sig, float *grad_texture, dbw_stream_t stream) {
    DBW_REQUIRE(texture && grad_maps && grad_texture, "null pointer");
    DBW_REQUIRE(n > 0 && h > 0 && w > 0 && decim >= 1, "bad size");
    DBW_REQUIRE(decim == 1 || (h % decim == 0 && w % decim == 0), "map size must be a multiple of the decimation factor");
    const long long work = (long long)n * h * w * 3;
    hipLaunchKernelGGL(texture_prep_bwd_kernel, dim3(grid_for(work)), dim3(NT), 0, (hipStream_t)stream, texture, n, h,
                       w, decim, grad_maps, grad_sig, grad_texture);
    return dbw_check_launch("texture_prep_bwd_kernel");
}

extern "C" int dbw_tv_l2sq(const float *maps, int n, int h, int w, int wrap_x, float scale, float *loss,
                           float *grad_maps, dbw_stream_t stream) {
    DBW_REQUIRE(maps && loss, "null pointer");
    DBW_REQUIRE(n > 0 && h > 1 && w > 1, "bad size");
    const long long rows = (long long)n * h;
    hipLaunchKernelGGL(tv_l2sq_kernel, dim3((unsigned)((w + NT - 1) / NT), (unsigned)(rows < 512 ? rows : 512)), dim3(NT), 0,
                       (hipStream_t)stream, maps, n, h, w, wrap_x, scale, loss, grad_maps);
    return dbw_check_launch("tv_l2sq_kernel");
}

namespace {
int check_sets(const dbw_texture_set *sets, int nsets) {
    DBW_REQUIRE(sets && nsets >= 1 && nsets <= MAX_SETS, "1..4 texture sets");
    for (int i = 0; i < nsets; ++i) {
        const dbw_texture_set &t = sets[i];
        DBW_REQUIRE(t.n > 0 && t.h > 1 && t.w > 1 && t.decim >= 1, "bad size");
        DBW_REQUIRE(t.decim == 1 || (t.h % t.decim == 0 && t.w % t.decim == 0), "map size must be a multiple of the decimation factor");
    }
    return DBW_OK;
}
TextureSets pack_sets(const dbw_texture_set *sets, int nsets) {
    TextureSets S;
    for (int i = 0; i < MAX_SETS; ++i) S.s[i] = sets[i < nsets ? i : 0];
    return S;
}
AdamGroups adam_groups(const int64_t *group_end, const float *lr, int ngroups, float beta1, float beta2, int step, float &bc2_sqrt) {
    const long long n = group_end[ngroups - 1];
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    AdamGroups G;
    for (int k = 0; k < MAX_SETS; ++k) {
        G.end[k] = k < ngroups ? group_end[k] : n;
        G.step_size[k] = (float)(lr[k < ngroups ? k : ngroups - 1] / bc1);
    }
    bc2_sqrt = (float)sqrt(bc2);
    return G;
}
}  // namespace

extern "C" int dbw_texture_prep_fwd_sets(const dbw_texture_set *sets, int nsets, dbw_stream_t stream) {
    if (int rc = check_sets(sets, nsets)) return rc;
    long long work = 0;
    for (int i = 0; i < nsets; ++i) {
        const dbw_texture_set &t = sets[i];
        DBW_REQUIRE(t.texture && t.maps, "null pointer");
        DBW_REQUIRE(t.decim == 1 || t.sig, "sig is required when decimating");
        const long long wk = t.decim > 1 ? (long long)t.n * (t.h / t.decim) * (t.w / t.decim) * 64 : (long long)t.n * t.h * t.w * 3;
        work = wk > work ? wk : work;
    }
    hipLaunchKernelGGL(texture_prep_fwd_sets_kernel, dim3(grid_for(work), (unsigned)nsets), dim3(NT), 0, (hipStream_t)stream,
                       pack_sets(sets, nsets));
    return dbw_check_launch("texture_prep_fwd_sets_kernel");
}

extern "C" int dbw_texture_prep_bwd_sets(const dbw_texture_set *sets, int nsets, dbw_stream_t stream) {
    if (int rc = check_sets(sets, nsets)) return rc;
    long long work = 0;
    for (int i = 0; i < nsets; ++i) {
        const dbw_texture_set &t = sets[i];
        DBW_REQUIRE(t.texture && t.grad_maps && t.grad_texture, "null pointer");
        const long long wk = (long long)t.n * t.h * t.w * 3;
        work = wk > work ? wk : work;
    }
    hipLaunchKernelGGL(texture_prep_bwd_sets_kernel, dim3(grid_for(work), (unsigned)nsets), dim3(NT), 0, (hipStream_t)stream,
                       pack_sets(sets, nsets));
    return dbw_check_launch("texture_prep_bwd_sets_kernel");
}

extern "C" int dbw_tv_l2sq_sets(const dbw_texture_set *sets, int nsets, float *loss, dbw_stream_t stream) {
    if (int rc = check_sets(sets, nsets)) return rc;
    DBW_REQUIRE(loss, "null pointer");
    long long rows = 0;
    int w = 0;
    for (int i = 0; i < nsets; ++i) {
        DBW_REQUIRE(sets[i].sig, "null pointer");
        const long long r = (long long)sets[i].n * sets[i].h;
        rows = r > rows ? r : rows;
        w = sets[i].w > w ? sets[i].w : w;
    }
    hipLaunchKernelGGL(tv_l2sq_sets_kernel, dim3((unsigned)((w + NT - 1) / NT), (unsigned)(rows < 512 ? rows : 512), (unsigned)nsets),
                       dim3(NT), 0, (hipStream_t)stream, pack_sets(sets, nsets), loss);
    return dbw_check_launch("tv_l2sq_sets_kernel");
}

extern "C" int dbw_adam_step_groups(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, const int64_t *group_end,
                                    const float *lr, int ngroups, float beta1, float beta2, float eps, int step, void *zero_buf,
                                    int64_t zero_bytes, const float *skip_flag, dbw_stream_t stream) {
    DBW_REQUIRE(param && grad && exp_avg && exp_avg_sq && group_end && lr, "null pointer");
    DBW_REQUIRE(zero_bytes >= 0 && (zero_bytes == 0 || (zero_buf && zero_bytes % 16 == 0 && ((uintptr_t)zero_buf & 15) == 0)),
                "zero_buf: 16-byte aligned, a multiple of 16 bytes");
    DBW_REQUIRE(ngroups >= 1 && ngroups <= MAX_SETS && step >= 1, "1..4 groups, step >= 1");
    for (int k = 0; k < ngroups; ++k) DBW_REQUIRE(group_end[k] >= (k ? group_end[k - 1] : 0), "group ends must not decrease");
    const long long n = group_end[ngroups - 1];
    if (n == 0) return DBW_OK;
    float bc2_sqrt;
    const AdamGroups G = adam_groups(group_end, lr, ngroups, beta1, beta2, step, bc2_sqrt);
    hipLaunchKernelGGL(adam_groups_kernel, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, G,
                       beta1, beta2, eps, bc2_sqrt, (uint4 *)zero_buf, (long long)(zero_bytes / 16), skip_flag);
    return dbw_check_launch("adam_groups_kernel");
}

bool dbw::adam_tail_fits(const AdamTailArgs &A) {
    if (!A.param || !A.grad || !A.exp_avg || !A.exp_avg_sq || !A.group_end || !A.lr || !A.void_raised || A.ngroups < 1 || A.ngroups > MAX_SETS) return false;
    if (A.ntex < 0 || A.ntex > 2 || A.zero_bytes < 0 || A.zero_bytes % 16 || ((uintptr_t)A.zero_buf & 15)) return false;
    if (A.hole_begin < 0 || A.hole_begin > A.hole_end || A.hole_end > A.zero_bytes || A.hole_begin % 16 || A.hole_end % 16) return false;
    const long long n = A.group_end[A.ngroups - 1];
    const char *hb = (const char *)A.zero_buf + A.hole_begin, *he = (const char *)A.zero_buf + A.hole_end;
    long long lo[2] = {0, 0}, hi[2] = {0, 0};
    for (int k = 0; k < A.ntex; ++k) {
        const dbw_texture_set &t = A.tex[k];
        if (!t.texture || !t.grad_maps || !t.grad_texture || t.n < 1 || t.h < 1 || t.w < 1 || t.decim < 1 || t.h % t.decim || t.w % t.decim) return false;
        lo[k] = (long long)(t.grad_texture - A.grad);
        hi[k] = lo[k] + (long long)t.n * t.h * t.w * 3;
        if (t.grad_texture < A.grad || hi[k] > n || t.texture != A.param + lo[k]) return false;
        const char *mb = (const char *)t.grad_maps, *me = mb + (size_t)t.n * (t.h / t.decim) * (t.w / t.decim) * 3 * sizeof(float);
        const char *zb = (const char *)A.zero_buf, *ze = zb + A.zero_bytes;
        if (A.hole_end > A.hole_begin ? (mb < hb || me > he) : (mb < ze && me > zb)) return false;     // (read while the arena loop clears)
    }
    return A.ntex < 2 || hi[0] <= lo[1] || hi[1] <= lo[0];
}

int dbw::launch_adam_tail(const AdamTailArgs &A, hipStream_t s) {
    DBW_REQUIRE(adam_tail_fits(A), "the texture sets must lie in the flat buffers, their maps' gradients in the hole of the arena");
    DBW_REQUIRE(A.step >= 1, "step >= 1");
    for (int k = 0; k < A.ngroups; ++k) DBW_REQUIRE(A.group_end[k] >= (k ? A.group_end[k - 1] : 0), "group ends must not decrease");
    AdamTailK K;
    memset(&K, 0, sizeof(K));
    K.p = A.param; K.g = A.grad; K.m = A.exp_avg; K.v = A.exp_avg_sq; K.n = A.group_end[A.ngroups - 1];
    K.G = adam_groups(A.group_end, A.lr, A.ngroups, A.beta1, A.beta2, A.step, K.bc2_sqrt);
    K.beta1 = A.beta1; K.beta2 = A.beta2; K.eps = A.eps;
    K.zero_buf = (uint4 *)A.zero_buf; K.zero_vec = A.zero_bytes / 16; K.hole_lo = A.hole_begin / 16; K.hole_hi = A.hole_end / 16;
    K.ntex = A.ntex; K.clear_maps = A.hole_end > A.hole_begin ? 1 : 0;
    for (int k = 0; k < A.ntex; ++k) {
        const dbw_texture_set &t = A.tex[k];
        K.t[k].tex = t.texture; K.t[k].gsig = t.grad_sig; K.t[k].gmaps = (float *)t.grad_maps;
        K.t[k].n = t.n; K.t[k].h = t.h; K.t[k].w = t.w; K.t[k].d = t.decim; K.t[k].off = (long long)(t.grad_texture - A.grad);
    }
    K.void_raised = A.void_raised; K.void_flag = A.void_flag;
    long long env = 0;
    for (int k = 0; k < 2; ++k) {
        K.skip_lo[k] = K.n; K.skip_len[k] = 0;
        if (k < A.ntex) { K.skip_lo[k] = K.t[k].off; K.skip_len[k] = (long long)K.t[k].n * K.t[k].h * K.t[k].w * 3; env += K.skip_len[k]; }
    }
    if (K.skip_lo[1] < K.skip_lo[0]) {
        std::swap(K.skip_lo[0], K.skip_lo[1]);
        std::swap(K.skip_len[0], K.skip_len[1]);
    }
    unsigned grid = grid_for(K.n);
    K.nenv = 0;
    if (A.ntex) {
        // the sets' share of the grid in proportion to their memory operations -- about 10 per element (texture, maps' and TV gradients in;
        // the map cleared, the gradient out; then Adam's 3 + 3) against Adam's 7 -- at least one workgroup for each half
        if (grid < 2) grid = 2;
        const double we = 10.0 / 7.0 * (double)env;
        const long long share = (long long)((double)grid * we / ((double)(K.n - env) + we) + 0.5);
        K.nenv = (int)std::min<long long>(grid - 1, std::max<long long>(1, share));
    }
    hipLaunchKernelGGL(adam_groups_tex_kernel, dim3(grid), dim3(NT), 0, s, K);
    return dbw_check_launch("adam_groups_tex_kernel");
}

// (tests: the step's last launch on the caller's buffers -- held against dbw_texture_prep_bwd_sets + dbw_adam_step_groups; not in the header)
extern "C" int dbw_debug_adam_tail(float *param, float *grad, float *exp_avg, float *exp_avg_sq, const int64_t *group_end, const float *lr,
                                   int ngroups, float beta1, float beta2, float eps, int step, void *zero_buf, int64_t zero_bytes,
                                   int64_t hole_begin, int64_t hole_end, const dbw_texture_set *sets, int nsets, const float *void_raised,
                                   float *void_flag, dbw_stream_t stream) {
    DBW_REQUIRE(nsets >= 0 && nsets <= 2 && (sets || nsets == 0), "0..2 texture sets");
    AdamTailArgs A;
    memset(&A, 0, sizeof(A));
    A.param = param; A.grad = grad; A.exp_avg = exp_avg; A.exp_avg_sq = exp_avg_sq; A.group_end = group_end; A.lr = lr; A.ngroups = ngroups;
    A.beta1 = beta1; A.beta2 = beta2; A.eps = eps; A.step = step;
    A.zero_buf = zero_buf; A.zero_bytes = zero_bytes; A.hole_begin = hole_begin; A.hole_end = hole_end;
    for (int k = 0; k < nsets; ++k) A.tex[k] = sets[k];
    A.ntex = nsets; A.void_raised = void_raised; A.void_flag = void_flag;
    return launch_adam_tail(A, (hipStream_t)stream);
}

extern "C" int dbw_composite_mse(const float *fg, const float *env, const float *imgs, int N, int H, int W,
                                 float scale, const float *scale_dev, float *rec, float *loss_sum, float *grad_fg,
                                 float *grad_env, dbw_stream_t stream) {
    DBW_REQUIRE(fg && env, "null pointer");
    DBW_REQUIRE(imgs || (!loss_sum && !grad_fg && rec), "imgs may only be NULL when just `rec` is wanted");
    DBW_REQUIRE((grad_fg && grad_env) || (!grad_fg && !grad_env), "grad_fg/grad_env: both or none");
    DBW_REQUIRE(N >= 0 && H > 0 && W > 0, "bad size");
    if (N == 0) return DBW_OK;
    const long long plane = (long long)H * W;
    long long gb = ((long long)N * plane + CNT - 1) / CNT;
    if (gb > 512) gb = 512;                 // 256 CUs x 2 resident 1024-thread blocks, grid-stride beyond that
    hipLaunchKernelGGL(composite_mse_kernel, dim3((unsigned)(gb < 1 ? 1 : gb)), dim3(CNT), 0, (hipStream_t)stream, fg,
                       env, imgs, N, plane, scale, scale_dev, rec, loss_sum, grad_fg, grad_env);
    return dbw_check_launch("composite_mse_kernel");
}

extern "C" int dbw_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                             float beta1, float beta2, float eps, int step, dbw_stream_t stream) {
    DBW_REQUIRE(param && grad && exp_avg && exp_avg_sq, "null pointer");
    DBW_REQUIRE(n >= 0 && step >= 1, "bad size/step");
    if (n == 0) return DBW_OK;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(NT), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, (long long)n, (float)(lr / bc1), beta1, beta2, eps, (float)sqrt(bc2));
    return dbw_check_launch("adam_kernel");
}
