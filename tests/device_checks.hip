// Checker-side DEVICE build of the product's shared arithmetic (test infrastructure, not product: built into
// tests/_build/libdbw_device_checks.so by differentiable-blocksworld_amd/build.py: build_device_checks, loaded by tests/device_checks.py).
// The kernels of libdbw_hip.so take their per-pair / per-vertex / per-lane arithmetic from host+device headers (csrc/raster_math.h,
// csrc/model_math.h, csrc/dbw_common.h); the host tests hold the HOST build of those headers to the oracle and to the reference's golden
// vectors -- these entry points evaluate the SAME inline functions on the GPU (its v_rcp_f32, its powf / logf / expf, its DPP
// lanes) on caller-supplied operands, compiled with the product's flags.  They used to be exported by the product library itself.
#include "../differentiable-blocksworld_amd/csrc/dbw_common.h"
#include "../differentiable-blocksworld_amd/csrc/model_math.h"

using namespace dbw;

namespace {

// div_fast (shared-reciprocal division of the rasteriser, raster_math.h) against the IEEE quotient on the real v_rcp_f32
__global__ void divcheck_kernel(const float *__restrict__ n, const float *__restrict__ d, long long count, unsigned long long *__restrict__ bad) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float q = div_fast(n[i], d[i], rcp_refined(d[i])), e = n[i] / d[i];
    if (__float_as_uint(q) != __float_as_uint(e) && !(q != q && e != e)) atomicAdd(bad, 1ull);
}

// lane_merge (dbw_common.h) on caller-supplied keys / values
template <int STEPS>
__global__ __launch_bounds__(64) void lane_merge_kernel(const int *__restrict__ keys, const int *__restrict__ active, const float *__restrict__ values,
                                                        int *__restrict__ active_out, float *__restrict__ values_out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    bool on = active[i] != 0;
    float v[3] = {values[i * 3], values[i * 3 + 1], values[i * 3 + 2]};
    lane_merge<3, STEPS>(keys[i], on, v);
    active_out[i] = on ? 1 : 0;
    values_out[i * 3] = v[0]; values_out[i * 3 + 1] = v[1]; values_out[i * 3 + 2] = v[2];
}

// the model-side arithmetic (model_math.h) with the device's powf / logf / expf
__global__ void model_math_kernel(int what, const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ c, int n,
                                  float ratio, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (what == 0) {
        // parametric_sq_point: a = (cos eta, sin eta, cos omega, sin omega) x n, b = (e1, e2) -> out (n, 9) = loc, d loc / d e1, d loc / d e2
        float loc[3], d1[3], d2[3];
        parametric_sq_point(a[i * 4], a[i * 4 + 1], a[i * 4 + 2], a[i * 4 + 3], b[0], b[1], ratio, loc, d1, d2);
        for (int k = 0; k < 3; ++k) { out[i * 9 + k] = loc[k]; out[i * 9 + 3 + k] = d1[k]; out[i * 9 + 6 + k] = d2[k]; }
    } else if (what == 1) {
        // implicit superquadric distance as the overlap term applies it: a = points (n, 3) in the block frame, b = (e1, e2) x n,
        // c = d loss / d sdf (n) -> out (n, 6) = sdf, d / d e1, d / d e2, d / d point (clamped coordinates carry no gradient)
        float pc[3];
        bool inr[3];
        for (int k = 0; k < 3; ++k) { const float v = a[i * 3 + k]; inr[k] = v >= -5.f && v <= 5.f; pc[k] = v < -5.f ? -5.f : (v > 5.f ? 5.f : v); }
        ImplicitSq im;
        const float sdf = implicit_sq_sdf2(pc, b[i * 2], b[i * 2 + 1], im);
        float ge1, ge2, gpc[3];
        implicit_sq_sdf2_bwd(pc, b[i * 2], b[i * 2 + 1], im, c[i], ge1, ge2, gpc);
        out[i * 6] = sdf; out[i * 6 + 1] = ge1; out[i * 6 + 2] = ge2;
        for (int k = 0; k < 3; ++k) out[i * 6 + 3 + k] = inr[k] ? gpc[k] : 0.f;
    } else if (what == 2) {
        // safe_pow: a = t (n), b[0] = exponent -> out (n, 2) = value, d / d t
        float dt, de;
        out[i * 2] = safe_pow_f(a[i], b[0], dt, de);
        out[i * 2 + 1] = dt;
    } else {
        // signed_pow: a = t (n), b[0] = exponent -> out (n)
        float dde;
        out[i] = spow(a[i], b[0], dde);
    }
}

// LdsAgg<3, LOG2> (dbw_common.h: the LDS hash table in front of the texel-gradient atomics; TexAgg = 256 slots, HardTexAgg = 64) on
// caller-supplied (key, active, value[3]) triples: every workgroup of 256 threads clears a table, runs `rounds` rounds of one of the
// three adds -- thread t of workgroup b takes triple (b * rounds + r) * 256 + t in round r -- and flushes into out (n_keys, 3).
// OP 0: add (active lanes only), 1: add_wave, 2: add_wave_merged<2>.  Active keys must lie in [0, n_keys): the caller checks.
template <int LOG2, int OP>
__global__ __launch_bounds__(256) void lds_agg_kernel(const int *__restrict__ keys, const int *__restrict__ active, const float *__restrict__ values,
                                                      int rounds, float *__restrict__ out) {
    typedef LdsAgg<3, LOG2> Agg;
    __shared__ double mem[(Agg::BYTES + 7) / 8];
    Agg agg;
    agg.bind(mem);
    agg.clear(threadIdx.x, 256);
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
        const long long i = ((long long)blockIdx.x * rounds + r) * 256 + threadIdx.x;
        const int key = keys[i];
        const bool on = active[i] != 0;
        float v[3] = {values[i * 3], values[i * 3 + 1], values[i * 3 + 2]};
        if (OP == 0) { if (on) agg.add(out, key, v); }
        else if (OP == 1) agg.add_wave(out, key, v, on);
        else agg.template add_wave_merged<2>(out, key, v, on);
    }
    __syncthreads();
    agg.flush(out, threadIdx.x, 256);
}

int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e)); return -3; }
    return 0;
}

}  // namespace

// counts in *mismatches (device, zeroed by the caller) the operand pairs whose shared-reciprocal quotient differs from n / d
extern "C" int dbwt_divcheck(const float *n, const float *d, long long count, unsigned long long *mismatches, void *stream) {
    if (!n || !d || !mismatches || count < 0) return -1;
    if (count == 0) return 0;
    hipLaunchKernelGGL(divcheck_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, d, count, mismatches);
    return launched("divcheck_kernel");
}

// waves * 64 lanes, `steps` (1..4) merging steps: keys (>= 0), active (0 / 1), values (lane, 3) in; active and values out
extern "C" int dbwt_lane_merge(const int *keys, const int *active, const float *values, int waves, int steps, int *active_out, float *values_out, void *stream) {
    if (!keys || !active || !values || !active_out || !values_out || waves < 0 || steps < 1 || steps > 4) return -1;
    if (waves == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
#define LM(S) hipLaunchKernelGGL(lane_merge_kernel<S>, dim3(waves), dim3(64), 0, s, keys, active, values, active_out, values_out)
    if (steps == 1) LM(1); else if (steps == 2) LM(2); else if (steps == 3) LM(3); else LM(4);
#undef LM
    return launched("lane_merge_kernel");
}

// workgroups * rounds * 256 triples (keys, active 0 / 1, values (., 3)); log2_slots 6 | 8; op 0 add, 1 add_wave, 2 add_wave_merged<2>;
// out (n_keys, 3) zeroed by the caller, every ACTIVE key in [0, n_keys) (inactive lanes may carry anything)
extern "C" int dbwt_lds_agg(const int *keys, const int *active, const float *values, int workgroups, int rounds, int log2_slots, int op,
                            float *out, void *stream) {
    if (!keys || !active || !values || !out || workgroups < 0 || rounds < 1 || (log2_slots != 6 && log2_slots != 8) || op < 0 || op > 2) return -1;
    if (workgroups == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
#define LA(L, O) hipLaunchKernelGGL((lds_agg_kernel<L, O>), dim3(workgroups), dim3(256), 0, s, keys, active, values, rounds, out)
    if (log2_slots == 6) { if (op == 0) LA(6, 0); else if (op == 1) LA(6, 1); else LA(6, 2); }
    else { if (op == 0) LA(8, 0); else if (op == 1) LA(8, 1); else LA(8, 2); }
#undef LA
    return launched("lds_agg_kernel");
}

// what = 0: superquadric surface point (superquadric.py:10-14); 1: implicit superquadric distance (superquadric.py:17-38, as_sdf = 2, clamped
// to [-5, 5] as the overlap term applies it); 2: safe_pow (pytorch.py:35-36); 3: signed_pow (pytorch.py:31-32) -- operands as in the kernel above
extern "C" int dbwt_model_math(int what, const float *a, const float *b, const float *c, int n, float ratio, float *out, void *stream) {
    if (what < 0 || what > 3 || !a || !b || !out || n < 0 || (what == 1 && !c)) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(model_math_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, (hipStream_t)stream, what, a, b, c, n, ratio, out);
    return launched("model_math_kernel");
}
