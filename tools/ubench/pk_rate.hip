// Microbenchmark (profiling aid, not product code): what a packed fp32 VALU instruction costs a SIMD next to a plain one.
// Chains of v_fma_f32, v_pk_fma_f32, v_pk_mul_f32, v_pk_add_f32 and a 1:1 mix of v_fma_f32 / v_pk_fma_f32, independent (eight
// accumulators round-robin) and dependent (one accumulator), at 1, 2, 4 and 5 waves per SIMD on every CU, operands in VGPRs.
// Each wave times its own loop with the shader clock (s_memtime); a SIMD that holds W waves spends (wave cycles) / (W x instructions)
// per wave-instruction.  The wall clock of the launch is printed next to it as a cross-check (at the clock the run reached).
// 256-thread workgroups (one wave per SIMD); dynamic LDS of a little over 160 KiB / (W + 1) per workgroup caps a CU at W of them and the grid is W per CU.
//   hipcc --offload-arch=gfx950 -O3 -o tools/ubench/pk_rate tools/ubench/pk_rate.hip     (tools/ubench/pk_rate.sh builds, runs and files it)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

typedef float f2v __attribute__((ext_vector_type(2)));
enum Op { FMA = 0, PK_FMA, PK_MUL, PK_ADD, MIX, N_OP };
static const char *OP_NAME[N_OP] = {"v_fma_f32", "v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32", "v_fma_f32 + v_pk_fma_f32 1:1"};
constexpr int BODY = 64;                        // wave-instructions per loop trip

// One asm statement per loop trip: between separate asm statements the compiler pads with s_nop, which has an issue cost of its own.
#define R8(x) x x x x x x x x
#define IND8(I) I " %0, %0, %8, %9\n" I " %1, %1, %8, %9\n" I " %2, %2, %8, %9\n" I " %3, %3, %8, %9\n" \
                I " %4, %4, %8, %9\n" I " %5, %5, %8, %9\n" I " %6, %6, %8, %9\n" I " %7, %7, %8, %9\n"
#define IND8_2(I) I " %0, %0, %8\n" I " %1, %1, %8\n" I " %2, %2, %8\n" I " %3, %3, %8\n" I " %4, %4, %8\n" I " %5, %5, %8\n" I " %6, %6, %8\n" I " %7, %7, %8\n"
#define MIX8 "v_fma_f32 %0, %0, %4, %5\n v_pk_fma_f32 %2, %2, %6, %7\n v_fma_f32 %1, %1, %4, %5\n v_pk_fma_f32 %3, %3, %6, %7\n" \
             "v_fma_f32 %0, %0, %4, %5\n v_pk_fma_f32 %2, %2, %6, %7\n v_fma_f32 %1, %1, %4, %5\n v_pk_fma_f32 %3, %3, %6, %7\n"
#define MIX8_DEP "v_fma_f32 %0, %0, %4, %5\n v_pk_fma_f32 %2, %2, %6, %7\n v_fma_f32 %0, %0, %4, %5\n v_pk_fma_f32 %2, %2, %6, %7\n" \
                 "v_fma_f32 %0, %0, %4, %5\n v_pk_fma_f32 %2, %2, %6, %7\n v_fma_f32 %0, %0, %4, %5\n v_pk_fma_f32 %2, %2, %6, %7\n"
#define DEP8(I) R8(I " %0, %0, %1, %2\n")
#define DEP8_2(I) R8(I " %0, %0, %1\n")
#define ACC8(a) "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7])

// BODY wave-instructions.  s / p: the plain and the packed accumulators (8 independent ones, or one: DEP).
template <int OP, bool DEP> __device__ __forceinline__ void body(float *s, f2v *p, float sb, float sc, f2v pb, f2v pc) {
    if (!DEP) {
        if (OP == FMA)    asm volatile(R8(IND8("v_fma_f32")) : ACC8(s) : "v"(sb), "v"(sc));
        if (OP == PK_FMA) asm volatile(R8(IND8("v_pk_fma_f32")) : ACC8(p) : "v"(pb), "v"(pc));
        if (OP == PK_MUL) asm volatile(R8(IND8_2("v_pk_mul_f32")) : ACC8(p) : "v"(pb));
        if (OP == PK_ADD) asm volatile(R8(IND8_2("v_pk_add_f32")) : ACC8(p) : "v"(pc));
        if (OP == MIX)    asm volatile(R8(MIX8) : "+v"(s[0]), "+v"(s[1]), "+v"(p[0]), "+v"(p[1]) : "v"(sb), "v"(sc), "v"(pb), "v"(pc));
    } else {
        if (OP == FMA)    asm volatile(R8(DEP8("v_fma_f32")) : "+v"(s[0]) : "v"(sb), "v"(sc));
        if (OP == PK_FMA) asm volatile(R8(DEP8("v_pk_fma_f32")) : "+v"(p[0]) : "v"(pb), "v"(pc));
        if (OP == PK_MUL) asm volatile(R8(DEP8_2("v_pk_mul_f32")) : "+v"(p[0]) : "v"(pb));
        if (OP == PK_ADD) asm volatile(R8(DEP8_2("v_pk_add_f32")) : "+v"(p[0]) : "v"(pc));
        // (dependent mix: one plain and one packed chain, interleaved)
        if (OP == MIX)    asm volatile(R8(MIX8_DEP) : "+v"(s[0]), "+v"(s[1]), "+v"(p[0]), "+v"(p[1]) : "v"(sb), "v"(sc), "v"(pb), "v"(pc));
    }
}

template <int OP, bool DEP> __global__ __launch_bounds__(256) void chain_kernel(unsigned *cycles, float *sink, int trips, float seed) {
    extern __shared__ float lds_cap[];          // (occupancy cap only)
    constexpr int NA = 8;
    float s[NA]; f2v p[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) { s[a] = seed + (float)(threadIdx.x + a); p[a] = f2v{s[a], s[a] + 1.f}; }
    const float sb = 1.f, sc = seed;            // x * 1 + 0: stays finite, no denormals
    const f2v pb = {1.f, 1.f}, pc = {seed, seed};
    __syncthreads();
    const unsigned long long c0 = __builtin_readcyclecounter();
    for (int t = 0; t < trips; ++t) body<OP, DEP>(s, p, sb, sc, pb, pc);
    const unsigned long long c1 = __builtin_readcyclecounter();
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < NA; ++a) acc += s[a] + p[a].x + p[a].y;
    if (acc == 123.456f) { sink[0] = acc; lds_cap[threadIdx.x] = acc; }      // (never true: keeps the chains alive)
    if ((threadIdx.x & 63) == 0) cycles[blockIdx.x * 4 + (threadIdx.x >> 6)] = (unsigned)(c1 - c0);
}

typedef void (*kern_t)(unsigned *, float *, int, float);
template <int OP> static kern_t pick(bool dep) { return dep ? chain_kernel<OP, true> : chain_kernel<OP, false>; }
static kern_t kernel_of(int op, bool dep) {
    switch (op) { case FMA: return pick<FMA>(dep); case PK_FMA: return pick<PK_FMA>(dep); case PK_MUL: return pick<PK_MUL>(dep);
                  case PK_ADD: return pick<PK_ADD>(dep); default: return pick<MIX>(dep); }
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const int n_cu = prop.multiProcessorCount, trips = 2048;
    const int waves[4] = {1, 2, 4, 5};
    const int max_blocks = n_cu * 5;
    unsigned *d_cyc; float *d_sink;
    CK(hipMalloc(&d_cyc, (size_t)max_blocks * 4 * sizeof(unsigned))); CK(hipMalloc(&d_sink, 256));
    std::vector<unsigned> h((size_t)max_blocks * 4);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    printf("%s, %d CUs; %d wave-instructions per wave and launch; cycles = shader clock (s_memtime), median over the waves of the best of 3 launches\n",
           prop.gcnArchName, n_cu, trips * BODY);
    printf("%-30s %-11s %5s | %14s %14s %12s | %9s %14s\n", "instruction", "chain", "waves", "cyc/inst, wave", "cyc/inst, SIMD", "max/median", "wall us", "wall ns/inst/SIMD");
    double simd_cost[N_OP][2][4];
    for (int op = 0; op < N_OP; ++op) for (int dep = 0; dep < 2; ++dep) for (int wi = 0; wi < 4; ++wi) {
        const int W = waves[wi], blocks = n_cu * W, n_waves = blocks * 4;
        const size_t lds = (size_t)(160 * 1024 / (W + 1) + 1024) & ~(size_t)1023;      // W fit into 160 KiB, W + 1 do not
        kern_t k = kernel_of(op, dep != 0);
        CK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        double best_med = 1e30, best_max = 0, best_ms = 1e30;
        for (int rep = 0; rep < 3; ++rep) {
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(k, dim3(blocks), dim3(256), lds, 0, d_cyc, d_sink, trips, 0.f);
            CK(hipGetLastError());
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            CK(hipMemcpy(h.data(), d_cyc, (size_t)n_waves * sizeof(unsigned), hipMemcpyDeviceToHost));
            std::sort(h.begin(), h.begin() + n_waves);
            const double med = h[n_waves / 2];
            if (med < best_med) { best_med = med; best_max = h[n_waves - 1]; }
            if (ms < best_ms) best_ms = ms;
        }
        const double n_inst = (double)trips * BODY;
        simd_cost[op][dep][wi] = best_med / (n_inst * W);
        printf("%-30s %-11s %5d | %14.2f %14.2f %12.2f | %9.1f %14.3f\n", OP_NAME[op], dep ? "dependent" : "independent", W,
               best_med / n_inst, best_med / (n_inst * W), best_max / best_med, best_ms * 1e3, best_ms * 1e6 / (n_inst * W));
    }
    printf("\nc = SIMD cycles of a packed instruction / SIMD cycles of v_fma_f32, same chain form and wave count\n");
    printf("%-30s %-11s %8s %8s %8s %8s\n", "instruction", "chain", "1 wave", "2 waves", "4 waves", "5 waves");
    for (int op = 1; op < N_OP; ++op) for (int dep = 0; dep < 2; ++dep) {
        printf("%-30s %-11s", OP_NAME[op], dep ? "dependent" : "independent");
        for (int wi = 0; wi < 4; ++wi) printf(" %8.2f", simd_cost[op][dep][wi] / simd_cost[FMA][dep][wi]);
        printf("\n");
    }
    return 0;
}
