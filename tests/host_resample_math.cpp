// Host build (g++) of csrc/resample_math.h for tests/test_host_resample_math.py, tests/test_dataset_host.py and tests/test_gpu_ingest.py:
// the same inline functions the ingest kernels compile, driven by the plain two-pass loop (horizontal into an 8-bit intermediate, then
// vertical) that the kernels tile.
#include <vector>

#include "../differentiable-blocksworld_amd/csrc/resample_math.h"

using namespace dbw;

extern "C" {

// dbw_resample_table on the host: returns ksize, fills out_size rows of [xmin, n, k_0 .. k_{ksize-1}] when table is given
int host_resample_table(int in_size, int out_size, int32_t *table, long long capacity_ints) {
    if (in_size <= 0 || out_size <= 0) return -1;
    const int ksize = resample_ksize(in_size, out_size);
    if (!table) return ksize;
    if (capacity_ints < (long long)out_size * (ksize + 2)) return -1;
    for (int xx = 0; xx < out_size; ++xx) resample_table_row(in_size, out_size, xx, ksize, table + (long long)xx * (ksize + 2));
    return ksize;
}

// dbw_images_resample_u8 on the host: src (N,Hin,Win,3) uint8 -> out_f32 (N,3,Hout,Wout) and / or out_u8 (N,Hout,Wout,3)
int host_images_resample_u8(const uint8_t *src, int N, int Hin, int Win, int Hout, int Wout, float *out_f32, uint8_t *out_u8) {
    const int kh = resample_ksize(Win, Wout), kv = resample_ksize(Hin, Hout);
    std::vector<int32_t> th((size_t)Wout * (kh + 2)), tv((size_t)Hout * (kv + 2));
    host_resample_table(Win, Wout, th.data(), (long long)th.size());
    host_resample_table(Hin, Hout, tv.data(), (long long)tv.size());
    std::vector<uint8_t> mid((size_t)Hin * Wout * 3);
    for (long long n = 0; n < N; ++n) {
        const uint8_t *s = src + n * Hin * Win * 3;
        const uint8_t *m = s;
        if (Win != Wout) {                  // an axis that keeps its size is skipped
            for (int y = 0; y < Hin; ++y)
                for (int x = 0; x < Wout; ++x) {
                    const int32_t *row = th.data() + (size_t)x * (kh + 2);
                    for (int c = 0; c < 3; ++c) mid[((size_t)y * Wout + x) * 3 + c] = resample_dot(s + ((long long)y * Win + row[0]) * 3 + c, 3, row + 2, row[1]);
                }
            m = mid.data();
        }
        for (int y = 0; y < Hout; ++y) {
            const int32_t *row = tv.data() + (size_t)y * (kv + 2);
            for (int x = 0; x < Wout; ++x)
                for (int c = 0; c < 3; ++c) {
                    const uint8_t v = Hin != Hout ? resample_dot(m + ((long long)row[0] * Wout + x) * 3 + c, (long long)Wout * 3, row + 2, row[1])
                                                  : m[((long long)y * Wout + x) * 3 + c];
                    if (out_u8) out_u8[((n * Hout + y) * Wout + x) * 3 + c] = v;
                    if (out_f32) out_f32[((n * 3 + c) * Hout + y) * Wout + x] = resample_to_float(v);
                }
        }
    }
    return 0;
}

int host_resample_to_float(const uint8_t *v, long long n, float *out) {
    for (long long i = 0; i < n; ++i) out[i] = resample_to_float(v[i]);
    return 0;
}

int host_resample_clip8(const int32_t *acc, long long n, uint8_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = resample_clip8(acc[i]);
    return 0;
}

}
