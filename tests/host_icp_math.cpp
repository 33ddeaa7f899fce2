// Host build (g++) of csrc/icp_math.h for tests/test_host_icp_math.py and tests/test_gpu_icp.py: the same inline functions the kernels of
// csrc/icp_align.hip compile.  With -DICP_MATH_MAIN the file is a program of its own, for a run under the sanitizers.
#include <stdio.h>

#include <vector>

#include "../differentiable-blocksworld_amd/csrc/icp_math.h"

using namespace dbw;

extern "C" {

// R6 (6), s (3), dM (9) -> gR6 (6), gs (3)
int host_icp_chain(const float *R6, const float *s, const float *dM, int anisotropic, float *gR6, float *gs) {
    Rot6 rot;
    float R[9];
    icp_rotation(R6, rot, R);
    icp_chain(rot, R, s, dM, anisotropic, gR6, gs);
    return 0;
}

// sums (26) -> dM (9), dT (3), the instance's loss
double host_icp_grad_MT(const double *sums, int N, int P1, int P2, float *dM, float *dT) {
    icp_grad_MT(sums, N, P1, P2, dM, dT);
    return icp_instance_loss(sums, P1, P2);
}

// n parameters through `steps` Adam steps (step numbers first_step, first_step + 1, ...); grads (steps, n)
int host_icp_adam(float *p, float *m, float *v, const float *grads, int n, int steps, int first_step, double lr) {
    for (int t = 0; t < steps; ++t) {
        const IcpAdam a = icp_adam_scalars(lr, first_step + t);
        for (int k = 0; k < n; ++k) icp_adam_update(p[k], m[k], v[k], grads[(size_t)t * n + k], a);
    }
    return 0;
}

// the rule on a loss sequence: kept[it] = 1 where the parameters of iteration it are kept -> the kept iteration (-1: none), *loss_min
int host_icp_keep_best(const double *losses, int n_iter, int N, int *kept, double *loss_min) {
    IcpMeter m;
    icp_meter_init(m);
    for (int it = 0; it < n_iter; ++it) kept[it] = icp_keep_best(m, losses[it], N, it) ? 1 : 0;
    *loss_min = m.loss_min;
    return (int)m.best_iter;
}

// rts (R 9 | T 3 | s 3) and p (n,3) -> q (n,3)
int host_icp_transform(const float *rts, const float *p, long long n, float *q) {
    float blk[12];
    icp_block(rts, rts + 9, rts + 12, blk);
    for (long long i = 0; i < n; ++i) icp_transform(blk, p[i * 3], p[i * 3 + 1], p[i * 3 + 2], q + i * 3);
    return 0;
}

// one instance's step from the identity start or from given state; param / m / v (12) are updated, rts (15) and blk (12) written
int host_icp_step(float *param, float *m, float *v, const double *sums, int N, int P1, int P2, int estimate_scale, int anisotropic, double lr,
                  int step, float *blk, float *rts) {
    icp_step(param, m, v, sums, N, P1, P2, estimate_scale, anisotropic, icp_adam_scalars(lr, step), blk, rts);
    return 0;
}

// the 13 sums of n pairs in index order
int host_icp_moments(const float *q, const float *g, const float *p, long long n, double *acc) {
    for (int k = 0; k < ICP_NSUM; ++k) acc[k] = 0.0;
    for (long long i = 0; i < n; ++i) icp_pair_moments(q + i * 3, g + i * 3, p + i * 3, acc);
    return 0;
}

}

#ifdef ICP_MATH_MAIN
// A few iterations on a small synthetic pairing, exactly sized heap buffers: a read or write outside them is the sanitizer's to report.
int main() {
    const int N = 1, P = 37;
    std::vector<float> p((size_t)P * 3), g((size_t)P * 3), q((size_t)P * 3);
    uint32_t seed = 12345u;
    for (size_t i = 0; i < p.size(); ++i) {
        seed = seed * 1664525u + 1013904223u; p[i] = (float)(seed >> 8) / 16777216.f - 0.5f;
        g[i] = 1.1f * p[i] + 0.03f;
    }
    std::vector<float> param(12), m(12, 0.f), v(12, 0.f), blk(12), rts(15);
    icp_identity(param.data(), rts.data(), blk.data());
    IcpMeter meter;
    icp_meter_init(meter);
    double first = 0.0, last = 0.0;
    for (int it = 0; it < 41; ++it) {
        for (int i = 0; i < P; ++i) icp_transform(blk.data(), p[i * 3], p[i * 3 + 1], p[i * 3 + 2], &q[i * 3]);
        std::vector<double> sums(26);
        host_icp_moments(q.data(), g.data(), p.data(), P, sums.data());
        host_icp_moments(q.data(), g.data(), p.data(), P, sums.data() + 13);
        last = icp_instance_loss(sums.data(), P, P);
        if (it == 0) first = last;
        icp_step(param.data(), m.data(), v.data(), sums.data(), N, P, P, 1, 1, icp_adam_scalars(0.01, it + 1), blk.data(), rts.data());
        icp_keep_best(meter, last, N, it);
    }
    printf("loss %g -> %g, kept iteration %d\n", first, last, (int)meter.best_iter);
    return last < first && meter.best_iter == 40.0 ? 0 : 1;
}
#endif
