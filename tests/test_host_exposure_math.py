"""CPU tests of the arithmetic of the exposure compensation: csrc/exposure_math.h built for the host by g++
(tests/host_exposure_math.cpp) against the numpy float64 restatement of tests/exposure_ref.py, on the cases of the GPU tests.

Forward: rec within 4 ulp of fp32.  Six fp32 operations lie between the inputs and rec -- exp, the two products and the sum of the
composite (1 - alpha is exact to half an ulp as well), the product with the gain, the sum with the offset -- each within half an ulp (exp:
one) of a result no larger than the largest of |gain * comp|, |b| and |rec|: the ulp is taken at that magnitude, since the last sum may
cancel.  Backward: every output against central differences of the float64 forward (and the analytic float64 gradients of exposure_ref
against the same differences, so that the GPU tests may use them).  theta = 0 gives the composite bit for bit."""
import numpy as np
import pytest
import torch

import exposure_ref as ER

IDS = [ER.case_id(c) for c in ER.CASES]


def _inputs(c, with_extra):
    return ER._np(c['fg']), ER._np(c['env']), ER._np(c['imgs']), ER._np(c['m']), (ER._np(c['x']) if with_extra else None)


@pytest.mark.parametrize('shape,mkind', ER.CASES, ids=IDS)
def test_forward_within_4_ulp(shape, mkind):
    c = ER.case(shape, mkind)
    rec, value, _, _, _ = ER.host(c, False, backward=False)
    ref = ER.reference(c, False)
    t = ER.rows64(ER._np(c['theta']), ER._np(c['ids']))
    fg, env = ER._np(c['fg']), ER._np(c['env'])
    comp = fg[:, :3] * fg[:, 3:4] + (1 - fg[:, 3:4]) * env[:, :3]
    scale_of = np.maximum(np.maximum(np.abs(np.exp(t[:, :3])[:, :, None, None] * comp), np.abs(t[:, 3:, None, None])), np.abs(ref['rec']))
    ulp = np.spacing(scale_of.astype(np.float32)).astype(np.float64)
    err = np.abs(rec.double().numpy() - ref['rec']) / ulp
    print(f'{ER.case_id((shape, mkind))}: rec worst {err.max():.2f} ulp; value {value:.9e} (float64 {ref["value"]:.9e})')
    assert err.max() <= 4.0
    assert abs(value - ref['value']) <= 1e-5 * abs(ref['value'])


@pytest.mark.parametrize('shape,mkind', ER.CASES, ids=IDS)
@pytest.mark.parametrize('with_extra', [False, True], ids=['mse', 'mse+grad_rec'])
def test_backward_against_central_differences(shape, mkind, with_extra):
    c = ER.case(shape, mkind)
    fg, env, imgs, m, x = _inputs(c, with_extra)
    theta, ids = ER._np(c['theta']), ER._np(c['ids'])
    loss = lambda fg_=fg, env_=env, th_=theta: ER.pixel_loss64(fg_, env_, imgs, m, x, th_, ids, c['scale'])
    # fg and env: the pixels are independent, so one pair of evaluations per channel differentiates every pixel at once
    h = 1e-6
    fd_fg, fd_env = np.zeros_like(fg), np.zeros_like(env)
    for ch in range(4):
        for arr, out, name in ((fg, fd_fg, 'fg'), (env, fd_env, 'env')):
            up, dn = arr.copy(), arr.copy()
            up[:, ch] += h
            dn[:, ch] -= h
            kw = 'fg_' if name == 'fg' else 'env_'
            out[:, ch] = (loss(**{kw: up}) - loss(**{kw: dn})) / (2 * h)
    # theta: one pair per entry of the table; rows outside the batch get exactly 0
    h = 1e-5
    fd_th = np.zeros_like(theta)
    for i in range(theta.shape[0]):
        for k in range(6):
            up, dn = theta.copy(), theta.copy()
            up[i, k] += h
            dn[i, k] -= h
            fd_th[i, k] = (loss(th_=up).sum() - loss(th_=dn).sum()) / (2 * h)
    ref = ER.reference(c, with_extra)
    big = lambda a: max(np.abs(a).max(), 1e-300)
    # the analytic float64 gradients are the differences' (truncation h^2, rounding 1e-16 / h)
    assert np.abs(ref['gfg'] - fd_fg).max() <= 1e-8 * big(fd_fg) + 1e-12 and np.abs(ref['genv'] - fd_env).max() <= 1e-8 * big(fd_env) + 1e-12
    assert np.abs(ref['gth'] - fd_th).max() <= 1e-8 * big(ref['ath']) + 1e-12
    # the host build of the header: fp32 per pixel (about eight roundings of 6e-8 on terms no larger than a few times the largest
    # element: 1e-5 of it leaves a margin of 20), the sums in fp64 over fp32 terms: 1e-5 of the sum of the terms' magnitudes
    _, _, gfg, genv, gth = ER.host(c, with_extra)
    e_fg, e_env = np.abs(gfg.double().numpy() - fd_fg).max(), np.abs(genv.double().numpy() - fd_env).max()
    e_th = np.abs(gth.numpy() - fd_th)
    print(f'{ER.case_id((shape, mkind))} extra={with_extra}: grad_fg err {e_fg:.2e} of {big(fd_fg):.2e}, grad_env err {e_env:.2e} of {big(fd_env):.2e}, '
          f'grad_theta err / sum|terms| {np.max(e_th / np.maximum(ref["ath"], 1e-300)):.2e}')
    assert e_fg <= 1e-5 * np.abs(fd_fg).max() + 1e-12 and e_env <= 1e-5 * np.abs(fd_env).max() + 1e-12
    assert (e_th <= 1e-5 * ref['ath'] + 1e-12).all()
    outside = [i for i in range(ER.V) if i not in ids.astype(int).tolist()]
    assert outside and not gth[outside].any() and not fd_th[outside].any()
    assert not genv[:, 3].any()


@pytest.mark.parametrize('shape,mkind', ER.CASES, ids=IDS)
def test_zero_theta_is_the_composite_bit_for_bit(shape, mkind):
    c = ER.case(shape, mkind)
    rec, value, gfg, genv, _ = ER.host(c, True, theta=torch.zeros(ER.V, 6))
    fg, env = c['fg'], c['env']
    comp = fg[:, :3] * fg[:, 3:4] + (1 - fg[:, 3:4]) * env[:, :3]          # torch on the CPU: one rounding per operation, the header's order
    assert torch.equal(rec, comp)
    # ... and so does an id outside the table, whatever theta holds
    for bad in (-1, ER.V):
        ids = torch.full_like(c['ids'], bad)
        rec_b, value_b, gfg_b, genv_b, gth_b = ER.host(c, True, ids=ids)
        assert torch.equal(rec_b, comp) and value_b == value and torch.equal(gfg_b, gfg) and torch.equal(genv_b, genv) and not gth_b.any()


def test_the_gradient_scales_with_the_upstream_scalar():
    c = ER.case((2, 5, 7), 'random')
    _, _, g1, e1, t1 = ER.host(c, False, upstream=1.0)
    _, _, g2, e2, t2 = ER.host(c, False, upstream=2.0)                    # (a power of two: exact)
    assert torch.equal(g2, 2 * g1) and torch.equal(e2, 2 * e1) and torch.equal(t2, 2 * t1)
    _, _, g0, e0, t0 = ER.host(c, True, upstream=0.0)                     # the scalar's gradient 0: what rec receives alone
    gain = torch.exp(c['theta'][c['ids'].long(), :3])[:, :, None, None]
    want = (gain * c['x']) * c['fg'][:, 3:4]                               # (torch's exp and libm's may differ in the last bit)
    assert float((g0[:, :3] - want).abs().max()) <= 1e-6 * float(want.abs().max())
