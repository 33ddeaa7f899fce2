"""CPU: the g++ build of csrc/cluster_math.h (tests/host_cluster_math.cpp) against the numpy restatement of tests/cluster_ref.py.

Bounds.  Labels, counts, seeding order and keys are integer results of fp32 arithmetic with one rounding per operation: equality.  The ten
sums add the same exact terms (products of fp32-derived doubles) in another order than numpy's pairwise sum does: 8 eps64 sum|term| per sum,
the bound of a reordered fp64 sum.  (Reordered, not running: cluster_ref.np_moments and host_cluster_moments say what a single running sum
over such terms does.)  The eigen-decomposition is judged by what it
must satisfy (cluster_ref.check_eigen), not against eigh: with repeated eigenvalues the vectors are not unique."""
import numpy as np
import pytest

import cluster_ref as CR


def test_labels_and_ties_are_exact_on_the_lattice():
    p, c = CR.lattice_cloud()
    p = p.copy()
    p[7, 1], p[11, 0], p[13, 2] = np.nan, np.inf, -np.inf
    labels, d2 = CR.host_assign(p, c)
    ref = CR.np_assign(p, c)
    assert np.array_equal(labels, ref) and (labels[[7, 11, 13]] == -1).all() and (labels >= -1).all()
    D = CR.np_dist2(p, c)
    fin = CR.np_finite(p)
    ties = int(((D[fin] == D[fin].min(1, keepdims=True)).sum(1) > 1).sum())
    assert ties > 20                                               # ties really occur: the duplicated centre alone makes some
    assert not (labels == len(c) - 1).any()                        # the duplicate of centre 1 loses every tie
    assert np.array_equal(d2[fin], D[fin].min(1)) and np.all(D[fin] == np.round(D[fin]))     # exact integer distances
    # a NaN centre is never the nearest; with nothing but NaN centres the label is 0
    c2 = c.copy()
    c2[0] = np.nan
    assert np.array_equal(CR.host_assign(p, c2)[0], CR.np_assign(p, c2)) and not (CR.host_assign(p, c2)[0] == 0).any()
    assert (CR.host_assign(p[fin], np.full((3, 3), np.nan, np.float32))[0] == 0).all()


@pytest.mark.parametrize('cloud', ['lattice', 'random'])
def test_moments_finish_and_rounds(cloud):
    if cloud == 'lattice':
        p, init = CR.lattice_cloud(1)
    else:
        p = CR.random_cloud(3000, 5)
        init = p[::500][:6].copy()
    K = len(init)
    ref = CR.np_fit(p, K, n_iter=3, init=init)
    for r, want in enumerate(ref):
        got = CR.host_fit(p, K, n_iter=r, init=init)
        assert got['rc'] == 0 and got['info'][0] == r and got['info'][3] == 0
        assert np.array_equal(got['labels'], want['labels']) and np.array_equal(got['counts'], want['counts']), r
        assert got['info'][2] == int((want['counts'] > 0).sum())
        err = np.abs(got['sums'] - want['sums'])
        print(f'{cloud} round {r}: worst sum error / bound {np.max(err / np.maximum(want["bound"], 1e-300)):.3f}')
        assert (err <= want['bound']).all(), r
        if cloud == 'lattice' and r == 0:                          # integer terms about integer centres: the sums are exact, and so is all that follows
            assert np.array_equal(got['sums'], want['sums']) and np.array_equal(got['mean'], want['mean'])
        assert CR.ulp_diff(got['centres'], want['centres']).max() <= (0 if r <= 1 and cloud == 'lattice' else 1), r
        assert np.abs(got['mean'] - want['mean']).max() <= 1e-12 and np.abs(got['cov'] - want['cov']).max() <= 1e-12
        changed = len(p) if r == 0 else int((ref[r - 1]['labels'] != want['labels']).sum())
        assert got['info'][1] == changed
    # an empty cluster keeps its centre, has zero covariance and identity axes; so has a cluster of one point
    p1 = np.array([[0, 0, 0], [0, 0, 1], [5, 5, 5]], np.float32)
    init = np.array([[0, 0, 0.4], [5, 5, 6], [100, 100, 100]], np.float32)
    got = CR.host_fit(p1, 3, n_iter=1, init=init)
    assert got['counts'].tolist() == [2, 1, 0] and np.array_equal(got['centres'][2], init[2]) and got['centres'][1].tolist() == [5, 5, 5]
    assert not got['cov'][1:].any() and np.array_equal(got['axes'][1], np.eye(3)) and np.array_equal(got['axes'][2], np.eye(3))
    assert not got['evals'][1:].any() and np.array_equal(got['mean'][2], init[2].astype(np.float64))


def test_refused_sizes():
    p = np.zeros((5, 3), np.float32)
    for K, n_iter in ((0, 1), (257, 1), (6, 1), (2, -1), (2, 65)):
        assert CR.host_fit(np.zeros((300, 3), np.float32) if K == 257 else p, K, n_iter=n_iter)['rc'] == -1


def _rot(rng):
    Q, _ = np.linalg.qr(rng.randn(3, 3))
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    return Q


def _sym6(A):
    return np.array([A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]])


def test_eigen_decomposition():
    rng = np.random.RandomState(3)
    cases = {'isotropic': np.eye(3) * 0.37, 'zero': np.zeros((3, 3)), 'diagonal': np.diag([1.0, 3.0, 2.0]), 'diagonal ties': np.diag([2.0, 2.0, 5.0])}
    for i in range(40):
        Q = _rot(rng)
        lam = np.sort(rng.uniform(0.01, 4, 3))[::-1] * 10.0 ** rng.randint(-6, 7)
        cases[f'full {i}'] = Q.T @ np.diag(lam) @ Q
        cases[f'rank 2 {i}'] = Q.T @ np.diag([lam[0], lam[1], 0.0]) @ Q
        cases[f'rank 1 {i}'] = np.outer(Q[0], Q[0]) * lam[0]
        cases[f'two equal {i}'] = Q.T @ np.diag([lam[0], lam[0], lam[2]]) @ Q
        cases[f'nearly isotropic {i}'] = np.eye(3) * lam[0] + 1e-9 * lam[0] * (Q + Q.T)
    names = list(cases)
    C = np.stack([_sym6((cases[n] + cases[n].T) / 2) for n in names])
    evals, axes = CR.host_eigen(C)
    for n, c, ev, ax in zip(names, C, evals, axes):
        CR.check_eigen(c, ev, ax, n)
    # a covariance through the whole chain: the axes of an elongated cloud
    Q = _rot(rng)
    p = ((rng.uniform(-1, 1, size=(5000, 3)) * [3.0, 1.0, 0.25]) @ Q + [4, -2, 1]).astype(np.float32)
    got = CR.host_fit(p, 1, n_iter=1)
    CR.check_eigen(got['cov'][0], got['evals'][0], got['axes'][0], 'cloud')
    assert np.abs(np.abs(got['axes'][0] @ Q.T) - np.eye(3)).max() < 0.05
    assert np.abs(np.sqrt(3 * got['evals'][0]) - [3.0, 1.0, 0.25]).max() < 0.05
    assert np.abs(got['cov'][0] - _sym6(np.cov(p.astype(np.float64).T, bias=True))).max() <= 1e-12


def test_seeding_order_and_keys():
    # keys: the largest far key is the largest distance, the largest near key the smallest, the lowest index on ties; key 0 is below all
    d = np.array([0.0, 2.5, 7.0, 2.5, 7.0, np.inf, 0.0, 1e-45], np.float32)
    far, near = CR.host_keys(d)
    assert int(far.argmax()) == 5 and int(far[:5].argmax()) == 2 and int(near.argmax()) == 0 and (far > 0).all() and (near > 0).all()
    assert [int(k >> np.uint64(32)) for k in far] == d.view(np.uint32).tolist()
    assert [0xffffffff - int(k & np.uint64(0xffffffff)) for k in far] == list(range(len(d)))
    assert np.array_equal(np.argsort(-far.astype(np.float64), kind='stable')[:2], [5, 2])
    for p, K in ((CR.lattice_cloud(2)[0], 12), (CR.random_cloud(777, 8), 16)):
        p = p.copy()
        p[3] = np.nan
        c, order = CR.host_seed(p, K)
        rc, rorder = CR.np_seed(p, K)
        assert np.array_equal(order, rorder) and np.array_equal(c, rc) and 3 not in order
        assert len(set(order.tolist())) == K
    # fewer distinct points than centres: the later centres repeat an earlier one (the lowest index whose distance is zero) and stay empty
    p = np.repeat(np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], np.float32), 5, axis=0)
    c, order = CR.host_seed(p, 5)
    assert np.array_equal(order, CR.np_seed(p, 5)[1]) and order[:3].tolist() == [0, 5, 10] and order[3:].tolist() == [0, 0]
    got = CR.host_fit(p, 5, n_iter=2)
    assert got['counts'].tolist() == [5, 5, 5, 0, 0] and got['info'][2] == 3
    # no finite point at all: zero centres, every label -1
    got = CR.host_fit(np.full((4, 3), np.nan, np.float32), 2, n_iter=1)
    assert got['rc'] == 0 and not got['centres'].any() and (got['labels'] == -1).all() and not got['counts'].any() and got['info'][2] == 0
