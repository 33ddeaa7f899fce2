"""Records tests/golden/ransac_plane.npz: the reference's own Ransac (src/utils/ransac.py, imported through make_golden.import_reference)
on a seeded cloud, for tests/test_host_plane_math.py and tests/test_gpu_worldfit.py.  Run from the repository root:

    python tests/golden/make_golden_plane.py

The cloud: 4096 points, 55 % on a tilted noisy ground z = p0 + p1 x + p2 y, the rest in a blob above it.  Recorded: the 100 triples
Ransac.fit itself draws (torch.randint under its use_seed, wrapped here), the inlier count of every hypothesis recomputed with the
reference's LSLinearRegressor.fit / predict, best_n, the first hypothesis that reaches it, the last best model's parameters and its
inlier mask (dtu_3d_process.py:39-40).  Only data goes into the file.

What a test may hold a restatement to is asserted here on the cloud that is written: against an fp64 cross-product restatement, at least
90 of the 100 hypotheses have a triangle with |m.z| / (|e1||e2|) > 0.05 (the reference's fp32 matrix inverse is meaningless on slivers),
on those the reference's count differs by at most the number of points whose fp64 |r^2 - thresh| < 1e-3 thresh, and the argmax agrees."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402
import make_golden                                              # noqa: E402

OUT = os.path.join(HERE, 'ransac_plane.npz')
MIN_SHAPE, EDGE = 0.05, 1e-3


def cloud(seed=20240):
    rng = np.random.RandomState(seed)
    N, k = 4096, int(0.55 * 4096)
    xy = rng.uniform(-1, 1, (N, 2))
    z = 0.07 + 0.25 * xy[:, 0] - 0.15 * xy[:, 1] + 0.01 * rng.randn(N)
    blob = 0.35 * rng.randn(N, 3) + np.array([0.1, -0.2, 0.6])
    pts = np.where((np.arange(N) < k)[:, None], np.concatenate([xy, z[:, None]], 1), blob)
    return pts[rng.permutation(N)].astype(np.float32)


def restated(points, triples, thresh):
    """fp64: (count, number of points within EDGE * thresh of the threshold, triangle shape |m.z| / (|e1||e2|)) per hypothesis"""
    p = points.astype(np.float64)
    out = []
    for t in triples:
        a, b, c = p[t]
        m = np.cross(b - a, c - a)
        shape = abs(m[2]) / max(np.linalg.norm(b - a) * np.linalg.norm(c - a), 1e-300)
        if m[2] == 0:
            out.append((-1, 0, 0.0))
            continue
        n = m / m[2]
        r2 = (p @ n - n @ a) ** 2
        out.append((int((r2 < thresh).sum()), int((np.abs(r2 - thresh) < EDGE * thresh).sum()), shape))
    return np.array(out)


def main():
    make_golden.import_reference()
    import importlib
    ransac = importlib.import_module('utils.ransac')
    pts = cloud()
    X, y = torch.from_numpy(pts[:, :2].copy()), torch.from_numpy(pts[:, 2:3].copy())
    drawn, randint = [], torch.randint

    def recording(*a, **kw):
        out = randint(*a, **kw)
        drawn.append(out.clone())
        return out
    r = ransac.Ransac()
    torch.randint = recording
    try:
        r.fit(X, y)
    finally:
        torch.randint = randint
    B, P = r.batch_size, r.n_points
    assert len(drawn) == r.n_iter // B and all(d.shape == (B * P,) for d in drawn)
    triples = torch.cat(drawn).view(-1, P).numpy().astype(np.int32)
    counts = []
    for idxs in drawn:
        m = ransac.LSLinearRegressor().fit(X[idxs].view(B, P, -1), y[idxs].view(B, P, -1))
        diff = (y[None].expand(B, -1, -1) - m.predict(X[None].expand(B, -1, -1))).flatten(1)
        counts.append((diff.pow(2) < r.thresh).sum(1))
    counts = torch.cat(counts).numpy().astype(np.int32)
    assert int(counts.max()) == r.best_n
    model = r.best_models[-1]
    mask = ((model.predict(X) - y).pow(2) < r.thresh)[:, 0].numpy()
    params = model.params.reshape(3).numpy().astype(np.float64)
    best = int(np.argmax(counts))

    ref = restated(pts, triples, r.thresh)
    ok = ref[:, 2] > MIN_SHAPE
    diff = np.abs(ref[:, 0] - counts)
    assert ok.sum() >= 90, ok.sum()
    assert (diff[ok] <= ref[ok, 1]).all(), (diff[ok], ref[ok, 1])
    assert ok[best] and int(np.argmax(np.where(ok, ref[:, 0], -1))) == best and int(mask.sum()) == r.best_n
    print(f'{int(ok.sum())} of {len(ok)} hypotheses compared, {int((diff[ok] > 0).sum())} differ from the fp64 restatement (by at most {int(diff[ok].max())}), '
          f'best {best} with {r.best_n} inliers, params {params}')
    np.savez_compressed(OUT, points=pts, triples=triples, counts=counts, best=np.int32(best), best_n=np.int32(r.best_n), params=params,
                        mask=mask, thresh=np.float64(r.thresh))


if __name__ == '__main__':
    main()
