"""The world frame of a custom scene from its point cloud and cameras: model.mesh's R_world, T_world and S_world, which the reference's
README (section 3, "Train on a custom scene") asks the user to estimate "by visual comparisons in plotly or Blender".

    rotation_to_euler(R)                          (elev, azim, roll) in degrees with mesh.world_rotation(elev, azim, roll) == R
    estimate_world_frame(points, cam2world, ...)  -> WorldFrame: a robust ground plane (eval3d.plane_ransac, the HIP kernel for device
                                                  tensors) and the frame derived from it
    WorldFrame.mesh_kwargs() / .yaml()            the three config entries, as a dict / as text for a config file

The model places a vertex v at (v * S_world) @ R_world + T_world (dbw.py:59,264): row 1 of R_world is the image of the model's +y axis, the
normal of its ground, and the initial ground is the model plane y = -0.9 T_range[1] (dbw.py:100)."""
import math

import numpy as np
import torch

from . import eval3d

MIN_POINTS = 100                 # below this the cloud is refused
MIN_OBJECT_POINTS = 50           # below this the object is placed under the cameras' common look-at point
SKY_DOME = 10                    # the sky dome's radius is SKY_DOME * S_world (z_far, dbw.py:74)


def rotation_to_euler(R):
    """(elev, azim, roll) in degrees of a proper rotation R (3,3): mesh.world_rotation(elev, azim, roll) gives R back.  With
    R = elev @ azim @ roll of mesh._axis_rotation, R[0] = (ca cr, ca sr, sa), R[1,2] = -se ca, R[2,2] = ce ca.  At the gimbal lock (ca = 0)
    only elev -+ roll is determined: roll is set to 0 there."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    ca = math.hypot(R[0, 0], R[0, 1])
    azim = math.atan2(R[0, 2], ca)
    if ca > 1e-9:
        roll = math.atan2(R[0, 1], R[0, 0])
        elev = math.atan2(-R[1, 2], R[2, 2])
    else:                        # R[1] = (sa sin(elev - sa roll), cos(elev - sa roll), 0)
        roll = 0.0
        elev = math.atan2(math.copysign(1.0, R[0, 2]) * R[1, 0], R[1, 1])
    return tuple(math.degrees(a) for a in (elev, azim, roll))


class WorldFrame:
    """The estimate: S_world (float), R_world ((elev, azim, roll) in degrees), T_world (3 floats), matrix (3,3: the rotation itself), plane
    ((n (3,), d): n . p = d, n towards the cameras), c (3,: the foot of the object on the plane), r (the object's radius), r0 (the cameras'
    median distance from their common look-at point), n_inliers (points of the cloud within tau of the plane), tau."""

    def __init__(self, S_world, R_world, T_world, matrix, plane, c, r, r0, n_inliers, tau):
        self.S_world, self.R_world, self.T_world = float(S_world), tuple(float(a) for a in R_world), tuple(float(t) for t in T_world)
        self.matrix, self.plane, self.c, self.r, self.r0, self.n_inliers, self.tau = matrix, plane, c, float(r), float(r0), int(n_inliers), float(tau)

    def mesh_kwargs(self):
        return {'S_world': self.S_world, 'R_world': list(self.R_world), 'T_world': list(self.T_world)}

    def yaml(self):
        """The three entries as YAML (flow lists), to be pasted under model.mesh of a config of this package or of the reference."""
        import yaml
        return yaml.safe_dump(self.mesh_kwargs(), default_flow_style=None, sort_keys=False)

    def __repr__(self):
        return (f'WorldFrame(S_world={self.S_world:.4f}, R_world=[{", ".join(f"{a:.2f}" for a in self.R_world)}], '
                f'T_world=[{", ".join(f"{t:.4f}" for t in self.T_world)}], n_inliers={self.n_inliers}, r={self.r:.4f}, r0={self.r0:.4f})')


def camera_rig(cam2world):
    """OpenGL camera-to-world matrices (V,4,4) or (V,3,4) -> (C (V,3) centres, c0 (3,) the least-squares point nearest all optical axes, r0 the
    median distance of the centres from it, u (3,) the normalised mean camera up), fp64 numpy.  ValueError for parallel cameras."""
    c2w = np.asarray(torch.as_tensor(cam2world).detach().cpu().numpy(), dtype=np.float64)
    if c2w.ndim != 3 or c2w.shape[1] < 3 or c2w.shape[2] != 4 or len(c2w) < 2:
        raise ValueError(f'world frame: cam2world (V,4,4) with V >= 2 expected, got {c2w.shape}')
    C, f, up = c2w[:, :3, 3], -c2w[:, :3, 2], c2w[:, :3, 1]
    f = f / np.linalg.norm(f, axis=1, keepdims=True)
    P = np.eye(3)[None] - f[:, :, None] * f[:, None, :]
    A, b = P.sum(0), (P @ C[:, :, None]).sum(0)[:, 0]
    if np.linalg.eigvalsh(A)[0] < 1e-6 * len(C):
        raise ValueError('world frame: the optical axes of the cameras are parallel, they have no common look-at point')
    c0 = np.linalg.solve(A, b)
    r0 = float(np.median(np.linalg.norm(C - c0, axis=1)))
    u = up.mean(0)
    if not r0 > 0 or not np.linalg.norm(u) > 1e-9:
        raise ValueError('world frame: the cameras sit on their look-at point, or their up vectors cancel')
    return C, c0, r0, u / np.linalg.norm(u)


def plane_rotation(n):
    """R_world (3,3) whose row 1 is the unit normal n: row 0 the normalised projection of the world x axis onto the plane (of the world y axis
    where |n.x| > 0.9), row 2 = row 0 x row 1.  The yaw about n is arbitrary: the blocks start at random rotations."""
    n = np.asarray(n, dtype=np.float64)
    a = np.array([0.0, 1.0, 0.0]) if abs(n[0]) > 0.9 else np.array([1.0, 0.0, 0.0])
    r0 = a - n * (a @ n)
    r0 = r0 / np.linalg.norm(r0)
    return np.stack([r0, n, np.cross(r0, n)])


def estimate_world_frame(points, cam2world, T_range=(1, 1, 1), n_hyp=512, tau_rel=0.02, max_tilt=60.0, min_side=0.9, refine=2, seed=0, ransac=None):
    """The world frame of a capture from its cloud `points` (N,3) and its OpenGL camera-to-world matrices, both in the frame the cameras
    R, T live in -> WorldFrame.  points on a cuda device: the plane fit is the HIP kernel; on the CPU: eval3d.plane_ransac_torch.

    1. cameras: centres C, the point c0 nearest all optical axes, r0 = median |C - c0|, u = the mean camera up (camera_rig);
    2. plane: eval3d.plane_ransac with thresh tau = tau_rel * r0, the normal within max_tilt degrees of u, at least min_side of the cameras
       more than tau above it; ValueError if no hypothesis is admissible or the cloud has fewer than 100 points;
    3. object points: height h = n . p - d > 2 tau and |p - c0| < 0.75 r0; the foot c is the point of the plane at the component-wise
       (lower) median of their in-plane coordinates, r the 0.9-quantile (the ceil(0.9 k)-th smallest of k) of max(in-plane distance from c, h);
       with fewer than 50 such points c is the foot of c0 and r = 0.4 r0;
    4. S_world = max(0.5 r, 1.5 max|C - c| / 10): DTU's S_world 0.5 goes with scenes in the unit sphere; every camera stays inside the sky dome;
    5. R_world = plane_rotation(n), reported as (elev, azim, roll); 6. T_world = c + n * 0.9 T_range[1] * S_world: the model's initial
    ground lies in the fitted plane.  Apart from the plane fit and the selection of step 3 (torch, on the device of the points) these
    are fp64 host operations on what two small reads bring back.  ransac: the plane fit to use instead of eval3d.plane_ransac (same
    signature: the tests pass the fp64 torch path)."""
    C, c0, r0, u = camera_rig(cam2world)
    points = torch.as_tensor(points)
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < MIN_POINTS:
        raise ValueError(f'world frame: a point cloud of at least {MIN_POINTS} points is needed (R_world: auto has no fallback), got '
                         f'{tuple(points.shape)}')
    tau = float(np.float32(tau_rel * r0))
    fit = (ransac or eval3d.plane_ransac)(points, n_hyp=n_hyp, thresh=tau, up=u, max_tilt=max_tilt, cams=C, min_side=min_side, refine=refine, seed=seed)
    got = torch.cat([fit.normal, fit.offset[None], fit.best[None].double(), fit.n_inliers[None].double()]).cpu().numpy()      # the one read
    if got[4] < 0:
        raise ValueError(f'world frame: none of the {n_hyp} plane hypotheses is admissible (normal within {max_tilt} degrees of the mean camera '
                         f'up, {min_side:.0%} of the cameras above it): the cloud shows no ground under the cameras')
    n, d = got[:3] / np.linalg.norm(got[:3]), float(got[3] / np.linalg.norm(got[:3]))
    Rw = plane_rotation(n)
    foot0 = c0 - n * (c0 @ n - d)

    dev = points.device
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)          # noqa: E731
    p = points.detach().to(torch.float64)
    h = p @ t(n) - d
    sel = (h > 2 * tau) & ((p - t(c0)).norm(dim=1) < 0.75 * r0)
    k = int(sel.sum())
    if k >= MIN_OBJECT_POINTS:
        q, hs = p[sel] - t(foot0), h[sel]
        s_, t_ = q @ t(Rw[0]), q @ t(Rw[2])
        ms, mt = s_.median(), t_.median()
        ext = torch.maximum(((s_ - ms) ** 2 + (t_ - mt) ** 2).sqrt(), hs)
        r = ext.kthvalue(max(1, math.ceil(0.9 * k))).values
        ms, mt, r = torch.stack([ms, mt, r]).cpu().tolist()
        c = foot0 + ms * Rw[0] + mt * Rw[2]
    else:
        c, r = foot0, 0.4 * r0
    S = max(0.5 * r, 1.5 * float(np.linalg.norm(C - c, axis=1).max()) / SKY_DOME)
    T = c + n * 0.9 * float(T_range[1]) * S
    return WorldFrame(S, rotation_to_euler(Rw), T.tolist(), Rw, (n, d), c, r, r0, int(got[5]), tau)


# ------------------------------------------------------------------------------------------------ where the blocks start
class BlockInit:
    """Block poses read off the clusters of a cloud: T (n,3), R_6d (n,6), S (n,3) fp32 tensors for the block slots index (n,) int64 (slot i gets
    the i-th most populous good cluster; the slots that are not in index keep their random draw), counts (n,) the points of each cluster,
    n_points_used the points that were clustered, n_blocks the model's block count."""

    def __init__(self, T, R_6d, S, index, counts, n_points_used, n_blocks):
        self.T, self.R_6d, self.S, self.index, self.counts = T, R_6d, S, index, counts
        self.n_points_used, self.n_blocks = int(n_points_used), int(n_blocks)

    def __len__(self):
        return int(self.index.shape[0])

    def as_dict(self):
        rows = lambda t: [[float(v) for v in r] for r in t.detach().cpu().tolist()]        # noqa: E731
        return {'n_blocks': self.n_blocks, 'n_points_used': self.n_points_used, 'index': [int(i) for i in self.index.cpu().tolist()],
                'counts': [int(c) for c in self.counts.cpu().tolist()], 'T': rows(self.T), 'R_6d': rows(self.R_6d), 'S': rows(self.S)}

    def yaml(self):
        """The seeded poses as YAML (flow lists): what <run_dir>/blocks_init.yml records."""
        import yaml
        return yaml.safe_dump(self.as_dict(), default_flow_style=None, sort_keys=False)

    def __repr__(self):
        return (f'BlockInit({len(self)} of {self.n_blocks} blocks from {self.n_points_used} points, counts='
                f'{[int(c) for c in self.counts.cpu().tolist()]})')


def blocks_from_points(points, S_world, R_world, T_world, n_blocks, T_range=(1, 1, 1), ratio_block_scene=0.25, scale_min=0.2, oversample=2, n_iter=20,
                       min_points=30, ground_margin=0.05, bound=2.0, extent_scale=math.sqrt(3), size_range=None, cluster=None):
    """Where the blocks of a model start, from the cloud `points` (N,3) of its scene (in the frame the cameras live in) -> BlockInit.  points
    on a cuda device: the clustering is the HIP kernel (eval3d.cluster_points); on the CPU: eval3d.cluster_points_torch.

    1. the model's scene frame: q = ((p - T_world) @ R_world^T) / S_world -- the model places v at (v * S_world) @ R_world + T_world; R_world is
       the (3,3) matrix (a (1,3,3) buffer is accepted), T_world (3,) or (1,3);
    2. the points kept: above the initial ground, q.y > -0.9 T_range[1] + ground_margin, and within |q.x| <= bound T_range[0],
       |q.z| <= bound T_range[2], q.y <= -0.9 T_range[1] + 2 bound T_range[1]; ValueError below MIN_POINTS of them;
    3. k-means with K' = min(oversample * n_blocks, 256, kept) centres: farthest-point seeding spends centres on stray points, and those
       clusters stay tiny -- oversampling is the defence against outliers;
    4. the clusters of at least min_points points, most populous first (the lower cluster index on ties), at most n_blocks: block slot i gets
       the i-th;
    5. T = the cluster's mean; R = its axes matrix (the model computes (v * S) @ R + T: row i of R is where block axis i points, the largest
       extent goes to block axis 0), R_6d = mesh.matrix_to_rotation_6d(R);
    6. the half-extent along axis i is a_i = extent_scale * sqrt(lambda_i) (a solid box, or a sphere's surface, of half-extent a has variance
       a^2 / 3) and a block's is ratio_block_scene * (exp(S_i) + scale_min): S_i = log(clamp(a_i / ratio_block_scene, lo, hi) - scale_min) with
       (lo, hi) = size_range or (scale_min + 0.1, 3.0).
    The selection of step 4 reads the counts (one small host read).  cluster: the clustering function to use instead of eval3d.cluster_points
    (same signature: the tests pass the torch path).  The fit is deterministic: the same cloud gives the same BlockInit on every call and on
    every rank of a data-parallel run."""
    from . import mesh
    points = torch.as_tensor(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f'blocks from points: points (N,3) expected, got {tuple(points.shape)}')
    n_blocks = int(n_blocks)
    if n_blocks < 1 or int(oversample) < 1:
        raise ValueError(f'blocks from points: n_blocks >= 1 and oversample >= 1 expected, got {n_blocks}, {oversample}')
    dev = points.device
    Rw = torch.as_tensor(R_world).detach().to(device=dev, dtype=torch.float32).reshape(3, 3)
    Tw = torch.as_tensor(T_world).detach().to(device=dev, dtype=torch.float32).reshape(1, 3)
    q = ((points.detach().to(torch.float32) - Tw) @ Rw.T) / float(S_world)
    tx, ty, tz = (float(t) for t in T_range)
    y0 = -0.9 * ty
    keep = (q[:, 1] > y0 + ground_margin) & (q[:, 1] <= y0 + 2 * bound * ty) & (q[:, 0].abs() <= bound * tx) & (q[:, 2].abs() <= bound * tz)
    q = q[keep].contiguous()
    kept = int(q.shape[0])
    if kept < MIN_POINTS:
        raise ValueError(f'blocks from points: at least {MIN_POINTS} points above the ground and within {bound} T_range of the scene are needed, '
                         f'got {kept} of {points.shape[0]}')
    K = min(int(oversample) * n_blocks, eval3d.CLUSTER_MAX_K, kept)
    fit = (cluster or eval3d.cluster_points)(q, K, n_iter=n_iter)
    counts = fit.counts.cpu().to(torch.int64)                                          # the one read
    order = torch.argsort(-counts, stable=True)                                        # most populous first, the lower index on ties
    good = order[counts[order] >= int(min_points)][:n_blocks].to(dev)
    lo, hi = size_range if size_range is not None else (scale_min + 0.1, 3.0)
    a = float(extent_scale) * fit.evals[good].clamp(min=0).sqrt()
    S = ((a / float(ratio_block_scene)).clamp(float(lo), float(hi)) - float(scale_min)).log().to(torch.float32)
    R_6d = mesh.matrix_to_rotation_6d(fit.axes[good].to(torch.float32))
    return BlockInit(fit.mean[good].to(torch.float32), R_6d, S, torch.arange(good.shape[0], device=dev), fit.counts[good], kept, n_blocks)
