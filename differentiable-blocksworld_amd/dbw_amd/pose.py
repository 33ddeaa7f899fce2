"""Camera pose refinement: one 6-vector delta = (w, tau) per training view that perturbs the view's camera in its own frame,
R' = R.E(w), T' = T.E(w) + tau (csrc/pose_math.h), optimised by Adam beside the model -- what Nerfstudio's camera optimiser does for the
poses of a capture that COLMAP or a phone's tracker left a pixel or two off.

PoseRefiner holds the state; ops.pose_apply (dbw_lens_pose_apply / dbw_lens_pose_chain) and the camera gradients of the render nodes
(dbw_lens_pose_grad) are the kernels.  The writers at the end put the refined poses back into the capture's own files."""
import json
import os

import numpy as np
import torch

from . import ops
from .refine import FlatRefiner, parse_entry

FLIP = np.array([-1.0, 1.0, -1.0])            # dataset.CustomScene: OpenGL camera axes -> the renderer's (PyTorch3D's)


class PoseRefiner(FlatRefiner):
    """delta (V,6) of a scene's V training views, its gradient and the two Adam moments as flat fp32 buffers on `device` (refine.FlatRefiner).
    apply(batch) -> the batch with R, T refined through ops.pose_apply (batch['view_ids']: the rows, distinct; 'view_ids_host', where the
    batch carries it, is the same on the host and spares the check a wait for the device -- whoever builds the batch guarantees that the
    two are equal, ops.pose_apply does not compare them); the backward of the step
    leaves d loss / d delta in `grad`; step() is dense Adam over all V rows like torch.optim.Adam on the tensor (rows of views outside the
    batch have zero gradient, their moments decay) and then clears `grad`.  rot / trans = False keep that half of delta at 0.
    adam_fn / apply_fn: stand-ins for ops.adam_step_ / ops.pose_apply with the same signatures (tests on CPU tensors: the kernels have no
    CPU form)."""

    STATE_KEY = 'delta'
    SAVED = ('rot', 'trans')

    def __init__(self, n_views, device, lr=1e-4, betas=(0.9, 0.999), rot=True, trans=True, eps=1e-8, adam_fn=None, apply_fn=None):
        self.n_views = int(n_views)
        self.rot, self.trans = bool(rot), bool(trans)
        super().__init__((self.n_views, 6), device, lr, betas, eps, adam_fn)
        self.delta = self._param()
        self.apply_fn = apply_fn or ops.pose_apply

    def apply(self, batch):
        if 'view_ids' not in batch:
            raise KeyError("PoseRefiner.apply: the batch carries no 'view_ids' (the rows of delta of its views)")
        extra = {'ids_host': batch['view_ids_host']} if 'view_ids_host' in batch else {}
        R, T = self.apply_fn(batch['R'], batch['T'], self.delta, batch['view_ids'], **extra)
        return dict(batch, R=R, T=T)

    def _mask_grad(self):
        g = self.grad.view(self.n_views, 6)
        if not self.rot:
            g[:, :3].zero_()
        if not self.trans:
            g[:, 3:].zero_()

    def refined(self, R0, T0):
        """All V refined poses from the V given ones (in the order of delta's rows), detached."""
        ids = torch.arange(self.n_views, device=R0.device, dtype=torch.int32)
        with torch.no_grad():
            R, T = self.apply_fn(R0, T0, self.delta.detach(), ids)
        return R, T

    def _state_mismatch(self, numel):
        return f"pose_refine: a state of {numel // 6} views for a refiner of {self.n_views}"


def parse_config(entry):
    """training.pose_refine of a config -> dict(lr, start_epoch, rot, trans), or None where the key is absent / null / false."""
    return parse_entry('pose_refine', entry, 1e-4, {'rot': (True, bool), 'trans': (True, bool)})


def _rodrigues64(w):
    """E = exp([w]x) in float64 with the sign convention of csrc/pose_math.h (K x = w x x for a column x)."""
    w = np.asarray(w, dtype=np.float64)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    t = float(w @ w)
    if t < 1e-8:
        a, b = 1.0 - t / 6.0, 0.5 - t / 24.0
    else:
        th = np.sqrt(t)
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / t
    return np.eye(3) + a * K + b * (K @ K)


def camera_corrections(delta):
    """(V,6) refinements -> (V,4,4) float64 matrices C with refined camera-to-world = camera-to-world @ C, for OpenGL camera-to-world
    matrices in the frame R, T live in.  The renderer's view coordinates are v = flip * v_gl; v' = v.E + tau there reads
    v_gl' = (D E^T D) v_gl + D tau with D = diag(flip): the world-to-camera matrix gains that factor on the left, the camera-to-world matrix
    its inverse on the right.  delta = 0 gives the identity exactly."""
    delta = np.asarray(delta, dtype=np.float64).reshape(-1, 6)
    out = np.tile(np.eye(4), (len(delta), 1, 1))
    for i, d in enumerate(delta):
        if not d.any():
            continue
        G = np.eye(4)
        G[:3, :3] = FLIP[:, None] * _rodrigues64(d[:3]).T * FLIP[None, :]
        G[:3, 3] = FLIP * d[3:]
        out[i] = np.linalg.inv(G)
    return out


def refined_transforms(scene, delta):
    """The capture's transforms.json (dataset.CustomScene `scene`, its TRAIN split) as a dict, with the transform_matrix of every training
    frame replaced by the refined camera-to-world matrix in the FILE's frame: the flip of CustomScene undone, world-to-camera inverted, and
    the way back through scale_mat -- the file's frame differs from the normalised one by a rigid motion and the scale 1 / s, so the
    correction of camera_corrections keeps its rotation and its translation is divided by s.  Rows of delta follow scene.ids()."""
    ids = list(scene.ids())
    delta = np.asarray(torch.as_tensor(delta).detach().cpu().reshape(-1, 6), dtype=np.float64)
    if len(delta) != len(ids):
        raise ValueError(f'{len(delta)} refinements for {len(ids)} training frames')
    with open(scene.data_path / 'transforms.json') as fp:
        meta = json.load(fp)
    inv_s = float(np.cbrt(np.linalg.det(scene.scale_mat.double().numpy()[:3, :3])))       # scale_mat = inv(diag(s, s, s, 1) @ rigid)
    C = camera_corrections(delta)
    C[:, :3, 3] *= inv_s
    for i, c in zip(ids, C):
        frame = meta['frames'][i]
        M = np.asarray(frame['transform_matrix'], dtype=np.float64)
        M4 = np.eye(4)
        M4[:M.shape[0], :4] = M[:, :4]
        frame['transform_matrix'] = (M4 @ c)[:M.shape[0]].tolist()
    return meta


def write_refined(scene, refiner, run_dir, R0, T0):
    """<run_dir>/transforms_refined.json for a custom capture, <run_dir>/poses_refined.npz (R, T, delta of the training views) for a
    scene of another kind (DTU / BlendedMVS: poses come from cameras.npz).  -> the path written."""
    delta = refiner.flat.detach().view(-1, 6).cpu()
    if getattr(scene, 'name', None) == 'custom':
        path = os.path.join(str(run_dir), 'transforms_refined.json')
        with open(path, 'w') as f:
            json.dump(refined_transforms(scene, delta), f, indent=1)
        return path
    R, T = refiner.refined(R0, T0)
    path = os.path.join(str(run_dir), 'poses_refined.npz')
    np.savez(path, R=R.cpu().numpy(), T=T.cpu().numpy(), delta=delta.numpy())
    return path
