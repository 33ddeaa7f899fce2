"""Intrinsics refinement: four numbers theta = (a_x, a_y, c_x, c_y) that correct the one pinhole matrix the views of a scene
share -- K'[0,0] = K0[0,0] exp(a_x), K'[1,1] = K0[1,1] exp(a_y), K'[0,2] = K0[0,2] + c_x, K'[1,2] = K0[1,2] + c_y (csrc/intrinsics_math.h) --
optimised by Adam beside the model: the focal length a phone exporter wrote down, or COLMAP's after a rectification, is a percent off.

IntrinsicsRefiner holds the state; ops.intrinsics_apply (dbw_lens_intrinsics_apply / dbw_lens_intrinsics_chain) and the K gradient of the
render nodes (dbw_lens_intrinsics_grad) are the kernels.  The writers at the end put the refined values into <run_dir>/intrinsics_refined.yml
and, where the trained pinhole is the file's own, back into the capture's transforms.json.

The gauge.  A focal scale and the cameras' distance along their axes change the image almost alike, and so do a principal-point offset and a
small rotation of every camera: with training.pose_refine on as well, the pairs are nearly degenerate and only their combination is
determined by the images.  The default therefore refines ONE shared focal scale and nothing else."""
import json
import os

import numpy as np
import torch

from . import ops
from .refine import FlatRefiner, parse_entry

FOCAL_MODES = ('shared', 'separate', False)


class IntrinsicsRefiner(FlatRefiner):
    """theta (4) of a scene's shared K0 (4,4), its gradient and the two Adam moments as flat fp32 buffers on `device` (refine.FlatRefiner).
    apply(batch) -> the batch with 'K_live' = ops.intrinsics_apply(K0, theta); the backward of the step leaves d loss / d theta in `grad`;
    step() is Adam on the four numbers and then clears `grad`.  focal: 'shared' -- one scale for both focal lengths: g_a_y is added into
    g_a_x before the step and a_x copied to a_y after it, so the two stay equal bit for bit --, 'separate', or False (both stay 0);
    principal=False keeps the offsets at 0.  A frozen component has its gradient zeroed: its moments stay 0 and so does it.
    adam_fn / apply_fn: stand-ins for ops.adam_step_ / ops.intrinsics_apply with the same signatures (tests on CPU tensors: the kernels have
    no CPU form)."""

    SAVED = ('focal', 'principal', 'K0')

    def __init__(self, K0, device, lr=1e-4, betas=(0.9, 0.999), focal='shared', principal=False, eps=1e-8, adam_fn=None, apply_fn=None):
        if focal is True:
            focal = 'shared'
        if focal not in FOCAL_MODES:
            raise ValueError(f"focal: 'shared', 'separate' or False, got {focal!r}")
        self.focal, self.principal = focal, bool(principal)
        self.K0 = torch.as_tensor(K0, dtype=torch.float32).reshape(-1, 4, 4)[0].detach().clone().contiguous().to(device)
        super().__init__((4,), device, lr, betas, eps, adam_fn)
        self.theta = self._param()
        self.apply_fn = apply_fn or ops.intrinsics_apply

    def apply(self, batch):
        return dict(batch, K_live=self.apply_fn(self.K0, self.theta))

    def _mask_grad(self):
        g = self.grad
        if self.focal == 'shared':
            g[0:1] += g[1:2]
            g[1:2].zero_()
        elif not self.focal:
            g[0:2].zero_()
        if not self.principal:
            g[2:4].zero_()

    def _after_update(self):
        if self.focal == 'shared':
            self.flat[1:2].copy_(self.flat[0:1])

    def refined(self):
        """K' (4,4), detached."""
        with torch.no_grad():
            return self.apply_fn(self.K0, self.theta.detach()).detach()

    def _state_mismatch(self, numel):
        return f"intrinsics_refine: a state of {numel} numbers, theta has 4"


def parse_config(entry):
    """training.intrinsics_refine of a config -> dict(lr, start_epoch, focal, principal), or None where the key is absent / null / false."""
    def focal_mode(focal):
        focal = 'shared' if focal is True else (False if focal is None else focal)
        if focal not in FOCAL_MODES:
            raise ValueError(f"training.intrinsics_refine.focal: 'shared', 'separate' or false, got {focal!r}")
        return focal
    return parse_entry('intrinsics_refine', entry, 1e-4, {'focal': ('shared', focal_mode), 'principal': (False, bool)})


def pixels(K, size):
    """(fl_x, fl_y, cx, cy) in pixels of an image of size (H, W) from an NDC matrix K: the inverse of dataset.CustomScene's construction
    (NDC unit = half the shorter side, the principal point's sign flipped, pixel centres at +0.5 like the file's)."""
    K = np.asarray(torch.as_tensor(K).detach().cpu().reshape(-1, 4, 4)[0], dtype=np.float64)
    H, W = size
    s = min(H, W) / 2.0
    return float(K[0, 0] * s), float(K[1, 1] * s), float(W / 2.0 - K[0, 2] * s), float(H / 2.0 - K[1, 2] * s)


def file_level_refusal(scene):
    """-> why refined fl_x, fl_y, cx, cy cannot be written back into this scene's transforms.json, or None where the trained pinhole is the
    file's own camera rescaled."""
    if getattr(scene, 'name', None) != 'custom':
        return f"a '{getattr(scene, 'name', None)}' scene has no transforms.json: its cameras come from projection matrices"
    if getattr(scene, 'cameras', 'shared') != 'shared':
        return "cameras: per_frame -- the trained K is the common pinhole the frames were rectified into, not a camera of the file"
    if any(float(c) != 0.0 for c in (scene.dist or ())):
        return 'the capture has lens coefficients: the trained K belongs to the rectified frames, the file values to the distorted ones'
    if float(scene.zoom) != 1.0:
        return f'the frames were zoomed by {scene.zoom}: the trained K is not the file camera'
    return None


def refined_transforms(scene, K, base=None):
    """The capture's transforms.json as a dict -- `base`: the dict to update instead (the one pose refinement made) -- with fl_x, fl_y, cx,
    cy replaced by those of the refined NDC matrix K at the file's own frame size, at the top level and on every frame that carries its own.
    ValueError where file_level_refusal(scene) says why not."""
    why = file_level_refusal(scene)
    if why is not None:
        raise ValueError(f'intrinsics_refine: no file-level values: {why}')
    if base is None:
        with open(scene.data_path / 'transforms.json') as fp:
            base = json.load(fp)
    values = dict(zip(('fl_x', 'fl_y', 'cx', 'cy'), pixels(K, scene.raw_img_size)))
    for k, v in values.items():
        on_frames = [f for f in base['frames'] if k in f]
        if k in base or not on_frames:
            base[k] = v
        for f in on_frames:
            f[k] = v
    return base


def write_refined(scene, refiner, run_dir, img_size, after_pose=False):
    """<run_dir>/intrinsics_refined.yml, always: K0, K', theta and the focal lengths and principal point in pixels of the training image size
    `img_size` (H, W).  For a custom capture whose trained pinhole is the file's own, also <run_dir>/transforms_refined.json with the refined
    fl_x, fl_y, cx, cy -- after_pose: the file pose refinement has just written there is updated; else it is made from the capture's
    transforms.json.  For any other scene the yml says why there is no such file.  -> the paths written."""
    import yaml
    run_dir = str(run_dir)
    K0, K1 = refiner.K0.detach().cpu(), refiner.refined().cpu()
    theta = [float(v) for v in refiner.flat.detach().cpu().tolist()]
    names = ('fl_x', 'fl_y', 'cx', 'cy')
    why = 'no training scene was given' if scene is None else file_level_refusal(scene)
    out = {'K0': [[float(v) for v in row] for row in K0.tolist()], 'K': [[float(v) for v in row] for row in K1.tolist()],
           'theta': dict(zip(('a_x', 'a_y', 'c_x', 'c_y'), theta)), 'focal': refiner.focal, 'principal': refiner.principal, 'n_steps': refiner.n_steps,
           'image_size': [int(img_size[0]), int(img_size[1])], 'pixels0': dict(zip(names, pixels(K0, img_size))),
           'pixels': dict(zip(names, pixels(K1, img_size))), 'transforms_refined': why is None}
    if why is not None:
        out['transforms_refined_reason'] = why
    paths = [os.path.join(run_dir, 'intrinsics_refined.yml')]
    with open(paths[0], 'w') as f:
        yaml.safe_dump(out, f, sort_keys=False)
    if why is None:
        path, base = os.path.join(run_dir, 'transforms_refined.json'), None
        if after_pose:
            with open(path) as f:
                base = json.load(f)
        with open(path, 'w') as f:
            json.dump(refined_transforms(scene, K1, base), f, indent=1)
        paths.append(path)
    return paths
