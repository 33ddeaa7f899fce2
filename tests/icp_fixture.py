"""Inputs of the gradient ICP tests (tests/test_icp_host.py on the CPU, tests/test_gpu_icp.py on the device), built once per process.

ellipsoid_pair(): two batch elements on the ellipsoid with semi-axes (0.5, 0.35, 0.25) plus noise of 0.01; the ground truth is the first
1900 points, the prediction the last 2300 (400 shared) moved by a known rotation, shift (0.03, -0.02, 0.04) and scale 1.1, so the alignment
has to find T ~ (0.030, -0.020, 0.040) and s ~ 1.10.  N = 2, P1 = 2300, P2 = 1900: no multiple of the search's 2048 queries per workgroup,
more than one workgroup.  Well conditioned at lr = 0.01: torch in fp32 and in fp64 agree to ~1e-7 in R, T, s after 31 iterations.

aligned_pair(): the two halves of one such cloud, already aligned: gradients near zero, where Adam amplifies rounding noise -- only fit for
the keep-best logic (checks kept at 0, 30, 40 of 41), never for a comparison of values.  The same holds for ellipsoid_pair at lr = 0.3
(checks kept at 0 and 40 of 41)."""
import functools
import json
import os

import torch

from dbw_amd import eval3d, mesh

AXES = (0.5, 0.35, 0.25)
SHIFT = (0.03, -0.02, 0.04)
SCALE = 1.1


def _ellipsoid(seed, N, P):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(N, P, 3, dtype=torch.float64, generator=gen)
    g = g / g.norm(dim=2, keepdim=True) * torch.tensor(AXES, dtype=torch.float64)
    return g + 0.01 * torch.randn(N, P, 3, dtype=torch.float64, generator=gen)


@functools.lru_cache(maxsize=None)
def ellipsoid_pair():
    """-> (pc_pred (2,2300,3), pc_gt (2,1900,3)) fp32 on the CPU"""
    N, P1, P2 = 2, 2300, 1900
    g = _ellipsoid(0, N, 4000)
    Rt = mesh.rotation_6d_to_matrix(torch.tensor([[1., 0.15, -0.1, -0.1, 1., 0.2], [1., -0.2, 0.1, 0.15, 1., -0.1]], dtype=torch.float64))
    pg = g[:, :P2]
    pp = (g[:, 4000 - P1:] - torch.tensor(SHIFT, dtype=torch.float64)) @ Rt.transpose(1, 2) / SCALE
    return pp.float().contiguous(), pg.float().contiguous()


@functools.lru_cache(maxsize=None)
def aligned_pair():
    """-> (pc_pred (1,1500,3), pc_gt (1,1500,3)) fp32 on the CPU"""
    g = _ellipsoid(1, 1, 3000).float()
    return g[:, 1500:].contiguous(), g[:, :1500].contiguous()


@functools.lru_cache(maxsize=None)
def torch_run(dtype, anisotropic, n_iter=31):
    """gradient_icp_torch on ellipsoid_pair at lr 0.01 on the CPU in `dtype` -> (cloud, [R, T, s], trace); shared, never modified"""
    pp, pg = ellipsoid_pair()
    return eval3d.gradient_icp_torch(pp.to(dtype), pg.to(dtype), True, anisotropic, lr=0.01, n_iter=n_iter, return_trace=True)


def reference_spread(anisotropic):
    """the largest difference between the fp32 and the fp64 torch runs in R, T, s and the cloud: the yardstick of the device comparison"""
    c32, p32, _ = torch_run(torch.float32, anisotropic)
    c64, p64, _ = torch_run(torch.float64, anisotropic)
    return max(float((a.double() - b).abs().max()) for a, b in zip([c32] + p32, [c64] + p64))


def sphere_pair():
    """an icosphere scaled into the unit cube (the ground-truth mesh) and a copy rotated, shifted and scaled by 1.1 (the prediction)
    -> (verts_pred, verts_gt, faces)"""
    verts, faces = mesh.get_icosphere(3)
    verts = verts * torch.tensor([0.5, 0.4, 0.3])
    R = mesh.rotation_6d_to_matrix(torch.tensor([1., 0.2, -0.1, -0.15, 1., 0.1]))
    return (verts @ R) * SCALE + torch.tensor([0.04, -0.03, 0.02]), verts, faces


SPHERE_NAMES = ['chamfer-L1', 'chamfer-L1-ICP', 'normal-cos', 'normal-cos-ICP']
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SPHERE_GOLDEN = os.path.join(GOLDEN, 'icp_sphere_scores.json')
SPHERE_INPUTS = os.path.join(GOLDEN, 'icp_sphere_inputs.npz')
SPHERE_ARRAYS = ('pc_gt', 'norm_gt', 'pc', 'normals', 'pc2', 'normals2')


def sphere_evaluator():
    from dbw_amd import metrics
    return metrics.MeshEvaluator(names=SPHERE_NAMES, fast_cpu=True, n_points=5000)


def draw_sphere_inputs():
    """the draw behind tests/golden/icp_sphere_inputs.npz: 5 000 ground-truth points and normals of the ground-truth mesh, then the evaluator's
    two draws on the prediction, all from one seeded CPU generator -> dict of (1,5000,3) fp32 arrays.  Only tests/golden/make_icp_golden.py
    calls it: which face a sample falls on depends on the last bit of the face areas, so another machine may draw other points."""
    vp, vg, faces = sphere_pair()
    gen = torch.Generator().manual_seed(11)
    pc_gt, norm_gt = eval3d.sample_points_from_meshes(vg, faces, 5000, return_normals=True, generator=gen)
    samples = sphere_evaluator().draw_samples((vp, faces), True, gen)
    return dict(zip(SPHERE_ARRAYS, [t.numpy() for t in (pc_gt, norm_gt) + tuple(samples)]))


@functools.lru_cache(maxsize=None)
def sphere_case():
    """the MeshEvaluator case of the tests: the sphere pair at the fast_cpu settings (30 iterations) cut to 5 000 points, ground truth
    and samples drawn once on the CPU from one seeded generator and recorded (tests/golden/icp_sphere_inputs.npz), so that the recorded
    scores belong to them on every machine -> (mesh_pred, pc_gt, norm_gt, evaluator, samples)"""
    import numpy as np
    vp, vg, faces = sphere_pair()
    with np.load(SPHERE_INPUTS) as z:
        pc_gt, norm_gt, *samples = [torch.from_numpy(z[k]) for k in SPHERE_ARRAYS]
    return (vp, faces), pc_gt, norm_gt, sphere_evaluator(), tuple(samples)


def sphere_golden():
    """the scores of sphere_case() by the CPU path (gradient_icp_torch) in fp32 and in fp64, recorded by tests/golden/make_icp_golden.py
    (17 s of brute-force searches on the CPU), with a checksum of the recorded samples -> dict(fp32=, fp64=, checksum=)"""
    with open(SPHERE_GOLDEN) as f:
        return json.load(f)


def sphere_checksum():
    _, pc_gt, _, _, samples = sphere_case()
    return [float(pc_gt.double().sum()), float(samples[0].double().sum()), float(samples[2].double().sum())]


# ---- the model-blocks case of evaluate_aligned ----------------------------------------------------------------------------------------------
BLOCKS_CFG = {'model': {'name': 'dbw', 'mesh': {'n_blocks': 4, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 256},
                        'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                        'rend_optim': {'coarse_learning': 1500, 'decimate_txt': 750, 'decimate_factor': 8, 'kill_blocks': True,
                                       'decouple_rendering': True, 'opacity_noise': True},
                        'loss': {'rgb_weight': 1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}}}
BLOCKS_SEED = 227391
BLOCKS_INPUTS = os.path.join(GOLDEN, 'icp_blocks_inputs.npz')
BLOCKS_GOLDEN = os.path.join(GOLDEN, 'icp_blocks_scores.json')
BLOCKS_ARRAYS = ('verts_unit', 'gt', 'gt_normals', 'pc', 'normals', 'pc2', 'normals2')


def blocks_model(device='cpu'):
    import dbw_amd
    torch.manual_seed(BLOCKS_SEED)
    model = dbw_amd.create_model(BLOCKS_CFG, (75, 100)).to(device)
    model.eval()
    return model


def blocks_evaluator():
    from dbw_amd import metrics
    return metrics.MeshEvaluator(names=SPHERE_NAMES, fast_cpu=True, n_points=5000)


def draw_blocks_inputs(verts, faces):
    """the draw behind tests/golden/icp_blocks_inputs.npz, from the live blocks (verts, faces on the CPU) of blocks_model(): a ground truth in
    another frame and scale (5 000 samples of the blocks themselves, rotated, scaled by 40 and shifted) and the evaluator's two draws on the
    blocks in the ground truth's unit-cube frame -> dict of fp32 arrays.  Only tests/golden/make_icp_golden.py calls it."""
    gen = torch.Generator().manual_seed(5)
    pts, nrm = eval3d.sample_points_from_meshes(verts, faces, 5000, return_normals=True, generator=gen)
    R = mesh.rotation_6d_to_matrix(torch.tensor([1., 0.1, -0.05, -0.1, 1., 0.05]))
    gt, gt_n = (pts[0] @ R) * 40 + torch.tensor([3., -2., 5.]), nrm[0] @ R
    off, sc = eval3d.unit_cube_frame(gt)
    verts_unit = (verts - off) / sc
    samples = blocks_evaluator().draw_samples((verts_unit, faces), True, gen)
    return dict(zip(BLOCKS_ARRAYS, [t.contiguous().numpy() for t in (verts_unit, gt, gt_n) + tuple(samples)]))


@functools.lru_cache(maxsize=None)
def blocks_case():
    """-> (verts_unit (V,3): the blocks in the ground truth's unit-cube frame, gt (5000,3) in its own frame, gt_normals, samples), as recorded"""
    import numpy as np
    with np.load(BLOCKS_INPUTS) as z:
        verts_unit, gt, gt_n, *samples = [torch.from_numpy(z[k]) for k in BLOCKS_ARRAYS]
    return verts_unit, gt, gt_n, tuple(samples)


def blocks_golden():
    """the scores of blocks_case() by the CPU path in fp32 and in fp64, recorded by tests/golden/make_icp_golden.py -> dict(fp32=, fp64=)"""
    with open(BLOCKS_GOLDEN) as f:
        return json.load(f)
