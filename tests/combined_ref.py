"""Checker side of the combined step (DESIGN.md "The combined step against float64"): ONE fixed case with every optional training term
switched on -- validity masks, the SSIM term, per-view exposure, pose refinement, intrinsics refinement, the surface term and the free-space
term -- and the float64 reference of its loss values and gradients.  A helper of tests/test_combined_step_host.py (CPU: the case is not
vacuous and the reference agrees with the per-feature references) and tests/test_gpu_combined_step.py (GPU); not a test.

The case is the geometry of __graft_entry__.smoke() (tests/test_gpu_pose.py:_smoke_model): 2 views of 32 x 48, 3 blocks, 16^2 textures,
4 faces per pixel, detach_bary, coarse phase, no opacity noise, seed 227391, the overlap samples fixed -- so that oracle.OracleDBW applies.
Everything that is random here is drawn from its own seeded generator; callers must not write into what they get.

The reference, reference(): the fp32 oracle composite (orc.predict with R', T', K' as leaves) carried on in torch float64 -- rec = exp(g) *
composite + b on the batch's rows of the exposure table, the masked MSE over 3 * sum(mask), weight * phase factor * the masked SSIM term
(metrics.ssim_map, padding=True) -- plus the oracle's regularisers; its backward leaves the image-and-regulariser gradient of the ten
parameters, of R', T', K' and of the exposure table.  delta_grad64 / ktheta_grad64 carry gR, gT / gK through the float64 chains of
tests/pose_ref.py and tests/intrinsics_ref.py.  The two 3D terms have float64 VALUE references (surface_value64, freespace_value64:
tests/surface_ref.py, tests/freespace_ref.py on the device's vertices and opacities); their gradients are held by additivity in the GPU test."""
import functools

import numpy as np
import torch

import freespace_ref as FR
import intrinsics_ref as IR
import oracle as O
import pose_ref as PR
import surface_ref as SR

H, W, NB, TS, FPP = 32, 48, 3, 16, 4                             # the geometry of __graft_entry__.smoke()
SEED = 227391
WEIGHT = 0.1                                                     # perceptual_weight
N_ROWS, ROWS = 5, [3, 1]                                         # the tables' rows, and the batch's rows of them
TAU = 0.3                                                        # surface.tau and freespace.tau of the case
BACK, MARGIN = 0.5, 0.02                                         # the documented defaults of surface.back and freespace.margin (dbw.py)
STEP = 7                                                         # what the tests set model._rng_step to
N_CLOUD, N_RAYS = 600, 600
REL = 1e-4                                                       # tests/test_gpu_model.py
ORDER_ULPS = 8                                                   # tests/test_gpu_pose.py: the room of reordered float atomic sums
PARAMS = ('sq_eps', 'S', 'R_6d', 'T', 'alpha_logit', 'R_6d_ground', 'T_ground', 'texture_bkg', 'texture_ground', 'textures')
RIGS = {'smoke': dict(), 'horizon': dict(dist=2.8, elev_deg=5.0, f_ndc=1.5)}      # (tests/test_gpu_env_backward.py: the horizon across the view)


def model_cfg(image_terms=True, terms3d=True):
    """The model config of the case: the smoke config plus the SSIM term (image_terms) and the two 3D terms (terms3d)."""
    loss = {'rgb_weight': 1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}
    if image_terms:
        loss.update(perceptual_weight=WEIGHT, perceptual_name='ssim')
    if terms3d:
        loss.update(surface_weight=1.0, surface={'points': 0, 'tau': TAU}, freespace_weight=1.0, freespace={'rays': 0, 'tau': TAU})
    return {'model': {'name': 'dbw', 'mesh': {'n_blocks': NB, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': TS},
                      'renderer': {'faces_per_pixel': FPP, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                     'opacity_noise': False},
                      'loss': loss}}


def oracle():
    """A fresh oracle model of the case (its parameters are those create_model draws under the same seed)."""
    return O.OracleDBW((H, W), n_blocks=NB, txt_size=TS, faces_per_pixel=FPP, seed=SEED)


def masks():
    """(2,1,H,W): the two rectangles of tests/test_gpu_exposure.py:test_model_losses_and_gradients, plus one column of fractional weights."""
    m = torch.ones(2, 1, H, W)
    m[0, :, 8:17, 20:33] = 0
    m[1, :, :, :5] = 0
    m[0, :, :, 40] = 0.25
    m[1, :, :, 40] = 0.5
    return m


def exposure_theta():
    """(5,6): _theta() of tests/test_gpu_exposure.py."""
    return (torch.rand(N_ROWS, 6, generator=torch.Generator().manual_seed(11)) - 0.5) * 0.6


def pose_delta():
    """(5,6): about 1 degree and 1 % of the camera distance (2.8) -- the `star` rows of tests/test_gpu_pose.py:_refinement_run at the batch's
    rows 3 and 1, other non-zero rows elsewhere (a step that read them would not meet the reference)."""
    d = torch.tensor([[0.006, 0.004, -0.007, -0.012, 0.01, 0.006],
                      [-0.010, 0.011, -0.009, -0.018, 0.02, 0.015],
                      [-0.008, -0.005, 0.009, 0.015, 0.012, -0.02],
                      [0.012, -0.009, 0.008, 0.02, -0.015, 0.018],
                      [0.003, 0.013, 0.004, -0.01, -0.017, 0.011]])
    return d


def intrinsics_theta():
    """(4): both focal lengths about 2 % off (one up, one down: focal 'separate'), the principal point 0.01 NDC off."""
    return torch.tensor([0.0198, -0.0202, 0.01, -0.01])


@functools.lru_cache(maxsize=None)
def case(rig='smoke'):
    """The fixed inputs on the CPU: dict(imgs, R, T, K (the batch's two views, before refinement), K0 (4,4), u (overlap samples), masks,
    mask_sum, exposure (5,6), delta (5,6), ktheta (4), rows, cloud (N,3), ends, frame, origins (the free-space rays), block_v (NB,nv,3):
    the oracle's posed block vertices the cloud and the rays were laid out around)."""
    orc = oracle()
    R, T, Km = O.synthetic_cameras(2, R_world=orc.R_world[0], **RIGS[rig])
    g = torch.Generator().manual_seed(0)
    imgs, u = torch.rand(2, 3, H, W, generator=g), torch.rand(NB, 1000, 3, generator=g)
    with torch.no_grad():
        block_v = orc.build_blocks(True, True, False)['verts'].reshape(NB, -1, 3).clone()
    m = masks()
    c = dict(imgs=imgs, R=R.contiguous(), T=T.contiguous(), K=Km, K0=Km[0].clone(), u=u, masks=m, mask_sum=float(m.double().sum()),
             exposure=exposure_theta(), delta=pose_delta(), ktheta=intrinsics_theta(), rows=list(ROWS), block_v=block_v)
    c['cloud'] = _cloud(block_v)
    c['ends'], c['frame'], c['origins'] = _rays(block_v, R, T)
    return c


def _cloud(block_v, n=N_CLOUD, shift=0.1, half=0.12):
    """tests/test_gpu_surface.py:_two_boxes for NB blocks -- points on the faces of a box next to each block, a tenth of a unit off its
    centre -- and, for every tenth point, a copy lifted 1.2 units off: farther than tau from every face, so that the truncation is live."""
    centres = block_v.mean(1)
    g = torch.Generator().manual_seed(5)
    p = (torch.rand(n, 3, generator=g) * 2 - 1) * half
    axis, side = torch.randint(0, 3, (n,), generator=g), torch.randint(0, 2, (n,), generator=g) * 2 - 1
    p[torch.arange(n), axis] = (side * half).float()
    p = p + centres[torch.arange(n) % NB] + shift
    up = torch.tensor([0.0, 1.0, 0.0]) @ O.world_rotation(115, 0, 0)            # the model frame's "up" in world coordinates
    p[::10] += 1.2 * up
    return p.contiguous()


def _rays(block_v, R, T, n=N_RAYS, stretch=1.8, clear=0.7):
    """tests/test_gpu_freespace.py:_rays_behind_the_blocks: rays from the two camera centres, each aimed at a jittered block vertex and
    carried on to `stretch` times its distance; ends closer than `clear` to a block vertex are left out.  Those rays end under the ground,
    which stops the ones that pass beside a block; every third ray is aimed one unit above its vertex and ends in the air over the
    ground: some rays are stopped and some are not (tests/test_combined_step_host.py)."""
    v = block_v.reshape(-1, 3)
    origins = -torch.einsum('nij,nj->ni', R, T)                  # x_cam = x R + T: the centres
    g = torch.Generator().manual_seed(5)
    frame = torch.randint(0, len(origins), (n,), generator=g)
    aim = v[torch.randint(0, len(v), (n,), generator=g)] + 0.12 * torch.randn(n, 3, generator=g)
    aim[::3] += torch.tensor([0.0, 1.0, 0.0]) @ O.world_rotation(115, 0, 0)      # (the model frame's "up" in world coordinates)
    ends = origins[frame] + stretch * (aim - origins[frame])
    keep = torch.cdist(ends, v).min(1).values > clear
    return ends[keep].contiguous(), frame[keep].to(torch.int32).contiguous(), origins.contiguous()


# ---------------------------------------------------------------------------------------------------------------- refinement on the host
def refined_cameras64(c):
    """(R' (2,3,3), T' (2,3), K' (4,4)) of the case in float64 rounded to fp32: what pose_apply / intrinsics_apply give up to their bars --
    the CPU tests' stand-in for the device's values."""
    R1, T1 = [], []
    for b, v in enumerate(c['rows']):
        r, t, _ = PR.refine_torch(c['R'][b], c['T'][b], c['delta'][v], torch.float64)
        R1.append(r.float())
        T1.append(t.float())
    return torch.stack(R1), torch.stack(T1), IR.refine_torch(c['K0'], c['ktheta'], torch.float64).float()


def delta_grad64(R0, T0, delta, rows, gR, gT):
    """The float64 chain of tests/pose_ref.py: d (sum gR . R' + sum gT . T') / d delta -> (V,6) float64; rows outside `rows` are 0."""
    d = delta.detach().double().clone().requires_grad_(True)
    total = 0.0
    for b, v in enumerate(rows):
        R1, T1, _ = PR.refine_torch(R0[b], T0[b], d[v], torch.float64)
        total = total + (R1 * gR[b].double()).sum() + (T1 * gT[b].double()).sum()
    total.backward()
    return d.grad


def ktheta_grad64(K0, ktheta, gK):
    """The float64 chain of tests/intrinsics_ref.py: d sum(gK . K') / d theta -> (4) float64."""
    th = ktheta.detach().double().clone().requires_grad_(True)
    (IR.refine_torch(K0, th, torch.float64) * gK.double()).sum().backward()
    return th.grad


# ---------------------------------------------------------------------------------------------------------------- the image terms, float64
def image_terms64(comp, imgs, mk, rows_theta, factor):
    """comp, imgs (N,3,H,W), mk (N,1,H,W), rows_theta (N,6) float64 -> (rec, rgb, perceptual): tests/test_gpu_exposure.py:242-256."""
    from dbw_amd import metrics
    rec = rows_theta[:, :3].exp()[:, :, None, None] * comp + rows_theta[:, 3:, None, None]
    count = 3 * mk.sum().item()
    rgb = (mk * (rec - imgs) ** 2).sum() / count
    per = WEIGHT * factor * ((1 - metrics.ssim_map(imgs * mk, rec * mk, padding=True)) * mk).sum() / count
    return rec, rgb, per


def reference(orc, imgs, R1, T1, K1, mk, theta, rows, u, verts_at=None, factor=1.0, n_threads=8):
    """The float64 reference of the image terms and the regularisers at the cameras (R1, T1, K1) -- fp32 CPU tensors, the device's where the
    caller has them -- and, with verts_at, at the device's vertices.  -> dict: rgb, perceptual, regs (the oracle's dict, fp32), total_img
    (their float64 sum), and the gradients of total_img: params {name: grad}, R, T (fp32 leaves of the oracle), K (4,4), theta (V,6)
    float64.  orc's parameter gradients are cleared first and hold the result afterwards."""
    for p in orc.p.values():
        p.grad = None
    Rl, Tl, Kl = (t.detach().clone().float().requires_grad_(True) for t in (R1, T1, K1))
    orc.Kmat = Kl                                                # (predict keeps a given matrix: the live K in place of the frozen one)
    comp = orc.predict(dict(R=Rl, T=Tl, K=Kl[None]), training=True, coarse=True, decimate=False, opacity_noise=None, n_threads=n_threads,
                       verts_at=verts_at)
    th = theta.detach().double().clone().requires_grad_(True)
    rec, rgb, per = image_terms64(comp.double(), imgs.double(), mk.double(), th[list(rows)], factor)
    w, orc.loss_weights = orc.loss_weights, {k: v for k, v in orc.loss_weights.items() if k != 'rgb'}
    try:
        regs = orc.compute_losses(imgs, None, coarse=True, overlap_points=u)
    finally:
        orc.loss_weights = w
    total = regs.pop('total').double() + rgb + per
    total.backward()
    return dict(rgb=rgb.item(), perceptual=per.item(), regs={k: v.item() for k, v in regs.items()}, total_img=total.item(), rec=rec.detach(),
                params={k: orc.p[k].grad.clone() for k in PARAMS}, R=Rl.grad.clone(), T=Tl.grad.clone(), K=Kl.grad.clone(), theta=th.grad.clone())


# ---------------------------------------------------------------------------------------------------------------- the 3D terms, float64 values
def term_scene(ground_v, block_v, faces, face_group, vert_group, group_alpha):
    """The scene the two 3D terms measure against, as tests/surface_ref.py and tests/freespace_ref.py take it: numpy, the vertices
    [ground, blocks] and the model's constant tables (dbw._surface_tables)."""
    n = lambda t: t.detach().cpu().numpy()                                      # noqa: E731
    verts = np.concatenate([n(ground_v).reshape(-1, 3), n(block_v).reshape(-1, 3)], 0).astype(np.float32)
    return dict(verts=verts, faces=n(faces).astype(np.int32), face_group=n(face_group).astype(np.int32), group_keep=None,
                vert_group=n(vert_group).astype(np.int32), group_alpha=n(group_alpha).astype(np.int32), n_blocks=NB)


def surface_value64(sc, cloud, alpha, weight=1.0, tau=TAU, back=BACK, idx=None):
    """weight * (forward mean + back * back mean) of tests/surface_ref.py on the points cloud[idx] (all of them in order without idx)."""
    pts = np.asarray(cloud, np.float32)
    drawn = pts if idx is None else pts[idx]
    fwd, bk = SR.term_value(drawn, sc['verts'], sc['faces'], None, tau, pts, np.asarray(alpha, np.float64), sc['vert_group'], back,
                            float(NB * SR.BNV))
    return weight * (fwd + back * bk)


def freespace_value64(sc, ends, frame, origins, alpha, weight=1.0, tau=TAU, margin=MARGIN):
    return weight * FR.term_value(np.asarray(ends, np.float32), np.asarray(frame), np.asarray(origins, np.float32), sc, np.asarray(alpha, np.float64),
                                  tau, margin)


def oracle_term_scene(orc):
    """term_scene from the oracle's own vertices and tables (the CPU tests: no model, no device) -> (sc, alpha (NB) float64)."""
    with torch.no_grad():
        env = orc.build_env(True, False)
        blocks = orc.build_blocks(True, True, False)
        alpha = orc._alpha.double().numpy()
    nvb, nfb = orc.bkg_verts.shape[0], len(orc.bkg_faces)
    ground_v = env['verts'][nvb:]
    gf = env['faces'][nfb:] - nvb
    ngv, nv = ground_v.shape[0], blocks['verts'].shape[0] // NB
    faces = torch.cat([gf, blocks['faces'] + ngv], 0)
    face_group = torch.tensor([0, len(gf)] + [len(gf) + (k + 1) * orc.BNF for k in range(NB)])
    vert_group = torch.cat([torch.full((ngv,), -1), torch.arange(NB).repeat_interleave(nv)])
    group_alpha = torch.tensor([-1] + list(range(NB)))
    return term_scene(ground_v, blocks['verts'], faces, face_group, vert_group, group_alpha), alpha


# ---------------------------------------------------------------------------------------------------------------- discrete decisions
def discrete_decisions(orc, R1, T1, K1, dtype):
    """What the oracle decides per pixel and per face at the cameras (R1, T1, K1), evaluated in `dtype`: for the env pass and the fg pass,
    pix_to_face (N,H,W,K) and the number of vertices of every face behind the near plane (0 .. 3: its clip case) -> dict."""
    out = {}
    with torch.no_grad():
        scenes = {'env': (orc.build_env(True, False), 0.0, 1), 'fg': (orc.build_blocks(True, True, False), 1e-4, FPP)}
        R, T, K = R1.to(dtype), T1.to(dtype), K1.to(dtype)
        for name, (scene, sigma, k) in scenes.items():
            sc = dict(scene, verts=scene['verts'].to(dtype), face_uvs=scene['face_uvs'].to(dtype), maps=[m.to(dtype) for m in scene['maps']])
            _, frag = O.render(sc, R, T, K, (H, W), sigma, k, True, None, orc.z_clip, n_threads=8, return_fragments=True)
            ndc = O.transform_to_ndc(sc['verts'], R, T, K, eps=1e-8)
            behind = (ndc[:, sc['faces']][..., 2] < orc.z_clip).sum(-1)
            out[name] = dict(pix_to_face=frag['pix_to_face'], behind=behind)
    return out
