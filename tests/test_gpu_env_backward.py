"""The hard single-layer pass's backward (sky dome + ground, K = 1, sigma = 0): the specialised kernel (lds_aggregate=True: hard
uv-fragments, several 8x8 tiles per wave) against the generic hard backward (lds_aggregate=False), texel and vertex gradients, at sizes
that are not multiples of the kernel's region, on views that see only sky, only ground or both, with full-resolution and decimated
(cell-resolution) maps, with and without constant sky geometry; and the conservation law of the texel scatter."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'differentiable-blocksworld_amd'))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'oracle'))
import oracle as O                                              # noqa: E402  (checker only)
from dbw_amd import ops                                         # noqa: E402
from dbw_amd.structures import PackedScene                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REL = 1e-5


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def _env(view, decimated, seed=7):
    """-> (PackedScene, number of sky faces) of the env scene; view 'sky' keeps the dome only."""
    m = O.OracleDBW((48, 64), n_blocks=2, txt_size=16, faces_per_pixel=1, seed=seed)
    with torch.no_grad():
        scene = m.build_env(True, False)
    nsky = int((scene['face_map'] == 0).sum())
    if view == 'sky':
        scene = dict(scene, faces=scene['faces'][:nsky], face_uvs=scene['face_uvs'][:nsky], face_map=scene['face_map'][:nsky])
    shapes = [tuple(mp.shape[:2]) for mp in scene['maps']]
    shift = 2 if decimated else 0
    g = torch.Generator().manual_seed(seed)
    maps = [torch.rand(h >> shift, w >> shift, 3, generator=g) for h, w in shapes]
    desc, _ = PackedScene.describe_maps(shapes, [(0, 0)] * len(shapes), DEV, shift=shift)
    flat = torch.cat([mp.reshape(-1) for mp in maps]).to(DEV)
    ps = PackedScene(scene['verts'].detach().to(DEV), scene['faces'].to(torch.int32).to(DEV), scene['face_uvs'].float().to(DEV),
                     scene['face_map'].to(torch.int32).to(DEV), desc, flat)
    return m, ps, nsky


def _cameras(m, view, n):
    if view == 'ground':             # looking steeply down with a narrow field of view
        return O.synthetic_cameras(n, R_world=m.R_world[0], dist=2.8, elev_deg=80.0, f_ndc=4.82)
    return O.synthetic_cameras(n, R_world=m.R_world[0], dist=2.8, elev_deg=5.0, f_ndc=1.5)     # horizon across the view


def _original_faces(ps, cams, H, W):
    """-> the original (local) face id of every pixel's fragment, -1 where it holds none"""
    R, T, Km = cams
    cfg = ops.RenderCfg(H, W, 1, 0.0, 0.001, True, False, ps.faces.shape[0])
    cl, p2f, _, _, _ = ops.render_fragments(ps.verts, ps.faces, R.to(DEV), T.to(DEV), Km[0].to(DEV), cfg)
    c2o = cl['c2o'].view(-1).long()
    p2f = p2f[..., 0].long()
    return torch.where(p2f >= 0, c2o[p2f.clamp(min=0)], torch.full_like(p2f, -1))


def _ground_verts(ps, nsky):
    m = torch.zeros(ps.verts.shape[0], dtype=torch.bool, device=DEV)
    m[ps.faces[nsky:].reshape(-1).long()] = True
    return m


def _grads(ps, cams, H, W, lds, const_faces=0, seed=5, signed=True):
    R, T, Km = cams
    maps = ps.maps.detach().clone().requires_grad_(True)
    verts = ps.verts.detach().clone().requires_grad_(True)
    cfg = ops.RenderCfg(H, W, 1, 0.0, 0.001, True, False, ps.faces.shape[0], lds_aggregate=lds, const_faces=const_faces)
    img = ops.render_scene(verts, maps, None, ps.faces, R.to(DEV), T.to(DEV), Km[0].to(DEV), ps.face_uvs, ps.face_map, ps.map_desc,
                           None, cfg)
    w = torch.rand(img.shape, generator=torch.Generator().manual_seed(seed)).to(DEV) - (0.5 if signed else 0.0)
    (img * w).sum().backward()
    return img.detach(), w, maps.grad, verts.grad


@pytest.mark.parametrize('decimated', [False, True])
@pytest.mark.parametrize('n', [1, 13])
@pytest.mark.parametrize('HW', [(300, 400), (75, 100), (37, 53)])
def test_specialised_env_backward_equals_generic(HW, n, decimated):
    m, ps, nsky = _env('mixed', decimated)
    cams = _cameras(m, 'mixed', n)
    faces = _original_faces(ps, cams, *HW)
    assert bool((faces >= nsky).any()) and bool(((faces >= 0) & (faces < nsky)).any())       # ground and sky on screen
    _, _, gm0, gv0 = _grads(ps, cams, *HW, lds=False)
    _, _, gm1, gv1 = _grads(ps, cams, *HW, lds=True)
    assert gm0.abs().max() > 0 and gv0[_ground_verts(ps, nsky)].abs().max() > 0       # (the ground's own geometry gradient, not the dome's)
    assert rel_err(gm1, gm0) < REL and rel_err(gv1, gv0) < REL


@pytest.mark.parametrize('const', [False, True])
@pytest.mark.parametrize('view', ['sky', 'ground', 'mixed'])
def test_specialised_env_backward_on_sky_ground_and_mixed_views(view, const):
    m, ps, nsky = _env(view, decimated=True, seed=11)
    cams = _cameras(m, view, 3)
    cf = nsky if const else 0
    faces = _original_faces(ps, cams, 75, 100)
    assert bool((faces >= 0).all())                          # every pixel holds a fragment of the env scene
    if view == 'ground':
        assert bool((faces >= nsky).all())
    elif view == 'sky':
        assert bool((faces < nsky).all())
    else:
        assert bool((faces >= nsky).any()) and bool((faces < nsky).any())
    img, _, gm0, gv0 = _grads(ps, cams, 75, 100, lds=False, const_faces=cf)
    _, _, gm1, gv1 = _grads(ps, cams, 75, 100, lds=True, const_faces=cf)
    assert img[:, 3].min() > 0.5                       # every pixel holds a fragment of the env scene
    assert rel_err(gm1, gm0) < REL
    if view == 'sky' and const:
        assert float(gv1.abs().max()) == 0.0 and float(gv0.abs().max()) == 0.0
    else:
        assert rel_err(gv1, gv0) < REL
    if view != 'sky':
        assert gv0[_ground_verts(ps, nsky)].abs().max() > 0


@pytest.mark.parametrize('decimated', [False, True])
def test_env_texel_gradients_conserve_the_image_gradient(decimated):
    """A hard K = 1 pixel has opacity 1 and its bilinear weights sum to 1: the texel gradients of channel c sum to the image gradient of c
    over the pixels that hold a fragment."""
    m, ps, _ = _env('mixed', decimated)
    cams = _cameras(m, 'mixed', 13)
    img, w, gm, _ = _grads(ps, cams, 300, 400, lds=True, signed=False)
    held = (img[:, 3:4] > 0.5).double()
    want = (w[:, :3].double() * held).sum((0, 2, 3))
    got = gm.view(-1, 3).double().sum(0)
    assert float(((got - want).abs() / want.abs().max()).max()) < 2e-4
