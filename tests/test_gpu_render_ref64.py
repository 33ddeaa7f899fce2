"""GPU: the render backward -- raster_bwd_kernel, project_clip_bwd_kernel, and the fused render_bwd_uv_kernel / render_bwd_hard_kernel /
shade_blend_bwd_kernel -- against the FLOAT64 oracle, element by element.  tests/test_gpu_parity.py holds these kernels to the fp32 oracle
in one max-norm per tensor; here every entry is held to the bar of tests/test_gpu_golden.py in units of what fp32 itself can do:

    bars(a, b) = max_i |a_i - b_i| / (1e-4 * |b_i| + 1e-6 * max|b|)        y = bars(oracle fp32, oracle fp64)      k = bars(hip, oracle fp64)
    assert k <= max(1, 4 * y)

(tests/render_ref64.py: the rule, the cases and their references, computed once per process; tests/test_render_ref64_host.py: the
preconditions -- y <= 10, equal discrete decisions, non-vacuity -- checked on the CPU for every case below; DESIGN.md "Render backward
against a float64 oracle": the measured table.)  Every case records its y and k (record_property)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import render_ref64 as R64                                      # noqa: E402
from dbw_amd import ops                                         # noqa: E402

DEV = 'cuda:0'


# ---------------------------------------------------------------------------------------------------------------------
# rasteriser backward, operator level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stream', R64.RASTER_STREAMS)
@pytest.mark.parametrize('switches', R64.RASTER_SWITCHES, ids=lambda s: f'persp{int(s[0])}_clip{int(s[1])}')
@pytest.mark.parametrize('shape', R64.RASTER_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}_K{s[2]}_F{s[3]}')
def test_rasterize_backward_equals_float64(shape, switches, stream, record_property):
    """dbw_rasterize_bwd on two packed meshes of different sizes: ragged images, K in {1, 5, 16, 25}, soft and hard, every
    perspective_correct x clip_barycentric combination; all three gradient streams through `rasterize_meshes_backward`, and each alone
    through autograd with the other two ABSENT (NULL pointers).  pix_to_face comes from the HIP forward and equals the fp32 oracle's;
    the reference is the oracle's backward on doubles with that selection.  Upstream: R64.raster_case (bary / zbuf upstream only where the
    barycentrics are well conditioned; dists everywhere)."""
    H, W, K, nf, blur, _ = shape
    persp, clipb = switches
    c = R64.raster_case(shape, switches)
    fvd = c['fv'].to(DEV).requires_grad_(True)
    out = ops.rasterize_meshes(fvd, c['first'].to(DEV), c['num'].to(DEV), None, (H, W), blur, K, 0, 0, persp, clipb, False)
    assert torch.equal(out[0].cpu(), c['fwd'][0])
    gz, gb, gd = [t.to(DEV) for t in c['up']['all']]
    if stream == 'all':
        grad = ops.rasterize_meshes_backward(fvd, out[0], gz, gb, gd, persp, clipb)
    else:
        sel = {'z': 0, 'bary': 1, 'dists': 2}[stream]
        (out[1 + sel] * (gz, gb, gd)[sel]).sum().backward()
        grad = fvd.grad
    assert grad.shape == c['fv'].shape
    R64.assert_within(grad, c['o32'][stream], c['o64'][stream], stream, record_property)


# ---------------------------------------------------------------------------------------------------------------------
# projection + z clipping backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extra', [0, 5000], ids=['lds_table', 'global_atomics'])
@pytest.mark.parametrize('persp', [True, False])
def test_project_clip_backward_equals_float64_autograd(persp, extra, record_property):
    """dbw_project_clip_bwd, vertex gradients, against fp64 autograd through O.transform_to_ndc and O.clip_faces: seven views that clip
    differently (cases 3 and 4 present), with and without perspective-correct clipping; the mesh as is (at most 4096 vertices: LDS table)
    and with 5000 unused vertices appended (accumulation straight into memory), whose rows must stay exactly 0.  The forward's slot
    bookkeeping equals the oracle's first."""
    c = R64.project_clip_case(persp)
    verts, faces, ref = c['verts'], c['faces'], c['o32']['cl']
    B, Fs, nv = c['R'].shape[0], faces.shape[0], verts.shape[0]
    fi = faces.to(torch.int32).to(DEV)
    args = (c['R'].to(DEV), c['T'].to(DEV), c['Kmat'].to(DEV))
    v = torch.cat([verts, torch.randn(extra, 3, generator=torch.Generator().manual_seed(2))]).to(DEV)
    cl = ops.project_clip(v, fi, *args, 1e-8, R64.Z_CLIP, persp)
    num = cl['num_faces'].cpu().long()
    assert torch.equal(num, ref['num_faces'])
    for b in range(B):
        n, s = int(num[b]), int(ref['first_idx'][b])
        assert torch.equal(cl['c2o'][b, :n].cpu().long(), ref['clipped_to_orig'][s:s + n] - b * Fs)
        assert torch.equal(cl['clip_code'][b, :n].cpu() >= 0, ref['has_conv'][s:s + n])
        nb_ref = ref['neighbor'][s:s + n]
        assert torch.equal(cl['neighbor'][b, :n].cpu().long(), torch.where(nb_ref >= 0, nb_ref - s + b * 2 * Fs, nb_ref))
    grad = ops.project_clip_bwd(v, fi, *args, cl, c['g'].to(DEV), 1e-8, R64.Z_CLIP, persp).clone()
    assert grad.shape == v.shape
    if extra:
        assert float(grad[nv:].abs().max()) == 0.0
    R64.assert_within(grad[:nv], c['o32']['grad'], c['o64']['grad'], 'g_verts', record_property)


# ---------------------------------------------------------------------------------------------------------------------
# full passes: image, g_verts, g_maps, g_alpha
# ---------------------------------------------------------------------------------------------------------------------
VARIANTS = [(True, False), (True, True), (False, False)]        # (ops.FUSED_FORWARD = ops.FUSED_BACKWARD, lds_aggregate): what test_gpu_parity.py runs


def _render_params():
    out = []
    for name in R64.PLAIN_CASES:
        for fused, lds in VARIANTS:
            if name == 'const_faces' and not fused:             # const_faces is a switch of the fused hard backward kernels
                continue
            out.append((name, 'all', fused, lds, 'plain'))
    for name in ('soft6', 'sigmoid6'):                            # the colour and the opacity branch of the blend backward, each alone
        for weight in ('rgb', 'alpha'):
            out += [(name, weight, fused, lds, 'plain') for fused, lds in VARIANTS]
    # the texel-gradient accumulators as the training phases use them (R64.RENDER_VARIANTS; fused kernels only): full-resolution maps through
    # the texture-space bins, decimated maps through the LDS table and through the wave-aggregated atomics
    out += [(name, 'all', True, False, 'bins') for name in R64.RENDER_VARIANTS['bins']]
    out += [(name, 'all', True, lds, 'decimated') for name in R64.RENDER_VARIANTS['decimated'] for lds in (True, False)]
    return [pytest.param(*p, id='-'.join(str(v) for v in (p if p[4] != 'plain' else p[:4]))) for p in out]


@pytest.mark.parametrize('name,weight,fused,lds,variant', _render_params())
def test_render_pass_equals_float64(name, weight, fused, lds, variant, monkeypatch, record_property):
    """project -> clip -> raster -> shade -> blend and back at 48x64 (and 45x61, no multiple of a tile), three views: the soft block pass for
    every compiled faces_per_pixel bucket, the fine pass (sigma 5e-6, no opacities), the hard environment pass in both rigs (attached
    barycentrics, z clipping live), the sigmoid opacity of clip_inside=False with detached barycentrics, and const_faces; fused kernels on
    uv-fragments / hard uv-fragments, with LDS aggregation and with atomics, and the operator-level kernels.  The upstream weight is
    zero on pixels where the fp32 and the fp64 oracle decide differently (none at these sizes; at most 2 %, host test).
    Variants 'bins' and 'decimated': the same bar on the texel paths of a training step -- unpadded 32x32 and 64x64 maps through the
    texture-space bins (records + dbw_texbin_reduce; wrapped footprints through the atomic fallback), cell-resolution maps with shift 2
    through LdsAgg and through the wave-aggregated atomics; the float64 gradient of a cell is the oracle's summed over the cell."""
    monkeypatch.setattr(ops, 'FUSED_FORWARD', fused)
    monkeypatch.setattr(ops, 'FUSED_BACKWARD', fused)
    res, ref = R64.render_three_ways(name, weight, lds=lds, variant=variant)
    assert 'g_verts' in res and 'g_maps' in res
    failed = []
    for t, (hip, o32, o64) in res.items():
        assert hip is not None and hip.shape == o64.shape, t
        try:
            R64.assert_within(hip, o32, o64, t, record_property)
        except AssertionError as e:                              # (every tensor is measured and recorded before the test fails)
            failed.append(str(e))
    assert not failed, '; '.join(failed)
