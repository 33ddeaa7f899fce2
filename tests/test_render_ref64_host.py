"""CPU: the preconditions of tests/test_gpu_render_ref64.py, for every case that file runs (tests/render_ref64.py holds the cases and the
rule).  They are conditions on the oracle alone, checked here so that a vacuous GPU test cannot hide:
  1. y = bars(oracle fp32, oracle fp64) <= 10 for every compared tensor (else 4 * y means nothing);
  2. the discrete decisions agree between fp32 and fp64: at most 2 % of a render's pixels are masked out of the upstream weight, and the
     clip bookkeeping (clipped_to_orig, has_conv) is equal outright;
  3. the operator-level raster cases are not vacuous: at least 40 % of the valid fragments lie inside their face, at least 20 % outside and
     carry a dists gradient (the K = 1, blur 0 shape has no outside fragment by construction: inside share 1), at most 1 % lose their
     bary / zbuf upstream to the amplification mask.
Plus the oracle's own pointer fix and the cause of the 1e5-sized fp32 gradients on fragments outside their face."""
import ctypes

import pytest
import torch

import oracle as O
import render_ref64 as R64


def _y_all(pairs):
    return {name: R64.yardstick(a, b) for name, (a, b) in pairs.items()}


@pytest.mark.parametrize('switches', R64.RASTER_SWITCHES)
@pytest.mark.parametrize('shape', R64.RASTER_SHAPES)
def test_raster_backward_cases_hold_their_preconditions(shape, switches, record_property):
    c = R64.raster_case(shape, switches)
    ys = _y_all({s: (c['o32'][s], c['o64'][s]) for s in R64.RASTER_STREAMS})
    for s, y in ys.items():
        record_property(f'y_{s}', round(y, 4))
    record_property('inside_share', round(c['inside_share'], 4))
    record_property('amp_masked', round(c['amp_masked'], 5))
    print(shape, switches, {s: round(y, 3) for s, y in ys.items()}, c['inside_share'], c['outside_share'], c['amp_masked'])
    assert max(ys.values()) <= R64.Y_CAP, ys
    for s in R64.RASTER_STREAMS:
        assert float(c['o64'][s].abs().max()) > 0, s
    assert c['inside_share'] >= R64.MIN_INSIDE
    if shape[4] > 0:
        assert c['outside_share'] >= R64.MIN_OUTSIDE
    else:
        assert c['inside_share'] == 1.0                       # blur 0: every fragment is inside its face
    assert c['amp_masked'] <= R64.MAX_AMP_MASKED
    # two images, the second mesh shorter: both are hit, and no fragment of image 1 names a face of mesh 0
    nf = shape[3]
    p2f = c['fwd'][0]
    assert (p2f[0] >= 0).any() and (p2f[1] >= 0).any() and int(p2f[0].max()) < nf <= int(p2f[1][p2f[1] >= 0].min()) and int(p2f[1].max()) < 2 * nf - 7


@pytest.mark.parametrize('persp', [True, False])
def test_project_clip_backward_case_holds_its_preconditions(persp, record_property):
    c = R64.project_clip_case(persp)
    a, b = c['o32']['cl'], c['o64']['cl']
    for key in ('clipped_to_orig', 'has_conv', 'num_faces', 'first_idx', 'neighbor'):
        assert torch.equal(a[key], b[key]), key
    assert (a['neighbor'] >= 0).any() and bool((a['has_conv'] & (a['neighbor'] < 0)).any()), 'cases 3 and 4 must both be present'
    assert int(a['num_faces'].min()) != int(a['num_faces'].max()), 'views must clip differently'
    y = R64.yardstick(c['o32']['grad'], c['o64']['grad'])
    record_property('y', round(y, 4))
    print('project_clip persp', persp, 'y', y)
    assert y <= R64.Y_CAP and float(c['o64']['grad'].abs().max()) > 0


@pytest.mark.parametrize('name,weight', [(n, 'all') for n in R64.RENDER_CASES] + [(n, w) for n in ('soft6', 'sigmoid6') for w in ('rgb', 'alpha')])
def test_render_cases_hold_their_preconditions(name, weight, record_property):
    res, ref = R64.render_three_ways(name, weight, hip=False)
    ys = _y_all({t: (v[1], v[2]) for t, v in res.items()})
    for t, y in ys.items():
        record_property(f'y_{t}', round(y, 4))
    record_property('masked', ref['masked'])
    print(name, weight, {t: round(y, 3) for t, y in ys.items()}, 'masked', ref['masked'])
    assert max(ys.values()) <= R64.Y_CAP, ys
    assert ref['masked'] <= R64.MAX_MASKED_PIXELS
    c = R64.render_case(name)
    assert set(res) == {'image', 'g_verts', 'g_maps'} | ({'g_alpha'} if c['faces_alpha'] is not None else set())
    assert float(res['g_verts'][2].abs().max()) > 0
    if weight != 'alpha':
        assert float(res['g_maps'][2].abs().max()) > 0
    else:
        assert float(res['g_maps'][2].abs().max()) == 0          # the opacity channel holds no colour: the kernels must leave exact zeros too
    if c['const_faces']:
        sky_only = torch.ones(c['scene']['verts'].shape[0], dtype=torch.bool)
        sky_only[c['scene']['faces'][c['const_faces']:].reshape(-1).long()] = False
        assert sky_only.any() and float(res['g_verts'][2][sky_only].abs().max()) == 0 and float(R64.render_refs('env_horizon')['o64']['g_verts'][sky_only].abs().max()) > 0


@pytest.mark.parametrize('variant,name', [(v, n) for v, names in R64.RENDER_VARIANTS.items() for n in names])
def test_render_variants_hold_their_preconditions(variant, name, record_property):
    """The 'bins' and 'decimated' variants of tests/test_gpu_render_ref64.py: the same preconditions with the map gradient in the form the
    variant stores its maps in, and what makes the variant more than the plain case -- footprints that wrap around the unpadded map, maps of
    several bins whose borders carry gradient, cells that are exactly the upsampled copy's."""
    res, ref = R64.render_three_ways(name, 'all', hip=False, variant=variant)
    ys = _y_all({t: (v[1], v[2]) for t, v in res.items()})
    for t, y in ys.items():
        record_property(f'y_{t}', round(y, 4))
    print(variant, name, {t: round(y, 3) for t, y in ys.items()}, 'masked', ref['masked'])
    assert max(ys.values()) <= R64.Y_CAP, ys
    assert ref['masked'] <= R64.MAX_MASKED_PIXELS
    c = R64.render_case(name)
    maps, shapes, pads, shift = R64.stored_maps(c, variant)
    g32, g64 = res['g_maps'][1], res['g_maps'][2]
    assert g64.dtype == torch.float64 and g64.numel() == g32.numel() == sum(m.numel() for m in maps) and float(g64.abs().max()) > 0
    assert abs(float(g64.sum()) - float(ref['o64']['g_maps'].sum())) <= 1e-9 * float(ref['o64']['g_maps'].abs().sum())    # nothing lost in the folding
    if variant == 'bins':
        assert shift == 0 and all(m.shape[:2] == s for m, s in zip(maps, shapes))
        if c['pads'] != (0, 0):
            # some footprints lie in the padding: the unpadded map sees them wrapped (the bins' atomic fallback)
            pl, pr = c['pads']
            at, in_pad = 0, 0.0
            for m in c['scene']['maps']:
                g = ref['o64']['g_maps'][at:at + m.numel()].reshape(m.shape)
                at += m.numel()
                in_pad += float(g[:, :pl].abs().sum() + g[:, m.shape[1] - pr:].abs().sum())
            assert in_pad > 0
        if name == 'soft6_ts64':
            g = g64.reshape(len(maps), 64, 64, 3)
            assert shapes[0] == (64, 64) and all(float(g[:, a:b, :].abs().sum()) > 0 and float(g[:, :, a:b].abs().sum()) > 0 for a, b in ((31, 32), (32, 33)))
    else:
        assert shift == R64.SHIFT and all(m.shape[0] << shift == s[0] and m.shape[1] << shift == s[1] for m, s in zip(maps, shapes))


@pytest.mark.parametrize('stream', [0, 1, 2])
def test_rasterize_bwd_raw_converts_fp32_upstream_for_fp64_faces(stream):
    """O.rasterize_bwd_raw used to pass data_ptr() of temporaries: with float64 face_verts and float32 upstream the three converted tensors
    were freed before the C call and shared one block (the zbuf stream came back exactly zero, the dists stream wrong).  Each stream alone:
    the call with float32 upstream equals the call with the upstream converted to doubles beforehand, and is not zero."""
    c = R64.raster_case(R64.RASTER_SHAPES[0], (True, True))
    fv, p2f = c['fv'].double(), c['fwd'][0]
    up = [torch.zeros_like(t) for t in c['up']['all']]
    up[stream] = c['up']['all'][stream]
    got = O.rasterize_bwd_raw(fv, p2f, *up)
    want = O.rasterize_bwd_raw(fv, p2f, *[t.double() for t in up])
    assert got.dtype == torch.float64 and float(want.abs().max()) > 0
    assert torch.equal(got, want)
    assert torch.equal(O.rasterize_bwd_raw(fv, p2f.to(torch.int32), *up), want)          # (and an index tensor that has to be converted)


def test_the_fp32_noise_on_outside_fragments_is_conditioning_of_the_clamped_perspective_denominator():
    """The fp32 oracle's gradient of face 52 of the first raster shape through zbuf and bary is ~1e5 where the fp64 one is ~10 (the unmasked
    upstream of test_rasterize_backward_matches_oracle).  On the fragment that carries it -- image 0, pixel (23, 49), layer 2, outside the
    face, in the blur band -- the fp64 analytic backward of the zbuf + bary streams agrees with fp64 central differences through
    dbw_ref_eval_pair_f64 (the tolerance of test_raster_backward_finite_difference_double), so the restated formula is right and the fp32 value
    is CONDITIONING.  The term: the pixel lies beyond the line on which the perspective denominator  t0 + t1 + t2  (t_i = w_i * z_j * z_k)
    vanishes, so persp_fwd clamps the denominator to kEpsilon = 1e-8 and the barycentrics before clipping are ~1e10; clip_fwd renormalises
    them, and being scale-invariant hands back a gradient that is orthogonal to them, so in persp_bwd
        g_denom = -(t0 g0 + t1 g1 + t2 g2) / denom^2
    is zero analytically; evaluated in floating point the sum leaves rounding of size eps * |t| * |g|, which 1 / denom^2 = 1e16 multiplies.
    In fp32 that is ~1e1 added to all three gt_i (against a true ~0.1), times z^2 / area ~ 1e3..1e4 in bary_bwd; in fp64 the same term leaves
    ~1e-4 absolute, which is what the finite differences below differ by.  (PyTorch3D's backward has the same term.)  Only fragments with
    the clamp active are affected: with either switch off, or inside a face (all t_i > 0), fp32 and fp64 agree."""
    shape = R64.RASTER_SHAPES[0]
    H, W = shape[:2]
    c = R64.raster_case(shape, (True, True))
    fv, (p2f, _, _, dists) = c['fv'], c['fwd']
    n, y, x, k, f = 0, 23, 49, 2, 52
    assert int(p2f[n, y, x, k]) == f and float(dists[n, y, x, k]) > 0
    ys, xs = R64.pixel_centres_f64(H, W)
    assert not bool(c['inside'][n, y, x, k])
    g = torch.Generator().manual_seed(3)
    gz, gb = torch.randn(p2f.shape, generator=g), torch.randn(p2f.shape + (3,), generator=g)           # (the unmasked upstream)
    one = torch.zeros(p2f.shape)
    one[n, y, x, k] = 1
    up = [gz * one, gb * one[..., None], torch.zeros(p2f.shape)]
    g32 = O.rasterize_bwd_raw(fv, p2f, *up)[f]
    g64 = O.rasterize_bwd_raw(fv.double(), p2f, *[t.double() for t in up])[f]
    lib = O.lib()
    face = fv[f].double()
    out5 = torch.zeros(5, dtype=torch.float64)

    def value(fx, clip=1):
        fx = fx.contiguous()
        lib.dbw_ref_eval_pair_f64(ctypes.c_void_p(fx.data_ptr()), ctypes.c_double(float(xs[x])), ctypes.c_double(float(ys[y])), 1, clip,
                                  ctypes.c_void_p(out5.data_ptr()))
        return float(out5[0] * gz[n, y, x, k].double() + (out5[1:4] * gb[n, y, x, k].double()).sum())
    # the clamp is active: barycentrics of ~1e9 before clipping (t_i / 1e-8 with t_i of order 10), O(1) and summing to one after it
    value(face, clip=0)
    assert float(out5[1:4].abs().max()) > 1e8
    value(face)
    assert float(out5[1:4].min()) == 0.0 and abs(float(out5[1:4].sum()) - 1) < 1e-12
    num = torch.zeros(9, dtype=torch.float64)
    h = 1e-6
    for i in range(9):
        d = torch.zeros(9, dtype=torch.float64)
        d[i] = h
        num[i] = (value(face + d.view(3, 3)) - value(face - d.view(3, 3))) / (2 * h)
    torch.testing.assert_close(g64, num.view(3, 3), rtol=1e-4, atol=1e-5)
    # ... and fp32 evaluates the same formula to noise: thousands of times the whole true gradient of the face
    assert float((g32.double() - g64).abs().max()) > 1e3 * float(g64.abs().max())
