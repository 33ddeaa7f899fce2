"""CPU tests of the arithmetic of the 8-bit frame export (csrc/frame_math.h, the header frames_u8_kernel compiles) built for the host with
g++ -ffp-contract=off (tests/host_frame_math.cpp):
  * the quantisation reproduces tests/golden/frames_u8.npz -- the bytes the reference's convert_to_img makes of the same floats
    (tests/golden/make_export_golden.py) -- BIT FOR BIT, exact k/255 and their fp32 neighbours included;
  * the background composite and the edge blend equal torch's fp32 evaluation of rgb * alpha + (1 - alpha) * bkg and
    img * (1 - mask) + mask * colour BIT FOR BIT: every operation rounds once on both sides, in the same order, so there is no tolerance;
  * the whole per-pixel chain (both orders of the two blends, the input clamp, the (N,H,W,3) layout) equals the same chain of torch
    expressions followed by the quantisation."""
import os

import numpy as np
import pytest
import torch

import frame_ref as FR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'frames_u8.npz')


def test_quantisation_reproduces_the_reference_bytes():
    z = np.load(GOLDEN)
    tags = sorted(k[:-3] for k in z.files if k.endswith('_in'))
    assert {'rand0', 'rand1', 'grid', 'grid_t', 'special'} <= set(tags)
    for tag in tags:
        x, want = torch.from_numpy(z[f'{tag}_in']), torch.from_numpy(z[f'{tag}_u8'])
        got = FR.frames_u8_host(x[None])[0]
        assert torch.equal(got, want), tag
        assert torch.equal(FR.frames_u8_host(x.permute(1, 2, 0).contiguous()[None], hwc=True)[0], want), tag
        assert torch.equal(FR.quantise(x).permute(1, 2, 0), want), tag                  # (the torch restatement the GPU tests use)
    g = z['grid_u8'].reshape(-1, 3)                                                    # the fixture does hold the hard cases
    assert len(np.unique(g)) == 256


def test_special_values():
    x = torch.tensor([float('nan'), -0.0, 0.0, 1.0, float('inf'), -float('inf'), 1e-45, 0.99999994, 1.0000001, 0.5])
    img = x.view(1, 1, 1, -1).expand(1, 3, 1, -1).contiguous()
    assert FR.frames_u8_host(img)[0, 0, :, 0].tolist() == [0, 0, 0, 255, 255, 0, 0, 254, 255, 127]
    assert torch.equal(FR.quantise(img)[0].permute(1, 2, 0), FR.frames_u8_host(img)[0])


def _rand(shape, g, lo=-0.2, hi=1.2):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def test_composite_and_edge_blend_are_bit_equal_to_torch_fp32():
    g = torch.Generator().manual_seed(11)
    n = 200000
    rgb, alpha, bkg = _rand((n,), g), _rand((n,), g, -0.1, 1.1), _rand((n,), g, 0, 1)
    k = torch.randint(0, 256, (n,), generator=g).float() / 255
    alpha[::7], rgb[::5], bkg[::3] = k[::7], k[::5], k[::3]                            # exact k/255, 0 and 1 among them
    assert torch.equal(FR.composite_host(rgb, alpha, bkg), rgb * alpha + (1 - alpha) * bkg)
    img, mask, col = _rand((n,), g), torch.rand(n, generator=g), _rand((n,), g, 0, 1)
    mask[::4] = (torch.randint(0, 17, (n,), generator=g).float() / 16)[::4]            # the values a 4x4 pooled binary mask takes
    assert torch.equal(FR.edge_blend_host(img, mask, col), img * (1 - mask) + mask * col)


@pytest.mark.parametrize('H,W', [(12, 16), (18, 27)])
def test_the_pixel_chain_equals_the_torch_chain(H, W):
    g = torch.Generator().manual_seed(H * W)
    N = 3
    src = _rand((N, 4, H, W), g)
    src[:, 3] = torch.rand(N, H, W, generator=g)
    bkg_img, bkg3 = torch.rand(3, H, W, generator=g), [0.25, 1.0, 0.6]
    mask = (torch.randint(0, 17, (N, 1, H, W), generator=g).float() / 16) * (torch.rand(N, 1, H, W, generator=g) < 0.3)
    col3, col_img = [0.3, 0.3, 0.3], torch.rand(N, 3, H, W, generator=g)
    rgb, a = src[:, :3], src[:, 3:]
    assert torch.equal(FR.frames_u8_host(src), FR.quantise(rgb).permute(0, 2, 3, 1))
    assert torch.equal(FR.frames_u8_host(rgb.contiguous()), FR.quantise(rgb).permute(0, 2, 3, 1))
    for bkg, b in ((bkg_img, bkg_img[None]), (bkg3, torch.tensor(bkg3).view(1, 3, 1, 1))):
        comp = rgb * a + (1 - a) * b
        assert torch.equal(FR.frames_u8_host(src, bkg=bkg), FR.quantise(comp).permute(0, 2, 3, 1))
        for col, c in ((col3, torch.tensor(col3).view(1, 3, 1, 1)), (col_img, col_img)):
            after = comp * (1 - mask) + mask * c
            assert torch.equal(FR.frames_u8_host(src, bkg=bkg, mask=mask, edge_color=col), FR.quantise(after).permute(0, 2, 3, 1))
            first = (rgb * (1 - mask) + mask * c) * a + (1 - a) * b
            assert torch.equal(FR.frames_u8_host(src, bkg=bkg, mask=mask, edge_color=col, edge_first=True), FR.quantise(first).permute(0, 2, 3, 1))
    cl = src.clamp(0, 1)
    comp = cl[:, :3] * cl[:, 3:] + (1 - cl[:, 3:]) * bkg_img[None]
    assert torch.equal(FR.frames_u8_host(src, bkg=bkg_img, clamp_input=True), FR.quantise(comp).permute(0, 2, 3, 1))
    plain = rgb * (1 - mask) + mask * col_img
    assert torch.equal(FR.frames_u8_host(rgb.contiguous(), mask=mask, edge_color=col_img), FR.quantise(plain).permute(0, 2, 3, 1))
