"""Checker side of the 8-bit frame export: csrc/frame_math.h built for the host with g++ (tests/host_frame_math.cpp) behind the arguments of
ops.frames_u8, and the quantisation rule restated with torch.  Used by tests/test_host_frame_math.py (against the reference's bytes) and
by tests/test_gpu_export.py (as the yardstick of the kernel)."""
import ctypes

import torch

from host_build import host_lib

HWC, EDGE_FIRST, CLAMP_INPUT = 1, 2, 4


def lib():
    return host_lib('frame_math')


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _f3(v):
    return None if v is None else (ctypes.c_float * 3)(*[float(x) for x in v])


def quantise(t):
    """clamp to [0, 1], times 255 in fp32, truncate (the reference's convert_to_img); NaN -> 0.  Any shape, fp32 -> uint8."""
    t = torch.nan_to_num(t.float(), nan=0.0)
    return (t.clamp(0, 1) * 255.0).to(torch.uint8)


def frames_u8_host(src, bkg=None, mask=None, edge_color=None, hwc=False, edge_first=False, clamp_input=False):
    """ops.frames_u8 on the CPU through the host build of frame_math.h: CPU tensors in, (N,H,W,3) uint8 out."""
    src = src.detach().cpu().float().contiguous()
    (N, H, W, C) = src.shape if hwc else (src.shape[0], src.shape[2], src.shape[3], src.shape[1])
    bkg3 = bkg_img = edge3 = edge_img = None
    if bkg is not None:
        if torch.is_tensor(bkg) and bkg.dim() == 3:
            bkg_img = bkg.detach().cpu().float().contiguous()
        else:
            bkg3 = _f3(torch.as_tensor(bkg).reshape(3).tolist())
    if mask is not None:
        mask = mask.detach().cpu().float().contiguous()
        if torch.is_tensor(edge_color) and edge_color.dim() == 4:
            edge_img = edge_color.detach().cpu().float().contiguous()
        else:
            edge3 = _f3(torch.as_tensor(edge_color).reshape(3).tolist())
    out = torch.empty(N, H, W, 3, dtype=torch.uint8)
    flags = (HWC if hwc else 0) | (EDGE_FIRST if edge_first else 0) | (CLAMP_INPUT if clamp_input else 0)
    rc = lib().host_frames_u8(_p(src), N, C, H, W, flags, bkg3, _p(bkg_img), _p(mask), edge3, _p(edge_img), _p(out))
    assert rc == 0
    return out


def composite_host(rgb, alpha, bkg):
    rgb, alpha, bkg = [t.float().contiguous() for t in torch.broadcast_tensors(rgb, alpha, bkg)]
    out = torch.empty_like(rgb)
    assert lib().host_composite(_p(rgb), _p(alpha), _p(bkg), ctypes.c_longlong(rgb.numel()), _p(out)) == 0
    return out


def edge_blend_host(img, mask, colour):
    img, mask, colour = [t.float().contiguous() for t in torch.broadcast_tensors(img, mask, colour)]
    out = torch.empty_like(img)
    assert lib().host_edge_blend(_p(img), _p(mask), _p(colour), ctypes.c_longlong(img.numel()), _p(out)) == 0
    return out
