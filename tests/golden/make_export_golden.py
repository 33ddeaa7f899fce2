"""
Generates tests/golden/frames_u8.npz by calling the REAL reference function utils/image.py:34-53 convert_to_img from
/root/reference/src (read-only, bytecode writing disabled) with the real PIL (plus an Image.ANTIALIAS shim: the constant left Pillow 10,
utils/image.py:22 names it in a default argument) and the stubs of make_golden.py for the other third-party packages.

Run here (the container that has /root/reference):   python tests/golden/make_export_golden.py
The fixture is data only: fp32 inputs and the bytes the reference makes of them.

Cases: `rand` (3,H,W) images spread over [-0.2, 1.2]; `grid` every exact k/255 in fp32 and its two fp32 neighbours (the values where a
multiply-truncate rule and any other rule part ways); `special` 0, -0, 1, values just outside [0, 1], denormals, +-inf.  NaN is left out:
numpy leaves that cast undefined, the project defines it as 0 (csrc/frame_math.h).
"""
import importlib
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG


def import_convert_to_img():
    MG.STUB_ROOTS.remove('PIL')
    from PIL import Image
    if not hasattr(Image, 'ANTIALIAS'):
        Image.ANTIALIAS = Image.LANCZOS
    sys.meta_path.insert(0, MG._Finder())
    sys.path.insert(0, MG.REF)
    return importlib.import_module('utils.image').convert_to_img


def main():
    convert_to_img = import_convert_to_img()
    g = torch.Generator().manual_seed(5150)
    out = {}

    def put(tag, img):              # img (3,H,W) fp32 -> (H,W,3) uint8 by the reference
        out[f'{tag}_in'] = img.numpy()
        out[f'{tag}_u8'] = np.asarray(convert_to_img(img))

    for i, (H, W) in enumerate([(24, 32), (18, 27), (5, 3)]):
        put(f'rand{i}', torch.rand(3, H, W, generator=g) * 1.4 - 0.2)
    k = torch.arange(256, dtype=torch.float32) / 255
    inf = torch.tensor(float('inf'))
    grid = torch.stack([torch.nextafter(k, -inf), k, torch.nextafter(k, inf)])            # (3,256)
    put('grid', grid.reshape(3, 16, 16).contiguous())
    put('grid_t', grid.t().reshape(256, 3).t().reshape(3, 16, 16).contiguous().flip(0))
    sp = torch.tensor([0.0, -0.0, 1.0, 1.0000001, -1e-30, 1e-45, 0.99999994, 0.5, 254.5 / 255, 255.5 / 255, 2.0, -3.0, float('inf'), -float('inf'),
                       0.003921568, 0.0039215689])
    put('special', torch.stack([sp, sp.flip(0), sp.roll(5)]).reshape(3, 4, 4).contiguous())
    for tag in ('rand0', 'grid', 'special'):        # the rule the issue states, checked where the fixture is made
        x = out[f'{tag}_in']
        want = (np.clip(x, 0, 1) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)
        assert np.array_equal(out[f'{tag}_u8'], want), tag
    path = os.path.join(HERE, 'frames_u8.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
