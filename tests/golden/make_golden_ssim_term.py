"""
Generates tests/golden/ssim_term.npz: the reference's own SSIMLoss (src/model/loss.py:124-156, padding=True, its default) as a loss --
SSIMLoss()(img1, img2).mean() and its autograd gradient with respect to the second argument -- on
  * img1 / img2 of tests/golden/ssim.npz (3 x 3 x 40 x 52, noise): `value`, `grad`;
  * one pair of 2 x 3 x 19 x 37 with constant blocks, rec == target on image 0 (ssim_term_ref.pair(*BLOCKS)): `blocks_a`, `blocks_b`,
    `blocks_value`, `blocks_grad`.
The reference is imported the way make_golden.py imports it (read-only, stubs for the third-party packages it lacks), at generation time
only; the fixture is data (inputs + recorded results), no reference source travels.

Run where the reference is present:   python tests/golden/make_golden_ssim_term.py
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'differentiable-blocksworld_amd'))


def term(loss, a, b):
    b = b.clone().requires_grad_(True)
    v = loss.SSIMLoss()(a, b).mean()
    g, = torch.autograd.grad(v, b)
    return v.detach().numpy(), g.numpy()


def main():
    import make_golden
    from ssim_term_ref import BLOCKS, pair
    loss = make_golden.import_reference()['model.loss']
    pin = np.load(os.path.join(HERE, 'ssim.npz'))
    out = {}
    out['value'], out['grad'] = term(loss, torch.from_numpy(pin['img1']), torch.from_numpy(pin['img2']))
    a, b = pair(*BLOCKS)
    out['blocks_a'], out['blocks_b'] = a.numpy(), b.numpy()
    out['blocks_value'], out['blocks_grad'] = term(loss, a, b)
    path = os.path.join(HERE, 'ssim_term.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path)} bytes; value {out["value"]:.8f}, blocks {out["blocks_value"]:.8f}')


if __name__ == '__main__':
    main()
