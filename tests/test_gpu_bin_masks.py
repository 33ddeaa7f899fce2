"""GPU: the cell masks of a bin's list entries (csrc/raster_bin.h: cell_bin_block).  A chunk of at most 8 / 16 / 32 entries spreads the
cell rows of an entry over 8 / 4 / 2 lanes and ORs the parts back together; a longer chunk keeps one lane per entry.  The per-tile lists
that come out must be the ones a tile finds by walking its coarse bin itself (dbw_debug_set_flags 4096: no per-tile lists), so the
rasteriser's output is compared bit for bit between the two, for list lengths on both sides of every threshold, a second chunk that is
short behind a full one, and two views of different lengths in one pass.  `-m gpu`."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dbw_amd import _lib, ops                                   # noqa: E402

DEV = 'cuda:0'
H, W, K = 72, 88, 4                                             # 2 x 2 bins, the last ones cut by the image; no multiple of 8 either
BLUR = math.log(1e4 - 1) * 1e-4


def _faces(n, seed, size):
    """n faces around the image centre, large enough to reach every bin and most of their cells"""
    g = torch.Generator().manual_seed(seed)
    c = (torch.rand(n, 1, 2, generator=g) * 2 - 1) * 0.5
    xy = c + (torch.rand(n, 3, 2, generator=g) * 2 - 1) * size
    z = torch.rand(n, 3, 1, generator=g) * 4.5 + 0.5
    return torch.cat([xy, z], -1)


def _raster(fv, first, num, flags):
    lib = _lib.load()
    lib.dbw_debug_set_flags(flags)
    try:
        out = ops._raster_fwd(fv, first, num, None, first.numel(), H, W, K, BLUR, True, True, False)
        torch.cuda.synchronize()
    finally:
        lib.dbw_debug_set_flags(0)
    return out


@pytest.mark.parametrize('counts', [(6, 8), (9, 14), (16, 17), (28, 32), (33, 50), (64, 70), (135, 3)])
@pytest.mark.parametrize('size', [0.9, 0.25])
def test_per_tile_lists_from_spread_cell_masks_equal_the_walk_of_the_coarse_bin(counts, size):
    fv = torch.cat([_faces(n, 11 * n + i, size) for i, n in enumerate(counts)]).contiguous().to(DEV)
    num = torch.tensor(counts, dtype=torch.int32, device=DEV)
    first = torch.tensor([0, counts[0]], dtype=torch.int32, device=DEV)
    lists = _raster(fv, first, num, 0)
    walk = _raster(fv, first, num, 4096)
    assert torch.equal(lists[0], walk[0]), f'pix_to_face differs on {(lists[0] != walk[0]).sum().item()} slots'
    for name, a, b in zip(('zbuf', 'bary', 'dists'), lists[1:], walk[1:]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    for n in range(2):                                          # (the case has fragments in both views)
        assert bool((lists[0][n, :, :, 0] >= 0).any())
