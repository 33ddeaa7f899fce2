"""GPU tests of the image ingest: ops.resample_u8 (dbw_images_resample_u8, both kernel forms) against tests/golden/resample_pil.npz -- the
bytes Pillow makes -- and the scene loaders of dbw_amd/dataset.py against the reference's transform restated with PIL and torch on the
host.  `-m gpu`.

Bounds: none.  The resample is integer arithmetic behind a table that the host builds in double precision, and ToTensor is one IEEE fp32
division: bytes and floats are compared EXACTLY, with the fixture (written by Pillow 12.2.0) and, where PIL imports, with live Pillow."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dbw_amd                                                  # noqa: E402
import resample_ref as RR                                       # noqa: E402
from dbw_amd import dataset as DS                               # noqa: E402
from dbw_amd import ops                                         # noqa: E402

DEV = 'cuda:0'
FUSED_MAX_KSIZE = 11                                            # DBW_RESAMPLE_FUSED_MAX_KSIZE of include/dbw_ingest.h


@pytest.fixture(scope='module')
def golden():
    z = np.load(RR.GOLDEN)
    return {tag: z[tag] for tag in RR.SHAPES}


def _batch(tag, N):
    a = RR.make_input(tag)
    return np.stack([a, a[::-1, ::-1].copy(), 255 - a][:N])


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('tag', sorted(RR.SHAPES))
def test_resample_u8_equals_pillow_bit_for_bit(golden, tag, N):
    size = RR.SHAPES[tag][1]
    b = _batch(tag, N)
    f32, u8 = ops.resample_u8(torch.from_numpy(b).to(DEV), size, out='both')
    assert f32.shape == (N, 3, *size) and f32.dtype == torch.float32 and u8.shape == (N, *size, 3) and u8.dtype == torch.uint8 and u8.is_cuda
    u8, f32 = u8.cpu(), f32.cpu()
    n_diff = int((u8[0].numpy() != golden[tag]).sum())
    print(f'{tag} N={N}: {b.shape[1:3]} -> {size}: {n_diff} bytes differ from the fixture')
    assert n_diff == 0
    want = RR.resample_host(torch.from_numpy(b), size, out='u8')                # images 1, 2: the host build, itself held to Pillow on the CPU
    assert torch.equal(u8, want)
    assert torch.equal(f32.view(torch.int32), want.permute(0, 3, 1, 2).float().div(255).contiguous().view(torch.int32))
    # each output alone gives the same
    assert torch.equal(ops.resample_u8(torch.from_numpy(b).to(DEV), size, out='u8').cpu(), u8)
    assert torch.equal(ops.resample_u8(torch.from_numpy(b).to(DEV), size, out='f32').cpu(), f32)


@pytest.mark.parametrize('form', ['auto', 'fused', 'general'])
def test_a_sliced_source_and_a_width_that_is_no_multiple_of_4(golden, form):
    """Sources 1, 2 and 3 bytes off the 16-byte alignment (the dword copy starts at another byte of every row), Wout = 13, 17 and 65."""
    for tag in ('stripes', 'odd', 'tiles', 'up'):
        a = RR.make_input(tag)
        for shift in (1, 2, 3):
            flat = torch.zeros(a.size + shift, dtype=torch.uint8, device=DEV)
            flat[shift:] = torch.from_numpy(a).reshape(-1).to(DEV)
            src = flat[shift:].view(1, *a.shape)
            assert src.data_ptr() % 4 == shift
            got = ops.resample_u8(src, RR.SHAPES[tag][1], out='u8', form=form)
            assert np.array_equal(got[0].cpu().numpy(), golden[tag]), (tag, shift)


@pytest.mark.parametrize('tag', ['ratio4', 'tiles', 'up', 'x_only', 'y_only', 'identity'])
def test_the_two_forms_give_the_same_bytes(golden, tag):
    size = RR.SHAPES[tag][1]
    src = torch.from_numpy(_batch(tag, 2)).to(DEV)
    ff, fu = ops.resample_u8(src, size, out='both', form='fused')
    gf, gu = ops.resample_u8(src, size, out='both', form='general')
    assert torch.equal(fu, gu) and torch.equal(ff.view(torch.int32), gf.view(torch.int32))
    assert np.array_equal(fu[0].cpu().numpy(), golden[tag])


def test_a_ratio_beyond_the_fused_bound_takes_the_general_form(golden):
    (Hin, Win), size = RR.SHAPES['tall']                                        # 400 x 8 -> 3 x 8: 269 weights per row
    assert ops.resample_table(Hin, size[0]).shape[1] - 2 > FUSED_MAX_KSIZE
    src = torch.from_numpy(_batch('tall', 3)).to(DEV)
    with pytest.raises(RuntimeError, match='fused form'):
        ops.resample_u8(src, size, form='fused')
    auto, gen = ops.resample_u8(src, size, out='u8'), ops.resample_u8(src, size, out='u8', form='general')
    assert torch.equal(auto, gen) and np.array_equal(auto[0].cpu().numpy(), golden['tall'])
    assert torch.equal(auto.cpu(), RR.resample_host(src.cpu(), size, out='u8'))
    # both axes beyond it, through the intermediate
    b = np.random.RandomState(5).randint(0, 256, (2, 90, 70, 3)).astype(np.uint8)
    got = ops.resample_u8(torch.from_numpy(b).to(DEV), (7, 9), out='u8')
    assert torch.equal(got.cpu(), RR.resample_host(torch.from_numpy(b), (7, 9), out='u8'))


def test_empty_batch_and_errors():
    assert ops.resample_u8(torch.zeros(0, 8, 8, 3, dtype=torch.uint8, device=DEV), (4, 4)).shape == (0, 3, 4, 4)
    with pytest.raises(TypeError):
        ops.resample_u8(torch.zeros(1, 8, 8, 3, device=DEV), (4, 4))
    with pytest.raises(ValueError):
        ops.resample_u8(torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device=DEV), (4, 4))


# ---- the scene loaders -------------------------------------------------------------------------------------------------------------------
from dataset_fixture import write_scene                         # noqa: E402


@pytest.fixture(scope='module')
def scene_root(tmp_path_factory):
    root = tmp_path_factory.mktemp('data')
    return root, write_scene(root, 'DTU', 'scan24', n_views=6, H=48, W=64, with_points=True)


def _cfg(n_blocks=3, txt=16):
    return {'model': {'name': 'dbw', 'mesh': {'n_blocks': n_blocks, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': txt},
                      'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True,
                                     'opacity_noise': False},
                      'loss': {'rgb_weight': 1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}},
            'training': {'batch_size': 2, 'n_epoches': 1, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 1e-3}, 'scheduler': {'name': 'multi_step'}}}


def test_dtu_scene_views_equal_the_reference_transform(scene_root):
    root, raw = scene_root
    scene = DS.DTUScene(root, 'scan24', [12, 16], 'train')
    views = scene.views(DEV, keep_raw=True)
    assert set(views) == {'imgs', 'K', 'R', 'T', 'raw'} and all(v.is_cuda for v in views.values())
    want = torch.stack([RR.to_tensor(RR.pil_resize(a, (12, 16))) for a in raw])                 # ToTensor(Resize(PIL image)) on the host
    assert views['imgs'].shape == (6, 3, 12, 16) and torch.equal(views['imgs'].cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(views['raw'].cpu(), torch.from_numpy(np.stack(raw)))
    # another img_size from the resident raw frames: no second decode; chunked uploads change nothing
    again = ops.resample_u8(views['raw'], (24, 32))
    assert torch.equal(again.cpu(), torch.stack([RR.to_tensor(RR.pil_resize(a, (24, 32))) for a in raw]))
    assert torch.equal(DS.DTUScene(root, 'scan24', [12, 16], 'train').views(DEV, chunk=4)['imgs'], views['imgs'])
    # a shuffled split carries the same pictures in its own order
    test = DS.DTUScene(root, 'scan24', [12, 16], 'test')
    assert torch.equal(test.views(DEV)['imgs'].cpu(), want[test.view_ids]) and sorted(test.view_ids) == list(range(6))


def test_a_forward_and_one_epoch_on_the_loaded_scene(scene_root):
    from dbw_amd.trainer import Trainer
    root, raw = scene_root
    cfg = _cfg()
    scene = DS.DTUScene(root, 'scan24', [12, 16], 'train')
    torch.manual_seed(227391)
    model = dbw_amd.create_model(cfg, (12, 16)).to(DEV).train()
    loader = scene.loader(2, DEV)
    assert len(loader) == 3 and loader.batch_size == 2 and loader.dataset is scene
    inp, labels = next(iter(loader))
    assert inp['imgs'].shape == (2, 3, 12, 16) and labels['points'].shape[0] == 2 and labels['points'].shape[2] == 3
    out = model(inp, labels)
    assert all(bool(torch.isfinite(v).all()) for v in out.values()) and float(out['total'].detach()) > 0
    model.zero_grad(set_to_none=True)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    tr = Trainer(cfg, model, scene.views(DEV))
    last = tr.run()
    torch.cuda.synchronize()
    assert tr.epoch == 2 and tr.n_iters == 3 and all(np.isfinite(float(v)) for v in last.values())
    moved = [k for k, v in model.named_parameters() if not torch.equal(v.detach(), before[k])]
    print('moved:', moved)
    assert len(moved) >= 3, moved                              # geometry, opacity and texture tensors all take a step
