"""CPU tests of the scene ingest's host side (dbw_amd/dataset.py, dbw_amd/train.py) on a synthetic scene written into tmp_path
(tests/dataset_fixture.py): file discovery, the splits of both dataset kinds against orders written down from the reference's rule
(np.random.seed(len(split + tag)), then shuffle; dtu.py:38-40, bmvs.py:41-47), the cameras, the ground-truth points, the loaders, the
config merge on copies of the reference's configs/dtu/{default,scan24}.yml (tests/golden/configs/dtu, settings only), and the command
line's refusal of a perceptual weight without weights.  ops.resample_u8 has no CPU path: a stand-in built on the host build of the same
header (tests/resample_ref.py) takes its place here; tests/test_gpu_ingest.py runs the real one."""
import os

import numpy as np
import pytest
import torch

import resample_ref as RR
from dataset_fixture import SCALE, write_scene
from dbw_amd import dataset as DS
from dbw_amd import ops, train
from dbw_amd.cameras import load_idr_cameras

CONFIGS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'configs', 'dtu')


@pytest.fixture()
def host_resample(monkeypatch):
    calls = []

    def stand_in(src_u8, size, out='f32', form='auto'):
        calls.append(tuple(src_u8.shape))
        return RR.resample_host(src_u8, size, out=out)
    monkeypatch.setattr(ops, 'resample_u8', stand_in)
    return calls


@pytest.fixture()
def root(tmp_path):
    frames = {'dtu': write_scene(tmp_path, 'DTU', 'scan24'), 'bmvs': write_scene(tmp_path, 'BlendedMVS', 'dog', n_views=12, seed=5)}
    return tmp_path, frames


def test_file_discovery_is_recursive_sorted_and_filtered(root):
    path, _ = root
    files = DS.get_files_from(path / 'DTU' / 'scan24' / 'image')
    rel = [os.path.relpath(f, path / 'DTU' / 'scan24' / 'image') for f in files]
    assert rel == [f'{i:06d}.png' for i in range(5)] + [os.path.join('sub', '000000.png')] and all(f.is_absolute() for f in files)
    assert DS.get_files_from(path / 'DTU' / 'scan24' / 'image', recursive=False) == files[:5]
    assert DS.IMG_EXTENSIONS == ['jpeg', 'jpg', 'JPG', 'png', 'ppm', 'JPEG']
    with pytest.raises(FileNotFoundError):
        DS.get_files_from(path / 'DTU' / 'scan99' / 'image')


def test_dtu_splits_follow_the_reference_rule(root):
    path, _ = root
    mk = lambda split, **kw: DS.DTUScene(path, 'scan24', [6, 8], split, **kw)
    assert DS.DTUScene.raw_img_size == (1200, 1600) and DS.DTUScene.name == 'dtu'
    assert mk('train').view_ids == [0, 1, 2, 3, 4, 5] and len(mk('train')) == 6
    assert mk('val').view_ids == [5, 1, 2, 3, 0, 4]                     # np.random.seed(len('valscan24') = 9); shuffle(range(6))
    assert mk('test').view_ids == [2, 5, 0, 3, 4, 1]                    # seed len('testscan24') = 10
    # view_ids: kept by train, shuffled by val, ignored by test (dtu.py:33-34)
    ids = [0, 2, 4, 5]
    assert mk('train', view_ids=ids).view_ids == ids and mk('val', view_ids=ids).view_ids == [2, 5, 0, 4] and ids == [0, 2, 4, 5]
    assert mk('test', view_ids=ids).view_ids == [2, 5, 0, 3, 4, 1] and len(mk('val', view_ids=ids)) == 4
    assert mk('train', view_ids=ids).img_size == (6, 8) and DS.DTUScene(path, 'scan24', 8, 'train').img_size == (8, 8)
    state = np.random.get_state()[1].copy()
    mk('test')
    assert np.array_equal(np.random.get_state()[1], state)              # use_seed puts the global generator back: it is never touched here


def test_bmvs_splits_follow_the_reference_rule(root):
    path, _ = root
    mk = lambda split, **kw: DS.BMVSScene(path, 'dog', [6, 8], split, **kw)
    assert DS.BMVSScene.raw_img_size == (576, 768) and DS.BMVSScene.name == 'bmvs'
    assert [len(mk(s)) for s in ('train', 'val', 'test')] == [12, 5, 10]                       # bmvs.py:41-47
    assert all(mk(s).view_ids == list(range(12)) for s in ('train', 'val', 'test'))            # no shuffling
    assert mk('val').ids() == [0, 1, 2, 3, 4] and mk('test').ids() == list(range(10))
    ids = [7, 3, 9]
    assert [len(mk(s, view_ids=ids)) for s in ('train', 'val', 'test')] == [3, 3, 3] and mk('test', view_ids=ids).ids() == ids
    assert torch.equal(mk('train').pc_gt, torch.zeros(1, 3))


def test_cameras_and_ground_truth_points(root):
    path, _ = root
    scene = DS.DTUScene(path, 'scan24', [6, 8], 'train')
    cams = load_idr_cameras(str(path / 'DTU' / 'scan24' / 'cameras.npz'), (1200, 1600))
    for k in ('K', 'R', 'T'):
        assert torch.equal(getattr(scene, k), cams[k]) and len(cams[k]) == 6
    assert torch.equal(scene.scale_mat, cams['scale_mat']) and np.allclose(scene.scale_mat.numpy(), SCALE)
    # the points of the PLY, brought into the normalised frame as dtu.py:46-50 does
    from dbw_amd.eval3d import read_ply_points
    pts = torch.from_numpy(read_ply_points(path / 'DTU' / 'Points' / 'stl' / 'stl024_total.ply')).float()
    inv = scene.scale_mat.inverse()
    assert scene.pc_gt.shape == (40, 3) and torch.equal(scene.pc_gt, pts @ inv[:3, :3] + inv[:3, 3])
    assert float(scene.pc_gt.abs().max()) < 2                          # 100 mm around the centre, over 350
    # without the file: a (1,3) zero tensor, like BlendedMVS
    write_scene(path, 'DTU', 'scan105', with_points=False)
    other = DS.DTUScene(path, 'scan105', [6, 8], 'test')
    assert torch.equal(other.pc_gt, torch.zeros(1, 3)) and other.view_ids == [4, 2, 5, 3, 0, 1]       # seed len('testscan105') = 11


def test_views_and_loader_on_the_host_stand_in(root, host_resample):
    path, frames = root
    scene = DS.DTUScene(path, 'scan24', [6, 8], 'val')
    views = scene.views('cpu', keep_raw=True)
    want = torch.stack([RR.to_tensor(RR.pil_resize(a, (6, 8))) for a in frames['dtu']])
    order = scene.view_ids
    assert torch.equal(views['imgs'], want[order]) and torch.equal(views['raw'], torch.from_numpy(np.stack(frames['dtu']))[order])
    for k in ('K', 'R', 'T'):
        assert torch.equal(views[k], getattr(scene, k)[order])
    assert host_resample == [(6, 24, 32, 3)]                             # one launch for the chunk
    scene.views('cpu')
    assert len(host_resample) == 1                                       # resident: no second decode
    loader = scene.loader(4, 'cpu')
    assert len(loader) == 2 and loader.batch_size == 4 and loader.dataset is scene and hasattr(loader.dataset, 'pc_gt')
    for _ in range(2):                                                   # re-walkable
        batches = list(loader)
        assert [b[0]['imgs'].shape[0] for b in batches] == [4, 2]
        assert torch.equal(torch.cat([b[0]['imgs'] for b in batches]), views['imgs'])
        assert torch.equal(torch.cat([b[0]['T'] for b in batches]), views['T'])
        assert batches[0][1]['points'].shape == (4, 40, 3) and set(batches[0][0]) == {'imgs', 'K', 'R', 'T'}
        p = batches[1][1]['points'][0]                                   # a draw without replacement of the scene's points
        assert torch.equal(p[p[:, 0].argsort()], scene.pc_gt[scene.pc_gt[:, 0].argsort()])
    # small chunks, only the views asked for
    few = DS.BMVSScene(path, 'dog', [6, 8], 'val')
    v = few.views('cpu', chunk=2)
    assert host_resample[1:] == [(2, 24, 32, 3), (2, 24, 32, 3), (1, 24, 32, 3)]
    assert torch.equal(v['imgs'], torch.stack([RR.to_tensor(RR.pil_resize(a, (6, 8))) for a in frames['bmvs'][:5]]))
    assert list(few.loader(2, 'cpu'))[0][1]['points'].shape == (2, 1, 3)


def test_create_train_val_test_shares_one_store(root, host_resample):
    path, frames = root
    cfg = {'dataset': {'name': 'dtu', 'tag': 'scan24', 'img_size': [6, 8]}, 'training': {'batch_size': 4}}
    tr, va, te = DS.create_train_val_test(cfg, path, 'cpu')
    assert cfg['dataset'] == {'name': 'dtu', 'tag': 'scan24', 'img_size': [6, 8]}
    assert (tr.split, va.split, te.split) == ('train', 'val', 'test') and tr.store is va.store is te.store
    assert len(host_resample) == 1
    a, b = tr.views('cpu')['imgs'], te.views('cpu')['imgs']
    assert len(host_resample) == 1 and torch.equal(b, a[te.view_ids])
    with pytest.raises(NotImplementedError, match='nerfstudio'):
        DS.create_train_val_test({'dataset': {'name': 'nerfstudio', 'tag': 'x', 'img_size': 8}}, path)
    other = DS.DTUScene(path, 'scan24', [12, 16], 'val')
    with pytest.raises(ValueError, match='store'):
        DS.DTUScene(path, 'scan24', [6, 8], 'val', store=other.store)


def test_load_config_merges_like_the_reference(tmp_path):
    cfg = DS.load_config(os.path.join(CONFIGS, 'scan24.yml'))
    assert cfg['dataset'] == {'name': 'dtu', 'tag': 'scan24', 'img_size': [300, 400]}
    assert cfg['model']['mesh'] == {'n_blocks': 10, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 256}
    assert cfg['model']['loss']['perceptual_weight'] == 0.1 and cfg['training']['optimizer'] == {'name': 'adam', 'lr': 5.0e-3, 'texture': {'lr': 5.0e-2}}
    assert cfg['training']['n_epoches'] == 1800 and cfg['training']['seed'] == 227391 and cfg['training']['resume'] is None
    assert list(cfg) == ['model', 'training', 'dataset']                 # the defaults first, then what the file adds
    # a recursive update: a nested key replaces its leaf only; an explicit default file wins over the one next to the config
    (tmp_path / 'default.yml').write_text('model:\n  mesh:\n    n_blocks: 3\n    txt_size: 8\ntraining:\n  seed: 1\n')
    (tmp_path / 'run.yml').write_text('model:\n  mesh:\n    n_blocks: 5\n  loss:\n    rgb_weight: 2\ndataset:\n  name: bmvs\n')
    got = DS.load_config(tmp_path / 'run.yml')
    assert got == {'model': {'mesh': {'n_blocks': 5, 'txt_size': 8}, 'loss': {'rgb_weight': 2}}, 'training': {'seed': 1}, 'dataset': {'name': 'bmvs'}}
    got = DS.load_config(tmp_path / 'run.yml', os.path.join(CONFIGS, 'default.yml'))
    assert got['model']['mesh']['n_blocks'] == 5 and got['model']['mesh']['txt_size'] == 256 and got['training']['seed'] == 227391
    os.makedirs(tmp_path / 'alone')
    (tmp_path / 'alone' / 'run.yml').write_text('dataset:\n  name: dtu\n')
    assert DS.load_config(tmp_path / 'alone' / 'run.yml') == {'dataset': {'name': 'dtu'}}
    with pytest.raises(FileNotFoundError):
        DS.load_config(tmp_path / 'missing.yml')
    with pytest.raises(FileNotFoundError):
        DS.load_config(tmp_path / 'run.yml', tmp_path / 'missing.yml')


def test_the_command_line_refuses_a_perceptual_weight_without_weights(tmp_path, capsys):
    base = ['--config', os.path.join(CONFIGS, 'scan24.yml'), '--tag', 't', '--data-root', str(tmp_path), '--runs-root', str(tmp_path / 'runs')]
    with pytest.raises(SystemExit) as e:
        train.main(base)
    assert 'perceptual_weight = 0.1' in str(e.value) and '--lpips-vgg' in str(e.value) and '--no-perceptual' in str(e.value)
    with pytest.raises(SystemExit):                                      # one of the two files is not enough
        train.main(base + ['--lpips-vgg', 'vgg.pth'])
    assert not (tmp_path / 'runs').exists()                              # refused before anything is written
    cfg = train.prepare_config(train.parse_args(base + ['--no-perceptual', '--epochs', '7']))
    assert cfg['model']['loss']['perceptual_weight'] == 0 and cfg['training']['n_epoches'] == 7
    assert 'perceptual_weight 0.1 -> 0' in capsys.readouterr().out
    cfg = train.prepare_config(train.parse_args(base + ['--lpips-vgg', 'a', '--lpips-lin', 'b']))
    assert cfg['model']['loss']['perceptual_weight'] == 0.1 and cfg['training']['n_epoches'] == 1800
