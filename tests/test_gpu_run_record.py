"""GPU tests of the run record (dbw_amd/runlog.py) on a real Trainer: the geometry of
tests/test_gpu_model.py::test_trainer_driver_optimises_schedules_and_checkpoints -- 8 training views of 48 x 64, 4 blocks, batch 4 (two
batches per epoch), 6 epochs: iterations 1 .. 12 -- with 2 held-out views behind a loader of batch size 1, train_stat_interval 3,
val_stat_interval 4, save_epoches [2].  Train rows at 3 = (2,1), 6 = (3,2), 9 = (5,1), 12 = (6,2); val rows, image logs and model.pkl at
4 = (2,2), 8 = (4,2), 12 = (6,2).  One uninterrupted recorded run is made once and shared."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

import oracle as O                                              # noqa: E402  (checker only)
import dbw_amd                                                  # noqa: E402
from dbw_amd import runlog                                      # noqa: E402
from dbw_amd.trainer import Trainer                             # noqa: E402
from trajectory import assert_same_trajectory                   # noqa: E402

DEV = 'cuda:0'
H, W, V, NVAL = 48, 64, 8, 2


class Stopped(Exception):
    pass


class Recorder(runlog.RunRecorder):
    """Counts the meter's host reads and stops the run where told."""
    stop_at = None

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.trace, self.reads = [], []
        inner = self.meter.read_reset
        self.meter.read_reset = lambda: (self.reads.append(self.cur_iter), inner())[1]

    def after_step(self, epoch, batch, losses, view_ids):
        super().after_step(epoch, batch, losses, view_ids)
        if self.stop_at == (epoch, batch):
            raise Stopped


class HeldOut:
    """A loader of batch size 1 over the held-out views that counts how often it is walked."""

    def __init__(self, batches):
        self.batches, self.walks = batches, 0

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        self.walks += 1
        return iter(self.batches)


def _cfg(val_interval=4):
    return {'model': {'name': 'dbw', 'mesh': {'n_blocks': 4, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 32},
                      'renderer': {'faces_per_pixel': 6, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'decimate_factor': 8, 'kill_blocks': True,
                                     'decouple_rendering': True, 'opacity_noise': False},
                      'loss': {'rgb_weight': 1, 'perceptual_weight': 0, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}},
            'training': {'batch_size': 4, 'n_epoches': 6, 'seed': 123,
                         'optimizer': {'name': 'adam', 'lr': 5.0e-3, 'texture': {'lr': 5.0e-2}},
                         'scheduler': {'name': 'multi_step', 'gamma': [0.1, 0.1], 'milestones': [4]},
                         'train_stat_interval': 3, 'val_stat_interval': val_interval, 'save_epoches': [2], 'resume': None, 'pretrained': None}}


@pytest.fixture(scope='module')
def scene():
    """The training views, the loader of the held-out ones, rendered from a target model."""
    torch.manual_seed(5)
    target = dbw_amd.create_model(_cfg(), (H, W)).to(DEV).eval()
    R, T, Km = O.synthetic_cameras(V + NVAL, R_world=target.R_world[0].cpu())
    views = {k: v.to(DEV) for k, v in dict(imgs=torch.zeros(V + NVAL, 3, H, W), R=R, T=T, K=Km).items()}
    with torch.no_grad():
        target.textures.add_(torch.randn_like(target.textures))
        target.alpha_logit.add_(3.0)
        views['imgs'] = target.predict(views, None).clamp(0, 1).contiguous()
    train = {k: v[:V].contiguous() for k, v in views.items()}
    return train, HeldOut([({k: v[i:i + 1].contiguous() for k, v in views.items()}, {'points': torch.zeros(1, 3, 3)}) for i in range(V, V + NVAL)])


def _trainer(scene, run_dir, seed=6, val_interval=4, **kw):
    train, val = scene
    cfg = _cfg(val_interval)
    torch.manual_seed(seed)
    model = dbw_amd.create_model(cfg, (H, W)).to(DEV)
    tr = Trainer(cfg, model, train)
    rec = Recorder(tr, run_dir, val=val, **kw)
    return tr, rec


@pytest.fixture(scope='module')
def full(scene, tmp_path_factory):
    run_dir = tmp_path_factory.mktemp('runs') / 'full'
    walks = scene[1].walks
    tr, rec = _trainer(scene, run_dir)
    tr.run()
    assert scene[1].walks == walks + 1
    torch.cuda.synchronize()
    return tr, rec, run_dir


def _rows(path):
    return [tuple(int(v) for v in ln.split('\t')[:3]) for ln in open(path).read().splitlines()[1:]]


TRAIN_ROWS = [(3, 2, 1), (6, 3, 2), (9, 5, 1), (12, 6, 2)]
VAL_ROWS = [(4, 2, 2), (8, 4, 2), (12, 6, 2)]


def test_files_of_a_run(full):
    tr, rec, run = full
    assert runlog.tick_iterations(6, 2, 3) == TRAIN_ROWS and runlog.tick_iterations(6, 2, 4) == VAL_ROWS
    assert _rows(run / 'train_metrics.tsv') == TRAIN_ROWS and _rows(run / 'val_metrics.tsv') == VAL_ROWS
    names = ['loss_rgb', 'loss_parsimony', 'loss_tv', 'loss_overlap', 'loss_total']
    assert open(run / 'train_metrics.tsv').readline() == 'iteration\tepoch\tbatch\ttime/img\t' + '\t'.join(names) + '\n'
    assert open(run / 'val_metrics.tsv').readline() == 'iteration\tepoch\tbatch\talpha0\talpha1\talpha2\talpha3\tval_PSNR\tval_SSIM\n'
    log = rec.train_metrics.read_log()
    assert all(np.isfinite(v) for c in ['time/img'] + names for v in log[c]) and all(v > 0 for v in log['time/img'])
    assert log['loss_rgb'][0] > log['loss_rgb'][-1], log['loss_rgb']
    for row in zip(*[log[c] for c in names]):
        assert abs(row[4] - sum(row[:4])) < 2e-6 + 1e-5 * row[4]
    vlog = rec.val_metrics.read_log()
    assert all(0 <= a <= 1 for k in range(4) for a in vlog[f'alpha{k}']) and all(5 < p < 60 for p in vlog['val_PSNR'])
    assert all(0 < s <= 1 for s in vlog['val_SSIM'])
    have = set(os.listdir(run))
    assert {'train_metrics.tsv', 'val_metrics.tsv', 'model.pkl', 'model_2.pkl', 'reconstructions', 'reconstructions_hard', 'reconstructions_syn',
            'txt_blocks'} <= have and have <= {'train_metrics.tsv', 'val_metrics.tsv', 'model.pkl', 'model_2.pkl', 'reconstructions',
                                               'reconstructions_hard', 'reconstructions_syn', 'txt_blocks', 'loss.pdf', 'opacity.pdf'}
    for tree in ('reconstructions', 'reconstructions_hard', 'reconstructions_syn', 'txt_blocks'):
        assert os.listdir(run / tree) == ['img0']                  # (the first validation batch holds one view)
        d = run / tree / 'img0'
        files = set(os.listdir(d))
        assert {'evolution', 'final.png'} <= files and len(files & {'evolution.mp4', 'evolution.gif'}) == 1
        assert ('input.png' in files) == (tree != 'txt_blocks')
        assert sorted(os.listdir(d / 'evolution'), key=lambda f: int(f[:-4])) == ['1.png', '4.png', '8.png', '12.png']
        size = Image.open(d / 'final.png').size
        assert (size[0] == 4 * size[1]) if tree == 'txt_blocks' else (size == (W, H)), size      # (4 square maps in a row)
    # the reconstruction before the first step and the one after the last differ
    first, last = [np.asarray(Image.open(run / 'reconstructions_hard' / 'img0' / 'evolution' / f)) for f in ('1.png', '12.png')]
    assert first.shape == (H, W, 3) and (first != last).any()
    ck, ck2 = [torch.load(run / f, map_location='cpu', weights_only=False) for f in ('model.pkl', 'model_2.pkl')]
    assert set(ck) == set(tr.state_dict()) | {'run_state'} and (ck['epoch'], ck['batch'], ck['run_state']['n_iters']) == (6, 2, 12)
    assert (ck2['epoch'], ck2['batch'], ck2['run_state']['n_iters'], ck2['optimizer_state']['n_steps']) == (2, 2, 4, 4)
    assert not [f for f in os.listdir(run) if f.endswith('.tmp')]


def test_the_meter_is_read_once_per_train_tick_and_never_in_between(full):
    tr, rec, run = full
    assert rec.reads == [3, 6, 9, 12]
    assert [t[:2] for t in rec.trace] == [(e, b) for e in range(1, 7) for b in (1, 2)]
    assert [t[4] for t in rec.trace] == list(range(1, 13))
    assert all(sorted(rec.trace[2 * e][2] + rec.trace[2 * e + 1][2]) == list(range(8)) for e in range(6))
    assert rec.trace[7][3] == pytest.approx((5e-3, 5e-2)) and rec.trace[8][3] == pytest.approx((5e-4, 5e-3))      # milestone 4


def test_validation_scores_agree_with_quantitative_eval(full, scene):
    tr, rec, run = full
    vlog = rec.val_metrics.read_log()
    walks = scene[1].walks
    res = tr.model.quantitative_eval(scene[1], DEV, hard_inference=True)
    assert scene[1].walks == walks + 1 and len(rec.val) == NVAL      # (the recorder walked the loader once, when it was built, not at its ticks)
    print(f"val_PSNR {vlog['val_PSNR'][-1]:.6f} vs {res['PSNR']:.6f}, val_SSIM {vlog['val_SSIM'][-1]:.6f} vs {res['SSIM']:.6f}")
    assert abs(vlog['val_PSNR'][-1] - res['PSNR']) < 2e-3 and abs(vlog['val_SSIM'][-1] - res['SSIM']) < 1e-4
    assert all(abs(vlog[f'alpha{k}'][-1] - res[f'alpha{k}']) < 1e-6 for k in range(4))


def _resumed(scene, full, tmp_path, val_interval, stop_at, resumed_from):
    tr_full, rec_full, run_full = full
    run = tmp_path / 'cut'
    tr, rec = _trainer(scene, run, val_interval=val_interval)
    rec.stop_at = stop_at
    with pytest.raises(Stopped):
        tr.run()
    done = len(rec.trace)
    assert rec.trace == rec_full.trace[:done] and not rec.loggers['reconstructions']._thread.is_alive()
    tr2, rec2 = _trainer(scene, run, seed=7, val_interval=val_interval, resume=str(run / 'model.pkl'))
    assert (rec2.epoch_start, rec2.batch_start) == resumed_from and rec2.cur_iter == (resumed_from[0] - 1) * 2 + resumed_from[1]
    assert tr2.epoch == resumed_from[0] and tr2.model.cur_epoch == resumed_from[0] - 1 and tr2.step_fn.n_steps == rec2.cur_iter - 1
    start = rec2.cur_iter
    tr2.run()
    torch.cuda.synchronize()
    # the same (epoch, batch, view indices, learning rates, n_steps) from there on, exactly
    assert len(rec2.trace) == 12 - start + 1 and rec2.trace == rec_full.trace[start - 1:]
    assert tr2.n_iters == 12 and tr2.epoch == 7
    assert_same_trajectory(tr2.step_fn.params.flat, tr_full.step_fn.params.flat, lr_max=5e-2)
    return run, rec2


def test_a_stopped_run_resumes_on_the_same_sequence(full, scene, tmp_path):
    """Stopped after the train tick of iteration 6 = (3,2); model.pkl is the one of the val tick at 4 = (2,2), a finished epoch whose
    scheduler step came after the save: the run resumes at (3,1) with the rates of epoch 3."""
    run, rec2 = _resumed(scene, full, tmp_path, 4, (3, 2), (3, 1))
    assert _rows(run / 'train_metrics.tsv') == TRAIN_ROWS and _rows(run / 'val_metrics.tsv') == VAL_ROWS
    assert rec2.reads == [6, 9, 12]
    assert sorted(os.listdir(run / 'reconstructions' / 'img0' / 'evolution'), key=lambda f: int(f[:-4])) == ['1.png', '4.png', '5.png', '8.png', '12.png']


def test_a_run_stopped_inside_an_epoch_resumes_inside_it(full, scene, tmp_path):
    """val_stat_interval 3: model.pkl at 3 = (2,1), 6, 9 = (5,1).  Stopped after iteration 9, the run resumes at (5,2): the second batch
    of the order epoch 5 drew, behind the milestone of epoch 4."""
    run, rec2 = _resumed(scene, full, tmp_path, 3, (5, 1), (5, 2))
    assert _rows(run / 'train_metrics.tsv') == TRAIN_ROWS and _rows(run / 'val_metrics.tsv') == TRAIN_ROWS
    assert rec2.trace[0][:2] == (5, 2) and rec2.trace[0][3] == pytest.approx((5e-4, 5e-3)) and rec2.reads == [12]


def test_pretrained_loads_the_parameters_and_starts_at_epoch_one(full, scene, tmp_path):
    tr_full, rec_full, run_full = full
    tr, rec = _trainer(scene, tmp_path / 'pre', seed=8, pretrained=str(run_full / 'model.pkl'), images=False)
    assert (rec.epoch_start, rec.batch_start, rec.cur_iter, tr.epoch, tr.model.cur_epoch, tr.step_fn.n_steps) == (1, 1, 1, 1, 0, 0)
    assert tr.step_fn.lrs == (5.0e-3, 5.0e-2) and float(tr.step_fn.exp_avg.abs().sum()) == 0
    for k, v in tr_full.model.state_dict().items():
        assert torch.equal(tr.model.state_dict()[k], v), k
    assert _rows(tmp_path / 'pre' / 'train_metrics.tsv') == []
    with pytest.raises(ValueError, match='both'):
        _trainer(scene, tmp_path / 'both', resume=str(run_full / 'model.pkl'), pretrained=str(run_full / 'model.pkl'))
    rec.close()
