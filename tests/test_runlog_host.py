"""CPU tests of the run record's host side (dbw_amd/runlog.py) and of the C boundary include/dbw_monitor.h (against its ctypes
binding and the library: tests/test_abi_families.py): the metric file byte for byte, the tick arithmetic and the resume position on a trainer without a GPU, the image logger's
files and queue, argument validation before any launch."""
import ctypes
import os
import threading

import numpy as np
import pytest
import torch
import torch.nn as nn
from PIL import Image

import frame_ref as FR
from dbw_amd import _lib, ops, runlog
from dbw_amd.trainer import Trainer


# ---- the C boundary (its prototypes, revision and symbols: tests/test_abi_families.py) ------------------------------------------------
def _score_args(**over):
    p = ctypes.c_void_p(256)
    a = dict(a=p, b=p, N=2, H=16, W=16, padding=0, workspace=p, ssim_map=None, out=p, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return list(a.values())


def test_entry_points_validate_before_any_launch():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    for name in ('a', 'b', 'out'):
        assert lib.dbw_image_scores(*_score_args(**{name: None})) == -1 and b'null pointer' in lib.dbw_last_error(), name
    for over in (dict(H=0), dict(W=-2), dict(N=-1), dict(H=1 << 16, W=1 << 16)):
        assert lib.dbw_image_scores(*_score_args(**over)) == -1 and b'bad size' in lib.dbw_last_error(), over
    for over in (dict(H=10), dict(W=10), dict(H=3, W=40)):          # no 11 x 11 window
        assert lib.dbw_image_scores(*_score_args(**over)) == -1 and b'H >= 11' in lib.dbw_last_error(), over
        assert lib.dbw_image_scores_workspace_bytes(2, over.get('H', 16), over.get('W', 16), 0) == 0
    assert lib.dbw_image_scores(*_score_args(padding=2)) == -1 and b'padding' in lib.dbw_last_error()
    assert lib.dbw_image_scores(*_score_args(workspace=None)) == -1 and b'workspace' in lib.dbw_last_error()
    assert lib.dbw_image_scores(*_score_args(workspace=ctypes.c_void_p(260))) == -1 and b'workspace' in lib.dbw_last_error()
    assert lib.dbw_image_scores(*_score_args(a=ctypes.c_void_p(258))) == -1 and b'misaligned' in lib.dbw_last_error()
    assert lib.dbw_image_scores(*_score_args(N=0)) == 0
    # one pair of doubles per 16 x 32 tile of outputs, per channel and image
    assert lib.dbw_image_scores_workspace_bytes(2, 16, 16, 0) == 2 * 3 * 1 * 16
    assert lib.dbw_image_scores_workspace_bytes(1, 48, 64, 1) == 3 * 3 * 2 * 16 and lib.dbw_image_scores_workspace_bytes(1, 48, 64, 0) == 3 * 3 * 2 * 16
    assert lib.dbw_image_scores_workspace_bytes(3, 40, 52, 0) == 3 * 3 * 2 * 2 * 16
    vals = (ctypes.c_void_p * 16)(*([256] * 16))
    vp = ctypes.cast(vals, ctypes.c_void_p)
    assert lib.dbw_meter_add(None, vp, 3, 1.0, 0, None) == -1 and b'null pointer' in lib.dbw_last_error()
    assert lib.dbw_meter_add(p, None, 3, 1.0, 0, None) == -1 and b'null pointer' in lib.dbw_last_error()
    for n in (0, 17, -1):
        assert lib.dbw_meter_add(p, vp, n, 1.0, 0, None) == -1 and b'1 .. 16' in lib.dbw_last_error(), n
        assert lib.dbw_meter_reset(p, n, None) == -1 and b'1 .. 16' in lib.dbw_last_error(), n
    assert lib.dbw_meter_add(p, vp, 3, 1.0, -1, None) == -1 and b'step' in lib.dbw_last_error()
    vals[1] = None
    assert lib.dbw_meter_add(p, vp, 3, 1.0, 0, None) == -1 and b'value pointer' in lib.dbw_last_error()
    assert lib.dbw_meter_add(ctypes.c_void_p(260), vp, 1, 1.0, 0, None) == -1 and b'aligned' in lib.dbw_last_error()
    assert lib.dbw_meter_reset(None, 3, None) == -1


def test_image_scores_on_the_cpu_goes_through_metrics():
    from dbw_amd import metrics
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(2, 3, 14, 20, generator=g), torch.rand(2, 3, 14, 20, generator=g)
    for pad in (False, True):
        mse, ssim, m = ops.image_scores(a, b, padding=pad, return_map=True)
        assert mse.dtype == ssim.dtype == torch.float64 and mse.shape == ssim.shape == (2,)
        assert torch.equal(m, metrics.ssim_map(a, b, padding=pad))
        assert torch.allclose(mse, ((a.double() - b.double()) ** 2).flatten(1).mean(1), rtol=1e-14)
        assert torch.allclose(ssim, m.double().flatten(1).mean(1), rtol=1e-14)
    with pytest.raises(ValueError, match='11 x 11'):
        ops.image_scores(a[:, :, :10], b[:, :, :10])


# ---- the metric file ---------------------------------------------------------------------------------------------------------------------
def test_metrics_file_is_the_reference_s_byte_for_byte(tmp_path):
    path = tmp_path / 'train_metrics.tsv'
    m = runlog.Metrics(['time/img', 'loss_rgb', 'loss_total'], path)
    assert path.read_bytes() == b'iteration\tepoch\tbatch\ttime/img\tloss_rgb\tloss_total\n'
    m.log(50, 1, 50, [0.00123449, 0.25, 1.5])
    m.log(100, 3, 2, [1e-7, float(np.float32(0.1)), 12345.678])
    want = (b'iteration\tepoch\tbatch\ttime/img\tloss_rgb\tloss_total\n'
            b'50\t1\t50\t0.001234\t0.250000\t1.500000\n'
            b'100\t3\t2\t0.000000\t0.100000\t12345.678000\n')
    assert path.read_bytes() == want
    assert m.read_log() == {'iteration': [50, 100], 'epoch': [1, 3], 'batch': [50, 2], 'time/img': [0.001234, 0.0], 'loss_rgb': [0.25, 0.1],
                            'loss_total': [1.5, 12345.678]}
    # append: the file stays and grows
    m2 = runlog.Metrics(['time/img', 'loss_rgb', 'loss_total'], path, append=True)
    assert path.read_bytes() == want
    m2.log(150, 4, 1, [0, 0, 0])
    assert path.read_bytes() == want + b'150\t4\t1\t0.000000\t0.000000\t0.000000\n'
    # append from iteration 100 on: the rows an interrupted run wrote past its checkpoint go, the others stay byte for byte
    runlog.Metrics(['time/img', 'loss_rgb', 'loss_total'], path, append=True, drop_from=100)
    assert path.read_bytes() == want[:want.index(b'100\t')]
    # append to a file that does not exist, and no append: a fresh header
    other = tmp_path / 'val_metrics.tsv'
    runlog.Metrics(['alpha0'], other, append=True)
    assert other.read_bytes() == b'iteration\tepoch\tbatch\talpha0\n'
    runlog.Metrics(['time/img', 'loss_rgb', 'loss_total'], path)
    assert path.read_bytes() == want[:want.index(b'50\t')]
    with pytest.raises(ValueError):
        m.log(1, 1, 1, [0.0])


# ---- ticks and resume on a trainer without a GPU -------------------------------------------------------------------------------------------
class ToyModel(nn.Module):
    """The members of DifferentiableBlocksWorld that Trainer and RunRecorder touch, over a two-term loss."""
    name, init_kwargs, sync_free, cur_epoch, n_blocks = 'toy', {}, True, 0, 2
    loss_weights = {'rgb': 1.0, 'reg': 1.0}
    loss_names = ['loss_rgb', 'loss_reg', 'loss_total']

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.S = nn.Parameter(torch.randn(4, 3))
        self.texture_bkg = nn.Parameter(torch.randn(2, 5))
        self.world_size, self._global_count = 1, None

    def step(self):
        self.cur_epoch += 1

    def set_cur_epoch(self, e):
        self.cur_epoch = e

    def get_opacities(self):
        return torch.tensor([0.75, 0.25])

    def forward(self, inp, labels=None):
        pred = inp['imgs'] * self.S.sum() + self.texture_bkg.sum()
        rgb = ((pred - 1.0) ** 2).sum() / (self._global_count or inp['imgs'].numel())
        reg = (self.S ** 2).mean() + (self.texture_bkg ** 2).mean()
        return {'rgb': rgb, 'reg': reg, 'total': rgb + reg}


def _torch_adam(p, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-8):
    m.mul_(betas[0]).add_(g, alpha=1 - betas[0])
    v.mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
    p.addcdiv_(m, v.sqrt() / (1 - betas[1] ** step) ** 0.5 + eps, value=-lr / (1 - betas[0] ** step))


class Stopped(Exception):
    pass


class Recorder(runlog.RunRecorder):
    """Counts the host reads, keeps the state of chosen positions, stops where told."""
    keep_at, stop_at = (), None

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.trace, self.reads, self.states = [], [], {}
        inner = self.meter.read_reset
        self.meter.read_reset = lambda: (self.reads.append(self.cur_iter), inner())[1]

    def after_step(self, epoch, batch, losses, view_ids):
        super().after_step(epoch, batch, losses, view_ids)
        if (epoch, batch) in self.keep_at:
            self.states[(epoch, batch)] = self.state_dict(epoch, batch)
        if self.stop_at == (epoch, batch):
            raise Stopped


def _toy_run(tmp_path, name, intervals=(3, 5), save_epoches=(), **rec_kw):
    cfg = {'training': {'batch_size': 2, 'n_epoches': 2, 'seed': 7, 'optimizer': {'name': 'adam', 'lr': 1e-2, 'texture': {'lr': 3e-2}},
                        'scheduler': {'name': 'multi_step', 'gamma': [0.5, 0.5], 'milestones': [1]},
                        'train_stat_interval': intervals[0], 'val_stat_interval': intervals[1], 'save_epoches': list(save_epoches)}}
    views = {'imgs': torch.rand(8, 3, 4, 4, generator=torch.Generator().manual_seed(3))}
    tr = Trainer(cfg, ToyModel(), views)
    tr.step_fn.adam_fn = _torch_adam
    assert tr.n_batches == 4
    rec = Recorder(tr, tmp_path / name, images=False, **rec_kw)
    return tr, rec


def _rows(path):
    return [tuple(int(v) for v in ln.split('\t')[:3]) for ln in open(path).read().splitlines()[1:]]


def test_tick_arithmetic_of_two_epochs_of_four_batches():
    """Intervals 3 (train) and 5 (val), iteration = (epoch - 1) * 4 + batch = 1 .. 8: a fresh run writes train rows at 3 = (1,3) and
    6 = (2,2), a val row at 5 = (2,1); a run that starts at (epoch 2, batch 3) is at iteration 7 and writes none; one from (epoch 1,
    batch 4) is at iteration 4 and writes train 6, val 5."""
    assert runlog.tick_iterations(2, 4, 3) == [(3, 1, 3), (6, 2, 2)] and runlog.tick_iterations(2, 4, 5) == [(5, 2, 1)]
    assert runlog.tick_iterations(2, 4, 3, 2, 3) == [] and runlog.tick_iterations(2, 4, 5, 2, 3) == []
    assert runlog.tick_iterations(2, 4, 3, 1, 4) == [(6, 2, 2)] and runlog.tick_iterations(2, 4, 5, 1, 4) == [(5, 2, 1)]
    assert runlog.start_position({'epoch': 2, 'batch': 2}, 4) == (2, 3) and runlog.start_position({'epoch': 2, 'batch': 4}, 4) == (3, 1)


def test_recorder_on_a_cpu_trainer_ticks_saves_and_resumes(tmp_path):
    tr, rec = _toy_run(tmp_path, 'full', save_epoches=[1])
    rec.keep_at = ((2, 1), (2, 2))
    tr.run()
    run = tmp_path / 'full'
    plots = ['loss.pdf', 'opacity.pdf'] if _has_matplotlib() else []
    assert sorted(os.listdir(run)) == sorted(['model.pkl', 'model_1.pkl', 'train_metrics.tsv', 'val_metrics.tsv'] + plots)
    assert _rows(run / 'train_metrics.tsv') == [(3, 1, 3), (6, 2, 2)] and _rows(run / 'val_metrics.tsv') == [(5, 2, 1)]
    assert open(run / 'train_metrics.tsv').readline() == 'iteration\tepoch\tbatch\ttime/img\tloss_rgb\tloss_reg\tloss_total\n'
    assert open(run / 'val_metrics.tsv').read().splitlines() == ['iteration\tepoch\tbatch\talpha0\talpha1', '5\t2\t1\t0.750000\t0.250000']
    assert rec.reads == [3, 6]                                      # the meter is read at the train ticks and never in between
    assert [t[:2] for t in rec.trace] == [(e, b) for e in (1, 2) for b in (1, 2, 3, 4)]
    assert sorted(i for t in rec.trace[:4] for i in t[2]) == list(range(8))
    assert [t[4] for t in rec.trace] == list(range(1, 9)) and rec.trace[0][3] == (1e-2, 3e-2) and rec.trace[4][3] == (5e-3, 1.5e-2)
    log = rec.train_metrics.read_log()
    assert all(np.isfinite(v) for c in rec.model.loss_names for v in log[c]) and log['loss_total'][0] > log['loss_total'][1]
    final = torch.load(run / 'model.pkl', weights_only=False)
    assert (final['epoch'], final['batch']) == (2, 4) and final['scheduler_state']['last_epoch'] == 2
    assert set(final) == set(tr.state_dict()) | {'run_state'} and set(final['run_state']) == {'perm_state', 'order', 'batch', 'n_iters'}
    first = torch.load(run / 'model_1.pkl', weights_only=False)
    assert (first['epoch'], first['batch'], first['run_state']['n_iters']) == (1, 4, 4)

    # resumed inside epoch 2, after its second batch: iterations 7 and 8, the same views, rates and step numbers, the same parameters
    ckpt = rec.states[(2, 2)]
    assert (ckpt['epoch'], ckpt['batch'], ckpt['scheduler_state']['last_epoch']) == (2, 2, 1)
    tr2, rec2 = _toy_run(tmp_path, 'full', resume=ckpt)
    assert (rec2.epoch_start, rec2.batch_start, rec2.cur_iter, tr2.epoch, tr2.model.cur_epoch) == (2, 3, 7, 2, 1)
    assert _rows(run / 'train_metrics.tsv') == [(3, 1, 3), (6, 2, 2)]            # appended to, nothing from iteration 7 on to drop
    tr2.run()
    assert rec2.trace == rec.trace[6:] and rec2.reads == []
    assert torch.equal(tr2.step_fn.params.flat, tr.step_fn.params.flat) and tr2.n_iters == 8
    assert _rows(run / 'train_metrics.tsv') == [(3, 1, 3), (6, 2, 2)] and _rows(run / 'val_metrics.tsv') == [(5, 2, 1)]

    # stopped after iteration 6, resumed from the model.pkl of the val tick at 5 = (2,1): row 6 is written again, once
    tr3, rec3 = _toy_run(tmp_path, 'cut')
    rec3.stop_at = (2, 2)
    with pytest.raises(Stopped):
        tr3.run()
    cut = tmp_path / 'cut'
    assert _rows(cut / 'train_metrics.tsv') == [(3, 1, 3), (6, 2, 2)]
    tr4, rec4 = _toy_run(tmp_path, 'cut', resume=str(cut / 'model.pkl'))
    assert (rec4.epoch_start, rec4.batch_start, rec4.cur_iter) == (2, 2, 6) and _rows(cut / 'train_metrics.tsv') == [(3, 1, 3)]
    tr4.run()
    assert rec4.trace == rec.trace[5:] and torch.equal(tr4.step_fn.params.flat, tr.step_fn.params.flat)
    assert _rows(cut / 'train_metrics.tsv') == [(3, 1, 3), (6, 2, 2)] and _rows(cut / 'val_metrics.tsv') == [(5, 2, 1)]

    # the same checkpoints without a recorder (--no-record --resume): position, schedule and order are read all the same
    for ck, n_left in ((ckpt, 2), (rec.states[(2, 1)], 3)):
        tr_n, rec_n = _toy_run(tmp_path, 'norec')
        tr_n.recorder = None
        assert runlog.load_checkpoint(tr_n, ck) == runlog.start_position(ck, 4) and tr_n.epoch == 2 and tr_n.step_fn.lrs == (5e-3, 1.5e-2)
        tr_n.run()
        assert tr_n.n_iters == 8 and tr_n.step_fn.n_steps == 8 and torch.equal(tr_n.step_fn.params.flat, tr.step_fn.params.flat), n_left
    with pytest.raises(ValueError, match='no run_state'):
        runlog.load_checkpoint(tr_n, {k: v for k, v in ckpt.items() if k != 'run_state'})

    # a second run() on the same trainer goes on recording: two epochs, then a third
    tr_s, rec_s = _toy_run(tmp_path, 'twice')
    tr_s.run(n_epoches=1)
    tr_s.run()
    assert [t[:2] for t in rec_s.trace] == [(e, b) for e in (1, 2) for b in (1, 2, 3, 4)] and _rows(tmp_path / 'twice' / 'train_metrics.tsv') == [(3, 1, 3), (6, 2, 2)]

    # a checkpoint without run_state, as Trainer.state_dict() makes it, resumes at the start of the next epoch
    tr5, _ = _toy_run(tmp_path, 'plain')
    tr5.recorder = None
    tr5.run_epoch()
    tr6, rec6 = _toy_run(tmp_path, 'plain', resume=tr5.state_dict())
    assert (rec6.epoch_start, rec6.batch_start, rec6.cur_iter, tr6.step_fn.n_steps) == (2, 1, 5, 4)
    rec6.close()

    # pretrained: the parameters, and a run from epoch 1
    tr7, rec7 = _toy_run(tmp_path, 'pre', pretrained=final)
    assert (rec7.epoch_start, rec7.batch_start, rec7.cur_iter, tr7.epoch, tr7.step_fn.n_steps) == (1, 1, 1, 1, 0)
    assert torch.equal(tr7.step_fn.params.flat, tr.step_fn.params.flat) and float(tr7.step_fn.exp_avg.abs().sum()) == 0
    rec7.close()


def _has_matplotlib():
    try:
        import matplotlib  # noqa: F401
        return True
    except ImportError:
        return False


def test_held_out_views_are_made_resident_once():
    """A loader is walked once at most -- a scene's loader draws its labels on the host at every walk -- and one with a dataset not at all."""
    views = {'imgs': torch.rand(5, 3, 4, 4), 'R': torch.rand(5, 3, 3), 'T': torch.rand(5, 3), 'K': torch.rand(5, 4, 4)}

    class Loader:
        walks, batch_size = 0, 2

        def __len__(self):
            return 3

        def __iter__(self):
            Loader.walks += 1
            for a in range(0, 5, 2):
                yield {k: v[a:a + 2] for k, v in views.items()}, {'points': torch.zeros(2, 7, 3)}

    class Scene:
        pc_gt, asked = torch.zeros(1, 3), 0

        def __len__(self):
            return 5

        def views(self, device):
            Scene.asked += 1
            return dict(views, raw=None)

    from dbw_amd.dataset import SceneLoader
    for val in (views, Loader(), SceneLoader(Scene(), 2, 'cpu')):
        got = runlog.held_out_batches(val, 'cpu', 2)
        assert [len(b[0]['imgs']) for b in got] == [2, 2, 1] and all(lab is None for _, lab in got)
        assert torch.equal(torch.cat([b[0]['K'] for b in got]), views['K']) and set(got[0][0]) == {'imgs', 'R', 'T', 'K'}
    assert Loader.walks == 1 and Scene.asked == 1
    assert runlog.held_out_batches(None, 'cpu', 2) == [] and runlog.held_out_batches([], 'cpu', 2) == []


def test_resume_together_with_pretrained_is_refused(tmp_path):
    with pytest.raises(ValueError, match='both'):
        runlog.resolve_start({'resume': 'a', 'pretrained': 'b'}, 'run')
    with pytest.raises(ValueError, match='both'):
        runlog.resolve_start({'pretrained': 'b'}, 'run', cli_resume=True)
    assert runlog.resolve_start({'resume': None, 'pretrained': None}, 'run') == (None, None)
    assert runlog.resolve_start({}, 'run', cli_resume=True) == ('run', None) and runlog.resolve_start({}, 'run', cli_resume='other') == ('other', None)
    assert runlog.resolve_start({'pretrained': 'b'}, 'run') == (None, 'b')
    with pytest.raises(ValueError, match='both'):
        _toy_run(tmp_path, 'x', resume={}, pretrained={})
    assert not (tmp_path / 'x').exists()                            # refused before anything is written


def test_a_non_finite_loss_stops_the_run_at_the_next_tick(tmp_path):
    tr, rec = _toy_run(tmp_path, 'nan')
    inner = tr.run_single_batch_train

    def poisoned(inp, global_count=None):
        losses, t0 = inner(inp, global_count)
        if tr.n_iters == 2:
            losses = dict(losses, reg=losses['reg'] * float('nan'))
        return losses, t0
    tr.run_single_batch_train = poisoned
    with pytest.raises(FloatingPointError, match='iteration 2 .*iteration 3'):
        tr.run()
    assert _rows(tmp_path / 'nan' / 'train_metrics.tsv') == [(3, 1, 3)]


def test_more_than_one_rank_is_refused(tmp_path):
    tr, rec = _toy_run(tmp_path, 'one')
    tr.step_fn.world_size = 2
    with pytest.raises(NotImplementedError, match='2 ranks'):
        runlog.RunRecorder(tr, tmp_path / 'two', images=False)


# ---- the image logger ----------------------------------------------------------------------------------------------------------------------
def _png(path):
    return torch.from_numpy(np.array(Image.open(path))).permute(2, 0, 1)


def test_image_logger_layout_and_bytes(tmp_path):
    g = torch.Generator().manual_seed(5)
    targets = torch.rand(3, 3, 10, 14, generator=g)
    lg = runlog.ImageLogger(tmp_path / 'reconstructions', targets, 'png')
    frames = {it: torch.rand(3, 3, 10, 14, generator=g) * 1.4 - 0.2 for it in (1, 4, 8)}
    frames[4][0, 0, 0, 0] = float('nan')
    for it, f in frames.items():
        lg.save(f, it)
    last = torch.rand(3, 3, 10, 14, generator=g)
    lg.save(last)
    videos = lg.save_video()
    lg.close()
    assert lg.pending() == 0 and lg.frames_written == 3 * 5 and not lg._thread.is_alive()
    for k in range(3):
        d = tmp_path / 'reconstructions' / f'img{k}'
        video = 'evolution.mp4' if videos[k].endswith('.mp4') else 'evolution.gif'
        assert sorted(os.listdir(d)) == sorted(['evolution', video, 'final.png', 'input.png'])
        assert sorted(os.listdir(d / 'evolution')) == ['1.png', '4.png', '8.png']
        assert torch.equal(_png(d / 'input.png'), FR.quantise(targets[k])) and torch.equal(_png(d / 'final.png'), FR.quantise(last[k]))
        for it, f in frames.items():
            assert torch.equal(_png(d / 'evolution' / f'{it}.png'), FR.quantise(f[k])), (k, it)
        if video.endswith('.gif'):
            assert Image.open(d / video).n_frames == 3
    lg.save(last, 9)                            # a closed logger starts its writer again: a trainer may run a second time
    lg.close()
    assert lg.frames_written == 3 * 6 and not lg._thread.is_alive() and os.path.exists(tmp_path / 'reconstructions' / 'img2' / 'evolution' / '9.png')
    # without targets: one image, no input.png (the texture log)
    tl = runlog.ImageLogger(tmp_path / 'txt_blocks', None, 'jpg')
    tl.save(torch.rand(1, 3, 8, 40, generator=g), 2)
    tl.close()
    assert sorted(os.listdir(tmp_path / 'txt_blocks' / 'img0')) == ['evolution'] and os.listdir(tmp_path / 'txt_blocks' / 'img0' / 'evolution') == ['2.jpg']
    with pytest.raises(ValueError):
        runlog.ImageLogger(tmp_path / 'bad', targets).save(torch.rand(2, 3, 10, 14))


def test_a_queue_of_depth_one_blocks_the_caller_and_still_writes_every_frame(tmp_path):
    import queue
    g = torch.Generator().manual_seed(6)
    lg = runlog.ImageLogger(tmp_path / 'log', None, 'png', queue_depth=1)
    caller = threading.current_thread().name
    seen, full_hits = set(), []
    gate = threading.Event()
    save, put = Image.Image.save, lg._queue.put

    def gated_save(self, *a, **k):             # the writer thread holds its first frame until the caller has met a full queue
        seen.add(threading.current_thread().name)
        assert gate.wait(60)
        return save(self, *a, **k)

    def watched_put(item):                     # the logger's put: when the queue is full, note it, let the writer go, then block as it does
        try:
            put(item, block=False)
        except queue.Full:
            full_hits.append(item)
            gate.set()
            put(item)
    Image.Image.save, lg._queue.put = gated_save, watched_put
    try:
        frames = [torch.rand(1, 3, 6, 9, generator=g) for _ in range(6)]
        for i, f in enumerate(frames):
            lg.save(f, i)
        assert full_hits and lg.frames_written < 6      # the caller ran ahead of the writer and was held at the full queue
        lg.close()
    finally:
        Image.Image.save = save
        gate.set()
    assert seen == {'dbw-image-logger'} and caller not in seen          # nothing is encoded on the calling thread
    assert lg.frames_written == 6 and lg.pending() == 0
    for i, f in enumerate(frames):
        assert torch.equal(_png(tmp_path / 'log' / 'img0' / 'evolution' / f'{i}.png'), FR.quantise(f[0]))
