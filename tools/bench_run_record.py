"""What recording a run costs: ms per step of Trainer.run at BASELINE config 2's geometry (49 views of 300 x 400, 10 blocks, 10 faces per
pixel, 256-texel maps) with the reference's batch size 4 -- 13 steps per epoch, `--steps` steps in whole epochs -- for
  none     no recorder attached (python -m dbw_amd.train --no-record),
  metrics  runlog.RunRecorder with the image logs off: the meter, the two metric files, the validation scores, model.pkl,
  all      everything on: the four image logs, their videos and the plots at the end too.
The intervals are those of the shipped configs (train_stat_interval 50, val_stat_interval 100); 5 further views are held out for the
validation scores and reach the recorder as python -m dbw_amd.train hands them over: a dataset.SceneLoader over a scene with a ground-truth
cloud of 3e6 points (the order of a DTU scan's), whose every walk draws 1e5 of them per view on the host.  Every repetition is a fresh model and trainer; the modes alternate within a repetition; the first repetition warms
up and is not reported.  The clock is the host's, around a run that ends in a device synchronise.

    python tools/bench_run_record.py [--modes none,metrics,all] [--steps 500] [--reps 5]  ->  one JSON line"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get('DBW_PACKAGE_DIR') or os.path.join(ROOT, 'differentiable-blocksworld_amd'))

import torch  # noqa: E402

V, NVAL, H, W, BATCH = 49, 5, 300, 400, 4


def make_cfg(n_epoches):
    return {'model': {'name': 'dbw', 'mesh': {'n_blocks': 10, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 256},
                      'renderer': {'faces_per_pixel': 10, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                      'rend_optim': {'coarse_learning': 1500, 'decimate_txt': 750, 'decimate_factor': 8, 'kill_blocks': True,
                                     'decouple_rendering': True, 'opacity_noise': True},
                      'loss': {'rgb_weight': 1, 'perceptual_weight': 0, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}},
            'training': {'batch_size': BATCH, 'n_epoches': n_epoches, 'seed': 4321, 'optimizer': {'name': 'adam', 'lr': 5.0e-3, 'texture': {'lr': 5.0e-2}},
                         'scheduler': {'name': 'multi_step', 'gamma': [0.1, 0.1], 'milestones': [1500]},
                         'train_stat_interval': 50, 'val_stat_interval': 100, 'save_epoches': []}}


def make_views(dev):
    import dbw_amd
    from dbw_amd import mesh as M
    cfg = make_cfg(1)
    torch.manual_seed(227391)
    target = dbw_amd.create_model(cfg, (H, W)).to(dev)
    R, T, K = M.synthetic_cameras(V + NVAL, R_world=target.R_world[0])
    with torch.no_grad():
        g = torch.Generator().manual_seed(99)
        target.T.add_(torch.randn(target.T.shape, generator=g).to(dev) * 0.2)
        target.alpha_logit.add_(2.0)
        target.textures.add_(torch.randn(target.textures.shape, generator=g).to(dev))
        target.eval()
        views = {'imgs': torch.zeros(V + NVAL, 3, H, W, device=dev), 'R': R.to(dev), 'T': T.to(dev), 'K': K.to(dev)}
        views['imgs'] = target.predict(views, None).clamp(0, 1).contiguous()
    train = {k: v[:V].contiguous() for k, v in views.items()}
    return train, HeldOutScene({k: v[V:].contiguous() for k, v in views.items()})


class HeldOutScene:
    """What dataset.SceneLoader asks of a scene: its length, views(device) and the ground-truth points."""

    def __init__(self, views):
        self._views = views
        self.pc_gt = torch.rand(3_000_000, 3, generator=torch.Generator().manual_seed(1))

    def __len__(self):
        return len(self._views['imgs'])

    def views(self, device):
        return {k: v.to(device) for k, v in self._views.items()}


def one_run(mode, train, val, n_epoches, dev, tmp):
    import dbw_amd
    from dbw_amd.trainer import Trainer
    cfg = make_cfg(n_epoches)
    torch.manual_seed(6)
    model = dbw_amd.create_model(cfg, (H, W)).to(dev)
    tr = Trainer(cfg, model, train)
    if mode != 'none':
        from dbw_amd.dataset import SceneLoader
        from dbw_amd.runlog import RunRecorder
        RunRecorder(tr, os.path.join(tmp, mode), val=SceneLoader(val, BATCH, dev), images=(mode == 'all'))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return 1e3 * dt / tr.n_iters, tr.n_iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--modes', default='none,metrics,all')
    ap.add_argument('--steps', type=int, default=500)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--label', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = 'cuda:0'
    modes = args.modes.split(',')
    n_batches = -(-V // BATCH)
    n_epoches = -(-args.steps // n_batches)
    train, val = make_views(dev)
    ms = {m: [] for m in modes}
    steps = 0
    for rep in range(args.reps + 1):
        for m in modes:
            tmp = tempfile.mkdtemp(prefix='dbw_bench_run_')
            try:
                t, steps = one_run(m, train, val, n_epoches, dev, tmp)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
            if rep > 0:
                ms[m].append(round(t, 4))
    out = {'label': args.label, 'steps': steps, 'batch': BATCH, 'views': V, 'HxW': [H, W], 'reps': args.reps,
           'ms_per_step': {m: {'median': sorted(v)[len(v) // 2], 'min': min(v), 'max': max(v), 'all': v} for m, v in ms.items()}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
