"""GPU helper: how far two processes running bench.py's timed path apart drift, step by step -- the reason `bench.py --dump-outputs` dumps
one step from the seeded state instead of the state the timed steps reach.  usage:
    dump_drift.py run OUT.npz            # the default workload, bench.py's seed and learning rates: losses / parameters / gradient after
                                         # steps 1..23 of one chain, and one step from the seeded state replayed after them
    dump_drift.py compare A.npz B.npz    # per step, over the ten parameter tensors: the worst max |a - b| / max |a|"""
import os
import sys

import numpy as np

STEPS = (1, 2, 3, 5, 9, 17, 23)


def run(path):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import bench
    from dbw_amd.parallel import ShardedTrainStep

    class A:
        views, H, W, blocks, fpp, txt = 49, 300, 400, 10, 10, 256
    model, inp = bench.build_workload(A, torch.device('cuda', 0))
    model.set_cur_epoch(0)
    model.sync_free = True
    step = ShardedTrainStep(model, lr=5e-3, lr_texture=5e-2, seed=227391)
    snap = (step.params.flat.clone(), step.exp_avg.clone(), step.exp_avg_sq.clone(), step.n_steps)
    out = {}

    def keep(tag, losses):
        torch.cuda.synchronize()
        out[f'{tag}/flat'] = step.params.flat.cpu().numpy()
        out[f'{tag}/grad'] = step.params.grad.cpu().numpy()
        out[f'{tag}/loss'] = np.array([float(losses[k]) for k in sorted(losses)])
    for i in range(1, max(STEPS) + 1):
        losses = step(inp, global_count=inp['imgs'].numel())
        if i in STEPS:
            keep(f'chain{i}', losses)
    step.params.flat.copy_(snap[0]); step.exp_avg.copy_(snap[1]); step.exp_avg_sq.copy_(snap[2]); step.n_steps = snap[3]
    keep('replay1', step(inp, global_count=inp['imgs'].numel()))
    np.savez(path, names=np.array([f'{n}:{o}:{k}' for n, o, k in step.params.names]), **out)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    names = [(n, int(o), int(k)) for n, o, k in (s.split(':') for s in a['names'])]
    for tag in [f'chain{i}' for i in STEPS] + ['replay1']:
        la, lb = a[f'{tag}/loss'], b[f'{tag}/loss']
        row = [f'{tag:8s} losses {np.max(np.abs(la - lb) / np.maximum(np.abs(la), 1e-30)):.1e}']
        for what in ('flat', 'grad'):
            worst = max((np.abs(a[f'{tag}/{what}'][o:o + k].astype(np.float64) - b[f'{tag}/{what}'][o:o + k]).max()
                         / max(float(np.abs(a[f'{tag}/{what}'][o:o + k]).max()), 1e-30), n) for n, o, k in names)
            row.append(f'{"parameters" if what == "flat" else "gradient"} {worst[0]:.1e} ({worst[1]})')
        print('  '.join(row))


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        run(sys.argv[2])
    else:
        compare(sys.argv[2], sys.argv[3])
