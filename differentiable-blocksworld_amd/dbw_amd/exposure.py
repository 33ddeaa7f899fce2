"""Per-view exposure compensation: one 6-vector theta = (g_r, g_g, g_b, b_r, b_g, b_b) per training view, applied to the
decoupled composite before both image terms, rec_c = exp(g_c) * comp_c + b_c, and optimised by Adam beside the model -- what Nerfstudio's
appearance embeddings and the exposure option of 3DGS do for a capture whose exposure and white balance change from frame to frame.

ExposureRefiner holds the state; ops.composite_mse_exposure (dbw_monitor_exposure_composite, csrc/exposure_loss.hip) is the kernel side.
write_exposures puts the fitted gains and offsets into the run directory."""
import os

import torch

from . import ops


class ExposureRefiner:
    """theta (V,6) of a scene's V training views, its gradient and the two Adam moments as flat fp32 buffers on `device`.
    attach(batch) -> the batch with 'exposure' = theta (batch['view_ids']: its rows, distinct; 'view_ids_host', where the batch carries it,
    rides along and spares the check of the ids a wait for the device); the backward of the step leaves d loss / d theta in `grad`;
    step() is dense Adam over all V rows like torch.optim.Adam on the tensor (rows of views outside the batch have zero gradient, their
    moments decay) and then clears `grad`.  bias = False keeps the three offsets at 0.  center = True subtracts the column means over the
    V views from theta after each step: a brightness shared by all gains (or offsets) and the textures is a gauge freedom of the loss,
    and the centring fixes it without a hyperparameter.
    adam_fn: a stand-in for ops.adam_step_ with the same signature (tests on CPU tensors: the kernel has no CPU form)."""

    def __init__(self, n_views, device, lr=1e-3, betas=(0.9, 0.999), bias=True, center=True, eps=1e-8, adam_fn=None):
        self.n_views, self.lr, self.betas, self.eps = int(n_views), float(lr), tuple(betas), float(eps)
        self.bias, self.center = bool(bias), bool(center)
        self.flat = torch.zeros(self.n_views * 6, dtype=torch.float32, device=device)
        self.grad = torch.zeros_like(self.flat)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.theta = self.flat.view(self.n_views, 6).requires_grad_(True)
        self.theta.grad = self.grad.view(self.n_views, 6)        # the backward accumulates straight into the flat buffer (parallel.FlatParams)
        self.n_steps = 0
        self.adam_fn = adam_fn or ops.adam_step_

    def attach(self, batch):
        if 'view_ids' not in batch:
            raise KeyError("ExposureRefiner.attach: the batch carries no 'view_ids' (the rows of theta of its views)")
        return dict(batch, exposure=self.theta)

    def step(self):
        if not self.bias:
            self.grad.view(self.n_views, 6)[:, 3:].zero_()
        self.n_steps += 1
        with torch.no_grad():
            self.adam_fn(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.lr, self.n_steps, self.betas, self.eps)
            if self.center and self.n_views > 0:
                t = self.flat.view(self.n_views, 6)
                t.sub_(t.mean(0, keepdim=True))
        self.grad.zero_()                                        # (enqueued behind the update: nothing waits for it)

    def gains_biases(self):
        """-> (gains exp(g) (V,3), biases (V,3)) on the host, float64."""
        t = self.flat.detach().view(self.n_views, 6).cpu().double()
        return t[:, :3].exp(), t[:, 3:].clone()

    def state_dict(self):
        return {'theta': self.flat.detach().clone(), 'exp_avg': self.exp_avg.clone(), 'exp_avg_sq': self.exp_avg_sq.clone(), 'n_steps': self.n_steps,
                'lr': self.lr, 'bias': self.bias, 'center': self.center}

    def load_state_dict(self, state):
        if state['theta'].numel() != self.flat.numel():
            raise ValueError(f"exposure: a state of {state['theta'].numel() // 6} views for a refiner of {self.n_views}")
        with torch.no_grad():
            self.flat.copy_(state['theta'].reshape(-1))
            self.exp_avg.copy_(state['exp_avg'].reshape(-1))
            self.exp_avg_sq.copy_(state['exp_avg_sq'].reshape(-1))
        self.n_steps = int(state['n_steps'])
        self.grad.zero_()


def parse_config(entry):
    """training.exposure of a config -> dict(lr, start_epoch, bias, center), or None where the key is absent / null / false."""
    if entry is None or entry is False:
        return None
    if entry is True:
        entry = {}
    if not isinstance(entry, dict):
        entry = {'lr': float(entry)}
    unknown = set(entry) - {'lr', 'start_epoch', 'bias', 'center'}
    if unknown:
        raise ValueError(f'training.exposure: unknown keys {sorted(unknown)} (lr, start_epoch, bias, center)')
    out = {'lr': float(entry.get('lr', 1e-3)), 'start_epoch': int(entry.get('start_epoch', 0)), 'bias': bool(entry.get('bias', True)),
           'center': bool(entry.get('center', True))}
    if not out['lr'] > 0:
        raise ValueError(f"training.exposure.lr must be positive, got {out['lr']}")
    return out


def write_exposures(refiner, run_dir, names=None):
    """<run_dir>/exposures.tsv: a line of column names, then one line per training view in the order of theta's rows -- the view's name
    (names[i], default its index), the gains exp(g) and the offsets b per channel, '{:.6f}'.  -> the path written."""
    gains, biases = refiner.gains_biases()
    if names is not None and len(names) != refiner.n_views:
        raise ValueError(f'{len(names)} names for {refiner.n_views} views')
    path = os.path.join(str(run_dir), 'exposures.tsv')
    with open(path, mode='w') as f:
        f.write('\t'.join(['view', 'gain_r', 'gain_g', 'gain_b', 'bias_r', 'bias_g', 'bias_b']) + '\n')
        for i in range(refiner.n_views):
            row = [float(v) for v in gains[i]] + [float(v) for v in biases[i]]
            f.write('\t'.join([str(i if names is None else names[i])] + ['{:.6f}'.format(v) for v in row]) + '\n')
    return path
