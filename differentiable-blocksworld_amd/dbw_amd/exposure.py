"""Per-view exposure compensation: one 6-vector theta = (g_r, g_g, g_b, b_r, b_g, b_b) per training view, applied to the
decoupled composite before both image terms, rec_c = exp(g_c) * comp_c + b_c, and optimised by Adam beside the model -- what Nerfstudio's
appearance embeddings and the exposure option of 3DGS do for a capture whose exposure and white balance change from frame to frame.

ExposureRefiner holds the state; ops.composite_mse_exposure (dbw_monitor_exposure_composite, csrc/exposure_loss.hip) is the kernel side.
write_exposures puts the fitted gains and offsets into the run directory."""
import os

import torch

from . import ops
from .refine import FlatRefiner, parse_entry


class ExposureRefiner(FlatRefiner):
    """theta (V,6) of a scene's V training views, its gradient and the two Adam moments as flat fp32 buffers on `device` (refine.FlatRefiner).
    attach(batch) -> the batch with 'exposure' = theta (batch['view_ids']: its rows, distinct; 'view_ids_host', where the batch carries it,
    rides along and spares the check of the ids a wait for the device); the backward of the step leaves d loss / d theta in `grad`;
    step() is dense Adam over all V rows like torch.optim.Adam on the tensor (rows of views outside the batch have zero gradient, their
    moments decay) and then clears `grad`.  bias = False keeps the three offsets at 0.  center = True subtracts the column means over the
    V views from theta after each step: a brightness shared by all gains (or offsets) and the textures is a gauge freedom of the loss,
    and the centring fixes it without a hyperparameter.
    adam_fn: a stand-in for ops.adam_step_ with the same signature (tests on CPU tensors: the kernel has no CPU form)."""

    SAVED = ('bias', 'center')

    def __init__(self, n_views, device, lr=1e-3, betas=(0.9, 0.999), bias=True, center=True, eps=1e-8, adam_fn=None):
        self.n_views = int(n_views)
        self.bias, self.center = bool(bias), bool(center)
        super().__init__((self.n_views, 6), device, lr, betas, eps, adam_fn)
        self.theta = self._param()

    def attach(self, batch):
        if 'view_ids' not in batch:
            raise KeyError("ExposureRefiner.attach: the batch carries no 'view_ids' (the rows of theta of its views)")
        return dict(batch, exposure=self.theta)

    def _mask_grad(self):
        if not self.bias:
            self.grad.view(self.n_views, 6)[:, 3:].zero_()

    def _after_update(self):
        if self.center and self.n_views > 0:
            t = self.flat.view(self.n_views, 6)
            t.sub_(t.mean(0, keepdim=True))

    def gains_biases(self):
        """-> (gains exp(g) (V,3), biases (V,3)) on the host, float64."""
        t = self.flat.detach().view(self.n_views, 6).cpu().double()
        return t[:, :3].exp(), t[:, 3:].clone()

    def _state_mismatch(self, numel):
        return f"exposure: a state of {numel // 6} views for a refiner of {self.n_views}"


def parse_config(entry):
    """training.exposure of a config -> dict(lr, start_epoch, bias, center), or None where the key is absent / null / false."""
    return parse_entry('exposure', entry, 1e-3, {'bias': (True, bool), 'center': (True, bool)})


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
