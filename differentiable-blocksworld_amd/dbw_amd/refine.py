"""What the refiners that train beside the model share (pose.PoseRefiner, exposure.ExposureRefiner, intrinsics.IntrinsicsRefiner): a small
parameter as a flat fp32 buffer with its gradient and the two Adam moments, the Adam step, the checkpoint state, and the common part of
their config entries."""
import torch

from . import ops


class FlatRefiner:
    """A parameter of shape `shape` as the flat fp32 buffer `flat` on `device`, its gradient `grad`, the Adam moments `exp_avg` /
    `exp_avg_sq` and the step counter `n_steps`.  _param() is the view of `flat` that takes part in autograd: its .grad is a view of `grad`,
    so the backward accumulates straight into the flat buffer (parallel.FlatParams).  step(): _mask_grad() (a class zeroes or folds the
    gradient of what it keeps frozen), Adam, _after_update() (under no_grad), and `grad` cleared.  adam_fn: a stand-in for ops.adam_step_
    with the same signature (tests on CPU tensors: the kernel has no CPU form).
    A class names its checkpoint: STATE_KEY is the key of the parameter, SAVED the attributes saved beside lr."""
    STATE_KEY = 'theta'
    SAVED = ()

    def __init__(self, shape, device, lr, betas, eps, adam_fn=None):
        self.lr, self.betas, self.eps = float(lr), tuple(betas), float(eps)
        self.shape = tuple(shape)
        n = 1
        for s in self.shape:
            n *= s
        self.flat = torch.zeros(n, dtype=torch.float32, device=device)
        self.grad = torch.zeros_like(self.flat)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.n_steps = 0
        self.adam_fn = adam_fn or ops.adam_step_

    def _param(self):
        p = self.flat.view(self.shape).requires_grad_(True)
        p.grad = self.grad.view(self.shape)
        return p

    def _mask_grad(self):
        pass

    def _after_update(self):
        pass

    def _state_mismatch(self, numel):
        """The refusal of a state whose parameter has `numel` numbers instead of flat's."""
        raise NotImplementedError

    def step(self):
        self._mask_grad()
        self.n_steps += 1
        with torch.no_grad():
            self.adam_fn(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.lr, self.n_steps, self.betas, self.eps)
            self._after_update()
        self.grad.zero_()                                        # (enqueued behind the update: nothing waits for it)

    def state_dict(self):
        state = {self.STATE_KEY: self.flat.detach().clone(), 'exp_avg': self.exp_avg.clone(), 'exp_avg_sq': self.exp_avg_sq.clone(),
                 'n_steps': self.n_steps, 'lr': self.lr}
        for k in self.SAVED:
            v = getattr(self, k)
            state[k] = v.clone() if torch.is_tensor(v) else v
        return state

    def load_state_dict(self, state):
        if state[self.STATE_KEY].numel() != self.flat.numel():
            raise ValueError(self._state_mismatch(state[self.STATE_KEY].numel()))
        with torch.no_grad():
            self.flat.copy_(state[self.STATE_KEY].reshape(-1))
            self.exp_avg.copy_(state['exp_avg'].reshape(-1))
            self.exp_avg_sq.copy_(state['exp_avg_sq'].reshape(-1))
        self.n_steps = int(state['n_steps'])
        self.grad.zero_()


def parse_entry(name, entry, default_lr, extras):
    """training.<name> of a config -> dict(lr, start_epoch, *extras), or None where the key is absent / null / false.  true: the defaults; a
    bare number: the learning rate.  extras: {key: (default, convert)}, convert(value) -> the value kept (it may refuse with ValueError)."""
    if entry is None or entry is False:
        return None
    if entry is True:
        entry = {}
    if not isinstance(entry, dict):
        entry = {'lr': float(entry)}
    keys = ['lr', 'start_epoch'] + list(extras)
    unknown = set(entry) - set(keys)
    if unknown:
        raise ValueError(f"training.{name}: unknown keys {sorted(unknown)} ({', '.join(keys)})")
    kept = {k: convert(entry.get(k, default)) for k, (default, convert) in extras.items()}
    out = {'lr': float(entry.get('lr', default_lr)), 'start_epoch': int(entry.get('start_epoch', 0)), **kept}
    if not out['lr'] > 0:
        raise ValueError(f"training.{name}.lr must be positive, got {out['lr']}")
    return out
