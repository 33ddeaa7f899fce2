"""The record of a run, with the files and the cadence of the reference's trainer (src/trainer.py:50-69,110-239): train_metrics.tsv and
val_metrics.tsv, the four image logs with their videos, model.pkl at every validation tick, model_<epoch>.pkl at `save_epoches`, loss.pdf
and opacity.pdf, and resuming from model.pkl.

The reference reads every loss on the host after every step (.item(), trainer.py:143) and encodes its PNGs on the training thread.  Here a
step is one C call that never waits for the host, so between two ticks everything stays on the device: the step's loss scalars are added
to a table there (DeviceMeter: dbw_meter_add, one small launch per step), the held-out views are scored by one kernel per batch
(ops.image_scores), frames are made 8-bit on the device (ops.frames_u8), copied to pinned memory on a side stream and encoded by a writer
thread.  The host waits for the device once per tick (DeviceMeter.read_reset, or the one read of the validation scores).

`time/img` is the wall time between two train ticks over the images trained on between them -- the reference's column is the host time of
each step, which does not exist where the host does not wait for its steps."""
import ctypes
import math
import os
import queue
import threading
import time

import torch

from . import _lib, ops

N_VIZ_SAMPLES = 4


# ---- the metric files ----------------------------------------------------------------------------------------------------------------------
class Metrics:
    """One tab-separated log, the reference's file byte for byte (utils/metrics.py:48,59): a header `iteration epoch batch <names>`, then
    one row per log() with the values as {:.6f}.  The file is truncated unless `append` is set and it exists; with `append`, rows from
    iteration `drop_from` on (what an interrupted run wrote after its last checkpoint) are dropped first, the others stay as they are."""

    def __init__(self, names, log_file, append=False, drop_from=None):
        self.names, self.log_file = list(names), str(log_file)
        header = 'iteration\tepoch\tbatch\t' + '\t'.join(self.names) + '\n'
        if not (append and os.path.exists(self.log_file)):
            with open(self.log_file, mode='w') as f:
                f.write(header)
        elif drop_from is not None:
            with open(self.log_file) as f:
                lines = f.readlines()
            kept = lines[:1] + [ln for ln in lines[1:] if ln.strip() and int(ln.split('\t', 1)[0]) < drop_from]
            if kept != lines:
                with open(self.log_file, mode='w') as f:
                    f.writelines(kept)

    def log(self, it, epoch, batch, values):
        if len(values) != len(self.names):
            raise ValueError(f'{len(self.names)} columns, {len(values)} values')
        with open(self.log_file, mode='a') as f:
            f.write(f'{it}\t{epoch}\t{batch}\t' + '\t'.join('{:.6f}'.format(float(v)) for v in values) + '\n')

    def read_log(self):
        """-> {column: [values]} with the columns of the header ('iteration', 'epoch', 'batch' as int); no pandas."""
        with open(self.log_file) as f:
            lines = [ln.rstrip('\n') for ln in f if ln.strip()]
        cols = lines[0].split('\t')
        out = {c: [] for c in cols}
        for ln in lines[1:]:
            for i, (c, v) in enumerate(zip(cols, ln.split('\t'))):
                out[c].append(int(v) if i < 3 else float(v))
        return out


# ---- running sums on the device --------------------------------------------------------------------------------------------------------------
class DeviceMeter:
    """Running weighted sums of the step's loss scalars, kept where the step leaves them.  add() is one dbw_meter_add on the current
    stream: no read, no wait.  read_reset() is the one place that waits for the device.  Tensors on the CPU (a model without a GPU) are
    added on the host with the same arithmetic."""

    def __init__(self, names, device):
        self.names, self.device = list(names), torch.device(device)
        n = len(self.names)
        if not 1 <= n <= _lib.METER_MAX_VALUES:
            raise ValueError(f'{n} values: a meter takes 1 .. {_lib.METER_MAX_VALUES}')
        self.table = torch.zeros(n + 2, dtype=torch.float64, device=self.device)
        self.table[n + 1] = -1.0
        self._ptrs = (ctypes.c_void_p * n)()
        self._keep = None
        if self.device.type == 'cuda':
            ops._monitor_lib()

    def add(self, loss_dict, N, step):
        """loss_dict: {name: 0-dim fp32 tensor} holding at least self.names; N: the weight (images of the step); step: its number."""
        n = len(self.names)
        vals = [loss_dict[k] for k in self.names]
        if self.device.type != 'cuda':
            t = self.table
            for i, v in enumerate(vals):
                t[i] += float(v.detach().float()) * float(N)
            t[n] += float(N)
            if t[n + 1] < 0 and not all(math.isfinite(float(v)) for v in vals):
                t[n + 1] = float(step)
            return
        for i, v in enumerate(vals):
            if not (torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float32 and v.numel() == 1):
                raise TypeError(f'{self.names[i]}: a single fp32 value on the GPU is expected, got {type(v).__name__}'
                                + (f' {v.dtype} {tuple(v.shape)} on {v.device}' if torch.is_tensor(v) else ''))
            self._ptrs[i] = v.data_ptr()
        self._keep = vals                   # (a value made for this step alone -- the total with the perceptual term -- lives until the next add)
        _lib.call('dbw_meter_add', self.table.data_ptr(), ctypes.cast(self._ptrs, ctypes.c_void_p), n, float(N), int(step),
                  torch.cuda.current_stream(self.device).cuda_stream)

    def read_reset(self):
        """-> ({name: weighted average}, the step at which a value first was not finite, or None).  One device-to-host copy and one wait."""
        n = len(self.names)
        host = self.table.tolist()
        if self.device.type == 'cuda':
            _lib.call('dbw_meter_reset', self.table.data_ptr(), n, torch.cuda.current_stream(self.device).cuda_stream)
        else:
            self.table.zero_()
            self.table[n + 1] = -1.0
        count = host[n]
        avg = {k: (host[i] / count if count else 0.0) for i, k in enumerate(self.names)}
        return avg, (int(host[n + 1]) if host[n + 1] >= 0 else None)


# ---- image logs ------------------------------------------------------------------------------------------------------------------------------
def _quantise_host(images):
    """The bytes ops.frames_u8 makes, for frames that live on the CPU: clamp to [0, 1], times 255 in fp32, truncate; NaN -> 0."""
    t = torch.nan_to_num(images.detach().float(), nan=0.0)
    return (t.clamp(0, 1) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


class ImageLogger:
    """The reference's layout (utils/image.py:164-217): <log_dir>/img{k}/input.png, img{k}/evolution/{it}.{ext}, img{k}/final.png and, by
    save_video(), img{k}/evolution.mp4 (.gif where export.save_video has no encoder).  save() converts on the device, starts the copy to
    pinned memory on a side stream and hands the rest to the writer thread through a bounded queue: a full queue blocks the caller, no image
    is encoded on the calling thread.  close() drains the queue and ends the thread (the next save() starts a new one); an error of the writer is raised by the next call."""

    def __init__(self, log_dir, target_images=None, out_ext='png', n_images=1, queue_depth=8):
        self.log_dir, self.out_ext = str(log_dir), out_ext
        self.n_images = len(target_images) if target_images is not None else n_images
        for k in range(self.n_images):
            os.makedirs(os.path.join(self.log_dir, f'img{k}', 'evolution'), exist_ok=True)
        self._queue = queue.Queue(maxsize=max(int(queue_depth), 1))
        self._error, self._side = None, None
        self.frames_written = 0
        self._thread = None
        if target_images is not None:
            self._enqueue(target_images, [os.path.join(self.log_dir, f'img{k}', 'input.png') for k in range(self.n_images)])

    def _writer(self):
        from PIL import Image
        while True:
            item = self._queue.get()
            try:
                if item is None:
                    return
                event, host, paths = item
                if event is not None:
                    event.synchronize()
                if self._error is None:
                    arr = host.numpy()
                    for k, p in enumerate(paths):
                        Image.fromarray(arr[k]).save(p)
                        self.frames_written += 1
            except Exception as e:                      # kept for the caller: a thread cannot raise into it
                self._error = e
            finally:
                self._queue.task_done()

    def _check(self):
        if self._error is not None:
            e, self._error = self._error, None
            raise RuntimeError(f'the image writer of {self.log_dir} failed: {e!r}') from e

    def _enqueue(self, images, paths):
        self._check()
        if images.dim() != 4 or images.shape[1] != 3 or len(images) != len(paths):
            raise ValueError(f'{len(paths)} frames of (3,H,W) expected, got {tuple(images.shape)}')
        if images.is_cuda:
            dev = images.device
            cur = torch.cuda.current_stream(dev)
            frames = ops.frames_u8(images)
            if self._side is None:
                self._side = torch.cuda.Stream(device=dev)
            self._side.wait_stream(cur)
            host = torch.empty(frames.shape, dtype=torch.uint8, pin_memory=True)
            with torch.cuda.stream(self._side):
                host.copy_(frames, non_blocking=True)
                event = torch.cuda.Event()
                event.record(self._side)
            frames.record_stream(self._side)
        else:
            host, event = _quantise_host(images), None
        if self._thread is None or not self._thread.is_alive():         # (the first frame, or the first after a close())
            self._thread = threading.Thread(target=self._writer, name='dbw-image-logger', daemon=True)
            self._thread.start()
        self._queue.put((event, host, paths))           # blocks while the queue is full

    def save(self, images, it=None):
        """images (n_images,3,H,W) fp32 -> evolution/{it}.{ext}, or final.png without `it`."""
        sub = ['final.png'] if it is None else ['evolution', f'{it}.{self.out_ext}']
        self._enqueue(images, [os.path.join(self.log_dir, f'img{k}', *sub) for k in range(self.n_images)])

    def drain(self):
        self._queue.join()
        self._check()

    def pending(self):
        return self._queue.unfinished_tasks

    def save_video(self, fps=24):
        """evolution/*.{ext} in the order of their iterations -> evolution.mp4 (or .gif) per image.  -> the paths written."""
        import numpy as np
        from PIL import Image
        from .export import save_video
        self.drain()
        out = []
        for k in range(self.n_images):
            folder = os.path.join(self.log_dir, f'img{k}', 'evolution')
            its = sorted(int(f[:-len(self.out_ext) - 1]) for f in os.listdir(folder) if f.endswith('.' + self.out_ext) and f[:-len(self.out_ext) - 1].isdigit())
            if its:
                frames = np.stack([np.asarray(Image.open(os.path.join(folder, f'{i}.{self.out_ext}')).convert('RGB')) for i in its])
                out.append(save_video(frames, os.path.join(self.log_dir, f'img{k}', 'evolution.mp4'), fps=fps))
        return out

    def close(self):
        """Drains the queue and ends the writer thread; a later save() starts a new one."""
        if self._thread is not None and self._thread.is_alive():
            self._queue.put(None)
            self._thread.join()
        self._check()


# ---- where a run starts ----------------------------------------------------------------------------------------------------------------------
def resolve_start(training_cfg, own_tag, cli_resume=None):
    """-> (resume_tag, pretrained_tag), at most one of them set, from cfg['training'].{resume, pretrained} and the command line's --resume
    (True: the run's own tag).  Both at once is an error, as in the reference (trainer.py:86)."""
    resume, pretrained = training_cfg.get('resume'), training_cfg.get('pretrained')
    if cli_resume:
        resume = own_tag if cli_resume is True else cli_resume
    if resume is not None and pretrained is not None:
        raise ValueError(f'training.resume ({resume!r}) and training.pretrained ({pretrained!r}) are both set: resume continues a run, '
                         'pretrained starts a new one from its weights -- give one of them')
    return resume, pretrained


def start_position(ckpt, n_batches):
    """(epoch_start, batch_start) of a run resumed from `ckpt`, as trainer.py:93-96 reads 'epoch' and 'batch': a checkpoint whose last
    batch ended an epoch starts the next one."""
    if ckpt['batch'] >= n_batches:
        return ckpt['epoch'] + 1, 1
    return ckpt['epoch'], ckpt['batch'] + 1


def tick_iterations(n_epoches, n_batches, interval, epoch_start=1, batch_start=1):
    """The (iteration, epoch, batch) at which a log of this interval writes a row, for a run from (epoch_start, batch_start)."""
    out = []
    for epoch in range(epoch_start, n_epoches + 1):
        for batch in range(batch_start if epoch == epoch_start else 1, n_batches + 1):
            it = (epoch - 1) * n_batches + batch
            if it % interval == 0:
                out.append((it, epoch, batch))
    return out


def load_checkpoint(trainer, ckpt):
    """Continue from `ckpt` -- a recorder's checkpoint or a plain Trainer.state_dict() -- : model, Adam moments and step count, scheduler,
    and the position.  -> (epoch_start, batch_start).  A checkpoint written inside an epoch -- its last batch included: the tick comes
    before the scheduler's step -- holds the schedule and the model's epoch count of the epochs FINISHED before it: both are brought to
    epoch_start - 1.  With a `run_state` the permutation generator and n_iters are restored, and a start inside an epoch walks the rest of
    that epoch's order (trainer._resume_pos)."""
    t = trainer
    t.load_state_dict(ckpt)
    epoch_start, batch_start = start_position(ckpt, t.n_batches)
    while t.scheduler.last_epoch < epoch_start - 1:
        t.step_fn.lrs = tuple(t.scheduler.step())
    t.epoch = epoch_start
    t.model.set_cur_epoch(epoch_start - 1)
    rs = ckpt.get('run_state')
    if rs is not None:
        t._perm_gen.set_state(rs['perm_state'].cpu())
        t.n_iters = rs['n_iters']
        if batch_start > 1:
            t._resume_pos = (rs['order'].cpu(), batch_start - 1)
    elif batch_start > 1:
        raise ValueError(f"the checkpoint stops inside epoch {ckpt['epoch']} (batch {ckpt['batch']} of {t.n_batches}) and has no run_state: the "
                         'order of that epoch is not known')
    return epoch_start, batch_start


def held_out_batches(val, device, batch_size):
    """The held-out views as a list of (inp, None), device tensors, made ONCE: a loader is not walked at every tick (a scene's loader draws
    1e5 ground-truth points per view on the host at every walk, which the scores do not read).  val: a dict of view tensors; a loader with
    a `dataset` that has views(device) (dataset.SceneLoader), sliced by its batch_size; or any iterable of (inp, labels), walked once."""
    if val is None:
        return []
    keys = ('imgs', 'R', 'T', 'K')
    if isinstance(val, dict):
        views, bs = val, batch_size
    elif hasattr(getattr(val, 'dataset', None), 'views'):
        if len(val.dataset) == 0:
            return []
        views, bs = val.dataset.views(device), int(getattr(val, 'batch_size', batch_size))
    else:
        return [({k: v.to(device) for k, v in inp.items() if torch.is_tensor(v)}, None) for inp, _ in val]
    views = {k: views[k].to(device) for k in keys if k in views}
    return [({k: v[a:a + bs] for k, v in views.items()}, None) for a in range(0, len(views['imgs']), bs)]


class RunRecorder:
    """Attached to a Trainer (trainer.recorder = this; the constructor does it), called by its loop: begin_run, begin_epoch, after_step,
    after_epoch, finish.  val: the held-out views -- a loader of (inp, labels), or a dict of view tensors, or None; they are made resident once
    (held_out_batches), the loader is not walked again.  viz: a dict of view tensors for the image logs; default: the first validation batch, or the first training
    views.  The cadence is the reference's (trainer.py:110-135), the intervals come from trainer.cfg['training'].

    resume: a checkpoint (dict, or the path of a model.pkl) to continue -- model, Adam moments and step count, scheduler, the position
    inside the epoch; the metric files are appended to.  pretrained: a checkpoint whose model state alone is loaded."""

    def __init__(self, trainer, run_dir, val=None, viz=None, resume=None, pretrained=None, images=True, queue_depth=8):
        if resume is not None and pretrained is not None:
            raise ValueError('resume and pretrained are both given: resume continues a run, pretrained starts a new one -- give one of them')
        if trainer.step_fn.world_size > 1:
            raise NotImplementedError(f'recording a run of {trainer.step_fn.world_size} ranks is not implemented: every rank would write the same '
                                      'files, and the losses it holds are those of its own shard -- train with --no-record, or on one GPU')
        tr = dict(trainer.cfg.get('training') or {})
        self.trainer, self.model, self.run_dir = trainer, trainer.model, str(run_dir)
        self.train_stat_interval = int(tr.get('train_stat_interval', 100))
        self.val_stat_interval = int(tr.get('val_stat_interval', 100))
        self.save_epoches = set(tr.get('save_epoches') or [])
        self.device = trainer.views['imgs'].device
        os.makedirs(self.run_dir, exist_ok=True)
        self.trace = None                   # a list: after_step appends (epoch, batch, view ids, learning rates, n_steps)
        self.epoch_start, self.batch_start = 1, 1
        self._order = None
        for ck, full in ((resume, True), (pretrained, False)):
            if ck is not None:
                ckpt = torch.load(ck, map_location=self.device, weights_only=False) if isinstance(ck, (str, os.PathLike)) else ck
                self._load(ckpt, full)
        nb = trainer.n_batches
        self.cur_iter = (self.epoch_start - 1) * nb + self.batch_start
        append = resume is not None
        self.val = held_out_batches(val, self.device, trainer.batch_size)
        self.has_val = len(self.val) > 0
        self.train_metrics = Metrics(['time/img'] + list(self.model.loss_names), os.path.join(self.run_dir, 'train_metrics.tsv'), append, self.cur_iter)
        names = [f'alpha{k}' for k in range(self.model.n_blocks)] + (['val_PSNR', 'val_SSIM'] if self.has_val else [])
        self.val_metrics = Metrics(names, os.path.join(self.run_dir, 'val_metrics.tsv'), append, self.cur_iter)
        self.meter = DeviceMeter(self.model.loss_names, self.device)
        self.loggers = {}
        if images:
            if viz is None:
                viz = next(iter(self.val))[0] if self.has_val else trainer.views
            self.viz = {k: (v[:N_VIZ_SAMPLES].to(self.device) if torch.is_tensor(v) else v) for k, v in viz.items()}
            for name in ('reconstructions', 'reconstructions_hard', 'reconstructions_syn'):
                self.loggers[name] = ImageLogger(os.path.join(self.run_dir, name), self.viz['imgs'], 'png', queue_depth=queue_depth)
            self.loggers['txt_blocks'] = ImageLogger(os.path.join(self.run_dir, 'txt_blocks'), None, 'png', queue_depth=queue_depth)
        self._t_tick, self._n_img = None, 0
        trainer.recorder = self

    # ---- checkpoints
    def _load(self, ckpt, full):
        t = self.trainer
        if not full:
            self.model.load_state_dict(ckpt['model_state'])
            return
        self.epoch_start, self.batch_start = load_checkpoint(t, ckpt)

    def state_dict(self, epoch, batch):
        t = self.trainer
        run_state = {'perm_state': t._perm_gen.get_state(), 'order': None if self._order is None else self._order.clone(), 'batch': batch,
                     'n_iters': t.n_iters}
        return dict(t.state_dict(), epoch=epoch, batch=batch, run_state=run_state)

    def save(self, epoch, batch, name='model.pkl'):
        """Written to a temporary name, then renamed: a crash leaves the previous file or the new one, never half of one."""
        path = os.path.join(self.run_dir, name)
        torch.save(self.state_dict(epoch, batch), path + '.tmp')
        os.replace(path + '.tmp', path)
        return path

    # ---- the trainer's calls
    def begin_run(self):
        self.log_images(self.cur_iter)
        self._t_tick, self._n_img = time.perf_counter(), 0

    def begin_epoch(self, order):
        self._order = order

    def after_step(self, epoch, batch, losses, view_ids):
        n = int(view_ids.numel())
        self.meter.add({f'loss_{k}': v for k, v in losses.items()}, n, self.cur_iter)
        self._n_img += n
        if self.trace is not None:
            self.trace.append((epoch, batch, tuple(view_ids.tolist()), tuple(self.trainer.step_fn.lrs), self.trainer.step_fn.n_steps))
        it = self.cur_iter
        if it % self.train_stat_interval == 0:
            self.log_train(it, epoch, batch)
        if it % self.val_stat_interval == 0:
            self.log_val(it, epoch, batch)
            self.log_images(it)
            self.save(epoch, batch)
        self.cur_iter += 1

    def after_epoch(self, epoch):
        if epoch in self.save_epoches:
            self.save(epoch, self.trainer.n_batches, name=f'model_{epoch}.pkl')

    def log_train(self, it, epoch, batch):
        avg, bad = self.meter.read_reset()                      # (the wait: what was enqueued up to here has run)
        now = time.perf_counter()
        t_img = (now - self._t_tick) / max(self._n_img, 1) if self._t_tick is not None else 0.0
        self._t_tick, self._n_img = now, 0
        self.train_metrics.log(it, epoch, batch, [t_img] + [avg[k] for k in self.model.loss_names])
        if bad is not None:
            raise FloatingPointError(f'a loss was not finite at iteration {bad} (found at the tick of iteration {it}): the run stops here')

    @torch.no_grad()
    def val_scores(self):
        """-> (2,) fp64 on the device: mean PSNR and mean SSIM over the held-out views, of the hard 4x supersampled render of the joined
        scene (what quantitative_eval renders), scored per view by ops.image_scores.  No host read."""
        m = self.model
        was_training = m.training
        m.eval()
        scene = m.build_scene(filter_transparent=True)
        psnr, ssim = [], []
        for inp, _ in self.val:
            m._ensure_cameras(inp)
            rec = m.renderer.render_packed(scene, inp['R'], inp['T'], viz_purpose=True)[:, :3]
            mse, s = ops.image_scores(inp['imgs'], rec, padding=False)
            psnr.append(-10.0 * torch.log10(mse))
            ssim.append(s)
        m.train(was_training)
        return torch.stack([torch.cat(psnr).mean(), torch.cat(ssim).mean()])

    def log_val(self, it, epoch, batch):
        vals = self.model.get_opacities().detach().double()
        if self.has_val:
            vals = torch.cat([vals, self.val_scores()])
        vals = vals.tolist()                                    # the one host read of the tick
        nb = self.model.n_blocks
        if not any(a > 0.01 for a in vals[:nb]):
            raise RuntimeError('No more blocks....')           # trainer.py:152-154
        self.val_metrics.log(it, epoch, batch, vals)

    @torch.no_grad()
    def log_images(self, it=None):
        """The four image logs (trainer.py:177-199) of the viz views: evolution/{it}, or final.png without `it`."""
        if not self.loggers:
            return
        m = self.model
        was_training = m.training
        m.eval()
        self.loggers['reconstructions'].save(m.predict(self.viz, None, w_edges=True), it)
        self.loggers['reconstructions_hard'].save(m.predict(self.viz, None, filter_transparent=True), it)
        self.loggers['reconstructions_syn'].save(m.predict_synthetic(self.viz, None), it)
        self.loggers['txt_blocks'].save(self._arranged_block_txt(), it)
        m.train(was_training)

    def _arranged_block_txt(self):
        """model.get_arranged_block_txt (rows of 5 maps, dbw.py:433-438); a model of fewer than 5 blocks, which has no full row, gets one
        row of all its maps."""
        m = self.model
        if m.n_blocks >= 5:
            return m.get_arranged_block_txt()
        maps = torch.sigmoid(m.textures.detach()).permute(0, 3, 1, 2)
        return torch.cat(list(maps), dim=2)[None].contiguous()

    def finish(self):
        """The end of a run (trainer.py:131-133,211-239): the last model.pkl, the plots, final.png and the videos."""
        t = self.trainer
        self.save(t.epoch - 1, t.n_batches)
        self.save_plots()
        self.log_images(None)
        for lg in self.loggers.values():
            lg.save_video()
        self.close()

    def save_plots(self):
        try:
            import matplotlib
            matplotlib.use('Agg')
            import matplotlib.pyplot as plt
        except ImportError:
            print('matplotlib is not installed: loss.pdf and opacity.pdf are skipped')
            return
        for metrics, key, title, name in ((self.train_metrics, 'loss', 'Loss', 'loss.pdf'), (self.val_metrics, 'alpha', 'Opacity', 'opacity.pdf')):
            log = metrics.read_log()
            cols = [c for c in log if key in c]
            if not log['iteration'] or not cols:
                continue
            fig, ax = plt.subplots(figsize=(10, 5))
            for c in cols:
                ax.plot(log['iteration'], log[c], label=c)
            ax.set_title(title)
            ax.set_xlabel('iteration')
            ax.legend(fontsize='small', ncol=2)
            fig.savefig(os.path.join(self.run_dir, name))
            plt.close(fig)

    def close(self):
        for lg in self.loggers.values():
            lg.close()
