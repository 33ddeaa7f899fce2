"""The step either side of the render path: learning-rate schedule, optimisation loop and
checkpointing with the semantics of the reference's src/scheduler.py:26-69, src/optimizer.py:6-18 and
src/trainer.py:109-169,201-209, driving `ShardedTrainStep` (flat parameter buffer, fused Adam, optional RCCL all-reduce).

Host-side scalars only; nothing here touches pixels.  The record of a run -- metric files, image logs, checkpoints, resuming -- is
runlog.RunRecorder's, which this loop calls when one is attached (`trainer.recorder`); without one the loop is what it was.  `evaluate`
ends a run like the reference's trainer.py:241-272."""
import time
from collections import Counter, OrderedDict

import torch

from .parallel import ShardedTrainStep, shard_views


class MultiStepLR:
    """Per-group learning rates, stepped once per EPOCH (trainer.py:127,163-169).  Reproduces the reference's chainable
    recurrence including its warm-up quirk (the constructor divides the freshly set warm-up lr by `warmup` once more,
    scheduler.py:41-46): pinned by tests/golden/lr_schedule.npz."""

    def __init__(self, base_lrs, milestones=None, gamma=0.1, warmup=0):
        self.base_lrs = [float(x) for x in base_lrs]
        self.milestones = Counter(milestones or [])
        self.gamma = [gamma] * len(self.base_lrs) if isinstance(gamma, float) else list(gamma)
        self.warmup = warmup
        self.last_epoch = 0
        self.lrs = self._next(list(self.base_lrs))
        if warmup > 0:
            self.lrs = [lr / warmup for lr in self.lrs]

    def _next(self, lrs):
        if self.warmup > self.last_epoch:
            return [lr / self.warmup * (self.last_epoch + 1) for lr in self.base_lrs]
        if self.last_epoch not in self.milestones:
            return lrs
        return [lr * g ** self.milestones[self.last_epoch] for lr, g in zip(lrs, self.gamma)]

    def step(self):
        self.last_epoch += 1
        self.lrs = self._next(self.lrs)
        return self.lrs

    def get_last_lr(self):
        return list(self.lrs)

    def state_dict(self):
        return {'last_epoch': self.last_epoch, 'lrs': list(self.lrs)}

    def load_state_dict(self, state):
        """Own state ({'last_epoch', 'lrs'}) or the state_dict of the reference's torch scheduler (src/scheduler.py: 'last_epoch',
        '_last_lr', '_step_count', ...): there the decayed rates are read from '_last_lr', or replayed from the base rates and the
        milestones when that key is missing too -- never left at the base values past a milestone."""
        self.last_epoch = int(state['last_epoch'])
        if 'lrs' in state:
            self.lrs = [float(x) for x in state['lrs']]
        elif '_last_lr' in state and len(state['_last_lr']) == len(self.base_lrs):
            self.lrs = [float(x) for x in state['_last_lr']]
        else:
            target, self.last_epoch = self.last_epoch, 0
            self.lrs = self._next(list(self.base_lrs))
            if self.warmup > 0:
                self.lrs = [lr / self.warmup for lr in self.lrs]
            while self.last_epoch < target:
                self.step()


class _RefinedLoader:
    """A loader over the training views in their order, with R, T replaced by the refined poses (Trainer.evaluate)."""

    def __init__(self, loader, R, T):
        self.loader, self.R, self.T = loader, R, T
        self.dataset, self.batch_size = loader.dataset, loader.batch_size

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        a = 0
        for inp, labels in self.loader:
            n = len(inp['R'])
            yield dict(inp, R=self.R[a:a + n].to(inp['R'].device), T=self.T[a:a + n].to(inp['T'].device)), labels
            a += n


class Trainer:
    """cfg: the reference's YAML dict (`model`, `training.{batch_size, optimizer, scheduler, n_epoches, seed}`).
    views: dict of tensors {'imgs' (V,3,H,W), 'R' (V,3,3), 'T' (V,3), 'K' (V,4,4)} resident on the device (the reference's
    DataLoader yields the same dict batch by batch, trainer.py:118,141); every key is batched alike, so the 'masks' (V,1,H,W) of a scene with
    validity masks (dataset.py) ride along, and each batch then carries 'mask_sum', the sum of its masks as a host number."""

    def __init__(self, cfg, model, views, process_group=None, sync_free=True, cache_perceptual_targets=True):
        tr = cfg['training']
        opt = dict(tr.get('optimizer') or {})
        if opt.pop('name', 'adam') != 'adam':
            raise NotImplementedError('only Adam (the optimiser of every shipped config, default.yml:31) is fused')
        txt = dict(opt.pop('texture', {}) or {})
        lr = opt.pop('lr', 1e-3)
        lr_txt = txt.pop('lr', lr)
        sch = dict(tr.get('scheduler') or {})
        if sch.pop('name', 'multi_step') != 'multi_step':
            raise NotImplementedError('only the multi_step scheduler')
        self.cfg, self.model, self.views = cfg, model, views
        self.recorder = None                # runlog.RunRecorder attaches itself here
        self._resume_pos = None             # (view order, batches done) of an epoch a resumed run re-enters: set by the recorder
        model.sync_free = sync_free
        self.step_fn = ShardedTrainStep(model, lr=lr, lr_texture=lr_txt, betas=opt.pop('betas', (0.9, 0.999)), eps=opt.pop('eps', 1e-8),
                                        process_group=process_group, seed=tr.get('seed'))
        if opt or txt:       # the reference forwards these to torch.optim.Adam (optimizer.py:9-18); the fused kernel implements plain Adam
            raise NotImplementedError(f'optimizer options not supported by the fused Adam: {sorted(opt) + ["texture." + k for k in sorted(txt)]}')
        self.scheduler = MultiStepLR([lr, lr_txt], **sch)
        self.step_fn.lrs = tuple(self.scheduler.get_last_lr())
        self.batch_size = tr.get('batch_size', 4)
        self.n_epoches = tr.get('n_epoches', 1)
        self.epoch, self.n_iters, self.time_per_img = 1, 0, 0.0
        V, ws = views['imgs'].shape[0], self.step_fn.world_size
        a, b = shard_views(V, ws, self.step_fn.rank)
        self.local = {k: v[a:b] for k, v in views.items()}
        self.shard_sizes = [shard_views(V, ws, r)[1] - shard_views(V, ws, r)[0] for r in range(ws)]
        self.n_batches = -(-max(self.shard_sizes) // self.batch_size)          # every rank runs this many steps per epoch
        self.per_view = views['imgs'][0].numel() if V else 0
        self._perm_gen = torch.Generator().manual_seed(int(tr.get('seed') or 0))
        # The perceptual criterion's target half is a constant per training view (frozen network, fixed images): a criterion that can keep
        # it (lpips_vgg.LPIPSVGG.cache_targets) computes it once for this rank's views, if that fits in a quarter of the free memory, and
        # every batch then carries the local indices of its views.  A third of the criterion's FLOPs; the values do not change.
        self.view_ids = False
        # Camera pose refinement (training.pose_refine: {lr, start_epoch, rot, trans}; pose.py): absent -> nothing is built and
        # no batch changes.  Present -> batches carry view_ids, their R, T go through the refiner from start_epoch on, and its Adam step
        # follows the model's.  `scene`: the training scene, for the files evaluate() writes (train.main sets it).
        self.pose, self.pose_cfg, self.scene = None, None, None
        from .pose import PoseRefiner, parse_config
        self.pose_cfg = parse_config(tr.get('pose_refine'))
        if self.pose_cfg is not None:
            if ws > 1:
                raise NotImplementedError('training.pose_refine under data parallelism: the pose gradients are per view and the ranks do not '
                                          'exchange them')
            self.pose = PoseRefiner(self.local['imgs'].shape[0], self.local['imgs'].device, lr=self.pose_cfg['lr'],
                                    betas=tuple((tr.get('optimizer') or {}).get('betas', (0.9, 0.999))), rot=self.pose_cfg['rot'],
                                    trans=self.pose_cfg['trans'])
        # Per-view exposure compensation (training.exposure: {lr, start_epoch, bias, center}; exposure.py): absent -> nothing
        # is built and no batch changes.  Present -> batches carry view_ids and, from start_epoch on, 'exposure' = theta; the refiner's
        # Adam step follows the model's.
        self.exposure, self.exposure_cfg = None, None
        from .exposure import ExposureRefiner, parse_config as parse_exposure
        self.exposure_cfg = parse_exposure(tr.get('exposure'))
        if self.exposure_cfg is not None:
            if ws > 1:
                raise NotImplementedError('training.exposure under data parallelism: the exposure gradients are per view and the ranks do '
                                          'not exchange them')
            self.exposure = ExposureRefiner(self.local['imgs'].shape[0], self.local['imgs'].device, lr=self.exposure_cfg['lr'],
                                            betas=tuple((tr.get('optimizer') or {}).get('betas', (0.9, 0.999))), bias=self.exposure_cfg['bias'],
                                            center=self.exposure_cfg['center'])
        # Intrinsics refinement (training.intrinsics_refine: {lr, start_epoch, focal, principal}; intrinsics.py): absent ->
        # nothing is built and no batch changes.  Present -> from start_epoch on batches carry 'K_live', the refined K with a gradient to
        # theta, and the refiner's Adam step follows the model's.
        self.intrinsics, self.intrinsics_cfg = None, None
        from .intrinsics import IntrinsicsRefiner, parse_config as parse_intrinsics
        self.intrinsics_cfg = parse_intrinsics(tr.get('intrinsics_refine'))
        if self.intrinsics_cfg is not None:
            if ws > 1:
                raise NotImplementedError('training.intrinsics_refine under data parallelism: the ranks do not exchange the gradient of K')
            if 'K' not in views:
                raise KeyError("training.intrinsics_refine: the views carry no 'K', the matrix to refine")
            self.intrinsics = IntrinsicsRefiner(views['K'][0], views['imgs'].device, lr=self.intrinsics_cfg['lr'],
                                                betas=tuple((tr.get('optimizer') or {}).get('betas', (0.9, 0.999))),
                                                focal=self.intrinsics_cfg['focal'], principal=self.intrinsics_cfg['principal'])
        # The surface term (model.loss.surface_weight) is one term on the whole cloud: every rank would add all of it
        if 'surface' in getattr(model, 'loss_weights', {}) and ws > 1:
            raise NotImplementedError('model.loss.surface_weight under data parallelism: every rank would add the whole term, and the ranks '
                                      'do not share out its points')
        # ... and so is the free-space term (model.loss.freespace_weight) on the capture's depth rays
        if 'freespace' in getattr(model, 'loss_weights', {}) and ws > 1:
            raise NotImplementedError('model.loss.freespace_weight under data parallelism: every rank would add the whole term, and the ranks '
                                      'do not share out its rays')
        # Validity masks ride along like every key of `views`; the sum of each view's mask is taken once, here (one host copy, fp64), so
        # that a batch carries its valid count as a host number ('mask_sum') and no step reads the device for it
        self.mask_sums = None
        if 'masks' in self.local:
            self.mask_sums = self.local['masks'].to(torch.float64).flatten(1).sum(1).cpu()
        fn = getattr(model, 'perceptual_fn', None)
        if (cache_perceptual_targets and 'perceptual' in getattr(model, 'loss_weights', {}) and hasattr(fn, 'cache_targets') and self.local['imgs'].is_cuda
                and self.local['imgs'].shape[0] > 0):
            need = fn.target_bytes(*self.local['imgs'].shape[2:], n_views=self.local['imgs'].shape[0])
            if need <= torch.cuda.mem_get_info(self.local['imgs'].device)[0] // 4:
                fn.cache_targets(self._perceptual_targets())
                self.view_ids = True
        self._cached_targets = self.view_ids        # (view_ids may also be on for the pose refiner alone: no cache to keep then)
        self.view_ids = self.view_ids or self.pose is not None or self.exposure is not None

    def _perceptual_targets(self):
        """What a caching criterion keeps the features of: this rank's images, times their masks where the views have them (the model calls
        such a criterion on imgs * masks).  The product is made once and kept: the criterion recognises its cache by the tensor."""
        if 'masks' not in self.local:
            return self.local['imgs']
        if getattr(self, '_masked_targets', None) is None:
            self._masked_targets = self.local['imgs'] * self.local['masks']
        return self._masked_targets

    # trainer.py:137-147
    def run_single_batch_train(self, inp, global_count=None):
        t0 = time.time()
        self.model.train()
        losses = self.step_fn(inp, global_count=global_count)
        self.n_iters += 1
        return losses, t0

    def global_count(self, batch):
        """Image elements of mini-batch `batch` over ALL ranks -- every rank derives it from the shard sizes, no collective."""
        bs = self.batch_size
        return self.per_view * sum(min(bs, max(0, v - batch * bs)) for v in self.shard_sizes)

    def run_epoch(self, shuffle=True):
        """One pass over this rank's views in mini-batches (DataLoader(shuffle=True) equivalent), then the per-epoch
        scheduler / model step (trainer.py:127,163-169).  A run resumed inside an epoch walks the rest of that epoch's order."""
        V = self.local['imgs'].shape[0]
        first = 0
        if self._resume_pos is not None:
            (order, first), self._resume_pos = self._resume_pos, None
        else:
            order = torch.randperm(V, generator=self._perm_gen) if shuffle else torch.arange(V)
        rec = self.recorder
        if rec is not None:
            rec.begin_epoch(order)
        if self._cached_targets:
            # the criterion is shared by whoever holds the model: if its cache is not (or no longer) the one of THESE views -- new weights,
            # another Trainer on other views -- the ids would index foreign features; built again (a forward pass over the views, once)
            fn = self.model.perceptual_fn
            targets = self._perceptual_targets()
            if not (hasattr(fn, 'cache_matches') and fn.cache_matches(targets)):
                fn.cache_targets(targets)
        last = None
        t_start, n_img = time.time(), 0
        # Uneven shards (49 views over 8 ranks: 7,6,...,6; batch 4 -> two steps everywhere, the second of sizes 3,2,...,2): all ranks
        # run n_batches steps -- a rank that has run out of views steps on an EMPTY batch (regularisers only) -- so that the
        # sequence of collectives is the same everywhere, and the MSE normalisation of a step is the size of its global batch
        for b in range(first, self.n_batches):
            ids = order[b * self.batch_size:(b + 1) * self.batch_size]
            idx = ids.to(self.local['imgs'].device)
            batch = {k: v[idx] for k, v in self.local.items()}
            if self.view_ids:
                batch['view_ids'] = idx
            if self.pose is not None or self.exposure is not None:
                batch['view_ids_host'] = ids                      # (the refiners check the ids without waiting for the device)
            if self.mask_sums is not None:
                batch['mask_sum'] = float(self.mask_sums[ids].sum())
            refine = self.pose is not None and self.epoch >= self.pose_cfg['start_epoch'] and idx.numel() > 0
            if refine:
                batch = self.pose.apply(batch)
            expose = self.exposure is not None and self.epoch >= self.exposure_cfg['start_epoch'] and idx.numel() > 0
            if expose:
                batch = self.exposure.attach(batch)
            focal = self.intrinsics is not None and self.epoch >= self.intrinsics_cfg['start_epoch'] and idx.numel() > 0
            if focal:
                batch = self.intrinsics.apply(batch)
            last, _ = self.run_single_batch_train(batch, self.global_count(b))
            if refine:
                self.pose.step()
            if expose:
                self.exposure.step()
            if focal:
                self.intrinsics.step()
            n_img += idx.numel()
            if rec is not None:
                rec.after_step(self.epoch, b + 1, last, ids)
        if self.local['imgs'].is_cuda:
            torch.cuda.synchronize()
        self.time_per_img = (time.time() - t_start) / max(n_img, 1)
        self.step_fn.lrs = tuple(self.scheduler.step())
        self.model.step()
        self.epoch += 1
        opac = self.model.get_opacities()
        if (opac > 0.01).sum() == 0:
            raise RuntimeError('No more blocks....')                   # trainer.py:152-154
        if rec is not None:
            rec.after_epoch(self.epoch - 1)
        return last

    def run(self, n_epoches=None):
        last = None
        rec = self.recorder
        if rec is None:
            for _ in range(self.epoch, (n_epoches or self.n_epoches) + 1):
                last = self.run_epoch()
            return last
        try:
            rec.begin_run()
            for _ in range(self.epoch, (n_epoches or self.n_epoches) + 1):
                last = self.run_epoch()
            rec.finish()
        except BaseException:
            try:                            # the writer threads end with the run, however it ends -- and the run's own error is the one raised
                rec.close()
            except Exception:
                pass
            raise
        return last

    # trainer.py:241-272
    def evaluate(self, loader, run_dir, dtu=None, aligned=None, parse=False, masks=None):
        """The end of a run: qualitative_eval into run_dir/quali_eval, quantitative_eval (hard inference) into run_dir/final_scores.tsv
        (a line of names, a line of values, '{:.5f}'), and -- dtu = dict(scale_mat=, scan_id=, dataset_dir=), further keywords of
        eval3d.evaluate_dtu allowed -- the official DTU scores of the blocks into run_dir; aligned = dict(points=, normals=), further
        keywords of eval3d.evaluate_aligned allowed -- the ICP-aligned Chamfer / normal scores against a ground-truth cloud in any frame
        into run_dir/aligned_scores.tsv.  parse=True: the scene parsing maps of the inputs into run_dir/quali_eval/parse
        (model.parse_views, export.write_parse).  masks: ground-truth foreground masks of ALL views of the loader in its order, (V,H,W) or
        (V,1,H,W), bool or 0 / 1, at the image size -- metrics.ProxyEvaluator scores the parse's foreground() (some block is what the
        pixel shows) against them into run_dir/mask_scores.tsv, written like final_scores.tsv.  loader: an iterable of (inp, labels) that
        can be walked twice (three times with masks).  -> the scores (with the DTU dict under 'dtu', the aligned scores under 'aligned'
        and the mask scores under 'masks' where asked for)."""
        import os
        run_dir = str(run_dir)
        os.makedirs(os.path.join(run_dir, 'quali_eval'), exist_ok=True)
        device = self.views['imgs'].device
        self.model.eval()
        if self.pose is not None:
            from .pose import write_refined
            if self.scene is not None:
                write_refined(self.scene, self.pose, run_dir, self.local['R'], self.local['T'])
            if getattr(loader, 'dataset', None) is not None and loader.dataset is self.scene:
                loader = _RefinedLoader(loader, *self.pose.refined(self.local['R'], self.local['T']))      # the training views: at their refined poses
        if self.intrinsics is not None:
            # the refined K' replaces the frozen one on the four renderers: every render from here on sees it (scores, export, parse)
            from .intrinsics import write_refined as write_intrinsics
            write_intrinsics(self.scene, self.intrinsics, run_dir, self.views['imgs'].shape[2:], after_pose=self.pose is not None and self.scene is not None
                             and getattr(self.scene, 'name', None) == 'custom')
            K1 = self.intrinsics.refined()[None]
            for r in (getattr(self.model, n, None) for n in ('renderer', 'renderer_fine', 'renderer_env', 'renderer_light')):
                if r is not None:
                    r.update_cameras(device=device, K=K1)
        if self.exposure is not None:
            # (the renders below stay uncompensated, at the canonical exposure: a held-out view has no fitted row)
            from .exposure import write_exposures
            write_exposures(self.exposure, run_dir)
        self.model.qualitative_eval(loader, device, path=os.path.join(run_dir, 'quali_eval'), **({'parse': True} if parse else {}))
        scores = self.model.quantitative_eval(loader, device, hard_inference=True)
        with open(os.path.join(run_dir, 'final_scores.tsv'), mode='w') as f:
            f.write('\t'.join(scores.keys()) + '\n')
            f.write('\t'.join('{:.5f}'.format(float(v)) for v in scores.values()) + '\n')
        if masks is not None:
            scores = dict(scores, masks=self._mask_scores(loader, device, masks, run_dir))
        if dtu is not None:
            from .eval3d import evaluate_dtu
            scores = dict(scores, dtu=evaluate_dtu(self.model, eval_dir=run_dir, **dtu))
        if aligned is not None:
            from .eval3d import evaluate_aligned
            scores = dict(scores, aligned=dict(evaluate_aligned(self.model, eval_dir=run_dir, **aligned)))
        return scores

    def _mask_scores(self, loader, device, masks, run_dir):
        """mask_iou of the parsed foreground against `masks` (evaluate's), view by view in the loader's order -> run_dir/mask_scores.tsv."""
        import os
        from .metrics import ProxyEvaluator
        masks = torch.as_tensor(masks)
        masks = masks[:, 0] if masks.dim() == 4 else masks
        if masks.dim() != 3 or tuple(masks.shape[1:]) != tuple(self.model.img_size):
            raise ValueError(f'masks are (V,H,W) or (V,1,H,W) at the image size {tuple(self.model.img_size)}, got {tuple(masks.shape)}')
        ev, seen = ProxyEvaluator(), 0
        for inp, _ in loader:
            inp = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in inp.items()}
            fg = self.model.parse_views(inp).foreground()
            if seen + len(fg) > len(masks):
                raise ValueError(f'{len(masks)} masks for more than {seen + len(fg) - 1} views')
            ev.update(fg.float(), (masks[seen:seen + len(fg)].to(device) != 0).float())
            seen += len(fg)
        if seen != len(masks):
            raise ValueError(f'{len(masks)} masks for {seen} views')
        out = OrderedDict(zip(ev.names, ev.compute()))
        with open(os.path.join(run_dir, 'mask_scores.tsv'), mode='w') as f:
            f.write('\t'.join(out.keys()) + '\n')
            f.write('\t'.join('{:.5f}'.format(float(v)) for v in out.values()) + '\n')
        return out

    # trainer.py:201-209 / 84-107
    def state_dict(self):
        """Same keys as trainer.py:201-209.  'epoch' / 'batch' = the last COMPLETED epoch and its number of batches, like the
        reference's end-of-epoch save, so either trainer resumes the other's checkpoint at the same epoch.  'model_state'
        interchanges; 'scheduler_state' is read in either form (MultiStepLR.load_state_dict takes the torch scheduler's keys too,
        this trainer writes {'last_epoch', 'lrs'}).  'optimizer_state' does NOT interchange: it holds the fused Adam's flat moment
        buffers ({'exp_avg', 'exp_avg_sq', 'n_steps'} in FlatParams order), not a torch.optim.Adam state_dict.  Under data
        parallelism 'batch' counts this trainer's batches per epoch, ceil(largest shard / batch_size), not the reference's
        len(loader) over all views: the reference would take such a checkpoint for a mid-epoch one."""
        return {'epoch': self.epoch - 1, 'batch': self.n_batches, 'model_name': self.model.name, 'model_kwargs': self.model.init_kwargs,
                'model_state': {k: v.detach().clone() for k, v in self.model.state_dict().items()},
                'optimizer_state': {'exp_avg': self.step_fn.exp_avg.clone(), 'exp_avg_sq': self.step_fn.exp_avg_sq.clone(),
                                    'n_steps': self.step_fn.n_steps},
                'scheduler_state': self.scheduler.state_dict(), **({} if self.pose is None else {'pose_refine': self.pose.state_dict()}),
                **({} if self.exposure is None else {'exposure': self.exposure.state_dict()}),
                **({} if self.intrinsics is None else {'intrinsics_refine': self.intrinsics.state_dict()})}

    def load_state_dict(self, ckpt):
        self.model.load_state_dict(ckpt['model_state'])
        o = ckpt['optimizer_state']
        if 'exp_avg' not in o:
            raise KeyError("optimizer_state is not a fused-Adam state ({'exp_avg', 'exp_avg_sq', 'n_steps'}): a reference checkpoint's "
                           'torch.optim.Adam state_dict cannot be loaded; load its model_state / scheduler_state and restart the moments')
        self.step_fn.exp_avg.copy_(o['exp_avg'])
        self.step_fn.exp_avg_sq.copy_(o['exp_avg_sq'])
        self.step_fn.n_steps = o['n_steps']
        self.scheduler.load_state_dict(ckpt['scheduler_state'])
        self.step_fn.lrs = tuple(self.scheduler.get_last_lr())
        self.epoch = ckpt['epoch'] + 1                         # trainer.py:94-97: resume with the epoch after the saved one
        self.model.set_cur_epoch(ckpt['epoch'])
        if self.pose is not None and 'pose_refine' in ckpt:
            self.pose.load_state_dict(ckpt['pose_refine'])
        if self.exposure is not None and 'exposure' in ckpt:
            self.exposure.load_state_dict(ckpt['exposure'])
        if self.intrinsics is not None and 'intrinsics_refine' in ckpt:
            self.intrinsics.load_state_dict(ckpt['intrinsics_refine'])
