"""python -m dbw_amd.train --config C --tag T --data-root D --runs-root R [--epochs N]
                          [--lpips-vgg F --lpips-lin F | --perceptual ssim | --no-perceptual] [--resume [TAG]] [--no-record]
                          [--pose-refine LR] [--blocks-init points] [--exposure LR] [--intrinsics-refine LR] [--surface WEIGHT]
                          [--freespace WEIGHT]

A run of one of the reference's configs, end to end, as its src/trainer.py:275-295 starts one: the config is loaded (the default.yml next
to it, then the file), the scenes of cfg['dataset'] (dtu, bmvs or custom) are read from <data-root>, the model is built from cfg['model'], trained by Trainer,
saved as <runs-root>/<dataset>/<tag>/model.pkl (Trainer.state_dict) and evaluated by Trainer.evaluate on the test split -- for a DTU scan
whose evaluation data (ObsMask/, Points/stl/) lies under <data-root>/DTU, the official scores too.

The run is recorded as the reference records it (runlog.RunRecorder: train_metrics.tsv, val_metrics.tsv with the scores of the validation
split, the image logs, model.pkl at every validation tick, model_<epoch>.pkl at training.save_epoches); --no-record trains without and
writes model.pkl at the end only.  training.resume: TAG (or --resume [TAG], default: this run's tag) continues the run of
<runs-root>/<dataset>/<TAG>/model.pkl where it stopped; training.pretrained: TAG starts from that run's weights.

model.mesh.R_world: auto (T_world: auto and S_world: auto beside it) on a custom scene with a point cloud: the three entries are estimated from
the cloud and the cameras (worldfit.estimate_world_frame), printed and written to <run_dir>/world_frame.yml before the model is built.

The perceptual term needs the weights of a VGG16 and of the LPIPS heads, which do not ship with the package: a config with
perceptual_weight > 0 is refused unless both files are given, or --no-perceptual sets the weight to 0 (and says so).  With
model.loss.perceptual_name: ssim -- or --perceptual ssim, which overrides the config's key -- the term is the built-in SSIM term
(metrics.SSIMTerm) and needs no file; giving the LPIPS weight files beside it is refused as a contradiction.

training.pose_refine: {lr, start_epoch, rot, trans} -- or --pose-refine LR -- refines the camera poses of the training views beside the model
(pose.py); the refined poses are written to <run_dir>/transforms_refined.json (custom captures) or poses_refined.npz at the end.

training.intrinsics_refine: {lr, start_epoch, focal, principal} -- or --intrinsics-refine LR -- refines the pinhole matrix the views share
beside the model (intrinsics.py): by default one scale of both focal lengths; the evaluation renders with the refined matrix,
which is written to <run_dir>/intrinsics_refined.yml and, for a capture without lens coefficients, into <run_dir>/transforms_refined.json.

training.exposure: {lr, start_epoch, bias, center} -- or --exposure LR -- fits a gain and an offset per colour channel and training view beside
the model (exposure.py): both image terms see exp(g) * render + b; the fitted values are written to <run_dir>/exposures.tsv at
the end, and the evaluation renders stay at the canonical exposure.

training.blocks_init: points -- or --blocks-init points, or the mapping {oversample, min_points, n_iter, ground_margin, extent_scale} -- on a
custom scene with a point cloud: the blocks start at the clusters of the cloud (worldfit.blocks_from_points: k-means and a PCA of every
cluster, on the device) and no longer at random poses; how many were seeded is printed and the poses are written to
<run_dir>/blocks_init.yml.  A resumed or pretrained start skips the fit: the checkpoint carries the blocks.

dataset.cloud: depth -- or the mapping {source: depth, unit, range, grid, bound, stride, edge, min_count} -- on a custom scene whose frames
ship depth maps and no .ply: the cloud both fits above use is made from the depth maps (ops.depth_cloud), its size is
printed and it is written to <run_dir>/depth_cloud.ply.

model.loss.surface_weight -- or --surface WEIGHT -- with model.loss.surface: {points, tau, back, ground, start_epoch, max_cloud} on a custom
scene with a point cloud: the surface term keeps the blocks on the cloud during training, loss_surface is a column of
train_metrics.tsv.  The steps then take the general path (the one-call C step stands aside, as for masks).

model.loss.freespace_weight -- or --freespace WEIGHT -- with model.loss.freespace: {rays, tau, margin, ground, start_epoch, max_rays} on a
custom scene with depth maps (dataset.cloud: depth): the free-space term pushes the blocks out of the space the depth rays
crossed on their way to the measured surface, loss_freespace is a column of train_metrics.tsv.  The general path, as above."""
import argparse
import os
import sys

import torch


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m dbw_amd.train', description='Train and evaluate a model specified by one of the YAML configs')
    ap.add_argument('-c', '--config', required=True, help='config file (its default.yml is looked up next to it)')
    ap.add_argument('-d', '--default', default=None, help='default config file, instead of the default.yml next to --config')
    ap.add_argument('-t', '--tag', required=True, help='run tag: the run directory is <runs-root>/<dataset name>/<tag>')
    ap.add_argument('--data-root', required=True, help='the directory that holds DTU/, BlendedMVS/ and custom/ (custom/<tag>/transforms.json: a capture of your own)')
    ap.add_argument('--runs-root', required=True)
    ap.add_argument('--epochs', type=int, default=None, help='override training.n_epoches')
    ap.add_argument('--lpips-vgg', default=None, help="state dict of torchvision's vgg16().features (torch.save)")
    ap.add_argument('--lpips-lin', default=None, help="state dict with lpips' lin{k}.model.1.weight tensors (torch.save)")
    ap.add_argument('--perceptual', choices=('lpips', 'ssim'), default=None,
                    help="the perceptual term, overriding model.loss.perceptual_name: 'ssim' is built in and needs no weight files")
    ap.add_argument('--no-perceptual', action='store_true', help='train without the perceptual term')
    ap.add_argument('--resume', nargs='?', const=True, default=None, metavar='TAG', help="continue the run TAG of this dataset (default: --tag's own run)")
    ap.add_argument('--no-record', action='store_true', help='no metric files, image logs or checkpoints during the run: model.pkl at the end only')
    ap.add_argument('--pose-refine', type=float, default=None, metavar='LR',
                    help='refine the camera poses of the training views beside the model, with this learning rate (training.pose_refine.lr)')
    ap.add_argument('--intrinsics-refine', type=float, default=None, metavar='LR',
                    help='refine the shared focal scale of the views beside the model, with this learning rate (training.intrinsics_refine.lr)')
    ap.add_argument('--exposure', type=float, default=None, metavar='LR',
                    help='fit a per-view exposure (gain and offset per channel) beside the model, with this learning rate (training.exposure.lr)')
    ap.add_argument('--blocks-init', choices=('points',), default=None,
                    help="'points': start the blocks at the clusters of the custom scene's point cloud (training.blocks_init)")
    ap.add_argument('--surface', type=float, default=None, metavar='WEIGHT',
                    help="keep the blocks on the custom scene's point cloud: the weight of the surface term (model.loss.surface_weight)")
    ap.add_argument('--freespace', type=float, default=None, metavar='WEIGHT',
                    help="keep the blocks out of the space the custom scene's depth rays crossed: the weight of the free-space term "
                         '(model.loss.freespace_weight)')
    ap.add_argument('--device', default='cuda:0')
    return ap.parse_args(argv)


def prepare_config(args):
    """The config of a run, with the perceptual term settled: kept (the built-in SSIM term, or LPIPS with both weight files given), dropped
    (--no-perceptual) or refused."""
    from .dataset import load_config
    cfg = load_config(args.config, args.default)
    loss = cfg.get('model', {}).get('loss', {})
    if getattr(args, 'perceptual', None) is not None:
        loss['perceptual_name'] = args.perceptual
    if (loss.get('perceptual_weight') or 0) > 0:
        if args.no_perceptual:
            print(f"--no-perceptual: perceptual_weight {loss['perceptual_weight']} -> 0, the run optimises the other terms only")
            loss['perceptual_weight'] = 0
        elif loss.get('perceptual_name', 'lpips') == 'ssim':
            if args.lpips_vgg or args.lpips_lin:
                raise SystemExit(f'{args.config}: perceptual_name = ssim is the built-in SSIM term and loads no weights: --lpips-vgg / --lpips-lin '
                                 'contradict it (drop them, or give --perceptual lpips)')
        elif not (args.lpips_vgg and args.lpips_lin):
            raise SystemExit(f"{args.config}: perceptual_weight = {loss['perceptual_weight']} needs the LPIPS network's weights, which do not "
                             'ship with this package: give --lpips-vgg and --lpips-lin, or --no-perceptual to train without the term, or '
                             '--perceptual ssim for the built-in SSIM term')
    if args.epochs is not None:
        cfg.setdefault('training', {})['n_epoches'] = args.epochs
    if getattr(args, 'pose_refine', None) is not None:
        entry = cfg.setdefault('training', {}).get('pose_refine')
        cfg['training']['pose_refine'] = dict(entry if isinstance(entry, dict) else {}, lr=args.pose_refine)
    if getattr(args, 'intrinsics_refine', None) is not None:
        entry = cfg.setdefault('training', {}).get('intrinsics_refine')
        cfg['training']['intrinsics_refine'] = dict(entry if isinstance(entry, dict) else {}, lr=args.intrinsics_refine)
    if getattr(args, 'exposure', None) is not None:
        entry = cfg.setdefault('training', {}).get('exposure')
        cfg['training']['exposure'] = dict(entry if isinstance(entry, dict) else {}, lr=args.exposure)
    if getattr(args, 'surface', None) is not None:
        cfg.setdefault('model', {}).setdefault('loss', {})['surface_weight'] = args.surface
    if getattr(args, 'freespace', None) is not None:
        cfg.setdefault('model', {}).setdefault('loss', {})['freespace_weight'] = args.freespace
    if getattr(args, 'blocks_init', None) is not None and not isinstance(cfg.setdefault('training', {}).get('blocks_init'), dict):
        cfg['training']['blocks_init'] = args.blocks_init      # (a mapping in the config already asks for the points, with its options)
    return cfg


WORLD_KEYS = ('R_world', 'T_world', 'S_world')


def wants_world_frame(cfg):
    """True where model.mesh says `R_world: auto` (T_world: auto and S_world: auto are accepted beside it, and only beside it)."""
    mesh = cfg.get('model', {}).get('mesh') or {}
    autos = [k for k in WORLD_KEYS if isinstance(mesh.get(k), str)]
    bad = [k for k in autos if mesh[k] != 'auto']
    if bad:
        raise SystemExit(f"model.mesh.{bad[0]}: '{mesh[bad[0]]}' is neither numbers nor 'auto'")
    if autos and 'R_world' not in autos:
        raise SystemExit(f"model.mesh.{autos[0]}: auto goes with R_world: auto (the three are estimated together from the scene's point cloud)")
    return bool(autos)


def resolve_world_frame(cfg, scene, device, run_dir=None, resume=None):
    """Replaces the `auto` entries of cfg['model']['mesh'] by numbers, in place: the three entries of the checkpoint `resume` (a path:
    its model_kwargs carry them, a resumed run does not fit again), or the estimate of scene.world_frame, which is printed and written to
    <run_dir>/world_frame.yml.  A scene without a cloud, and the scale_mat-normalised DTU / BlendedMVS scenes, are refused."""
    if not wants_world_frame(cfg):
        return None
    mesh = cfg['model']['mesh']
    if resume is not None:
        kept = torch.load(resume, map_location='cpu', weights_only=False)['model_kwargs']['mesh']
        mesh.update({k: kept[k] for k in WORLD_KEYS})
        print(f"R_world: auto -> the world frame of {resume}: " + ', '.join(f'{k}={mesh[k]}' for k in WORLD_KEYS))
        return None
    if not hasattr(scene, 'world_frame'):
        raise SystemExit(f"model.mesh.R_world: auto is for custom scenes: a '{scene.name}' scene is normalised by its scale_mat, and the "
                         'R_world, T_world, S_world its config ships with hold')
    try:
        frame = scene.world_frame(device, T_range=mesh.get('T_range', (1, 1, 1)))
    except ValueError as e:
        raise SystemExit(f'model.mesh.R_world: auto: {e}') from e
    mesh.update(frame.mesh_kwargs())
    print(f'R_world: auto -> {frame}')
    if run_dir is not None:
        with open(os.path.join(run_dir, 'world_frame.yml'), 'w') as f:
            f.write(frame.yaml())
    return frame


def resolve_depth_cloud(scene, device, run_dir=None):
    """dataset.cloud: depth -- the cloud of the capture's depth maps is built now (scene.cloud: the fits that follow find it cached), its size
    is printed and, with a run directory, it is written to <run_dir>/depth_cloud.ply -> the points, or None for any other scene."""
    if getattr(scene, 'cloud_options', None) is None:
        return None
    try:
        points = scene.cloud(device)
    except ValueError as e:
        raise SystemExit(f'dataset.cloud: {e}') from e
    info = scene.cloud_info
    print(f"depth_cloud: {info['points']} points from {info['samples']} samples of {info['frames']} frames")
    if run_dir is not None:
        from .export import save_ply
        save_ply(os.path.join(run_dir, 'depth_cloud.ply'), points)
    return points


BLOCKS_INIT_KEYS = ('oversample', 'min_points', 'n_iter', 'ground_margin', 'extent_scale')


def blocks_init_options(cfg):
    """None where training.blocks_init is absent (or null / false), else the keyword arguments it gives worldfit.blocks_from_points: {} for
    `points`, the mapping's entries for a mapping of BLOCKS_INIT_KEYS.  The key lives under `training`: model.mesh refuses keys it does not
    know."""
    entry = (cfg.get('training') or {}).get('blocks_init')
    if entry is None or entry is False:
        return None
    if entry == 'points':
        return {}
    if isinstance(entry, dict):
        bad = [k for k in entry if k not in BLOCKS_INIT_KEYS]
        if bad:
            raise SystemExit(f"training.blocks_init.{bad[0]}: not one of {', '.join(BLOCKS_INIT_KEYS)}")
        return dict(entry)
    raise SystemExit(f"training.blocks_init: '{entry}' is neither 'points' nor a mapping of {', '.join(BLOCKS_INIT_KEYS)}")


def resolve_blocks_init(cfg, scene, model, device, run_dir=None, start=None):
    """training.blocks_init: the blocks of `model` are started at the clusters of the scene's cloud (scene.block_init), the number seeded is
    printed and the poses are written to <run_dir>/blocks_init.yml -> the BlockInit.  With `start` (the checkpoint of a resumed or pretrained
    run, a path) nothing is fitted: the checkpoint carries the blocks.  A scene without a cloud is refused, and so are the DTU / BlendedMVS
    scenes: their cloud is the ground truth the scores are computed against.

    Data parallel: every rank computes the same init from the same cloud -- the fit has no random draw and adds its sums in a fixed order, so
    the ranks start from the same bytes without a broadcast."""
    opts = blocks_init_options(cfg)
    if opts is None:
        return None
    if start is not None:
        print(f'blocks_init: points -> skipped, {start} carries the blocks')
        return None
    if not hasattr(scene, 'block_init'):
        raise SystemExit(f"training.blocks_init is for custom scenes: the cloud of a '{scene.name}' scene is the ground truth its scores are "
                         'computed against, and the blocks must not start from it')
    try:
        init = scene.block_init(model, device, **opts)
    except ValueError as e:
        raise SystemExit(f'training.blocks_init: {e}') from e
    print(f'blocks_init: points -> {len(init)} of {init.n_blocks} blocks seeded from {init.n_points_used} points '
          f'(cluster sizes {[int(c) for c in init.counts.cpu().tolist()]}), the others keep their random draw')
    if run_dir is not None:
        with open(os.path.join(run_dir, 'blocks_init.yml'), 'w') as f:
            f.write(init.yaml())
    return init


def resolve_surface(scene, model, device):
    """model.loss.surface_weight > 0: the model gets the scene's cloud (scene.cloud: the .ply or the depth cloud) for the surface term
     and the number of points it keeps is printed -> that number, or None without the weight.  A custom scene without a cloud is
    refused with the scene's own words, and so are the DTU / BlendedMVS scenes: their cloud is the ground truth the scores are computed
    against.  A resumed run comes here too: a checkpoint does not carry the cloud."""
    if 'surface' not in getattr(model, 'loss_weights', {}):
        return None
    if scene.name != 'custom':
        raise SystemExit(f"model.loss.surface_weight is for custom scenes: the cloud of a '{scene.name}' scene is the ground truth its scores are "
                         'computed against')
    try:
        points = scene.cloud(device)
    except ValueError as e:
        raise SystemExit(f'model.loss.surface_weight: {e}') from e
    n = model.set_surface_points(points)
    c = model.surface_cfg
    print(f"surface: weight {model.loss_weights['surface']:g} on {n} of {len(points)} points, {c['points'] or n} a step, tau {c['tau']:g}, "
          f"back {c['back']:g}, from epoch {c['start_epoch']}")
    return n


def resolve_freespace(scene, model, device):
    """model.loss.freespace_weight > 0: the model gets the scene's depth rays (scene.rays: every depth sample of a capture with
    dataset.cloud: depth, from its camera's centre) for the free-space term and the number it keeps is printed -> that number,
    or None without the weight.  A custom scene without depth maps is refused with the scene's own words, and so are the DTU / BlendedMVS
    scenes: they ship no depth maps, and their cloud is the ground truth the scores are computed against.  A resumed run comes here too: a
    checkpoint does not carry the rays."""
    if 'freespace' not in getattr(model, 'loss_weights', {}):
        return None
    if scene.name != 'custom':
        raise SystemExit(f"model.loss.freespace_weight is for custom scenes with depth maps: a '{scene.name}' scene ships none, and its cloud is "
                         'the ground truth its scores are computed against')
    try:
        ends, frame, origins = scene.rays(device)
    except ValueError as e:
        raise SystemExit(f'model.loss.freespace_weight: {e}') from e
    n = model.set_freespace_rays(ends, frame, origins)
    scene.release_rays(device)                      # (the model keeps its own, thinned copy: the scene's full set is read by nothing else)
    c = model.freespace_cfg
    print(f"freespace: weight {model.loss_weights['freespace']:g} on {n} of {len(ends)} rays of {len(origins)} frames, {c['rays'] or n} a step, "
          f"tau {c['tau']:g}, margin {c['margin']:g}, from epoch {c['start_epoch']}")
    return n


def main(argv=None):
    args = parse_args(argv)
    cfg = prepare_config(args)
    wants_world_frame(cfg)                      # (a malformed entry is refused before anything is read)
    blocks_init_options(cfg)
    from . import create_model
    from .dataset import create_train_val_test
    from .runlog import RunRecorder, resolve_start
    from .trainer import Trainer
    run_dir = os.path.join(args.runs_root, cfg['dataset']['name'], args.tag)
    os.makedirs(run_dir, exist_ok=True)
    resume, pretrained = resolve_start(cfg['training'], args.tag, args.resume)
    start = {}
    for key, tag in (('resume', resume), ('pretrained', pretrained)):
        if tag is not None:
            start[key] = os.path.join(args.runs_root, cfg['dataset']['name'], str(tag), 'model.pkl')
            if not os.path.exists(start[key]):
                raise SystemExit(f'training.{key} = {tag}: {start[key]} does not exist')
    seed = cfg['training'].get('seed', 4321)
    torch.manual_seed(seed)
    train, val, test = create_train_val_test(cfg, args.data_root, args.device)
    resolve_depth_cloud(train, args.device, run_dir)
    resolve_world_frame(cfg, train, args.device, run_dir, start.get('resume'))
    model = create_model(cfg, train.img_size).to(args.device).train()
    resolve_blocks_init(cfg, train, model, args.device, run_dir, start.get('resume') or start.get('pretrained'))
    resolve_surface(train, model, args.device)
    resolve_freespace(train, model, args.device)
    if 'perceptual' in model.loss_weights and model.perceptual_name != 'ssim':     # (ssim: the model installed its built-in term)
        from .lpips_vgg import LPIPSVGG
        net = LPIPSVGG()
        net.load_weights(torch.load(args.lpips_vgg, map_location='cpu'), torch.load(args.lpips_lin, map_location='cpu'))
        model.set_perceptual(net.to(args.device))
    trainer = Trainer(cfg, model, train.views(args.device))
    trainer.scene = train                       # (pose refinement: the refined poses go back into the capture's own files)
    print(f'Trainer init: config_file={args.config}, run_dir={run_dir}, n_epoches={trainer.n_epoches}')
    if args.no_record:
        if 'resume' in start:                   # (a recorded run's model.pkl may stop inside an epoch: the position and the schedule are the recorder's to read)
            from .runlog import load_checkpoint
            pos = load_checkpoint(trainer, torch.load(start['resume'], map_location=args.device, weights_only=False))
            print(f'Training state: epoch={pos[0]}, batch={pos[1]}, lr={trainer.step_fn.lrs[0]}')
        elif 'pretrained' in start:
            model.load_state_dict(torch.load(start['pretrained'], map_location=args.device, weights_only=False)['model_state'])
    else:
        rec = RunRecorder(trainer, run_dir, val=val.loader(trainer.batch_size, args.device) if len(val) else None, **start)
        print(f'Training state: epoch={rec.epoch_start}, batch={rec.batch_start}, lr={trainer.step_fn.lrs[0]}')
    last = trainer.run()
    if last is not None:
        print('last step: ' + ', '.join(f'{k}={float(v):.5f}' for k, v in last.items()))
    if args.no_record:                          # (a recorded run wrote it, with the state a resume needs)
        torch.save(trainer.state_dict(), os.path.join(run_dir, 'model.pkl'))
    dtu = None
    dtu_dir = os.path.join(args.data_root, 'DTU')
    if train.name == 'dtu' and os.path.isdir(os.path.join(dtu_dir, 'ObsMask')) and os.path.isdir(os.path.join(dtu_dir, 'Points', 'stl')):
        dtu = dict(scale_mat=train.scale_mat.to(args.device), scan_id=int(train.tag.replace('scan', '')), dataset_dir=dtu_dir)
    if len(test) == 0:                          # (a custom capture of fewer than 10 frames: the 0.9 split leaves none out)
        print(f"the test split of '{train.tag}' is empty: evaluating on the {len(train)} training views")
        test = train
    scores = trainer.evaluate(test.loader(trainer.batch_size, args.device), run_dir, dtu=dtu)
    print('final_scores: ' + ', '.join(f'{k}={v:.5f}' for k, v in scores.items() if not isinstance(v, dict)))
    return scores


if __name__ == '__main__':
    main(sys.argv[1:])
