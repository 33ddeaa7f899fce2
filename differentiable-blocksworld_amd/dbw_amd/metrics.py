"""Evaluation metrics of the reference's `quantitative_eval` (src/model/dbw.py:464-493): PSNR from the MSE
(loss.py:28-29) and SSIM with an 11-tap Gaussian window, sigma 1.5, C1 = 0.01^2, C2 = 0.03^2 (loss.py:124-156; the
evaluation uses it WITHOUT padding).  Host-side torch code run once per evaluation -- not part of the hot path.

The reference convolves with the 11x11 outer product of the 1-D Gaussian; the window is separable, so this file filters rows
and columns with the 1-D kernel (22 instead of 121 taps per pixel and statistic).  tests/golden/ssim.npz pins it against the
reference's own SSIMLoss.

Also the reference's score keeping (utils/metrics.py): `Metrics` (named running averages with a TSV log), `MeshEvaluator` (Chamfer-L1 and
normal consistency of a mesh against a ground-truth cloud, raw and after a gradient ICP: eval3d.gradient_icp) and `ProxyEvaluator`
(mask IoU)."""
import math
import os
from collections import OrderedDict, defaultdict

import torch
import torch.nn.functional as F


class AverageMeter:
    """Running average weighted by the batch size (utils/metrics.py:17-35)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.sum = self.avg = 0.0
        self.count = 0

    def update(self, val, N=1):
        if isinstance(val, torch.Tensor):
            if val.numel() != 1:
                raise ValueError('AverageMeter takes scalars')
            val = val.item()
        self.val = val
        self.sum += val * N
        self.count += N
        self.avg = self.sum / self.count if self.count else 0.0


def mse2psnr(mse):
    """-10 log10(mse) for images in [0, 1]."""
    return -10.0 * torch.log(mse) / math.log(10.0)


def gaussian_window(size=11, sigma=1.5, device=None, dtype=torch.float32):
    x = torch.arange(size, dtype=torch.float64) - size // 2
    g = torch.exp(-x * x / (2.0 * sigma * sigma))
    return (g / g.sum()).to(dtype=dtype, device=device)


def _blur(x, g, pad):
    """Depthwise separable Gaussian filter of (N,C,H,W)."""
    C, k = x.shape[1], g.numel()
    x = F.conv2d(x, g.view(1, 1, 1, k).expand(C, 1, 1, k), padding=(0, pad), groups=C)
    return F.conv2d(x, g.view(1, 1, k, 1).expand(C, 1, k, 1), padding=(pad, 0), groups=C)


def ssim_map(img1, img2, window_size=11, sigma=1.5, padding=False):
    """Per-pixel SSIM of two (N,C,H,W) images in [0,1]; padding=False keeps only windows that lie inside the image."""
    g = gaussian_window(window_size, sigma, img1.device, img1.dtype)
    pad = window_size // 2 if padding else 0
    mu1, mu2 = _blur(img1, g, pad), _blur(img2, g, pad)
    s11 = _blur(img1 * img1, g, pad) - mu1 * mu1
    s22 = _blur(img2 * img2, g, pad) - mu2 * mu2
    s12 = _blur(img1 * img2, g, pad) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))


def ssim(img1, img2, window_size=11, padding=False):
    """Mean SSIM per image, (N,)."""
    return ssim_map(img1, img2, window_size, padding=padding).flatten(1).mean(1)


class SSIMTerm(torch.nn.Module):
    """The reference's SSIMLoss (loss.py:124-156, padding=True) as the perceptual term of the loss (`perceptual_name: ssim`):
    criterion(imgs, rec) -> mean over the batch, the channels and the pixels of 1 - SSIM, a scalar (ops.ssim_term: one HIP kernel for value
    and gradient on the GPU).  The reference's forward returns one value per image, with which its total loss is a vector for more than one
    view; the mean over the batch equals it for one view and is what LPIPSLoss makes of its per-image values.  No parameters, no weights to
    load, no target cache.  takes_masks: a batch with validity masks hands them over (masks (N,1,H,W) weights, count = 3 * their sum as a
    host number) and the term is ops.ssim_term's masked form, instead of being called on images multiplied by the masks."""
    takes_masks = True

    def forward(self, imgs, rec, masks=None, count=None):
        from .ops import ssim_term
        return ssim_term(imgs, rec) if masks is None else ssim_term(imgs, rec, masks=masks, count=count)


CHAMFER_FACTOR = 10            # utils/metrics.py:14: the usual factor Chamfer is reported with (OccNet, DVR)


class Metrics:
    """Named running averages with a TSV log (utils/metrics.py:38-107): a header `iteration epoch batch <names>` when the file is created,
    a line per log() with the averages as '{:.6f}', byte for byte the reference's file."""
    log_data = True

    def __init__(self, *names, log_file=None, append=False):
        self.names = list(names)
        self.meters = defaultdict(AverageMeter)
        if log_file is not None and self.log_data:
            self.log_file = str(log_file)
            if not os.path.exists(self.log_file) or not append:
                with open(self.log_file, mode='w') as f:
                    f.write('iteration\tepoch\tbatch\t' + '\t'.join(self.names) + '\n')
        else:
            self.log_file = None

    def log_and_reset(self, *names, it=None, epoch=None, batch=None):
        self.log(it, epoch, batch)
        self.reset(*names)

    def log(self, it, epoch, batch):
        if self.log_file is not None:
            with open(self.log_file, mode='a') as file:
                file.write(f'{it}\t{epoch}\t{batch}\t' + '\t'.join(map('{:.6f}'.format, self.values)) + '\n')

    def reset(self, *names):
        for name in (names if len(names) else self.names):
            self[name].reset()

    def read_log(self):
        """The log as {column: list}, the rows in file order: iteration / epoch / batch as int where they parse as one (else the text, e.g.
        'None'), the metrics as float.  {} without a log file.  (The reference returns a pandas DataFrame indexed by iteration.)"""
        if self.log_file is None:
            return {}
        with open(self.log_file) as f:
            rows = [line.rstrip('\n').split('\t') for line in f if line.strip()]
        out = OrderedDict((name, []) for name in rows[0])
        for row in rows[1:]:
            for k, (name, v) in enumerate(zip(rows[0], row)):
                if k < 3:
                    out[name].append(int(v) if v.lstrip('-').isdigit() else v)
                else:
                    out[name].append(float(v))
        return out

    def __getitem__(self, name):
        return self.meters[name]

    def __repr__(self):
        return ', '.join(['{}={:.4f}'.format(name, self[name].avg) for name in self.names])

    def __len__(self):
        return len(self.names)

    @property
    def values(self):
        return [self[name].avg for name in self.names]

    def update(self, *name_val, N=1):
        if len(name_val) == 1:
            d = name_val[0]
            if not isinstance(d, dict):
                raise TypeError('Metrics.update takes a dict, or a name and a value')
            for k, v in d.items():
                self.update(k, v, N=N)
        else:
            name, val = name_val
            if name not in self.names:
                raise KeyError(f'{name} not in current metrics')
            if isinstance(val, (tuple, list)):
                self[name].update(val[0], N=val[1])
            else:
                self[name].update(val, N=N)

    def get_named_values(self, filter_fn=None):
        pairs = list(zip(self.names, self.values))
        return pairs if filter_fn is None else [kv for kv in pairs if filter_fn(kv[0])]


class _Evaluator:
    def compute(self):
        return self.metrics.values

    def __repr__(self):
        return self.metrics.__repr__()

    def log_and_reset(self, it, epoch, batch):
        self.metrics.log_and_reset(it=it, epoch=epoch, batch=batch)

    def read_log(self):
        return self.metrics.read_log()


class MeshEvaluator(_Evaluator):
    """utils/metrics.py:110-197 on one (verts (V,3), faces (F,3)) mesh and a ground-truth cloud in the unit cube: Chamfer-L1 (x10) and
    normal consistency between N surface samples and the cloud, as they are ('chamfer-L1', 'normal-cos') and after the mesh was normalised
    to the unit cube and aligned by eval3d.gradient_icp (lr 0.01) ('chamfer-L1-ICP', 'normal-cos-ICP').

    N and n_iter are as fast_cpu decides (50 000 / 30 or 100 000 / 100); `n_points` overrides N.  Built: icp_type='gradient'.  Refused:
    icp_type='normal' (PyTorch3D's SVD-based iterative_closest_point is not built) and the 3D-IoU scores, which raise where the reference
    raises (voxels given while '3D-IoU' is among the names).  Without normals only the Chamfer scores are returned.  The ground truth is
    scored whole, whatever its size, as in the reference (whose `if self.N < len(pc_gt)` tests the batch size, 1, and never subsamples):
    the scores depend on no random draw but the samples'."""
    default_names = ['chamfer-L1', 'chamfer-L1-ICP', 'normal-cos', 'normal-cos-ICP', '3D-IoU', '3D-IoU-ICP']

    def __init__(self, names=None, log_file=None, run_icp=True, estimate_scale=True, anisotropic_scale=True, icp_type='gradient',
                 fast_cpu=False, append=False, n_points=None):
        self.names = list(names) if names is not None else list(self.default_names)
        self.metrics = Metrics(*self.names, log_file=log_file, append=append)
        self.run_icp, self.estimate_scale, self.ani_scale = run_icp, estimate_scale, anisotropic_scale
        if icp_type == 'normal':
            raise NotImplementedError("MeshEvaluator: icp_type='normal' is PyTorch3D's iterative_closest_point (closed-form SVD steps), which is "
                                      "not built; use icp_type='gradient'")
        if icp_type != 'gradient':
            raise ValueError(f"MeshEvaluator: icp_type must be 'gradient' or 'normal', got {icp_type!r}")
        self.icp_type, self.fast_cpu = icp_type, fast_cpu
        self.N = int(n_points) if n_points is not None else (50000 if fast_cpu else 100000)

    @property
    def n_iter(self):
        return 30 if self.fast_cpu else 100

    def update(self, mesh_pred, labels):
        res = self.evaluate(mesh_pred, labels['points'], labels.get('normals'), vox_gt=labels.get('voxels'))
        self.metrics.update(res, N=1)

    def draw_samples(self, mesh_pred, with_normals=True, generator=None):
        """The two draws of evaluate(): N samples of the mesh, then N of the normalised mesh -> (pc, normals, pc2, normals2), (1,N,3) each
        (the normals None without with_normals).  For evaluate(samples=...), to score the same draw twice."""
        from .eval3d import normalize_mesh, sample_points_from_meshes
        verts, faces = mesh_pred
        out = []
        meshes = [(verts, faces)] + ([normalize_mesh(verts, faces)] if self.run_icp else [])
        for v, f in meshes:
            r = sample_points_from_meshes(v, f, self.N, return_normals=with_normals, generator=generator)
            out += list(r) if with_normals else [r, None]
        return tuple(out) if self.run_icp else tuple(out) + (None, None)

    def evaluate(self, mesh_pred, pc_gt, norm_gt=None, vox_gt=None, generator=None, samples=None):
        """mesh_pred (verts, faces); pc_gt (1,P,3) or (P,3) inside [-0.5, 0.5]^3, touching it (ValueError otherwise); norm_gt like pc_gt or
        None.  generator: of the sample draws (on the mesh's device); samples: draw_samples() of an
        earlier call, on any device, instead of drawing.  -> OrderedDict of the scores among `names`."""
        from .eval3d import chamfer_distance, gradient_icp
        if vox_gt is not None and '3D-IoU' in self.names:
            raise NotImplementedError('not implemented for batch processing')
        verts, faces = mesh_pred
        dev, dt = verts.device, verts.dtype
        pc_gt = torch.as_tensor(pc_gt).to(device=dev, dtype=dt).reshape(1, -1, 3)
        with_normals = norm_gt is not None
        if with_normals:
            norm_gt = torch.as_tensor(norm_gt).to(device=dev, dtype=dt).reshape(1, -1, 3)
        if not abs(float(pc_gt.abs().max()) - 0.5) < 0.01:
            raise ValueError('MeshEvaluator: the ground truth must fit the unit cube [-0.5, 0.5]^3 and touch it (largest absolute coordinate '
                             f'within 0.01 of 0.5, got {float(pc_gt.abs().max()):.4f}): see eval3d.unit_cube_frame')
        if samples is None:
            samples = self.draw_samples((verts.detach(), faces), with_normals, generator)
        pc_pred, norm_pred, pc_pred2, norm_pred2 = [None if t is None else t.to(device=dev, dtype=dt) for t in samples]
        pcs, norms, tags = [pc_pred], [norm_pred], ['']
        if self.run_icp:
            pc_icp = gradient_icp(pc_pred2, pc_gt, self.estimate_scale, self.ani_scale, lr=0.01, n_iter=self.n_iter)[0]
            pcs, norms, tags = pcs + [pc_icp], norms + [norm_pred2], tags + ['-ICP']
        results = []
        for pc, norm, tag in zip(pcs, norms, tags):
            cham, normal = chamfer_distance(pc_gt, pc, x_normals=norm_gt, y_normals=norm if with_normals else None, return_L1=True)
            results.append(('chamfer-L1' + tag, cham.item() * CHAMFER_FACTOR))
            if with_normals:
                results.append(('normal-cos' + tag, 1 - normal.item()))
        return OrderedDict(r for r in results if r[0] in self.names)


class ProxyEvaluator(_Evaluator):
    """utils/metrics.py:200-228: the IoU of predicted and ground-truth masks, averaged over the masks seen."""
    default_names = ['mask_iou']

    def __init__(self, names=None, log_file=None, append=False):
        self.names = list(names) if names is not None else list(self.default_names)
        self.metrics = Metrics(*self.names, log_file=log_file, append=append)

    def update(self, mask_pred, mask_gt):
        for k in range(len(mask_pred)):
            self.metrics.update(self.evaluate(mask_pred[k], mask_gt[k]))

    def evaluate(self, mask_pred, mask_gt):
        miou = (mask_pred * mask_gt).sum() / (mask_pred + mask_gt).clamp(0, 1).sum()
        return OrderedDict(r for r in [('mask_iou', miou.item())] if r[0] in self.names)
