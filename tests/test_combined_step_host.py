"""CPU preconditions of the combined step (tests/combined_ref.py, DESIGN.md "The combined step against float64"): the fixed case is not
vacuous, the fp32 oracle and a float64 run of it make the same discrete decisions on it, the float64 restatement of the image terms is the
one the per-feature references hold, the float64 chains for delta and the intrinsics theta meet central differences, and
configs/custom_full.yml loads, builds a Trainer with all three refiners and is refused under two ranks."""
import os

import numpy as np
import pytest
import torch

import combined_ref as CR
import exposure_ref as ER
import freespace_ref as FR
import intrinsics_ref as IR
import masked_loss_ref as MR
import pose_ref as PR
import ssim_term_ref as TR
import surface_ref as SR
from dbw_amd import dataset, exposure, intrinsics, phase, pose
from dbw_amd.trainer import Trainer
from test_parallel_cpu import ToyModel, torch_adam


@pytest.fixture(scope='module')
def smoke_reference():
    """The float64 reference of the case at the host's refined cameras (float64 apply, rounded to fp32), computed once."""
    c = CR.case()
    orc = CR.oracle()
    R1, T1, K1 = CR.refined_cameras64(c)
    ref = CR.reference(orc, c['imgs'], R1, T1, K1, c['masks'], c['exposure'], c['rows'], c['u'], factor=phase.late_factor(True))
    ref['delta'] = CR.delta_grad64(c['R'], c['T'], c['delta'], c['rows'], ref['R'], ref['T'])
    ref['ktheta'] = CR.ktheta_grad64(c['K0'], c['ktheta'], ref['K'])
    return c, orc, (R1, T1, K1), ref


def test_the_fixed_case_is_not_vacuous(smoke_reference):
    c, orc, (R1, T1, K1), ref = smoke_reference
    # every reference gradient has a largest element above 1e-6 of the largest parameter gradient
    big = max(float(g.abs().max()) for g in ref['params'].values())
    tensors = dict(ref['params'], R=ref['R'], T=ref['T'], K=ref['K'], exposure=ref['theta'], delta=ref['delta'], ktheta=ref['ktheta'])
    for k, g in tensors.items():
        print(f'{k}: max |grad| {float(g.abs().max()):.3e} ({float(g.abs().max()) / big:.2e} of the largest parameter gradient)')
        assert float(g.abs().max()) > 1e-6 * big, k
    assert big > 0 and ref['rgb'] > 0 and ref['perceptual'] > 0 and all(v >= 0 for v in ref['regs'].values())
    # the refiners' rows: the batch's and no other
    outside = [v for v in range(CR.N_ROWS) if v not in c['rows']]
    assert not ref['theta'][outside].any() and not ref['delta'][outside].any() and bool(c['delta'][outside].all()) and bool(c['exposure'][outside].all())
    assert all(bool(ref[k][c['rows']].all()) for k in ('theta', 'delta')) and bool(ref['ktheta'].all()) and not ref['K'][2].any()
    # the masks remove between 10 % and 60 % of the pixels (by weight: 1 - their mean), with holes and fractional weights
    removed = 1.0 - float(c['masks'].double().mean())
    print(f'masks: {100 * removed:.2f} % of the pixels removed by weight, {100 * float((c["masks"] == 0).double().mean()):.2f} % zeroed')
    assert 0.10 <= removed <= 0.60 and bool((c['masks'] == 0).any()) and {0.25, 0.5} <= set(c['masks'].unique().tolist())
    assert c['mask_sum'] == float(c['masks'].double().sum())
    # the 3D terms, on the oracle's own vertices: some rays are stopped and some are not, some points are nearer than tau and some at tau
    sc, alpha = CR.oracle_term_scene(orc)
    h = FR.first_hits(c['ends'].numpy(), c['frame'].numpy(), c['origins'].numpy(), sc['verts'], sc['faces'], None, CR.TAU, CR.MARGIN)
    stopped = (h['face'] >= 0) & (h['psi'] > 0)
    on_block = h['face'] >= sc['face_group'][1]
    print(f'rays: {len(stopped)}, {100 * stopped.mean():.1f} % stopped ({100 * on_block.mean():.1f} % by a block), {100 * h["flagged"].mean():.2f} % flagged')
    assert 200 <= len(stopped) <= 1000 and 0.1 < stopped.mean() < 0.9 and on_block.mean() > 0.1 and (stopped & ~on_block).any()
    assert set(np.unique(c['frame'].numpy())) == {0, 1}
    near = SR.nearest_on_surface(c['cloud'].numpy(), sc['verts'], sc['faces'], None)
    inside = near['d2'] < CR.TAU ** 2
    print(f'cloud: {len(inside)} points, {100 * inside.mean():.1f} % nearer than tau')
    assert 0.5 < inside.mean() < 0.95
    assert CR.surface_value64(sc, c['cloud'], alpha) > 0 and CR.freespace_value64(sc, c['ends'], c['frame'], c['origins'], alpha) > 0


@pytest.mark.parametrize('rig', sorted(CR.RIGS))
def test_fp32_and_float64_oracle_make_the_same_discrete_decisions(rig):
    """The same pix_to_face and the same clip case of every face in both passes, without a tolerance.  The smoke cameras do clip: in each
    view faces of the sky dome and of the ground straddle the near plane (clip cases with one and with two vertices behind it), and the
    backward walks their slots; at this field of view none of them reaches a pixel, and neither does one under the `horizon` rig of
    tests/test_gpu_env_backward.py, which is run here as well for its other split of the env layer."""
    c = CR.case(rig)
    orc = CR.oracle()
    R1, T1, K1 = CR.refined_cameras64(c)
    d32, d64 = CR.discrete_decisions(orc, R1, T1, K1, torch.float32), CR.discrete_decisions(orc, R1, T1, K1, torch.float64)
    for name in ('env', 'fg'):
        a, b = d32[name], d64[name]
        assert torch.equal(a['pix_to_face'], b['pix_to_face']), (rig, name, int((a['pix_to_face'] != b['pix_to_face']).sum()))
        assert torch.equal(a['behind'], b['behind']), (rig, name)
        cases = [[int((a['behind'][v] == k).sum()) for k in range(4)] for v in range(2)]
        seen = a['pix_to_face'][a['pix_to_face'] >= 0]
        straddling = int((((a['behind'].reshape(-1)[seen]) % 3) != 0).sum())
        print(f'{rig} {name}: faces with 0 / 1 / 2 / 3 vertices behind the near plane per view {cases}; fragments of a straddling face: {straddling}')
        assert bool((a['pix_to_face'] >= 0).any())
    env = d32['env']['behind']
    assert all(bool((env[v] == 1).any()) and bool((env[v] == 2).any()) for v in range(2))      # z-clipped faces of both kinds, in every view


def test_the_image_term_restatement_is_the_per_feature_references():
    """image_terms64 on random layers against tests/exposure_ref.py (rec and the masked MSE), tests/masked_loss_ref.py (the masked SSIM
    term) and, under masks of ones, tests/ssim_term_ref.py (the plain one): the same formulas in float64, to rounding."""
    c = CR.case()
    g = torch.Generator().manual_seed(3)
    fg, env = torch.rand(2, 4, CR.H, CR.W, generator=g), torch.rand(2, 4, CR.H, CR.W, generator=g)
    fg64, env64 = fg.double(), env.double()
    comp = fg64[:, :3] * fg64[:, 3:4] + (1 - fg64[:, 3:4]) * env64[:, :3]
    factor = phase.late_factor(True)
    for mk in (c['masks'], torch.ones_like(c['masks'])):
        rec, rgb, per = CR.image_terms64(comp, c['imgs'].double(), mk.double(), c['exposure'].double()[c['rows']], factor)
        count = MR.count_of(mk)
        rec_e, value_e, comp_e, _ = ER.forward64(fg.double().numpy(), env.double().numpy(), c['imgs'].numpy(), mk.numpy(), c['exposure'].numpy(), c['rows'], 1.0 / count)
        assert np.abs(comp.numpy() - comp_e).max() <= 1e-15 and np.abs(rec.numpy() - rec_e).max() <= 1e-14
        assert abs(rgb.item() - value_e) <= 1e-13 * value_e
        v_m, _ = MR.term_torch(c['imgs'], rec, mk, torch.float64)
        assert abs(per.item() - CR.WEIGHT * factor * v_m.item()) <= 1e-13 * per.item()
        if bool((mk == 1).all()):
            v_p, _ = TR.term_torch(c['imgs'], rec, torch.float64)
            assert abs(per.item() - CR.WEIGHT * factor * v_p.item()) <= 1e-12 * per.item()


def test_the_float64_chains_meet_central_differences(smoke_reference):
    c, _, _, ref = smoke_reference
    gR, gT, gK = ref['R'].double(), ref['T'].double(), ref['K'].double()

    def f_pose(d):
        total = 0.0
        for b, v in enumerate(c['rows']):
            R1, T1, _ = PR.refine_torch(c['R'][b], c['T'][b], d[v], torch.float64)
            total = total + float((R1 * gR[b]).sum() + (T1 * gT[b]).sum())
        return total

    def f_k(th):
        return float((IR.refine_torch(c['K0'], th, torch.float64) * gK).sum())

    h = 1e-6
    for name, f, x, got in (('delta', f_pose, c['delta'].double(), ref['delta']), ('ktheta', f_k, c['ktheta'].double(), ref['ktheta'])):
        fd = torch.zeros_like(x)
        for i in range(x.numel()):
            e = torch.zeros_like(x).reshape(-1)
            e[i] = h
            fd.reshape(-1)[i] = (f(x + e.view_as(x)) - f(x - e.view_as(x))) / (2 * h)
        err = float((fd - got).abs().max())
        print(f'{name}: chain against central differences {err:.2e} of {float(got.abs().max()):.2e}')
        # central differences at h = 1e-6 in float64: truncation ~ h^2 |f'''|, rounding ~ 1e-16 |f| / h -- both below 1e-8 of the gradient here
        assert err <= 1e-7 * float(got.abs().max()), name


# ---------------------------------------------------------------------------------------------------------------- configs/custom_full.yml
def _full_cfg():
    here = os.path.dirname(os.path.abspath(__file__))
    return dataset.load_config(os.path.join(here, '..', 'differentiable-blocksworld_amd', 'configs', 'custom_full.yml'))


def _views():
    gen = torch.Generator().manual_seed(1)
    return {'imgs': torch.rand(5, 3, 4, 4, generator=gen), 'R': torch.eye(3).expand(5, 3, 3).contiguous(), 'T': torch.randn(5, 3, generator=gen),
            'K': IR.K0[None].repeat(5, 1, 1)}


def test_the_full_config_holds_every_optional_key_at_its_default():
    from dbw_amd import dbw
    cfg = _full_cfg()
    tr, loss = cfg['training'], cfg['model']['loss']
    assert pose.parse_config(tr['pose_refine']) == pose.parse_config(True) == {'lr': 1e-4, 'start_epoch': 0, 'rot': True, 'trans': True}
    assert exposure.parse_config(tr['exposure']) == exposure.parse_config(True) == {'lr': 1e-3, 'start_epoch': 0, 'bias': True, 'center': True}
    assert intrinsics.parse_config(tr['intrinsics_refine']) == intrinsics.parse_config(True) == {'lr': 1e-4, 'start_epoch': 0, 'focal': 'shared',
                                                                                                  'principal': False}
    assert dbw.parse_surface_config(loss['surface']) == dbw.parse_surface_config(None) and set(loss['surface']) == set(dbw.SURFACE_KEYS)
    assert dbw.parse_freespace_config(loss['freespace']) == dbw.parse_freespace_config(None) and set(loss['freespace']) == set(dbw.FREESPACE_KEYS)
    assert loss['surface_weight'] > 0 and loss['freespace_weight'] > 0 and loss['perceptual_name'] == 'ssim' and loss['perceptual_weight'] > 0
    assert cfg['dataset'] == {'name': 'custom', 'tag': 'my_capture', 'downscale_factor': 2, 'masks': True, 'cloud': 'depth'}
    assert cfg['model']['rend_optim']['decouple_rendering'] is True


def test_the_full_config_builds_a_trainer_with_all_three_refiners_and_is_refused_under_two_ranks(monkeypatch):
    cfg = _full_cfg()
    tr = Trainer(cfg, ToyModel(), _views())
    assert tr.pose is not None and tr.exposure is not None and tr.intrinsics is not None and tr.view_ids
    assert tr.pose.n_views == 5 and tr.exposure.n_views == 5 and torch.equal(tr.intrinsics.K0, IR.K0) and tr.batch_size == 4
    assert {'pose_refine', 'exposure', 'intrinsics_refine'} <= set(tr.state_dict())
    # one epoch on the toy model: every batch carries all three, and each refiner steps once per batch
    tr.step_fn.adam_fn = torch_adam
    for ref in (tr.pose, tr.exposure, tr.intrinsics):
        ref.adam_fn = torch_adam
    tr.pose.apply_fn = lambda R, T, delta, ids, ids_host=None: (R + 0 * delta[ids.long()].sum(), T + delta[ids.long(), 3:])
    tr.intrinsics.apply_fn = lambda K0, theta: IR.refine_torch(K0, theta, torch.float32)
    seen, step = [], tr.run_single_batch_train
    tr.run_single_batch_train = lambda batch, count=None: (seen.append(batch), step(batch, count))[1]
    tr.run_epoch(shuffle=False)
    assert len(seen) == 2 and all(b['R'].requires_grad and b['exposure'] is tr.exposure.theta and b['K_live'].requires_grad for b in seen)
    assert all(torch.equal(b['view_ids'].cpu(), b['view_ids_host']) for b in seen)
    assert tr.pose.n_steps == tr.exposure.n_steps == tr.intrinsics.n_steps == 2
    # under two ranks the first refiner's refusal comes first
    import dbw_amd.trainer as T

    class TwoRanks(T.ShardedTrainStep):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.world_size = 2
    monkeypatch.setattr(T, 'ShardedTrainStep', TwoRanks)
    with pytest.raises(NotImplementedError, match='training.pose_refine under data parallelism'):
        Trainer(cfg, ToyModel(), _views())
