"""GPU: the surface term (csrc/surface_term.hip) at its launch edges, and in the model.

Records are held to the g++ build of the same header (tests/host_surface.cpp) byte for byte, with the box test on and off, with the draw
and with all points in order.  The value and the gradients are held to float64 references (tests/surface_ref.py for the value,
eval3d.surface_term_torch in float64 for the gradients) at one element-wise bar of surface_ref.bars.  A point enters the gradient
comparison unless the float64 reference itself cannot say which closest point it has (surface_ref.kept_for_gradients); the share left
out is asserted to stay below 1 %."""
import functools

import numpy as np
import pytest
import torch

import surface_ref as SR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TAU, BACK, SEED, STEP = 0.1, 0.5, 20240917, 41
MS = [1, 63, 64, 257, 1000]
SCENES = ['one_face', 'blocks', 'dropped', 'degenerate']


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == 'one_face':
        sc = dict(verts=np.array([[-0.2, 0.0, 0.1], [0.3, 0.05, 0.0], [0.0, 0.4, -0.1]], np.float32), faces=np.array([[0, 1, 2]], np.int32),
                  face_group=np.array([0, 1], np.int32), group_keep=None, vert_group=np.zeros(3, np.int32), n_blocks=1)
        rng = np.random.default_rng(3)
        cloud = (rng.normal(0, 0.15, (1000, 3)) + [0.03, 0.15, 0.0]).astype(np.float32)
        cloud[1], cloud[2] = (50.0, 40.0, -30.0), sc['verts'][0]
        return sc, cloud
    sc = SR.scene(3, ground=True, seed=4, drop=1 if name == 'dropped' else None, degenerate=name == 'degenerate')
    return sc, SR.cloud_near(sc, 1000, seed=5)


def _dev(sc, cloud):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)        # noqa: E731
    alpha = torch.linspace(0.9, 0.3, sc['n_blocks']).to(DEV)
    return dict(points=t(cloud), verts=t(sc['verts']), faces=t(sc['faces']), face_group=t(sc['face_group']), group_keep=t(sc['group_keep']),
                vert_alpha=alpha, vert_group=t(sc['vert_group']))


def _back_count(sc):
    return float(sc['n_blocks'] * (3 if len(sc['verts']) == 3 else SR.BNV))


@pytest.mark.parametrize('M', MS)
@pytest.mark.parametrize('name', SCENES)
def test_records_equal_the_host_build_and_the_value_meets_the_reference(name, M):
    from dbw_amd import ops
    sc, cloud = _scene(name)
    keep = SR.face_keep_of(sc)
    for n_points, pts in ((M, cloud), (0, cloud[:M])):
        d = _dev(sc, pts)
        want, rho = SR.host_records(pts, sc, n_points, SEED, STEP, TAU, cull=0)
        assert np.array_equal(want, SR.host_records(pts, sc, n_points, SEED, STEP, TAU, cull=1)[0])
        got = {}
        for cull in (0, 1):
            rec, value, _ = ops.surface_records(**d, n_points=n_points, tau=TAU, back=BACK, seed=SEED, step=STEP, back_count=_back_count(sc), cull=cull,
                                                faces_host=torch.from_numpy(sc['faces']))
            got[cull] = (rec.cpu().numpy().view(np.uint32), value.cpu().numpy())
            assert got[cull][0].shape == (M, 4) and np.array_equal(got[cull][0], want), (name, M, n_points, cull)
        assert got[0][1].tobytes() == got[1][1].tobytes()
        drawn = pts[SR.draw_indices(SEED, STEP, M, len(pts))] if n_points else pts
        fwd, bk = SR.term_value(drawn, sc['verts'], sc['faces'], keep, TAU, pts, d['vert_alpha'].cpu().numpy(), sc['vert_group'], BACK, _back_count(sc))
        k = (SR.bars(got[1][1][0], fwd), SR.bars(got[1][1][1], bk))
        print(f'{name} M={M} n_points={n_points}: value {k[0]:.4f} / {k[1]:.4f} bars')
        assert max(k) <= 1.0
        assert abs(float(rho.astype(np.float64).mean()) - got[1][1][0]) <= 1e-12 + 1e-7 * fwd      # the same fp32 rho, summed in fp64
    if name != 'one_face' and M == 1000:
        rec = got[1][0]
        d2 = rec[:, 0].view(np.float32)
        assert d2[1] > TAU * TAU and d2[2] == 0.0                   # one point beyond tau, one exactly on the surface
        assert keep[rec[:, 1].astype(np.int64)].all()               # no record names a face of a dropped group


@functools.lru_cache(maxsize=None)
def _gradient_case(name):
    """The points the float64 reference keeps (as a cloud of their own, all of it in order) and the reference's gradients on them."""
    from dbw_amd import eval3d
    sc, cloud = _scene(name)
    near = SR.nearest_on_surface(cloud, sc['verts'], sc['faces'], SR.face_keep_of(sc))
    kept = SR.kept_for_gradients(near, TAU)
    left_out = 1.0 - kept.mean()
    pts = np.ascontiguousarray(cloud[kept])
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))        # noqa: E731
    v = t(sc['verts']).double().requires_grad_()
    a = torch.linspace(0.9, 0.3, sc['n_blocks']).double().requires_grad_()
    val = eval3d.surface_term_torch(t(pts), v, t(sc['faces']), t(sc['face_group']), t(sc['group_keep']), a, t(sc['vert_group']), n_points=0, tau=TAU,
                                    back=BACK, seed=SEED, step=STEP, weight=1.7, back_count=_back_count(sc))
    val.backward()
    return sc, pts, left_out, val.item(), v.grad.numpy(), a.grad.numpy()


@pytest.mark.parametrize('segment', [0, 64])
@pytest.mark.parametrize('name', SCENES)
def test_gradients_meet_the_float64_reference(name, segment):
    from dbw_amd import ops
    sc, pts, left_out, val, gv, ga = _gradient_case(name)
    print(f'{name}: {100 * left_out:.2f} % of the points left out, {len(pts)} kept')
    assert left_out <= 0.01 and len(pts) > 64 * 2
    d = _dev(sc, pts)
    verts, alpha = d['verts'].clone().requires_grad_(), d['vert_alpha'].clone().requires_grad_()
    args = dict(d, verts=verts, vert_alpha=alpha)
    out = ops.surface_term(**args, n_points=0, tau=TAU, back=BACK, seed=SEED, step=STEP, weight=1.7, back_count=_back_count(sc), segment=segment)
    assert out.dtype == torch.float32 and out.dim() == 0
    (3.0 * out).backward()
    k = (SR.bars(out.item(), val), SR.bars(verts.grad.cpu().numpy() / 3.0, gv), SR.bars(alpha.grad.cpu().numpy() / 3.0, ga))
    print(f'{name} segment={segment}: value {k[0]:.4f}, vertex gradient {k[1]:.4f}, opacity gradient {k[2]:.4f} bars')
    assert max(k) <= 1.0
    # the same bytes on a second call (another segment length is another order of addition and may differ in the last bits)
    verts2, alpha2 = d['verts'].clone().requires_grad_(), d['vert_alpha'].clone().requires_grad_()
    out2 = ops.surface_term(**dict(d, verts=verts2, vert_alpha=alpha2), n_points=0, tau=TAU, back=BACK, seed=SEED, step=STEP, weight=1.7,
                            back_count=_back_count(sc), segment=segment)
    (3.0 * out2).backward()
    for x, y in ((out, out2), (verts.grad, verts2.grad), (alpha.grad, alpha2.grad)):
        assert x.detach().cpu().numpy().tobytes() == y.detach().cpu().numpy().tobytes()


def test_the_backward_draws_what_the_forward_drew():
    """With the draw, the backward finds a record's point again from (seed, step, i): the same bytes as the gathered cloud in order."""
    from dbw_amd import ops
    sc, cloud = _scene('blocks')
    d = _dev(sc, cloud)
    idx = torch.from_numpy(SR.draw_indices(SEED, STEP, 257, len(cloud))).to(DEV)
    kw = dict(tau=TAU, back=0.0, seed=SEED, step=STEP)
    outs = []
    for pts, n_points in ((d['points'], 257), (d['points'][idx].contiguous(), 0)):
        dd = dict(d, points=pts)
        rec, value, ws = ops.surface_records(**dd, n_points=n_points, segment=64, **kw)
        gv, ga = ops.surface_grads(**dd, records=rec, workspace=ws, n_points=n_points, weight=2.0, segment=64, **kw)
        outs.append((rec.cpu().numpy().tobytes(), value.cpu().numpy().tobytes(), gv.cpu().numpy().tobytes(), ga.cpu().numpy().tobytes()))
        assert float(gv.abs().max()) > 0 and float(ga.abs().max()) == 0.0
    assert outs[0] == outs[1]
    # without back_count the block vertices are counted (n_blocks * BNV, not V: the ground has vertices too); malformed shapes get the message
    kb = dict(kw, back=BACK)
    want = ops.surface_records(**d, n_points=257, back_count=3.0 * SR.BNV, **kb)[1].cpu().numpy()
    assert ops.surface_records(**d, n_points=257, **kb)[1].cpu().numpy().tobytes() == want.tobytes() and want[1] > 0
    assert len(sc['verts']) > 3 * SR.BNV
    with pytest.raises(ValueError, match=r'points \(N,3\), verts \(V,3\), faces \(F,3\) expected'):
        ops.surface_records(**dict(d, points=d['points'].reshape(-1)), n_points=257, **kw)
    # a workspace sized for one segment is refused for five: the partials of the segments are its last part
    rec, value, ws = ops.surface_records(**d, n_points=257, **kw)
    with pytest.raises(ValueError, match='give surface_records the same segment'):
        ops.surface_grads(**d, records=rec, workspace=ws, n_points=257, weight=2.0, segment=64, **kw)


def test_a_face_index_outside_the_vertices_is_vertex_0_to_both_calls():
    """Without faces_host nothing refuses an index of V: the gather reads it as vertex 0, and the backward gives that corner's gradient to
    vertex 0 -- records, value and both gradients are the bytes of the same call with the index 0."""
    from dbw_amd import ops
    sc, cloud = _scene('blocks')
    kw = dict(n_points=257, tau=TAU, back=BACK, seed=SEED, step=STEP, back_count=_back_count(sc), segment=64)
    rec = ops.surface_records(**_dev(sc, cloud), **kw)[0].cpu().numpy()
    inside = rec[:, 0].view(np.float32) < TAU * TAU
    f = int(np.bincount(rec[inside, 1], minlength=len(sc['faces'])).argmax())           # the face most records inside tau name
    outs = []
    for index in (0, len(sc['verts'])):
        faces = sc['faces'].copy()
        faces[f, 2] = index
        d = _dev(dict(sc, faces=faces), cloud)
        rec, value, ws = ops.surface_records(**d, **kw)
        gv, ga = ops.surface_grads(**d, records=rec, workspace=ws, weight=2.0, **kw)
        outs.append([x.cpu().numpy() for x in (rec, value, gv, ga)])
    rec = outs[0][0]
    assert ((rec[:, 1] == f) & (rec[:, 0].view(np.float32) < TAU * TAU) & (rec[:, 3].view(np.float32) > 0)).any()      # the moved corner carries gradient
    assert np.abs(outs[0][2][0]).max() > 0
    for x, y in zip(*outs):
        assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the term in the model
def _tiny_model(loss, surface=None, n_blocks=2, size=(16, 24)):
    from dbw_amd import create_model
    loss = dict(loss)
    if surface is not None:
        loss['surface'] = surface
    cfg = {'model': {'name': 'dbw', 'mesh': {'n_blocks': n_blocks, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True, 'opacity_noise': False},
                     'loss': loss}}
    torch.manual_seed(7)
    return create_model(cfg, size).to(DEV).train()


def _inputs(model, size=(16, 24)):
    import oracle as O
    R, T, K = O.synthetic_cameras(2, R_world=model.R_world[0].cpu())
    g = torch.Generator().manual_seed(0)
    return {'imgs': torch.rand(2, 3, *size, generator=g).to(DEV), 'R': R.to(DEV), 'T': T.to(DEV), 'K': K.to(DEV)}


def _two_boxes(model, n=2000, shift=0.1, half=0.12):
    """A cloud on the faces of two boxes, each next to one of the model's two blocks (a tenth of a unit off its centre)."""
    with torch.no_grad():
        centres = model.blocks_mesh(filter_transparent=False)[0].reshape(2, -1, 3).mean(1).cpu()
    g = torch.Generator().manual_seed(5)
    p = (torch.rand(n, 3, generator=g) * 2 - 1) * half
    axis, side = torch.randint(0, 3, (n,), generator=g), torch.randint(0, 2, (n,), generator=g) * 2 - 1
    p[torch.arange(n), axis] = side * half
    return (p + centres[torch.arange(n) % 2] + shift).to(DEV)


FULL = {'rgb_weight': 1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}


def test_the_model_adds_the_term_and_its_gradient_reaches_shape_pose_and_opacity():
    model = _tiny_model(dict(FULL, surface_weight=1.0), {'points': 512, 'tau': 0.3})
    inp = _inputs(model)
    model.set_surface_points(_two_boxes(model))
    plain = _tiny_model(FULL)
    assert list(plain(inp)) == ['rgb', 'parsimony', 'tv', 'overlap', 'total']
    model.zero_grad(set_to_none=True)
    losses = model(inp)
    assert list(losses) == ['rgb', 'parsimony', 'tv', 'overlap', 'surface', 'total'] and losses['surface'].dtype == torch.float32
    s = float(losses['surface'].detach())
    assert 0.0 < s <= 1.0 * (0.3 ** 2) * (1 + 0.5) and abs(float(losses['total']) - sum(float(v) for k, v in losses.items() if k != 'total')) < 1e-5
    for k in ('rgb', 'parsimony', 'tv', 'overlap'):                 # the other terms are those of the model without the weight
        assert abs(float(losses[k]) - float(plain(inp)[k])) <= 1e-6 * max(1.0, abs(float(losses[k]))), k
    losses['surface'].backward()
    for name in ('sq_eps', 'S', 'R_6d', 'T', 'alpha_logit', 'R_6d_ground', 'T_ground'):
        g = getattr(model, name).grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
    assert model.texture_bkg.grad is None or not bool(model.texture_bkg.grad.any())
    # in eval mode the term is there and zero: an evaluation does not search the cloud and its total does not count the term
    model.eval()
    with torch.no_grad():
        ev = model(inp)
    model.train()
    assert float(ev['surface']) == 0.0 and abs(float(ev['total']) - sum(float(v) for k, v in ev.items() if k != 'total')) < 1e-5
    # before start_epoch the term is there and zero
    late = _tiny_model(dict(FULL, surface_weight=1.0), {'points': 512, 'tau': 0.3, 'start_epoch': 3})
    late.set_surface_points(_two_boxes(late))
    assert float(late(inp)['surface']) == 0.0
    late.set_cur_epoch(2)
    assert float(late(inp)['surface']) > 0.0


def test_thirty_adam_steps_on_the_term_alone_lower_it():
    model = _tiny_model({'rgb_weight': 0, 'surface_weight': 1.0}, {'points': 0, 'tau': 0.3, 'back': 0.5})
    inp = _inputs(model)
    model.set_surface_points(_two_boxes(model))
    opt = torch.optim.Adam([p for n, p in model.named_parameters() if not n.startswith('texture')], lr=5e-3)
    values = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        losses = model(inp)
        assert list(losses) == ['surface', 'total']
        losses['total'].backward()
        opt.step()
        values.append(float(losses['surface']))
    print('surface term over 30 Adam steps:', [round(v, 6) for v in values[::5]], round(values[-1], 6))
    assert all(np.isfinite(values)) and values[-1] < values[0]


def test_the_trainer_writes_the_column_and_without_the_weight_takes_the_c_step(tmp_path, monkeypatch, capsys):
    import yaml
    import custom_fixture as CF
    from dbw_amd import parallel, train
    CF.write_capture(tmp_path, 'cap', with_points=True)
    cfg = {'dataset': {'name': 'custom', 'tag': 'cap'},
           'model': {'name': 'dbw', 'mesh': {'n_blocks': 2, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True, 'opacity_noise': False},
                     'loss': dict(FULL, perceptual_weight=0, surface={'points': 64, 'tau': 0.5})},
           'training': {'batch_size': 2, 'n_epoches': 2, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 1e-3}, 'scheduler': {'name': 'multi_step'},
                        'train_stat_interval': 1, 'val_stat_interval': 1000}}
    path = tmp_path / 'cap.yml'
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    calls = {'c': 0, 'all': 0}
    c_iter, call = parallel.ShardedTrainStep._c_iteration, parallel.ShardedTrainStep.__call__
    monkeypatch.setattr(parallel.ShardedTrainStep, '_c_iteration', lambda self, inp: calls.__setitem__('c', calls['c'] + 1) or c_iter(self, inp))
    monkeypatch.setattr(parallel.ShardedTrainStep, '__call__', lambda self, *a, **k: calls.__setitem__('all', calls['all'] + 1) or call(self, *a, **k))
    common = ['--config', str(path), '--data-root', str(tmp_path), '--runs-root', str(tmp_path / 'runs'), '--no-perceptual', '--device', DEV, '--epochs', '2']

    def columns(tag):
        lines = (tmp_path / 'runs' / 'custom' / tag / 'train_metrics.tsv').read_text().splitlines()
        head = lines[0].split('\t')
        return head, [dict(zip(head, ln.split('\t'))) for ln in lines[1:]]

    scores = train.main(common + ['--tag', 'with', '--surface', '0.5'])
    out = capsys.readouterr().out
    assert 'surface: weight 0.5 on 30 of 30 points, 64 a step, tau 0.5, back 0.5, from epoch 1' in out and np.isfinite(float(scores['PSNR']))
    head, rows = columns('with')
    assert 'loss_surface' in head and head.index('loss_surface') == head.index('loss_total') - 1 and rows
    assert all(np.isfinite(float(r['loss_surface'])) and float(r['loss_surface']) > 0 for r in rows)
    assert calls['all'] > 0 and calls['c'] == 0                    # the general path, every step
    calls.update(c=0, all=0)
    train.main(common + ['--tag', 'without'])
    head, rows = columns('without')
    assert 'loss_surface' not in head and rows and 'surface:' not in capsys.readouterr().out
    assert calls['all'] > 0 and calls['c'] == calls['all']         # the one-call C step, as before
