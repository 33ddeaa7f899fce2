"""GPU: the free-space term (csrc/freespace_term.hip) at its launch edges, and in the model.

Records are held to the g++ build of the same header (tests/host_freespace.cpp) byte for byte, in both schedules of the forward, with the
slab test on and off, with the draw and with all rays in order.  The value and the gradients are held to float64 references (tests/freespace_ref.py for the value,
ops.freespace_term_torch in float64 for the gradients) at one element-wise bar of freespace_ref.bars.  A ray enters the gradient
comparison unless the float64 reference itself flags it (freespace_ref.first_hits: next to an edge, the graze threshold or a threshold of
the penalty); the flagged share is asserted to stay at or below 2 % on every shape."""
import functools

import numpy as np
import pytest
import torch

import freespace_ref as FR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TAU, MARGIN, SEED, STEP = 0.1, 0.02, 20240917, 41
MS = [1, 63, 64, 257, 1000]
SCENES = ['one_face', 'blocks', 'dropped', 'degenerate', 'inside']


@functools.lru_cache(maxsize=None)
def _scene(name):
    sc, origins = FR.scene(name)
    ends, frame = FR.rays_through(sc, origins, 1000, seed=5)
    return sc, origins, ends, frame


def _alpha(sc):
    return np.linspace(0.9, 0.3, sc['n_blocks']).astype(np.float32)


def _dev(sc, origins, ends, frame):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)        # noqa: E731
    return dict(ends=t(ends), frame=t(frame), origins=t(origins), verts=t(sc['verts']), faces=t(sc['faces']), face_group=t(sc['face_group']),
                group_keep=t(sc['group_keep']), group_alpha=t(sc['group_alpha']), vert_alpha=t(_alpha(sc)))


@pytest.mark.parametrize('M', MS)
@pytest.mark.parametrize('name', SCENES)
def test_records_equal_the_host_build_and_the_value_meets_the_reference(name, M):
    from dbw_amd import ops
    sc, origins, ends, frame = _scene(name)
    for n_rays, (p, fr) in ((M, (ends, frame)), (0, (ends[:M], frame[:M]))):
        d = _dev(sc, origins, p, fr)
        want, psi = FR.host_records(p, fr, origins, sc, n_rays, SEED, STEP, TAU, MARGIN, cull=0)
        assert np.array_equal(want, FR.host_records(p, fr, origins, sc, n_rays, SEED, STEP, TAU, MARGIN, cull=1)[0])
        got = {}
        for layout in (1, 2, 0):                                    # both schedules of the forward, and the default
            for cull in (0, 1):
                rec, value, _ = ops.freespace_records(**d, n_rays=n_rays, tau=TAU, margin=MARGIN, seed=SEED, step=STEP, cull=cull, layout=layout,
                                                      faces_host=torch.from_numpy(sc['faces']))
                got[cull] = (rec.cpu().numpy().view(np.uint32), value.cpu().numpy())
                assert got[cull][0].shape == (M, 4) and np.array_equal(got[cull][0], want), (name, M, n_rays, cull, layout)
                assert got[cull][1].tobytes() == got.setdefault('value', got[cull][1]).tobytes(), (name, M, n_rays, cull, layout)
        idx = FR.draw_indices(SEED, STEP, M, len(p)) if n_rays else np.arange(M)
        ref = FR.term_value(p[idx], fr[idx], origins, sc, _alpha(sc), TAU, MARGIN)
        k = FR.bars(got[1][1][0], ref)
        print(f'{name} M={M} n_rays={n_rays}: value {k:.4f} bars ({got[1][1][0]:.6e})')
        assert k <= 1.0
        face = want[:, 1].astype(np.int32)
        a = FR.face_alpha(sc, _alpha(sc).astype(np.float64))[np.maximum(face, 0)]
        assert abs(float((a * psi.astype(np.float64)).mean()) - got[1][1][0]) <= 1e-12 + 1e-7 * ref      # the same fp32 psi, summed in fp64
    if M == 1000:
        rec = got[1][0]
        face, t = rec[:, 1].astype(np.int32), rec[:, 0].view(np.float32)
        assert face[1] == -1 and np.isnan(t[1]) and face[3] == -1                # the ray of another frame table, the ray of zero length
        hit = face >= 0
        assert 0.2 < hit.mean() < 0.9 and (t[hit] > 0).all() and (t[hit] < 1).all()
        assert FR.face_keep_of(sc)[face[hit]].all()                            # no record names a face of a dropped group
        if name == 'inside':
            blk2 = (face >= sc['face_group'][3]) & (face < sc['face_group'][4])
            assert blk2[frame == 4].mean() > 0.9                               # a camera inside block 2 sees its faces from behind


@functools.lru_cache(maxsize=None)
def _gradient_case(name):
    """The rays the float64 reference does not flag (as a ray set of their own, all of it in order) and the reference's gradients on them."""
    from dbw_amd import ops
    sc, origins, ends, frame = _scene(name)
    h = FR.first_hits(ends, frame, origins, sc['verts'], sc['faces'], FR.face_keep_of(sc), TAU, MARGIN)
    kept = ~h['flagged']
    p, fr = np.ascontiguousarray(ends[kept]), np.ascontiguousarray(frame[kept])
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))        # noqa: E731
    v = t(sc['verts']).double().requires_grad_()
    a = torch.from_numpy(_alpha(sc)).double().requires_grad_()
    val = ops.freespace_term_torch(t(p), t(fr), t(origins), v, t(sc['faces']), t(sc['face_group']), t(sc['group_keep']), t(sc['group_alpha']), a,
                                   n_rays=0, tau=TAU, margin=MARGIN, seed=SEED, step=STEP, weight=1.7)
    val.backward()
    return sc, origins, p, fr, float(h['flagged'].mean()), val.item(), v.grad.numpy(), a.grad.numpy()


@pytest.mark.parametrize('segment', [0, 64])
@pytest.mark.parametrize('name', SCENES)
def test_gradients_meet_the_float64_reference(name, segment):
    from dbw_amd import ops
    sc, origins, p, fr, flagged, val, gv, ga = _gradient_case(name)
    print(f'{name}: {100 * flagged:.2f} % of the rays flagged, {len(p)} kept')
    assert flagged <= FR.FLAG_CAP and len(p) > 64 * 15
    d = _dev(sc, origins, p, fr)
    verts, alpha = d['verts'].clone().requires_grad_(), d['vert_alpha'].clone().requires_grad_()
    kw = dict(n_rays=0, tau=TAU, margin=MARGIN, seed=SEED, step=STEP, weight=1.7, segment=segment)
    out = ops.freespace_term(**dict(d, verts=verts, vert_alpha=alpha), **kw)
    assert out.dtype == torch.float32 and out.dim() == 0
    (3.0 * out).backward()
    k = (FR.bars(out.item(), val), FR.bars(verts.grad.cpu().numpy() / 3.0, gv), FR.bars(alpha.grad.cpu().numpy() / 3.0, ga))
    print(f'{name} segment={segment}: value {k[0]:.4f}, vertex gradient {k[1]:.4f}, opacity gradient {k[2]:.4f} bars')
    assert np.abs(gv).max() > 0 and np.abs(ga).max() > 0 and max(k) <= 1.0
    # the same bytes on a second call (another segment length is another order of addition and may differ in the last bits)
    verts2, alpha2 = d['verts'].clone().requires_grad_(), d['vert_alpha'].clone().requires_grad_()
    out2 = ops.freespace_term(**dict(d, verts=verts2, vert_alpha=alpha2), **kw)
    (3.0 * out2).backward()
    for x, y in ((out, out2), (verts.grad, verts2.grad), (alpha.grad, alpha2.grad)):
        assert x.detach().cpu().numpy().tobytes() == y.detach().cpu().numpy().tobytes()


def test_the_backward_draws_what_the_forward_drew():
    """With the draw, the backward finds a record's ray again from (seed, step, i): the same bytes as the gathered rays in order."""
    from dbw_amd import ops
    sc, origins, ends, frame = _scene('blocks')
    d = _dev(sc, origins, ends, frame)
    idx = torch.from_numpy(FR.draw_indices(SEED, STEP, 257, len(ends))).to(DEV)
    kw = dict(tau=TAU, margin=MARGIN, seed=SEED, step=STEP)
    outs = []
    for (p, fr), n_rays in (((d['ends'], d['frame']), 257), ((d['ends'][idx].contiguous(), d['frame'][idx].contiguous()), 0)):
        dd = dict(d, ends=p, frame=fr)
        rec, value, ws = ops.freespace_records(**dd, n_rays=n_rays, segment=64, **kw)
        gv, ga = ops.freespace_grads(**dd, records=rec, workspace=ws, n_rays=n_rays, weight=2.0, segment=64, **kw)
        outs.append((rec.cpu().numpy().tobytes(), value.cpu().numpy().tobytes(), gv.cpu().numpy().tobytes(), ga.cpu().numpy().tobytes()))
        assert float(gv.abs().max()) > 0 and float(ga.abs().max()) > 0
    assert outs[0] == outs[1]
    # another step draws other rays
    rec2 = ops.freespace_records(**d, n_rays=257, tau=TAU, margin=MARGIN, seed=SEED, step=STEP + 1)[0]
    assert rec2.cpu().numpy().tobytes() != ops.freespace_records(**d, n_rays=257, **kw)[0].cpu().numpy().tobytes()
    # without opacities every a is 1 and there is no opacity gradient; malformed shapes get the message
    rec, value, ws = ops.freespace_records(**dict(d, vert_alpha=None), n_rays=257, **kw)
    gv, ga = ops.freespace_grads(**dict(d, vert_alpha=None), records=rec, workspace=ws, n_rays=257, weight=2.0, **kw)
    assert ga is None and float(value[0]) > float(ops.freespace_records(**d, n_rays=257, **kw)[1][0]) > 0
    with pytest.raises(ValueError, match=r'ends \(Nr,3\), origins \(Nf,3\), verts \(V,3\), faces \(F,3\) expected'):
        ops.freespace_records(**dict(d, ends=d['ends'].reshape(-1)), n_rays=257, **kw)
    with pytest.raises(ValueError, match='group_alpha has 3 entries for 4 groups'):
        ops.freespace_records(**dict(d, group_alpha=d['group_alpha'][:3].contiguous()), n_rays=257, **kw)
    # a workspace sized for one segment is refused for five: the partials of the segments are its last part
    rec, value, ws = ops.freespace_records(**d, n_rays=257, **kw)
    with pytest.raises(ValueError, match='give freespace_records the same segment'):
        ops.freespace_grads(**d, records=rec, workspace=ws, n_rays=257, weight=2.0, segment=64, **kw)


def test_a_face_index_outside_the_vertices_is_vertex_0_to_both_calls():
    """Without faces_host nothing refuses an index of V: the gather reads it as vertex 0, and the backward gives that corner's gradient to
    vertex 0 -- records, value and both gradients are the bytes of the same call with the index 0."""
    from dbw_amd import ops
    sc, origins, ends, frame = _scene('blocks')
    kw = dict(n_rays=257, tau=TAU, margin=MARGIN, seed=SEED, step=STEP, segment=64)
    rec = ops.freespace_records(**_dev(sc, origins, ends, frame), **kw)[0].cpu().numpy()
    f = int(np.bincount(rec[rec[:, 1] >= 0, 1], minlength=len(sc['faces'])).argmax())    # the face most rays meet first
    outs = []
    for index in (0, len(sc['verts'])):
        faces = sc['faces'].copy()
        faces[f, 0] = index
        d = _dev(dict(sc, faces=faces), origins, ends, frame)
        rec, value, ws = ops.freespace_records(**d, **kw)
        gv, ga = ops.freespace_grads(**d, records=rec, workspace=ws, weight=2.0, **kw)
        outs.append([x.cpu().numpy() for x in (rec, value, gv, ga)])
    rec, b = outs[0][0], outs[0][0][:, 2:].view(np.float32)
    assert ((rec[:, 1] == f) & (1 - b[:, 0] - b[:, 1] > 0)).any() and np.abs(outs[0][2][0]).max() > 0             # the moved corner carries gradient
    for x, y in zip(*outs):
        assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the term in the model
def _tiny_model(loss, n_blocks=2, size=(16, 24)):
    from dbw_amd import create_model
    cfg = {'model': {'name': 'dbw', 'mesh': {'n_blocks': n_blocks, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True, 'opacity_noise': False},
                     'loss': dict(loss)}}
    torch.manual_seed(7)
    return create_model(cfg, size).to(DEV).train()


def _inputs(model, size=(16, 24)):
    import oracle as O
    R, T, K = O.synthetic_cameras(2, R_world=model.R_world[0].cpu())
    g = torch.Generator().manual_seed(0)
    return {'imgs': torch.rand(2, 3, *size, generator=g).to(DEV), 'R': R.to(DEV), 'T': T.to(DEV), 'K': K.to(DEV)}


def _rays_behind_the_blocks(model, inp, n=4000, stretch=1.8, clear=0.7):
    """Rays from the batch's two camera centres through the model's two blocks to ends well behind them (each aimed at a jittered block
    vertex and carried on to `stretch` times its distance; ends closer than `clear` to any block vertex are left out): the measured surface
    lies behind the blocks, which float in the space the rays cross -> (ends, frame, origins, the distance of the nearest end to a vertex)."""
    with torch.no_grad():
        v = model.blocks_mesh(filter_transparent=False)[0].reshape(-1, 3).cpu()
    origins = -torch.einsum('nij,nj->ni', inp['R'].cpu(), inp['T'].cpu().reshape(-1, 3))        # x_cam = x R + T: the centres
    g = torch.Generator().manual_seed(5)
    frame = torch.randint(0, len(origins), (n,), generator=g)
    aim = v[torch.randint(0, len(v), (n,), generator=g)] + 0.05 * torch.randn(n, 3, generator=g)
    ends = origins[frame] + stretch * (aim - origins[frame])
    keep = torch.cdist(ends, v).min(1).values > clear
    ends, frame = ends[keep].contiguous(), frame[keep].to(torch.int32).contiguous()
    assert len(ends) > n // 4
    return ends.to(DEV), frame.to(DEV), origins.contiguous().to(DEV), float(torch.cdist(ends, v).min())


FULL = {'rgb_weight': 1, 'parsimony_weight': 0.01, 'tv_weight': 0.1, 'overlap_weight': 1}


def test_the_model_adds_the_term_and_its_gradient_reaches_shape_pose_and_opacity():
    model = _tiny_model(dict(FULL, freespace_weight=1.0, freespace={'rays': 512, 'tau': 0.3}))
    inp = _inputs(model)
    ends, frame, origins, _ = _rays_behind_the_blocks(model, inp)
    assert model.set_freespace_rays(ends, frame, origins) == len(ends)
    plain = _tiny_model(FULL)
    assert list(plain(inp)) == ['rgb', 'parsimony', 'tv', 'overlap', 'total']
    model.zero_grad(set_to_none=True)
    losses = model(inp)
    assert list(losses) == ['rgb', 'parsimony', 'tv', 'overlap', 'freespace', 'total'] and losses['freespace'].dtype == torch.float32
    s = float(losses['freespace'].detach())
    assert s > 0.0 and abs(float(losses['total']) - sum(float(v) for k, v in losses.items() if k != 'total')) < 1e-5
    for k in ('rgb', 'parsimony', 'tv', 'overlap'):                 # the other terms are those of the model without the weight
        assert abs(float(losses[k]) - float(plain(inp)[k])) <= 1e-6 * max(1.0, abs(float(losses[k]))), k
    losses['freespace'].backward()
    for name in ('sq_eps', 'S', 'R_6d', 'T', 'alpha_logit'):
        g = getattr(model, name).grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
    assert model.texture_bkg.grad is None or not bool(model.texture_bkg.grad.any())
    # in eval mode the term is there and zero: an evaluation's total does not count the term
    model.eval()
    with torch.no_grad():
        ev = model(inp)
    model.train()
    assert float(ev['freespace']) == 0.0 and abs(float(ev['total']) - sum(float(v) for k, v in ev.items() if k != 'total')) < 1e-5
    # before start_epoch the term is there and zero
    late = _tiny_model(dict(FULL, freespace_weight=1.0, freespace={'rays': 512, 'tau': 0.3, 'start_epoch': 3}))
    late.set_freespace_rays(ends, frame, origins)
    assert float(late(inp)['freespace']) == 0.0
    late.set_cur_epoch(2)
    assert float(late(inp)['freespace']) > 0.0
    # beside the surface term: both columns, the surface term first
    both = _tiny_model(dict(FULL, surface_weight=1.0, freespace_weight=1.0, surface={'points': 256}, freespace={'rays': 256}))
    both.set_freespace_rays(ends, frame, origins)
    both.set_surface_points(ends)
    out = both(inp)
    assert list(out) == ['rgb', 'parsimony', 'tv', 'overlap', 'surface', 'freespace', 'total'] and float(out['freespace']) > 0 and float(out['surface']) > 0


def test_a_floating_block_is_invisible_to_the_surface_term_and_moved_by_this_one():
    """Two blocks floating between the cameras and a measured plane 1.5 units behind them, farther than the surface term's tau from every
    point: the surface term gives T a gradient of exactly 0, the free-space term a non-zero one, and thirty Adam steps on the free-space term
    alone lower it."""
    loss = {'rgb_weight': 0, 'surface_weight': 1.0, 'freespace_weight': 1.0, 'surface': {'points': 0, 'tau': 0.1, 'ground': False},
            'freespace': {'rays': 0, 'tau': 0.1, 'ground': False}}
    model = _tiny_model(loss)
    inp = _inputs(model)
    ends, frame, origins, gap = _rays_behind_the_blocks(model, inp)
    assert gap > 0.1 + 0.5                                          # every point is far beyond tau of every vertex
    model.set_surface_points(ends)
    model.set_freespace_rays(ends, frame, origins)
    model.zero_grad(set_to_none=True)
    losses = model(inp)
    assert list(losses) == ['surface', 'freespace', 'total']
    losses['surface'].backward(retain_graph=True)
    assert model.T.grad is None or float(model.T.grad.abs().max()) == 0.0
    assert model.sq_eps.grad is None or float(model.sq_eps.grad.abs().max()) == 0.0
    model.zero_grad(set_to_none=True)
    losses['freespace'].backward()
    assert model.T.grad is not None and float(model.T.grad.abs().max()) > 0 and bool(torch.isfinite(model.T.grad).all())
    # the term alone, thirty steps
    alone = _tiny_model({'rgb_weight': 0, 'freespace_weight': 1.0, 'freespace': {'rays': 0, 'tau': 0.1, 'ground': False}})
    alone.set_freespace_rays(ends, frame, origins)
    opt = torch.optim.Adam([p for n, p in alone.named_parameters() if not n.startswith('texture')], lr=5e-3)
    values = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        out = alone(inp)
        assert list(out) == ['freespace', 'total']
        out['total'].backward()
        opt.step()
        values.append(float(out['freespace']))
    print('free-space term over 30 Adam steps:', [round(v, 6) for v in values[::5]], round(values[-1], 6))
    assert all(np.isfinite(values)) and values[0] > 0 and values[-1] < values[0]


def test_the_trainer_writes_the_column_and_without_the_weight_takes_the_c_step(tmp_path, monkeypatch, capsys):
    import yaml
    import depth_fixture as DF
    from dbw_amd import parallel, train
    DF.write_depth_capture(tmp_path, 'cap')
    cfg = {'dataset': {'name': 'custom', 'tag': 'cap', 'cloud': 'depth'},
           'model': {'name': 'dbw', 'mesh': {'n_blocks': 2, 'S_world': 0.5, 'R_world': [115, 0, 0], 'txt_size': 16},
                     'renderer': {'faces_per_pixel': 4, 'cameras': {'name': 'perspective'}, 'detach_bary': True, 'z_clip': 0.001},
                     'rend_optim': {'coarse_learning': True, 'decimate_txt': False, 'kill_blocks': True, 'decouple_rendering': True, 'opacity_noise': False},
                     'loss': dict(FULL, perceptual_weight=0, freespace={'rays': 64, 'tau': 0.5})},
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

    scores = train.main(common + ['--tag', 'with', '--freespace', '0.5'])
    out = capsys.readouterr().out
    assert 'freespace: weight 0.5 on ' in out and ' rays of 6 frames, 64 a step, tau 0.5, margin 0.02, from epoch 1' in out
    assert np.isfinite(float(scores['PSNR']))
    head, rows = columns('with')
    assert 'loss_freespace' in head and head.index('loss_freespace') == head.index('loss_total') - 1 and rows
    assert all(np.isfinite(float(r['loss_freespace'])) and float(r['loss_freespace']) >= 0 for r in rows)
    assert calls['all'] > 0 and calls['c'] == 0                    # the general path, every step
    calls.update(c=0, all=0)
    train.main(common + ['--tag', 'without'])
    head, rows = columns('without')
    assert 'loss_freespace' not in head and rows and 'freespace:' not in capsys.readouterr().out
    assert calls['all'] > 0 and calls['c'] == calls['all']         # the one-call C step, as before
