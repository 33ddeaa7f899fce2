"""GPU tests of the scene parsing maps (include/dbw_viz.h: dbw_viz_parse_fwd, csrc/scene_parse.hip, ops.parse_scene, Renderer.parse_packed,
DifferentiableBlocksWorld.parse_views, export.write_parse, qualitative_eval(parse=True), Trainer.evaluate(masks=...)).  `-m gpu`.

The yardstick is the ORACLE's own rasteriser: O.render(scene, R, T, K, (H, W), 0.0, 32, False, return_fragments=True) on the joined scene
(sky, ground, blocks), evaluated AT the vertices the device rendered (lit_ref.oracle_scene, as tests/test_gpu_lit.py does).  From its
sorted lists of up to 32 faces per pixel: label = label of entry 0, depth = zbuf[..., 0], cover = OR over the list, counts = sums of
these.  That derivation is complete only while no list is full, so every use asserts the longest list < 32 -- no pixel is ever masked out.
Everything is compared EXACTLY: labels, words and counts are integers, and the project holds face indices and depths bit-equal to the
oracle at shared vertices (tests/test_gpu_parity.py), so depth is torch.equal too.

Set-up: that of test_gpu_lit._setup (seed 227391, 5 blocks, txt_size 16, sq_eps perturbed by randn * 2 of generator seed 5, alpha_logit
2), seen by 3 cameras at 8 degrees of elevation: at the default 30 the ground fills every pixel and the sky is never seen."""
import functools
import math
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lit_ref as LR                                            # noqa: E402
import oracle as O                                              # noqa: E402  (checker only)
from dbw_amd import export, ops                                 # noqa: E402
from dbw_amd.parse import SceneParse                            # noqa: E402
from test_gpu_lit import _setup                                 # noqa: E402

DEV = 'cuda:0'
LIST = 32
SIZES = [(40, 56), (18, 27)]            # 18 x 27: no multiple of the 16 x 16 tile in either direction; both: more than one tile per view


def _cameras(elev):
    return O.synthetic_cameras(3, R_world=O.world_rotation(115, 0, 0), elev_deg=elev)


def _face_labels(model, kept, w_bkg=True):
    """(F,) int32 on the CPU: 0 sky, 1 ground, 2 + k for block k of `kept` (original indices), in the face order of build_scene."""
    return torch.cat([torch.zeros(model.bkg_n_faces if w_bkg else 0, dtype=torch.int32), torch.ones(model.ground_n_faces, dtype=torch.int32),
                      (2 + torch.tensor(kept, dtype=torch.int32)).repeat_interleave(model.BNF)])


@functools.lru_cache(maxsize=None)
def _case(H, W, kill=False, w_bkg=True, elev=8.0):
    """The model, its joined host-packed scene, the inputs at the cameras of `elev`, and the oracle's lists -- computed once, never changed."""
    model, _, inp30, _ = _setup(H, W, kill=kill)
    R, T, Km = _cameras(elev)
    inp = dict(imgs=inp30['imgs'], R=R.to(DEV), T=T.to(DEV), K=Km.to(DEV))
    with torch.no_grad(), model._host_packed_rebuild():
        scene = model.build_scene(filter_transparent=True, w_bkg=w_bkg)
    with torch.no_grad():
        _, frag = O.render(LR.oracle_scene(scene), R, T, Km[0], (H, W), 0.0, LIST, False, n_threads=8, return_fragments=True)
    return types.SimpleNamespace(model=model, scene=scene, inp=inp, cams=(R, T, Km), frag=frag, kept=[0, 2, 4] if kill else [0, 1, 2, 3, 4])


def _derive(frag, face_label):
    """The oracle's lists -> (label u8, depth f32, cover i64, counts i32) on the CPU.  Packed face indices are taken modulo F."""
    p2f = frag['pix_to_face']
    valid = p2f >= 0
    longest, shortest = int(valid.sum(-1).max()), int(valid.sum(-1).min())
    print(f'oracle lists: longest {longest}, shortest {shortest} of {p2f.shape[-1]}')
    assert p2f.shape[-1] == LIST and longest < LIST, 'a full list: the derivation of the coverage word would be incomplete'
    table = torch.as_tensor(face_label).long()
    lab = table[p2f.clamp(min=0) % len(table)]
    label = torch.where(valid[..., 0], lab[..., 0], torch.tensor(255)).to(torch.uint8)
    depth = frag['zbuf'][..., 0].float()
    cover = torch.zeros(p2f.shape[:3], dtype=torch.int64)
    counts = torch.zeros(p2f.shape[0], 64, 2, dtype=torch.int32)
    for l in range(64):
        has = ((lab == l) & valid).any(-1)
        cover |= torch.where(has, torch.tensor(-2 ** 63 if l == 63 else 1 << l), torch.tensor(0))
        counts[:, l, 0] = has.sum((1, 2))
        counts[:, l, 1] = (label == l).sum((1, 2))
    return label, depth, cover, counts


def _assert_equal(got, want, what):
    names = ('label', 'depth', 'cover', 'counts')
    got = [t.cpu() for t in got]
    for name, g, w in zip(names, got, want):
        bad = int((g != w).sum())
        print(f'{what}: {name}: {bad} of {g.numel()} entries differ')
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), (what, name)


def _raw(sp):
    return sp.label, sp.depth, sp.cover, sp.counts


@pytest.mark.parametrize('H,W', SIZES)
def test_parse_views_equals_the_oracle_derivation(H, W):
    c = _case(H, W)
    m = c.model
    sp = m.parse_views(c.inp)
    assert isinstance(sp, SceneParse) and sp.n_blocks == 5 and sp.kept.tolist() == [True] * 5
    assert sp.label.shape == sp.depth.shape == sp.cover.shape == (3, H, W) and sp.counts.shape == (3, 64, 2)
    assert (sp.label.dtype, sp.depth.dtype, sp.cover.dtype, sp.counts.dtype) == (torch.uint8, torch.float32, torch.int64, torch.int32)
    want = _derive(c.frag, _face_labels(m, c.kept))
    _assert_equal(_raw(sp), want, f'{H}x{W}')                                                            # 1
    label, depth, cover, counts = [t.cpu() for t in _raw(sp)]
    total = counts.sum(0)
    print(f'{H}x{W}: visible pixels per label 0..6: {total[:7, 1].tolist()}, amodal: {total[:7, 0].tolist()}')
    assert bool((total[:7, 1] > 0).all()) and not total[7:].any() and not (label == 255).any()          # 2: sky, ground and each block are seen
    if (H, W) == (40, 56):
        assert total[:7, 1].tolist() == [2429, 3514, 182, 52, 222, 153, 168]                             # (the oracle's counts at this size)
    assert bool((counts[:, 2:7, 1] < counts[:, 2:7, 0]).any())                                           # 3: some block is partly hidden
    assert bool((counts[..., 1] <= counts[..., 0]).all()) and int(counts[..., 1].sum()) == 3 * H * W
    for l in range(64):                                                                                  # 4, 5
        assert torch.equal(counts[:, l, 0].long(), ((cover >> l) & 1).sum((1, 2))), l
        assert torch.equal(counts[:, l, 1].long(), (label == l).sum((1, 2))), l
    again = m.parse_views(c.inp)                                                                         # 6
    for a, b in zip(_raw(sp), _raw(again)):
        assert torch.equal(a, b)
    # 7: where the new kernel and the K = 1 fragment pass overlap, they agree: nearest face and its depth
    cfg = ops.RenderCfg(H, W, 1, 0.0, 0.001, True, False, c.scene.faces.shape[0], 1e-8)
    Kmat = m.renderer.cameras.K[0].to(DEV).contiguous()
    cl, p2f, zbuf, _, _ = ops.render_fragments(c.scene.verts, c.scene.faces, c.inp['R'], c.inp['T'], Kmat, cfg)
    p2f = p2f[..., 0].long()
    orig = cl['c2o'].view(-1)[p2f.clamp(min=0)].long()
    lab1 = torch.where(p2f >= 0, _face_labels(m, c.kept).to(DEV).long()[orig], torch.tensor(255, device=DEV)).to(torch.uint8)
    assert torch.equal(sp.label, lab1) and torch.equal(sp.depth, zbuf[..., 0])
    # the methods, on real maps
    for k in range(5):
        assert torch.equal(sp.amodal(k).cpu(), ((cover >> (2 + k)) & 1).bool()) and torch.equal(sp.modal(k).cpu(), label == 2 + k)
        assert not bool((sp.modal(k) & ~sp.amodal(k)).any())
    assert torch.equal(sp.foreground().cpu(), label >= 2)
    occ = sp.occlusion().cpu()
    assert occ.shape == (3, 5) and bool(((occ >= 0) & (occ < 1)).all()) and float(occ.max()) > 0
    img = sp.colors()
    assert img.shape == (3, 3, H, W) and img.device.type == 'cuda' and float(img.min()) >= 0 and float(img.max()) <= 1


def test_areas_at_the_default_cameras():
    """The 30 degree ring of test_gpu_lit._setup: the ground fills the picture, no sky; the areas the oracle gives for blocks 1 and 3."""
    c = _case(40, 56)
    R, T, Km = _cameras(30.0)
    sp = c.model.parse_views(dict(c.inp, R=R.to(DEV), T=T.to(DEV)))
    amodal, visible = [t.sum(0).tolist() for t in sp.areas()]
    print(f'30 degrees: amodal {amodal}, visible {visible}, sky pixels {int((sp.label == 0).sum())}')
    assert int((sp.label == 0).sum()) == 0 and int(sp.counts[:, 1, 0].sum()) == 3 * 40 * 56
    assert (amodal[1], visible[1]) == (94, 44) and (amodal[3], visible[3]) == (217, 151)


@pytest.mark.parametrize('H,W', SIZES)
def test_every_bit_of_the_coverage_word(H, W):
    """8: a synthetic table, face_label = face index % 64, on the same scene and the same oracle lists: bits 32 to 63 without a 50-block
    scene.  The table arrives once as the host copy the library validates, once as a device tensor."""
    c = _case(H, W)
    n_faces = c.scene.faces.shape[0]
    table = (torch.arange(n_faces) % 64).to(torch.int32)
    cfg = ops.RenderCfg(H, W, 1, 0.0, 0.001, True, False, n_faces, 1e-8)
    Kmat = c.model.renderer.cameras.K[0].to(DEV).contiguous()
    got = ops.parse_scene(c.scene.verts, c.scene.faces, table, c.inp['R'], c.inp['T'], Kmat, cfg)
    want = _derive(c.frag, table)
    _assert_equal(got, want, f'{H}x{W}, labels = face % 64')
    seen = want[3][:, :, 0].sum(0)
    print(f'{H}x{W}: labels with covered pixels: {int((seen > 0).sum())} of 64; sign bit set on {int((want[2] < 0).sum())} pixels')
    assert int((seen[32:] > 0).sum()) >= 16 and int((want[2] < 0).sum()) > 0
    if (H, W) == (40, 56):
        assert bool((seen > 0).all())
    on_device = ops.parse_scene(c.scene.verts, c.scene.faces, table.to(DEV), c.inp['R'], c.inp['T'], Kmat, cfg)
    for a, b in zip(got, on_device):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match=r'face_label\[64\] = 64 is outside \[0, 64\)'):
        ops.parse_scene(c.scene.verts, c.scene.faces, torch.arange(n_faces) % 65, c.inp['R'], c.inp['T'], Kmat, cfg)
    with pytest.raises(ValueError, match='entries for'):
        ops.parse_scene(c.scene.verts, c.scene.faces, table[:-1], c.inp['R'], c.inp['T'], Kmat, cfg)


def test_labels_keep_their_block_index_when_blocks_are_dropped():
    """9: block 1 killed, block 3 below 0.5: the kept blocks 0, 2, 4 keep the labels 2, 4, 6; a sync_free model gives the same tensors
    and keeps the per-step state of its last forward."""
    H, W = 40, 56
    c = _case(H, W, kill=True)
    m = c.model
    assert c.scene.faces.shape[0] == m.env_n_faces + 3 * m.BNF
    sp = m.parse_views(c.inp, filter_transparent=True)
    assert sp.kept.tolist() == [True, False, True, False, True] and sp.n_blocks == 5
    _assert_equal(_raw(sp), _derive(c.frag, _face_labels(m, [0, 2, 4])), 'killed blocks')
    assert not sp.counts[:, [3, 5]].any() and bool((sp.counts[:, [2, 4, 6], 1].sum(0) > 0).all())
    assert not sp.amodal(1).any() and not sp.modal(3).any() and bool(torch.isnan(sp.occlusion()[:, [1, 3]]).all())
    # filter_transparent=False: kill_blocks still drops block 1, block 3 (opacity 0.27) is back under its own label
    loose = m.parse_views(c.inp, filter_transparent=False)
    assert loose.kept.tolist() == [True, False, True, True, True] and not loose.counts[:, 3].any() and int(loose.counts[:, 5, 0].sum()) > 0
    assert m.sync_free is False
    m.sync_free = True
    try:
        with torch.no_grad():
            m.build_blocks_scene(filter_transparent=False)                  # the state a training forward leaves behind
        alpha, keep = m._alpha, m._keep_mask
        assert keep is not None
        sf = m.parse_views(c.inp, filter_transparent=True)
        assert m.sync_free is True and m._alpha is alpha and m._keep_mask is keep
        for a, b in zip(_raw(sp), _raw(sf)):
            assert torch.equal(a, b)
    finally:
        m.sync_free = False


def test_without_the_sky_dome_empty_pixels_are_marked():
    """11: w_bkg=False: label 255 and depth -1 exactly where the oracle's list is empty."""
    H, W = 18, 27
    c = _case(H, W, w_bkg=False)
    m = c.model
    assert c.scene.faces.shape[0] == m.ground_n_faces + 5 * m.BNF
    sp = m.parse_views(c.inp, w_bkg=False)
    want = _derive(c.frag, _face_labels(m, c.kept, w_bkg=False))
    _assert_equal(_raw(sp), want, 'no sky dome')
    empty = (c.frag['pix_to_face'] < 0).all(-1)
    print(f'no sky dome: {int(empty.sum())} of {empty.numel()} pixels see nothing')
    assert 0 < int(empty.sum()) < empty.numel()
    assert torch.equal(sp.label.cpu() == 255, empty) and torch.equal(sp.depth.cpu() == -1, empty) and torch.equal(sp.cover.cpu() == 0, empty)
    assert not sp.counts[:, 0].any() and int(sp.counts[..., 1].sum()) == int((~empty).sum())
    assert bool((sp.colors()[:, :, empty[0]][0] == 1).all())                 # painted white


class _Loader(list):
    batch_size = 1


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _view_loader(inp):
    loader = _Loader([({k: v[i:i + 1] for k, v in inp.items()}, None) for i in range(3)])
    loader.dataset = types.SimpleNamespace()
    return loader


def _parent_file_set(files):
    ext = 'mp4' if any(f.endswith('.mp4') for f in files) else 'gif'
    meshes = ['mesh.mtl', 'mesh.obj', 'mesh.png', 'mesh_full.mtl', 'mesh_full.obj', 'mesh_full.png', f'rotated_mesh.{ext}']
    textures = [os.path.join('textures', n) for n in ['bkg.png', 'ground.png'] + [f'block_{k:02d}.png' for k in range(5)]]
    per_input = [f'{i}_{n}' for i in range(3) for n in ('inp.png', 'rec.png', 'rec_col.png', 'rec_col_inp.png', 'rec_syn_nobkg.png',
                                                         'rec_syn_nobkg_edged.png', f'rec_traj.{ext}', f'rec_traj_syn.{ext}')]
    return sorted(meshes + textures + per_input)


PARSE_FILES = sorted(os.path.join('parse', n) for n in ['block_visibility.tsv'] + [f'{n}_{v:03d}.{e}' for v in range(3)
                                                                                     for n, e in (('label', 'png'), ('depth', 'npy'), ('cover', 'npy'))])


def test_qualitative_eval_writes_the_parse_files(tmp_path):
    """10: the files of export.write_parse under <path>/parse, their content against the oracle derivation, the occlusion column against
    SceneParse.occlusion(); without the new argument the file set of the parent commit."""
    H, W = 40, 56
    c = _case(H, W)
    model, inp = c.model, c.inp
    loader = _view_loader(inp)
    model.qualitative_eval(loader, DEV, path=tmp_path / 'q', NV=4, parse=True)
    files = _files(tmp_path / 'q')
    assert [f for f in files if f.startswith('parse')] == PARSE_FILES
    assert [f for f in files if not f.startswith('parse')] == _parent_file_set(files)
    model.qualitative_eval(loader, DEV, path=tmp_path / 'plain', NV=4)
    assert _files(tmp_path / 'plain') == _parent_file_set(files)
    sp = model.parse_views(inp)
    want = _derive(c.frag, _face_labels(model, c.kept))
    for v in range(3):
        assert np.array_equal(np.load(tmp_path / 'q' / 'parse' / f'cover_{v:03d}.npy'), want[2][v].numpy())
        assert np.array_equal(np.load(tmp_path / 'q' / 'parse' / f'depth_{v:03d}.npy'), want[1][v].numpy())
    from PIL import Image
    png = torch.from_numpy(np.array(Image.open(tmp_path / 'q' / 'parse' / 'label_001.png').convert('RGB')))
    assert torch.equal(png, (sp.colors()[1].cpu().clamp(0, 1) * 255.0).to(torch.uint8).permute(1, 2, 0))
    assert len(torch.unique(png.reshape(-1, 3), dim=0)) >= 4                    # sky, ground and at least two blocks in their colours
    rows = [line.rstrip('\n').split('\t') for line in open(tmp_path / 'q' / 'parse' / 'block_visibility.tsv')]
    assert rows[0] == ['block', 'kept'] + [f'{n}_{v}' for v in range(3) for n in ('amodal', 'visible', 'occlusion')] and len(rows) == 6
    occ, (amodal, visible) = sp.occlusion().cpu(), [t.cpu() for t in sp.areas()]
    for k in range(5):
        assert rows[1 + k][:2] == [str(k), '1']
        for v in range(3):
            assert rows[1 + k][2 + 3 * v:5 + 3 * v] == [str(int(amodal[v, k])), str(int(visible[v, k])), '{:.5f}'.format(float(occ[v, k]))]
            assert math.isnan(float(occ[v, k])) or float(occ[v, k]) == 1 - int(visible[v, k]) / int(amodal[v, k])


def test_trainer_scores_the_parsed_foreground_against_masks(tmp_path):
    """10: Trainer.evaluate(masks = the oracle's foreground) writes a mask_iou of exactly 1.00000; its qualitative_eval, called without the
    new argument, writes the file set of the parent commit."""
    from collections import OrderedDict
    from dbw_amd.trainer import Trainer
    H, W = 18, 27
    c = _case(H, W)
    model, _, _, _ = _setup(H, W)                                            # (a model of its own: the trainer takes it over)
    loader = _view_loader(c.inp)
    cfg = {'training': {'batch_size': 1, 'n_epoches': 1, 'seed': 3, 'optimizer': {'name': 'adam', 'lr': 1e-3}, 'scheduler': {'name': 'multi_step'}}}
    tr = Trainer(cfg, model, c.inp)
    fg = _derive(c.frag, _face_labels(model, c.kept))[0] >= 2                # a block is entry 0 of the oracle's list
    masks = fg[:, None].float()                                              # (V,1,H,W), 0 / 1
    assert 0 < float(masks.mean()) < 1
    scores = tr.evaluate(loader, tmp_path / 'run', masks=masks)
    assert scores['masks']['mask_iou'] == 1.0 and 'n_blocks' in scores
    assert open(tmp_path / 'run' / 'mask_scores.tsv').read() == 'mask_iou\n1.00000\n'
    files = _files(tmp_path / 'run' / 'quali_eval')
    assert files == _parent_file_set(files)
    assert sorted(os.listdir(tmp_path / 'run')) == ['final_scores.tsv', 'mask_scores.tsv', 'quali_eval']
    # (V,H,W) bool masks are the same question; a wrong mask is seen; a wrong number of masks is refused
    assert tr._mask_scores(loader, DEV, fg, str(tmp_path / 'run'))['mask_iou'] == 1.0
    assert tr._mask_scores(loader, DEV, ~fg, str(tmp_path / 'run'))['mask_iou'] == 0.0
    with pytest.raises(ValueError, match='masks for'):
        tr._mask_scores(loader, DEV, masks[:2], str(tmp_path / 'run'))
    with pytest.raises(ValueError, match='at the image size'):
        tr._mask_scores(loader, DEV, masks[..., :-1], str(tmp_path / 'run'))
    # parse=True reaches qualitative_eval (which the test above runs for real)
    calls = []
    model.qualitative_eval = lambda *a, **k: calls.append(k)
    model.quantitative_eval = lambda *a, **k: OrderedDict(n_blocks=5)
    tr.evaluate(loader, tmp_path / 'run2', parse=True)
    tr.evaluate(loader, tmp_path / 'run2')
    assert calls[0].get('parse') is True and 'parse' not in calls[1]
