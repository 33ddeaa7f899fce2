"""Float64 yardstick for the render backward -- a helper of tests/test_render_ref64_host.py (CPU) and tests/test_gpu_render_ref64.py (GPU),
not a test.  DESIGN.md "Render backward against a float64 oracle".

Unit of error: the element-wise bar of tests/test_gpu_golden.py (assert_close, BASELINE.json's 1e-4),
    bars(a, b) = max_i |a_i - b_i| / (1e-4 * |b_i| + 1e-6 * max|b|),       b the float64 result.
For every compared tensor   y = bars(oracle fp32, oracle fp64)   (CPU only, deterministic)   and   k = bars(hip, oracle fp64);   the GPU
tests assert  k <= max(1, 4 * y):  one bar where fp32 can meet it, else four times (two bits) what the serial fp32 restatement of the same
operation loses -- one bit for the kernels' summation order (wave aggregation + atomics against the oracle's serial loop), one for v_exp_f32
and the shared-reciprocal division of the fused kernels.  The host test holds every case to y <= 10, so that 4 * y still means something.

Every reference is computed once per process (functools.lru_cache) and shared by the cases that run the kernels in another configuration;
callers must not write into what they get."""
import functools

import torch

import oracle as O

Y_CAP = 10.0                   # host precondition 1: the fp32 oracle itself within ten bars of the fp64 one
FACTOR = 4.0                   # k <= max(1, FACTOR * y)
MAX_MASKED_PIXELS = 0.02       # host precondition 2: share of pixels whose discrete decisions differ between fp32 and fp64
MIN_INSIDE, MIN_OUTSIDE = 0.40, 0.20   # host precondition 3 (operator-level raster cases)
AMP_CAP = 64.0                 # fragments whose barycentrics amplify rounding by more than this carry no bary / zbuf upstream
MAX_AMP_MASKED = 0.01


def bars(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    assert a.shape == b.shape and b.dtype == torch.float64
    if b.numel() == 0 or float(b.abs().max()) == 0.0:
        return 0.0 if a.numel() == 0 or float(a.abs().max()) == 0.0 else float('inf')
    tol = 1e-4 * b.abs() + 1e-6 * b.abs().max()
    return float(((a - b).abs() / tol).max())


def yardstick(o32, o64):
    return bars(o32, o64)


def assert_within(hip, o32, o64, name, record=None):
    """The assertion that goes with the yardstick; records y and k (record = pytest's record_property) and returns them."""
    y, k = yardstick(o32, o64), bars(hip, o64)
    if record is not None:
        record(f'y_{name}', round(y, 4))
        record(f'k_{name}', round(k, 4))
    print(f'{name}: y = {y:.3f}  k = {k:.3f}  bound = {max(1.0, FACTOR * y):.3f}')
    assert k <= max(1.0, FACTOR * y), f'{name}: k = {k:.3f} bars > max(1, {FACTOR:g} * y), y = {y:.3f}'
    return y, k


# ---------------------------------------------------------------------------------------------------------------------
# operator-level rasteriser backward
# ---------------------------------------------------------------------------------------------------------------------
RASTER_SHAPES = [(40, 56, 5, 80, 2e-3, 11), (45, 61, 16, 150, 1e-3, 7), (23, 29, 25, 120, 2e-3, 9), (17, 70, 1, 40, 0.0, 5)]   # H, W, K, nf, blur, seed
RASTER_SWITCHES = [(True, True), (True, False), (False, True), (False, False)]        # perspective_correct, clip_barycentric
RASTER_STREAMS = ['all', 'z', 'bary', 'dists']


def random_faces(n_faces, seed, zmin=0.5, zmax=5.0, spread=1.2, size=0.5):
    """tests/test_gpu_parity.py: random_faces (that module needs a GPU build to import)."""
    g = torch.Generator().manual_seed(seed)
    c = (torch.rand(n_faces, 1, 2, generator=g) * 2 - 1) * spread
    xy = c + (torch.rand(n_faces, 3, 2, generator=g) * 2 - 1) * size
    z = torch.rand(n_faces, 3, 1, generator=g) * (zmax - zmin) + zmin
    return torch.cat([xy, z], -1).contiguous()


def pixel_centres_f64(H, W):
    """NDC pixel centres in fp64 -> (ys (H,), xs (W,)), through the oracle's own pix_to_ndc."""
    lib = O.lib()
    ys = torch.tensor([lib.dbw_ref_pix_to_ndc_f64(H - 1 - y, H, W) for y in range(H)], dtype=torch.float64)
    xs = torch.tensor([lib.dbw_ref_pix_to_ndc_f64(W - 1 - x, W, H) for x in range(W)], dtype=torch.float64)
    return ys, xs


def fragment_masks_f64(fv, p2f, persp):
    """Per fragment, in fp64 from the plain barycentrics w of the pixel centre: valid, inside (every w_i > 0: the sign the rasteriser
    gives the distance), amplification = sum|w_i / z_i| / |sum w_i / z_i| under perspective correction, sum|w_i| otherwise -- the factor by
    which the rounding of the w_i grows in the normalised barycentrics (w sums to 1, so it is 1 inside a face)."""
    N, H, W, K = p2f.shape
    fv = fv.double()
    ys, xs = pixel_centres_f64(H, W)
    valid = p2f >= 0
    f = fv[p2f.clamp(min=0)]                                     # (N,H,W,K,3,3)
    px, py = xs.view(1, 1, W, 1), ys.view(1, H, 1, 1)

    def edge(ax, ay, bx, by, qx, qy):
        return (qx - ax) * (by - ay) - (qy - ay) * (bx - ax)
    x0, y0, x1, y1, x2, y2 = f[..., 0, 0], f[..., 0, 1], f[..., 1, 0], f[..., 1, 1], f[..., 2, 0], f[..., 2, 1]
    area = edge(x0, y0, x1, y1, x2, y2) + 1e-8
    w = torch.stack([edge(x1, y1, x2, y2, px, py), edge(x2, y2, x0, y0, px, py), edge(x0, y0, x1, y1, px, py)], -1) / area[..., None]
    inside = valid & (w > 0).all(-1)
    if persp:
        t = w / f[..., :, 2]
        amp = t.abs().sum(-1) / t.sum(-1).abs().clamp(min=1e-300)
    else:
        amp = w.abs().sum(-1)
    return valid, inside, torch.where(valid, amp, torch.zeros_like(amp))


@functools.lru_cache(maxsize=None)
def raster_case(shape, switches):
    """One operator-level case: scene, fp32 forward, masked upstream, and the fp32 / fp64 oracle gradient of every stream.
    Two meshes of different face counts packed back to back (two images); upstream randn from generator seed 3.  With both switches on,
    the zbuf and bary upstream is zero on fragments outside their face (signed distance >= 0): beyond the line through the blur band on
    which the perspective denominator vanishes it is clamped to 1e-8, and the fp32 backward of such a fragment is rounding noise times 1e16
    (tests/test_render_ref64_host.py settles that against fp64 finite differences); no pass of the model feeds a fragment outside its face
    a bary or zbuf gradient.  In the other three combinations it is zero on fragments whose amplification exceeds AMP_CAP.  The dists
    upstream is everywhere."""
    H, W, K, nf, blur, seed = shape
    persp, clipb = switches
    fv = torch.cat([random_faces(nf, seed), random_faces(nf, seed + 1)], 0)
    first, num = torch.tensor([0, nf]), torch.tensor([nf, nf - 7])
    fwd = O.rasterize_fwd_raw(fv, first, num, None, (H, W), blur, K, persp, clipb, n_threads=8)
    p2f = fwd[0]
    g = torch.Generator().manual_seed(3)
    gz, gb, gd = torch.randn(fwd[1].shape, generator=g), torch.randn(fwd[2].shape, generator=g), torch.randn(fwd[3].shape, generator=g)
    valid, inside, amp = fragment_masks_f64(fv, p2f, persp)
    drop = (valid & ~inside) if (persp and clipb) else (amp > AMP_CAP)
    keep = (~drop).float()
    gz, gb = gz * keep, gb * keep[..., None]
    zero = [torch.zeros_like(gz), torch.zeros_like(gb), torch.zeros_like(gd)]
    up = {'all': [gz, gb, gd], 'z': [gz, zero[1], zero[2]], 'bary': [zero[0], gb, zero[2]], 'dists': [zero[0], zero[1], gd]}
    o32 = {s: O.rasterize_bwd_raw(fv, p2f, *u, persp, clipb) for s, u in up.items()}
    o64 = {s: O.rasterize_bwd_raw(fv.double(), p2f, *[t.double() for t in u], persp, clipb) for s, u in up.items()}
    nv = max(int(valid.sum()), 1)
    return dict(fv=fv, first=first, num=num, fwd=fwd, up=up, o32=o32, o64=o64, valid=valid, inside=inside, amp=amp,
                inside_share=int(inside.sum()) / nv, outside_share=int((valid & ~inside & (gd != 0)).sum()) / nv,
                amp_masked=(0.0 if (persp and clipb) else int((valid & drop).sum()) / nv))


# ---------------------------------------------------------------------------------------------------------------------
# projection + z clipping backward
# ---------------------------------------------------------------------------------------------------------------------
def camera_inside_scene(seed, B=3):
    """tests/test_gpu_parity.py: _camera_inside_scene -- a closed icosphere around the cameras, many faces straddle z = z_clip."""
    torch.manual_seed(seed)
    verts, faces = O.get_icosphere(2, flip_faces=True)
    verts = verts * 3.0 + 0.05 * torch.randn_like(verts)
    C = torch.randn(B, 3) * 0.4
    R, T = O.look_at_cameras(C, at=(0.3, 0.2, 2.5))
    Kmat = torch.tensor([[2.1, 0, 0.05, 0], [0, 2.1, -0.03, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=torch.float32)
    return verts, faces, R, T, Kmat


Z_CLIP = 0.25


@functools.lru_cache(maxsize=None)
def project_clip_case(persp):
    """Vertex gradient of  sum(clipped face_verts * g)  by autograd through O.transform_to_ndc and O.clip_faces, in fp32 and in fp64.
    g (B, 2F, 3, 3) in the library's slot layout (view b's clipped faces in [b, :num_faces[b]]); the oracle packs the views back to back."""
    verts, faces, R, T, Kmat = camera_inside_scene(3, B=7)
    B, Fs = R.shape[0], faces.shape[0]
    g = torch.randn(B, 2 * Fs, 3, 3, generator=torch.Generator().manual_seed(1))
    out = {}
    for dt in (torch.float32, torch.float64):
        v = verts.detach().to(dt).clone().requires_grad_(True)
        ndc = O.transform_to_ndc(v, R.to(dt), T.to(dt), Kmat.to(dt), 1e-8)
        fv = ndc[:, faces].reshape(B * Fs, 3, 3)
        cl = O.clip_faces(fv, torch.arange(B) * Fs, torch.full((B,), Fs), Z_CLIP, persp)
        gp = torch.cat([g[b, :int(cl['num_faces'][b])] for b in range(B)]).to(dt)
        (cl['face_verts'] * gp).sum().backward()
        out[dt] = dict(grad=v.grad.detach(), cl={k: (t.detach() if torch.is_tensor(t) else t) for k, t in cl.items()})
    return dict(verts=verts, faces=faces, R=R, T=T, Kmat=Kmat, g=g, o32=out[torch.float32], o64=out[torch.float64])


# ---------------------------------------------------------------------------------------------------------------------
# full passes
# ---------------------------------------------------------------------------------------------------------------------
def _model(seed=3, n_blocks=4, ts=32, hw=(48, 64), fpp=6):
    m = O.OracleDBW(hw, n_blocks=n_blocks, txt_size=ts, faces_per_pixel=fpp, seed=seed)
    R, T, Km = O.synthetic_cameras(3, R_world=m.R_world[0], dist=2.8)
    return m, R, T, Km


def _block_alpha(m, scene):
    return (torch.rand(scene['faces'].shape[0] // m.BNF, generator=torch.Generator().manual_seed(1)) * 0.8 + 0.1).repeat_interleave(m.BNF)


def _soft(fpp, hw=(48, 64), clip_inside=True, ts=32, decimate=0, seed=3):
    """decimate d: the maps are the nearest-upsampled copy of their d x d cell averages (dbw.py:331-334), as the decimated training phase
    renders them.  The maps of the scene carry the circular padding `pads` = m.txt_padding in u."""
    m, R, T, Km = _model(seed=seed, fpp=fpp, hw=hw, ts=ts)
    m.decim_factor = decimate or m.decim_factor
    with torch.no_grad():
        scene = m.build_blocks(True, True, bool(decimate), None, kill_blocks=False)
    bg = (0., 0., 0.) if clip_inside else (0.1, 0.2, 0.3)
    return dict(scene=scene, R=R, T=T, Kmat=Km[0], H=hw[0], W=hw[1], sigma=1e-4, K=fpp, detach_bary=True, faces_alpha=_block_alpha(m, scene), bg=bg,
                clip_inside=clip_inside, const_faces=0, pads=tuple(m.txt_padding), decimate=decimate)


def _fine():
    """Model seed 6: with seed 5 (test_render_fine_pass_no_alpha_matches_oracle) the fp32 oracle's own texel gradient is 13.2 bars from the
    fp64 one (sigma = 5e-6 turns the rounding of a distance into 1e-3 of an opacity), over Y_CAP; the next seed holds it (5.8)."""
    m, R, T, Km = _model(seed=6)
    with torch.no_grad():
        scene = m.build_blocks(True, False, False, None, kill_blocks=False)
    return dict(scene=scene, R=R, T=T, Kmat=Km[0], H=48, W=64, sigma=5e-6, K=6, detach_bary=True, faces_alpha=None, bg=(0., 0., 0.), clip_inside=True,
                const_faces=0)


def _env(rig, hw=(48, 64), const=False, seed=7, decimate=0):
    m, _, _, _ = _model(seed=seed, ts=16, hw=hw)
    m.decim_factor = decimate or m.decim_factor
    R, T, Km = O.synthetic_cameras(3, R_world=m.R_world[0], dist=2.8, elev_deg=rig[0], f_ndc=rig[1])
    with torch.no_grad():
        scene = m.build_env(True, bool(decimate))
    nsky = int((scene['face_map'] == 0).sum())
    return dict(scene=scene, R=R, T=T, Kmat=Km[0], H=hw[0], W=hw[1], sigma=0.0, K=1, detach_bary=False, faces_alpha=None, bg=(0.1, 0.2, 0.3),
                clip_inside=True, const_faces=nsky if const else 0, pads=(0, 0), decimate=decimate)


RENDER_CASES = {
    'soft6': lambda: _soft(6), 'soft16': lambda: _soft(16), 'soft25': lambda: _soft(25), 'fine': _fine,
    'env_down': lambda: _env((30.0, 4.82)), 'env_horizon': lambda: _env((5.0, 1.5)),
    'sigmoid6': lambda: _soft(6, clip_inside=False),                 # clip_inside=False, detached barycentrics
    'const_faces': lambda: _env((5.0, 1.5), const=True),             # the sky dome's vertices are constants
    # 45x61 is no multiple of the 8x8 / 16x16 tiles.  The environment's geometry is fixed, the seed draws its textures: the ground's large
    # faces at a grazing angle (some clipped at the near plane) leave one or two vertex-gradient entries whose fp32 error depends on them.
    # Seed 7 at this size measures y(g_verts) = 1.7 with the vectorised CPU kernels of torch but 9.7 with the scalar ones (6.6 on another
    # host), seed 8 measures 51; seed 9 holds 2.5 / 3.1 -- a case that sits at the cap on some host would make the host test a coin toss.
    'soft6_45x61': lambda: _soft(6, hw=(45, 61)), 'env_45x61': lambda: _env((5.0, 1.5), hw=(45, 61), seed=9),
}
# The texel-gradient accumulators of a training step (DESIGN.md "Texel-gradient accumulators against a float64 scatter").  A VARIANT hands
# the library the same scene in the form a training phase stores it, and the oracle's map gradient is brought into that form:
#   'bins'       full-resolution maps WITHOUT their circular padding (+ the wrap in the descriptor) and the texture-space bins of
#                describe_bins, lds_aggregate off: records + dbw_texbin_reduce, wrapped footprints through the atomic fallback of the same pass;
#   'decimated'  cell-resolution maps + descriptor shift 2 (LdsAgg when lds_aggregate is on, wave-aggregated atomics otherwise); the case's
#                maps are the nearest-upsampled copy of the cells, the gradient of a cell is the sum over its 4x4 texels.
# 64x64 maps: four bins per map, bilinear footprints cross from one into the halo of the next.  At 48x64 pixels such a map is minified and
# its texel gradients are sums of few, unevenly weighted fragments: the fp32 oracle's own y(g_maps) measures 7.5, 10.9, 7.2, 26, 8.0, 9.3,
# 9.5, 90 for model seeds 3 ... 10 -- at or near the cap -- and 5.2 for seed 12, which is taken.
SHIFT = 2
VARIANT_CASES = {
    'soft6_ts64': lambda: _soft(6, ts=64, seed=12),
    'soft6_dec4': lambda: _soft(6, decimate=1 << SHIFT), 'env_horizon_dec4': lambda: _env((5.0, 1.5), decimate=1 << SHIFT),
}
PLAIN_CASES = list(RENDER_CASES)                         # what the 'plain' variant runs (as before)
RENDER_CASES.update(VARIANT_CASES)
RENDER_VARIANTS = {'bins': ['soft6', 'soft16', 'soft6_45x61', 'soft6_ts64'], 'decimated': ['soft6_dec4', 'env_horizon_dec4']}
RENDER_WEIGHTS = ['all', 'rgb', 'alpha']      # upstream on every channel / the colour channels only / the opacity channel only
TENSORS = ['image', 'g_verts', 'g_maps', 'g_alpha']


@functools.lru_cache(maxsize=None)
def render_case(name):
    return RENDER_CASES[name]()


def _oracle_render(c, dt, w, n_threads=8):
    sc = c['scene']
    verts = sc['verts'].detach().to(dt).requires_grad_(True)
    maps = [m.detach().to(dt).requires_grad_(True) for m in sc['maps']]
    fa = None if c['faces_alpha'] is None else c['faces_alpha'].detach().to(dt).requires_grad_(True)
    scene = dict(sc, verts=verts, maps=maps, face_uvs=sc['face_uvs'].to(dt))
    B = c['R'].shape[0]
    fa_rep = None if fa is None else fa.repeat(B)
    img, frag = O.render(scene, c['R'].to(dt), c['T'].to(dt), c['Kmat'].to(dt), (c['H'], c['W']), c['sigma'], c['K'], c['detach_bary'], fa_rep, 0.001,
                         c['bg'], n_threads=n_threads, return_fragments=True, clip_inside=c['clip_inside'])
    res = {'image': img.detach()}
    if w is not None:
        (img * w.to(dt)).sum().backward()
        res['g_maps'] = torch.cat([(m.grad if m.grad is not None else torch.zeros_like(m)).reshape(-1) for m in maps])
        gv = verts.grad if verts.grad is not None else torch.zeros_like(verts)
        if c['const_faces']:
            # const_faces: the vertices only the first `const_faces` faces use get no gradient (sky and ground share no vertex)
            only = torch.ones(verts.shape[0], dtype=torch.bool)
            only[sc['faces'][c['const_faces']:].reshape(-1).long()] = False
            gv = gv * (~only)[:, None].to(dt)
        res['g_verts'] = gv
        if fa is not None:
            res['g_alpha'] = fa.grad
    return res, frag


@functools.lru_cache(maxsize=None)
def render_refs(name, weight='all', seed=0):
    """The oracle in fp32 and in fp64 on one case -> dict(o32, o64, w, M, masked).  M (B,1,H,W): the pixels on which all K pix_to_face
    entries and all signs of dists agree between the two; the upstream image weight w (torch.rand from generator `seed`, restricted to the
    channels of `weight`) is multiplied by M in every evaluation, so a discrete decision that rounding moves is in nobody's gradient."""
    c = render_case(name)
    with torch.no_grad():
        f32 = _oracle_render(c, torch.float32, None)[1]
        f64 = _oracle_render(c, torch.float64, None)[1]
    same = (f32['pix_to_face'] == f64['pix_to_face']) & ((f32['dists'] > 0) == (f64['dists'] > 0)) & ((f32['dists'] < 0) == (f64['dists'] < 0))
    M = same.all(-1)[:, None].float()
    B = c['R'].shape[0]
    w = torch.rand((B, 4, c['H'], c['W']), generator=torch.Generator().manual_seed(seed))
    if weight == 'rgb':
        w[:, 3] = 0
    elif weight == 'alpha':
        w[:, :3] = 0
    else:
        assert weight == 'all'
    w = w * M
    o32 = _oracle_render(c, torch.float32, w)[0]
    o64 = _oracle_render(c, torch.float64, w)[0]
    return dict(o32=o32, o64=o64, w=w, M=M, masked=1.0 - float(M.mean()), p2f=f32['pix_to_face'])


def stored_maps(c, variant='plain'):
    """The maps of a case as `variant` stores them -> (maps [(h, w, 3)], full-resolution shapes [(h, w)], pads (pl, pr), shift)."""
    maps = [m.detach() for m in c['scene']['maps']]
    if variant == 'plain':
        return maps, [m.shape[:2] for m in maps], (0, 0), 0
    pl, pr = c['pads']
    unpadded = [m[:, pl:m.shape[1] - pr] for m in maps]
    shapes = [m.shape[:2] for m in unpadded]
    if variant == 'bins':
        return unpadded, shapes, (pl, pr), 0
    assert variant == 'decimated' and c['decimate'] == 1 << SHIFT
    d = c['decimate']
    cells = [m[::d, ::d].contiguous() for m in unpadded]
    for m, cell in zip(unpadded, cells):                        # the case's maps ARE the nearest-upsampled copy of the cells
        assert m.shape[0] % d == 0 and m.shape[1] % d == 0 and torch.equal(cell.repeat_interleave(d, 0).repeat_interleave(d, 1), m)
    return cells, shapes, (pl, pr), SHIFT


def stored_map_grads(c, g_flat, variant='plain'):
    """The oracle's gradient of the case's (padded, full-resolution) maps, flat -> the gradient of the maps of stored_maps(c, variant), flat:
    a padding column is a copy of the column it wraps to (F.pad circular: the last pl columns on the left, the first pr on the right) and
    hands its gradient to it; a cell takes the sum over its texels."""
    if variant == 'plain':
        return g_flat
    pl, pr = c['pads']
    out, at = [], 0
    for m in c['scene']['maps']:
        h, wp = m.shape[:2]
        g = g_flat[at:at + h * wp * 3].reshape(h, wp, 3)
        at += h * wp * 3
        w = wp - pl - pr
        u = g[:, pl:pl + w].clone()
        if pl:
            u[:, w - pl:] += g[:, :pl]
        if pr:
            u[:, :pr] += g[:, pl + w:]
        if variant == 'decimated':
            d = c['decimate']
            u = u.reshape(h // d, d, w // d, d, 3).sum((1, 3))
        out.append(u.reshape(-1))
    assert at == g_flat.numel()
    return torch.cat(out)


def hip_render(name, w, lds, variant='plain'):
    """The library on the same case with the same (masked) upstream weight -> dict like the oracle's.  ops.FUSED_FORWARD / FUSED_BACKWARD are
    the caller's to set.  variant: how the maps are stored (stored_maps); 'bins' also hands the pass its texture-space bins."""
    from dbw_amd import ops
    from dbw_amd.structures import PackedScene
    DEV = 'cuda:0'
    c = render_case(name)
    scene = c['scene']
    maps, shapes, pads, shift = stored_maps(c, variant)
    desc, n_floats = PackedScene.describe_maps(shapes, [pads] * len(maps), DEV, shift=shift)
    flat = torch.cat([m.reshape(-1) for m in maps]).detach().to(DEV)
    assert flat.numel() == n_floats
    ps = PackedScene(scene['verts'].detach().to(DEV), scene['faces'].to(torch.int32).to(DEV), scene['face_uvs'].float().to(DEV),
                     scene['face_map'].to(torch.int32).to(DEV), desc, flat)
    ps.verts.requires_grad_(True)
    ps.maps.requires_grad_(True)
    fa = None if c['faces_alpha'] is None else c['faces_alpha'].detach().to(DEV).requires_grad_(True)
    texbins = None
    if variant == 'bins':
        assert not lds and ops.TEXTURE_BINS
        texbins = PackedScene.describe_bins(shapes, DEV)
    cfg = ops.RenderCfg(c['H'], c['W'], c['K'], c['sigma'], 0.001, True, c['detach_bary'], scene['faces'].shape[0], lds_aggregate=lds, texbins=texbins,
                        clip_inside=c['clip_inside'], const_faces=c['const_faces'])
    img = ops.render_scene(ps.verts, ps.maps, fa, ps.faces, c['R'].to(DEV), c['T'].to(DEV), c['Kmat'].to(DEV), ps.face_uvs, ps.face_map,
                           ps.map_desc, ops.make_bg(c['bg']), cfg)
    (img * w.to(DEV)).sum().backward()
    res = {'image': img.detach(), 'g_maps': ps.maps.grad, 'g_verts': ps.verts.grad}
    if fa is not None:
        res['g_alpha'] = fa.grad
    return res


def render_three_ways(name, weight='all', lds=False, seed=0, hip=True, variant='plain'):
    """_render_both of tests/test_gpu_parity.py with a third leg: {tensor: (hip or None, oracle fp32, oracle fp64)} and the reference record.
    variant: the library renders from the maps as stored_maps keeps them, and both oracle map gradients are brought into that form."""
    ref = render_refs(name, weight, seed)
    got = hip_render(name, ref['w'], lds, variant) if hip else {}
    out = {t: (got.get(t), ref['o32'][t], ref['o64'][t]) for t in TENSORS if t in ref['o64']}
    out['g_maps'] = (out['g_maps'][0],) + tuple(stored_map_grads(render_case(name), g, variant) for g in out['g_maps'][1:])
    # the image on the pixels of M only (elsewhere the evaluations may have picked different faces)
    out['image'] = tuple(None if i is None else i.detach().cpu().double() * ref['M'].double() for i in out['image'])
    return out, ref
