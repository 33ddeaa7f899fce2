"""Checker side: plain float64 references (numpy) of the model-side kernels of csrc/texture.hip and csrc/model_ops.hip, written from the
formulas of the reference project (src/model/dbw.py:223,273-311,331-334,343-352,366-405, src/model/loss.py:46, src/utils/superquadric.py:10-38,
src/utils/pytorch.py:31-36, src/optimizer.py:6-18 = torch.optim.Adam, pytorch3d's rotation_6d_to_matrix) -- not from the kernels.

Every function takes the float32 inputs the kernel gets, promotes them to float64 and returns a dict: the value and every gradient, and
next to each output `X` a magnitude `M_X` of the same shape: the float64 sum of the absolute values of the terms that make up the element
(a cancelling sum keeps the size of what cancelled; a chain of linear maps is pushed through with the maps' absolute values).  The error
of a float32 result is measured with `err` below: per element, against M, with a floor of the smallest normal float32 per summed term.

tests/test_model_kernels_ref_host.py holds every function here against torch float64 autograd of the same expression (1e-12)."""
import numpy as np

F32_TINY = float(np.finfo(np.float32).tiny)          # 2^-126, the smallest normal float32
SAFE_POW_EPS = 1e-6                                  # pytorch.py:35 (SQRT_EPS)
CLAMP = 5.0                                          # superquadric.py:24


def f64(x):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def err(got, ref, M, count=1):
    """max over elements of |got - ref| / (M + tiny), tiny = count x the smallest normal float32 (count: the number of terms of the
    element's reduction).  A difference of at most `tiny` itself does not count: sigmoid(-90) = 8e-40 is below the normal float32 range, the
    kernels (and torch) return 0 for it, and 8e-40 against M + tiny = 8e-40 + 1.2e-38 would otherwise read as an error of 0.06.
    A NaN or inf in `got` is an infinite error."""
    got, ref, M = f64(got), f64(ref), f64(M)
    assert got.shape == ref.shape == M.shape, (got.shape, ref.shape, M.shape)
    if got.size == 0:
        return 0.0
    tiny = F32_TINY * count
    e = np.maximum(np.abs(got - ref) - tiny, 0.0) / (M + tiny)
    e = np.where(np.isfinite(got), e, np.inf)
    return float(e.max())


def f32v(x):
    """a scalar argument as the C ABI receives it: rounded to float32"""
    return float(np.float32(x))


def sigmoid(x):
    x = f64(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


# ---- texture preparation (dbw.py:273-278,288-293,306,331-334) ---------------------------------------------------------------------------
def _cells(x, d):
    n, h, w, c = x.shape
    return x.reshape(n, h // d, d, w // d, d, c)


def _up(x, d):
    return np.repeat(np.repeat(x, d, axis=1), d, axis=2)


def texture_prep_fwd(tex, d):
    """tex (n,h,w,3) logits -> sig = sigmoid(tex), maps = avg_pool(sig, d) at cell resolution (n,h/d,w/d,3)"""
    s = sigmoid(tex)
    maps = _cells(s, d).mean(axis=(2, 4))
    return dict(sig=s, M_sig=s, maps=maps, M_maps=maps)


def texture_prep_bwd(tex, d, gmaps, gsig=None):
    """gtex = (gmaps[cell] / d^2 + gsig) s (1 - s)"""
    s = sigmoid(tex)
    gc = _up(f64(gmaps), d) / (d * d)
    gs = np.zeros_like(s) if gsig is None else f64(gsig)
    ds = s * (1.0 - s)
    return dict(gtex=(gc + gs) * ds, M_gtex=(np.abs(gc) + np.abs(gs)) * ds)


# ---- TV (dbw.py:378-387, loss.py:46) --------------------------------------------------------------------------------------------------
def tv_l2sq(maps, wrap, scale=1.0):
    """maps (n,h,w,3): scale * [sum dx^2 / (h (w - 1 + wrap)) + sum dy^2 / ((h - 1) w)], the sums over all maps (dbw.py:385); with `wrap`
    the x differences close the seam (dbw.py:383: diff(..., append=first column)).  -> value, grad (d value / d maps)"""
    m, scale = f64(maps), f32v(scale)
    n, h, w, _ = m.shape
    sx, sy = 1.0 / (h * (w - 1 + (1 if wrap else 0))), 1.0 / ((h - 1) * w)
    dx = (np.roll(m, -1, axis=2) - m) if wrap else (m[:, :, 1:] - m[:, :, :-1])
    dy = m[:, 1:] - m[:, :-1]
    value = scale * ((dx ** 2).sum() * sx + (dy ** 2).sum() * sy)
    g, M = np.zeros_like(m), np.zeros_like(m)
    tx, ty = 2.0 * scale * sx * dx, 2.0 * scale * sy * dy
    if wrap:
        g += np.roll(tx, 1, axis=2) - tx
        M += np.abs(np.roll(tx, 1, axis=2)) + np.abs(tx)
    else:
        g[:, :, 1:] += tx; g[:, :, :-1] -= tx
        M[:, :, 1:] += np.abs(tx); M[:, :, :-1] += np.abs(tx)
    g[:, 1:] += ty; g[:, :-1] -= ty
    M[:, 1:] += np.abs(ty); M[:, :-1] += np.abs(ty)
    return dict(value=value, M_value=abs(value), grad=g, M_grad=M, terms=dx.size + dy.size)


# ---- decoupled composite + MSE (dbw.py:223,366-367) -------------------------------------------------------------------------------------
def composite_mse(fg, env, img=None, scale=1.0, up=1.0):
    """fg, env (N,4,H,W), img (N,3,H,W) or None.  rec = fg_rgb mask + (1 - mask) env_rgb; value = scale sum (rec - img)^2; gfg, genv =
    d (up value) / d fg, env (N,4,H,W; genv's channel 3 is zero)."""
    f, e, scale, up = f64(fg), f64(env), f32v(scale), f32v(up)
    m = f[:, 3:4]
    t1, t2 = f[:, :3] * m, (1.0 - m) * e[:, :3]
    out = dict(rec=t1 + t2, M_rec=np.abs(t1) + np.abs(t2))
    if img is None:
        return out
    t = f64(img)
    d, Md = out['rec'] - t, out['M_rec'] + np.abs(t)
    out['value'] = scale * (d ** 2).sum()
    out['M_value'] = abs(out['value'])
    k = 2.0 * scale * up
    gr, Mgr = k * d, abs(k) * Md
    gfg, Mfg, genv, Menv = np.zeros_like(f), np.zeros_like(f), np.zeros_like(e), np.zeros_like(e)
    gfg[:, :3], Mfg[:, :3] = gr * m, Mgr * np.abs(m)
    gfg[:, 3], Mfg[:, 3] = (gr * (f[:, :3] - e[:, :3])).sum(1), (Mgr * (np.abs(f[:, :3]) + np.abs(e[:, :3]))).sum(1)
    genv[:, :3], Menv[:, :3] = gr * (1.0 - m), Mgr * np.abs(1.0 - m)
    out.update(gfg=gfg, M_gfg=Mfg, genv=genv, M_genv=Menv)
    return out


# ---- Adam (optimizer.py:6-18: torch.optim.Adam, no weight decay, no amsgrad) -------------------------------------------------------------
def adam(p, g, m, v, step, lr, beta1, beta2, eps):
    """One step from a given state; lr a scalar or per element (parameter groups differ in lr only).  beta1, beta2, eps, lr: the float32
    values the C ABI receives."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    b1, b2, eps = float(np.float32(beta1)), float(np.float32(beta2)), float(np.float32(eps))
    lr = f64(np.asarray(lr, dtype=np.float32))
    t1, t2 = b1 * m, (1.0 - b1) * g
    m1, Mm = t1 + t2, np.abs(t1) + np.abs(t2)
    v1 = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v1) / np.sqrt(1.0 - b2 ** step) + eps
    ss = lr / (1.0 - b1 ** step)
    return dict(p=p - ss * m1 / denom, M_p=np.abs(p) + ss * Mm / denom, m=m1, M_m=Mm, v=v1, M_v=v1)


def group_lr(group_end, lrs, n):
    """per-element learning rate of contiguous groups [end[k-1], end[k])"""
    out = np.empty(n, dtype=np.float32)
    lo = 0
    for e, lr in zip(group_end, lrs):
        out[lo:e] = lr
        lo = e
    assert lo == n
    return out


# ---- block opacities (dbw.py:297-311), parsimony (dbw.py:373-377, pytorch.py:35) --------------------------------------------------------
def block_alpha_fwd(logit, noise, noise_scale, thresh):
    lg = f64(logit)
    x = lg if noise is None else lg + float(np.float32(noise_scale)) * f64(noise)
    a = sigmoid(x)
    clean = sigmoid(lg)
    keep = (clean > float(np.float32(thresh))) if thresh >= 0 else np.ones(lg.shape, dtype=bool)
    return dict(alpha=a, M_alpha=a, alpha_full=a * keep, M_alpha_full=a * keep, keep=keep, clean=clean)


def block_alpha_bwd(alpha, keep, g_alpha, g_alpha_full):
    """alpha (Kb) as the kernel reads it; g_alpha (Kb, parts) or None; g_alpha_full (Kb) or None; keep (Kb) or None (all kept)"""
    a = f64(alpha)
    g, M = np.zeros_like(a), np.zeros_like(a)
    if g_alpha is not None:
        g += f64(g_alpha).sum(1); M += np.abs(f64(g_alpha)).sum(1)
    if g_alpha_full is not None:
        k = np.ones_like(a) if keep is None else (np.asarray(keep) != 0)
        g += k * f64(g_alpha_full); M += k * np.abs(f64(g_alpha_full))
    return dict(g_logit=g * a * (1 - a), M_g_logit=M * a * (1 - a))


def sqrt_mean(x, eps, scale):
    """scale mean(clamp(x, eps)^0.5); grad = 0 where x <= eps (the clamp passes no gradient; at x == eps torch's clamp does, the kernel's
    `x > eps` does not: callers keep away from it or state the side)"""
    x = f64(x)
    eps, scale = float(np.float32(eps)), float(np.float32(scale))
    r = np.sqrt(np.maximum(x, eps))
    value = scale * r.mean()
    grad = np.where(x > eps, scale * 0.5 / r / x.size, 0.0)
    return dict(value=value, M_value=abs(scale) * r.mean(), grad=grad, M_grad=np.abs(grad))


# ---- 6D rotation (pytorch3d rotation_6d_to_matrix) ----------------------------------------------------------------------------------------
def rot6d(a6):
    """a6 (...,6) -> R (...,3,3) with rows b1, b2, b3"""
    a6 = f64(a6)
    a1, a2 = a6[..., :3], a6[..., 3:]
    b1 = a1 / np.linalg.norm(a1, axis=-1, keepdims=True)
    u = a2 - (b1 * a2).sum(-1, keepdims=True) * b1
    b2 = u / np.linalg.norm(u, axis=-1, keepdims=True)
    return np.stack([b1, b2, np.cross(b1, b2)], axis=-2)


def rot6d_bwd(a6, G):
    """a6 (6), G (3,3) = d L / d R -> d L / d a6 (6)"""
    a6, G = f64(a6), f64(G)
    a1, a2 = a6[:3], a6[3:]
    n1 = np.linalg.norm(a1)
    b1 = a1 / n1
    d = b1 @ a2
    u = a2 - d * b1
    n2 = np.linalg.norm(u)
    b2 = u / n2
    gb1 = G[0] + np.cross(b2, G[2])
    gb2 = G[1] + np.cross(G[2], b1)
    gu = (gb2 - b2 * (b2 @ gb2)) / n2
    ga2 = gu - (gu @ b1) * b1
    gb1 = gb1 - (gu @ b1) * a2 - d * gu
    ga1 = (gb1 - b1 * (b1 @ gb1)) / n1
    return np.concatenate([ga1, ga2])


def rot6d_bwd_M(a6, MG):
    """the magnitude of rot6d_bwd's result: the same chain with every sum taken over absolute values (MG (3,3) >= 0 the magnitude of G).
    Not |Jacobian| @ MG: the chain's own differences (gb - b (b . gb), gu - (gu . b1) b1) cancel, and an element of the 6-vector that
    comes out near 0 is still made of terms of the size of its neighbours."""
    a6, MG = f64(a6), f64(MG)
    a1, a2 = a6[:3], a6[3:]
    n1 = np.linalg.norm(a1)
    b1 = a1 / n1
    d = b1 @ a2
    u = a2 - d * b1
    n2 = np.linalg.norm(u)
    b2 = u / n2
    A = np.abs

    def cross_M(x, My):          # |x| x My with every product positive
        x = A(x)
        return np.array([x[1] * My[2] + x[2] * My[1], x[2] * My[0] + x[0] * My[2], x[0] * My[1] + x[1] * My[0]])
    Mb1 = MG[0] + cross_M(b2, MG[2])
    Mb2 = MG[1] + cross_M(b1, MG[2])
    Mu = (Mb2 + A(b2) * (A(b2) @ Mb2)) / n2
    Ma2 = Mu + (Mu @ A(b1)) * A(b1)
    Mb1 = Mb1 + (Mu @ A(b1)) * A(a2) + abs(d) * Mu
    Ma1 = (Mb1 + A(b1) * (A(b1) @ Mb1)) / n1
    return np.concatenate([Ma1, Ma2])


def _rot_grad(a6, G, MG):
    return rot6d_bwd(a6, G), rot6d_bwd_M(a6, MG)


# ---- posing (dbw.py:282-287,343-352) ----------------------------------------------------------------------------------------------------
def _pose_fwd(loc, Sv, R, T, S_world, Rw, Tw):
    """((loc * Sv) @ R + T) * S_world @ Rw + Tw for one primitive, loc (nv,3) -> world, M"""
    s = loc * Sv
    l = (s @ R + T) * S_world
    Ml = (np.abs(s) @ np.abs(R) + np.abs(T)) * S_world
    return l @ Rw + Tw, Ml @ np.abs(Rw) + np.abs(Tw)


def _pose_bwd(loc, Sv, R, S_world, Rw, g):
    """-> gT, M | gSv, M | gR (3,3), M | gloc (nv,3), M  (per primitive; g (nv,3) = d L / d world)"""
    gl, Mgl = S_world * (g @ Rw.T), S_world * (np.abs(g) @ np.abs(Rw).T)
    gs, Mgs = gl @ R.T, Mgl @ np.abs(R).T
    s = loc * Sv
    return (gl.sum(0), Mgl.sum(0), (gs * loc).sum(0), (Mgs * np.abs(loc)).sum(0), s.T @ gl, np.abs(s).T @ Mgl, gs * Sv, Mgs * Sv)


def posed_mesh(base, R6, T, S_world, Rw, Tw, gverts=None):
    """the ground: verts = ((base @ rot6d(R6)) + T) * S_world @ Rw + Tw; with gverts: g_R6 (6), g_T (3)"""
    base, T, Rw, S_world = f64(base), f64(T).reshape(3), f64(Rw).reshape(3, 3), f32v(S_world)
    Tw = np.zeros(3) if Tw is None else f64(Tw).reshape(3)
    a6 = f64(R6).reshape(6)
    R = rot6d(a6)
    v, Mv = _pose_fwd(base, np.ones(3), R, T, S_world, Rw, Tw)
    out = dict(verts=v, M_verts=Mv)
    if gverts is not None:
        gT, MgT, _, _, gR, MgR, _, _ = _pose_bwd(base, np.ones(3), R, S_world, Rw, f64(gverts))
        g6, M6 = _rot_grad(a6, gR, MgR)
        out.update(g_R6=g6, M_g_R6=M6, g_T=gT, M_g_T=MgT)
    return out


# ---- superquadric blocks (superquadric.py:10-14, pytorch.py:31-32, dbw.py:297-311,343-352) ------------------------------------------------
def _spow(t, e):
    """signed_pow(t, e) = sign(t) |t|^e and its derivative in e (0 where t == 0, as torch's pow backward has it)"""
    ab = np.abs(t)
    r = np.sign(t) * ab ** e
    with np.errstate(divide='ignore', invalid='ignore'):
        de = np.where(ab == 0, 0.0, r * np.log(np.where(ab == 0, 1.0, ab)))
    return r, de


def exponents(sq_eps):
    se = sigmoid(sq_eps)
    return se * 1.8 + 0.1, 1.8 * se * (1 - se)          # dbw.py:343-344; d eps / d sq_eps


def sq_blocks(sq_eps, S, R6, T, trig, ratio, scale_min, S_world, Rw, Tw, gverts=None):
    """sq_eps (Kb,2) S (Kb,3) R6 (Kb,6) T (Kb,3) trig (4,Kb,nv) = cos eta, sin eta, cos omega, sin omega.  -> verts (Kb,nv,3); with gverts
    (Kb,nv,3): g_sq_eps, g_S, g_R6, g_T"""
    sq_eps, S, R6, T, trig, Rw = f64(sq_eps), f64(S), f64(R6), f64(T), f64(trig), f64(Rw).reshape(3, 3)
    Tw = np.zeros(3) if Tw is None else f64(Tw).reshape(3)
    ratio, scale_min, S_world = f32v(ratio), f32v(scale_min), f32v(S_world)
    Kb, nv = trig.shape[1], trig.shape[2]
    e, dedx = exponents(sq_eps)
    Sv = np.exp(S) + scale_min
    names = ('verts', 'g_sq_eps', 'g_S', 'g_R6', 'g_T')
    shapes = ((Kb, nv, 3), (Kb, 2), (Kb, 3), (Kb, 6), (Kb, 3))
    out = {}
    for n_, s_ in zip(names, shapes):
        out[n_], out['M_' + n_] = np.zeros(s_), np.zeros(s_)
    for k in range(Kb):
        A, dA = _spow(trig[0, k], e[k, 0]); C, dC = _spow(trig[1, k], e[k, 0])
        Bc, dBc = _spow(trig[2, k], e[k, 1]); Bs, dBs = _spow(trig[3, k], e[k, 1])
        loc = np.stack([A * Bs, C, A * Bc], -1) * ratio
        de1 = np.stack([dA * Bs, dC, dA * Bc], -1) * ratio
        de2 = np.stack([A * dBs, np.zeros(nv), A * dBc], -1) * ratio
        R = rot6d(R6[k])
        out['verts'][k], out['M_verts'][k] = _pose_fwd(loc, Sv[k], R, T[k], S_world, Rw, Tw)
        if gverts is None:
            continue
        gT, MgT, gSv, MgSv, gR, MgR, gloc, Mgloc = _pose_bwd(loc, Sv[k], R, S_world, Rw, f64(gverts)[k])
        out['g_T'][k], out['M_g_T'][k] = gT, MgT
        out['g_S'][k], out['M_g_S'][k] = gSv * np.exp(S[k]), MgSv * np.exp(S[k])
        out['g_R6'][k], out['M_g_R6'][k] = _rot_grad(R6[k], gR, MgR)
        ge = np.array([(gloc * de1).sum(), (gloc * de2).sum()])
        Mge = np.array([(Mgloc * np.abs(de1)).sum(), (Mgloc * np.abs(de2)).sum()])
        out['g_sq_eps'][k], out['M_g_sq_eps'][k] = ge * dedx[k], Mge * dedx[k]
    if gverts is None:
        out = {k: v for k, v in out.items() if k.endswith('verts')}
    return out


def sq_local_points(e, trig, ratio):
    """The block-frame point of every vertex and its derivatives in the two exponents (superquadric.py:10-14; what the step's prologue keeps
    for its tail, 9 floats per vertex): e (Kb,2) the exponents, trig (4,Kb,nv) -> loc, de1, de2 (Kb,nv,3), each with M_ = its absolute value
    (every element is one product)"""
    e, trig, ratio = f64(e), f64(trig), f32v(ratio)
    e1, e2 = e[:, 0, None], e[:, 1, None]
    A, dA = _spow(trig[0], e1); C, dC = _spow(trig[1], e1)
    Bc, dBc = _spow(trig[2], e2); Bs, dBs = _spow(trig[3], e2)
    out = dict(loc=np.stack([A * Bs, C, A * Bc], -1) * ratio, de1=np.stack([dA * Bs, dC, dA * Bc], -1) * ratio,
               de2=np.stack([A * dBs, np.zeros_like(A), A * dBc], -1) * ratio)
    out.update({'M_' + k: np.abs(v) for k, v in list(out.items())})
    return out


def sq_local(sq_eps, trig, ratio):
    """sq_local_points at the exponents of sq_eps (dbw.py:343-344)"""
    return sq_local_points(exponents(sq_eps)[0], trig, ratio)


# ---- the loss values of a step (dbw.py:361-408: what compute_losses returns) ---------------------------------------------------------------
def loss_finish(part, scale, tv_value_scale, vals):
    """part (n) the per-tile sums of squared differences, vals (8) float32 with parsimony, tv, overlap in slots 1..3 -> rgb = scale sum(part)
    in float64 (M_rgb: the same over absolute values), and out5 = rgb, parsimony, tv * tv_value_scale, overlap, total in float64"""
    p, v, scale, tvs = f64(part).reshape(-1), f64(vals), f32v(scale), f32v(tv_value_scale)
    rgb = scale * p.sum()
    out5 = np.array([rgb, v[1], v[2] * tvs, v[3], rgb + v[1] + v[2] * tvs + v[3]])
    return dict(rgb=rgb, M_rgb=abs(scale) * np.abs(p).sum(), sum=p.sum(), M_sum=np.abs(p).sum(), out5=out5)


# ---- overlap (dbw.py:389-405; superquadric.py:17-38 with safe=True, as_sdf=2) -----------------------------------------------------------
def _safe_pow(t, e):
    """clamp(t, 1e-6)^e -> value, d / d t (0 below the clamp), d / d e"""
    c = np.maximum(t, SAFE_POW_EPS)
    r = c ** e
    return r, np.where(t >= SAFE_POW_EPS, e * r / c, 0.0), r * np.log(c)


def implicit_sdf(pts, e1, e2, w):
    """superquadric.py:17-38 (safe=True, as_sdf=2) of pts (n,3) for one pair of exponents: ((x^2)^(1/e2) + (z^2)^(1/e2))^(e2/e1) +
    (y^2)^(1/e1))^(e1/2) - 1 on the point clamped to [-5, 5]^3, every power through safe_pow; and the gradients of sum(w sdf):
    gpts (n,3), ge (n,2) = every point's share of d / d (e1, e2)"""
    pts, w = f64(pts), f64(w)
    pc = np.clip(pts, -CLAMP, CLAMP)
    inr = (pts >= -CLAMP) & (pts <= CLAMP)
    x2, y2, z2 = pc[:, 0] ** 2, pc[:, 1] ** 2, pc[:, 2] ** 2
    X, dXt, dXe = _safe_pow(x2, 1 / e2); Y, dYt, dYe = _safe_pow(y2, 1 / e1); Z, dZt, dZe = _safe_pow(z2, 1 / e2)
    W, dWt, dWe = _safe_pow(X + Z, e2 / e1)
    Q, dQt, dQe = _safe_pow(W + Y, e1 / 2)
    gr, gex, gXZ = w * dQt, w * dQt * dWe, w * dQt * dWt
    t1 = [w * dQe * 0.5, gex * (-e2 / e1 ** 2), gr * dYe * (-1 / e1 ** 2)]
    t2 = [gex / e1, gXZ * dXe * (-1 / e2 ** 2), gXZ * dZe * (-1 / e2 ** 2)]
    gp = np.stack([gXZ * dXt * 2 * pc[:, 0], gr * dYt * 2 * pc[:, 1], gXZ * dZt * 2 * pc[:, 2]], -1) * inr
    return dict(sdf=Q - 1, M_sdf=Q + 1, gpts=gp, M_gpts=np.abs(gp), ge=np.stack([sum(t1), sum(t2)], 1),
                M_ge=np.stack([sum(np.abs(t) for t in t1), sum(np.abs(t) for t in t2)], 1))


def overlap_points(u, S, R6, T, ratio, scale_min):
    """the sample points (no gradient): ((u * 2 - 1) * ratio * S_k) @ R_k + T_k -> (Kb * npts, 3)"""
    ratio, scale_min = f32v(ratio), f32v(scale_min)
    u, Sv = f64(u), np.exp(f64(S)) + scale_min
    R = rot6d(R6)
    return ((((u * 2 - 1) * ratio * Sv[:, None]) @ R) + f64(T)[:, None]).reshape(-1, 3)


def overlap(u, sq_eps, S, R6, T, alpha, ratio, scale_min, temperature, thresh, scale=1.0):
    """-> value, g_sq_eps, g_S, g_R6, g_T, g_alpha (+ M_ each) and `cond`: how close the samples come to the three branches
    (min |sum - thresh|, min relative |x^2 - 1e-6|, min ||inv| - 5|)"""
    sq_eps, S, R6, T, alpha = f64(sq_eps), f64(S), f64(R6), f64(T), f64(alpha)
    ratio, scale_min, temperature, thresh, scale = (f32v(x) for x in (ratio, scale_min, temperature, thresh, scale))
    Kb = alpha.shape[0]
    pts = overlap_points(u, S, R6, T, ratio, scale_min)
    P = pts.shape[0]
    e, dedx = exponents(sq_eps)
    Sv = np.exp(S) + scale_min
    R = rot6d(R6)                                                     # (Kb,3,3)
    q = pts[None] - T[:, None]                                        # (Kb,P,3)
    sr = Sv * ratio
    inv = np.einsum('kpc,kic->kpi', q, R) / sr[:, None]
    pc = np.clip(inv, -CLAMP, CLAMP)
    inr = (inv >= -CLAMP) & (inv <= CLAMP)
    e1, e2 = e[:, 0, None], e[:, 1, None]
    x2, y2, z2 = pc[..., 0] ** 2, pc[..., 1] ** 2, pc[..., 2] ** 2
    X, dXt, dXe = _safe_pow(x2, 1 / e2); Y, dYt, dYe = _safe_pow(y2, 1 / e1); Z, dZt, dZe = _safe_pow(z2, 1 / e2)
    W, dWt, dWe = _safe_pow(X + Z, e2 / e1)
    r = W + Y
    Q, dQt, dQe = _safe_pow(r, e1 / 2)
    sdf = Q - 1
    occ = sigmoid(-sdf / temperature)
    tot = (occ * alpha[:, None]).sum(0)                               # (P)
    act = tot - thresh > 0
    value = scale * np.where(act, tot - thresh, 0.0).sum() / P
    M_value = scale * np.where(act, tot + abs(thresh), 0.0).sum() / P
    go = np.where(act, scale / P, 0.0)[None]                          # (1,P)
    out = dict(value=value, M_value=M_value)
    out['g_alpha'] = (go * occ).sum(1); out['M_g_alpha'] = out['g_alpha'].copy()
    g = go * alpha[:, None] * occ * (1 - occ) * (-1 / temperature)    # d / d sdf (Kb,P)
    gr = g * dQt
    gex = gr * dWe
    gXZ = gr * dWt
    t1 = [g * dQe * 0.5, gex * (-e2 / e1 ** 2), gr * dYe * (-1 / e1 ** 2)]
    t2 = [gex / e1, gXZ * dXe * (-1 / e2 ** 2), gXZ * dZe * (-1 / e2 ** 2)]
    ge = np.stack([sum(t1).sum(1), sum(t2).sum(1)], 1)
    Mge = np.stack([sum(np.abs(t) for t in t1).sum(1), sum(np.abs(t) for t in t2).sum(1)], 1)
    out['g_sq_eps'], out['M_g_sq_eps'] = ge * dedx, Mge * dedx
    gp = np.stack([gXZ * dXt * 2 * pc[..., 0], gr * dYt * 2 * pc[..., 1], gXZ * dZt * 2 * pc[..., 2]], -1) * inr      # (Kb,P,3)
    gSv = -(gp * inv).sum(1) / Sv
    MgSv = np.abs(gp * inv).sum(1) / Sv
    out['g_S'], out['M_g_S'] = gSv * np.exp(S), MgSv * np.exp(S)
    gi = gp / sr[:, None]                                             # d / d (q . R_i)
    gR = np.einsum('kpi,kpc->kic', gi, q)
    MgR = np.einsum('kpi,kpc->kic', np.abs(gi), np.abs(q))
    out['g_T'] = -np.einsum('kpi,kic->kc', gi, R)
    out['M_g_T'] = np.einsum('kpi,kic->kc', np.abs(gi), np.abs(R))
    out['g_R6'], out['M_g_R6'] = np.zeros((Kb, 6)), np.zeros((Kb, 6))
    for k in range(Kb):
        out['g_R6'][k], out['M_g_R6'][k] = _rot_grad(R6[k], gR[k], MgR[k])
    sq = np.stack([x2, y2, z2])
    out['cond'] = dict(sum=float(np.abs(tot - thresh).min()), pow=float((np.abs(sq - SAFE_POW_EPS) / SAFE_POW_EPS).min()),
                       clamp=float(np.abs(np.abs(inv) - CLAMP).min()),
                       inner=float(min((np.abs(X + Z - SAFE_POW_EPS) / SAFE_POW_EPS).min(), (np.abs(r - SAFE_POW_EPS) / SAFE_POW_EPS).min())),
                       active=int(act.sum()), clamped=int((~inr).sum()), points=P)
    return out


# ==== torch's own formulation of the same operations, any dtype and device ================================================================
# float64 on the CPU: autograd holds the hand-written gradients above (tests/test_model_kernels_ref_host.py, 1e-12).
# float32 on the GPU: the yardstick of the kernels' bars (tests/test_gpu_model_kernels.py) -- the expressions tests/test_gpu_model.py uses
# as its references.
def _t(x, dtype, device, grad=False):
    import torch
    if x is None:
        return None
    t = x.detach().clone() if hasattr(x, 'detach') else torch.as_tensor(np.asarray(x))
    return t.to(device=device, dtype=dtype).requires_grad_(grad)


def _np(d):
    return {k: (v.detach().cpu().numpy() if hasattr(v, 'detach') else v) for k, v in d.items()}


def torch_texture_prep(tex, d, gmaps, gsig, dtype, device):
    import torch
    import torch.nn.functional as F
    t = _t(tex, dtype, device, True)
    sig = torch.sigmoid(t)
    maps = sig if d == 1 else F.avg_pool2d(sig.permute(0, 3, 1, 2), d, stride=d).permute(0, 2, 3, 1)
    L = (maps * _t(gmaps, dtype, device)).sum()
    if gsig is not None:
        L = L + (sig * _t(gsig, dtype, device)).sum()
    g, = torch.autograd.grad(L, t)
    return _np(dict(sig=sig, maps=maps, gtex=g))


def torch_tv(maps, wrap, scale, dtype, device):
    import torch
    m, scale = _t(maps, dtype, device, True), f32v(scale)
    l2sq = lambda t: t.pow(2).sum(-1)                                       # loss.py:46
    if wrap:                                                                # dbw.py:383-385
        v = l2sq(torch.diff(m, dim=2, append=m[:, :, 0:1])).sum(0).mean() + l2sq(torch.diff(m, dim=1)).sum(0).mean()
    else:                                                                   # dbw.py:380 (one map: the mean over maps is the sum)
        v = sum(l2sq(torch.diff(m, dim=k)).sum(0).mean() for k in [1, 2])
    v = v * scale
    g, = torch.autograd.grad(v, m)
    return _np(dict(value=v, grad=g))


def torch_composite(fg, env, img, scale, up, dtype, device):
    import torch
    f, e, scale, up = _t(fg, dtype, device, True), _t(env, dtype, device, True), f32v(scale), f32v(up)
    rec = f[:, :3] * f[:, 3:4] + (1 - f[:, 3:4]) * e[:, :3]                  # dbw.py:223
    if img is None:
        return _np(dict(rec=rec))
    v = ((rec - _t(img, dtype, device)) ** 2).sum() * scale                 # dbw.py:366-367 (scale = weight / count)
    gf, ge = torch.autograd.grad(v * up, (f, e))
    return _np(dict(rec=rec, value=v, gfg=gf, genv=ge))


def torch_adam(p, g, m, v, step, lr, beta1, beta2, eps, dtype, device, group_end=None):
    """torch.optim.Adam from a preloaded state; lr a scalar, or a list with group_end (one param group per range)"""
    import torch
    p, g, m, v = (_t(x, dtype, device) for x in (p, g, m, v))
    ends = [p.numel()] if group_end is None else list(group_end)
    lrs = [lr] if group_end is None else list(lr)
    lo, groups, parts = 0, [], []
    for e_, lr_ in zip(ends, lrs):
        if e_ > lo:
            q = p[lo:e_].clone().requires_grad_(True)
            q.grad = g[lo:e_].clone()
            groups.append(dict(params=[q], lr=float(np.float32(lr_))))
            parts.append((q, lo, e_))
        lo = e_
    opt = torch.optim.Adam(groups, betas=(float(np.float32(beta1)), float(np.float32(beta2))), eps=float(np.float32(eps)), foreach=False)
    for q, lo, e_ in parts:
        opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m[lo:e_].clone(), exp_avg_sq=v[lo:e_].clone())
    opt.step()
    cat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs])
    return _np(dict(p=cat([q for q, _, _ in parts]), m=cat([opt.state[q]['exp_avg'] for q, _, _ in parts]),
                    v=cat([opt.state[q]['exp_avg_sq'] for q, _, _ in parts])))


def torch_block_alpha(logit, noise, noise_scale, thresh, g_alpha, g_alpha_full, dtype, device):
    """dbw.py:297-311; g_alpha (Kb, parts) or None, g_alpha_full (Kb) or None: the upstream gradients of alpha and alpha_full"""
    import torch
    lg = _t(logit, dtype, device, True)
    a = torch.sigmoid(lg if noise is None else lg + f32v(noise_scale) * _t(noise, dtype, device))
    keep = (torch.sigmoid(lg) > f32v(thresh)) if thresh >= 0 else torch.ones_like(lg, dtype=torch.bool)
    af = a * keep
    L = a.sum() * 0
    if g_alpha is not None:
        L = L + (a[:, None] * _t(g_alpha, dtype, device)).sum()
    if g_alpha_full is not None:
        L = L + (af * _t(g_alpha_full, dtype, device)).sum()
    g, = torch.autograd.grad(L, lg)
    return _np(dict(alpha=a, alpha_full=af, keep=keep, g_logit=g))


def torch_sqrt_mean(x, eps, scale, dtype, device):
    import torch
    t = _t(x, dtype, device, True)
    v = t.clamp(float(np.float32(eps))).pow(0.5).mean() * f32v(scale)              # pytorch.py:35, dbw.py:376
    g, = torch.autograd.grad(v, t)
    return _np(dict(value=v, grad=g))


def _torch_rot6d(d6):
    import torch
    import torch.nn.functional as F
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def torch_posed_mesh(base, R6, T, S_world, Rw, Tw, gverts, dtype, device):
    import torch
    r6, t, S_world = _t(R6, dtype, device, True), _t(T, dtype, device, True), f32v(S_world)
    v = ((_t(base, dtype, device)[None] @ _torch_rot6d(r6.reshape(1, 6)) + t.reshape(1, 1, 3)) * S_world @ _t(Rw, dtype, device).reshape(3, 3)
         + _t(Tw, dtype, device).reshape(3))[0]
    out = dict(verts=v)
    if gverts is not None:
        g6, gt = torch.autograd.grad((v * _t(gverts, dtype, device)).sum(), (r6, t))
        out.update(g_R6=g6.reshape(6), g_T=gt.reshape(3))
    return _np(out)


def _torch_signed_pow(t, e):                                                 # pytorch.py:31-32
    import torch
    return torch.sign(t) * torch.abs(t).pow(e)


def torch_sq_blocks(sq_eps, S, R6, T, trig, ratio, scale_min, S_world, Rw, Tw, gverts, dtype, device):
    import torch
    P = [_t(x, dtype, device, True) for x in (sq_eps, S, R6, T)]
    tr = _t(trig, dtype, device)
    ratio, scale_min, S_world = f32v(ratio), f32v(scale_min), f32v(S_world)
    eps = torch.sigmoid(P[0]) * 1.8 + 0.1
    e1, e2 = eps[:, 0:1], eps[:, 1:2]
    ce, se, co, so = _torch_signed_pow(tr[0], e1), _torch_signed_pow(tr[1], e1), _torch_signed_pow(tr[2], e2), _torch_signed_pow(tr[3], e2)
    loc = torch.stack([ce * so, se, ce * co], -1) * ratio
    Sv = P[1].exp() + scale_min
    v = ((loc * Sv[:, None]) @ _torch_rot6d(P[2]) + P[3][:, None]) * S_world @ _t(Rw, dtype, device).reshape(3, 3) + _t(Tw, dtype, device).reshape(3)
    out = dict(verts=v)
    if gverts is not None:
        gs = torch.autograd.grad((v * _t(gverts, dtype, device)).sum(), P)
        out.update(g_sq_eps=gs[0], g_S=gs[1], g_R6=gs[2], g_T=gs[3])
    return _np(out)


def torch_sq_local(sq_eps, trig, ratio, dtype, device):
    """the block-frame points and their exponent derivatives (sq_local_points) in torch's own operations"""
    import torch
    tr, ratio = _t(trig, dtype, device), f32v(ratio)
    eps = torch.sigmoid(_t(sq_eps, dtype, device)) * 1.8 + 0.1
    e1, e2 = eps[:, 0:1], eps[:, 1:2]

    def sp(t, e):
        r = _torch_signed_pow(t, e)
        return r, torch.where(t == 0, torch.zeros_like(r), r * torch.log(torch.abs(t)))
    (A, dA), (C, dC), (Bc, dBc), (Bs, dBs) = sp(tr[0], e1), sp(tr[1], e1), sp(tr[2], e2), sp(tr[3], e2)
    return _np(dict(loc=torch.stack([A * Bs, C, A * Bc], -1) * ratio, de1=torch.stack([dA * Bs, dC, dA * Bc], -1) * ratio,
                    de2=torch.stack([A * dBs, torch.zeros_like(A), A * dBc], -1) * ratio))


def torch_implicit_sdf(pts, e1, e2, w, dtype, device):
    import torch
    p, e = _t(pts, dtype, device, True), torch.tensor([e1, e2], dtype=dtype, device=device, requires_grad=True)
    sp = lambda t, ex: t.clamp(SAFE_POW_EPS).pow(ex)
    pc = p.clamp(-CLAMP, CLAMP)
    x2, y2, z2 = [pc[..., k].pow(2) for k in range(3)]
    sdf = sp(sp(sp(x2, 1 / e[1]) + sp(z2, 1 / e[1]), e[1] / e[0]) + sp(y2, 1 / e[0]), e[0] / 2) - 1
    gp, ge = torch.autograd.grad((sdf * _t(w, dtype, device)).sum(), (p, e))
    return _np(dict(sdf=sdf, gpts=gp, ge_sum=ge))


def torch_overlap(u, sq_eps, S, R6, T, alpha, ratio, scale_min, temperature, thresh, scale, dtype, device):
    import torch
    P = [_t(x, dtype, device, True) for x in (sq_eps, S, R6, T, alpha)]
    N = P[4].shape[0]
    ratio, scale_min, temperature, thresh, scale = (f32v(x) for x in (ratio, scale_min, temperature, thresh, scale))
    eps = torch.sigmoid(P[0]) * 1.8 + 0.1
    e1, e2 = eps[:, 0:1], eps[:, 1:2]
    Sv, R, Tt = P[1].exp() + scale_min, _torch_rot6d(P[2]), P[3]
    with torch.no_grad():
        pts = ((_t(u, dtype, device) * 2 - 1) * ratio * Sv[:, None]) @ R + Tt[:, None]
        pts = pts.view(-1, 3)[None].expand(N, -1, -1)
    inv = ((pts - Tt[:, None]) @ R.transpose(1, 2)) / (Sv[:, None] * ratio)
    sp = lambda t, e: t.clamp(SAFE_POW_EPS).pow(e)
    pc = inv.clamp(-CLAMP, CLAMP)
    x2, y2, z2 = [pc[..., k].pow(2) for k in range(3)]
    x, y, z = sp(x2, 1 / e2), sp(y2, 1 / e1), sp(z2, 1 / e2)
    sdf = sp(sp(x + z, e2 / e1) + y, e1 / 2) - 1
    occ = torch.sigmoid(-sdf / temperature) * P[4][:, None]
    v = (occ.sum(0) - thresh).clamp(0).mean() * scale
    gs = torch.autograd.grad(v, P, allow_unused=True)
    gs = [torch.zeros_like(p) if g is None else g for g, p in zip(gs, P)]
    return _np(dict(value=v, g_sq_eps=gs[0], g_S=gs[1], g_R6=gs[2], g_T=gs[3], g_alpha=gs[4]))


# ==== shared fixtures: inputs whose conditioning the host test asserts before anything runs on a GPU ======================================
OVERLAP_CONSTS = dict(ratio=0.5, scale_min=0.2, temperature=0.005)          # dbw.py's ratio_block_scene, scale_min, OVERLAP_TEMPERATURE
# name -> (Kb, npts, thresh, seed).  The seed is chosen such that no sample lies within 1e-3 of sum = thresh, within 1e-4 (relative) of a
# safe_pow clamp (x^2 = 1e-6 for any coordinate and block, and the two inner sums) or within 1e-4 of |inv| = 5: across each of these
# branches the value is continuous and the gradient is not, and no sample is left out of a comparison.  And such that float32 sample points
# alone cost less than a quarter of the gradient floor (overlap_point_rounding).
OVERLAP_CASES = {
    'kb1-300': (1, 300, 0.5, 0),
    'kb2-100': (2, 100, 0.6, 0),
    'kb3-100': (3, 100, 0.3, 1),
    'kb5-1000': (5, 1000, 1.95, 1),
    'kb64-64': (64, 64, 1.95, 1),
    'kb5-below-threshold': (5, 100, 6.0, 0),
}
OVERLAP_MARGINS = dict(sum=1e-3, pow=1e-4, inner=1e-4, clamp=1e-4)
# The cases of the step's fused regularisers launch (tests/test_gpu_step_kernels.py), same conditions on the seed: P = Kb npts at the edges
# of its 256-point workgroups -- 1; 64 (one full wave: the last size at which the LDS atomics have one order); 255, 256 (one workgroup);
# 257 (one point in a second one); 64 blocks in one workgroup (the finish runs on `tid < nb` of 256 threads); 64 x 40 = 10 workgroups
STEP_OVERLAP_CASES = {
    'kb1-1': (1, 1, 0.3, 10),
    'kb2-32': (2, 32, 0.6, 6),
    'kb3-85': (3, 85, 0.3, 1),
    'kb4-64': (4, 64, 0.6, 0),
    'kb64-4': (64, 4, 1.95, 0),
    'kb1-257': (1, 257, 0.5, 0),
    'kb64-40': (64, 40, 1.95, 0),
}
# ... and one case for bit-equality with the operator kernels alone: 64 blocks x 1 sample = one wave, so the LDS atomics have one order and
# the finish of all 64 blocks (dead ones, the opacities at the parsimony clamp) is compared bit for bit.  Its gradients are NOT held to
# float64: with one sample per block nothing averages out, and torch's float32 on the CPU reads 2.8e-4 to 1 (a flipped branch) on every one
# of 80 seeds tried, 9.4e-3 on this one -- above the gradient floor before any kernel runs (overlap_float32_cost).  The branch margins hold.
STEP_BITWISE_CASES = {'kb64-1': (64, 1, 1.95, 0)}


def overlap_case(name):
    """Blocks pulled together so that they overlap (T scaled to 0.15), exponents over the whole range, 6D vectors random and not
    orthonormal; the last block of a case with Kb >= 3 is small and away from the others (its |inv| > 5 clamp masks the other blocks'
    samples' gradients) -- 1.6 from the origin, not further: see overlap_point_rounding; alpha holds an exact 0 when Kb >= 3."""
    step = {**STEP_OVERLAP_CASES, **STEP_BITWISE_CASES}
    Kb, npts, thresh, seed = (OVERLAP_CASES.get(name) or step[name])
    rng = np.random.RandomState(1000 + seed)
    c = dict(Kb=Kb, npts=npts, thresh=thresh, scale=1.3, **OVERLAP_CONSTS)
    c['sq_eps'] = (rng.rand(Kb, 2) * 6 - 3).astype(np.float32)
    c['S'] = (rng.randn(Kb, 3) * 0.3).astype(np.float32)
    c['R6'] = rng.randn(Kb, 6).astype(np.float32)
    c['T'] = (rng.randn(Kb, 3) * 0.15).astype(np.float32)
    c['alpha'] = (rng.rand(Kb) * 0.9 + 0.05).astype(np.float32)
    c['u'] = rng.rand(Kb, npts, 3).astype(np.float32)
    if Kb >= 3:
        c['S'][-1] = -4.0
        c['T'][-1] = (0.9, -0.8, 1.0)
        c['alpha'][1] = 0.0
    if name in step and Kb >= 5:        # the parsimony term of the same launch: an opacity exactly at its clamp and one just above it
        c['alpha'][2], c['alpha'][3] = np.float32(PARSIMONY_EPS), np.nextafter(np.float32(PARSIMONY_EPS), np.float32(1))
    return c


def overlap_ref(c):
    return overlap(c['u'], c['sq_eps'], c['S'], c['R6'], c['T'], c['alpha'], c['ratio'], c['scale_min'], c['temperature'], c['thresh'], c['scale'])


OVERLAP_GRADS = ('g_sq_eps', 'g_S', 'g_R6', 'g_T', 'g_alpha')
POINT_ROUNDING_MARGIN = 0.25          # of the gradient floor


def overlap_point_rounding(c, ref=None):
    """What float32 sample points alone cost: the reference with its points rounded once to float32 and everything else in float64,
    against the reference, in `err`, the largest over the gradients.  occupancy = sigmoid(-sdf / 0.005) turns a point's half ulp into
    200 x as much in the exponent, so a scene with large coordinates is out of any float32 kernel's reach; a case must keep this below
    POINT_ROUNDING_MARGIN of the gradient floor for the floor to be about the kernel."""
    global overlap_points
    ref = ref or overlap_ref(c)
    exact = overlap_points
    overlap_points = lambda *a: exact(*a).astype(np.float32).astype(np.float64)
    try:
        per = overlap_ref(c)
    finally:
        overlap_points = exact
    return max(err(per[k], ref[k], ref['M_' + k], 9 * c['Kb'] * c['npts']) for k in OVERLAP_GRADS)


FLOAT32_COST_MARGIN = 0.5             # of the gradient floor


def overlap_float32_cost(c, ref=None):
    """What float32 alone costs the gradients of a case: torch's float32 formulation on the CPU (no kernel in it) against the reference,
    in `err`.  The fewer samples a case has the less their roundings average out behind occupancy = sigmoid(-sdf / 0.005): of the
    2 x 32 cases tried for the step's one-wave launch most read 1e-4 to 1e-2 here, some 1 (a sample's branch flips in float32).  A case of
    STEP_OVERLAP_CASES, and a set of samples the step's generator draws, must keep this below FLOAT32_COST_MARGIN of the gradient floor,
    so that at least half of the floor is about the kernel."""
    import torch
    ref = ref or overlap_ref(c)
    t = torch_overlap(c['u'], c['sq_eps'], c['S'], c['R6'], c['T'], c['alpha'], c['ratio'], c['scale_min'], c['temperature'], c['thresh'], c['scale'],
                      torch.float32, 'cpu')
    return max(err(t[k], ref[k], ref['M_' + k], 9 * c['Kb'] * c['npts']) for k in OVERLAP_GRADS)


def well_conditioned(cond):
    return all(cond[k] > m for k, m in OVERLAP_MARGINS.items())


ALPHA_KB = (1, 63, 64, 65, 200)
ALPHA_THRESH = (-1.0, 0.01, 0.5)
ALPHA_MARGIN = 1e-3


def alpha_logits(Kb):
    """randn * 3 with +-90 planted (Kb >= 63); no logit within 1e-3 of logit(thresh) for any of ALPHA_THRESH -- asserted by the host test"""
    rng = np.random.RandomState(50 + Kb)
    lg = (rng.randn(Kb) * 3).astype(np.float32)
    if Kb >= 63:
        lg[0], lg[Kb - 1], lg[7] = 90.0, -90.0, 0.25
    return lg, (rng.randn(Kb)).astype(np.float32)


def alpha_margin(lg):
    th = np.array([t for t in ALPHA_THRESH if t >= 0], dtype=np.float64)
    return float(np.abs(f64(lg)[:, None] - np.log(th / (1 - th))[None]).min())


PARSIMONY_N = (1, 64, 65, 1000)
PARSIMONY_EPS = 1e-6


def parsimony_values(n):
    """opacities in [0, 1] with entries below the clamp (0, 1e-8), one exactly at it (index 2: the kernel's `x > eps` is false there -- the
    clamped side, no gradient -- where torch.clamp's backward passes the gradient at equality), the rest above; none other within 1e-4
    (relative) of it"""
    rng = np.random.RandomState(70 + n)
    x = (rng.rand(n) * 0.98 + 0.01).astype(np.float32)
    if n >= 64:
        x[0], x[1], x[2], x[n - 1] = 0.0, 1e-8, np.float32(PARSIMONY_EPS), 1.0
    return x


def parsimony_margin(x):
    d = np.abs(f64(x) - f32v(PARSIMONY_EPS)) / f32v(PARSIMONY_EPS)
    return float(d[d > 0].min()) if (d > 0).any() else np.inf


# ==== the bars ==========================================================================================================================
# family -> torch float32 against float64 on the MI355X with `err`, (value, gradient): the largest over the family's cases of
# tests/test_gpu_model_kernels.py (the table of its docstring and of profiles/model_kernels_fp64.md).  Adam has values only (p, m, v): its entry is one number.
TORCH_FP32 = {
    'prep': (4.22e-07, 1.0),
    'tv': (7.57e-08, 2.05e-07),
    'composite': (1.55e-07, 2.67e-07),
    'adam': (1.84e-07,),
    'blocks': (1.74e-07, 1.20e-05),
    'mesh': (1.28e-07, 3.71e-08),
    'overlap': (2.18e-07, 2.98e-05),
    'alpha': (2.62e-07, 1.50e-07),
    'parsimony': (5.24e-08, 1.79e-07),
}
# what tests/test_gpu_model.py asks of the same family today, in this metric: a bar is never looser (value, gradient)
FLOOR = {
    'prep': (1e-6, 1e-4),          # rel_err < 1e-6 of sig and maps (entries in (0, 1): the largest is ~1)
    'tv': (1e-5, 1e-4),            # |tv - ref| < 1e-5 |ref|
    'composite': (6e-6, 1e-4),     # |loss - ref| < 1e-6 absolute on a loss of 1/6 (uniform images); rec: rel_err < 1e-6, the tighter one, is used for rec
    'adam': (1e-5,),               # rel_err(p) < 1e-5 after five steps
    'blocks': (1e-5, 1e-4),        # rel_err(verts) < 1e-5
    'mesh': (1e-5, 1e-4),
    'overlap': (1e-4, 1e-4),       # |ov - ref| < 1e-4 ref
    'alpha': (1e-6, 1e-4),
    'parsimony': (1e-5, 1e-4),     # the fused losses: rel_err < 1e-5
}
FACTOR = 8.0


def bar(family, which, G=1):
    """which: 0 value, 1 gradient.  8 x torch's float32 error (the device's expf / powf / logf against the host's, serial or atomic
    summation order against torch's pairwise sums), never looser than FLOOR.  G > 1: the value is the sum of G workgroups' partial sums
    through float32 atomics in arrival order, whose error may grow like sqrt(G) against torch's pairwise sum (the losses of TV and of
    composite + MSE)."""
    return min(FACTOR * TORCH_FP32[family][which] * G ** 0.5, FLOOR[family][which])
