"""tests/lpips_head_ref.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Float64 reference of one tap's head of the perceptual criterion (csrc/lpips_head.hip; dbw_amd/lpips_vgg.py: _FusedHead), in plain torch, on
whatever device its inputs live on (the large cases evaluate it on the GPU in double), one image at a time so that the double-precision
temporaries of a 1080x1920 tap stay a few GB:

    value[n] = mean_pixels sum_c w_c (a_c - f_c r)^2,      r = 1 / (|f| + 1e-10),  |f| = sqrt(sum_c f_c^2)
    d value[n] / d f_k = (1 / HW) [ r q_k - f_k (q . f) / (|f| (|f| + 1e-10)^2) ],      q_c = -2 w_c (a_c - f_c r)

with the kernel's convention for a pixel whose tap is all zero: only the r q term (k2 = 0), where autograd of the plain formulation gives
0 * inf = NaN.  The errors of a float32 result against it are measured by `head_errors`, the same way for the kernel and for torch's own
float32 formulation (which sets the kernel's bar, tests/test_gpu_lpips_head.py)."""
import torch
import torch.nn.functional as F

EPS = 1e-10


def unit(f):
    """normalize_tensor of lpips: over channels (dim 1), in the precision of f"""
    return f / (f.pow(2).sum(1, keepdim=True).sqrt() + EPS)


def _row(a_unit, ids, n):
    return a_unit[int(ids[n]) if ids is not None else n].double()


def head_value(f, a_unit, w, ids=None):
    """f (N,C,h,w), a_unit (V,C,h,w) unit-normalised targets (row ids[n], or n, belongs to image n), w (C,) -> (N,) float64"""
    w64 = w.double().view(-1, 1, 1)
    out = []
    for n in range(f.shape[0]):
        f64 = f[n].double()
        u = f64 / (f64.pow(2).sum(0, keepdim=True).sqrt() + EPS)
        out.append((w64 * (_row(a_unit, ids, n) - u) ** 2).sum(0).mean())
    return torch.stack(out) if out else torch.zeros(0, dtype=torch.float64, device=f.device)


def head_grad_image(f_n, a_n, w, g_n):
    """One image of head_grad: f_n, a_n (C,h,w), g_n a number -> (C,h,w) float64."""
    f64, a64, w64 = f_n.double(), a_n.double(), w.double().view(-1, 1, 1)
    s = f64.pow(2).sum(0, keepdim=True).sqrt()
    r = 1.0 / (s + EPS)
    q = -2.0 * w64 * (a64 - f64 * r)
    qf = (q * f64).sum(0, keepdim=True)
    k2 = torch.where(s > 0, qf / (s * (s + EPS) ** 2).clamp(min=1e-300), torch.zeros_like(s))
    return (float(g_n) / (f64.shape[1] * f64.shape[2])) * (r * q - f64 * k2)


def head_grad(f, a_unit, w, g, ids=None):
    """Gradient of sum_n g[n] value[n] to f: (N,C,h,w) float64, the closed form above."""
    return torch.stack([head_grad_image(f[n], _row(a_unit, ids, n), w, g[n]) for n in range(f.shape[0])])


def plain_value(f, a_unit, w, ids=None):
    """The formulation torch runs (the non-fused branch of LPIPSVGG.forward), in the precision of its inputs, differentiable: (N,)"""
    na = a_unit[:f.shape[0]] if ids is None else a_unit.index_select(0, ids)
    return F.conv2d((na - unit(f)) ** 2, w.view(1, -1, 1, 1)).mean((2, 3)).view(-1)


def zero_pixels(f):
    """(N,h,w) bool: the pixels whose tap is all zero"""
    return (f == 0).all(1)


def head_errors(v, gf, f, a_unit, w, g, ids=None, identical=()):
    """Errors of a float32 result (v (N,) values, gf (N,C,h,w) gradient of sum_n g[n] value[n]) against the float64 reference on the same
    float32 inputs, no element left out.  -> dict of floats:
      value      per image |v - v64| / |v64|; an image of `identical` (its target is its own unit tap: v64 ~ 0): |v - v64| over the smallest
                 value among the other images
      grad       per element |g - g64| / (max_c |g64[n,:,p]| + 1e-2 max |g64[n]|), the maxima over the pixels that are not all zero; an
                 image of `identical`: |g - g64| over max |g64| of the first other image (whose grad_value is not 0); an image whose
                 grad_value is 0: the gradient must be exactly 0
      zero_grad  the all-zero pixels (their gradient is ~1e10 x the others': r = 1 / 1e-10), each against its own max_c |g64[n,:,p]|
    NaN in v or gf on a compared element makes the error NaN (and `nan_elems` counts them): a bar `err <= bar` then fails."""
    N = f.shape[0]
    v64 = head_value(f, a_unit, w, ids)
    others = [n for n in range(N) if n not in identical]
    e = {'value': 0.0, 'grad': 0.0, 'zero_grad': 0.0, 'zero_pixels': 0, 'nan_elems': 0}

    def worst(key, t):
        if t.numel():
            bad = int(torch.isnan(t).sum())
            e['nan_elems'] += bad
            e[key] = float('nan') if bad or e[key] != e[key] else max(e[key], float(t.max()))

    for n in range(N):
        d = (v[n].double() - v64[n]).abs()
        worst('value', (d / v64[others].abs().min() if n in identical else d / v64[n].abs()).reshape(1))
    generic = None
    for n in others + list(identical):
        g64 = head_grad_image(f[n], _row(a_unit, ids, n), w, g[n])
        err = (gf[n].double() - g64).abs()
        zero = zero_pixels(f[n:n + 1])[0]
        e['zero_pixels'] += int(zero.sum())
        pix = g64.abs().amax(0)                                   # (h,w): each pixel's own scale
        top = float(pix[~zero].max()) if bool((~zero).any()) else 0.0
        if float(g[n]) == 0.0:
            worst('grad', torch.where(gf[n] == 0, 0.0, float('inf')).reshape(-1))
            continue
        if generic is None and n not in identical:
            generic = top
        if n in identical:
            worst('grad', (err / generic)[:, ~zero])
        else:
            worst('grad', (err / (pix + 1e-2 * top))[:, ~zero])
        # (a zero pixel whose target has no channel with w > 0 either: the gradient is exactly 0 there)
        worst('zero_grad', torch.where(pix > 0, err / pix.clamp(min=1e-300), torch.where(err == 0, 0.0, float('inf')))[:, zero])
    return e
