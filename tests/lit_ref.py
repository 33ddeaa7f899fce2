"""Yardstick of the lit visualisation renders: a torch (CPU, fp32) restatement of the lighting rules of csrc/light_math.h, written
independently of it and applied to the ORACLE's fragments (oracle.render(..., return_fragments=True)).

PyTorch3D 0.7.1 is on none of the project's machines, so like the kernel this restates the published algorithm
(pytorch3d/renderer/mesh/shading.py: flat_shading, phong_shading, _apply_lighting; lighting.py: DirectionalLights.diffuse;
Meshes.faces_normals_packed / verts_normals_packed).  Cross products are written ELEMENT-WISE, products rounded and then the difference:
torch.cross is not bit-equal to that expression, and on the sliver faces of superquadrics with small exponents the cross product
cancels, so product and yardstick must form the same fp32 one; everything behind it is well conditioned."""
import torch
import torch.nn.functional as F

NORM_EPS = 1e-6


def cross(a, b):
    ax, ay, az = a.unbind(-1)
    bx, by, bz = b.unbind(-1)
    return torch.stack([ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx], dim=-1)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(c):
    """c / max(sqrt(c . c), 1e-6) with the CORRECTLY ROUNDED fp32 square root and quotient the library computes (IEEE sqrt / division):
    torch's vectorised CPU sqrt and its broadcast division are not correctly rounded on every build (measured: 150 and 418 of 20 000
    random normals differ from numpy's and g++'s), so both are taken in fp64 and rounded once -- for sqrt and division of fp32 operands
    that IS the correctly rounded fp32 result (53 >= 2 * 24 + 2 bits)."""
    length = torch.sqrt(dot(c, c).double()).float().clamp(min=NORM_EPS)
    return (c.double() / length.double()[..., None]).float()


def corner_cross(verts, faces, corner=0):
    """(F,3) unnormalised cross product of every face taken at `corner` (verts_normals_packed's three terms; corner 0 = the face normal's)."""
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    if corner == 1:
        return cross(v2 - v1, v0 - v1)
    if corner == 2:
        return cross(v0 - v2, v1 - v2)
    return cross(v1 - v0, v2 - v0)


def face_normals(verts, faces):
    return normalize(corner_cross(verts, faces, 0))


def vertex_normals(verts, faces):
    """Area-weighted: the corner cross products summed per vertex in ascending (face, corner) order, then normalised."""
    contrib = torch.stack([corner_cross(verts, faces, c) for c in range(3)], dim=1).reshape(-1, 3)       # row face * 3 + corner
    s = torch.zeros(verts.shape[0], 3).numpy()
    rows = contrib.numpy()
    for e, v in enumerate(faces.reshape(-1).tolist()):          # (a plain loop: the order of the fp32 sums is part of the statement)
        s[v] += rows[e]
    return normalize(torch.from_numpy(s))


def light_dir_world(direction, R):
    """direction (1 | B, 3) camera space -> (B,3) unit world directions: direction @ R[b]^T (the light is fixed to the camera)."""
    d = torch.as_tensor(direction, dtype=torch.float32).reshape(-1, 3)
    return normalize(d[:, 0:1] * R[:, :, 0] + d[:, 1:2] * R[:, :, 1] + d[:, 2:3] * R[:, :, 2])


def gain(n, d, ka, kd):
    """n, d (...,3) unit vectors -> (...,3): ambient + diffuse * relu(n . d)."""
    ka, kd = [torch.as_tensor(k, dtype=torch.float32).reshape(3) for k in (ka, kd)]
    return ka + kd * dot(n, d).clamp(min=0)[..., None]


def fragment_gains(frag, verts, faces, R, direction, ka, kd, phong):
    """(N,H,W,K,3) gain of every fragment (anything at empty slots).  frag: the oracle's fragments -- pix_to_face packed ORIGINAL face ids
    (b * F + j), bary w.r.t. the original face."""
    p2f = frag['pix_to_face']
    N = p2f.shape[0]
    Fs = faces.shape[0]
    j = p2f.clamp(min=0) % Fs
    d = light_dir_world(direction, R).expand(N, 3)[:, None, None, None, :]
    if phong:
        vn = vertex_normals(verts, faces)[faces[j]]                                     # (N,H,W,K,3 corners,3)
        b = frag['bary']
        n = normalize((b[..., 0:1] * vn[..., 0, :] + b[..., 1:2] * vn[..., 1, :]) + b[..., 2:3] * vn[..., 2, :])
    else:
        n = face_normals(verts, faces)[j]
    return gain(n, d.expand_as(n), ka, kd)


def render_lit(O, scene, R, T, Kmat, size, sigma, K, direction, ka, kd, phong, faces_alpha=None, background=(1., 1., 1.), n_threads=8,
               detach_bary=False):
    """(B,4,H,W): the oracle's rasterisation and texels of `scene`, lit, through the oracle's layered blend."""
    with torch.no_grad():
        _, frag = O.render(scene, R, T, Kmat, size, sigma, K, detach_bary, faces_alpha, 0.001, background, n_threads=n_threads, return_fragments=True)
        g = fragment_gains(frag, scene['verts'], scene['faces'], R, direction, ka, kd, phong)
        return O.layered_rgb_blend(frag['texels'] * g, frag['pix_to_face'], frag['dists'], sigma, background, faces_alpha)


def oracle_scene(scene):
    """A device PackedScene as the dict the oracle renders: its fp32 vertices and tables on the CPU, every map materialised with its
    circular padding (the yardstick is evaluated AT the vertices the device rendered: the rasterisers then agree bit for bit)."""
    flat = scene.maps.detach().cpu()
    maps = []
    for off, h, w, pl, pr, sh, _, _ in scene.map_desc.cpu().tolist():
        assert sh == 0, 'full-resolution maps only'
        m = flat[off:off + h * w * 3].view(h, w, 3)
        if pl or pr:
            m = F.pad(m.permute(2, 0, 1)[None], pad=(pl, pr, 0, 0), mode='circular')[0].permute(1, 2, 0)
        maps.append(m)
    return dict(verts=scene.verts.detach().cpu(), faces=scene.faces.cpu().long(), face_uvs=scene.face_uvs.detach().cpu(),
                face_map=scene.face_map.cpu().long(), maps=maps)
