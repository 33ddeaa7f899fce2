"""CPU tests of the lighting arithmetic of the lit visualisation renders (csrc/light_math.h, the header the kernels of render_lit.hip
compile) built for the host with g++ (tests/host_light_math.cpp), against the torch restatement the GPU tests use as their yardstick
(tests/lit_ref.py) and against closed-form answers:
  * face normals, and the cross products in front of them, BIT-EQUAL to the element-wise restatement, on random triangles and on slivers
    (whose cross product cancels: product and yardstick must form the same fp32 one);
  * vertex normals, gains and the Phong interpolation at rtol 1e-5 / atol 1e-6 (the bar tests/test_host_shade_math.py uses for values);
  * a face that looks at the light has gain ka + kd, at 60 degrees ka + kd / 2, at 90 degrees and beyond ka; a degenerate face has gain
    ka and no NaN; flat and Phong shading agree on a planar mesh (atol 1e-6: gains are at most 1.1, a normalisation and a dot product
    lie in between)."""
import ctypes
import math

import pytest
import torch

import lit_ref as LR
import oracle as O
from dbw_amd import ops
from host_build import host_lib

KA, KD = [0.7, 0.7, 0.7], [0.4, 0.4, 0.4]


def lib():
    return host_lib('light_math')


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def host_face_normals(verts, faces):
    f = faces.to(torch.int32).contiguous()
    n, c = torch.empty(len(f), 3), torch.empty(len(f), 3)
    assert lib().host_face_normals(_p(verts), _p(f), len(f), _p(n)) == 0 and lib().host_face_cross(_p(verts), _p(f), len(f), _p(c)) == 0
    return n, c


def host_vertex_normals(verts, faces):
    f = faces.to(torch.int32).contiguous()
    start, adj = ops.vertex_adjacency(f, verts.shape[0])
    out = torch.empty_like(verts)
    assert lib().host_vertex_normals(_p(verts), _p(f), _p(start), _p(adj), verts.shape[0], len(f), _p(out)) == 0
    return out


def host_flat_gains(verts, faces, direction, ka=KA, kd=KD):
    f = faces.to(torch.int32).contiguous()
    d, g = torch.empty(3), torch.empty(len(f), 3)
    assert lib().host_flat_gains(_p(verts), _p(f), len(f), _f3(direction), _f3(ka), _f3(kd), _p(d), _p(g)) == 0
    return d, g


def host_phong_gains(bo, j, faces, vn, d_unit, ka=KA, kd=KD):
    f, j = faces.to(torch.int32).contiguous(), j.to(torch.int32).contiguous()
    n, g = torch.empty(len(j), 3), torch.empty(len(j), 3)
    assert lib().host_phong_gains(_p(bo), _p(j), len(j), _p(f), _p(vn), _f3(d_unit), _f3(ka), _f3(kd), _p(n), _p(g)) == 0
    return n, g


def _triangles(n, sliver, seed):
    g = torch.Generator().manual_seed(seed)
    v0 = torch.randn(n, 3, generator=g)
    v1 = v0 + torch.randn(n, 3, generator=g) * torch.rand(n, 1, generator=g) * 2
    if sliver:      # the second vertex pair 1e-3 apart relative to the edge length
        v2 = v1 + LR.normalize(torch.randn(n, 3, generator=g)) * 1e-3 * (v1 - v0).norm(dim=-1, keepdim=True)
    else:
        v2 = v0 + torch.randn(n, 3, generator=g)
    verts = torch.stack([v0, v1, v2], 1).reshape(-1, 3).contiguous()
    return verts, torch.arange(3 * n).view(n, 3)


@pytest.mark.parametrize('sliver', [False, True])
def test_face_normals_are_bit_equal_to_the_elementwise_restatement(sliver):
    verts, faces = _triangles(20000, sliver, 3 + sliver)
    n, c = host_face_normals(verts, faces)
    assert torch.equal(c, LR.corner_cross(verts, faces, 0))
    assert torch.equal(n, LR.face_normals(verts, faces))
    big = c.norm(dim=-1) > 1e-5                             # (below 1e-6 the clamped norm takes over: shorter than a unit vector by design)
    assert torch.isfinite(n).all() and big.float().mean() > 0.9 and ((n.norm(dim=-1) - 1).abs() < 1e-5)[big].all()
    if sliver:      # ... which is what makes the order matter: against fp64 an fp32 sliver normal is visibly off
        n64 = torch.nn.functional.normalize(torch.cross((verts[1::3] - verts[0::3]).double(), (verts[2::3] - verts[0::3]).double(), dim=-1), dim=-1)
        assert float((n.double() - n64).abs().max()) > 1e-5


def _blob(seed=0):
    verts, faces = O.get_icosphere(2)
    g = torch.Generator().manual_seed(seed)
    verts = (verts * (1 + 0.3 * torch.rand(verts.shape[0], 1, generator=g)) * torch.tensor([1.0, 0.6, 1.7])).contiguous()
    return verts, faces


def test_vertex_normals_and_adjacency():
    verts, faces = _blob()
    start, adj = ops.vertex_adjacency(faces.to(torch.int32), verts.shape[0])
    assert start[0] == 0 and start[-1] == adj.numel() == faces.numel() and (start[1:] >= start[:-1]).all()
    for v in (0, 5, verts.shape[0] - 1):                   # a vertex's entries: exactly its (face, corner) pairs, ascending
        ent = adj[start[v]:start[v + 1]].tolist()
        assert ent == sorted(ent) and [(e >> 2, e & 3) for e in ent] == [(f, c) for f in range(len(faces)) for c in range(3) if faces[f, c] == v]
    vn = host_vertex_normals(verts, faces)
    torch.testing.assert_close(vn, LR.vertex_normals(verts, faces), rtol=1e-5, atol=1e-6)
    assert torch.equal(vn, host_vertex_normals(verts, faces))
    # area weighting: the fp64 sum of the incident faces' (area-scaled) normals
    cr = torch.cross((verts[faces[:, 1]] - verts[faces[:, 0]]).double(), (verts[faces[:, 2]] - verts[faces[:, 0]]).double(), dim=-1)
    s = torch.zeros(verts.shape[0], 3, dtype=torch.float64).index_add_(0, faces.reshape(-1), cr.repeat_interleave(3, 0))
    torch.testing.assert_close(vn.double(), torch.nn.functional.normalize(s, dim=-1), rtol=1e-5, atol=1e-6)
    assert (LR.dot(vn, LR.normalize(verts)) > 0.5).all()   # outward, like the faces' winding


def test_gains_and_phong_interpolation_match_the_restatement():
    verts, faces = _blob(1)
    g = torch.Generator().manual_seed(2)
    for direction in ([1, 0.25, -1], [0.3, -2.0, 0.4], [0, 0, -1]):
        R = O.random_rotations(1)
        dw = LR.light_dir_world([direction], R)[0]
        raw = (torch.tensor([direction], dtype=torch.float32) @ R[0].t())[0]          # unnormalised, as the entry point takes it
        d, gains = host_flat_gains(verts, faces, raw)
        torch.testing.assert_close(d, dw, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(gains, LR.gain(LR.face_normals(verts, faces), dw.expand(len(faces), 3), KA, KD), rtol=1e-5, atol=1e-6)
        assert gains.min() >= 0.7 - 1e-6 and gains.max() <= 1.1 + 1e-6 and gains.max() > 1.0 and (gains == 0.7).any()
        M = 5000
        j = torch.randint(0, len(faces), (M,), generator=g)
        bo = torch.rand(M, 3, generator=g)
        bo = (bo / bo.sum(-1, keepdim=True)).contiguous()
        vn = LR.vertex_normals(verts, faces)
        n, pg = host_phong_gains(bo, j, faces, vn, dw)
        c = vn[faces[j]]
        n_ref = LR.normalize((bo[:, 0:1] * c[:, 0] + bo[:, 1:2] * c[:, 1]) + bo[:, 2:3] * c[:, 2])
        torch.testing.assert_close(n, n_ref, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(pg, LR.gain(n_ref, dw.expand(M, 3), KA, KD), rtol=1e-5, atol=1e-6)
    # per-channel colours
    _, gc = host_flat_gains(verts, faces, [0., 1., 0.], ka=[0.1, 0.2, 0.3], kd=[0.5, 0.0, 1.0])
    torch.testing.assert_close(gc, LR.gain(LR.face_normals(verts, faces), torch.tensor([0., 1., 0.]).expand(len(faces), 3), [0.1, 0.2, 0.3],
                                           [0.5, 0.0, 1.0]), rtol=1e-5, atol=1e-6)


def test_closed_form_gains():
    ka, kd = 0.7, 0.4
    verts = torch.tensor([[0., 0, 0], [2., 0, 0], [0., 3, 0],              # normal (0, 0, 1)
                          [1., 1, 1], [1., 1, 1], [1., 1, 1]])             # degenerate: three equal vertices
    faces = torch.tensor([[0, 1, 2], [3, 4, 5]])
    s, c = math.sin(math.radians(60)), math.cos(math.radians(60))
    for direction, want in (([0, 0, 1], ka + kd), ([0, 0, 5.0], ka + kd), ([s, 0, c], ka + kd / 2), ([0, -s, c], ka + kd / 2), ([1, 0, 0], ka),
                            ([-3, 2, 0], ka), ([0, 0, -1], ka), ([0.5, 0.5, -0.1], ka)):
        _, g = host_flat_gains(verts, faces, direction)
        assert torch.isfinite(g).all()
        assert float((g[0] - want).abs().max()) <= 1e-6, (direction, g[0])
        assert float((g[1] - ka).abs().max()) <= 1e-6, (direction, g[1])               # degenerate face: the ambient term alone
    n, _ = host_face_normals(verts, faces)
    assert torch.equal(n[0], torch.tensor([0., 0, 1])) and torch.equal(n[1], torch.zeros(3))
    # a light of zero length (normalised with the clamped norm: the zero vector) leaves the ambient term
    _, g = host_flat_gains(verts, faces, [0, 0, 0])
    assert float((g - ka).abs().max()) <= 1e-6


def test_flat_and_phong_agree_on_a_planar_mesh():
    verts, faces = O.get_plane()
    for _ in range(3):
        verts, faces = O.subdivide(verts, faces)
    g = torch.Generator().manual_seed(4)
    verts = (verts * torch.tensor([3.0, 1.0, 0.7]) @ O.random_rotations(1)[0] + torch.tensor([0.3, -1.0, 2.0])).contiguous()
    vn = host_vertex_normals(verts, faces)
    d, flat = host_flat_gains(verts, faces, [1, 0.25, -1])
    if float(flat.max()) <= 0.7:                            # the plane looks away from this light: flip it
        d, flat = host_flat_gains(verts, faces, [-1, -0.25, 1])
    assert flat.max() > 0.75
    M = 4000
    j = torch.randint(0, len(faces), (M,), generator=g)
    bo = torch.rand(M, 3, generator=g)
    bo = (bo / bo.sum(-1, keepdim=True)).contiguous()
    _, pg = host_phong_gains(bo, j, faces, vn, d)
    assert float((pg - flat[j]).abs().max()) <= 1e-6
