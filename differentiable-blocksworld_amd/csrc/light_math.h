// Lighting arithmetic of the lit visualisation renders (render_lit.hip), written once for the device (hipcc) and for the host (g++:
// tests/test_host_light_math.py builds it into a checker-side shared object and compares it, without a GPU, with the torch restatement
// tests/lit_ref.py and with closed-form answers).
//
// PARITY UNPINNED (as DESIGN.md 2 says of the rest of PyTorch3D): PyTorch3D 0.7.1 is on none of the project's machines, so this restates
// the published algorithm -- pytorch3d/renderer/mesh/shading.py (flat_shading, phong_shading, _apply_lighting),
// pytorch3d/renderer/lighting.py (DirectionalLights.diffuse), Meshes.faces_normals_packed / verts_normals_packed -- and is checked
// against a second restatement, not against the library itself.  All fp32, one rounding per operation (-ffp-contract=off):
//  * face normal of the ORIGINAL (unclipped) face: e1 = v1 - v0, e2 = v2 - v0, c = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z,
//    e1.x*e2.y - e1.y*e2.x) -- products rounded, then the difference -- and n = c / max(sqrt((c.x^2 + c.y^2) + c.z^2), 1e-6).  The
//    ORDER is part of the contract: superquadrics with small exponents have sliver faces whose cross product cancels, and a checker
//    that forms it differently (torch.cross is not bit-equal to this expression) is up to 5e-3 away on them;
//  * vertex normal (Phong): the sum over the faces incident to the vertex of the UNNORMALISED cross product taken at that corner
//    ((v1-v0)x(v2-v0) at corner 0, (v2-v1)x(v0-v1) at corner 1, (v0-v2)x(v1-v2) at corner 2: area weighted), normalised the same way;
//  * light: d = the view's world direction (direction @ R^T: the light is fixed to the camera), normalised the same way; it points FROM
//    the surface TO the light.  gain = ambient + diffuse * relu(n . d) per channel (materials: PyTorch3D's defaults, all ones), and the
//    shaded colour is gain * texel.  No specular term: every light the reference builds has specular_color 0 (the host refuses others);
//  * flat: n = the face normal.  Phong: n = the three vertex normals interpolated with the fragment's barycentrics w.r.t. the original
//    face, then normalised.
#pragma once
#include "raster_math.h"      // DBW_HD, f3

namespace dbw {

constexpr float LIGHT_NORM_EPS = 1e-6f;      // F.normalize(eps=1e-6)

DBW_HD f3 light_sub(const float *a, const float *b) { f3 r; r.x = a[0] - b[0]; r.y = a[1] - b[1]; r.z = a[2] - b[2]; return r; }

DBW_HD f3 light_cross(f3 a, f3 b) {
    f3 c;
    c.x = a.y * b.z - a.z * b.y;
    c.y = a.z * b.x - a.x * b.z;
    c.z = a.x * b.y - a.y * b.x;
    return c;
}

DBW_HD float light_dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

DBW_HD f3 light_normalize(f3 c) {
    float len = sqrtf(light_dot(c, c));
    if (!(len > LIGHT_NORM_EPS)) len = LIGHT_NORM_EPS;
    f3 n; n.x = c.x / len; n.y = c.y / len; n.z = c.z / len;
    return n;
}

// unnormalised cross product of a face at one of its corners (world vertices, 3 floats each); corner 0 = the face normal's
DBW_HD f3 corner_cross(const float *v0, const float *v1, const float *v2, int corner) {
    if (corner == 1) return light_cross(light_sub(v2, v1), light_sub(v0, v1));
    if (corner == 2) return light_cross(light_sub(v0, v2), light_sub(v1, v2));
    return light_cross(light_sub(v1, v0), light_sub(v2, v0));
}

DBW_HD f3 face_normal(const float *v0, const float *v1, const float *v2) { return light_normalize(corner_cross(v0, v1, v2, 0)); }

// gain[ch] = ambient[ch] + diffuse[ch] * relu(n . d); n and d unit vectors
DBW_HD void light_gain(f3 n, f3 d, const float ambient[3], const float diffuse[3], float gain[3]) {
    float c = light_dot(n, d);
    if (!(c > 0.f)) c = 0.f;           // relu; a NaN cosine (no input produces one: both normalisations are guarded) would give the ambient term
    gain[0] = ambient[0] + diffuse[0] * c;
    gain[1] = ambient[1] + diffuse[1] * c;
    gain[2] = ambient[2] + diffuse[2] * c;
}

// Phong: the vertex normals n0, n1, n2 (3 floats each) interpolated with the barycentrics of the original face, normalised
DBW_HD f3 phong_normal(const float bo[3], const float *n0, const float *n1, const float *n2) {
    f3 n;
    n.x = (bo[0] * n0[0] + bo[1] * n1[0]) + bo[2] * n2[0];
    n.y = (bo[0] * n0[1] + bo[1] * n1[1]) + bo[2] * n2[1];
    n.z = (bo[0] * n0[2] + bo[1] * n1[2]) + bo[2] * n2[2];
    return light_normalize(n);
}

}  // namespace dbw
