// Camera transform and near-plane clipping arithmetic shared by the device kernels (hipcc, project_clip.hip) and the host (g++:
// tests/test_host_camera_math.py builds it into a checker-side shared object and holds it, without a GPU, bit for bit to
// oracle/oracle.py::transform_to_ndc + clip_faces, and its backward to autograd).  SURVEY.md A.2, A.4.  The backward half -- project_bwd and
// clip_slot_walk -- is also what the camera-side gradients of camera_grad.hip are built from (pose_math.h, intrinsics_math.h).
#pragma once
#include "raster_math.h"      // DBW_HD, f3

namespace dbw {

struct Cam {
    float R[9], T[3], K[16];
};

DBW_HD void load_cam(const float *R, const float *T, const float *Kmat, int b, Cam &c) {
#pragma unroll
    for (int i = 0; i < 9; ++i) c.R[i] = R[b * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) c.T[i] = T[b * 3 + i];
#pragma unroll
    for (int i = 0; i < 16; ++i) c.K[i] = Kmat[i];
}

struct Proj {
    float vx, vy, vz;   // view space
    float px, py, pw;   // before the perspective divide
    float denom;
    f3 ndc;             // x,y NDC, z = view depth
};

// view depth of a world point: the one quantity near-plane clipping classifies a vertex by (clip_emit_count)
DBW_HD float view_z(const float *X, const Cam &c) { return X[0] * c.R[2] + X[1] * c.R[5] + X[2] * c.R[8] + c.T[2]; }

DBW_HD Proj project(const float *X, const Cam &c, float eps) {
    Proj o;
    const float x = X[0], y = X[1], z = X[2];
    o.vx = x * c.R[0] + y * c.R[3] + z * c.R[6] + c.T[0];
    o.vy = x * c.R[1] + y * c.R[4] + z * c.R[7] + c.T[1];
    o.vz = view_z(X, c);
    o.px = o.vx * c.K[0] + o.vy * c.K[1] + o.vz * c.K[2] + c.K[3];
    o.py = o.vx * c.K[4] + o.vy * c.K[5] + o.vz * c.K[6] + c.K[7];
    o.pw = o.vx * c.K[12] + o.vy * c.K[13] + o.vz * c.K[14] + c.K[15];
    const float sgn = o.pw > 0.f ? 1.f : (o.pw < 0.f ? -1.f : 1.f);
    const float ab = o.pw < 0.f ? -o.pw : o.pw;
    o.denom = sgn * (ab < eps ? eps : ab);
    o.ndc.x = o.px / o.denom;
    o.ndc.y = o.py / o.denom;
    o.ndc.z = o.vz;
    return o;
}

// intersection of segment pa->pb with z = c; w returned
DBW_HD f3 clip_point(f3 pa, f3 pb, float c, int persp, float &w) {
    w = (pa.z - c) / (pa.z - pb.z);
    const float omw = 1.f - w;
    f3 q;
    q.z = pa.z * omw + pb.z * w;
    if (persp) {
        q.x = ((pa.x * pa.z) * omw + (pb.x * pb.z) * w) / c;
        q.y = ((pa.y * pa.z) * omw + (pb.y * pb.z) * w) / c;
    } else {
        q.x = pa.x * omw + pb.x * w;
        q.y = pa.y * omw + pb.y * w;
    }
    return q;
}


// One face after the camera transform -> 0, 1 or 2 triangles: untouched (no vertex behind z = zc), dropped (all three),
// case 3 (two behind; p1 = the vertex in front -> (p4, p5, p1)) or case 4 (one behind; p1 = the vertex behind -> (p4, p2, p5) and
// (p5, p2, p3)).  code = i1 | kind << 2 (i1 = slot of p1 in the original face; kind 0 / 1 / 2 = which clipped triangle), -1 for an
// untouched face; w2, w3 = the (detached) interpolation weights of p4 on p1-p2 and p5 on p1-p3.
struct ClippedFace {
    int emit, code0, code1;
    float w2, w3;
    f3 t0[3], t1[3];
};
DBW_HD void clip_face(const f3 p[3], int zc_on, float zc, int persp, ClippedFace &o) {
    int nbh = 0, behind_mask = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (zc_on && p[i].z < zc) { ++nbh; behind_mask |= 1 << i; }
    o.emit = nbh == 0 ? 1 : (nbh == 3 ? 0 : (nbh == 2 ? 1 : 2));
    o.code0 = o.code1 = -1; o.w2 = o.w3 = 0.f;
    if (nbh == 0) { o.t0[0] = p[0]; o.t0[1] = p[1]; o.t0[2] = p[2]; return; }
    if (nbh == 3) return;
    // vertex roles rotated by i1 with selects (runtime indexing would put p[] in scratch memory on the device)
    const int i1 = nbh == 2 ? ((behind_mask == 6) ? 0 : (behind_mask == 5 ? 1 : 2)) : ((behind_mask == 1) ? 0 : (behind_mask == 2 ? 1 : 2));
    const f3 p1 = i1 == 0 ? p[0] : (i1 == 1 ? p[1] : p[2]), p2 = i1 == 0 ? p[1] : (i1 == 1 ? p[2] : p[0]),
             p3 = i1 == 0 ? p[2] : (i1 == 1 ? p[0] : p[1]);
    const f3 p4 = clip_point(p1, p2, zc, persp, o.w2), p5 = clip_point(p1, p3, zc, persp, o.w3);
    if (nbh == 2) {
        o.t0[0] = p4; o.t0[1] = p5; o.t0[2] = p1;
        o.code0 = i1 | (0 << 2);
    } else {
        o.t0[0] = p4; o.t0[1] = p2; o.t0[2] = p5;
        o.t1[0] = p5; o.t1[1] = p2; o.t1[2] = p3;
        o.code0 = i1 | (1 << 2); o.code1 = i1 | (2 << 2);
    }
}

// number of triangles clip_face emits for a face whose vertices have view depths z0, z1, z2 (its `emit`, without the rest)
DBW_HD int clip_emit_count(float z0, float z1, float z2, int zc_on, float zc) {
    const int nbh = (zc_on && z0 < zc ? 1 : 0) + (zc_on && z1 < zc ? 1 : 0) + (zc_on && z2 < zc ? 1 : 0);
    return nbh == 0 ? 1 : (nbh == 3 ? 0 : (nbh == 2 ? 1 : 2));
}

// Backward of project for one vertex: the gradients gpx, gpy, gpw of the three projected rows from the ndc gradient g (gpw = 0 where
// |pw| < eps, the clamp of the denominator), next to the forward values every consumer needs.  The ONE statement of this arithmetic:
// the world-space (vertex_bwd), camera (pose_math.h::vertex_cam_grad) and K (intrinsics_math.h::vertex_k_grad) gradients all start here.
struct ProjGrad {
    Proj pr;
    float gpx, gpy, gpw;
};
DBW_HD ProjGrad project_bwd(const float *X, const Cam &c, float eps, f3 g) {
    ProjGrad o;
    o.pr = project(X, c, eps);
    o.gpx = g.x / o.pr.denom; o.gpy = g.y / o.pr.denom;
    const float gden = -(g.x * o.pr.px + g.y * o.pr.py) / (o.pr.denom * o.pr.denom);
    const float ab = o.pr.pw < 0.f ? -o.pr.pw : o.pr.pw;
    o.gpw = ab >= eps ? gden : 0.f;
    return o;
}

// d(ndc vertex)/d(view-space vertex): the part of the gradient that belongs to the camera of the view (pose_math.h: g_T += gview,
// g_R[r][c] += X_r * gview_c); g.z reaches the view depth directly
DBW_HD f3 view_grad(const ProjGrad &p, const Cam &c, f3 g) {
    f3 o;
    o.x = p.gpx * c.K[0] + p.gpy * c.K[4] + p.gpw * c.K[12];
    o.y = p.gpx * c.K[1] + p.gpy * c.K[5] + p.gpw * c.K[13];
    o.z = p.gpx * c.K[2] + p.gpy * c.K[6] + p.gpw * c.K[14] + g.z;
    return o;
}

// d(ndc vertex)/d(world vertex): the world-space gradient of one vertex of one view
DBW_HD f3 vertex_bwd(const float *verts, int vi, const Cam &c, float eps, f3 g) {
    const f3 gv = view_grad(project_bwd(verts + (long long)vi * 3, c, eps, g), c, g);
    f3 o;
    o.x = gv.x * c.R[0] + gv.y * c.R[1] + gv.z * c.R[2];
    o.y = gv.x * c.R[3] + gv.y * c.R[4] + gv.z * c.R[5];
    o.z = gv.x * c.R[6] + gv.y * c.R[7] + gv.z * c.R[8];
    return o;
}

// grads of q = clip_point(pa, pb) (w detached) pushed to ga, gb
DBW_HD void clip_point_bwd(f3 pa, f3 pb, float c, int persp, float w, f3 gq, f3 &ga, f3 &gb) {
    const float omw = 1.f - w;
    ga.z += gq.z * omw; gb.z += gq.z * w;
    if (persp) {
        ga.x += gq.x * pa.z * omw / c; ga.y += gq.y * pa.z * omw / c;
        ga.z += (gq.x * pa.x + gq.y * pa.y) * omw / c;
        gb.x += gq.x * pb.z * w / c; gb.y += gq.y * pb.z * w / c;
        gb.z += (gq.x * pb.x + gq.y * pb.y) * w / c;
    } else {
        ga.x += gq.x * omw; ga.y += gq.y * omw;
        gb.x += gq.x * w; gb.y += gq.y * w;
    }
}

// The clipping case analysis of the backward, stated ONCE: the gradients gv0..gv2 of the three ORIGINAL vertices' ndc positions (slots of
// the mesh face) from those of one clipped-face slot's three vertices ga, gb, gc.  cd < 0: the face was not clipped.  Otherwise i1 = cd & 3
// is the slot of p1 in the original face, kind = cd >> 2 says which clipped triangle this is ((p4, p5, p1), (p4, p2, p5), (p5, p2, p3));
// q0..q2 = the projected original vertices (read only for a clipped face); w2, w3 = the detached weights of p4 on p1-p2 and p5 on p1-p3.
DBW_HD void clip_slot_bwd(int cd, f3 q0, f3 q1, f3 q2, float zc, int persp, float w2, float w3, f3 ga, f3 gb, f3 gc, f3 &gv0, f3 &gv1, f3 &gv2) {
    if (cd < 0) { gv0 = ga; gv1 = gb; gv2 = gc; return; }
    const int i1 = cd & 3, kind = cd >> 2;
    // vertex roles rotated by i1 with selects (runtime indexing would put the arrays in scratch memory)
    const f3 P1 = i1 == 0 ? q0 : (i1 == 1 ? q1 : q2), P2 = i1 == 0 ? q1 : (i1 == 1 ? q2 : q0), P3 = i1 == 0 ? q2 : (i1 == 1 ? q0 : q1);
    f3 g1{0.f, 0.f, 0.f}, g2{0.f, 0.f, 0.f}, g3{0.f, 0.f, 0.f};
    if (kind == 0) {          // (p4, p5, p1)
        clip_point_bwd(P1, P2, zc, persp, w2, ga, g1, g2);
        clip_point_bwd(P1, P3, zc, persp, w3, gb, g1, g3);
        g1.x += gc.x; g1.y += gc.y; g1.z += gc.z;
    } else if (kind == 1) {   // (p4, p2, p5)
        clip_point_bwd(P1, P2, zc, persp, w2, ga, g1, g2);
        g2.x += gb.x; g2.y += gb.y; g2.z += gb.z;
        clip_point_bwd(P1, P3, zc, persp, w3, gc, g1, g3);
    } else {                  // (p5, p2, p3)
        clip_point_bwd(P1, P3, zc, persp, w3, ga, g1, g3);
        g2.x += gb.x; g2.y += gb.y; g2.z += gb.z;
        g3.x += gc.x; g3.y += gc.y; g3.z += gc.z;
    }
    gv0 = i1 == 0 ? g1 : (i1 == 1 ? g3 : g2);
    gv1 = i1 == 0 ? g2 : (i1 == 1 ? g1 : g3);
    gv2 = i1 == 0 ? g3 : (i1 == 1 ? g2 : g1);
}

// Backward of project + clip_face for ONE clipped-face slot, up to the vertices: the vertex backward of project_clip.hip, the camera and K
// gradients of camera_grad.hip and the host builds under tests/ all walk a slot through here and differ in the sink.  g = the nine
// gradient components of the slot's three vertices, vi0..vi2 = the mesh face's vertex indices, cd = the slot's code (clip_face), cw2 = the
// slot's two detached weights w2, w3.  Every original vertex whose ndc gradient is not all zero is handed to sink(i, vertex index,
// gradient), i = 0, 1, 2 in this order.  The projections and the weights are read for a clipped face only, inside its branch: hoisting
// them costs the vertex backward a wave per SIMD in registers.
DBW_HD bool all_zero(f3 g) { return g.x == 0.f && g.y == 0.f && g.z == 0.f; }
template <class Sink>
DBW_HD void clip_slot_walk(const float *verts, int vi0, int vi1, int vi2, const Cam &c, float eps, float zc, int persp, int cd, const float *cw2,
                           const float (&g)[9], Sink &&sink) {
    const f3 ga{g[0], g[1], g[2]}, gb{g[3], g[4], g[5]}, gc{g[6], g[7], g[8]};
    f3 gv0 = ga, gv1 = gb, gv2 = gc;
    if (cd >= 0) {
        const f3 q0 = project(verts + (long long)vi0 * 3, c, eps).ndc, q1 = project(verts + (long long)vi1 * 3, c, eps).ndc,
                 q2 = project(verts + (long long)vi2 * 3, c, eps).ndc;
        clip_slot_bwd(cd, q0, q1, q2, zc, persp, cw2[0], cw2[1], ga, gb, gc, gv0, gv1, gv2);
    }
    if (!all_zero(gv0)) sink(0, vi0, gv0);
    if (!all_zero(gv1)) sink(1, vi1, gv1);
    if (!all_zero(gv2)) sink(2, vi2, gv2);
}

}  // namespace dbw
