// pt_scene_certify.h — private to pt_scene_host.cpp: what the host certifies about a mesh in f64 — closed, convex (per instance, in world space), its inner balls.
#ifndef PT_SCENE_CERTIFY_H
#define PT_SCENE_CERTIFY_H
#include <algorithm>

#include "../../include/pt_api.h"
#include "pt_scene_bvh.h"

namespace pth {
namespace {

// ---- a closed mesh's inner sphere (pt_blob.h PT_MESH_INNER_*), all in f64 -------------------------------------------------------------
// Closed = every undirected edge (vertices compared by POSITION: OBJ files repeat vertices along seams) belongs to exactly two triangles.  The centre is the point
// of a 9 x 9 x 9 grid over the bounding box that is farthest from the surface among those at odd crossing parity along three axis rays (all three must agree);
// the radius 0.98 x its distance to the nearest triangle.  Any failure — an open edge, a degenerate triangle, rays that disagree, a ball smaller than 2 % of the
// box — and the mesh simply has no ball.
struct D3 { double x, y, z; };
static inline D3 d3(const float* p) { return D3{p[0], p[1], p[2]}; }
static inline D3 dsub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
static inline double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline D3 dcross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// squared distance from p to triangle abc (Ericson, Real-Time Collision Detection 5.1.5)
static double point_triangle_dist2(D3 p, D3 a, D3 b, D3 c) {
    const D3 ab = dsub(b, a), ac = dsub(c, a), ap = dsub(p, a);
    const double d1 = ddot(ab, ap), d2 = ddot(ac, ap);
    auto len2 = [](D3 v) { return ddot(v, v); };
    if (d1 <= 0 && d2 <= 0) return len2(ap);
    const D3 bp = dsub(p, b); const double d3_ = ddot(ab, bp), d4 = ddot(ac, bp);
    if (d3_ >= 0 && d4 <= d3_) return len2(bp);
    const double vc = d1 * d4 - d3_ * d2;
    if (vc <= 0 && d1 >= 0 && d3_ <= 0) { const double v = d1 / (d1 - d3_); return len2(dsub(ap, D3{ab.x * v, ab.y * v, ab.z * v})); }
    const D3 cp = dsub(p, c); const double d5 = ddot(ab, cp), d6 = ddot(ac, cp);
    if (d6 >= 0 && d5 <= d6) return len2(cp);
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0 && d2 >= 0 && d6 <= 0) { const double w = d2 / (d2 - d6); return len2(dsub(ap, D3{ac.x * w, ac.y * w, ac.z * w})); }
    const double va = d3_ * d6 - d5 * d4;
    if (va <= 0 && (d4 - d3_) >= 0 && (d5 - d6) >= 0) { const double w = (d4 - d3_) / ((d4 - d3_) + (d5 - d6)); const D3 bc = dsub(c, b); return len2(dsub(bp, D3{bc.x * w, bc.y * w, bc.z * w})); }
    const double denom = 1.0 / (va + vb + vc), v = vb * denom, w = vc * denom;
    return len2(dsub(ap, D3{ab.x * v + ac.x * w, ab.y * v + ac.y * w, ab.z * v + ac.z * w}));
}
// crossings of the ray p + t e_axis, t > 0, with the triangles; -1 if the ray passes within 1e-9 (relative) of an edge or vertex (the caller drops the point)
static int axis_crossings(D3 p, int axis, const float* V, const uint32_t* ix, uint32_t faces, double scale) {
    const int u = (axis + 1) % 3, v = (axis + 2) % 3;
    auto comp = [](D3 q, int k) { return k == 0 ? q.x : (k == 1 ? q.y : q.z); };
    int n = 0;
    for (uint32_t f = 0; f < faces; ++f) {
        const D3 a = d3(V + 3 * ix[3 * f]), b = d3(V + 3 * ix[3 * f + 1]), c = d3(V + 3 * ix[3 * f + 2]);
        const double pu = comp(p, u), pv = comp(p, v);
        const double au = comp(a, u) - pu, av = comp(a, v) - pv, bu_ = comp(b, u) - pu, bv = comp(b, v) - pv, cu = comp(c, u) - pu, cv = comp(c, v) - pv;
        const double e0 = bu_ * cv - bv * cu, e1 = cu * av - cv * au, e2 = au * bv - av * bu_;   // 2D edge functions of the projection
        const double eps = 1e-9 * scale * scale;
        const int pos = (e0 > eps) + (e1 > eps) + (e2 > eps), neg = (e0 < -eps) + (e1 < -eps) + (e2 < -eps);
        if (pos == 3 || neg == 3) {                       // strictly inside the projected triangle: the ray's line crosses the triangle's plane there
            const double det = e0 + e1 + e2;
            const double t = (e0 * (comp(a, axis) - comp(p, axis)) + e1 * (comp(b, axis) - comp(p, axis)) + e2 * (comp(c, axis) - comp(p, axis))) / det;
            if (std::fabs(t) < 1e-9 * scale) return -1;
            if (t > 0) ++n;
        } else if (!(pos > 0 && neg > 0)) return -1;      // on, or too close to, an edge, a vertex, or the line of a triangle seen edge-on: this point is not used
    }
    return n;
}
// Closed = every undirected edge (end points compared by the BIT PATTERNS of their positions) belongs to exactly two triangles, and no triangle is degenerate:
// not an edge of length 0 and — round-5 advisor — not a sliver either.  A T-junction filled with a zero-area triangle (three distinct collinear vertices) still pairs
// every edge twice, but the watertight triangle test is watertight only across edges computed from the SAME vertex pair (mesh.rs:67-198): through such a junction a ray
// can meet the det == 0 triangle alone and pass.  "Closed" is what the shortcuts below argue from, so such a mesh is not closed.
static bool mesh_is_closed(const float* V, uint32_t vertex_count, const uint32_t* ix, uint32_t faces, const Box& mb) {
    struct Key { uint32_t a[3], b[3]; bool operator<(const Key& o) const { return std::memcmp(this, &o, sizeof(Key)) < 0; } };
    auto pos = [&](uint32_t v, uint32_t* out) { for (int k = 0; k < 3; ++k) { float x = V[3 * v + k]; if (x == 0.0f) x = 0.0f; std::memcpy(&out[k], &x, 4); } };   // (-0 = +0)
    const double ex = (double)mb.mx[0] - mb.mn[0], ey = (double)mb.mx[1] - mb.mn[1], ez = (double)mb.mx[2] - mb.mn[2];
    const double extent = std::fmax(ex, std::fmax(ey, ez));
    std::vector<Key> edges; edges.reserve((size_t)faces * 3);
    for (uint32_t f = 0; f < faces; ++f) {
        for (int k = 0; k < 3; ++k) if (ix[3 * f + k] >= vertex_count) return false;
        const D3 a = d3(V + 3 * ix[3 * f]), b = d3(V + 3 * ix[3 * f + 1]), c = d3(V + 3 * ix[3 * f + 2]);
        const D3 n = dcross(dsub(b, a), dsub(c, a));
        if (!(std::sqrt(ddot(n, n)) > 1e-10 * extent * extent)) return false;     // twice the area: a sliver (or NaN)
        for (int k = 0; k < 3; ++k) {
            const uint32_t v0 = ix[3 * f + k], v1 = ix[3 * f + (k + 1) % 3];
            Key e; pos(v0, e.a); pos(v1, e.b);
            if (std::memcmp(e.a, e.b, 12) == 0) return false;                    // a degenerate edge
            if (std::memcmp(e.a, e.b, 12) > 0) { uint32_t t[3]; std::memcpy(t, e.a, 12); std::memcpy(e.a, e.b, 12); std::memcpy(e.b, t, 12); }
            edges.push_back(e);
        }
    }
    std::sort(edges.begin(), edges.end());
    for (size_t i = 0; i < edges.size();) {
        size_t j = i; while (j < edges.size() && std::memcmp(&edges[j], &edges[i], sizeof(Key)) == 0) ++j;
        if (j - i != 2) return false;
        i = j;
    }
    return true;
}

// ---- a CONVEX closed mesh instance (pt_blob.h PT_INST_CONVEX_*), certified in f64 in WORLD space ---------------------------------------------------------------------
// What stage_shade argues from when it marks a light-sample ray that leaves such an instance (outward: the instance cannot be hit again; inward: nothing but this
// instance's own surface — or something inside it — can be the closest hit, and no light is inside).  Every number the argument uses is checked here, for the vertices
// as the engine sees them (f32 positions through the instance's f32 forward matrix) and the normals as hit_record makes them (vertex normals, or the face normal, through
// the transposed reverse matrix):
//   closed (above); at most 4096 faces; world coordinates within 64 (one f32 ulp there is 4e-6: a hundred times below the margins);
//   every face's hit normals lie on its outward side; per face: the largest angle delta between the face's own normal and its hit normals (0 for a flat-shaded face), faces
//   with cos(delta) < 0.5 taking no claim;
//   CONVEX: no vertex lies more than 2e-4 above any face's plane (the gem's facets are planar to 1e-4) and some vertex lies 1e-2 below it;
//   OUT, face by face: the threshold 0.02 + sin(delta) a direction's cosine to the hit normal must exceed (PT_TRI_OUT_SHIFT);
//   IN, face by face: the face's three corners, moved 1e-3 against the face normal (where pt.rs:176 puts an inward ray's origin), lie at least 1e-4 below EVERY face plane —
//   so does every point of the face (the planes' half-spaces are convex); such a face's triangle carries PT_TRI_IN_SAFE and hit_record hands it on in the hit's instance word;
//   and the world box of every light-tagged instance is disjoint from this instance's (both widened by 1e-3).
static uint32_t convex_certificate(const float* V, uint32_t vertex_count, const uint32_t* ix, uint32_t faces, const float* N, const pt_instance& in, const Box& wbox,
                                   const std::vector<Box>& light_boxes, std::vector<uint32_t>* face_flags) {
    if (faces < 4 || faces > 4096 || vertex_count > 3 * 4096) return 0u;
    auto world = [&](const float* p) {
        if (!in.has_transform) return D3{p[0], p[1], p[2]};
        const float* m = in.forward;
        return D3{(double)m[0] * p[0] + (double)m[1] * p[1] + (double)m[2] * p[2] + m[3], (double)m[4] * p[0] + (double)m[5] * p[1] + (double)m[6] * p[2] + m[7],
                  (double)m[8] * p[0] + (double)m[9] * p[1] + (double)m[10] * p[2] + m[11]};
    };
    auto world_normal = [&](D3 n) {   // hit_record: normalize(reverse^T n)
        if (in.has_transform) { const float* r = in.reverse; n = D3{r[0] * n.x + r[4] * n.y + r[8] * n.z, r[1] * n.x + r[5] * n.y + r[9] * n.z, r[2] * n.x + r[6] * n.y + r[10] * n.z}; }
        const double l = std::sqrt(ddot(n, n));
        return D3{n.x / l, n.y / l, n.z / l};
    };
    std::vector<D3> W(vertex_count);
    for (uint32_t v = 0; v < vertex_count; ++v) {
        W[v] = world(V + 3 * v);
        if (!(std::fabs(W[v].x) <= 64.0 && std::fabs(W[v].y) <= 64.0 && std::fabs(W[v].z) <= 64.0)) return 0u;
    }
    const double kSlack = 2e-4, kThick = 1e-2, kOffset = 1e-3, kInside = 1e-4, kMinCos = 0.5;
    std::vector<D3> fn(faces); std::vector<double> fd(faces), fsin(faces), fcos(faces);   // per face: the plane, and the sine / cosine of the largest angle between its normal and its hit normals
    for (uint32_t f = 0; f < faces; ++f) {
        const D3 a = W[ix[3 * f]], b = W[ix[3 * f + 1]], c = W[ix[3 * f + 2]];
        D3 g = dcross(dsub(b, a), dsub(c, a));
        const double l = std::sqrt(ddot(g, g));
        if (!(l > 0)) return 0u;
        g = D3{g.x / l, g.y / l, g.z / l};
        // the hit normals of this face, as hit_record makes them (local: the vertex normals, or cross(p0 - p2, p1 - p2))
        D3 local[3]; int count = 0;
        if (N != nullptr) for (int k = 0; k < 3; ++k) local[count++] = d3(N + 3 * ix[3 * f + k]);
        else { const D3 p0 = d3(V + 3 * ix[3 * f]), p1 = d3(V + 3 * ix[3 * f + 1]), p2 = d3(V + 3 * ix[3 * f + 2]); local[count++] = dcross(dsub(p0, p2), dsub(p1, p2)); }
        const D3 first = world_normal(local[0]);
        if (ddot(first, g) < 0) g = D3{-g.x, -g.y, -g.z};   // (the face's plane normal on the side the hit normals point to: it must turn out to be the OUTWARD side, below)
        // a hit's normal is normalize(sum b_i n_i), b_i >= 0: no farther from the face's normal than the farthest n_i (a flat-shaded face: the face's own, rounding apart)
        double cmin = 1.0;
        for (int k = 0; k < count; ++k) cmin = std::fmin(cmin, ddot(world_normal(local[k]), g));
        if (!(cmin > 0.0)) return 0u;                        // a hit normal on the other side of its own face
        fn[f] = g; fd[f] = ddot(g, a); fcos[f] = cmin; fsin[f] = std::sqrt(std::fmax(0.0, 1.0 - cmin * cmin));
    }
    for (uint32_t f = 0; f < faces; ++f) {
        double hi = -INFINITY, lo = INFINITY;
        for (uint32_t v = 0; v < vertex_count; ++v) { const double sd = ddot(fn[f], W[v]) - fd[f]; hi = std::fmax(hi, sd); lo = std::fmin(lo, sd); }
        if (!(hi <= kSlack && lo <= -kThick)) return 0u;   // not convex (or the normals point inward, or the body is a sliver)
    }
    // OUT, face by face: the origin p + 1e-3 n (n a hit normal) lies 1e-3 cos(delta) above the face's plane — at least 5e-4: above the slack — and a direction with
    // n . d > sin(delta) has angle(d, face normal) <= angle(d, n) + delta < 90 degrees: it moves away from the plane.  The threshold rides in the triangle's flag word in
    // units of 2^-15, rounded up, + 0.02 (rounding of n . d in f32, of a normal's length: 1e-6).
    face_flags->assign(faces, 0u);
    bool any_out = false;
    for (uint32_t f = 0; f < faces; ++f) {
        if (!(fcos[f] >= kMinCos)) continue;
        const uint32_t tq = (uint32_t)std::ceil((fsin[f] + 0.02) * 32768.0);
        if (tq == 0u || tq > 32767u) continue;
        (*face_flags)[f] = tq << PT_TRI_OUT_SHIFT;
        any_out = true;
    }
    if (!any_out) return 0u;
    uint32_t flags = PT_INST_CONVEX_OUT;
    // IN is a property of a FACE (a sharp edge — the brilliant cut has 64 faces at edges of 97 degrees — puts the corner of one face, moved inward, OUTSIDE the next
    // face's plane): `in_safe[f]`, and the instance takes the flag when any of its faces is safe
    // (the origin is p - 1e-3 n with n within delta of the face's normal: it lies within 1e-3 * 2 sin(delta / 2) of p - 1e-3 n_f, so that point must clear every plane by that much more)
    bool inside_ok = false;
    std::vector<char> in_safe(faces, 0);   // (0 none, 1 the whole face, 2 its inside only)
    for (uint32_t f = 0; f < faces; ++f) {
        if (!(fcos[f] >= kMinCos)) continue;
        const double need = kInside + kOffset * std::sqrt(std::fmax(0.0, 2.0 - 2.0 * fcos[f]));   // 2 sin(delta / 2) = sqrt(2 - 2 cos delta)
        bool ok = true;
        for (int k = 0; k < 3 && ok; ++k) {
            const D3 p = W[ix[3 * f + k]], q = D3{p.x - kOffset * fn[f].x, p.y - kOffset * fn[f].y, p.z - kOffset * fn[f].z};
            for (uint32_t g = 0; g < faces; ++g) if (!(ddot(fn[g], q) - fd[g] <= -need)) { ok = false; break; }
        }
        if (!ok) {   // the face without a strip of PT_TRI_INNER_BARY along its edges (hit_record tests the hit's barycentric coordinates): the corners of that inner triangle
            ok = true;
            const double e = PT_TRI_INNER_BARY * 0.98;   // (the device compares f32 barycentrics: a margin for their rounding)
            for (int k = 0; k < 3 && ok; ++k) {
                const D3 a = W[ix[3 * f + k]], b = W[ix[3 * f + (k + 1) % 3]], c = W[ix[3 * f + (k + 2) % 3]];
                const D3 p = D3{(1 - 2 * e) * a.x + e * b.x + e * c.x, (1 - 2 * e) * a.y + e * b.y + e * c.y, (1 - 2 * e) * a.z + e * b.z + e * c.z};
                const D3 q = D3{p.x - kOffset * fn[f].x, p.y - kOffset * fn[f].y, p.z - kOffset * fn[f].z};
                for (uint32_t g = 0; g < faces; ++g) if (!(ddot(fn[g], q) - fd[g] <= -need)) { ok = false; break; }
            }
            in_safe[f] = ok ? 2 : 0;
        } else in_safe[f] = 1;
        inside_ok = inside_ok || ok;
    }
    bool lights_clear = true;
    for (const Box& lb : light_boxes) {
        bool apart = false;
        for (int k = 0; k < 3; ++k) apart = apart || (double)lb.mn[k] - 1e-3 > (double)wbox.mx[k] + 1e-3 || (double)lb.mx[k] + 1e-3 < (double)wbox.mn[k] - 1e-3;
        lights_clear = lights_clear && apart;
    }
    if (inside_ok && lights_clear) {
        flags |= PT_INST_CONVEX_IN;
        for (uint32_t f = 0; f < faces; ++f) (*face_flags)[f] |= in_safe[f] == 1 ? PT_TRI_IN_SAFE : (in_safe[f] == 2 ? PT_TRI_IN_SAFE_INNER : 0u);
    }
    return flags;
}

static bool inner_sphere(const float* V, uint32_t vertex_count, const uint32_t* ix, uint32_t faces, const Box& mb, float* centre, float* radius, std::vector<float>* more = nullptr) {
    if (!mesh_is_closed(V, vertex_count, ix, faces, mb)) return false;
    const double sx = (double)mb.mx[0] - mb.mn[0], sy = (double)mb.mx[1] - mb.mn[1], sz = (double)mb.mx[2] - mb.mn[2];
    const double scale = std::fmax(sx, std::fmax(sy, sz));
    if (!(scale > 0) || !(sx > 0 && sy > 0 && sz > 0)) return false;
    const int G = 9;
    double best_r2 = 0; D3 best{0, 0, 0};
    struct Cand { D3 p; double r2; };
    std::vector<Cand> inside_points;   // (every inside grid point with its distance: the candidates of the further balls, below)
    const bool want_more = more != nullptr && faces <= 20000;
    for (int gx = 0; gx < G; ++gx) for (int gy = 0; gy < G; ++gy) for (int gz = 0; gz < G; ++gz) {
        // (grid points at irrational-ish offsets, so that axis rays do not run along the seams of symmetric models)
        const D3 p{mb.mn[0] + sx * (gx + 0.5137) / G, mb.mn[1] + sy * (gy + 0.4871) / G, mb.mn[2] + sz * (gz + 0.5063) / G};
        double r2 = INFINITY;
        const double stop_below = want_more ? 0.0 : best_r2;
        for (uint32_t f = 0; f < faces && r2 > stop_below; ++f)
            r2 = std::fmin(r2, point_triangle_dist2(p, d3(V + 3 * ix[3 * f]), d3(V + 3 * ix[3 * f + 1]), d3(V + 3 * ix[3 * f + 2])));
        if (!(r2 > (want_more ? 1e-6 * scale * scale : best_r2))) continue;
        bool inside = true;
        for (int axis = 0; axis < 3 && inside; ++axis) { const int n = axis_crossings(p, axis, V, ix, faces, scale); inside = n > 0 && (n & 1) == 1; }
        if (!inside) continue;
        if (want_more) inside_points.push_back(Cand{p, r2});
        if (r2 > best_r2) { best_r2 = r2; best = p; }
    }
    if (!(best_r2 > 0)) return false;
    // refine the centre: a pattern search from the best grid point (the distance field has no other structure to use), steps from a grid cell down to 1e-4 of the box.
    // A step is taken only to a point that is farther from the surface; it cannot leave the inside: the segment to it stays within the old ball.
    auto dist2 = [&](D3 p, double stop_below) {
        double r2 = INFINITY;
        for (uint32_t f = 0; f < faces && r2 > stop_below; ++f) r2 = std::fmin(r2, point_triangle_dist2(p, d3(V + 3 * ix[3 * f]), d3(V + 3 * ix[3 * f + 1]), d3(V + 3 * ix[3 * f + 2])));
        return r2;
    };
    for (double step = scale / G; step > 1e-4 * scale; step *= 0.5) {
        for (int tries = 0; tries < 64; ++tries) {
            bool moved = false;
            for (int k = 0; k < 6; ++k) {
                const double s1 = (k & 1) ? -step : step;
                if (!(step < std::sqrt(best_r2))) break;      // (the new centre must lie inside the present ball)
                D3 q = best; if (k / 2 == 0) q.x += s1; else if (k / 2 == 1) q.y += s1; else q.z += s1;
                const double r2 = dist2(q, best_r2);
                if (r2 > best_r2) { best_r2 = r2; best = q; moved = true; }
            }
            if (!moved) break;
        }
    }
    const double r = 0.98 * std::sqrt(best_r2);
    if (!(r > 0.02 * scale)) return false;
    centre[0] = (float)best.x; centre[1] = (float)best.y; centre[2] = (float)best.z; *radius = (float)(r * 0.9999);
    // Further balls (at most PT_MESH_MORE_BALLS): greedily the inside grid point farthest from the surface whose CENTRE lies outside every ball taken so far — a
    // ball somewhere else in the body — as long as it is at least a quarter of the first one's radius.  (What they buy was priced on C3's rays before it was built:
    // the first ball catches 24 % of the blocked rays that enter the gem's box, eight balls 58 %.)
    if (want_more) {
        std::vector<D3> centres{best}; std::vector<double> radii{r};
        while (centres.size() < 1 + PT_MESH_MORE_BALLS) {
            const Cand* pick = nullptr;
            for (const Cand& c : inside_points) {
                bool outside_all = true;
                for (size_t k = 0; k < centres.size() && outside_all; ++k) { const D3 dd = dsub(c.p, centres[k]); outside_all = ddot(dd, dd) > radii[k] * radii[k]; }
                if (outside_all && (pick == nullptr || c.r2 > pick->r2)) pick = &c;
            }
            if (pick == nullptr || !(0.98 * std::sqrt(pick->r2) >= PT_MESH_MORE_MIN * r)) break;
            const double rr = 0.98 * std::sqrt(pick->r2);
            centres.push_back(pick->p); radii.push_back(rr);
            more->push_back((float)pick->p.x); more->push_back((float)pick->p.y); more->push_back((float)pick->p.z); more->push_back((float)(rr * 0.9999));
        }
    }
    return true;
}

}  // namespace
}  // namespace pth
#endif
