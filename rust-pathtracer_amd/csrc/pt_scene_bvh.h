// pt_scene_bvh.h — private to pt_scene_host.cpp: the axis-aligned box and the builder of both BVH levels.
#ifndef PT_SCENE_BVH_H
#define PT_SCENE_BVH_H
#include <cmath>
#include <cstring>
#include <vector>

#include "pt_blob.h"

namespace pth {
namespace {

struct Box { float mn[3], mx[3]; };

Box box_empty() { Box b; for (int i = 0; i < 3; ++i) { b.mn[i] = INFINITY; b.mx[i] = -INFINITY; } return b; }
void box_grow(Box& b, const float* p) { for (int i = 0; i < 3; ++i) { b.mn[i] = std::fmin(b.mn[i], p[i]); b.mx[i] = std::fmax(b.mx[i], p[i]); } }
void box_expand(Box& b, const Box& o) { for (int i = 0; i < 3; ++i) { b.mn[i] = std::fmin(b.mn[i], o.mn[i]); b.mx[i] = std::fmax(b.mx[i], o.mx[i]); } }
Box box_of_corners(const float* a, const float* b) {  // AABB::new, src/aabb.rs:16-21
    Box r; for (int i = 0; i < 3; ++i) { r.mn[i] = std::fmin(a[i], b[i]); r.mx[i] = std::fmax(a[i], b[i]); } return r;
}
void box_center(const Box& b, float* c) { for (int i = 0; i < 3; ++i) c[i] = b.mn[i] + (b.mx[i] - b.mn[i]) / 2.0f; }
float box_area(const Box& b) {  // src/aabb.rs:97-100
    float sx = b.mx[0] - b.mn[0], sy = b.mx[1] - b.mn[1], sz = b.mx[2] - b.mn[2];
    return 2.0f * (sx * sy + sx * sz + sy * sz);
}

uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
float bits_f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// Which form of the filtered slab test a box takes (pt_device.h aabb_classify_by / aabb_classify_code): 0 = it has thickness on every axis, 1 / 2 / 3 = flat
// along x / y / z only, 4 = flat along more than one axis; not 0 = "flat".  mn, mx: three floats each, or — a box read back from a record — three words each,
// then compared as words.
template <class T> uint32_t box_test_form(const T* mn, const T* mx) {
    const int fx = mn[0] == mx[0], fy = mn[1] == mx[1], fz = mn[2] == mx[2];
    return fx + fy + fz == 0 ? 0u : (fx + fy + fz > 1 ? 4u : (fx ? 1u : (fy ? 2u : 3u)));
}

// Skip-link BVH in pre-order, SAH with 6 buckets on the widest centroid axis, median split when the centroids
// coincide, one shape per leaf: the reference's build (src/accelerator/bvh.rs:299-457) emitted directly in
// the flattened order of src/accelerator/lbvh.rs:47-163, with each leaf merged into its navigator node.
struct BvhBuilder {
    const std::vector<Box>& shapes;
    std::vector<uint32_t>& out;  // PT_NODE_WORDS per node
    std::vector<uint32_t> leaf_of_shape;  // node index of each shape's leaf
    std::vector<char> no_cull;            // per shape (empty = none): its computed hit distance may fall short of its box (spheres): nodes holding one are never culled
    std::vector<float> sphere_radius;     // per shape (empty = none): > 0 an untransformed sphere's radius, +inf a sphere that must never be culled (transformed), 0 no sphere
    std::vector<float> node_margin;       // out, per node (filled when sphere_radius is given): pt_blob.h PT_HDR_TOP_MARGIN
    explicit BvhBuilder(const std::vector<Box>& s, std::vector<uint32_t>& o) : shapes(s), out(o), leaf_of_shape(s.size(), 0) {}

    uint32_t node_count() const { return (uint32_t)(out.size() / PT_NODE_WORDS); }

    void split(const std::vector<uint32_t>& idx, std::vector<uint32_t>& li, Box& lb, std::vector<uint32_t>& ri, Box& rb) {
        Box bounds = box_empty(), cbounds = box_empty();
        for (uint32_t i : idx) { float c[3]; box_center(shapes[i], c); box_expand(bounds, shapes[i]); box_grow(cbounds, c); }
        float size[3] = {cbounds.mx[0] - cbounds.mn[0], cbounds.mx[1] - cbounds.mn[1], cbounds.mx[2] - cbounds.mn[2]};
        float widest = std::fmax(std::fmax(size[0], size[1]), std::fmax(size[2], 0.0f));
        int axis = 0;
        for (int a = 0; a < 3; ++a) if (size[a] >= widest) axis = a;  // largest lane index among ties (bvh.rs:348-353)
        float extent = (0.0f >= widest) ? 0.0f : cbounds.mx[axis] - cbounds.mn[axis];
        if (extent < 0.00001f) {
            size_t half = idx.size() / 2;
            li.assign(idx.begin(), idx.begin() + half); ri.assign(idx.begin() + half, idx.end());
            lb = box_empty(); for (uint32_t i : li) box_expand(lb, shapes[i]);
            rb = box_empty(); for (uint32_t i : ri) box_expand(rb, shapes[i]);
            return;
        }
        const int NB = 6;
        size_t count[NB] = {0, 0, 0, 0, 0, 0}; Box bb[NB]; std::vector<uint32_t> members[NB];
        for (int b = 0; b < NB; ++b) bb[b] = box_empty();
        for (uint32_t i : idx) {
            float c[3]; box_center(shapes[i], c);
            float rel = (c[axis] - cbounds.mn[axis]) / extent;
            float fb = rel * ((float)NB - 0.01f);
            int b = fb >= 0.0f ? (int)fb : 0; if (b > NB - 1) b = NB - 1;
            count[b]++; box_expand(bb[b], shapes[i]); members[b].push_back(i);
        }
        int best = 0; float best_cost = INFINITY; lb = box_empty(); rb = box_empty();
        for (int k = 0; k < NB - 1; ++k) {
            size_t nl = 0, nr = 0; Box l = box_empty(), r = box_empty();
            for (int j = 0; j <= k; ++j) { nl += count[j]; box_expand(l, bb[j]); }
            for (int j = k + 1; j < NB; ++j) { nr += count[j]; box_expand(r, bb[j]); }
            float cost = ((float)nl * box_area(l) + (float)nr * box_area(r)) / box_area(bounds);
            if (cost < best_cost) { best = k; best_cost = cost; lb = l; rb = r; }
        }
        li.clear(); ri.clear();
        for (int j = 0; j <= best; ++j) li.insert(li.end(), members[j].begin(), members[j].end());
        for (int j = best + 1; j < NB; ++j) ri.insert(ri.end(), members[j].begin(), members[j].end());
    }

    void emit(const std::vector<uint32_t>& idx, const Box& box) {
        size_t at = out.size();
        out.resize(at + PT_NODE_WORDS, 0);
        bool leaf = idx.size() == 1;
        const Box& b = leaf ? shapes[idx[0]] : box;
        if (!leaf) { std::vector<uint32_t> li, ri; Box lb, rb; split(idx, li, lb, ri, rb); emit(li, lb); emit(ri, rb); }
        // [3]: the node to continue with when this subtree is done or skipped; bit 31 (PT_NODE_FLAT) marks a box of zero thickness,
        // which the filtered slab test must take axis by axis (aabb_classify)
        bool keep = false;
        if (!no_cull.empty()) for (uint32_t i : idx) keep = keep || no_cull[i] != 0;
        const uint32_t code = box_test_form(b.mn, b.mx);
        out[at + 0] = fbits(b.mn[0]); out[at + 1] = fbits(b.mn[1]); out[at + 2] = fbits(b.mn[2]); out[at + 3] = node_count() | (code != 0u ? PT_NODE_FLAT : 0u) | (keep ? PT_NODE_NO_CULL : 0u) | code << 27;
        out[at + 4] = fbits(b.mx[0]); out[at + 5] = fbits(b.mx[1]); out[at + 6] = fbits(b.mx[2]); out[at + 7] = leaf ? idx[0] : PT_NODE_INNER;
        if (leaf) leaf_of_shape[idx[0]] = (uint32_t)(at / PT_NODE_WORDS);
        if (!sphere_radius.empty()) {
            float rmax = 0.0f;
            for (uint32_t i : idx) rmax = std::fmax(rmax, sphere_radius[i]);
            const double dx = (double)b.mx[0] - b.mn[0], dy = (double)b.mx[1] - b.mn[1], dz = (double)b.mx[2] - b.mn[2];
            const double m0 = 3.5 * rmax + PT_SPHERE_CULL_K * (std::sqrt(dx * dx + dy * dy + dz * dz) + rmax);
            if (node_margin.size() < at / PT_NODE_WORDS + 1) node_margin.resize(at / PT_NODE_WORDS + 1, 0.0f);
            node_margin[at / PT_NODE_WORDS] = rmax > 0.0f ? std::nextafterf((float)m0, INFINITY) : 0.0f;   // (inf stays inf)
        }
    }

    void build() {
        if (shapes.empty()) return;
        std::vector<uint32_t> idx(shapes.size());
        for (size_t i = 0; i < idx.size(); ++i) idx[i] = (uint32_t)i;
        if (idx.size() == 1) { emit(idx, shapes[0]); return; }
        std::vector<uint32_t> li, ri; Box lb, rb;
        split(idx, li, lb, ri, rb);  // the root itself has no node (lbvh.rs:134-140)
        emit(li, lb); emit(ri, rb);
    }
};

}  // namespace
}  // namespace pth
#endif
