// Scene parsing maps (include/dbw_viz.h: dbw_viz_parse_fwd; csrc/scene_parse.hip): what a pixel keeps while its tile's faces go by, host
// and device code like the other *_math.h headers (the CPU tests compile it with g++: tests/host_parse_math.cpp).
//
// The inside test and pz of a (pixel, face) pair are eval_pair's (raster_math.h), fed by raster_tile (raster_common.h) exactly as into the
// training path's TopK -- nothing of that arithmetic is restated here.  What differs is what is KEPT: one nearest fragment (a TopK<1>: the
// rasteriser's own (pz, face index) order and its sibling rule, so the nearest face is the one a K = 1 pass stores) and a 64-bit coverage
// word, bit l = some face with label l passed the inside test at this pixel, however many faces lie in front of it.  A sorted list cannot
// give the second: it is capped at DBW_MAX_FACES_PER_PIXEL = 25 entries and a 50-block scene puts 100 faces on a ray.
#pragma once
#include "raster_math.h"

namespace dbw {

constexpr int PARSE_MAX_LABELS = 64;        // == DBW_VIZ_MAX_LABELS: one bit of the coverage word each
constexpr int PARSE_NO_LABEL = 255;         // `label` where no face passes

// ---- labels and their bits --------------------------------------------------------------------------------------------------------------
DBW_HD bool parse_label_ok(int label) { return (unsigned)label < (unsigned)PARSE_MAX_LABELS; }
// index of the first entry of a label table outside [0, 64), -1 if there is none
DBW_HD long long parse_first_bad_label(const int32_t *face_label, long long F) {
    for (long long j = 0; j < F; ++j)
        if (!parse_label_ok(face_label[j])) return j;
    return -1;
}
// (bit 63 is a legal label: the word is unsigned here and the sign bit of the int64 the caller sees)
DBW_HD uint64_t parse_bit(int label) { return 1ull << (label & (PARSE_MAX_LABELS - 1)); }
DBW_HD bool parse_covers(uint64_t cover, int label) { return ((cover >> (label & (PARSE_MAX_LABELS - 1))) & 1ull) != 0ull; }
// lowest label of a non-zero word, which loses it
DBW_HD int parse_pop_label(uint64_t &rem) {
    const int l = __builtin_ctzll(rem);
    rem &= rem - 1ull;
    return l;
}
// label of clipped face f (a row of the clipped face table of N views with `F` original faces each): that of the original face c2o[f]; an
// unclipped table holds the views' faces one after the other.  An index outside [0, F) -- the unused rows behind a view's num_faces hold
// anything -- is folded into the table: such a row is never rasterised, and nothing is read out of bounds for it.  The label itself is
// folded into [0, 64) as well: tables that were not validated on the host (dbw_viz.h) stay memory safe.
DBW_HD int parse_clipped_label(const int32_t *face_label, const int32_t *c2o, long long f, int F) {
    long long j = c2o ? (long long)c2o[f] : f;
    j %= F;
    if (j < 0) j += F;
    return face_label[j] & (PARSE_MAX_LABELS - 1);
}

// ---- what a pixel keeps -----------------------------------------------------------------------------------------------------------------
// The list type raster_tile / eval_staged_chunk write to (the interface of TopK they use: init, sibling, insert / insert_ordered).
//  * nearest: TopK<1> under the full (pz, face index) key -- insert(), not insert_ordered(): one 64-bit compare more per kept pair and
//    the result does not depend on the order the faces arrive in;
//  * cover: every pair that passed the inside test sets the bit of its face's label, BEFORE the nearest rule looks at it.  The two
//    triangles of a clipped quad (the sibling rule) share their original face and with it their label.
// `lab`: label of every clipped face (parse_clipped_label), indexed like the face records.  The face index of a call is the same for all
// pixels of a wave, so on the device the label arrives through a scalar load and the shift is scalar too.
struct ParsePixel {
    TopK<1> top;
    uint64_t cover;
    const int32_t *lab;

    DBW_HD void init() { top.init(); cover = 0ull; }
    DBW_HD void see(bool on, int id) { if (on) cover |= parse_bit(lab[id]); }
    DBW_HD bool sibling(int K, bool on, int nb, float dist, float pz, int id, const pay4 &v, pay4 *home, int stride, int lane) {
        see(on, id);
        return top.sibling(K, on, nb, dist, pz, id, v, home, stride, lane);
    }
    DBW_HD void insert(int K, bool on, float pz, int id, const pay4 &v, pay4 *home, int stride, int lane) {
        see(on, id);
        top.insert(K, on, pz, id, v, home, stride, lane);
    }
    DBW_HD void insert_ordered(int K, bool on, float pz, int id, const pay4 &v, pay4 *home, int stride, int lane) { insert(K, on, pz, id, v, home, stride, lane); }
    // -> the pixel's outputs: label (PARSE_NO_LABEL where no face passed), depth (-1 there: what zbuf[..., 0] holds) and the clipped face
    DBW_HD void result(int &label, float &depth, int &face) const {
        label = PARSE_NO_LABEL; depth = -1.f; face = -1;
        pay4 v;
        float pz;
        int fi;
        if (top.get(0, nullptr, 0, 0, pz, fi, v)) { label = lab[fi]; depth = pz; face = fi; }
    }
};

// ---- counts -----------------------------------------------------------------------------------------------------------------------------
// counts (64, 2) of one view: [l][0] pixels whose coverage word has bit l (amodal area), [l][1] pixels whose nearest face has label l
// (visible area).  The definition, one pixel at a time; the kernel adds the same integers a wave at a time (ballot + popcount per label
// present), a workgroup at a time in LDS, and then with one integer atomic per non-zero counter.
DBW_HD void parse_count_pixel(int32_t *counts, uint64_t cover, int label) {
    uint64_t rem = cover;
    while (rem) counts[parse_pop_label(rem) * 2] += 1;
    if (label != PARSE_NO_LABEL) counts[label * 2 + 1] += 1;
}

}  // namespace dbw
