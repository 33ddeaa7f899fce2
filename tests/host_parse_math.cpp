// Host build (g++) of csrc/parse_math.h for tests/test_host_parse_math.py: the same inline functions scene_parse_kernel compiles, driven by
// the loop that kernel runs (one lane per pixel there, one iteration here).  The (pixel, face) inside test and pz are INPUTS here: they are
// eval_pair's (tests/test_host_raster_math.py holds that one).
#include "../differentiable-blocksworld_amd/csrc/parse_math.h"

using namespace dbw;

extern "C" {

// P pixels, M candidate faces in ARRIVAL order: ids (M) clipped face indices, pass (P,M) 0 / 1 the inside test, pz (P,M) depths, lab
// (faces) the label of every clipped face.  -> label (P) u8, depth (P), cover (P) i64, face (P), counts (64,2) summed over the pixels.
int host_parse_pixels(const int *ids, const unsigned char *pass, const float *pz, const int *lab, int P, int M, unsigned char *label, float *depth,
                      long long *cover, int *face, int *counts) {
    for (int i = 0; i < PARSE_MAX_LABELS * 2; ++i) counts[i] = 0;
    for (int p = 0; p < P; ++p) {
        ParsePixel q;
        q.lab = lab;
        q.init();
        const pay4 v{-1.f, 0.f, 0.f, 0.f};
        for (int m = 0; m < M; ++m) q.insert_ordered(1, pass[p * M + m] != 0, pz[p * M + m], ids[m], v, nullptr, 0, 0);
        int l, f;
        float d;
        q.result(l, d, f);
        label[p] = (unsigned char)l; depth[p] = d; cover[p] = (long long)q.cover; face[p] = f;
        parse_count_pixel(counts, q.cover, l);
    }
    return 0;
}

long long host_first_bad_label(const int *face_label, long long F) { return parse_first_bad_label(face_label, F); }

// labels of the rows [0, F_total) of a clipped face table (c2o may be null: an unclipped table)
int host_clipped_labels(const int *face_label, const int *c2o, long long F_total, int F, int *out) {
    for (long long f = 0; f < F_total; ++f) out[f] = parse_clipped_label(face_label, c2o, f, F);
    return 0;
}

unsigned long long host_parse_bit(int label) { return parse_bit(label); }
int host_parse_covers(unsigned long long cover, int label) { return parse_covers(cover, label) ? 1 : 0; }
int host_parse_constants(int *out) { out[0] = PARSE_MAX_LABELS; out[1] = PARSE_NO_LABEL; return 0; }

}
