// Arithmetic of the 8-bit frame export (frame_export.hip), written once for the device (hipcc) and for the host (g++:
// tests/test_host_frame_math.py builds it into a checker-side shared object and compares it, without a GPU, with the bytes of the
// reference's convert_to_img and with torch's fp32 evaluation of the composite and the edge blend).
//
// All fp32, one rounding per operation (-ffp-contract=off), in the order the Python expressions evaluate:
//  * composite over a background (renderer._composite_bkg, PREMULTIPLIED rgb as it stands there): (rgb * alpha) + ((1 - alpha) * bkg);
//  * edge blend (Renderer.draw_edges): (img * (1 - mask)) + (mask * colour);
//  * quantise (the reference's convert_to_img, utils/image.py:51-53; save_video, :98, gives the same bytes): clamp to [0, 1], multiply
//    by 255.0f, truncate toward zero.  NaN -> 0 (numpy leaves that cast undefined; a frame must not depend on it).
#pragma once
#include <stdint.h>

#include "raster_math.h"      // DBW_HD

namespace dbw {

// frame flags of dbw_frames_u8 (include/dbw_export.h: DBW_FRAME_*)
constexpr int FRAME_HWC = 1, FRAME_EDGE_FIRST = 2, FRAME_CLAMP_INPUT = 4;

DBW_HD float frame_clamp01(float x) { return !(x > 0.f) ? 0.f : (x > 1.f ? 1.f : x); }       // NaN and -0 -> +0

DBW_HD float frame_composite(float rgb, float alpha, float bkg) {
    const float a = rgb * alpha, b = (1.f - alpha) * bkg;
    return a + b;
}

DBW_HD float frame_edge_blend(float img, float mask, float colour) {
    const float a = img * (1.f - mask), b = mask * colour;
    return a + b;
}

DBW_HD uint8_t frame_quantise(float x) { return (uint8_t)(int)(frame_clamp01(x) * 255.0f); }

// One pixel: px = (r, g, b, alpha); bkg / colour: 3 floats each; has_bkg / has_mask switch the two optional steps.  flags:
// FRAME_CLAMP_INPUT clamps the four channels first (render_rotated_views clamps its render before the composite), FRAME_EDGE_FIRST
// blends the edges in front of the composite (render_views paints them on the premultiplied rgb) instead of behind it.
DBW_HD void frame_pixel(const float px[4], bool has_bkg, const float bkg[3], bool has_mask, float mask, const float colour[3], int flags,
                        uint8_t out[3]) {
    float c[3] = {px[0], px[1], px[2]}, alpha = px[3];
    if (flags & FRAME_CLAMP_INPUT) {
        for (int k = 0; k < 3; ++k) c[k] = frame_clamp01(c[k]);
        alpha = frame_clamp01(alpha);
    }
    if (has_mask && (flags & FRAME_EDGE_FIRST))
        for (int k = 0; k < 3; ++k) c[k] = frame_edge_blend(c[k], mask, colour[k]);
    if (has_bkg)
        for (int k = 0; k < 3; ++k) c[k] = frame_composite(c[k], alpha, bkg[k]);
    if (has_mask && !(flags & FRAME_EDGE_FIRST))
        for (int k = 0; k < 3; ++k) c[k] = frame_edge_blend(c[k], mask, colour[k]);
    for (int k = 0; k < 3; ++k) out[k] = frame_quantise(c[k]);
}

}  // namespace dbw
