// The gather-and-box launch of csrc/surface_term.hip for the terms that walk the same faces (csrc/freespace_term.hip): one workgroup per
// group writes the 9 coordinates of each of its kept faces into tri (12 floats a face; floats 9..11 are left to the caller) and the group's
// axis-aligned box into boxes (8 floats a group: lo at 0..2, hi at 4..6; +inf / -inf for a group that is dropped or empty).  A face index
// outside [0, V) is read as vertex 0.  Returns dbw_check_launch's code.
#pragma once
#include "dbw_common.h"

int dbw_surface_box_launch(const float *verts, int V, const int32_t *faces, int F, const int32_t *face_group, const int32_t *group_keep, int G,
                           float *tri, float *boxes, hipStream_t stream);
