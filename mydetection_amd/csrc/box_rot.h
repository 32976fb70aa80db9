// cos and sin of a box angle in degrees, as every kernel that places rotated boxes on pixels takes them (draw.hip, crop.hip;
// include/mydet.h has the rule): angle == 0 gives c = 1, s = 0 with no trigonometric call, anything else cosf / sinf of
// fmodf(angle, 360) * (pi / 180) in float32.  QUARTERS (the chip sampler) adds exact values where fmodf(angle, 360) is +-90,
// +-180 or +-270, so that a quarter turn maps pixel centres to pixel centres; the overlay renderer keeps cosf / sinf there.
#pragma once
#include "common.h"

template <bool QUARTERS>
__device__ __forceinline__ void box_rotation(float ang, float &c, float &s) {
    c = 1.0f;
    s = 0.0f;
    if (ang != 0.0f) {
        const float r = fmodf(ang, 360.0f);
        if (QUARTERS && (r == 90.0f || r == -270.0f)) { c = 0.0f; s = 1.0f; return; }
        if (QUARTERS && (r == 180.0f || r == -180.0f)) { c = -1.0f; s = 0.0f; return; }
        if (QUARTERS && (r == 270.0f || r == -90.0f)) { c = 0.0f; s = -1.0f; return; }
        const float rad = r * 0.017453292519943295f;
        c = cosf(rad);
        s = sinf(rad);
    }
}
