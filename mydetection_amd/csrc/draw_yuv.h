// RGB -> Y'CbCr of a colour, as the kernels that paint into 4:2:0 planes take it (draw.hip, redact.hip; include/mydet.h has the
// formula and the table, ops.rgb_to_yuv is its host form).  The only copy of the table.
#pragma once
#include "pixel_math.h"

// RGB -> Y'CbCr rows, 8 fraction bits: [matrix: 0 = BT.601, 1 = BT.709][range: 0 = limited, 1 = full]
struct DrawYuvK { int y[3], u[3], v[3], yoff; };
constexpr DrawYuvK DRAW_YUV[2][2] = {
    {{{66, 129, 25}, {-38, -74, 112}, {112, -94, -18}, 16}, {{77, 150, 29}, {-43, -85, 128}, {128, -107, -21}, 0}},
    {{{47, 157, 16}, {-26, -86, 112}, {112, -102, -10}, 16}, {{54, 183, 18}, {-29, -99, 128}, {128, -116, -12}, 0}}};

// r | g << 8 | b << 16  ->  y | u << 8 | v << 16
__host__ __device__ __forceinline__ uint32_t draw_yuv_of(const DrawYuvK &k, uint32_t rgb) {
    const int r = px_chan(rgb, 0), g = px_chan(rgb, 1), b = px_chan(rgb, 2);
    const int y = ((k.y[0] * r + k.y[1] * g + k.y[2] * b + 128) >> 8) + k.yoff;
    const int u = ((k.u[0] * r + k.u[1] * g + k.u[2] * b + 128) >> 8) + 128;
    const int v = ((k.v[0] * r + k.v[1] * g + k.v[2] * b + 128) >> 8) + 128;
    return px_pack(px_clamp(y, 0, 255), px_clamp(u, 0, 255), px_clamp(v, 0, 255));
}
