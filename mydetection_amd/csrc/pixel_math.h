// The 8-bit pixel arithmetic every image kernel shares (boxops.hip, frames.hip, yuv420.hip), defined once so that "the bits
// of mydet_resize_bilinear_u8 + mydet_preprocess_u8_f32" is one piece of code and not a promise between copies.
#pragma once
#include "common.h"

__host__ __device__ __forceinline__ int px_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A pixel as one dword: r | g << 8 | b << 16
__host__ __device__ __forceinline__ uint32_t px_pack(int r, int g, int b) { return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16); }
__host__ __device__ __forceinline__ int px_chan(uint32_t v, int c) { return (int)((v >> (8 * c)) & 255u); }

// One output of Pillow's 8-bit fixed-point filter, three channels: clip8((2^21 + sum in * w) >> 22), w 22-bit integers
struct PxFilter {
    int a[3] = {1 << 21, 1 << 21, 1 << 21};
    __device__ __forceinline__ void add(int r, int g, int b, int w) { a[0] += r * w; a[1] += g * w; a[2] += b * w; }
    __device__ __forceinline__ void add(uint32_t packed, int w) { add(px_chan(packed, 0), px_chan(packed, 1), px_chan(packed, 2), w); }
    __device__ __forceinline__ int clip8(int c) const { return px_clamp(a[c] >> 22, 0, 255); }
    __device__ __forceinline__ uint32_t pixel() const { return px_pack(clip8(0), clip8(1), clip8(2)); }
};

// uint8 channel value -> network input: x / 255, then with norm (x - mean) / std, in that operation order
__device__ __forceinline__ float px_to_float(int v, int norm, float mean, float sd) {
    float f = (float)v / 255.0f;
    if (norm) f = (f - mean) / sd;
    return f;
}
