// What every kernel that READS 4:2:0 frames shares (yuv420.hip, crop.hip): the one coefficient table, the source descriptor and
// its checks (include/mydet.h: mydet_yuv420_src), the 10-bit rule, and the fetches -- four neighbouring pixels (yuv_quad) or one
// (yuv_pixel) as packed RGB dwords.  Defined once so that "the bits of mydet_yuv420_to_rgb_u8" is one piece of code.
#pragma once
#include "pixel_math.h"

namespace {

// cy, crv, cgu, cgv, cbu, luma offset: [matrix: 0 = BT.601, 1 = BT.709][range: 0 = limited, 1 = full]
struct YuvCoef { int cy, crv, cgu, cgv, cbu, yoff; };
constexpr YuvCoef YUV_COEF[2][2] = {{{298, 409, 100, 208, 516, 16}, {256, 359, 88, 183, 454, 0}},
                                    {{298, 459, 55, 136, 541, 16}, {256, 403, 48, 120, 475, 0}}};

// One source of the 4:2:0 family (include/mydet.h: mydet_yuv420_src).  p[2] is null for the semi-planar layouts.
struct YuvSrc {
    const unsigned char *p[3];                 // Y; interleaved chroma or U; V
    int64_t img[3], row[3];                    // bytes between frames / rows of each plane
    int H, W;
    int wide;                                  // every plane allows the wide reads of its layout (yuv_quad)
    uint32_t pair_sel;                         // v_perm_b32 selector that puts the two chroma pairs of a quad into (U, V) order
    YuvCoef k;
};

__device__ __forceinline__ uint32_t yuv_rgb(const YuvCoef &k, int Y, int U, int V) {
    const int c = k.cy * (Y - k.yoff) + 128, d = U - 128, e = V - 128;
    return px_pack(px_clamp((c + k.crv * e) >> 8, 0, 255), px_clamp((c - k.cgu * d - k.cgv * e) >> 8, 0, 255),
                   px_clamp((c + k.cbu * d) >> 8, 0, 255));
}

// A stored sample as 8 bits.  BPS = 2: little-endian words, the ten bits are the high ones of a semi-planar layout (P010) and
// the low ones of a planar layout (I010); the other six are ignored.  s8 = min(255, (v10 + 2) >> 2).
template <int BPS, bool PLANAR>
__device__ __forceinline__ uint32_t yuv_s8(uint32_t w) {
    if constexpr (BPS == 1) {
        return w;
    } else {
        const uint32_t v10 = PLANAR ? (w & 1023u) : ((w & 0xffffu) >> 6);
        return min(255u, (v10 + 2u) >> 2);
    }
}

// N (4 or 2) neighbouring samples from p as packed bytes, sample k in bits [8k, 8k + 8); a sample at or beyond `valid` is zero
// and is not read.  One N * BPS byte read when `wide` (p is then a multiple of N * BPS) and all N are valid, else by samples.
template <int BPS, bool PLANAR, int N>
__device__ __forceinline__ uint32_t yuv_samples(const unsigned char *p, int valid, int wide) {
    uint32_t v = 0;
    if (wide && valid >= N) {
        if constexpr (BPS == 1 && N == 4) {
            v = *reinterpret_cast<const uint32_t *>(p);
        } else if constexpr (BPS == 1) {
            v = *reinterpret_cast<const uint16_t *>(p);
        } else if constexpr (N == 4) {
            const uint2 t = *reinterpret_cast<const uint2 *>(p);
            v = yuv_s8<BPS, PLANAR>(t.x & 0xffffu) | (yuv_s8<BPS, PLANAR>(t.x >> 16) << 8) |
                (yuv_s8<BPS, PLANAR>(t.y & 0xffffu) << 16) | (yuv_s8<BPS, PLANAR>(t.y >> 16) << 24);
        } else {
            const uint32_t t = *reinterpret_cast<const uint32_t *>(p);
            v = yuv_s8<BPS, PLANAR>(t & 0xffffu) | (yuv_s8<BPS, PLANAR>(t >> 16) << 8);
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < valid) {
                uint32_t t;
                if constexpr (BPS == 1) t = p[k];
                else t = reinterpret_cast<const uint16_t *>(p)[k];
                v |= yuv_s8<BPS, PLANAR>(t) << (8 * k);
            }
    }
    return v;
}

// Four neighbouring pixels of source row `row` of frame `b` from column c (c % 4 == 0) as packed dwords; a pixel at or beyond W
// is zero.  The only code that depends on the layout.  A Y row holds W samples; an interleaved chroma row 2 * ceil(W / 2), the
// pair of pixel c + k starting at sample c + (k & ~1); a planar chroma row ceil(W / 2), the sample of pixel c + k at (c + k) >> 1.
// Wide reads per quad, taken when the address, pitch and frame stride of every plane are multiples of the bytes read there:
//   NV12 / NV21  Y 4 bytes, chroma 4 bytes at byte c                      every plane: 4
//   I420         Y 4 bytes, U and V 2 bytes at byte c / 2                 Y: 4, U and V: 2
//   P010         Y 8 bytes, chroma 8 bytes at byte 2c                     every plane: 8
//   I010         Y 8 bytes, U and V 4 bytes at byte c                     Y: 8, U and V: 4
// Otherwise, and in a row's partial last quad, the samples are read one by one (the 16-bit layouts need even addresses: the
// entry points refuse anything else).
template <int BPS, bool PLANAR>
__device__ __forceinline__ uint4 yuv_quad(const YuvSrc &s, int b, int row, int c) {
    const unsigned char *yr = s.p[0] + (int64_t)b * s.img[0] + (int64_t)row * s.row[0] + c * BPS;
    const unsigned char *ur = s.p[1] + (int64_t)b * s.img[1] + (int64_t)(row >> 1) * s.row[1];
    const int ny = s.W - c;                                             // valid samples from c on
    const uint32_t yw = yuv_samples<BPS, PLANAR, 4>(yr, ny, s.wide);
    uint32_t cw;                                                        // the two pairs: bytes (first, second) x 2
    if constexpr (PLANAR) {
        const unsigned char *vr = s.p[2] + (int64_t)b * s.img[2] + (int64_t)(row >> 1) * s.row[2];
        const int nc = ((s.W + 1) >> 1) - (c >> 1);
        const uint32_t u = yuv_samples<BPS, PLANAR, 2>(ur + (c >> 1) * BPS, nc, s.wide);
        const uint32_t v = yuv_samples<BPS, PLANAR, 2>(vr + (c >> 1) * BPS, nc, s.wide);
        cw = (u & 255u) | ((v & 255u) << 8) | ((u >> 8) << 16) | ((v >> 8) << 24);
    } else {
        cw = yuv_samples<BPS, PLANAR, 4>(ur + c * BPS, ((s.W + 1) & ~1) - c, s.wide);
        cw = __builtin_amdgcn_perm(cw, cw, s.pair_sel);                 // NV21: (V, U) -> (U, V); the identity otherwise
    }
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t pair = cw >> (16 * (k >> 1));
        v[k] = k < ny ? yuv_rgb(s.k, (yw >> (8 * k)) & 255u, pair & 255u, (pair >> 8) & 255u) : 0u;
    }
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// One pixel (row, x) of frame `b`, inside the frame: the dword yuv_quad gives for it, from single-sample reads (the chroma pair
// of an interleaved layout is one 2-sample read, wide when the plane allows).
template <int BPS, bool PLANAR>
__device__ __forceinline__ uint32_t yuv_pixel(const YuvSrc &s, int b, int row, int x) {
    const unsigned char *yr = s.p[0] + (int64_t)b * s.img[0] + (int64_t)row * s.row[0] + (int64_t)x * BPS;
    const unsigned char *ur = s.p[1] + (int64_t)b * s.img[1] + (int64_t)(row >> 1) * s.row[1];
    const uint32_t yv = yuv_samples<BPS, PLANAR, 2>(yr, 1, 0);
    uint32_t u, v;
    if constexpr (PLANAR) {
        const unsigned char *vr = s.p[2] + (int64_t)b * s.img[2] + (int64_t)(row >> 1) * s.row[2];
        u = yuv_samples<BPS, PLANAR, 2>(ur + (int64_t)(x >> 1) * BPS, 1, 0);
        v = yuv_samples<BPS, PLANAR, 2>(vr + (int64_t)(x >> 1) * BPS, 1, 0);
    } else {
        uint32_t pair = yuv_samples<BPS, PLANAR, 2>(ur + (int64_t)(x >> 1) * 2 * BPS, 2, s.wide);
        pair = __builtin_amdgcn_perm(pair, pair, s.pair_sel);           // NV21: (V, U) -> (U, V); the identity otherwise
        u = pair & 255u;
        v = (pair >> 8) & 255u;
    }
    return yuv_rgb(s.k, (int)yv, (int)u, (int)v);
}

// bytes per sample and plane count of a layout selector; false for an unknown one
inline bool yuv_layout(int layout, int &bps, bool &planar, bool &v_first) {
    switch (layout) {
    case MYDET_YUV420_NV12: bps = 1; planar = false; v_first = false; return true;
    case MYDET_YUV420_NV21: bps = 1; planar = false; v_first = true; return true;
    case MYDET_YUV420_I420: bps = 1; planar = true; v_first = false; return true;
    case MYDET_YUV420_P010: bps = 2; planar = false; v_first = false; return true;
    case MYDET_YUV420_I010: bps = 2; planar = true; v_first = false; return true;
    }
    return false;
}

// The checks every entry point shares; fills `s`, `bps` and `planar`
int yuv_source(YuvSrc &s, int &bps, bool &planar, const mydet_yuv420_src *src, int B, int H, int W) {
    bool v_first;
    if (!src || !src->plane[0] || !src->plane[1] || B <= 0 || H <= 0 || W <= 0) return MYDET_E_BADARG;
    if (!yuv_layout(src->layout, bps, planar, v_first)) return MYDET_E_BADARG;
    if (src->matrix < 0 || src->matrix > 1 || src->full_range < 0 || src->full_range > 1) return MYDET_E_BADARG;
    if ((src->plane[2] != nullptr) != planar) return MYDET_E_BADARG;
    const int64_t cw = ((int64_t)W + 1) / 2;
    const int64_t need[3] = {(int64_t)W * bps, (planar ? cw : 2 * cw) * bps, cw * bps};
    const int wide[3] = {4 * bps, planar ? 2 * bps : 4 * bps, 2 * bps};           // bytes of a plane's wide read (yuv_quad)
    s.wide = 1;
    for (int i = 0; i < (planar ? 3 : 2); ++i) {
        if (src->row_bytes[i] < need[i] || src->img_bytes[i] < 0) return MYDET_E_BADARG;
        const uintptr_t bits = (uintptr_t)src->plane[i] | (uintptr_t)src->row_bytes[i] | (uintptr_t)src->img_bytes[i];
        if (bits & (uintptr_t)(bps - 1)) return MYDET_E_BADARG;                   // a 16-bit sample at an odd address
        if (bits & (uintptr_t)(wide[i] - 1)) s.wide = 0;
    }
    for (int i = 0; i < 3; ++i) {
        const bool used = i < 2 || planar;
        s.p[i] = used ? static_cast<const unsigned char *>(src->plane[i]) : nullptr;
        s.img[i] = used ? src->img_bytes[i] : 0;
        s.row[i] = used ? src->row_bytes[i] : 0;
    }
    s.H = H; s.W = W;
    s.pair_sel = v_first ? 0x02030001u : 0x03020100u;
    s.k = YUV_COEF[src->matrix][src->full_range];
    return 0;
}

// CALL(BPS, PLANAR) for the layout's instance
#define YUV_DISPATCH(bps, planar, CALL)                    \
    do {                                                   \
        if ((bps) == 1 && !(planar)) { CALL(1, false); }   \
        else if ((bps) == 1) { CALL(1, true); }            \
        else if (!(planar)) { CALL(2, false); }            \
        else { CALL(2, true); }                            \
    } while (0)

}  // namespace
