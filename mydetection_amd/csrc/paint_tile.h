// What the kernels that paint a list of boxes IN PLACE into frames share (draw.hip, redact.hip; crop.hip takes the list check):
// the planes of a target, a lane's pixel group with its loads and its one store, the reader of a list row, the compaction of
// a chunk's hits into LDS and the list checks.  Defined once so that an alignment or odd-edge rule is one piece of code.
//
// Geometry.  One workgroup of 256 lanes per image tile.  FMT 0 = RGB: a tile of 64 x 16 pixels, a lane owns 4 neighbouring
// pixels of a row (12 bytes).  FMT 1 = interleaved chroma (NV12 / NV21), 2 = planar chroma (I420): a tile of 128 x 16, a lane
// owns two neighbouring chroma quads -- 4 x 2 luma pixels (rows i0, i0 + 1, i0 even; columns j0 .. j0 + 3) and their 2 chroma
// samples --, so luma and chroma come from one evaluation.  A group is read and written with dwords (planar chroma: 16 bits)
// when it lies whole inside the frame and the address, pitch and frame stride of the plane allow (`wide`), byte by byte
// otherwise.  A mask over the group has bit 4 * r + k for pixel (i0 + r, j0 + k).
#pragma once
#include "box_rot.h"
#include "pixel_math.h"

namespace {

constexpr int PT_THREADS = 256;

// ------------------------------------------------------------------------------------------------------------- planes
struct PaintPlanes {
    unsigned char *p[3];                     // RGB: p[0] = the frames.  4:2:0: Y; interleaved chroma or U; V
    int64_t img[3], row[3];                  // bytes between frames / rows
    int wide[3];                             // the plane takes the dword (planar chroma: 16-bit) accesses
    int v_first;                             // NV21: the pair is (V, U)
};

// The planes of RGB frames of width W; the entry point's error code
inline int paint_planes_rgb(PaintPlanes &t, unsigned char *dst, int64_t img_bytes, int64_t row_bytes, int W) {
    if (!dst || row_bytes < (int64_t)W * 3 || img_bytes < 0) return MYDET_E_BADARG;
    t.p[0] = dst; t.img[0] = img_bytes; t.row[0] = row_bytes;
    t.wide[0] = (((uintptr_t)dst | (uintptr_t)img_bytes | (uintptr_t)row_bytes) & 3) == 0;
    return 0;
}

// The planes of an 8-bit 4:2:0 source (include/mydet.h: mydet_yuv420_src) of width W; the entry point's error code
inline int paint_planes_yuv420(PaintPlanes &t, const mydet_yuv420_src *planes, int W) {
    if (!planes || !planes->plane[0] || !planes->plane[1]) return MYDET_E_BADARG;
    if (planes->layout != MYDET_YUV420_NV12 && planes->layout != MYDET_YUV420_NV21 && planes->layout != MYDET_YUV420_I420)
        return MYDET_E_BADARG;                                            // unknown, or a 10-bit layout
    if (planes->matrix < 0 || planes->matrix > 1 || planes->full_range < 0 || planes->full_range > 1) return MYDET_E_BADARG;
    const bool planar = planes->layout == MYDET_YUV420_I420;
    if ((planes->plane[2] != nullptr) != planar) return MYDET_E_BADARG;
    const int64_t cw = ((int64_t)W + 1) / 2;
    const int64_t need[3] = {(int64_t)W, planar ? cw : 2 * cw, cw};
    const int wide[3] = {4, planar ? 2 : 4, 2};
    for (int i = 0; i < (planar ? 3 : 2); ++i) {
        if (planes->row_bytes[i] < need[i] || planes->img_bytes[i] < 0) return MYDET_E_BADARG;
        const uintptr_t bits = (uintptr_t)planes->plane[i] | (uintptr_t)planes->row_bytes[i] | (uintptr_t)planes->img_bytes[i];
        t.p[i] = static_cast<unsigned char *>(const_cast<void *>(planes->plane[i]));
        t.img[i] = planes->img_bytes[i]; t.row[i] = planes->row_bytes[i];
        t.wide[i] = (bits & (uintptr_t)(wide[i] - 1)) == 0;
    }
    t.v_first = planes->layout == MYDET_YUV420_NV21;
    return 0;
}

// -------------------------------------------------------------------------------------------------------- pixel group
// The pixels one lane owns (see the top): nr x nc of them lie inside the H x W frame, with nq chroma samples
struct PaintGroup {
    int nr, nc, nq;
    unsigned char *yo, *uo, *vo;             // RGB: yo.  Interleaved chroma: uo = the pair of the first quad
    bool ywords, cwords;                     // the luma / RGB rows, the chroma samples take the wide accesses
};

template <int FMT>
__device__ __forceinline__ PaintGroup paint_group(const PaintPlanes &t, int H, int W, int b, int i0, int j0) {
    PaintGroup u;
    u.nr = px_clamp(H - i0, 0, FMT == 0 ? 1 : 2);
    u.nc = u.nr ? px_clamp(W - j0, 0, 4) : 0;
    u.nq = (u.nc + 1) >> 1;
    u.uo = u.vo = nullptr;
    u.cwords = false;
    if (FMT == 0) {
        u.yo = t.p[0] + (int64_t)b * t.img[0] + (int64_t)i0 * t.row[0] + (int64_t)j0 * 3;
    } else {
        u.yo = t.p[0] + (int64_t)b * t.img[0] + (int64_t)i0 * t.row[0] + j0;
        const int cw = (W + 1) >> 1;
        if (FMT == 2) {
            u.uo = t.p[1] + (int64_t)b * t.img[1] + (int64_t)(i0 >> 1) * t.row[1] + (j0 >> 1);
            u.vo = t.p[2] + (int64_t)b * t.img[2] + (int64_t)(i0 >> 1) * t.row[2] + (j0 >> 1);
        } else {
            u.uo = t.p[1] + (int64_t)b * t.img[1] + (int64_t)(i0 >> 1) * t.row[1] + j0;
        }
        u.cwords = u.nq == 2 && (j0 >> 1) + 2 <= cw && (FMT == 2 ? (t.wide[1] && t.wide[2]) : t.wide[1]);
    }
    u.ywords = t.wide[0] && u.nc == 4;
    return u;
}

// The mask of the group's pixels inside the frame, and of a mask's chroma quads (bit q: a pixel of quad q is in it)
__device__ __forceinline__ unsigned paint_inside(const PaintGroup &u) {
    const unsigned rowbits = (1u << u.nc) - 1u;
    return u.nr == 2 ? (rowbits | (rowbits << 4)) : (u.nr ? rowbits : 0u);
}
__device__ __forceinline__ unsigned paint_quads(unsigned mask) { return ((mask & 0x33u) ? 1u : 0u) | ((mask & 0xccu) ? 2u : 0u); }

// The group's pixels inside the frame: RGB px[k] = r | g << 8 | b << 16.  The others are left as they are.
__device__ __forceinline__ void paint_load(const PaintGroup &u, uint32_t px[4]) {
    if (u.ywords) {
        const uint32_t *o4 = reinterpret_cast<const uint32_t *>(u.yo);
        const uint32_t w0 = o4[0], w1 = o4[1], w2 = o4[2];
        px[0] = w0 & 0xffffffu; px[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8); px[2] = (w1 >> 16) | ((w2 & 0xffu) << 16); px[3] = w2 >> 8;
    } else {
        for (int k = 0; k < u.nc; ++k) px[k] = px_pack(u.yo[3 * k], u.yo[3 * k + 1], u.yo[3 * k + 2]);
    }
}

// 4:2:0: Y[r][k] and the chroma samples U[q], V[q] of the quads
template <int FMT>
__device__ __forceinline__ void paint_load(const PaintPlanes &t, const PaintGroup &u, int Y[2][4], int U[2], int V[2]) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r >= u.nr) continue;
        const unsigned char *yr = u.yo + (int64_t)r * t.row[0];
        if (u.ywords) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(yr);
#pragma unroll
            for (int k = 0; k < 4; ++k) Y[r][k] = (int)((w >> (8 * k)) & 255u);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < u.nc) Y[r][k] = yr[k];
        }
    }
    if (FMT == 2) {
        if (u.cwords) {
            const uint32_t a = *reinterpret_cast<const uint16_t *>(u.uo), v = *reinterpret_cast<const uint16_t *>(u.vo);
            U[0] = a & 255u; U[1] = a >> 8; V[0] = v & 255u; V[1] = v >> 8;
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q) if (q < u.nq) { U[q] = u.uo[q]; V[q] = u.vo[q]; }
        }
    } else {
        const int su = t.v_first ? 1 : 0;                                // byte of U inside an interleaved pair
        if (u.cwords) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(u.uo);
            U[0] = (w >> (8 * su)) & 255u; V[0] = (w >> (8 * (1 - su))) & 255u;
            U[1] = (w >> (16 + 8 * su)) & 255u; V[1] = (w >> (16 + 8 * (1 - su))) & 255u;
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q) if (q < u.nq) { U[q] = u.uo[2 * q + su]; V[q] = u.uo[2 * q + 1 - su]; }
        }
    }
}

// The sums of the group's two halves (columns j0, j0 + 1 and j0 + 2, j0 + 3) over the pixels inside the frame: s[h] = (R, G, B)
// or (Y, U, V) -- one chroma sample per half --; have[h]: the half has a pixel
template <int FMT>
__device__ __forceinline__ void paint_load_halves(const PaintPlanes &t, const PaintGroup &u, int s[2][3], bool have[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) { s[h][0] = s[h][1] = s[h][2] = 0; have[h] = u.nc > 2 * h; }
    if (!u.nc) return;
    if constexpr (FMT == 0) {
        uint32_t px[4] = {0, 0, 0, 0};
        paint_load(u, px);
#pragma unroll
        for (int k = 0; k < 4; ++k)                                       // pixels past nc are 0
#pragma unroll
            for (int c = 0; c < 3; ++c) s[k >> 1][c] += px_chan(px[k], c);
    } else {
        int Y[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, U[2] = {0, 0}, V[2] = {0, 0};
        paint_load<FMT>(t, u, Y, U, V);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k >> 1][0] += Y[r][k];
#pragma unroll
        for (int q = 0; q < 2; ++q) { s[q][1] = U[q]; s[q][2] = V[q]; }
    }
}

// Stores the pixels of `cov` (a mask inside paint_inside): wide stores where a whole row of the group is covered and the plane
// allows, the bytes of the covered pixels otherwise
__device__ __forceinline__ void paint_store(const PaintGroup &u, const uint32_t px[4], unsigned cov) {
    if (u.ywords && cov == 0xfu) {
        uint32_t *o4 = reinterpret_cast<uint32_t *>(u.yo);
        o4[0] = px[0] | (px[1] << 24);
        o4[1] = (px[1] >> 8) | (px[2] << 16);
        o4[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (cov & (1u << k)) {
                u.yo[3 * k] = (unsigned char)px[k]; u.yo[3 * k + 1] = (unsigned char)(px[k] >> 8); u.yo[3 * k + 2] = (unsigned char)(px[k] >> 16);
            }
    }
}

// 4:2:0: the luma pixels of `cov`, and chroma sample q iff bit q of `cq` is set
template <int FMT>
__device__ __forceinline__ void paint_store(const PaintPlanes &t, const PaintGroup &u, const int Y[2][4], const int U[2], const int V[2],
                                            unsigned cov, unsigned cq) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned m = (cov >> (4 * r)) & 15u;
        if (!m) continue;
        unsigned char *yr = u.yo + (int64_t)r * t.row[0];
        if (u.ywords && m == 15u) {
            *reinterpret_cast<uint32_t *>(yr) = (uint32_t)Y[r][0] | ((uint32_t)Y[r][1] << 8) | ((uint32_t)Y[r][2] << 16) | ((uint32_t)Y[r][3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (m & (1u << k)) yr[k] = (unsigned char)Y[r][k];
        }
    }
    if (FMT == 2) {
        if (u.cwords && cq == 3u) {
            *reinterpret_cast<uint16_t *>(u.uo) = (uint16_t)(U[0] | (U[1] << 8));
            *reinterpret_cast<uint16_t *>(u.vo) = (uint16_t)(V[0] | (V[1] << 8));
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q) if (cq & (1u << q)) { u.uo[q] = (unsigned char)U[q]; u.vo[q] = (unsigned char)V[q]; }
        }
    } else {
        const int su = t.v_first ? 1 : 0;
        if (u.cwords && cq == 3u) {
            const uint32_t p0 = (uint32_t)(su ? (V[0] | (U[0] << 8)) : (U[0] | (V[0] << 8)));
            const uint32_t p1 = (uint32_t)(su ? (V[1] | (U[1] << 8)) : (U[1] | (V[1] << 8)));
            *reinterpret_cast<uint32_t *>(u.uo) = p0 | (p1 << 16);
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q) if (cq & (1u << q)) { u.uo[2 * q + su] = (unsigned char)U[q]; u.uo[2 * q + 1 - su] = (unsigned char)V[q]; }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------- the list
// The rows of frame b: min(count, K), count NULL meaning K; zero or less: nothing to paint
__device__ __forceinline__ int paint_count(const mydet_draw_list &l, int b) {
    const int cnt = l.count ? l.count[(int64_t)b * l.count_stride] : l.K;
    return min(cnt, l.K);
}

struct PaintRow { float cx, cy, w, h, c, s; };                           // centre, sizes, cos, sin

// Row r of frame b: false when the rules skip it (a value that is not finite, w <= 0 or h <= 0), else its box and rotation.
// The redaction's reader.  draw_collect (draw.hip) keeps the same lines of its own: through this function draw_rgb_kernel
// measured 0.1 - 0.4 % above its parent in half of its cases, with its own lines in none (profiles/paint_tile.md).
__device__ __forceinline__ bool paint_row(const mydet_draw_list &l, int b, int r, PaintRow &o) {
    const float *bx = l.box + (int64_t)b * l.box_frame_stride + (int64_t)r * l.box_row_stride;
    o.cx = bx[0]; o.cy = bx[1]; o.w = bx[2]; o.h = bx[3];
    const float ang = l.angle ? l.angle[(int64_t)b * l.angle_frame_stride + (int64_t)r * l.angle_row_stride] : 0.0f;
    o.c = 1.0f; o.s = 0.0f;
    if (!(isfinite(o.cx) && isfinite(o.cy) && isfinite(o.w) && isfinite(o.h) && isfinite(ang) && o.w > 0.0f && o.h > 0.0f)) return false;
    box_rotation<false>(ang, o.c, o.s);
    return true;
}

// (ex, ey): the half extents of the bounding box of a rotated rectangle of half sizes (ra, rb), one pixel wider (the margin for
// float32 rounding); paint_reaches: that bounding box around (cx, cy) against [x0, x1] x [y0, y1]
__device__ __forceinline__ void paint_extents(float c, float s, float ra, float rb, float &ex, float &ey) {
    ex = fabsf(c) * ra + fabsf(s) * rb + 1.0f;
    ey = fabsf(s) * ra + fabsf(c) * rb + 1.0f;
}
__device__ __forceinline__ bool paint_reaches(float cx, float cy, float ex, float ey, float x0, float y0, float x1, float y1) {
    return !(cx - ex > x1 || cx + ex < x0 || cy - ey > y1 || cy + ey < y0);
}

// One chunk of PT_THREADS rows, one per lane, compacted in lane order: a lane with `hit` gets its slot from `write(slot)`, where
// it stores its own hit record; returns the number of hits.  Every lane of the workgroup calls it (two barriers inside: the
// records are visible on return).  wave_cnt: PT_THREADS / 64 ints of LDS.
template <typename Write>
__device__ __forceinline__ int paint_compact(bool hit, int *wave_cnt, Write write) {
    const int tid = threadIdx.x;
    const unsigned long long m = __ballot(hit);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) wave_cnt[wv] = __popcll(m);
    __syncthreads();
    int base = 0, total = 0;
    for (int k = 0; k < PT_THREADS / 64; ++k) {
        const int n = wave_cnt[k];
        if (k < wv) base += n;
        total += n;
    }
    if (hit) write(base + __popcll(m & ((1ull << lane) - 1ull)));
    __syncthreads();
    return total;
}

// The host-side check of a list: NULL list or box plane, K outside 1 .. MYDET_DRAW_MAX_BOXES, a negative stride of a plane the
// caller reads -- box, angle and count; with `keys` the score, cls and id planes too
inline int paint_list_check(const mydet_draw_list *l, bool keys) {
    if (!l || !l->box || l->K < 1 || l->K > MYDET_DRAW_MAX_BOXES) return MYDET_E_BADARG;
    const int64_t strides[] = {l->box_frame_stride, l->box_row_stride, l->angle_frame_stride, l->angle_row_stride, l->count_stride,
                               l->score_frame_stride, l->score_row_stride, l->cls_frame_stride, l->cls_row_stride, l->id_frame_stride,
                               l->id_row_stride};
    for (int k = 0; k < (keys ? 11 : 5); ++k)
        if (strides[k] < 0) return MYDET_E_BADARG;
    return 0;
}

}  // namespace
