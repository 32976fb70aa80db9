// IoU of two rotated rectangles as the exact area of their intersection, in float32 and in registers only.
//
// A rectangle is its centre, its two half-extent vectors and its area, in the vertex convention of the reference's
// xywha2vertex (utils/bbox_ops.py:137-172; angle clockwise in image coordinates):
//   hori = (w/2 cos a, w/2 sin a),  verti = (h/2 sin a, -h/2 cos a),  corners = centre +- verti +- hori,  area = w h.
// The reference rasterises these corners (iou_rle, utils/bbox_ops.py:52-100); here the area is exact -- see include/mydet.h.
//
// Method: box j's corners are expressed in box i's own (unnormalised) frame, x = (p - ci) . hori_i, y = (p - ci) . verti_i,
// in which box i is the axis-aligned rectangle |x| <= |hori_i|^2, |y| <= |verti_i|^2 and every area is the true one times
// area_i / 4.  Working from ci keeps the cancellation at the size of the boxes, not of the image coordinates.  The quad is
// then clipped against the four sides in turn (Sutherland-Hodgman).  Clipping moves every vertex continuously with the
// input, so coincident and parallel edges (duplicates are the common case in NMS) cost round-off only -- no edge is counted
// twice or dropped -- PROVIDED no vertex is ever dropped.  A generic pair needs 5, 6, 7, 8 slots after the four stages, but a
// corner of j that lies on a side of i within round-off may be classified outside while both its neighbours are inside and
// is then replaced by two crossing points.  Such a cluster of two points reaches the second side through that corner as two
// vertices, so a side whose two corners both coincide with corners of j sees up to four near-boundary vertices, i.e. two
// separate outside runs, each turning m >= 1 vertices into 2: the list grows by at most 1 at the first side (its corners are
// single vertices and adjacent) and by at most 2 at each later one.  The stages therefore hold 5, 7, 9 and 11 vertices;
// the extra ones are (near-)duplicates and add nothing to the shoelace sum.  Between two sides the polygon is turned by
// 90 degrees, so every stage clips against "x <= bound".  The vertex lists live in fixed slots: every index below is a compile-time constant
// after unrolling and an append is a chain of selects, so nothing is indexed dynamically and nothing goes to scratch.
#pragma once

namespace rotiou {

struct Box {
    float cx, cy;       // centre
    float hx, hy;       // hori
    float vx, vy;       // verti
    float area;         // w * h
};

// (cx, cy, w, h, degrees) -> Box; radians = deg * pi / 180 in float32, taken on the remainder of deg modulo 90
__device__ __forceinline__ Box make_box(float cx, float cy, float w, float h, float deg) {
    // deg = r + 90 k with |r| <= 45, exact in float32; the quarter turns are then sign changes and swaps.  The same
    // rectangle written with w and h swapped at +-90 k degrees gets bit-identical half-extent vectors this way, and the
    // radians are rounded at 0.8 instead of at 3 or 6 (a thin box turns its long side by L/2 per radian of error).
    const float k = rintf(deg / 90.0f);
    const float rad = (deg - 90.0f * k) * 3.14159265358979323846f / 180.0f;
    const float sr = sinf(rad), cr = cosf(rad);
    const int quad = (int)k & 3;
    const float s = quad == 0 ? sr : quad == 1 ? cr : quad == 2 ? -sr : -cr;
    const float c = quad == 0 ? cr : quad == 1 ? -sr : quad == 2 ? -cr : sr;
    const float hw = w / 2.0f, hh = h / 2.0f;
    Box b;
    b.cx = cx; b.cy = cy;
    b.hx = hw * c; b.hy = hw * s;
    b.vx = hh * s; b.vy = -hh * c;
    b.area = w * h;
    return b;
}

// One Sutherland-Hodgman stage: the first n (<= NIN) vertices of p, clipped to x <= bound, into the NOUT slots of q;
// returns the vertex count.  NOUT is chosen by the argument above so that no vertex is lost; the final min() only keeps the
// count inside the slots for inputs that are not rectangles at all (NaN, infinities).
template <int NIN, int NOUT>
__device__ __forceinline__ int clip_x_le(const float (&px)[NIN], const float (&py)[NIN], int n, float bound,
                                         float (&qx)[NOUT], float (&qy)[NOUT]) {
    float d[NIN];
#pragma unroll
    for (int k = 0; k < NIN; ++k) d[k] = bound - px[k];            // >= 0: inside
#pragma unroll
    for (int s = 0; s < NOUT; ++s) { qx[s] = 0.0f; qy[s] = 0.0f; }
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < NIN; ++k) {
        const bool live = k < n;
        // the vertex after k: the list closes at n
        const int k1 = k + 1 < NIN ? k + 1 : 0;
        const bool wrap = k + 1 >= n;
        const float ny = wrap ? py[0] : py[k1];
        const float nd = wrap ? d[0] : d[k1];
        const bool in_a = d[k] >= 0.0f, in_b = nd >= 0.0f;
        const bool keep = live && in_a;
#pragma unroll
        for (int s = 0; s <= (2 * k < NOUT - 1 ? 2 * k : NOUT - 1); ++s)
            if (keep && cnt == s) { qx[s] = px[k]; qy[s] = py[k]; }
        cnt += keep ? 1 : 0;
        const bool cross = live && (in_a != in_b);
        // crossing point of the edge with x = bound (d[k] and nd have opposite signs there, so 0 <= t <= 1)
        const float t = d[k] * __builtin_amdgcn_rcpf(d[k] - nd);
        const float iy = py[k] + t * (ny - py[k]);
#pragma unroll
        for (int s = 0; s <= (2 * k + 1 < NOUT - 1 ? 2 * k + 1 : NOUT - 1); ++s)
            if (cross && cnt == s) { qx[s] = bound; qy[s] = iy; }
        cnt += cross ? 1 : 0;
    }
    return cnt < NOUT ? cnt : NOUT;
}

// (x, y) -> (y, -x): the side "y <= b" becomes "x <= b"
template <int N>
__device__ __forceinline__ void turn(const float (&qx)[N], const float (&qy)[N], float (&px)[N], float (&py)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) { px[k] = qy[k]; py[k] = -qx[k]; }
}

// IoU of boxes i and j.  Exactly 0 when they do not intersect, when fewer than 3 vertices are left or when either area
// is 0; NaN only as 0 / 0, when both areas are 0 (a NaN compares false, i.e. "not suppressed").  One division.
__device__ __forceinline__ float rot_iou(const Box &bi, const Box &bj) {
    const float dx = bj.cx - bi.cx, dy = bj.cy - bi.cy;
    // corners of j from i's centre: tl, tr, br, bl = centre + verti - hori, + verti + hori, - verti + hori, - verti - hori
    const float ax[4] = {dx + bj.vx - bj.hx, dx + bj.vx + bj.hx, dx - bj.vx + bj.hx, dx - bj.vx - bj.hx};
    const float ay[4] = {dy + bj.vy - bj.hy, dy + bj.vy + bj.hy, dy - bj.vy + bj.hy, dy - bj.vy - bj.hy};
    const float bx = bi.hx * bi.hx + bi.hy * bi.hy, by = bi.vx * bi.vx + bi.vy * bi.vy;
    float p4x[4], p4y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p4x[k] = ax[k] * bi.hx + ay[k] * bi.hy;
        p4y[k] = ax[k] * bi.vx + ay[k] * bi.vy;
    }
    const float sum_area = bi.area + bj.area;
    float q = 0.0f;                                                // 4 x the clipped area in i's frame = area_i x the true one
    // j's bounding box in i's frame misses i: nothing to clip (most pairs of real detections)
    const float xlo = fminf(fminf(p4x[0], p4x[1]), fminf(p4x[2], p4x[3])), xhi = fmaxf(fmaxf(p4x[0], p4x[1]), fmaxf(p4x[2], p4x[3]));
    const float ylo = fminf(fminf(p4y[0], p4y[1]), fminf(p4y[2], p4y[3])), yhi = fmaxf(fmaxf(p4y[0], p4y[1]), fmaxf(p4y[2], p4y[3]));
    // (a box of zero area has no interior: the doubled edge would otherwise leave a round-off sliver instead of 0)
    if (xlo < bx && xhi > -bx && ylo < by && yhi > -by && bi.area != 0.0f && bj.area != 0.0f) {
        constexpr int NV = 11;
        float q5x[5], q5y[5], p5x[5], p5y[5];
        int n = clip_x_le<4, 5>(p4x, p4y, 4, bx, q5x, q5y);        //  x <= bx
        turn<5>(q5x, q5y, p5x, p5y);
        float q7x[7], q7y[7], p7x[7], p7y[7];
        n = clip_x_le<5, 7>(p5x, p5y, n, by, q7x, q7y);            //  y <= by
        turn<7>(q7x, q7y, p7x, p7y);
        float q9x[9], q9y[9], p9x[9], p9y[9];
        n = clip_x_le<7, 9>(p7x, p7y, n, bx, q9x, q9y);            // -x <= bx
        turn<9>(q9x, q9y, p9x, p9y);
        float q8x[NV], q8y[NV];
        n = clip_x_le<9, NV>(p9x, p9y, n, by, q8x, q8y);           // -y <= by
        // shoelace sum over the n vertices (twice the signed area; the orientation depends on the frame)
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int k1 = k + 1 < NV ? k + 1 : 0;
            const bool wrap = k + 1 >= n;
            const float nx = wrap ? q8x[0] : q8x[k1], ny = wrap ? q8y[0] : q8y[k1];
            const float term = q8x[k] * ny - nx * q8y[k];
            sum += k < n ? term : 0.0f;
        }
        q = n >= 3 ? 2.0f * fabsf(sum) : 0.0f;
    }
    // inter = q / area_i;  IoU = inter / (area_i + area_j - inter) = q / (area_i (area_i + area_j) - q)
    const bool hit = q > 0.0f;
    const float num = hit ? q : 0.0f;
    const float den = hit ? bi.area * sum_area - q : sum_area;
    return num / den;
}

}  // namespace rotiou
