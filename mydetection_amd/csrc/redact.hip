// Redaction: the boxes (or ellipses) of a list become a mosaic, a smooth blur or one colour, IN PLACE, in uint8 RGB frames or in
// the planes of the 8-bit 4:2:0 layouts (include/mydet.h: mydet_redact_boxes_rgb_u8, mydet_redact_boxes_yuv420_u8, where the
// rules are; DESIGN.md has them too).  Built with -ffp-contract=off: coverage is a float32 expression that must not be fused.
//
// A redacted pixel is a function of the ORIGINAL frame, and in `smooth` of cells that other workgroups repaint, so the entry
// point issues two kernels on the stream:
//   means  one workgroup of 256 lanes per block of whole cells, at least 64 x 16 pixels and a multiple of 4 pixels wide, so a
//          lane owns a pixel group of paint_tile.h and takes its loads.  A block that no padded box reaches (one cell further
//          in `smooth`) reads nothing.  The others sum their pixels per cell with integer LDS atomics into 16 copies of the
//          block's sums (lanes of a wave that hit one cell spread over them), add the copies up and write every cell's mean as
//          one dword r | g << 8 | b << 16 (y | u << 8 | v << 16: the chroma cells of c/2 samples lie on the luma cells) into the
//          workspace [B][nI][nJ].  Integer sums: any order gives the same bytes.  No global atomics, nothing to clear.
//   paint  the tiles, the hit compaction and the store of paint_tile.h; it reads the list and the workspace only and stores the
//          covered pixels.
// `solid` needs the second kernel alone.
#include "draw_yuv.h"
#include "paint_tile.h"

namespace {

constexpr int RD_THREADS = PT_THREADS;
constexpr int RD_COPIES = 16;                // copies of a block's cell sums in LDS
constexpr int RD_CELLS = 64;                 // cells of a means block at most (cell 4: 4 x 16)

struct RedactHit { float cx, cy, ra, rb, c, s; };                        // centre, padded half sizes, cos, sin

// n / d for 0 <= n < 2^24 as a multiplication: m = ceil(2^s / d), s = 24 + ceil(log2 d) (Granlund and Montgomery: exact).  The
// divisors (cell sizes, groups of a block row) are launch constants, and a 32-bit division costs a lane some 35 instructions.
struct RedactDiv { uint32_t m; int s; };
RedactDiv redact_div_of(int d) {
    int l = 0;
    while ((1 << l) < d) ++l;
    return {(uint32_t)(((1ull << (24 + l)) + (uint64_t)d - 1) / (uint64_t)d), 24 + l};
}
__device__ __forceinline__ int redact_div(int n, const RedactDiv &d) { return (int)(((uint64_t)(uint32_t)n * d.m) >> d.s); }

struct RedactArgs {
    mydet_draw_list l;
    mydet_redact_style s;
    int H, W, nI, nJ;                        // the view and its cell grid
    int GI, GJ;                              // cells of a means block
    RedactDiv by_cell[2], by_two[2], by_whole[2];   // / cc, / (2 cc), / (4 cc^2) for cc = cell [0] and cell / 2 [1] (the chroma grid)
    RedactDiv by_groups;                     // / (pixel groups of a means block's row)
    PaintPlanes t;
    uint32_t color;                          // solid: r | g << 8 | b << 16, or y | u << 8 | v << 16
    uint32_t *means;                         // [B][nI][nJ]
};

// Row r of frame b: false when the rules skip it or the class filter leaves it out; else its geometry and (ex, ey), the half
// extents of the padded shape's bounding box
__device__ __forceinline__ bool redact_row(const RedactArgs &p, int b, int r, RedactHit &o, float &ex, float &ey) {
    const mydet_draw_list &l = p.l;
    if (p.s.n_classes > 0) {
        const int64_t cls = l.cls[(int64_t)b * l.cls_frame_stride + (int64_t)r * l.cls_row_stride];
        bool in = false;
        for (int k = 0; k < p.s.n_classes; ++k) in = in || cls == (int64_t)p.s.classes[k];
        if (!in) return false;
    }
    PaintRow g;
    if (!paint_row(l, b, r, g)) return false;
    o.cx = g.cx; o.cy = g.cy; o.c = g.c; o.s = g.s;
    o.ra = (g.w * 0.5f) * p.s.pad; o.rb = (g.h * 0.5f) * p.s.pad;
    paint_extents(o.c, o.s, o.ra, o.rb, ex, ey);
    return true;
}

__device__ __forceinline__ bool redact_covers(const RedactHit &h, int shape, int i, int j) {
    const float dx = ((float)j + 0.5f) - h.cx, dy = ((float)i + 0.5f) - h.cy;
    const float a = fabsf(dx * h.c + dy * h.s), b = fabsf(dy * h.c - dx * h.s);
    if (shape == MYDET_REDACT_BOX) return a <= h.ra && b <= h.rb;
    const float u = a * h.rb, v = b * h.ra, w = h.ra * h.rb;
    return u * u + v * v <= w * w;
}

__device__ __forceinline__ int redact_mean(int S, int n) { return (2 * S + n) / (2 * n); }

template <int FMT>
__global__ __launch_bounds__(RD_THREADS) void redact_means_kernel(const RedactArgs p) {
    __shared__ int sums[RD_COPIES][RD_CELLS][3];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int c = p.s.cell;
    const int I0 = blockIdx.y * p.GI, J0 = blockIdx.x * p.GJ;
    const int y0 = I0 * c, x0 = J0 * c;
    const int cnt = paint_count(p.l, b);
    if (cnt <= 0) return;
    {                                                                     // does a padded box reach the block, or (smooth) its neighbours?
        const float d = p.s.mode == MYDET_REDACT_SMOOTH ? (float)c : 0.0f;
        const float bx0 = (float)x0 - d, by0 = (float)y0 - d, bx1 = (float)(x0 + p.GJ * c) + d, by1 = (float)(y0 + p.GI * c) + d;
        int hit = 0;
        for (int r = tid; r < cnt; r += RD_THREADS) {
            RedactHit h;
            float ex, ey;
            if (redact_row(p, b, r, h, ex, ey) && paint_reaches(h.cx, h.cy, ex, ey, bx0, by0, bx1, by1)) hit = 1;
        }
        if (!__syncthreads_or(hit)) return;
    }
    for (int e = tid; e < RD_COPIES * RD_CELLS * 3; e += RD_THREADS) (&sums[0][0][0])[e] = 0;
    __syncthreads();
    constexpr int UH = FMT == 0 ? 1 : 2;                                  // rows of a lane's group
    const int ng = (p.GJ * c) >> 2, units = ng * ((p.GI * c) / UH);
    const int copy = tid & (RD_COPIES - 1);
    for (int idx = tid; idx < units; idx += RD_THREADS) {
        const int ur = redact_div(idx, p.by_groups), g = idx - ur * ng;
        const int i0 = y0 + ur * UH, j0 = x0 + 4 * g;
        const PaintGroup u = paint_group<FMT>(p.t, p.H, p.W, b, i0, j0);
        int s[2][3];
        bool have[2];
        paint_load_halves<FMT>(p.t, u, s, have);
        const int ci = redact_div(ur * UH, p.by_cell[0]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (!have[h]) continue;
            int *dst = sums[copy][ci * p.GJ + redact_div(4 * g + 2 * h, p.by_cell[0])];
            atomicAdd(dst, s[h][0]); atomicAdd(dst + 1, s[h][1]); atomicAdd(dst + 2, s[h][2]);
        }
    }
    __syncthreads();
    const int ch = (p.H + 1) >> 1, cw = (p.W + 1) >> 1, hc = c >> 1;
    for (int e = tid; e < p.GI * p.GJ; e += RD_THREADS) {
        const int ci = e / p.GJ, I = I0 + ci, J = J0 + (e - ci * p.GJ);
        if (I >= p.nI || J >= p.nJ) continue;
        int S[3] = {0, 0, 0};
        for (int k = 0; k < RD_COPIES; ++k) { S[0] += sums[k][e][0]; S[1] += sums[k][e][1]; S[2] += sums[k][e][2]; }
        const int n = (min(p.H, (I + 1) * c) - I * c) * (min(p.W, (J + 1) * c) - J * c);
        const int n2 = FMT == 0 ? n : (min(ch, (I + 1) * hc) - I * hc) * (min(cw, (J + 1) * hc) - J * hc);      // chroma samples of the cell
        p.means[((int64_t)b * p.nI + I) * p.nJ + J] = px_pack(redact_mean(S[0], n), redact_mean(S[1], n2), redact_mean(S[2], n2));
    }
}

// Rows lo, lo + 1, ... (one per lane, below cnt) of frame b against the tile [tx0, tx0 + TW) x [ty0, ty0 + TH): the hits into
// `hits`; returns their number.  Every lane of the workgroup calls it (two barriers inside).
__device__ int redact_collect(const RedactArgs &p, int b, int lo, int cnt, int tx0, int ty0, int TW, int TH, RedactHit *hits, int *wave_cnt) {
    const int r = lo + (int)threadIdx.x;
    RedactHit h;
    float ex, ey;
    const bool hit = r < cnt && redact_row(p, b, r, h, ex, ey) &&
                     paint_reaches(h.cx, h.cy, ex, ey, (float)tx0, (float)ty0, (float)(tx0 + TW), (float)(ty0 + TH));
    return paint_compact(hit, wave_cnt, [&](int slot) { hits[slot] = h; });
}

// The new value at sample (i, j) of the luma / RGB grid (G = 0: cells of c x c samples) or of the chroma grid (G = 1: c/2 x c/2):
// r | g << 8 | b << 16 (y | u << 8 | v << 16), the channels lo .. hi - 1 of it.  M: the frame's cell means.
template <int G>
__device__ __forceinline__ uint32_t redact_value(const RedactArgs &p, const uint32_t *M, int i, int j, int lo, int hi) {
    if (p.s.mode == MYDET_REDACT_SOLID) return p.color;
    if (p.s.mode == MYDET_REDACT_MOSAIC) return M[(int64_t)redact_div(i, p.by_cell[G]) * p.nJ + redact_div(j, p.by_cell[G])];
    const int cc = G ? p.s.cell >> 1 : p.s.cell, t = 2 * cc;
    const int u = 2 * j + 1 - cc, v = 2 * i + 1 - cc;
    const int Jf = u < 0 ? -1 : redact_div(u, p.by_two[G]), If = v < 0 ? -1 : redact_div(v, p.by_two[G]);
    const int fx = u - t * Jf, fy = v - t * If;
    const int Ja = px_clamp(Jf, 0, p.nJ - 1), Jb = px_clamp(Jf + 1, 0, p.nJ - 1);
    const int Ia = px_clamp(If, 0, p.nI - 1), Ib = px_clamp(If + 1, 0, p.nI - 1);
    const uint32_t maa = M[(int64_t)Ia * p.nJ + Ja], mab = M[(int64_t)Ia * p.nJ + Jb];
    const uint32_t mba = M[(int64_t)Ib * p.nJ + Ja], mbb = M[(int64_t)Ib * p.nJ + Jb];
    const int half = 2 * cc * cc;
    uint32_t out = 0;
    for (int k = lo; k < hi; ++k) {
        const int top = (t - fx) * px_chan(maa, k) + fx * px_chan(mab, k), bot = (t - fx) * px_chan(mba, k) + fx * px_chan(mbb, k);
        out |= (uint32_t)redact_div((t - fy) * top + fy * bot + half, p.by_whole[G]) << (8 * k);
    }
    return out;
}

template <int FMT>
__global__ __launch_bounds__(RD_THREADS) void redact_paint_kernel(const RedactArgs p) {
    __shared__ RedactHit hits[RD_THREADS];
    __shared__ int wave_cnt[RD_THREADS / 64];
    constexpr int TW = FMT == 0 ? 64 : 128;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * 16;
    const int cnt = paint_count(p.l, b);
    if (cnt <= 0) return;
    const int i0 = FMT == 0 ? ty0 + (tid >> 4) : ty0 + 2 * (tid >> 5);
    const int j0 = FMT == 0 ? tx0 + 4 * (tid & 15) : tx0 + 4 * (tid & 31);
    const PaintGroup u = paint_group<FMT>(p.t, p.H, p.W, b, i0, j0);
    const unsigned all = paint_inside(u);
    unsigned cov = 0;                                                     // bit 4 * r + k: pixel (i0 + r, j0 + k) is redacted
    for (int lo = 0; lo < cnt; lo += RD_THREADS) {
        const int n = redact_collect(p, b, lo, cnt, tx0, ty0, TW, 16, hits, wave_cnt);
        for (int e = 0; e < n && cov != all; ++e) {
            const RedactHit h = hits[e];
#pragma unroll
            for (int r = 0; r < (FMT == 0 ? 1 : 2); ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned bit = 1u << (4 * r + k);
                    if ((all & bit) && !(cov & bit) && redact_covers(h, p.s.shape, i0 + r, j0 + k)) cov |= bit;
                }
        }
        __syncthreads();                                                  // the list is rewritten by the next chunk
    }
    if (!cov) return;
    const uint32_t *M = p.means + (int64_t)b * p.nI * p.nJ;
    if constexpr (FMT == 0) {
        uint32_t px[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) if (cov & (1u << k)) px[k] = redact_value<0>(p, M, i0, j0 + k, 0, 3);
        paint_store(u, px, cov);
    } else {
        int Y[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, U[2] = {0, 0}, V[2] = {0, 0};
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (cov & (1u << (4 * r + k))) Y[r][k] = px_chan(redact_value<0>(p, M, i0 + r, j0 + k, 0, 1), 0);
        const unsigned cq = paint_quads(cov);                             // a chroma sample is redacted iff a pixel of its quad is
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (cq & (1u << q)) {
                const uint32_t v = redact_value<1>(p, M, i0 >> 1, (j0 >> 1) + q, 1, 3);
                U[q] = px_chan(v, 1); V[q] = px_chan(v, 2);
            }
        paint_store<FMT>(p.t, u, Y, U, V, cov, cq);
    }
}

bool redact_cell_ok(int cell) { return cell >= MYDET_REDACT_MIN_CELL && cell <= MYDET_REDACT_MAX_CELL && cell % 2 == 0; }

// The checks both entry points share; fills the list, the style, the view, the cell grid and the means block of `p`
int redact_check(const mydet_draw_list *l, const mydet_redact_style *s, int B, int H, int W, void *workspace, RedactArgs &p) {
    if (!s || B <= 0 || H <= 0 || W <= 0 || paint_list_check(l, true)) return MYDET_E_BADARG;
    if (s->mode != MYDET_REDACT_MOSAIC && s->mode != MYDET_REDACT_SMOOTH && s->mode != MYDET_REDACT_SOLID) return MYDET_E_BADARG;
    if (s->shape != MYDET_REDACT_BOX && s->shape != MYDET_REDACT_ELLIPSE) return MYDET_E_BADARG;
    if (!redact_cell_ok(s->cell) || !(s->pad > 0.0f) || !(s->pad <= 3.402823466e38f)) return MYDET_E_BADARG;
    if (s->n_classes < 0 || s->n_classes > MYDET_REDACT_MAX_CLASSES || (s->n_classes > 0 && !l->cls)) return MYDET_E_BADARG;
    if (s->mode != MYDET_REDACT_SOLID && !workspace) return MYDET_E_BADARG;
    const int c = s->cell;
    p.l = *l; p.s = *s; p.H = H; p.W = W;
    p.nI = (H + c - 1) / c; p.nJ = (W + c - 1) / c;
    p.GI = (16 + c - 1) / c;                                              // at least 16 rows
    p.GJ = (64 + c - 1) / c;                                              // at least 64 columns, a multiple of 4: the groups stay aligned
    if ((p.GJ * c) % 4) ++p.GJ;
    p.means = static_cast<uint32_t *>(workspace);
    if (p.GI * p.GJ > RD_CELLS) return MYDET_E_UNSUPP;
    if (H >= (1 << 22) || W >= (1 << 22)) return MYDET_E_UNSUPP;          // redact_div takes values below 2^24: 2 * W + 1 is one
    for (int g = 0; g < 2; ++g) {
        const int cc = g ? c / 2 : c;
        p.by_cell[g] = redact_div_of(cc); p.by_two[g] = redact_div_of(2 * cc); p.by_whole[g] = redact_div_of(4 * cc * cc);
    }
    p.by_groups = redact_div_of((p.GJ * c) / 4);
    if (B > 65535 || (H + 15) / 16 > 65535) return MYDET_E_UNSUPP;
    return 0;
}

template <int FMT>
int redact_launch(const RedactArgs &p, int B, hipStream_t stream) {
    if (p.s.mode != MYDET_REDACT_SOLID) {
        const dim3 grid((unsigned)((p.nJ + p.GJ - 1) / p.GJ), (unsigned)((p.nI + p.GI - 1) / p.GI), (unsigned)B);
        hipLaunchKernelGGL(redact_means_kernel<FMT>, grid, dim3(RD_THREADS), 0, stream, p);
        const int code = mydet_launch_status();
        if (code) return code;
    }
    constexpr int TW = FMT == 0 ? 64 : 128;
    const dim3 grid((unsigned)((p.W + TW - 1) / TW), (unsigned)((p.H + 15) / 16), (unsigned)B);
    hipLaunchKernelGGL(redact_paint_kernel<FMT>, grid, dim3(RD_THREADS), 0, stream, p);
    return mydet_launch_status();
}

}  // namespace

extern "C" int64_t mydet_redact_workspace_bytes(int B, int H, int W, int cell) {
    if (B <= 0 || H <= 0 || W <= 0 || !redact_cell_ok(cell)) return MYDET_E_BADARG;
    return (int64_t)B * ((H + cell - 1) / cell) * ((W + cell - 1) / cell) * 4;
}

extern "C" int mydet_redact_boxes_rgb_u8(unsigned char *dst, int B, int H, int W, int64_t img_bytes, int64_t row_bytes,
                                         const mydet_draw_list *list, const mydet_redact_style *style, void *workspace, void *stream) {
    RedactArgs p = {};
    int code = redact_check(list, style, B, H, W, workspace, p);
    if (!code) code = paint_planes_rgb(p.t, dst, img_bytes, row_bytes, W);
    if (code) return code;
    p.color = px_pack(style->color[0], style->color[1], style->color[2]);
    return redact_launch<0>(p, B, (hipStream_t)stream);
}

extern "C" int mydet_redact_boxes_yuv420_u8(const mydet_yuv420_src *planes, int B, int H, int W, const mydet_draw_list *list,
                                            const mydet_redact_style *style, void *workspace, void *stream) {
    RedactArgs p = {};
    int code = redact_check(list, style, B, H, W, workspace, p);
    if (!code) code = paint_planes_yuv420(p.t, planes, W);
    if (code) return code;
    p.color = draw_yuv_of(DRAW_YUV[planes->matrix][planes->full_range], px_pack(style->color[0], style->color[1], style->color[2]));
    return planes->layout == MYDET_YUV420_I420 ? redact_launch<2>(p, B, (hipStream_t)stream) : redact_launch<1>(p, B, (hipStream_t)stream);
}
