// Appearance descriptors: a 128-bin colour histogram of every detection, sampled out of uint8 RGB frames or out of the planes of
// the 4:2:0 layouts, one launch per batch (include/mydet.h: mydet_appear_boxes_rgb_u8, where the rule is; DESIGN.md section 4 has
// it too).  Built with -ffp-contract=off: the sample coordinates are float32 expressions that must not be fused.
//
// grid = (groups of 4 rows, B frames), 256 lanes: one wavefront per box.  The 32 x 16 samples of a box are taken 64 at a time
// (lane = 4 sample rows x 16 columns, so the lanes of a wave read neighbouring pixels), each lane adds its 8 samples into the
// wave's 128 LDS counters with integer atomics -- any order gives the same sums -- and the 256-byte row leaves as one dword per
// lane.  Every row k < K is written: a row at or beyond the frame's count is zeros.  A tap is clamped into the H x W view before
// it addresses anything.  The 4:2:0 form converts every tap with yuv_pixel (yuv_fetch.h): the table, the formula and the 10-bit
// rule of yuv420.hip.
#include "paint_tile.h"
#include "yuv_fetch.h"

namespace {

constexpr int AP_THREADS = 256, AP_WAVES = AP_THREADS / 64;
constexpr int AP_BINS = MYDET_APPEAR_BINS;
constexpr int AP_ROWS = 32, AP_COLS = 16;                  // samples per box: 512
constexpr float AP_MAX = 536870912.0f;                     // 2^29: a sample beyond it (or NaN) is not counted

struct AppearArgs {
    mydet_draw_list l;
    int H, W;
    const unsigned char *src;                              // RGB frames (SRC 0)
    int64_t img, row;
    YuvSrc y;                                              // 4:2:0 planes (SRC 1..4)
    uint16_t *desc;
    int64_t frame;                                         // elements between the descriptors of two frames
};

// SRC: 0 RGB; 1 + 2 * (BPS - 1) + PLANAR for the 4:2:0 fetch (as crop.hip).  The pixel at (y, x), inside the view.
template <int SRC>
__device__ __forceinline__ uint32_t appear_pixel(const AppearArgs &p, int b, int y, int x) {
    if constexpr (SRC == 0) {
        const unsigned char *s = p.src + (int64_t)b * p.img + (int64_t)y * p.row + (int64_t)x * 3;
        return px_pack(s[0], s[1], s[2]);
    } else {
        return yuv_pixel<1 + ((SRC - 1) >> 1), ((SRC - 1) & 1) != 0>(p.y, b, y, x);
    }
}

template <int SRC>
__global__ __launch_bounds__(AP_THREADS) void appear_kernel(const AppearArgs p) {
    __shared__ uint32_t hist[AP_WAVES][AP_BINS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y, k = blockIdx.x * AP_WAVES + wave;
    int n = p.l.count ? p.l.count[(int64_t)b * p.l.count_stride] : p.l.K;
    n = max(0, min(n, p.l.K));                                            // a bad-class frame (a negative count) has no rows
    hist[wave][lane] = 0u;
    hist[wave][lane + 64] = 0u;
    __syncthreads();
    if (k < n) {
        const float *bx = p.l.box + (int64_t)b * p.l.box_frame_stride + (int64_t)k * p.l.box_row_stride;
        const float cx = bx[0], cy = bx[1], w = bx[2], h = bx[3];
        const float ang = p.l.angle ? p.l.angle[(int64_t)b * p.l.angle_frame_stride + (int64_t)k * p.l.angle_row_stride] : 0.0f;
        float c, s;
        box_rotation<true>(ang, c, s);
        const float sx = w * 0.75f / 16.0f, sy = h * 0.75f / 32.0f;
        const int j = lane & 15;
        const float lx = ((float)j + 0.5f - 8.0f) * sx;
#pragma unroll
        for (int q = 0; q < AP_ROWS * AP_COLS / 64; ++q) {
            const int i = q * 4 + (lane >> 4);
            const float ly = ((float)i + 0.5f - 16.0f) * sy;
            const float X = cx + lx * c - ly * s, Y = cy + lx * s + ly * c;
            if (fabsf(X) <= AP_MAX && fabsf(Y) <= AP_MAX) {                // false for NaN
                const int x = min(max((int)floorf(X), 0), p.W - 1), y = min(max((int)floorf(Y), 0), p.H - 1);
                const uint32_t v = appear_pixel<SRC>(p, b, y, x);
                const int bin = (i >> 4) * 64 + (px_chan(v, 0) >> 6) * 16 + (px_chan(v, 1) >> 6) * 4 + (px_chan(v, 2) >> 6);
                atomicAdd(&hist[wave][bin], 1u);
            }
        }
    }
    __syncthreads();
    if (k < p.l.K) {
        uint32_t *o = reinterpret_cast<uint32_t *>(p.desc + (int64_t)b * p.frame + (int64_t)k * AP_BINS);
        o[lane] = hist[wave][2 * lane] | (hist[wave][2 * lane + 1] << 16);
    }
}

// The checks both entry points share; fills everything of `p` but the source
int appear_setup(AppearArgs &p, dim3 &grid, const mydet_draw_list *l, uint16_t *desc, int64_t frame_stride, int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || paint_list_check(l, false) || !desc) return MYDET_E_BADARG;
    if (((uintptr_t)desc & 3) || (frame_stride & 1) || frame_stride < (int64_t)l->K * AP_BINS) return MYDET_E_BADARG;
    if (B > 65535 || H > (1 << 24) || W > (1 << 24)) return MYDET_E_UNSUPP;
    p.l = *l; p.H = H; p.W = W;
    p.desc = desc; p.frame = frame_stride;
    grid = dim3((unsigned)((l->K + AP_WAVES - 1) / AP_WAVES), (unsigned)B);
    return 0;
}

}  // namespace

extern "C" int mydet_appear_boxes_rgb_u8(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes, int64_t src_row_bytes,
                                         const mydet_draw_list *list, uint16_t *desc, int64_t desc_frame_stride, void *stream) {
    AppearArgs p = {};
    dim3 grid;
    const int code = appear_setup(p, grid, list, desc, desc_frame_stride, B, H, W);
    if (code) return code;
    if (!src || src_row_bytes < (int64_t)W * 3 || src_img_bytes < 0) return MYDET_E_BADARG;
    p.src = src; p.img = src_img_bytes; p.row = src_row_bytes;
    hipLaunchKernelGGL((appear_kernel<0>), grid, dim3(AP_THREADS), 0, (hipStream_t)stream, p);
    return mydet_launch_status();
}

extern "C" int mydet_appear_boxes_yuv420(const mydet_yuv420_src *src, int B, int H, int W, const mydet_draw_list *list, uint16_t *desc,
                                         int64_t desc_frame_stride, void *stream) {
    AppearArgs p = {};
    dim3 grid;
    int bps;
    bool planar;
    const int source = yuv_source(p.y, bps, planar, src, B, H, W);
    if (source) return source;
    const int code = appear_setup(p, grid, list, desc, desc_frame_stride, B, H, W);
    if (code) return code;
#define APPEAR_YUV(BPS, PLANAR) \
    hipLaunchKernelGGL((appear_kernel<1 + 2 * (BPS - 1) + (PLANAR ? 1 : 0)>), grid, dim3(AP_THREADS), 0, (hipStream_t)stream, p)
    YUV_DISPATCH(bps, planar, APPEAR_YUV);
#undef APPEAR_YUV
    return mydet_launch_status();
}
