// The lr_tb box layer of the EfficientDet + custom FCOS head (_LR_TB_last, models/rpns.py:208-229):
//
//     dlr = depthwise3x3_pad1(x; W_lr0)        lr = conv_1x3_pad(0,1)(dlr; W_lr1) + b_lr1     (2 channels)
//     dtb = depthwise3x3_pad1(x; W_tb0)        tb = conv_3x1_pad(1,0)(dtb; W_tb1) + b_tb1     (2 channels)
//     ltrb = (lr[0], tb[0], lr[1], tb[1])
//
// The second conv pads the DEPTHWISE output: a depthwise value at a column (lr) / row (tb) outside the image is 0,
// not the 3x3 evaluated over the halo.  Every level of every image runs in ONE launch through a tile table (as
// sepconv.hip), so the 5x5 / 10x10 levels do not pay a launch each.
//
// One 256-thread workgroup owns an 8x8 output tile of one image, all channels:
//   1. the 12x12 input patch around the tile -> LDS (its four corner pixels are loaded but never read), float4 per thread,
//      loads unconditional at clamped coordinates, out-of-image pixels stored as the depthwise conv's zeros
//   2. "walkers": a lane owns a 4-channel group (lanes 0..31 of each half-wave = groups 0..31, C <= 128) and one row
//      (lr) or one column (tb) of the tile.  It slides a 3x3 window along its row / column and computes the 10
//      depthwise values that row / column needs (x' = -1..8 for lr, y' = -1..8 for tb), forced to 0 outside the image,
//      and folds each straight into the 8 x 2 partial outputs it feeds (4-channel dots) -- no depthwise map is stored
//   3. the partial outputs are summed over the 32 lanes of the half-wave by DPP (fixed order: bit-reproducible), the
//      lr and tb halves of a pixel meet in a 1 KiB LDS block, and 64 lanes write one 16-byte ltrb store per pixel.
// A workgroup runs 16 walkers: round 0 the 8 rows (lr), round 1 the 8 columns (tb), one per half-wave.
// LDS (144 C + 256) floats: 51.7 KB at C = 88 (3 workgroups per CU); above 64 KiB (C > 113) the kernel opts in.
#include "common.h"

namespace {

constexpr int LT_MAX = MYDET_LR_TB_MAX_LEVELS;
constexpr int LT_CMAX = MYDET_LR_TB_MAX_C;
constexpr int TS = 8, HP = TS + 4;

struct LtLevel {
    const float *x;
    int64_t ldx;
    const float *w;
    float *y;
    int64_t ldy;
    int H, W, vec, tiles_x, tiles_per_img, tile_begin;
};
struct LtArgs {
    int n, B, C;
    LtLevel p[LT_MAX];
};

__device__ __forceinline__ f32x4 lt_load(const float *p, int vec) {
    if (vec) return *reinterpret_cast<const f32x4 *>(p);
    return f32x4{p[0], p[1], p[2], p[3]};                        // pitch not a multiple of 4 floats / unaligned base
}

__device__ __forceinline__ float lt_dot4(f32x4 w, f32x4 d, float acc) {
    acc = fmaf(w[0], d[0], acc);
    acc = fmaf(w[1], d[1], acc);
    acc = fmaf(w[2], d[2], acc);
    return fmaf(w[3], d[3], acc);
}

// depthwise 3x3 of one 4-channel group from three rows (or columns) of the window, taps in (kh, kw) order
__device__ __forceinline__ f32x4 lt_dw(const f32x4 (&wd)[9], const f32x4 (&win)[3][3]) {
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = fmaf(wd[kh * 3 + kw][j], win[kh][kw][j], d[j]);
    return d;
}

template <int CTRL>
__device__ __forceinline__ float lt_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, false));
}

// sum over the 32 lanes of each half-wave; every lane of rows 1 and 3 (lanes 16..31, 48..63) ends with its half's sum
__device__ __forceinline__ float lt_half_sum(float v) {
    v += lt_dpp<0xb1>(v);                                   // quad_perm [1,0,3,2]
    v += lt_dpp<0x4e>(v);                                   // quad_perm [2,3,0,1]
    v += lt_dpp<0x141>(v);                                  // row_half_mirror
    v += lt_dpp<0x140>(v);                                  // row_mirror: the row's sum in every lane of the row
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xa, 0xf, false));   // row_bcast15 -> rows 1, 3
    return v;
}

__global__ __launch_bounds__(256) void lr_tb_kernel(const LtArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int C = a.C, CG = C >> 2;
    float *patch = lds;                                     // [12 * 12 pixels][C]
    float *res = lds + HP * HP * C;                         // [64 pixels][l, t, r, b]
    const int tid = threadIdx.x, bid = blockIdx.x;
    int pi = 0;
    for (int i = 1; i < a.n; ++i)
        if (bid >= a.p[i].tile_begin) pi = i;               // uniform
    const LtLevel &P = a.p[pi];
    const int t = bid - P.tile_begin;
    const int b = t / P.tiles_per_img, r = t - b * P.tiles_per_img;
    const int ty = r / P.tiles_x, tx = r - ty * P.tiles_x;
    const int oy0 = ty * TS, ox0 = tx * TS;
    const int H = P.H, W = P.W;
    const int64_t ldx = P.ldx;
    const float *xb = P.x + (int64_t)b * H * W * ldx;

    // 1. input patch -> LDS, eight float4 loads per thread in flight at a time (two rounds at C = 88)
    constexpr int NB = 8;
    const int n4 = HP * HP * CG;
    for (int i0 = tid; i0 < n4; i0 += NB * 256) {
        f32x4 v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int i = min(i0 + k * 256, n4 - 1);
            const int pix = i / CG, g = i - pix * CG;
            const int py = pix / HP, px = pix - py * HP;
            const int iy = oy0 - 2 + py, ix = ox0 - 2 + px;
            const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);
            v[k] = lt_load(xb + ((int64_t)cy * W + cx) * ldx + 4 * g, P.vec);
            if (iy != cy || ix != cx) v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int i = i0 + k * 256;
            if (i < n4) {
                const int pix = i / CG, g = i - pix * CG;
                *reinterpret_cast<f32x4 *>(patch + pix * C + 4 * g) = v[k];
            }
        }
    }
    __syncthreads();

    // 2-3. walkers: round 0 = lr along row `id`, round 1 = tb along column `id`
    const int lane = tid & 63, g = lane & 31, id = (tid >> 6) * 2 + (lane >> 5);
    const bool active = g < CG;
    const float *w = P.w;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        float acc[2][TS];
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int j = 0; j < TS; ++j) acc[o][j] = 0.f;
        if (active) {
            f32x4 wd[9], w1[2][3];
            const float *wdp = w + (round == 0 ? 0 : 9 * C) + 4 * g;
            const float *w1p = w + (round == 0 ? 18 * C : 24 * C) + 4 * g;
#pragma unroll
            for (int k = 0; k < 9; ++k) wd[k] = *reinterpret_cast<const f32x4 *>(wdp + k * C);
#pragma unroll
            for (int o = 0; o < 2; ++o)
#pragma unroll
                for (int k = 0; k < 3; ++k) w1[o][k] = *reinterpret_cast<const f32x4 *>(w1p + (o * 3 + k) * C);
            // lr: window rows = patch rows id+1..id+3 (input rows id-1..id+1), sliding along patch columns 0..11;
            // tb: window columns = patch columns id+1..id+3, sliding along patch rows 0..11.  win[kh][kw] in tap order.
            const int step = round == 0 ? C : HP * C;           // one patch column (lr) / row (tb) further
            const int across = round == 0 ? HP * C : C;         // the next tap row (lr) / column (tb)
            const float *base = patch + (round == 0 ? (id + 1) * HP * C : (id + 1) * C) + 4 * g;
            f32x4 win[3][3];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const f32x4 v = *reinterpret_cast<const f32x4 *>(base + s * step + q * across);
                    if (round == 0) win[q][s] = v; else win[s][q] = v;
                }
            const int lim = round == 0 ? W : H, org = round == 0 ? ox0 : oy0;
#pragma unroll
            for (int di = 0; di < TS + 2; ++di) {               // depthwise position d = di - 1 along the walk
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const f32x4 v = *reinterpret_cast<const f32x4 *>(base + (di + 2) * step + q * across);
                    if (round == 0) win[q][2] = v; else win[2][q] = v;
                }
                f32x4 d = lt_dw(wd, win);
                if ((unsigned)(org + di - 1) >= (unsigned)lim) d = f32x4{0.f, 0.f, 0.f, 0.f};   // the second conv's padding
                // output j takes tap k from position j + k - 1 = di - 1
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int j = di - k;
                    if (j >= 0 && j < TS) {
#pragma unroll
                        for (int o = 0; o < 2; ++o) acc[o][j] = lt_dot4(w1[o][k], d, acc[o][j]);
                    }
                }
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    if (round == 0) { win[q][0] = win[q][1]; win[q][1] = win[q][2]; }
                    else { win[0][q] = win[1][q]; win[1][q] = win[2][q]; }
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int j = 0; j < TS; ++j) acc[o][j] = lt_half_sum(acc[o][j]);
        // lanes 16..23 of each half hold the sums; lane 16 + j writes position j of its row / column
        const int j = g - 16;
        if (j >= 0 && j < TS) {
            float v0 = acc[0][0], v1 = acc[1][0];
#pragma unroll
            for (int k = 1; k < TS; ++k) {
                v0 = j == k ? acc[0][k] : v0;
                v1 = j == k ? acc[1][k] : v1;
            }
            const int pix = round == 0 ? id * TS + j : j * TS + id;
            res[pix * 4 + round] = v0 + w[30 * C + round];          // l (round 0) / t (round 1)
            res[pix * 4 + 2 + round] = v1 + w[30 * C + 2 + round];  // r / b
        }
    }
    __syncthreads();
    if (tid < TS * TS) {
        const int oy = oy0 + (tid >> 3), ox = ox0 + (tid & 7);
        if (oy < H && ox < W)
            *reinterpret_cast<f32x4 *>(P.y + (((int64_t)b * H + oy) * W + ox) * P.ldy) = *reinterpret_cast<const f32x4 *>(res + tid * 4);
    }
}

}  // namespace

extern "C" int mydet_lr_tb_levels_f32(int n, const mydet_lr_tb_level *levels, int B, int C, void *stream) {
    if (n <= 0 || n > LT_MAX || !levels || B <= 0 || C <= 0 || (C & 3) || C > LT_CMAX) return MYDET_E_BADARG;
    LtArgs a;
    a.n = n; a.B = B; a.C = C;
    int64_t tiles = 0;
    for (int i = 0; i < n; ++i) {
        const mydet_lr_tb_level &s = levels[i];
        LtLevel &p = a.p[i];
        if (!s.x || !s.w || !s.y || s.H <= 0 || s.W <= 0 || s.ldx < C || s.ldy < 4 || (s.ldy & 3) || !al16(s.w) ||
            !al16(s.y) || (reinterpret_cast<uintptr_t>(s.x) & 3))
            return MYDET_E_BADARG;
        p.x = s.x; p.ldx = s.ldx; p.w = s.w; p.y = s.y; p.ldy = s.ldy; p.H = s.H; p.W = s.W;
        p.vec = al16(s.x) && (s.ldx & 3) == 0;
        p.tiles_x = (s.W + TS - 1) / TS;
        p.tiles_per_img = p.tiles_x * ((s.H + TS - 1) / TS);
        p.tile_begin = (int)tiles;
        tiles += (int64_t)p.tiles_per_img * B;
        if (tiles > 0x7fffffff) return MYDET_E_UNSUPP;
    }
    const int lds = (HP * HP * C + TS * TS * 4) * (int)sizeof(float);
    if (lds > 65536) {
        static unsigned long long opted = 0;
        const int e = mydet_lds_opt_in(opted, lr_tb_kernel, lds);
        if (e) return e;
    }
    hipLaunchKernelGGL(lr_tb_kernel, dim3((unsigned)tiles), dim3(256), lds, (hipStream_t)stream, a);
    return mydet_launch_status();
}
