// The pixels a weight-gradient tile of ONE tap has to visit.
//
// For tap (ddy, ddx) (source pixel = output pixel + (ddy, ddx), same-size source) the output pixels whose source lies inside the
// image form the rectangle [y0, y0 + hv) x [x0, x0 + wv) of every image: nv = hv * wv pixels per image instead of H * W.  The
// walk enumerates them image by image, row by row:
//     i -> img = i / nv, j = i - img * nv, yy = j / wv, xx = j - yy * wv, pixel = img * H*W + (y0 + yy) * W + x0 + xx
// One set of inline functions for the kernels (igemm_wgrad_p3_kernel / igemm_wgrad_p3w_kernel stage row i of the walk instead of
// pixel i) and for the host (uclstm_igemm_wgrad_walk), so that what the tests enumerate is what the kernels read.  The 4-wave
// kernel has no second wave on its SIMD to hide integer arithmetic behind, so it calls the three steps of valid_walk_pixel one
// at a time between its MFMAs; the 8-wave kernel and the host call valid_walk_pixel.
#pragma once
#include "common.h"

constexpr uint32_t WALK_NONE = 0xffffffffu;      // entry past the end of the walk

// FastDiv of common.h without its special case: q = umulhi(2 m, magic) >> shift with magic = ceil(2^(31 + l) / d), shift = l,
// 2^(l-1) < d <= 2^l -- the same quotient m * magic / 2^(31 + l), exact for every m < 2^31, and d == 1 is magic 2^31, shift 0
// instead of a branch (the walk runs among the MFMAs of the kernels' main loop, which must stay one basic block).  d == 0 as 1.
struct WalkDiv {
    uint32_t magic, shift;
};
static inline WalkDiv make_walkdiv(uint32_t d) {
    if (d < 1) d = 1;
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    WalkDiv f;
    f.magic = (uint32_t)(((1ull << (31 + l)) + d - 1) / d);
    f.shift = l;
    return f;
}
// the multiply of the division (the quarter-rate instruction) and the whole division
__host__ __device__ inline uint32_t walk_div_hi(uint32_t m, const WalkDiv& f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(m << 1, f.magic);
#else
    return (uint32_t)(((uint64_t)(m << 1) * f.magic) >> 32);
#endif
}
__host__ __device__ inline uint32_t walk_div(uint32_t m, const WalkDiv& f) { return walk_div_hi(m, f) >> f.shift; }

// SMALL: H and W are powers of two and n_img * H * W < 2^24 -- the products are 24-bit multiplies (full rate on the device, the
// 32-bit multiply is quarter rate) and the pixel index is put together with shifts.  The kernels run SMALL walks only.
template <bool SMALL>
__host__ __device__ inline uint32_t walk_mul(uint32_t a, uint32_t b) {
    if constexpr (SMALL) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __umul24(a, b);
#else
        return (a & 0xffffffu) * (b & 0xffffffu);
#endif
    } else {
        return a * b;
    }
}

struct ValidWalk {
    int32_t y0, x0, hv, wv;
    int32_t nv;              // pixels of the rectangle (0: the tap never falls inside the image)
    int32_t HW, W;
    int32_t lHW, lW;         // their logarithms when both are powers of two (SMALL walks), else -1
    uint32_t total;          // entries of the walk: n_img * nv (a kernel block lowers it to the end of its own range)
    WalkDiv dNv, dWv;
};

// dNv / dWv: make_walkdiv of hv * wv and of wv (host only: it divides in 64 bits; the kernels take them from a table in their arguments)
__host__ __device__ inline ValidWalk make_valid_walk(int n_img, int H, int W, int ddy, int ddx, const WalkDiv& dNv, const WalkDiv& dWv) {
    ValidWalk w;
    const int ay = ddy < 0 ? -ddy : ddy, ax = ddx < 0 ? -ddx : ddx;
    w.y0 = ddy < 0 ? ay : 0;
    w.x0 = ddx < 0 ? ax : 0;
    w.hv = H > ay ? H - ay : 0;
    w.wv = W > ax ? W - ax : 0;
    w.nv = w.hv * w.wv;
    w.HW = H * W;
    w.W = W;
    w.lW = w.lHW = -1;
    if ((H & (H - 1)) == 0 && (W & (W - 1)) == 0) {
        int lw = 0, lh = 0;
        while ((1 << lw) < W) ++lw;
        while ((1 << lh) < H) ++lh;
        w.lW = lw;
        w.lHW = lw + lh;
    }
    w.total = (uint32_t)n_img * (uint32_t)w.nv;
    w.dNv = dNv;
    w.dWv = dWv;
    return w;
}
__host__ __device__ inline bool valid_walk_small(const ValidWalk& w, int n_img) {
    return w.lW >= 0 && (int64_t)n_img * w.HW < ((int64_t)1 << 24);
}

// the three steps of entry i: image and index inside the rectangle; row and column of the rectangle; the pixel index
template <bool SMALL>
__host__ __device__ inline uint32_t walk_in_image(const ValidWalk& w, uint32_t i, uint32_t img) { return i - walk_mul<SMALL>(img, (uint32_t)w.nv); }
template <bool SMALL>
__host__ __device__ inline uint32_t walk_in_row(const ValidWalk& w, uint32_t j, uint32_t yy) { return j - walk_mul<SMALL>(yy, (uint32_t)w.wv); }
template <bool SMALL>
__host__ __device__ inline uint32_t walk_compose(const ValidWalk& w, uint32_t i, uint32_t img, uint32_t yy, uint32_t xx) {
    uint32_t p;
    if constexpr (SMALL) p = (img << w.lHW) + (((uint32_t)w.y0 + yy) << w.lW) + (uint32_t)w.x0 + xx;
    else p = img * (uint32_t)w.HW + ((uint32_t)w.y0 + yy) * (uint32_t)w.W + (uint32_t)w.x0 + xx;
    return i < w.total ? p : WALK_NONE;
}

// pixel index (img * H*W + y * W + x) of entry i, WALK_NONE past the end
template <bool SMALL>
__host__ __device__ inline uint32_t valid_walk_pixel(const ValidWalk& w, uint32_t i) {
    const uint32_t img = walk_div(i, w.dNv);
    const uint32_t j = walk_in_image<SMALL>(w, i, img);
    const uint32_t yy = walk_div(j, w.dWv);
    const uint32_t xx = walk_in_row<SMALL>(w, j, yy);
    return walk_compose<SMALL>(w, i, img, yy, xx);
}

// 64-pixel K-tiles of a walk, and the share of them that pixel range `sp` of `splits` owns: [kb, kb + kt)
__host__ __device__ inline int valid_walk_ktiles(uint32_t total) { return (int)((total + 63u) >> 6); }
__host__ __device__ inline void valid_walk_range(uint32_t total, int splits, int sp, int& kb, int& kt) {
    const int n = valid_walk_ktiles(total);
    const int per = (n + splits - 1) / splits;
    kb = sp * per;
    kt = n - kb < per ? n - kb : per;
    if (kt < 0) kt = 0;
}
