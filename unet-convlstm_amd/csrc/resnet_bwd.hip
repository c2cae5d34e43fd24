// Backward of the HBM-bound encoder stages of the ResNet18-encoder model (resnet.py: a trainable encoder): the gradient of
// MaxPool2d(3, 2, 1) and of the BasicBlock tail relu(bn(z) + bn_r(r)).  As resnet.hip and pointwise.hip they move 16 bytes (8 act16
// channels) per lane per access on NHWC tensors, allocate nothing and never synchronise.  No atomics anywhere: the pooling gradient
// is a GATHER (the arg-max of every window is recomputed from the input by the thread that owns the pixels it can land on, so the
// forward pass stores no index and no two threads write one element), and
// the BatchNorm sums go through caller-owned rows of block totals that a second kernel adds in a fixed order.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int ROWS_CAP = 1024;         // rows of block totals of the reduction (four blocks per CU, as uclstm_bn_bwd_reduce)
constexpr int MIN_PIX = 32;            // pixels per block before a further block is worth its row

__device__ __forceinline__ void unpack8(const uint4 u, float (&f)[8]) {
    Pack16 p;
    p.u = u;
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = act_to_f32(p.e[i]);
}
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
    Pack16 p;
#pragma unroll
    for (int i = 0; i < 8; ++i) p.e[i] = f32_to_act(f[i]);
    return p.u;
}
__device__ __forceinline__ void load8f(const float* p, float (&f)[8]) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

int ew_grid(int64_t items) {
    int64_t b = (items + NT - 1) / NT;
    if (b > 256 * 8) b = 256 * 8;
    return (int)(b < 1 ? 1 : b);
}
bool aligned16(const void* p) { return p && ((uintptr_t)p % 16) == 0; }

// ---------------------------------------------------------------------------------------------
// MaxPool2d(3, 2, 1) backward, gather form
// ---------------------------------------------------------------------------------------------
// One thread per (2 x 2 block of input pixels, 16-byte chunk): block (j, i) holds the pixels (2j + py, 2i + px) and lies in the four
// windows (j + wy, i + wx), wy, wx in {0, 1} -- window (wj, wi) covers the rows 2wj - 1 .. 2wj + 1, clipped to the image as in
// maxpool3s2_kernel.  The thread scans each of its windows once in scan order with a strict '>' (the FIRST maximum wins: ATen's
// rule, as uclstm_maxpool2_bwd) and hands the window's dp to the block pixel at that position, if it is one: pixel (py, px) sits at
// row py + 1 - 2wy, column px + 1 - 2wx of the window.  36 loads of `a` (25 distinct chunks) per four outputs; a pixel that
// recomputed its own windows alone would need 8 .. 32.  There are Ho x Wo blocks (Ho = ceil(H / 2)); with an odd H or W the last
// block row / column holds pixels outside the image, which are neither read nor written.  Sum order: dskip, then the windows
// (j, i), (j, i + 1), (j + 1, i), (j + 1, i + 1), in f32, rounded once.
__global__ void maxpool3s2_bwd_kernel(const uint4* __restrict__ a, const uint4* __restrict__ dp, const uint4* __restrict__ dskip,
                                      uint4* __restrict__ da, int64_t chunks, FastDiv dcpc, FastDiv dWo, FastDiv dHo, int H, int W) {
    const int cpc = dcpc.d, Wo = dWo.d, Ho = dHo.d;
    for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < chunks; idx += (int64_t)gridDim.x * NT) {
        const uint32_t blk = fdiv((uint32_t)idx, dcpc);
        const uint32_t cc = (uint32_t)idx - blk * cpc;
        const uint32_t t = fdiv(blk, dWo);
        const int i = (int)(blk - t * Wo);
        const uint32_t img = fdiv(t, dHo);
        const int j = (int)(t - img * Ho);
        const int64_t ibase = (int64_t)img * H * W;
        float o[4][8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = 2 * j + (k >> 1), x = 2 * i + (k & 1);
            if (dskip && y < H && x < W) {
                unpack8(dskip[(ibase + (int64_t)y * W + x) * cpc + cc], o[k]);
            } else {
#pragma unroll
                for (int c = 0; c < 8; ++c) o[k][c] = 0.f;
            }
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int wy = w >> 1, wx = w & 1;
            const int wj = j + wy, wi = i + wx;
            if (wj >= Ho || wi >= Wo) continue;
            float m[8];
            int arg[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                m[c] = -INFINITY;
                arg[c] = -1;
            }
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int ys = 2 * wj + dy - 1;
                if ((unsigned)ys >= (unsigned)H) continue;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int xs = 2 * wi + dx - 1;
                    if ((unsigned)xs >= (unsigned)W) continue;
                    float v[8];
                    unpack8(a[(ibase + (int64_t)ys * W + xs) * cpc + cc], v);
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        if (v[c] > m[c]) {
                            m[c] = v[c];
                            arg[c] = dy * 3 + dx;
                        }
                }
            }
            float g[8];
            unpack8(dp[(((int64_t)img * Ho + wj) * Wo + wi) * cpc + cc], g);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int dy = (k >> 1) + 1 - 2 * wy, dx = (k & 1) + 1 - 2 * wx;          // compile-time after unrolling
                if (dy < 0 || dx < 0) continue;
                const int pos = dy * 3 + dx;
#pragma unroll
                for (int c = 0; c < 8; ++c) o[k][c] += (arg[c] == pos) ? g[c] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = 2 * j + (k >> 1), x = 2 * i + (k & 1);
            if (y < H && x < W) da[(ibase + (int64_t)y * W + x) * cpc + cc] = pack8(o[k]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// relu(bn(z) + bn_r(r)) backward
// ---------------------------------------------------------------------------------------------
// thread = one 16-byte channel chunk (cc) of every rows-th pixel row of its block, as bn_bwd_reduce_kernel of pointwise.hip
struct ColGeom {
    int cpc, rows, active;
};
ColGeom col_geom(int Cp) {
    ColGeom g;
    g.cpc = Cp / 8;
    g.rows = NT / g.cpc;
    g.active = g.rows * g.cpc;
    return g;
}
int reduce_blocks(int64_t pixels) {
    int64_t nb = (pixels + MIN_PIX - 1) / MIN_PIX;
    if (nb > ROWS_CAP) nb = ROWS_CAP;
    return (int)(nb < 1 ? 1 : nb);
}

// the ReLU mask of bn_add_relu_kernel (resnet.hip): the same two expressions, then the same add
__device__ __forceinline__ bool tail_positive(float zv, float sc, float sh, float rv, bool raff, float rsc, float rsh) {
    const float v = zv * sc + sh;
    const float q = raff ? rv * rsc + rsh : rv;
    return v + q > 0.f;
}

// partials[block][c] = (sum g, rstd_z * sum g*(z - mean_z), rstd_r * sum g*(r - mean_r)) over the block's pixels (the third is 0
// without a BatchNorm on r).  Block b takes the pixels (b + k*gridDim.x)*rows + prow, k = 0, 1, ...: the blocks read next to each
// other at every moment; the mapping is fixed, so the sums are reproducible.
__global__ void bn_add_relu_bwd_reduce_kernel(const uint4* __restrict__ z, const float* __restrict__ scale, const float* __restrict__ shift,
                                              const float* __restrict__ mean, const float* __restrict__ rstd, const uint4* __restrict__ r,
                                              const float* __restrict__ rscale, const float* __restrict__ rshift,
                                              const float* __restrict__ rmean, const float* __restrict__ rrstd,
                                              const uint4* __restrict__ da, float* __restrict__ partials, int64_t pixels, int Cp,
                                              ColGeom cg) {
    extern __shared__ float red[];          // [rows][cpc*24]
    const bool raff = rscale != nullptr;
    const int width = cg.cpc * 24;
    if ((int)threadIdx.x < cg.active) {
        const int cc = threadIdx.x % cg.cpc, prow = threadIdx.x / cg.cpc, c0 = cc * 8;
        float sc[8], sh[8], mu[8], rsc[8], rsh[8], rmu[8];
        load8f(scale + c0, sc);
        load8f(shift + c0, sh);
        load8f(mean + c0, mu);
#pragma unroll
        for (int i = 0; i < 8; ++i) rsc[i] = rsh[i] = rmu[i] = 0.f;
        if (raff) {
            load8f(rscale + c0, rsc);
            load8f(rshift + c0, rsh);
            load8f(rmean + c0, rmu);
        }
        float s1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s2[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s3[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int64_t step = (int64_t)gridDim.x * cg.rows;
        int64_t p = (int64_t)blockIdx.x * cg.rows + prow;
        // (one pixel row per trip: with two in flight the kernel needs more than the 128 VGPRs of four waves per SIMD and spills 76 bytes
        // per lane; a block walks at most five rows at the shapes of the encoder)
        for (; p < pixels; p += step) {
            const int64_t ia = p * cg.cpc + cc;
            float zv[8], rv[8], gv[8];
            unpack8(z[ia], zv);
            unpack8(r[ia], rv);
            unpack8(da[ia], gv);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float g0 = tail_positive(zv[i], sc[i], sh[i], rv[i], raff, rsc[i], rsh[i]) ? gv[i] : 0.f;
                s1[i] += g0;
                s2[i] = fmaf(g0, zv[i] - mu[i], s2[i]);
                s3[i] = fmaf(g0, rv[i] - rmu[i], s3[i]);
            }
        }
        float rs[8], rrs[8];
        load8f(rstd + c0, rs);
#pragma unroll
        for (int i = 0; i < 8; ++i) rrs[i] = 0.f;
        if (raff) load8f(rrstd + c0, rrs);
        float* out = red + prow * width + cc * 24;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            out[i * 3] = s1[i];
            out[i * 3 + 1] = s2[i] * rs[i];
            out[i * 3 + 2] = s3[i] * rrs[i];
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < width; j += NT) {
        float t = 0.f;
        for (int k = 0; k < cg.rows; ++k) t += red[k * width + j];
        partials[(int64_t)blockIdx.x * Cp * 3 + j] = t;
    }
}

// Fixed-order sum of the rows: block = 32 consecutive (channel, j) entries, 8 row lanes each adding every 8th row in f64, then
// lane 0 adds the 8 lane sums in order (bn_bwd_sum_kernel of pointwise.hip, for three columns and two tables).
__global__ __launch_bounds__(256) void bn_add_relu_bwd_sum_kernel(const float* __restrict__ partials, float* __restrict__ sums,
                                                                  float* __restrict__ rsums, int rows, int Cp) {
    __shared__ double red[8][32];
    const int e = blockIdx.x * 32 + (threadIdx.x & 31);          // entry c*3 + j
    const int lane = threadIdx.x >> 5;
    double t = 0.0;
    if (e < Cp * 3)
        for (int b = lane; b < rows; b += 8) t += (double)partials[(int64_t)b * Cp * 3 + e];
    red[lane][threadIdx.x & 31] = t;
    __syncthreads();
    if (lane == 0 && e < Cp * 3) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += red[k][threadIdx.x];
        const int c = e / 3, j = e - 3 * c;
        if (j == 0) {
            sums[c * 2] = (float)s;
            if (rsums) rsums[c * 2] = (float)s;
        } else if (j == 1) {
            sums[c * 2 + 1] = (float)s;
        } else if (rsums) {
            rsums[c * 2 + 1] = (float)s;
        }
    }
}

// dz = sc*(g - s1/n - xhat*s2/n) = sc*g + k1*z + k0,  k1 = -sc*rs*s2/n,  k0 = -sc*s1/n - k1*mu  (bn_bwd_apply_cols_kernel), with the
// constants of both operands in registers; a block owns a contiguous pixel range.
__global__ void bn_add_relu_bwd_apply_kernel(const uint4* __restrict__ z, const float* __restrict__ scale, const float* __restrict__ shift,
                                             const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ sums,
                                             const uint4* __restrict__ r, const float* __restrict__ rscale, const float* __restrict__ rshift,
                                             const float* __restrict__ rmean, const float* __restrict__ rrstd,
                                             const float* __restrict__ rsums, const uint4* __restrict__ da, uint4* __restrict__ dz,
                                             uint4* __restrict__ dr, int64_t pixels, ColGeom cg, int64_t pix_per_block, float inv_n) {
    if ((int)threadIdx.x >= cg.active) return;
    const bool raff = rscale != nullptr;
    const int cc = threadIdx.x % cg.cpc, prow = threadIdx.x / cg.cpc, c0 = cc * 8;
    const int64_t p0 = (int64_t)blockIdx.x * pix_per_block;
    const int64_t p1 = min(pixels, p0 + pix_per_block);
    float sc[8], sh[8], k1[8], k0[8], rsc[8], rsh[8], rk1[8], rk0[8];
    {
        float mu[8], rs[8];
        load8f(scale + c0, sc);
        load8f(shift + c0, sh);
        load8f(mean + c0, mu);
        load8f(rstd + c0, rs);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float s1 = sums[(c0 + i) * 2], s2 = sums[(c0 + i) * 2 + 1];
            k1[i] = -sc[i] * rs[i] * s2 * inv_n;
            k0[i] = -sc[i] * s1 * inv_n - k1[i] * mu[i];
        }
    }
    if (raff) {
        float mu[8], rs[8];
        load8f(rscale + c0, rsc);
        load8f(rshift + c0, rsh);
        load8f(rmean + c0, mu);
        load8f(rrstd + c0, rs);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float s1 = rsums[(c0 + i) * 2], s2 = rsums[(c0 + i) * 2 + 1];
            rk1[i] = -rsc[i] * rs[i] * s2 * inv_n;
            rk0[i] = -rsc[i] * s1 * inv_n - rk1[i] * mu[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) rsc[i] = rsh[i] = rk1[i] = rk0[i] = 0.f;
    }
    for (int64_t p = p0 + prow; p < p1; p += cg.rows) {
        const int64_t ia = p * cg.cpc + cc;
        float zv[8], rv[8], gv[8], o[8];
        unpack8(z[ia], zv);
        unpack8(r[ia], rv);
        unpack8(da[ia], gv);
#pragma unroll
        for (int i = 0; i < 8; ++i) gv[i] = tail_positive(zv[i], sc[i], sh[i], rv[i], raff, rsc[i], rsh[i]) ? gv[i] : 0.f;
        if (dz) {
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = sc[i] * gv[i] + k1[i] * zv[i] + k0[i];
            dz[ia] = pack8(o);
        }
        if (dr) {
            if (raff) {
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = rsc[i] * gv[i] + rk1[i] * rv[i] + rk0[i];
                dr[ia] = pack8(o);
            } else {
                dr[ia] = pack8(gv);
            }
        }
    }
}

// the checks the two passes share; NULL-ness of the r group must be all or nothing
bool tail_args_ok(const void* z, const float* scale, const float* shift, const float* mean, const float* rstd, const void* r,
                  const float* rscale, const float* rshift, const float* rmean, const float* rrstd, const float* rsums, const void* da,
                  int64_t pixels, int Cp) {
    if (!aligned16(z) || !aligned16(r) || !aligned16(da) || pixels <= 0 || Cp <= 0 || (Cp % 8) || Cp / 8 > NT) return false;
    if (!aligned16(scale) || !aligned16(shift) || !aligned16(mean) || !aligned16(rstd)) return false;
    const int given = (rscale != nullptr) + (rshift != nullptr) + (rmean != nullptr) + (rrstd != nullptr) + (rsums != nullptr);
    if (given != 0 && given != 5) return false;
    if (given && (!aligned16(rscale) || !aligned16(rshift) || !aligned16(rmean) || !aligned16(rrstd))) return false;
    return pixels * (Cp / 8) < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int32_t uclstm_maxpool3s2_bwd(const void* a, const void* dp, const void* dskip, void* da, int32_t n_img, int32_t H, int32_t W,
                                         int32_t Cp, void* stream) {
    if (!aligned16(a) || !aligned16(dp) || !aligned16(da) || (dskip && !aligned16(dskip)) || n_img <= 0 || H <= 0 || W <= 0 || Cp <= 0 ||
        (Cp % 8))
        return UCLSTM_E_BADARG;
    if ((int64_t)n_img * H * W * (Cp / 8) >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t chunks = (int64_t)n_img * Ho * Wo * (Cp / 8);          // one thread per 2 x 2 block of input pixels and chunk
    UCLSTM_LAUNCH(maxpool3s2_bwd_kernel, dim3(ew_grid(chunks)), dim3(NT), 0, (hipStream_t)stream, (const uint4*)a, (const uint4*)dp,
                  (const uint4*)dskip, (uint4*)da, chunks, make_fastdiv(Cp / 8), make_fastdiv(Wo), make_fastdiv(Ho), H, W);
    return UCLSTM_OK;
}

#ifndef UCLSTM_ACT_F16
extern "C" int64_t uclstm_bn_add_relu_bwd_rows(int64_t pixels) {
    if (pixels <= 0) return UCLSTM_E_BADARG;
    return reduce_blocks(pixels);
}
#endif

extern "C" int32_t uclstm_bn_add_relu_bwd_reduce(const void* z, const float* scale, const float* shift, const float* mean,
                                                 const float* rstd, const void* r, const float* rscale, const float* rshift,
                                                 const float* rmean, const float* rrstd, const void* da, float* partials, float* sums,
                                                 float* rsums, int64_t pixels, int32_t Cp, void* stream) {
    if (!tail_args_ok(z, scale, shift, mean, rstd, r, rscale, rshift, rmean, rrstd, rsums, da, pixels, Cp) || !partials || !sums)
        return UCLSTM_E_BADARG;
    const ColGeom cg = col_geom(Cp);
    const int nb = reduce_blocks(pixels);
    const size_t lds = (size_t)cg.rows * cg.cpc * 24 * sizeof(float);          // <= 24 KiB
    UCLSTM_LAUNCH(bn_add_relu_bwd_reduce_kernel, dim3(nb), dim3(NT), lds, (hipStream_t)stream, (const uint4*)z, scale, shift, mean, rstd,
                  (const uint4*)r, rscale, rshift, rmean, rrstd, (const uint4*)da, partials, pixels, Cp, cg);
    UCLSTM_LAUNCH(bn_add_relu_bwd_sum_kernel, dim3((Cp * 3 + 31) / 32), dim3(256), 0, (hipStream_t)stream, partials, sums, rsums, nb, Cp);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_bn_add_relu_bwd_apply(const void* z, const float* scale, const float* shift, const float* mean,
                                                const float* rstd, const float* sums, const void* r, const float* rscale,
                                                const float* rshift, const float* rmean, const float* rrstd, const float* rsums,
                                                const void* da, void* dz, void* dr, int64_t pixels, int32_t Cp, void* stream) {
    if (!tail_args_ok(z, scale, shift, mean, rstd, r, rscale, rshift, rmean, rrstd, rsums, da, pixels, Cp) || !sums) return UCLSTM_E_BADARG;
    if ((!dz && !dr) || (dz && !aligned16(dz)) || (dr && !aligned16(dr))) return UCLSTM_E_BADARG;
    const ColGeom cg = col_geom(Cp);
    int64_t nb = (pixels + MIN_PIX - 1) / MIN_PIX;
    if (nb > 4096) nb = 4096;
    const int64_t ppb = (pixels + nb - 1) / nb;
    UCLSTM_LAUNCH(bn_add_relu_bwd_apply_kernel, dim3((unsigned)nb), dim3(NT), 0, (hipStream_t)stream, (const uint4*)z, scale, shift, mean,
                  rstd, sums, (const uint4*)r, rscale, rshift, rmean, rrstd, rsums, (const uint4*)da, (uint4*)dz, (uint4*)dr, pixels, cg, ppb,
                  (float)(1.0 / (double)pixels));
    return UCLSTM_OK;
}
