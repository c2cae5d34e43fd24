// HBM-bound kernels of the ResNet18-encoder model (resnet.py: PretrainedTemporalUNet) around the MFMA GEMMs: the 7x7 / stride 2
// first-layer gather, MaxPool2d(3, 2, 1), the residual tail of a BasicBlock (two per-channel affines, add, ReLU), nearest x2
// upsampling both ways, and the 3x3 output head with f32 accumulation and f32 NCHW output.  Like pointwise.hip they move 16
// bytes (8 act16 channels) per lane per access on NHWC tensors, allocate nothing and never synchronise; the head's parameter
// gradients reduce in registers, then across the block in LDS, and finish with one f32 atomic per (block, column) -- or, in the
// ORDERED instance (deterministic mode), with one stored row of block totals per block that uclstm_ordered_sum_f32 adds in
// row order.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int HEAD_CO = 4;             // most output channels of the head kernels (accumulators are registers: an instance per count)
constexpr int HEAD_CPC = 8;            // 16-byte chunks per pixel of the head's input (Cp <= 64)
constexpr int ORDERED_ROWS_CAP = 1024; // as the other ordered reductions: the finisher's chain stays a few us

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
// First layer: 7x7 / stride 2 / pad 3 gather of the f32 NCHW input (K = (tap, c), zero outside and in the K padding)
// ---------------------------------------------------------------------------------------------
__global__ void im2col7x7s2_kernel(const float* __restrict__ x, uint4* __restrict__ out, int64_t items, int C, int kpc, int H, int W,
                                   FastDiv dHoWo, FastDiv dWo, FastDiv dkpc, FastDiv dinner, FastDiv dC, int64_t inner_stride,
                                   int64_t outer_stride) {
    const int HoWo = dHoWo.d, Wo = dWo.d, HW = H * W;
    for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < items; idx += (int64_t)gridDim.x * NT) {
        // idx = (img*kpc + kc)*HoWo + pix: a wave reads runs of the input rows and writes 16 bytes per lane
        const uint32_t t = fdiv((uint32_t)idx, dHoWo);
        const uint32_t pix = (uint32_t)idx - t * HoWo;
        const uint32_t img = fdiv(t, dkpc);
        const uint32_t kc = t - img * kpc;
        const int yo = (int)fdiv(pix, dWo);
        const int xo = (int)pix - yo * Wo;
        const uint32_t o = fdiv(img, dinner);
        const uint32_t in = img - o * dinner.d;
        const float* src = x + (int64_t)in * outer_stride + (int64_t)o * inner_stride;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t k = kc * 8 + i;
            const uint32_t tap = fdiv(k, dC);
            const int c = (int)(k - tap * C);
            const int ys = 2 * yo + (int)(tap / 7) - 3, xs = 2 * xo + (int)(tap % 7) - 3;
            const bool ok = tap < 49 && (unsigned)ys < (unsigned)H && (unsigned)xs < (unsigned)W;
            const float t8 = src[ok ? (int64_t)c * HW + ys * W + xs : 0];          // branch-free, as in im2col_first_kernel
            v[i] = ok ? t8 : 0.f;
        }
        out[((int64_t)img * HoWo + pix) * kpc + kc] = pack8(v);
    }
}

// ---------------------------------------------------------------------------------------------
// MaxPool2d(3, 2, 1): the padding is -inf (it never wins), windows are clipped to the image
// ---------------------------------------------------------------------------------------------
__global__ void maxpool3s2_kernel(const uint4* __restrict__ a, uint4* __restrict__ p, int64_t chunks, FastDiv dcpc, FastDiv dWo,
                                  FastDiv dHo, int H, int W) {
    const int cpc = dcpc.d, Wo = dWo.d, Ho = dHo.d;
    for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < chunks; idx += (int64_t)gridDim.x * NT) {
        const uint32_t opix = fdiv((uint32_t)idx, dcpc);
        const uint32_t cc = (uint32_t)idx - opix * cpc;
        const uint32_t t = fdiv(opix, dWo);
        const int xo = (int)(opix - t * Wo);
        const uint32_t img = fdiv(t, dHo);
        const int yo = (int)(t - img * Ho);
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int ys = 2 * yo + dy - 1;
            if ((unsigned)ys >= (unsigned)H) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int xs = 2 * xo + dx - 1;
                if ((unsigned)xs >= (unsigned)W) continue;
                float v[8];
                unpack8(a[(((int64_t)img * H + ys) * W + xs) * cpc + cc], v);
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = fmaxf(o[i], v[i]);
            }
        }
        p[idx] = pack8(o);          // the window's centre (2yo, 2xo) is always inside the image: no -inf is stored
    }
}

// ---------------------------------------------------------------------------------------------
// a = relu((z*scale + shift) + (r*rscale + rshift)); a null pair is the identity
// ---------------------------------------------------------------------------------------------
__global__ void bn_add_relu_kernel(const uint4* __restrict__ z, const float* __restrict__ scale, const float* __restrict__ shift,
                                   const uint4* __restrict__ r, const float* __restrict__ rscale, const float* __restrict__ rshift,
                                   uint4* __restrict__ a, int64_t chunks, FastDiv dcpc) {
    for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < chunks; idx += (int64_t)gridDim.x * NT) {
        const uint32_t pix = fdiv((uint32_t)idx, dcpc);
        const int c0 = (int)((uint32_t)idx - pix * dcpc.d) * 8;
        float v[8], q[8];
        unpack8(z[idx], v);
        unpack8(r[idx], q);
        if (scale) {
            float sc[8], sh[8];
            load8f(scale + c0, sc);
            load8f(shift + c0, sh);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = v[i] * sc[i] + sh[i];
        }
        if (rscale) {
            float sc[8], sh[8];
            load8f(rscale + c0, sc);
            load8f(rshift + c0, sh);
#pragma unroll
            for (int i = 0; i < 8; ++i) q[i] = q[i] * sc[i] + sh[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i] + q[i], 0.f);
        a[idx] = pack8(v);
    }
}

// ---------------------------------------------------------------------------------------------
// Nearest x2 upsampling: one thread per INPUT chunk (one load, four stores / four loads, one store)
// ---------------------------------------------------------------------------------------------
__global__ void upsample2_fwd_kernel(const uint4* __restrict__ a, uint4* __restrict__ out, int64_t chunks, FastDiv dcpc, FastDiv dW,
                                     FastDiv dH) {
    const int cpc = dcpc.d, W = dW.d, H = dH.d;
    for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < chunks; idx += (int64_t)gridDim.x * NT) {
        const uint32_t pix = fdiv((uint32_t)idx, dcpc);
        const uint32_t cc = (uint32_t)idx - pix * cpc;
        const uint32_t t = fdiv(pix, dW);
        const uint32_t x = pix - t * W;
        const uint32_t img = fdiv(t, dH);
        const uint32_t y = t - img * H;
        const int64_t row = (int64_t)2 * W * cpc;
        const int64_t base = (((int64_t)img * 2 * H + 2 * y) * 2 * W + 2 * x) * cpc + cc;
        const uint4 v = a[idx];
        out[base] = v;
        out[base + cpc] = v;
        out[base + row] = v;
        out[base + row + cpc] = v;
    }
}

__global__ void upsample2_bwd_kernel(const uint4* __restrict__ dout, uint4* __restrict__ da, int64_t chunks, FastDiv dcpc, FastDiv dW,
                                     FastDiv dH) {
    const int cpc = dcpc.d, W = dW.d, H = dH.d;
    for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < chunks; idx += (int64_t)gridDim.x * NT) {
        const uint32_t pix = fdiv((uint32_t)idx, dcpc);
        const uint32_t cc = (uint32_t)idx - pix * cpc;
        const uint32_t t = fdiv(pix, dW);
        const uint32_t x = pix - t * W;
        const uint32_t img = fdiv(t, dH);
        const uint32_t y = t - img * H;
        const int64_t row = (int64_t)2 * W * cpc;
        const int64_t base = (((int64_t)img * 2 * H + 2 * y) * 2 * W + 2 * x) * cpc + cc;
        float d00[8], d01[8], d10[8], d11[8], o[8];
        unpack8(dout[base], d00);
        unpack8(dout[base + cpc], d01);
        unpack8(dout[base + row], d10);
        unpack8(dout[base + row + cpc], d11);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = ((d00[i] + d01[i]) + d10[i]) + d11[i];          // scan order: a pure function of the input
        da[idx] = pack8(o);
    }
}

// ---------------------------------------------------------------------------------------------
// Output head: conv3x3 pad 1, C (<= 64) -> Co (<= 4) channels, f32 accumulation, f32 NCHW output
// ---------------------------------------------------------------------------------------------
// One thread per pixel; the weights sit in LDS as [tap][co][c] (zero beyond C), every lane of a wave reads the same words
// (broadcast).  acc = b, then += a*w over (ky, kx, c) in that order, taps outside the image skipped.  NCO = Co: the accumulators
// are registers.
template <int NCO>
__global__ void head3x3_fwd_kernel(const uint4* __restrict__ a, const float* __restrict__ w, const float* __restrict__ b,
                                   float* __restrict__ y, int64_t pixels, FastDiv dHW, FastDiv dW, int H, int cpc, int C) {
    extern __shared__ float wl[];          // [9][NCO][cpc*8]
    const int HW = dHW.d, W = dW.d, cw = cpc * 8;
    for (int j = threadIdx.x; j < 9 * NCO * cw; j += NT) {
        const int c = j % cw, co = (j / cw) % NCO, tap = j / (cw * NCO);
        wl[j] = c < C ? w[(co * C + c) * 9 + tap] : 0.f;
    }
    __syncthreads();
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * NT) {
        const uint32_t img = fdiv((uint32_t)p, dHW);
        const uint32_t pix = (uint32_t)p - img * HW;
        const int y0 = (int)fdiv(pix, dW);
        const int x0 = (int)pix - y0 * W;
        float acc[NCO];
#pragma unroll
        for (int co = 0; co < NCO; ++co) acc[co] = b ? b[co] : 0.f;
        for (int ky = 0; ky < 3; ++ky) {
            const int ys = y0 + ky - 1;
            if ((unsigned)ys >= (unsigned)H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int xs = x0 + kx - 1;
                if ((unsigned)xs >= (unsigned)W) continue;
                const uint4* ap = a + (((int64_t)img * H + ys) * W + xs) * cpc;
                const float* wt = wl + (ky * 3 + kx) * NCO * cw;
                for (int cc = 0; cc < cpc; ++cc) {
                    float v[8];
                    unpack8(ap[cc], v);
#pragma unroll
                    for (int co = 0; co < NCO; ++co) {
                        float wv[8];
                        load8f(wt + co * cw + cc * 8, wv);
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[co] += v[i] * wv[i];
                    }
                }
            }
        }
#pragma unroll
        for (int co = 0; co < NCO; ++co) y[((int64_t)img * NCO + co) * HW + pix] = acc[co];
    }
}

// da[p][c] = act16(sum over (co, ky, kx) of dy[co][y+1-ky][x+1-kx] * w[co][c][ky][kx]), f32 sum in that order; padding channels
// stay exactly zero.  One thread per (pixel, 16-byte chunk); weights in LDS as [co][tap][c].
__global__ void head3x3_bwd_da_kernel(const float* __restrict__ w, const float* __restrict__ dy, uint4* __restrict__ da, int64_t chunks,
                                      FastDiv dcpc, FastDiv dHW, FastDiv dW, int H, int C, int Co) {
    extern __shared__ float wl[];          // [Co][9][cpc*8]
    const int cpc = dcpc.d, HW = dHW.d, W = dW.d, cw = cpc * 8;
    for (int j = threadIdx.x; j < Co * 9 * cw; j += NT) {
        const int c = j % cw, tap = (j / cw) % 9, co = j / (9 * cw);
        wl[j] = c < C ? w[(co * C + c) * 9 + tap] : 0.f;
    }
    __syncthreads();
    for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < chunks; idx += (int64_t)gridDim.x * NT) {
        const uint32_t p = fdiv((uint32_t)idx, dcpc);
        const uint32_t cc = (uint32_t)idx - p * cpc;
        const uint32_t img = fdiv(p, dHW);
        const uint32_t pix = p - img * HW;
        const int y0 = (int)fdiv(pix, dW);
        const int x0 = (int)pix - y0 * W;
        float o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int co = 0; co < Co; ++co) {
            const float* g0 = dy + ((int64_t)img * Co + co) * HW;
            for (int ky = 0; ky < 3; ++ky) {
                const int ys = y0 + 1 - ky;
                if ((unsigned)ys >= (unsigned)H) continue;
                for (int kx = 0; kx < 3; ++kx) {
                    const int xs = x0 + 1 - kx;
                    if ((unsigned)xs >= (unsigned)W) continue;
                    const float g = g0[ys * W + xs];
                    float wv[8];
                    load8f(wl + (co * 9 + ky * 3 + kx) * cw + cc * 8, wv);
#pragma unroll
                    for (int i = 0; i < 8; ++i) o[i] += g * wv[i];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if ((int)(cc * 8 + i) >= C) o[i] = 0.f;                               // g may be inf: inf * 0 must not reach the padding
        da[idx] = pack8(o);
    }
}

// dw[co][c][ky][kx] += sum_p dy[co][p] * a[c][y+ky-1][x+kx-1];  db[co] += sum_p dy[co][p].  A block owns a pixel range; a thread
// owns one (tap, 16-byte chunk) pair of one of `rows` interleaved pixel rows and keeps NCO (= Co) x 8 sums in registers; the rows meet in
// LDS and thread j adds column j over the rows in row order.  ORDERED: no atomics; `dw` is then the block-partial buffer
// [gridDim.x][dw_cols] and `db` the block-partial buffer [gridDim.x][Co]; every element of the block's two rows is stored.
template <bool ORDERED, int NCO>
__global__ void head3x3_bwd_dw_kernel(const uint4* __restrict__ a, const float* __restrict__ dy, float* __restrict__ dw,
                                      float* __restrict__ db, int64_t pixels, FastDiv dHW, FastDiv dW, FastDiv dcpc, int H, int C,
                                      int rows, int64_t pix_per_block) {
    extern __shared__ float red[];          // [rows][9*cpc*NCO*8 + NCO]
    constexpr int Co = NCO;
    const int cpc = dcpc.d, HW = dHW.d, W = dW.d;
    const int pairs = 9 * cpc, width = pairs * NCO * 8 + NCO;
    const int64_t p0 = (int64_t)blockIdx.x * pix_per_block;
    const int64_t p1 = min(pixels, p0 + pix_per_block);
    if ((int)threadIdx.x < rows * pairs) {
        const int prow = threadIdx.x / pairs, pair = threadIdx.x - prow * pairs;
        const int tap = (int)fdiv((uint32_t)pair, dcpc), cc = pair - tap * cpc;
        const int ky = tap / 3, kx = tap - 3 * ky;
        const bool centre = tap == 4 && cc == 0;
        float s[NCO][8], sb[NCO];
#pragma unroll
        for (int co = 0; co < NCO; ++co) {
            sb[co] = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) s[co][i] = 0.f;
        }
        for (int64_t p = p0 + prow; p < p1; p += rows) {
            const uint32_t img = fdiv((uint32_t)p, dHW);
            const uint32_t pix = (uint32_t)p - img * HW;
            const int y0 = (int)fdiv(pix, dW);
            const int x0 = (int)pix - y0 * W;
            const int ys = y0 + ky - 1, xs = x0 + kx - 1;
            float g[NCO];
#pragma unroll
            for (int co = 0; co < NCO; ++co) g[co] = dy[((int64_t)img * Co + co) * HW + pix];
            if (centre) {
#pragma unroll
                for (int co = 0; co < NCO; ++co) sb[co] += g[co];
            }
            if ((unsigned)ys < (unsigned)H && (unsigned)xs < (unsigned)W) {
                float v[8];
                unpack8(a[(((int64_t)img * H + ys) * W + xs) * cpc + cc], v);
#pragma unroll
                for (int co = 0; co < NCO; ++co)
#pragma unroll
                    for (int i = 0; i < 8; ++i) s[co][i] += g[co] * v[i];
            }
        }
        float* r = red + prow * width;
#pragma unroll
        for (int co = 0; co < NCO; ++co)
#pragma unroll
            for (int i = 0; i < 8; ++i) r[(pair * NCO + co) * 8 + i] = s[co][i];
        if (centre) {
#pragma unroll
            for (int co = 0; co < NCO; ++co) r[pairs * NCO * 8 + co] = sb[co];
        }
    }
    __syncthreads();
    const int dw_cols = Co * C * 9;
    for (int j = threadIdx.x; j < width; j += NT) {
        float t = 0.f;
        for (int r = 0; r < rows; ++r) t += red[r * width + j];
        if (j < pairs * NCO * 8) {
            const int pair = j / (NCO * 8), co = (j >> 3) % NCO, i = j & 7;
            const int tap = (int)fdiv((uint32_t)pair, dcpc), c = (pair - tap * cpc) * 8 + i;
            if (c < C) {
                const int col = (co * C + c) * 9 + tap;
                if constexpr (ORDERED) dw[(int64_t)blockIdx.x * dw_cols + col] = t;
                else if (dw) atomicAdd(dw + col, t);
            }
        } else {
            const int co = j - pairs * NCO * 8;
            if constexpr (ORDERED) db[(int64_t)blockIdx.x * Co + co] = t;
            else if (db) atomicAdd(db + co, t);
        }
    }
}

bool head_args_ok(const void* a, const float* w, int64_t n_img, int H, int W, int Cp, int C, int Co) {
    if (!aligned16(a) || !w || n_img <= 0 || H <= 0 || W <= 0 || C <= 0 || Cp < C || (Cp % 8) || Cp > 8 * HEAD_CPC || Co <= 0 ||
        Co > HEAD_CO)
        return false;
    return n_img * H * W * (Cp / 8) < ((int64_t)1 << 31);
}
struct HeadGeom {
    int rows, nb;
    int64_t ppb;
    size_t lds;
};
HeadGeom head_geom(int64_t pixels, int cpc, int Co, int nb) {
    HeadGeom g;
    g.rows = NT / (9 * cpc);
    g.nb = nb;
    g.ppb = (pixels + nb - 1) / nb;
    g.lds = (size_t)g.rows * (9 * cpc * Co * 8 + Co) * sizeof(float);
    return g;
}
// the head kernels keep Co accumulators (or Co x 8 sums) in registers: one instance per output-channel count
#define UCLSTM_HEAD_BY_CO(Co_, LAUNCH_) \
    switch (Co_) {                      \
        case 1: LAUNCH_(1); break;      \
        case 2: LAUNCH_(2); break;      \
        case 3: LAUNCH_(3); break;      \
        default: LAUNCH_(4); break;     \
    }

template <bool ORDERED>
int32_t head_bwd_dw(const void* a, const float* dy, float* dw, float* db, int64_t pixels, int H, int W, int Cp, int C, int Co,
                    const HeadGeom& g, hipStream_t st) {
#define UCLSTM_HEAD_DW(N_)                                                                                                                  \
    UCLSTM_LAUNCH((head3x3_bwd_dw_kernel<ORDERED, N_>), dim3(g.nb), dim3(NT), g.lds, st, (const uint4*)a, dy, dw, db, pixels, make_fastdiv(H * W), \
                  make_fastdiv(W), make_fastdiv(Cp / 8), H, C, g.rows, g.ppb)
    UCLSTM_HEAD_BY_CO(Co, UCLSTM_HEAD_DW)
#undef UCLSTM_HEAD_DW
    return UCLSTM_OK;
}
// pixel ranges of the head's parameter-gradient reduction: 2048 pixels each (a thread row then walks >= 73 of them), at most 1024
int head_blocks(int64_t pixels) {
    int64_t nb = (pixels + 2047) / 2048;
    if (nb > ORDERED_ROWS_CAP) nb = ORDERED_ROWS_CAP;
    return (int)(nb < 1 ? 1 : nb);
}

int32_t head_bwd_da(const float* w, const float* dy, void* da, int64_t n_img, int H, int W, int Cp, int C, int Co, hipStream_t st) {
    if (!aligned16(da)) return UCLSTM_E_BADARG;
    const int64_t chunks = n_img * H * W * (Cp / 8);
    UCLSTM_LAUNCH(head3x3_bwd_da_kernel, dim3(ew_grid(chunks)), dim3(NT), (size_t)Co * 9 * Cp * sizeof(float), st, w, dy, (uint4*)da, chunks,
                  make_fastdiv(Cp / 8), make_fastdiv(H * W), make_fastdiv(W), H, C, Co);
    return UCLSTM_OK;
}

}  // namespace

extern "C" int32_t uclstm_im2col7x7s2_first(const float* x, void* out, int32_t n_img, int32_t C, int32_t Kp, int32_t H, int32_t W,
                                            int32_t inner, int64_t inner_stride, int64_t outer_stride, void* stream) {
    if (!x || !aligned16(out) || n_img <= 0 || C <= 0 || Kp < 49 * C || (Kp % 8) || H <= 0 || W <= 0 || inner <= 0 || (n_img % inner))
        return UCLSTM_E_BADARG;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t items = (int64_t)n_img * (Kp / 8) * Ho * Wo;
    if (items >= ((int64_t)1 << 31) || (int64_t)C * H * W >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(im2col7x7s2_kernel, dim3(ew_grid(items)), dim3(NT), 0, (hipStream_t)stream, x, (uint4*)out, items, C, Kp / 8, H, W,
                  make_fastdiv(Ho * Wo), make_fastdiv(Wo), make_fastdiv(Kp / 8), make_fastdiv(inner), make_fastdiv(C), inner_stride,
                  outer_stride);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_maxpool3s2_fwd(const void* a, void* p, int32_t n_img, int32_t H, int32_t W, int32_t Cp, void* stream) {
    if (!aligned16(a) || !aligned16(p) || n_img <= 0 || H <= 0 || W <= 0 || Cp <= 0 || (Cp % 8)) return UCLSTM_E_BADARG;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    if ((int64_t)n_img * H * W * (Cp / 8) >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    const int64_t chunks = (int64_t)n_img * Ho * Wo * (Cp / 8);
    UCLSTM_LAUNCH(maxpool3s2_kernel, dim3(ew_grid(chunks)), dim3(NT), 0, (hipStream_t)stream, (const uint4*)a, (uint4*)p, chunks,
                  make_fastdiv(Cp / 8), make_fastdiv(Wo), make_fastdiv(Ho), H, W);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_bn_add_relu(const void* z, const float* scale, const float* shift, const void* r, const float* rscale,
                                      const float* rshift, void* a, int64_t pixels, int32_t Cp, void* stream) {
    if (!aligned16(z) || !aligned16(r) || !aligned16(a) || pixels <= 0 || Cp <= 0 || (Cp % 8)) return UCLSTM_E_BADARG;
    if ((scale == nullptr) != (shift == nullptr) || (rscale == nullptr) != (rshift == nullptr)) return UCLSTM_E_BADARG;
    if ((scale && (!aligned16(scale) || !aligned16(shift))) || (rscale && (!aligned16(rscale) || !aligned16(rshift)))) return UCLSTM_E_BADARG;
    const int64_t chunks = pixels * (Cp / 8);
    if (chunks >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(bn_add_relu_kernel, dim3(ew_grid(chunks)), dim3(NT), 0, (hipStream_t)stream, (const uint4*)z, scale, shift, (const uint4*)r,
                  rscale, rshift, (uint4*)a, chunks, make_fastdiv(Cp / 8));
    return UCLSTM_OK;
}

static bool upsample_args_ok(const void* lo, const void* hi, int32_t n_img, int32_t H, int32_t W, int32_t Cp) {
    if (!aligned16(lo) || !aligned16(hi) || n_img <= 0 || H <= 0 || W <= 0 || Cp <= 0 || (Cp % 8)) return false;
    return (int64_t)n_img * H * W * 4 * (Cp / 8) < ((int64_t)1 << 31);
}

extern "C" int32_t uclstm_upsample2_fwd(const void* a, void* out, int32_t n_img, int32_t H, int32_t W, int32_t Cp, void* stream) {
    if (!upsample_args_ok(a, out, n_img, H, W, Cp)) return UCLSTM_E_BADARG;
    const int64_t chunks = (int64_t)n_img * H * W * (Cp / 8);
    UCLSTM_LAUNCH(upsample2_fwd_kernel, dim3(ew_grid(chunks)), dim3(NT), 0, (hipStream_t)stream, (const uint4*)a, (uint4*)out, chunks,
                  make_fastdiv(Cp / 8), make_fastdiv(W), make_fastdiv(H));
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_upsample2_bwd(const void* dout, void* da, int32_t n_img, int32_t H, int32_t W, int32_t Cp, void* stream) {
    if (!upsample_args_ok(da, dout, n_img, H, W, Cp)) return UCLSTM_E_BADARG;
    const int64_t chunks = (int64_t)n_img * H * W * (Cp / 8);
    UCLSTM_LAUNCH(upsample2_bwd_kernel, dim3(ew_grid(chunks)), dim3(NT), 0, (hipStream_t)stream, (const uint4*)dout, (uint4*)da, chunks,
                  make_fastdiv(Cp / 8), make_fastdiv(W), make_fastdiv(H));
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_head3x3_fwd(const void* a, const float* w, const float* b, float* y, int64_t n_img, int32_t H, int32_t W,
                                      int32_t Cp, int32_t C, int32_t Co, void* stream) {
    if (!head_args_ok(a, w, n_img, H, W, Cp, C, Co) || !y) return UCLSTM_E_BADARG;
    const int64_t pixels = n_img * H * W;
#define UCLSTM_HEAD_FWD(N_)                                                                                                           \
    UCLSTM_LAUNCH(head3x3_fwd_kernel<N_>, dim3(ew_grid(pixels)), dim3(NT), (size_t)9 * N_ * Cp * sizeof(float), (hipStream_t)stream, \
                  (const uint4*)a, w, b, y, pixels, make_fastdiv(H * W), make_fastdiv(W), H, Cp / 8, C)
    UCLSTM_HEAD_BY_CO(Co, UCLSTM_HEAD_FWD)
#undef UCLSTM_HEAD_FWD
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_head3x3_bwd(const void* a, const float* w, const float* dy, void* da, float* dw, float* db, int64_t n_img,
                                      int32_t H, int32_t W, int32_t Cp, int32_t C, int32_t Co, void* stream) {
    if (!head_args_ok(a, w, n_img, H, W, Cp, C, Co) || !dy) return UCLSTM_E_BADARG;
    const int64_t pixels = n_img * H * W;
    if (da) {
        const int32_t rc = head_bwd_da(w, dy, da, n_img, H, W, Cp, C, Co, (hipStream_t)stream);
        if (rc != UCLSTM_OK) return rc;
    }
    if (dw || db) {
        const int32_t rc = head_bwd_dw<false>(a, dy, dw, db, pixels, H, W, Cp, C, Co, head_geom(pixels, Cp / 8, Co, head_blocks(pixels)),
                                              (hipStream_t)stream);
        if (rc != UCLSTM_OK) return rc;
    }
    return UCLSTM_OK;
}

// The ordered form reads 16-bit activations behind ONE symbol with an explicit activation type: the body is compiled in both
// passes under UCLSTM_ACT_IMPL(name), the public entry point exists in the bfloat16 pass only and dispatches (as pointwise.hip).
__attribute__((visibility("hidden"))) int32_t UCLSTM_ACT_IMPL(head3x3_bwd_ordered)(const void* a, const float* w, const float* dy, void* da,
                                                                                  float* partials, float* dw, float* db, int32_t accumulate,
                                                                                  int64_t n_img, int32_t H, int32_t W, int32_t Cp, int32_t C,
                                                                                  int32_t Co, void* stream) {
    if (!head_args_ok(a, w, n_img, H, W, Cp, C, Co) || !dy) return UCLSTM_E_BADARG;
    if ((dw || db) && !partials) return UCLSTM_E_BADARG;
    const int64_t pixels = n_img * H * W;
    if (da) {
        const int32_t rc = head_bwd_da(w, dy, da, n_img, H, W, Cp, C, Co, (hipStream_t)stream);
        if (rc != UCLSTM_OK) return rc;
    }
    if (dw || db) {
        const HeadGeom g = head_geom(pixels, Cp / 8, Co, head_blocks(pixels));
        const int dw_cols = Co * C * 9;
        float* pdb = partials + (int64_t)g.nb * dw_cols;
        const int32_t rc0 = head_bwd_dw<true>(a, dy, partials, pdb, pixels, H, W, Cp, C, Co, g, (hipStream_t)stream);
        if (rc0 != UCLSTM_OK) return rc0;
        if (dw) {
            const int32_t rc = uclstm_ordered_sum_f32(partials, g.nb, dw_cols, dw, accumulate, stream);
            if (rc != UCLSTM_OK) return rc;
        }
        if (db) {
            const int32_t rc = uclstm_ordered_sum_f32(pdb, g.nb, Co, db, accumulate, stream);
            if (rc != UCLSTM_OK) return rc;
        }
    }
    return UCLSTM_OK;
}

#ifndef UCLSTM_ACT_F16
int32_t head3x3_bwd_ordered_impl_f16(const void*, const float*, const float*, void*, float*, float*, float*, int32_t, int64_t, int32_t, int32_t,
                                     int32_t, int32_t, int32_t, void*);

extern "C" int64_t uclstm_head3x3_bwd_ordered_rows(int64_t n_img, int32_t H, int32_t W) {
    if (n_img <= 0 || H <= 0 || W <= 0) return UCLSTM_E_BADARG;
    return head_blocks(n_img * H * W);
}

extern "C" int32_t uclstm_head3x3_bwd_ordered(const void* a, const float* w, const float* dy, void* da, float* partials, float* dw, float* db,
                                              int32_t accumulate, int64_t n_img, int32_t H, int32_t W, int32_t Cp, int32_t C, int32_t Co,
                                              int32_t act_type, void* stream) {
    if (act_type == UCLSTM_ACT_TYPE_BF16)
        return UCLSTM_ACT_IMPL(head3x3_bwd_ordered)(a, w, dy, da, partials, dw, db, accumulate, n_img, H, W, Cp, C, Co, stream);
    if (act_type == UCLSTM_ACT_TYPE_F16)
        return head3x3_bwd_ordered_impl_f16(a, w, dy, da, partials, dw, db, accumulate, n_img, H, W, Cp, C, Co, stream);
    return UCLSTM_E_BADARG;
}
#endif
