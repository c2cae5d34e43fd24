// Loss (main.py:28-72) and optimiser (main.py:106-108) kernels: one pass each over f32 planes /
// flat parameter buffers, wave-shuffle + LDS block reduction, one f64 atomic per block -- or, in the ORDERED forms of the
// three reductions (deterministic mode), one stored row of block totals per block and a second launch that adds the rows in order.
#include "common.h"

#include <cfloat>
#include <type_traits>

namespace {

constexpr int NT = 256;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// reduce K doubles per thread across the block; thread 0 gets the totals
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* red /* [4][K] */) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = red[k] + red[K + k] + red[2 * K + k] + red[3 * K + k];
}

// the same block totals, stored: thread k < K writes column k of the block's row (the four wave sums added in the order above)
template <int K>
__device__ __forceinline__ void block_sum_store(double (&v)[K], double* red /* [4][K] */, double* __restrict__ row) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
    __syncthreads();
    const int t = threadIdx.x;
    if (t < K) row[t] = red[t] + red[K + t] + red[2 * K + t] + red[3 * K + t];
}

__device__ __forceinline__ float sgn(float v) { return (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : 0.f); }

// sums: [0] sum(ad*w*m) [1] sum(w*m) [2] sum(gd*mc) [3] sum(mc).  ORDERED: sums is the partial buffer [gridDim.x][4], no atomics
template <bool ORDERED>
__global__ void loss_fwd_kernel(const float* __restrict__ yp, const float* __restrict__ y, const float* __restrict__ mask,
                                double* __restrict__ sums, int64_t total, FastDiv dHW, FastDiv dW, int H, int W) {
    __shared__ double red[16];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int HW = dHW.d;
    for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NT) {
        const uint32_t pl = fdiv((uint32_t)idx, dHW);
        const uint32_t pix = (uint32_t)idx - pl * HW;
        const int i = (int)fdiv(pix, dW);
        const int j = (int)pix - i * W;
        const float a = yp[idx], b = y[idx];
        const float m = mask ? mask[idx] : 1.f;
        const float ab = fabsf(b);
        const float w = 1.f + 4.f * ab * ab * ab;               // main.py:38
        acc[0] += (double)(fabsf(a - b) * w * m);
        acc[1] += (double)(w * m);
        if (i < H - 1 && j < W - 1) {                            // main.py:57-62 crop
            const float dxp = yp[idx + 1] - a, dyp = yp[idx + W] - a;
            const float dxg = y[idx + 1] - b, dyg = y[idx + W] - b;
            acc[2] += (double)((fabsf(dxp - dxg) + fabsf(dyp - dyg)) * m);
            acc[3] += (double)m;
        }
    }
    if constexpr (ORDERED) {
        block_sum_store<4>(acc, red, sums + (int64_t)blockIdx.x * 4);
    } else {
        block_sum<4>(acc, red);
        if (threadIdx.x == 0)
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(sums + k, acc[k]);
    }
}

__global__ void loss_bwd_kernel(const float* __restrict__ yp, const float* __restrict__ y, const float* __restrict__ mask,
                                const float* __restrict__ coefs, float* __restrict__ grad, int64_t total, FastDiv dHW, FastDiv dW,
                                int H, int W) {
    const int HW = dHW.d;
    const float c1 = coefs[0], c2 = coefs[1];
    for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NT) {
        const uint32_t pl = fdiv((uint32_t)idx, dHW);
        const uint32_t pix = (uint32_t)idx - pl * HW;
        const int i = (int)fdiv(pix, dW);
        const int j = (int)pix - i * W;
        const float a = yp[idx], b = y[idx];
        const float m = mask ? mask[idx] : 1.f;
        const float ab = fabsf(b);
        float g = c1 * sgn(a - b) * (1.f + 4.f * ab * ab * ab) * m;
        float gg = 0.f;
        // cell (i,j) itself: -sx(i,j) - sy(i,j)
        if (i < H - 1 && j < W - 1) {
            const float sx = sgn((yp[idx + 1] - a) - (y[idx + 1] - b));
            const float sy = sgn((yp[idx + W] - a) - (y[idx + W] - b));
            gg -= (sx + sy) * m;
        }
        // cell (i,j-1): +sx(i,j-1)
        if (j >= 1 && i < H - 1) {
            const float ml = mask ? mask[idx - 1] : 1.f;
            gg += sgn((a - yp[idx - 1]) - (b - y[idx - 1])) * ml;
        }
        // cell (i-1,j): +sy(i-1,j)
        if (i >= 1 && j < W - 1) {
            const float mu = mask ? mask[idx - W] : 1.f;
            gg += sgn((a - yp[idx - W]) - (b - y[idx - W])) * mu;
        }
        grad[idx] = g + c2 * gg;
    }
}

// ORDERED: out is the partial buffer [gridDim.x], no atomics
template <bool ORDERED>
__global__ void sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ out) {
    __shared__ double red[4];
    double acc[1] = {0.0};
    const int64_t n4 = n >> 2;
    const float4* g4 = (const float4*)g;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * NT) {
        const float4 v = g4[i];
        acc[0] += (double)(v.x * v.x + v.y * v.y) + (double)(v.z * v.z + v.w * v.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const float v = g[(n4 << 2) + threadIdx.x];
        acc[0] += (double)(v * v);
    }
    if constexpr (ORDERED) {
        block_sum_store<1>(acc, red, out + blockIdx.x);
    } else {
        block_sum<1>(acc, red);
        if (threadIdx.x == 0) atomicAdd(out, acc[0]);
    }
}

// step_overflowed (common.h): the one predicate of the kernels that skip an overflowed fp16 step (adamw_scaled_kernel,
// adamw_groups_kernel with state), of the one that backs the scale off and does not count it (loss_scale_update_kernel), of the
// EMA sweep and of the statistics record (param_stats.hip).

__global__ void adamw_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                             int64_t n, const double* __restrict__ sumsq, float max_norm, float lr, float b1, float b2, float eps,
                             float wd, float inv_bc1, float inv_sqrt_bc2) {
    float coef = 1.f;
    if (sumsq && max_norm > 0.f) {                               // max_norm <= 0: no clipping, as in every sibling
        const float total = (float)sqrt(*sumsq);
        coef = fminf(max_norm / (total + 1e-6f), 1.f);          // torch.nn.utils.clip_grad_norm_ (main.py:106)
    }
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const float gi = g[i] * coef;
        float w = p[i] * (1.f - lr * wd);                        // decoupled decay (AdamW, main.py:275)
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
        w -= lr * inv_bc1 * mi / denom;
        p[i] = w;
        m[i] = mi;
        v[i] = vi;
    }
}

// The same update with every hyper-parameter and the step count read from DEVICE memory, so that the launch can sit in a
// captured HIP graph and still follow a learning-rate schedule: hyper = {lr, beta1, beta2, eps, weight_decay, max_norm
// (<= 0: no clipping), steps done so far (float, exact up to 2^24), reserved}.  adamw_advance_kernel bumps the count afterwards.
__global__ void adamw_dev_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                                 int64_t n, const double* __restrict__ sumsq, const float* __restrict__ hyper) {
    const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], max_norm = hyper[5];
    const double step = (double)hyper[6] + 1.0;
    const float inv_bc1 = (float)(1.0 / (1.0 - pow((double)b1, step)));          // as the host computes them for adamw_kernel
    const float inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, step)));
    float coef = 1.f;
    if (sumsq && max_norm > 0.f) {
        const float total = (float)sqrt(*sumsq);
        coef = fminf(max_norm / (total + 1e-6f), 1.f);
    }
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const float gi = g[i] * coef;
        float w = p[i] * (1.f - lr * wd);
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
        w -= lr * inv_bc1 * mi / denom;
        p[i] = w;
        m[i] = mi;
        v[i] = vi;
    }
}
__global__ void adamw_advance_kernel(float* hyper) {
    if (threadIdx.x == 0 && blockIdx.x == 0) hyper[6] += 1.f;
}

// fp16 training: the gradient buffer holds scale x the true gradient (loss scaling keeps fp16 activation gradients out of the
// subnormal range).  state = {scale, growth tracker, successful steps}.  Same update as adamw_kernel on g / scale; nothing is
// touched on an overflowed step (step_overflowed: it is skipped, the scale backs off in loss_scale_update_kernel); Adam's
// bias-correction step is the device-side count of successful steps, the corrections are computed as adamw_dev_kernel computes
// them (pow in double, rounded once).  The arithmetic is adamw_groups_kernel's, spelled out in the same way with contraction
// off: that kernel with state, one run and one group gives the same bits.
__global__ void adamw_scaled_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                                    int64_t n, const double* __restrict__ sumsq, float max_norm, float lr, float b1, float b2, float eps,
                                    float wd, const float* __restrict__ state) {
#pragma clang fp contract(off)
    const double ss = *sumsq;
    if (step_overflowed(ss)) return;
    const float inv_scale = 1.f / state[0];
    const double step = (double)state[2] + 1.0;
    const float lr_bc1 = lr * (float)(1.0 / (1.0 - pow((double)b1, step)));
    const float inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, step)));
    const float decay = __builtin_fmaf(-lr, wd, 1.f);            // decoupled decay factor 1 - lr * wd
    float coef = inv_scale;
    if (max_norm > 0.f) {
        const float total = (float)sqrt(ss) * inv_scale;
        coef *= fminf(max_norm / (total + 1e-6f), 1.f);
    }
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const float gi = g[i] * coef;
        const float mi = __builtin_fmaf(1.f - b1, gi, b1 * m[i]);
        const float vi = b2 * v[i] + ((1.f - b2) * gi) * gi;
        const float denom = __builtin_fmaf(sqrtf(vi), inv_sqrt_bc2, eps);
        p[i] = decay * p[i] - (lr_bc1 * mi) / denom;
        m[i] = mi;
        v[i] = vi;
    }
}

// AdamW over parameter groups in ONE sweep.  runs = i64[n_runs][3] {begin, end, group}: ascending, gap-free, covering [0, n)
// (the flat buffer keeps the model's registration order, so groups interleave).  hyper = f32[8 * (1 + n_groups)]: block 0 is
// global {max_norm (<= 0: no clipping), steps done so far (exact up to 2^24), reserved x 6}, block 1 + k is group k
// {lr, beta1, beta2, eps, weight_decay, reserved x 3}.  Every block first derives the groups' bias corrections into LDS (as
// adamw_dev_kernel computes them).  A block then walks its grid-stride chunks in ascending order, so its run index only ever
// moves forward: one binary search for the first chunk, after that a chunk inside the current run costs no table read at all,
// and a lane reloads its six group values from LDS only where its group changes.  state (optional) = {scale, growth tracker,
// successful steps}: the semantics of adamw_scaled_kernel, with the bias-correction step taken from state[2].
__global__ void adamw_groups_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                                    int64_t n, const double* __restrict__ sumsq, const int64_t* __restrict__ runs, int n_runs,
                                    const float* __restrict__ hyper, int n_groups, const float* __restrict__ state) {
    // With one group the result must equal adamw_dev_kernel's bit for bit.  Which products of that kernel's update the compiler
    // fuses into multiply-adds depends on the code around them, so here the fused ones are spelled out (they are the ones
    // adamw_dev_kernel compiles to) and contraction is off for everything else.
#pragma clang fp contract(off)
    extern __shared__ float gh[];                                // [n_groups][8]: lr / bc1, b1, b2, eps, 1 - lr wd, 1 / sqrt(bc2), -, -
    const float max_norm = hyper[0];
    float coef = 1.f;
    double step;
    if (state) {
        const double ss = *sumsq;
        if (step_overflowed(ss)) return;                         // touch nothing (uniform over the grid)
        const float inv_scale = 1.f / state[0];
        step = (double)state[2] + 1.0;
        coef = inv_scale;
        if (max_norm > 0.f) {
            const float total = (float)sqrt(ss) * inv_scale;
            coef *= fminf(max_norm / (total + 1e-6f), 1.f);
        }
    } else {
        step = (double)hyper[1] + 1.0;
        if (sumsq && max_norm > 0.f) {
            const float total = (float)sqrt(*sumsq);
            coef = fminf(max_norm / (total + 1e-6f), 1.f);
        }
    }
    for (int k = threadIdx.x; k < n_groups; k += NT) {
        const float* h = hyper + 8 * (1 + k);
        const float glr = h[0], gb1 = h[1], gb2 = h[2];
        gh[8 * k + 0] = glr * (float)(1.0 / (1.0 - pow((double)gb1, step)));
        gh[8 * k + 1] = gb1;
        gh[8 * k + 2] = gb2;
        gh[8 * k + 3] = h[3];
        gh[8 * k + 4] = __builtin_fmaf(-glr, h[4], 1.f);                      // decoupled decay factor 1 - lr * wd
        gh[8 * k + 5] = (float)(1.0 / sqrt(1.0 - pow((double)gb2, step)));
    }
    __syncthreads();
    // A chunk is U * NT elements, lane t takes elements t, NT + t, ...: with one element per lane (adamw_dev_kernel's loop) the
    // bytes in flight, 32 waves x 64 lanes x 16 B per CU, just cover HBM's latency; a full chunk issues all its 4 * U loads first.
    constexpr int U = 4;
    int64_t c0 = (int64_t)blockIdx.x * (U * NT);                 // first element of this block's current chunk
    if (c0 >= n) return;
    int r = 0;
    for (int hi = n_runs - 1; r < hi;) {                         // last run whose begin <= c0
        const int mid = (r + hi + 1) >> 1;
        if (runs[3 * mid] <= c0) r = mid; else hi = mid - 1;
    }
    int64_t r_end = runs[3 * r + 1];
    int r_grp = (int)runs[3 * r + 2];
    int cur = -1;
    float lr_bc1 = 0.f, b1 = 0.f, b2 = 0.f, eps = 1.f, decay = 1.f, inv_sqrt_bc2 = 0.f;
    // A lane that walks the table waits for its table read with vmcnt(0), which also drains every store issued before: so a
    // chunk's loads go out first, then all its lookups, then the updates and their stores (lookup in front of the loads was
    // measured: +12 %, the previous chunk's stores had to land before anything new was in flight).
    auto group_of = [&](int64_t i) {
        int rt = r, grp = r_grp;
        for (int64_t et = r_end; i >= et && rt + 1 < n_runs;) {  // only in a chunk that a run boundary crosses
            ++rt;
            et = runs[3 * rt + 1];
            grp = (int)runs[3 * rt + 2];
        }
        return grp;
    };
    auto update = [&](int64_t i, int grp, float g_raw, float p_old, float m_old, float v_old) {
        if (grp != cur) {
            cur = grp;
            const float* h = gh + 8 * min(max(grp, 0), n_groups - 1);
            lr_bc1 = h[0], b1 = h[1], b2 = h[2], eps = h[3], decay = h[4], inv_sqrt_bc2 = h[5];
        }
        const float gi = g_raw * coef;
        const float mi = __builtin_fmaf(1.f - b1, gi, b1 * m_old);
        const float vi = b2 * v_old + ((1.f - b2) * gi) * gi;
        const float denom = __builtin_fmaf(sqrtf(vi), inv_sqrt_bc2, eps);
        p[i] = decay * p_old - (lr_bc1 * mi) / denom;
        m[i] = mi;
        v[i] = vi;
    };
    for (; c0 < n; c0 += (int64_t)gridDim.x * (U * NT)) {
        while (c0 >= r_end && r + 1 < n_runs) {
            ++r;
            r_end = runs[3 * r + 1];
            r_grp = (int)runs[3 * r + 2];
        }
        const int64_t i0 = c0 + threadIdx.x;
        if (c0 + U * NT <= n) {                                  // a full chunk (uniform): no bounds test on the loads
            float g_raw[U], p_old[U], m_old[U], v_old[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                g_raw[u] = g[i0 + u * NT];
                p_old[u] = p[i0 + u * NT];
                m_old[u] = m[i0 + u * NT];
                v_old[u] = v[i0 + u * NT];
            }
            int grp[U];
#pragma unroll
            for (int u = 0; u < U; ++u) grp[u] = group_of(i0 + u * NT);
#pragma unroll
            for (int u = 0; u < U; ++u) update(i0 + u * NT, grp[u], g_raw[u], p_old[u], m_old[u], v_old[u]);
        } else {                                                 // the buffer's last, partial chunk
            for (int u = 0; u < U; ++u) {
                const int64_t i = i0 + u * NT;
                if (i < n) update(i, group_of(i), g[i], p[i], m[i], v[i]);
            }
        }
    }
}
__global__ void adamw_groups_advance_kernel(float* hyper) {
    if (threadIdx.x == 0 && blockIdx.x == 0) hyper[1] += 1.f;
}

__global__ void loss_scale_update_kernel(float* __restrict__ state, const double* __restrict__ sumsq, float growth, float backoff,
                                         int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double ss = *sumsq;
    if (step_overflowed(ss)) {
        state[0] = fmaxf(state[0] * backoff, 1.f);
        state[1] = 0.f;
    } else {
        state[2] += 1.f;
        state[1] += 1.f;
        if (state[1] >= (float)interval) {
            state[0] = fminf(state[0] * growth, 16777216.f);
            state[1] = 0.f;
        }
    }
}

// Exponential moving average of the weights, one sweep behind the AdamW kernels: ema[i] = d * ema[i] + (1 - d) * p[i], written
// as one rounded subtraction and one fma.  state = f32[8] {decay, warmup, every, steps seen, updates done, reserved x 3}; the two
// counts are exact up to 2^24 and are bumped by ema_advance_kernel AFTER the sweep, so every block reads the old ones.  sumsq
// (optional): the step this sweep follows was skipped where step_overflowed says so -- the predicate of the AdamW kernels and of
// loss_scale_update_kernel on the same *sumsq -- and then nothing is touched (uniform over the grid).  Update number k uses
// d = min(decay, (1 + k) / (warmup + k)) (warmup <= 0: decay), derived in double and rounded once as the bias corrections of
// adamw_dev_kernel are.  ema_due / ema_decay are the one definition for the sweep and the count kernel.
__device__ __forceinline__ bool ema_due(const float* __restrict__ state) {
    const double every = fmax((double)state[2], 1.0);
    return fmod((double)state[3] + 1.0, every) == 0.0;
}
__device__ __forceinline__ float ema_decay(const float* __restrict__ state) {
    const double decay = (double)state[0], warmup = (double)state[1], k = (double)state[4] + 1.0;
    return (float)(warmup > 0.0 ? fmin(decay, (1.0 + k) / (warmup + k)) : decay);
}
constexpr int EMA_U = 4;                                         // loads in flight per lane and stream, as adamw_groups_kernel's U
constexpr int EMA_GRID_CAP = 2048;
__global__ void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n, const double* __restrict__ sumsq,
                                  const float* __restrict__ state) {
#pragma clang fp contract(off)
    if (sumsq && step_overflowed(*sumsq)) return;
    if (!ema_due(state)) return;
    const float d = ema_decay(state);
    constexpr int U = EMA_U;
    for (int64_t c0 = (int64_t)blockIdx.x * (U * NT); c0 < n; c0 += (int64_t)gridDim.x * (U * NT)) {
        const int64_t i0 = c0 + threadIdx.x;
        if (c0 + U * NT <= n) {                                  // a full chunk (uniform): no bounds test on the loads
            float e[U], w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                e[u] = ema[i0 + u * NT];
                w[u] = p[i0 + u * NT];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) ema[i0 + u * NT] = __builtin_fmaf(d, e[u] - w[u], w[u]);
        } else {                                                 // the buffer's last, partial chunk
            for (int u = 0; u < U; ++u) {
                const int64_t i = i0 + u * NT;
                if (i < n) {
                    const float w = p[i];
                    ema[i] = __builtin_fmaf(d, ema[i] - w, w);
                }
            }
        }
    }
}
__global__ void ema_advance_kernel(float* __restrict__ state, const double* __restrict__ sumsq) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (sumsq && step_overflowed(*sumsq)) return;
    const bool due = ema_due(state);
    state[3] += 1.f;
    if (due) state[4] += 1.f;
}

// a <-> b, element for element, the chunked walk of ema_update_kernel: the caller has checked that the ranges are disjoint
__global__ void swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n) {
    constexpr int U = EMA_U;
    for (int64_t c0 = (int64_t)blockIdx.x * (U * NT); c0 < n; c0 += (int64_t)gridDim.x * (U * NT)) {
        const int64_t i0 = c0 + threadIdx.x;
        if (c0 + U * NT <= n) {
            float x[U], y[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                x[u] = a[i0 + u * NT];
                y[u] = b[i0 + u * NT];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                a[i0 + u * NT] = y[u];
                b[i0 + u * NT] = x[u];
            }
        } else {
            for (int u = 0; u < U; ++u) {
                const int64_t i = i0 + u * NT;
                if (i < n) {
                    const float x = a[i], y = b[i];
                    a[i] = y;
                    b[i] = x;
                }
            }
        }
    }
}

// NPZSequenceDataset.__getitem__ for a batch (train/unet.py:273-304): mask from RAW channel 0 (> 1.1) before scaling,
// x / norm_const, y clipped -> asinh(y / scale) -> [-1, 1]
__global__ void dataset_transform_kernel(const float* __restrict__ xr, const float* __restrict__ yr, float* __restrict__ x,
                                         float* __restrict__ y, float* __restrict__ mask, int64_t total, FastDiv dHW, int C, float inv_norm,
                                         float min_vel, float max_vel, int clip, float inv_yscale, float tmin, float inv_trange) {
    const int HW = dHW.d;
    for (int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NT) {
        const uint32_t f = fdiv((uint32_t)idx, dHW);               // frame
        const uint32_t pix = (uint32_t)idx - f * HW;
        const float* xf = xr + (int64_t)f * C * HW + pix;
        mask[idx] = xf[0] > 1.1f ? 1.f : 0.f;
        for (int c = 0; c < C; ++c) x[(int64_t)f * C * HW + (int64_t)c * HW + pix] = xf[(int64_t)c * HW] * inv_norm;
        float v = yr[idx];
        if (clip) v = fminf(fmaxf(v, min_vel), max_vel);
        y[idx] = 2.f * (asinhf(v * inv_yscale) - tmin) * inv_trange - 1.f;
    }
}

// V consecutive floats as one access: V = 4 is a 16-byte load / store, V = 1 the scalar path
template <int V>
__device__ __forceinline__ void load_px(const float* __restrict__ p, float (&r)[V]) {
    if constexpr (V == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = v[k];
    } else {
        r[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void store_px(float* __restrict__ p, const float (&r)[V]) {
    if constexpr (V == 4) {
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = r[k];
        *reinterpret_cast<f32x4*>(p) = v;
    } else {
        *p = r[0];
    }
}

// NPZSequenceDataset.__getitem__ for the sequences idx[0 .. n_out) of a RAW dataset resident on the device: the arithmetic of
// dataset_transform_kernel (plus the two other target transforms), the source frame found through the index vector.
// A block iteration is one CHUNK = NT work items (V pixels each) of ONE output frame, so the sequence index is uniform: it is
// read once per chunk (a scalar load), clamped into [0, n_seq) -- never a wild read -- and every lane's loads go to a clamped
// address unconditionally ("Branch-free loads"); lanes past the end of the frame only skip their stores.
// CT: the channel count when it is known at compile time (2: all C + 1 loads are issued before the first store), 0 = runtime C.
template <int V, int CT>
__global__ __launch_bounds__(NT) void dataset_gather_transform_kernel(
        const float* __restrict__ xa, const float* __restrict__ ya, const int64_t* __restrict__ idx, int64_t n_seq, int n_chunks,
        FastDiv dCpf, FastDiv dT, int Crt, int HW, float* __restrict__ x, float* __restrict__ y, float* __restrict__ mask, int transform,
        float inv_norm, float min_vel, float max_vel, int clip, float inv_yscale, float tmin, float inv_trange) {
    const int C = CT > 0 ? CT : Crt;
    const int per = HW / V;                                         // work items per frame
    const int cpf = (int)dCpf.d, T = (int)dT.d;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t f = fdiv((uint32_t)chunk, dCpf);             // output frame = o * T + t
        const uint32_t o = fdiv(f, dT);                             // output sequence
        int64_t row = idx ? idx[o] : (int64_t)o;
        row = row < 0 ? 0 : (row >= n_seq ? n_seq - 1 : row);
        const int64_t sf = row * T + (int64_t)(f - o * (uint32_t)T);   // source frame
        const int q = (chunk - (int)f * cpf) * NT + (int)threadIdx.x;
        const bool live = q < per;
        const int px = (live ? q : per - 1) * V;
        const float* xs = xa + sf * C * HW + px;
        float* xd = x + (int64_t)f * C * HW + px;
        const int64_t od = (int64_t)f * HW + px;
        float v[V], c0[V], m[V];
        load_px<V>(ya + sf * HW + px, v);
        load_px<V>(xs, c0);
        if constexpr (CT > 0) {
            float cc[CT > 1 ? CT - 1 : 1][V];
#pragma unroll
            for (int c = 1; c < CT; ++c) load_px<V>(xs + (int64_t)c * HW, cc[c - 1]);
            if (live) {
#pragma unroll
                for (int c = 1; c < CT; ++c) {
#pragma unroll
                    for (int k = 0; k < V; ++k) cc[c - 1][k] *= inv_norm;
                    store_px<V>(xd + (int64_t)c * HW, cc[c - 1]);
                }
            }
        } else {
            for (int c = 1; c < C; ++c) {
                float r[V];
                load_px<V>(xs + (int64_t)c * HW, r);
#pragma unroll
                for (int k = 0; k < V; ++k) r[k] *= inv_norm;
                if (live) store_px<V>(xd + (int64_t)c * HW, r);
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            m[k] = c0[k] > 1.1f ? 1.f : 0.f;
            c0[k] *= inv_norm;
            float w = v[k];
            if (clip) w = fminf(fmaxf(w, min_vel), max_vel);
            v[k] = 2.f * (target_fwd(w, transform, inv_yscale) - tmin) * inv_trange - 1.f;
        }
        if (live) {
            store_px<V>(xd, c0);
            store_px<V>(mask + od, m);
            store_px<V>(y + od, v);
        }
    }
}

// Epoch metrics of main.py:114-142 as running sums: de-normalise (train/unet.py:316-319) prediction and target,
// d = pred - target, sums += (sum |d| m, sum d^2 m, sum d m, sum m).  ORDERED: sums is the partial buffer [gridDim.x][4], no atomics
template <bool ORDERED>
__global__ void metric_sums_kernel(const float* __restrict__ yp, const float* __restrict__ y, const float* __restrict__ mask,
                                   double* __restrict__ sums, int64_t n, float yscale, float tmin, float trange) {
    __shared__ double red[16];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const float a = sinhf((yp[i] + 1.f) * 0.5f * trange + tmin) * yscale;
        const float b = sinhf((y[i] + 1.f) * 0.5f * trange + tmin) * yscale;
        const float m = mask ? (mask[i] != 0.f ? 1.f : 0.f) : 1.f;
        const double d = (double)(a - b);
        acc[0] += fabs(d) * m;
        acc[1] += d * d * m;
        acc[2] += d * m;
        acc[3] += m;
    }
    if constexpr (ORDERED) {
        block_sum_store<4>(acc, red, sums + (int64_t)blockIdx.x * 4);
    } else {
        block_sum<4>(acc, red);
        if (threadIdx.x == 0)
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(sums + k, acc[k]);
    }
}

// Stage 2 of the ordered f64 reductions: thread c owns output column c and adds the `rows` block partials of that column strictly
// in row order, out[c] = (accumulate ? out[c] : 0) + p[0][c] + p[1][c] + ... (eight loads in flight, one dependent chain of adds).
__global__ __launch_bounds__(64) void ordered_sum_f64_kernel(const double* __restrict__ p, int rows, int cols, double* __restrict__ out,
                                                            int accumulate) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= cols) return;
    double acc = accumulate ? out[c] : 0.0;
    const double* q = p + c;
    int r = 0;
    for (; r + 8 <= rows; r += 8) {
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = q[(int64_t)(r + u) * cols];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += t[u];
    }
    for (; r < rows; ++r) acc += q[(int64_t)r * cols];
    out[c] = acc;
}

int grid_for(int64_t items, int cap) {
    int64_t b = (items + NT - 1) / NT;
    if (b > cap) b = cap;
    return (int)(b < 1 ? 1 : b);
}
constexpr int ORDERED_ROWS_CAP = 1024;          // = the grids of the atomic forms: the producers are the same launches

}  // namespace

extern "C" int32_t uclstm_loss_fwd(const float* y_pred, const float* y, const float* mask, double* sums, int64_t planes, int32_t H,
                                   int32_t W, void* stream) {
    if (!y_pred || !y || !sums || planes <= 0 || H <= 0 || W <= 0) return UCLSTM_E_BADARG;
    const int64_t total = planes * H * W;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(loss_fwd_kernel<false>, dim3(grid_for(total, 1024)), dim3(NT), 0, (hipStream_t)stream, y_pred, y, mask, sums, total,
                       make_fastdiv(H * W), make_fastdiv(W), H, W);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_loss_bwd(const float* y_pred, const float* y, const float* mask, const float* coefs, float* grad,
                                   int64_t planes, int32_t H, int32_t W, void* stream) {
    if (!y_pred || !y || !grad || !coefs || planes <= 0 || H <= 0 || W <= 0) return UCLSTM_E_BADARG;
    const int64_t total = planes * H * W;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(loss_bwd_kernel, dim3(grid_for(total, 2048)), dim3(NT), 0, (hipStream_t)stream, y_pred, y, mask, coefs, grad,
                       total, make_fastdiv(H * W), make_fastdiv(W), H, W);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_sumsq(const float* g, int64_t n, double* out, void* stream) {
    if (!g || !out || n <= 0 || ((uintptr_t)g % 16)) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(sumsq_kernel<false>, dim3(grid_for((n + 3) / 4, 1024)), dim3(NT), 0, (hipStream_t)stream, g, n, out);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_adamw_step(float* p, float* m, float* v, const float* g, int64_t n, const double* sumsq, float max_norm,
                                     float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream) {
    if (!p || !m || !v || !g || n <= 0 || step < 1) return UCLSTM_E_BADARG;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    UCLSTM_LAUNCH(adamw_kernel, dim3(grid_for(n, 2048)), dim3(NT), 0, (hipStream_t)stream, p, m, v, g, n, sumsq, max_norm, lr, beta1,
                       beta2, eps, weight_decay, (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2)));
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_adamw_step_dev(float* p, float* m, float* v, const float* g, int64_t n, const double* sumsq, float* hyper,
                                         void* stream) {
    if (!p || !m || !v || !g || n <= 0 || !hyper || ((uintptr_t)hyper % 16)) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(adamw_dev_kernel, dim3(grid_for(n, 2048)), dim3(NT), 0, (hipStream_t)stream, p, m, v, g, n, sumsq, (const float*)hyper);
    UCLSTM_LAUNCH(adamw_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hyper);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_adamw_step_scaled(float* p, float* m, float* v, const float* g, int64_t n, const double* sumsq, float max_norm,
                                            float lr, float beta1, float beta2, float eps, float weight_decay, const float* scale_state,
                                            void* stream) {
    if (!p || !m || !v || !g || n <= 0 || !sumsq || !scale_state) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(adamw_scaled_kernel, dim3(grid_for(n, 2048)), dim3(NT), 0, (hipStream_t)stream, p, m, v, g, n, sumsq, max_norm, lr, beta1,
                  beta2, eps, weight_decay, scale_state);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_adamw_step_groups(float* p, float* m, float* v, const float* g, int64_t n, const double* sumsq,
                                            const int64_t* runs, int32_t n_runs, float* hyper, int32_t n_groups,
                                            const float* scale_state, void* stream) {
    if (!p || !m || !v || !g || n <= 0 || !runs || n_runs <= 0 || !hyper || ((uintptr_t)hyper % 16) || n_groups <= 0 ||
        n_groups > 1024 || (scale_state && !sumsq))
        return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(adamw_groups_kernel, dim3(grid_for((n + 3) / 4, 2048)), dim3(NT), (size_t)n_groups * 8 * sizeof(float), (hipStream_t)stream, p, m,
                  v, g, n, sumsq, runs, n_runs, (const float*)hyper, n_groups, scale_state);
    // with scale_state the step count is scale_state[2], advanced by uclstm_loss_scale_update
    if (!scale_state) UCLSTM_LAUNCH(adamw_groups_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hyper);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_loss_scale_update(float* scale_state, const double* sumsq, float growth, float backoff, int32_t interval,
                                            void* stream) {
    if (!scale_state || !sumsq || growth < 1.f || backoff <= 0.f || backoff > 1.f || interval < 1) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scale_state, sumsq, growth, backoff, interval);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_ema_update(float* ema, const float* p, int64_t n, const double* sumsq, float* ema_state, void* stream) {
    if (!ema || !p || n <= 0 || !ema_state) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(ema_update_kernel, dim3(grid_for((n + EMA_U - 1) / EMA_U, EMA_GRID_CAP)), dim3(NT), 0, (hipStream_t)stream, ema, p, n, sumsq,
                  (const float*)ema_state);
    UCLSTM_LAUNCH(ema_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ema_state, sumsq);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_swap_f32(float* a, float* b, int64_t n, void* stream) {
    if (!a || !b || n < 0 || a == b) return UCLSTM_E_BADARG;
    if (n > (int64_t)(UINTPTR_MAX / sizeof(float))) return UCLSTM_E_BADARG;
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
    if (ua < ub ? ub - ua < bytes : ua - ub < bytes) return UCLSTM_E_BADARG;          // the ranges overlap
    if (n == 0) return UCLSTM_OK;
    UCLSTM_LAUNCH(swap_f32_kernel, dim3(grid_for((n + EMA_U - 1) / EMA_U, EMA_GRID_CAP)), dim3(NT), 0, (hipStream_t)stream, a, b, n);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_dataset_transform(const float* x_raw, const float* y_raw, float* x, float* y, float* mask, int64_t n_frames,
                                            int32_t C, int32_t HW, float norm_const, float min_vel, float max_vel, int32_t clip,
                                            float y_scale, float trans_min, float trans_max, void* stream) {
    if (!x_raw || !y_raw || !x || !y || !mask || n_frames <= 0 || C <= 0 || HW <= 0 || norm_const == 0.f || y_scale == 0.f ||
        trans_max == trans_min)
        return UCLSTM_E_BADARG;
    const int64_t total = n_frames * HW;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(dataset_transform_kernel, dim3(grid_for(total, 2048)), dim3(NT), 0, (hipStream_t)stream, x_raw, y_raw, x, y, mask, total,
                  make_fastdiv(HW), C, 1.0f / norm_const, min_vel, max_vel, clip, 1.0f / y_scale, trans_min,
                  1.0f / (trans_max - trans_min));
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_dataset_gather_transform(const float* x_all, const float* y_all, const int64_t* idx, int64_t n_seq, int64_t n_out,
                                                   int32_t T, int32_t C, int32_t HW, float* x, float* y, float* mask, int32_t transform,
                                                   float norm_const, float min_vel, float max_vel, int32_t clip, float y_scale,
                                                   float trans_min, float trans_max, void* stream) {
    if (!x_all || !y_all || !x || !y || !mask || n_seq <= 0 || n_out <= 0 || T <= 0 || C <= 0 || HW <= 0 || transform < 0 ||
        transform > 2 || norm_const == 0.f || trans_max == trans_min || (transform != 0 && !(y_scale > 0.f)) || (!idx && n_out > n_seq))
        return UCLSTM_E_BADARG;
    const int64_t frame_px = (int64_t)T * HW;                                  // < 2^62
    if (n_out > (((int64_t)1 << 31) - 1) / frame_px) return UCLSTM_E_BADARG;    // n_out * T * HW >= 2^31
    const bool vec = HW % 4 == 0 && (((uintptr_t)x_all | (uintptr_t)y_all | (uintptr_t)x | (uintptr_t)y | (uintptr_t)mask) % 16) == 0;
    const int per = vec ? HW / 4 : HW;                                         // work items per frame
    const int cpf = (per + NT - 1) / NT;                                       // chunks per frame
    const int64_t n_chunks = n_out * T * cpf;                                  // <= n_out * T * HW < 2^31
    const int grid = (int)(n_chunks < 2048 ? n_chunks : 2048);
    const float inv_yscale = transform != 0 ? 1.0f / y_scale : 1.0f;
#define UCLSTM_GATHER_LAUNCH(V, CT)                                                                                                      \
    UCLSTM_LAUNCH((dataset_gather_transform_kernel<V, CT>), dim3(grid), dim3(NT), 0, (hipStream_t)stream, x_all, y_all, idx, n_seq,     \
                  (int)n_chunks, make_fastdiv(cpf), make_fastdiv(T), C, HW, x, y, mask, transform, 1.0f / norm_const, min_vel, max_vel, \
                  clip, inv_yscale, trans_min, 1.0f / (trans_max - trans_min))
    if (vec) {
        if (C == 2) UCLSTM_GATHER_LAUNCH(4, 2);
        else UCLSTM_GATHER_LAUNCH(4, 0);
    } else {
        if (C == 2) UCLSTM_GATHER_LAUNCH(1, 2);
        else UCLSTM_GATHER_LAUNCH(1, 0);
    }
#undef UCLSTM_GATHER_LAUNCH
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_metric_sums(const float* y_pred, const float* y, const float* mask, double* sums, int64_t n, float y_scale,
                                      float trans_min, float trans_max, void* stream) {
    if (!y_pred || !y || !sums || n <= 0) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(metric_sums_kernel<false>, dim3(grid_for(n, 1024)), dim3(NT), 0, (hipStream_t)stream, y_pred, y, mask, sums, n, y_scale,
                  trans_min, trans_max - trans_min);
    return UCLSTM_OK;
}

// ---- ordered (deterministic-mode) forms of the three f64 reductions: producer rows + ordered_sum_f64_kernel ----
extern "C" int64_t uclstm_loss_fwd_ordered_rows(int64_t planes, int32_t H, int32_t W) {
    if (planes <= 0 || H <= 0 || W <= 0 || planes * H * W >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    return grid_for(planes * H * W, ORDERED_ROWS_CAP);
}
extern "C" int32_t uclstm_loss_fwd_ordered(const float* y_pred, const float* y, const float* mask, double* partials, double* sums,
                                           int32_t accumulate, int64_t planes, int32_t H, int32_t W, void* stream) {
    if (!y_pred || !y || !partials || !sums || planes <= 0 || H <= 0 || W <= 0) return UCLSTM_E_BADARG;
    const int64_t total = planes * H * W;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    const int rows = grid_for(total, ORDERED_ROWS_CAP);
    UCLSTM_LAUNCH(loss_fwd_kernel<true>, dim3(rows), dim3(NT), 0, (hipStream_t)stream, y_pred, y, mask, partials, total, make_fastdiv(H * W),
                  make_fastdiv(W), H, W);
    UCLSTM_LAUNCH(ordered_sum_f64_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, rows, 4, sums, accumulate);
    return UCLSTM_OK;
}

extern "C" int64_t uclstm_sumsq_ordered_rows(int64_t n) {
    if (n <= 0) return UCLSTM_E_BADARG;
    return grid_for((n + 3) / 4, ORDERED_ROWS_CAP);
}
extern "C" int32_t uclstm_sumsq_ordered(const float* g, int64_t n, double* partials, double* out, int32_t accumulate, void* stream) {
    if (!g || !partials || !out || n <= 0 || ((uintptr_t)g % 16)) return UCLSTM_E_BADARG;
    const int rows = grid_for((n + 3) / 4, ORDERED_ROWS_CAP);
    UCLSTM_LAUNCH(sumsq_kernel<true>, dim3(rows), dim3(NT), 0, (hipStream_t)stream, g, n, partials);
    UCLSTM_LAUNCH(ordered_sum_f64_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, rows, 1, out, accumulate);
    return UCLSTM_OK;
}

extern "C" int64_t uclstm_metric_sums_ordered_rows(int64_t n) {
    if (n <= 0) return UCLSTM_E_BADARG;
    return grid_for(n, ORDERED_ROWS_CAP);
}
extern "C" int32_t uclstm_metric_sums_ordered(const float* y_pred, const float* y, const float* mask, double* partials, double* sums,
                                              int32_t accumulate, int64_t n, float y_scale, float trans_min, float trans_max, void* stream) {
    if (!y_pred || !y || !partials || !sums || n <= 0) return UCLSTM_E_BADARG;
    const int rows = grid_for(n, ORDERED_ROWS_CAP);
    UCLSTM_LAUNCH(metric_sums_kernel<true>, dim3(rows), dim3(NT), 0, (hipStream_t)stream, y_pred, y, mask, partials, n, y_scale, trans_min,
                  trans_max - trans_min);
    UCLSTM_LAUNCH(ordered_sum_f64_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, rows, 4, sums, accumulate);
    return UCLSTM_OK;
}

// ---- the metric sums per target channel (vector targets): ordered form only ----
namespace {

struct MetricConsts {                               // uclstm_target_consts [Cy] as a kernel argument
    float yscale[UCLSTM_VEC_MAX], tmin[UCLSTM_VEC_MAX], trange[UCLSTM_VEC_MAX];
};

__device__ __forceinline__ float metric_denorm(float v, int transform, float yscale, float tmin, float trange) {
    const float yt = (v + 1.f) * 0.5f * trange + tmin;          // as metric_sums_kernel
    if (transform == 1) return sinhf(yt) * yscale;
    if (transform == 2) return sgn(yt) * expm1f(fabsf(yt)) * yscale;
    return yt;
}

// An item is one pixel of one frame: its mask is read once and serves the CY channels of that pixel.  The block's row of the
// partial buffer is [CY][4]; no atomics.
template <int CY>
__global__ __launch_bounds__(NT) void metric_sums_vec_kernel(const float* __restrict__ yp, const float* __restrict__ y,
                                                             const float* __restrict__ mask, double* __restrict__ partials, int64_t items,
                                                             FastDiv dHW, int transform, MetricConsts k) {
    __shared__ double red[4 * CY * 4];
    double acc[CY * 4];
#pragma unroll
    for (int u = 0; u < CY * 4; ++u) acc[u] = 0.0;
    const int HW = (int)dHW.d;
    for (int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x; q < items; q += (int64_t)gridDim.x * NT) {
        const uint32_t f = fdiv((uint32_t)q, dHW);
        const int64_t base = q + (int64_t)f * (CY - 1) * HW;     // element of channel 0: (f * CY) * HW + pixel
        const float m = mask ? (mask[q] != 0.f ? 1.f : 0.f) : 1.f;
#pragma unroll
        for (int c = 0; c < CY; ++c) {
            const float a = metric_denorm(yp[base + (int64_t)c * HW], transform, k.yscale[c], k.tmin[c], k.trange[c]);
            const float b = metric_denorm(y[base + (int64_t)c * HW], transform, k.yscale[c], k.tmin[c], k.trange[c]);
            const double d = (double)(a - b);
            acc[c * 4 + 0] += fabs(d) * m;
            acc[c * 4 + 1] += d * d * m;
            acc[c * 4 + 2] += d * m;
            acc[c * 4 + 3] += m;
        }
    }
    block_sum_store<CY * 4>(acc, red, partials + (int64_t)blockIdx.x * (CY * 4));
}

}  // namespace

extern "C" int64_t uclstm_metric_sums_vec_rows(int64_t n_frames, int32_t Cy, int32_t HW) {
    if (n_frames <= 0 || Cy < 1 || Cy > UCLSTM_VEC_MAX || HW <= 0 || n_frames > (((int64_t)1 << 31) - 1) / ((int64_t)Cy * HW))
        return UCLSTM_E_BADARG;
    return grid_for(n_frames * HW, ORDERED_ROWS_CAP);
}
extern "C" int32_t uclstm_metric_sums_vec(const float* y_pred, const float* y, const float* mask, double* partials, double* sums,
                                          int32_t accumulate, int64_t n_frames, int32_t Cy, int32_t HW, int32_t transform,
                                          const uclstm_target_consts* consts, void* stream) {
    if (!y_pred || !y || !partials || !sums || !consts || transform < 0 || transform > 2) return UCLSTM_E_BADARG;
    const int64_t rows64 = uclstm_metric_sums_vec_rows(n_frames, Cy, HW);
    if (rows64 < 1) return UCLSTM_E_BADARG;
    const int rows = (int)rows64;
    MetricConsts k;
    for (int c = 0; c < UCLSTM_VEC_MAX; ++c) {
        const uclstm_target_consts& t = consts[c < Cy ? c : 0];
        k.yscale[c] = t.y_scale;
        k.tmin[c] = t.trans_min;
        k.trange[c] = t.trans_max - t.trans_min;
    }
    const int64_t items = n_frames * HW;
#define UCLSTM_METRIC_VEC_LAUNCH(CY)                                                                                                   \
    UCLSTM_LAUNCH(metric_sums_vec_kernel<CY>, dim3(rows), dim3(NT), 0, (hipStream_t)stream, y_pred, y, mask, partials, items,           \
                  make_fastdiv(HW), transform, k)
    switch (Cy) {
        case 1: UCLSTM_METRIC_VEC_LAUNCH(1); break;
        case 2: UCLSTM_METRIC_VEC_LAUNCH(2); break;
        case 3: UCLSTM_METRIC_VEC_LAUNCH(3); break;
        default: UCLSTM_METRIC_VEC_LAUNCH(4); break;
    }
#undef UCLSTM_METRIC_VEC_LAUNCH
    UCLSTM_LAUNCH(ordered_sum_f64_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, rows, Cy * 4, sums, accumulate);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_ordered_sum_f64(const double* partials, int32_t rows, int32_t cols, double* out, int32_t accumulate, void* stream) {
    if (!partials || !out || rows <= 0 || cols <= 0) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(ordered_sum_f64_kernel, dim3((cols + 63) / 64), dim3(64), 0, (hipStream_t)stream, partials, rows, cols, out, accumulate);
    return UCLSTM_OK;
}

// ---- the loss with its point term and weight as parameters (uclstm_loss_spec) ----
// The kernels above with the spec as template parameters: POINT (L1 / L2 / Huber), POWER of the weight (1..4), GRAD (the gradient
// term exists) and V, the elements one thread takes from a row (4 with 16-byte loads when the row length allows, else 1).  The
// host picks the instance, so no element branches on the spec.  Without the gradient term the planes are one flat array.
namespace {

enum { PW_OFF = 0, PW_MASK = 1, PW_NO_MASK = 2 };   // plane weights: none / with a mask / with mask == NULL
constexpr int SPEC_GRID_CAP_V4 = 512;           // blocks of the V = 4 instances (fwd atomic form and bwd): 16 bytes per stream and thread

template <int V>
__device__ __forceinline__ void load_v(const float* __restrict__ p, float (&o)[V]) {
    if constexpr (V == 4) {
        const float4 t = *(const float4*)p;
        o[0] = t.x, o[1] = t.y, o[2] = t.z, o[3] = t.w;
    } else {
        o[0] = *p;
    }
}

template <int POWER>
__device__ __forceinline__ float spec_weight(float b, float gain) {
    const float ab = fabsf(b);
    if constexpr (POWER == 1) return 1.f + gain * ab;
    else if constexpr (POWER == 2) return 1.f + gain * ab * ab;
    else if constexpr (POWER == 3) return 1.f + gain * ab * ab * ab;          // main.py:38 at gain 4
    else return 1.f + gain * ab * ab * ab * ab;
}

template <int POINT>
__device__ __forceinline__ float spec_rho(float d, float delta) {
    if constexpr (POINT == UCLSTM_LOSS_POINT_L1) return fabsf(d);
    else if constexpr (POINT == UCLSTM_LOSS_POINT_L2) return d * d;
    else {
        const float ad = fabsf(d);
        return ad <= delta ? 0.5f * d * d : delta * (ad - 0.5f * delta);
    }
}

template <int POINT>
__device__ __forceinline__ float spec_drho(float d, float delta) {
    if constexpr (POINT == UCLSTM_LOSS_POINT_L1) return sgn(d);
    else if constexpr (POINT == UCLSTM_LOSS_POINT_L2) return 2.f * d;
    else return fminf(fmaxf(d, -delta), delta);
}

// The mask of the V elements at idx when it is BROADCAST over channels (the _bc entry points): plane p reads mask plane p / mask_div.
// dPl divides by the H*W elements of a plane, dMd by mask_div.  Returns the pointer mk with mk[idx + j] = the mask of element idx + j
// for every j inside the plane of idx (the neighbours the backward kernel reads).  A group of V lies inside one plane with the
// gradient term (rows are a multiple of V long) or when H*W is a multiple of V; otherwise every element finds its own plane.
template <int V, bool GRAD>
__device__ __forceinline__ const float* load_mask_bc(const float* __restrict__ mask, int64_t idx, const FastDiv& dPl, const FastDiv& dMd,
                                                     float (&m)[V]) {
    const uint32_t pl = fdiv((uint32_t)idx, dPl);
    const float* mk = mask - (int64_t)(pl - fdiv(pl, dMd)) * dPl.d;
    if (GRAD || V == 1 || dPl.d % V == 0) {
        load_v<V>(mk + idx, m);
    } else {
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const uint32_t q = fdiv((uint32_t)(idx + u), dPl);
            m[u] = mask[idx + u - (int64_t)(q - fdiv(q, dMd)) * dPl.d];
        }
    }
    return mk;
}

// The plane weights of the V elements at idx (the _pw entry points): plane p has weight plane_w[p mod period], dPer divides by the
// period.  One plane per group under the conditions of load_mask_bc, otherwise every element finds its own plane.
template <int V, bool GRAD>
__device__ __forceinline__ void load_plane_w(const float* __restrict__ plane_w, int64_t idx, const FastDiv& dPl, const FastDiv& dPer,
                                             float (&q)[V]) {
    if (GRAD || V == 1 || dPl.d % V == 0) {
        const uint32_t pl = fdiv((uint32_t)idx, dPl);
        const float w = plane_w[pl - fdiv(pl, dPer) * dPer.d];
#pragma unroll
        for (int u = 0; u < V; ++u) q[u] = w;
    } else {
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const uint32_t pl = fdiv((uint32_t)(idx + u), dPl);
            q[u] = plane_w[pl - fdiv(pl, dPer) * dPer.d];
        }
    }
}

// items = total / V groups of V elements of one row; dHW / dW divide by the groups of a plane / of a row (GRAD only).
// sums as loss_fwd_kernel; without GRAD columns 2 and 3 are the zeros acc starts with.
// PW (the _pw entry points, always with BC): every term of the four sums is multiplied by the weight of its plane,
// plane_w[plane mod dPer.d].  mask may be NULL there, which is an instance of its own (PW_NO_MASK): a mask load under a run-time
// branch makes the loads issued before it wait at the join.  Without PW neither plane_w nor dPer is read.
template <int POINT, int POWER, bool GRAD, bool ORDERED, int V, bool BC = false, int PW = PW_OFF>
__global__ void loss_spec_fwd_kernel(const float* __restrict__ yp, const float* __restrict__ y, const float* __restrict__ mask,
                                     double* __restrict__ sums, int64_t items, FastDiv dHW, FastDiv dW, int H, int W, float delta,
                                     float gain, FastDiv dPl, FastDiv dMd, const float* __restrict__ plane_w, FastDiv dPer) {
    __shared__ double red[16];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    // PW_NO_MASK: a one the compiler does not see (mask is NULL), so that the multiplications by m stay, and with them the
    // contractions, and the bits, of the plain instances under a NULL mask
    [[maybe_unused]] const float no_mask = mask ? 0.f : 1.f;
    for (int64_t it = (int64_t)blockIdx.x * NT + threadIdx.x; it < items; it += (int64_t)gridDim.x * NT) {
        const int64_t idx = it * V;
        float a[V], b[V], m[V];
        [[maybe_unused]] float q[V];
        if constexpr (PW != PW_OFF) load_plane_w<V, GRAD>(plane_w, idx, dPl, dPer, q);     // issued with the loads of the planes, not after them
        load_v<V>(yp + idx, a);
        load_v<V>(y + idx, b);
        if constexpr (BC && PW != PW_NO_MASK) load_mask_bc<V, GRAD>(mask, idx, dPl, dMd, m);
        else if (!BC && mask) load_v<V>(mask + idx, m);
        else
#pragma unroll
            for (int u = 0; u < V; ++u) m[u] = PW == PW_NO_MASK ? no_mask : 1.f;
        if constexpr (PW != PW_OFF) {
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const float w = spec_weight<POWER>(b[u], gain);
                acc[0] += (double)(spec_rho<POINT>(a[u] - b[u], delta) * w * m[u] * q[u]);
                acc[1] += (double)(w * m[u] * q[u]);
                m[u] *= q[u];                                    // the gradient term below sums gd * (mc * q) and mc * q
            }
        } else {
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const float w = spec_weight<POWER>(b[u], gain);
                acc[0] += (double)(spec_rho<POINT>(a[u] - b[u], delta) * w * m[u]);
                acc[1] += (double)(w * m[u]);
            }
        }
        if constexpr (GRAD) {
            const uint32_t pl = fdiv((uint32_t)it, dHW);
            const uint32_t pix = (uint32_t)it - pl * dHW.d;
            const int i = (int)fdiv(pix, dW);
            const int j = ((int)pix - i * (int)dW.d) * V;
            if (i < H - 1) {                                     // main.py:57-62 crop
                float an[V], bn[V];
                load_v<V>(yp + idx + W, an);
                load_v<V>(y + idx + W, bn);
                const bool has_r = j + V < W;                    // the group's last element has a right neighbour
                const float ar = has_r ? yp[idx + V] : 0.f, br = has_r ? y[idx + V] : 0.f;
#pragma unroll
                for (int u = 0; u < V; ++u) {
                    if (u < V - 1 || has_r) {
                        const float axr = (u < V - 1) ? a[(u + 1) % V] : ar, bxr = (u < V - 1) ? b[(u + 1) % V] : br;
                        const float dxp = axr - a[u], dyp = an[u] - a[u];
                        const float dxg = bxr - b[u], dyg = bn[u] - b[u];
                        acc[2] += (double)((fabsf(dxp - dxg) + fabsf(dyp - dyg)) * m[u]);
                        acc[3] += (double)m[u];
                    }
                }
            }
        }
    }
    if constexpr (ORDERED) {
        block_sum_store<4>(acc, red, sums + (int64_t)blockIdx.x * 4);
    } else {
        block_sum<4>(acc, red);
        if (threadIdx.x == 0)
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(sums + k, acc[k]);
    }
}

// PW as in the forward kernel: every neighbour of the gradient term lies in the element's own plane, so the weighted gradient is the
// plain one times the weight of the plane.
template <int POINT, int POWER, bool GRAD, int V, bool BC = false, int PW = PW_OFF>
__global__ void loss_spec_bwd_kernel(const float* __restrict__ yp, const float* __restrict__ y, const float* __restrict__ mask,
                                     const float* __restrict__ coefs, float* __restrict__ grad, int64_t items, FastDiv dHW, FastDiv dW,
                                     int H, int W, float delta, float gain, FastDiv dPl, FastDiv dMd, const float* __restrict__ plane_w,
                                     FastDiv dPer) {
    const float c1 = coefs[0];
    float c2 = 0.f;
    if constexpr (GRAD) c2 = coefs[1];
    // PW_NO_MASK: a one the compiler does not see (mask is NULL), so that the multiplications by m stay, and with them the
    // contractions, and the bits, of the plain instances under a NULL mask
    [[maybe_unused]] const float no_mask = mask ? 0.f : 1.f;
    for (int64_t it = (int64_t)blockIdx.x * NT + threadIdx.x; it < items; it += (int64_t)gridDim.x * NT) {
        const int64_t idx = it * V;
        float a[V], b[V], m[V], g[V];
        [[maybe_unused]] float q[V];
        if constexpr (PW != PW_OFF) load_plane_w<V, GRAD>(plane_w, idx, dPl, dPer, q);     // issued with the loads of the planes, not after them
        load_v<V>(yp + idx, a);
        load_v<V>(y + idx, b);
        const float* mk = mask;                                  // BC: shifted so that mk + idx is the mask of this plane
        if constexpr (BC && PW != PW_NO_MASK) mk = load_mask_bc<V, GRAD>(mask, idx, dPl, dMd, m);
        else if (!BC && mask) load_v<V>(mask + idx, m);
        else
#pragma unroll
            for (int u = 0; u < V; ++u) m[u] = PW == PW_NO_MASK ? no_mask : 1.f;
#pragma unroll
        for (int u = 0; u < V; ++u) g[u] = c1 * spec_drho<POINT>(a[u] - b[u], delta) * spec_weight<POWER>(b[u], gain) * m[u];
        if constexpr (GRAD) {
            const uint32_t pl = fdiv((uint32_t)it, dHW);
            const uint32_t pix = (uint32_t)it - pl * dHW.d;
            const int i = (int)fdiv(pix, dW);
            const int j = ((int)pix - i * (int)dW.d) * V;
            float gg[V];
#pragma unroll
            for (int u = 0; u < V; ++u) gg[u] = 0.f;
            if (i < H - 1) {
                // cell (i,j) itself: -sx(i,j) - sy(i,j)
                float an[V], bn[V];
                load_v<V>(yp + idx + W, an);
                load_v<V>(y + idx + W, bn);
                const bool has_r = j + V < W;
                const float ar = has_r ? yp[idx + V] : 0.f, br = has_r ? y[idx + V] : 0.f;
#pragma unroll
                for (int u = 0; u < V; ++u) {
                    if (u < V - 1 || has_r) {
                        const float axr = (u < V - 1) ? a[(u + 1) % V] : ar, bxr = (u < V - 1) ? b[(u + 1) % V] : br;
                        const float sx = sgn((axr - a[u]) - (bxr - b[u]));
                        const float sy = sgn((an[u] - a[u]) - (bn[u] - b[u]));
                        gg[u] -= (sx + sy) * m[u];
                    }
                }
                // cell (i,j-1): +sx(i,j-1)
                const bool has_l = j >= 1;
                const float al = has_l ? yp[idx - 1] : 0.f, bl = has_l ? y[idx - 1] : 0.f;
                const float ml = (has_l && mask) ? mk[idx - 1] : 1.f;
#pragma unroll
                for (int u = 0; u < V; ++u) {
                    if (u > 0 || has_l) {
                        const float axl = (u > 0) ? a[(u + V - 1) % V] : al, bxl = (u > 0) ? b[(u + V - 1) % V] : bl;
                        const float mxl = (u > 0) ? m[(u + V - 1) % V] : ml;
                        gg[u] += sgn((a[u] - axl) - (b[u] - bxl)) * mxl;
                    }
                }
            }
            // cell (i-1,j): +sy(i-1,j)
            if (i >= 1) {
                float au[V], bu[V], mu[V];
                load_v<V>(yp + idx - W, au);
                load_v<V>(y + idx - W, bu);
                if (mask) load_v<V>(mk + idx - W, mu);
                else
#pragma unroll
                    for (int u = 0; u < V; ++u) mu[u] = 1.f;
#pragma unroll
                for (int u = 0; u < V; ++u)
                    if (j + u < W - 1) gg[u] += sgn((a[u] - au[u]) - (b[u] - bu[u])) * mu[u];
            }
#pragma unroll
            for (int u = 0; u < V; ++u) g[u] += c2 * gg[u];
        }
        if constexpr (PW != PW_OFF)
#pragma unroll
            for (int u = 0; u < V; ++u) g[u] *= q[u];
        if constexpr (V == 4) *(float4*)(grad + idx) = make_float4(g[0], g[1], g[2], g[3]);
        else grad[idx] = g[0];
    }
}

bool loss_spec_ok(const uclstm_loss_spec* s) {
    if (!s || s->point < UCLSTM_LOSS_POINT_L1 || s->point > UCLSTM_LOSS_POINT_HUBER || s->weight_power < 1 || s->weight_power > 4)
        return false;
    if (s->point == UCLSTM_LOSS_POINT_HUBER && !(s->delta > 0.f && s->delta <= FLT_MAX)) return false;
    return s->weight_gain >= 0.f && s->weight_gain <= FLT_MAX;               // false for NaN as well
}

// Calls f(point, power, grad, v) with integral constants for the spec's instance.
template <typename T, T X>
using ic = std::integral_constant<T, X>;
template <typename F>
int32_t loss_spec_dispatch(const uclstm_loss_spec* s, bool vec, F&& f) {
    auto on_v = [&](auto point, auto power, auto grad) { return vec ? f(point, power, grad, ic<int, 4>{}) : f(point, power, grad, ic<int, 1>{}); };
    auto on_grad = [&](auto point, auto power) { return s->grad_term ? on_v(point, power, ic<bool, true>{}) : on_v(point, power, ic<bool, false>{}); };
    auto on_power = [&](auto point) {
        switch (s->weight_power) {
            case 1: return on_grad(point, ic<int, 1>{});
            case 2: return on_grad(point, ic<int, 2>{});
            case 3: return on_grad(point, ic<int, 3>{});
            default: return on_grad(point, ic<int, 4>{});
        }
    };
    switch (s->point) {
        case UCLSTM_LOSS_POINT_L1: return on_power(ic<int, UCLSTM_LOSS_POINT_L1>{});
        case UCLSTM_LOSS_POINT_L2: return on_power(ic<int, UCLSTM_LOSS_POINT_L2>{});
        default: return on_power(ic<int, UCLSTM_LOSS_POINT_HUBER>{});
    }
}

// V = 4: every base 16-byte aligned and rows (with the gradient term) or the whole array (without) a multiple of four long
bool loss_spec_vec(const uclstm_loss_spec* s, int64_t total, int W, const void* p0, const void* p1, const void* p2, const void* p3) {
    const uintptr_t bases = (uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2 | (uintptr_t)p3;
    return bases % 16 == 0 && (s->grad_term ? W % 4 == 0 : total % 4 == 0);
}

// BC: the mask is broadcast over channels, plane p reads mask plane p / mask_div (the _bc entry points); the grids, and so the
// partition of the elements over blocks and threads, are those of the plain form.  PW: a weight per plane, plane_w[plane mod period]
// (the _pw entry points, on the broadcast-mask indexing whatever mask_div is); the same grids again.
template <bool ORDERED, bool BC = false, bool PW = false>
int32_t loss_spec_fwd_launch(const uclstm_loss_spec* s, const float* y_pred, const float* y, const float* mask, double* out, int64_t total,
                             int H, int W, int rows, hipStream_t stream, int mask_div = 1, const float* plane_w = nullptr,
                             int period = 1) {
    const bool vec = loss_spec_vec(s, total, W, y_pred, y, mask, nullptr);
    return loss_spec_dispatch(s, vec, [&](auto point, auto power, auto grad, auto v) -> int32_t {
        constexpr int V = decltype(v)::value;
        const int grid = ORDERED ? rows : grid_for(total / V, V == 4 ? SPEC_GRID_CAP_V4 : 1024);
        auto launch = [&](auto pw) -> int32_t {
            UCLSTM_LAUNCH((loss_spec_fwd_kernel<decltype(point)::value, decltype(power)::value, decltype(grad)::value, ORDERED, V, BC,
                                                decltype(pw)::value>),
                          dim3(grid), dim3(NT), 0, stream, y_pred, y, mask, out, total / V, make_fastdiv(H * (W / V)), make_fastdiv(W / V), H,
                          W, s->delta, s->weight_gain, make_fastdiv(H * W), make_fastdiv(mask_div), plane_w, make_fastdiv(period));
            return UCLSTM_OK;
        };
        if constexpr (!PW) return launch(ic<int, PW_OFF>{});
        else return mask ? launch(ic<int, PW_MASK>{}) : launch(ic<int, PW_NO_MASK>{});
    });
}

template <bool BC = false, bool PW = false>
int32_t loss_spec_bwd_launch(const uclstm_loss_spec* s, const float* y_pred, const float* y, const float* mask, const float* coefs,
                             float* grad, int64_t total, int H, int W, hipStream_t stream, int mask_div = 1,
                             const float* plane_w = nullptr, int period = 1) {
    const bool vec = loss_spec_vec(s, total, W, y_pred, y, mask, grad);
    return loss_spec_dispatch(s, vec, [&](auto point, auto power, auto grd, auto v) -> int32_t {
        constexpr int V = decltype(v)::value;
        auto launch = [&](auto pw) -> int32_t {
            UCLSTM_LAUNCH((loss_spec_bwd_kernel<decltype(point)::value, decltype(power)::value, decltype(grd)::value, V, BC, decltype(pw)::value>),
                          dim3(grid_for(total / V, V == 4 ? SPEC_GRID_CAP_V4 : 2048)), dim3(NT), 0, stream, y_pred, y, mask, coefs, grad,
                          total / V, make_fastdiv(H * (W / V)), make_fastdiv(W / V), H, W, s->delta, s->weight_gain, make_fastdiv(H * W),
                          make_fastdiv(mask_div), plane_w, make_fastdiv(period));
            return UCLSTM_OK;
        };
        if constexpr (!PW) return launch(ic<int, PW_OFF>{});
        else return mask ? launch(ic<int, PW_MASK>{}) : launch(ic<int, PW_NO_MASK>{});
    });
}

}  // namespace

extern "C" int32_t uclstm_loss_spec_fwd(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask, double* sums,
                                        int64_t planes, int32_t H, int32_t W, void* stream) {
    if (!loss_spec_ok(spec) || !y_pred || !y || !sums || planes <= 0 || H <= 0 || W <= 0) return UCLSTM_E_BADARG;
    const int64_t total = planes * H * W;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    return loss_spec_fwd_launch<false>(spec, y_pred, y, mask, sums, total, H, W, 0, (hipStream_t)stream);
}

extern "C" int32_t uclstm_loss_spec_fwd_ordered(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                                double* partials, double* sums, int32_t accumulate, int64_t planes, int32_t H, int32_t W,
                                                void* stream) {
    if (!loss_spec_ok(spec) || !y_pred || !y || !partials || !sums || planes <= 0 || H <= 0 || W <= 0) return UCLSTM_E_BADARG;
    const int64_t total = planes * H * W;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    const int rows = grid_for(total, ORDERED_ROWS_CAP);          // = uclstm_loss_fwd_ordered_rows, whatever V is
    const int32_t rc = loss_spec_fwd_launch<true>(spec, y_pred, y, mask, partials, total, H, W, rows, (hipStream_t)stream);
    if (rc != UCLSTM_OK) return rc;
    UCLSTM_LAUNCH(ordered_sum_f64_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, rows, 4, sums, accumulate);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_loss_spec_bwd(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                        const float* coefs, float* grad, int64_t planes, int32_t H, int32_t W, void* stream) {
    if (!loss_spec_ok(spec) || !y_pred || !y || !grad || !coefs || planes <= 0 || H <= 0 || W <= 0) return UCLSTM_E_BADARG;
    const int64_t total = planes * H * W;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    return loss_spec_bwd_launch(spec, y_pred, y, mask, coefs, grad, total, H, W, (hipStream_t)stream);
}

// ---- the same three with the mask broadcast over channels: plane p reads mask plane p / mask_div ----
extern "C" int32_t uclstm_loss_spec_fwd_bc(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask, double* sums,
                                           int64_t planes, int32_t H, int32_t W, int32_t mask_div, void* stream) {
    if (!loss_spec_ok(spec) || !y_pred || !y || !mask || !sums || planes <= 0 || H <= 0 || W <= 0 || mask_div < 1) return UCLSTM_E_BADARG;
    const int64_t total = planes * H * W;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    return loss_spec_fwd_launch<false, true>(spec, y_pred, y, mask, sums, total, H, W, 0, (hipStream_t)stream, mask_div);
}

extern "C" int32_t uclstm_loss_spec_fwd_ordered_bc(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                                   double* partials, double* sums, int32_t accumulate, int64_t planes, int32_t H,
                                                   int32_t W, int32_t mask_div, void* stream) {
    if (!loss_spec_ok(spec) || !y_pred || !y || !mask || !partials || !sums || planes <= 0 || H <= 0 || W <= 0 || mask_div < 1)
        return UCLSTM_E_BADARG;
    const int64_t total = planes * H * W;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    const int rows = grid_for(total, ORDERED_ROWS_CAP);          // = uclstm_loss_fwd_ordered_rows, whatever V is
    const int32_t rc = loss_spec_fwd_launch<true, true>(spec, y_pred, y, mask, partials, total, H, W, rows, (hipStream_t)stream, mask_div);
    if (rc != UCLSTM_OK) return rc;
    UCLSTM_LAUNCH(ordered_sum_f64_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, rows, 4, sums, accumulate);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_loss_spec_bwd_bc(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                           const float* coefs, float* grad, int64_t planes, int32_t H, int32_t W, int32_t mask_div,
                                           void* stream) {
    if (!loss_spec_ok(spec) || !y_pred || !y || !mask || !grad || !coefs || planes <= 0 || H <= 0 || W <= 0 || mask_div < 1)
        return UCLSTM_E_BADARG;
    const int64_t total = planes * H * W;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    return loss_spec_bwd_launch<true>(spec, y_pred, y, mask, coefs, grad, total, H, W, (hipStream_t)stream, mask_div);
}

// ---- the same three with a weight per plane: plane p counts plane_w[p mod period] times in each of the four sums ----
namespace {
bool loss_pw_ok(const float* mask, const float* plane_w, int32_t period, int64_t planes, int32_t mask_div) {
    return plane_w && period >= 1 && planes > 0 && planes % period == 0 && mask_div >= 1 && (mask || mask_div == 1);
}
}  // namespace

extern "C" int32_t uclstm_loss_spec_fwd_pw(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                           const float* plane_w, int32_t period, double* sums, int64_t planes, int32_t H, int32_t W,
                                           int32_t mask_div, void* stream) {
    if (!loss_spec_ok(spec) || !y_pred || !y || !sums || H <= 0 || W <= 0 || !loss_pw_ok(mask, plane_w, period, planes, mask_div))
        return UCLSTM_E_BADARG;
    const int64_t total = planes * H * W;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    return loss_spec_fwd_launch<false, true, true>(spec, y_pred, y, mask, sums, total, H, W, 0, (hipStream_t)stream, mask_div, plane_w, period);
}

extern "C" int32_t uclstm_loss_spec_fwd_ordered_pw(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                                   const float* plane_w, int32_t period, double* partials, double* sums,
                                                   int32_t accumulate, int64_t planes, int32_t H, int32_t W, int32_t mask_div,
                                                   void* stream) {
    if (!loss_spec_ok(spec) || !y_pred || !y || !partials || !sums || H <= 0 || W <= 0 ||
        !loss_pw_ok(mask, plane_w, period, planes, mask_div))
        return UCLSTM_E_BADARG;
    const int64_t total = planes * H * W;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    const int rows = grid_for(total, ORDERED_ROWS_CAP);          // = uclstm_loss_fwd_ordered_rows, whatever V is
    const int32_t rc = loss_spec_fwd_launch<true, true, true>(spec, y_pred, y, mask, partials, total, H, W, rows, (hipStream_t)stream, mask_div,
                                                              plane_w, period);
    if (rc != UCLSTM_OK) return rc;
    UCLSTM_LAUNCH(ordered_sum_f64_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, rows, 4, sums, accumulate);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_loss_spec_bwd_pw(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                           const float* plane_w, int32_t period, const float* coefs, float* grad, int64_t planes,
                                           int32_t H, int32_t W, int32_t mask_div, void* stream) {
    if (!loss_spec_ok(spec) || !y_pred || !y || !grad || !coefs || H <= 0 || W <= 0 || !loss_pw_ok(mask, plane_w, period, planes, mask_div))
        return UCLSTM_E_BADARG;
    const int64_t total = planes * H * W;
    if (total >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    return loss_spec_bwd_launch<true, true>(spec, y_pred, y, mask, coefs, grad, total, H, W, (hipStream_t)stream, mask_div, plane_w, period);
}

namespace {
__global__ void stream_spin_kernel(long ticks) {
    const long t0 = wall_clock64();                      // constant 100 MHz counter
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
}  // namespace

extern "C" int32_t uclstm_stream_spin(int32_t microseconds, void* stream) {
    if (microseconds <= 0 || microseconds > 100000) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(stream_spin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long)microseconds * 100);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_abi_version(void) { return UCLSTM_ABI_VERSION; }
extern "C" const char* uclstm_build_arch(void) { return "gfx950"; }
extern "C" const char* uclstm_last_error_string(void) { return hipGetErrorString((hipError_t)g_uclstm_last_hip_error); }
