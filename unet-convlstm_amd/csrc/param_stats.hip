// Per-tensor statistics of the optimiser's flat buffers (FusedAdamW.attach_monitor): one sweep over parameters, gradients and
// the weights of the previous record, eight f64 numbers per tensor into a record ring on the device.  Two launches per call:
//   phase 1  one block per row of the block table {tensor, start, count}: the block's eight partial results, stored (no atomics)
//   phase 2  one block per tensor: its partial rows added (or maxed) in block order into ring[slot][tensor]; block 0 writes the
//            record's meta row and advances the counts
// Whether this call records, and into which slot, is read from the device state, so the launch arguments never change and a
// captured call advances the ring on replay.  state = int64[8] {every, steps_seen, records_done, due, slot, reserved x 3}:
// phase 1 decides from {every, steps_seen, records_done} and its block 0 leaves the decision in {due, slot}; phase 2 reads only
// {due, slot}, and its block 0 alone reads and advances {steps_seen, records_done}.  No word is read and written in one launch.
// f32 only: this file is compiled once (no _f16 twin).
#include "common.h"

namespace {

constexpr int PS_NT = 256;
constexpr int PS_CHUNK = 16384;                  // elements one block reduces: 16 float4 per lane and buffer
constexpr int PS_U = 4;                          // float4 loads in flight per lane and buffer
constexpr int PS_COLS = 8;
constexpr int PS_STAGE = 128;                    // partial rows phase 2 stages in LDS at a time (8 KiB)

__device__ __forceinline__ bool finite32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct StatAcc {
    double gss = 0.0, pss = 0.0, dss = 0.0;
    float gmax = 0.f, pmax = 0.f;                // maxima of |f32| are f32 values: widened once, at the end
    uint32_t gnf = 0, gz = 0, pnf = 0;           // at most PS_CHUNK per block
};

template <bool HAS_PREV>
__device__ __forceinline__ void stat_one(StatAcc& a, float g, float p, float q) {
#pragma clang fp contract(off)
    const bool gf = finite32(g), pf = finite32(p);
    const double gd = (double)(gf ? g : 0.f), pd = (double)(pf ? p : 0.f);
    a.gss += gd * gd;
    a.pss += pd * pd;
    a.gmax = fmaxf(a.gmax, gf ? fabsf(g) : 0.f);
    a.pmax = fmaxf(a.pmax, pf ? fabsf(p) : 0.f);
    a.gnf += gf ? 0u : 1u;
    a.pnf += pf ? 0u : 1u;
    a.gz += (g == 0.f) ? 1u : 0u;
    if constexpr (HAS_PREV) {
        const double d = (pf && finite32(q)) ? (double)p - (double)q : 0.0;
        a.dss += d * d;
    }
}

// column c of a row: 1 and 5 are maxima, the others sums
template <int C>
__device__ __forceinline__ double stat_join(double a, double b) {
    if constexpr (C == 1 || C == 5) return fmax(a, b);
    return a + b;
}

template <int C>
__device__ __forceinline__ void wave_join(double (&v)[PS_COLS]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[C] = stat_join<C>(v[C], __shfl_xor(v[C], o, 64));
    if constexpr (C + 1 < PS_COLS) wave_join<C + 1>(v);
}

template <int C>
__device__ __forceinline__ double waves_join(const double* red, int c) {
    if (c == C) return stat_join<C>(stat_join<C>(stat_join<C>(red[C], red[PS_COLS + C]), red[2 * PS_COLS + C]), red[3 * PS_COLS + C]);
    if constexpr (C + 1 < PS_COLS) return waves_join<C + 1>(red, c);
    return 0.0;
}

template <bool HAS_PREV>
__global__ __launch_bounds__(PS_NT) void param_stats_blocks_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                                  float* __restrict__ prev, int64_t n, const int64_t* __restrict__ blocks,
                                                                  double* __restrict__ partials, int64_t history,
                                                                  int64_t* __restrict__ state) {
    __shared__ double red[4 * PS_COLS];
    const int64_t every = state[0] > 0 ? state[0] : 1;
    const bool due = (state[1] + 1) % every == 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state[3] = due ? 1 : 0;
        const int64_t slot = state[2] % history;
        state[4] = slot < 0 ? 0 : slot;
    }
    if (!due) return;                                            // uniform over the grid: no sweep, prev stays
    const int64_t* row = blocks + (int64_t)blockIdx.x * 3;
    const int64_t start = row[1];
    int64_t count = row[2];
    if (start < 0 || count < 0 || count > PS_CHUNK || start > n - count) count = 0;      // a row outside the buffer reads nothing
    const int t = threadIdx.x;
    StatAcc a;
    // the flat buffers are 16-byte aligned (checked by the host), a tensor starts at any element: scalar head up to the next
    // multiple of four elements, float4 body, scalar tail
    int head = (int)((4 - (start & 3)) & 3);
    if (head > count) head = (int)count;
    const int nvec = (int)((count - head) >> 2);
    const int tail = (int)(count - head - 4 * (int64_t)nvec);
    if (t < head) {
        const int64_t i = start + t;
        const float w = p[i];
        stat_one<HAS_PREV>(a, g[i], w, HAS_PREV ? prev[i] : 0.f);
        if constexpr (HAS_PREV) prev[i] = w;
    }
    const int64_t body = start + head;
    const float4* p4 = (const float4*)(p + body);
    const float4* g4 = (const float4*)(g + body);
    float4* q4 = HAS_PREV ? (float4*)(prev + body) : nullptr;
    int i = t;
    for (; i + (PS_U - 1) * PS_NT < nvec; i += PS_U * PS_NT) {
        float4 w[PS_U], d[PS_U], q[PS_U];
#pragma unroll
        for (int u = 0; u < PS_U; ++u) {
            w[u] = p4[i + u * PS_NT];
            d[u] = g4[i + u * PS_NT];
            if constexpr (HAS_PREV) q[u] = q4[i + u * PS_NT];
            else q[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < PS_U; ++u) {
            stat_one<HAS_PREV>(a, d[u].x, w[u].x, q[u].x);
            stat_one<HAS_PREV>(a, d[u].y, w[u].y, q[u].y);
            stat_one<HAS_PREV>(a, d[u].z, w[u].z, q[u].z);
            stat_one<HAS_PREV>(a, d[u].w, w[u].w, q[u].w);
            if constexpr (HAS_PREV) q4[i + u * PS_NT] = w[u];
        }
    }
    for (; i < nvec; i += PS_NT) {
        const float4 w = p4[i], d = g4[i];
        const float4 q = HAS_PREV ? q4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        stat_one<HAS_PREV>(a, d.x, w.x, q.x);
        stat_one<HAS_PREV>(a, d.y, w.y, q.y);
        stat_one<HAS_PREV>(a, d.z, w.z, q.z);
        stat_one<HAS_PREV>(a, d.w, w.w, q.w);
        if constexpr (HAS_PREV) q4[i] = w;
    }
    if (t < tail) {
        const int64_t j = body + 4 * (int64_t)nvec + t;
        const float w = p[j];
        stat_one<HAS_PREV>(a, g[j], w, HAS_PREV ? prev[j] : 0.f);
        if constexpr (HAS_PREV) prev[j] = w;
    }
    // wave shuffles, then LDS: a fixed tree, so the block's row is a function of its elements alone
    double v[PS_COLS] = {a.gss, (double)a.gmax, (double)a.gnf, (double)a.gz, a.pss, (double)a.pmax, (double)a.pnf, a.dss};
    wave_join<0>(v);
    const int lane = t & 63, wave = t >> 6;
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < PS_COLS; ++c) red[wave * PS_COLS + c] = v[c];
    __syncthreads();
    if (t < PS_COLS) partials[(int64_t)blockIdx.x * PS_COLS + t] = waves_join<0>(red, t);
}

// A tensor's partial rows, strictly in block order: PS_STAGE rows at a time go to LDS through the whole block's registers
// (contiguous 16-byte-per-lane loads, the next stage's in flight while this one is added), then thread c < 8 adds or maxes
// column c down the staged rows.  The chain of adds is the order, the loads are not part of it.
__global__ __launch_bounds__(PS_NT) void param_stats_tensors_kernel(const int64_t* __restrict__ tensor_blocks, int64_t n_blocks,
                                                                   const double* __restrict__ partials, double* __restrict__ ring,
                                                                   double* __restrict__ meta, const double* __restrict__ sumsq,
                                                                   const float* __restrict__ scale, int64_t* __restrict__ state) {
    __shared__ double2 stage[PS_STAGE * PS_COLS / 2];
    const bool due = state[3] != 0;
    const int64_t slot = state[4];
    const int t = threadIdx.x;
    if (due) {                                                   // uniform over the grid
        const int64_t first = tensor_blocks[(int64_t)blockIdx.x * 2];
        int64_t nb = tensor_blocks[(int64_t)blockIdx.x * 2 + 1];
        if (first < 0 || nb < 0 || first > n_blocks - nb) nb = 0;                          // uniform over the block
        const bool is_max = t == 1 || t == 5;
        double acc = 0.0;
        constexpr int PER = PS_STAGE * PS_COLS / 2 / PS_NT;      // 16-byte pieces of a stage per thread
        const double2* src = (const double2*)(partials + first * PS_COLS);                // a row is 64 bytes: 16-byte aligned
        const int64_t pieces = nb * (PS_COLS / 2);
        double2 next[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int64_t i = t + u * PS_NT;
            next[u] = i < pieces ? src[i] : make_double2(0.0, 0.0);
        }
        for (int64_t base = 0; base < nb; base += PS_STAGE) {
            const int rows = (int)(nb - base < PS_STAGE ? nb - base : PS_STAGE);
#pragma unroll
            for (int u = 0; u < PER; ++u) stage[t + u * PS_NT] = next[u];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < PER; ++u) {                      // the next stage's rows travel while this one is added
                const int64_t i = (base + PS_STAGE) * (PS_COLS / 2) + t + u * PS_NT;
                next[u] = i < pieces ? src[i] : make_double2(0.0, 0.0);
            }
            if (t < PS_COLS) {
                const double* col = (const double*)stage + t;
                int r = 0;
                for (; r + 16 <= rows; r += 16) {                // 16 LDS reads in flight, one chain of adds
                    double x[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) x[u] = col[(r + u) * PS_COLS];
#pragma unroll
                    for (int u = 0; u < 16; ++u) acc = is_max ? fmax(acc, x[u]) : acc + x[u];
                }
                for (; r < rows; ++r) {
                    const double x = col[r * PS_COLS];
                    acc = is_max ? fmax(acc, x) : acc + x;
                }
            }
            __syncthreads();
        }
        if (t < PS_COLS) ring[(slot * gridDim.x + blockIdx.x) * PS_COLS + t] = acc;
    }
    if (blockIdx.x == 0 && t == 0) {
        const int64_t seen = state[1] + 1;
        state[1] = seen;
        if (due) {
            double* m = meta + slot * 4;
            m[0] = (double)seen;
            m[1] = scale ? (double)*scale : 1.0;
            m[2] = sumsq ? *sumsq : __builtin_nan("");
            m[3] = (sumsq && step_overflowed(*sumsq)) ? 1.0 : 0.0;
            state[2] += 1;
        }
    }
}

}  // namespace

extern "C" int64_t uclstm_param_stats_chunk(void) { return PS_CHUNK; }

extern "C" int32_t uclstm_param_stats(const float* p, const float* g, float* prev, int64_t n, const int64_t* blocks, int64_t n_blocks,
                                      const int64_t* tensor_blocks, int32_t n_tensors, double* partials, double* ring, double* meta,
                                      int32_t history, const double* sumsq, const float* scale, int64_t* state, void* stream) {
    if (!p || !g || !blocks || !tensor_blocks || !partials || !ring || !meta || !state) return UCLSTM_E_BADARG;
    if (((uintptr_t)partials % 16)) return UCLSTM_E_BADARG;
    if (n <= 0 || n_blocks <= 0 || n_blocks > 0x7fffffff || n_tensors <= 0 || history <= 0) return UCLSTM_E_BADARG;
    if (((uintptr_t)p % 16) || ((uintptr_t)g % 16) || ((uintptr_t)prev % 16)) return UCLSTM_E_BADARG;
    const hipStream_t s = (hipStream_t)stream;
    if (prev)
        UCLSTM_LAUNCH(param_stats_blocks_kernel<true>, dim3((unsigned)n_blocks), dim3(PS_NT), 0, s, p, g, prev, n, blocks, partials,
                      (int64_t)history, state);
    else
        UCLSTM_LAUNCH(param_stats_blocks_kernel<false>, dim3((unsigned)n_blocks), dim3(PS_NT), 0, s, p, g, prev, n, blocks, partials,
                      (int64_t)history, state);
    UCLSTM_LAUNCH(param_stats_tensors_kernel, dim3((unsigned)n_tensors), dim3(PS_NT), 0, s, tensor_blocks, (int64_t)n_blocks,
                  (const double*)partials, ring, meta, sumsq, scale, state);
    return UCLSTM_OK;
}
