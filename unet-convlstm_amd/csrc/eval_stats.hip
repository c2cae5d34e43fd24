// Evaluation statistics of train/get_metrics.py:117-358 and test.py:333-351 in ONE pass over (y_pred, y, mask): de-normalise,
// per-(frame, chunk) f64 sums and min/max rows, three np.histogram-style histograms, the np.digitize count of the target and
// the "up to K points per target bin" scatter sample as a reservoir.  Traffic: 8 B (12 B with a mask) per pixel, read once; what
// bounds the kernel is recorded in DESIGN.md section 3 and profiles/eval_report.txt.
//
// One kernel, eval_stats_kernel<CY, VEC, LDS>, and one device body, channel_stats, serve both entry points: uclstm_eval_stats
// is the CY = 1 instantiation on one plane of P elements, uclstm_eval_stats_vec runs the body once per target channel of a
// frame of [Cy][HW] planes and, from CY = 2 on, adds the statistics that need two channels of one pixel (below).
//
// Reproducibility: a block owns one chunk of one frame (the chunk size depends on nothing but this file), every thread owns
// fixed pixels of it, and the row is reduced in a fixed order and written with plain stores -- no floating-point atomic
// anywhere.  Counts are integers: LDS u32 counters per block, flushed with 64-bit integer atomics (sums of integers do not
// depend on the order).  Only WHICH pairs the reservoir keeps depends on the arrival order of blocks.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int PPT = 8;                           // pixels per thread
constexpr int CHUNK = NT * PPT;                  // pixels of one frame per block: 2048 (a 512 x 512 frame is 128 blocks)
constexpr int ROW = UCLSTM_EVAL_ROW;             // doubles per table row
constexpr int VROW = UCLSTM_EVAL_VROW;
constexpr size_t LDS_BUDGET = 60 * 1024;         // counters beyond this live in global memory (per-pixel integer atomics)

struct Args {                                    // one channel: a plane of P elements per frame
    const float* yp;
    const float* y;
    const float* mask;
    int64_t yp_sb, yp_st, y_sb, y_st, m_sb, m_st;
    FastDiv dT, dCpf;                            // frame -> (b, t), block -> (frame, chunk)
    int P;
    int transform;
    float yscale, tmin, trange;
    double* table;
    int bins;
    double h_lo, h_hi, h_step, h_norm;           // np.histogram: edges lo + i * step (last = hi), first guess (x - lo) * norm
    double e_lo, e_hi, e_step, e_norm;
    unsigned long long* hist;                    // [3][bins]
    double d_lo, d_w, d_inv_w, d_last;           // np.digitize over edges lo + i * w, i < n_edges
    int n_edges;
    unsigned long long* dig;                     // [n_edges + 1]
    int K;
    unsigned long long seed;
    float2* scatter;                             // [n_edges + 1][K]
};

struct PairArgs {
    int w_chan, h_chan;                          // the horizontal pair, both >= 0 or the vector part does not exist
    float w_sign, h_sign;
    double s_hi, s_step, s_norm;                 // speed histograms over [0, s_hi]
    double p_hi, p_step, p_norm;                 // endpoint error over [0, p_hi]
    double t_step, t_norm;                       // direction error over [-180, 180]
    int dir_bins;
    float min_speed;
    double* vtable;
    unsigned long long* vhist;                   // [3][bins]
    unsigned long long* dir_hist;                // [dir_bins]
};

template <int CY>
struct KArgs {
    Args ch[CY];                                 // channel c as uclstm_eval_stats sees it in place: yp / y + c * P, its constants, ranges
                                                 // and slices of hist / dig / scatter; table + c * ROW (a row is [CY][ROW])
    PairArgs v;                                  // read from CY = 2 on
};

__device__ __forceinline__ float denorm(float v, const Args& a) {
    const float yt = (v + 1.f) * 0.5f * a.trange + a.tmin;      // as metric_sums_kernel
    if (a.transform == UCLSTM_EVAL_ASINH) return sinhf(yt) * a.yscale;
    if (a.transform == UCLSTM_EVAL_SIGNED_LOG) {
        const float s = (yt > 0.f) ? 1.f : ((yt < 0.f) ? -1.f : 0.f);
        return s * expm1f(fabsf(yt)) * a.yscale;
    }
    return yt;
}

// np.histogram(x, bins, range=(lo, hi)): -1 when x is outside [lo, hi] (or NaN); x == hi belongs to the last bin.  numpy
// guesses the bin from (x - lo) * norm and then corrects it against the edges themselves; so does this.
__device__ __forceinline__ int hist_bin(float xf, double lo, double hi, double step, double norm, int bins) {
    const double x = (double)xf;
    if (!(x >= lo && x <= hi)) return -1;
    int k = (int)((x - lo) * norm);
    k = min(k, bins - 1);
    const double e0 = lo + (double)k * step;
    const double e1 = (k + 1 == bins) ? hi : lo + (double)(k + 1) * step;
    if (x < e0 && k > 0) --k;
    else if (x >= e1 && k + 1 < bins) ++k;
    return k;
}

// np.digitize(x, edges): number of edges <= x, 0 .. n_edges (NaN sorts behind the last edge)
__device__ __forceinline__ int digitize_bin(float xf, const Args& a) {
    const double x = (double)xf;
    if (x < a.d_lo) return 0;
    if (!(x < a.d_last)) return a.n_edges;
    int k = (int)((x - a.d_lo) * a.d_inv_w);                     // edges[k] <= x < edges[k + 1], up to rounding of the quotient
    k = min(max(k, 0), a.n_edges - 2);
    if (x < a.d_lo + (double)k * a.d_w) --k;
    else if (x >= a.d_lo + (double)(k + 1) * a.d_w) ++k;
    return k + 1;
}

// counter[bin] += 1 for every lane with act, returning the lane's rank (the counter before its own increment) when RANK.
// Cloud data is skewed -- most lanes of a wave hit ONE bin, and 64 LDS atomics on one address are executed one after the
// other -- so up to TRIES times the bin of the first pending lane is looked at: a group of >= 8 lanes is added by its leader
// as one atomic and ranked by lane order; smaller groups and whatever is left take one atomic per lane.  Must be called by
// whole waves (act = false for lanes with nothing to add).
template <bool RANK, int TRIES>
__device__ __forceinline__ uint32_t count_in_lds(uint32_t* cnt, int bin, bool act) {
    const int lane = threadIdx.x & 63;
    const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    bool pending = act;
    uint32_t rank = 0;
#pragma unroll
    for (int t = 0; t < TRIES; ++t) {
        const uint64_t todo = __ballot(pending);
        if (!todo) break;
        const int lead = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
        const int cand = __builtin_amdgcn_readlane(bin, lead);
        const bool mine = pending && bin == cand;
        const uint64_t m = __ballot(mine);
        const int n = __popcll(m);
        if (n >= 8) {
            uint32_t base = 0;
            if (lane == lead) base = atomicAdd(cnt + cand, (uint32_t)n);
            if (RANK) {
                base = __builtin_amdgcn_readlane(base, lead);
                if (mine) rank = base + (uint32_t)__popcll(m & lt);
            }
        } else if (mine) {
            rank = atomicAdd(cnt + bin, 1u);
        }
        pending = pending && !mine;
    }
    if (pending) rank = atomicAdd(cnt + bin, 1u);
    return rank;
}

// counter-based hash of (seed, bin, ticket): splitmix64's finaliser over the mixed key
__device__ __forceinline__ uint64_t hash3(uint64_t seed, uint32_t bin, uint64_t t) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (t + 1) + 0xD1B54A32D192ED03ull * (uint64_t)(bin + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Reservoir sampling (algorithm R) with the ticket as the item index: the first K tickets of a bin fill its slots, ticket
// t >= K replaces slot j = hash mod (t + 1) when j < K.  The reduction of the 64-bit hash to [0, t] is the high half of
// hash * (t + 1): the same uniform slot as a remainder, without a 64-bit division per pixel.  One 8-byte store per pair.
// Stores of one launch land in any order: a replacement that hashed to slot j < K can be overtaken by the FILL of ticket j
// from another block of the same launch and is then lost, so while a bin's first K tickets are still in flight the sample
// leans slightly towards them; it is exactly uniform over the pixels of later launches (stream order), approximately within
// the launch that fills the bin.
__device__ __forceinline__ void scatter_store(const Args& a, int bin, uint64_t t, float gt, float pr) {
    uint64_t slot = t;
    if (t >= (uint64_t)a.K) slot = __umul64hi(hash3(a.seed, (uint32_t)bin, t), t + 1);
    if (slot < (uint64_t)a.K) a.scatter[(int64_t)bin * a.K + (int64_t)slot] = make_float2(gt, pr);
}

// The eight elements of a chunk that this thread owns; past the end of the plane: 0.  VEC: P % 4 == 0, bases and strides
// 16-byte aligned, so a quad is inside or outside.  A lane past the end reads the chunk's first element (left > 0: it exists)
// and drops it: loads without a branch around them are issued together, those of the caller's next plane included.
template <bool VEC>
__device__ __forceinline__ void load_chunk(const float* p, int left, float (&v)[PPT]) {
    if (VEC) {
#pragma unroll
        for (int q = 0; q < PPT / 4; ++q) {
            const int o = (q * NT + (int)threadIdx.x) * 4;
            const bool in = o < left;
            const float4 x = *(const float4*)(p + (in ? o : 0));
            v[4 * q + 0] = in ? x.x : 0.f, v[4 * q + 1] = in ? x.y : 0.f, v[4 * q + 2] = in ? x.z : 0.f, v[4 * q + 3] = in ? x.w : 0.f;
        }
    } else {
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int o = q * NT + (int)threadIdx.x;
            const float x = p[o < left ? o : 0];
            v[q] = o < left ? x : 0.f;
        }
    }
}

// lanes -> wave with xor shuffles, 32 .. 1
template <int N>
__device__ __forceinline__ void wave_sum(double (&s)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
}

// One channel's whole job for the chunk of this block (`left` > 0 pixels at offsets off_p / off_y of the channel's bases, of
// which ok[] count): both loads, de-normalisation, the f64 sums and f32 extremes, the four bins and their counters (`cnt`:
// this channel's hist gt | pred | err [bins], digitize [nd], bases lo | hi [nd] of dynamic LDS, zeroed; unused when !LDS), the
// table row at blockIdx.x * row_stride, the flush of the counters and the scatter sample.  Two block barriers.  vp / vy come
// back de-normalised.
template <bool VEC, bool LDS>
__device__ __forceinline__ void channel_stats(const Args& a, const bool (&ok)[PPT], int64_t off_p, int64_t off_y, int left, uint32_t* cnt,
                                              double (&red_s)[4][8], float (&red_m)[4][6], int row_stride, float (&vp)[PPT],
                                              float (&vy)[PPT]) {
    const int nd = a.n_edges + 1;
    uint32_t* h_gt = cnt;
    uint32_t* h_pr = cnt + a.bins;
    uint32_t* h_er = cnt + 2 * a.bins;
    uint32_t* dg = cnt + 3 * a.bins;
    uint32_t* base_lo = dg + nd;
    uint32_t* base_hi = base_lo + nd;
    load_chunk<VEC>(a.yp + off_p, left, vp);
    load_chunk<VEC>(a.y + off_y, left, vy);

    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // n, |d|, d^2, d, gt, gt^2, pred, pred^2
    const float inf = __builtin_inff();
    float mn_g = inf, mx_g = -inf, mn_p = inf, mx_p = -inf, mn_d = inf, mx_d = -inf;
    int dbin[PPT];
    uint32_t rank[PPT];
    uint64_t ticket[PPT];                        // !LDS only
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const float pr = denorm(vp[q], a), gt = denorm(vy[q], a);
        const float df = pr - gt;
        vp[q] = pr, vy[q] = gt;
        const bool v = ok[q];
        if (v) {
            const double d = (double)df, g = (double)gt, p = (double)pr;
            s[0] += 1.0, s[1] += fabs(d), s[2] += d * d, s[3] += d;
            s[4] += g, s[5] += g * g, s[6] += p, s[7] += p * p;
            mn_g = fminf(mn_g, gt), mx_g = fmaxf(mx_g, gt);
            mn_p = fminf(mn_p, pr), mx_p = fmaxf(mx_p, pr);
            mn_d = fminf(mn_d, df), mx_d = fmaxf(mx_d, df);
        }
        const int bg = v ? hist_bin(gt, a.h_lo, a.h_hi, a.h_step, a.h_norm, a.bins) : -1;
        const int bp = v ? hist_bin(pr, a.h_lo, a.h_hi, a.h_step, a.h_norm, a.bins) : -1;
        const int be = v ? hist_bin(df, a.e_lo, a.e_hi, a.e_step, a.e_norm, a.bins) : -1;
        dbin[q] = v ? digitize_bin(gt, a) : -1;
        if (LDS) {
            count_in_lds<false, 2>(h_gt, bg, bg >= 0);
            count_in_lds<false, 1>(h_pr, bp, bp >= 0);
            count_in_lds<false, 1>(h_er, be, be >= 0);
            rank[q] = count_in_lds<true, 2>(dg, dbin[q], v);
        } else {
            if (bg >= 0) atomicAdd(a.hist + bg, 1ull);
            if (bp >= 0) atomicAdd(a.hist + a.bins + bp, 1ull);
            if (be >= 0) atomicAdd(a.hist + 2 * a.bins + be, 1ull);
            ticket[q] = v ? atomicAdd(a.dig + dbin[q], 1ull) : 0ull;
        }
    }

    // the chunk's row: lanes -> wave (xor shuffles), waves -> block in wave order
    wave_sum(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn_g = fminf(mn_g, __shfl_xor(mn_g, o, 64)), mx_g = fmaxf(mx_g, __shfl_xor(mx_g, o, 64));
        mn_p = fminf(mn_p, __shfl_xor(mn_p, o, 64)), mx_p = fmaxf(mx_p, __shfl_xor(mx_p, o, 64));
        mn_d = fminf(mn_d, __shfl_xor(mn_d, o, 64)), mx_d = fmaxf(mx_d, __shfl_xor(mx_d, o, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) red_s[wave][k] = s[k];
        red_m[wave][0] = mn_g, red_m[wave][1] = mx_g, red_m[wave][2] = mn_p;
        red_m[wave][3] = mx_p, red_m[wave][4] = mn_d, red_m[wave][5] = mx_d;
    }
    __syncthreads();                             // also: every LDS counter of this channel is final
    if (threadIdx.x < ROW) {
        const int k = threadIdx.x;
        double v = 0.0;
        if (k < 8) {
            v = ((red_s[0][k] + red_s[1][k]) + red_s[2][k]) + red_s[3][k];
        } else if (k < 14) {
            const int j = k - 8;
            const float m0 = red_m[0][j], m1 = red_m[1][j], m2 = red_m[2][j], m3 = red_m[3][j];
            v = (double)((j & 1) ? fmaxf(fmaxf(m0, m1), fmaxf(m2, m3)) : fminf(fminf(m0, m1), fminf(m2, m3)));
        }
        a.table[(int64_t)blockIdx.x * row_stride + k] = v;
    }

    if (LDS) {
        for (int i = threadIdx.x; i < 3 * a.bins; i += NT) {
            const uint32_t c = cnt[i];
            if (c) atomicAdd(a.hist + i, (unsigned long long)c);
        }
        // one reservation per (block, non-empty target bin): tickets base .. base + c - 1 belong to this block
        for (int i = threadIdx.x; i < nd; i += NT) {
            const uint32_t c = dg[i];
            if (!c) continue;
            if (a.K > 0) {
                const unsigned long long base = atomicAdd(a.dig + i, (unsigned long long)c);
                base_lo[i] = (uint32_t)base;
                base_hi[i] = (uint32_t)(base >> 32);
            } else {
                atomicAdd(a.dig + i, (unsigned long long)c);
            }
        }
        if (a.K > 0) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < PPT; ++q) {
                const int bin = dbin[q];
                if (bin < 0) continue;
                const uint64_t base = ((uint64_t)base_hi[bin] << 32) | base_lo[bin];
                scatter_store(a, bin, base + rank[q], vy[q], vp[q]);
            }
        }
    } else if (a.K > 0) {
#pragma unroll
        for (int q = 0; q < PPT; ++q)
            if (dbin[q] >= 0) scatter_store(a, dbin[q], ticket[q], vy[q], vp[q]);
    }
}

// A block owns one chunk of one frame for all CY channels, one mask plane for all of them.  Dynamic LDS: per channel the
// counters of channel_stats; from CY = 2 on then speed gt | pred | epe [bins], dir [dir_bins].  CY = 1 is the scalar report:
// a pair needs two distinct channels, so the vector part below and its registers do not exist there.
//
// Registers at CY >= 2: the channels are a fully unrolled loop; a channel's values, bins and ranks die with its iteration,
// because its scatter tickets are reserved and used inside it.  Only the mask bits and the four f32 components of the
// horizontal pair live across the loop.  Resource usage, timing and the variants tried (loading a channel ahead, an occupancy
// floor): profiles/eval_report_vec.txt, profiles/eval_stats_body_audit.txt.
template <int CY, bool VEC, bool LDS>
__global__ __launch_bounds__(NT) void eval_stats_kernel(const KArgs<CY> ka) {
    extern __shared__ uint32_t sm[];
    __shared__ double red_s[CY][4][8];
    __shared__ float red_m[CY][4][6];
    const Args& a0 = ka.ch[0];
    const int bins = a0.bins, nd = a0.n_edges + 1;
    const int per = 3 * bins + 3 * nd;
    if (LDS) {
        // one channel: its counters alone (the ticket bases are written before they are read); more: everything allocated
        const int live = CY >= 2 ? CY * per + 3 * bins + ka.v.dir_bins : 3 * bins + nd;
        for (int i = threadIdx.x; i < live; i += NT) sm[i] = 0u;
        __syncthreads();
    }

    const uint32_t frame = fdiv(blockIdx.x, a0.dCpf);
    const int chunk = (int)(blockIdx.x - frame * a0.dCpf.d);
    const uint32_t b = fdiv(frame, a0.dT);
    const uint32_t t = frame - b * a0.dT.d;
    const int p0 = chunk * CHUNK;
    const int64_t off_p = (int64_t)b * a0.yp_sb + (int64_t)t * a0.yp_st + p0;
    const int64_t off_y = (int64_t)b * a0.y_sb + (int64_t)t * a0.y_st + p0;
    const int left = a0.P - p0;                  // pixels of this chunk: > 0, the last chunk of a frame may be partial

    bool ok[PPT];
    {
        float m[PPT];
        if (a0.mask) load_chunk<VEC>(a0.mask + (int64_t)b * a0.m_sb + (int64_t)t * a0.m_st + p0, left, m);
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int o = VEC ? ((q / 4) * NT + (int)threadIdx.x) * 4 : q * NT + (int)threadIdx.x;      // a quad is inside or outside
            ok[q] = o < left && (a0.mask ? m[q] != 0.f : true);
        }
    }

    float ga[PPT], gb[PPT], pa[PPT], pb[PPT];    // CY >= 2: the pair in the image frame, a along +column, b along +row
    if constexpr (CY >= 2) {
#pragma unroll
        for (int q = 0; q < PPT; ++q) ga[q] = gb[q] = pa[q] = pb[q] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < CY; ++c) {
        float vp[PPT], vy[PPT];
        channel_stats<VEC, LDS>(ka.ch[c], ok, off_p, off_y, left, sm + c * per, red_s[c], red_m[c], CY * ROW, vp, vy);
        if constexpr (CY >= 2) {
            if (c == ka.v.w_chan) {
#pragma unroll
                for (int q = 0; q < PPT; ++q) ga[q] = ka.v.w_sign * vy[q], pa[q] = ka.v.w_sign * vp[q];
            }
            if (c == ka.v.h_chan) {
#pragma unroll
                for (int q = 0; q < PPT; ++q) gb[q] = ka.v.h_sign * vy[q], pb[q] = ka.v.h_sign * vp[q];
            }
        }
    }

    if constexpr (CY >= 2) {
        const PairArgs& va = ka.v;
        if (va.w_chan < 0 || va.h_chan < 0) return;              // the same in every thread
        __shared__ double red_v[4][12];
        __shared__ float red_x[4][3];
        uint32_t* vh = sm + CY * per;
        uint32_t* dh = vh + 3 * bins;
        // n, |ds|, ds^2, ds, s_g, s_p, epe, epe^2, n_dir, |dth|, dth, dth^2 in f64 from f32 per-pixel values; max epe, s_g, s_p
        double s[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const float inf = __builtin_inff();
        float mx_e = -inf, mx_g = -inf, mx_p = -inf;
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const bool v = ok[q];
            const float sg = sqrtf(ga[q] * ga[q] + gb[q] * gb[q]), sp = sqrtf(pa[q] * pa[q] + pb[q] * pb[q]);
            const float da = pa[q] - ga[q], db = pb[q] - gb[q];
            const float epe = sqrtf(da * da + db * db), ds = sp - sg;
            float th = atan2f(ga[q] * pb[q] - gb[q] * pa[q], ga[q] * pa[q] + gb[q] * pb[q]) * 57.29577951308232f;
            th = (th <= -180.f) ? 180.f : fminf(th, 180.f);          // (-180, 180]
            const bool vd = v && sg >= va.min_speed && sp >= va.min_speed;
            if (v) {
                const double d = (double)ds, e = (double)epe;
                s[0] += 1.0, s[1] += fabs(d), s[2] += d * d, s[3] += d;
                s[4] += (double)sg, s[5] += (double)sp, s[6] += e, s[7] += e * e;
                mx_e = fmaxf(mx_e, epe), mx_g = fmaxf(mx_g, sg), mx_p = fmaxf(mx_p, sp);
            }
            if (vd) {
                const double x = (double)th;
                s[8] += 1.0, s[9] += fabs(x), s[10] += x, s[11] += x * x;
            }
            const int bg = v ? hist_bin(sg, 0.0, va.s_hi, va.s_step, va.s_norm, bins) : -1;
            const int bp = v ? hist_bin(sp, 0.0, va.s_hi, va.s_step, va.s_norm, bins) : -1;
            const int be = v ? hist_bin(epe, 0.0, va.p_hi, va.p_step, va.p_norm, bins) : -1;
            const int bt = vd ? hist_bin(th, -180.0, 180.0, va.t_step, va.t_norm, va.dir_bins) : -1;
            if (LDS) {
                count_in_lds<false, 2>(vh, bg, bg >= 0);
                count_in_lds<false, 1>(vh + bins, bp, bp >= 0);
                count_in_lds<false, 1>(vh + 2 * bins, be, be >= 0);
                count_in_lds<false, 1>(dh, bt, bt >= 0);
            } else {
                if (bg >= 0) atomicAdd(va.vhist + bg, 1ull);
                if (bp >= 0) atomicAdd(va.vhist + bins + bp, 1ull);
                if (be >= 0) atomicAdd(va.vhist + 2 * bins + be, 1ull);
                if (bt >= 0) atomicAdd(va.dir_hist + bt, 1ull);
            }
        }
        wave_sum(s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mx_e = fmaxf(mx_e, __shfl_xor(mx_e, o, 64));
            mx_g = fmaxf(mx_g, __shfl_xor(mx_g, o, 64));
            mx_p = fmaxf(mx_p, __shfl_xor(mx_p, o, 64));
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) red_v[wave][k] = s[k];
            red_x[wave][0] = mx_e, red_x[wave][1] = mx_g, red_x[wave][2] = mx_p;
        }
        __syncthreads();
        if (threadIdx.x < VROW) {
            const int k = threadIdx.x;
            double v = 0.0;
            if (k < 12) v = ((red_v[0][k] + red_v[1][k]) + red_v[2][k]) + red_v[3][k];
            else if (k < 15) v = (double)fmaxf(fmaxf(red_x[0][k - 12], red_x[1][k - 12]), fmaxf(red_x[2][k - 12], red_x[3][k - 12]));
            va.vtable[(int64_t)blockIdx.x * VROW + k] = v;
        }
        if (LDS) {
            for (int i = threadIdx.x; i < 3 * bins; i += NT) {
                const uint32_t n = vh[i];
                if (n) atomicAdd(va.vhist + i, (unsigned long long)n);
            }
            for (int i = threadIdx.x; i < va.dir_bins; i += NT) {
                const uint32_t n = dh[i];
                if (n) atomicAdd(va.dir_hist + i, (unsigned long long)n);
            }
        }
    }
}

int64_t rows_for(int64_t P, int64_t frames) { return frames * ((P + CHUNK - 1) / CHUNK); }

// ---------------------------------------------------------------------------------------------
// host: the two descriptors name what they share alike, so the helpers below read it from either
// ---------------------------------------------------------------------------------------------
struct Channel {                                 // what a channel has of its own
    float y_scale, trans_min, trans_max;
    double hist_lo, hist_hi, err_lo, err_hi, dig_lo, dig_w;
};

// frames of `planes` planes of P elements; *cpf chunks per plane, *rows blocks
template <class D>
bool shared_ok(const D* d, int64_t P, int64_t planes, int64_t* cpf, int64_t* rows) {
    if (!d->y_pred || !d->y || !d->table || !d->hist || !d->dig_count) return false;
    if (P <= 0 || d->B <= 0 || d->T <= 0) return false;
    if (d->bins < 1 || d->bins > 4096 || d->n_edges < 2 || d->n_edges > 65536) return false;
    if (d->K < 0 || (d->K > 0 && (!d->scatter || ((uintptr_t)d->scatter % 8)))) return false;
    if (d->transform != UCLSTM_EVAL_NONE && d->transform != UCLSTM_EVAL_ASINH && d->transform != UCLSTM_EVAL_SIGNED_LOG) return false;
    if (d->pred_stride_b < 0 || d->pred_stride_t < 0 || d->y_stride_b < 0 || d->y_stride_t < 0 ||
        (d->mask && (d->mask_stride_b < 0 || d->mask_stride_t < 0)))
        return false;
    const int64_t lim = (int64_t)1 << 31;
    const int64_t frames = (int64_t)d->B * d->T;
    if (P >= lim || frames >= lim || frames * planes >= lim || frames * planes * P >= lim) return false;
    *cpf = (P + CHUNK - 1) / CHUNK;
    *rows = frames * *cpf;
    return *rows * NT < ((int64_t)1 << 32);                      // one block per row, in grid.x
}

bool channel_ok(int transform, const Channel& k) {
    if (!(k.hist_hi > k.hist_lo) || !(k.err_hi > k.err_lo)) return false;
    if (!(k.dig_w > 0.0) || !(k.dig_lo == k.dig_lo)) return false;
    return transform == UCLSTM_EVAL_NONE || k.y_scale != 0.f;
}

// channel c of a frame of planes of P elements, with its slices of table / hist / dig_count / scatter
template <class D>
void fill_channel(Args& a, const D* d, int64_t P, int64_t cpf, int c, const Channel& k) {
    const int nd = d->n_edges + 1;
    a.yp = d->y_pred + c * P, a.y = d->y + c * P, a.mask = d->mask;
    a.yp_sb = d->pred_stride_b, a.yp_st = d->pred_stride_t, a.y_sb = d->y_stride_b, a.y_st = d->y_stride_t;
    a.m_sb = d->mask ? d->mask_stride_b : 0, a.m_st = d->mask ? d->mask_stride_t : 0;
    a.dT = make_fastdiv((uint32_t)d->T), a.dCpf = make_fastdiv((uint32_t)cpf);
    a.P = (int)P;
    a.transform = d->transform;
    a.yscale = k.y_scale, a.tmin = k.trans_min, a.trange = k.trans_max - k.trans_min;
    a.table = d->table + c * ROW;
    a.bins = d->bins;
    a.h_lo = k.hist_lo, a.h_hi = k.hist_hi, a.h_step = (k.hist_hi - k.hist_lo) / d->bins, a.h_norm = d->bins / (k.hist_hi - k.hist_lo);
    a.e_lo = k.err_lo, a.e_hi = k.err_hi, a.e_step = (k.err_hi - k.err_lo) / d->bins, a.e_norm = d->bins / (k.err_hi - k.err_lo);
    a.hist = (unsigned long long*)d->hist + (int64_t)c * 3 * d->bins;
    a.d_lo = k.dig_lo, a.d_w = k.dig_w, a.d_inv_w = 1.0 / k.dig_w, a.d_last = k.dig_lo + (double)(d->n_edges - 1) * k.dig_w;
    a.n_edges = d->n_edges;
    a.dig = (unsigned long long*)d->dig_count + (int64_t)c * nd;
    a.K = d->K, a.seed = d->seed, a.scatter = d->scatter ? (float2*)d->scatter + (int64_t)c * nd * d->K : nullptr;
}

// VEC: 16-byte loads when every plane, base and stride is a multiple of 4 elements; LDS: `words` counters fit the budget
template <int CY, class D>
int32_t launch(const KArgs<CY>& ka, const D* d, int64_t P, size_t words, int64_t rows, void* stream) {
    auto quad = [](const float* p, int64_t sb, int64_t st) { return !p || (((uintptr_t)p % 16) == 0 && sb % 4 == 0 && st % 4 == 0); };
    const bool vec = P % 4 == 0 && quad(d->y_pred, d->pred_stride_b, d->pred_stride_t) && quad(d->y, d->y_stride_b, d->y_stride_t) &&
                     quad(d->mask, ka.ch[0].m_sb, ka.ch[0].m_st);
    const size_t lds = words * sizeof(uint32_t);
    const dim3 grid((unsigned)rows), block(NT);
    hipStream_t s = (hipStream_t)stream;
    if (lds <= LDS_BUDGET) {
        if (vec) UCLSTM_LAUNCH((eval_stats_kernel<CY, true, true>), grid, block, lds, s, ka);
        else UCLSTM_LAUNCH((eval_stats_kernel<CY, false, true>), grid, block, lds, s, ka);
    } else {
        if (vec) UCLSTM_LAUNCH((eval_stats_kernel<CY, true, false>), grid, block, 0, s, ka);
        else UCLSTM_LAUNCH((eval_stats_kernel<CY, false, false>), grid, block, 0, s, ka);
    }
    return UCLSTM_OK;
}

Channel channel_of(const uclstm_eval_vec_desc* d, int c) {
    return {d->consts[c].y_scale, d->consts[c].trans_min, d->consts[c].trans_max, d->hist_lo[c], d->hist_hi[c],
            d->err_lo[c], d->err_hi[c], d->dig_lo[c], d->dig_w[c]};
}

template <int CY>
int32_t launch_vec(const uclstm_eval_vec_desc* d, int64_t cpf, int64_t rows, void* stream) {
    KArgs<CY> ka = {};
    for (int c = 0; c < CY; ++c) fill_channel(ka.ch[c], d, d->HW, cpf, c, channel_of(d, c));
    const bool pair = d->w_chan >= 0 && d->h_chan >= 0;
    PairArgs& v = ka.v;
    v.w_chan = pair ? d->w_chan : -1, v.h_chan = pair ? d->h_chan : -1;
    v.w_sign = (float)d->w_sign, v.h_sign = (float)d->h_sign;
    v.s_hi = d->speed_hi, v.s_step = d->speed_hi / d->bins, v.s_norm = d->bins / d->speed_hi;
    v.p_hi = d->epe_hi, v.p_step = d->epe_hi / d->bins, v.p_norm = d->bins / d->epe_hi;
    v.t_step = 360.0 / d->dir_bins, v.t_norm = d->dir_bins / 360.0;
    v.dir_bins = d->dir_bins, v.min_speed = (float)d->min_speed;
    v.vtable = d->vtable, v.vhist = (unsigned long long*)d->vhist, v.dir_hist = (unsigned long long*)d->dir_hist;
    // the speed and direction counters count towards the budget at every Cy
    const size_t words = (size_t)CY * (3 * (size_t)d->bins + 3 * (size_t)(d->n_edges + 1)) + 3 * (size_t)d->bins + (size_t)d->dir_bins;
    return launch<CY>(ka, d, d->HW, words, rows, stream);
}

}  // namespace

extern "C" int64_t uclstm_eval_stats_rows(int64_t P, int64_t frames) {
    if (P <= 0 || frames <= 0 || P >= ((int64_t)1 << 31) || frames >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;
    return rows_for(P, frames);
}

extern "C" int32_t uclstm_eval_stats(const uclstm_eval_desc* d, void* stream) {
    int64_t cpf, rows;
    if (!d || !shared_ok(d, d->P, 1, &cpf, &rows)) return UCLSTM_E_BADARG;
    const Channel k = {d->y_scale, d->trans_min, d->trans_max, d->hist_lo, d->hist_hi, d->err_lo, d->err_hi, d->dig_lo, d->dig_w};
    if (!channel_ok(d->transform, k)) return UCLSTM_E_BADARG;
    KArgs<1> ka = {};
    fill_channel(ka.ch[0], d, d->P, cpf, 0, k);
    return launch<1>(ka, d, d->P, 3 * (size_t)d->bins + 3 * (size_t)(d->n_edges + 1), rows, stream);
}

extern "C" int32_t uclstm_eval_stats_vec(const uclstm_eval_vec_desc* d, void* stream) {
    int64_t cpf, rows;
    if (!d || d->Cy < 1 || d->Cy > UCLSTM_VEC_MAX || !shared_ok(d, d->HW, d->Cy, &cpf, &rows)) return UCLSTM_E_BADARG;
    for (int c = 0; c < d->Cy; ++c)
        if (!channel_ok(d->transform, channel_of(d, c))) return UCLSTM_E_BADARG;
    if (d->w_chan < -1 || d->w_chan >= d->Cy || d->h_chan < -1 || d->h_chan >= d->Cy) return UCLSTM_E_BADARG;
    if (d->w_chan >= 0 && d->w_chan == d->h_chan) return UCLSTM_E_BADARG;
    if ((d->w_sign != 1 && d->w_sign != -1) || (d->h_sign != 1 && d->h_sign != -1)) return UCLSTM_E_BADARG;
    if (!(d->speed_hi > 0.0) || !(d->epe_hi > 0.0) || !(d->min_speed >= 0.0)) return UCLSTM_E_BADARG;
    if (d->dir_bins < 1 || d->dir_bins > 4096) return UCLSTM_E_BADARG;
    if (d->w_chan >= 0 && d->h_chan >= 0 && (!d->vtable || !d->vhist || !d->dir_hist)) return UCLSTM_E_BADARG;
    switch (d->Cy) {
        case 1: return launch_vec<1>(d, cpf, rows, stream);
        case 2: return launch_vec<2>(d, cpf, rows, stream);
        case 3: return launch_vec<3>(d, cpf, rows, stream);
        default: return launch_vec<4>(d, cpf, rows, stream);
    }
}
