// On-device augmentation of the resident dataset (flips, transpose, crop, time window) and the plane mover behind test-time
// averaging.  Every augmentation here is an index remap: out[i][j] = s[a][b] with (a, b) = (j, i) for codes with t, else (i, j);
// then a = Hc-1-a for v, b = Wc-1-b for h (code = h | v << 1 | t << 2: the eight elements of the dihedral group).  The per-pixel
// arithmetic is that of dataset_gather_transform_kernel (loss_optim.hip), applied AFTER the move: it commutes with the remap, so a
// batch is bit-identical to the plain kernel's batch moved with torch.flip / transpose / slicing.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int TS = 32;            // a block iteration is one TS x TS tile of ONE output frame: 4 pixels per thread
constexpr int TP = TS + 1;        // LDS row pitch in dwords: bank = (a/4) % 32 per 32-lane half, so tile[r][c] and tile[c][r] with
                                  // c = lane are both one dword per bank (row-wise: r*33 + c, column-wise: c*33 + r = c + r mod 32)

// The thread's four pixels of a tile, (row(k), col(k)), k = 0..3.  V = 1: rows tid/32 + 8k of column tid%32 (a 32-lane half is one
// row segment); V = 4: the four consecutive columns 4*(tid%8) + k of row tid/8 (one 16-byte access).
template <int V>
struct Slot {
    int u, w;
    __device__ __forceinline__ Slot() : u(V == 4 ? (int)threadIdx.x >> 3 : (int)threadIdx.x >> 5),
                                        w(V == 4 ? ((int)threadIdx.x & 7) * 4 : (int)threadIdx.x & 31) {}
    __device__ __forceinline__ int row(int k) const { return V == 4 ? u : u + 8 * k; }
    __device__ __forceinline__ int col(int k) const { return V == 4 ? w + k : w; }
};

// One tile of one move, uniform over the block.  The source pixel of output (i, j) is s[sa0 + sda * slow][sb0 + sdb * fast] with
// (slow, fast) = (i, j), or (j, i) for codes with t: `fast` runs along a source row.
struct D4Tile {
    int sa0, sda, sb0, sdb;       // v: sa0 = Hc-1, sda = -1;  h: sb0 = Wc-1, sdb = -1;  else 0, +1
    int S0, Slim, F0, Flim;       // tile origin and frame extent of the slow / fast output coordinate
    int I0, J0, Ho, Wo;           // tile origin and extent in output (i, j)
    bool h, tr;
};
__device__ __forceinline__ D4Tile d4_tile(int code, int Hc, int Wc, int ti, int tj) {
    D4Tile g;
    g.h = code & 1;
    g.tr = code & 4;
    g.sa0 = (code & 2) ? Hc - 1 : 0;
    g.sda = (code & 2) ? -1 : 1;
    g.sb0 = g.h ? Wc - 1 : 0;
    g.sdb = g.h ? -1 : 1;
    g.Ho = g.tr ? Wc : Hc;
    g.Wo = g.tr ? Hc : Wc;
    g.I0 = ti * TS;
    g.J0 = tj * TS;
    g.S0 = g.tr ? g.J0 : g.I0;
    g.Slim = Hc;
    g.F0 = g.tr ? g.I0 : g.J0;
    g.Flim = Wc;
    return g;
}

// Source values of the thread's slot, read along source rows for EVERY code (lanes follow `fast`, ascending or descending: one
// contiguous row segment per 32-lane half, or one 16-byte access per lane).  Unconditional loads from addresses clamped into the
// frame ("Branch-free loads").  s: the plane at the crop origin; pitch: the source row length.
// Codes without t: r[k] is the thread's output pixel (I0 + row(k), J0 + col(k)).  Codes with t: it is output pixel
// (I0 + col(k), J0 + row(k)), and d4_put / d4_get turn the tile.
template <int V>
__device__ __forceinline__ void d4_load(const float* __restrict__ s, int pitch, const D4Tile& g, float (&r)[4]) {
    const Slot<V> t;
    if constexpr (V == 4) {
        const int sl = min(g.S0 + t.u, g.Slim - 1), f4 = min(g.F0 + t.w, g.Flim - 4);
        const f32x4 e = *reinterpret_cast<const f32x4*>(s + (g.sa0 + g.sda * sl) * pitch + (g.h ? g.sb0 - 3 - f4 : f4));
        // h reverses the four values.  Not `h ? e[3 - k] : e[k]`: the compiler folds that select into the load and makes four 4-byte
        // loads at selected offsets of it; v_perm_b32 with a uniform selector (all of one operand) keeps the 16-byte load
#pragma unroll
        for (int k = 0; k < 4; ++k)
            r[k] = __uint_as_float(__builtin_amdgcn_perm(__float_as_uint(e[3 - k]), __float_as_uint(e[k]), g.h ? 0x07060504u : 0x03020100u));
    } else {
        const int b = g.sb0 + g.sdb * min(g.F0 + t.w, g.Flim - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = s[(g.sa0 + g.sda * min(g.S0 + t.row(k), g.Slim - 1)) * pitch + b];
    }
}
// the transposition: written row-wise as loaded, read column-wise (both conflict-free with the pitch TP, see above; for V = 4 a
// half holds 4 rows x 8 column groups of 4 and (row + col) mod 32 is again one dword per bank)
template <int V>
__device__ __forceinline__ void d4_put(float* __restrict__ tile, const float (&r)[4]) {
    const Slot<V> t;
#pragma unroll
    for (int k = 0; k < 4; ++k) tile[t.row(k) * TP + t.col(k)] = r[k];
}
template <int V>
__device__ __forceinline__ void d4_get(const float* __restrict__ tile, float (&r)[4]) {
    const Slot<V> t;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = tile[t.col(k) * TP + t.row(k)];
}
// the thread's slot in the output plane: element offset of pixel k (V = 4: of the 16-byte group, k = 0) and whether it is inside.
// A dead lane gets the clamped offset, so a read-modify-write may load from it unconditionally.
template <int V>
__device__ __forceinline__ int d4_out(const D4Tile& g, int k, bool& live) {
    const Slot<V> t;
    const int i = g.I0 + t.row(k), j = g.J0 + t.col(k);
    live = i < g.Ho && j < g.Wo;
    return min(i, g.Ho - 1) * g.Wo + min(j, g.Wo - V);
}

template <int V>
__device__ __forceinline__ void store_slot(float* __restrict__ p, const D4Tile& g, const float (&r)[4]) {
    bool live;
    if constexpr (V == 4) {
        const int o = d4_out<4>(g, 0, live);
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = r[k];
        if (live) *reinterpret_cast<f32x4*>(p + o) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int o = d4_out<1>(g, k, live);
            if (live) p[o] = r[k];
        }
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The host tables of a gather as ONE kernel argument (52 bytes of the kernarg segment for CYMAX = 1, 112 for UCLSTM_VEC_MAX:
// nothing to upload).  map[code]: byte c = the entry of output channel c (bits 0-2 source channel, bit 7 negate the raw value; a
// move acts on vector channels too: sign under mirrors, swap under transposes).  Every index into the arrays below is a
// compile-time constant (unrolled loops), so they stay scalar registers.
template <int CYMAX>
struct GatherTables {
    uint32_t map[8];
    float min_vel[CYMAX], max_vel[CYMAX], inv_yscale[CYMAX], tmin[CYMAX], inv_trange[CYMAX];
};

// the per-pixel target arithmetic of dataset_gather_transform_kernel; `flip` = 0x80000000 negates the RAW value first
__device__ __forceinline__ float target_px(float raw, uint32_t flip, int clip, float min_vel, float max_vel, int transform,
                                           float inv_yscale, float tmin, float inv_trange) {
    float w = __uint_as_float(__float_as_uint(raw) ^ flip);
    if (clip) w = fminf(fmaxf(w, min_vel), max_vel);
    return 2.f * (target_fwd(w, transform, inv_yscale) - tmin) * inv_trange - 1.f;
}

// dataset_gather_transform_kernel with a per-sequence remap, for y_all [n_seq][T_src][Cy][Hs][Ws]: output sequence o reads table
// row aug[o] = {code, oy, ox, t0}, uniform per block iteration like the sequence index, and clamped like it (code & 7, or & 3
// without flag bit 0; the window kept inside the source; on the 16-byte path ox rounded down to a multiple of 4) -- a bad table
// never becomes a wild read.  aug == NULL: code 0 at the origin of the source (the plain gather).
// The mask is taken at the SOURCE pixel: it travels with channel 0.  CT as in the plain kernel (2: all loads before the first store).
// CYMAX = 1 is the scalar target (and a one-channel vector dataset, which may still negate): Cy is the constant 1, so the tail
// loop and the channel clamps fold away.  CYMAX = UCLSTM_VEC_MAX: Cy >= 2 at run time; target channel 0 travels with the x channels
// exactly as the one target does, channels 1 .. Cy-1 follow, one plane at a time through tile[0].
// Their loads are NOT hoisted above the first store: with asinh the kernel is bound by the per-pixel arithmetic (three asinhf per
// 44 bytes where the scalar target has one per 28), and a channel's arithmetic then hides the next channel's loads; issuing all
// loads first measured 7 % slower at Cy = 3 (profiles/vector_targets_ab.txt).
// Output channel c reads the plane of source channel (entry & 7), clamped into [0, Cy) like everything else read from a table.
template <int V, int CT, int CYMAX>
__global__ __launch_bounds__(NT) void dataset_gather_tiles_kernel(
        const float* __restrict__ xa, const float* __restrict__ ya, const int64_t* __restrict__ idx, const int32_t* __restrict__ aug,
        int64_t n_seq, int n_chunks, FastDiv dTiles, FastDiv dTj, FastDiv dT, int T_src, int Crt, int Cyrt, int Hs, int Ws, int Ho,
        int Wo, int flags, float* __restrict__ x, float* __restrict__ y, float* __restrict__ mask, int transform, float inv_norm,
        int clip, GatherTables<CYMAX> tb) {
    __shared__ float tile[3][TS * TP];
    const int C = CT > 0 ? CT : Crt;
    const int Cy = CYMAX > 1 ? Cyrt : 1;
    const int T = (int)dT.d, HWs = Hs * Ws, HWo = Ho * Wo;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t f = fdiv((uint32_t)chunk, dTiles);           // output frame = o * T + t
        const uint32_t tl = (uint32_t)chunk - f * dTiles.d;
        const uint32_t ti = fdiv(tl, dTj);
        const uint32_t o = fdiv(f, dT);                             // output sequence
        int64_t row = idx ? idx[o] : (int64_t)o;
        row = row < 0 ? 0 : (row >= n_seq ? n_seq - 1 : row);
        int code = 0, oy = 0, ox = 0, t0 = 0;
        if (aug) {                                                  // uniform
            const int32_t* ar = aug + (int64_t)o * 4;
            code = ar[0] & ((flags & 1) ? 7 : 3);
            oy = clampi(ar[1], 0, Hs - Ho);
            ox = clampi(ar[2], 0, Ws - Wo);
            if (V == 4) ox &= ~3;
            t0 = clampi(ar[3], 0, T_src - T);
        }
        uint32_t mrow = tb.map[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) mrow = code == k ? tb.map[k] : mrow;
        const D4Tile g = d4_tile(code, Ho, Wo, (int)ti, (int)(tl - ti * dTj.d));
        const int64_t sf = row * T_src + t0 + (int64_t)(f - o * (uint32_t)T);   // source frame
        const int org = oy * Ws + ox;
        const float* xs = xa + sf * C * HWs + org;
        const float* ys = ya + sf * Cy * HWs + org;
        float* xd = x + (int64_t)f * C * HWo;
        float* yd = y + (int64_t)f * Cy * HWo;
        const int64_t od = (int64_t)f * HWo;
        float v[4], c0[4], m[4];
        d4_load<V>(ys + (int64_t)min((int)(mrow & 7u), Cy - 1) * HWs, Ws, g, v);
        d4_load<V>(xs, Ws, g, c0);
        if constexpr (CT > 0) {
            static_assert(CT <= 2, "one LDS plane per channel plus the target");
            float cc[CT > 1 ? CT - 1 : 1][4];
#pragma unroll
            for (int c = 1; c < CT; ++c) d4_load<V>(xs + (int64_t)c * HWs, Ws, g, cc[c - 1]);
            if (g.tr) {
                d4_put<V>(tile[0], v);
                d4_put<V>(tile[1], c0);
#pragma unroll
                for (int c = 1; c < CT; ++c) d4_put<V>(tile[1 + c], cc[c - 1]);
                __syncthreads();
                d4_get<V>(tile[0], v);
                d4_get<V>(tile[1], c0);
#pragma unroll
                for (int c = 1; c < CT; ++c) d4_get<V>(tile[1 + c], cc[c - 1]);
                __syncthreads();                                    // the next planes write the tiles again
            }
#pragma unroll
            for (int c = 1; c < CT; ++c) {
#pragma unroll
                for (int k = 0; k < 4; ++k) cc[c - 1][k] *= inv_norm;
                store_slot<V>(xd + (int64_t)c * HWo, g, cc[c - 1]);
            }
        } else {
            if (g.tr) {
                d4_put<V>(tile[0], v);
                d4_put<V>(tile[1], c0);
                __syncthreads();
                d4_get<V>(tile[0], v);
                d4_get<V>(tile[1], c0);
            }
            for (int c = 1; c < C; ++c) {
                float r[4];
                d4_load<V>(xs + (int64_t)c * HWs, Ws, g, r);
                if (g.tr) {
                    d4_put<V>(tile[2], r);
                    __syncthreads();
                    d4_get<V>(tile[2], r);
                    __syncthreads();
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] *= inv_norm;
                store_slot<V>(xd + (int64_t)c * HWo, g, r);
            }
            if (g.tr) __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            m[k] = c0[k] > 1.1f ? 1.f : 0.f;
            c0[k] *= inv_norm;
            v[k] = target_px(v[k], (mrow & 0x80u) << 24, clip, tb.min_vel[0], tb.max_vel[0], transform, tb.inv_yscale[0], tb.tmin[0],
                             tb.inv_trange[0]);
        }
        store_slot<V>(xd, g, c0);
        store_slot<V>(mask + od, g, m);
        store_slot<V>(yd, g, v);
#pragma unroll
        for (int c = 1; c < CYMAX; ++c) {
            if (c < Cy) {                                           // uniform
                const uint32_t e = mrow >> (8 * c);
                float r[4];
                d4_load<V>(ys + (int64_t)min((int)(e & 7u), Cy - 1) * HWs, Ws, g, r);
                if (g.tr) {
                    d4_put<V>(tile[0], r);
                    __syncthreads();
                    d4_get<V>(tile[0], r);
                    __syncthreads();
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    r[k] = target_px(r[k], (e & 0x80u) << 24, clip, tb.min_vel[c], tb.max_vel[c], transform, tb.inv_yscale[c], tb.tmin[c],
                                     tb.inv_trange[c]);
                store_slot<V>(yd + (int64_t)c * HWo, g, r);
            }
        }
    }
}

// dst = (accumulate ? dst : 0) + scale * (+-move(src) + off[c]) over frames of Cy planes of H x W: the same tile mover, one plane
// per block iteration's tile.  Plane p = f * Cy + c reads the plane of its source channel; map: byte c = the entry of output
// channel c, as above.  CYMAX = 1: Cy is the constant 1 and p is the frame (the scalar mover, and a one-channel vector frame).
template <int CYMAX>
struct PlaneTables {
    uint32_t map;
    float off[CYMAX];
};
template <int V, int CYMAX>
__global__ __launch_bounds__(NT) void plane_d4_kernel(const float* __restrict__ src, float* __restrict__ dst, int n_chunks, FastDiv dTiles,
                                                      FastDiv dTj, FastDiv dCy, int H, int W, int code, int accumulate, float scale,
                                                      PlaneTables<CYMAX> tb) {
    __shared__ float tile[TS * TP];
    const int HW = H * W, Cy = CYMAX > 1 ? (int)dCy.d : 1;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t p = fdiv((uint32_t)chunk, dTiles);
        const uint32_t tl = (uint32_t)chunk - p * dTiles.d;
        const uint32_t ti = fdiv(tl, dTj);
        const uint32_t f = CYMAX > 1 ? fdiv(p, dCy) : p;
        const int c = (int)(p - f * (uint32_t)Cy);
        uint32_t e = tb.map;
        float off = tb.off[0];
#pragma unroll
        for (int k = 1; k < CYMAX; ++k) {
            e = c == k ? tb.map >> (8 * k) : e;
            off = c == k ? tb.off[k] : off;
        }
        const uint32_t flip = (e & 0x80u) << 24;
        const D4Tile g = d4_tile(code, H, W, (int)ti, (int)(tl - ti * dTj.d));
        float r[4], d[4];
        d4_load<V>(src + ((int64_t)f * Cy + min((int)(e & 7u), Cy - 1)) * HW, W, g, r);
        float* out = dst + (int64_t)p * HW;
        if (accumulate) {                                           // uniform; dead lanes read their clamped slot
            bool live;
            if constexpr (V == 4) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(out + d4_out<4>(g, 0, live));
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = q[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = out[d4_out<1>(g, k, live)];
            }
        }
        if (g.tr) {
            d4_put<V>(tile, r);
            __syncthreads();
            d4_get<V>(tile, r);
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {                               // off = -0.f (uclstm_plane_d4) leaves every value as it is, -0.f too
            const float t = scale * (__uint_as_float(__float_as_uint(r[k]) ^ flip) + off);
            r[k] = accumulate ? d[k] + t : t;
        }
        store_slot<V>(out, g, r);
    }
}

inline int tiles_of(int n) { return (n + TS - 1) / TS; }

// the kernel tables from the host arrays of an entry point (chan_map NULL: identity; channels past Cy repeat channel 0)
template <int CYMAX>
GatherTables<CYMAX> gather_tables(int Cy, const int8_t* chan_map, const uclstm_target_consts* consts, int transform) {
    GatherTables<CYMAX> tb;
    for (int c = 0; c < CYMAX; ++c) {
        const uclstm_target_consts& k = consts[c < Cy ? c : 0];
        tb.min_vel[c] = k.min_vel;
        tb.max_vel[c] = k.max_vel;
        tb.inv_yscale[c] = transform != 0 ? 1.0f / k.y_scale : 1.0f;
        tb.tmin[c] = k.trans_min;
        tb.inv_trange[c] = 1.0f / (k.trans_max - k.trans_min);
    }
    for (int code = 0; code < 8; ++code) {
        tb.map[code] = 0;
        for (int c = 0; c < Cy; ++c) tb.map[code] |= (uint32_t)(chan_map ? (uint8_t)chan_map[code * Cy + c] : (uint8_t)c) << (8 * c);
    }
    return tb;
}
template <int CYMAX>
PlaneTables<CYMAX> plane_tables(int Cy, const int8_t* chan_map, const float* offset) {
    PlaneTables<CYMAX> tb;
    tb.map = 0;
    for (int c = 0; c < CYMAX; ++c) {
        if (c < Cy) tb.map |= (uint32_t)(chan_map ? (uint8_t)chan_map[c] : (uint8_t)c) << (8 * c);
        tb.off[c] = (offset && c < Cy) ? offset[c] : 0.f;
    }
    return tb;
}

// What the two gather entry points share: the argument checks, the 2^31 limits, the 16-byte-path condition, the grid and the
// dispatch.  The caller vouches for 1 <= Cy <= UCLSTM_VEC_MAX and consts [Cy].
int32_t gather_tiles(const float* x_all, const float* y_all, const int64_t* idx, const int32_t* aug, int64_t n_seq, int64_t n_out,
                     int32_t T_src, int32_t T_out, int32_t C, int32_t Cy, int32_t Hs, int32_t Ws, int32_t Ho, int32_t Wo, int32_t flags,
                     const int8_t* chan_map, float* x, float* y, float* mask, int32_t transform, float norm_const, int32_t clip,
                     const uclstm_target_consts* consts, void* stream) {
    if (!x_all || !y_all || !x || !y || !mask || n_seq <= 0 || n_out <= 0 || T_src <= 0 || T_out <= 0 || C <= 0 || Hs <= 0 || Ws <= 0 ||
        Ho <= 0 || Wo <= 0 || Ho > Hs || Wo > Ws || T_out > T_src || flags < 0 || flags > 3 || ((flags & 1) && Ho != Wo) ||
        transform < 0 || transform > 2 || norm_const == 0.f || (!idx && n_out > n_seq))
        return UCLSTM_E_BADARG;
    for (int c = 0; c < Cy; ++c)
        if (consts[c].trans_max == consts[c].trans_min || (transform != 0 && !(consts[c].y_scale > 0.f))) return UCLSTM_E_BADARG;
    if ((int64_t)Cy * Hs * Ws >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;    // Ho * Wo <= Hs * Ws: offsets inside a frame are ints
    const int64_t frame_px = (int64_t)T_out * Cy * ((int64_t)Ho * Wo);         // < 2^62 + 2
    if (n_out > (((int64_t)1 << 31) - 1) / frame_px) return UCLSTM_E_BADARG;    // n_out * T_out * Cy * Ho * Wo >= 2^31
    // the 16-byte path must be valid for the whole launch: every row, every window start and every pointer on a 16-byte boundary
    const bool vec = Ws % 4 == 0 && Wo % 4 == 0 && (flags & 2) &&
                     (((uintptr_t)x_all | (uintptr_t)y_all | (uintptr_t)x | (uintptr_t)y | (uintptr_t)mask) % 16) == 0;
    const int ntj = tiles_of(Wo), tiles = tiles_of(Ho) * ntj;
    const int64_t n_chunks = n_out * T_out * tiles;                            // <= n_out * T_out * Ho * Wo < 2^31
    const int grid = (int)(n_chunks < 2048 ? n_chunks : 2048);
#define UCLSTM_GATHER_LAUNCH(V, CT, CYMAX)                                                                                              \
    UCLSTM_LAUNCH((dataset_gather_tiles_kernel<V, CT, CYMAX>), dim3(grid), dim3(NT), 0, (hipStream_t)stream, x_all, y_all, idx, aug,     \
                  n_seq, (int)n_chunks, make_fastdiv(tiles), make_fastdiv(ntj), make_fastdiv(T_out), T_src, C, Cy, Hs, Ws, Ho, Wo, flags, \
                  x, y, mask, transform, 1.0f / norm_const, clip, gather_tables<CYMAX>(Cy, chan_map, consts, transform))
#define UCLSTM_GATHER_CT(V, CYMAX)                  \
    do {                                            \
        if (C == 2) UCLSTM_GATHER_LAUNCH(V, 2, CYMAX); \
        else UCLSTM_GATHER_LAUNCH(V, 0, CYMAX);     \
    } while (0)
    if (Cy == 1) {                                                              // the scalar target's own instantiations
        if (vec) UCLSTM_GATHER_CT(4, 1);
        else UCLSTM_GATHER_CT(1, 1);
    } else {
        if (vec) UCLSTM_GATHER_CT(4, UCLSTM_VEC_MAX);
        else UCLSTM_GATHER_CT(1, UCLSTM_VEC_MAX);
    }
#undef UCLSTM_GATHER_CT
#undef UCLSTM_GATHER_LAUNCH
    return UCLSTM_OK;
}

// the same for the two plane movers; the caller vouches for 1 <= Cy <= UCLSTM_VEC_MAX
int32_t plane_tiles(const float* src, float* dst, int64_t n_frames, int32_t Cy, int32_t H, int32_t W, int32_t code, const int8_t* chan_map,
                    const float* offset, int32_t accumulate, float scale, void* stream) {
    if (!src || !dst || n_frames <= 0 || H <= 0 || W <= 0 || code < 0 || code > 7) return UCLSTM_E_BADARG;
    const int64_t plane_px = (int64_t)H * W;
    if (plane_px >= ((int64_t)1 << 31) / Cy || n_frames > (((int64_t)1 << 31) - 1) / (plane_px * Cy)) return UCLSTM_E_BADARG;
    const int Ho = (code & 4) ? W : H, Wo = (code & 4) ? H : W;
    // rows of both planes on 16-byte boundaries; with t the loads also run in groups of 4 along the output's rows (Ho = W)
    const bool vec = W % 4 == 0 && Wo % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) % 16) == 0;
    const int ntj = tiles_of(Wo), tiles = tiles_of(Ho) * ntj;
    const int64_t n_chunks = n_frames * Cy * tiles;
    const int grid = (int)(n_chunks < 2048 ? n_chunks : 2048);
#define UCLSTM_PLANE_LAUNCH(V, CYMAX)                                                                                                   \
    UCLSTM_LAUNCH((plane_d4_kernel<V, CYMAX>), dim3(grid), dim3(NT), 0, (hipStream_t)stream, src, dst, (int)n_chunks, make_fastdiv(tiles), \
                  make_fastdiv(ntj), make_fastdiv(Cy), H, W, code, accumulate, scale, plane_tables<CYMAX>(Cy, chan_map, offset))
    if (Cy == 1) {
        if (vec) UCLSTM_PLANE_LAUNCH(4, 1);
        else UCLSTM_PLANE_LAUNCH(1, 1);
    } else {
        if (vec) UCLSTM_PLANE_LAUNCH(4, UCLSTM_VEC_MAX);
        else UCLSTM_PLANE_LAUNCH(1, UCLSTM_VEC_MAX);
    }
#undef UCLSTM_PLANE_LAUNCH
    return UCLSTM_OK;
}

}  // namespace

extern "C" int32_t uclstm_dataset_gather_augment(const float* x_all, const float* y_all, const int64_t* idx, const int32_t* aug,
                                                 int64_t n_seq, int64_t n_out, int32_t T_src, int32_t T_out, int32_t C, int32_t Hs,
                                                 int32_t Ws, int32_t Ho, int32_t Wo, int32_t flags, float* x, float* y, float* mask,
                                                 int32_t transform, float norm_const, float min_vel, float max_vel, int32_t clip,
                                                 float y_scale, float trans_min, float trans_max, void* stream) {
    if (!aug) return UCLSTM_E_BADARG;
    const uclstm_target_consts k = {min_vel, max_vel, y_scale, trans_min, trans_max};
    return gather_tiles(x_all, y_all, idx, aug, n_seq, n_out, T_src, T_out, C, 1, Hs, Ws, Ho, Wo, flags, NULL, x, y, mask, transform,
                        norm_const, clip, &k, stream);
}

extern "C" int32_t uclstm_dataset_gather_vec(const float* x_all, const float* y_all, const int64_t* idx, const int32_t* aug, int64_t n_seq,
                                             int64_t n_out, int32_t T_src, int32_t T_out, int32_t C, int32_t Cy, int32_t Hs, int32_t Ws,
                                             int32_t Ho, int32_t Wo, int32_t flags, const int8_t* chan_map, float* x, float* y,
                                             float* mask, int32_t transform, float norm_const, int32_t clip,
                                             const uclstm_target_consts* consts, void* stream) {
    if (!consts || Cy < 1 || Cy > UCLSTM_VEC_MAX) return UCLSTM_E_BADARG;
    return gather_tiles(x_all, y_all, idx, aug, n_seq, n_out, T_src, T_out, C, Cy, Hs, Ws, Ho, Wo, flags, chan_map, x, y, mask, transform,
                        norm_const, clip, consts, stream);
}

extern "C" int32_t uclstm_plane_d4(const float* src, float* dst, int64_t n_planes, int32_t H, int32_t W, int32_t code,
                                   int32_t accumulate, float scale, void* stream) {
    static const float no_offset = -0.f;                                        // v + -0.f is v for every v, v = -0.f included
    return plane_tiles(src, dst, n_planes, 1, H, W, code, NULL, &no_offset, accumulate, scale, stream);
}

extern "C" int32_t uclstm_plane_d4_vec(const float* src, float* dst, int64_t n_frames, int32_t Cy, int32_t H, int32_t W, int32_t code,
                                       const int8_t* chan_map, const float* offset, int32_t accumulate, float scale, void* stream) {
    if (Cy < 1 || Cy > UCLSTM_VEC_MAX) return UCLSTM_E_BADARG;
    return plane_tiles(src, dst, n_frames, Cy, H, W, code, chan_map, offset, accumulate, scale, stream);
}
