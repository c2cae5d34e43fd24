// Moving-sprite batches rendered on the device (digits/build_moving_mnist.py:16-47): D glyphs per sequence move with integer
// velocities and bounce off the frame; frame = glyph byte / 255 where the byte is non-zero (a later sprite overwrites), the velocity
// map adds the sprite's CURRENT vx at the same pixels.  Positions and velocities are integers and a frame value is a byte over 255,
// so the batch is bit-identical to the host generator's.  Only writes go to memory: x, y, mask (and optionally the reference's own
// two-plane layout) -- every element of every output is written, background included.
//
// One block (one wave) owns NT pixel groups of ONE sequence and walks time forward, one trajectory step per frame: lane d walks
// sprite d in registers and publishes its position through LDS.  The sequence's D glyphs are staged once in LDS as zero-padded rows
// and reused for all T frames.
#include "common.h"

namespace {

constexpr int NT = 64;            // one wave per block: [32,20,2,64,64] is 512 blocks of 1024 / 64 groups, two per CU
constexpr int MAXD = 8;
constexpr int MAXG = 64;          // glyph rows / columns
constexpr int PADL = 4;           // zero bytes in front of a glyph row in LDS (and at least 4 behind it)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// LDS image: glyph d, row r at byte (d * gh + r) * pitch, as [PADL zeros][gw bytes][>= 4 zeros], pitch % 4 == 0, plus 4 bytes of
// slack behind the last row.  A group of V pixels whose first glyph column is dx in [-V, gw] (clamped into that range: a group
// further away reads the padding) takes its V bytes from ONE unconditional read; bytes outside the glyph are zero = transparent.
template <int V>
__device__ __forceinline__ uint32_t glyph_bytes(const uint32_t* __restrict__ glyphs, int row_byte, int dx, int gw) {
    if constexpr (V == 4) {
        const int a = row_byte + PADL + clampi(dx, -4, gw);
        const uint32_t lo = glyphs[a >> 2], hi = glyphs[(a >> 2) + 1];     // hi: inside the row's padding or the slack
        return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)a & 3u);      // ({hi, lo} >> 8 * (a & 3)): the four bytes at a
    } else {
        return reinterpret_cast<const uint8_t*>(glyphs)[row_byte + PADL + clampi(dx, -1, gw)];
    }
}

template <int V>
__device__ __forceinline__ void store_group(float* __restrict__ p, const float (&r)[V]) {
    if constexpr (V == 4) {
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = r[k];
        *reinterpret_cast<f32x4*>(p) = v;
    } else {
        p[0] = r[0];
    }
}

// table: int32 [n_out][D][5] rows {glyph, x0, y0, vx, vy}, clamped on the way in (glyph into the bank, the start into the frame,
// speeds into [-127, 127]): a bad table never becomes a wild access.  V: pixels per thread (4: 16-byte stores); CT: compile-time
// channel count (0: run-time loop).  dGroups: groups per row (W / V); dFill: dwords (fill_vec) or bytes of a padded LDS row.
template <int V, int CT>
__global__ __launch_bounds__(NT) void sprites_render_kernel(
        const uint8_t* __restrict__ bank, int n_glyph, int gh, int gw, int pitch, int fill_vec, FastDiv dFill,
        const int32_t* __restrict__ table, FastDiv dBands, FastDiv dGroups, int D, int T, int Crt, int H, int W, float v_scale,
        float* __restrict__ x, float* __restrict__ y, float* __restrict__ mask, float* __restrict__ raw) {
    extern __shared__ uint32_t glyphs[];
    __shared__ int4 state[2][MAXD];                                 // {x, y, vx, -} of the D sprites, for even / odd frames
    const int C = CT > 0 ? CT : Crt;
    const int tid = (int)threadIdx.x;
    const uint32_t o = fdiv(blockIdx.x, dBands);                    // output sequence
    const uint32_t band = blockIdx.x - o * dBands.d;
    const int32_t* __restrict__ rows = table + (int64_t)o * D * 5;
    const int gsz = gh * gw, img = gh * pitch;                      // bytes of a glyph in the bank / in LDS

    // ---- the D glyphs into LDS, padding included: every byte of the image is written here
    for (int d = 0; d < D; ++d) {
        const uint8_t* __restrict__ src = bank + (int64_t)clampi(rows[d * 5], 0, n_glyph - 1) * gsz;
        if (fill_vec) {                                             // gw % 4 == 0 and a 4-byte aligned bank: whole dwords
            const int pq = pitch >> 2;
            for (int q = tid; q < gh * pq; q += NT) {
                const int r = (int)fdiv((uint32_t)q, dFill), c = (q - r * pq) * 4 - PADL;
                const uint32_t v = *reinterpret_cast<const uint32_t*>(src + r * gw + clampi(c, 0, gw - 4));
                glyphs[d * (img >> 2) + q] = (c >= 0 && c < gw) ? v : 0u;
            }
        } else {
            uint8_t* g8 = reinterpret_cast<uint8_t*>(glyphs);
            for (int i = tid; i < img; i += NT) {
                const int r = (int)fdiv((uint32_t)i, dFill), c = i - r * pitch - PADL;
                const uint8_t v = src[r * gw + clampi(c, 0, gw - 1)];
                g8[d * img + i] = (c >= 0 && c < gw) ? v : (uint8_t)0;
            }
        }
    }
    if (tid == 0) glyphs[(D * img) >> 2] = 0u;                      // the slack
    __syncthreads();

    // ---- trajectories: lane d < D owns sprite d and keeps {x, y, vx, vy} in registers for the whole walk (the other lanes walk a copy of
    // the last sprite, which nobody reads); every frame the owners publish their state in LDS, double-buffered: ONE barrier per frame
    const int32_t* __restrict__ mine = rows + min(tid, D - 1) * 5;
    int px = clampi(mine[1], 0, W - gw), py = clampi(mine[2], 0, H - gh);
    int vx = clampi(mine[3], -127, 127), vy = clampi(mine[4], -127, 127);

    // ---- the thread's V pixels; a lane past the frame computes the last group and stores nothing
    const uint32_t n_groups = (uint32_t)H * dGroups.d, gid0 = band * NT + (uint32_t)tid;
    const bool live = gid0 < n_groups;
    const uint32_t gid = live ? gid0 : n_groups - 1;
    const int r = (int)fdiv(gid, dGroups), c0 = (int)(gid - (uint32_t)r * dGroups.d) * V;
    const int pix = r * W + c0;
    const int64_t HW = (int64_t)H * W;

    for (int t = 0; t < T; ++t) {
        if (tid < D) state[t & 1][tid] = make_int4(px, py, vx, 0);
        __syncthreads();
        uint32_t fb[V];           // the byte on top (0: background)
        int vm[V];                // sum of vx over the sprites that cover the pixel
#pragma unroll
        for (int k = 0; k < V; ++k) fb[k] = 0u, vm[k] = 0;
        for (int d = 0; d < D; ++d) {
            const int4 s = state[t & 1][d];                         // one address for the whole wave: a broadcast read
            const int dy = r - s.y;
            uint32_t w = glyph_bytes<V>(glyphs, (d * gh + clampi(dy, 0, gh - 1)) * pitch, c0 - s.x, gw);
            w = (uint32_t)dy < (uint32_t)gh ? w : 0u;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const uint32_t b = (w >> (8 * k)) & 255u;
                fb[k] = b ? b : fb[k];
                vm[k] += b ? s.z : 0;
            }
        }
        float fr[V], tv[V], mk[V], vv[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            fr[k] = (float)fb[k] / 255.0f;                          // IEEE divisions: the host's float32(b / 255.0), vmap / v_scale
            vv[k] = (float)vm[k];
            tv[k] = vv[k] / v_scale;
            mk[k] = fb[k] ? 1.f : 0.f;
        }
        if (live) {
            const int64_t f = (int64_t)o * T + t;
            float* xd = x + f * C * HW + pix;
            if constexpr (CT > 0) {
#pragma unroll
                for (int c = 0; c < CT; ++c) store_group<V>(xd + c * HW, fr);
            } else {
                for (int c = 0; c < C; ++c) store_group<V>(xd + c * HW, fr);
            }
            store_group<V>(y + f * HW + pix, tv);
            store_group<V>(mask + f * HW + pix, mk);
            if (raw) {                                              // uniform
                store_group<V>(raw + f * 2 * HW + pix, fr);
                store_group<V>(raw + (f * 2 + 1) * HW + pix, vv);
            }
        }
        // one step: no closed form, the clamp drops the overshoot
        px += vx;
        py += vy;
        if (px < 0 || px > W - gw) {
            vx = -vx;
            px = clampi(px, 0, W - gw);
        }
        if (py < 0 || py > H - gh) {
            vy = -vy;
            py = clampi(py, 0, H - gh);
        }
    }
}

}  // namespace

extern "C" int32_t uclstm_sprites_render(const uint8_t* bank, int32_t n_glyph, int32_t gh, int32_t gw, const int32_t* table,
                                         int64_t n_out, int32_t D, int32_t T, int32_t C, int32_t H, int32_t W, float v_scale,
                                         float* x, float* y, float* mask, float* raw, void* stream) {
    if (!bank || !table || !x || !y || !mask || n_glyph <= 0 || gh <= 0 || gw <= 0 || gh > MAXG || gw > MAXG || H <= 0 || W <= 0 ||
        gh > H || gw > W || D < 1 || D > MAXD || T < 1 || C < 1 || n_out <= 0 || !(v_scale != 0.f))
        return UCLSTM_E_BADARG;
    const int64_t HW = (int64_t)H * W;
    if (HW >= ((int64_t)1 << 31)) return UCLSTM_E_BADARG;                       // offsets inside a frame are ints
    if (n_out > (((int64_t)1 << 31) - 1) / ((int64_t)T * HW)) return UCLSTM_E_BADARG;   // frames, blocks and n_out * D * 5 stay below 2^31
    // the 16-byte path must be valid for the whole launch: every row of every plane and every pointer on a 16-byte boundary
    const bool vec = W % 4 == 0 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)mask | (uintptr_t)raw) % 16) == 0;
    const int per_row = vec ? W / 4 : W;
    const int64_t bands = ceil_div64((int64_t)H * per_row, NT);
    const int64_t grid = n_out * bands;                                        // <= n_out * H * W < 2^31
    const int pitch = round_up32(gw + PADL + 4, 4);
    const int fill_vec = gw % 4 == 0 && (uintptr_t)bank % 4 == 0;
    const size_t lds = (size_t)D * gh * pitch + 4;                             // <= 8 * 64 * 72 + 4 bytes
#define UCLSTM_SPRITES_LAUNCH(V, CT)                                                                                                  \
    UCLSTM_LAUNCH((sprites_render_kernel<V, CT>), dim3((unsigned)grid), dim3(NT), lds, (hipStream_t)stream, bank, n_glyph, gh, gw,    \
                  pitch, fill_vec, make_fastdiv(fill_vec ? pitch / 4 : pitch), table, make_fastdiv((uint32_t)bands),                  \
                  make_fastdiv(per_row), D, T, C, H, W, v_scale, x, y, mask, raw)
    if (vec) {
        if (C == 2) UCLSTM_SPRITES_LAUNCH(4, 2);
        else UCLSTM_SPRITES_LAUNCH(4, 0);
    } else {
        if (C == 2) UCLSTM_SPRITES_LAUNCH(1, 2);
        else UCLSTM_SPRITES_LAUNCH(1, 0);
    }
#undef UCLSTM_SPRITES_LAUNCH
    return UCLSTM_OK;
}
