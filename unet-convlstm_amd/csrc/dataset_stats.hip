// Dataset statistics on the device: exact k-th order statistics of an f32 array by radix select, and min / max / counts.
//
// Both work on the order-preserving u32 image of an f32 ("key"): all bits inverted for negatives, the sign bit set for
// non-negatives; -0.0 is +0.0 first (numpy compares them equal) and NaNs are counted and kept out of every histogram.  The `abs`
// kind clears the sign before that.  Everything that is added is an integer (LDS and global integer atomics), so every result is
// a pure function of the multiset of inputs: no run-to-run variation, whatever the order of the blocks.
//
// Select: most significant digit first, 11 / 11 / 10 bits.  One pass reads the data ONCE for all slots: a block keeps one u32
// histogram per slot in LDS (8 slots x 2048 bins x 4 B = 64 KiB, the most one block may ask for without an opt-in) and flushes
// its non-zero bins into the u64 counters of the workspace.  Slots of one kind whose decided digits agree share one histogram
// (their "leader"), so the usual two-sided percentile pair costs two histograms in pass 0, not one per slot.  A one-block narrow
// kernel then walks each slot's histogram, fixes the slot's next digit and the rank that remains below it, and clears the
// counters.  Nothing is read back between the passes.
//
// Targets here are mostly exact zeros, which would put all 64 lanes of a wave on one LDS word.  wave_hist_add therefore merges
// inside the wave first: the lanes whose digit equals the first pending lane's are found with one ballot and added once, as
// their population count; whatever is left after that round adds for itself.  A lane whose four elements of a 16-byte
// load agree goes in with weight 4, so a constant input costs one LDS add per wave and load.
#include "common.h"

#ifndef UCLSTM_ACT_F16

namespace {

constexpr int NT = 256;
constexpr int MAX_SLOTS = UCLSTM_SELECT_MAX_SLOTS;
constexpr int BINS = UCLSTM_SELECT_BINS;                  // pitch of a slot's counters in the workspace; pass 2 uses the first 1024
// Ballot rounds of wave_hist_add before the lanes that are left add for themselves, and 16-byte loads a lane has in flight.
// Measured on 67 M elements, 6 slots, pass 0 (profiles/dataset_stats_ab.txt): rounds 1 / 2 / 4 / 8 = 178 / 236 / 560 / 997 us on
// random normal data -- a round costs more than the LDS conflicts it removes once the most frequent digit is gone; loads 1 / 2 / 4
// = 255 / 236 / 228 us at 2 rounds.
constexpr int MERGE_ROUNDS = 1;
constexpr int QUADS = 2;
constexpr int BLOCK_ELEMS = 1 << 16;                      // a block zeroes and flushes up to 64 KiB of LDS: give it at least this much to read
constexpr int LDS_PER_CU = 160 << 10;
constexpr uint32_t STATE_MAGIC = 0x53454c31u;             // "SEL1"
constexpr unsigned long long NO_LEADER = ~0ull;

typedef unsigned long long u64;

__host__ __device__ constexpr int pass_bins(int pass) { return pass == 2 ? 1024 : 2048; }
__host__ __device__ constexpr int pass_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }

__device__ __forceinline__ bool bits_nan(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ uint32_t key_signed(uint32_t b) {
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint32_t key_abs(uint32_t b) { return (b & 0x7fffffffu) | 0x80000000u; }
__device__ __forceinline__ uint32_t key_bits(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// h[d] += w for every lane with act, as few LDS adds as the wave's digits allow (see the head of the file).  Called by whole waves.
__device__ __forceinline__ void wave_hist_add(uint32_t* h, uint32_t d, bool act, int lane, uint32_t w) {
    u64 todo = __ballot(act);
    for (int r = 0; r < MERGE_ROUNDS && todo; ++r) {
        const int first = __ffsll((long long)todo) - 1;
        const uint32_t df = (uint32_t)__shfl((int)d, first);
        const u64 same = __ballot(act && d == df);
        if (lane == first) atomicAdd(h + df, w * (uint32_t)__popcll(same));
        act = act && d != df;
        todo &= ~same;
    }
    if (act) atomicAdd(h + d, w);
}

struct SlotSet {
    uint32_t prefix[MAX_SLOTS];       // the digits decided so far, in place, lower bits zero
    uint32_t lead_mask;               // slots that own a histogram in this pass
    uint32_t abs_mask;
    int n_slots;
};

template <int PASS>
__device__ __forceinline__ bool slot_digit(const SlotSet& S, int s, uint32_t bits, uint32_t& d) {
    const uint32_t k = (S.abs_mask >> s & 1) ? key_abs(bits) : key_signed(bits);
    d = (k >> pass_shift(PASS)) & (pass_bins(PASS) - 1);
    if (PASS == 0) return true;
    return (k >> pass_shift(PASS - 1)) == (S.prefix[s] >> pass_shift(PASS - 1));
}

// One 16-byte load of every lane of a wave into the histograms of the slots that own one; returns the lane's NaNs.
template <int PASS>
__device__ __forceinline__ uint32_t hist_quad(const SlotSet& S, uint32_t* lds, uint4 e, bool valid, int lane) {
    constexpr int NB = pass_bins(PASS);
    const bool n0 = bits_nan(e.x), n1 = bits_nan(e.y), n2 = bits_nan(e.z), n3 = bits_nan(e.w);
#pragma unroll
    for (int s = 0; s < MAX_SLOTS; ++s) {
        if (!(S.lead_mask >> s & 1)) continue;
        uint32_t d0, d1, d2, d3;
        const bool m0 = slot_digit<PASS>(S, s, e.x, d0) && valid && !n0;
        const bool m1 = slot_digit<PASS>(S, s, e.y, d1) && valid && !n1;
        const bool m2 = slot_digit<PASS>(S, s, e.z, d2) && valid && !n2;
        const bool m3 = slot_digit<PASS>(S, s, e.w, d3) && valid && !n3;
        if (PASS > 0 && !__ballot(m0 || m1 || m2 || m3)) continue;          // nothing of this load shares the slot's digits: the usual case
        uint32_t* h = lds + s * NB;
        const bool uni = m0 && m1 && m2 && m3 && d0 == d1 && d1 == d2 && d2 == d3;
        wave_hist_add(h, d0, uni, lane, 4);
        wave_hist_add(h, d0, m0 && !uni, lane, 1);
        wave_hist_add(h, d1, m1 && !uni, lane, 1);
        wave_hist_add(h, d2, m2 && !uni, lane, 1);
        wave_hist_add(h, d3, m3 && !uni, lane, 1);
    }
    return valid ? (uint32_t)n0 + n1 + n2 + n3 : 0u;
}

template <int PASS>
__global__ __launch_bounds__(NT) void select_hist_kernel(const float* __restrict__ v, int head, int nvec, int tail, u64* __restrict__ ws,
                                                         int n_slots, uint32_t abs_mask) {
    extern __shared__ uint32_t lds[];                     // [n_slots][bins]
    constexpr int NB = pass_bins(PASS);
    const int tid = threadIdx.x, lane = tid & 63;
    SlotSet S;
    S.n_slots = n_slots, S.abs_mask = abs_mask, S.lead_mask = 0;
#pragma unroll
    for (int s = 0; s < MAX_SLOTS; ++s) {
        S.prefix[s] = s < n_slots ? (uint32_t)ws[UCLSTM_SELECT_WS_PREFIX + s] : 0u;
        if (s < n_slots && ws[UCLSTM_SELECT_WS_LEADER + s] == (u64)s) S.lead_mask |= 1u << s;
    }
    for (int i = tid; i < n_slots * NB; i += NT) lds[i] = 0;
    __syncthreads();

    uint32_t nan = 0;
    // 16-byte body: whole waves walk the quads, so that every lane reaches every ballot; QUADS loads are in flight per lane
    const uint4* __restrict__ q = reinterpret_cast<const uint4*>(v + head);
    const int stride = gridDim.x * NT * QUADS;
    for (int base = (blockIdx.x * NT + (tid & ~63)) * QUADS; base < nvec; base += stride) {
        uint4 e[QUADS];
#pragma unroll
        for (int u = 0; u < QUADS; ++u) {
            const int i = base + u * 64 + lane;
            e[u] = i < nvec ? q[i] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < QUADS; ++u) nan += hist_quad<PASS>(S, lds, e[u], base + u * 64 + lane < nvec, lane);
    }
    // scalar head (lanes 0..2) and tail (lanes 8..10) of a base that is not 16-byte aligned / a length that is no multiple of 4
    if (blockIdx.x == 0 && tid < 64) {
        int idx = -1;
        if (lane < head) idx = lane;
        else if (lane >= 8 && lane - 8 < tail) idx = head + 4 * nvec + (lane - 8);
        const uint32_t b = idx >= 0 ? __float_as_uint(v[idx]) : 0u;
        const bool ok = idx >= 0 && !bits_nan(b);
        if (PASS == 0 && idx >= 0 && !ok) ++nan;
#pragma unroll
        for (int s = 0; s < MAX_SLOTS; ++s) {
            if (!(S.lead_mask >> s & 1)) continue;
            uint32_t d;
            const bool m = slot_digit<PASS>(S, s, b, d) && ok;
            wave_hist_add(lds + s * NB, d, m, lane, 1);
        }
    }
    if (PASS == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nan += (uint32_t)__shfl_xor((int)nan, o);
        if (lane == 0 && nan) atomicAdd(ws + UCLSTM_SELECT_WS_NAN, (u64)nan);
        if (blockIdx.x == 0 && tid == 0) atomicAdd(ws + UCLSTM_SELECT_WS_COUNT, (u64)(head + 4 * (int64_t)nvec + tail));
    }
    __syncthreads();
    for (int s = 0; s < n_slots; ++s) {
        if (!(S.lead_mask >> s & 1)) continue;
        for (int i = tid; i < NB; i += NT) {
            const uint32_t c = lds[s * NB + i];
            if (c) atomicAdd(ws + UCLSTM_SELECT_WS_HIST + s * BINS + i, (u64)c);
        }
    }
}

struct Ranks {
    int64_t r[MAX_SLOTS];
};

__device__ void set_leaders(u64* ws, int n_slots, uint32_t abs_mask, u64 flags) {
    for (int s = 0; s < n_slots; ++s) {
        u64 lead = (flags >> s & 1) ? NO_LEADER : (u64)s;
        for (int t = 0; t < s && lead == (u64)s; ++t)
            if (!(flags >> t & 1) && (abs_mask >> t & 1) == (abs_mask >> s & 1) && ws[UCLSTM_SELECT_WS_PREFIX + t] == ws[UCLSTM_SELECT_WS_PREFIX + s])
                lead = (u64)t;
        ws[UCLSTM_SELECT_WS_LEADER + s] = lead;
    }
}

__global__ __launch_bounds__(NT) void select_begin_kernel(u64* ws, Ranks ranks, int n_slots, uint32_t abs_mask) {
    for (int i = threadIdx.x; i < UCLSTM_SELECT_WS_HIST + MAX_SLOTS * BINS; i += NT) ws[i] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 flags = 0;
        for (int s = 0; s < n_slots; ++s) {
            if (ranks.r[s] < 0) flags |= 1ull << s;
            ws[UCLSTM_SELECT_WS_RANK + s] = ranks.r[s] < 0 ? 0 : (u64)ranks.r[s];
        }
        ws[UCLSTM_SELECT_WS_FLAGS] = flags;
        set_leaders(ws, n_slots, abs_mask, flags);
    }
}

// One block.  Slot by slot: 256 partial sums of the leader's counters, their exclusive scan, and the one bin whose run of ranks
// [below, below + count) holds the slot's rank.  All counts and ranks are u64: a dataset may hold more than 2^32 elements.
__global__ __launch_bounds__(NT) void select_narrow_kernel(u64* ws, int n_slots, int pass, uint32_t abs_mask) {
    __shared__ u64 part[NT];
    __shared__ u64 excl[NT];
    __shared__ u64 new_rank[MAX_SLOTS];
    __shared__ uint32_t new_prefix[MAX_SLOTS];
    __shared__ u64 new_flags;
    const int tid = threadIdx.x;
    const int per = pass_bins(pass) / NT, shift = pass_shift(pass);
    const u64 flags = ws[UCLSTM_SELECT_WS_FLAGS];
    if (tid == 0) new_flags = flags;
    __syncthreads();
    for (int s = 0; s < n_slots; ++s) {
        const uint32_t prefix = (uint32_t)ws[UCLSTM_SELECT_WS_PREFIX + s];
        if (flags >> s & 1) {                                      // uniform
            if (tid == 0) new_prefix[s] = prefix, new_rank[s] = 0;
            continue;
        }
        const u64* h = ws + UCLSTM_SELECT_WS_HIST + ws[UCLSTM_SELECT_WS_LEADER + s] * BINS + tid * per;
        const u64 rank = ws[UCLSTM_SELECT_WS_RANK + s];
        u64 c[8], sum = 0;
        for (int j = 0; j < per; ++j) c[j] = h[j], sum += c[j];
        part[tid] = sum;
        __syncthreads();
        if (tid == 0) {
            u64 run = 0;
            for (int i = 0; i < NT; ++i) excl[i] = run, run += part[i];
            new_prefix[s] = prefix, new_rank[s] = 0;
            if (rank >= run) new_flags |= 1ull << s;               // the rank is not below the number of elements counted
        }
        __syncthreads();
        u64 below = excl[tid];
        for (int j = 0; j < per; ++j) {
            if (rank >= below && rank - below < c[j]) {
                new_prefix[s] = prefix | (uint32_t)(tid * per + j) << shift;
                new_rank[s] = rank - below;
            }
            below += c[j];
        }
        __syncthreads();
    }
    for (int i = tid; i < n_slots * BINS; i += NT) ws[UCLSTM_SELECT_WS_HIST + i] = 0;
    __syncthreads();
    if (tid == 0) {
        for (int s = 0; s < n_slots; ++s) {
            ws[UCLSTM_SELECT_WS_PREFIX + s] = new_prefix[s];
            ws[UCLSTM_SELECT_WS_RANK + s] = new_rank[s];
        }
        ws[UCLSTM_SELECT_WS_FLAGS] = new_flags;
        set_leaders(ws, n_slots, abs_mask, new_flags);
    }
}

__global__ void select_finish_kernel(const u64* ws, int n_slots, float* out_values, u64* out_info) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const u64 flags = ws[UCLSTM_SELECT_WS_FLAGS];
    for (int s = 0; s < n_slots; ++s)
        out_values[s] = __uint_as_float((flags >> s & 1) ? 0x7fc00000u : key_bits((uint32_t)ws[UCLSTM_SELECT_WS_PREFIX + s]));
    out_info[0] = ws[UCLSTM_SELECT_WS_NAN];
    out_info[1] = ws[UCLSTM_SELECT_WS_COUNT];
    out_info[2] = flags;
    out_info[3] = 0;
}

// min / max as keys, NaN count, non-zero count (NaNs included, as np.count_nonzero), element count: one integer atomic each per block
__global__ __launch_bounds__(NT) void extremes_kernel(const float* __restrict__ v, int head, int nvec, int tail, u64* __restrict__ out) {
    __shared__ uint32_t s_min[NT / 64], s_max[NT / 64], s_nan[NT / 64], s_nz[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    uint32_t kmin = 0xffffffffu, kmax = 0u, nan = 0, nz = 0;
    auto take = [&](uint32_t b) {
        if (bits_nan(b)) {
            ++nan, ++nz;
            return;
        }
        const uint32_t k = key_signed(b);
        kmin = min(kmin, k), kmax = max(kmax, k);
        nz += (b & 0x7fffffffu) != 0;
    };
    const uint4* __restrict__ q = reinterpret_cast<const uint4*>(v + head);
    const int stride = gridDim.x * NT;
    for (int i = blockIdx.x * NT + tid; i < nvec; i += 2 * stride) {           // two loads in flight
        const uint4 e = q[i];
        const uint4 f = i + stride < nvec ? q[i + stride] : e;                 // past the end: e again, which changes no extreme ...
        take(e.x), take(e.y), take(e.z), take(e.w);
        if (i + stride < nvec) take(f.x), take(f.y), take(f.z), take(f.w);     // ... and is not counted
    }
    if (blockIdx.x == 0) {
        if (tid < head) take(__float_as_uint(v[tid]));
        else if (tid >= 8 && tid - 8 < tail) take(__float_as_uint(v[head + 4 * nvec + (tid - 8)]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o));
        kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o));
        nan += (uint32_t)__shfl_xor((int)nan, o);
        nz += (uint32_t)__shfl_xor((int)nz, o);
    }
    if (lane == 0) s_min[tid >> 6] = kmin, s_max[tid >> 6] = kmax, s_nan[tid >> 6] = nan, s_nz[tid >> 6] = nz;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NT / 64; ++w) kmin = min(kmin, s_min[w]), kmax = max(kmax, s_max[w]), nan += s_nan[w], nz += s_nz[w];
        if (kmin <= kmax) {                                        // at least one element that is no NaN
            atomicMin(out + UCLSTM_EXTREMES_MIN_KEY, (u64)kmin);
            atomicMax(out + UCLSTM_EXTREMES_MAX_KEY, (u64)kmax);
        }
        if (nan) atomicAdd(out + UCLSTM_EXTREMES_NAN, (u64)nan);
        if (nz) atomicAdd(out + UCLSTM_EXTREMES_NONZERO, (u64)nz);
        if (blockIdx.x == 0) atomicAdd(out + UCLSTM_EXTREMES_COUNT, (u64)(head + 4 * (int64_t)nvec + tail));
    }
}

__global__ void extremes_begin_kernel(u64* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = 0; i < UCLSTM_EXTREMES_WORDS; ++i) out[i] = 0;
    out[UCLSTM_EXTREMES_MIN_KEY] = 0xffffffffull;
}

// v[0..n) = `head` scalars up to the first 16-byte boundary, `nvec` quads, `tail` scalars
struct Split {
    int head, nvec, tail, blocks;
};
// Compute units of the current device (256 when it cannot be asked).  Grids are whole multiples of what is resident at once:
// a grid-stride kernel with 1.3 rounds of blocks runs its last third at a third of the machine.
int compute_units() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        cus = 256;
    }
    return cus;
}
Split split_for(const float* v, int64_t n, int blocks_per_cu) {
    Split p;
    const int64_t to_boundary = (int64_t)((16 - (uintptr_t)v % 16) % 16 / 4);
    p.head = (int)(n < to_boundary ? n : to_boundary);
    p.nvec = (int)((n - p.head) / 4);
    p.tail = (int)(n - p.head - 4 * (int64_t)p.nvec);
    const int64_t want = ceil_div64(n, BLOCK_ELEMS);
    const int64_t resident = (int64_t)compute_units() * blocks_per_cu;
    p.blocks = (int)(want < 1 ? 1 : want > resident ? resident : want);
    return p;
}
bool data_ok(const float* v, int64_t n) { return v && (uintptr_t)v % 4 == 0 && n >= 0 && n < ((int64_t)1 << 31); }
bool state_ok(const uclstm_select_state* st) {
    return st && st->magic == STATE_MAGIC && st->workspace && st->n_slots >= 1 && st->n_slots <= MAX_SLOTS;
}

}  // namespace

extern "C" int64_t uclstm_select_workspace_bytes(void) { return (int64_t)UCLSTM_SELECT_WS_WORDS * 8; }

extern "C" int32_t uclstm_select_begin(uclstm_select_state* st, void* workspace, const int64_t* ranks, const int32_t* kinds,
                                       int32_t n_slots, void* stream) {
    if (!st) return UCLSTM_E_BADARG;
    st->magic = 0;
    if (!workspace || (uintptr_t)workspace % 8 || !ranks || !kinds || n_slots < 1 || n_slots > MAX_SLOTS) return UCLSTM_E_BADARG;
    Ranks r = {};
    uint32_t abs_mask = 0;
    for (int s = 0; s < n_slots; ++s) {
        if (kinds[s] != UCLSTM_SELECT_SIGNED && kinds[s] != UCLSTM_SELECT_ABS) return UCLSTM_E_BADARG;
        if (kinds[s] == UCLSTM_SELECT_ABS) abs_mask |= 1u << s;
        r.r[s] = ranks[s];
    }
    UCLSTM_LAUNCH(select_begin_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (u64*)workspace, r, (int)n_slots, abs_mask);
    st->workspace = workspace, st->n_slots = n_slots, st->abs_mask = abs_mask, st->phase = 0, st->magic = STATE_MAGIC;
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_select_accumulate(uclstm_select_state* st, int32_t pass, const float* v, int64_t n, void* stream) {
    if (!state_ok(st) || pass < 0 || pass > 2 || pass != st->phase || !data_ok(v, n)) return UCLSTM_E_BADARG;
    if (n == 0) return UCLSTM_OK;
    const size_t lds = (size_t)st->n_slots * pass_bins(pass) * sizeof(uint32_t);
    const int per_cu = (int)(LDS_PER_CU / lds);
    const Split p = split_for(v, n, per_cu > 8 ? 8 : per_cu);                  // 8 blocks of 4 waves fill a compute unit
    u64* ws = (u64*)st->workspace;
    hipStream_t s = (hipStream_t)stream;
    if (pass == 0) UCLSTM_LAUNCH(select_hist_kernel<0>, dim3(p.blocks), dim3(NT), lds, s, v, p.head, p.nvec, p.tail, ws, (int)st->n_slots, st->abs_mask);
    else if (pass == 1) UCLSTM_LAUNCH(select_hist_kernel<1>, dim3(p.blocks), dim3(NT), lds, s, v, p.head, p.nvec, p.tail, ws, (int)st->n_slots, st->abs_mask);
    else UCLSTM_LAUNCH(select_hist_kernel<2>, dim3(p.blocks), dim3(NT), lds, s, v, p.head, p.nvec, p.tail, ws, (int)st->n_slots, st->abs_mask);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_select_narrow(uclstm_select_state* st, int32_t pass, void* stream) {
    if (!state_ok(st) || pass < 0 || pass > 2 || pass != st->phase) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(select_narrow_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (u64*)st->workspace, (int)st->n_slots, (int)pass, st->abs_mask);
    st->phase = pass + 1;
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_select_finish(uclstm_select_state* st, float* out_values, uint64_t* out_info, void* stream) {
    if (!state_ok(st) || st->phase != 3 || !out_values || !out_info || (uintptr_t)out_values % 4 || (uintptr_t)out_info % 8) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(select_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const u64*)st->workspace, (int)st->n_slots, out_values, (u64*)out_info);
    st->magic = 0;
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_dataset_extremes_begin(uint64_t* out, void* stream) {
    if (!out || (uintptr_t)out % 8) return UCLSTM_E_BADARG;
    UCLSTM_LAUNCH(extremes_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (u64*)out);
    return UCLSTM_OK;
}

extern "C" int32_t uclstm_dataset_extremes(const float* v, int64_t n, uint64_t* out, void* stream) {
    if (!out || (uintptr_t)out % 8 || !data_ok(v, n)) return UCLSTM_E_BADARG;
    if (n == 0) return UCLSTM_OK;
    const Split p = split_for(v, n, 8);
    UCLSTM_LAUNCH(extremes_kernel, dim3(p.blocks), dim3(NT), 0, (hipStream_t)stream, v, p.head, p.nvec, p.tail, (u64*)out);
    return UCLSTM_OK;
}

#endif  // UCLSTM_ACT_F16
