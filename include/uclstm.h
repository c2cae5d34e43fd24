/*
 * uclstm.h -- C ABI of libuclstm.so, the MI355X (gfx950) UNet-ConvLSTM hot path.
 *
 * The reference (dordanino12/unet-convlstm) has no FFI layer: its boundary is the
 * Python nn.Module surface of train/unet.py.  This header is what that surface binds
 * to underneath (see INTEGRATION.md for the ctypes stub): every entry point takes plain
 * device pointers, sizes and a hipStream_t (passed as void*), launches asynchronously
 * on that stream, allocates nothing, never synchronises, and returns 0 or a negative
 * UCLSTM_E_* code (the host mirror turns those into Python exceptions).
 *
 * Data layout in HBM:
 *   activations  bf16, NHWC, channel count padded to a multiple of 8 ("Cp"), pad = 0
 *   cell state   f32,  NHWC, Cp channels
 *   weights      repacked from the reference's f32 OIHW into bf16 [N][Ktot] panels,
 *                K ordered (tap, source, channel) with every (tap, source) segment padded
 *                to a multiple of 64 (uclstm_pack_weights)
 *
 * Each function cites the reference lines (relative to the reference checkout) whose
 * eager ATen calls it replaces.
 */
#ifndef UCLSTM_H
#define UCLSTM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UCLSTM_ABI_VERSION 16

#define UCLSTM_OK            0
#define UCLSTM_E_BADARG     -1   /* shape / alignment / null-pointer contract violated      */
#define UCLSTM_E_LAUNCH     -2   /* hipLaunchKernel reported an error (hipGetLastError)      */
#define UCLSTM_E_NODEVICE   -3   /* no gfx950 device visible                                 */

/* activation type of the entry points that read 16-bit activations but have no _f16 twin (the *_ordered reductions) */
#define UCLSTM_ACT_TYPE_BF16 0
#define UCLSTM_ACT_TYPE_F16  1

/* ------------------------------------------------------------------------------------ */
/* Implicit-GEMM convolution family                                                     */
/* ------------------------------------------------------------------------------------ */

/* One input tensor of a (possibly channel-concatenated) convolution:
 * bf16 [n_img][Hs][Ws][C], placed at (offY, offX) inside the output pixel frame
 * (the F.pad of train/unet.py:95-97; 0 when sizes match). */
typedef struct {
    const void* ptr;
    int32_t C;          /* padded channel count, multiple of 8 */
    int32_t Hs, Ws;
    int32_t offY, offX;
} uclstm_src;

/* One destination of the epilogue: columns [n_begin, n_end) of the GEMM go to channels
 * [c_off, c_off + n_end - n_begin) of bf16 [n_img][Hd][Wd][C] at pixel
 * (y*scale + oy, x*scale + ox); pixels falling outside are dropped.
 * The wgrad kernel READS its dY operand through the same table. */
typedef struct {
    void* ptr;
    int32_t n_begin, n_end;     /* multiples of 8 */
    int32_t C, c_off;
    int32_t Hd, Wd;
    int32_t scale, oy, ox;
} uclstm_seg;

#define UCLSTM_EPI_STORE 0   /* bias (+ per-column affine, ReLU) -> bf16 segments (+ BN partial sums) */
#define UCLSTM_EPI_LSTM  1   /* gate nonlinearities + cell update, train/unet.py:29-35                */
#define UCLSTM_EPI_ATOMIC 2  /* split-K: f32 atomic accumulation of the raw tile into acc_out (small-M GEMMs
                              * of the ConvLSTM recurrence, where 128x128 tiles alone cannot fill 256 CUs)    */

typedef struct {
    /* output pixel grid: n_img images of H x W; BatchNorm statistic groups (timesteps)
     * are `groups` equal runs of images (train/unet.py:179, :196 call BN once per t). */
    int32_t n_img, H, W, groups;
    /* tap geometry: source pixel = (y*scale + tap/ktap - pad - offY, x*scale + tap%ktap - pad - offX)
     *   3x3 pad 1 conv: ktap 3, scale 1, pad 1      1x1 conv / plain GEMM: ktap 1, scale 1, pad 0
     *   ConvTranspose2d(k2,s2) input-gradient gather: ktap 2, scale 2, pad 0 */
    int32_t ktap, scale, pad;
    int32_t nsrc;
    uclstm_src src[2];
    /* packed weights bf16 [N][Ktot], Ktot = ktap*ktap*(kseg[0]+kseg[1]), kseg[s] = roundup(src[s].C, 64) */
    const void* wp;
    int32_t N, Ktot;
    const float* bias;           /* [N] f32 or NULL */
    const float* col_scale;      /* [N] optional per-column scale  (eval-mode BatchNorm fold) */
    const float* col_shift;      /* [N] optional per-column shift  */
    int32_t relu;
    int32_t epi;
    /* UCLSTM_EPI_STORE */
    int32_t nseg;
    uclstm_seg seg[4];
    float* stats;                /* optional [groups][tiles_per_group][N][2] partial (sum, sumsq) of the STORED bf16 values */
    /* UCLSTM_EPI_LSTM: N = 64*ceil(Hd/16) gate-interleaved rows */
    int32_t Hd_p;                /* padded hidden channels, multiple of 8 */
    const float* c_prev;         /* f32 [pixels][Hd_p] or NULL (zero state, train/unet.py:23-25) */
    float* c_out;                /* f32 [pixels][Hd_p] */
    void* h_out;                 /* bf16 [pixels][Hd_p] */
    void* gates_out;             /* bf16 [pixels][4][Hd_p] post-activation i,f,g,o or NULL (inference) */
    const float* pre_add;        /* f32 [pixels][N] or NULL: pre-activations added to the GEMM result before the
                                  * nonlinearities, in panel-row order -- the x half W_x * x_t of the gate convolution when
                                  * it has been hoisted out of the recurrence (train/unet.py:55-57 recomputes it inside the
                                  * time loop; it does not depend on h) and this launch carries only W_h * h_{t-1} */
    /* UCLSTM_EPI_ATOMIC: acc_out[pixel*acc_ld + n] += tile (no bias); the caller zeroes / pre-loads acc_out.
     * acc_slab > 0: no atomics -- K range r STORES its tile into acc_out + r*acc_slab (floats); every element of each
     * of the uclstm_igemm_ksplit_used() slabs is written exactly once and the consumer adds the slabs
     * (global f32 atomics run at ~1.3 TB/s on MI355X, plain stores at ~6 TB/s). */
    float* acc_out;
    int32_t acc_ld;
    int32_t ksplit;              /* requested K ranges (>= 1) */
    int64_t acc_slab;
} uclstm_igemm_desc;

/* Rows of `stats` per group for a descriptor with N panel rows: ceil((n_img/groups)*H*W / tile_pixels),
 * tile_pixels = 256 when N <= 64 (64 x 256 block shape) else 128. */
int32_t uclstm_igemm_tiles_per_group(int32_t n_img, int32_t H, int32_t W, int32_t groups, int32_t N);

/* out = conv(src) as one MFMA implicit GEMM.  Replaces, depending on the descriptor:
 *   nn.Conv2d 3x3 of DoubleConv (train/unet.py:70-71) incl. the cat([skip, up]) of :98,
 *   its input gradient (flipped/transposed panel), ConvTranspose2d forward and input
 *   gradient (:90,:94), and with UCLSTM_EPI_LSTM the whole ConvLSTMCell.forward (:21-36:
 *   cat + conv + chunk + sigmoid/tanh + cell update in one kernel).
 *
 * Size limits of ONE launch.  Sources and the panel are read through 32-bit buffer descriptors in which bit 31 of the byte
 * offset means "outside the tensor" (that is how padding costs nothing), so:
 *   refused (UCLSTM_E_BADARG, nothing is launched):
 *     - a source with  n_img*Hs*Ws*C*2 + 2*(max(pad+offY, 0)*Ws + max(pad+offX, 0) + 1)*C  >=  2^31 - 2^22  bytes (the second
 *       term is the descriptor's bias: the base address lies that far before the tensor so that tap offsets stay positive);
 *     - a panel with  N*Ktot*2 >= 2^31 - 2^22  bytes;  n_img*H*W >= 2^31 output pixels;  more than 2^31 - 1 blocks.
 *   re-routed (same result, another kernel; uclstm_igemm_fwd_shape tells which):
 *     - the flat kernel (4) indexes destination pixels with 32 bits: a destination of n_img*Hd*Wd >= 2^31 pixels sends the
 *       descriptor to shape 0 / 1;
 *     - the ring kernel (3) asks n_img*(W/64)*(H+1) < 2^30 and the patch loop (2) n_img*(H+1)*(W+1) < 2^30 of their padded
 *       index spaces, else shape 1 / 0.  Their sources have 64 channels and more, so the byte limit above (2^24 pixels at 64
 *       channels) is always reached first: a descriptor at the byte limit still runs the kernel of its shape, and one image
 *       more is refused, whichever kernel it was.
 *   not limited: destinations (seg[].ptr), stats, c_prev / c_out / h_out / gates_out / pre_add and acc_out are addressed with
 *     64-bit offsets and may exceed 2 GiB and 4 GiB (a 64 -> 160-channel launch at the source limit stores 5 GiB).
 * Callers with larger tensors cut the launch into image ranges (ops.py: LAUNCH_BYTES_LIMIT = 2^31 - 2^23 bytes per tensor and
 * launch, whole BatchNorm groups when `stats` is set).  tests/test_high_offset_cases_host.py pins every figure above,
 * tests/test_gpu_high_offset.py runs every kernel at its limit. */
int32_t uclstm_igemm_fwd(const uclstm_igemm_desc* d, void* stream);
/* Which kernel uclstm_igemm_fwd would run for this descriptor (same validation, nothing is launched): 0 = per-tap loop,
 * 128 x 128 tile; 1 = per-tap loop, 64 rows x 256 pixels (C_out <= 64); 2 = patch loop, 128 rows x 256 pixels (3x3 / pad 1 /
 * stride 1, every source on the output grid with C % 64 == 0, >= 2 channel chunks, 256 | pixels per group, patch <= 448
 * rows); 3 = the 64 -> 64-channel ring kernel; 4 = the flat kernel, persistent 128 rows x 256 pixels with a three-stage ring
 * over all its tiles (UCLSTM_EPI_STORE, one source with C % 64 == 0 or C < 64 and zero offsets, pad 0, Ktot <= 512, 256 | pixels per group,
 * and either ktap 1 / scale 1 / source on the output grid or ktap 2 / scale 2 / source twice the output grid: ConvTranspose2d
 * forward and input gradient, the pre-gathered first layer; its statistics rows are those of shapes 0 / 1 for the same N).  Negative: UCLSTM_E_*.  Tests use it to assert that a parity case really exercised the kernel it
 * is meant for. */
int32_t uclstm_igemm_fwd_shape(const uclstm_igemm_desc* desc);
/* Number of non-empty K ranges uclstm_igemm_fwd will use for (Ktot, kernel width, requested ksplit): the slab count of acc_slab
 * mode.  K ranges are whole (source, 64-channel) chunks of ktap*ktap K-steps: steps per range = ktap^2 * ceil(chunks / ksplit). */
int32_t uclstm_igemm_ksplit_used(int32_t Ktot, int32_t ktap, int32_t ksplit);

/* n (1..4) INDEPENDENT descriptors as ONE launch: the per-timestep gate convolutions of the model's three ConvLSTMs
 * (bottleneck + two skip LSTMs, train/unet.py:185-191 runs them one after the other) each fill the chip for one or two rounds of
 * blocks only; as one grid -- members ordered longest block first -- their drains and fills overlap.  Every member must be a
 * descriptor uclstm_igemm_fwd would run on the patch shape (uclstm_igemm_fwd_shape == 2) with UCLSTM_EPI_LSTM or UCLSTM_EPI_ATOMIC
 * (slab mode), all with the same nsrc; anything else is UCLSTM_E_BADARG and the caller launches the members one by one.
 * Results are bit-identical to n separate uclstm_igemm_fwd launches.  Every member is validated as uclstm_igemm_fwd validates
 * it: the size limits stated there hold per member, and one member beyond them refuses the whole group (likewise for
 * uclstm_igemm_fwd_group_tap below). */
int32_t uclstm_igemm_fwd_group(const uclstm_igemm_desc* descs, int32_t n, void* stream);
/* Validation only: the block count of the launch uclstm_igemm_fwd_group would make (>= 1), or UCLSTM_E_*. */
int32_t uclstm_igemm_fwd_group_blocks(const uclstm_igemm_desc* descs, int32_t n);

/* The same for the 128 x 128 per-tap shape: n (1..4) INDEPENDENT descriptors as ONE launch, for the cell steps the patch shape
 * cannot take (it needs 256 | pixels) -- the small images of a frame-by-frame rollout, whose grids of a few tiles or a few
 * dozen split-K blocks would otherwise each pay a launch, a fill and a drain of their own.  Every member must be a descriptor
 * uclstm_igemm_fwd would run on shape 0 (uclstm_igemm_fwd_shape == 0) with ktap == 3 and UCLSTM_EPI_LSTM or UCLSTM_EPI_ATOMIC
 * in slab mode (acc_slab > 0), all with the same nsrc.  Anything else -- a patch-shape or 64 x 256 member, a 5x5 / 7x7 cell,
 * atomic accumulation, mixed nsrc, n outside 1..4 -- is UCLSTM_E_BADARG and nothing is launched.  Members are ordered longest
 * block first (K-steps per block; ties keep the caller's order) and every member's first block id is a multiple of 8, so a
 * member's tile order is that of a launch of its own.  Results are bit-identical to n separate uclstm_igemm_fwd launches: the
 * blocks run the same kernel body and slab mode stores, it does not add. */
int32_t uclstm_igemm_fwd_group_tap(const uclstm_igemm_desc* descs, int32_t n, void* stream);
/* Validation only: the block count of the launch uclstm_igemm_fwd_group_tap would make -- the sum of the members' own grids,
 * each rounded up to a multiple of 8 -- or UCLSTM_E_*. */
int32_t uclstm_igemm_fwd_group_tap_blocks(const uclstm_igemm_desc* descs, int32_t n);

/* Weight gradient  dWp[n][k] (+)= sum_pixels dY[pixel][n] * A[pixel][k]  (f32 [N][Ktot], same
 * K order as the forward panel).  dY is read through seg[] (nseg >= 1); `splits` pixel ranges
 * (0 = chosen by the library for its tile shape and the 256 CUs) accumulate with f32 atomics, so dWp
 * must be zeroed by the caller.  Replaces the autograd weight-gradient of the convolutions above. */
typedef struct {
    int32_t n_img, H, W;
    int32_t ktap, scale, pad;
    int32_t nsrc;
    uclstm_src src[2];
    int32_t N, Ktot;
    int32_t nseg;
    uclstm_seg seg[4];
    float* dwp;
    int32_t splits;
    int32_t accumulate; /* reserved: no kernel reads it.  Atomic mode (slab == 0) always ADDS to dwp, slab mode always STORES */
    int32_t overlapped; /* != 0: the launch runs beside other GEMMs (side stream): the automatic range count (splits = 0) then
                         * minimises interference (few slabs, grid below the CU count) instead of the kernel's own duration */
    int32_t reserved_;
    int64_t slab;     /* 0: pixel ranges ADD into dwp with f32 atomics (dwp zeroed by the caller).  > 0 (>= N*Ktot): range r
                       * STORES its partial panel to dwp + r*slab (floats), nothing needs zeroing, and uclstm_unpack_wgrad adds
                       * the uclstm_igemm_wgrad_splits() slabs (float atomics ~1.3 TB/s, stores ~6 TB/s on MI355X). */
} uclstm_wgrad_desc;
/* Size limits of ONE launch (tests/test_high_offset_cases_host.py pins them, tests/test_gpu_high_offset.py runs every kernel at
 * its limit):
 *   refused (UCLSTM_E_BADARG): a source or a dY tensor of  n_img*H*W*C >= 2^31 - 2^20  ELEMENTS (just under 4 GiB);
 *     n_img*H*W >= 2^31 - 4096 pixels.
 *   re-routed to generic addressing (0, 64-bit pointers, same result): the buffer-addressed kernels (1, 2, 3) take dY of
 *     n_img*H*W*C*2 < 2^31 - 2^22  bytes and sources of  n_img*H*W*C*2 + (Ws+1)*C*2 < 2^31 - 2^22  bytes (32-bit descriptors,
 *     bit 31 = "outside the tensor"); the ring kernel (4) takes  n_img*H*W*128 < 2^31 - 2^22  and  n_img*(W/64)*(H+1) < 2^30
 *     and otherwise leaves the descriptor to kernels 1 / 0.  Operands between 2 GiB and the element limit therefore run, on
 *     generic addressing.
 *   The valid-pixel walk of the 256 x 256 kernel is used below 2^24 - 4096 pixels; its dY rows are at least 512 bytes, so the
 *     byte limit above (about 2^22 pixels) is always reached first.
 * dwp is addressed with 64-bit offsets. */
int32_t uclstm_igemm_wgrad(const uclstm_wgrad_desc* d, void* stream);
/* Pixel ranges (= slabs in slab mode) the launch above will use for this descriptor; d->dwp may be NULL.  Call it with
 * splits = 0, size dwp as [result][N][Ktot], then launch with splits = result. */
int32_t uclstm_igemm_wgrad_splits(const uclstm_wgrad_desc* d);
/* Which kernel uclstm_igemm_wgrad would run for this descriptor (nothing is launched): 4 = ring-staged kernel of the 64-channel
 * full-resolution layers (slab mode only), 3 = 256 x 256 tile, 8-phase pipeline (C_out >= 256), 2 = 128 x 128 tile,
 * 1 = 64 x 256 / 64 x 192 tile (C_out <= 64), 0 = generic addressing (non-power-of-two images,
 * ConvTranspose, offset sources, kernels wider than 3x3).  Used by bench.py to price each kernel separately. */
int32_t uclstm_igemm_wgrad_shape(const uclstm_wgrad_desc* d);
/* The valid-pixel walk of one tap (host only, nothing is launched): a 256 x 256 tile of a 3x3 / pad 1 launch whose tiles each
 * belong to one tap reduces over the output pixels whose source pixel (y + tap / ktap - pad, x + tap % ktap - pad) lies inside
 * the image, image by image and row by row -- n_img * hv * wv entries instead of n_img * H * W.  Fills pixels[k] with the pixel
 * index (img * H * W + y * W + x) of entry i0 + k for k in [0, n), -1 past the end, through the same inline function the kernels
 * stage with (csrc/wgrad_walk.h), and returns the number of entries of the whole walk (>= 0) or UCLSTM_E_BADARG.  Reads n_img,
 * H, W, ktap and pad of the descriptor only.  UCLSTM_WGRAD_VALID=0 (read once per process) makes those launches walk every pixel. */
int64_t uclstm_igemm_wgrad_walk(const uclstm_wgrad_desc* d, int32_t tap, int64_t i0, int32_t n, int32_t* pixels);

/* ------------------------------------------------------------------------------------ */
/* Weight panels                                                                        */
/* ------------------------------------------------------------------------------------ */
#define UCLSTM_NMODE_IDENTITY 0   /* row n <-> entity n (valid n < n_valid)                               */
#define UCLSTM_NMODE_LSTM     1   /* gate-interleaved: n = hb*64 + gate*16 + j <-> gate*n_valid + hb*16 + j */
#define UCLSTM_NMODE_TAPMAJOR 2   /* n = tapn*n_cp + co (ConvTranspose forward), valid co < n_valid        */
#define UCLSTM_KMODE_IDENTITY 0   /* channel c of source s <-> choff[s] + c (valid c < cvalid[s])          */
#define UCLSTM_KMODE_GATES    1   /* c = gate*k_hdp + hc <-> gate*k_hd + hc (valid hc < k_hd)              */
#define UCLSTM_KMODE_IM2COL   2   /* c = tap*k_hd + ci (pre-gathered first layer), tap < k_hdp             */

typedef struct {
    int32_t N, Ktot;
    int32_t taps, nsrc;
    int32_t kseg[2], cvalid[2], choff[2];
    int32_t n_mode, n_valid, n_cp;
    int32_t k_mode, k_hdp, k_hd;
    int32_t tap_flip;
    /* element offset in the f32 source tensor = n_ent*stride_n + k_ent*stride_k
     *                                         + tap_eff*stride_tap + tapn*stride_ntap */
    int64_t stride_n, stride_k, stride_tap, stride_ntap;
} uclstm_pack_desc;

/* f32 reference layout (OIHW conv weight, train/unet.py:19,:70; [in,out,2,2] convT weight, :90)
 * -> bf16 panel [N][Ktot] (zero padded). */
int32_t uclstm_pack_weights(const uclstm_pack_desc* d, const float* w, void* wp, void* stream);
/* Batched packing: a training step repacks every panel after the optimiser step (~100 launches of 3-15 us: a latency chain the
 * step's first convolutions wait for).  Descriptors, pointers and block ranges are the same every step, so the host fills a
 * job table once (uclstm_pack_job_init, host side: returns the job's kernel family 0..4 and fills gx / nblocks / div; block0 =
 * running sum of nblocks over the jobs of ONE family), copies it to the device, and launches one kernel per family. */
typedef struct {
    uclstm_pack_desc d;
    const float* w;
    void* wp;
    int32_t block0, nblocks, gx, family;
    uint32_t div[15];
    int32_t pad_;
} uclstm_pack_job;
int32_t uclstm_pack_job_init(uclstm_pack_job* job /* HOST memory */, const uclstm_pack_desc* d, const float* w, void* wp, int32_t block0);
int32_t uclstm_pack_weights_batched(const uclstm_pack_job* jobs_dev /* DEVICE memory, jobs of one family ordered by block0 */,
                                    int32_t njobs, int32_t family, int32_t total_blocks, void* stream);

/* f32 panel gradient [N][Ktot] -> f32 gradient in the reference layout:
 * grad = (accumulate ? grad : 0) + dWp  on every valid element.  With more than 64 slabs the slabs are first folded into
 * slab 0 in place: dwp is scratch of the weight-gradient GEMM and is CONSUMED by this call. */
int32_t uclstm_unpack_wgrad(const uclstm_pack_desc* d, const float* dwp, int32_t nslab /* dWp = sum of nslab slabs */,
                            int64_t slab /* floats between slabs */, float* grad, int32_t accumulate, void* stream);
/* Ordered form of uclstm_unpack_wgrad (deterministic mode): the same result contract with NO atomics on any path, a pure function
 * of dwp, grad and the shapes.  uclstm_unpack_wgrad_ordered_groups (a function of the descriptor and nslab alone, 1 .. 1024) says
 * into how many slab groups G the call splits the slabs, per = ceil(nslab / G) consecutive slabs each.
 *   G == 1: the non-atomic paths of uclstm_unpack_wgrad (fold / row-family kernel / one thread per element), which add the slabs
 *           in index order; `scratch` is not touched and may be NULL.
 *   G  > 1: two launches.  Stage 1: group g adds its slabs g*per .. min(nslab, (g+1)*per) - 1 in that order, starting from 0, and
 *           STORES the sum to scratch[g][idx] (scratch: f32 [G][N*Ktot], caller-owned, need not be initialised; every element of
 *           every row is written, zeros for an empty group or a padding element).  Stage 2: one thread per element,
 *           grad[off] = (accumulate ? grad[off] : 0) + scratch[0][idx] + scratch[1][idx] + ... + scratch[G-1][idx], left to right.
 * Nobody zeroes anything.  As uclstm_unpack_wgrad, dwp may be consumed. */
int32_t uclstm_unpack_wgrad_ordered_groups(const uclstm_pack_desc* d, int32_t nslab);
int32_t uclstm_unpack_wgrad_ordered(const uclstm_pack_desc* d, const float* dwp, int32_t nslab, int64_t slab, float* scratch,
                                    float* grad, int32_t accumulate, void* stream);
/* bias [n_valid*(4 if LSTM)] f32 -> panel-row order [N] f32 (zero padded). */
int32_t uclstm_pack_bias(const uclstm_pack_desc* d, const float* b, float* bp, void* stream);

/* ------------------------------------------------------------------------------------ */
/* BatchNorm2d + ReLU (train/unet.py:70-71), per-timestep statistics                    */
/* ------------------------------------------------------------------------------------ */
/* From the conv epilogue's partial sums build, per (group, channel): scale = gamma*rstd,
 * shift = beta - mean*scale, mean, rstd; then update running_mean/var with momentum 0.1 and
 * the unbiased variance, once per group IN ORDER (the reference calls BN once per timestep).
 * momentum < 0 means BatchNorm2d(momentum=None): cumulative average, group g uses the factor
 * 1/(-momentum + g), i.e. pass -(num_batches_tracked + 1).
 * `stats` is CONSUMED (its tile-0 slots are overwritten with mean/variance).  stats == NULL:
 * evaluation mode, scale/shift from the running statistics (groups = 1), nothing is updated. */
int32_t uclstm_bn_finalize(float* stats, int32_t groups, int32_t tiles_per_group, int32_t Cp, int32_t C,
                           int64_t count_per_group, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum, float eps,
                           float* scale, float* shift, float* mean, float* rstd, void* stream);
/* The same split in two, so that the sequential part leaves the critical path: uclstm_bn_stats_fwd is ONE launch that reduces the
 * partial sums and writes scale / shift / mean / rstd (`stats` is consumed as above); uclstm_bn_running_stats applies the in-order
 * momentum steps to the running statistics from what that launch left in `stats` -- nothing in the forward or backward pass waits
 * for it (the host layer runs it on its second stream). */
int32_t uclstm_bn_stats_fwd(float* stats, int32_t groups, int32_t tiles_per_group, int32_t Cp, int32_t C, int64_t count_per_group,
                            const float* gamma, const float* beta, float eps, float* scale, float* shift, float* mean, float* rstd,
                            void* stream);
int32_t uclstm_bn_running_stats(const float* stats, int32_t groups, int32_t tiles_per_group, int32_t Cp, int32_t C,
                                int64_t count_per_group, float* running_mean, float* running_var, float momentum, void* stream);

/* Statistics over all ranks of a data-parallel run (SyncBatchNorm): uclstm_bn_stats_fwd cut in two where the other ranks' sums
 * come in.  Every rank must hold the same count per group.
 *   uclstm_bn_stats_partial:   sums64[g][c] = (sum, sum of squares) in f64 (f64 [groups][Cp][2], 16-byte aligned) of the epilogue's
 *     f32 partials, in the summation order of uclstm_bn_stats_fwd (16 strided tile lanes in f64, then the lane sums left to
 *     right).  `stats` is NOT consumed.  The caller adds the sums64 of all ranks (all-reduce, SUM).
 *   uclstm_bn_stats_from_sums: from the added sums and world_count_per_group = ranks * count_per_group:  m = s1/n,
 *     var = max(0, s2/n - m*m), then scale / shift / mean / rstd exactly as uclstm_bn_stats_fwd (mean and variance rounded to f32
 *     before rstd), pad channels zero, and (mean, variance) left in the tile-0 slots of `stats`, where uclstm_bn_running_stats --
 *     called with world_count_per_group for the unbiased variance -- finds them.
 * With one rank the pair gives the bits of uclstm_bn_stats_fwd. */
int32_t uclstm_bn_stats_partial(const float* stats, int32_t groups, int32_t tiles_per_group, int32_t Cp, double* sums64, void* stream);
int32_t uclstm_bn_stats_from_sums(const double* sums64, int64_t world_count_per_group, float* stats, int32_t groups,
                                  int32_t tiles_per_group, int32_t Cp, int32_t C, const float* gamma, const float* beta, float eps,
                                  float* scale, float* shift, float* mean, float* rstd, void* stream);
/* The same for the backward pass: the f32 (sum g, sum g*xhat) of pass 1 (`sums`, n = groups*Cp*2 values, left untouched: the
 * parameter gradients keep reading them) as f64 in `sums64`, the all-reduce payload; then sums_dz = (float)(sums64 * inv_world),
 * inv_world = 1 / ranks in (0, 1].  The apply kernels divide by the LOCAL count, so with equal counts on every rank they compute
 * S_global / n_global from sums_dz.  With one rank sums_dz has the bits of sums. */
int32_t uclstm_bn_bwd_sums_stage(const float* sums, double* sums64, int64_t n, void* stream);
int32_t uclstm_bn_bwd_sums_finish(const double* sums64, double inv_world, float* sums_dz, int64_t n, void* stream);

/* a = relu(z*scale[g] + shift[g]),  g = pixel / pixels_per_group;  z, a bf16 [pixels][Cp]. */
int32_t uclstm_bn_apply_relu(const void* z, void* a, const float* scale, const float* shift,
                             int64_t pixels, int64_t pixels_per_group, int32_t Cp, void* stream);
/* Backward pass 1: sums[g][c] = (sum g_, sum g_*xhat), g_ = dA * [scale*z+shift > 0].  Deterministic (no atomics): every
 * block writes its partial sums into `partials` ([uclstm_bn_bwd_reduce_rows()][Cp][2] floats, caller-allocated, need not
 * be initialised), a second kernel adds them in a fixed order into `sums` ([groups][Cp][2], overwritten). */
int64_t uclstm_bn_bwd_reduce_rows(int64_t pixels, int64_t pixels_per_group);
int32_t uclstm_bn_bwd_reduce(const void* z, const void* da, const float* scale, const float* shift,
                             const float* mean, const float* rstd, float* partials, float* sums,
                             int64_t pixels, int64_t pixels_per_group, int32_t Cp, void* stream);
/* Backward pass 2: dz = scale*(g_ - s1/n - xhat*s2/n)  (bf16). */
int32_t uclstm_bn_bwd_apply(const void* z, const void* da, const float* scale, const float* shift,
                            const float* mean, const float* rstd, const float* sums, void* dz,
                            int64_t pixels, int64_t pixels_per_group, int32_t Cp, void* stream);

/* MaxPool2d(2) fused into the BatchNorm stage that feeds it (the second stage of inc / down1..3; train/unet.py:81, :166-169: every
 * encoder block output goes to the next block's pooling AND to the decoder's skip connection).  H and W even.
 *   uclstm_bn_apply_relu_pool:  a = bf16(relu(z*scale + shift)) as uclstm_bn_apply_relu, and p = max over each 2x2 window of a.
 *   backward: the gradient of a is dskip (bf16, same shape as a; NULL = none) + scatter(dp) to the window's first maximum in scan
 *   order (ATen's rule, uclstm_maxpool2_bwd), rounded to bf16 as that kernel would have stored it -- formed on the fly inside the
 *   BatchNorm backward reduction / apply (same partials / sums / dz contract as uclstm_bn_bwd_reduce / _apply; `partials` has
 *   uclstm_bn_pool_bwd_rows() rows), with the arg-max recomputed from z. */
int64_t uclstm_bn_pool_bwd_rows(int64_t n_img, int32_t H, int32_t W, int32_t Cp, int32_t groups);
int32_t uclstm_bn_apply_relu_pool(const void* z, void* a, void* p, const float* scale, const float* shift, int64_t n_img, int32_t H,
                                  int32_t W, int32_t Cp, int32_t groups, void* stream);
int32_t uclstm_bn_pool_bwd_reduce(const void* z, const void* dskip, const void* dp, const float* scale, const float* shift,
                                  const float* mean, const float* rstd, float* partials, float* sums, int64_t n_img, int32_t H,
                                  int32_t W, int32_t Cp, int32_t groups, void* stream);
int32_t uclstm_bn_pool_bwd_apply(const void* z, const void* dskip, const void* dp, const float* scale, const float* shift,
                                 const float* mean, const float* rstd, const float* sums, void* dz, int64_t n_img, int32_t H,
                                 int32_t W, int32_t Cp, int32_t groups, void* stream);

/* The model's output head fused into its last BatchNorm stage (up0's second conv -> BatchNorm -> ReLU -> OutConv 1x1 with ONE
 * output channel; train/unet.py:70-71, :101-107, :196-199).  That activation feeds only the output convolution: unfused, a training
 * step makes six passes over the largest tensor of the model for it and its gradient; fused, neither exists in memory.
 *   forward:   y[p] = b + sum_c w[c] * bf16(relu(z[p][c]*scale[g][c] + shift[g][c]))            (y f32 [pixels] = NCHW with C = 1)
 *   backward:  da[p][c] = bf16(dy[p] * w[c]) computed on the fly inside the BatchNorm backward reduction / apply (same partials /
 *              sums / dz contract as uclstm_bn_bwd_reduce / _apply); dw[c] += sum_p dy[p] * a[p][c], db += sum_p dy[p].
 * Cp / 8 must be a power of two <= 64; `partials` has uclstm_bn_bwd_reduce_rows() rows. */
int32_t uclstm_bn_head_fwd(const void* z, const float* scale, const float* shift, const float* w, const float* b, float* y,
                           int64_t pixels, int64_t pixels_per_group, int32_t Cp, int32_t C, void* stream);
int32_t uclstm_bn_head_bwd_reduce(const void* z, const float* dy, const float* scale, const float* shift, const float* mean,
                                  const float* rstd, const float* w, float* partials, float* sums, float* dw, float* db,
                                  int64_t pixels, int64_t pixels_per_group, int32_t Cp, int32_t C, void* stream);
int32_t uclstm_bn_head_bwd_apply(const void* z, const float* dy, const float* scale, const float* shift, const float* mean,
                                 const float* rstd, const float* sums, const float* w, void* dz, int64_t pixels,
                                 int64_t pixels_per_group, int32_t Cp, int32_t C, void* stream);

/* Ordered form of uclstm_bn_head_bwd_reduce (deterministic mode; ONE symbol for both activation types, act_type =
 * UCLSTM_ACT_TYPE_BF16 / UCLSTM_ACT_TYPE_F16): partials / sums exactly as there; the head's C + 1 columns (dw[0..C-1], db) no
 * longer end in one atomic per block but go through `head_partials` (f32 [rows][C + 1], rows = the row count of `partials`,
 * caller-owned, need not be initialised): block r stores row r, then one thread per column adds the rows in index order,
 *   dw[c] = dw[c] + hp[0][c] + hp[1][c] + ... + hp[rows-1][c]   (left to right; db likewise from column C).
 * The += into dw / db stays (they are attached gradient buffers, train/unet.py:101-107); nothing is zeroed by anybody. */
int32_t uclstm_bn_head_bwd_reduce_ordered(const void* z, const float* dy, const float* scale, const float* shift, const float* mean,
                                          const float* rstd, const float* w, float* partials, float* head_partials, float* sums,
                                          float* dw, float* db, int64_t pixels, int64_t pixels_per_group, int32_t Cp, int32_t C,
                                          int32_t act_type, void* stream);

/* Parameter gradients of the BatchNorm (train/unet.py:70) from the sums of pass 1, summed over the groups in order:
 * dbeta[c] = (accumulate ? dbeta[c] : 0) + sum_g sums[g][c][0],  dgamma likewise from sums[g][c][1],  c < C. */
int32_t uclstm_bn_bwd_param_grads(const float* sums, int32_t groups, int32_t Cp, int32_t C, float* dgamma, float* dbeta,
                                  int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------ */
/* MaxPool2d(2) (train/unet.py:81)                                                      */
/* ------------------------------------------------------------------------------------ */
int32_t uclstm_maxpool2_fwd(const void* a, void* p, int32_t n_img, int32_t H, int32_t W, int32_t Cp, void* stream);
/* da must be zero-filled by the caller when H or W is odd. First maximum in window scan order wins (ATen rule).
 * add (may be NULL; H and W even): a second gradient of the same tensor, bf16 [n_img][H][W][Cp] -- da = add + scatter(dp).
 * The UNet feeds every encoder output both to the next Down and to the decoder (train/unet.py:166-169, :188-196), so its
 * gradient is always such a sum. */
int32_t uclstm_maxpool2_bwd(const void* a, const void* dp, const void* add, void* da, int32_t n_img, int32_t H, int32_t W, int32_t Cp,
                            void* stream);

/* Finish of a split-K convolution with the STORE epilogue: out[pixel][c] = act16(relu?((sum of the nslab f32 slabs
 * pre[s*slab + pixel*ld + c] + bias[c]) * col_scale[c] + col_shift[c])), c < C (C % 8 == 0, ld >= C) -- the expression of
 * uclstm_igemm_fwd's own epilogue.  For inference convolutions on few pixels (a 32 x 32 bottleneck is 32 tiles on 256 CUs): the
 * GEMM runs as UCLSTM_EPI_ATOMIC K ranges in slab mode and this kernel applies bias / folded BatchNorm / ReLU
 * (train/unet.py:70-71 in eval mode). */
int32_t uclstm_splitk_finish(const float* pre, int32_t nslab, int64_t slab, int32_t ld, const float* bias, const float* col_scale,
                             const float* col_shift, int32_t relu, void* out, int64_t pixels, int32_t C, void* stream);

/* ------------------------------------------------------------------------------------ */
/* ConvLSTM backward point-wise part (autograd of train/unet.py:29-35)                  */
/* ------------------------------------------------------------------------------------ */
/* dh = dh_a (+ dh_b); dc = dc_io + dh*o*(1-tanh(c)^2); dgates = pre-activation gradients
 * bf16 [pixels][4][Hd_p] (i,f,g,o); dc_io <- dc*f (gradient w.r.t. c_prev). */
int32_t uclstm_lstm_bwd_pointwise(const void* gates, const float* c_prev, const float* c_new,
                                  const void* dh_a, const void* dh_b, int32_t dh_b_is_f32 /* 0 bf16, 1 f32, 2 f32 and cleared after reading */,
                                  int32_t dh_b_nslab /* f32 only: dh_b is the sum of this many slabs */, int64_t dh_b_slab /* floats between slabs */,
                                  float* dc_io, int32_t dc_is_zero, void* dgates, int64_t pixels, int32_t Hd_p, void* stream);
/* Gate nonlinearities + cell update (train/unet.py:29-35) for the split-K form of the cell: `pre` is the f32
 * pre-activation [pixels][N] in the gate-interleaved panel-row order (N = 64*ceil(Hd/16)), bias in the same order. */
int32_t uclstm_lstm_fwd_pointwise(float* pre, int32_t nslab /* pre-activation = sum of nslab slabs (0 allowed with pre_add) */,
                                  int64_t slab /* floats between slabs */,
                                  int32_t clear /* != 0: zero what was read (atomic accumulator reused by the next step) */,
                                  const float* pre_add /* f32 [pixels][N] or NULL: added to the slabs (hoisted W_x * x_t) */,
                                  const float* bias, const float* c_prev, float* c_out, void* h_out,
                                  void* gates_out, int64_t pixels, int32_t Hd_p, void* stream);
/* n (1..4) independent cells in one launch (the model's three ConvLSTMs advance in lockstep in the forward pass,
 * uclstm_igemm_fwd_group); fields as the arguments above. */
typedef struct {
    float* pre;
    const float* pre_add;
    const float* bias;
    const float* c_prev;
    float* c_out;
    void* h_out;
    void* gates_out;
    int64_t slab;
    int64_t pixels;
    int32_t nslab, clear, Hd_p, reserved_;
} uclstm_lstm_fwd_pw_args;
int32_t uclstm_lstm_fwd_pointwise_group(const uclstm_lstm_fwd_pw_args* args, int32_t n, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Layout / boundary kernels                                                            */
/* ------------------------------------------------------------------------------------ */
/* f32 NCHW [..] -> bf16 NHWC with channel padding. Image i of the output reads image
 * (i % inner)*outer_stride + (i / inner)*inner_stride of the input (elements), which lets
 * [B,T,C,H,W] be read time-major (train/unet.py:180 indexes x_seq[:, t]). */
int32_t uclstm_nchw_to_nhwc(const float* x, void* out, int32_t n_img, int32_t C, int32_t Cp, int32_t H, int32_t W,
                            int32_t inner, int64_t inner_stride, int64_t outer_stride, void* stream);
int32_t uclstm_nhwc_to_nchw(const void* a, float* out, int32_t n_img, int32_t C, int32_t Cp, int32_t H, int32_t W, void* stream);
/* Gradient of the above (f32 NCHW -> bf16 NHWC is linear): */
int32_t uclstm_nchw_grad_to_nhwc(const float* g, void* out, int32_t n_img, int32_t C, int32_t Cp, int32_t H, int32_t W, void* stream);
/* First-layer gather: out[img][y][x][tap*C + c] = x[img'][c][y+dy-1][x+dx-1] (zero outside), Kp = padded 9*C. */
int32_t uclstm_im2col3x3_first(const float* x, void* out, int32_t n_img, int32_t C, int32_t Kp, int32_t H, int32_t W,
                               int32_t inner, int64_t inner_stride, int64_t outer_stride, void* stream);
/* f32 [pixels][Cp] <-> NCHW for the cell state at module boundaries. */
int32_t uclstm_nchw_to_nhwc_f32(const float* x, float* out, int32_t n_img, int32_t C, int32_t Cp, int32_t H, int32_t W, void* stream);
int32_t uclstm_nhwc_to_nchw_f32(const float* a, float* out, int32_t n_img, int32_t C, int32_t Cp, int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------------------------ */
/* OutConv 1x1 (train/unet.py:101-107): bf16 NHWC in, f32 NCHW out                      */
/* ------------------------------------------------------------------------------------ */
int32_t uclstm_outconv_fwd(const void* a, const float* w, const float* b, float* y,
                           int64_t n_img, int32_t HW, int32_t Cp, int32_t C, int32_t Co, void* stream);
/* da bf16 [pixels][Cp]; dw [Co][C], db [Co] accumulate with atomics (caller zeroes).  da NULL: no input gradient; dw or db
 * NULL (frozen weight and bias): no parameter-gradient kernel. */
int32_t uclstm_outconv_bwd(const void* a, const float* w, const float* dy, void* da, float* dw, float* db,
                           int64_t n_img, int32_t HW, int32_t Cp, int32_t C, int32_t Co, void* stream);

/* Ordered form (deterministic mode; one symbol, act_type as above).  da as uclstm_outconv_bwd.  Pixel range r (of
 * uclstm_outconv_bwd_ordered_rows, a function of the shape alone, 1 .. 1024) stores its block totals to row r of `partials`
 * (f32 [rows][Co*C + Co]: the dw columns in [co][c] order, then the Co db columns; caller-owned, need not be initialised, every
 * element is written); then one thread per column adds the rows in index order,
 *   out = (accumulate ? out : 0) + p[0][col] + p[1][col] + ... + p[rows-1][col]   (left to right),
 * into dw [Co][C] / db [Co].  dw or db NULL: that output is skipped; both NULL: no parameter-gradient launch, partials unused. */
int64_t uclstm_outconv_bwd_ordered_rows(int64_t n_img, int32_t HW);
int32_t uclstm_outconv_bwd_ordered(const void* a, const float* w, const float* dy, void* da, float* partials, float* dw, float* db,
                                   int32_t accumulate, int64_t n_img, int32_t HW, int32_t Cp, int32_t C, int32_t Co,
                                   int32_t act_type, void* stream);

/* ------------------------------------------------------------------------------------ */
/* SpatialAttention (train/unet.py:113-125): mean & max over channels -> k x k conv (2 -> 1, no bias) -> sigmoid -> scale */
/* ------------------------------------------------------------------------------------ */
/* x, out bf16 [n_img][H][W][Cp] (C valid channels); w f32 [2][k][k] (the reference's [1,2,k,k] conv weight, k odd <= 15).
 * Outputs kept for the backward pass: att f32 [pixels] (the sigmoid map), desc f32 [pixels][2] (mean, max), argmax int32
 * [pixels] (first channel attaining the max: where torch.max routes the gradient). */
int32_t uclstm_attention_fwd(const void* x, const float* w, void* out, float* att, float* desc, int32_t* argmax, int32_t n_img,
                             int32_t H, int32_t W, int32_t Cp, int32_t C, int32_t k, void* stream);
/* dx bf16 = gradient w.r.t. x; dw f32 [2][k][k] = (dw_accumulate ? dw : 0) + weight gradient (deterministic block reductions);
 * scratch: f32 [3 * pixels + 2] work space.  dw NULL (frozen weight): the weight-gradient kernel is not launched. */
int32_t uclstm_attention_bwd(const void* x, const void* dout, const float* w, const float* att, const float* desc,
                             const int32_t* argmax, void* dx, float* dw, int32_t dw_accumulate, float* scratch, int32_t n_img,
                             int32_t H, int32_t W, int32_t Cp, int32_t C, int32_t k, void* stream);

/* column sums of a bf16 [pixels][Cp] tensor into f32 [Cp] (bias gradients); out must be zeroed. */
int32_t uclstm_colsum(const void* a, float* out, int64_t pixels, int32_t Cp, void* stream);
/* Ordered form (deterministic mode; one symbol, act_type as above): pixel range r (of uclstm_colsum_ordered_rows, a function of
 * pixels and Cp alone, 1 .. 1024) stores its column sums to row r of `partials` (f32 [rows][Cp], caller-owned, need not be
 * initialised; a range without pixels stores zeros), then one thread per column adds the rows in index order,
 *   out[c] = (accumulate ? out[c] : 0) + p[0][c] + p[1][c] + ... + p[rows-1][c]   (left to right).  Nobody zeroes anything. */
int64_t uclstm_colsum_ordered_rows(int64_t pixels, int32_t Cp);
int32_t uclstm_colsum_ordered(const void* a, float* partials, float* out, int64_t pixels, int32_t Cp, int32_t accumulate,
                              int32_t act_type, void* stream);
/* The finishing step of the ordered reductions on its own: out[c] = (accumulate ? out[c] : 0) + partials[0][c] + partials[1][c] +
 * ... + partials[rows-1][c] for c < cols, one thread per column, the additions strictly left to right (partials [rows][cols]). */
int32_t uclstm_ordered_sum_f32(const float* partials, int32_t rows, int32_t cols, float* out, int32_t accumulate, void* stream);
int32_t uclstm_ordered_sum_f64(const double* partials, int32_t rows, int32_t cols, double* out, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Loss (main.py:28-72) -- weighted L1 + 0.005 * gradient L1, f32 [n][H][W] planes      */
/* ------------------------------------------------------------------------------------ */
/* sums[0..3] = sum(ad*w*m), sum(w*m), sum(gd*mc), sum(mc)  (m = 1 when mask == NULL); caller zeroes sums. */
int32_t uclstm_loss_fwd(const float* y_pred, const float* y, const float* mask, double* sums,
                        int64_t planes, int32_t H, int32_t W, void* stream);
/* Ordered form (deterministic mode): block r of the same sweep stores its four block totals to partials[r][0..3] (f64 [rows][4],
 * rows = uclstm_loss_fwd_ordered_rows, a function of the shape alone, 1 .. 1024; caller-owned, need not be initialised), then
 * sums[k] = (accumulate ? sums[k] : 0) + p[0][k] + p[1][k] + ... + p[rows-1][k], left to right.  Nobody zeroes anything. */
int64_t uclstm_loss_fwd_ordered_rows(int64_t planes, int32_t H, int32_t W);
int32_t uclstm_loss_fwd_ordered(const float* y_pred, const float* y, const float* mask, double* partials, double* sums,
                                int32_t accumulate, int64_t planes, int32_t H, int32_t W, void* stream);
/* grad = coefs[0] * d(sum ad*w*m)/dy_pred + coefs[1] * d(sum gd*mc)/dy_pred; coefs is a DEVICE f32[2]
 * (1/denominators times the upstream gradient), so the step never syncs with the host. */
int32_t uclstm_loss_bwd(const float* y_pred, const float* y, const float* mask, const float* coefs,
                        float* grad, int64_t planes, int32_t H, int32_t W, void* stream);

/* The same loss with its point term and its weight as parameters (LossSpec).  With d = y_pred - y:
 *   rho(d)  = |d| (L1) / d^2 (L2) / Huber: 0.5 d^2 where |d| <= delta, else delta (|d| - 0.5 delta)
 *   rho'(d) = sign(d), sign(0) = 0 / 2 d / clamp(d, -delta, delta)
 *   w       = 1 + weight_gain * |y|^weight_power, the power by repeated multiplication
 * The gradient term is the one above (L1 on the forward differences of the cropped (H-1) x (W-1) cells, the mask at the cell);
 * with grad_term == 0 it does not exist: no neighbour is read, sums[2] and sums[3] are stored as 0 and coefs[1] is not used.
 * The struct lives in HOST memory and is read at launch; the weight of the gradient term and the epsilon of the denominators
 * stay with the caller (they enter through the denominators and coefs, as above).  f32 planes only: no _f16 twin.
 * UCLSTM_E_BADARG before any launch: NULL spec / inputs / outputs / coefs, point or weight_power out of range, Huber with
 * delta <= 0 or not finite, weight_gain negative or not finite, sizes <= 0, planes*H*W >= 2^31. */
#define UCLSTM_LOSS_POINT_L1 0
#define UCLSTM_LOSS_POINT_L2 1
#define UCLSTM_LOSS_POINT_HUBER 2
typedef struct uclstm_loss_spec {
    int32_t point;         /* UCLSTM_LOSS_POINT_* */
    int32_t weight_power;  /* 1 .. 4 */
    float delta;           /* Huber threshold; ignored by L1 and L2 */
    float weight_gain;     /* >= 0 */
    int32_t grad_term;     /* 0: no gradient term */
    int32_t reserved[3];   /* 0 */
} uclstm_loss_spec;
/* sums[0..3] = sum(rho*w*m), sum(w*m), sum(gd*mc), sum(mc) as uclstm_loss_fwd: f64 atomics, caller zeroes sums. */
int32_t uclstm_loss_spec_fwd(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask, double* sums,
                             int64_t planes, int32_t H, int32_t W, void* stream);
/* Ordered form: partials f64 [uclstm_loss_fwd_ordered_rows][4] and sums as uclstm_loss_fwd_ordered; nobody zeroes anything. */
int32_t uclstm_loss_spec_fwd_ordered(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                     double* partials, double* sums, int32_t accumulate, int64_t planes, int32_t H, int32_t W,
                                     void* stream);
/* grad = coefs[0] * rho'(d) * w * m + coefs[1] * d(sum gd*mc)/dy_pred; coefs is a DEVICE f32[2] as for uclstm_loss_bwd. */
int32_t uclstm_loss_spec_bwd(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                             const float* coefs, float* grad, int64_t planes, int32_t H, int32_t W, void* stream);
/* The three entry points above with a mask that is BROADCAST over channels (main.py:40-43, :64-66 with y [B,T,Cy,H,W] and
 * mask [B,T,1,H,W]): plane p of y_pred / y / grad reads mask plane p / mask_div, so mask holds ceil(planes / mask_div) planes of
 * H x W.  Same partition of the elements over blocks and the same arithmetic per element as the entry points above: with the
 * mask expanded to one plane per plane of y they return the same bits (ordered form and bwd; the atomic form up to the order of
 * its atomics).  16-byte loads need W % 4 == 0 with the gradient term, H*W % 4 == 0 without.  UCLSTM_E_BADARG as above, and for a
 * NULL mask or mask_div < 1. */
int32_t uclstm_loss_spec_fwd_bc(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask, double* sums,
                                int64_t planes, int32_t H, int32_t W, int32_t mask_div, void* stream);
int32_t uclstm_loss_spec_fwd_ordered_bc(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                        double* partials, double* sums, int32_t accumulate, int64_t planes, int32_t H, int32_t W,
                                        int32_t mask_div, void* stream);
int32_t uclstm_loss_spec_bwd_bc(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                const float* coefs, float* grad, int64_t planes, int32_t H, int32_t W, int32_t mask_div, void* stream);
/* The same three with a WEIGHT PER PLANE (loss.WeightedLossSpec: per-frame and per-channel weights).  plane_w is a DEVICE
 * f32[period]; plane p of y_pred / y / grad has the weight q = plane_w[p % period] (for y [B,T,Cy,H,W]: period = T*Cy and
 * plane_w[t*Cy + c] = frame weight t x channel weight c).  Every term of the four sums carries it,
 *   sums = sum(rho*w*m*q), sum(w*m*q), sum(gd*mc*q), sum(mc*q),
 * one more f32 multiplication per term, and since every neighbour of the gradient term lies in the element's own plane
 *   grad = q * (coefs[0] * rho'(d) * w * m + coefs[1] * d(sum gd*mc)/dy_pred).
 * mask_div as for the _bc entry points; 1 = a mask plane per plane, or no mask (mask may be NULL only then).  Same grids and the
 * same partition of the elements as the plain entry points: a table of ones returns their bits (ordered form and bwd).
 * UCLSTM_E_BADARG as above (but for the NULL mask at mask_div == 1), and for a NULL plane_w, period < 1, planes % period != 0 or a
 * NULL mask with mask_div > 1.  f32 planes only: no _f16 twin. */
int32_t uclstm_loss_spec_fwd_pw(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                const float* plane_w, int32_t period, double* sums, int64_t planes, int32_t H, int32_t W,
                                int32_t mask_div, void* stream);
int32_t uclstm_loss_spec_fwd_ordered_pw(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                        const float* plane_w, int32_t period, double* partials, double* sums, int32_t accumulate,
                                        int64_t planes, int32_t H, int32_t W, int32_t mask_div, void* stream);
int32_t uclstm_loss_spec_bwd_pw(const uclstm_loss_spec* spec, const float* y_pred, const float* y, const float* mask,
                                const float* plane_w, int32_t period, const float* coefs, float* grad, int64_t planes, int32_t H,
                                int32_t W, int32_t mask_div, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Optimiser(main.py:106-108): global-norm clip + AdamW on flat f32 buffers            */
/* ------------------------------------------------------------------------------------ */
int32_t uclstm_sumsq(const float* g, int64_t n, double* out /* accumulates, caller zeroes */, void* stream);
/* Ordered form (deterministic mode): partials f64 [uclstm_sumsq_ordered_rows] (1 .. 1024 rows, a function of n alone), one stored
 * block total each; *out = (accumulate ? *out : 0) + p[0] + p[1] + ... + p[rows-1], left to right.  Nobody zeroes anything.
 * The clip coefficient of main.py:106 is derived from this sum, so it reaches every parameter. */
int64_t uclstm_sumsq_ordered_rows(int64_t n);
int32_t uclstm_sumsq_ordered(const float* g, int64_t n, double* partials, double* out, int32_t accumulate, void* stream);
/* p,m,v,g flat f32 [n]; grad is scaled by min(1, max_norm/(sqrt(*sumsq)+1e-6)) read on device (no host sync); sumsq == NULL
 * or max_norm <= 0: no clipping.  Adam's bias corrections 1 - beta^step are computed in double and rounded to f32 once, here and
 * in every entry point below. */
int32_t uclstm_adamw_step(float* p, float* m, float* v, const float* g, int64_t n, const double* sumsq, float max_norm,
                          float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream);

/* uclstm_adamw_step with every hyper-parameter and the step count in DEVICE memory: hyper = f32[8] {lr, beta1, beta2, eps,
 * weight_decay, max_norm (<= 0: no clipping), optimiser steps done so far, reserved}; the count is incremented on the device
 * after the update.  Nothing about the launch depends on host state, so it can be captured in a HIP graph and replayed while a
 * scheduler changes lr between replays (one small host-to-device copy). */
int32_t uclstm_adamw_step_dev(float* p, float* m, float* v, const float* g, int64_t n, const double* sumsq, float* hyper, void* stream);

/* AdamW over parameter groups (per-group lr, betas, eps, weight_decay; ONE global gradient norm) in one sweep over the flat
 * buffers, whatever the number of groups; hyper-parameters and the step count in DEVICE memory as for uclstm_adamw_step_dev,
 * so the launch can be captured.  The flat layout is not sorted by group (it keeps the model's registration order), so
 * groups interleave; two device tables say which element belongs where:
 *   runs  = i64[n_runs][3] {begin, end, group}: half-open element ranges in ascending order, the first beginning at 0, each
 *           beginning where the previous one ends, the last ending at n; 0 <= group < n_groups.  The CALLER checks this on the
 *           host before the launch (the library cannot read a device table); neighbouring tensors of one group are one run.
 *   hyper = f32[8 * (1 + n_groups)], 16-byte aligned: block 0 is global {max_norm (<= 0: no clipping), optimiser steps done
 *           so far, reserved x 6}; block 1 + k belongs to group k {lr, beta1, beta2, eps, weight_decay, reserved x 3}.
 * n_groups <= 1024.  sumsq as for uclstm_adamw_step (over ALL groups; may be NULL without clipping and scale_state).
 * scale_state == NULL: bias corrections from hyper[1] + 1, computed as uclstm_adamw_step_dev does, and hyper[1] is
 * incremented on the device after the sweep; with one run and one group the result equals uclstm_adamw_step_dev bit for bit.
 * scale_state != NULL (DEVICE f32[3], layout below; sumsq required): the semantics of uclstm_adamw_step_scaled -- update
 * on g / scale, clip on the unscaled norm, NOTHING is touched on an overflowed step (*sumsq NaN or infinite), the
 * bias-correction step is scale_state[2] + 1 -- and hyper[1] is left alone: uclstm_loss_scale_update, still a launch of its
 * own, counts the step.  With one run and one group the result equals uclstm_adamw_step_scaled bit for bit. */
int32_t uclstm_adamw_step_groups(float* p, float* m, float* v, const float* g, int64_t n, const double* sumsq,
                                 const int64_t* runs, int32_t n_runs, float* hyper, int32_t n_groups,
                                 const float* scale_state, void* stream);

/* fp16 training (the _f16 twins below): the backward pass runs on loss * scale so that fp16 activation gradients stay out of
 * the subnormal range, and g holds scale x the true gradient.  scale_state = DEVICE f32[3] {scale, growth tracker, successful
 * steps}.  uclstm_adamw_step_scaled is uclstm_adamw_step on g / scale (clip on the unscaled norm when max_norm > 0, Adam's
 * bias correction from the device-side count of successful steps, scale_state[2] + 1, computed as everywhere else) to within
 * f32 rounding of the update, and does NOTHING on an OVERFLOWED step: *sumsq (of the scaled gradients; required) is NaN or
 * infinite.  uclstm_loss_scale_update applies the same test to the same *sumsq: after an overflowed step it multiplies the
 * scale by `backoff` (not below 1) and counts nothing; otherwise it counts a successful step and multiplies the scale by
 * `growth` (not above 2^24) every `interval` good steps in a row.  A step is therefore never skipped and counted, or applied and
 * backed off.  No host synchronisation. */
int32_t uclstm_adamw_step_scaled(float* p, float* m, float* v, const float* g, int64_t n, const double* sumsq, float max_norm,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, const float* scale_state,
                                 void* stream);
int32_t uclstm_loss_scale_update(float* scale_state, const double* sumsq, float growth, float backoff, int32_t interval,
                                 void* stream);

/* Exponential moving average of the weights, one sweep launched behind any of the AdamW entry points above: ema, p flat f32 [n].
 * ema_state = DEVICE f32[8] {decay, warmup, every, steps_seen, updates_done, reserved x 3}: steps_seen counts the applied
 * optimiser steps this average has seen, updates_done the updates of ema made; both exact up to 2^24.
 *   sumsq != NULL and *sumsq NaN or infinite (the test of uclstm_adamw_step_scaled / uclstm_loss_scale_update on the same
 *   value): the optimiser skipped that step, and NOTHING is touched, neither ema nor a count.  sumsq == NULL: never skipped.
 *   Otherwise the step is seen, and ema is updated only if (steps_seen + 1) % every == 0, with the decay of update number
 *   k = updates_done + 1: d = decay when warmup <= 0, else min(decay, (1 + k) / (warmup + k)), computed in double and rounded
 *   to f32 once; ema[i] = fmaf(d, ema[i] - p[i], p[i]).
 * The counts are advanced by a one-thread kernel launched behind the sweep in the same call, so every block of the sweep reads
 * the old ones; the arguments never change, so the call can sit in a captured graph.  No atomics, no reductions.
 * UCLSTM_E_BADARG before any launch for a NULL ema / p / ema_state or n <= 0. */
int32_t uclstm_ema_update(float* ema, const float* p, int64_t n, const double* sumsq /* nullable */, float* ema_state, void* stream);
/* Exchange the contents of two DISJOINT f32 buffers in place (no temporary): a[i] <-> b[i] for i in [0, n).  UCLSTM_E_BADARG and
 * nothing written for a NULL a / b, n < 0, a == b or overlapping ranges; n == 0 is UCLSTM_OK without a launch. */
int32_t uclstm_swap_f32(float* a, float* b, int64_t n, void* stream);

/* Per-tensor statistics of the optimiser's flat buffers, one call behind any of the AdamW entry points above (and behind
 * uclstm_ema_update): p = the parameters after the step, g = the gradients as the step read them, prev (nullable) = the
 * parameters at the previous record, all flat f32 [n] and 16-byte aligned (as is partials).  Two launches, no atomics: the numbers are a function
 * of the inputs alone.
 *   blocks         DEVICE int64 [n_blocks][3]  {tensor, start, count}: the elements one block reduces, count <=
 *                  uclstm_param_stats_chunk(), never across two tensors, ordered by tensor and then by start
 *   tensor_blocks  DEVICE int64 [n_tensors][2] {first_block, n_blocks_of_tensor}
 *   partials       DEVICE f64 [n_blocks][8]    scratch of the caller
 *   ring           DEVICE f64 [history][n_tensors][8], meta DEVICE f64 [history][4]
 *   state          DEVICE int64 [8] {every, steps_seen, records_done, due, slot, reserved x 3}: the caller sets every (>= 1) and
 *                  zeroes the rest; due and slot are scratch between the two launches of one call
 * Every call adds 1 to steps_seen.  It records iff the new steps_seen % every == 0; otherwise every block returns after
 * reading the state: nothing else is read or written, prev included.  A record goes to slot = records_done % history, then
 * records_done += 1.  Row ring[slot][tensor], over the elements of the tensor, everything widened to f64:
 *   [0] sum g^2 over finite g        [1] max |g| over finite g (0: none)   [2] non-finite g       [3] g == 0 (+0 and -0)
 *   [4] sum p^2 over finite p        [5] max |p| over finite p             [6] non-finite p
 *   [7] sum (p - prev)^2 where both are finite; 0 without prev
 * and with prev the same pass then writes prev[i] = p[i]: column 7 is the change since the previous record.  Sums are added
 * within a block by a fixed tree and across a tensor's blocks in block order.
 * Row meta[slot] = {steps_seen, *scale or 1, *sumsq or NaN, skipped}; skipped = 1 iff sumsq != NULL and *sumsq is NaN or
 * infinite, the test of uclstm_adamw_step_scaled / uclstm_adamw_step_groups / uclstm_loss_scale_update on the same value.
 * sumsq, scale: nullable DEVICE scalars, read only.  Slot and counts are read from the device, the arguments never change: the
 * call can sit in a captured graph and advances the ring on every replay.  The counts are int64.
 * UCLSTM_E_BADARG before any launch for a NULL p / g / blocks / tensor_blocks / partials / ring / meta / state, a misaligned
 * p / g / prev / partials, n <= 0, n_blocks <= 0, n_tensors <= 0, history <= 0.  The tables live on the device and are not checked here
 * (the host mirror does); a row that points outside [0, n) or is longer than the chunk reads and writes nothing. */
int64_t uclstm_param_stats_chunk(void);
int32_t uclstm_param_stats(const float* p, const float* g, float* prev /* nullable */, int64_t n, const int64_t* blocks, int64_t n_blocks,
                           const int64_t* tensor_blocks, int32_t n_tensors, double* partials, double* ring, double* meta,
                           int32_t history, const double* sumsq /* nullable */, const float* scale /* nullable */, int64_t* state,
                           void* stream);

/* ------------------------------------------------------------------------------------ */
/* Data path around the step                              */
/* ------------------------------------------------------------------------------------ */
/* NPZSequenceDataset.__getitem__ (train/unet.py:273-304) for n_frames = batch*T frames on device: mask = raw x channel 0
 * > 1.1 (BEFORE scaling, :279), x = x_raw / norm_const (:283), y = 2*(asinh(clip(y_raw)/y_scale) - trans_min)/(trans_max -
 * trans_min) - 1 (:287-299).  x_raw/x: f32 [n_frames][C][HW]; y_raw/y/mask: f32 [n_frames][HW]. */
int32_t uclstm_dataset_transform(const float* x_raw, const float* y_raw, float* x, float* y, float* mask, int64_t n_frames,
                                 int32_t C, int32_t HW, float norm_const, float min_vel, float max_vel, int32_t clip,
                                 float y_scale, float trans_min, float trans_max, void* stream);
/* NPZSequenceDataset.__getitem__ (train/unet.py:273-304) for the sequences idx[0..n_out) of a RAW dataset resident on the device:
 * x_all f32 [n_seq][T][C][HW], y_all f32 [n_seq][T][1][HW]  ->  x [n_out][T][C][HW], y, mask [n_out][T][1][HW] (f32).
 * idx: device int64 [n_out], NULL = identity (then n_out <= n_seq); an index outside [0, n_seq) is clamped into it by the
 * kernel (the caller validates; the clamp only keeps a bad index from becoming a wild read).
 * transform: 0 none, 1 asinh(v / y_scale), 2 signed_log = sign(v) * log1p(|v| / y_scale); otherwise the arithmetic of
 * uclstm_dataset_transform.  16-byte loads / stores when HW % 4 == 0 and all five data pointers are 16-byte aligned, a scalar
 * path otherwise.  f32 only (no _f16 twin).  Requires n_out * T * HW < 2^31, y_scale > 0 for transforms 1 / 2. */
int32_t uclstm_dataset_gather_transform(const float* x_all, const float* y_all, const int64_t* idx, int64_t n_seq, int64_t n_out,
                                        int32_t T, int32_t C, int32_t HW, float* x, float* y, float* mask, int32_t transform,
                                        float norm_const, float min_vel, float max_vel, int32_t clip, float y_scale,
                                        float trans_min, float trans_max, void* stream);
/* uclstm_dataset_gather_transform with a per-sequence index remap (augmentation): output sequence o takes the device table row
 * aug[o] = {code, oy, ox, t0} (int32 x 4).  From source frame t0 + t the window [oy, oy + Hc) x [ox, ox + Wc) is cut (s) and moved:
 * out[i][j] = s[a][b], (a, b) = (j, i) if code & 4 (t) else (i, j); then a = Hc-1-a if code & 2 (v); then b = Wc-1-b if code & 1
 * (h) -- torch: flip(-1) for h, then flip(-2) for v, then transpose(-2, -1) for t.  The output frame is Ho x Wo = Hc x Wc, or
 * Wc x Hc with t; one launch has one output shape, so codes with t require Ho == Wo.
 * x_all f32 [n_seq][T_src][C][Hs][Ws], y_all f32 [n_seq][T_src][1][Hs][Ws] -> x [n_out][T_out][C][Ho][Wo], y, mask
 * [n_out][T_out][1][Ho][Wo].  The mask is raw channel 0 > 1.1 at the SOURCE pixel; the arithmetic is per pixel and that of
 * uclstm_dataset_gather_transform, so the result is bit-identical to that entry point's output moved the same way.  Scalar
 * targets only: a vector target (horizontal velocity components) needs sign changes under mirrors and a swap under transposes;
 * that is uclstm_dataset_gather_vec below.
 * flags: bit 0 = the table may hold codes with t (requires Ho == Wo); bit 1 = every ox in the table is a multiple of 4.
 * The kernel clamps what it reads from the table like idx (the caller validates): code & 7, or & 3 when bit 0 is clear; oy, ox, t0
 * into the range that keeps the window inside the source (ox rounded down to a multiple of 4 on the 16-byte path).
 * 16-byte loads / stores when Ws % 4 == 0, Wo % 4 == 0, bit 1 is set and all five data pointers are 16-byte aligned; a scalar path
 * otherwise.  Every code reads and writes along rows; codes with t turn 32 x 32 tiles through LDS.  f32 only (no _f16 twin).
 * Requires Ho <= Hs, Wo <= Ws, T_out <= T_src, n_out * T_out * Ho * Wo < 2^31, Hs * Ws < 2^31. */
int32_t uclstm_dataset_gather_augment(const float* x_all, const float* y_all, const int64_t* idx, const int32_t* aug,
        int64_t n_seq, int64_t n_out, int32_t T_src, int32_t T_out, int32_t C, int32_t Hs, int32_t Ws, int32_t Ho, int32_t Wo,
        int32_t flags, float* x, float* y, float* mask, int32_t transform, float norm_const, float min_vel, float max_vel, int32_t clip,
        float y_scale, float trans_min, float trans_max, void* stream);
/* dst = (accumulate ? dst : 0) + scale * move(src) with the same mover and codes 0..7: src f32 [n_planes][H][W]; dst
 * [n_planes][H][W], or [n_planes][W][H] for codes with t.  src and dst must not overlap.  Requires n_planes * H * W < 2^31. */
int32_t uclstm_plane_d4(const float* src, float* dst, int64_t n_planes, int32_t H, int32_t W, int32_t code, int32_t accumulate,
                        float scale, void* stream);
/* Vector targets: Cy = 1 .. UCLSTM_VEC_MAX target channels per frame (the reference's u_map, v_map, w_map,
 * preprocessing/build_WVU_maps.py:162), each with its own normalisation constants.  UCLSTM_VEC_MAX equals the head kernels'
 * limit on output channels (HEAD_MAX_OUT). */
#define UCLSTM_VEC_MAX 4
typedef struct {
    float min_vel, max_vel, y_scale, trans_min, trans_max;
} uclstm_target_consts;
/* uclstm_dataset_gather_augment for y_all f32 [n_seq][T_src][Cy][Hs][Ws] -> y [n_out][T_out][Cy][Ho][Wo]; x_all, x and mask
 * ([n_out][T_out][1][Ho][Wo], raw x channel 0 > 1.1 at the source pixel) as there.  A move also acts on the channels: a component
 * along image columns changes sign under h, one along rows under v, and the two change places under t.  chan_map is a HOST table
 * int8 [8][Cy], row = code: output channel c takes the plane of source channel (entry & 7), clamped into [0, Cy), and negates
 * its RAW value when bit 7 of the entry is set; NULL = identity.  Output channel c is then clipped and transformed with
 * consts[c] (HOST [Cy]) by the arithmetic of uclstm_dataset_gather_transform; 1 / norm_const, 1 / y_scale and
 * 1 / (trans_max - trans_min) are derived as there.  Both tables are read at launch and travel as kernel arguments: nothing is
 * allocated, copied or synchronised.  aug == NULL: no remap (code 0, window at the origin, t0 = 0).
 * Bit for bit: without aug, channel c equals uclstm_dataset_gather_transform on channel c with consts[c]; with aug, the batch
 * equals the plain call on the raw data moved with flip / transpose / channel permutation / negation; with Cy = 1 and an
 * identity chan_map it equals uclstm_dataset_gather_augment.  Both entry points launch ONE kernel, so flags, the clamping of idx
 * and of the table, the conditions of the 16-byte path and the tile mover are those of uclstm_dataset_gather_augment; Cy = 1 (from
 * either entry point) has instantiations of its own, in which the loop over further target channels does not exist.  f32 only (no
 * _f16 twin).
 * UCLSTM_E_BADARG before any launch for: Cy outside [1, UCLSTM_VEC_MAX], a NULL x_all / y_all / x / y / mask / consts, y_scale <= 0
 * under transforms 1 / 2, trans_max == trans_min, and the limits of uclstm_dataset_gather_augment with Cy in the products
 * (n_out * T_out * Cy * Ho * Wo < 2^31, Cy * Hs * Ws < 2^31). */
int32_t uclstm_dataset_gather_vec(const float* x_all, const float* y_all, const int64_t* idx, const int32_t* aug /* NULL: no remap */,
        int64_t n_seq, int64_t n_out, int32_t T_src, int32_t T_out, int32_t C, int32_t Cy, int32_t Hs, int32_t Ws, int32_t Ho, int32_t Wo,
        int32_t flags, const int8_t* chan_map /* HOST [8][Cy]: bits 0-2 source channel, bit 7 negate; NULL: identity */,
        float* x, float* y, float* mask, int32_t transform, float norm_const, int32_t clip,
        const uclstm_target_consts* consts /* HOST [Cy] */, void* stream);
/* uclstm_plane_d4 over frames of Cy channels with a channel map and an affine term, the way back of test-time averaging for
 * NORMALISED vector predictions: src f32 [n_frames][Cy][H][W], dst [n_frames][Cy][H][W] ([W][H] for codes with t),
 *   dst[f][c] = (accumulate ? dst[f][c] : 0) + scale * (s * move(src[f][source channel]) + offset[c]),  s = -1 with bit 7, else 1,
 * evaluated in that order in f32.  chan_map HOST int8 [Cy] (one row of the table above, NULL = identity), offset HOST f32 [Cy]
 * (NULL = zeros); both travel as kernel arguments.  The kernel is uclstm_plane_d4's: that entry point is Cy = 1 with the identity
 * map and the offset -0.f, which leaves every value as it is (+0.f, the NULL here, turns a -0.f into +0.f and nothing else).
 * src and dst must not overlap.  UCLSTM_E_BADARG for a NULL src / dst, Cy
 * outside [1, UCLSTM_VEC_MAX], code outside [0, 7], sizes <= 0, n_frames * Cy * H * W >= 2^31. */
int32_t uclstm_plane_d4_vec(const float* src, float* dst, int64_t n_frames, int32_t Cy, int32_t H, int32_t W, int32_t code,
        const int8_t* chan_map /* HOST [Cy], as above */, const float* offset /* HOST [Cy] */, int32_t accumulate, float scale, void* stream);
/* Moving-sprite sequences rendered on the device (digits/build_moving_mnist.py:16-47), one launch per batch.
 * bank: uint8 [n_glyph][gh][gw]; table: int32 [n_out][D][5], rows {glyph, x0, y0, vx, vy}.  Per sequence, sprites d = 0..D-1 in
 * order, frames t = 0..T-1: where the glyph byte g > 0 inside the box at (x, y): frame = g / 255 (a later sprite overwrites) and
 * vmap += vx (the CURRENT vx); then x += vx, y += vy; if x < 0 or x > W - gw: vx = -vx and x is clamped into [0, W - gw]; the same
 * for y with H - gh.  Outputs (f32, every element written, background = 0): x [n_out][T][C][H][W] = frame in every channel,
 * y [n_out][T][1][H][W] = vmap / v_scale (an IEEE division), mask [n_out][T][1][H][W] = frame > 0 as 0 / 1, and, unless NULL,
 * raw [n_out][T][2][H][W] = {frame, vmap} (the reference's `data` layout).  Bit-identical to the host generator.
 * The kernel clamps what it reads from the table (the caller validates): glyph into [0, n_glyph), x0 / y0 into the frame, vx / vy
 * into [-127, 127].  16-byte stores when W % 4 == 0 and every output pointer is 16-byte aligned, a scalar path otherwise.
 * f32 only (no _f16 twin).  UCLSTM_E_BADARG before any launch for: a NULL bank / table / x / y / mask, gh or gw outside [1, 64],
 * gw > W, gh > H, D outside [1, 8], T < 1, C < 1, n_glyph < 1, n_out < 1, v_scale == 0, n_out * T * H * W >= 2^31. */
int32_t uclstm_sprites_render(const uint8_t* bank, int32_t n_glyph, int32_t gh, int32_t gw, const int32_t* table, int64_t n_out,
                              int32_t D, int32_t T, int32_t C, int32_t H, int32_t W, float v_scale, float* x, float* y,
                              float* mask, float* raw, void* stream);
/* Epoch metric block of main.py:114-142 as running sums: sums[0..3] += sum|d|m, sum d^2 m, sum d m, sum m with
 * d = denormalize(y_pred) - denormalize(y) (train/unet.py:316-319, asinh transform); mask may be NULL. */
int32_t uclstm_metric_sums(const float* y_pred, const float* y, const float* mask, double* sums, int64_t n, float y_scale,
                           float trans_min, float trans_max, void* stream);

/* Ordered form (deterministic mode): partials f64 [uclstm_metric_sums_ordered_rows][4] (1 .. 1024 rows, a function of n alone) as
 * for uclstm_loss_fwd_ordered; sums[k] = (accumulate ? sums[k] : 0) + p[0][k] + ... + p[rows-1][k], left to right (main.py:114-142
 * keeps running sums over an epoch: accumulate = 1). */
int64_t uclstm_metric_sums_ordered_rows(int64_t n);
int32_t uclstm_metric_sums_ordered(const float* y_pred, const float* y, const float* mask, double* partials, double* sums,
                                   int32_t accumulate, int64_t n, float y_scale, float trans_min, float trans_max, void* stream);
/* The same four running sums PER TARGET CHANNEL: y_pred / y f32 [n_frames][Cy][HW], mask [n_frames][1][HW] broadcast over the
 * channels (may be NULL), sums f64 [Cy][4].  Channel c is de-normalised with consts[c] (HOST [Cy], a kernel argument; min_vel and
 * max_vel are not used) and by `transform` (0 none, 1 asinh: sinh(yt) * y_scale, 2 signed_log: sign(yt) * expm1(|yt|) * y_scale).
 * One form only, the ordered one: partials f64 [uclstm_metric_sums_vec_rows][Cy][4] hold one stored block total each (a block
 * owns a slice of every frame, all channels), and sums[c][k] = (accumulate ? sums[c][k] : 0) + p[0][c][k] + p[1][c][k] + ...,
 * left to right.  No floating-point atomics: the result is a function of the inputs alone.  UCLSTM_E_BADARG for a NULL y_pred / y /
 * partials / sums / consts, Cy outside [1, UCLSTM_VEC_MAX], transform outside [0, 2], sizes <= 0, n_frames * Cy * HW >= 2^31. */
int64_t uclstm_metric_sums_vec_rows(int64_t n_frames, int32_t Cy, int32_t HW);
int32_t uclstm_metric_sums_vec(const float* y_pred, const float* y, const float* mask, double* partials, double* sums,
                               int32_t accumulate, int64_t n_frames, int32_t Cy, int32_t HW, int32_t transform,
                               const uclstm_target_consts* consts /* HOST [Cy] */, void* stream);

/* Evaluation report of train/get_metrics.py:117-358 and test.py:333-351 in one pass over f32 y_pred / y / mask (mask may be
 * NULL; a pixel counts when mask != 0).  Each tensor is [B][T] frames of P = C*H*W contiguous elements, addressed as
 * base + b * stride_b + t * stride_t (elements, >= 0): the model's stacked output, a transposed view of a [T,B,...] buffer, is
 * read in place.  16-byte loads are used when P % 4 == 0 and every base and stride is a multiple of 4 elements.
 * Prediction and target are de-normalised in f32 (train/unet.py NPZSequenceDataset.denormalize): yt = (v + 1) / 2 *
 * (trans_max - trans_min) + trans_min, then by `transform`; d = pred - target.
 *   table      f64 [uclstm_eval_stats_rows(P, B*T)][UCLSTM_EVAL_ROW], WRITTEN (not accumulated) by this call: frame f = b*T + t
 *              owns rows f*cpf .. (f+1)*cpf - 1 (cpf = rows / (B*T)), one per chunk of the plane; a row is
 *              {n, sum|d|, sum d^2, sum d, sum gt, sum gt^2, sum pred, sum pred^2, min gt, max gt, min pred, max pred, min d,
 *              max d, 0, 0}; a row without a valid pixel holds n = 0, min = +inf, max = -inf.  Rows depend on the inputs only
 *              (no floating-point atomics): summing the rows of a frame in index order is bitwise reproducible.
 *   hist       u64 [3][bins], ACCUMULATED: np.histogram(x, bins, range) counts of gt and pred over [hist_lo, hist_hi] and of d
 *              over [err_lo, err_hi] (outside: dropped; x == upper edge: last bin).
 *   dig_count  u64 [n_edges + 1], ACCUMULATED: counts of np.digitize(gt, edges), edges[i] = dig_lo + i * dig_w, i < n_edges
 *              (index 0: below the first edge, n_edges: at or above the last).
 *   scatter    f32 [n_edges + 1][K][2] (8-byte aligned; NULL when K == 0): per digitize bin a uniform sample of up to K
 *              (gt, pred) pairs over everything added so far -- the pixel with ticket t (its rank in the bin, from dig_count)
 *              goes to slot t while t < K, afterwards to slot j = hash(seed, bin, t) reduced to [0, t] when j < K (reservoir
 *              sampling).  Slots [0, min(dig_count[bin], K)) are filled; which pairs survive depends on the order in which
 *              blocks arrive.  hist, dig_count and scatter must be zeroed by the caller before the first call.
 * Counters that fit 60 KiB of LDS (3 * bins + 3 * (n_edges + 1) words) are kept per block and flushed once; larger
 * configurations count with one global integer atomic per pixel and counter (correct, slow). */
#define UCLSTM_EVAL_ROW         16
#define UCLSTM_EVAL_NONE         0
#define UCLSTM_EVAL_ASINH        1
#define UCLSTM_EVAL_SIGNED_LOG   2
typedef struct {
    const float* y_pred; int64_t pred_stride_b, pred_stride_t;
    const float* y;      int64_t y_stride_b, y_stride_t;
    const float* mask;   int64_t mask_stride_b, mask_stride_t;
    int32_t B, T;
    int64_t P;
    int32_t transform;                 /* UCLSTM_EVAL_* */
    float y_scale, trans_min, trans_max;
    double* table;
    int32_t bins, n_edges;
    double hist_lo, hist_hi, err_lo, err_hi;
    double dig_lo, dig_w;
    uint64_t* hist;
    uint64_t* dig_count;
    float* scatter;
    uint64_t seed;
    int32_t K, reserved_;
} uclstm_eval_desc;
/* UCLSTM_E_BADARG before any launch for: a NULL descriptor / y_pred / y / table / hist / dig_count (or scatter with K > 0),
 * P <= 0, B or T <= 0, bins outside [1, 4096], hi <= lo, dig_w <= 0, n_edges outside [2, 65536], K < 0, an unknown transform,
 * a negative stride, B*T*P >= 2^31 or >= 2^24 rows. */
int32_t uclstm_eval_stats(const uclstm_eval_desc* d, void* stream);
/* Rows of `table` one uclstm_eval_stats call over `frames` frames of P elements writes (a function of P and frames only), or
 * UCLSTM_E_BADARG. */
int64_t uclstm_eval_stats_rows(int64_t P, int64_t frames);

/* The same report for VECTOR targets in one launch per batch: y_pred / y are [B][T] frames of [Cy][HW] (the planes of a frame
 * contiguous, channel stride HW, frames addressed by the batch / time strides in elements as above: the model's transposed
 * output view is read in place), mask is [B][T][1][HW], broadcast over the channels (may be NULL; a pixel counts when
 * mask != 0).  Cy = 1 .. UCLSTM_VEC_MAX.  Everything below travels in the descriptor by value; nothing is allocated, copied or
 * synchronised.
 * Per channel c, de-normalised with consts[c] (min_vel / max_vel unused) and `transform`, with ranges hist_lo/hi[c],
 * err_lo/hi[c] and edges dig_lo[c] + i * dig_w[c]; bins, n_edges, K and seed are common:
 *   table      f64 [rows][Cy][UCLSTM_EVAL_ROW], rows = uclstm_eval_stats_rows(HW, B*T), WRITTEN
 *   hist       u64 [Cy][3][bins], ACCUMULATED
 *   dig_count  u64 [Cy][n_edges + 1], ACCUMULATED
 *   scatter    f32 [Cy][n_edges + 1][K][2], ACCUMULATED (8-byte aligned; NULL when K == 0)
 * with the meaning of every field that of uclstm_eval_stats.  Bit for bit: channel c's rows, histogram counts and digitize counts
 * equal what uclstm_eval_stats writes when pointed at channel c in place (bases + c * HW, the same strides, P = HW, the
 * one-channel mask, consts[c]); the scatter sample obeys the same rule (slots [0, min(dig_count, K)) filled with (gt, pred)
 * pairs of that channel and bin).
 * Vector part, only when w_chan >= 0 and h_chan >= 0 (otherwise vtable / vhist / dir_hist may be NULL and are not touched).  In
 * the image frame, with the de-normalised f32 components a = w_sign * v[w_chan] along +column and b = h_sign * v[h_chan] along
 * +row, target g and prediction p:  speed s = sqrt(a^2 + b^2), ds = s_p - s_g;  endpoint error epe = sqrt((a_p - a_g)^2 +
 * (b_p - b_g)^2);  direction error dth = atan2(a_g * b_p - b_g * a_p, a_g * a_p + b_g * b_p) in degrees, in (-180, 180],
 * positive when the prediction is turned from +column towards +row relative to the target, counted only where s_g >= min_speed
 * and s_p >= min_speed (min_speed is compared as an f32).  These per-pixel values are computed in F32 (sqrtf, atan2f); every
 * sum is accumulated in f64.
 *   vtable     f64 [rows][UCLSTM_EVAL_VROW], WRITTEN: {n, sum|ds|, sum ds^2, sum ds, sum s_g, sum s_p, sum epe, sum epe^2, n_dir,
 *              sum|dth|, sum dth, sum dth^2, max epe, max s_g, max s_p, 0}; a row without a valid pixel holds n = 0 and
 *              max = -inf.  No floating-point atomics, a fixed order: bitwise reproducible like `table`.
 *   vhist      u64 [3][bins], ACCUMULATED: s_g and s_p over [0, speed_hi], epe over [0, epe_hi] (the rule of `hist`)
 *   dir_hist   u64 [dir_bins], ACCUMULATED: dth over [-180, 180] (the rule of `hist`)
 * Counters live in LDS when Cy * (3 * bins + 3 * (n_edges + 1)) + 3 * bins + dir_bins words fit 60 KiB, otherwise every count is a
 * global integer atomic.  f32 only (no _f16 twin). */
#define UCLSTM_EVAL_VROW        16
typedef struct {
    const float* y_pred; int64_t pred_stride_b, pred_stride_t;
    const float* y;      int64_t y_stride_b, y_stride_t;
    const float* mask;   int64_t mask_stride_b, mask_stride_t;
    int32_t B, T, Cy;
    int32_t transform;                 /* UCLSTM_EVAL_* */
    int64_t HW;
    uclstm_target_consts consts[UCLSTM_VEC_MAX];
    double hist_lo[UCLSTM_VEC_MAX], hist_hi[UCLSTM_VEC_MAX], err_lo[UCLSTM_VEC_MAX], err_hi[UCLSTM_VEC_MAX];
    double dig_lo[UCLSTM_VEC_MAX], dig_w[UCLSTM_VEC_MAX];
    int32_t bins, n_edges, K, dir_bins;
    uint64_t seed;
    int32_t w_chan, h_chan;            /* channel index, or -1 for none */
    int32_t w_sign, h_sign;            /* +1 / -1 */
    double speed_hi, epe_hi, min_speed;
    double* table;
    uint64_t* hist;
    uint64_t* dig_count;
    float* scatter;
    double* vtable;
    uint64_t* vhist;
    uint64_t* dir_hist;
} uclstm_eval_vec_desc;
/* UCLSTM_E_BADARG before any launch for: every condition of uclstm_eval_stats (per channel where the field is per channel), Cy
 * outside [1, UCLSTM_VEC_MAX], w_chan or h_chan outside [-1, Cy) or equal to each other when >= 0, a sign other than +1 / -1,
 * speed_hi <= 0, epe_hi <= 0, min_speed < 0 or NaN, dir_bins outside [1, 4096], a NULL vtable / vhist / dir_hist while both
 * channels are given, B*T*Cy*HW >= 2^31. */
int32_t uclstm_eval_stats_vec(const uclstm_eval_vec_desc* d, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Dataset statistics (train/unet.py:222-262, get_data_min_max.py) -- csrc/dataset_stats.hip */
/* ------------------------------------------------------------------------------------ */
/* The percentile branch of the reference dataset's constructor needs order statistics of Y and |Y| and the maximum of X.  Both
 * entry-point families below work on the order-preserving u32 KEY of an f32: -0.0 becomes +0.0 (numpy compares them equal), then
 * all bits are inverted for a negative value and the sign bit is set for a non-negative one.  NaNs are counted and take no part.
 * Integer atomics only: every result is a pure function of the multiset of elements, identical from run to run.
 *
 * Rank select: up to UCLSTM_SELECT_MAX_SLOTS slots (rank, kind) are served together; slot s yields the element at index rank[s]
 * of the ascending order of the non-NaN elements (kind UCLSTM_SELECT_SIGNED) or of their absolute values (UCLSTM_SELECT_ABS).
 * Most significant digit first in three passes of 11 / 11 / 10 key bits.  The array may arrive in pieces, and every piece is read
 * once per pass for all slots:
 *     begin;  for pass in 0, 1, 2: { accumulate(pass, piece) for every piece, any number, any split;  narrow(pass) };  finish
 * Everything is chained on `stream`; the host reads nothing back in between.  The pieces of the three passes must hold the same
 * elements (in any order).
 *
 * uclstm_select_state is HOST memory, owned by the caller and written by these calls only (it records the workspace and which
 * call comes next).  `workspace` is DEVICE memory, uclstm_select_workspace_bytes() bytes, 8-byte aligned, as u64 words:
 *     [UCLSTM_SELECT_WS_COUNT] elements seen in pass 0     [UCLSTM_SELECT_WS_NAN] NaNs among them
 *     [UCLSTM_SELECT_WS_FLAGS] bit s: slot s is out of range
 *     [UCLSTM_SELECT_WS_PREFIX + s] the key digits of slot s decided so far, in place (lower bits zero)
 *     [UCLSTM_SELECT_WS_RANK + s]   the slot's rank among the elements that share those digits
 *     [UCLSTM_SELECT_WS_LEADER + s] the slot whose counters slot s reads in the current pass (slots of one kind with equal
 *                                   decided digits share them; all ones for an out-of-range slot)
 *     [UCLSTM_SELECT_WS_HIST + s*UCLSTM_SELECT_BINS + d] elements counted for digit d (2048 digits in passes 0 and 1, 1024 in pass 2)
 * narrow(pass) turns the counters into the next digit and the remaining rank of every slot and clears them.  Counters and ranks
 * are 64-bit throughout.
 *
 * begin: ranks and kinds are host arrays of n_slots entries.  accumulate: v f32 device, 4-byte aligned, 0 <= n < 2^31 elements per
 * call (n = 0 launches nothing); larger arrays are split by the caller.  A 16-byte aligned base is read with 16-byte loads, any
 * other base through a scalar head and tail.  finish: out_values f32 [n_slots] and out_info u64 [4] are device memory;
 * out_info = { NaN count, element count, out-of-range mask, 0 }.  A slot whose rank is negative or not below the number of
 * non-NaN elements is out of range: its bit is set in out_info[2] and its out_values entry is a quiet NaN; the other slots are
 * unaffected.  finish ends the state; begin starts it again.
 * UCLSTM_E_BADARG before any launch for: a NULL state / workspace / ranks / kinds / v / out_values / out_info, a misaligned
 * workspace, v or output, n_slots outside [1, 8], an unknown kind, n outside [0, 2^31), a state that begin has not set up, and a
 * call out of the order above (accumulate or narrow of another pass than the current one, finish before narrow(2)). */
#define UCLSTM_SELECT_MAX_SLOTS 8
#define UCLSTM_SELECT_BINS 2048
#define UCLSTM_SELECT_SIGNED 0
#define UCLSTM_SELECT_ABS 1
#define UCLSTM_SELECT_WS_COUNT 0
#define UCLSTM_SELECT_WS_NAN 1
#define UCLSTM_SELECT_WS_FLAGS 2
#define UCLSTM_SELECT_WS_PREFIX 8
#define UCLSTM_SELECT_WS_RANK 16
#define UCLSTM_SELECT_WS_LEADER 24
#define UCLSTM_SELECT_WS_HIST 32
#define UCLSTM_SELECT_WS_WORDS (UCLSTM_SELECT_WS_HIST + UCLSTM_SELECT_MAX_SLOTS * UCLSTM_SELECT_BINS)
typedef struct {
    void* workspace;
    int32_t n_slots;
    uint32_t abs_mask;
    int32_t phase;
    uint32_t magic;
} uclstm_select_state;
int64_t uclstm_select_workspace_bytes(void);
int32_t uclstm_select_begin(uclstm_select_state* state, void* workspace, const int64_t* ranks, const int32_t* kinds, int32_t n_slots,
                            void* stream);
int32_t uclstm_select_accumulate(uclstm_select_state* state, int32_t pass, const float* v, int64_t n, void* stream);
int32_t uclstm_select_narrow(uclstm_select_state* state, int32_t pass, void* stream);
int32_t uclstm_select_finish(uclstm_select_state* state, float* out_values, uint64_t* out_info, void* stream);
/* Extremes in one pass, accumulating over calls like the select: out u64 [UCLSTM_EXTREMES_WORDS] device memory, set up by
 * uclstm_dataset_extremes_begin and updated by every uclstm_dataset_extremes(v, n) on the same stream:
 *     [UCLSTM_EXTREMES_MIN_KEY] / [UCLSTM_EXTREMES_MAX_KEY] smallest / largest signed key of the non-NaN elements (0xffffffff / 0
 *                               while there is none: min key > max key means "no such element")
 *     [UCLSTM_EXTREMES_NAN] NaNs   [UCLSTM_EXTREMES_NONZERO] elements != 0 (NaNs included, as np.count_nonzero)
 *     [UCLSTM_EXTREMES_COUNT] elements
 * The value behind a key k: the f32 with bits k ^ 0x80000000 when k >= 2^31, ~k otherwise.  v, n and UCLSTM_E_BADARG as
 * uclstm_select_accumulate (plus a NULL or misaligned out). */
#define UCLSTM_EXTREMES_MIN_KEY 0
#define UCLSTM_EXTREMES_MAX_KEY 1
#define UCLSTM_EXTREMES_NAN 2
#define UCLSTM_EXTREMES_NONZERO 3
#define UCLSTM_EXTREMES_COUNT 4
#define UCLSTM_EXTREMES_WORDS 8
int32_t uclstm_dataset_extremes_begin(uint64_t* out, void* stream);
int32_t uclstm_dataset_extremes(const float* v, int64_t n, uint64_t* out, void* stream);

/* Scheduling aid, no reference counterpart: one wavefront that busy-waits `microseconds` of the constant 100 MHz wall clock on
 * `stream`.  The host layer uses it to find out whether two HIP streams really execute concurrently (streams that the
 * runtime multiplexes onto the same hardware queue serialise; which streams collide changes when e.g. an RCCL
 * communicator has created streams of its own first). */
int32_t uclstm_stream_spin(int32_t microseconds, void* stream);

/* ------------------------------------------------------------------------------------ */
/* ResNet18-encoder model (train/resnet18.py: PretrainedTemporalUNet) -- csrc/resnet.hip */
/* ------------------------------------------------------------------------------------ */
/* HBM-bound NHWC kernels around the GEMMs of the reference's shipped configuration (smp.Unet("resnet18", in_channels=2,
 * decoder_channels=(256,128,64,32,16)), train/resnet18.py:26-33).  Its strided convolutions (3x3 / stride 2 / pad 1 and
 * 1x1 / stride 2) are uclstm_igemm_fwd descriptors with scale = 2; nothing here is a GEMM.  All pointers to 16-bit tensors and
 * to per-channel f32 vectors must be 16-byte aligned. */

/* conv1 gather (7x7, stride 2, pad 3) of the f32 NCHW input: out[img][yo][xo][tap*C + c] = x[img'][c][2*yo+dy-3][2*xo+dx-3]
 * (tap = dy*7 + dx; zero outside the image and for the K padding tap*C + c >= 49*C), out bf16 [n_img][Ho][Wo][Kp] with
 * Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1, Kp >= 49*C a multiple of 8.  Image addressing (inner, inner_stride, outer_stride) as
 * uclstm_im2col3x3_first.  The convolution is then a plain GEMM over K = Kp (ktap 1) that can emit BatchNorm partial sums. */
int32_t uclstm_im2col7x7s2_first(const float* x, void* out, int32_t n_img, int32_t C, int32_t Kp, int32_t H, int32_t W,
                                 int32_t inner, int64_t inner_stride, int64_t outer_stride, void* stream);
/* MaxPool2d(3, stride 2, padding 1): p bf16 [n_img][Ho][Wo][Cp], Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1.  Windows are clipped to the
 * image (the padding never wins); odd H / W allowed. */
int32_t uclstm_maxpool3s2_fwd(const void* a, void* p, int32_t n_img, int32_t H, int32_t W, int32_t Cp, void* stream);
/* Tail of a BasicBlock: a = bf16(relu((z*scale[c] + shift[c]) + (r*rscale[c] + rshift[c]))) in f32 on bf16 [pixels][Cp] tensors,
 * scale / shift / rscale / rshift f32 [Cp].  A NULL (scale, shift) or (rscale, rshift) pair is the identity on that operand:
 * the plain residual (r as it is), the downsample branch's BatchNorm (both pairs), and evaluation mode, where the affines
 * were folded into the convolutions (both NULL).  One of a pair NULL and the other not is UCLSTM_E_BADARG. */
int32_t uclstm_bn_add_relu(const void* z, const float* scale, const float* shift, const void* r, const float* rscale,
                           const float* rshift, void* a, int64_t pixels, int32_t Cp, void* stream);
/* Nearest-neighbour x2 upsampling (smp's decoder block): out bf16 [n_img][2H][2W][Cp], out[2y+i][2x+j] = a[y][x]. */
int32_t uclstm_upsample2_fwd(const void* a, void* out, int32_t n_img, int32_t H, int32_t W, int32_t Cp, void* stream);
/* Its gradient: da[y][x] = bf16(((d[2y][2x] + d[2y][2x+1]) + d[2y+1][2x]) + d[2y+1][2x+1]) in f32, in that order. */
int32_t uclstm_upsample2_bwd(const void* dout, void* da, int32_t n_img, int32_t H, int32_t W, int32_t Cp, void* stream);
/* Segmentation head: conv3x3 pad 1 with bias, a bf16 [n_img][H][W][Cp] (C <= Cp <= 64 valid channels), w f32 [Co][C][3][3],
 * b f32 [Co] or NULL, y f32 NCHW [n_img][Co][H][W], Co <= 4.  f32 accumulation: acc = b, then += a*w over (ky, kx, c) in that
 * order; y is never rounded to 16 bits. */
int32_t uclstm_head3x3_fwd(const void* a, const float* w, const float* b, float* y, int64_t n_img, int32_t H, int32_t W, int32_t Cp,
                           int32_t C, int32_t Co, void* stream);
/* da bf16 [pixels][Cp] (padding channels zero); dw [Co][C][3][3] and db [Co] accumulate (+=) with one f32 atomic per block and
 * column (caller zeroes, or passes attached gradient buffers).  Any of da / dw / db NULL: that output is skipped; dw and db both
 * NULL: no parameter-gradient launch. */
int32_t uclstm_head3x3_bwd(const void* a, const float* w, const float* dy, void* da, float* dw, float* db, int64_t n_img, int32_t H,
                           int32_t W, int32_t Cp, int32_t C, int32_t Co, void* stream);
/* Ordered form (deterministic mode; one symbol, act_type as above).  da as uclstm_head3x3_bwd.  Pixel range r (of
 * uclstm_head3x3_bwd_ordered_rows, a function of the shape alone, 1 .. 1024) stores its block totals to `partials` (f32,
 * rows*(Co*C*9) + rows*Co elements: the block [rows][Co*C*9] of dw columns in [co][c][ky][kx] order, then the block [rows][Co] of
 * db columns; caller-owned, need not be initialised, every element is written); then one thread per column adds the rows in
 * index order, out = (accumulate ? out : 0) + p[0][col] + p[1][col] + ... + p[rows-1][col] (left to right, uclstm_ordered_sum_f32).
 * dw or db NULL: that output is skipped; both NULL: no parameter-gradient launch, partials unused. */
int64_t uclstm_head3x3_bwd_ordered_rows(int64_t n_img, int32_t H, int32_t W);
int32_t uclstm_head3x3_bwd_ordered(const void* a, const float* w, const float* dy, void* da, float* partials, float* dw, float* db,
                                   int32_t accumulate, int64_t n_img, int32_t H, int32_t W, int32_t Cp, int32_t C, int32_t Co,
                                   int32_t act_type, void* stream);

/* Backward of the two point-wise stages of the encoder (csrc/resnet_bwd.hip).  No atomics: both are pure functions of their
 * inputs, so deterministic mode needs no second form.
 *
 * Gradient of uclstm_maxpool3s2_fwd, gather form: every INPUT pixel looks at the (at most four) clipped 3x3 windows that contain
 * it, recomputes each window's arg-max from `a` (first maximum in scan order, strict '>': ATen's rule; post-ReLU inputs are full of
 * exact ties) and adds the dp of the windows it wins, window rows first, then columns:
 *   da[y][x] = bf16((dskip ? dskip[y][x] : 0) + sum dp[yo][xo]),   one f32 sum, rounded once.
 * a, dskip (may be NULL), da: bf16 [n_img][H][W][Cp]; dp: bf16 [n_img][Ho][Wo][Cp].  Every element of da is written. */
int32_t uclstm_maxpool3s2_bwd(const void* a, const void* dp, const void* dskip, void* da, int32_t n_img, int32_t H, int32_t W,
                              int32_t Cp, void* stream);
/* Gradient of uclstm_bn_add_relu with both operands through a BatchNorm of the whole batch (one group, n = pixels):
 *   u = (z*scale + shift) + (r*rscale + rshift) in f32 exactly as the forward kernel forms it,  g = da * [u > 0].
 * Pass 1 writes sums[c] = (sum g, sum g*xhat_z) and, when r has a BatchNorm, rsums[c] = (sum g, sum g*xhat_r), both f32 [Cp][2] in
 * the layout of uclstm_bn_bwd_reduce (uclstm_bn_bwd_param_grads reads them with groups = 1), xhat = (x - mean)*rstd.  Block b
 * stores row b of `partials` (f32 [rows][Cp][3], rows = uclstm_bn_add_relu_bwd_rows, caller-owned, need not be initialised); a second kernel
 * adds the rows in a fixed order.
 * Pass 2: dz = bf16(scale*(g - s1/n - xhat_z*s2/n)), dr likewise with r's constants and rsums.  All-zero sums give the
 * evaluation-statistics form scale*g, for either operand on its own.
 * (rscale, rshift, rmean, rrstd, rsums) all NULL: r is the plain residual, dr = bf16(g).  dz or dr NULL: that output is not
 * written (both NULL is UCLSTM_E_BADARG).  Cp / 8 <= 256. */
int64_t uclstm_bn_add_relu_bwd_rows(int64_t pixels);
int32_t uclstm_bn_add_relu_bwd_reduce(const void* z, const float* scale, const float* shift, const float* mean, const float* rstd,
                                      const void* r, const float* rscale, const float* rshift, const float* rmean,
                                      const float* rrstd, const void* da, float* partials, float* sums, float* rsums,
                                      int64_t pixels, int32_t Cp, void* stream);
int32_t uclstm_bn_add_relu_bwd_apply(const void* z, const float* scale, const float* shift, const float* mean, const float* rstd,
                                     const float* sums, const void* r, const float* rscale, const float* rshift,
                                     const float* rmean, const float* rrstd, const float* rsums, const void* da, void* dz,
                                     void* dr, int64_t pixels, int32_t Cp, void* stream);

/* ------------------------------------------------------------------------------------ */
/* fp16 twins (BASELINE.json configs[3]: "fp16 MFMA")                                    */
/* ------------------------------------------------------------------------------------ */
/* Every entry point above that reads or writes 16-bit activations or weight panels exists a second time with the suffix
 * _f16 and the IDENTICAL signature, where every "bf16" in the comments above reads "IEEE binary16": activations, h, gates,
 * gate gradients and panels are _Float16 and the GEMMs issue v_mfma_f32_16x16x32_f16.  Accumulators, cell state, BatchNorm
 * statistics, weight gradients and everything the optimiser touches are f32 in both families, so the remaining entry
 * points (finalize / parameter-gradient / unpack / loss / optimiser ...) are shared.  fp16 gradients need loss scaling
 * (uclstm_loss_scale_update below).  The same sources are compiled twice (csrc/common.h); this is a storage-type twin, not
 * a second backend. */
#define UCLSTM_F16_TWIN(fn) __typeof__(fn) fn##_f16;
UCLSTM_F16_TWIN(uclstm_igemm_fwd)
UCLSTM_F16_TWIN(uclstm_igemm_fwd_group)
UCLSTM_F16_TWIN(uclstm_igemm_wgrad)
UCLSTM_F16_TWIN(uclstm_pack_weights)
UCLSTM_F16_TWIN(uclstm_pack_weights_batched)
UCLSTM_F16_TWIN(uclstm_bn_apply_relu)
UCLSTM_F16_TWIN(uclstm_bn_bwd_reduce)
UCLSTM_F16_TWIN(uclstm_bn_bwd_apply)
UCLSTM_F16_TWIN(uclstm_bn_apply_relu_pool)
UCLSTM_F16_TWIN(uclstm_bn_pool_bwd_reduce)
UCLSTM_F16_TWIN(uclstm_bn_pool_bwd_apply)
UCLSTM_F16_TWIN(uclstm_bn_head_fwd)
UCLSTM_F16_TWIN(uclstm_bn_head_bwd_reduce)
UCLSTM_F16_TWIN(uclstm_bn_head_bwd_apply)
UCLSTM_F16_TWIN(uclstm_maxpool2_fwd)
UCLSTM_F16_TWIN(uclstm_maxpool2_bwd)
UCLSTM_F16_TWIN(uclstm_lstm_bwd_pointwise)
UCLSTM_F16_TWIN(uclstm_lstm_fwd_pointwise)
UCLSTM_F16_TWIN(uclstm_lstm_fwd_pointwise_group)
UCLSTM_F16_TWIN(uclstm_splitk_finish)
UCLSTM_F16_TWIN(uclstm_nchw_to_nhwc)
UCLSTM_F16_TWIN(uclstm_nhwc_to_nchw)
UCLSTM_F16_TWIN(uclstm_nchw_grad_to_nhwc)
UCLSTM_F16_TWIN(uclstm_im2col3x3_first)
UCLSTM_F16_TWIN(uclstm_outconv_fwd)
UCLSTM_F16_TWIN(uclstm_outconv_bwd)
UCLSTM_F16_TWIN(uclstm_colsum)
UCLSTM_F16_TWIN(uclstm_attention_fwd)
UCLSTM_F16_TWIN(uclstm_attention_bwd)
/* the twins of csrc/resnet.hip, as one list (the host mirror keeps the same list: _lib.RESNET_F16_TWINS) */
#define UCLSTM_RESNET_F16_TWINS(TWIN) \
    TWIN(uclstm_im2col7x7s2_first) TWIN(uclstm_maxpool3s2_fwd) TWIN(uclstm_bn_add_relu) TWIN(uclstm_upsample2_fwd) \
    TWIN(uclstm_upsample2_bwd) TWIN(uclstm_head3x3_fwd) TWIN(uclstm_head3x3_bwd)
UCLSTM_RESNET_F16_TWINS(UCLSTM_F16_TWIN)
/* the twins of csrc/resnet_bwd.hip (the host mirror: _lib.RESNET_BWD_F16_TWINS) */
#define UCLSTM_RESNET_BWD_F16_TWINS(TWIN) \
    TWIN(uclstm_maxpool3s2_bwd) TWIN(uclstm_bn_add_relu_bwd_reduce) TWIN(uclstm_bn_add_relu_bwd_apply)
UCLSTM_RESNET_BWD_F16_TWINS(UCLSTM_F16_TWIN)
/* the twin of the per-tap group launch (the host mirror: _lib.TAP_GROUP_F16_TWINS) */
#define UCLSTM_TAP_GROUP_F16_TWINS(TWIN) TWIN(uclstm_igemm_fwd_group_tap)
UCLSTM_TAP_GROUP_F16_TWINS(UCLSTM_F16_TWIN)

/* Library self-description (used by the loader to check the build). */
int32_t uclstm_abi_version(void);
const char* uclstm_build_arch(void);
/* SHA-256 (hex) of the sources the library was built from: csrc/*, this header and the compiler flags
 * (unet-convlstm_amd/build.py: source_hash).  The loader refuses a library whose hash differs from the tree's. */
const char* uclstm_source_hash(void);
/* hipGetErrorString of the most recent launch that returned UCLSTM_E_LAUNCH. */
const char* uclstm_last_error_string(void);

#ifdef __cplusplus
}
#endif
#endif /* UCLSTM_H */
