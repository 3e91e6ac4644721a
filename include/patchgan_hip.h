/*
 * patchgan_hip.h -- C ABI of libpatchgan_hip.so (gfx950 / MI355X only).
 *
 * The reference (ramanakumars/patchGAN v0.2.2) has no native layer of its own:
 * every entry point below replaces the ATen operator that a line of the
 * reference's Python invokes, cited as file:line into /root/reference.
 *
 * Conventions
 *   - every tensor is fp32, device memory, NHWC ("pixel-major"): element
 *     (n, h, w, c) of a tensor with pixel stride `ld` lives at
 *     base[((n*H + h)*W + w)*ld + c].  `ld >= C` lets a tensor be a channel
 *     slice of a wider buffer, which is how torch.cat (unet.py:127,
 *     trainer.py:65,96,98) is made free.  Base pointers, `ld` and channel
 *     counts must be multiples of 4 floats (16 B) unless stated otherwise.
 *   - 4x4 convolution weights are kept in ONE packed layout for all uses:
 *         P[tap = kh*4 + kw][a][b]          (a*b floats per tap, b fastest)
 *     where a torch weight tensor W[a][b][kh][kw] has (a, b) = (Cout, Cin) for
 *     nn.Conv2d and (Cin, Cout) for nn.ConvTranspose2d.  Channel dim `a` lives
 *     on the SMALL spatial side (conv output / convT input), `b` on the BIG side
 *     (conv input / convT output);  big = stride*small - 1 + k.
 *   - all calls are asynchronous on `stream` (a hipStream_t passed as void*),
 *     never allocate, never synchronise; the caller owns all memory including
 *     the workspace.  Return 0 on success or a negative PG_E* code; nothing is
 *     launched when an error is returned.
 *   - containment: a call writes the C channels of each pixel of its output
 *     tensors and nothing else of the buffer they are slices of (not the other
 *     ld - C channels of a pixel, nothing before the first or after the last
 *     pixel), the documented element count of its flat outputs (dP: 16*Ca*Cb
 *     floats, dbias: Ca floats, stats, coef, S, ...), at most ws_bytes bytes of
 *     the workspace and at most the queried bytes of a hand-over buffer; it
 *     reads its inputs only.  The two exceptions write WHOLE pixels and say so:
 *     pg_pad8_bf16 and pg_din_fill zero their pad channels.
 *   - thread-compatible: no global mutable state (pg_conv_time_next keeps two thread-local event handles).
 */
#ifndef PATCHGAN_HIP_H
#define PATCHGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_OK 0
#define PG_EINVAL (-1)   /* bad shape / null pointer / misaligned pointer or ld */
#define PG_EWORKSPACE (-2) /* workspace too small */
#define PG_ELAUNCH (-3)  /* hipGetLastError() != hipSuccess after a launch */

/* activation codes (unet.py:12-17,42-51; disc.py:20,29,39,46) */
#define PG_ACT_NONE 0
#define PG_ACT_LEAKY 1   /* LeakyReLU(0.2) */
#define PG_ACT_RELU 2
#define PG_ACT_TANH 3
#define PG_ACT_SIGMOID 4

/* algorithm selector for the three conv entry points */
#define PG_ALGO_AUTO 0   /* fastest fp32 kernel for the geometry: PG_ALGO_MFMA, except Winograd on MFMA (fp32; 0.6e-6 .. 4e-6
                            relative error in the max norm, max |error| / max |result|, forward and data gradient, 4e-6 .. 8e-6
                            weight gradient over 8 k summed pixels and growing with their number, instead of 1e-7; per element
                            at most 1.7e-6 of sum |x| |w|, 3 .. 6e-8 rms: tests/test_wino1_gpu.py) for wide stride-1 layers
                            (F(2x2,4x4) / F(3x3,4x4); weight gradient F(4x4,2x2) / F(4x4,3x3)) and channel-heavy stride-2
                            layers (polyphase F(3x3,2x2)) */
#define PG_ALGO_DIRECT 1 /* one-thread-per-output reference-quality kernels (any channel count) */
#define PG_ALGO_MFMA 2   /* LDS-tiled implicit GEMM on v_mfma_f32_32x32x2_f32 (channels % 4 == 0) */
#define PG_ALGO_BF16 3   /* same kernels with operand tiles rounded to bf16 in LDS and v_mfma_f32_32x32x16_bf16 (fp32
                            tensors, fp32 accumulate); layers the fast path does not cover fall back to fp32 */

#define PG_ALGO_MASK 0xF
/* Per-call tuning bits, OR-ed into the `algo` argument of the three conv entry points (and into pg_conv_describe's op as
 * op + 16 * (PG_ALGO_* | PG_TUNE_*)).  They override the size heuristics of PG_ALGO_AUTO (and the process-wide PATCHGAN_*
 * environment defaults that exist for A/B timing); results stay inside the stated per-kernel tolerances either way. */
#define PG_TUNE_WINO2_ALL 0x010   /* polyphase Winograd forward / data gradient on every stride-2 layer the geometry allows */
#define PG_TUNE_WINO2_OFF 0x020   /* ... on none */
#define PG_TUNE_WINO2W_ALL 0x040  /* polyphase Winograd weight gradient on every stride-2 layer the geometry allows */
#define PG_TUNE_WINO2W_OFF 0x080  /* ... on none */
#define PG_TUNE_WINO_OFF 0x100    /* no Winograd path at all: the kernels of PG_ALGO_MFMA */
#define PG_TUNE_WINOW_OFF 0x200   /* stride-1 weight gradient on the implicit GEMM */
#define PG_TUNE_WINO1_F2 0x400    /* stride-1 forward / data gradient: F(2x2,4x4) tiles */
#define PG_TUNE_WINO1_F3 0x800    /* ... F(3x3,4x4) tiles (needs Cin % 64 == 0) */
#define PG_TUNE_WINO_DMA 0x1000   /* stride-1 64-tile Winograd GEMMs staged by LDS-DMA (k_wino_gemm_dma) instead of registers */
#define PG_TUNE_BF16X_OFF 0x2000  /* PG_ALGO_BF16 on bf16 tensors: the register-staged k_*_bf16 kernels instead of the LDS-DMA
                                     kernels of conv_bf16.hip (k_conv_bf16x; input channels % 64 == 0) */
#define PG_TUNE_BF16X_RING 0x4000 /* k_conv_bf16x staging pinned: three-stage LDS ring of 32-wide K chunks (DMA two chunks ahead) */
#define PG_TUNE_BF16X_FLAT 0x8000 /* ... one LDS buffer of 64-wide K chunks */
#define PG_TUNE_S3_OFF 0x40000    /* polyphase Winograd GEMMs of PG_ALGO_AUTO on v_mfma_f32_32x32x2_f32 (k_wino_bgemm) instead of their default
                                     split-bf16 form k_wino_bgemm_s3: every fp32 operand value split into three bf16 pieces (8 + 8 + 8
                                     significand bits, exact) while it is staged, the six products with combined weight >= 2^-16 summed by
                                     v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- fp32-grade results (the dropped terms are <= 2^-25
                                     relative; per-kernel error against float64 as for the fp32 kernel) at 2.7x fewer matrix-pipe cycles.
                                     The bit also selects the fp32-MFMA forms of the other two split-bf16 GEMM families: the Winograd weight
                                     gradients (k_wino_wgrad_gemm instead of k_wino_wgrad_gemm_s3) and the row-fused stride-1 F(3x3,4x4) GEMM
                                     (k_wino_gemm_row instead of k_wino_gemm_row_s3) */

/* bf16 activation storage on the PG_ALGO_BF16 kernels: OR-ed into `algo` like the PG_TUNE_* bits.  The tensor named carries bf16
 * elements (NHWC, `ld` in bf16 elements, 8-byte-aligned base; 16-byte-aligned base and ld % 8 == 0 for the LDS-DMA kernels); weights,
 * biases, weight gradients and split-K slabs stay fp32.
 * pg_conv4x4_big2small: BIG = input, SMALL = output; pg_conv4x4_small2big: SMALL = input, BIG = output; pg_conv4x4_wgrad: both
 * or neither (dbias allowed with Ca % 4 == 0).  Honoured where a bf16 kernel covers the call -- input channels % 4 == 0 and >= 32 (the
 * register-staged kernels), % 64 == 0 (the LDS-DMA kernels of conv_bf16.hip), or a <= 8-channel `big` in 8-channel pixels (ld_big == 8,
 * pad channels zero: pg_pad8_bf16); pg_conv4x4_small2big onto <= 8 channels takes PG_IO_SMALL_BF16 alone and writes fp32.  Any other
 * combination returns PG_EINVAL. */
#define PG_IO_BIG_BF16 0x10000
#define PG_IO_SMALL_BF16 0x20000
#define PG_IO_MASK 0x30000

typedef struct pg_conv_geom {
    int N;        /* batch */
    int Hb, Wb;   /* big spatial extent  (conv input  / convT output) */
    int Hs, Ws;   /* small spatial extent (conv output / convT input)  */
    int Ca;       /* channels on the small side = weight dim a */
    int Cb;       /* channels on the big side   = weight dim b */
    int stride;   /* 1 or 2; kernel 4x4, padding 1 always (unet.py:80-81, disc.py:16-17) */
} pg_conv_geom;

int pg_version(void);

/* Byte extent (pixels * ld * element size of a tensor's view) below which the buffer-load kernels -- every fast fp32 kernel and
 * ALL kernels that take bf16 tensors (PG_IO_*) -- can address a tensor: their gathers use 32-bit byte offsets with an
 * out-of-range sentinel.  fp32 tensors beyond it run on the generic kernels (64-bit addressing); a bf16 tensor beyond it has no
 * kernel (PG_EINVAL), and the size queries below (pg_conv_u_bytes, pg_conv_stats_chunks, pg_conv_v_bytes, pg_conv_mul_ok), which
 * see the geometry only, do not know the views: a caller that plans hand-overs or bf16 storage checks its views against this
 * number first (patchgan_amd.engine does: ConvOp.fits / _bf16_tensors_ok; tiled inference streams its tiles in bounded batches). */
size_t pg_conv_max_tensor_bytes(void);

/* Bytes of workspace that lets op (0 = big2small, 1 = small2big, 2 = wgrad) use its preferred
 * split-K factor / Winograd path for geometry g under ANY algo / PG_TUNE_* combination.  A smaller (or NULL) workspace is
 * legal: the split shrinks, the Winograd paths fall back to the implicit GEMM.  Two exceptions return PG_EWORKSPACE (nothing launched):
 *   - pg_conv4x4_wgrad (and _wgrad_x) with dbias != NULL keeps the bias gradient's partial column sums at the head of the workspace:
 *     below 1024 * Ca floats rounded up to 256 bytes it is refused; without dbias any size, NULL included, is PG_OK;
 *   - bf16 tensors (PG_IO_*) run on bf16 kernels only, and the LDS-DMA kernels read packed bf16 weights from the workspace (unless
 *     pg_conv_extras.u_cache holds them).  Where the register-staged bf16 kernels do not cover the call -- big2small from 8-channel
 *     pixels, views or map sizes only the LDS-DMA kernels take -- a workspace without room for the pack leaves no kernel: pg_conv_kernel
 *     then names a kernel without "bf16" for that size, and the call is refused.  (PG_EINVAL is for a call that has no bf16 kernel at
 *     pg_conv_workspace_bytes() either.)
 * A call writes nothing beyond the first ws_bytes bytes of `ws`, whatever path it takes. */
size_t pg_conv_workspace_bytes(const pg_conv_geom* g, int op);   /* op 3 = pg_conv4x4_bwd_big */

/* Reports which kernel the MFMA path of op would launch for g with a workspace of ws_bytes: tile_id
 * (0 = 128x128, 1 = 128x64, 2 = 128x32, 3 = 64x128, 4 = 64x64 output tile per workgroup; the kernel symbol is
 * k_big2small / k_small2big / k_wgrad <MR,NR,WM,WN> with <2,2,2,2>, <2,1,2,2>, <1,1,4,1>, <1,2,2,2>, <1,1,2,2>), the
 * split-K factor and the number of workgroups.  For op 2, tile_id + 10 / + 20 means the taps-folded-into-N kernel
 * k_wgrad_tapn<..., 1> / <..., 2> (few big-side / small-side channels); for ops 0/1, + 30 means the row-GEMM +
 * col2im / tap-gather path.  + 100 (+ 200: power-of-two pixel decode, wgrad) marks the fast buffer-load variant
 * (k_b2s_fast / k_s2b_fast / k_wgrad_fast) that runs when tensors are 16-byte aligned.  `op` may carry the algorithm as
 * op + 16 * PG_ALGO_*; for PG_ALGO_AUTO (op < 16) wide stride-1 layers report the Winograd kernels instead: + 40 / + 50 =
 * k_wino_gemm<2,1,2,2,2,2> / <1,1,2,2,4,2>, + 90 = its F(3x3,4x4) instance <1,1,2,2,2,3> (ops 0/1; tile / split of the implicit-GEMM plan otherwise unchanged), 60 =
 * k_wino_wgrad_gemm<2,2,2,2> with split = its K slices (op 2; 63: 64x64 tiles <1,1,2,2>; 61 / 62: its polyphase stride-2 form with 128x128 / 64x64 tiles; by default the split-bf16
 * forms k_wino_wgrad_gemm_s3<2,2,2,2,1,2> / <1,1,2,2,2,3>, and k_wino_gemm_row_s3<2> for + 90's row-fused form), 70 / 71 = k_wino_bgemm_s3<2,2,2,2,2> / <1,2,2,2,3>
 * (under PG_TUNE_S3_OFF k_wino_bgemm<2,2,2,2> / <1,2,2,2>, 72 / 73 = k_wino_bgemm_mz<...>) (polyphase Winograd of a stride-2 layer, ops 0/1).  80 + Cb: the image-facing forward kernels k_b2s_tapk / k_b2s_tapkp<Cb> (op 0, <= 5 big-side
 * channels).  Codes >= 1000: 1000 + 100 * ring + 10 * dir + tile = the LDS-DMA bf16 kernels k_conv_bf16x on bf16 tensors, 1020 + tile =
 * k_wgrad_bf16x, 1030 + tile = bf16 row GEMM + col2im, 1040 + tile = k_conv_bf16x on 8-channel pixels, 1050 = the one-channel head's data
 * gradient k_s2b_ca1 / k_s2b_ca1_s1, 1060 + Cb (1070 + Cb: from a bf16 tensor) = the one-pass transposed convolution onto <= 8 channels
 * k_s2b_tapnf<Cb> (Cb > 4: two launches, <4> + <Cb - 4>).  The numbers are encoded from the plan of the one planner that the entry points
 * launch from, made for 16-byte-aligned contiguous tensors.  For profiling only. */
int pg_conv_describe(const pg_conv_geom* g, int op, size_t ws_bytes, int* tile_id, int* split, long* workgroups);

/* The kernel symbol (as rocprofv3 prints it, without the namespace / argument list) of the main GEMM kernel that op would
 * launch -- read from the plan of the same planner call the entry points make (with the views of a 16-byte-aligned contiguous call), so
 * profiles can be attributed without re-deriving the dispatch --
 * its split-K factor, and the FLOPs that kernel executes on the MFMA pipe (the direct-convolution count 2*N*Hs*Ws*16*Ca*Cb
 * for the implicit-GEMM kernels, 2.25-4x fewer for the Winograd kernels, ragged tiles included).  `op` as in
 * pg_conv_describe.  For profiling only. */
int pg_conv_kernel(const pg_conv_geom* g, int op, size_t ws_bytes, char* name, size_t name_len, int* split, double* mfma_flops);

/* The two FLOP counts of that kernel: `executed` as pg_conv_kernel reports it (a Winograd kernel's ragged edge tiles are whole tiles on
 * the MFMA pipe: up to 27 % of the work on 16x16 maps), `useful` = the same algorithm's count on the exact extents (H / m instead of
 * ceil(H / m) tiles).  bench.py's roofline.frac / roofline.frac_useful; the direct-convolution count is 2*N*Hs*Ws*16*Ca*Cb for every
 * kernel.  For profiling only (replaces nothing in the reference: torch.profiler's per-op FLOP column is the closest thing). */
int pg_conv_kernel_flops(const pg_conv_geom* g, int op, size_t ws_bytes, double* executed, double* useful);

/* Arms per-launch timing: the NEXT pg_conv4x4_* call on this thread records the caller-owned hipEvent_t `ev_start`
 * immediately before and `ev_stop` immediately after its main GEMM kernel on the launch stream (the split-K reduce, the
 * bias column sums and the col2im / gather pass are outside the pair), then disarms itself.  Thread-local state; the
 * default (never armed) adds nothing to a launch.  Used by bench.py's roofline leg. */
int pg_conv_time_next(void* ev_start, void* ev_stop);

/* small[n,p,q,a] = act( sum_{kh,kw,b} big[n, s*p-1+kh, s*q-1+kw, b] * P[kh*4+kw][a][b] + bias[a] )
 * Replaces: nn.Conv2d forward (unet.py:19; disc.py:19,27,37,45) with (a,b) = (Cout,Cin), and the
 * data-gradient of nn.ConvTranspose2d (unet.py:53, aten::convolution_backward) with (a,b) = (Cin,Cout).
 * bias may be NULL; act is a PG_ACT_* code applied in the epilogue. */
int pg_conv4x4_big2small(const float* big, int ld_big, const float* P, const float* bias,
                         float* small, int ld_small, const pg_conv_geom* g, int act, int algo,
                         void* ws, size_t ws_bytes, void* stream);

/* big[n,h,w,b] = act( sum_{kh,kw,a : (h+1-kh)%s==0, (w+1-kw)%s==0}
 *                      small[n,(h+1-kh)/s,(w+1-kw)/s,a] * P[kh*4+kw][a][b] + bias[b] )
 * Replaces: nn.ConvTranspose2d forward (unet.py:53) with (a,b) = (Cin,Cout), and the data-gradient of
 * nn.Conv2d (aten::convolution_backward) with (a,b) = (Cout,Cin). */
int pg_conv4x4_small2big(const float* small, int ld_small, const float* P, const float* bias,
                         float* big, int ld_big, const pg_conv_geom* g, int act, int algo,
                         void* ws, size_t ws_bytes, void* stream);

/* dP[kh*4+kw][a][b] = sum_{n,p,q} small[n,p,q,a] * big[n, s*p-1+kh, s*q-1+kw, b]
 * Replaces: the weight-gradient half of aten::convolution_backward for both nn.Conv2d
 * (small = dL/dy, big = x) and nn.ConvTranspose2d (small = x, big = dL/dy).
 * Deterministic (fixed-order split-K slabs, no float atomics).  dbias (may be NULL) receives
 * sum_{n,p,q} small[n,p,q,a] (the Conv2d bias gradient, disc.py:19,45). */
int pg_conv4x4_wgrad(const float* small, int ld_small, const float* big, int ld_big,
                     float* dP, float* dbias, const pg_conv_geom* g, int algo,
                     void* ws, size_t ws_bytes, void* stream);

/* Optional hand-overs between calls on the SAME layer, for the Winograd paths of PG_ALGO_AUTO (all fields may be NULL / 0):
 *   part     out: InstanceNorm partial sums of the output (the conv epilogue emits sum / sum of squares -- unet.py:19-20,53-55,
 *            a Conv2d / ConvTranspose2d feeding an InstanceNorm2d): part[((n * chunks + chunk) * C + c) * 2 + {0, 1}], fp64,
 *            fixed summation order, chunks = pg_conv_stats_chunks(...)
 *   v_keep   big2small: write the polyphase-transformed input here (pg_conv_v_bytes) instead of into the workspace ...
 *   v_pre    wgrad: ... so that the weight gradient of the same layer (same `big` tensor) reads it instead of redoing the transform
 *   u_cache  big2small / small2big: the transformed weights of this (layer, direction) live here (pg_conv_u_bytes) ...
 *   u_valid  ... and, when non-zero, already hold the transform of the CURRENT weights: the weight transform is skipped
 *            (the discriminator's weights serve two forward and two data-gradient passes per step, trainer.py:66,98-99).
 * The size queries mirror the dispatch for 16-byte-aligned tensors and return 0 when the call would not take a path that has
 * such an operand; passing a hand-over to a call that does not take that path returns PG_EINVAL (nothing is launched: not the
 * weight gradient's bias column sums either) -- under PG_ALGO_DIRECT, whose kernels have no such operand, always.  The queries take
 * the workspace size of the CALL: with a smaller workspace a Winograd path falls back and its hand-overs go with it (the query
 * returns 0, the call refuses them). */
typedef struct pg_conv_extras {
    double* part;
    float* v_keep;
    const float* v_pre;
    float* u_cache;
    int u_valid;
    /* small2big as a data gradient: out = conv(...) * f'(t), the activation backward of the layer BELOW folded into the epilogue
     * (trainer.py:89,106: autograd's TanhBackward / LeakyReluBackward between two ConvolutionBackward nodes).  mul_t = that layer's
     * activation OUTPUT [pixels of big][Cb], pixel stride mul_ld, storage type of `big`; mul_act = its PG_ACT_* (the derivative is
     * expressed through the output).  Honoured where pg_conv_mul_ok() != 0; elsewhere PG_EINVAL. */
    const void* mul_t;
    int mul_ld;
    int mul_act;
    /* big2small with v_keep, as ONE PART of a larger batch: the kept transform is V[point][tile][k] with the tiles of the whole batch
     * running inside every point's plane, so a call over samples [n0, n0 + N) of a batch of Nt writes (and its GEMM reads) rows
     * [v_tile0, v_tile0 + tiles(N)) of every plane of the buffer sized for Nt (pg_conv_v_bytes of the Nt geometry):
     *   v_stride  floats between two planes = tiles(Nt) * k (k = 4 * Cb on the polyphase path, Cb on the stride-1 path); 0 = the
     *             dense layout of this call's own N (and then v_tile0 must be 0)
     *   v_tile0   first tile row = n0 * tiles(1)
     * Rows outside the range are not touched.  Per-tile arithmetic does not depend on either field.  Honoured by the polyphase
     * path and by the row-fused F(3x3,4x4) path (the only ones that keep V); PG_EINVAL where the range leaves the plane, the strided
     * buffer is beyond the kernels' 32-bit offsets, or v_keep is NULL.  Whether the parts of a batch compute what the whole-batch call
     * computes, bit for bit, is answered by pg_conv_batch_halves_same(). */
    long long v_stride;
    long long v_tile0;
} pg_conv_extras;
/* 1 if pg_conv4x4_big2small on geometry g (N samples) and on the same geometry with 2 * N samples do the same arithmetic per sample:
 * the same path and kernel symbol, no split over K in either, and a kept V (pg_conv_v_bytes) in both or in neither -- decided by the
 * planner the entry points launch from, for 16-byte-aligned contiguous tensors.  ws_bytes_n / ws_bytes_2n: the workspace sizes the two
 * calls would be made with.  Then two half calls (v_stride / v_tile0 above) fill what the whole call fills.  0 otherwise. */
int pg_conv_batch_halves_same(const pg_conv_geom* g, int algo, size_t ws_bytes_n, size_t ws_bytes_2n);
int pg_conv_mul_ok(const pg_conv_geom* g, int algo, size_t ws_bytes);   /* small2big: the kernel of this call can apply mul_t */
int pg_conv_stats_chunks(const pg_conv_geom* g, int op, int algo, size_t ws_bytes);   /* op 0 big2small, 1 small2big */
size_t pg_conv_u_bytes(const pg_conv_geom* g, int op, int algo, size_t ws_bytes);      /* op 0 big2small, 1 small2big */
size_t pg_conv_v_bytes(const pg_conv_geom* g, int algo, size_t ws_bytes);              /* big2small forward -> wgrad */
int pg_conv4x4_big2small_x(const float* big, int ld_big, const float* P, const float* bias, float* small, int ld_small,
                           const pg_conv_geom* g, int act, int algo, void* ws, size_t ws_bytes, void* stream,
                           const pg_conv_extras* x);
int pg_conv4x4_small2big_x(const float* small, int ld_small, const float* P, const float* bias, float* big, int ld_big,
                           const pg_conv_geom* g, int act, int algo, void* ws, size_t ws_bytes, void* stream,
                           const pg_conv_extras* x);
int pg_conv4x4_wgrad_x(const float* small, int ld_small, const float* big, int ld_big, float* dP, float* dbias,
                       const pg_conv_geom* g, int algo, void* ws, size_t ws_bytes, void* stream, const pg_conv_extras* x);
/* The weight preparations (Winograd weight transforms; packed bf16 weights) of SEVERAL layers in one launch per kernel family: item i
 * fills items[i].u with exactly what the call `op` (0 big2small, 1 small2big) on that geometry / algo / workspace size would write into
 * pg_conv_extras.u_cache with u_valid == 0 (pg_conv_u_bytes(...) bytes; PG_EINVAL, nothing launched, if that is 0 for any item).
 * The caller then passes u_valid = 1.  A network's weights change once per step (trainer.py:90,107 optimizer.step()): one call per
 * network and step instead of one small transform kernel per layer, direction and step. */
typedef struct pg_conv_prep_item {
    pg_conv_geom g;
    int op;
    int algo;
    size_t ws_bytes;
    const float* P;
    void* u;
} pg_conv_prep_item;
int pg_conv_prep_batch(int n, const pg_conv_prep_item* items, void* stream);
/* pg_instnorm_act_fwd with the statistics pass replaced by the producer's partial sums: merge (fixed order) + normalise. */
int pg_instnorm_act_fwd_parts(const float* y, int ld_y, float* out, int ld_out, float* stats, const double* part, int chunks,
                              int N, int HW, int C, int act, float eps, float drop_p, uint64_t seed, void* stream);

/* bf16 activation storage.  The *_t forms of the InstanceNorm / activation entry points take tensors that are
 * fp32 OR bf16 (NHWC, `ld` in elements of the tensor's own type; 4-element accesses need 16- resp. 8-byte alignment, else the
 * scalar kernels run): bit i of `dt` set = the i-th tensor argument, in signature order, is bf16 --
 *     pg_instnorm_act_fwd_t / _fwd_parts_t: y, out;   pg_instnorm_act_bwd_t: g1, g2, y, dy;   pg_act_fwd_t: y, out;
 *     pg_act_bwd_t: g1, g2, a, dy.
 * Statistics (fp32), partial sums (fp64) and every arithmetic step are those of the fp32 entry points: a bf16 tensor is widened
 * on load and rounded to nearest-even on store.  dt = 0 is exactly the fp32 entry point.  pg_act_fwd_t with PG_ACT_NONE converts
 * between the two storage types. */
int pg_instnorm_act_fwd_t(const void* y, int ld_y, void* out, int ld_out, float* stats, int N, int HW, int C, int act, float eps,
                          float drop_p, uint64_t seed, void* ws, size_t ws_bytes, void* stream, int dt);
int pg_instnorm_act_fwd_parts_t(const void* y, int ld_y, void* out, int ld_out, float* stats, const double* part, int chunks,
                                int N, int HW, int C, int act, float eps, float drop_p, uint64_t seed, void* stream, int dt);
int pg_instnorm_act_bwd_t(const void* g1, int ld_g1, const void* g2, int ld_g2, const void* y, int ld_y, const float* stats,
                          void* dy, int ld_dy, int N, int HW, int C, int act, float drop_p, uint64_t seed, void* ws,
                          size_t ws_bytes, void* stream, int dt);
/* Affine InstanceNorm2d (nn.InstanceNorm2d(C, affine=True): a learnable per-channel scale gamma and shift beta, no running
 * statistics) + activation + dropout.  The plain *_t entry points with gamma, beta (C floats each, 4-byte aligned) after the
 * tensors; dt masks, `ld`, nullable g2, dropout and stream as there; same plans (single-workgroup under 512 pixels, chunked above),
 * same statistics (fp64 sums, stats = (mean, rstd)).  Every product and sum below is rounded on its own in fp32:
 *     forward    a = rstd * gamma,  b = beta - mean * a,  z = y * a + b,  out = keep / (1 - p) * act(z)
 *     backward   dz = g * keep / (1 - p) * act'(z)        (z: the forward's bits, recomputed from stats, gamma, beta)
 *                s1 = sum dz,  s2 = sum dz * (y - mean)   (per (n, c), fp64: the plain kernel's sums)
 *                dy = ((dz - s1 / HW - (y - mean) * s2 * rstd^2 / HW) * rstd) * gamma
 * With gamma = 1, beta = 0, out and dy are the plain entry points' bit for bit.
 * Parameter gradients: dgamma, dbeta (C floats each, NULL together: not computed -- the generator step's pass through D) are
 * WRITTEN, not added to: the backward leaves (s1, s2 * rstd) per (n, c) in fp64 in the first N * C * 16 bytes (rounded up to 256) of
 * ws, and one more kernel sums them over n in ascending order in fp64:  dbeta[c] = sum_n s1,  dgamma[c] = sum_n s2 * rstd.  No
 * atomics: equal inputs give equal bits.  ws: pg_instnorm_affine_workspace_bytes (that table + the plain workspace), 16-byte
 * aligned; REQUIRED (PG_EINVAL) where dgamma is given, otherwise as for the plain entry points. */
size_t pg_instnorm_affine_workspace_bytes(int N, int HW, int C);
int pg_instnorm_affine_act_fwd_t(const void* y, int ld_y, void* out, int ld_out, const float* gamma, const float* beta, float* stats,
                                 int N, int HW, int C, int act, float eps, float drop_p, uint64_t seed, void* ws, size_t ws_bytes,
                                 void* stream, int dt);
int pg_instnorm_affine_act_fwd_parts_t(const void* y, int ld_y, void* out, int ld_out, const float* gamma, const float* beta,
                                       float* stats, const double* part, int chunks, int N, int HW, int C, int act, float eps,
                                       float drop_p, uint64_t seed, void* stream, int dt);
int pg_instnorm_affine_act_bwd_t(const void* g1, int ld_g1, const void* g2, int ld_g2, const void* y, int ld_y, const float* gamma,
                                 const float* beta, const float* stats, void* dy, int ld_dy, float* dgamma, float* dbeta, int N,
                                 int HW, int C, int act, float drop_p, uint64_t seed, void* ws, size_t ws_bytes, void* stream,
                                 int dt);
int pg_act_fwd_t(const void* y, int ld_y, void* out, int ld_out, long npix, int C, int act, float drop_p, uint64_t seed,
                 void* stream, int dt);
int pg_act_bwd_t(const void* g1, int ld_g1, const void* g2, int ld_g2, const void* a, int ld_a, void* dy, int ld_dy, long npix,
                 int C, int act, float drop_p, uint64_t seed, void* stream, int dt);

/* Backward of a layer whose BIG side carries the incoming gradient -- nn.ConvTranspose2d (unet.py:53) with small = the layer's
 * input x and big = dL/dy -- in ONE call (aten::convolution_backward, trainer.py:89, is one op producing both):
 *     dP     = pg_conv4x4_wgrad(small = x, big = dy)                  (no bias: UpSampleBlock has none)
 *     dsmall = pg_conv4x4_big2small(big = dy, P)                      (dL/dx, no bias, no activation)
 * Where both halves take the polyphase Winograd path, the transformed gradient V(dy) is computed ONCE and read by both
 * GEMMs (the dy tile shared between the data- and the weight-gradient, north_star's "wgrad/dgrad fused"); otherwise the
 * call is exactly the two calls above.  Bit-identical to them either way.  ws: pg_conv_workspace_bytes(g, 3). */
int pg_conv4x4_bwd_big(const float* small, int ld_small, const float* big, int ld_big, const float* P, float* dP,
                       float* dsmall, int ld_dsmall, const pg_conv_geom* g, int algo, void* ws, size_t ws_bytes, void* stream);
/* ... with the data gradient's transformed weights in a caller-owned cache (x->u_cache / u_valid as for pg_conv4x4_big2small_x,
 * size pg_conv_u_bytes(g, 0, ...); every other field of x must be NULL / 0). */
int pg_conv4x4_bwd_big_x(const float* small, int ld_small, const float* big, int ld_big, const float* P, float* dP,
                         float* dsmall, int ld_dsmall, const pg_conv_geom* g, int algo, void* ws, size_t ws_bytes, void* stream,
                         const pg_conv_extras* x);

/* As pg_conv_time_next, for pg_conv4x4_bwd_big: the first pair goes around its weight-gradient GEMM, the second around its
 * data-gradient GEMM. */
int pg_conv_time_next2(void* ev_start, void* ev_stop, void* ev_start2, void* ev_stop2);

/* InstanceNorm2d(eps, biased var, no affine; unet.py:20,55, disc.py:32,42) + activation + Dropout(p)
 * (unet.py:28,65) over y[N, HW, C]:   out = dropout(act((y - mean_nc) * rstd_nc)).
 * stats[(n*C + c)*2 + {0,1}] receives (mean, rstd).  drop_p == 0 disables dropout; otherwise element e =
 * (n*HW + pix)*C + c is kept iff pg_dropout_keep(seed, e) and scaled by 1/(1-p). */
int pg_instnorm_act_fwd(const float* y, int ld_y, float* out, int ld_out, float* stats,
                        int N, int HW, int C, int act, float eps,
                        float drop_p, uint64_t seed, void* ws, size_t ws_bytes, void* stream);

/* Workspace (fp64 partial sums) that lets the two InstanceNorm entry points use their chunked, fully parallel path on
 * large planes; with ws == NULL or too small they fall back to one workgroup per (sample, channel group). */
size_t pg_instnorm_workspace_bytes(int N, int HW, int C);

/* Backward of the block above: given g = dL/dout (= g1 + g2, g2 may be NULL: the skip connection's
 * second consumer), the saved y and stats, writes dy = dL/dy. */
int pg_instnorm_act_bwd(const float* g1, int ld_g1, const float* g2, int ld_g2,
                        const float* y, int ld_y, const float* stats, float* dy, int ld_dy,
                        int N, int HW, int C, int act, float drop_p, uint64_t seed,
                        void* ws, size_t ws_bytes, void* stream);

/* Backward of a plain activation (+dropout) from its OUTPUT a:  dy = (g1+g2) * keep/(1-p) * act'(a).
 * act' from the output: leaky a>0?1:0.2, relu a>0, tanh 1-a^2, sigmoid a(1-a), none 1.  `a` may be NULL for
 * PG_ACT_NONE.  With drop_p > 0, `a` is the POST-dropout tensor pg_act_fwd wrote for the same (drop_p, seed) --
 * keep/(1-p) * act(y), zeros where dropped -- and the kernel multiplies it by (1-p) before taking act'; a caller that
 * saved the pre-dropout activation must pass drop_p = 0 and apply the mask to g itself. */
int pg_act_bwd(const float* g1, int ld_g1, const float* g2, int ld_g2, const float* a, int ld_a,
               float* dy, int ld_dy, long npix, int C, int act, float drop_p, uint64_t seed, void* stream);

/* Elementwise activation (+dropout) forward, for blocks without a norm whose conv could not fuse it. */
int pg_act_fwd(const float* y, int ld_y, float* out, int ld_out, long npix, int C, int act,
               float drop_p, uint64_t seed, void* stream);

/* Softmax over the channel dim (nn.Softmax(dim=1), unet.py:48-49); C need not be a multiple of 4. */
int pg_softmax_fwd(const float* y, int ld_y, float* out, int ld_out, long npix, int C, void* stream);
int pg_softmax_bwd(const float* g1, int ld_g1, const float* g2, int ld_g2, const float* out, int ld_out,
                   float* dy, int ld_dy, long npix, int C, void* stream);

/* Writes the dropout keep-mask (1.0 / 0.0) the kernels above use, for tests. */
int pg_dropout_mask(float* mask, long nelem, float drop_p, uint64_t seed, void* stream);

/* ---- BatchNorm2d (eps, momentum, affine, tracked running statistics; unet.py:20,55 and disc.py:32,42 with
 * norm_layer=nn.BatchNorm2d) + activation + Dropout(p), fp32 tensors.  y[N, HW, C] splits into `nseg` (1 or 2) SEGMENTS of
 * N / nseg consecutive samples, each normalised with its own batch statistics over its (N / nseg) * HW pixels: nseg = 2 is the
 * discriminator step's one pass over din[2N], which the reference runs as two calls (trainer.py:97,99).
 *   coef[(s*C + c)*4 + {0..3}] = (mean, rstd, scale = weight*rstd, shift = bias - mean*scale);  out = drop(act(y*scale + shift)).
 *   bstat[(s*C + c)*2 + {0,1}] = (batch mean, unbiased batch variance), fp64 (may be NULL): the input of the running update.
 * Statistics: fp64 partial sums per (sample, pixel chunk, channel), merged in a fixed order (bit-reproducible).  Where a call is one
 * kernel (planes the chunk plan does not split) the variance is two passes, a sum of (y - mean)^2.  Everywhere else -- the chunked
 * path, pg_batchnorm_stats, `part`, the split form -- it is E[y^2] - mean^2 in fp64, clamped at 0: rstd carries a relative
 * 2^-48 (1 + mean^2 / (var + eps)) there on top of its fp32 rounding.  Every
 * (N / nseg) * HW must be > 1 (torch raises "Expected more than 1 value per channel when training" there).  Dropout as
 * pg_instnorm_act_fwd.  ws: pg_batchnorm_workspace_bytes -- REQUIRED: unlike the InstanceNorm entry points, pg_batchnorm_act_fwd,
 * pg_batchnorm_stats (from y; with `part` it takes none) and pg_batchnorm_act_bwd do not fall back: a NULL or smaller workspace
 * returns PG_EWORKSPACE (nothing launched), whatever kernel the views would select. */
size_t pg_batchnorm_workspace_bytes(int N, int HW, int C, int nseg);
int pg_batchnorm_act_fwd(const float* y, int ld_y, float* out, int ld_out, const float* weight, const float* bias, float* coef,
                         double* bstat, int N, int HW, int C, int nseg, int act, float eps, float drop_p, uint64_t seed, void* ws,
                         size_t ws_bytes, void* stream);
/* The statistics half of pg_batchnorm_act_fwd (coef, bstat), from the producer's partial sums part[N][chunks][C][2] where the
 * conv epilogue emitted them (pg_conv_extras.part; y unused), else (part == NULL) from a pass over y. */
int pg_batchnorm_stats(const float* y, int ld_y, const double* part, int chunks, const float* weight, const float* bias, float* coef,
                       double* bstat, int N, int HW, int C, int nseg, float eps, void* ws, size_t ws_bytes, void* stream);
/* The normalise half: out = drop(act(y*scale + shift)) with the coefficients of the sample's segment. */
int pg_batchnorm_act_apply(const float* y, int ld_y, float* out, int ld_out, const float* coef, int N, int HW, int C, int nseg,
                           int act, float drop_p, uint64_t seed, void* stream);
/* Evaluation mode (module.eval()): coef[C][4] from the running statistics, on the device; apply with nseg = 1. */
int pg_batchnorm_eval_coef(const float* running_mean, const float* running_var, const float* weight, const float* bias, int C,
                           float eps, float* coef, void* stream);
/* Backward (trainer.py:89,106): dz = (g1 + g2) -> dropout mask -> act'(y*scale + shift); per segment
 *   train != 0:  dy = scale * (dz - sum(dz)/M - xhat * sum(dz*xhat)/M),   xhat = (y - mean) * rstd
 *   train == 0:  dy = scale * dz  (the running statistics are constants: coef from pg_batchnorm_eval_coef)
 * dweight[c] = sum over segments of sum(dz*xhat), dbias[c] = of sum(dz) -- both written (not accumulated), or both NULL (skipped). */
int pg_batchnorm_act_bwd(const float* g1, int ld_g1, const float* g2, int ld_g2, const float* y, int ld_y, const float* coef,
                         float* dy, int ld_dy, float* dweight, float* dbias, int N, int HW, int C, int nseg, int train, int act,
                         float drop_p, uint64_t seed, void* ws, size_t ws_bytes, void* stream);
/* ---- the split form (nn.SyncBatchNorm under data parallelism): "reduce -> coefficients -> apply" with room for the caller's
 * collective between the reduce and the rest.  mom[(s*C + c)*2 + {0,1}] is a caller-owned fp64 buffer of LOCAL moments per (segment,
 * channel), merged in a fixed order (bit-reproducible); the caller SUM-reduces it across ranks and passes `count`, the GLOBAL number of
 * values per (segment, channel).  A LOCAL (N / nseg) * HW of 1 is legal here; count must be > 1.  ws: pg_batchnorm_workspace_bytes of
 * the LOCAL geometry, REQUIRED as above (pg_batchnorm_moments_fwd with `part` takes none).
 *   pg_batchnorm_moments_fwd:        mom = (sum y, sum y^2), from the conv's partial sums `part` (as pg_batchnorm_stats) or a pass over y
 *   pg_batchnorm_coef_from_moments:  coef / bstat (may be NULL) as pg_batchnorm_stats writes them, from mom and count; then
 *                                    pg_batchnorm_act_apply finishes the forward
 *   pg_batchnorm_moments_bwd:        mom = (sum dz, sum dz*xhat), dz as pg_batchnorm_act_bwd forms it; dweight / dbias (both or neither)
 *                                    = the LOCAL sums over the segments, written
 *   pg_batchnorm_bwd_apply:          dy = scale * (dz - mom0/count - xhat * mom1/count) */
int pg_batchnorm_moments_fwd(const float* y, int ld_y, const double* part, int chunks, double* mom, int N, int HW, int C, int nseg,
                             void* ws, size_t ws_bytes, void* stream);
int pg_batchnorm_coef_from_moments(const double* mom, double count, const float* weight, const float* bias, float eps, float* coef,
                                   double* bstat, int C, int nseg, void* stream);
int pg_batchnorm_moments_bwd(const float* g1, int ld_g1, const float* g2, int ld_g2, const float* y, int ld_y, const float* coef,
                             double* mom, float* dweight, float* dbias, int N, int HW, int C, int nseg, int act, float drop_p,
                             uint64_t seed, void* ws, size_t ws_bytes, void* stream);
int pg_batchnorm_bwd_apply(const float* g1, int ld_g1, const float* g2, int ld_g2, const float* y, int ld_y, const float* coef,
                           const double* mom, double count, float* dy, int ld_dy, int N, int HW, int C, int nseg, int act,
                           float drop_p, uint64_t seed, void* ws, size_t ws_bytes, void* stream);
/* Running statistics of up to PG_BN_MAX_LAYERS BatchNorm layers in ONE launch: per layer, `nslots` batch statistics
 * bstat[slot][C][2] folded in slot order (running = (1 - momentum) * running + momentum * batch, in double, stored as float after
 * each), num_batches_tracked += nslots on the device (a replayed hipGraph keeps counting). */
#define PG_BN_MAX_LAYERS 16
typedef struct pg_bn_update_item {
    const double* bstat;
    float* running_mean;
    float* running_var;
    int64_t* num_batches_tracked;
    int C;
} pg_bn_update_item;
int pg_batchnorm_update_running(int n, const pg_bn_update_item* items, int nslots, float momentum, void* stream);

/* ---- losses (losses.py:18-39, trainer.py:71-85,101-103) ------------------------------------------
 * Stage 1 (per rank): pg_loss_reduce accumulates, for each (sample n, channel c), the five sums
 *   S[n][c][0..4] = { sum y*p, sum y, sum p, sum bce_elem(p, y), sum |p - y| }       (double)
 * over HW, where y is the target tensor or, when y == NULL, the constant `tconst`;
 * bce_elem = -( y*max(log p,-100) + (1-y)*max(log(1-p),-100) ).  C need not be a multiple of 4. */
int pg_loss_reduce(const float* p, int ld_p, const float* y, int ld_y, float tconst,
                   int N, int HW, int C, double* S, void* stream);
/* Number of doubles S must hold for pg_loss_reduce(N, HW, C): N*C*5 results, followed by scratch for the per-split
 * partial sums large maps are reduced through. */
long pg_loss_reduce_doubles(int N, int HW, int C);
/* Largest N * C for which pg_loss_value_grad (value + gradient of a loss term in one launch, its per-(sample, channel) table in LDS)
 * applies; beyond it the caller uses pg_loss_finalize + pg_loss_grad (same results).  Replaces nothing in the reference. */
int pg_loss_fused_max_nc(void);

/* Stage 2: gradient of a scalar loss wrt p from per-(n,c) coefficients:
 *   mode 0 (affine in y; focal-Tversky):   g = coef[n][c][0] * y + coef[n][c][1]
 *   mode 1 (BCE):                           g = coef[n][c][0] * (p - y) / max(p*(1-p), 1e-12)
 *   mode 2 (MAE):                           g = coef[n][c][0] * sign(p - y)
 * coef is float [N][C][2] on the device. */
int pg_loss_grad(const float* p, int ld_p, const float* y, int ld_y, float tconst,
                 const float* coef, float* g, int ld_g, int N, int HW, int C, int mode, void* stream);

/* Stage 1b: local2[0] = sum_n (1 - T_n) with T_n = (tp+1)/(tp + beta*fn + (1-beta)*fp + 1) (losses.py:20-26,
 * tp/fn/fp summed over all channels of sample n); local2[1] = sum_{n,c} S[n][c][1] (= torch.sum(target),
 * trainer.py:77).  Under data parallelism the caller all-reduces local2 (sum) before stage 2. */
int pg_loss_prepare(const double* S, int N, int C, float beta, double* local2, void* stream);

/* Stage 2: from S and the (global) sums gsum2, write the loss value and the coefficients for pg_loss_grad.
 * Bglobal = global batch size (N on one GPU).  Gradients are seeded for a SUM all-reduce across ranks.
 *   PG_LOSS_TVERSKY : loss = alpha * (gsum2[0]/Bglobal)^gamma                          (global value)
 *   PG_LOSS_WBCE    : loss = alpha * sum w[n][c]*S[n][c][3] / (Bglobal*C*HW), w = C>1 ? 1 - S[n][c][1]/gsum2[1] : 1
 *   PG_LOSS_MAE     : loss = alpha * sum S[n][c][4] / (Bglobal*C*HW)
 *   PG_LOSS_BCE     : loss = alpha * sum S[n][c][3] / (Bglobal*C*HW)     (nn.BCELoss, mean; alpha = 1 or 0.5)
 * For the last three the value is this rank's partial (sum over ranks = global loss). */
#define PG_LOSS_TVERSKY 0
#define PG_LOSS_WBCE 1
#define PG_LOSS_MAE 2
#define PG_LOSS_BCE 3
int pg_loss_finalize(const double* S, const double* gsum2, int mode, int N, int C, int HW, int Bglobal,
                     float alpha, float beta, float gamma, float* coef, float* loss_out, void* stream);
/* gsum2 == NULL (one process: nothing to all-reduce): pg_loss_finalize computes the two terms of pg_loss_prepare itself.
 *
 * The same loss evaluation in TWO launches instead of five (losses.py:18-39 + trainer.py:71-85,101-103 are a handful of
 * elementwise / reduction ATen ops per term; here: one reduction pass, one value + gradient pass):
 *   pg_loss_reduce_parts   stage 1 without its combine launch: S receives the partial slabs [nsplit][N*C][5]; returns nsplit >= 1
 *                          (the buffer size is pg_loss_reduce_doubles(N, HW, C) as before) or a negative PG_E* code
 *   pg_loss_value_grad     adds the slabs in slab order, forms gsum2 (or takes the all-reduced one), writes the loss value to
 *                          loss_out and -- g != NULL -- the gradient wrt p into g, with exactly the arithmetic of
 *                          pg_loss_reduce's combine + pg_loss_prepare + pg_loss_finalize + pg_loss_grad (bit-identical results).
 *                          S_out (may be NULL) receives the summed S[N*C][5].  Needs N*C <= 256 (PG_EINVAL beyond: use the
 *                          staged entry points). */
int pg_loss_reduce_parts(const float* p, int ld_p, const float* y, int ld_y, float tconst, int N, int HW, int C, double* S,
                         void* stream);
int pg_loss_value_grad(const double* Spart, int nsplit, double* S_out, const double* gsum2, int mode, int N, int C, int HW,
                       int Bglobal, float alpha, float beta, float gamma, const float* p, int ld_p, const float* y, int ld_y,
                       float tconst, float* g, int ld_g, float* loss_out, void* stream);

/* ---- segmentation metrics (beyond the reference, which reports loss scalars only; the call sites are patchgan_amd's
 * Trainer.batch(train=False) beside the segmentation loss's pg_loss_reduce_parts, and Trainer.evaluate) -------------
 * The integer counts IoU / Dice / precision / recall / pixel accuracy are made of.  p (prediction) and y (target) are fp32 NHWC channel
 * slices as pg_loss_reduce takes them.  K = 2 for C == 1, else K = C; `counts` holds K*K + 1 64-bit words on the device and the call
 * ADDS to them (one buffer collects a whole validation pass; the caller zeroes it):
 *   counts[t*K + q]  pixels of true class t predicted as class q
 *   counts[K*K]      ignored pixels
 *   C == 1: q = (p >= threshold), t = (y >= 0.5f); nothing is ignored.
 *   C  > 1: q / t = FIRST index of the maximum of p[0..C) / y[0..C) (strict `>` scan from channel 0: numpy.argmax, pg_tiles_blend --
 *           q is the class patchgan_infer writes); `threshold` is not read.  A pixel whose largest y is <= 0 has no listed label (a
 *           one-hot mask over a label subset): it is ignored -- counts[K*K] += 1 and nothing else.
 * Inputs are finite (NaN: unspecified).  Integer atomics only: the sums do not depend on arrival order.
 * PG_EINVAL before any launch: NULL p, y or counts; N, HW or C <= 0; C > pg_seg_confusion_max_c(); ld_p < C; ld_y < C. */
int pg_seg_confusion_max_c(void);    /* 32 */
int pg_seg_confusion(const float* p, int ld_p, const float* y, int ld_y, int N, int HW, int C, float threshold,
                     unsigned long long* counts, void* stream);
/* Per-class prediction histograms: the table every score CURVE is made of (IoU / Dice / precision / recall at every threshold k / bins,
 * average precision, the threshold to infer with; patchgan_amd's Trainer.metric_bins launches it after pg_seg_confusion on the same
 * views).  p and y as above; `hist` holds C*2*bins + 1 64-bit words on the device and the call ADDS to them:
 *   hist[(c*2 + t)*bins + b]  pixels of channel c with label t (one-vs-rest) whose prediction p[c] falls into bin b
 *   hist[C*2*bins]            ignored pixels
 *   bin:   b = bins-1 if p >= 1; b = 0 if p <= 0; otherwise b = (int)(p * (float)bins).  bins is a power of two in 16..1024, so the
 *          product is exact in fp32 and b >= k exactly when p >= k / bins: the sums over b >= k are the counts pg_seg_confusion gives
 *          at threshold k / bins.
 *   label: C == 1: t = (y >= 0.5f), nothing is ignored.  C > 1: t = (c == first index of the maximum of y[0..C)), the scan of
 *          pg_seg_confusion; a pixel whose largest y is <= 0 only adds 1 to the ignored word, every other pixel adds one count per
 *          channel.
 * Inputs are finite (NaN: unspecified).  Integer atomics only: the sums do not depend on arrival order.
 * PG_EINVAL before any launch: NULL p, y or hist; N, HW or C <= 0; C > pg_seg_confusion_max_c(); bins not a power of two in
 * 16..1024; C * bins > pg_seg_hist_max_words(); ld_p < C; ld_y < C. */
int pg_seg_hist_max_words(void);     /* 8192: largest C * bins */
int pg_seg_hist(const float* p, int ld_p, const float* y, int ld_y, int N, int HW, int C, int bins, unsigned long long* hist,
                void* stream);

/* ---- optimizer (torch.optim.Adam defaults, trainer.py:169-172) -----------------------------------
 * m += (g-m)*(1-b1); v = v*b2 + (1-b2)*g*g; p -= (lr/bc1) * m / (sqrt(v)/sqrt_bc2 + eps)
 * over n contiguous floats; bc1 = 1-b1^t and sqrt_bc2 = sqrt(1-b2^t) are computed by the caller. */
int pg_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                 float eps, float bc1, float sqrt_bc2, void* stream);
/* The same update with the two step-dependent scalars read from DEVICE memory: scalars[0] = lr / bc1, scalars[1] = sqrt(bc2) (floats the
 * caller wrote there, stream-ordered before this launch).  The launch then carries nothing that changes from step to step, so a
 * captured hipGraph of the whole G+D step (Trainer.graph) can be replayed with a new Adam step count and learning rate
 * (optimizer.step() of trainer.py:90,107 inside the replayed step). */
int pg_adam_step_dev(float* p, const float* g, float* m, float* v, long n, float beta1, float beta2, float eps, const float* scalars,
                     void* stream);
/* Both forms with an exponential moving average of the parameters kept in the same pass: after the Adam update of an element,
 * ema += (p_new - ema) * (1 - ema_decay) in fp32, from the value just stored to p (5 reads + 4 writes per element; the update followed
 * by a separate averaging pass takes 4 + 3 and 2 + 1).  p, m and v receive exactly what pg_adam_step / pg_adam_step_dev give them.
 * `ema` holds n floats and must not alias p, g, m or v; the pointer requirements are those of pg_adam_step (non-NULL, 16-byte
 * aligned).  ema_decay in [0, 1): PG_EINVAL for a NaN or a value outside, before any launch. */
int pg_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float beta1, float beta2,
                     float eps, float bc1, float sqrt_bc2, float ema_decay, void* stream);
int pg_adam_ema_step_dev(float* p, const float* g, float* m, float* v, float* ema, long n, float beta1, float beta2, float eps,
                         const float* scalars, float ema_decay, void* stream);

/* ---- gradient-norm clipping and non-finite step skip (beyond the reference, whose users put torch.nn.utils.clip_grad_norm_ between
 * backward() and optimizer.step(); the call site is patchgan_amd's Trainer._adam_step with Trainer.clip_grad_norm set) -----------------
 * pg_grad_norm: the 2-norm of the n floats of g, the sum of squares accumulated in fp64 (the square of a float is exact there, and
 * 1e25 * sqrt(k) is a norm, not inf).  Two launches: workgroup b of B = pg_grad_norm_workspace_bytes(n) / 8 sums the 16-byte groups
 * b*256 + lane, + B*256, ... of g (one fp64 accumulator per lane and component, then lanes, then waves, in a fixed tree; the n % 4 tail
 * elements go to the first lanes of workgroup 0) into ws[b]; one workgroup then sums ws[0 .. B) in a fixed order and writes `stat`.  No
 * floating-point atomics, nothing depends on which workgroup finishes first: equal inputs give equal bits.
 * The status block lives on the device, one per network, 64 bytes, 16-byte aligned; the caller zeroes it once (that also resets the
 * accumulators) and every call updates it:
 *   norm     (float)sqrt(sumsq)
 *   coef     min(1, max_norm / (norm + 1e-6)) formed in double from the fp64 norm, rounded once (torch's clip_grad_norm_); 0 on a skip
 *   apply    1, or 0 = "skip": sumsq is not finite (a NaN or +-inf anywhere in g)
 *   steps, clipped (coef < 1), skipped: counts of calls;  max_norm, sum_norm: the largest and the fp64 sum of the FINITE norms
 *   sumsq    the fp64 sum of squares of this call
 * max_norm > 0, +inf allowed (coef == 1 exactly: a pure monitor).  PG_EINVAL before any launch, nothing touched: max_norm <= 0 or NaN,
 * n <= 0, a NULL g, ws or stat, g or stat not 16-byte aligned, ws not 8-byte aligned, ws_bytes < pg_grad_norm_workspace_bytes(n). */
typedef struct pg_grad_stat {
    float norm, coef;
    unsigned apply, reserved;
    unsigned long long steps, clipped, skipped;
    double max_norm, sum_norm, sumsq;
} pg_grad_stat;
long pg_grad_norm_workspace_bytes(long n);          /* 8 bytes per workgroup of the first launch; 0 for n <= 0 */
int pg_grad_norm(const float* g, long n, double max_norm, void* ws, long ws_bytes, pg_grad_stat* stat, void* stream);
/* pg_adam_step / pg_adam_ema_step (ema != NULL) / their _dev forms on g' = g * stat->coef: ONE fp32 product per element, what torch's
 * grad.mul_(coef) stores; g itself is only read (28 / 36 bytes per parameter, as without clipping).  With stat->apply == 0 the kernel
 * returns before it loads anything else: p, m, v and ema keep their bits.  With coef == 1 the results are bit-identical to the plain
 * calls.  `stat` is what pg_grad_norm wrote, stream-ordered before this launch.  ema_decay is read only with ema != NULL. */
int pg_adam_clip_step(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float beta1, float beta2, float eps,
                      float bc1, float sqrt_bc2, float ema_decay, const pg_grad_stat* stat, void* stream);
int pg_adam_clip_step_dev(float* p, const float* g, float* m, float* v, float* ema, long n, float beta1, float beta2, float eps,
                          const float* scalars, float ema_decay, const pg_grad_stat* stat, void* stream);

/* ---- decoupled weight decay (beyond the reference, whose users swap optim.Adam for optim.AdamW; the call site is patchgan_amd's
 * Trainer._adam_step with Trainer.weight_decay set) ---------------------------------------------------------------------------------
 * Per element: p0 = p * decay_mul as ONE fp32 product, then exactly the update of pg_adam_step on (p0, g * coef, m, v), then the
 * average of pg_adam_ema_step from the stored p.  decay_mul is formed by the caller in double and rounded once,
 * (float)(1.0 - (double)lr * weight_decay): torch.optim.AdamW's param.mul_(1 - lr * weight_decay) ahead of the moment updates -- the
 * decay uses lr, not lr / bc1 --, so m and v do not depend on it.  One multiply and no memory access more: 28 / 36 bytes per
 * parameter as without it.
 * ema == NULL: no weight average (ema_decay is not read).  stat == NULL: no clipping (coef = 1, no skip); otherwise `stat` is what
 * pg_grad_norm wrote, and stat->apply == 0 ends the kernel before it loads anything else: p (its decay included), m, v and ema keep
 * their bits.  All four combinations are legal.  With decay_mul == 1 the results are bit-identical to pg_adam_step /
 * pg_adam_ema_step / pg_adam_clip_step (and their _dev forms) for the same (ema, stat).
 * The _dev form reads scalars[0] = lr / bc1, scalars[1] = sqrt(bc2), scalars[2] = decay_mul from device memory (pg_adam_step_dev).
 * PG_EINVAL before any launch, nothing touched: the pointer and alignment rules of pg_adam_step (ema and stat, where given, 16-byte
 * aligned as well; bc1, sqrt_bc2 > 0; a NULL scalars); decay_mul NaN or outside (0, 1]; beta1 or beta2 NaN or outside [0, 1);
 * with ema != NULL an ema_decay NaN or outside [0, 1). */
int pg_adamw_step(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float beta1, float beta2, float eps,
                  float bc1, float sqrt_bc2, float decay_mul, float ema_decay, const pg_grad_stat* stat, void* stream);
int pg_adamw_step_dev(float* p, const float* g, float* m, float* v, float* ema, long n, float beta1, float beta2, float eps,
                      const float* scalars /* [0] lr / bc1, [1] sqrt(bc2), [2] decay_mul */, float ema_decay,
                      const pg_grad_stat* stat, void* stream);

/* ---- gradient accumulation (beyond the reference, whose users sum .grad over a few backward() calls before optimizer.step(); the
 * call site is patchgan_amd's Trainer._adam_step with Trainer.accumulate set) ----------------------------------------------------------
 * One streaming pass over n contiguous floats of the accumulator `acc` and the flat gradient `g`, element by element:
 *   PG_ACC_BEGIN       acc = g                     (g only read;   8 bytes per element)
 *   PG_ACC_ADD         acc = acc + g               (g only read;  12 bytes per element)
 *   PG_ACC_CLOSE       g = (acc + g) * scale       (acc only read; 12 bytes per element)
 *   PG_ACC_CLOSE_ONLY  g = acc * scale             (acc only read;  8 bytes per element: a window closed short of its last gradient)
 * ONE fp32 add and then ONE fp32 multiply, never fused (the library is built without contraction): numpy.float32 arithmetic in that
 * order gives the same bits; NaN and inf propagate.  `scale` is 1 / (number of gradients in the window), formed by the caller in double
 * and rounded once; the first two modes do not read it.  No atomics, nothing depends on the order of the workgroups.
 * PG_EINVAL before any launch, nothing touched: a NULL acc or g, either not 16-byte aligned, n <= 0, an unknown mode, ranges
 * [acc, acc + n) and [g, g + n) that intersect, and in the two closing modes a scale that is NaN or outside (0, 1]. */
#define PG_ACC_BEGIN 0
#define PG_ACC_ADD 1
#define PG_ACC_CLOSE 2
#define PG_ACC_CLOSE_ONLY 3
int pg_grad_accum(float* acc, float* g, long n, int mode, float scale, void* stream);

/* ---- spectral normalisation of conv weights (beyond the reference, whose users wrap each nn.Conv2d of the discriminator in
 * torch.nn.utils.spectral_norm; the call sites are patchgan_amd's Discriminator(spectral_norm=True) and Trainer._enqueue_step /
 * _adam_step) --------------------------------------------------------------------------------------------------------------------
 * One item per conv layer, at most PG_SN_MAX_LAYERS per call.  W is the layer's PACKED block [16 taps][Cout][Cin] (tap = kh*4 + kw);
 * torch's matrix is Wm = weight.reshape(Cout, Cin*16), Wm[o][ci*16 + tap] = W[(tap*Cout + o)*Cin + ci].  u (Cout floats) and v (Cin*16
 * floats) are stored in torch's order -- weight_u / weight_v of the state_dict --, the kernels do the index arithmetic.  eps = 1e-12.
 * pg_spectral_fwd, per item (what one forward of torch's hook computes, in training mode with `iterate`, in eval mode without):
 *   iterate != 0:  t = Wm^T u;  v <- t / max(|t|_2, eps);   s = Wm v;  u <- s / max(|s|_2, eps);  sigma = u^T s with the u just stored
 *   iterate == 0:  u, v are only read;                      s = Wm v;                             sigma = u^T s
 *   w_hat = W / sigma, element by element in the packed layout (16*Cout*Cin floats; must not alias W).
 *   With flat != NULL the call also copies every float of flat[0 .. nflat) that lies outside the items' blocks to the same offset of
 *   `eff` (biases, norm parameters): the items' W are then blocks of `flat` in ascending order and w_hat == eff + (W - flat), nflat % 4
 *   == 0 -- `eff` ends up as the network's parameter buffer with every conv weight normalised.  flat == eff == NULL: no copy.
 *   Up to five launches (k_sn_wtu, k_sn_v -- only with an iterating item --, k_sn_wv, k_sn_u, k_sn_scale), each over all items.
 * pg_spectral_bwd: the flat gradient `grad` (ngrad floats) holds, at g_off of each item, the gradient w.r.t. w_hat in the packed layout
 *   and receives the gradient w.r.t. W in place, u, v, sigma constants and sigma differentiated:
 *   c = <dw_hat, w_hat> over the layer;  dW[o][k] = (dw_hat[o][k] - c * u[o] * v[k]) / sigma.  Floats outside the blocks are not touched.
 *   Two launches (k_sn_dot, k_sn_map); u, v, sigma, w_hat are what pg_spectral_fwd left, stream-ordered before this call.
 * Arithmetic: every sum is fp64 in an order that depends on the shapes alone -- per lane in index order, the 64 lanes of a wave by
 * halving distances 32 .. 1, waves and workgroup partials in index order --, phases exchange partial sums through `ws` between
 * launches, no workgroup reads what another wrote in the same launch, no floating-point atomics: equal inputs give equal bits in
 * every launch mode, run and rank (as pg_grad_norm).  Each stored float is ONE rounding of an fp64 expression of the stored fp32
 * inputs: v = fl(t / max(sqrt(sum t^2), eps)) with t the fp64 column sums, u likewise from the fp64 row sums s of W and the STORED
 * v, sigma = fl(sum_o u[o] * s[o]), w_hat = fl(W / sigma), dW = fl((dw_hat - (c * u[o]) * v[k]) / sigma) with c the fp64 dot product.
 * `ws`: pg_spectral_workspace_bytes(n, items) bytes (0 for a bad list), 8-byte aligned, one per stream that runs these calls.
 * PG_EINVAL before any launch, nothing touched: n <= 0 or > PG_SN_MAX_LAYERS, NULL items, a NULL W / w_hat / u / v / sigma, Cout or
 * Cin <= 0 or > 65536, W or w_hat not 16-byte aligned, g_off < 0 or not a multiple of 4, a NULL or misaligned or too small ws;
 * pg_spectral_fwd: flat / eff not both NULL or both 16-byte aligned with the items laid out as above; pg_spectral_bwd: a NULL or
 * misaligned grad, a block that ends beyond ngrad.  The all-zero matrix (sigma == 0) divides by zero, as torch does. */
#define PG_SN_MAX_LAYERS 16
typedef struct pg_spectral_item {
    const float* W;      /* packed weights [16][Cout][Cin] */
    float* w_hat;        /* out: W / sigma, the same layout */
    float* u;            /* [Cout], updated when iterate != 0 */
    float* v;            /* [Cin*16] in torch's (ci, kh, kw) order, updated when iterate != 0 */
    float* sigma;        /* out: one float */
    long g_off;          /* pg_spectral_bwd: first float of the layer's block in the flat gradient */
    int Cout, Cin, iterate;
} pg_spectral_item;
long pg_spectral_workspace_bytes(int n, const pg_spectral_item* items);
int pg_spectral_fwd(int n, const pg_spectral_item* items, const float* flat, float* eff, long nflat, void* ws, long ws_bytes,
                    void* stream);
int pg_spectral_bwd(int n, const pg_spectral_item* items, float* grad, long ngrad, void* ws, long ws_bytes, void* stream);

/* ---- layout(the reference is NCHW end to end; trainer.py:55-66) ---------------------------------- */
int pg_nchw_to_nhwc(const float* src, float* dst, int ld_dst, int N, int C, int H, int W, void* stream);
int pg_nhwc_to_nchw(const float* src, int ld_src, float* dst, int N, int C, int H, int W, void* stream);
/* The discriminator's two concatenated inputs in one pass (trainer.py:65-66,96-99: torch.cat((x, y), 1) and torch.cat((x, gen_img), 1)):
 * real[n][hw][0 .. ld) = x[n] | y[n] | 0-pad, fake[n][hw][0 .. ld) = x[n] | 0 (the generator's output is written into channels Cx ..
 * Cx + Cy - 1 of `fake` later); x, y contiguous NCHW fp32, real / fake NHWC with pixel stride ld (Cx + Cy <= ld <= 8). */
int pg_din_fill(const float* x, const float* y, float* real, float* fake, int ld, int N, int Cx, int Cy, int H, int W, void* stream);
/* dst[pix*ld_dst + c] = src[pix*ld_src + c] for c < C  (channel-slice copy; C need not be a multiple of 4) */
int pg_copy_channels(const float* src, int ld_src, float* dst, int ld_dst, long npix, int C, void* stream);
int pg_fill(float* dst, long n, float value, void* stream);
/* fp32 NHWC channel slice (C <= 8, pixel stride ld_src) -> bf16 tensor in 8-channel pixels (ld 8, channels C..7 zero, 16-byte-aligned
 * dst): the form in which the PG_ALGO_BF16 kernels take the image-facing tensors (x, x | mask, dL/d(generator output)) -- one 16-byte
 * LDS-DMA piece per pixel.  pg_conv4x4_big2small / _wgrad with PG_IO_BIG_BF16, Cb <= 8 and ld_big == 8 read that layout. */
int pg_pad8_bf16(const float* src, int ld_src, void* dst, long npix, int C, void* stream);

/* ---- input pipeline on the device (io.py:42-56: the dataset's `/ 255.` and one-hot mask) ----------------
 * dst[pix*ld_dst + c] = (float)src[pix*C + c] / div : decoded image bytes [npix][C] (HWC) into an NHWC channel slice */
int pg_u8_to_f32(const unsigned char* src, float* dst, int ld_dst, long npix, int C, float div, void* stream);
/* dst[pix*ld_dst + i] = ((unsigned char)(src[pix] + add) == labels[i]) ? 1 : 0 for i < nlabels <= PG_MAX_LABELS; `labels` is
 * a HOST array (copied into the launch); add = 1 reproduces the reference's uint8 `read_image(mask) + 1` incl. 255 -> 0 */
#define PG_MAX_LABELS 32
int pg_labels_to_onehot(const unsigned char* src, float* dst, int ld_dst, long npix, const int* labels, int nlabels, int add,
                        void* stream);

/* ---- tiled inference (infer.py:14-68: n_crop / build_mask around the generator forward) -----------
 * Tile k of an axis of `extent` pixels starts at k*eff - max(k*eff + size - extent, 0), eff = int(overlap*size),
 * k < pg_tiles_count(extent, size, eff) = ceil(extent / eff) (0 if extent < size: the reference cannot tile such an image).
 * Tiles are numbered row-major over (y tile, x tile) -- the reference's j*ncropsy + i on the square images it supports. */
int pg_tiles_count(int extent, int size, int eff);
/* n_crop (infer.py:14-35): image [C,H,W] (CHW, the dataset item layout) -> tiles [ny*nx, size, size, ld] NHWC, the batch
 * the generator kernels read */
int pg_tiles_gather(const float* image, int C, int H, int W, int size, int eff, float* tiles, int ld, void* stream);
/* build_mask (infer.py:38-68): predicted tiles [ny*nx, size, size, ld] NHWC -> overlap average in double, in tile order
 * (bit-identical to the reference's `mask += tile.double(); mask / count`), `>= threshold` -> {0,1} when threshold > 0.
 * mask: [C,H,W] doubles or NULL; argmax: [H,W] int64 class index (first maximum, numpy.argmax) or NULL. */
int pg_tiles_blend(const float* tiles, int ld, int C, int size, int eff, int H, int W, double threshold, double* mask,
                   long long* argmax, void* stream);

/* ---- test-time augmentation and windowed blend around the same tiles ------------------------------
 * K = 1, 2, 4 or 8 variants of every tile travel through the generator as further samples: with T = ny*nx tiles the batch holds
 * K*T samples and variant k of tile t is sample k*T + t (K = 1: the layout of pg_tiles_gather).  Variant k is the [C,size,size]
 * tile after, in this order,  k & 4: transpose(-1,-2);  k & 2: flip(-2);  k & 1: flip(-1)  -- K = 2 the horizontal flip, K = 4 both
 * flips, K = 8 the dihedral group.  The largest K: */
int pg_tiles_tta_max(void);   /* 8 */
/* image [C,H,W] -> tiles [K*ny*nx, size, size, ld] NHWC.  PG_EINVAL before any launch: NULL image or tiles, C <= 0, ld < C,
 * K not in {1,2,4,8}, H or W smaller than size. */
int pg_tiles_gather_tta(const float* image, int C, int H, int W, int size, int eff, int K, float* tiles, int ld, void* stream);
/* predicted tiles [K*ny*nx, size, size, ld] -> weighted average in the image frame.  `window`: `size` doubles on the device, every
 * one finite and > 0 (the caller's duty); tile t at (sy, sx) weighs pixel (h, w) with window[h - sy] * window[w - sx].  Prediction
 * variant k is read through the inverse map (the three steps undone in reverse order).  Per pixel and class, in doubles, each
 * product and sum rounded once and none contracted into an FMA:
 *     for t ascending over the tiles covering (h, w):  wgt = window[h - sy] * window[w - sx]
 *         for k < K:  acc = acc + wgt * (double)pred[k*T + t];  wsum = wsum + wgt
 *     v = acc / wsum
 * then threshold and first-maximum argmax as in pg_tiles_blend, whose result this is bit for bit when the window is all ones and
 * K = 1.  Only the covering tiles are visited; duplicate tiles (the clamped end of an axis) each count.  mask: [C,H,W] doubles or
 * NULL; argmax: [H,W] int64 or NULL.  PG_EINVAL before any launch: NULL tiles or window, both outputs NULL, C <= 0, ld < C,
 * K not in {1,2,4,8}, H or W smaller than size. */
int pg_tiles_blend_win(const float* tiles, int ld, int C, int size, int eff, int H, int W, int K, const double* window,
                       double threshold, double* mask, long long* argmax, void* stream);

/* ---- differentiable augmentation of the discriminator's inputs (beyond the reference; Zhao et al. 2020, "Differentiable Augmentation
 * for Data-Efficient GAN Training": the call sites are patchgan_amd's Trainer.diffaug) ---------------------------------------------------
 * A per-sample map T of pixels -- horizontal flip, then translation with zero padding, then a zeroed box --, applied to what the
 * discriminator reads (real and fake alike) and, as its exact adjoint, to the gradient that returns to the generator.  Policy bits: */
#define PG_AUG_FLIP 1
#define PG_AUG_TRANSLATION 2
#define PG_AUG_CUTOUT 4
/* The table: params[N][8] int32 on the device, row n = {flip, ty, tx, cut_top, cut_left, cut_h, cut_w, 0} of GLOBAL sample sample0 + n.
 * Every draw is a pure function of (seed, step count t, global sample index s, draw index k), all arithmetic modulo 2^64, with
 * mix64 = pg_mix64 of csrc/pg_common.h (x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31),
 * GOLD = 0x9e3779b97f4a7c15 and DOMAIN = 0x6469666661756721:
 *     key  = mix64(mix64((seed ^ DOMAIN) + GOLD * (t + 1)) + GOLD * (s + 1))
 *     r[k] = mix64(key + GOLD * (k + 1))
 *     flip     = r[0] >> 63
 *     ty       = (r[1] >> 32) % (2 * (H / 8) + 1) - H / 8          tx = (r[2] >> 32) % (2 * (W / 8) + 1) - W / 8
 *     cut_h    = H / 2,  cut_w = W / 2
 *     cut_top  = (r[3] >> 32) % (H + 1) - cut_h / 2                 cut_left = (r[4] >> 32) % (W + 1) - cut_w / 2
 * (integer divisions; the modulo bias of 32 random bits over at most a few thousand values is ignored).  The box covers rows
 * cut_top <= h < cut_top + cut_h and columns likewise, and may hang over the border.  A policy bit that is off gives the neutral
 * value: flip 0, ty = tx = 0, the empty box {0, 0, 0, 0}.  A counter-based stream like the dropout mask's: a table split into two
 * calls with shifted sample0 has the same rows, and the ranks of a data-parallel job draw what the single process draws.
 * The step count t: with counter != NULL (a 64-bit device word, 8-byte aligned) t = *counter and the kernel stores t + 1 behind
 * every read of it -- the launch then carries nothing that changes from step to step, so a captured step replays with fresh draws
 * (as pg_adam_step_dev and pg_batchnorm_update_running do); with counter == NULL, t is the host argument `step`.  One workgroup.
 * Writes the N * 8 table words and the counter word, nothing else.  PG_EINVAL before any launch: NULL or misaligned params,
 * misaligned counter, N, H or W <= 0, sample0 < 0, policy outside 0 .. 7. */
int pg_diffaug_params(uint64_t seed, unsigned long long* counter, uint64_t step, int policy, long sample0, int N, int H, int W, int* params,
                      void* stream);
/* dst = T(src): fp32 NHWC channel slices [N,H,W,C] (C need not be a multiple of 4; 16-byte moves where bases, ld and C allow).  Per
 * output pixel (h, w) of sample n, with row n of the table:  inside the box -> 0;  hs = h - ty, ws = w - tx, outside the image -> 0;
 * if flip: ws = W - 1 - ws;  dst[n,h,w,:] = src[n,hs,ws,:].  Values are moved, never computed on: bit-exact.  The table is trusted
 * for its VALUES only (any int32 content is safe: coordinates are checked before the read).  Writes the C channels of each dst
 * pixel.  PG_EINVAL before any launch: NULL pointers, ld < C, N*H*W >= 2^31, src and dst ranges that intersect. */
int pg_diffaug_fwd(const float* src, int ld_src, float* dst, int ld_dst, const int* params, int N, int H, int W, int C, void* stream);
/* dsrc = T^t(g), the exact adjoint, written as a gather: T is an injective partial map of pixels, so every dsrc element is one g
 * element or 0 and is written exactly once -- no atomics.  Per dsrc pixel (hs, w0):  ws = flip ? W - 1 - w0 : w0;  h = hs + ty,
 * w = ws + tx;  outside the image or inside the box -> 0;  dsrc[n,hs,w0,:] = g[n,h,w,:].  Same argument rules as pg_diffaug_fwd. */
int pg_diffaug_bwd(const float* g, int ld_g, float* dsrc, int ld_dsrc, const int* params, int N, int H, int W, int C, void* stream);

/* ---- GAN objectives on the discriminator's patch map (beyond the reference, whose objective is nn.BCELoss on a sigmoid map; the call
 * sites are patchgan_amd's Trainer.gan_mode) -------------------------------------------------------------------------------------------
 * A term is one mean over the n = N*HW values d[i * ld] of a one-channel patch map -- logits, or probabilities for PG_GAN_LSGAN on a
 * sigmoid head --, its per-element value e(d) by `kind`:
 *   PG_GAN_LSGAN       e = (d - target)^2                                           de/dd = 2 (d - target)        (F.mse_loss)
 *   PG_GAN_HINGE_D     target == 1:  e = max(0, 1 - d)                              de/dd = -1 where 1 - d > 0, else 0
 *                      target == 0:  e = max(0, 1 + d)                              de/dd = +1 where 1 + d > 0, else 0   (F.relu)
 *   PG_GAN_HINGE_G     e = -d                                                       de/dd = -1
 *   PG_GAN_BCE_LOGITS  e = max(d, 0) - d * target + log1p(exp(-|d|))                de/dd = sigmoid(d) - target
 *                                                                                   (F.binary_cross_entropy_with_logits)
 * A value exactly on a hinge margin contributes 0 to value and gradient (torch's relu backward).  A NaN in d gives a NaN value and a
 * NaN gradient at that element in every kind, the hinges included.
 *   *value = fl32(scale * sum_i e(d[i])),  scale = alpha / (Bglobal * HW) formed by the caller in double: this rank's partial of the
 *            global mean (the sum over ranks is the loss; PG_LOSS_BCE's convention).  e is fp32 arithmetic, the sum fp64 in an order
 *            that depends on n alone (per lane in index order, a halving tree over the workgroup, workgroup partials in index order).
 *   g[i * ld_g] = fl32(scale) * de/dd, in fp32, seeded for a SUM all-reduce; g == NULL: value only.
 * Up to PG_GAN_MAX_TERMS terms per call run in ONE launch, one workgroup per term, while every n <= pg_gan_loss_single_max(); a call
 * with a larger term takes the partial-slab path instead -- one launch that writes each workgroup's partial sum into `ws` (and the
 * gradients) and one that adds them in index order -- and needs pg_gan_loss_workspace_bytes(nterms, terms) bytes of 8-byte-aligned
 * `ws` (0 on the one-launch path, where ws may be NULL).  No workgroup reads what another wrote in the same launch; the path and the
 * result bits are functions of the arguments alone.
 * PG_EINVAL before any launch, nothing written: NULL terms, nterms <= 0 or > pg_gan_loss_max_terms(), a NULL d or value, n <= 0,
 * ld < 1, g with ld_g < 1, an unknown kind, PG_GAN_HINGE_D with a target other than 0 or 1, a NULL, misaligned or too small ws where
 * one is needed. */
#define PG_GAN_LSGAN 0
#define PG_GAN_HINGE_D 1
#define PG_GAN_HINGE_G 2
#define PG_GAN_BCE_LOGITS 3
#define PG_GAN_MAX_TERMS 4
typedef struct pg_gan_term {
    const float* d;      /* patch values, element i at d[i * ld] */
    float* g;            /* out: gradient, element i at g[i * ld_g]; NULL = value only */
    float* value;        /* out: one float */
    double scale;        /* alpha / (Bglobal * HW) */
    long n;              /* N * HW */
    int ld, ld_g, kind;
    float target;
} pg_gan_term;
int pg_gan_loss_max_terms(void);      /* PG_GAN_MAX_TERMS */
long pg_gan_loss_single_max(void);    /* the largest n of the one-launch path */
long pg_gan_loss_workspace_bytes(int nterms, const pg_gan_term* terms);      /* 0 for a bad list as well */
int pg_gan_loss(int nterms, const pg_gan_term* terms, void* ws, long ws_bytes, void* stream);

/* ---- segmentation objectives on the generator's output (beyond the reference, whose objectives are focal-Tversky, weighted BCE and
 * MAE; the call sites are patchgan_amd's Trainer.loss_type = 'ce' | 'focal' | 'dice' and their '+'-joined sums) -------------------------
 * p (the generator's output, probabilities of a softmax or sigmoid head) and y (the target) are fp32 NHWC channel slices as
 * pg_loss_reduce takes them: element (n, i, c) at [(n * HW + i) * ld + c], 4-byte aligned only, any C >= 1 with ld >= C, any N, any HW,
 * any N * C; every pixel offset is formed in 64 bits.  `terms` is an OR of PG_SEG_CE, PG_SEG_FOCAL, PG_SEG_DICE.  With
 *   lp = max(log p, -100),  lq = max(log(1 - p), -100)   (logf(p), log1pf(-p): pg_loss_reduce's bce_elem),  q = 1 - p,
 *   x^k = x^(k-1) * x from x^0 = 1 (repeated multiplication, no powf),  g = focal_gamma, an integer in 0 .. PG_SEG_FOCAL_GAMMA_MAX,
 *   a1 = focal_alpha, a0 = 1 - focal_alpha, or a1 = a0 = 1 for focal_alpha == PG_SEG_FOCAL_ALPHA_NONE,
 * the members are
 *   PG_SEG_CE     e = -y lp                                                    de/dp = -y / max(p, 1e-12)
 *                 value scale_ce * sum e, scale_ce = alpha / (Bglobal * HW): categorical cross-entropy on probabilities, a mean over
 *                 pixels.  A pixel whose y is all zero has no listed label (the pixels pg_seg_confusion ignores): it adds nothing to
 *                 value or gradient and still counts in the normaliser.  Needs C >= 2.  Not logit-space cross-entropy: the head stays
 *                 pg_softmax_fwd / pg_softmax_bwd, so a softmax output that underflows to 0 at the labelled class gets lp = -100 and
 *                 a gradient -y / 1e-12 which pg_softmax_bwd multiplies by p = 0.
 *   PG_SEG_FOCAL  e = -(a1 y q^g lp + a0 (1 - y) p^g lq)                        (Lin et al. 2017, the binary form on every channel)
 *                 de/dp = -a1 y (q^g / max(p, 1e-12) - g q^(g-1) lp) - a0 (1 - y) (g p^(g-1) lq - p^g / max(q, 1e-12));
 *                 for g == 0 the two g * ... terms are absent (never 0 * x): with PG_SEG_FOCAL_ALPHA_NONE that is bce_elem.
 *                 value scale_focal * sum e, scale_focal = alpha / (Bglobal * C * HW).
 *   PG_SEG_DICE   per (n, c) over HW: I = sum p y, P = sum p, Y = sum y, D = (2 I + s) / (P + Y + s), s = dice_smooth > 0;
 *                 value scale_dice * sum_{n,c} (1 - D), scale_dice = alpha / (Bglobal * C);
 *                 gradient k0[n,c] * y + k1[n,c], k0 = fl32(-2 scale_dice / den), k1 = fl32(scale_dice (2 I + s) / den^2),
 *                 den = P + Y + s, both formed in fp64 from the fp64 sums.
 * The scales are formed by the caller in double (as pg_gan_term.scale): each value is this rank's partial of the global mean and the
 * gradients are seeded for a SUM all-reduce (PG_LOSS_MAE's convention); the loss needs no collective.  Element arithmetic is fp32, in
 * the order the expressions above are written from the left (-ffp-contract=off); sums and Dice coefficients are fp64.
 * A NaN in p gives a NaN value and a NaN gradient at that element in every member (the clamps keep it, for any y); under PG_SEG_DICE
 * the whole (n, c) plane's gradient is NaN.
 *
 * Two launches per evaluation:
 *   pg_seg_loss_reduce      for each (sample n, slab z, channel c) the five sums {I, P, Y, sum e_ce, sum e_focal} over the slab's pixels
 *                           into ws[((n * nslab + z) * C + c) * 5 + k]; sums the mask does not select are written as 0.
 *                           nslab = pg_seg_loss_slabs(N, HW) = clamp(HW / 1024, 1, min(128, max(1, 1024 / N))): two slabs from
 *                           HW = 2048 on.  Slab z holds the pixels z * 256 + t + 256 * nslab * j of the sample; lane t adds its
 *                           pixels in index order, a wave of 64 lanes by a halving tree, the four waves in wave order.
 *   pg_seg_loss_value_grad  adds the slabs of every sum in slab order, then
 *                           *value = fl32(scale_ce * S_ce + scale_focal * S_focal + scale_dice * S_dice), the selected members in that
 *                           order in fp64, S_x the sum of the member's per-(n, c) terms: lane i of 48 adds the pairs i, i + 48, ... of
 *                           the (n, c) index n * C + c in index order, then one halving tree;
 *                           g != NULL: g[(n * HW + i) * ld_g + c] for c < C and nothing else -- pad channels of a wider pixel and
 *                           everything outside the view stay untouched -- = the selected members' gradients fl32(scale_ce) * de/dp,
 *                           fl32(scale_focal) * de/dp, k0 y + k1, each rounded to fp32 and added in fp32 in that order.
 *                           g == NULL (evaluation): the value only, with the same bits.
 * No floating-point atomics, no workgroup reads what another wrote in the same launch, no last-arriving workgroup: the launch
 * sequence and the result bits are functions of the arguments alone.  A workgroup of the gradient pass covers pixels of ONE sample and
 * forms that sample's Dice coefficients from the slabs, four channels at a time: there is no table and no limit on N * C.
 * `ws`: pg_seg_loss_workspace_bytes(N, HW, C) bytes, 8-byte aligned, written by the first call and read by the second.
 * PG_EINVAL before any launch, nothing written: a NULL p, y, value or ws; ws misaligned or ws_bytes too small; N, HW or C <= 0; an ld
 * < C (ld_g only where g is given); terms 0 or with an unknown bit; PG_SEG_CE with C < 2; focal_gamma outside
 * 0 .. PG_SEG_FOCAL_GAMMA_MAX; focal_alpha neither in (0, 1) nor PG_SEG_FOCAL_ALPHA_NONE; dice_smooth not finite or <= 0 (the settings
 * are checked whether or not the mask selects their member: pass the defaults 2, PG_SEG_FOCAL_ALPHA_NONE, 1). */
#define PG_SEG_CE 1
#define PG_SEG_FOCAL 2
#define PG_SEG_DICE 4
#define PG_SEG_FOCAL_GAMMA_MAX 8
#define PG_SEG_FOCAL_ALPHA_NONE (-1.0f)
long pg_seg_loss_workspace_bytes(int N, int HW, int C);      /* 0 for N, HW or C <= 0 */
int pg_seg_loss_slabs(int N, int HW);                        /* nslab; 0 for N or HW <= 0 */
int pg_seg_loss_reduce(const float* p, int ld_p, const float* y, int ld_y, int N, int HW, int C, int terms, int focal_gamma,
                       float focal_alpha, void* ws, long ws_bytes, void* stream);
int pg_seg_loss_value_grad(const void* ws, long ws_bytes, const float* p, int ld_p, const float* y, int ld_y, int N, int HW, int C,
                           int terms, int focal_gamma, float focal_alpha, float dice_smooth, double scale_ce, double scale_focal,
                           double scale_dice, float* g, int ld_g, float* value, void* stream);
/* Per-class weights (patchgan_amd's Trainer.class_weights).  Every member's value is linear in the per-(n, c) sums pg_seg_loss_reduce
 * writes, so the weights enter in phase 2 only: pg_seg_loss_reduce and its workspace are used unchanged, and
 * pg_seg_loss_value_grad_w is pg_seg_loss_value_grad (the same kernel body, arguments, address forms and summation orders) with
 * w_c = cw[c], C floats in DEVICE memory, 4-byte aligned, read once per (n, c) pair for the value and once per group of four
 * channels for the gradient:
 *   value     each pair's term times (double)w_c before it enters the pair accumulators: w_c S_ce[n,c], w_c S_focal[n,c],
 *             w_c (1 - D[n,c]); order, scales and the single rounding to float as above.
 *   gradient  fl32(scale_ce * w_c) and fl32(scale_focal * w_c) (one rounding from double each) in place of fl32(scale_ce) /
 *             fl32(scale_focal); k0 = fl32(-2 scale_dice w_c / den), k1 = fl32(scale_dice w_c (2 I + s) / den^2), w_c entering in
 *             fp64.  The element expressions and the order in which a sum's members are added are unchanged.
 * With every w_c == 1 the value and every gradient element are those of pg_seg_loss_value_grad, bit for bit.  A channel with
 * w_c == 0 gets a gradient of +-0 wherever p is not NaN; a NaN in p still comes out as NaN in the value and at that element (under
 * PG_SEG_DICE in the whole (n, c) plane), whatever the weight.
 * The denominators stay B HW, B C HW and B C: 'ce' is F.cross_entropy(logits, labels, weight=w, reduction='sum') / (B HW), NOT torch's
 * reduction='mean', which divides by the sum of the weights of the batch's labelled pixels -- a batch-dependent denominator would need
 * a collective under data parallelism and a window of accumulated micro-batches would no longer be the large batch.
 * The kernel cannot read the weights before it launches: the caller keeps them finite and >= 0 (engine.check_seg_loss does).
 * PG_EINVAL before any launch, nothing written: a NULL cw and everything pg_seg_loss_value_grad refuses. */
int pg_seg_loss_value_grad_w(const void* ws, long ws_bytes, const float* p, int ld_p, const float* y, int ld_y, int N, int HW, int C,
                             int terms, int focal_gamma, float focal_alpha, float dice_smooth, double scale_ce, double scale_focal,
                             double scale_dice, const float* cw, float* g, int ld_g, float* value, void* stream);
/* Per-class pixel counts of a target (what 'balanced' class weights are made of; Trainer.estimate_class_weights): one pass over y
 * alone, y an fp32 NHWC channel slice as above (any C >= 1 -- not limited to pg_seg_confusion_max_c() --, any ld_y >= C, 4-byte
 * aligned, 64-bit offsets).  `counts` holds C + 2 64-bit words on the device and the call ADDS to them (the caller zeroes them):
 *   counts[c]     += pixels with y_c >= 0.5f          (a NaN is not >= 0.5; a soft or multi-hot pixel counts in every such channel)
 *   counts[C]     += pixels with no channel >= 0.5f   (unlabelled)
 *   counts[C + 1] += N * HW
 * Integer sums only (64-bit per-workgroup counters, one integer atomicAdd per non-zero counter): exactly NumPy's counts, in any order.
 * PG_EINVAL before any launch: NULL y or counts; N, HW or C <= 0; ld_y < C. */
int pg_seg_label_count(const float* y, int ld_y, int N, int HW, int C, unsigned long long* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PATCHGAN_HIP_H */
