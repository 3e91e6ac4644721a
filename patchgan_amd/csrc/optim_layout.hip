// optim_layout.hip -- fused Adam over a flat parameter buffer, NCHW <-> NHWC at the API edge, fills/copies.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "patchgan_hip.h"
#include "pg_common.h"

namespace {

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float lr_over_bc1, float beta1,
                                         float beta2, float eps, float sqrt_bc2) {
    // torch single-tensor Adam: exp_avg.lerp_(grad, 1-b1); exp_avg_sq.mul_(b2).addcmul_(g, g, value=1-b2);
    // denom = sqrt(v)/sqrt(bc2) + eps; p.addcdiv_(m, denom, value=-lr/bc1)
    m = m + (g - m) * (1.f - beta1);
    v = v * beta2 + (1.f - beta2) * g * g;
    const float denom = sqrtf(v) / sqrt_bc2 + eps;
    p = p - lr_over_bc1 * (m / denom);
}

// DEV: the two step-dependent scalars (lr / bc1, sqrt(bc2)) come from device memory -- the form a captured hipGraph replays with a
// new Adam step count (pg_adam_step_dev); otherwise they are kernel arguments.  Same arithmetic either way.
// EMA: the exponential moving average of the parameters is updated in the same pass, e += (p_new - e) * (1 - decay), from the value
// just computed for the store (pg_adam_ema_step*: 5 reads + 4 writes per element; Adam and a separate averaging pass take 4 + 3 and
// 2 + 1).  adam_one is the same code in all four instantiations and the library is built without fp contraction: p, m, v do not
// depend on EMA.
template <bool EMA>
__device__ __forceinline__ void ema_one(float& e, float p_new, float c) {
    if constexpr (EMA) e = e + (p_new - e) * c;
}

// CLIP: the gradient is scaled by the coefficient pg_grad_norm left in the status block, g' = g * coef as ONE fp32 product (what
// torch's grad.mul_(coef) stores; g itself is only read), and a block that says "skip" ends the kernel before anything else is loaded:
// p, m, v and ema keep their bits.  The flag is uniform for the grid.  coef == 1: g * 1.f == g, the results of the plain forms.
template <bool CLIP>
__device__ __forceinline__ float clip_one(float g, float coef) {
    if constexpr (CLIP) return g * coef;
    return g;
}

// WD: decoupled weight decay (pg_adamw_step*), p0 = p * decay_mul as ONE fp32 product ahead of the moment updates -- what torch's
// single-tensor AdamW does with param.mul_(1 - lr * weight_decay) --, then adam_one on p0: one multiply, no memory access; m and v do
// not see it.  The caller forms decay_mul in double and rounds once; the DEV form reads it as scal[2].  decay_mul == 1: p * 1.f == p,
// the results of the forms without it.  Behind the CLIP early return: a skipped step does not decay either.
template <bool WD>
__device__ __forceinline__ float decay_one(float p, float decay_mul) {
    if constexpr (WD) return p * decay_mul;
    return p;
}

template <bool DEV, bool EMA, bool CLIP, bool WD>
__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                       long n, float lr_over_bc1, float beta1, float beta2, float eps, float sqrt_bc2, const float* __restrict__ scal,
                       float* __restrict__ ema, float ema_decay, const pg_grad_stat* __restrict__ stat, float decay_mul) {
    float coef = 1.f;
    if constexpr (CLIP) {
        if (stat->apply == 0u) return;
        coef = stat->coef;
    }
    if constexpr (DEV) {
        lr_over_bc1 = scal[0];
        sqrt_bc2 = scal[1];
        if constexpr (WD) decay_mul = scal[2];
    }
    const float c = 1.f - ema_decay;
    const long n4 = n >> 2;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        float4 ee = {0.f, 0.f, 0.f, 0.f};
        if constexpr (EMA) ee = reinterpret_cast<float4*>(ema)[i];
        pp.x = decay_one<WD>(pp.x, decay_mul);
        pp.y = decay_one<WD>(pp.y, decay_mul);
        pp.z = decay_one<WD>(pp.z, decay_mul);
        pp.w = decay_one<WD>(pp.w, decay_mul);
        adam_one(pp.x, clip_one<CLIP>(gg.x, coef), mm.x, vv.x, lr_over_bc1, beta1, beta2, eps, sqrt_bc2);
        adam_one(pp.y, clip_one<CLIP>(gg.y, coef), mm.y, vv.y, lr_over_bc1, beta1, beta2, eps, sqrt_bc2);
        adam_one(pp.z, clip_one<CLIP>(gg.z, coef), mm.z, vv.z, lr_over_bc1, beta1, beta2, eps, sqrt_bc2);
        adam_one(pp.w, clip_one<CLIP>(gg.w, coef), mm.w, vv.w, lr_over_bc1, beta1, beta2, eps, sqrt_bc2);
        ema_one<EMA>(ee.x, pp.x, c);
        ema_one<EMA>(ee.y, pp.y, c);
        ema_one<EMA>(ee.z, pp.z, c);
        ema_one<EMA>(ee.w, pp.w, c);
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
        if constexpr (EMA) reinterpret_cast<float4*>(ema)[i] = ee;
    }
    for (long i = (n4 << 2) + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) {
        float pi = decay_one<WD>(p[i], decay_mul);
        adam_one(pi, clip_one<CLIP>(g[i], coef), m[i], v[i], lr_over_bc1, beta1, beta2, eps, sqrt_bc2);
        p[i] = pi;
        if constexpr (EMA) ema_one<EMA>(ema[i], pi, c);
    }
}

// ---- gradient accumulation (pg_grad_accum) ----------------------------------------------------------------------------------------------
// One streaming pass over the accumulator and the flat gradient, MODE = PG_ACC_*: per element ONE fp32 add and then ONE fp32 multiply
// where the mode has them (the library is built without fp contraction: never an fma), so a float32 replay on the host gives the same
// bits, NaN and inf included.  The operand a mode only reads is const here and never stored.
template <int MODE>
__device__ __forceinline__ float acc_one(float a, float g, float scale) {
    if constexpr (MODE == PG_ACC_BEGIN) return g;
    if constexpr (MODE == PG_ACC_ADD) return a + g;
    if constexpr (MODE == PG_ACC_CLOSE) return (a + g) * scale;
    return a * scale;                                   // PG_ACC_CLOSE_ONLY
}

template <int MODE>
__global__ void k_grad_accum(float* __restrict__ acc, float* __restrict__ g, long n, float scale) {
    constexpr bool READ_A = MODE != PG_ACC_BEGIN, READ_G = MODE != PG_ACC_CLOSE_ONLY;
    constexpr bool TO_ACC = MODE == PG_ACC_BEGIN || MODE == PG_ACC_ADD;
    const long n4 = n >> 2;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 aa = {0.f, 0.f, 0.f, 0.f}, gg = {0.f, 0.f, 0.f, 0.f}, r;
        if constexpr (READ_A) aa = reinterpret_cast<const float4*>(acc)[i];
        if constexpr (READ_G) gg = reinterpret_cast<const float4*>(g)[i];
        r.x = acc_one<MODE>(aa.x, gg.x, scale);
        r.y = acc_one<MODE>(aa.y, gg.y, scale);
        r.z = acc_one<MODE>(aa.z, gg.z, scale);
        r.w = acc_one<MODE>(aa.w, gg.w, scale);
        reinterpret_cast<float4*>(TO_ACC ? acc : g)[i] = r;
    }
    for (long i = (n4 << 2) + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) {
        const float a = READ_A ? acc[i] : 0.f, x = READ_G ? g[i] : 0.f;
        (TO_ACC ? acc : g)[i] = acc_one<MODE>(a, x, scale);
    }
}

// ---- global gradient norm (pg_grad_norm) ------------------------------------------------------------------------------------------------
// The sum of squares of n floats in fp64, in an order that depends on n alone.  k_sumsq_part: workgroup b of B (norm_blocks(n)) takes the
// 16-byte groups b * 256 + lane + k * B * 256, k = 0, 1, ... -- one fp64 accumulator per component, so four independent chains per lane
// --, lane t < n % 4 of workgroup 0 adds tail element (n & ~3) + t, the lane's sum is (x + y) + (z + w) (+ tail); the 64 lanes of a wave
// are folded by halving distances 32 .. 1, the four wave sums are added in order, ws[b] gets the result.  k_sumsq_finish: one workgroup,
// lane t sums ws[t], ws[t + 256], ... in order, the same fold, and lane 0 writes the status block.  No atomics, no arrival order.
constexpr int NORM_THREADS = 256;
constexpr int NORM_MAX_BLOCKS = 2048;          // 8 workgroups per CU; 16 KiB of partials

__device__ __forceinline__ double norm_block_sum(double a) {
    __shared__ double part[NORM_THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];          // (read by every lane; lane 0's value is the one used)
}

__global__ __launch_bounds__(NORM_THREADS) void k_sumsq_part(const float* __restrict__ g, long n, double* __restrict__ ws) {
    const long n4 = n >> 2;
    const long stride = (long)gridDim.x * NORM_THREADS;
    double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
#pragma unroll 4
    for (long i = blockIdx.x * (long)NORM_THREADS + threadIdx.x; i < n4; i += stride) {
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        const double x = gg.x, y = gg.y, z = gg.z, w = gg.w;
        ax += x * x;
        ay += y * y;
        az += z * z;
        aw += w * w;
    }
    double a = (ax + ay) + (az + aw);
    if (blockIdx.x == 0 && (long)threadIdx.x < (n & 3)) {
        const double t = g[(n4 << 2) + threadIdx.x];
        a += t * t;
    }
    a = norm_block_sum(a);
    if (threadIdx.x == 0) ws[blockIdx.x] = a;
}

__global__ __launch_bounds__(NORM_THREADS) void k_sumsq_finish(const double* __restrict__ ws, int nblocks, double max_norm,
                                                               pg_grad_stat* __restrict__ stat) {
    double a = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += NORM_THREADS) a += ws[i];
    a = norm_block_sum(a);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(a);
    const bool finite = isfinite(a);           // (a NaN or +-inf anywhere in g makes the sum NaN or +inf: 1e38^2 * 2^40 is far from fp64's end)
    float coef = 0.f;
    if (finite) {
        const double c = max_norm / (norm + 1e-6);          // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1)
        coef = (float)(c < 1.0 ? c : 1.0);
    }
    stat->norm = (float)norm;
    stat->coef = coef;
    stat->apply = finite ? 1u : 0u;
    stat->sumsq = a;
    stat->steps += 1ull;
    if (finite) {
        if (coef < 1.f) stat->clipped += 1ull;
        if (norm > stat->max_norm) stat->max_norm = norm;
        stat->sum_norm += norm;
    } else {
        stat->skipped += 1ull;
    }
}

int norm_blocks(long n) {
    long b = ((n >> 2) + NORM_THREADS - 1) / NORM_THREADS;
    if (b > NORM_MAX_BLOCKS) b = NORM_MAX_BLOCKS;
    if (b < 1) b = 1;
    return (int)b;
}

// dst NHWC (pixel stride ld_dst) <- src NCHW; one thread per PIXEL: the C plane reads of a wave are C coalesced rows (one thread per
// (pixel, channel) read a different cache line per lane and paid three 64-bit divisions per element), the C floats of a pixel are
// written together
__global__ void k_nchw_to_nhwc(const float* __restrict__ src, float* __restrict__ dst, int ld_dst, int N, int C,
                               long HW) {
    const long npix = (long)N * HW;
    if (npix < 0x7fffffffL && C <= 8) {
        const unsigned np = (unsigned)npix, hwu = (unsigned)HW, stride = gridDim.x * blockDim.x;
        for (unsigned pix = blockIdx.x * blockDim.x + threadIdx.x; pix < np; pix += stride) {
            const unsigned n = pix / hwu, hw = pix - n * hwu;
            const float* sp = src + (size_t)n * C * HW + hw;
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = (c < C) ? sp[(size_t)c * HW] : 0.f;
            float* dp = dst + (size_t)pix * ld_dst;
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c < C) dp[c] = v[c];
        }
        return;
    }
    const long total = npix * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long pix = i / C;
        const long n = pix / HW, hw = pix - n * HW;
        dst[pix * ld_dst + c] = src[(n * C + c) * HW + hw];
    }
}

// The discriminator's input buffer din[2N][HW][ld] in ONE pass (trainer.py:65,96,98: cat((x, y), 1) and cat((x, G(x)), 1)): sample n of
// the real half = x[n] | y[n], of the fake half = x[n] | 0 (the generator's head writes its output there later in the step); channels
// Cx + Cy .. ld - 1 (the pad of an 8-float pixel) = 0.  One thread per pixel: Cx + Cy coalesced plane reads, then the two pixels as
// 16-byte stores where ld == 8 (the three separate pg_nchw_to_nhwc calls wrote 3 + 3 + 4 scalars per pixel at a 28-byte stride and ran
// at 0.6 TB/s on 512 x 512 inputs).
template <bool V8>
__global__ __launch_bounds__(256) void k_din_fill(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ real,
                                                  float* __restrict__ fake, int ld, int N, int Cx, int Cy, unsigned HW) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const unsigned np = (unsigned)N * HW, stride = gridDim.x * blockDim.x;
    for (unsigned pix = blockIdx.x * blockDim.x + threadIdx.x; pix < np; pix += stride) {
        const unsigned n = pix / HW, hw = pix - n * HW;
        const float* xp = x + (size_t)n * Cx * HW + hw;
        const float* yp = y + (size_t)n * Cy * HW + hw;
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = c < Cx ? xp[(size_t)c * HW] : (c < Cx + Cy ? yp[(size_t)(c - Cx) * HW] : 0.f);
        float* rp = real + (size_t)pix * ld;
        float* fp = fake + (size_t)pix * ld;
        if (V8) {
            *reinterpret_cast<f32x4*>(rp) = f32x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(rp + 4) = f32x4{v[4], v[5], v[6], v[7]};
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = c < Cx ? v[c] : 0.f;
            *reinterpret_cast<f32x4*>(fp) = f32x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(fp + 4) = f32x4{v[4], v[5], v[6], v[7]};
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c < ld) {
                    rp[c] = v[c];
                    fp[c] = c < Cx ? v[c] : 0.f;
                }
        }
    }
}

// dst NCHW <- src NHWC; one thread per NCHW element (pixel fastest)
__global__ void k_nhwc_to_nchw(const float* __restrict__ src, int ld_src, float* __restrict__ dst, int N, int C,
                               long HW) {
    const long total = (long)N * HW * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long hw = i % HW;
        const long nc = i / HW;
        const int c = (int)(nc % C);
        const long n = nc / C;
        dst[i] = src[(n * HW + hw) * ld_src + c];
    }
}

// decoded image bytes [npix][C] (HWC, what a JPEG decoder hands over) -> float NHWC slice: value / 255.f, the reference's
// `read_image(...) / 255.` (io.py:42) computed on the device
__global__ void k_u8_to_f32(const uint8_t* __restrict__ src, float* __restrict__ dst, int ld_dst, long npix, int C, float div) {
    const long total = npix * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long pix = i / C;
        dst[pix * ld_dst + c] = (float)src[i] / div;
    }
}

// label map bytes [npix] -> one-hot float NHWC slice of nl channels: dst[pix][i] = ((uint8)(src + add) == labels[i])
// (io.py:43,53-56: `read_image(mask, GRAY) + 1` is uint8 arithmetic -- 255 wraps to 0 -- then `mask[i, labels == label] = 1`)
struct LabelSet {
    int v[PG_MAX_LABELS];
};
__global__ void k_labels_onehot(const uint8_t* __restrict__ src, float* __restrict__ dst, int ld_dst, long npix, LabelSet ls,
                                int nl, int add) {
    for (long pix = blockIdx.x * (long)blockDim.x + threadIdx.x; pix < npix; pix += (long)gridDim.x * blockDim.x) {
        const int v = (uint8_t)(src[pix] + add);
        for (int i = 0; i < nl; ++i) dst[pix * ld_dst + i] = (v == ls.v[i]) ? 1.f : 0.f;
    }
}

__global__ void k_copy_channels(const float* __restrict__ src, int ld_src, float* __restrict__ dst, int ld_dst,
                                long npix, int C) {
    const long total = npix * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long pix = i / C;
        dst[pix * ld_dst + c] = src[pix * ld_src + c];
    }
}

__global__ void k_fill(float* __restrict__ dst, long n, float value) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = value;
}

// fp32 NHWC channel slice (C <= 8 channels, pixel stride ld_src) -> bf16 8-channel pixels: one 16-byte store per pixel, pads zero
template <bool V8>      // V8: 8-float source pixels, 16-byte aligned (two 16-byte loads per pixel instead of C scalar ones at a ragged stride)
__global__ void k_pad8_bf16(const float* __restrict__ src, int ld_src, unsigned* __restrict__ dst, long npix, int C) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < npix; i += (long)gridDim.x * blockDim.x) {
        float v[8];
        if (V8) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(src + i * 8), b = *reinterpret_cast<const f32x4*>(src + i * 8 + 4);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[c] = c < C ? a[c] : 0.f;
                v[4 + c] = 4 + c < C ? b[c] : 0.f;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = (c < C) ? src[i * ld_src + c] : 0.f;
        }
        u32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bf16x2 h;
            h[0] = (__bf16)v[2 * k];
            h[1] = (__bf16)v[2 * k + 1];
            o[k] = __builtin_bit_cast(unsigned, h);
        }
        *reinterpret_cast<u32x4*>(dst + 4 * i) = o;
    }
}

int blocks_for(long total) {
    long b = (total + 255) / 256;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (int)b;
}

// (a NaN fails every comparison below)
bool adamw_args_ok(float beta1, float beta2, float decay_mul, const float* ema, float ema_decay) {
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return false;
    if (!(decay_mul > 0.f && decay_mul <= 1.f)) return false;
    return !ema || (ema_decay >= 0.f && ema_decay < 1.f);
}

// (a null pointer counts as aligned: the entry point has decided already whether it may be null)
template <class... P>
bool aligned16(const P*... ptrs) {
    return (((uintptr_t)ptrs | ...) & 15) == 0;
}

// The one launch site of k_adam, behind the validation of all eight pg_adam* entry points.  dev and wd are the entry point's (pg_adamw_*
// is WD also with a multiplier of 1), EMA and CLIP follow the pointers.  Every launch passes every argument; the fillers of the forms
// without a feature -- scalars null, lr_over_bc1 = sqrt_bc2 = 0 (dev), decay_mul = 1 -- are the callers', ema_decay = 0 without an
// average is set here.  (The forms stand in the order the code object has always held them -- template kernels are emitted in the
// order the file first names them --, so the device assembly of two revisions compares file against file.)
int adam_launch(bool dev, bool wd, float* p, const float* g, float* m, float* v, float* ema, long n, float lr_over_bc1, float beta1, float beta2,
                float eps, float sqrt_bc2, const float* scalars, float decay_mul, float ema_decay, const pg_grad_stat* stat, void* stream) {
    auto* kernel = k_adam<false, false, false, false>;
    switch (dev << 3 | (ema != nullptr) << 2 | (stat != nullptr) << 1 | (int)wd) {          // DEV EMA CLIP WD
    case 0b1000: kernel = k_adam<true, false, false, false>; break;
    case 0b0100: kernel = k_adam<false, true, false, false>; break;
    case 0b1100: kernel = k_adam<true, true, false, false>; break;
    case 0b0110: kernel = k_adam<false, true, true, false>; break;
    case 0b0010: kernel = k_adam<false, false, true, false>; break;
    case 0b1110: kernel = k_adam<true, true, true, false>; break;
    case 0b1010: kernel = k_adam<true, false, true, false>; break;
    case 0b0111: kernel = k_adam<false, true, true, true>; break;
    case 0b0101: kernel = k_adam<false, true, false, true>; break;
    case 0b0011: kernel = k_adam<false, false, true, true>; break;
    case 0b0001: kernel = k_adam<false, false, false, true>; break;
    case 0b1111: kernel = k_adam<true, true, true, true>; break;
    case 0b1101: kernel = k_adam<true, true, false, true>; break;
    case 0b1011: kernel = k_adam<true, false, true, true>; break;
    case 0b1001: kernel = k_adam<true, false, false, true>; break;
    }
    hipLaunchKernelGGL(kernel, dim3(blocks_for(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr_over_bc1, beta1, beta2, eps,
                       sqrt_bc2, scalars, ema, ema ? ema_decay : 0.f, stat, decay_mul);
    return pg_launch_status();
}

}  // namespace

extern "C" {

int pg_version(void) { return 2; }

int pg_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                 float bc1, float sqrt_bc2, void* stream) {
    if (!p || !g || !m || !v || n <= 0 || bc1 <= 0.f || sqrt_bc2 <= 0.f) return PG_EINVAL;
    if (!aligned16(p, g, m, v)) return PG_EINVAL;
    return adam_launch(false, false, p, g, m, v, nullptr, n, lr / bc1, beta1, beta2, eps, sqrt_bc2, nullptr, 1.f, 0.f, nullptr, stream);
}

int pg_adam_step_dev(float* p, const float* g, float* m, float* v, long n, float beta1, float beta2, float eps, const float* scalars,
                     void* stream) {
    if (!p || !g || !m || !v || !scalars || n <= 0) return PG_EINVAL;
    if (!aligned16(p, g, m, v)) return PG_EINVAL;
    return adam_launch(true, false, p, g, m, v, nullptr, n, 0.f, beta1, beta2, eps, 0.f, scalars, 1.f, 0.f, nullptr, stream);
}

int pg_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float beta1, float beta2, float eps,
                     float bc1, float sqrt_bc2, float ema_decay, void* stream) {
    if (!p || !g || !m || !v || !ema || n <= 0 || bc1 <= 0.f || sqrt_bc2 <= 0.f) return PG_EINVAL;
    if (!(ema_decay >= 0.f && ema_decay < 1.f)) return PG_EINVAL;      // (a NaN fails both comparisons)
    if (!aligned16(p, g, m, v, ema)) return PG_EINVAL;
    return adam_launch(false, false, p, g, m, v, ema, n, lr / bc1, beta1, beta2, eps, sqrt_bc2, nullptr, 1.f, ema_decay, nullptr, stream);
}

int pg_adam_ema_step_dev(float* p, const float* g, float* m, float* v, float* ema, long n, float beta1, float beta2, float eps,
                         const float* scalars, float ema_decay, void* stream) {
    if (!p || !g || !m || !v || !ema || !scalars || n <= 0) return PG_EINVAL;
    if (!(ema_decay >= 0.f && ema_decay < 1.f)) return PG_EINVAL;
    if (!aligned16(p, g, m, v, ema)) return PG_EINVAL;
    return adam_launch(true, false, p, g, m, v, ema, n, 0.f, beta1, beta2, eps, 0.f, scalars, 1.f, ema_decay, nullptr, stream);
}

long pg_grad_norm_workspace_bytes(long n) { return n > 0 ? (long)norm_blocks(n) * (long)sizeof(double) : 0; }

int pg_grad_norm(const float* g, long n, double max_norm, void* ws, long ws_bytes, pg_grad_stat* stat, void* stream) {
    if (!g || !ws || !stat || n <= 0 || !(max_norm > 0.0)) return PG_EINVAL;          // (a NaN fails the comparison)
    if ((((uintptr_t)g | (uintptr_t)stat) & 15) || ((uintptr_t)ws & 7)) return PG_EINVAL;
    const int nb = norm_blocks(n);
    if (ws_bytes < (long)nb * (long)sizeof(double)) return PG_EINVAL;
    hipLaunchKernelGGL(k_sumsq_part, dim3(nb), dim3(NORM_THREADS), 0, (hipStream_t)stream, g, n, (double*)ws);
    hipLaunchKernelGGL(k_sumsq_finish, dim3(1), dim3(NORM_THREADS), 0, (hipStream_t)stream, (const double*)ws, nb, max_norm, stat);
    return pg_launch_status();
}

int pg_adam_clip_step(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float beta1, float beta2, float eps,
                      float bc1, float sqrt_bc2, float ema_decay, const pg_grad_stat* stat, void* stream) {
    if (!p || !g || !m || !v || !stat || n <= 0 || bc1 <= 0.f || sqrt_bc2 <= 0.f) return PG_EINVAL;
    if (ema && !(ema_decay >= 0.f && ema_decay < 1.f)) return PG_EINVAL;
    if (!aligned16(p, g, m, v, ema, stat)) return PG_EINVAL;
    return adam_launch(false, false, p, g, m, v, ema, n, lr / bc1, beta1, beta2, eps, sqrt_bc2, nullptr, 1.f, ema_decay, stat, stream);
}

int pg_adam_clip_step_dev(float* p, const float* g, float* m, float* v, float* ema, long n, float beta1, float beta2, float eps,
                          const float* scalars, float ema_decay, const pg_grad_stat* stat, void* stream) {
    if (!p || !g || !m || !v || !scalars || !stat || n <= 0) return PG_EINVAL;
    if (ema && !(ema_decay >= 0.f && ema_decay < 1.f)) return PG_EINVAL;
    if (!aligned16(p, g, m, v, ema, stat)) return PG_EINVAL;
    return adam_launch(true, false, p, g, m, v, ema, n, 0.f, beta1, beta2, eps, 0.f, scalars, 1.f, ema_decay, stat, stream);
}

int pg_adamw_step(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float beta1, float beta2, float eps,
                  float bc1, float sqrt_bc2, float decay_mul, float ema_decay, const pg_grad_stat* stat, void* stream) {
    if (!p || !g || !m || !v || n <= 0 || !(bc1 > 0.f) || !(sqrt_bc2 > 0.f)) return PG_EINVAL;
    if (!adamw_args_ok(beta1, beta2, decay_mul, ema, ema_decay)) return PG_EINVAL;
    if (!aligned16(p, g, m, v, ema, stat)) return PG_EINVAL;
    return adam_launch(false, true, p, g, m, v, ema, n, lr / bc1, beta1, beta2, eps, sqrt_bc2, nullptr, decay_mul, ema_decay, stat, stream);
}

int pg_adamw_step_dev(float* p, const float* g, float* m, float* v, float* ema, long n, float beta1, float beta2, float eps,
                      const float* scalars, float ema_decay, const pg_grad_stat* stat, void* stream) {
    if (!p || !g || !m || !v || !scalars || n <= 0) return PG_EINVAL;
    if (!adamw_args_ok(beta1, beta2, 1.f, ema, ema_decay)) return PG_EINVAL;      // (decay_mul lives on the device: scalars[2])
    if (!aligned16(p, g, m, v, ema, stat)) return PG_EINVAL;
    return adam_launch(true, true, p, g, m, v, ema, n, 0.f, beta1, beta2, eps, 0.f, scalars, 1.f, ema_decay, stat, stream);
}

int pg_grad_accum(float* acc, float* g, long n, int mode, float scale, void* stream) {
    if (!acc || !g || n <= 0) return PG_EINVAL;
    if (((uintptr_t)acc | (uintptr_t)g) & 15) return PG_EINVAL;
    const uintptr_t a0 = (uintptr_t)acc, g0 = (uintptr_t)g, bytes = (uintptr_t)n * sizeof(float);
    if (a0 < g0 + bytes && g0 < a0 + bytes) return PG_EINVAL;
    const bool closing = mode == PG_ACC_CLOSE || mode == PG_ACC_CLOSE_ONLY;
    if (!closing && mode != PG_ACC_BEGIN && mode != PG_ACC_ADD) return PG_EINVAL;
    if (closing && !(scale > 0.f && scale <= 1.f)) return PG_EINVAL;      // (a NaN fails both comparisons; inf the second)
    const dim3 grid(blocks_for(n / 4 + 1)), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (mode) {
    case PG_ACC_BEGIN: hipLaunchKernelGGL(k_grad_accum<PG_ACC_BEGIN>, grid, block, 0, s, acc, g, n, scale); break;
    case PG_ACC_ADD: hipLaunchKernelGGL(k_grad_accum<PG_ACC_ADD>, grid, block, 0, s, acc, g, n, scale); break;
    case PG_ACC_CLOSE: hipLaunchKernelGGL(k_grad_accum<PG_ACC_CLOSE>, grid, block, 0, s, acc, g, n, scale); break;
    default: hipLaunchKernelGGL(k_grad_accum<PG_ACC_CLOSE_ONLY>, grid, block, 0, s, acc, g, n, scale); break;
    }
    return pg_launch_status();
}

int pg_nchw_to_nhwc(const float* src, float* dst, int ld_dst, int N, int C, int H, int W, void* stream) {
    if (!src || !dst || N <= 0 || C <= 0 || H <= 0 || W <= 0 || ld_dst < C) return PG_EINVAL;
    const long HW = (long)H * W;
    hipLaunchKernelGGL(k_nchw_to_nhwc, dim3(blocks_for(C <= 8 ? (long)N * HW : (long)N * HW * C)), dim3(256), 0, (hipStream_t)stream, src, dst,
                       ld_dst, N, C, HW);
    return pg_launch_status();
}

int pg_pad8_bf16(const float* src, int ld_src, void* dst, long npix, int C, void* stream) {
    if (!src || !dst || npix <= 0 || C <= 0 || C > 8 || ld_src < C || ((uintptr_t)dst & 15)) return PG_EINVAL;
    if (ld_src == 8 && ((uintptr_t)src & 15) == 0)
        hipLaunchKernelGGL(k_pad8_bf16<true>, dim3(blocks_for(npix)), dim3(256), 0, (hipStream_t)stream, src, ld_src, (unsigned*)dst, npix, C);
    else
        hipLaunchKernelGGL(k_pad8_bf16<false>, dim3(blocks_for(npix)), dim3(256), 0, (hipStream_t)stream, src, ld_src, (unsigned*)dst, npix, C);
    return pg_launch_status();
}

int pg_din_fill(const float* x, const float* y, float* real, float* fake, int ld, int N, int Cx, int Cy, int H, int W, void* stream) {
    if (!x || !y || !real || !fake || N <= 0 || Cx <= 0 || Cy <= 0 || Cx + Cy > 8 || ld < Cx + Cy || ld > 8 || H <= 0 || W <= 0) return PG_EINVAL;
    const long HW = (long)H * W;
    if ((long)N * HW >= 0x7fffffffL) return PG_EINVAL;
    const bool v8 = ld == 8 && (((uintptr_t)real | (uintptr_t)fake) & 15) == 0;
    if (v8)
        hipLaunchKernelGGL(k_din_fill<true>, dim3(blocks_for((long)N * HW)), dim3(256), 0, (hipStream_t)stream, x, y, real, fake, ld, N, Cx, Cy,
                           (unsigned)HW);
    else
        hipLaunchKernelGGL(k_din_fill<false>, dim3(blocks_for((long)N * HW)), dim3(256), 0, (hipStream_t)stream, x, y, real, fake, ld, N, Cx, Cy,
                           (unsigned)HW);
    return pg_launch_status();
}

int pg_nhwc_to_nchw(const float* src, int ld_src, float* dst, int N, int C, int H, int W, void* stream) {
    if (!src || !dst || N <= 0 || C <= 0 || H <= 0 || W <= 0 || ld_src < C) return PG_EINVAL;
    const long HW = (long)H * W;
    hipLaunchKernelGGL(k_nhwc_to_nchw, dim3(blocks_for((long)N * HW * C)), dim3(256), 0, (hipStream_t)stream, src, ld_src,
                       dst, N, C, HW);
    return pg_launch_status();
}

int pg_copy_channels(const float* src, int ld_src, float* dst, int ld_dst, long npix, int C, void* stream) {
    if (!src || !dst || npix <= 0 || C <= 0 || ld_src < C || ld_dst < C) return PG_EINVAL;
    hipLaunchKernelGGL(k_copy_channels, dim3(blocks_for(npix * C)), dim3(256), 0, (hipStream_t)stream, src, ld_src, dst,
                       ld_dst, npix, C);
    return pg_launch_status();
}

int pg_u8_to_f32(const unsigned char* src, float* dst, int ld_dst, long npix, int C, float div, void* stream) {
    if (!src || !dst || npix <= 0 || C <= 0 || ld_dst < C || div == 0.f) return PG_EINVAL;
    hipLaunchKernelGGL(k_u8_to_f32, dim3(blocks_for(npix * C)), dim3(256), 0, (hipStream_t)stream, src, dst, ld_dst, npix, C,
                       div);
    return pg_launch_status();
}

int pg_labels_to_onehot(const unsigned char* src, float* dst, int ld_dst, long npix, const int* labels, int nlabels, int add,
                        void* stream) {
    if (!src || !dst || !labels || npix <= 0 || nlabels <= 0 || nlabels > PG_MAX_LABELS || ld_dst < nlabels) return PG_EINVAL;
    LabelSet ls;
    for (int i = 0; i < PG_MAX_LABELS; ++i) ls.v[i] = i < nlabels ? labels[i] : -1;
    hipLaunchKernelGGL(k_labels_onehot, dim3(blocks_for(npix)), dim3(256), 0, (hipStream_t)stream, src, dst, ld_dst, npix, ls,
                       nlabels, add);
    return pg_launch_status();
}

int pg_fill(float* dst, long n, float value, void* stream) {
    if (!dst || n <= 0) return PG_EINVAL;
    hipLaunchKernelGGL(k_fill, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, dst, n, value);
    return pg_launch_status();
}

}  // extern "C"
