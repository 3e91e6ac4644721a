// segloss.hip -- segmentation objectives on the generator's output (categorical cross-entropy, focal loss, soft Dice and their sums):
// value and gradient seed in two launches, placed where pg_loss_reduce_parts / pg_loss_value_grad sit in the step.  patchgan_hip.h
// states the expressions.  Element arithmetic fp32, sums and Dice coefficients fp64, every summation order a function of (N, HW, C).
//
//   pg_seg_loss_reduce      per (sample, slab, channel) the sums over the slab's pixels of {p y, p, y, e_ce, e_focal}
//   pg_seg_loss_value_grad  adds the slabs in slab order; workgroup 0 writes the value, the others the gradient of one sample's pixels
//   pg_seg_loss_value_grad_w  the same kernel body with a per-class weight w_c on every (sample, channel) term (template flag W)
//   pg_seg_label_count      per-class pixel counts of the target (what 'balanced' class weights are made of): integers only
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include "patchgan_hip.h"
#include "pg_common.h"

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_SUMS = 5;                 // I = sum p y, P = sum p, Y = sum y, sum e_ce, sum e_focal
constexpr int SEG_SLAB_PIXELS = 1024;       // a sample has HW / 1024 slabs (at least 1) ...
constexpr int SEG_SLAB_BLOCKS = 1024;       // ... at most 1024 / N of them (at least 1) ...
constexpr int SEG_SLAB_MAX = 128;           // ... and at most 128
constexpr int SEG_GRAD_PIXELS = 2048;       // phase 2: a workgroup takes ~2048 pixels of one sample, at most ~2048 workgroups in all
constexpr int SEG_GRAD_BLOCKS = 2048;
constexpr int SEG_VALUE_TILE = 48;          // phase 2, workgroup 0: (sample, channel) pairs per round (48 * 5 sums <= 256 lanes)

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

inline int seg_nslab(int N, int HW) {
    int ns = HW / SEG_SLAB_PIXELS;
    const int cap = SEG_SLAB_BLOCKS / N;
    if (ns > cap) ns = cap;
    if (ns > SEG_SLAB_MAX) ns = SEG_SLAB_MAX;
    return ns < 1 ? 1 : ns;
}
inline int seg_nchunk(int N, int HW) {
    int nc = (HW + SEG_GRAD_PIXELS - 1) / SEG_GRAD_PIXELS;
    const int cap = SEG_GRAD_BLOCKS / N;
    if (nc > cap) nc = cap;
    return nc < 1 ? 1 : nc;
}
inline long seg_ws_doubles(int N, int HW, int C) { return (long)N * seg_nslab(N, HW) * C * SEG_SUMS; }

struct SegArgs {
    const float* p;
    const float* y;
    float* g;
    float* value;
    double* ws;
    const float* cw;                        // per-class weights, C floats (the weighted entry point only)
    double scale_ce, scale_focal, scale_dice;
    long ld_p, ld_y, ld_g;
    int N, HW, C, terms, gamma, nslab, nchunk;
    float a1, a0, smooth;
};

// four consecutive floats behind a pointer that is 4-byte aligned only: one 16-byte access where the address allows it, two 8-byte ones,
// or 4 + 8 + 4 (an address that is 4 mod 8: the mask slice that starts 3 floats into an 8-float pixel)
__device__ __forceinline__ f4 seg_load4(const float* q) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(q);
    if ((a & 15) == 0) return *reinterpret_cast<const f4*>(q);
    if ((a & 7) == 0) {
        const f2 lo = *reinterpret_cast<const f2*>(q), hi = *reinterpret_cast<const f2*>(q + 2);
        return f4{lo[0], lo[1], hi[0], hi[1]};
    }
    const float x0 = q[0];
    const f2 mid = *reinterpret_cast<const f2*>(q + 1);
    return f4{x0, mid[0], mid[1], q[3]};
}
__device__ __forceinline__ void seg_store4(float* q, f4 v) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(q);
    if ((a & 15) == 0) {
        *reinterpret_cast<f4*>(q) = v;
    } else if ((a & 7) == 0) {
        *reinterpret_cast<f2*>(q) = f2{v[0], v[1]};
        *reinterpret_cast<f2*>(q + 2) = f2{v[2], v[3]};
    } else {
        q[0] = v[0];
        *reinterpret_cast<f2*>(q + 1) = f2{v[1], v[2]};
        q[3] = v[3];
    }
}
// channels [0, nc) of a pixel's group of four; the others are not read (0)
__device__ __forceinline__ f4 seg_load(const float* q, int nc) {
    if (nc == 4) return seg_load4(q);
    f4 v = {0.f, 0.f, 0.f, 0.f};
    v[0] = q[0];
    if (nc > 1) v[1] = q[1];
    if (nc > 2) v[2] = q[2];
    return v;
}

// clamps that keep a NaN (fmaxf would return the bound): a NaN in p comes out as a NaN in every value and gradient it enters
__device__ __forceinline__ float seg_max(float x, float lo) { return x != x ? x : fmaxf(x, lo); }
__device__ __forceinline__ float seg_logp(float p) { return seg_max(logf(p), -100.f); }          // as pg_loss_reduce's bce_elem
__device__ __forceinline__ float seg_logq(float p) { return seg_max(log1pf(-p), -100.f); }

// x^k by repeated multiplication from the left: x^0 = 1, x^k = x^(k-1) * x.  lo = x^(k-1) (1 for k <= 1), hi = x^k.
__device__ __forceinline__ void seg_pow(float x, int k, float& lo, float& hi) {
    lo = 1.f;
    for (int i = 1; i < k; ++i) lo *= x;
    hi = k > 0 ? lo * x : 1.f;
}

__device__ __forceinline__ float seg_ce_elem(float y, float lp) { return -(y * lp); }
__device__ __forceinline__ float seg_ce_grad(float p, float y) { return -y / seg_max(p, 1e-12f); }
__device__ __forceinline__ float seg_focal_elem(float p, float y, float lp, float lq, int gamma, float a1, float a0) {
    float plo, phi, qlo, qhi;
    seg_pow(p, gamma, plo, phi);
    seg_pow(1.f - p, gamma, qlo, qhi);
    return -(((a1 * y) * qhi) * lp + ((a0 * (1.f - y)) * phi) * lq);
}
__device__ __forceinline__ float seg_focal_grad(float p, float y, float lp, float lq, int gamma, float a1, float a0) {
    const float q = 1.f - p, gf = (float)gamma;
    float plo, phi, qlo, qhi;
    seg_pow(p, gamma, plo, phi);
    seg_pow(q, gamma, qlo, qhi);
    float A = qhi / seg_max(p, 1e-12f);
    float B = phi / seg_max(q, 1e-12f);
    if (gamma > 0) {          // (never evaluated as 0 * x)
        A = A - (gf * qlo) * lp;
        B = (gf * plo) * lq - B;
    } else {
        B = -B;
    }
    return -((a1 * y) * A + (a0 * (1.f - y)) * B);
}

// a wave's sum by a halving tree (lane l += lane l + 32, 16, ... 1): the result is lane 0's
__device__ __forceinline__ double seg_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// the slabs of one sum in slab order, 16 loads in flight at a time
__device__ __forceinline__ double seg_slab_sum(const double* __restrict__ q, long stride, int nslab) {
    double v = 0.0;
    int z = 0;
    for (; z + 16 <= nslab; z += 16) {
        double t[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) t[k] = q[(long)(z + k) * stride];
#pragma unroll
        for (int k = 0; k < 16; ++k) v += t[k];
    }
    for (; z < nslab; ++z) v += q[(long)z * stride];
    return v;
}

// Phase 1.  Workgroup b = n * nslab + z takes the pixels z * 256 + tid, + 256 * nslab, ... of sample n, four channels at a time; a lane
// adds its pixels in index order, a wave by seg_wave_sum, the four waves in wave order.  ws[((n * nslab + z) * C + c) * 5 + k]; sums
// the term mask does not select are written as 0.
__global__ __launch_bounds__(SEG_THREADS) void k_seg_loss_reduce(SegArgs a) {
    __shared__ double red[SEG_THREADS / 64][4 * SEG_SUMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long n = blockIdx.x / a.nslab;
    const int z = blockIdx.x % a.nslab;
    const bool ce = a.terms & PG_SEG_CE, focal = a.terms & PG_SEG_FOCAL, dice = a.terms & PG_SEG_DICE;
    const bool need_lp = ce || focal;
    for (int c0 = 0; c0 < a.C; c0 += 4) {
        const int nc = a.C - c0 < 4 ? a.C - c0 : 4;
        double s[4][SEG_SUMS];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k = 0; k < SEG_SUMS; ++k) s[c][k] = 0.0;
        for (long i = (long)z * SEG_THREADS + tid; i < a.HW; i += (long)SEG_THREADS * a.nslab) {
            const long pix = n * a.HW + i;
            const f4 pv = seg_load(a.p + pix * a.ld_p + c0, nc), yv = seg_load(a.y + pix * a.ld_y + c0, nc);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c < nc) {
                    const float p = pv[c], y = yv[c];
                    if (dice) {
                        s[c][0] += (double)(p * y);
                        s[c][1] += (double)p;
                        s[c][2] += (double)y;
                    }
                    if (need_lp) {
                        const float lp = seg_logp(p);
                        if (ce) s[c][3] += (double)seg_ce_elem(y, lp);
                        if (focal) s[c][4] += (double)seg_focal_elem(p, y, lp, seg_logq(p), a.gamma, a.a1, a.a0);
                    }
                }
            }
        }
        __syncthreads();          // (the previous group's read of red is over)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k = 0; k < SEG_SUMS; ++k) {
                const bool on = k < 3 ? dice : (k == 3 ? ce : focal);
                double v = 0.0;
                if (on) v = seg_wave_sum(s[c][k]);
                if (lane == 0) red[wave][c * SEG_SUMS + k] = v;
            }
        __syncthreads();
        if (tid < nc * SEG_SUMS) {
            double v = red[0][tid];
            for (int w = 1; w < SEG_THREADS / 64; ++w) v += red[w][tid];
            a.ws[((long)blockIdx.x * a.C + c0) * SEG_SUMS + tid] = v;
        }
    }
}

// Phase 2.  Workgroup 0: the value.  Workgroup 1 + n * nchunk + j: the gradient of the pixels j * 256 + tid, + 256 * nchunk, ... of
// sample n, four channels at a time, the Dice coefficients of those channels formed from the slabs in front of each group.
// W: every (n, c) term of the value, the two fp32 scales and the Dice coefficients of channel c carry w_c = cw[c], entering in fp64;
// the weights are read once per pair (value) and once per channel group (gradient), never per pixel.  !W is the code without them.
template <bool W>
__global__ __launch_bounds__(SEG_THREADS) void k_seg_loss_value_grad(SegArgs a) {
    __shared__ double sums[SEG_VALUE_TILE * SEG_SUMS];
    __shared__ float coef[8];
    const int tid = threadIdx.x;
    const bool ce = a.terms & PG_SEG_CE, focal = a.terms & PG_SEG_FOCAL, dice = a.terms & PG_SEG_DICE;
    const long zstride = (long)a.C * SEG_SUMS;          // doubles from one slab of a sample to the next
    const double s = (double)a.smooth;
    if (blockIdx.x == 0) {
        // (sample, channel) pairs in rounds of 48: lane t < 240 adds the slabs of one sum of one pair, lane i < 48 then adds the pair's
        // three terms to its own accumulators (pairs i, i + 48, ... in index order); wave 0's tree and one rounding end it
        const long NC = (long)a.N * a.C;
        double acc_ce = 0.0, acc_focal = 0.0, acc_dice = 0.0;
        for (long i0 = 0; i0 < NC; i0 += SEG_VALUE_TILE) {
            const int cnt = NC - i0 < SEG_VALUE_TILE ? (int)(NC - i0) : SEG_VALUE_TILE;
            __syncthreads();
            if (tid < cnt * SEG_SUMS) {
                const long i = i0 + tid / SEG_SUMS;
                const int k = tid % SEG_SUMS;
                const long n = i / a.C, c = i % a.C;
                const bool on = k < 3 ? dice : (k == 3 ? ce : focal);
                sums[tid] = on ? seg_slab_sum(a.ws + (n * a.nslab * a.C + c) * SEG_SUMS + k, zstride, a.nslab) : 0.0;
            }
            __syncthreads();
            if (tid < cnt) {
                const double* q = sums + tid * SEG_SUMS;
                if (W) {
                    const double w = (double)a.cw[(i0 + tid) % a.C];
                    if (ce) acc_ce += w * q[3];
                    if (focal) acc_focal += w * q[4];
                    if (dice) acc_dice += w * (1.0 - (2.0 * q[0] + s) / (q[1] + q[2] + s));
                } else {
                    if (ce) acc_ce += q[3];
                    if (focal) acc_focal += q[4];
                    if (dice) acc_dice += 1.0 - (2.0 * q[0] + s) / (q[1] + q[2] + s);
                }
            }
        }
        if (tid < 64) {
            acc_ce = seg_wave_sum(acc_ce);
            acc_focal = seg_wave_sum(acc_focal);
            acc_dice = seg_wave_sum(acc_dice);
            if (tid == 0) {
                double v = 0.0;
                if (ce) v += a.scale_ce * acc_ce;
                if (focal) v += a.scale_focal * acc_focal;
                if (dice) v += a.scale_dice * acc_dice;
                *a.value = (float)v;
            }
        }
        return;
    }
    const long b = (long)blockIdx.x - 1;
    const long n = b / a.nchunk;
    const int j = (int)(b % a.nchunk);
    const float sf_ce = (float)a.scale_ce, sf_focal = (float)a.scale_focal;
    for (int c0 = 0; c0 < a.C; c0 += 4) {
        const int nc = a.C - c0 < 4 ? a.C - c0 : 4;
        float sc_ce[4], sc_focal[4];          // the group's fp32 scales: one rounding from double each
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (W) {
                const double w = c < nc ? (double)a.cw[c0 + c] : 0.0;      // (a uniform load per channel of the group)
                sc_ce[c] = (float)(a.scale_ce * w);
                sc_focal[c] = (float)(a.scale_focal * w);
            } else {
                sc_ce[c] = sf_ce;
                sc_focal[c] = sf_focal;
            }
        }
        if (dice) {
            __syncthreads();      // (the previous group's reads of coef are over)
            if (tid < nc * 3) {
                const int c = tid / 3, k = tid % 3;
                sums[tid] = seg_slab_sum(a.ws + (n * a.nslab * a.C + c0 + c) * SEG_SUMS + k, zstride, a.nslab);
            }
            __syncthreads();
            if (tid < nc) {
                const double I = sums[tid * 3], den = sums[tid * 3 + 1] + sums[tid * 3 + 2] + s;
                const double sd = W ? a.scale_dice * (double)a.cw[c0 + tid] : a.scale_dice;
                coef[tid * 2 + 0] = (float)(-2.0 * sd / den);
                coef[tid * 2 + 1] = (float)(sd * (2.0 * I + s) / (den * den));
            }
            __syncthreads();
        }
        for (long i = (long)j * SEG_THREADS + tid; i < a.HW; i += (long)SEG_THREADS * a.nchunk) {
            const long pix = n * a.HW + i;
            const f4 pv = seg_load(a.p + pix * a.ld_p + c0, nc), yv = seg_load(a.y + pix * a.ld_y + c0, nc);
            f4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c < nc) {
                    const float p = pv[c], y = yv[c];
                    float gsum = 0.f;
                    bool first = true;
                    if (ce) {
                        gsum = sc_ce[c] * seg_ce_grad(p, y);
                        first = false;
                    }
                    if (focal) {
                        const float gf = sc_focal[c] * seg_focal_grad(p, y, seg_logp(p), seg_logq(p), a.gamma, a.a1, a.a0);
                        gsum = first ? gf : gsum + gf;
                        first = false;
                    }
                    if (dice) {
                        const float gd = coef[c * 2] * y + coef[c * 2 + 1];
                        gsum = first ? gd : gsum + gd;
                    }
                    r[c] = gsum;
                }
            }
            float* gp = a.g + pix * a.ld_g + c0;
            if (nc == 4) {
                seg_store4(gp, r);
            } else {
                gp[0] = r[0];
                if (nc > 1) gp[1] = r[1];
                if (nc > 2) gp[2] = r[2];
            }
        }
    }
}

// the settings both entry points take: 0 = fine
int seg_check(int N, int HW, int C, int terms, int focal_gamma, float focal_alpha) {
    if (N <= 0 || HW <= 0 || C <= 0) return PG_EINVAL;
    if (terms <= 0 || (terms & ~(PG_SEG_CE | PG_SEG_FOCAL | PG_SEG_DICE))) return PG_EINVAL;
    if ((terms & PG_SEG_CE) && C < 2) return PG_EINVAL;
    if (focal_gamma < 0 || focal_gamma > PG_SEG_FOCAL_GAMMA_MAX) return PG_EINVAL;
    if (!(focal_alpha == PG_SEG_FOCAL_ALPHA_NONE || (focal_alpha > 0.f && focal_alpha < 1.f))) return PG_EINVAL;
    return PG_OK;
}
bool seg_ws_ok(const void* ws, long ws_bytes, int N, int HW, int C) {
    return ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= seg_ws_doubles(N, HW, C) * (long)sizeof(double);
}
SegArgs seg_args(const float* p, int ld_p, const float* y, int ld_y, int N, int HW, int C, int terms, int focal_gamma, float focal_alpha,
                 void* ws) {
    SegArgs a = {};
    a.p = p, a.y = y, a.ws = (double*)ws;
    a.ld_p = ld_p, a.ld_y = ld_y;
    a.N = N, a.HW = HW, a.C = C, a.terms = terms, a.gamma = focal_gamma;
    a.nslab = seg_nslab(N, HW), a.nchunk = seg_nchunk(N, HW);
    const bool none = focal_alpha == PG_SEG_FOCAL_ALPHA_NONE;
    a.a1 = none ? 1.f : focal_alpha;
    a.a0 = none ? 1.f : 1.f - focal_alpha;
    return a;
}

// both phase-2 entry points: the checks, then the kernel without (W = false, cw unused) or with the per-class weights
template <bool W>
int seg_value_grad(const void* ws, long ws_bytes, const float* p, int ld_p, const float* y, int ld_y, int N, int HW, int C, int terms,
                   int focal_gamma, float focal_alpha, float dice_smooth, double scale_ce, double scale_focal, double scale_dice,
                   const float* cw, float* g, int ld_g, float* value, void* stream) {
    if (!p || !y || !value || seg_check(N, HW, C, terms, focal_gamma, focal_alpha) != PG_OK || ld_p < C || ld_y < C) return PG_EINVAL;
    if (!(dice_smooth > 0.f) || !std::isfinite(dice_smooth)) return PG_EINVAL;
    if (g && ld_g < C) return PG_EINVAL;
    if (!seg_ws_ok(ws, ws_bytes, N, HW, C)) return PG_EINVAL;
    SegArgs a = seg_args(p, ld_p, y, ld_y, N, HW, C, terms, focal_gamma, focal_alpha, const_cast<void*>(ws));
    a.g = g, a.ld_g = ld_g, a.value = value, a.smooth = dice_smooth, a.cw = cw;
    a.scale_ce = scale_ce, a.scale_focal = scale_focal, a.scale_dice = scale_dice;
    const long blocks = g ? 1 + (long)N * a.nchunk : 1;
    if (blocks > 0x7fffffffL) return PG_EINVAL;
    hipLaunchKernelGGL(k_seg_loss_value_grad<W>, dim3((unsigned)blocks), dim3(SEG_THREADS), 0, (hipStream_t)stream, a);
    return pg_launch_status();
}

// ---- per-class pixel counts of the target (pg_seg_label_count) ----------------------------------------------------------------------
// One pass over y alone: thread t of workgroup b takes the pixels b * 512 + t, + 512 * gridDim, ..., four of them per trip (their loads
// issued together), four channels at a time.  A wave counts a channel's hits (y_c >= 0.5f: false for a NaN) with one ballot per pixel
// and ONE lane adds the four popcounts to the workgroup's table of 64-bit counters in LDS (a 64-bit local cannot wrap, whatever N * HW
// is); the table goes to the 64-bit global words with one integer atomicAdd per non-zero counter when the workgroup is done.  At most
// 256 workgroups of 512 threads: every workgroup's adds land on the same few words and serialise there.  (Measured on cfg4's target,
// 8 x 512^2 x 4 in 8-float pixels, and cfg2's, 16 x 256^2 x 1 in 4-float pixels: 21.5 and 12.8 us; the first version -- up to 1024
// workgroups of 256 threads, one pixel per trip -- took 36.3 and 30.5 us; pg_seg_confusion on the same views 27.7 and 12.2 us.
// EXPERIMENTS.md.)  The table holds 1024 channels: a wider target is counted table by table, and the pass over the first table looks
// through the channels behind it only until it finds the pixel's label (the unlabelled count needs every channel).
// Integer sums only: the result does not depend on the order of arrival.
constexpr int SEG_COUNT_THREADS = 512;
constexpr int SEG_COUNT_BLOCKS = 256;
constexpr int SEG_COUNT_TABLE = 1024;
constexpr int SEG_COUNT_UNROLL = 4;

__global__ __launch_bounds__(SEG_COUNT_THREADS) void k_seg_label_count(const float* __restrict__ y, long ld_y, long npix, int C,
                                                                       unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long tab[SEG_COUNT_TABLE + 1];
    constexpr int U = SEG_COUNT_UNROLL;
    const int tid = threadIdx.x, lane = tid & 63;
    const long stride = (long)gridDim.x * SEG_COUNT_THREADS;
    const long trips = (npix + stride - 1) / stride;      // the same for every thread: the ballots below see whole waves
    for (int k0 = 0; k0 < C; k0 += SEG_COUNT_TABLE) {
        const int kc = C - k0 < SEG_COUNT_TABLE ? C - k0 : SEG_COUNT_TABLE;
        for (int i = tid; i <= kc; i += SEG_COUNT_THREADS) tab[i] = 0ull;
        __syncthreads();
        for (long trip = 0; trip < trips; trip += U) {
            const float* yp[U];                           // (read only where valid)
            bool valid[U], any[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long pix = (trip + u) * stride + (long)blockIdx.x * SEG_COUNT_THREADS + tid;
                valid[u] = pix < npix;                    // (a trip past the last one lies past npix as well)
                yp[u] = y + pix * ld_y;
                any[u] = false;
            }
            for (int c0 = 0; c0 < kc; c0 += 4) {
                const int nc = kc - c0 < 4 ? kc - c0 : 4;
                f4 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    v[u] = f4{0.f, 0.f, 0.f, 0.f};
                    if (valid[u]) v[u] = seg_load(yp[u] + k0 + c0, nc);
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c < nc) {
                        unsigned int hits = 0;
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const bool hit = v[u][c] >= 0.5f;
                            any[u] |= hit;
                            hits += (unsigned int)__popcll(__ballot(hit));
                        }
                        if (lane == 0 && hits) atomicAdd(&tab[c0 + c], (unsigned long long)hits);
                    }
                }
            }
            if (k0 == 0) {
                unsigned int none = 0;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (valid[u])
                        for (int c = kc; c < C && !any[u]; ++c) any[u] = yp[u][c] >= 0.5f;
                    none += (unsigned int)__popcll(__ballot(valid[u] && !any[u]));
                }
                if (lane == 0 && none) atomicAdd(&tab[kc], (unsigned long long)none);
            }
        }
        __syncthreads();
        for (int i = tid; i < kc; i += SEG_COUNT_THREADS) {
            const unsigned long long v = tab[i];
            if (v) atomicAdd(&counts[k0 + i], v);
        }
        if (k0 == 0 && tid == 0) {
            if (tab[kc]) atomicAdd(&counts[C], tab[kc]);
            if (blockIdx.x == 0) atomicAdd(&counts[(long)C + 1], (unsigned long long)npix);
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

long pg_seg_loss_workspace_bytes(int N, int HW, int C) {
    if (N <= 0 || HW <= 0 || C <= 0) return 0;
    return seg_ws_doubles(N, HW, C) * (long)sizeof(double);
}

int pg_seg_loss_slabs(int N, int HW) { return (N <= 0 || HW <= 0) ? 0 : seg_nslab(N, HW); }

int pg_seg_loss_reduce(const float* p, int ld_p, const float* y, int ld_y, int N, int HW, int C, int terms, int focal_gamma,
                       float focal_alpha, void* ws, long ws_bytes, void* stream) {
    if (!p || !y || seg_check(N, HW, C, terms, focal_gamma, focal_alpha) != PG_OK || ld_p < C || ld_y < C) return PG_EINVAL;
    if (!seg_ws_ok(ws, ws_bytes, N, HW, C)) return PG_EINVAL;
    const SegArgs a = seg_args(p, ld_p, y, ld_y, N, HW, C, terms, focal_gamma, focal_alpha, ws);
    if ((long)N * a.nslab > 0x7fffffffL) return PG_EINVAL;
    hipLaunchKernelGGL(k_seg_loss_reduce, dim3((unsigned)(N * a.nslab)), dim3(SEG_THREADS), 0, (hipStream_t)stream, a);
    return pg_launch_status();
}

int pg_seg_loss_value_grad(const void* ws, long ws_bytes, const float* p, int ld_p, const float* y, int ld_y, int N, int HW, int C,
                           int terms, int focal_gamma, float focal_alpha, float dice_smooth, double scale_ce, double scale_focal,
                           double scale_dice, float* g, int ld_g, float* value, void* stream) {
    return seg_value_grad<false>(ws, ws_bytes, p, ld_p, y, ld_y, N, HW, C, terms, focal_gamma, focal_alpha, dice_smooth, scale_ce,
                                 scale_focal, scale_dice, nullptr, g, ld_g, value, stream);
}

int pg_seg_loss_value_grad_w(const void* ws, long ws_bytes, const float* p, int ld_p, const float* y, int ld_y, int N, int HW, int C,
                             int terms, int focal_gamma, float focal_alpha, float dice_smooth, double scale_ce, double scale_focal,
                             double scale_dice, const float* cw, float* g, int ld_g, float* value, void* stream) {
    if (!cw) return PG_EINVAL;
    return seg_value_grad<true>(ws, ws_bytes, p, ld_p, y, ld_y, N, HW, C, terms, focal_gamma, focal_alpha, dice_smooth, scale_ce,
                                scale_focal, scale_dice, cw, g, ld_g, value, stream);
}

int pg_seg_label_count(const float* y, int ld_y, int N, int HW, int C, unsigned long long* counts, void* stream) {
    if (!y || !counts || N <= 0 || HW <= 0 || C <= 0 || ld_y < C) return PG_EINVAL;
    const long npix = (long)N * HW;
    const long per = (long)SEG_COUNT_THREADS * SEG_COUNT_UNROLL;
    long b = (npix + per - 1) / per;
    if (b > SEG_COUNT_BLOCKS) b = SEG_COUNT_BLOCKS;
    hipLaunchKernelGGL(k_seg_label_count, dim3((unsigned)b), dim3(SEG_COUNT_THREADS), 0, (hipStream_t)stream, y, (long)ld_y, npix, C,
                       counts);
    return pg_launch_status();
}

}  // extern "C"
