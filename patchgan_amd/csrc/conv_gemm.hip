// conv_gemm.hip -- the three GEMM-shaped 4x4 convolution kernels of the patchGAN hot path for gfx950.
//
//   big2small : small[n,p,q,a]   = sum_{tap,b} big[n,s*p-1+kh,s*q-1+kw,b] * P[tap][a][b]      (conv fwd, convT dgrad)
//   small2big : big[n,h,w,b]     = sum_{tap,a} small[n,(h+1-kh)/s,(w+1-kw)/s,a] * P[tap][a][b]  (convT fwd, conv dgrad)
//   wgrad     : dP[tap][a][b]    = sum_{n,p,q} small[n,p,q,a] * big[n,s*p-1+kh,s*q-1+kw,b]     (both weight grads)
//
// Each is an im2col-free implicit GEMM: 256-thread workgroups (4 waves of 64), operand tiles staged
// global -> registers -> LDS (prefetch of chunk c+1 issued before the MFMAs of chunk c), fp32 MFMA
// v_mfma_f32_32x32x2_f32 (exact fp32 fma chain, 64 FLOP/clk/SIMD), deterministic split-K through slabs.
// NHWC: a K-chunk of 32 consecutive (tap, channel) indices is 128 contiguous bytes of one input pixel.
//
// MFMA operand maps (cdna_hip_programming.md section 3): lane l holds A[i = l&31][k = l>>5] and
// B[k = l>>5][j = l&31]; C/D: col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5).
// K-contiguous operands are read from LDS as one ds_read_b128 per lane per 8 k: lane (row, h) takes
// k = 8*kk + 4*h + j (j = 0..3) for MFMA j, the same permutation of K on both operands.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <vector>
#include "patchgan_hip.h"
#include "pg_common.h"
#include "conv_wino.h"
#include "conv_bf16.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Geom {
    int N, Hb, Wb, Hs, Ws, Ca, Cb, s;
};

constexpr int KC = 32;        // K-chunk (floats)
constexpr int LDK = KC + 4;   // LDS row pitch of a K-contiguous tile: 36 floats -> conflict-free ds_read_b128

__device__ __forceinline__ f32x4 ld4(const float* p, bool ok) {
    f32x4 v = *reinterpret_cast<const f32x4*>(p);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    return ok ? v : z;
}

// ------------------------------------------------------------------------------------------------
// big2small: rows = small pixels (n,p,q), cols = a, K = (tap, b) with b fastest.
// ------------------------------------------------------------------------------------------------
template <int MR, int NR, int WM, int WN>
__global__ __launch_bounds__(256) void k_big2small(const float* __restrict__ big, int ld_big,
                                                   const float* __restrict__ P, float* __restrict__ out, int ld_out,
                                                   long slab_stride, Geom g, int chunks_per_slice, int veck,
                                                   const float* __restrict__ bias, int act) {
    constexpr int BM = WM * MR * 32, BN = WN * NR * 32;
    constexpr int AI = BM / 32, BI = BN / 32;
    __shared__ __attribute__((aligned(16))) float smem[(BM + BN) * LDK];
    float* As = smem;
    float* Bs = smem + BM * LDK;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lrow = lane & 31, lh = lane >> 5;
    const int M = g.N * g.Hs * g.Ws, K = 16 * g.Cb;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int nchunks = (K + KC - 1) / KC;
    const int c_begin = blockIdx.z * chunks_per_slice;
    const int c_end = min(nchunks, c_begin + chunks_per_slice);

    const int kq = tid & 7, r0 = tid >> 3;
    int a_noff[AI], a_h0[AI], a_w0[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        int m = m0 + r0 + 32 * i;
        if (m < M) {
            int n = m / (g.Hs * g.Ws);
            int rem = m - n * (g.Hs * g.Ws);
            int p = rem / g.Ws, q = rem - p * g.Ws;
            a_noff[i] = n * g.Hb * g.Wb;
            a_h0[i] = g.s * p - 1;
            a_w0[i] = g.s * q - 1;
        } else {
            a_noff[i] = 0;
            a_h0[i] = -1000000;
            a_w0[i] = 0;
        }
    }

    f32x4 ra[AI], rb[BI];
    // (tap, b) of this thread's float4 advance by KC per chunk: no division in the K loop when Cb >= KC
    int cur_tap = (c_begin * KC + kq * 4) / g.Cb;
    int cur_b = (c_begin * KC + kq * 4) - cur_tap * g.Cb;
    const bool inc_ok = g.Cb >= KC;
    auto load_chunk = [&](int c) {
        const int k = c * KC + kq * 4;
        if (veck) {
            int tap, b;
            if (inc_ok) {
                tap = cur_tap;
                b = cur_b;
                cur_b += KC;
                if (cur_b >= g.Cb) {
                    cur_b -= g.Cb;
                    ++cur_tap;
                }
            } else {
                tap = k / g.Cb;
                b = k - tap * g.Cb;
            }
            const int kh = tap >> 2, kw = tap & 3;
            const bool kok = k < K;
#pragma unroll
            for (int i = 0; i < AI; ++i) {
                int h = a_h0[i] + kh, w = a_w0[i] + kw;
                bool ok = kok && (unsigned)h < (unsigned)g.Hb && (unsigned)w < (unsigned)g.Wb;
                const float* p = ok ? big + ((long)(a_noff[i] + h * g.Wb + w) * ld_big + b) : big;
                ra[i] = ld4(p, ok);
            }
#pragma unroll
            for (int i = 0; i < BI; ++i) {
                int a = n0 + r0 + 32 * i;
                bool ok = kok && a < g.Ca;
                const float* p = ok ? P + ((long)(tap * g.Ca + a) * g.Cb + b) : P;
                rb[i] = ld4(p, ok);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ke = k + e;
                const int tap = ke / g.Cb, b = ke - tap * g.Cb;
                const int kh = tap >> 2, kw = tap & 3;
                const bool kok = ke < K;
#pragma unroll
                for (int i = 0; i < AI; ++i) {
                    int h = a_h0[i] + kh, w = a_w0[i] + kw;
                    bool ok = kok && (unsigned)h < (unsigned)g.Hb && (unsigned)w < (unsigned)g.Wb;
                    const float* p = ok ? big + ((long)(a_noff[i] + h * g.Wb + w) * ld_big + b) : big;
                    float v = *p;
                    ra[i][e] = ok ? v : 0.f;
                }
#pragma unroll
                for (int i = 0; i < BI; ++i) {
                    int a = n0 + r0 + 32 * i;
                    bool ok = kok && a < g.Ca;
                    const float* p = ok ? P + ((long)(tap * g.Ca + a) * g.Cb + b) : P;
                    float v = *p;
                    rb[i][e] = ok ? v : 0.f;
                }
            }
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < AI; ++i) *reinterpret_cast<f32x4*>(&As[(r0 + 32 * i) * LDK + kq * 4]) = ra[i];
#pragma unroll
        for (int i = 0; i < BI; ++i) *reinterpret_cast<f32x4*>(&Bs[(r0 + 32 * i) * LDK + kq * 4]) = rb[i];
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (c_begin < c_end) {
        load_chunk(c_begin);
        store_chunk();
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = (c + 1 < c_end);
        if (more) load_chunk(c + 1);
#pragma unroll
        for (int kk = 0; kk < KC / 8; ++kk) {
            f32x4 af[MR], bf[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i)
                af[i] = *reinterpret_cast<const f32x4*>(&As[((wm * MR + i) * 32 + lrow) * LDK + kk * 8 + lh * 4]);
#pragma unroll
            for (int j = 0; j < NR; ++j)
                bf[j] = *reinterpret_cast<const f32x4*>(&Bs[((wn * NR + j) * 32 + lrow) * LDK + kk * 8 + lh * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < MR; ++i)
#pragma unroll
                    for (int j = 0; j < NR; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            store_chunk();
            __syncthreads();
        }
    }

    float* o = out + (long)blockIdx.z * slab_stride;
    const bool fin = (slab_stride == 0);
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int col = n0 + (wn * NR + j) * 32 + lrow;
            const float bv = (fin && bias != nullptr && col < g.Ca) ? bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int m = m0 + (wm * MR + i) * 32 + row;
                if (m < M && col < g.Ca) {
                    float v = acc[i][j][r];
                    if (fin) v = pg_act(v + bv, act);
                    o[(long)m * ld_out + col] = v;
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------
// small2big: per output-parity class (stride 2: 4 classes of 2x2 taps; stride 1: 1 class of 4x4 taps):
// rows = big pixels of the class, cols = b, K = (tloc, a) with a fastest.  A is K-contiguous (small).
// P[tap][a][:] rows are N-contiguous in memory: each lane owns one column n and fetches 4 consecutive k with
// scalar loads (a wave-load is 64 consecutive floats of one weight row), so the tile lands K-contiguous in
// LDS and the MFMA loop is the same ds_read_b128 loop as big2small.
// ------------------------------------------------------------------------------------------------
template <int MR, int NR, int WM, int WN>
__global__ __launch_bounds__(256) void k_small2big(const float* __restrict__ small, int ld_small,
                                                   const float* __restrict__ P, float* __restrict__ out, int ld_out,
                                                   long slab_stride, Geom g, int chunks_per_slice, int veck, int vecn,
                                                   const float* __restrict__ bias, int act) {
    constexpr int BM = WM * MR * 32, BN = WN * NR * 32;
    constexpr int AI = BM / 32;
    constexpr int BG = 256 / BN;        // thread groups along k
    constexpr int NQ = 8 / BG;          // k-quads per thread per chunk
    __shared__ __attribute__((aligned(16))) float smem[(BM + BN) * LDK];
    float* As = smem;
    float* Bs = smem + BM * LDK;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lrow = lane & 31, lh = lane >> 5;

    const int ncls = (g.s == 2) ? 4 : 1;
    const int cls = blockIdx.z % ncls, slice = blockIdx.z / ncls;
    const int ah = (g.s == 2) ? (cls >> 1) : 0, aw = (g.s == 2) ? (cls & 1) : 0;
    const int T = (g.s == 2) ? 2 : 4;                    // taps per dim in this class
    const int Hc = (g.s == 2) ? (g.Hb - ah + 1) / 2 : g.Hb;
    const int Wc = (g.s == 2) ? (g.Wb - aw + 1) / 2 : g.Wb;
    const int kh0 = (g.s == 2) ? (1 - ah) : 0, kw0 = (g.s == 2) ? (1 - aw) : 0;
    const int Mc = g.N * Hc * Wc, K = T * T * g.Ca;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    if (m0 >= Mc) return;   // uniform per block (classes can differ in size for odd Hb/Wb)
    const int nchunks = (K + KC - 1) / KC;
    const int c_begin = slice * chunks_per_slice;
    const int c_end = min(nchunks, c_begin + chunks_per_slice);

    const int kq = tid & 7, r0 = tid >> 3;
    int a_noff[AI], a_ib[AI], a_jb[AI];   // small-pixel base: ih = ib - th, iw = jb - tw
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        int m = m0 + r0 + 32 * i;
        if (m < Mc) {
            int n = m / (Hc * Wc);
            int rem = m - n * (Hc * Wc);
            int ii = rem / Wc, jj = rem - ii * Wc;
            a_noff[i] = n * g.Hs * g.Ws;
            a_ib[i] = (g.s == 2) ? ii + ah : ii + 1;
            a_jb[i] = (g.s == 2) ? jj + aw : jj + 1;
        } else {
            a_noff[i] = 0;
            a_ib[i] = -1000000;
            a_jb[i] = 0;
        }
    }
    const int bn = tid % BN, bg = tid / BN;       // this thread's B column and k-group
    const int ncol = n0 + bn;
    const bool n_ok = ncol < g.Cb;

    // incremental (tloc, a) for the A float4 and for each B quad (valid when Ca >= KC and Ca % 4 == 0)
    const bool inc_ok = veck && g.Ca >= KC;
    int a_tl = (c_begin * KC + kq * 4) / g.Ca;
    int a_a = (c_begin * KC + kq * 4) - a_tl * g.Ca;
    int b_tl[NQ], b_a[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int k = c_begin * KC + 4 * (bg + BG * i);
        b_tl[i] = k / g.Ca;
        b_a[i] = k - b_tl[i] * g.Ca;
    }

    f32x4 ra[AI], rb[NQ];
    auto load_chunk = [&](int c) {
        const int k = c * KC + kq * 4;
        if (veck) {
            int tl, a;
            if (inc_ok) {
                tl = a_tl;
                a = a_a;
                a_a += KC;
                if (a_a >= g.Ca) {
                    a_a -= g.Ca;
                    ++a_tl;
                }
            } else {
                tl = k / g.Ca;
                a = k - tl * g.Ca;
            }
            const int th = tl / T, tw = tl - th * T;
            const bool kok = k < K;
#pragma unroll
            for (int i = 0; i < AI; ++i) {
                int ih = a_ib[i] - th, iw = a_jb[i] - tw;
                bool ok = kok && (unsigned)ih < (unsigned)g.Hs && (unsigned)iw < (unsigned)g.Ws;
                const float* p = ok ? small + ((long)(a_noff[i] + ih * g.Ws + iw) * ld_small + a) : small;
                ra[i] = ld4(p, ok);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ke = k + e;
                const int tl = ke / g.Ca, a = ke - tl * g.Ca;
                const int th = tl / T, tw = tl - th * T;
                const bool kok = ke < K;
#pragma unroll
                for (int i = 0; i < AI; ++i) {
                    int ih = a_ib[i] - th, iw = a_jb[i] - tw;
                    bool ok = kok && (unsigned)ih < (unsigned)g.Hs && (unsigned)iw < (unsigned)g.Ws;
                    const float* p = ok ? small + ((long)(a_noff[i] + ih * g.Ws + iw) * ld_small + a) : small;
                    float v = *p;
                    ra[i][e] = ok ? v : 0.f;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int kb = c * KC + 4 * (bg + BG * i);
            if (inc_ok) {
                const int tl = b_tl[i], a = b_a[i];
                b_a[i] += KC;
                if (b_a[i] >= g.Ca) {
                    b_a[i] -= g.Ca;
                    ++b_tl[i];
                }
                const int th = tl / T, tw = tl - th * T;
                const int tap = (kh0 + g.s * th) * 4 + (kw0 + g.s * tw);
                const bool ok = n_ok && kb < K;
                const float* col = ok ? P + (long)(tap * g.Ca + a) * g.Cb + ncol : P;
                const long st = ok ? g.Cb : 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = col[e * st];
                    rb[i][e] = ok ? v : 0.f;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int ke = kb + e;
                    const int tl = ke / g.Ca, a = ke - tl * g.Ca;
                    const int th = tl / T, tw = tl - th * T;
                    const int tap = (kh0 + g.s * th) * 4 + (kw0 + g.s * tw);
                    const bool ok = n_ok && ke < K;
                    float v = *(ok ? P + (long)(tap * g.Ca + a) * g.Cb + ncol : P);
                    rb[i][e] = ok ? v : 0.f;
                }
            }
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < AI; ++i) *reinterpret_cast<f32x4*>(&As[(r0 + 32 * i) * LDK + kq * 4]) = ra[i];
#pragma unroll
        for (int i = 0; i < NQ; ++i) *reinterpret_cast<f32x4*>(&Bs[bn * LDK + 4 * (bg + BG * i)]) = rb[i];
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (c_begin < c_end) {
        load_chunk(c_begin);
        store_chunk();
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = (c + 1 < c_end);
        if (more) load_chunk(c + 1);
#pragma unroll
        for (int kk = 0; kk < KC / 8; ++kk) {
            f32x4 af[MR], bf[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i)
                af[i] = *reinterpret_cast<const f32x4*>(&As[((wm * MR + i) * 32 + lrow) * LDK + kk * 8 + lh * 4]);
#pragma unroll
            for (int j = 0; j < NR; ++j)
                bf[j] = *reinterpret_cast<const f32x4*>(&Bs[((wn * NR + j) * 32 + lrow) * LDK + kk * 8 + lh * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < MR; ++i)
#pragma unroll
                    for (int j = 0; j < NR; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            store_chunk();
            __syncthreads();
        }
    }

    // epilogue: row m of the class -> big pixel (n, s*ii+ah, s*jj+aw); slabs mirror the [N,Hb,Wb,Cb] layout.
    const bool fin = (slab_stride == 0);
    float* o = out + (long)slice * slab_stride;
    const int ldo = fin ? ld_out : g.Cb;
    float bv[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int col = n0 + (wn * NR + j) * 32 + lrow;
        bv[j] = (fin && bias != nullptr && col < g.Cb) ? bias[col] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < MR; ++i) {
        // rows of this lane: base + {0..3} + 8*{0..3} + 4*lh ; decode the first, then step (the 16 rows of a lane
        // are at most 28 apart, so a carry chain in (jj, ii, n) is cheaper than 16 divisions)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int m = m0 + (wm * MR + i) * 32 + row;
            if (m < Mc) {
                int n = m / (Hc * Wc);
                int rem = m - n * (Hc * Wc);
                int ii = rem / Wc, jj = rem - ii * Wc;
                int h = (g.s == 2) ? 2 * ii + ah : ii, w = (g.s == 2) ? 2 * jj + aw : jj;
                float* orow = o + (long)((n * g.Hb + h) * g.Wb + w) * ldo;
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    const int col = n0 + (wn * NR + j) * 32 + lrow;
                    if (col < g.Cb) {
                        float v = acc[i][j][r];
                        if (fin) v = pg_act(v + bv[j], act);
                        orow[col] = v;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// wgrad: per tap, rows = a, cols = b, K = small pixels.  Both operands are contiguous along their
// non-K dim, so LDS tiles are [k][m] / [k][n] and fragments are single ds_read_b32 (natural K order).
// grid: x = tilesA*tilesB, y = 16 taps, z = K slices.  Output slab z is [16][Ca][Cb].
// ------------------------------------------------------------------------------------------------
template <int MR, int NR, int WM, int WN>
__global__ __launch_bounds__(256) void k_wgrad(const float* __restrict__ small, int ld_small,
                                               const float* __restrict__ big, int ld_big,
                                               float* __restrict__ out, long slab_stride, Geom g,
                                               int chunks_per_slice, int tilesB, int vecm, int vecn) {
    constexpr int BM = WM * MR * 32, BN = WN * NR * 32;
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int AQ = BM / 4, AROWS = 256 / AQ, AI = KC / AROWS;
    constexpr int BQ = BN / 4, BROWS = 256 / BQ, BI = KC / BROWS;
    __shared__ __attribute__((aligned(16))) float smem[KC * LDA + KC * LDB];
    float* As = smem;
    float* Bs = smem + KC * LDA;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lrow = lane & 31, lh = lane >> 5;
    const int tile_a = blockIdx.x / tilesB, tile_b = blockIdx.x % tilesB;
    const int m0 = tile_a * BM, n0 = tile_b * BN;
    const int tap = blockIdx.y, kh = tap >> 2, kw = tap & 3;
    const int Kp = g.N * g.Hs * g.Ws;   // pixels
    const int nchunks = (Kp + KC - 1) / KC;
    const int c_begin = blockIdx.z * chunks_per_slice;
    const int c_end = min(nchunks, c_begin + chunks_per_slice);

    const int aq = tid % AQ, arow0 = tid / AQ;
    const int bq = tid % BQ, brow0 = tid / BQ;
    const bool inc_ok = g.Ws >= 16 && g.Hs >= 2;
    int r_n[BI], r_p[BI], r_q[BI];
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        const int pix = c_begin * KC + brow0 + BROWS * i;
        r_n[i] = pix / (g.Hs * g.Ws);
        const int rem = pix - r_n[i] * (g.Hs * g.Ws);
        r_p[i] = rem / g.Ws;
        r_q[i] = rem - r_p[i] * g.Ws;
    }

    f32x4 ra[AI], rb[BI];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            const int pix = c * KC + arow0 + AROWS * i;
            const int a = m0 + aq * 4;
            const bool pok = pix < Kp;
            const float* row = small + (long)pix * ld_small;
            if (vecm) {
                bool ok = pok && a < g.Ca;
                ra[i] = ld4(ok ? row + a : small, ok);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bool ok = pok && (a + e) < g.Ca;
                    float v = *(ok ? row + a + e : small);
                    ra[i][e] = ok ? v : 0.f;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < BI; ++i) {
            const int pix = c * KC + brow0 + BROWS * i;
            const int b = n0 + bq * 4;
            bool pok = pix < Kp;
            int n, p, q;
            if (inc_ok) {   // carry chain instead of two divisions per row and chunk
                n = r_n[i];
                p = r_p[i];
                q = r_q[i];
                r_q[i] += KC;
                while (r_q[i] >= g.Ws) {
                    r_q[i] -= g.Ws;
                    ++r_p[i];
                }
                while (r_p[i] >= g.Hs) {
                    r_p[i] -= g.Hs;
                    ++r_n[i];
                }
            } else {
                n = pix / (g.Hs * g.Ws);
                int rem = pix - n * (g.Hs * g.Ws);
                p = rem / g.Ws;
                q = rem - p * g.Ws;
            }
            int h = g.s * p - 1 + kh, w = g.s * q - 1 + kw;
            pok = pok && (unsigned)h < (unsigned)g.Hb && (unsigned)w < (unsigned)g.Wb;
            const float* row = big + (long)((n * g.Hb + h) * g.Wb + w) * ld_big;
            if (vecn) {
                bool ok = pok && b < g.Cb;
                rb[i] = ld4(ok ? row + b : big, ok);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bool ok = pok && (b + e) < g.Cb;
                    float v = *(ok ? row + b + e : big);
                    rb[i][e] = ok ? v : 0.f;
                }
            }
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < AI; ++i) *reinterpret_cast<f32x4*>(&As[(arow0 + AROWS * i) * LDA + aq * 4]) = ra[i];
#pragma unroll
        for (int i = 0; i < BI; ++i) *reinterpret_cast<f32x4*>(&Bs[(brow0 + BROWS * i) * LDB + bq * 4]) = rb[i];
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (c_begin < c_end) {
        load_chunk(c_begin);
        store_chunk();
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = (c + 1 < c_end);
        if (more) load_chunk(c + 1);
#pragma unroll
        for (int kk = 0; kk < KC / 2; ++kk) {
            float af[MR], bf[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i) af[i] = As[(kk * 2 + lh) * LDA + (wm * MR + i) * 32 + lrow];
#pragma unroll
            for (int j = 0; j < NR; ++j) bf[j] = Bs[(kk * 2 + lh) * LDB + (wn * NR + j) * 32 + lrow];
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            store_chunk();
            __syncthreads();
        }
    }

    float* o = out + (long)blockIdx.z * slab_stride + (long)tap * g.Ca * g.Cb;
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int col = n0 + (wn * NR + j) * 32 + lrow;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int a = m0 + (wm * MR + i) * 32 + row;
                if (a < g.Ca && col < g.Cb) o[(long)a * g.Cb + col] = acc[i][j][r];
            }
        }
}

// ------------------------------------------------------------------------------------------------
// wgrad with the 16 taps folded into the GEMM N dimension, for layers with very few channels on one side
// (the image-facing layers: enc0 / d0 have Cb = 3..10, dec6 has Cb = output_nc, the D head has Ca = 1).  The
// per-tap kernel above would pad those channels to a 32-wide MFMA tile 16 times over; here N = 16*C is dense.
//   MODE 1 (Cb <= 8): rows m = a, cols n = (tap, b), K = small pixels
//        A[k][m] = small[pix][a]              B[k][n] = big[img, s*p-1+kh, s*q-1+kw][b]
//   MODE 2 (Ca <= 8): rows m = b, cols n = (tap, a), K = big pixels
//        A[k][m] = big[pix][b]                B[k][n] = small[img, (h+1-kh)/s, (w+1-kw)/s][a]
// Output element (tap, a, b) -> slab[(tap*Ca + a)*Cb + b].  X = the row tensor, Y = the gathered tensor.
// ------------------------------------------------------------------------------------------------
template <int MR, int NR, int WM, int WN, int MODE>
__global__ __launch_bounds__(256) void k_wgrad_tapn(const float* __restrict__ X, int ld_x,
                                                    const float* __restrict__ Y, int ld_y, float* __restrict__ out,
                                                    long slab_stride, Geom g, int chunks_per_slice, int tilesN,
                                                    int vecm, int vecy) {
    constexpr int BM = WM * MR * 32, BN = WN * NR * 32;
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int AQ = BM / 4, AROWS = 256 / AQ, AI = KC / AROWS;
    constexpr int BQ = BN / 4, BROWS = 256 / BQ, BI = KC / BROWS;
    __shared__ __attribute__((aligned(16))) float smem[KC * LDA + KC * LDB];
    float* As = smem;
    float* Bs = smem + KC * LDA;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lrow = lane & 31, lh = lane >> 5;
    const int tile_m = blockIdx.x / tilesN, tile_n = blockIdx.x % tilesN;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int Cx = (MODE == 1) ? g.Ca : g.Cb;            // channels of the row tensor  (GEMM M)
    const int Cy = (MODE == 1) ? g.Cb : g.Ca;            // channels of the gathered tensor
    const int Hx = (MODE == 1) ? g.Hs : g.Hb, Wx = (MODE == 1) ? g.Ws : g.Wb;
    const int Ndim = 16 * Cy;
    const int Kp = g.N * Hx * Wx;
    const int nchunks = (Kp + KC - 1) / KC;
    const int c_begin = blockIdx.z * chunks_per_slice;
    const int c_end = min(nchunks, c_begin + chunks_per_slice);

    const int aq = tid % AQ, arow0 = tid / AQ;
    const int bq = tid % BQ, brow0 = tid / BQ;
    // this thread's four gathered columns are fixed for the whole K loop
    int e_kh[4], e_kw[4], e_c[4];
    bool e_ok[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int n = n0 + bq * 4 + e;
        const int tap = n / Cy;
        e_ok[e] = n < Ndim;
        e_c[e] = n - tap * Cy;
        e_kh[e] = tap >> 2;
        e_kw[e] = tap & 3;
    }

    const bool inc_ok = Wx >= 16 && Hx >= 2;
    int r_n[BI], r_p[BI], r_q[BI];
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        const int pix = c_begin * KC + brow0 + BROWS * i;
        r_n[i] = pix / (Hx * Wx);
        const int rem = pix - r_n[i] * (Hx * Wx);
        r_p[i] = rem / Wx;
        r_q[i] = rem - r_p[i] * Wx;
    }

    f32x4 ra[AI], rb[BI];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            const int pix = c * KC + arow0 + AROWS * i;
            const int m = m0 + aq * 4;
            const bool pok = pix < Kp;
            const float* row = X + (long)pix * ld_x;
            if (vecm) {
                bool ok = pok && m < Cx;
                ra[i] = ld4(ok ? row + m : X, ok);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bool ok = pok && (m + e) < Cx;
                    float v = *(ok ? row + m + e : X);
                    ra[i][e] = ok ? v : 0.f;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < BI; ++i) {
            const int pix = c * KC + brow0 + BROWS * i;
            const bool pok = pix < Kp;
            int img, r, cc;
            if (inc_ok) {
                img = r_n[i];
                r = r_p[i];
                cc = r_q[i];
                r_q[i] += KC;
                while (r_q[i] >= Wx) {
                    r_q[i] -= Wx;
                    ++r_p[i];
                }
                while (r_p[i] >= Hx) {
                    r_p[i] -= Hx;
                    ++r_n[i];
                }
            } else {
                img = pix / (Hx * Wx);
                const int rem = pix - img * (Hx * Wx);
                r = rem / Wx;
                cc = rem - r * Wx;
            }
            if (MODE == 1 && vecy) {
                // Cb == 4: this thread's four columns are the four channels of ONE tap: one 16-byte load
                const int h = g.s * r - 1 + e_kh[0], w = g.s * cc - 1 + e_kw[0];
                const bool ok = pok && e_ok[0] && (unsigned)h < (unsigned)g.Hb && (unsigned)w < (unsigned)g.Wb;
                rb[i] = ld4(ok ? Y + (long)((img * g.Hb + h) * g.Wb + w) * ld_y : Y, ok);
                continue;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bool ok = pok && e_ok[e];
                long off;
                if (MODE == 1) {
                    const int h = g.s * r - 1 + e_kh[e], w = g.s * cc - 1 + e_kw[e];
                    ok = ok && (unsigned)h < (unsigned)g.Hb && (unsigned)w < (unsigned)g.Wb;
                    off = (long)((img * g.Hb + h) * g.Wb + w) * ld_y + e_c[e];
                } else {
                    const int hh = r + 1 - e_kh[e], ww = cc + 1 - e_kw[e];
                    ok = ok && hh >= 0 && ww >= 0;
                    int p = hh, q = ww;
                    if (g.s == 2) {
                        ok = ok && ((hh & 1) == 0) && ((ww & 1) == 0);
                        p = hh >> 1;
                        q = ww >> 1;
                    }
                    ok = ok && p < g.Hs && q < g.Ws;
                    off = (long)((img * g.Hs + p) * g.Ws + q) * ld_y + e_c[e];
                }
                float v = *(ok ? Y + off : Y);
                rb[i][e] = ok ? v : 0.f;
            }
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < AI; ++i) *reinterpret_cast<f32x4*>(&As[(arow0 + AROWS * i) * LDA + aq * 4]) = ra[i];
#pragma unroll
        for (int i = 0; i < BI; ++i) *reinterpret_cast<f32x4*>(&Bs[(brow0 + BROWS * i) * LDB + bq * 4]) = rb[i];
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (c_begin < c_end) {
        load_chunk(c_begin);
        store_chunk();
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = (c + 1 < c_end);
        if (more) load_chunk(c + 1);
#pragma unroll
        for (int kk = 0; kk < KC / 2; ++kk) {
            float af[MR], bf[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i) af[i] = As[(kk * 2 + lh) * LDA + (wm * MR + i) * 32 + lrow];
#pragma unroll
            for (int j = 0; j < NR; ++j) bf[j] = Bs[(kk * 2 + lh) * LDB + (wn * NR + j) * 32 + lrow];
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            store_chunk();
            __syncthreads();
        }
    }

    float* o = out + (long)blockIdx.z * slab_stride;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int n = n0 + (wn * NR + j) * 32 + lrow;
        if (n >= Ndim) continue;
        const int tap = n / Cy, cy = n - tap * Cy;
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int m = m0 + (wm * MR + i) * 32 + row;
                if (m < Cx) {
                    const long idx = (MODE == 1) ? ((long)(tap * g.Ca + m) * g.Cb + cy) : ((long)(tap * g.Ca + cy) * g.Cb + m);
                    o[idx] = acc[i][j][r];
                }
            }
    }
}

// ================================================================================================
// Fast variants (the hot path whenever channels are multiples of 4, buffers are 16-byte aligned, every tensor
// they gather from spans < FAST_LIMIT = 1.5 GiB and the packed weights < FAST_P_LIMIT = 1 GiB; the table next to
// FAST_LIMIT says which operand each planner path checks): same tiling and MFMA loop as the generic kernels above, but
//   * operand gathers are raw buffer loads (hardware range check: an out-of-range offset returns 0), so the
//     zero padding, ragged tiles and K tails cost one v_cndmask instead of a divergent branch per load,
//   * all offsets are 32-bit element offsets from a per-row base computed once per tile; tap validity is a
//     16-bit mask per row (one shift+and per load),
//   * the loads of chunk c+1 are spread over the four 8-k steps of chunk c, inside ONE basic block, so the
//     scheduler interleaves their address arithmetic with the MFMAs instead of running it ahead of them.
// ================================================================================================
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int OOB = 0x7fffffff;
// Scheduling fence that only vector-memory instructions may not cross (LLVM sched_barrier mask: ALU | VALU | SALU |
// DS | DS-read | DS-write may; MFMA and VMEM may not).  Without it hipcc sinks the next chunk's buffer loads to the END of the MFMA
// sequence (to shorten their destination registers' live ranges), so their latency lands on the barrier instead of
// under 48 MFMAs.
#define PIN_VMEM() __builtin_amdgcn_sched_barrier(0x386)
// element offset -> byte offset without signed overflow (sentinel offsets exceed INT_MAX/4 on purpose)
__device__ __forceinline__ int b4(int elem_off) { return (int)((unsigned)elem_off << 2); }
__device__ __forceinline__ int xcd_remap(int bid, int nblk) { return pg_xcd_remap(bid, nblk); }   // pg_common.h

// byte offset of a gather element, forced out of range (bit 31 set: >= 2 GiB > any descriptor here) when !ok.
// Written as an OR so the offset arithmetic stays unconditional: with `ok ? off : OOB` hipcc sinks the arithmetic into
// an exec-masked region per load, which splits the MFMA loop into many scheduling regions.
__device__ __forceinline__ int voff(int elem_off, bool ok) {
    return (int)(((unsigned)elem_off << 2) | (ok ? 0u : 0x80000000u));
}

__device__ __forceinline__ f32x4 bload4(__amdgpu_buffer_rsrc_t r, int byte_off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}
__device__ __forceinline__ float bload1(__amdgpu_buffer_rsrc_t r, int byte_off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}

__device__ __noinline__ float pg_act_slow(float v, int act) { return pg_act(v, act); }
__device__ __forceinline__ float pg_act_epi(float v, int act) {
    if (act == PG_ACT_NONE) return v;
    if (act == PG_ACT_LEAKY) return v > 0.f ? v : 0.2f * v;
    if (act == PG_ACT_RELU) return v > 0.f ? v : 0.f;
    return pg_act_slow(v, act);
}

// ONE = true turns the kernel into a plain row GEMM  out[m][a] = sum_b big[m][b] * P[a][b]  (a 1x1 "convolution" over
// the N*Hb*Wb pixels of `big`): the first half of the taps-folded-into-N path for layers with <= 8 channels on the
// output side, whose second half is a col2im / tap-gather pass (k_col2im_small2big, k_gather_big2small).
template <int MR, int NR, int WM, int WN, bool ONE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_b2s_fast(const float* __restrict__ big, int ld_big,
                                                  const float* __restrict__ P, float* __restrict__ out, int ld_out,
                                                  long slab_stride, Geom g, int chunks_per_slice,
                                                  const float* __restrict__ bias, int act, int big_bytes, int p_bytes) {
    constexpr int BM = WM * MR * 32, BN = WN * NR * 32;
    constexpr int AI = BM / 32, BI = BN / 32;
    __shared__ __attribute__((aligned(16))) float smem[(BM + BN) * LDK];
    float* As = smem;
    float* Bs = smem + BM * LDK;
    const __amdgpu_buffer_rsrc_t rbig = __builtin_amdgcn_make_buffer_rsrc((void*)big, 0, big_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rP = __builtin_amdgcn_make_buffer_rsrc((void*)P, 0, p_bytes, 0x00020000);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lrow = lane & 31, lh = lane >> 5;
    const int M = ONE ? g.N * g.Hb * g.Wb : g.N * g.Hs * g.Ws;
    const int K = ONE ? g.Cb : 16 * g.Cb;               // K % 32 == 0 (Cb % 4 == 0; ONE requires Cb % 32 == 0)
    const int m0 = xcd_remap(blockIdx.x, gridDim.x) * BM, n0 = blockIdx.y * BN;
    const int nchunks = K / KC;
    const int c_begin = blockIdx.z * chunks_per_slice;
    const int c_end = min(nchunks, c_begin + chunks_per_slice);

    const int kq = tid & 7, r0 = tid >> 3;
    int a_off[AI], a_mask[AI], b_off[BI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int m = m0 + r0 + 32 * i;
        const int mm = min(m, M - 1);
        if (ONE) {
            a_off[i] = mm * ld_big;
            a_mask[i] = (m < M) ? 1 : 0;
            continue;
        }
        const int n = mm / (g.Hs * g.Ws);
        const int rem = mm - n * (g.Hs * g.Ws);
        const int p = rem / g.Ws, q = rem - p * g.Ws;
        const int h0 = g.s * p - 1, w0 = g.s * q - 1;
        a_off[i] = ((n * g.Hb + h0) * g.Wb + w0) * ld_big;
        int wv = 0, mask = 0;          // tap (kh, kw) is inside the image iff row kh and column kw both are
#pragma unroll
        for (int t = 0; t < 4; ++t) wv |= ((unsigned)(w0 + t) < (unsigned)g.Wb) ? (1 << t) : 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) mask |= ((unsigned)(h0 + t) < (unsigned)g.Hb) ? (wv << (4 * t)) : 0;
        a_mask[i] = (m < M) ? mask : 0;
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        const int a = n0 + r0 + 32 * i;
        b_off[i] = (a < g.Ca) ? a * g.Cb : 0x10000000;
    }
    const int CaCb = g.Ca * g.Cb;
    int cur_tap = (c_begin * KC + kq * 4) / g.Cb;
    int cur_b = (c_begin * KC + kq * 4) - cur_tap * g.Cb;

    f32x4 ra[AI], rb[BI];
    int tapoff = 0, pboff = 0, ctap = 0;
    auto next_tap = [&]() {   // (tap, b) of the next chunk for this thread's float4; Cb >= KC: at most one wrap
        const int tap = cur_tap, b = cur_b;
        cur_b += KC;
        const bool wrap = cur_b >= g.Cb;
        cur_b = wrap ? cur_b - g.Cb : cur_b;
        cur_tap = wrap ? cur_tap + 1 : cur_tap;
        ctap = tap;
        tapoff = ((tap >> 2) * g.Wb + (tap & 3)) * ld_big + b;
        pboff = tap * CaCb + b;
    };
    auto load_a = [&](int i, bool on) {
        const bool ok = on && ((a_mask[i] >> ctap) & 1);
        ra[i] = bload4(rbig, voff(a_off[i] + tapoff, ok));
    };
    auto load_b = [&](int i, bool on) { rb[i] = bload4(rP, voff(b_off[i] + pboff, on)); };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < AI; ++i) *reinterpret_cast<f32x4*>(&As[(r0 + 32 * i) * LDK + kq * 4]) = ra[i];
#pragma unroll
        for (int i = 0; i < BI; ++i) *reinterpret_cast<f32x4*>(&Bs[(r0 + 32 * i) * LDK + kq * 4]) = rb[i];
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (c_begin < c_end) {
        next_tap();
#pragma unroll
        for (int i = 0; i < AI; ++i) load_a(i, true);
#pragma unroll
        for (int i = 0; i < BI; ++i) load_b(i, true);
        store_chunk();
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = (c + 1 < c_end);
        next_tap();
#pragma unroll
        for (int kk = 0; kk < KC / 8; ++kk) {
            f32x4 af[MR], bf[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i)
                af[i] = *reinterpret_cast<const f32x4*>(&As[((wm * MR + i) * 32 + lrow) * LDK + kk * 8 + lh * 4]);
#pragma unroll
            for (int j = 0; j < NR; ++j)
                bf[j] = *reinterpret_cast<const f32x4*>(&Bs[((wn * NR + j) * 32 + lrow) * LDK + kk * 8 + lh * 4]);
            if (kk < AI) load_a(kk, more);
            if (kk < BI) load_b(kk, more);
            PIN_VMEM();
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < MR; ++i)
#pragma unroll
                    for (int j = 0; j < NR; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            store_chunk();
            __syncthreads();
        }
    }

    float* o = out + (long)blockIdx.z * slab_stride;
    const bool fin = (slab_stride == 0);
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int col = n0 + (wn * NR + j) * 32 + lrow;
            const float bv = (fin && bias != nullptr && col < g.Ca) ? bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int m = m0 + (wm * MR + i) * 32 + row;
                if (m < M && col < g.Ca) {
                    float v = acc[i][j][r];
                    if (fin) v = pg_act_epi(v + bv, act);
                    o[(long)m * ld_out + col] = v;
                }
            }
        }
}

template <int MR, int NR, int WM, int WN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_s2b_fast(const float* __restrict__ small, int ld_small,
                                                  const float* __restrict__ P, float* __restrict__ out, int ld_out,
                                                  long slab_stride, Geom g, int chunks_per_slice,
                                                  const float* __restrict__ bias, int act, int small_bytes,
                                                  int p_bytes) {
    constexpr int BM = WM * MR * 32, BN = WN * NR * 32;
    constexpr int AI = BM / 32;
    constexpr int BG = 256 / BN;        // thread groups along k
    constexpr int NQ = 8 / BG;          // k-quads per thread per chunk
    __shared__ __attribute__((aligned(16))) float smem[(BM + BN) * LDK];
    float* As = smem;
    float* Bs = smem + BM * LDK;
    const __amdgpu_buffer_rsrc_t rsm = __builtin_amdgcn_make_buffer_rsrc((void*)small, 0, small_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rP = __builtin_amdgcn_make_buffer_rsrc((void*)P, 0, p_bytes, 0x00020000);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lrow = lane & 31, lh = lane >> 5;

    const int ncls = (g.s == 2) ? 4 : 1;
    const int cls = blockIdx.z % ncls, slice = blockIdx.z / ncls;
    const int ah = (g.s == 2) ? (cls >> 1) : 0, aw = (g.s == 2) ? (cls & 1) : 0;
    const int T = (g.s == 2) ? 2 : 4, Tsh = (g.s == 2) ? 1 : 2;
    const int Hc = (g.s == 2) ? (g.Hb - ah + 1) / 2 : g.Hb;
    const int Wc = (g.s == 2) ? (g.Wb - aw + 1) / 2 : g.Wb;
    const int kh0 = (g.s == 2) ? (1 - ah) : 0, kw0 = (g.s == 2) ? (1 - aw) : 0;
    const int Mc = g.N * Hc * Wc, K = T * T * g.Ca;
    const int m0 = xcd_remap(blockIdx.x, gridDim.x) * BM, n0 = blockIdx.y * BN;
    if (m0 >= Mc) return;
    const int nchunks = (K + KC - 1) / KC;
    const int c_begin = slice * chunks_per_slice;
    const int c_end = min(nchunks, c_begin + chunks_per_slice);

    const int kq = tid & 7, r0 = tid >> 3;
    int a_off[AI], a_mask[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int m = m0 + r0 + 32 * i;
        const int mm = min(m, Mc - 1);
        const int n = mm / (Hc * Wc);
        const int rem = mm - n * (Hc * Wc);
        const int ii = rem / Wc, jj = rem - ii * Wc;
        const int ib = (g.s == 2) ? ii + ah : ii + 1, jb = (g.s == 2) ? jj + aw : jj + 1;
        a_off[i] = ((n * g.Hs + ib) * g.Ws + jb) * ld_small;
        int wv = 0, mask = 0;          // local tap (th, tw) reads small pixel (ib - th, jb - tw)
#pragma unroll
        for (int t = 0; t < 4; ++t) wv |= (t < T && (unsigned)(jb - t) < (unsigned)g.Ws) ? (1 << t) : 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) mask |= (t < T && (unsigned)(ib - t) < (unsigned)g.Hs) ? (wv << (T * t)) : 0;
        a_mask[i] = (m < Mc) ? mask : 0;
    }
    const int bn = tid % BN, bg = tid / BN;
    const int ncol = n0 + bn;
    const int ncol_off = (ncol < g.Cb) ? ncol : 0x10000000;
    const int CaCb = g.Ca * g.Cb;

    // incremental (tloc, a) per k-quad: A float4 (index 0) and the NQ quads of B (1..NQ); Ca >= KC: <= 1 wrap
    int q_tl[NQ + 1], q_a[NQ + 1];
    {
        const int k = c_begin * KC + kq * 4;
        q_tl[0] = k / g.Ca;
        q_a[0] = k - q_tl[0] * g.Ca;
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int k = c_begin * KC + 4 * (bg + BG * i);
        q_tl[i + 1] = k / g.Ca;
        q_a[i + 1] = k - q_tl[i + 1] * g.Ca;
    }
    auto quad = [&](int qi, int& tl, int& a) {   // returns (tloc, a) of quad qi for the chunk being loaded
        tl = q_tl[qi];
        a = q_a[qi];
        const int na = a + KC;
        const bool wrap = na >= g.Ca;
        q_a[qi] = wrap ? na - g.Ca : na;
        q_tl[qi] = wrap ? tl + 1 : tl;
    };

    f32x4 ra[AI], rb[NQ];
    int a_tl = 0, a_koff = OOB;
    auto next_a = [&](int c) {
        const int k = c * KC + kq * 4;
        int tl, a;
        quad(0, tl, a);
        a_tl = tl;
        const int th = tl >> Tsh, tw = tl & (T - 1);
        a_koff = (k < K) ? (a - (th * g.Ws + tw) * ld_small) : 0x20000000;
    };
    auto load_a = [&](int i, bool on) {
        const bool ok = on && ((a_mask[i] >> a_tl) & 1) && (a_koff < 0x10000000);
        ra[i] = bload4(rsm, voff(a_off[i] + a_koff, ok));
    };
    auto load_b = [&](int i, int c, bool on) {
        const int kb = c * KC + 4 * (bg + BG * i);
        int tl, a;
        quad(i + 1, tl, a);
        if (BN >= 64) {   // a wave shares one k-quad (bg = tid / BN is wave-uniform): keep its decode on the scalar unit
            tl = __builtin_amdgcn_readfirstlane(tl);
            a = __builtin_amdgcn_readfirstlane(a);
        }
        const int th = tl >> Tsh, tw = tl & (T - 1);
        const int tap = (kh0 + g.s * th) * 4 + (kw0 + g.s * tw);
        const bool ok = on && kb < K;
        const int rowoff = tap * CaCb + a * g.Cb;
        const int base = voff(rowoff + ncol_off, ok);
        const int st = g.Cb * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) rb[i][e] = bload1(rP, base + e * st);
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < AI; ++i) *reinterpret_cast<f32x4*>(&As[(r0 + 32 * i) * LDK + kq * 4]) = ra[i];
#pragma unroll
        for (int i = 0; i < NQ; ++i) *reinterpret_cast<f32x4*>(&Bs[bn * LDK + 4 * (bg + BG * i)]) = rb[i];
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (c_begin < c_end) {
        next_a(c_begin);
#pragma unroll
        for (int i = 0; i < AI; ++i) load_a(i, true);
#pragma unroll
        for (int i = 0; i < NQ; ++i) load_b(i, c_begin, true);
        store_chunk();
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = (c + 1 < c_end);
        next_a(c + 1);
#pragma unroll
        for (int kk = 0; kk < KC / 8; ++kk) {
            f32x4 af[MR], bf[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i)
                af[i] = *reinterpret_cast<const f32x4*>(&As[((wm * MR + i) * 32 + lrow) * LDK + kk * 8 + lh * 4]);
#pragma unroll
            for (int j = 0; j < NR; ++j)
                bf[j] = *reinterpret_cast<const f32x4*>(&Bs[((wn * NR + j) * 32 + lrow) * LDK + kk * 8 + lh * 4]);
            if (kk < AI) load_a(kk, more);
            if (kk < NQ) load_b(kk, c + 1, more);
            PIN_VMEM();
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < MR; ++i)
#pragma unroll
                    for (int j = 0; j < NR; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            store_chunk();
            __syncthreads();
        }
    }

    const bool fin = (slab_stride == 0);
    float* o = out + (long)slice * slab_stride;
    const int ldo = fin ? ld_out : g.Cb;
    float bv[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int col = n0 + (wn * NR + j) * 32 + lrow;
        bv[j] = (fin && bias != nullptr && col < g.Cb) ? bias[col] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < MR; ++i) {
        // decode the lane's first row with two divisions, then walk the other 15 (at most 28 rows further) with a
        // carry chain: 64 divisions per thread in the epilogue cost as much as several K-chunks
        const int mb = m0 + (wm * MR + i) * 32 + 4 * lh;
        const int mbc = min(mb, Mc - 1);
        const int nb0 = mbc / (Hc * Wc);
        const int remb = mbc - nb0 * (Hc * Wc);
        const int ib0 = remb / Wc, jb0 = remb - ib0 * Wc;
        const bool chain = Wc >= 16 && Hc >= 2;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int m = m0 + (wm * MR + i) * 32 + row;
            if (m < Mc) {
                int n, ii, jj;
                if (chain) {
                    const int d = (r & 3) + 8 * (r >> 2);      // 0..27 rows past the decoded one
                    jj = jb0 + d;
                    ii = ib0;
                    n = nb0;
                    bool w1 = jj >= Wc;
                    jj = w1 ? jj - Wc : jj;
                    ii = w1 ? ii + 1 : ii;
                    w1 = jj >= Wc;
                    jj = w1 ? jj - Wc : jj;
                    ii = w1 ? ii + 1 : ii;
                    w1 = ii >= Hc;
                    ii = w1 ? ii - Hc : ii;
                    n = w1 ? n + 1 : n;
                } else {
                    n = m / (Hc * Wc);
                    const int rem = m - n * (Hc * Wc);
                    ii = rem / Wc;
                    jj = rem - ii * Wc;
                }
                const int h = (g.s == 2) ? 2 * ii + ah : ii, w = (g.s == 2) ? 2 * jj + aw : jj;
                float* orow = o + (long)((n * g.Hb + h) * g.Wb + w) * ldo;
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    const int col = n0 + (wn * NR + j) * 32 + lrow;
                    if (col < g.Cb) {
                        float v = acc[i][j][r];
                        if (fin) v = pg_act_epi(v + bv[j], act);
                        orow[col] = v;
                    }
                }
            }
        }
    }
}

template <int MR, int NR, int WM, int WN, bool POW2>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_wgrad_fast(const float* __restrict__ small, int ld_small,
                                                    const float* __restrict__ big, int ld_big,
                                                    float* __restrict__ out, long slab_stride, Geom g,
                                                    int chunks_per_slice, int tilesB, int small_bytes, int big_bytes) {
    constexpr int BM = WM * MR * 32, BN = WN * NR * 32;
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int AQ = BM / 4, AROWS = 256 / AQ, AI = KC / AROWS;
    constexpr int BQ = BN / 4, BROWS = 256 / BQ, BI = KC / BROWS;
    __shared__ __attribute__((aligned(16))) float smem[KC * LDA + KC * LDB];
    float* As = smem;
    float* Bs = smem + KC * LDA;
    const __amdgpu_buffer_rsrc_t rsm = __builtin_amdgcn_make_buffer_rsrc((void*)small, 0, small_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rbig = __builtin_amdgcn_make_buffer_rsrc((void*)big, 0, big_bytes, 0x00020000);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lrow = lane & 31, lh = lane >> 5;
    const int tile_a = blockIdx.x / tilesB, tile_b = blockIdx.x % tilesB;
    const int m0 = tile_a * BM, n0 = tile_b * BN;
    const int tap = blockIdx.y, kh = tap >> 2, kw = tap & 3;
    const int Kp = g.N * g.Hs * g.Ws;
    const int nchunks = (Kp + KC - 1) / KC;
    const int c_begin = blockIdx.z * chunks_per_slice;
    const int c_end = min(nchunks, c_begin + chunks_per_slice);

    const int aq = tid % AQ, arow0 = tid / AQ;
    const int bq = tid % BQ, brow0 = tid / BQ;
    const int a_col = (m0 + aq * 4 < g.Ca) ? m0 + aq * 4 : 0x10000000;      // small rows beyond Kp are out of range by
    const int b_col = (n0 + bq * 4 < g.Cb) ? n0 + bq * 4 : 0x10000000;      // construction of small_bytes
    // pixel -> (img, p, q): shifts when Hs, Ws are powers of two (every UNet layer), else a branch-free carry chain
    // (needs Ws >= 16 and Hs >= 2: a step of KC = 32 pixels wraps q at most twice and p at most once)
    const int lgW = 31 - __builtin_clz(g.Ws), lgH = 31 - __builtin_clz(g.Hs);
    int r_n[BI], r_p[BI], r_q[BI];
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        const int pix = c_begin * KC + brow0 + BROWS * i;
        r_n[i] = pix / (g.Hs * g.Ws);
        const int rem = pix - r_n[i] * (g.Hs * g.Ws);
        r_p[i] = rem / g.Ws;
        r_q[i] = rem - r_p[i] * g.Ws;
    }

    f32x4 ra[AI], rb[BI];
    auto load_a = [&](int i, int c, bool on) {
        const int pix = c * KC + arow0 + AROWS * i;
        const bool ok = on && pix < Kp;
        ra[i] = bload4(rsm, voff(pix * ld_small + a_col, ok));
    };
    auto load_b = [&](int i, int c, bool on) {
        const int pix = c * KC + brow0 + BROWS * i;
        int n, p, q;
        if (POW2) {
            q = pix & (g.Ws - 1);
            p = (pix >> lgW) & (g.Hs - 1);
            n = pix >> (lgW + lgH);
        } else {
            n = r_n[i];
            p = r_p[i];
            q = r_q[i];
            int nq = q + KC, np = p, nn = n;
            bool w = nq >= g.Ws;
            nq = w ? nq - g.Ws : nq;
            np = w ? np + 1 : np;
            w = nq >= g.Ws;
            nq = w ? nq - g.Ws : nq;
            np = w ? np + 1 : np;
            w = np >= g.Hs;
            np = w ? np - g.Hs : np;
            nn = w ? nn + 1 : nn;
            r_q[i] = nq;
            r_p[i] = np;
            r_n[i] = nn;
        }
        const int h = g.s * p - 1 + kh, w = g.s * q - 1 + kw;
        const bool ok = on && pix < Kp && (unsigned)h < (unsigned)g.Hb && (unsigned)w < (unsigned)g.Wb;
        rb[i] = bload4(rbig, voff(((n * g.Hb + h) * g.Wb + w) * ld_big + b_col, ok));
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < AI; ++i) *reinterpret_cast<f32x4*>(&As[(arow0 + AROWS * i) * LDA + aq * 4]) = ra[i];
#pragma unroll
        for (int i = 0; i < BI; ++i) *reinterpret_cast<f32x4*>(&Bs[(brow0 + BROWS * i) * LDB + bq * 4]) = rb[i];
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (c_begin < c_end) {
#pragma unroll
        for (int i = 0; i < AI; ++i) load_a(i, c_begin, true);
#pragma unroll
        for (int i = 0; i < BI; ++i) load_b(i, c_begin, true);
        store_chunk();
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = (c + 1 < c_end);
#pragma unroll
        for (int kq4 = 0; kq4 < 4; ++kq4) {          // 4 groups of 4 k-pairs
            if (kq4 < AI) load_a(kq4, c + 1, more);
            if (kq4 < BI) load_b(kq4, c + 1, more);
            if (kq4 + 4 < AI) load_a(kq4 + 4, c + 1, more);
            if (kq4 + 4 < BI) load_b(kq4 + 4, c + 1, more);
            PIN_VMEM();
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const int kk = kq4 * 4 + k4;
                float af[MR], bf[NR];
#pragma unroll
                for (int i = 0; i < MR; ++i) af[i] = As[(kk * 2 + lh) * LDA + (wm * MR + i) * 32 + lrow];
#pragma unroll
                for (int j = 0; j < NR; ++j) bf[j] = Bs[(kk * 2 + lh) * LDB + (wn * NR + j) * 32 + lrow];
#pragma unroll
                for (int i = 0; i < MR; ++i)
#pragma unroll
                    for (int j = 0; j < NR; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();
        if (more) {
            store_chunk();
            __syncthreads();
        }
    }

    float* o = out + (long)blockIdx.z * slab_stride + (long)tap * g.Ca * g.Cb;
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int col = n0 + (wn * NR + j) * 32 + lrow;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int a = m0 + (wm * MR + i) * 32 + row;
                if (a < g.Ca && col < g.Cb) o[(long)a * g.Cb + col] = acc[i][j][r];
            }
        }
}


// ------------------------------------------------------------------------------------------------
// big2small for image-facing layers with 1..3 (5..8: 64-pixel tiles) big-side channels (enc0 / d0 forward, dec6 data gradient):
// the whole contraction K = 16*CB <= 48 (128) fits one LDS tile, so the kernel is one shot -- gather 128 pixels x K and 64 x K weights,
// one barrier, K/2 MFMAs per 32x32 tile, bias + activation, store -- and is bound by the HBM write of its output.
// ------------------------------------------------------------------------------------------------
template <int CB, int MI = 2>      // MI: 32-row MFMA tiles per wave: 128 (CB <= 4) or 64 (CB <= 8, K <= 128) pixels per workgroup
__global__ __launch_bounds__(256) void k_b2s_tapk(const float* __restrict__ big, int ld_big, const float* __restrict__ P,
                                                  float* __restrict__ out, int ld_out, Geom g, const float* __restrict__ bias,
                                                  int act, int vec4, int vec_out) {
    constexpr int K = 16 * CB, LDT = K + 4, TM = 64 * MI;
    __shared__ __attribute__((aligned(16))) float smem[(TM + 64) * LDT];
    float* As = smem;
    float* Bs = smem + TM * LDT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lrow = lane & 31, lh = lane >> 5;
    const int M = g.N * g.Hs * g.Ws;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * 64;
    // A: TM pixels x 16 taps, one (pixel, tap) item = CB consecutive floats; a thread owns one pixel and 8 (4) taps
    {
        constexpr int TPT = 16 * TM / 256;
        const int r = tid & (TM - 1), t0 = (tid / TM) * TPT;
        const int m = m0 + r;
        const int mm = min(m, M - 1);
        const int n = mm / (g.Hs * g.Ws);
        const int rem = mm - n * (g.Hs * g.Ws);
        const int p = rem / g.Ws, q = rem - p * g.Ws;
        const int h0 = g.s * p - 1, w0 = g.s * q - 1;
        const float* base = big + ((long)(n * g.Hb + h0) * g.Wb + w0) * ld_big;
#pragma unroll
        for (int tt = 0; tt < TPT; ++tt) {
            const int tap = t0 + tt, kh = tap >> 2, kw = tap & 3;
            const bool ok = m < M && (unsigned)(h0 + kh) < (unsigned)g.Hb && (unsigned)(w0 + kw) < (unsigned)g.Wb;
            const float* src = base + ((long)kh * g.Wb + kw) * ld_big;
            float* dst = &As[r * LDT + tap * CB];
            if (CB == 4 && vec4) {
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(dst) = ok ? *reinterpret_cast<const f32x4*>(src) : z;
            } else {
#pragma unroll
                for (int c = 0; c < CB; ++c) dst[c] = ok ? src[c] : 0.f;
            }
        }
    }
    // B: 64 output channels x K, Bs[a][tap*CB + c] = P[(tap*Ca + a)*CB + c]
    for (int item = tid; item < 64 * 16; item += 256) {
        const int a = item & 63, tap = item >> 6;
        const bool ok = n0 + a < g.Ca;
#pragma unroll
        for (int c = 0; c < CB; ++c) Bs[a * LDT + tap * CB + c] = ok ? P[((long)tap * g.Ca + n0 + a) * CB + c] : 0.f;
    }
    __syncthreads();
    f32x16 acc[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < K / 8; ++kk) {
        f32x4 af[MI], bf;
#pragma unroll
        for (int i = 0; i < MI; ++i) af[i] = *reinterpret_cast<const f32x4*>(&As[((wm * MI + i) * 32 + lrow) * LDT + kk * 8 + lh * 4]);
        bf = *reinterpret_cast<const f32x4*>(&Bs[(wn * 32 + lrow) * LDT + kk * 8 + lh * 4]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < MI; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[e], af[i][e], acc[i], 0, 0, 0);   // D[channel][pixel]
    }
    // transposed product (weights as the A operand): a lane owns pixel lrow of its tile and, per accumulator quad, 4 consecutive
    // channels -- one 16-byte store instead of four 4-byte ones (the kernel is bound by its output stores)
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int m = m0 + (wm * MI + i) * 32 + lrow;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ch = n0 + wn * 32 + 8 * q + 4 * lh;
            if (m >= M || ch >= g.Ca) continue;
            if (vec_out) {
                f32x4 bv = {0.f, 0.f, 0.f, 0.f};
                if (bias != nullptr) bv = *reinterpret_cast<const f32x4*>(bias + ch);
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = pg_act_epi(acc[i][4 * q + e] + bv[e], act);
                *reinterpret_cast<f32x4*>(out + (long)m * ld_out + ch) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (ch + e < g.Ca) out[(long)m * ld_out + ch + e] = pg_act_epi(acc[i][4 * q + e] + (bias != nullptr ? bias[ch + e] : 0.f), act);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The same layers (1..4 big-side channels) as a PERSISTENT, software-pipelined kernel.  The one-shot form above serialises, per
// workgroup, gather -> LDS -> 64 MFMAs per wave -> stores, and the co-resident workgroups of a CU run those phases in lockstep:
// measured on d0 at batch 32 (ablation builds, tools/ab_tapkp.sh) the phase times simply ADD -- 19 us of loads / staging, 28 us of
// MFMAs (= the fp32 MFMA peak for the layer's 4.3 GFLOP) and 17 us of stores give the 67-77 us of the launch: nothing overlaps.
// Here ONE wave keeps all three in flight: a workgroup holds its weight FRAGMENTS in registers for its whole life, walks pixel
// tiles t = blockIdx.x, + gridDim.x, ... (neighbouring workgroups work on neighbouring tiles: the 4-row input windows overlap in
// L2) with two accumulator sets and two LDS buffers, and inside the MFMA sequence of tile t it issues, one group per k-step,
// the bias / activation / 16-byte stores of tile t - 1 (the other accumulator set), while the gather loads of tile t + 1 are in
// flight; their LDS stores go to the other buffer after the last MFMA has been issued.  One barrier per tile.
// ------------------------------------------------------------------------------------------------
// Branch-free: gathers are raw buffer loads whose offset is forced out of range for padding / ragged rows (the hardware returns 0),
// stores are raw buffer stores dropped the same way, the activation is a template parameter -- the whole tile step is ONE basic block,
// so hipcc keeps the interleave below (an earlier form with `ok ? *src : 0` loads compiled to a branch and an `s_waitcnt vmcnt(0)` per
// load: the phases ran strictly one after the other again).
// ACT: 0 none, 1 LeakyReLU(0.2) (other activations: the one-shot kernel).  WIDE: one 16-byte load per tap (CB == 4, or CB == 3 inside
// pixels of stride % 4 == 0: the 4th float is dropped), else CB scalar loads.
// STATS (K5: InstanceNorm statistics from the conv epilogue, unet.py:19-20; ACT == 0, no bias): next to the stores of a finished tile each
// wave also emits the sums / sums of squares of ITS 64 pixels x 32 channels -- a lane adds its two row tiles (fp32: one rounding per
// pair), the 64 lanes exchange them through a wave-private LDS patch, lane (slot, half) sums 32 pixels in fp64 and writes
// part[((n * chunks + chunk) * Ca + c) * 2 + {0, 1}], chunk = 2 * (tile within the sample) + wm.  Tiles never straddle samples
// (Hs * Ws % 128 == 0, checked by the host); fixed order, deterministic.
template <int CB, int ACT, bool WIDE, bool STATS = false>
__global__ __launch_bounds__(256, STATS ? 1 : 2) void k_b2s_tapkp(const float* __restrict__ big, int ld_big, const float* __restrict__ P,
                                                      float* __restrict__ out, int ld_out, Geom g, const float* __restrict__ bias,
                                                      int big_bytes, int out_bytes, int ntiles, double* __restrict__ part = nullptr) {
    constexpr int K = 16 * CB, LDT = K + 4, TM = 128, MI = 2, TPT = 8, NKK = K / 8, PC = WIDE ? 4 : CB;
    constexpr int SROW = 68;       // stats patch: 32 value slots x (64 lanes + 4 pad) floats per wave
    __shared__ __attribute__((aligned(16))) float smem[2 * TM * LDT + (STATS ? 4 * 32 * SROW : 0)];
    const __amdgpu_buffer_rsrc_t rbig = __builtin_amdgcn_make_buffer_rsrc((void*)big, 0, big_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, out_bytes, 0x00020000);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lrow = lane & 31, lh = lane >> 5;
    const int M = g.N * g.Hs * g.Ws, HWs = g.Hs * g.Ws;
    const int n0 = blockIdx.y * 64;
    // weight fragments of this wave's 32 output channels, for the whole kernel: bfr[kk][e] = W[a][k = 8 kk + 4 lh + e], k = tap * CB + c
    f32x4 bfr[NKK];
    {
        const int a = min(n0 + wn * 32 + lrow, g.Ca - 1);        // (rows beyond Ca are computed and never stored)
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            if (CB == 4) {                 // k = 4 tap + c with tap = 2 kk + lh: the tap's four channels are 16 contiguous, aligned bytes
                bfr[kk] = *reinterpret_cast<const f32x4*>(P + ((long)(2 * kk + lh) * g.Ca + a) * 4);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = kk * 8 + lh * 4 + e, tap = k / CB, c = k - tap * CB;
                    bfr[kk][e] = P[((long)tap * g.Ca + a) * CB + c];
                }
            }
        }
    }
    // bias of this lane's four channel quads (channels n0 + 32 wn + 8 q + 4 lh .. + 3; Ca % 4 == 0)
    f32x4 bv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ch = min(n0 + wn * 32 + 8 * q + 4 * lh, g.Ca - 4);
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        bv[q] = bias != nullptr ? *reinterpret_cast<const f32x4*>(bias + ch) : z;
    }
    // gather role of this thread: pixel r of the tile, taps t0 .. t0 + 7 (16 * 128 items / 256 threads)
    const int r = tid & (TM - 1), t0 = (tid / TM) * TPT;
    float pre[TPT][PC];
    auto gather = [&](int tile) {
        const int m = tile * TM + r;
        const int mm = min(m, M - 1);
        const int n = mm / HWs;
        const int rem = mm - n * HWs;
        const int p = rem / g.Ws, q = rem - p * g.Ws;
        const int h0 = g.s * p - 1, w0 = g.s * q - 1;
        const int base = ((n * g.Hb + h0) * g.Wb + w0) * ld_big;       // element offset of the window's first pixel (may be negative: masked)
#pragma unroll
        for (int tt = 0; tt < TPT; ++tt) {
            const int tap = t0 + tt, kh = tap >> 2, kw = tap & 3;
            const bool ok = (m < M) & ((unsigned)(h0 + kh) < (unsigned)g.Hb) & ((unsigned)(w0 + kw) < (unsigned)g.Wb);
            const int eo = base + (kh * g.Wb + kw) * ld_big;
            if (WIDE) {
                const f32x4 v = bload4(rbig, voff(eo, ok));
#pragma unroll
                for (int c = 0; c < 4; ++c) pre[tt][c] = v[c];
            } else {
#pragma unroll
                for (int c = 0; c < CB; ++c) pre[tt][c] = bload1(rbig, voff(eo + c, ok));
            }
        }
    };
    auto stage = [&](float* As) {
#pragma unroll
        for (int tt = 0; tt < TPT; ++tt) {
            float* dst = &As[r * LDT + (t0 + tt) * CB];
            if (CB == 4) {
                f32x4 v;
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = pre[tt][c];
                *reinterpret_cast<f32x4*>(dst) = v;
            } else {
#pragma unroll
                for (int c = 0; c < CB; ++c) dst[c] = pre[tt][c];
            }
        }
    };
    // store group gi = (i, q) of a finished tile: pixel lrow of row tile i, channels 8 q + 4 lh .. + 3 of this wave's 32
    auto store_group = [&](const f32x16 (&ac)[MI], int tile_done, int gi) {
        const int i = gi >> 2, q = gi & 3;
        const int m = tile_done * TM + (wm * MI + i) * 32 + lrow;
        const int ch = n0 + wn * 32 + 8 * q + 4 * lh;
        const bool ok = (m < M) & (ch < g.Ca);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x = ac[i][4 * q + e] + bv[q][e];
            v[e] = ACT == 1 ? (x > 0.f ? x : 0.2f * x) : x;
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rout, voff(m * ld_out + ch, ok), 0, 0);
    };
    // STATS: the two halves of the exchange (wave-private LDS patch: program order + lgkmcnt order them, no barrier)
    float* spatch = smem + 2 * TM * LDT + wave * 32 * SROW;
    auto stats_put = [&](const f32x16 (&ac)[MI]) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            spatch[j * SROW + lane] = ac[0][j] + ac[1][j];
            spatch[(16 + j) * SROW + lane] = __builtin_fmaf(ac[0][j], ac[0][j], ac[1][j] * ac[1][j]);
        }
    };
    auto stats_get = [&](int tile_done) {
        // this lane: slot v = lane & 31 (0..15: sum of accumulator register v, 16..31: its squares), half h = lane >> 5 of the writers
        const int v = lane & 31, h = lane >> 5;
        double sum = 0.0;
#pragma unroll
        for (int p4 = 0; p4 < 8; ++p4) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(&spatch[v * SROW + h * 32 + p4 * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) sum += (double)t[e];
        }
        const int rr = v & 15;
        const int ch = n0 + wn * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * h;
        const int tps = HWs / TM;                              // tiles per sample
        const int n = tile_done / tps, chunk = 2 * (tile_done - n * tps) + wm;
        if (tile_done < ntiles && ch < g.Ca) part[(((long)n * (2 * tps) + chunk) * g.Ca + ch) * 2 + (v >> 4)] = sum;
    };
    // one tile: MFMAs of `tile` from As into `cur`, the stores of `prev_tile` (accumulators `prev`) woven between the k-steps, then
    // the next tile's staged registers into the other LDS buffer
    auto step = [&](f32x16 (&cur)[MI], const f32x16 (&prev)[MI], int prev_tile, const float* As, float* As_next, int next2) {
        if (STATS) stats_put(prev);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) cur[i][rr] = 0.f;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            f32x4 af[MI];
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = *reinterpret_cast<const f32x4*>(&As[((wm * MI + i) * 32 + lrow) * LDT + kk * 8 + lh * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < MI; ++i) cur[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(bfr[kk][e], af[i][e], cur[i], 0, 0, 0);   // D[channel][pixel]
#pragma unroll
            for (int gi = (kk * 8) / NKK; gi < ((kk + 1) * 8) / NKK; ++gi) store_group(prev, prev_tile, gi);
            if (STATS && kk == NKK / 2) stats_get(prev_tile);
            __builtin_amdgcn_sched_barrier(0);         // keep the stores of the previous tile BETWEEN the MFMA groups
        }
        stage(As_next);            // (registers of the tile after this one; zeros beyond the last tile)
        __syncthreads();           // As_next is complete; every wave is done reading As (it is overwritten one step later)
        gather(next2);             // the tile two steps ahead (>= ntiles: every load out of range, no traffic)
    };
    float* A0 = smem;
    float* A1 = smem + TM * LDT;
    f32x16 accA[MI], accB[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) accB[i][rr] = 0.f;
    const int G = gridDim.x, big_tile = 0x3fffff;      // big_tile * TM >= M: every row masked
    int tile = blockIdx.x;
    gather(tile);
    stage(A0);
    __syncthreads();
    gather(tile + G < ntiles ? tile + G : big_tile);
    int prev_tile = big_tile;      // nothing to store in the first step
    for (;;) {
        step(accA, accB, prev_tile, A0, A1, tile + 2 * G < ntiles ? tile + 2 * G : big_tile);
        prev_tile = tile;
        tile += G;
        if (tile >= ntiles) {
#pragma unroll
            for (int gi = 0; gi < 8; ++gi) store_group(accA, prev_tile, gi);
            if (STATS) {
                stats_put(accA);
                stats_get(prev_tile);
            }
            break;
        }
        step(accB, accA, prev_tile, A1, A0, tile + 2 * G < ntiles ? tile + 2 * G : big_tile);
        prev_tile = tile;
        tile += G;
        if (tile >= ntiles) {
#pragma unroll
            for (int gi = 0; gi < 8; ++gi) store_group(accB, prev_tile, gi);
            if (STATS) {
                stats_put(accB);
                stats_get(prev_tile);
            }
            break;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient of the same image-facing layers (enc0, d0: Cb = 3 / 4; dec6: Cb = output_nc) with the 16 taps folded into N, as a
// PERSISTENT kernel: dP[(tap, b)][a] = sum_pix small[pix][a] * big[window(pix), tap][b].  The taps-in-N kernel k_wgrad_tapn<.., 1> cuts
// the pixel dimension into ~1000 slices of 8 chunks (one 16-KB slab each, a 16-MB reduce) and every workgroup pays a prologue and an
// epilogue for 256 pixels; it ran at 45-74 us on layers whose MFMA and HBM times are ~15 us each.  Here <= 512 workgroups walk
// 128-pixel tiles t = blockIdx.x, + gridDim.x, ..., accumulate their BM x BN block of dP over all of them in ONE accumulator set,
// and write one slab at the end (fixed-order reduce over the workgroups as before: deterministic).  Per tile: the small-side tile
// [128 pixels][BM channels] (contiguous rows) and the gathered window tile [128 pixels][16 CB] come through registers (branch-free
// buffer loads, issued for tile t + 1 before the MFMAs of tile t) into LDS; both MFMA operands are read with ds_read_b32 (pixel =
// the MFMA's k index).  WM x WN waves: 2 x 2 (64 channels x 64 columns) for CB >= 3, 4 x 1 (128 channels x 32 columns) for CB <= 2.
// ------------------------------------------------------------------------------------------------
template <int CB, bool WIDE, int WM>
__global__ __launch_bounds__(256, 2) void k_wgrad_tapnp(const float* __restrict__ small, int ld_small, const float* __restrict__ big,
                                                        int ld_big, float* __restrict__ slabs, long slab_stride, Geom g,
                                                        int small_bytes, int big_bytes, int ntiles) {
    constexpr int WN = 4 / WM, BM = 32 * WM, K = 16 * CB, TM = 128, TPT = 8, PC = WIDE ? 4 : CB;
    constexpr int LDA = BM + 4, LDB = 32 * WN + 4;          // (columns >= K of the window tile are zero)
    constexpr int AQ = BM / 4, ALD = TM * AQ / 256;         // float4 loads of the small-side tile per thread
    __shared__ __attribute__((aligned(16))) float smem[TM * LDA + TM * LDB];
    float* As = smem;
    float* Bs = smem + TM * LDA;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)small, 0, small_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)big, 0, big_bytes, 0x00020000);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lrow = lane & 31, lh = lane >> 5;
    const int M = g.N * g.Hs * g.Ws, HWs = g.Hs * g.Ws;
    const int a0 = blockIdx.y * BM;
    // the window tile's pad columns are written once
    for (int i = tid; i < TM * LDB; i += 256) Bs[i] = 0.f;
    __syncthreads();
    const int r = tid & (TM - 1), t0 = (tid / TM) * TPT;    // gather role: pixel r of the tile, taps t0 .. t0 + 7
    f32x4 pa[ALD];
    float pb[TPT][PC];
    auto fetch = [&](int tile) {
#pragma unroll
        for (int i = 0; i < ALD; ++i) {
            const int idx = tid + 256 * i, pix = idx / AQ, q4 = idx - pix * AQ;
            const int m = tile * TM + pix, a = a0 + q4 * 4;
            pa[i] = bload4(rs, voff(m * ld_small + a, (m < M) & (a < g.Ca)));
        }
        const int m = tile * TM + r;
        const int mm = min(m, M - 1);
        const int n = mm / HWs;
        const int rem = mm - n * HWs;
        const int p = rem / g.Ws, q = rem - p * g.Ws;
        const int h0 = g.s * p - 1, w0 = g.s * q - 1;
        const int base = ((n * g.Hb + h0) * g.Wb + w0) * ld_big;
#pragma unroll
        for (int tt = 0; tt < TPT; ++tt) {
            const int tap = t0 + tt, kh = tap >> 2, kw = tap & 3;
            const bool ok = (m < M) & ((unsigned)(h0 + kh) < (unsigned)g.Hb) & ((unsigned)(w0 + kw) < (unsigned)g.Wb);
            const int eo = base + (kh * g.Wb + kw) * ld_big;
            if (WIDE) {
                const f32x4 v = bload4(rb, voff(eo, ok));
#pragma unroll
                for (int c = 0; c < 4; ++c) pb[tt][c] = v[c];
            } else {
#pragma unroll
                for (int c = 0; c < CB; ++c) pb[tt][c] = bload1(rb, voff(eo + c, ok));
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < ALD; ++i) {
            const int idx = tid + 256 * i, pix = idx / AQ, q4 = idx - pix * AQ;
            *reinterpret_cast<f32x4*>(&As[pix * LDA + q4 * 4]) = pa[i];
        }
#pragma unroll
        for (int tt = 0; tt < TPT; ++tt) {
            float* dst = &Bs[r * LDB + (t0 + tt) * CB];
            if (CB == 4) {
                f32x4 v;
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = pb[tt][c];
                *reinterpret_cast<f32x4*>(dst) = v;
            } else {
#pragma unroll
                for (int c = 0; c < CB; ++c) dst[c] = pb[tt][c];
            }
        }
    };
    f32x16 acc;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.f;
    const int G = gridDim.x, big_tile = 0x3fffff;
    int tile = blockIdx.x;
    fetch(tile);
    for (; tile < ntiles; tile += G) {
        stage();
        __syncthreads();
        fetch(tile + G < ntiles ? tile + G : big_tile);     // in flight under the MFMAs below (beyond the last tile: every load masked)
        __builtin_amdgcn_sched_barrier(0x386);
#pragma unroll 16
        for (int s2 = 0; s2 < TM / 2; ++s2) {
            const float af = As[(2 * s2 + lh) * LDA + wm * 32 + lrow];
            const float bf = Bs[(2 * s2 + lh) * LDB + wn * 32 + lrow];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf, acc, 0, 0, 0);          // D[channel a][column (tap, b)]
        }
        __syncthreads();
    }
    // one slab per workgroup column: slab[(tap * Ca + a) * Cb + b]
    float* o = slabs + (long)blockIdx.x * slab_stride;
    const int col = wn * 32 + lrow;
    if (col < K) {
        const int tap = col / CB, b = col - tap * CB;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int a = a0 + wm * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (a < g.Ca) o[((long)tap * g.Ca + a) * CB + b] = acc[rr];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// ConvTranspose2d(4, 2, 1) onto <= 4 channels (the generator's head dec6, the discriminator's first-layer data gradient) in ONE pass,
// taps folded into N:
//     D[p][(b, tap)] = small[p][:] . P[tap][:][b]                      (MFMA 16x16x4: rows = small pixels, one 16-column tile = the 16
//                                                                       taps of output channel b)
//     big[n, h, w, b] = act(bias[b] + the four D entries that reach (h, w))
// The two-launch form (row GEMM k_b2s_fast<.., true> + k_col2im_s2_lds) writes D to HBM and reads it back: 16.8 / 67 MB each way at
// batch 16, 57 / 70 us for layers whose own traffic is 138 / 84 MB (22 / 13 us).  Here a workgroup owns a TF_H x TF_W block of small
// pixels of one sample, keeps its D block in LDS, and writes the (2 TF_H - 2) x (2 TF_W - 2) output pixels all of whose four taps lie
// inside the block; blocks step by TF_H - 1 / TF_W - 1 small pixels (one row / column of every block is recomputed by its
// neighbour: 18 % more MFMA work on a memory-bound kernel, re-read from L2), and start at small pixel -1 (zeros) so the image border
// needs no special case.  PERSISTENT: <= 512 workgroups walk blocks blockIdx.x, + gridDim.x, ...; the lanes' operand rows come
// straight from global memory in MFMA fragment order (lane (pixel r, k group q) loads 16 bytes = 4 consecutive channels, which feed
// four MFMAs; the matching weight fragments are read from an LDS image of P with the same k order), no LDS staging of `small`, and
// block t + 1's loads are issued before block t's MFMAs (two register sets).
// ------------------------------------------------------------------------------------------------
constexpr int TF_H = 8, TF_W = 16;
typedef __bf16 tf_bf16x8 __attribute__((ext_vector_type(8)));
// BF: `small` is a bf16 tensor (PG_ALGO_BF16 with bf16 activation storage): a lane's 16 bytes are 8 consecutive channels = its operand of
// one v_mfma_f32_16x16x32_bf16, the weights are rounded to bf16 as they are laid into LDS ([(b, tap)][k], k contiguous), fp32 accumulation
// and an fp32 result as everywhere in that mode.  KK = operand loads per pixel: Ca / 16 (fp32) or Ca / 32 (bf16).
template <int CB, int KK, bool BF>
__global__ __launch_bounds__(256, 2) void k_s2b_tapnf(const void* __restrict__ small_v, int ld_small, const float* __restrict__ P,
                                                      const float* __restrict__ bias, float* __restrict__ big, int ld_big, Geom g, int act,
                                                      int small_bytes, int big_bytes, int nbh, int nbw, int nblocks, int vec4, int cb_total,
                                                      int b0) {
    // (5 .. 8 output channels run as two launches: channels b0 .. b0 + CB - 1 of cb_total each)
    constexpr int Ca = (BF ? 32 : 16) * KK;
    constexpr int SK = 16 * CB + 4;      // fp32: k-row pitch of the weight image: the four k groups of a fragment read land in four bank quarters
    constexpr int SKB = Ca + 8;          // bf16: (b, tap)-row pitch in elements (16 bytes of padding: conflict-free ds_read_b128 per 16 lanes)
    // D block in LDS: [pixel][tap][channel], so a lane's CB channels of one (pixel, tap) are one ds_write / one ds_read (CB = 4: 16 bytes)
    constexpr int SD = (CB % 4 == 0) ? 16 * CB + 4 : (CB % 2 == 0) ? 16 * CB + 2 : 16 * CB + 1;
    constexpr int OH = 2 * TF_H - 2, OW = 2 * TF_W - 2;
    constexpr int BS_BYTES = BF ? 16 * CB * SKB * 2 : Ca * SK * 4;
    __shared__ __attribute__((aligned(16))) char Bs_raw[BS_BYTES];
    __shared__ __attribute__((aligned(16))) float Ds[TF_H * TF_W * SD];
    float* const Bs = reinterpret_cast<float*>(Bs_raw);
    __bf16* const Bh = reinterpret_cast<__bf16*>(Bs_raw);
    const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc((void*)small_v, 0, small_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc((void*)big, 0, big_bytes, 0x00020000);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, q = lane >> 4;
    for (int i = tid; i < Ca * CB * 16; i += 256) {
        if constexpr (BF) {                                  // Bh[(b, tap)][k] = bf16(P[tap][k][b])
            const int k = i % Ca, bt = i / Ca, tap = bt & 15, b = bt >> 4;
            Bh[bt * SKB + k] = (__bf16)P[((long)tap * Ca + k) * cb_total + b0 + b];
        } else {                                             // Bs[k][b][tap] = P[tap][k][b]
            const int tap = i & 15, b = (i >> 4) % CB, k = i / (16 * CB);
            Bs[k * SK + b * 16 + tap] = P[((long)tap * Ca + k) * cb_total + b0 + b];
        }
    }
    float bv[CB];
#pragma unroll
    for (int b = 0; b < CB; ++b) bv[b] = bias ? bias[b0 + b] : 0.f;
    __syncthreads();

    const int G = gridDim.x;
    int blk = xcd_remap(blockIdx.x, G);
    // this lane's two pixel rows of block `b`: rows 2 * wave + {0, 1} of the block, column c
    auto issue = [&](f32x4 (&a)[2][KK], int b) {
        const bool on = b < nblocks;
        const int bb = on ? b : 0;
        const int bj = bb % nbw, t = bb / nbw;
        const int bi = t % nbh, n = t / nbh;
        const int j = bj * (TF_W - 1) - 1 + c;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const int i = bi * (TF_H - 1) - 1 + 2 * wave + rt;
            const bool ok = on && (unsigned)i < (unsigned)g.Hs && (unsigned)j < (unsigned)g.Ws;
            const int off = ((n * g.Hs + i) * g.Ws + j) * ld_small + q * (BF ? 8 : 4);
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                if constexpr (BF)
                    a[rt][kk] = bload4(rS, (int)(((unsigned)(off + kk * 32) << 1) | (ok ? 0u : 0x80000000u)));
                else
                    a[rt][kk] = bload4(rS, voff(off + kk * 16, ok));
            }
        }
    };
    auto body = [&](f32x4 (&cur)[2][KK], f32x4 (&nxt)[2][KK], int b) {
        issue(nxt, b + G);
        PIN_VMEM();
        f32x4 acc[2][CB];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) acc[rt][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (BF) {
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                tf_bf16x8 bf[CB];
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) bf[cb] = *reinterpret_cast<const tf_bf16x8*>(Bh + (cb * 16 + c) * SKB + kk * 32 + q * 8);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb)
                        acc[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(tf_bf16x8, cur[rt][kk]), bf[cb], acc[rt][cb], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float bf[CB];
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb) bf[cb] = Bs[(kk * 16 + q * 4 + e) * SK + cb * 16 + c];
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                        for (int cb = 0; cb < CB; ++cb)
                            acc[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[rt][kk][e], bf[cb], acc[rt][cb], 0, 0, 0);
                }
        }
        // D block -> LDS: lane (tap c, group q) holds pixels 4 q + {0..3} of its two block rows
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                for (int e = 0; e < 4; ++e) Ds[((2 * wave + rt) * TF_W + q * 4 + e) * SD + c * CB + cb] = acc[rt][cb][e];
        __syncthreads();
        const int bj = b % nbw, t = b / nbw;
        const int bi = t % nbh, n = t / nbh;
        const int h0 = 2 * (bi * (TF_H - 1) - 1) + 1, w0 = 2 * (bj * (TF_W - 1) - 1) + 1;
        for (int o = tid; o < OH * OW; o += 256) {
            const int oh = o / OW, ow = o - oh * OW;
            const int h = h0 + oh, w = w0 + ow;
            // output row h0 + oh (h0 odd): oh even -> rows oh/2 (kh 2) and oh/2 + 1 (kh 0); oh odd -> rows (oh+1)/2 (kh 1) and (oh-1)/2 (kh 3)
            const int la = (oh + 1) >> 1, ka = (oh & 1) ? 1 : 2, lb = (oh & 1) ? la - 1 : la + 1, kb = (oh & 1) ? 3 : 0;
            const int ma = (ow + 1) >> 1, ua = (ow & 1) ? 1 : 2, mb = (ow & 1) ? ma - 1 : ma + 1, ub = (ow & 1) ? 3 : 0;
            const float* d00 = Ds + (la * TF_W + ma) * SD + (ka * 4 + ua) * CB;
            const float* d01 = Ds + (la * TF_W + mb) * SD + (ka * 4 + ub) * CB;
            const float* d10 = Ds + (lb * TF_W + ma) * SD + (kb * 4 + ua) * CB;
            const float* d11 = Ds + (lb * TF_W + mb) * SD + (kb * 4 + ub) * CB;
            const bool ok = (unsigned)h < (unsigned)g.Hb && (unsigned)w < (unsigned)g.Wb;
            const int eo = ((n * g.Hb + h) * g.Wb + w) * ld_big + b0;
            float v[CB];
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) v[cb] = pg_act_epi(bv[cb] + ((d00[cb] + d01[cb]) + (d10[cb] + d11[cb])), act);
            if (CB % 4 == 0 && vec4) {
#pragma unroll
                for (int c4 = 0; c4 < CB / 4; ++c4) {
                    const f32x4 o4 = {v[(4 * c4) % CB], v[(4 * c4 + 1) % CB], v[(4 * c4 + 2) % CB], v[(4 * c4 + 3) % CB]};
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o4), rO, voff(eo + 4 * c4, ok), 0, 0);
                }
            } else {
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v[cb]), rO, voff(eo + cb, ok), 0, 0);
            }
        }
        __syncthreads();
    };
    f32x4 A0[2][KK], A1[2][KK];
    issue(A0, blk);
    while (blk < nblocks) {
        body(A0, A1, blk);
        blk += G;
        if (blk >= nblocks) break;
        body(A1, A0, blk);
        blk += G;
    }
}

// ================================================================================================
// bf16 variants (PG_ALGO_BF16; the "next" row f2, BASELINE config 4): tensors stay fp32 in HBM and in the C ABI -- fp32
// master weights, fp32 InstanceNorm statistics, fp32 accumulation -- but operand tiles are rounded to bf16 (RNE,
// v_cvt_pk_bf16_f32) as they are staged into LDS and multiplied on v_mfma_f32_32x32x16_bf16 (16x the fp32 MFMA rate),
// which moves these kernels from MFMA-bound to load-bound.  Same tiling, gathers and split-K as the fast fp32 kernels.
// LDS rows are 32 bf16 + 8 pad = 80 B: conflict-free ds_read_b128 of a lane's 8 consecutive k.
// ================================================================================================
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
constexpr int LDKH = KC + 8;
__device__ __forceinline__ bf16x4 to_bf16(f32x4 v) {
    bf16x4 r;
    r[0] = (__bf16)v[0];
    r[1] = (__bf16)v[1];
    r[2] = (__bf16)v[2];
    r[3] = (__bf16)v[3];
    return r;
}

// bf16 activation storage: 8-byte loads of 4 bf16 (byte offset = element offset * 2), stored to LDS as they are
__device__ __forceinline__ bf16x4 bload2h(__amdgpu_buffer_rsrc_t r, int byte_off) {
    return __builtin_bit_cast(bf16x4, __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, 0));
}
__device__ __forceinline__ int voffh(int elem_off, bool ok) {
    return (int)(((unsigned)elem_off << 1) | (ok ? 0u : 0x80000000u));
}
// epilogue store of one value into an fp32 or a bf16 tensor (element index idx)
__device__ __forceinline__ void store_io(float* base, long idx, float v, int out_bf) {
    if (out_bf)
        reinterpret_cast<__bf16*>(base)[idx] = (__bf16)v;
    else
        base[idx] = v;
}

// HIN: the activation operand(s) are stored as bf16 in HBM (bf16 storage mode) instead of fp32 rounded in the kernel
template <int MR, int NR, int WM, int WN, bool ONE, bool HIN = false>
__global__ __launch_bounds__(256) void k_b2s_bf16(const float* __restrict__ big, int ld_big,
                                                  const float* __restrict__ P, float* __restrict__ out, int ld_out,
                                                  long slab_stride, Geom g, int chunks_per_slice,
                                                  const float* __restrict__ bias, int act, int big_bytes, int p_bytes, int out_bf) {
    constexpr int BM = WM * MR * 32, BN = WN * NR * 32;
    constexpr int AI = BM / 32, BI = BN / 32;
    __shared__ __attribute__((aligned(16))) __bf16 smem[(BM + BN) * LDKH];
    __bf16* As = smem;
    __bf16* Bs = smem + BM * LDKH;
    const __amdgpu_buffer_rsrc_t rbig = __builtin_amdgcn_make_buffer_rsrc((void*)big, 0, big_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rP = __builtin_amdgcn_make_buffer_rsrc((void*)P, 0, p_bytes, 0x00020000);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lrow = lane & 31, lh = lane >> 5;
    const int M = ONE ? g.N * g.Hb * g.Wb : g.N * g.Hs * g.Ws;
    const int K = ONE ? g.Cb : 16 * g.Cb;               // K % 32 == 0 (Cb % 4 == 0; ONE requires Cb % 32 == 0)
    const int m0 = xcd_remap(blockIdx.x, gridDim.x) * BM, n0 = blockIdx.y * BN;
    const int nchunks = K / KC;
    const int c_begin = blockIdx.z * chunks_per_slice;
    const int c_end = min(nchunks, c_begin + chunks_per_slice);

    const int kq = tid & 7, r0 = tid >> 3;
    int a_off[AI], a_mask[AI], b_off[BI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int m = m0 + r0 + 32 * i;
        const int mm = min(m, M - 1);
        if (ONE) {
            a_off[i] = mm * ld_big;
            a_mask[i] = (m < M) ? 1 : 0;
            continue;
        }
        const int n = mm / (g.Hs * g.Ws);
        const int rem = mm - n * (g.Hs * g.Ws);
        const int p = rem / g.Ws, q = rem - p * g.Ws;
        const int h0 = g.s * p - 1, w0 = g.s * q - 1;
        a_off[i] = ((n * g.Hb + h0) * g.Wb + w0) * ld_big;
        int wv = 0, mask = 0;          // tap (kh, kw) is inside the image iff row kh and column kw both are
#pragma unroll
        for (int t = 0; t < 4; ++t) wv |= ((unsigned)(w0 + t) < (unsigned)g.Wb) ? (1 << t) : 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) mask |= ((unsigned)(h0 + t) < (unsigned)g.Hb) ? (wv << (4 * t)) : 0;
        a_mask[i] = (m < M) ? mask : 0;
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        const int a = n0 + r0 + 32 * i;
        b_off[i] = (a < g.Ca) ? a * g.Cb : 0x10000000;
    }
    const int CaCb = g.Ca * g.Cb;
    int cur_tap = (c_begin * KC + kq * 4) / g.Cb;
    int cur_b = (c_begin * KC + kq * 4) - cur_tap * g.Cb;

    f32x4 ra[AI], rb[BI];
    bf16x4 rah[AI];
    int tapoff = 0, pboff = 0, ctap = 0;
    auto next_tap = [&]() {   // (tap, b) of the next chunk for this thread's float4; Cb >= KC: at most one wrap
        const int tap = cur_tap, b = cur_b;
        cur_b += KC;
        const bool wrap = cur_b >= g.Cb;
        cur_b = wrap ? cur_b - g.Cb : cur_b;
        cur_tap = wrap ? cur_tap + 1 : cur_tap;
        ctap = tap;
        tapoff = ((tap >> 2) * g.Wb + (tap & 3)) * ld_big + b;
        pboff = tap * CaCb + b;
    };
    auto load_a = [&](int i, bool on) {
        const bool ok = on && ((a_mask[i] >> ctap) & 1);
        if constexpr (HIN)
            rah[i] = bload2h(rbig, voffh(a_off[i] + tapoff, ok));
        else
            ra[i] = bload4(rbig, voff(a_off[i] + tapoff, ok));
    };
    auto load_b = [&](int i, bool on) { rb[i] = bload4(rP, voff(b_off[i] + pboff, on)); };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < AI; ++i) *reinterpret_cast<bf16x4*>(&As[(r0 + 32 * i) * LDKH + kq * 4]) = HIN ? rah[i] : to_bf16(ra[i]);
#pragma unroll
        for (int i = 0; i < BI; ++i) *reinterpret_cast<bf16x4*>(&Bs[(r0 + 32 * i) * LDKH + kq * 4]) = to_bf16(rb[i]);
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (c_begin < c_end) {
        next_tap();
#pragma unroll
        for (int i = 0; i < AI; ++i) load_a(i, true);
#pragma unroll
        for (int i = 0; i < BI; ++i) load_b(i, true);
        store_chunk();
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = (c + 1 < c_end);
        next_tap();
#pragma unroll
        for (int i = 0; i < AI; ++i) load_a(i, more);
#pragma unroll
        for (int i = 0; i < BI; ++i) load_b(i, more);
        PIN_VMEM();
#pragma unroll
        for (int ks = 0; ks < KC / 16; ++ks) {
            bf16x8 af[MR], bf[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i)
                af[i] = *reinterpret_cast<const bf16x8*>(&As[((wm * MR + i) * 32 + lrow) * LDKH + ks * 16 + lh * 8]);
#pragma unroll
            for (int j = 0; j < NR; ++j)
                bf[j] = *reinterpret_cast<const bf16x8*>(&Bs[((wn * NR + j) * 32 + lrow) * LDKH + ks * 16 + lh * 8]);
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            store_chunk();
            __syncthreads();
        }
    }

    float* o = out + (long)blockIdx.z * slab_stride;
    const bool fin = (slab_stride == 0);
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int col = n0 + (wn * NR + j) * 32 + lrow;
            const float bv = (fin && bias != nullptr && col < g.Ca) ? bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int m = m0 + (wm * MR + i) * 32 + row;
                if (m < M && col < g.Ca) {
                    float v = acc[i][j][r];
                    if (fin) v = pg_act_epi(v + bv, act);
                    store_io(o, (long)m * ld_out + col, v, out_bf);
                }
            }
        }
}

template <int MR, int NR, int WM, int WN, bool HIN = false>
__global__ __launch_bounds__(256) void k_s2b_bf16(const float* __restrict__ small, int ld_small,
                                                  const float* __restrict__ P, float* __restrict__ out, int ld_out,
                                                  long slab_stride, Geom g, int chunks_per_slice,
                                                  const float* __restrict__ bias, int act, int small_bytes,
                                                  int p_bytes, int out_bf) {
    constexpr int BM = WM * MR * 32, BN = WN * NR * 32;
    constexpr int AI = BM / 32;
    constexpr int BG = 256 / BN;        // thread groups along k
    constexpr int NQ = 8 / BG;          // k-quads per thread per chunk
    __shared__ __attribute__((aligned(16))) __bf16 smem[(BM + BN) * LDKH];
    __bf16* As = smem;
    __bf16* Bs = smem + BM * LDKH;
    const __amdgpu_buffer_rsrc_t rsm = __builtin_amdgcn_make_buffer_rsrc((void*)small, 0, small_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rP = __builtin_amdgcn_make_buffer_rsrc((void*)P, 0, p_bytes, 0x00020000);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lrow = lane & 31, lh = lane >> 5;

    const int ncls = (g.s == 2) ? 4 : 1;
    const int cls = blockIdx.z % ncls, slice = blockIdx.z / ncls;
    const int ah = (g.s == 2) ? (cls >> 1) : 0, aw = (g.s == 2) ? (cls & 1) : 0;
    const int T = (g.s == 2) ? 2 : 4, Tsh = (g.s == 2) ? 1 : 2;
    const int Hc = (g.s == 2) ? (g.Hb - ah + 1) / 2 : g.Hb;
    const int Wc = (g.s == 2) ? (g.Wb - aw + 1) / 2 : g.Wb;
    const int kh0 = (g.s == 2) ? (1 - ah) : 0, kw0 = (g.s == 2) ? (1 - aw) : 0;
    const int Mc = g.N * Hc * Wc, K = T * T * g.Ca;
    const int m0 = xcd_remap(blockIdx.x, gridDim.x) * BM, n0 = blockIdx.y * BN;
    if (m0 >= Mc) return;
    const int nchunks = (K + KC - 1) / KC;
    const int c_begin = slice * chunks_per_slice;
    const int c_end = min(nchunks, c_begin + chunks_per_slice);

    const int kq = tid & 7, r0 = tid >> 3;
    int a_off[AI], a_mask[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int m = m0 + r0 + 32 * i;
        const int mm = min(m, Mc - 1);
        const int n = mm / (Hc * Wc);
        const int rem = mm - n * (Hc * Wc);
        const int ii = rem / Wc, jj = rem - ii * Wc;
        const int ib = (g.s == 2) ? ii + ah : ii + 1, jb = (g.s == 2) ? jj + aw : jj + 1;
        a_off[i] = ((n * g.Hs + ib) * g.Ws + jb) * ld_small;
        int wv = 0, mask = 0;          // local tap (th, tw) reads small pixel (ib - th, jb - tw)
#pragma unroll
        for (int t = 0; t < 4; ++t) wv |= (t < T && (unsigned)(jb - t) < (unsigned)g.Ws) ? (1 << t) : 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) mask |= (t < T && (unsigned)(ib - t) < (unsigned)g.Hs) ? (wv << (T * t)) : 0;
        a_mask[i] = (m < Mc) ? mask : 0;
    }
    const int bn = tid % BN, bg = tid / BN;
    const int ncol = n0 + bn;
    const int ncol_off = (ncol < g.Cb) ? ncol : 0x10000000;
    const int CaCb = g.Ca * g.Cb;

    // incremental (tloc, a) per k-quad: A float4 (index 0) and the NQ quads of B (1..NQ); Ca >= KC: <= 1 wrap
    int q_tl[NQ + 1], q_a[NQ + 1];
    {
        const int k = c_begin * KC + kq * 4;
        q_tl[0] = k / g.Ca;
        q_a[0] = k - q_tl[0] * g.Ca;
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int k = c_begin * KC + 4 * (bg + BG * i);
        q_tl[i + 1] = k / g.Ca;
        q_a[i + 1] = k - q_tl[i + 1] * g.Ca;
    }
    auto quad = [&](int qi, int& tl, int& a) {   // returns (tloc, a) of quad qi for the chunk being loaded
        tl = q_tl[qi];
        a = q_a[qi];
        const int na = a + KC;
        const bool wrap = na >= g.Ca;
        q_a[qi] = wrap ? na - g.Ca : na;
        q_tl[qi] = wrap ? tl + 1 : tl;
    };

    f32x4 ra[AI], rb[NQ];
    bf16x4 rah[AI];
    int a_tl = 0, a_koff = OOB;
    auto next_a = [&](int c) {
        const int k = c * KC + kq * 4;
        int tl, a;
        quad(0, tl, a);
        a_tl = tl;
        const int th = tl >> Tsh, tw = tl & (T - 1);
        a_koff = (k < K) ? (a - (th * g.Ws + tw) * ld_small) : 0x20000000;
    };
    auto load_a = [&](int i, bool on) {
        const bool ok = on && ((a_mask[i] >> a_tl) & 1) && (a_koff < 0x10000000);
        if constexpr (HIN)
            rah[i] = bload2h(rsm, voffh(a_off[i] + a_koff, ok));
        else
            ra[i] = bload4(rsm, voff(a_off[i] + a_koff, ok));
    };
    auto load_b = [&](int i, int c, bool on) {
        const int kb = c * KC + 4 * (bg + BG * i);
        int tl, a;
        quad(i + 1, tl, a);
        if (BN >= 64) {   // a wave shares one k-quad (bg = tid / BN is wave-uniform): keep its decode on the scalar unit
            tl = __builtin_amdgcn_readfirstlane(tl);
            a = __builtin_amdgcn_readfirstlane(a);
        }
        const int th = tl >> Tsh, tw = tl & (T - 1);
        const int tap = (kh0 + g.s * th) * 4 + (kw0 + g.s * tw);
        const bool ok = on && kb < K;
        const int rowoff = tap * CaCb + a * g.Cb;
        const int base = voff(rowoff + ncol_off, ok);
        const int st = g.Cb * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) rb[i][e] = bload1(rP, base + e * st);
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < AI; ++i) *reinterpret_cast<bf16x4*>(&As[(r0 + 32 * i) * LDKH + kq * 4]) = HIN ? rah[i] : to_bf16(ra[i]);
#pragma unroll
        for (int i = 0; i < NQ; ++i) *reinterpret_cast<bf16x4*>(&Bs[bn * LDKH + 4 * (bg + BG * i)]) = to_bf16(rb[i]);
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (c_begin < c_end) {
        next_a(c_begin);
#pragma unroll
        for (int i = 0; i < AI; ++i) load_a(i, true);
#pragma unroll
        for (int i = 0; i < NQ; ++i) load_b(i, c_begin, true);
        store_chunk();
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = (c + 1 < c_end);
        next_a(c + 1);
#pragma unroll
        for (int i = 0; i < AI; ++i) load_a(i, more);
#pragma unroll
        for (int i = 0; i < NQ; ++i) load_b(i, c + 1, more);
        PIN_VMEM();
#pragma unroll
        for (int ks = 0; ks < KC / 16; ++ks) {
            bf16x8 af[MR], bf[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i)
                af[i] = *reinterpret_cast<const bf16x8*>(&As[((wm * MR + i) * 32 + lrow) * LDKH + ks * 16 + lh * 8]);
#pragma unroll
            for (int j = 0; j < NR; ++j)
                bf[j] = *reinterpret_cast<const bf16x8*>(&Bs[((wn * NR + j) * 32 + lrow) * LDKH + ks * 16 + lh * 8]);
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            store_chunk();
            __syncthreads();
        }
    }

    const bool fin = (slab_stride == 0);
    float* o = out + (long)slice * slab_stride;
    const int ldo = fin ? ld_out : g.Cb;
    float bv[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int col = n0 + (wn * NR + j) * 32 + lrow;
        bv[j] = (fin && bias != nullptr && col < g.Cb) ? bias[col] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < MR; ++i) {
        // decode the lane's first row with two divisions, then walk the other 15 (at most 28 rows further) with a
        // carry chain: 64 divisions per thread in the epilogue cost as much as several K-chunks
        const int mb = m0 + (wm * MR + i) * 32 + 4 * lh;
        const int mbc = min(mb, Mc - 1);
        const int nb0 = mbc / (Hc * Wc);
        const int remb = mbc - nb0 * (Hc * Wc);
        const int ib0 = remb / Wc, jb0 = remb - ib0 * Wc;
        const bool chain = Wc >= 16 && Hc >= 2;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int m = m0 + (wm * MR + i) * 32 + row;
            if (m < Mc) {
                int n, ii, jj;
                if (chain) {
                    const int d = (r & 3) + 8 * (r >> 2);      // 0..27 rows past the decoded one
                    jj = jb0 + d;
                    ii = ib0;
                    n = nb0;
                    bool w1 = jj >= Wc;
                    jj = w1 ? jj - Wc : jj;
                    ii = w1 ? ii + 1 : ii;
                    w1 = jj >= Wc;
                    jj = w1 ? jj - Wc : jj;
                    ii = w1 ? ii + 1 : ii;
                    w1 = ii >= Hc;
                    ii = w1 ? ii - Hc : ii;
                    n = w1 ? n + 1 : n;
                } else {
                    n = m / (Hc * Wc);
                    const int rem = m - n * (Hc * Wc);
                    ii = rem / Wc;
                    jj = rem - ii * Wc;
                }
                const int h = (g.s == 2) ? 2 * ii + ah : ii, w = (g.s == 2) ? 2 * jj + aw : jj;
                const long orow = (long)((n * g.Hb + h) * g.Wb + w) * ldo;
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    const int col = n0 + (wn * NR + j) * 32 + lrow;
                    if (col < g.Cb) {
                        float v = acc[i][j][r];
                        if (fin) v = pg_act_epi(v + bv[j], act);
                        store_io(o, orow + col, v, out_bf);
                    }
                }
            }
        }
    }
}

typedef short s16x4 __attribute__((ext_vector_type(4)));
// 8 consecutive k (rows p .. p + 7*pitch) of this lane's column as an MFMA bf16 fragment: two ds_read_b64_tr_b16
__device__ __forceinline__ bf16x8 tr_frag(const __bf16* p, int pitch) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p + 4 * pitch));
    // (whole-vector casts: an element-by-element short -> __bf16 bit_cast of the two results is miscompiled by this hipcc
    // into v_perm / v_mov of the first dword only)
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, both);
}

template <int MR, int NR, int WM, int WN, bool POW2, bool HIN = false>
__global__ __launch_bounds__(256) void k_wgrad_bf16(const float* __restrict__ small, int ld_small,
                                                    const float* __restrict__ big, int ld_big,
                                                    float* __restrict__ out, long slab_stride, Geom g,
                                                    int chunks_per_slice, int tilesB, int small_bytes, int big_bytes) {
    constexpr int BM = WM * MR * 32, BN = WN * NR * 32;
    constexpr int LDA = BM + 8, LDB = BN + 8;     // bf16 elements; rows stay 8-byte aligned
    constexpr int AQ = BM / 4, AROWS = 256 / AQ, AI = KC / AROWS;
    constexpr int BQ = BN / 4, BROWS = 256 / BQ, BI = KC / BROWS;
    __shared__ __attribute__((aligned(16))) __bf16 smem[KC * LDA + KC * LDB];
    __bf16* As = smem;
    __bf16* Bs = smem + KC * LDA;
    const __amdgpu_buffer_rsrc_t rsm = __builtin_amdgcn_make_buffer_rsrc((void*)small, 0, small_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rbig = __builtin_amdgcn_make_buffer_rsrc((void*)big, 0, big_bytes, 0x00020000);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int lrow = lane & 31, lh = lane >> 5;
    const int tile_a = blockIdx.x / tilesB, tile_b = blockIdx.x % tilesB;
    const int m0 = tile_a * BM, n0 = tile_b * BN;
    const int tap = blockIdx.y, kh = tap >> 2, kw = tap & 3;
    const int Kp = g.N * g.Hs * g.Ws;
    const int nchunks = (Kp + KC - 1) / KC;
    const int c_begin = blockIdx.z * chunks_per_slice;
    const int c_end = min(nchunks, c_begin + chunks_per_slice);

    // transposed fragment reads: 16-lane group gr = lane >> 4 covers columns (gr & 1) * 16 .. +15 and k rows (gr >> 1) * 8 .. +7
    const int tr_row = ((lane >> 4) >> 1) * 8 + ((lane & 15) >> 2), tr_col = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;
    const int aq = tid % AQ, arow0 = tid / AQ;
    const int bq = tid % BQ, brow0 = tid / BQ;
    const int a_col = (m0 + aq * 4 < g.Ca) ? m0 + aq * 4 : 0x10000000;      // small rows beyond Kp are out of range by
    const int b_col = (n0 + bq * 4 < g.Cb) ? n0 + bq * 4 : 0x10000000;      // construction of small_bytes
    // pixel -> (img, p, q): shifts when Hs, Ws are powers of two (every UNet layer), else a branch-free carry chain
    // (needs Ws >= 16 and Hs >= 2: a step of KC = 32 pixels wraps q at most twice and p at most once)
    const int lgW = 31 - __builtin_clz(g.Ws), lgH = 31 - __builtin_clz(g.Hs);
    int r_n[BI], r_p[BI], r_q[BI];
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        const int pix = c_begin * KC + brow0 + BROWS * i;
        r_n[i] = pix / (g.Hs * g.Ws);
        const int rem = pix - r_n[i] * (g.Hs * g.Ws);
        r_p[i] = rem / g.Ws;
        r_q[i] = rem - r_p[i] * g.Ws;
    }

    f32x4 ra[AI], rb[BI];
    bf16x4 rah[AI], rbh[BI];
    auto load_a = [&](int i, int c, bool on) {
        const int pix = c * KC + arow0 + AROWS * i;
        const bool ok = on && pix < Kp;
        if constexpr (HIN)
            rah[i] = bload2h(rsm, voffh(pix * ld_small + a_col, ok));
        else
            ra[i] = bload4(rsm, voff(pix * ld_small + a_col, ok));
    };
    auto load_b = [&](int i, int c, bool on) {
        const int pix = c * KC + brow0 + BROWS * i;
        int n, p, q;
        if (POW2) {
            q = pix & (g.Ws - 1);
            p = (pix >> lgW) & (g.Hs - 1);
            n = pix >> (lgW + lgH);
        } else {
            n = r_n[i];
            p = r_p[i];
            q = r_q[i];
            int nq = q + KC, np = p, nn = n;
            bool w = nq >= g.Ws;
            nq = w ? nq - g.Ws : nq;
            np = w ? np + 1 : np;
            w = nq >= g.Ws;
            nq = w ? nq - g.Ws : nq;
            np = w ? np + 1 : np;
            w = np >= g.Hs;
            np = w ? np - g.Hs : np;
            nn = w ? nn + 1 : nn;
            r_q[i] = nq;
            r_p[i] = np;
            r_n[i] = nn;
        }
        const int h = g.s * p - 1 + kh, w = g.s * q - 1 + kw;
        const bool ok = on && pix < Kp && (unsigned)h < (unsigned)g.Hb && (unsigned)w < (unsigned)g.Wb;
        if constexpr (HIN)
            rbh[i] = bload2h(rbig, voffh(((n * g.Hb + h) * g.Wb + w) * ld_big + b_col, ok));
        else
            rb[i] = bload4(rbig, voff(((n * g.Hb + h) * g.Wb + w) * ld_big + b_col, ok));
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < AI; ++i) *reinterpret_cast<bf16x4*>(&As[(arow0 + AROWS * i) * LDA + aq * 4]) = HIN ? rah[i] : to_bf16(ra[i]);
#pragma unroll
        for (int i = 0; i < BI; ++i) *reinterpret_cast<bf16x4*>(&Bs[(brow0 + BROWS * i) * LDB + bq * 4]) = HIN ? rbh[i] : to_bf16(rb[i]);
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (c_begin < c_end) {
#pragma unroll
        for (int i = 0; i < AI; ++i) load_a(i, c_begin, true);
#pragma unroll
        for (int i = 0; i < BI; ++i) load_b(i, c_begin, true);
        store_chunk();
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = (c + 1 < c_end);
#pragma unroll
        for (int i = 0; i < AI; ++i) load_a(i, c + 1, more);
#pragma unroll
        for (int i = 0; i < BI; ++i) load_b(i, c + 1, more);
        PIN_VMEM();
#pragma unroll
        for (int ks = 0; ks < KC / 16; ++ks) {
            // tiles are [k][m] (K is the pixel axis here and both operands are contiguous along channels in memory, so there is
            // no K-contiguous image to stage): the fragments -- 8 consecutive k of the lane's column -- come from two transposed
            // LDS reads (ds_read_b64_tr_b16: per 16-lane group a 4-row x 16-column block, lane 4q+p addresses row q / columns
            // 4p.., lane i receives column i of the four rows; verified with tools/tr_probe.hip) instead of 8 ds_read_u16
            bf16x8 af[MR], bf[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i) af[i] = tr_frag(&As[(ks * 16 + tr_row) * LDA + (wm * MR + i) * 32 + tr_col], LDA);
#pragma unroll
            for (int j = 0; j < NR; ++j) bf[j] = tr_frag(&Bs[(ks * 16 + tr_row) * LDB + (wn * NR + j) * 32 + tr_col], LDB);
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            store_chunk();
            __syncthreads();
        }
    }

    float* o = out + (long)blockIdx.z * slab_stride + (long)tap * g.Ca * g.Cb;
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int col = n0 + (wn * NR + j) * 32 + lrow;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int a = m0 + (wm * MR + i) * 32 + row;
                if (a < g.Ca && col < g.Cb) o[(long)a * g.Cb + col] = acc[i][j][r];
            }
        }
}

// ------------------------------------------------------------------------------------------------
// Second halves of the taps-folded-into-N forward paths.  D is the row GEMM's output:
//   small2big:  D[small pixel][(tap, b)]  ->  big[n,h,w,b] = act(sum over the taps that reach (h,w) + bias[b])
//   big2small:  D[big pixel][(tap, a)]    ->  small[n,p,q,a] = act(sum_{kh,kw in range} D[(s*p-1+kh, s*q-1+kw)] + bias[a])
// and the weight re-layout the first needs: W'[(tap*Cb + b)][a] = P[tap][a][b] (a few KB).
// ------------------------------------------------------------------------------------------------
// The same gather for stride 2 with the D rows staged through LDS: a workgroup owns the 2*CT_H x 2*CT_W big pixels of one sample
// that descend from a CT_H x CT_W block of small pixels, loads the (CT_H + 2) x (CT_W + 2) small pixels' D rows that reach them
// once, coalesced (a row is 16 * Cb contiguous floats), and sums the four taps of every output from LDS.  (The kernel above reads
// each D row in 16-byte pieces from four different pixels' threads: 1.3 - 2.3 TB/s at 512 x 512.)
constexpr int CT_H = 4, CT_W = 16;
__global__ __launch_bounds__(256) void k_col2im_s2_lds(const float* __restrict__ D, const float* __restrict__ bias, float* __restrict__ big,
                                                       int ld_big, Geom g, int act, int tiles_h, int tiles_w) {
    extern __shared__ __attribute__((aligned(16))) float rows[];   // [(CT_H + 2) * (CT_W + 2)][Nc]
    const int Nc = 16 * g.Cb, nq = Nc >> 2;
    int t = blockIdx.x;
    const int tw = t % tiles_w;
    t /= tiles_w;
    const int th = t % tiles_h, n = t / tiles_h;
    const int a0 = th * CT_H, b0 = tw * CT_W;                     // first small pixel of the block; staged rows start one earlier
    constexpr int RW = CT_W + 2, NR_ = (CT_H + 2) * RW;
    for (int i = threadIdx.x; i < NR_ * nq; i += 256) {
        const int r = i / nq, q = i - r * nq;
        const int ih = a0 - 1 + r / RW, iw = b0 - 1 + r % RW;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)ih < (unsigned)g.Hs && (unsigned)iw < (unsigned)g.Ws)
            v = *reinterpret_cast<const f32x4*>(D + (long)((n * g.Hs + ih) * g.Ws + iw) * Nc + 4 * q);
        *reinterpret_cast<f32x4*>(rows + r * Nc + 4 * q) = v;
    }
    __syncthreads();
    const int npx = 2 * CT_H * 2 * CT_W;
    for (int i = threadIdx.x; i < npx * g.Cb; i += 256) {
        const int b = i % g.Cb, p = i / g.Cb;
        const int hl = p / (2 * CT_W), wl = p - hl * (2 * CT_W);
        const int h = 2 * a0 + hl, w = 2 * b0 + wl;
        if (h >= g.Hb || w >= g.Wb) continue;
        // big row h = 2a + r: taps kh with (h + 1 - kh) even -> kh = 1 - r + 2j (j = 0, 1), small row a + r - j
        const int rh = hl & 1, rw = wl & 1, al = hl >> 1, bl = wl >> 1;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int kh = 1 - rh + 2 * j, ihl = al + rh - j + 1;             // + 1: the staged block starts at a0 - 1
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int kw = 1 - rw + 2 * k, iwl = bl + rw - k + 1;
                acc += rows[(ihl * RW + iwl) * Nc + (kh * 4 + kw) * g.Cb + b];      // out-of-image small pixels were staged as zeros
            }
        }
        if (bias) acc += bias[b];
        big[((long)(n * g.Hb + h) * g.Wb + w) * ld_big + b] = pg_act_epi(acc, act);
    }
}

__global__ void k_col2im_small2big(const float* __restrict__ D, const float* __restrict__ bias, float* __restrict__ big,
                                   int ld_big, Geom g, int act) {
    const long total = (long)g.N * g.Hb * g.Wb * g.Cb;
    const int Nc = 16 * g.Cb;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int b = (int)(idx % g.Cb);
        const long pix = idx / g.Cb;
        const int n = (int)(pix / (g.Hb * g.Wb));
        const int rem = (int)(pix - (long)n * g.Hb * g.Wb);
        const int h = rem / g.Wb, w = rem - h * g.Wb;
        float acc = 0.f;
#pragma unroll
        for (int kh = 0; kh < 4; ++kh) {
            const int hh = h + 1 - kh;
            if (hh < 0 || (g.s == 2 && (hh & 1))) continue;
            const int ih = g.s == 2 ? hh >> 1 : hh;
            if (ih >= g.Hs) continue;
#pragma unroll
            for (int kw = 0; kw < 4; ++kw) {
                const int ww = w + 1 - kw;
                if (ww < 0 || (g.s == 2 && (ww & 1))) continue;
                const int iw = g.s == 2 ? ww >> 1 : ww;
                if (iw >= g.Ws) continue;
                acc += D[(long)((n * g.Hs + ih) * g.Ws + iw) * Nc + (kh * 4 + kw) * g.Cb + b];
            }
        }
        if (bias) acc += bias[b];
        big[pix * ld_big + b] = pg_act_epi(acc, act);
    }
}

__global__ void k_gather_big2small(const float* __restrict__ D, const float* __restrict__ bias,
                                   float* __restrict__ small, int ld_small, Geom g, int act) {
    const long total = (long)g.N * g.Hs * g.Ws * g.Ca;
    const int Nc = 16 * g.Ca;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int a = (int)(idx % g.Ca);
        const long pix = idx / g.Ca;
        const int n = (int)(pix / (g.Hs * g.Ws));
        const int rem = (int)(pix - (long)n * g.Hs * g.Ws);
        const int p = rem / g.Ws, q = rem - p * g.Ws;
        float acc = 0.f;
#pragma unroll
        for (int kh = 0; kh < 4; ++kh) {
            const int h = g.s * p - 1 + kh;
            if ((unsigned)h >= (unsigned)g.Hb) continue;
#pragma unroll
            for (int kw = 0; kw < 4; ++kw) {
                const int w = g.s * q - 1 + kw;
                if ((unsigned)w >= (unsigned)g.Wb) continue;
                acc += D[(long)((n * g.Hb + h) * g.Wb + w) * Nc + (kh * 4 + kw) * g.Ca + a];
            }
        }
        if (bias) acc += bias[a];
        small[pix * ld_small + a] = pg_act_epi(acc, act);
    }
}

__global__ void k_pack_taps_b(const float* __restrict__ P, float* __restrict__ Wp, int Ca, int Cb) {
    const int total = 16 * Ca * Cb;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int a = i % Ca;                 // Wp[(tap*Cb + b)*Ca + a]
        const int tb = i / Ca;
        const int b = tb % Cb, tap = tb / Cb;
        Wp[i] = P[(long)(tap * Ca + a) * Cb + b];
    }
}

// ------------------------------------------------------------------------------------------------
// split-K reduce (+ bias + activation):  out[r*ld_out + c] = act(sum_z slab[z][r*cols + c] + bias[c])
// ------------------------------------------------------------------------------------------------
__global__ void k_slab_reduce(const float* __restrict__ slabs, long slab_stride, int S, float* __restrict__ out,
                              int ld_out, long rows, int cols, const float* __restrict__ bias, int act, int out_bf) {
    const long total = rows * cols;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cols;
        const int c = (int)(i - r * cols);
        float v = slabs[i];
        for (int z = 1; z < S; ++z) v += slabs[(long)z * slab_stride + i];
        if (bias) v += bias[c];
        store_io(out, r * ld_out + c, pg_act(v, act), out_bf);
    }
}

__global__ void k_slab_reduce4(const float* __restrict__ slabs, long slab_stride, int S, float* __restrict__ out,
                               int ld_out, long rows, int cols, const float* __restrict__ bias, int act, int out_bf, pg_epi_mul mul) {
    const int cq = cols >> 2;
    const long total = rows * cq;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cq;
        const int c = (int)(i - r * cq) << 2;
        const long off = r * cols + c;
        f32x4 v = *reinterpret_cast<const f32x4*>(slabs + off);
        int z = 1;
        for (; z + 8 <= S; z += 8) {        // eight independent loads in flight, summed in slab order
            f32x4 t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = *reinterpret_cast<const f32x4*>(slabs + (long)(z + k) * slab_stride + off);
#pragma unroll
            for (int k = 0; k < 8; ++k) v += t[k];
        }
        for (; z < S; ++z) v += *reinterpret_cast<const f32x4*>(slabs + (long)z * slab_stride + off);
        if (bias) v += *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = pg_act_epi(v[e], act);
        if (mul.t) {
            f32x4 tv;
            if (out_bf) {
                const bf16x4 h = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(mul.t) + r * mul.ld + c);
                tv = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
            } else {
                tv = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(mul.t) + r * mul.ld + c);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= pg_act_grad_from_out(tv[e], mul.act);
        }
        if (out_bf)
            *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(out) + r * ld_out + c) = to_bf16(v);
        else
            *reinterpret_cast<f32x4*>(out + r * ld_out + c) = v;
    }
}

// many slabs, few outputs (the taps-in-N weight gradients: up to 512 slabs of a few thousand floats): 8 z-lanes per
// output share the slab loop, combined through LDS in lane order (deterministic)
__global__ __launch_bounds__(256) void k_slab_reduce_z(const float* __restrict__ slabs, long slab_stride, int S,
                                                       float* __restrict__ out, int ld_out, long rows, int cols) {
    __shared__ float red[8][32];
    const int ol = threadIdx.x & 31, zl = threadIdx.x >> 5;
    const long i = (long)blockIdx.x * 32 + ol;
    const long total = rows * cols;
    float v = 0.f;
    if (i < total) {
        int z = zl;
        for (; z + 56 < S; z += 64) {          // eight independent loads in flight, added in slab order
            float t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = slabs[(long)(z + 8 * k) * slab_stride + i];
#pragma unroll
            for (int k = 0; k < 8; ++k) v += t[k];
        }
        for (; z < S; z += 8) v += slabs[(long)z * slab_stride + i];
    }
    red[zl][ol] = v;
    __syncthreads();
    if (zl == 0 && i < total) {
        float t = red[0][ol];
#pragma unroll
        for (int k = 1; k < 8; ++k) t += red[k][ol];
        const long r = i / cols;
        out[r * ld_out + (i - r * cols)] = t;
    }
}

// column sums of a [rows][C] matrix (pixel stride ld): partial[chunk][c] over row chunks (bias gradient).
// 256 threads = 64 channels x 4 row lanes; fixed-order combine.
__global__ __launch_bounds__(256) void k_colsum_partial(const float* __restrict__ x, int ld, long rows, int C,
                                                        long rows_per_chunk, float* __restrict__ partial) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cl;
    const long r_begin = blockIdx.x * rows_per_chunk;
    const long r_end = min(rows, r_begin + rows_per_chunk);
    float s = 0.f;
    if (c < C)
        for (long r = r_begin + rl; r < r_end; r += 4) s += x[r * ld + c];
    red[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < C) partial[(long)blockIdx.x * C + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

// float4 variant (C % 4 == 0, 16-byte aligned rows): 256 threads = 16 channel quads x 16 row lanes, four independent
// loads in flight per lane; fixed-order combine.
template <bool HB>      // HB: x holds bf16 elements (bf16 activation storage)
__global__ __launch_bounds__(256) void k_colsum_partial4(const float* __restrict__ x, int ld, long rows, int C,
                                                         long rows_per_chunk, float* __restrict__ partial) {
    __shared__ f32x4 red[16][16];
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.y * 64 + cl * 4;
    const long r_begin = blockIdx.x * rows_per_chunk;
    const long r_end = min(rows, r_begin + rows_per_chunk);
    auto ld4 = [&](long idx) -> f32x4 {
        if constexpr (HB) {
            const bf16x4 h = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(x) + idx);
            return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
        } else {
            return *reinterpret_cast<const f32x4*>(x + idx);
        }
    };
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
    if (c < C) {
        long r = r_begin + rl;
        for (; r + 48 < r_end; r += 64) {
            s0 += ld4(r * ld + c);
            s1 += ld4((r + 16) * ld + c);
            s2 += ld4((r + 32) * ld + c);
            s3 += ld4((r + 48) * ld + c);
        }
        for (; r < r_end; r += 16) s0 += ld4(r * ld + c);
    }
    red[rl][cl] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (rl == 0 && c < C) {
        f32x4 t = red[0][cl];
#pragma unroll
        for (int i = 1; i < 16; ++i) t += red[i][cl];
        *reinterpret_cast<f32x4*>(partial + (long)blockIdx.x * C + c) = t;
    }
}

// ------------------------------------------------------------------------------------------------
// direct kernels: one thread per output element, no LDS, no MFMA.  Any channel count / alignment.
// ------------------------------------------------------------------------------------------------
__global__ void k_big2small_direct(const float* __restrict__ big, int ld_big, const float* __restrict__ P,
                                   const float* __restrict__ bias, float* __restrict__ small, int ld_small, Geom g,
                                   int act) {
    const long total = (long)g.N * g.Hs * g.Ws * g.Ca;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int a = (int)(idx % g.Ca);
        const long m = idx / g.Ca;
        const int n = (int)(m / (g.Hs * g.Ws));
        const int rem = (int)(m - (long)n * g.Hs * g.Ws);
        const int p = rem / g.Ws, q = rem - p * g.Ws;
        float acc = 0.f;
        for (int kh = 0; kh < 4; ++kh) {
            const int h = g.s * p - 1 + kh;
            if ((unsigned)h >= (unsigned)g.Hb) continue;
            for (int kw = 0; kw < 4; ++kw) {
                const int w = g.s * q - 1 + kw;
                if ((unsigned)w >= (unsigned)g.Wb) continue;
                const float* xi = big + (long)((n * g.Hb + h) * g.Wb + w) * ld_big;
                const float* wi = P + (long)((kh * 4 + kw) * g.Ca + a) * g.Cb;
                for (int b = 0; b < g.Cb; ++b) acc = fmaf(xi[b], wi[b], acc);
            }
        }
        if (bias) acc += bias[a];
        small[m * ld_small + a] = pg_act(acc, act);
    }
}

// small -> big from a ONE-channel `small` (the discriminator head's data gradient, disc.py:45: Conv2d(512, 1, 4, 1, 1) backward):
// out[pixel][b] = sum over the <= 16 taps that reach the pixel of small[pixel'] * P[tap][0][b] -- 16 FMAs per output, bound by the
// HBM write of `big`.  A thread owns 4 consecutive b (its 16 tap weights = 16 float4 in registers) and walks pixels; the tap
// values of a pixel are the same address for every thread of the workgroup (one broadcast load each).  Output fp32 or bf16
// (out_bf); mul: times f'(t) of the layer below (pg_epi_mul; t in the output's storage type).  Many short workgroups: the per-pixel
// chain (16 loads, FMAs, store) is latency-bound, ~8 workgroups per CU hide it (64-pixel workgroups: 70 us, 7-pixel ones: 40 us;
// a 4-pixel software pipeline per thread: slower, 64 more registers).
// Stride-1 form (the discriminator head's data gradient, disc.py:45: Cout = 1, 4x4, stride 1): a workgroup first stages its SAMPLE's
// whole one-channel map (Hs x Ws floats, a few KB) into LDS inside a zero border of two, so that the 16 taps of a pixel are 16
// unmasked, conflict-free broadcast reads -- the generic kernel below fetched them with 16 global loads per pixel AND PER WAVE (64
// identical addresses each: ~1 M broadcast loads per launch through the address path, 1.4 TB/s of output where stores alone run 6).
// grid (workgroups per sample, N); a thread keeps its channel quad's 16 weight vectors in registers and walks pixels.
__global__ __launch_bounds__(256) void k_s2b_ca1_s1(const float* __restrict__ small, int ld_small, const float* __restrict__ P,
                                                    const float* __restrict__ bias, float* __restrict__ big, int ld_big, Geom g, int act,
                                                    int out_bf, pg_epi_mul mul, int pix_per_block) {
    extern __shared__ __attribute__((aligned(16))) float xs[];     // [(Hs + 4)][(Ws + 4)], the map at (2, 2)
    const int n = blockIdx.y, PW = g.Ws + 4, HWs = g.Hs * g.Ws, HWb = g.Hb * g.Wb;
    for (int i = threadIdx.x; i < (g.Hs + 4) * PW; i += 256) xs[i] = 0.f;
    __syncthreads();
    for (int i = threadIdx.x; i < HWs; i += 256) {
        const int ih = i / g.Ws, iw = i - ih * g.Ws;
        xs[(ih + 2) * PW + iw + 2] = small[(long)(n * HWs + i) * ld_small];
    }
    const int cq = g.Cb >> 2;
    const int qd = threadIdx.x % cq, np = 256 / cq;
    const int lane_p = (cq % 64 == 0) ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / cq) : (int)threadIdx.x / cq;
    const int b = qd * 4;
    f32x4 w[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) w[t] = *reinterpret_cast<const f32x4*>(P + (long)t * g.Cb + b);      // Ca == 1: P[tap][0][b]
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias) bv = *reinterpret_cast<const f32x4*>(bias + b);
    __syncthreads();
    const int p0 = blockIdx.x * pix_per_block, p1 = min(HWb, p0 + pix_per_block);
    for (int pix = p0 + lane_p; pix < p1; pix += np) {
        const int h = pix / g.Wb, wq = pix - h * g.Wb;
        // tap (kh, kw) reads small[h + 1 - kh][wq + 1 - kw] = xs[h + 3 - kh][wq + 3 - kw]
        const float* xr = xs + (h + 3) * PW + wq + 3;
        f32x4 acc = bv;
        // The tap values never reach a packed multiply straight from the LDS return: `acc += x * w` compiles to v_pk_mul_f32 with the
        // scalar x broadcast through op_sel, and where that takes its LOW half from the ODD register of a pair that a ds_read2_b32
        // has just returned, lanes 48-63 of the low half were seen to use the register's OLD content although s_waitcnt lgkmcnt had
        // been satisfied (one tap of e0 / e2 dropped, ~1 call in 40, only next to another process on the GPU: EXPERIMENTS.md,
        // "k_s2b_ca1_s1: cause").  A plain VALU read of the returned register is safe (v_readfirstlane where the wave's pixel is
        // uniform -- the values then live in scalar registers --, a v_mov_b32 otherwise); tests/test_codeobj_cpu.py scans the
        // library for the failing operand form.
        float xv[16];
#pragma unroll
        for (int kh = 0; kh < 4; ++kh)
#pragma unroll
            for (int kw = 0; kw < 4; ++kw) xv[kh * 4 + kw] = xr[-kh * PW - kw];
        if (cq % 64 == 0) {
#pragma unroll
            for (int t = 0; t < 16; ++t) xv[t] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, xv[t])));
        } else {
#pragma unroll
            for (int t = 0; t < 16; ++t) asm volatile("v_mov_b32 %0, %1" : "=v"(xv[t]) : "v"(xv[t]));
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) acc += xv[t] * w[t];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = pg_act_epi(acc[e], act);
        const long m = (long)n * HWb + pix;
        if (mul.t) {
            f32x4 tv;
            if (out_bf) {
                const bf16x4 hv = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(mul.t) + m * mul.ld + b);
                tv = f32x4{(float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]};
            } else {
                tv = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(mul.t) + m * mul.ld + b);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] *= pg_act_grad_from_out(tv[e], mul.act);
        }
        if (out_bf)
            *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(big) + m * ld_big + b) = to_bf16(acc);
        else
            *reinterpret_cast<f32x4*>(big + m * ld_big + b) = acc;
    }
}

__global__ __launch_bounds__(256) void k_s2b_ca1(const float* __restrict__ small, int ld_small, const float* __restrict__ P,
                                                 const float* __restrict__ bias, float* __restrict__ big, int ld_big, Geom g, int act,
                                                 int out_bf, pg_epi_mul mul, int pix_per_block) {
    constexpr int PP = 2;                                          // pixels per thread and trip
    const int cq = g.Cb >> 2;                                      // channel quads
    // host: 256 % cq == 0, cq <= 256.  With >= 64 quads (Cb >= 256: the discriminator head at ndf >= 32) a wave works on ONE pixel:
    // its pixel index is made provably wave-uniform (readfirstlane), so the pixel decode, the 16 tap addresses and the tap loads
    // themselves run on the scalar unit (s_load) instead of once per lane -- the kernel was bound by that per-lane integer work
    const int qd = threadIdx.x % cq, np = 256 / cq;
    const int lane_p = (cq % 64 == 0) ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / cq) : (int)threadIdx.x / cq;
    const int b = qd * 4;
    f32x4 w[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) w[t] = *reinterpret_cast<const f32x4*>(P + (long)t * g.Cb + b);      // Ca == 1: P[tap][0][b]
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias) bv = *reinterpret_cast<const f32x4*>(bias + b);
    const int total = g.N * g.Hb * g.Wb;                           // (host: < 2^31; 32-bit pixel decode: a 64-bit division per pixel
    const int p0 = blockIdx.x * pix_per_block;                     //  was the single most expensive thing in this kernel)
    const int p1 = min(total, p0 + pix_per_block);
    const int HWb = g.Hb * g.Wb;
    for (int m0 = p0 + lane_p; m0 < p1; m0 += np * PP) {
        // the taps' inputs: UNCONDITIONAL loads from clamped addresses, masked afterwards -- all of them (and the multiplier's loads)
        // are in flight together; `ok ? small[..] : 0` compiled to a branch and a wait per tap
        float xv[PP][16];
        f32x4 tv[PP];
        int mm[PP];
        bool live[PP];
#pragma unroll
        for (int u = 0; u < PP; ++u) {
            const int m = m0 + u * np;
            live[u] = m < p1;
            mm[u] = live[u] ? m : p1 - 1;
            const int n = mm[u] / HWb;
            const int rem = mm[u] - n * HWb;
            const int h = rem / g.Wb, wq = rem - h * g.Wb;
#pragma unroll
            for (int kh = 0; kh < 4; ++kh) {
                const int hh = h + 1 - kh;
                const int ih = (g.s == 2) ? hh >> 1 : hh;
                const bool okh = (hh >= 0) & !((g.s == 2) & (hh & 1)) & (ih < g.Hs);
                const int ihc = min(max(ih, 0), g.Hs - 1);
#pragma unroll
                for (int kw = 0; kw < 4; ++kw) {
                    const int ww = wq + 1 - kw;
                    const int iw = (g.s == 2) ? ww >> 1 : ww;
                    const bool ok = okh & (ww >= 0) & !((g.s == 2) & (ww & 1)) & (iw < g.Ws);
                    const int iwc = min(max(iw, 0), g.Ws - 1);
                    const float x = small[(long)((n * g.Hs + ihc) * g.Ws + iwc) * ld_small];
                    xv[u][kh * 4 + kw] = ok ? x : 0.f;
                }
            }
            if (mul.t) {
                if (out_bf) {
                    const bf16x4 hv = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(mul.t) + (long)mm[u] * mul.ld + b);
                    tv[u] = f32x4{(float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]};
                } else {
                    tv[u] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(mul.t) + (long)mm[u] * mul.ld + b);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PP; ++u) {
            f32x4 acc = bv;
#pragma unroll
            for (int t = 0; t < 16; ++t) acc += xv[u][t] * w[t];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = pg_act_epi(acc[e], act);
            if (mul.t) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] *= pg_act_grad_from_out(tv[u][e], mul.act);
            }
            if (live[u]) {
                if (out_bf)
                    *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(big) + (long)mm[u] * ld_big + b) = to_bf16(acc);
                else
                    *reinterpret_cast<f32x4*>(big + (long)mm[u] * ld_big + b) = acc;
            }
        }
    }
}

__global__ void k_small2big_direct(const float* __restrict__ small, int ld_small, const float* __restrict__ P,
                                   const float* __restrict__ bias, float* __restrict__ big, int ld_big, Geom g,
                                   int act) {
    const long total = (long)g.N * g.Hb * g.Wb * g.Cb;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int b = (int)(idx % g.Cb);
        const long m = idx / g.Cb;
        const int n = (int)(m / (g.Hb * g.Wb));
        const int rem = (int)(m - (long)n * g.Hb * g.Wb);
        const int h = rem / g.Wb, w = rem - h * g.Wb;
        float acc = 0.f;
        for (int kh = 0; kh < 4; ++kh) {
            const int hh = h + 1 - kh;
            if (hh < 0 || (hh % g.s) != 0) continue;
            const int ih = hh / g.s;
            if (ih >= g.Hs) continue;
            for (int kw = 0; kw < 4; ++kw) {
                const int ww = w + 1 - kw;
                if (ww < 0 || (ww % g.s) != 0) continue;
                const int iw = ww / g.s;
                if (iw >= g.Ws) continue;
                const float* xi = small + (long)((n * g.Hs + ih) * g.Ws + iw) * ld_small;
                const float* wi = P + (long)(kh * 4 + kw) * g.Ca * g.Cb + b;
                for (int a = 0; a < g.Ca; ++a) acc = fmaf(xi[a], wi[(long)a * g.Cb], acc);
            }
        }
        if (bias) acc += bias[b];
        big[m * ld_big + b] = pg_act(acc, act);
    }
}

// one thread per (slice, tap, a, b); pixels of the slice summed serially (deterministic)
__global__ void k_wgrad_direct(const float* __restrict__ small, int ld_small, const float* __restrict__ big,
                               int ld_big, float* __restrict__ out, long slab_stride, Geom g, long pix_per_slice) {
    const long per = 16L * g.Ca * g.Cb;
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (idx >= per) return;
    const int b = (int)(idx % g.Cb);
    const int a = (int)((idx / g.Cb) % g.Ca);
    const int tap = (int)(idx / ((long)g.Cb * g.Ca));
    const int kh = tap >> 2, kw = tap & 3;
    const long Kp = (long)g.N * g.Hs * g.Ws;
    const long p_begin = blockIdx.y * pix_per_slice;
    const long p_end = min(Kp, p_begin + pix_per_slice);
    float acc = 0.f;
    for (long pix = p_begin; pix < p_end; ++pix) {
        const int n = (int)(pix / (g.Hs * g.Ws));
        const int rem = (int)(pix - (long)n * g.Hs * g.Ws);
        const int p = rem / g.Ws, q = rem - p * g.Ws;
        const int h = g.s * p - 1 + kh, w = g.s * q - 1 + kw;
        if ((unsigned)h >= (unsigned)g.Hb || (unsigned)w >= (unsigned)g.Wb) continue;
        acc = fmaf(small[pix * ld_small + a], big[(long)((n * g.Hb + h) * g.Wb + w) * ld_big + b], acc);
    }
    out[(long)blockIdx.y * slab_stride + idx] = acc;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Optional per-launch timing (bench.py's roofline leg): pg_conv_time_next() arms two caller-owned events; the next conv
// entry point on this thread records them immediately before and after its main GEMM kernel (not the split-K reduce,
// not the bias column-sum), then disarms.  Thread-local; no effect unless armed.
thread_local hipEvent_t t_ev0 = nullptr, t_ev1 = nullptr;
thread_local hipEvent_t t_ev2 = nullptr, t_ev3 = nullptr;   // second pair: the second GEMM of pg_conv4x4_bwd_big
struct TimedLaunch {
    hipStream_t st;
    hipEvent_t e1;
    explicit TimedLaunch(hipStream_t s) : st(s), e1(t_ev1) {
        if (t_ev0) (void)hipEventRecord(t_ev0, st);
        t_ev0 = nullptr;
        t_ev1 = nullptr;
    }
    ~TimedLaunch() {
        if (e1) (void)hipEventRecord(e1, st);
    }
};

// bytes spanned by a [pixels][C] view with pixel stride ld (what the buffer descriptor of the fast kernels covers)
inline long tensor_bytes(long pixels, int ld, int C, bool bf = false) { return ((pixels - 1) * (long)ld + C) * (bf ? 2 : 4); }
inline bool aligned_io(const void* p, bool bf) { return (reinterpret_cast<uintptr_t>(p) & (bf ? 7 : 15)) == 0; }
constexpr long FAST_LIMIT = 0x60000000L;   // 1.5 GiB: keeps every 32-bit byte offset, incl. the +0x40000000 sentinel, < 2^32
constexpr long FAST_P_LIMIT = 0x40000000L; // packed weights: the invalid-row sentinel (+1 GiB) must land beyond the block
// Which view each planner path holds below FAST_LIMIT (tensor_bytes of the call's ld; a view beyond it takes the next path down):
//   path                                             op     checked                   beyond the limit
//   any path, bf16 tensors (PG_IO_*)                 0-2    every bf16 tensor         PG_EINVAL (plan_conv)
//   Bf16x (k_conv_bf16x / k_conv_bf16r)              0, 1   input                     register-staged k_*_bf16, else PG_EINVAL
//   Bf16xTapn (bf16 row GEMM + col2im)               1      small                     Bf16x
//   Tapnf / TapnfBf (k_s2b_tapnf)                    1      small and big             row GEMM + col2im
//   TapnRowGemm (+k_gather_big2small / +k_col2im..)  0 / 1  input (big / small)       Tapk(p) / Gemm
//   Tapkp (k_b2s_tapkp)                              0      big and small             Tapk
//   Gemm with p.fast (k_b2s_fast, k_s2b_fast,        0, 1   input; the packed         generic k_big2small / k_small2big
//        k_*_bf16 on fp32 tensors)                          weights < FAST_P_LIMIT
//   Gemm with p.fast (k_wgrad_fast, k_wgrad_bf16)    2      small and big             generic k_wgrad
//   Bf16xWgrad (k_wgrad_bf16x)                       2      small and big             Gemm, else PG_EINVAL
//   WgradTapnp (k_wgrad_tapnp)                       2      small and big             WgradTapn
//   no limit, 64-bit addressing in the kernels: Direct, Ca1 (k_s2b_ca1 / _s1), Wino1, Wino2 (polyphase), WinoWgrad, Wino2Wgrad,
//   Tapk (k_b2s_tapk), WgradTapn, the generic Gemm kernels, and the fp32 OUTPUT of every path that checks its input only
inline bool force_generic() {
    static const bool v = pg_exp_env("PATCHGAN_GENERIC_KERNELS") != nullptr;   // debugging aid: disable the fast variants
    return v;
}

bool geom_ok(const pg_conv_geom* g) {
    if (!g) return false;
    if (g->N <= 0 || g->Hb <= 0 || g->Wb <= 0 || g->Hs <= 0 || g->Ws <= 0 || g->Ca <= 0 || g->Cb <= 0) return false;
    if (g->stride != 1 && g->stride != 2) return false;
    // small = floor((big + 2 - 4)/s) + 1 (nn.Conv2d) ; for stride 2 the big side may also be 2*small (convT)
    const int hs = (g->Hb - 2) / g->stride + 1, ws = (g->Wb - 2) / g->stride + 1;
    if (g->Hb < 2 || g->Wb < 2) return false;
    if (hs != g->Hs || ws != g->Ws) return false;
    // 32-bit index headroom inside the kernels
    const double big_elems = (double)g->N * g->Hb * g->Wb, small_elems = (double)g->N * g->Hs * g->Ws;
    if (big_elems > 2.0e9 || small_elems > 2.0e9) return false;
    if (16.0 * g->Ca * g->Cb > 2.0e9) return false;
    return true;
}

Geom to_geom(const pg_conv_geom* g) { return Geom{g->N, g->Hb, g->Wb, g->Hs, g->Ws, g->Ca, g->Cb, g->stride}; }

struct Tile {
    int id, bm, bn;
};
// tile ids: 0 = 128x128, 1 = 128x64, 2 = 128x32, 3 = 64x128, 4 = 64x64
Tile pick_tile(long rows, int cols) {
    if (rows > 64) {
        if (cols > 64) return {0, 128, 128};
        if (cols > 32) return {1, 128, 64};
        return {2, 128, 32};
    }
    if (cols > 64) return {3, 64, 128};
    if (cols > 32) return {4, 64, 64};
    return {2, 128, 32};
}

// Split K until two workgroups per CU exist: one 4-wave workgroup per CU leaves the MFMA pipe idle while that workgroup stages its next tile
// (measured 55 vs 80 TFLOP/s on the same kernel ALONE on the chip at 1 vs 2 workgroups per CU).  Round 6: in the two-stream training step the
// kernel is not alone and a target of 256 measured FASTER (cfg2 step, same box, target 128 / 192 / 256 / 320 / 384 / 512 / 1024: 7.48 / 7.13 /
// 7.03 / 7.20 / 7.13 / 7.14 / 7.08 ms) -- not adopted: the other slices are another order of the sums, and the cfg2 loss curve, a chaotic
// quantity, then sits at 1.8e-4 from the reference's (step 3) instead of inside the north star's 1e-4 (tests/test_step_gpu.py).
constexpr int TARGET_BLOCKS = 512;

int pick_split(long tiles, int nchunks, int min_chunks) {
    static const int target = pg_exp_env("PATCHGAN_SPLIT_TARGET") ? atoi(pg_exp_env("PATCHGAN_SPLIT_TARGET")) : TARGET_BLOCKS;
    if (tiles >= target) return 1;
    static const int minc = pg_exp_env("PATCHGAN_SPLIT_MINCHUNKS") ? atoi(pg_exp_env("PATCHGAN_SPLIT_MINCHUNKS")) : 0;
    if (minc > 0) min_chunks = minc;
    long s = (target + tiles - 1) / tiles;
    long smax = nchunks / min_chunks;
    if (smax < 1) smax = 1;
    if (s > smax) s = smax;
    if (s > 1024) s = 1024;
    return (int)s;
}

struct Plan {
    Tile t;
    int tiles_m, tiles_n, ncls, nchunks, split, cps;
    long out_elems;   // elements of one slab
};

// A 128x128 tiling that yields 256..511 workgroups would need split-K 2 (slab write + reduce pass) to reach two
// workgroups per CU; the 128x64 tile reaches the same occupancy without the slabs at the same MFMA efficiency.
Tile refine_tile(Tile t, long rows, int cols, int ncls) {
    static const bool off = pg_exp_env("PATCHGAN_TILE_REFINE") == nullptr;   // measured slower than split-K 2: off by default
    if (off || t.id != 0) return t;
    const long tiles = ((rows + 127) / 128) * ((cols + 127) / 128) * ncls;
    if (tiles >= 256 && tiles < 512) return {1, 128, 64};
    return t;
}

Plan plan_b2s(const pg_conv_geom* g) {
    Plan p;
    const long M = (long)g->N * g->Hs * g->Ws;
    p.t = refine_tile(pick_tile(M, g->Ca), M, g->Ca, 1);
    p.tiles_m = (int)((M + p.t.bm - 1) / p.t.bm);
    p.tiles_n = (g->Ca + p.t.bn - 1) / p.t.bn;
    p.ncls = 1;
    p.nchunks = (16 * g->Cb + KC - 1) / KC;
    p.split = pick_split((long)p.tiles_m * p.tiles_n, p.nchunks, 8);
    p.out_elems = M * g->Ca;
    return p;
}

Plan plan_s2b(const pg_conv_geom* g) {
    Plan p;
    p.ncls = (g->stride == 2) ? 4 : 1;
    const int Hc = (g->stride == 2) ? (g->Hb + 1) / 2 : g->Hb, Wc = (g->stride == 2) ? (g->Wb + 1) / 2 : g->Wb;
    const long Mc = (long)g->N * Hc * Wc;   // largest class
    p.t = refine_tile(pick_tile(Mc, g->Cb), Mc, g->Cb, p.ncls);
    p.tiles_m = (int)((Mc + p.t.bm - 1) / p.t.bm);
    p.tiles_n = (g->Cb + p.t.bn - 1) / p.t.bn;
    const int taps = (g->stride == 2) ? 4 : 16;
    p.nchunks = (taps * g->Ca + KC - 1) / KC;
    p.split = pick_split((long)p.tiles_m * p.tiles_n * p.ncls, p.nchunks, 8);
    p.out_elems = (long)g->N * g->Hb * g->Wb * g->Cb;
    return p;
}

// wgrad kernel choice: 0 = one GEMM per tap, 1 / 2 = taps folded into N (few big-side / small-side channels)
int wgrad_mode(const pg_conv_geom* g) {
    if (g->Cb <= 8) return 1;
    if (g->Ca <= 8) return 2;
    return 0;
}

Plan plan_wgrad(const pg_conv_geom* g) {
    Plan p;
    const int mode = wgrad_mode(g);
    long Kp;
    if (mode == 0) {
        p.t = pick_tile(g->Ca, g->Cb);
        p.tiles_m = (g->Ca + p.t.bm - 1) / p.t.bm;
        p.tiles_n = (g->Cb + p.t.bn - 1) / p.t.bn;
        p.ncls = 16;
        Kp = (long)g->N * g->Hs * g->Ws;
    } else {
        const int Mdim = (mode == 1) ? g->Ca : g->Cb, Ndim = 16 * ((mode == 1) ? g->Cb : g->Ca);
        p.t = pick_tile(Mdim, Ndim);
        p.tiles_m = (Mdim + p.t.bm - 1) / p.t.bm;
        p.tiles_n = (Ndim + p.t.bn - 1) / p.t.bn;
        p.ncls = 1;
        Kp = (mode == 1) ? (long)g->N * g->Hs * g->Ws : (long)g->N * g->Hb * g->Wb;
    }
    p.nchunks = (int)((Kp + KC - 1) / KC);
    p.split = pick_split((long)p.tiles_m * p.tiles_n * p.ncls, p.nchunks, 8);
    if (mode != 0) {
        // the taps-in-N kernels stream a huge K (every pixel) into one or two tiles: latency-bound per workgroup, so they
        // want far more, shorter slices than the MFMA-bound kernels (measured 83 us at 512 slices vs 187 us at 128)
        static const int tt = pg_exp_env("PATCHGAN_TAPN_SPLIT") ? atoi(pg_exp_env("PATCHGAN_TAPN_SPLIT")) : 1024;
        long want = tt / ((long)p.tiles_m * p.tiles_n);
        long smax = p.nchunks / 4;
        if (want > smax) want = smax;
        p.split = want < 1 ? 1 : (int)want;
    }
    p.out_elems = 16L * g->Ca * g->Cb;
    return p;
}

constexpr int DIRECT_WGRAD_SLICES = 64;
constexpr int COLSUM_CHUNKS = 1024;
// the bias gradient's partial column sums, reserved at the head of the weight gradient's workspace
inline size_t colsum_bytes(int Ca) { return ((size_t)COLSUM_CHUNKS * Ca * sizeof(float) + 255) & ~(size_t)255; }

void clamp_split(Plan& p, size_t ws_bytes, size_t reserved) {
    size_t avail = ws_bytes > reserved ? ws_bytes - reserved : 0;
    long smax = (long)(avail / (sizeof(float) * (size_t)p.out_elems));
    if (p.split > 1 && smax < p.split) p.split = smax < 2 ? 1 : (int)smax;
    p.cps = (p.nchunks + p.split - 1) / p.split;
    p.split = (p.nchunks + p.cps - 1) / p.cps;   // drop empty slices
}

int launch_reduce(const float* slabs, long slab_stride, int S, float* out, int ld_out, long rows, int cols,
                  const float* bias, int act, hipStream_t st, int out_bf = 0, pg_epi_mul mul = pg_epi_mul{nullptr, 0, 0}) {
    if (S >= 64 && !bias && act == PG_ACT_NONE && rows * cols <= (1L << 22) && !out_bf && !mul.t) {
        const long total = rows * cols;
        hipLaunchKernelGGL(k_slab_reduce_z, dim3((unsigned)((total + 31) / 32)), dim3(256), 0, st, slabs, slab_stride, S, out,
                           ld_out, rows, cols);
        return hipGetLastError() == hipSuccess ? PG_OK : PG_ELAUNCH;
    }
    if ((cols % 4 == 0) && (ld_out % 4 == 0) && (slab_stride % 4 == 0) && aligned16(slabs) &&
        ((reinterpret_cast<uintptr_t>(out) & (out_bf ? 7 : 15)) == 0) && (!bias || aligned16(bias))) {
        const long total4 = rows * (cols / 4);
        int blocks = (int)std::min<long>((total4 + 255) / 256, 16384);
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL(k_slab_reduce4, dim3(blocks), dim3(256), 0, st, slabs, slab_stride, S, out, ld_out, rows, cols,
                           bias, act, out_bf, mul);
        return hipGetLastError() == hipSuccess ? PG_OK : PG_ELAUNCH;
    }
    if (mul.t) return PG_EINVAL;       // (the callers that pass a multiplier satisfy the alignment of the vector form)
    const long total = rows * cols;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_slab_reduce, dim3(blocks), dim3(256), 0, st, slabs, slab_stride, S, out, ld_out, rows, cols,
                       bias, act, out_bf);
    return hipGetLastError() == hipSuccess ? PG_OK : PG_ELAUNCH;
}

// the five <MR,NR,WM,WN> tilings behind the tile ids of pick_tile(): f receives the tuple as a type,
//     for_tile(id, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL((k<PG_TILE(T), ...>), ...); });
template <int MR_, int NR_, int WM_, int WN_>
struct TileT {
    static constexpr int MR = MR_, NR = NR_, WM = WM_, WN = WN_;
};
#define PG_TILE(T) T::MR, T::NR, T::WM, T::WN
template <class F>
inline void for_tile(int tile_id, F&& f) {
    switch (tile_id) {
        case 0: f(TileT<2, 2, 2, 2>{}); break;
        case 1: f(TileT<2, 1, 2, 2>{}); break;
        case 2: f(TileT<1, 1, 4, 1>{}); break;
        case 3: f(TileT<1, 2, 2, 2>{}); break;
        default: f(TileT<1, 1, 2, 2>{}); break;
    }
}
// a run-time flag as a template argument: f(std::true_type{}) / f(std::false_type{})
template <class F>
inline void for_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// taps-folded-into-N forward paths: eligibility and workspace (floats)
inline bool s2b_tapn_ok(const Geom& g) { return g.Cb <= 8 && g.Ca % KC == 0 && !force_generic(); }
// the one-pass form of it (k_s2b_tapnf): stride 2 onto <= 8 channels (5 .. 8: two launches of <= 4) from 32 / 64 / 128
inline bool tapnf_enabled() {
    static const bool off = pg_exp_env("PATCHGAN_NO_TAPNF") != nullptr;
    return !off;
}
inline bool s2b_tapnf_ok(const Geom& g) {
    return g.s == 2 && g.Cb <= 8 && (g.Ca == 32 || g.Ca == 64 || g.Ca == 128) && !force_generic() && tapnf_enabled();
}
inline bool b2s_tapn_ok(const Geom& g) { return g.Ca <= 8 && g.Cb % KC == 0 && !force_generic(); }
inline size_t s2b_tapn_ws(const Geom& g) {
    return ((size_t)16 * g.Cb * g.Ca + (size_t)g.N * g.Hs * g.Ws * 16 * g.Cb) * sizeof(float) + 256;
}
inline size_t b2s_tapn_ws(const Geom& g) { return (size_t)g.N * g.Hb * g.Wb * 16 * g.Ca * sizeof(float); }

inline bool tapkp_enabled() {          // PATCHGAN_TAPK_ONESHOT=1 (experiment): the one-shot k_b2s_tapk instead of the persistent k_b2s_tapkp
    static const bool off = [] {
        const char* e = pg_exp_env("PATCHGAN_TAPK_ONESHOT");
        return e && e[0] == '1';
    }();
    return !off;
}
// persistent taps-in-N weight gradient (k_wgrad_tapnp): <= 4 big-side channels, enough 128-pixel tiles to give every workgroup a few
inline int wgrad_tapnp_slabs(const Geom& g) {
    const long tiles = ((long)g.N * g.Hs * g.Ws + 127) / 128;
    const long rows = (g.Ca + (g.Cb <= 2 ? 127 : 63)) / (g.Cb <= 2 ? 128 : 64);
    return (int)std::max<long>(1, std::min<long>(tiles, 512 / rows));
}
inline bool wgrad_tapnp_ok(const Geom& g) {
    return g.Cb <= 4 && g.Ca % 4 == 0 && (long)g.N * g.Hs * g.Ws >= 4096 && (long)g.N * g.Hs * g.Ws < 0x3fffffL * 64 && !force_generic() &&
           tapkp_enabled();
}
// chunks per sample of the persistent image-facing kernel's InstanceNorm partial sums (2 per 128-pixel tile: one per wave row); 0: n/a
inline int tapkp_stats_chunks(const Geom& g) {
    const long hw = (long)g.Hs * g.Ws;
    if (g.Cb > 4 || g.Ca % 4 != 0 || hw % 128 != 0 || (g.Ca <= 8 && g.Cb % KC == 0) || force_generic()) return 0;
    return (int)(2 * (hw / 128));
}
inline bool tapk_enabled() {
    static const bool off = [] {
        const char* e = pg_exp_env("PATCHGAN_NO_TAPK");
        return e && e[0] == '1';
    }();
    return !off;
}
// Per-call tuning: the PG_TUNE_* bits of the `algo` argument over the process-wide defaults (the PATCHGAN_* environment
// switches, read once: they exist for same-device A/B timing; tests and callers use the bits).
struct Tune {
    bool wino;      // any Winograd path
    bool winow;     // stride-1 Winograd weight gradient
    int wino2;      // polyphase stride-2 forward / data gradient: 0 off, 1 wherever the geometry allows, 2 size heuristic
    int wino2w;     // polyphase stride-2 weight gradient: same codes
    int mo1;        // stride-1 tile edge: 0 heuristic, 2 / 3 pinned
    int dma;        // stride-1 GEMM staging: 0 registers, 1 LDS-DMA ring for F(3x3,4x4), 2 also for 64-tile F(2x2,4x4)
    bool bf16x;     // PG_ALGO_BF16 on bf16 tensors: the LDS-DMA kernels of conv_bf16.hip (off: the register-staged k_*_bf16)
    int bf16ring;   // ... their staging: 1 three-stage ring of 32-wide chunks, 0 one buffer of 64-wide chunks, -1 per-layer default
    bool s3;        // polyphase Winograd GEMMs in split-bf16 form (k_wino_bgemm_s3) instead of v_mfma_f32_32x32x2_f32 (k_wino_bgemm)
    bool s3w;       // the Winograd weight-gradient GEMMs likewise (k_wino_wgrad_gemm_s3 instead of k_wino_wgrad_gemm)
    bool s3r;       // the row-fused stride-1 F(3x3,4x4) GEMM likewise (k_wino_gemm_row_s3 instead of k_wino_gemm_row)
};
inline int env_int(const char* name, int dflt) {
    const char* e = pg_exp_env(name);
    return e ? atoi(e) : dflt;
}
inline Tune tune_of(int algo) {
    static const Tune env = [] {
        Tune t;
        t.wino = env_int("PATCHGAN_NO_WINOGRAD", 0) != 1;
        t.winow = env_int("PATCHGAN_NO_WINOGRAD_WGRAD", 0) != 1;
        t.wino2 = env_int("PATCHGAN_WINO2", 2);
        t.wino2w = env_int("PATCHGAN_WINO2_WGRAD", 2);
        t.mo1 = env_int("PATCHGAN_WINO1_TILE", 0);
        t.dma = pg_wino_dma_mode();
        t.bf16x = env_int("PATCHGAN_NO_BF16X", 0) != 1;
        t.bf16ring = -1;      // (pinned only per call: PG_TUNE_BF16X_RING / _FLAT)
        t.s3 = env_int("PATCHGAN_S3", 1) != 0;
        t.s3w = env_int("PATCHGAN_S3W", 1) != 0;
        t.s3r = env_int("PATCHGAN_S3R", 1) != 0;
        return t;
    }();
    Tune t = env;
    if (algo & PG_TUNE_WINO_OFF) t.wino = false;
    if (algo & PG_TUNE_WINOW_OFF) t.winow = false;
    if (algo & PG_TUNE_WINO2_ALL) t.wino2 = 1;
    if (algo & PG_TUNE_WINO2_OFF) t.wino2 = 0;
    if (algo & PG_TUNE_WINO2W_ALL) t.wino2w = 1;
    if (algo & PG_TUNE_WINO2W_OFF) t.wino2w = 0;
    if (algo & PG_TUNE_WINO1_F2) t.mo1 = 2;
    if (algo & PG_TUNE_WINO1_F3) t.mo1 = 3;
    if (algo & PG_TUNE_WINO_DMA) t.dma = 2;
    if (algo & PG_TUNE_BF16X_OFF) t.bf16x = false;
    if (algo & PG_TUNE_BF16X_RING) t.bf16ring = 1;
    if (algo & PG_TUNE_BF16X_FLAT) t.bf16ring = 0;
    if (algo & PG_TUNE_S3_OFF) t.s3 = t.s3w = t.s3r = false;
    if (force_generic()) t.wino = t.bf16x = false;
    return t;
}
// every path on, for sizing a workspace that serves any tuning
inline Tune tune_widest(int mo1) { return Tune{true, true, 1, 1, mo1, 0, true, -1, true, true, true}; }

// stride-1 layers only: forward is a pad-1 correlation big -> small, the data gradient a pad-2 correlation small -> big
inline bool wino_b2s_ok(const Geom& g, const Tune& t) {
    return g.s == 1 && t.wino && pg_wino_geom_ok(g.N, g.Hs, g.Ws, g.Cb, g.Ca, t.mo1);
}
inline bool wino_s2b_ok(const Geom& g, const Tune& t) {
    return g.s == 1 && t.wino && pg_wino_geom_ok(g.N, g.Hb, g.Wb, g.Ca, g.Cb, t.mo1);
}
// stride-2 big -> small polyphase Winograd: where the channel counts are large against the tile count (measured per
// layer of cfg2, tools/layer_bench.py) unless the tuning forces it on / off
inline bool wino2_b2s_ok(const Geom& g, const Tune& t) {
    if (g.s != 2 || t.wino2 == 0 || !t.wino || !pg_wino2_geom_ok(g.N, g.Hs, g.Ws, g.Ca, g.Cb)) return false;
    if (t.wino2 == 1) return true;
    // measured on the cfg2 layers (F(3x3,2x2)): 128->256 ch -31 %, 256->512 on 16x16 -11 %, 256->1024 -25 %, 128->512 -35 %,
    // 64->256 -18 %, 64->128 -10..-16 %; 512->512 on 8x8 and smaller maps slower (weight transform dominates)
    return pg_wino2_tiles_b2s(g.N, g.Hs, g.Ws) >= 512 && g.Cb >= 64 && g.Ca >= 128;
}
inline bool wino2_s2b_ok(const Geom& g, const Tune& t) {
    if (g.s != 2 || t.wino2 == 0 || !t.wino || !pg_wino2c_geom_ok(g.N, g.Hb, g.Wb, g.Ca, g.Cb)) return false;
    if (t.wino2 == 1) return true;
    // measured on the cfg2 layers (F(3x3,2x2), shared windows): 128->64 ch -16..-18 %, 256->128 -23..-27 %, 512->256 -22 %,
    // 1024->256 -28 %, 512->128 -38 %, 256->64 -27 %; 8x8 maps and smaller: no gain (weight transform dominates)
    return pg_wino2_tiles_s2b(g.N, g.Hb, g.Wb) >= 512 && g.Cb >= 64 && g.Ca >= 128;
}
inline bool wino2_wgrad_ok(const Geom& g, const Tune& t) {
    if (g.s != 2 || t.wino2w == 0 || !t.wino || !pg_wino2_wgrad_geom_ok(g.N, g.Hs, g.Ws, g.Ca, g.Cb)) return false;
    if (t.wino2w == 1) return true;
    // measured on the cfg2 layers (64x64 output tiles unless 128x128 ones alone fill the chip): 256x128 ch -16 %, 512x256 -20 %,
    // 512x128 -17 %, 256x64 -15 %, 1024x256 +-0; 128 small-side channels: +35 % in round 1, -8 ... -13 % since the XCD-contiguous
    // 4-waves-per-SIMD form of the GEMM (enc1 184 -> 170, d1 at 2N 319 -> 277 us, before counting the V it now gets from the forward
    // call) -- taken where the K dimension is long (>= 4096 tiles)
    const long T = (long)g.N * ((g.Hs + 2) / 3) * ((g.Ws + 2) / 3);
    return g.Cb >= 64 && ((T >= 512 && g.Ca >= 256) || (T >= 4096 && g.Ca >= 128));
}
inline bool wino_wgrad_ok(const Geom& g, const Tune& t) {
    return g.s == 1 && t.winow && t.wino && pg_wino_wgrad_geom_ok(g.N, g.Hs, g.Ws, g.Ca, g.Cb);
}

// small -> big from a one-channel small (fp32) onto Cb % 4 == 0 channels, 256 % (Cb / 4) == 0: k_s2b_ca1; fp32 output under any
// MFMA algo, bf16 output (PG_IO_BIG_BF16 alone) under PG_ALGO_BF16
inline bool s2b_ca1_ok(const Geom& g, int algo_full) {
    const int a = algo_full & PG_ALGO_MASK, io = algo_full & PG_IO_MASK;
    if (g.Ca != 1 || g.Cb % 4 != 0 || g.Cb > 1024 || 256 % (g.Cb / 4) != 0 || a == PG_ALGO_DIRECT || force_generic()) return false;
    return io == 0 || (io == PG_IO_BIG_BF16 && a == PG_ALGO_BF16);
}
// PG_ALGO_BF16 with the input activation stored as bf16: the LDS-DMA kernels of conv_bf16.hip (dir 0: big -> small, 1: small -> big)
inline bool bf16x_ok(const Geom& g, int dir, int algo_full, const Tune& t) {
    if ((algo_full & PG_ALGO_MASK) != PG_ALGO_BF16 || !t.bf16x) return false;
    if (!(algo_full & (dir == 0 ? PG_IO_BIG_BF16 : PG_IO_SMALL_BF16))) return false;
    // big -> small from a few-channel `big`: the 8-channel-pixel form (dir 2; the caller also checks ld_big == 8)
    if (dir == 0 && g.Cb <= 8) return pg_bf16x_geom_ok(2, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, g.Cb, g.s);
    return pg_bf16x_geom_ok(dir, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, g.Cb, g.s);
}
// small -> big onto a few-channel `big` from a bf16 `small`: row GEMM on the bf16 kernels (dir 3) + k_col2im_small2big; fp32 output
inline bool bf16x_s2b_tapn_ok(const Geom& g, int algo_full, const Tune& t) {
    if ((algo_full & PG_ALGO_MASK) != PG_ALGO_BF16 || !t.bf16x) return false;
    if ((algo_full & PG_IO_MASK) != PG_IO_SMALL_BF16 || g.Cb > 8) return false;
    return pg_bf16x_geom_ok(3, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, 16 * g.Cb, g.s);
}
inline bool s2b_tapnf_bf_ok(const Geom& g, int algo_full, const Tune& t) {
    if ((algo_full & PG_ALGO_MASK) != PG_ALGO_BF16 || !t.bf16x || (algo_full & PG_IO_MASK) != PG_IO_SMALL_BF16) return false;
    return s2b_tapnf_ok(g);
}
inline long tapnf_blocks(const Geom& g) {
    return (long)g.N * ((g.Hb + 2 * TF_H - 2) / (2 * TF_H - 2)) * ((g.Wb + 2 * TF_W - 2) / (2 * TF_W - 2));
}
// its workgroups per chip by LDS and registers: 2 per CU for 128 fp32 input channels, else 3
inline int tapnf_wgs(const Geom& g, bool bf) {
    static const int wgs_env = pg_exp_env("PATCHGAN_TAPNF_WG") ? atoi(pg_exp_env("PATCHGAN_TAPNF_WG")) : 0;
    return wgs_env > 0 ? wgs_env : (g.Ca == 128 && !bf) ? 512 : 768;
}
// one launch of k_s2b_tapnf (the planner has checked eligibility, alignment and the 32-bit offset limits)
static int launch_tapnf(bool bf, const void* small, int ld_small, const float* P, const float* bias, float* big, int ld_big, const Geom& g,
                        int act, long small_bytes, long big_bytes, hipStream_t st) {
    const int nbh = (g.Hb + 2 * TF_H - 2) / (2 * TF_H - 2), nbw = (g.Wb + 2 * TF_W - 2) / (2 * TF_W - 2);
    const long nb = tapnf_blocks(g);
    if (nb >= 0x7fffffffL) return PG_EINVAL;
    const dim3 grid((unsigned)std::min<long>(nb, tapnf_wgs(g, bf)));
    const int v4 = (g.Cb % 4 == 0 && ld_big % 4 == 0 && aligned16(big)) ? 1 : 0;
    const int sb = (int)small_bytes, bb = (int)big_bytes;
    TimedLaunch timed(st);
#define PG_TAPNF(CBv, KKv, BFv)                                                                                                     \
    hipLaunchKernelGGL((k_s2b_tapnf<CBv, KKv, BFv>), grid, dim3(256), 0, st, small, ld_small, P, bias, big, ld_big, g, act, sb, bb, nbh, nbw, \
                       (int)nb, v4, g.Cb, b0)
#define PG_TAPNF_K(CBv)                                                                                                             \
    if (bf) {                                                                                                                       \
        switch (g.Ca) {                                                                                                             \
            case 32: PG_TAPNF(CBv, 1, true); break;                                                                                 \
            case 64: PG_TAPNF(CBv, 2, true); break;                                                                                 \
            default: PG_TAPNF(CBv, 4, true); break;                                                                                 \
        }                                                                                                                           \
    } else {                                                                                                                        \
        switch (g.Ca) {                                                                                                             \
            case 32: PG_TAPNF(CBv, 2, false); break;                                                                                \
            case 64: PG_TAPNF(CBv, 4, false); break;                                                                                \
            default: PG_TAPNF(CBv, 8, false); break;                                                                                \
        }                                                                                                                           \
    }
    for (int b0 = 0; b0 < g.Cb; b0 += 4) {
        switch (std::min(4, g.Cb - b0)) {
            case 1: PG_TAPNF_K(1) break;
            case 2: PG_TAPNF_K(2) break;
            case 3: PG_TAPNF_K(3) break;
            default: PG_TAPNF_K(4) break;
        }
        if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
    }
#undef PG_TAPNF_K
#undef PG_TAPNF
    return PG_OK;
}
inline size_t bf16x_s2b_tapn_ws(const Geom& g) {
    return pg_bf16x_w_bytes(g.Ca, g.Cb) + (size_t)g.N * g.Hs * g.Ws * 16 * g.Cb * sizeof(float);
}
// packed bf16 weights (unless the caller owns them) followed by the split-K slabs
inline size_t bf16x_ws(const Geom& g, int dir) {
    if (dir == 0 && g.Cb <= 8) dir = 2;
    const pg_bf16x_plan p = pg_bf16x_plan_of(dir, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, g.Cb, g.s, -1);
    return pg_bf16x_w_bytes(g.Ca, g.Cb) + (p.split > 1 ? (size_t)p.split * p.out_elems * sizeof(float) : 0);
}
inline bool bf16x_wgrad_ok(const Geom& g, int algo_full, const Tune& t) {
    if ((algo_full & PG_ALGO_MASK) != PG_ALGO_BF16 || !t.bf16x || (algo_full & PG_IO_MASK) != PG_IO_MASK) return false;
    return pg_bf16x_wgrad_geom_ok(g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, g.Cb, g.s);
}
inline bool aligned_bf_view(const void* p, int ld, bool bf) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld % (bf ? 8 : 4)) == 0;
}

// ------------------------------------------------------------------------------------------------
// The planner: which path a call takes is decided HERE, once, in launch order.  The entry points plan with the views of the
// call and switch on ConvPlan::path; the pg_conv_* queries plan with Views == nullptr (16-byte-aligned contiguous tensors
// below pg_conv_max_tensor_bytes, no bias, identity activation -- what the header promises for them) and read fields.
// ------------------------------------------------------------------------------------------------
enum class Path {
    Direct,                                                                                    // PG_ALGO_DIRECT
    Ca1, Wino1, Wino2, Bf16x, Bf16xTapn, TapnfBf, Tapnf, TapnRowGemm, Tapkp, Tapk, Gemm,       // big -> small / small -> big
    WinoWgrad, Wino2Wgrad, Bf16xWgrad, WgradTapnp, WgradTapn                                   // weight gradient (and Gemm)
};

// what only a launch knows
struct Views {
    const void *small, *big;
    int ld_small, ld_big;
    const float *P, *bias;     // ops 0 / 1: the packed weights and the epilogue's bias; op 2: dP and dbias
    int act;
    void* ws;
    const pg_conv_extras* x;   // never null
};
static const pg_conv_extras NO_EXTRAS = {nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, 0, 0, 0};
// hand-overs a query asks about (a launch reads them from Views::x)
enum { OFFER_PART = 1, OFFER_U = 2, OFFER_V = 4, OFFER_MUL = 8 };

struct ConvPlan {
    int rc = PG_OK;            // PG_EINVAL: the call passes a hand-over (or bf16 tensors) to a path that has no use for it
    Path path = Path::Gemm;    // what the entry point launches
    Path mfma = Path::Gemm;    // ... if it were not PG_ALGO_DIRECT (pg_conv_describe documents "the MFMA path"); else == path
    Plan gemm{};               // the implicit-GEMM plan, split clamped to the workspace (pg_conv_describe reports it beside Wino1 / WgradTapnp)
    pg_bf16x_plan bx{};        // Bf16x / Bf16xTapn / Bf16xWgrad
    int xdir = 0;              // Bf16x: direction of conv_bf16.h (2: 8-channel pixels)
    Tile tile{};               // Gemm / WgradTapn / TapnRowGemm: output tile of the main kernel
    int split = 1;             // split-K factor (slabs) of the main kernel
    long workgroups = 0;
    bool fast = false, pow2 = false;    // implicit GEMM: buffer-load variant, its power-of-two pixel decode (op 2)
    int veck = 0, vecn = 0, mode = 0;   // its vector-access flags (op 2: of `small` / `big`); op 2: wgrad_mode()
    int mo = 0;                         // Wino1: output tile edge
    bool small_tile = false, mz = false;   // Wino1: 64-tile rows, Wino2: 64-row tiles, Wino*Wgrad: 64x64 output tiles; Wino2: k_wino_bgemm_mz
    bool ca1_s1 = false;                // Ca1: the LDS-staged per-sample form
    int vec4 = 0, vec_out = 0;          // Tapk / Tapkp
    size_t reserved = 0;       // op 2: bytes of the workspace that hold the bias gradient's column sums
    size_t ws_needed = 0;      // the largest workspace any path this geometry / algo is eligible for asks for
    size_t u_bytes = 0;        // cached weight transform / pack the path reads (0: none)
    int stats_chunks = 0;      // InstanceNorm partial-sum chunks per sample its epilogue writes (0: none)
    bool mul_ok = false;       // its epilogue takes pg_conv_extras.mul_t
};

// which pack of the weights a Bf16x call reads.  small -> big reads the SAME packed copy as big -> small (transposed staging in the
// kernel): one pack per layer serves both -- not the ring-staged variant (PG_TUNE_BF16X_RING: it keeps the per-tap transposed pack;
// callers that share one cache entry between the two directions of a layer must not set that bit, engine._ucache checks it), and not
// the window-staged kernel, which reads weight fragments straight from global memory (K contiguous per output channel)
inline int bf16x_pack_dir(const ConvPlan& p, int ring) { return p.bx.win ? 4 + p.xdir : p.xdir == 1 ? (ring > 0 ? 1 : 0) : p.xdir; }

struct PlanCtx {
    const Geom& g;
    int algo, io;
    const Tune& tune;
    size_t ws_bytes;
    const Views* v;        // nullptr: a query
    bool part, has_u, has_v, mul;
};
inline void need(ConvPlan& p, size_t bytes) { p.ws_needed = std::max(p.ws_needed, bytes); }
inline ConvPlan& take(ConvPlan& p, Path w) {
    p.mfma = w;
    if (p.path != Path::Direct) p.path = w;
    return p;
}
inline ConvPlan& fail(ConvPlan& p) {
    p.rc = PG_EINVAL;
    return p;
}
inline long gemm_workgroups(const Plan& q) { return (long)q.tiles_m * q.tiles_n * q.ncls * q.split; }
inline bool mul_misaligned(const PlanCtx& c, int elems) {
    return c.v && c.v->x->mul_t && (!aligned16(c.v->x->mul_t) || c.v->x->mul_ld % elems);
}

// the LDS-DMA bf16 kernels (ops 0 / 1).  false: not eligible after all (alignment, workspace) -- the chain goes on to the
// register-staged kernels
bool plan_bf16x(ConvPlan& p, const PlanCtx& c, int dir) {
    const Geom& g = c.g;
    const Views* v = c.v;
    const bool out_bf = c.io & (dir == 0 ? PG_IO_SMALL_BF16 : PG_IO_BIG_BF16);
    const size_t wb = pg_bf16x_w_bytes(g.Ca, g.Cb);
    p.u_bytes = wb;
    need(p, bf16x_ws(g, dir));
    if (c.mul && (dir != 1 || mul_misaligned(c, out_bf ? 8 : 4))) return fail(p), true;
    if (v && c.part && (c.mul || v->bias || v->act != PG_ACT_NONE)) return fail(p), true;
    p.xdir = (dir == 0 && g.Cb <= 8) ? 2 : dir;     // few-channel big: only in 8-channel pixels (16 bytes = one DMA piece per pixel)
    if (v) {
        const void* in = dir == 0 ? v->big : v->small;
        const void* out = dir == 0 ? v->small : v->big;
        const int ld_in = dir == 0 ? v->ld_big : v->ld_small, ld_out = dir == 0 ? v->ld_small : v->ld_big;
        if (p.xdir == 2 && ld_in != 8) return false;
        const long in_pix = (long)g.N * (dir == 0 ? g.Hb * g.Wb : g.Hs * g.Ws);
        if (!aligned_bf_view(in, ld_in, true) || !aligned_bf_view(out, ld_out, out_bf) || !aligned16(v->P) || (v->bias && !aligned16(v->bias)) ||
            tensor_bytes(in_pix, ld_in, p.xdir == 0 ? g.Cb : p.xdir == 2 ? 8 : g.Ca, true) >= FAST_LIMIT)
            return false;
        if (!c.has_u && (!v->ws || !aligned16(v->ws))) return false;
    }
    if (!c.has_u && c.ws_bytes < wb) return false;     // (a cached pack leaves the whole workspace to the slabs)
    p.bx = pg_bf16x_plan_of(p.xdir, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, g.Cb, g.s, c.tune.bf16ring);
    pg_bf16x_clamp(&p.bx, c.has_u ? c.ws_bytes : c.ws_bytes - wb);
    const int chunks = pg_bf16x_stats_chunks(p.xdir, &p.bx, g.N, g.Hb, g.Wb, g.Hs, g.Ws);
    // the queries promise the statistics epilogue and the multiplier only with the full workspace of the path (unsplit K), and the
    // statistics only between bf16 tensors of more than 8 channels
    const bool full_ws = c.ws_bytes >= bf16x_ws(g, dir);
    p.stats_chunks = v ? chunks : (c.io == PG_IO_MASK && p.xdir != 2 && full_ws) ? chunks : 0;
    p.mul_ok = dir == 1 && (v || full_ws);
    if (c.part && (!p.stats_chunks || !out_bf)) return fail(p), true;
    p.split = p.bx.split;
    p.workgroups = (long)p.bx.tiles_m * p.bx.tiles_n * p.bx.ncls * p.bx.split;
    take(p, Path::Bf16x);
    return true;
}

// the Winograd paths of ops 0 / 1 (PG_ALGO_AUTO): F(2x2,4x4) / F(3x3,4x4) of a stride-1 layer, polyphase F(3x3,2x2) of a stride-2 layer.
// true: taken (or the call fails on it)
bool plan_wino(ConvPlan& p, const PlanCtx& c, int op) {
    const Geom& g = c.g;
    const Views* v = c.v;
    if (c.algo != PG_ALGO_AUTO) return false;
    const int Ho = op == 0 ? g.Hs : g.Hb, Wo = op == 0 ? g.Ws : g.Wb, Ci = op == 0 ? g.Cb : g.Ca, Co = op == 0 ? g.Ca : g.Cb, mo1 = c.tune.mo1;
    if (op == 0 ? wino_b2s_ok(g, c.tune) : wino_s2b_ok(g, c.tune)) {
        const size_t wsb = pg_wino_ws_bytes(g.N, Ho, Wo, Ci, Co, mo1);
        need(p, wsb);
        if (c.ws_bytes >= wsb &&
            (!v || (aligned16(v->P) && aligned16(v->ws) &&
                    (op == 0 ? pg_wino_eligible(g.N, g.Hb, g.Wb, g.Cb, g.Hs, g.Ws, g.Ca, v->ld_big, v->big, mo1)
                             : pg_wino_eligible(g.N, g.Hs, g.Ws, g.Ca, g.Hb, g.Wb, g.Cb, v->ld_small, v->small, mo1))))) {
            if (c.part || (op == 1 && mul_misaligned(c, 4))) return fail(p), true;
            if (c.has_v && !(wino_wgrad_ok(g, c.tune) && pg_wino_wgrad_v_bytes(g.N, g.Hs, g.Ws, g.Ca, g.Cb, mo1))) return fail(p), true;
            p.u_bytes = pg_wino_u_bytes(g.N, Ho, Wo, Ci, Co, mo1);
            p.mo = pg_wino_mo(g.N, Ho, Wo, Ci, Co, mo1);
            p.small_tile = pg_wino_small_tile(g.N, Ho, Wo, Ci, Co, mo1);
            p.mul_ok = op == 1;
            return take(p, Path::Wino1), true;
        }
    }
    if (op == 0 ? wino2_b2s_ok(g, c.tune) : wino2_s2b_ok(g, c.tune)) {
        const size_t wsb = op == 0 ? pg_wino2_ws_bytes(g.N, g.Hs, g.Ws, g.Ca, g.Cb) : pg_wino2c_ws_bytes(g.N, g.Hb, g.Wb, g.Ca, g.Cb);
        need(p, wsb);
        if (c.ws_bytes >= wsb && (!v || ((v->ld_big % 4 == 0) && (v->ld_small % 4 == 0) && aligned16(v->big) && aligned16(v->P) &&
                                         aligned16(v->small) && aligned16(v->ws) && (!v->bias || aligned16(v->bias))))) {
            p.stats_chunks = op == 0 ? pg_wino2_b2s_stats_chunks(g.N, g.Hs, g.Ws, g.Ca) : pg_wino2_s2b_stats_chunks(g.N, g.Hb, g.Wb, g.Cb);
            if ((c.part && !p.stats_chunks) || (op == 1 && mul_misaligned(c, 4)) || (c.has_v && pg_wino2_mo() != 3)) return fail(p), true;
            p.u_bytes = pg_wino2_u_bytes(g.Ca, g.Cb);
            const long T = op == 0 ? pg_wino2_tiles_b2s(g.N, g.Hs, g.Ws) : pg_wino2_tiles_s2b(g.N, g.Hb, g.Wb);
            const long X = (long)(pg_wino2_mo() + 1) * (pg_wino2_mo() + 1);
            p.small_tile = T < 1024;
            p.mz = !c.tune.s3 && (op == 0 ? pg_wino2_b2s_zb(g.N, g.Hs, g.Ws, g.Ca) : pg_wino2_s2b_zb(g.N, g.Hb, g.Wb, g.Cb)) > 1;
            p.workgroups = X * ((T + (T >= 1024 ? 127 : 63)) / (T >= 1024 ? 128 : 64)) * (((op == 0 ? g.Ca : 4 * g.Cb) + 127) / 128);
            p.mul_ok = op == 1;
            return take(p, Path::Wino2), true;
        }
    }
    return false;
}

// the row GEMM D[input pixel][(tap, output channel)] of the taps-folded-into-N paths, Nc = 16 * output channels wide
inline ConvPlan& take_row_gemm(ConvPlan& p, long rows, int Nc) {
    p.tile = pick_tile(rows, Nc);
    p.workgroups = ((rows + p.tile.bm - 1) / p.tile.bm) * ((Nc + p.tile.bn - 1) / p.tile.bn);
    return take(p, Path::TapnRowGemm);
}

ConvPlan plan_big2small(const pg_conv_geom* gg, const PlanCtx& c) {
    ConvPlan p;
    const Geom& g = c.g;
    const Views* v = c.v;
    const bool q = !v;
    p.gemm = plan_b2s(gg);
    if (p.gemm.split > 1) need(p, (size_t)p.gemm.split * p.gemm.out_elems * sizeof(float));
    clamp_split(p.gemm, c.ws_bytes, 0);
    const bool in_bf = c.io & PG_IO_BIG_BF16;
    const long p_bytes = 16L * g.Ca * g.Cb * 4;
    p.veck = (g.Cb % 4 == 0) && (q || ((v->ld_big % 4 == 0) && aligned_io(v->big, in_bf) && aligned16(v->P)));
    p.fast = p.veck && g.Cb >= KC && (q || tensor_bytes((long)g.N * g.Hb * g.Wb, v->ld_big, g.Cb, in_bf) < FAST_LIMIT) &&
             p_bytes < FAST_P_LIMIT && !force_generic();
    if (c.algo == PG_ALGO_DIRECT) {
        p.path = Path::Direct;
        if (v) return (c.part || c.has_u || c.has_v) ? fail(p) : p;     // (the direct kernels have no operand to hand over: the queries say 0)
    }
    if (plan_wino(p, c, 0)) return p;
    if (bf16x_ok(g, 0, c.algo | c.io, c.tune) && !c.has_v && plan_bf16x(p, c, 0)) return p;
    p.u_bytes = 0;
    // only the Winograd and Bf16x paths (and, for the partial sums, the persistent image-facing kernel below) have operands to hand over
    if (c.has_v || c.has_u) return fail(p);
    const int kp_chunks = (c.algo == PG_ALGO_AUTO && tapk_enabled() && tapkp_enabled()) ? tapkp_stats_chunks(g) : 0;
    if (c.part && !(kp_chunks > 0 && (q || (!v->bias && v->act == PG_ACT_NONE)))) return fail(p);
    // (the queries report the row-GEMM path whatever the tensor storage, as they always have: engine._bf16_tensors_ok reads "no bf16
    //  kernel" from it and keeps such a layer's tensors fp32; a launch on bf16 tensors goes on to the k_*_bf16 implicit GEMM)
    if ((q || !c.io) && b2s_tapn_ok(g)) {
        need(p, b2s_tapn_ws(g));
        if (c.ws_bytes >= b2s_tapn_ws(g) && (q || ((v->ld_big % 4 == 0) && aligned16(v->big) && aligned16(v->P) && aligned16(v->ws) &&
                                                   tensor_bytes((long)g.N * g.Hb * g.Wb, v->ld_big, g.Cb) < FAST_LIMIT))) {
            // D[big pixel][(tap, a)] = big . P^T (row GEMM over the pixels), then gather the 16 taps per output pixel
            return take_row_gemm(p, (long)g.N * g.Hb * g.Wb, 16 * g.Ca);
        }
    }
    if (g.Cb <= 5 && !c.io && !force_generic() && tapk_enabled()) {     // (6..8 channels: measured slower than the generic kernel)
        // K = 16*Cb <= 48: one-shot kernel (with 4 channels the pipelined generic kernel is as fast: 46 TFLOP/s both)
        const long pix = (long)g.N * g.Hs * g.Ws;
        p.vec4 = (g.Cb == 4) && (q || ((v->ld_big % 4 == 0) && aligned16(v->big)));
        p.vec_out = (g.Ca % 4 == 0) && (q || ((v->ld_small % 4 == 0) && aligned16(v->small) && (!v->bias || aligned16(v->bias))));
        const int tmk = g.Cb <= 4 ? 128 : 64;
        p.workgroups = ((pix + tmk - 1) / tmk) * ((g.Ca + 63) / 64);      // (tiles: the persistent form walks them with fewer workgroups)
        const bool persistent =
            g.Cb <= 4 && tapkp_enabled() && p.vec_out && (g.Cb != 4 || p.vec4) && pix < 0x3fffffL * 64 &&
            (q || ((v->act == PG_ACT_NONE || v->act == PG_ACT_LEAKY) && tensor_bytes((long)g.N * g.Hb * g.Wb, v->ld_big, g.Cb) < FAST_LIMIT &&
                   tensor_bytes(pix, v->ld_small, g.Ca) < FAST_LIMIT));
        if (c.part && !persistent) return fail(p);       // (a view the persistent kernel does not take: unaligned output, tensor beyond 32-bit offsets)
        p.stats_chunks = persistent ? kp_chunks : 0;
        return take(p, persistent ? Path::Tapkp : Path::Tapk);
    }
    if (v && c.io && !p.fast) return fail(p);               // bf16 tensors only on the fast bf16 kernels
    p.tile = p.gemm.t;
    p.split = p.gemm.split;
    p.workgroups = gemm_workgroups(p.gemm);
    return take(p, Path::Gemm);
}

ConvPlan plan_small2big(const pg_conv_geom* gg, const PlanCtx& c) {
    ConvPlan p;
    const Geom& g = c.g;
    const Views* v = c.v;
    const bool q = !v;
    p.gemm = plan_s2b(gg);
    if (p.gemm.split > 1) need(p, (size_t)p.gemm.split * p.gemm.out_elems * sizeof(float));
    clamp_split(p.gemm, c.ws_bytes, 0);
    const bool in_bf = c.io & PG_IO_SMALL_BF16, out_bf = c.io & PG_IO_BIG_BF16;
    const long p_bytes = 16L * g.Ca * g.Cb * 4;
    const long small_pix = (long)g.N * g.Hs * g.Ws, big_pix = (long)g.N * g.Hb * g.Wb;
    p.veck = (g.Ca % 4 == 0) && (q || ((v->ld_small % 4 == 0) && aligned_io(v->small, in_bf)));
    p.vecn = (g.Cb % 4 == 0) && (q || aligned16(v->P));
    p.fast = p.veck && g.Ca >= KC && (q || tensor_bytes(small_pix, v->ld_small, g.Ca, in_bf) < FAST_LIMIT) && p_bytes < FAST_P_LIMIT &&
             !force_generic();
    if (c.algo == PG_ALGO_DIRECT) {
        p.path = Path::Direct;
        if (v) return (c.mul || c.part || c.has_u) ? fail(p) : p;
    }
    if (s2b_ca1_ok(g, c.algo | c.io) && !c.part && !c.has_u &&
        (q || (aligned16(v->P) && (!v->bias || aligned16(v->bias)) && aligned_bf_view(v->big, v->ld_big, out_bf) &&
               (!c.mul || aligned_bf_view(v->x->mul_t, v->x->mul_ld, out_bf))))) {
        static const bool no_s1 = pg_exp_env("PATCHGAN_NO_CA1S1") != nullptr;
        p.ca1_s1 = !no_s1 && g.s == 1 && (size_t)(g.Hs + 4) * (g.Ws + 4) * sizeof(float) <= 48 * 1024 && g.Hb == g.Hs + 1 && g.Wb == g.Ws + 1;
        p.mul_ok = true;
        p.workgroups = 2048;       // (nominal: the launch sizes ~1536 workgroups of whole pixel trips)
        return take(p, Path::Ca1);
    }
    if (plan_wino(p, c, 1)) return p;
    // the two row-GEMM + col2im paths are what the one-pass kernels (k_s2b_tapnf) fall back to on a view they do not take: sized first
    const bool tapn = (q || !c.io) && s2b_tapn_ok(g) /* q: as in plan_big2small */, tapn_bf = bf16x_s2b_tapn_ok(g, c.algo | c.io, c.tune);
    if (tapn) need(p, s2b_tapn_ws(g) + 256);
    if (tapn_bf) need(p, bf16x_s2b_tapn_ws(g) + 256);
    const bool no_extras = !c.part && !c.has_u && !c.mul;
    // the one-pass kernel on a bf16 / an fp32 `small` (the latter below the bf16 row GEMMs in launch order)
    auto tapnf_views = [&](bool bf) {
        return q || ((v->ld_small % (bf ? 8 : 4) == 0) && aligned16(v->small) && tensor_bytes(small_pix, v->ld_small, g.Ca, bf) < FAST_LIMIT &&
                     tensor_bytes(big_pix, v->ld_big, g.Cb) < FAST_LIMIT);
    };
    auto take_tapnf = [&](bool bf) -> ConvPlan& {
        p.workgroups = std::min<long>(tapnf_blocks(g), tapnf_wgs(g, bf));
        return take(p, bf ? Path::TapnfBf : Path::Tapnf);
    };
    if (s2b_tapnf_bf_ok(g, c.algo | c.io, c.tune) && no_extras && tapnf_views(true)) return take_tapnf(true);
    if (tapn_bf && no_extras && c.ws_bytes >= bf16x_s2b_tapn_ws(g) &&
        (q || (v->ws && aligned16(v->ws) && aligned_bf_view(v->small, v->ld_small, true) && aligned16(v->P) &&
               tensor_bytes(small_pix, v->ld_small, g.Ca, true) < FAST_LIMIT))) {
        // D[small pixel][(tap, b)] = small . W' (bf16 row GEMM), then col2im: each big pixel sums the taps that reach it
        p.bx = pg_bf16x_plan_of(3, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, 16 * g.Cb, g.s, 0);
        p.workgroups = (long)p.bx.tiles_m * p.bx.tiles_n;
        return take(p, Path::Bf16xTapn);
    }
    if (bf16x_ok(g, 1, c.algo | c.io, c.tune) && plan_bf16x(p, c, 1)) return p;
    p.u_bytes = 0;
    p.mul_ok = false;
    if (!no_extras) return fail(p);
    if (!c.io && s2b_tapnf_ok(g) && tapnf_views(false)) return take_tapnf(false);
    if (tapn && c.ws_bytes >= s2b_tapn_ws(g) &&
        (q || ((v->ld_small % 4 == 0) && aligned16(v->small) && aligned16(v->P) && aligned16(v->ws) &&
               tensor_bytes(small_pix, v->ld_small, g.Ca) < FAST_LIMIT))) {
        // D[small pixel][(tap, b)] = small . W' (row GEMM), then col2im: each big pixel sums the taps that reach it
        return take_row_gemm(p, small_pix, 16 * g.Cb);
    }
    if (v && c.io && !p.fast) return fail(p);
    p.tile = p.gemm.t;
    p.split = p.gemm.split;
    p.workgroups = gemm_workgroups(p.gemm);
    return take(p, Path::Gemm);
}

// c.has_v: v_pre is passed; Views::bias: dbias (the queries plan with the column sums reserved)
ConvPlan plan_wgrad_conv(const pg_conv_geom* gg, const PlanCtx& c) {
    ConvPlan p;
    const Geom& g = c.g;
    const Views* v = c.v;
    const bool q = !v;
    const size_t colsum = colsum_bytes(g.Ca);
    p.reserved = (q || v->bias) ? colsum : 0;
    p.gemm = plan_wgrad(gg);
    p.mode = wgrad_mode(gg);
    need(p, colsum + (p.gemm.split > 1 ? (size_t)p.gemm.split * p.gemm.out_elems * sizeof(float) : 0));
    clamp_split(p.gemm, c.ws_bytes, p.reserved);
    const long Kp = (long)g.N * g.Hs * g.Ws, big_pix = (long)g.N * g.Hb * g.Wb;
    const bool in_bf = c.io != 0;
    const bool al4 = q || ((v->ld_small % 4 == 0) && (v->ld_big % 4 == 0) && aligned16(v->small) && aligned16(v->big) && aligned16(v->ws));
    if (c.algo == PG_ALGO_DIRECT) {
        need(p, colsum + (size_t)DIRECT_WGRAD_SLICES * p.gemm.out_elems * sizeof(float));
        p.path = Path::Direct;
        if (v) return c.has_v ? fail(p) : p;
    }
    // F(4x4,2x2) / F(4x4,3x3) of a stride-1 layer (w1), polyphase F(2x2,3x3) of a stride-2 layer
    const bool w1 = c.algo == PG_ALGO_AUTO && wino_wgrad_ok(g, c.tune), w2 = c.algo == PG_ALGO_AUTO && wino2_wgrad_ok(g, c.tune);
    if (w1 || w2) {
        const size_t wsb = w1 ? pg_wino_wgrad_ws_bytes(g.N, g.Hs, g.Ws, g.Ca, g.Cb) : pg_wino2_wgrad_ws_bytes(g.N, g.Hs, g.Ws, g.Ca, g.Cb);
        need(p, colsum + wsb);
        if (al4 && (w1 || q || aligned16(v->P)) && c.ws_bytes >= p.reserved + wsb) {
            if (w1 && c.has_v && !pg_wino_wgrad_v_bytes(g.N, g.Hs, g.Ws, g.Ca, g.Cb, c.tune.mo1)) return fail(p);
            p.small_tile = w1 ? pg_wino_wgrad_tile64(g.Ca, g.Cb, c.tune.s3w) : pg_wino2_wgrad_tile64(g.Ca, g.Cb, c.tune.s3w);
            p.split = w1 ? pg_wino_wgrad_slices(g.N, g.Hs, g.Ws, g.Ca, g.Cb, c.tune.s3w) : pg_wino2_wgrad_slices(g.N, g.Hs, g.Ws, g.Ca, g.Cb, c.tune.s3w);
            const int tt = p.small_tile ? 64 : 128;
            p.workgroups = (w1 ? 25L * ((g.Ca + tt - 1) / tt) * ((g.Cb + tt - 1) / tt) : 16L * ((g.Ca + 127) / 128) * ((4 * g.Cb + 127) / 128)) * p.split;
            return take(p, w1 ? Path::WinoWgrad : Path::Wino2Wgrad);
        }
    }
    if (c.has_v) return fail(p);     // pg_conv_v_bytes said 0 for this call: there is no transformed operand to reuse
    if (bf16x_wgrad_ok(g, c.algo | c.io, c.tune)) {
        p.bx = pg_bf16x_wgrad_plan(g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, g.Cb, g.s);
        need(p, colsum + (p.bx.split > 1 ? (size_t)p.bx.split * p.bx.out_elems * sizeof(float) : 0));
        if (q || ((g.Cb > 8 || v->ld_big == 8) && aligned_bf_view(v->small, v->ld_small, true) && aligned_bf_view(v->big, v->ld_big, true) &&
                  aligned16(v->P) && (c.ws_bytes <= p.reserved || aligned16(v->ws)) && tensor_bytes(Kp, v->ld_small, g.Ca, true) < FAST_LIMIT &&
                  tensor_bytes(big_pix, v->ld_big, g.Cb > 8 ? g.Cb : 8, true) < FAST_LIMIT)) {
            // (the queries describe this kernel without a bias gradient: the bf16 networks' convolutions that reach it have no bias)
            const size_t res = q ? 0 : p.reserved;
            pg_bf16x_clamp(&p.bx, c.ws_bytes > res ? c.ws_bytes - res : 0);
            p.split = p.bx.split;
            p.workgroups = (long)p.bx.tiles_m * p.bx.tiles_n * 16 * p.bx.split;
            return take(p, Path::Bf16xWgrad);
        }
    }
    if (v && c.io && p.mode != 0) return fail(p);
    p.tile = p.gemm.t;
    p.split = p.gemm.split;
    p.workgroups = gemm_workgroups(p.gemm);
    p.veck = (g.Ca % 4 == 0) && (q || ((v->ld_small % 4 == 0) && aligned_io(v->small, in_bf)));
    p.vecn = (g.Cb % 4 == 0) && (q || ((v->ld_big % 4 == 0) && aligned_io(v->big, in_bf)));
    if (p.mode == 0) {
        p.pow2 = ((g.Hs & (g.Hs - 1)) == 0) && ((g.Ws & (g.Ws - 1)) == 0);
        p.fast = p.veck && p.vecn && !force_generic() && (p.pow2 || (g.Ws >= 16 && g.Hs >= 2)) &&
                 (q || (tensor_bytes(Kp, v->ld_small, g.Ca, in_bf) < FAST_LIMIT && tensor_bytes(big_pix, v->ld_big, g.Cb, in_bf) < FAST_LIMIT));
        if (v && c.io && !p.fast) return fail(p);
        return take(p, Path::Gemm);
    }
    if (p.mode == 1 && !c.io && wgrad_tapnp_ok(g)) {
        // persistent form: one slab per workgroup column, reduced in workgroup order
        const int G = wgrad_tapnp_slabs(g);
        // (not sized for: it runs where the workspace that the layer's other paths asked for happens to hold its slabs)
        const size_t wsb = (size_t)G * p.gemm.out_elems * sizeof(float);
        if (p.veck && c.ws_bytes >= p.reserved + wsb &&
            (q || (aligned16(v->ws) && (g.Cb != 4 || ((v->ld_big % 4 == 0) && aligned16(v->big))) &&
                   tensor_bytes(Kp, v->ld_small, g.Ca) < FAST_LIMIT && tensor_bytes(big_pix, v->ld_big, g.Cb) < FAST_LIMIT))) {
            p.split = G;
            return take(p, Path::WgradTapnp);
        }
    }
    return take(p, Path::WgradTapn);
}

ConvPlan plan_conv(const pg_conv_geom* gg, int op, int algo_full, const Tune& tune, size_t ws_bytes, const Views* v, int offer = 0) {
    const Geom g = to_geom(gg);
    const pg_conv_extras* x = v ? v->x : &NO_EXTRAS;
    const PlanCtx c{g, algo_full & PG_ALGO_MASK, algo_full & PG_IO_MASK, tune, ws_bytes, v,
                    v ? x->part != nullptr : (offer & OFFER_PART) != 0, v ? x->u_cache != nullptr : (offer & OFFER_U) != 0,
                    v ? (x->v_keep || x->v_pre) : (offer & OFFER_V) != 0, v ? x->mul_t != nullptr : (offer & OFFER_MUL) != 0};
    // a bf16 tensor of FAST_LIMIT bytes or more has no kernel, as an input or as an OUTPUT (patchgan_hip.h, pg_conv_max_tensor_bytes):
    // the paths below check the tensors they gather from, which let a bf16 output beyond the limit through
    if (v && ((c.io & PG_IO_BIG_BF16 && tensor_bytes((long)g.N * g.Hb * g.Wb, v->ld_big, g.Cb, true) >= FAST_LIMIT) ||
              (c.io & PG_IO_SMALL_BF16 && tensor_bytes((long)g.N * g.Hs * g.Ws, v->ld_small, g.Ca, true) >= FAST_LIMIT))) {
        ConvPlan p;
        return fail(p);
    }
    return op == 0 ? plan_big2small(gg, c) : op == 1 ? plan_small2big(gg, c) : plan_wgrad_conv(gg, c);
}

// pg_conv4x4_bwd_big: V(big) computed once for the polyphase weight gradient and data gradient of a stride-2 layer
bool plan_share_v(const Geom& g, int algo_full, const Tune& tune, size_t ws_bytes, bool views_ok, size_t* needed) {
    if (!(wino2_b2s_ok(g, tune) && wino2_wgrad_ok(g, tune))) return false;
    const size_t wsb = pg_wino2_v_bytes(g.N, g.Hs, g.Ws, g.Cb) +
                       std::max(pg_wino2_ws_bytes(g.N, g.Hs, g.Ws, g.Ca, g.Cb), pg_wino2_wgrad_ws_bytes(g.N, g.Hs, g.Ws, g.Ca, g.Cb));
    if (needed) *needed = wsb;
    return (algo_full & PG_ALGO_MASK) == PG_ALGO_AUTO && pg_wino2_mo() == 3 && views_ok && ws_bytes >= wsb;
}

// ---- what the queries report of a plan ----
// pg_conv_describe's documented numbers
void describe_plan(const ConvPlan& p, const Geom& g, int op, int* tile_id, int* split, long* workgroups) {
    const int gemm_code = p.gemm.t.id + (op == 2 ? 10 * p.mode : 0) + (p.fast ? (p.pow2 ? 200 : 100) : 0);
    // beside the Wino1 codes, and for the persistent form of k_wgrad_tapn, the tile / split / workgroups are those of the implicit-GEMM plan
    const bool of_gemm = p.mfma == Path::Wino1 || p.mfma == Path::WgradTapnp;
    int code = gemm_code;
    switch (p.mfma) {
        case Path::Bf16xWgrad: code = 1020 + p.bx.tile; break;
        case Path::Ca1: code = 1050; break;
        case Path::TapnfBf: code = 1070 + g.Cb; break;
        case Path::Tapnf: code = 1060 + g.Cb; break;
        case Path::Bf16xTapn: code = 1030 + p.bx.tile; break;
        case Path::Bf16x: code = p.xdir == 2 ? 1040 + p.bx.tile : 1000 + 100 * (p.bx.win ? 2 : p.bx.ring) + 10 * op + p.bx.tile; break;
        case Path::TapnRowGemm: code = p.tile.id + 30; break;
        case Path::Wino1: code = gemm_code + (p.mo == 3 ? 90 : p.small_tile ? 50 : 40); break;
        case Path::Tapk:
        case Path::Tapkp: code = 80 + g.Cb; break;
        case Path::Wino2: code = (p.small_tile ? 71 : 70) + (p.mz ? 2 : 0); break;
        case Path::Wino2Wgrad: code = p.small_tile ? 62 : 61; break;
        case Path::WinoWgrad: code = p.small_tile ? 63 : 60; break;
        default: break;
    }
    if (tile_id) *tile_id = code;
    if (split) *split = of_gemm ? p.gemm.split : p.split;
    if (workgroups) *workgroups = of_gemm ? gemm_workgroups(p.gemm) : p.workgroups;
}

// FLOPs of the main kernel: executed (ragged tiles padded to whole ones) / useful (the algorithm's count on the exact extents)
void flops_of(const ConvPlan& p, const Geom& g, int op, double* executed, double* useful) {
    // the Winograd kernels' counts, given how many tiles cover an extent (tiles(extent, tile edge)); halo: the polyphase data gradient's
    // extra window per class, counted with the whole tiles only
    auto count = [&](auto tiles, int halo) -> double {
        const int m2 = pg_wino2_mo(), m1 = p.mo == 3 ? 3 : 2, wr = pg_wino_wgrad_r(g.N, g.Hs, g.Ws);
        const int ho = op == 0 ? g.Hs : g.Hb, wo = op == 0 ? g.Ws : g.Wb;
        switch (p.path) {
            case Path::WinoWgrad: return 2.0 * (wr + 3) * (wr + 3) * g.N * tiles(g.Hs, wr) * tiles(g.Ws, wr) * g.Ca * g.Cb;
            case Path::Wino2Wgrad: return 2.0 * 16 * g.N * tiles(g.Hs, 3) * tiles(g.Ws, 3) * g.Ca * 4.0 * g.Cb;
            case Path::Wino2:
                return op == 0 ? 2.0 * (m2 + 1) * (m2 + 1) * g.N * tiles(g.Hs, m2) * tiles(g.Ws, m2) * 4.0 * g.Cb * g.Ca
                               : 2.0 * 4 * (m2 + 1) * (m2 + 1) * g.N * tiles(tiles(g.Hb, 2) + halo, m2) * tiles(tiles(g.Wb, 2) + halo, m2) * (double)g.Ca * g.Cb;
            case Path::Wino1: return 2.0 * (m1 + 3) * (m1 + 3) * g.N * tiles(ho, m1) * tiles(wo, m1) * (double)g.Ca * g.Cb;
            default: return 2.0 * g.N * g.Hs * g.Ws * 16.0 * g.Ca * g.Cb;
        }
    };
    if (executed)
        *executed = p.path == Path::WinoWgrad ? pg_wino_wgrad_flops(g.N, g.Hs, g.Ws, g.Ca, g.Cb) : count([](long a, long b) { return (a + b - 1) / b; }, 1);
    if (useful) *useful = count([](double a, double b) { return a / b; }, 0);
}

// the kernel symbol of the main kernel (profiling only: the one place that formats text)
void name_of(const ConvPlan& p, const Geom& g, int op, int algo_full, const Tune& tune, char* buf, size_t len) {
    static const char* const TILE[5] = {"2,2,2,2", "2,1,2,2", "1,1,4,1", "1,2,2,2", "1,1,2,2"};
    const char* tl = TILE[p.tile.id];
    const bool bf = p.path == Path::TapnfBf;
    switch (p.path) {
        case Path::Direct: snprintf(buf, len, "%s", op == 0 ? "k_big2small_direct" : op == 1 ? "k_small2big_direct" : "k_wgrad_direct"); break;
        case Path::Tapnf:
        case Path::TapnfBf:       // one-pass taps-in-N ConvTranspose2d onto <= 4 channels; 5 .. 8 channels: two launches
            if (g.Cb <= 4) snprintf(buf, len, "k_s2b_tapnf<%d%s>", g.Cb, bf ? ",bf16" : "");
            else snprintf(buf, len, "k_s2b_tapnf<4%s>+k_s2b_tapnf<%d%s>", bf ? ",bf16" : "", g.Cb - 4, bf ? ",bf16" : "");
            break;
        case Path::Ca1: snprintf(buf, len, p.ca1_s1 ? "k_s2b_ca1_s1" : "k_s2b_ca1"); break;
        case Path::Bf16xWgrad: snprintf(buf, len, "%s", pg_bf16x_wgrad_kernel_name(p.bx.tile)); break;
        case Path::Bf16xTapn: snprintf(buf, len, "%s+k_col2im_small2big", pg_bf16x_kernel_name(3, p.bx.tile, 0)); break;
        case Path::Bf16x:
            snprintf(buf, len, "%s", p.xdir == 2 ? pg_bf16x_kernel_name(2, p.bx.tile, 0) : pg_bf16x_kernel_name(op, p.bx.tile, p.bx.win ? 2 : p.bx.ring));
            break;
        case Path::WinoWgrad:
        case Path::Wino2Wgrad:
            if (tune.s3w) snprintf(buf, len, "k_wino_wgrad_gemm_s3<%s>", p.small_tile ? "1,1,2,2,2,3" : "2,2,2,2,1,2");
            else snprintf(buf, len, "k_wino_wgrad_gemm<%s>", p.small_tile ? "1,1,2,2" : "2,2,2,2");
            break;
        case Path::Tapkp:
        case Path::Tapk: snprintf(buf, len, p.path == Path::Tapkp ? "k_b2s_tapkp<%d>" : "k_b2s_tapk<%d>", g.Cb); break;
        case Path::Wino2:
            if (tune.s3)       // split-bf16 form (the default): 128-row tiles at two waves per SIMD, 64-row tiles at three
                snprintf(buf, len, "k_wino_bgemm_s3<%s>", p.small_tile ? "1,2,2,2,3" : "2,2,2,2,2");
            else
                snprintf(buf, len, "k_wino_bgemm%s<%s>", p.mz ? "_mz" : "", p.small_tile ? "1,2,2,2" : "2,2,2,2");
            break;
        case Path::Wino1:
            if (p.mo == 3 && tune.dma) snprintf(buf, len, "k_wino_gemm_dma<3,4,2>");
            else if (p.mo != 3 && p.small_tile && tune.dma == 2) snprintf(buf, len, "k_wino_gemm_dma<2,3,3>");
            else if (p.mo == 3 && pg_wino_row_on())
                snprintf(buf, len, (tune.s3r && (op == 0 ? g.Cb : g.Ca) % 32 == 0) ? "k_wino_gemm_row_s3<2>" : "k_wino_gemm_row<4,1>");
            else snprintf(buf, len, "k_wino_gemm<%s>", p.mo == 3 ? "1,1,2,2,2,3" : p.small_tile ? "1,1,2,2,4,2" : "2,1,2,2,2,2");
            break;
        case Path::TapnRowGemm: snprintf(buf, len, "k_b2s_fast<%s,true>+%s", tl, op == 0 ? "k_gather_big2small" : "k_col2im_small2big"); break;
        case Path::WgradTapnp: snprintf(buf, len, "k_wgrad_tapnp<%d>", g.Cb); break;
        case Path::WgradTapn: snprintf(buf, len, "k_wgrad_tapn<%s,%d>", tl, p.mode); break;
        case Path::Gemm: {
            const bool half = (algo_full & PG_ALGO_MASK) == PG_ALGO_BF16 && p.fast;
            // bf16 kernels: the trailing template argument says whether the activation operand(s) are stored as bf16 (PG_IO_* bits)
            const int io = algo_full & PG_IO_MASK;
            const char* hin = (op == 0 ? (io & PG_IO_BIG_BF16) : op == 1 ? (io & PG_IO_SMALL_BF16) : io == PG_IO_MASK) ? "true" : "false";
            const char* p2 = p.pow2 ? "true" : "false";
            if (half && op == 0) snprintf(buf, len, "k_b2s_bf16<%s,false,%s>", tl, hin);
            else if (half && op == 1) snprintf(buf, len, "k_s2b_bf16<%s,%s>", tl, hin);
            else if (half) snprintf(buf, len, "k_wgrad_bf16<%s,%s,%s>", tl, p2, hin);
            else if (p.fast && op == 0) snprintf(buf, len, "k_b2s_fast<%s,false>", tl);
            else if (p.fast && op == 1) snprintf(buf, len, "k_s2b_fast<%s>", tl);
            else if (p.fast) snprintf(buf, len, "k_wgrad_fast<%s,%s>", tl, p2);
            else snprintf(buf, len, "%s<%s>", op == 0 ? "k_big2small" : op == 1 ? "k_small2big" : "k_wgrad", tl);
        } break;
    }
}

// a query's plan: `op` carries the algorithm as opcode + 16 * (PG_ALGO_* | PG_IO_* | PG_TUNE_*)
bool query_plan(const pg_conv_geom* g, int op, int algo_full, size_t ws_bytes, int offer, ConvPlan* p) {
    const int algo = algo_full & PG_ALGO_MASK;
    if (!geom_ok(g) || op < 0 || op > 2 || algo < PG_ALGO_AUTO || algo > PG_ALGO_BF16) return false;
    *p = plan_conv(g, op, algo_full, tune_of(algo_full), ws_bytes, nullptr, offer);
    return true;
}

}  // namespace

extern "C" {

size_t pg_conv_max_tensor_bytes(void) { return (size_t)FAST_LIMIT; }

size_t pg_conv_workspace_bytes(const pg_conv_geom* g, int op) {
    if (!geom_ok(g) || op < 0 || op > 3) return 0;
    size_t bytes = 0;
    if (op == 3) {      // pg_conv4x4_bwd_big: its two halves back to back, or V shared + the larger of the two remainders
        bytes = std::max(pg_conv_workspace_bytes(g, 0), pg_conv_workspace_bytes(g, 2));
        size_t shared = 0;
        plan_share_v(to_geom(g), PG_ALGO_AUTO, tune_widest(0), 0, true, &shared);
        return (std::max(bytes, shared) + 255) & ~(size_t)255;
    }
    // what the planner asks for at most, whichever algo, tensor storage and PG_TUNE_* combination the call comes with (every path on;
    // both tile edges of the stride-1 Winograd paths); PG_ALGO_AUTO covers PG_ALGO_MFMA
    static const int ALGOS[] = {PG_ALGO_AUTO, PG_ALGO_DIRECT, PG_ALGO_BF16 | PG_IO_BIG_BF16, PG_ALGO_BF16 | PG_IO_SMALL_BF16,
                                PG_ALGO_BF16 | PG_IO_MASK};
    for (int mo1 = 2; mo1 <= 3; ++mo1)
        for (int a : ALGOS) bytes = std::max(bytes, plan_conv(g, op, a, tune_widest(mo1), 0, nullptr).ws_needed);
    return (bytes + 255) & ~(size_t)255;
}

int pg_conv_time_next(void* ev_start, void* ev_stop) {
    t_ev0 = (hipEvent_t)ev_start;
    t_ev1 = (hipEvent_t)ev_stop;
    t_ev2 = t_ev3 = nullptr;
    return PG_OK;
}

int pg_conv_time_next2(void* ev_start, void* ev_stop, void* ev_start2, void* ev_stop2) {
    t_ev0 = (hipEvent_t)ev_start;
    t_ev1 = (hipEvent_t)ev_stop;
    t_ev2 = (hipEvent_t)ev_start2;
    t_ev3 = (hipEvent_t)ev_stop2;
    return PG_OK;
}

int pg_conv_describe(const pg_conv_geom* g, int op, size_t ws_bytes, int* tile_id, int* split, long* workgroups) {
    ConvPlan p;
    if (!query_plan(g, op & 15, op >> 4, ws_bytes, 0, &p)) return PG_EINVAL;
    describe_plan(p, to_geom(g), op & 15, tile_id, split, workgroups);
    return PG_OK;
}

int pg_conv_kernel(const pg_conv_geom* g, int op, size_t ws_bytes, char* name, size_t name_len, int* split, double* mfma_flops) {
    ConvPlan p;
    if (!query_plan(g, op & 15, op >> 4, ws_bytes, 0, &p)) return PG_EINVAL;
    if (name && name_len) name_of(p, to_geom(g), op & 15, op >> 4, tune_of(op >> 4), name, name_len);
    if (split && p.path == Path::Direct) describe_plan(p, to_geom(g), op & 15, nullptr, split, nullptr);      // (of the MFMA path, as pg_conv_describe)
    else if (split) *split = p.split;
    flops_of(p, to_geom(g), op & 15, mfma_flops, nullptr);
    return PG_OK;
}

int pg_conv_kernel_flops(const pg_conv_geom* g, int op, size_t ws_bytes, double* executed, double* useful) {
    ConvPlan p;
    if (!query_plan(g, op & 15, op >> 4, ws_bytes, 0, &p)) return PG_EINVAL;
    flops_of(p, to_geom(g), op & 15, executed, useful);
    return PG_OK;
}

size_t pg_conv_u_bytes(const pg_conv_geom* g, int op, int algo, size_t ws_bytes) {
    ConvPlan p;
    if ((op != 0 && op != 1) || !query_plan(g, op, algo, ws_bytes, OFFER_U, &p)) return 0;
    return p.rc == PG_OK ? p.u_bytes : 0;
}

int pg_conv_stats_chunks(const pg_conv_geom* g, int op, int algo, size_t ws_bytes) {
    ConvPlan p;
    if ((op != 0 && op != 1) || !query_plan(g, op, algo, ws_bytes, OFFER_PART, &p)) return 0;
    return p.rc == PG_OK ? p.stats_chunks : 0;
}

int pg_conv_mul_ok(const pg_conv_geom* g, int algo, size_t ws_bytes) {
    ConvPlan p;
    if (!query_plan(g, 1, algo, ws_bytes, 0, &p)) return 0;
    return p.mul_ok ? 1 : 0;
}

// kept V: where the forward call and the weight gradient of the layer both take a Winograd path of the same family
size_t pg_conv_v_bytes(const pg_conv_geom* g, int algo, size_t ws_bytes) {
    ConvPlan f, w;
    if (!query_plan(g, 0, algo, ws_bytes, OFFER_V, &f) || f.rc != PG_OK || !query_plan(g, 2, algo, ws_bytes, 0, &w)) return 0;
    if (f.path == Path::Wino1 && w.path == Path::WinoWgrad) return pg_wino_wgrad_v_bytes(g->N, g->Hs, g->Ws, g->Ca, g->Cb, tune_of(algo).mo1);
    if (f.path == Path::Wino2 && w.path == Path::Wino2Wgrad) return pg_wino2_v_bytes(g->N, g->Hs, g->Ws, g->Cb);
    return 0;
}

// the parts of a batch compute what the whole-batch call computes: same path and kernel, no split over K, V kept in both or in neither
int pg_conv_batch_halves_same(const pg_conv_geom* g, int algo, size_t ws_bytes_n, size_t ws_bytes_2n) {
    if (!geom_ok(g) || g->N > (1 << 29)) return 0;
    pg_conv_geom g2 = *g;
    g2.N *= 2;
    ConvPlan a, b;
    if (!geom_ok(&g2) || !query_plan(g, 0, algo, ws_bytes_n, 0, &a) || !query_plan(&g2, 0, algo, ws_bytes_2n, 0, &b)) return 0;
    if (a.rc != PG_OK || b.rc != PG_OK || a.path != b.path || a.split != 1 || b.split != 1) return 0;
    const Tune tune = tune_of(algo);
    if (a.path == Path::Wino1) {
        // the fully fused F(3x3,4x4) GEMM splits its K range by the grid it gets from the batch; the row-fused form never does
        const bool rows = a.mo == 3 && b.mo == 3 && pg_wino_row_on() && !tune.dma;
        if (!rows && (pg_wino_gemm_slices(g->N, g->Hs, g->Ws, g->Cb, g->Ca, tune.mo1) != 1 ||
                      pg_wino_gemm_slices(g2.N, g->Hs, g->Ws, g->Cb, g->Ca, tune.mo1) != 1))
            return 0;
    }
    char na[128], nb[128];
    name_of(a, to_geom(g), 0, algo, tune, na, sizeof na);
    name_of(b, to_geom(&g2), 0, algo, tune, nb, sizeof nb);
    if (strcmp(na, nb) != 0) return 0;
    return (pg_conv_v_bytes(g, algo, ws_bytes_n) != 0) == (pg_conv_v_bytes(&g2, algo, ws_bytes_2n) != 0) ? 1 : 0;
}

int pg_conv_prep_batch(int n, const pg_conv_prep_item* items, void* stream) {
    if (n < 0 || (n > 0 && !items)) return PG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    std::vector<pg_wino_prep> wv;
    std::vector<pg_bf16x_pack_item> bv;
    for (int i = 0; i < n; ++i) {
        const pg_conv_prep_item& it = items[i];
        ConvPlan p;
        if ((it.op != 0 && it.op != 1) || !it.P || !it.u || !aligned16(it.P) || !aligned16(it.u) ||
            !query_plan(&it.g, it.op, it.algo, it.ws_bytes, OFFER_U, &p) || p.rc != PG_OK || !p.u_bytes)
            return PG_EINVAL;
        const int Ca = it.g.Ca, Cb = it.g.Cb;
        if (p.path == Path::Wino1) wv.push_back(it.op == 0 ? pg_wino_prep{it.P, (float*)it.u, Ca, Cb, 0, p.mo, 0} : pg_wino_prep{it.P, (float*)it.u, Cb, Ca, 0, p.mo, 1});
        else if (p.path == Path::Wino2) wv.push_back(pg_wino_prep{it.P, (float*)it.u, Ca, Cb, it.op == 0 ? 1 : 2, 0, 0});
        else bv.push_back(pg_bf16x_pack_item{it.P, it.u, Ca, Cb, bf16x_pack_dir(p, tune_of(it.algo).bf16ring)});
    }
    for (size_t o = 0; o < wv.size(); o += PG_WINO_PREP_MAX) {
        const int rc = pg_wino_prep_batch((int)std::min<size_t>(PG_WINO_PREP_MAX, wv.size() - o), wv.data() + o, st);
        if (rc != PG_OK) return rc;
    }
    for (size_t o = 0; o < bv.size(); o += PG_BF16X_PACK_MAX) {
        const int rc = pg_bf16x_pack_batch((int)std::min<size_t>(PG_BF16X_PACK_MAX, bv.size() - o), bv.data() + o, st);
        if (rc != PG_OK) return rc;
    }
    return PG_OK;
}

}  // extern "C"

namespace {

// ---- one launch function per path ----
struct Call {       // a planned call
    ConvPlan p;
    Views v;
    Geom g;
    int algo, io;   // PG_ALGO_*, PG_IO_* bits
    Tune tune;
    size_t ws_bytes;
    hipStream_t st;
};
inline int launched() { return hipGetLastError() == hipSuccess ? PG_OK : PG_ELAUNCH; }
inline pg_epi_mul mul_of(const Call& c) { return pg_epi_mul{c.v.x->mul_t, c.v.x->mul_ld, c.v.x->mul_act}; }

// Path::Bf16x (dir 0: big -> small, 1: small -> big): pack (or reuse) the weights, main kernel, split-K reduce
int launch_bf16x(const Call& c, int dir) {
    const Geom& g = c.g;
    const ConvPlan& p = c.p;
    const pg_conv_extras& x = *c.v.x;
    const void* in = dir == 0 ? c.v.big : c.v.small;
    void* out = const_cast<void*>(dir == 0 ? c.v.small : c.v.big);
    const int ld_in = dir == 0 ? c.v.ld_big : c.v.ld_small, ld_out = dir == 0 ? c.v.ld_small : c.v.ld_big;
    const bool out_bf = c.io & (dir == 0 ? PG_IO_SMALL_BF16 : PG_IO_BIG_BF16);
    const int Cin = p.xdir == 0 ? g.Cb : p.xdir == 2 ? 8 : g.Ca, Cout = dir == 1 ? g.Cb : g.Ca;
    const long in_pix = (long)g.N * (dir == 0 ? g.Hb * g.Wb : g.Hs * g.Ws), out_pix = (long)g.N * (dir == 0 ? g.Hs * g.Ws : g.Hb * g.Wb);
    const long in_bytes = tensor_bytes(in_pix, ld_in, Cin, true);
    void* W = x.u_cache ? (void*)x.u_cache : c.v.ws;
    float* slabs = (float*)((char*)c.v.ws + (x.u_cache ? 0 : pg_bf16x_w_bytes(g.Ca, g.Cb)));
    const int pack = bf16x_pack_dir(p, c.tune.bf16ring), bt = (p.xdir == 1 && pack == 0) ? 1 : 0;
    if (!(x.u_cache && x.u_valid)) {
        int rc = pg_bf16x_pack(c.v.P, W, g.Ca, g.Cb, pack, c.st);
        if (rc != PG_OK) return rc;
    }
    const pg_epi_mul mul = mul_of(c);
    int rc;
    {
        TimedLaunch timed(c.st);
        if (p.split == 1)
            rc = pg_bf16x_conv(p.xdir, in, ld_in, in_bytes, W, out, ld_out, 0L, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, g.Cb, g.s, &p.bx, c.v.bias, c.v.act,
                               out_bf ? 1 : 0, c.st, mul, x.part, x.part ? p.stats_chunks : 0, bt);
        else
            rc = pg_bf16x_conv(p.xdir, in, ld_in, in_bytes, W, slabs, Cout, p.bx.out_elems, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, g.Cb, g.s, &p.bx,
                               nullptr, 0, 0, c.st, pg_epi_mul{nullptr, 0, 0}, nullptr, 0, bt);
    }
    if (rc != PG_OK || p.split == 1) return rc;
    return launch_reduce(slabs, p.bx.out_elems, p.split, (float*)out, ld_out, out_pix, Cout, c.v.bias, c.v.act, c.st, out_bf ? 1 : 0, mul);
}

// Path::Wino1 (ops 0 / 1): F(2x2,4x4) / F(3x3,4x4) of a stride-1 layer; (Hi, Wi, Ci) the input side, (Ho, Wo, Co) the output side
int launch_wino1(const Call& c, int op) {
    const Geom& g = c.g;
    const pg_conv_extras& x = *c.v.x;
    const int mo1 = c.tune.mo1;
    const float* in = (const float*)(op == 0 ? c.v.big : c.v.small);
    float* out = (float*)const_cast<void*>(op == 0 ? c.v.small : c.v.big);
    const int ld_in = op == 0 ? c.v.ld_big : c.v.ld_small, ld_out = op == 0 ? c.v.ld_small : c.v.ld_big;
    const int Hi = op == 0 ? g.Hb : g.Hs, Wi = op == 0 ? g.Wb : g.Ws, Ci = op == 0 ? g.Cb : g.Ca;
    const int Ho = op == 0 ? g.Hs : g.Hb, Wo = op == 0 ? g.Ws : g.Wb, Co = op == 0 ? g.Ca : g.Cb;
    const pg_epi_mul mul = op == 0 ? pg_epi_mul{nullptr, 0, 0} : mul_of(c);
    // (a kept V that is part of a larger batch's: only the row-fused form reads it -- refused before anything is launched)
    if ((x.v_stride || x.v_tile0) && (op != 0 || !pg_wino_gemm_rows(g.N, Ho, Wo, Ci, Co, mo1, c.tune.dma, out, ld_out, c.v.bias, mul))) return PG_EINVAL;
    int rc = op == 0 ? pg_wino_prepare(in, ld_in, c.v.P, 0, g.N, Hi, Wi, Ci, Ho, Wo, Co, 1, c.v.ws, c.st, mo1, x.u_cache, x.u_valid, x.v_keep,
                                       (long)x.v_stride, (long)x.v_tile0)
                     : pg_wino_prepare(in, ld_in, c.v.P, 1, g.N, Hi, Wi, Ci, Ho, Wo, Co, 2, c.v.ws, c.st, mo1, x.u_cache, x.u_valid);
    if (rc != PG_OK) return rc;
    const int nsl = pg_wino_gemm_rows(g.N, Ho, Wo, Ci, Co, mo1, c.tune.dma, out, ld_out, c.v.bias, mul) ? 1 : pg_wino_gemm_slices(g.N, Ho, Wo, Ci, Co, mo1);
    {
        TimedLaunch timed(c.st);
        rc = pg_wino_gemm(c.v.bias, out, ld_out, g.N, Ci, Ho, Wo, Co, c.v.act, c.v.ws, c.st, mo1, c.tune.dma, x.u_cache, mul, op == 0 ? x.v_keep : nullptr,
                          c.tune.s3r, (long)x.v_stride, (long)x.v_tile0);
    }
    if (rc != PG_OK || nsl == 1) return rc;
    const long pix = (long)g.N * Ho * Wo;
    return launch_reduce(pg_wino_gemm_slabs(c.v.ws, g.N, Ho, Wo, Ci, Co, mo1), pix * Co, nsl, out, ld_out, pix, Co, c.v.bias, c.v.act, c.st, 0, mul);
}

// Path::Wino2 (ops 0 / 1): polyphase Winograd of a stride-2 layer (times its own main GEMM)
int launch_wino2(const Call& c, int op) {
    const Geom& g = c.g;
    const pg_conv_extras& x = *c.v.x;
    hipEvent_t e0 = t_ev0, e1 = t_ev1;
    t_ev0 = nullptr;
    t_ev1 = nullptr;
    if (op == 0)
        return pg_wino2_b2s((const float*)c.v.big, c.v.ld_big, c.v.P, c.v.bias, (float*)const_cast<void*>(c.v.small), c.v.ld_small, g.N, g.Hb, g.Wb, g.Hs,
                            g.Ws, g.Ca, g.Cb, c.v.act, c.v.ws, c.st, e0, e1, nullptr, x.part, x.v_keep, x.u_cache, x.u_valid, c.tune.s3, (long)x.v_stride,
                            (long)x.v_tile0);
    return pg_wino2_s2b((const float*)c.v.small, c.v.ld_small, c.v.P, c.v.bias, (float*)const_cast<void*>(c.v.big), c.v.ld_big, g.N, g.Hb, g.Wb, g.Hs, g.Ws,
                        g.Ca, g.Cb, c.v.act, c.v.ws, c.st, e0, e1, x.part, x.u_cache, x.u_valid, mul_of(c), c.tune.s3);
}

// Path::TapnRowGemm (ops 0 / 1): D[input pixel][(tap, output channel)] = in . W (row GEMM over the pixels) into the workspace; the
// caller gathers (op 0) / scatters (op 1) the 16 taps
int launch_row_gemm(const Call& c, const float* in, int ld_in, const float* W, float* D, long M, int Hi, int Wi, int Cin, int Nc) {
    const Tile& t = c.p.tile;
    Geom g1{c.g.N, Hi, Wi, Hi, Wi, Nc, Cin, 1};
    dim3 grid((unsigned)((M + t.bm - 1) / t.bm), (Nc + t.bn - 1) / t.bn, 1);
    TimedLaunch timed(c.st);
    for_tile(t.id, [&](auto tt) {
        using T = decltype(tt);
        hipLaunchKernelGGL((k_b2s_fast<PG_TILE(T), true>), grid, dim3(256), 0, c.st, in, ld_in, W, D, Nc, 0L, g1, Cin / KC, (const float*)nullptr, 0,
                           (int)tensor_bytes(M, ld_in, Cin), (int)((long)Nc * Cin * 4));
    });
    return launched();
}

// Path::Gemm of ops 0 / 1: the implicit GEMM straight into the output, or split-K slabs + reduce
int launch_gemm(const Call& c, int op) {
    const Geom& g = c.g;
    const ConvPlan& p = c.p;
    const Plan& q = p.gemm;
    hipStream_t st = c.st;
    const float* in = (const float*)(op == 0 ? c.v.big : c.v.small);
    float* out = (float*)const_cast<void*>(op == 0 ? c.v.small : c.v.big);
    const int ld_in = op == 0 ? c.v.ld_big : c.v.ld_small, ld_out = op == 0 ? c.v.ld_small : c.v.ld_big, Cout = op == 0 ? g.Ca : g.Cb;
    const long in_pix = (long)g.N * (op == 0 ? g.Hb * g.Wb : g.Hs * g.Ws), out_pix = (long)g.N * (op == 0 ? g.Hs * g.Ws : g.Hb * g.Wb);
    const bool in_bf = c.io & (op == 0 ? PG_IO_BIG_BF16 : PG_IO_SMALL_BF16), out_bf = c.io & (op == 0 ? PG_IO_SMALL_BF16 : PG_IO_BIG_BF16);
    const bool split = q.split > 1;
    float* dst = split ? (float*)c.v.ws : out;
    const int ld_dst = split ? Cout : ld_out, act = split ? 0 : c.v.act, obf = split ? 0 : (int)out_bf;
    const long stride = split ? q.out_elems : 0L;
    const float *P = c.v.P, *bias = split ? nullptr : c.v.bias;
    const int in_bytes = (int)tensor_bytes(in_pix, ld_in, op == 0 ? g.Cb : g.Ca, in_bf), p_bytes = (int)(16L * g.Ca * g.Cb * 4);
    dim3 grid(q.tiles_m, q.tiles_n, q.ncls * q.split);
    {
        TimedLaunch timed(st);
        for_tile(q.t.id, [&](auto tt) {
            using T = decltype(tt);
            if (p.fast && c.algo == PG_ALGO_BF16)
                for_bool(in_bf, [&](auto hin) {
                    constexpr bool HIN = decltype(hin)::value;
                    if (op == 0)
                        hipLaunchKernelGGL((k_b2s_bf16<PG_TILE(T), false, HIN>), grid, dim3(256), 0, st, in, ld_in, P, dst, ld_dst, stride, g, q.cps, bias, act,
                                           in_bytes, p_bytes, obf);
                    else
                        hipLaunchKernelGGL((k_s2b_bf16<PG_TILE(T), HIN>), grid, dim3(256), 0, st, in, ld_in, P, dst, ld_dst, stride, g, q.cps, bias, act, in_bytes,
                                           p_bytes, obf);
                });
            else if (p.fast && op == 0)
                hipLaunchKernelGGL((k_b2s_fast<PG_TILE(T), false>), grid, dim3(256), 0, st, in, ld_in, P, dst, ld_dst, stride, g, q.cps, bias, act,
                                   in_bytes, p_bytes);
            else if (p.fast)
                hipLaunchKernelGGL((k_s2b_fast<PG_TILE(T)>), grid, dim3(256), 0, st, in, ld_in, P, dst, ld_dst, stride, g, q.cps, bias, act, in_bytes,
                                   p_bytes);
            else if (op == 0)
                hipLaunchKernelGGL((k_big2small<PG_TILE(T)>), grid, dim3(256), 0, st, in, ld_in, P, dst, ld_dst, stride, g, q.cps, p.veck, bias, act);
            else
                hipLaunchKernelGGL((k_small2big<PG_TILE(T)>), grid, dim3(256), 0, st, in, ld_in, P, dst, ld_dst, stride, g, q.cps, p.veck, p.vecn, bias,
                                   act);
        });
    }
    if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
    if (!split) return PG_OK;
    return launch_reduce(dst, q.out_elems, q.split, out, ld_out, out_pix, Cout, c.v.bias, c.v.act, st, out_bf);
}

int launch_b2s(const Call& c) {
    const Geom& g = c.g;
    const ConvPlan& p = c.p;
    const pg_conv_extras& x = *c.v.x;
    hipStream_t st = c.st;
    const float* big = (const float*)c.v.big;
    float* small = (float*)const_cast<void*>(c.v.small);
    const float *P = c.v.P, *bias = c.v.bias;
    const int ld_big = c.v.ld_big, ld_small = c.v.ld_small, act = c.v.act;
    const long pix = (long)g.N * g.Hs * g.Ws, big_pix = (long)g.N * g.Hb * g.Wb;
    switch (p.path) {
        case Path::Direct:
            hipLaunchKernelGGL(k_big2small_direct, dim3((int)std::min<long>((pix * g.Ca + 255) / 256, 65536)), dim3(256), 0, st, big, ld_big, P, bias, small,
                               ld_small, g, act);
            return launched();
        case Path::Wino1: return launch_wino1(c, 0);
        case Path::Wino2: return launch_wino2(c, 0);
        case Path::Bf16x: return launch_bf16x(c, 0);
        case Path::TapnRowGemm: {
            float* D = (float*)c.v.ws;
            int rc = launch_row_gemm(c, big, ld_big, P, D, big_pix, g.Hb, g.Wb, g.Cb, 16 * g.Ca);
            if (rc != PG_OK) return rc;
            hipLaunchKernelGGL(k_gather_big2small, dim3((int)std::min<long>((pix * g.Ca + 255) / 256, 8192)), dim3(256), 0, st, D, bias, small, ld_small, g,
                               act);
            return launched();
        }
        case Path::Tapkp: {
            // persistent form: 2 workgroups per CU (two LDS buffers of 9 .. 35 KB, two accumulator sets), each walking tiles blockIdx.x, + gridDim.x, ...
            const int ntiles = (int)((pix + 127) / 128), gy = (g.Ca + 63) / 64;
            static const int pwg = pg_exp_env("PATCHGAN_TAPKP_WG") ? atoi(pg_exp_env("PATCHGAN_TAPKP_WG")) : 512;
            const bool wide = g.Cb == 4 || ((g.Cb == 3) && (ld_big % 4 == 0) && (ld_big >= 4) && aligned16(big));
            // with the statistics epilogue: one workgroup per CU (88 .. 104 KB of LDS); act == none, no bias, whole tiles per sample (planner)
            dim3 pgrid((unsigned)std::min<long>(ntiles, std::max<long>(1, (x.part ? 256 : pwg) / (long)gy)), gy, 1);
            const int big_b = (int)tensor_bytes(big_pix, ld_big, g.Cb), out_b = (int)tensor_bytes(pix, ld_small, g.Ca);
            TimedLaunch timed(st);
            auto go = [&](auto cb, auto wd) {
                constexpr int CB = decltype(cb)::value;
                constexpr bool WD = decltype(wd)::value;
                if (x.part)
                    hipLaunchKernelGGL((k_b2s_tapkp<CB, 0, WD, true>), pgrid, dim3(256), 0, st, big, ld_big, P, small, ld_small, g, bias, big_b, out_b, ntiles,
                                       x.part);
                else if (act == PG_ACT_LEAKY)
                    hipLaunchKernelGGL((k_b2s_tapkp<CB, 1, WD>), pgrid, dim3(256), 0, st, big, ld_big, P, small, ld_small, g, bias, big_b, out_b, ntiles);
                else
                    hipLaunchKernelGGL((k_b2s_tapkp<CB, 0, WD>), pgrid, dim3(256), 0, st, big, ld_big, P, small, ld_small, g, bias, big_b, out_b, ntiles);
            };
            using std::integral_constant;
            switch (g.Cb) {
                case 1: go(integral_constant<int, 1>{}, std::false_type{}); break;
                case 2: go(integral_constant<int, 2>{}, std::false_type{}); break;
                case 3: wide ? go(integral_constant<int, 3>{}, std::true_type{}) : go(integral_constant<int, 3>{}, std::false_type{}); break;
                default: go(integral_constant<int, 4>{}, std::true_type{}); break;
            }
            return launched();
        }
        case Path::Tapk: {
            const int tmk = g.Cb <= 4 ? 128 : 64, vec4 = p.vec4, vec_out = p.vec_out;
            dim3 grid((unsigned)((pix + tmk - 1) / tmk), (g.Ca + 63) / 64, 1);
            TimedLaunch timed(st);
            switch (g.Cb) {
                case 1: hipLaunchKernelGGL(k_b2s_tapk<1>, grid, dim3(256), 0, st, big, ld_big, P, small, ld_small, g, bias, act, vec4, vec_out); break;
                case 2: hipLaunchKernelGGL(k_b2s_tapk<2>, grid, dim3(256), 0, st, big, ld_big, P, small, ld_small, g, bias, act, vec4, vec_out); break;
                case 3: hipLaunchKernelGGL(k_b2s_tapk<3>, grid, dim3(256), 0, st, big, ld_big, P, small, ld_small, g, bias, act, vec4, vec_out); break;
                case 5: hipLaunchKernelGGL((k_b2s_tapk<5, 1>), grid, dim3(256), 0, st, big, ld_big, P, small, ld_small, g, bias, act, 0, vec_out); break;
                case 6: hipLaunchKernelGGL((k_b2s_tapk<6, 1>), grid, dim3(256), 0, st, big, ld_big, P, small, ld_small, g, bias, act, 0, vec_out); break;
                case 7: hipLaunchKernelGGL((k_b2s_tapk<7, 1>), grid, dim3(256), 0, st, big, ld_big, P, small, ld_small, g, bias, act, 0, vec_out); break;
                case 8: hipLaunchKernelGGL((k_b2s_tapk<8, 1>), grid, dim3(256), 0, st, big, ld_big, P, small, ld_small, g, bias, act, 0, vec_out); break;
                default: hipLaunchKernelGGL(k_b2s_tapk<4>, grid, dim3(256), 0, st, big, ld_big, P, small, ld_small, g, bias, act, vec4, vec_out); break;
            }
            return launched();
        }
        default: break;
    }
    return launch_gemm(c, 0);
}

// the col2im half of the taps-folded-into-N small -> big paths
int launch_col2im(const float* D, const float* bias, float* big, int ld_big, const Geom& g, int act, hipStream_t st) {
    const size_t lds = (size_t)(CT_H + 2) * (CT_W + 2) * 16 * g.Cb * sizeof(float);
    if (g.s == 2) {                    // (a D row is 16 * Cb floats: always whole float4s)
        if (lds <= 64 * 1024 && aligned16(D)) {
            const int tiles_h = (g.Hs + CT_H) / CT_H, tiles_w = (g.Ws + CT_W) / CT_W;      // big rows reach one small row past Hs - 1
            hipLaunchKernelGGL(k_col2im_s2_lds, dim3((unsigned)(g.N * tiles_h * tiles_w)), dim3(256), lds, st, D, bias, big, ld_big, g, act,
                               tiles_h, tiles_w);
            return launched();
        }
    }
    const long total = (long)g.N * g.Hb * g.Wb * g.Cb;
    hipLaunchKernelGGL(k_col2im_small2big, dim3((int)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0, st, D, bias, big, ld_big, g, act);
    return launched();
}

int launch_s2b(const Call& c) {
    const Geom& g = c.g;
    const ConvPlan& p = c.p;
    hipStream_t st = c.st;
    const float* small = (const float*)c.v.small;
    float* big = (float*)const_cast<void*>(c.v.big);
    const float *P = c.v.P, *bias = c.v.bias;
    const int ld_big = c.v.ld_big, ld_small = c.v.ld_small, act = c.v.act;
    const long pix = (long)g.N * g.Hs * g.Ws, big_pix = (long)g.N * g.Hb * g.Wb;
    const bool out_bf = c.io & PG_IO_BIG_BF16;
    switch (p.path) {
        case Path::Direct:
            hipLaunchKernelGGL(k_small2big_direct, dim3((int)std::min<long>((big_pix * g.Cb + 255) / 256, 65536)), dim3(256), 0, st, small, ld_small, P, bias,
                               big, ld_big, g, act);
            return launched();
        case Path::Ca1: {
            const pg_epi_mul mul = mul_of(c);
            TimedLaunch timed(st);
            if (p.ca1_s1) {
                // per-sample form: ~1536 workgroups in all, whole pixel rows of the workgroup (256 / (Cb / 4) pixels per trip)
                const int npr = 256 / (g.Cb / 4), hwb = g.Hb * g.Wb;
                const long per = std::max<long>(1, 1536 / g.N);
                static const int minpix = pg_exp_env("PATCHGAN_CA1S1_MINPIX") ? atoi(pg_exp_env("PATCHGAN_CA1S1_MINPIX")) : 0;
                const int ppb1 = std::max(minpix, (int)(((hwb + per - 1) / per + npr - 1) / npr * npr));
                hipLaunchKernelGGL(k_s2b_ca1_s1, dim3((unsigned)((hwb + ppb1 - 1) / ppb1), g.N), dim3(256), (size_t)(g.Hs + 4) * (g.Ws + 4) * sizeof(float), st,
                                   small, ld_small, P, bias, big, ld_big, g, act, out_bf ? 1 : 0, mul, ppb1);
                return launched();
            }
            // pixels per workgroup: ~1500 workgroups, whole trips of 2 pixels per thread row (256 / (Cb / 4) pixel rows per workgroup)
            const int trip = 2 * (256 / (g.Cb / 4));
            static const int ca1_wgs = pg_exp_env("PATCHGAN_CA1_WGS") ? atoi(pg_exp_env("PATCHGAN_CA1_WGS")) : 1536;
            const int ppb = (int)std::max<long>(trip, ((big_pix / ca1_wgs + trip - 1) / trip) * trip);
            hipLaunchKernelGGL(k_s2b_ca1, dim3((unsigned)((big_pix + ppb - 1) / ppb)), dim3(256), 0, st, small, ld_small, P, bias, big, ld_big, g, act,
                               out_bf ? 1 : 0, mul, ppb);
            return launched();
        }
        case Path::Wino1: return launch_wino1(c, 1);
        case Path::Wino2: return launch_wino2(c, 1);
        case Path::TapnfBf:
        case Path::Tapnf: {
            const bool bf = p.path == Path::TapnfBf;
            return launch_tapnf(bf, small, ld_small, P, bias, big, ld_big, g, act, tensor_bytes(pix, ld_small, g.Ca, bf), tensor_bytes(big_pix, ld_big, g.Cb),
                                st);
        }
        case Path::Bf16xTapn: {
            const int Nc = 16 * g.Cb;
            float* D = (float*)((char*)c.v.ws + pg_bf16x_w_bytes(g.Ca, g.Cb));
            int rc = pg_bf16x_pack(P, c.v.ws, g.Ca, g.Cb, 1, st);
            if (rc != PG_OK) return rc;
            {
                TimedLaunch timed(st);
                rc = pg_bf16x_conv(3, small, ld_small, tensor_bytes(pix, ld_small, g.Ca, true), c.v.ws, D, Nc, 0L, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, Nc, g.s,
                                   &p.bx, nullptr, 0, 0, st);
            }
            if (rc != PG_OK) return rc;
            return launch_col2im(D, bias, big, ld_big, g, act, st);
        }
        case Path::Bf16x: return launch_bf16x(c, 1);
        case Path::TapnRowGemm: {
            const int Nc = 16 * g.Cb;
            float* Wp = (float*)c.v.ws;
            float* D = Wp + (((size_t)Nc * g.Ca + 63) & ~(size_t)63);
            const float* W = P;
            if (g.Cb > 1) {
                hipLaunchKernelGGL(k_pack_taps_b, dim3((Nc * g.Ca + 255) / 256), dim3(256), 0, st, P, Wp, g.Ca, g.Cb);
                if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
                W = Wp;
            }
            int rc = launch_row_gemm(c, small, ld_small, W, D, pix, g.Hs, g.Ws, g.Ca, Nc);
            if (rc != PG_OK) return rc;
            return launch_col2im(D, bias, big, ld_big, g, act, st);
        }
        default: break;
    }
    return launch_gemm(c, 1);
}

// the main kernel of the weight gradient (after the bias gradient's column sums); Views::P is dP
int launch_wgrad(const Call& c) {
    const Geom& g = c.g;
    const ConvPlan& p = c.p;
    hipStream_t st = c.st;
    const float *small = (const float*)c.v.small, *big = (const float*)c.v.big;
    float* dP = const_cast<float*>(c.v.P);
    const int ld_big = c.v.ld_big, ld_small = c.v.ld_small;
    const long Kp = (long)g.N * g.Hs * g.Ws, big_pix = (long)g.N * g.Hb * g.Wb, per = 16L * g.Ca * g.Cb;
    float* rest = (float*)((char*)c.v.ws + p.reserved);
    const bool in_bf = c.io != 0;
    auto reduce = [&](const float* slabs, int n) { return launch_reduce(slabs, per, n, dP, g.Cb, 16L * g.Ca, g.Cb, nullptr, 0, st); };
    switch (p.path) {
        case Path::Direct: {
            long smax = (long)((c.ws_bytes - p.reserved) / (sizeof(float) * (size_t)per));
            int slices = (int)std::min<long>(std::min<long>(DIRECT_WGRAD_SLICES, smax), Kp);
            if (slices < 1) slices = 1;
            long pps = (Kp + slices - 1) / slices;
            slices = (int)((Kp + pps - 1) / pps);
            float* dst = slices == 1 ? dP : rest;
            hipLaunchKernelGGL(k_wgrad_direct, dim3((int)((per + 255) / 256), slices), dim3(256), 0, st, small, ld_small, big, ld_big, dst, per, g, pps);
            if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
            return slices == 1 ? PG_OK : reduce(dst, slices);
        }
        case Path::WinoWgrad:
        case Path::Wino2Wgrad: {
            hipEvent_t e0 = t_ev0, e1 = t_ev1;
            t_ev0 = nullptr;
            t_ev1 = nullptr;
            return (p.path == Path::WinoWgrad ? pg_wino_wgrad : pg_wino2_wgrad)(small, ld_small, big, ld_big, dP, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, g.Cb, rest,
                                                                              st, e0, e1, c.v.x->v_pre, c.tune.s3w);
        }
        case Path::Bf16xWgrad: {
            float* dst = p.split == 1 ? dP : rest;
            int rc;
            {
                TimedLaunch timed(st);
                rc = pg_bf16x_wgrad(small, ld_small, tensor_bytes(Kp, ld_small, g.Ca, true), big, ld_big, tensor_bytes(big_pix, ld_big, g.Cb > 8 ? g.Cb : 8, true),
                                    dst, p.split == 1 ? 0L : p.bx.out_elems, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, g.Cb, g.s, &p.bx, st);
            }
            if (rc != PG_OK || p.split == 1) return rc;
            return reduce(dst, p.split);
        }
        case Path::WgradTapnp: {
            const int ntiles = (int)((Kp + 127) / 128), G = p.split;
            const int small_b = (int)tensor_bytes(Kp, ld_small, g.Ca), big_b = (int)tensor_bytes(big_pix, ld_big, g.Cb);
            const bool wide3 = (g.Cb == 3) && (ld_big % 4 == 0) && (ld_big >= 4) && aligned16(big);
            {
                TimedLaunch timed(st);
                const dim3 grid(G, g.Cb <= 2 ? (g.Ca + 127) / 128 : (g.Ca + 63) / 64, 1);
                auto go = [&](auto kernel) {
                    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, small, ld_small, big, ld_big, rest, per, g, small_b, big_b, ntiles);
                };
                if (g.Cb == 1) go(k_wgrad_tapnp<1, false, 4>);
                else if (g.Cb == 2) go(k_wgrad_tapnp<2, false, 4>);
                else if (g.Cb == 4) go(k_wgrad_tapnp<4, true, 2>);
                else if (wide3) go(k_wgrad_tapnp<3, true, 2>);
                else go(k_wgrad_tapnp<3, false, 2>);
            }
            if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
            return reduce(rest, G);
        }
        default: break;
    }
    // Path::Gemm (one GEMM per tap) / Path::WgradTapn (taps folded into N): into dP, or split-K slabs + reduce
    const Plan& q = p.gemm;
    float* dst = q.split == 1 ? dP : rest;
    {
        TimedLaunch timed(st);
        if (p.path == Path::Gemm) {
            dim3 grid(q.tiles_m * q.tiles_n, 16, q.split);
            const int small_bytes = (int)tensor_bytes(Kp, ld_small, g.Ca, in_bf), big_bytes = (int)tensor_bytes(big_pix, ld_big, g.Cb, in_bf);
            for_tile(q.t.id, [&](auto tt) {
                using T = decltype(tt);
                if (!p.fast)
                    hipLaunchKernelGGL((k_wgrad<PG_TILE(T)>), grid, dim3(256), 0, st, small, ld_small, big, ld_big, dst, q.out_elems, g, q.cps, q.tiles_n, p.veck,
                                       p.vecn);
                else
                    for_bool(p.pow2, [&](auto p2) {
                        if (c.algo == PG_ALGO_BF16)
                            for_bool(in_bf, [&](auto hin) {
                                hipLaunchKernelGGL((k_wgrad_bf16<PG_TILE(T), decltype(p2)::value, decltype(hin)::value>), grid, dim3(256), 0, st, small, ld_small,
                                                   big, ld_big, dst, q.out_elems, g, q.cps, q.tiles_n, small_bytes, big_bytes);
                            });
                        else
                            hipLaunchKernelGGL((k_wgrad_fast<PG_TILE(T), decltype(p2)::value>), grid, dim3(256), 0, st, small, ld_small, big, ld_big, dst,
                                               q.out_elems, g, q.cps, q.tiles_n, small_bytes, big_bytes);
                    });
            });
        } else {
            dim3 grid(q.tiles_m * q.tiles_n, 1, q.split);
            const int vecy = (g.Cb == 4) && (ld_big % 4 == 0) && aligned16(big);
            for_tile(q.t.id, [&](auto tt) {
                using T = decltype(tt);
                if (p.mode == 1)
                    hipLaunchKernelGGL((k_wgrad_tapn<PG_TILE(T), 1>), grid, dim3(256), 0, st, small, ld_small, big, ld_big, dst, q.out_elems, g, q.cps, q.tiles_n,
                                       p.veck, vecy);
                else
                    hipLaunchKernelGGL((k_wgrad_tapn<PG_TILE(T), 2>), grid, dim3(256), 0, st, big, ld_big, small, ld_small, dst, q.out_elems, g, q.cps, q.tiles_n,
                                       p.vecn, 0);
            });
        }
    }
    if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
    return q.split == 1 ? PG_OK : reduce(dst, q.split);
}

// The code of a refused call.  bf16 tensors run on the bf16 kernels only, and the LDS-DMA ones read packed bf16 weights from the
// workspace: where the register-staged kernels do not cover the call (8-channel pixels, ...) a NULL or smaller workspace leaves no
// kernel.  That is PG_EWORKSPACE -- the same call with pg_conv_workspace_bytes() is accepted -- and not PG_EINVAL.
int refusal(int rc, int op, const Views& v, const pg_conv_geom* gg, int algo_full, size_t ws_bytes) {
    if (rc != PG_EINVAL || !(algo_full & PG_IO_MASK)) return rc;
    const size_t full = pg_conv_workspace_bytes(gg, op);
    if (v.ws && ws_bytes >= full) return rc;
    Views w = v;
    if (!w.ws) w.ws = reinterpret_cast<void*>(uintptr_t(256));      // (planned, never launched: only its alignment is looked at)
    return plan_conv(gg, op, algo_full, tune_of(algo_full), full, &w).rc == PG_OK ? PG_EWORKSPACE : rc;
}

// plan the call and launch its path
int run_conv(int op, const Views& v, const pg_conv_geom* gg, int algo_full, size_t ws_bytes, void* stream) {
    if (!v.ws) ws_bytes = 0;
    Call c{ConvPlan{}, v, to_geom(gg), algo_full & PG_ALGO_MASK, algo_full & PG_IO_MASK, tune_of(algo_full), ws_bytes, (hipStream_t)stream};
    c.p = plan_conv(gg, op, algo_full, c.tune, ws_bytes, &c.v);
    if (c.p.rc != PG_OK) return refusal(c.p.rc, op, v, gg, algo_full, ws_bytes);
    return op == 0 ? launch_b2s(c) : op == 1 ? launch_s2b(c) : launch_wgrad(c);
}

}  // namespace

// A hand-over is taken only where its size query, asked with the workspace of THIS call, reports a size: the caller could not have
// sized the buffer otherwise (pg_conv_v_bytes is 0 where the layer's weight gradient would not read the kept V, although the forward
// path has one; the bf16 kernels promise their statistics epilogue only with the path's full workspace).  Else PG_EINVAL, nothing launched.
static bool hand_overs_sized(const pg_conv_geom* gg, int op, int algo, const void* ws, size_t ws_bytes, const pg_conv_extras& x) {
    const size_t wb = ws ? ws_bytes : 0;
    if (x.part && (op > 1 || pg_conv_stats_chunks(gg, op, algo, wb) == 0)) return false;
    if (x.u_cache && (op > 1 || pg_conv_u_bytes(gg, op, algo, wb) == 0)) return false;
    if ((x.v_keep || x.v_pre) && pg_conv_v_bytes(gg, algo, wb) == 0) return false;
    return true;
}

extern "C" {

int pg_conv4x4_big2small_x(const float* big, int ld_big, const float* P, const float* bias, float* small, int ld_small,
                           const pg_conv_geom* gg, int act, int algo, void* ws, size_t ws_bytes, void* stream, const pg_conv_extras* xp) {
    const pg_conv_extras& x = xp ? *xp : NO_EXTRAS;
    if ((x.u_cache && !aligned16(x.u_cache)) || (x.v_keep && !aligned16(x.v_keep)) || x.v_pre) return PG_EINVAL;
    if (!geom_ok(gg) || !big || !P || !small || ld_big < gg->Cb || ld_small < gg->Ca) return PG_EINVAL;
    if (act < PG_ACT_NONE || act > PG_ACT_SIGMOID) return PG_EINVAL;
    // bf16 activation storage: PG_IO_BIG_BF16 = input, PG_IO_SMALL_BF16 = output
    if ((algo & PG_IO_MASK) && (algo & PG_ALGO_MASK) != PG_ALGO_BF16) return PG_EINVAL;
    if (!hand_overs_sized(gg, 0, algo, ws, ws_bytes, x)) return PG_EINVAL;
    if (x.v_stride || x.v_tile0) {
        // the kept V as rows [v_tile0, v_tile0 + tiles) of a larger batch's planes: the range stays inside a plane, the strided buffer
        // inside the kernels' 32-bit offsets
        ConvPlan f;
        if (!x.v_keep || x.v_stride < 0 || x.v_tile0 < 0 || !query_plan(gg, 0, algo, ws ? ws_bytes : 0, OFFER_V, &f)) return PG_EINVAL;
        if (f.path != Path::Wino1 && f.path != Path::Wino2) return PG_EINVAL;
        const bool w1 = f.path == Path::Wino1;
        const long X = w1 ? 36 : 16, K = w1 ? gg->Cb : 4L * gg->Cb;
        const long T = w1 ? (long)gg->N * ((gg->Hs + 2) / 3) * ((gg->Ws + 2) / 3) : pg_wino2_tiles_b2s(gg->N, gg->Hs, gg->Ws);
        const long zs = x.v_stride ? (long)x.v_stride : T * K;
        if ((zs & 3) || (x.v_tile0 + T) * K > zs || (double)X * zs * 4 >= 1.5e9) return PG_EINVAL;
    }
    return run_conv(0, Views{small, big, ld_small, ld_big, P, bias, act, ws, &x}, gg, algo, ws_bytes, stream);
}

int pg_conv4x4_big2small(const float* big, int ld_big, const float* P, const float* bias, float* small,
                         int ld_small, const pg_conv_geom* gg, int act, int algo, void* ws, size_t ws_bytes,
                         void* stream) {
    return pg_conv4x4_big2small_x(big, ld_big, P, bias, small, ld_small, gg, act, algo, ws, ws_bytes, stream, nullptr);
}

int pg_conv4x4_small2big_x(const float* small, int ld_small, const float* P, const float* bias, float* big, int ld_big,
                           const pg_conv_geom* gg, int act, int algo, void* ws, size_t ws_bytes, void* stream, const pg_conv_extras* xp) {
    const pg_conv_extras& x = xp ? *xp : NO_EXTRAS;
    if ((x.u_cache && !aligned16(x.u_cache)) || x.v_keep || x.v_pre || x.v_stride || x.v_tile0) return PG_EINVAL;
    if (x.mul_t && (x.mul_ld < gg->Cb || x.mul_act < PG_ACT_NONE || x.mul_act > PG_ACT_SIGMOID || x.part)) return PG_EINVAL;
    if (!geom_ok(gg) || !big || !P || !small || ld_big < gg->Cb || ld_small < gg->Ca) return PG_EINVAL;
    if (act < PG_ACT_NONE || act > PG_ACT_SIGMOID) return PG_EINVAL;
    // PG_IO_SMALL_BF16 = input, PG_IO_BIG_BF16 = output
    if ((algo & PG_IO_MASK) && (algo & PG_ALGO_MASK) != PG_ALGO_BF16) return PG_EINVAL;
    if (!hand_overs_sized(gg, 1, algo, ws, ws_bytes, x)) return PG_EINVAL;
    return run_conv(1, Views{small, big, ld_small, ld_big, P, bias, act, ws, &x}, gg, algo, ws_bytes, stream);
}

int pg_conv4x4_small2big(const float* small, int ld_small, const float* P, const float* bias, float* big,
                         int ld_big, const pg_conv_geom* gg, int act, int algo, void* ws, size_t ws_bytes,
                         void* stream) {
    return pg_conv4x4_small2big_x(small, ld_small, P, bias, big, ld_big, gg, act, algo, ws, ws_bytes, stream, nullptr);
}

static int wgrad_impl(const float* small, int ld_small, const float* big, int ld_big, float* dP, float* dbias,
                      const pg_conv_geom* gg, int algo, void* ws, size_t ws_bytes, void* stream, const float* v_pre) {
    if (!geom_ok(gg) || !big || !dP || !small || ld_big < gg->Cb || ld_small < gg->Ca) return PG_EINVAL;
    if (v_pre && !aligned16(v_pre)) return PG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Geom g = to_geom(gg);
    const int io = algo & PG_IO_MASK;                 // both activation operands bf16, or neither
    if (io && ((algo & PG_ALGO_MASK) != PG_ALGO_BF16 || io != PG_IO_MASK)) return PG_EINVAL;
    if (io && dbias && !((g.Ca % 4 == 0) && (ld_small % 4 == 0) && aligned_io(small, true))) return PG_EINVAL;
    if (!ws) ws_bytes = 0;
    pg_conv_extras x = NO_EXTRAS;
    x.v_pre = v_pre;
    if (!hand_overs_sized(gg, 2, algo, ws, ws_bytes, x)) return PG_EINVAL;
    if (dbias) {
        if (ws_bytes < colsum_bytes(g.Ca)) return PG_EWORKSPACE;
        // nothing is launched when an error is returned: the column sums start only for a call that the planner accepts
        const Views vw{small, big, ld_small, ld_big, dP, dbias, PG_ACT_NONE, ws, &x};
        const int prc = plan_conv(gg, 2, algo, tune_of(algo), ws_bytes, &vw).rc;
        if (prc != PG_OK) return refusal(prc, 2, vw, gg, algo, ws_bytes);
        const long Kp = (long)g.N * g.Hs * g.Ws;
        float* part = (float*)ws;
        int chunks = (int)std::min<long>(COLSUM_CHUNKS, Kp);
        long rpc = (Kp + chunks - 1) / chunks;
        chunks = (int)((Kp + rpc - 1) / rpc);
        if (io)
            hipLaunchKernelGGL(k_colsum_partial4<true>, dim3(chunks, (g.Ca + 63) / 64), dim3(256), 0, st, small, ld_small, Kp, g.Ca,
                               rpc, part);
        else if ((g.Ca % 4 == 0) && (ld_small % 4 == 0) && aligned16(small) && aligned16(part))
            hipLaunchKernelGGL(k_colsum_partial4<false>, dim3(chunks, (g.Ca + 63) / 64), dim3(256), 0, st, small, ld_small, Kp, g.Ca,
                               rpc, part);
        else
            hipLaunchKernelGGL(k_colsum_partial, dim3(chunks, (g.Ca + 63) / 64), dim3(256), 0, st, small, ld_small, Kp, g.Ca,
                               rpc, part);
        if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
        int rc = launch_reduce(part, g.Ca, chunks, dbias, g.Ca, 1, g.Ca, nullptr, 0, st);
        if (rc != PG_OK) return rc;
    }
    return run_conv(2, Views{small, big, ld_small, ld_big, dP, dbias, PG_ACT_NONE, ws, &x}, gg, algo, ws_bytes, stream);
}

int pg_conv4x4_wgrad(const float* small, int ld_small, const float* big, int ld_big, float* dP, float* dbias,
                     const pg_conv_geom* gg, int algo, void* ws, size_t ws_bytes, void* stream) {
    return wgrad_impl(small, ld_small, big, ld_big, dP, dbias, gg, algo, ws, ws_bytes, stream, nullptr);
}

int pg_conv4x4_wgrad_x(const float* small, int ld_small, const float* big, int ld_big, float* dP, float* dbias,
                       const pg_conv_geom* gg, int algo, void* ws, size_t ws_bytes, void* stream, const pg_conv_extras* x) {
    if (x && (x->part || x->v_keep || x->u_cache || x->v_stride || x->v_tile0)) return PG_EINVAL;
    return wgrad_impl(small, ld_small, big, ld_big, dP, dbias, gg, algo, ws, ws_bytes, stream, x ? x->v_pre : nullptr);
}

int pg_conv4x4_bwd_big(const float* small, int ld_small, const float* big, int ld_big, const float* P, float* dP,
                       float* dsmall, int ld_dsmall, const pg_conv_geom* gg, int algo, void* ws, size_t ws_bytes, void* stream) {
    return pg_conv4x4_bwd_big_x(small, ld_small, big, ld_big, P, dP, dsmall, ld_dsmall, gg, algo, ws, ws_bytes, stream, nullptr);
}

int pg_conv4x4_bwd_big_x(const float* small, int ld_small, const float* big, int ld_big, const float* P, float* dP,
                         float* dsmall, int ld_dsmall, const pg_conv_geom* gg, int algo, void* ws, size_t ws_bytes, void* stream,
                         const pg_conv_extras* x) {
    if (!geom_ok(gg) || !small || !big || !P || !dP || !dsmall) return PG_EINVAL;
    if (x && (x->part || x->v_keep || x->v_pre || x->mul_t || x->v_stride || x->v_tile0)) return PG_EINVAL;      // only the data gradient's u_cache / u_valid
    float* const Uext = x ? x->u_cache : nullptr;
    const int u_valid = x ? x->u_valid : 0;
    if (Uext && !aligned16(Uext)) return PG_EINVAL;
    if (ld_small < gg->Ca || ld_big < gg->Cb || ld_dsmall < gg->Ca) return PG_EINVAL;
    if (Uext && pg_conv_u_bytes(gg, 0, algo, ws ? ws_bytes : 0) == 0) return PG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Geom g = to_geom(gg);
    const Tune tune = tune_of(algo);
    if (!ws) ws_bytes = 0;
    const bool views_ok = (ld_small % 4 == 0) && (ld_big % 4 == 0) && (ld_dsmall % 4 == 0) && aligned16(small) && aligned16(big) &&
                          aligned16(P) && aligned16(dP) && aligned16(dsmall) && aligned16(ws);
    hipEvent_t e0 = t_ev0, e1 = t_ev1, e2 = t_ev2, e3 = t_ev3;
    if (!plan_share_v(g, algo, tune, ws_bytes, views_ok, nullptr)) {       // the two halves as separate calls (each consumes one armed event pair)
        t_ev2 = t_ev3 = nullptr;
        int rc = pg_conv4x4_wgrad(small, ld_small, big, ld_big, dP, nullptr, gg, algo, ws, ws_bytes, stream);
        if (rc != PG_OK) return rc;
        t_ev0 = e2;
        t_ev1 = e3;
        if (Uext) {
            pg_conv_extras xu{};
            xu.u_cache = Uext;
            xu.u_valid = u_valid;
            return pg_conv4x4_big2small_x(big, ld_big, P, nullptr, dsmall, ld_dsmall, gg, PG_ACT_NONE, algo, ws, ws_bytes, stream, &xu);
        }
        return pg_conv4x4_big2small(big, ld_big, P, nullptr, dsmall, ld_dsmall, gg, PG_ACT_NONE, algo, ws, ws_bytes, stream);
    }
    t_ev0 = t_ev1 = t_ev2 = t_ev3 = nullptr;
    // V(big) once; the weight-gradient GEMM and the data-gradient GEMM both read it (ws: V | DY S, then V | U M)
    float* V = (float*)ws;
    void* rest = (char*)ws + pg_wino2_v_bytes(g.N, g.Hs, g.Ws, g.Cb);
    int rc = pg_wino2_v(big, ld_big, V, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Cb, st);
    if (rc != PG_OK) return rc;
    rc = pg_wino2_wgrad(small, ld_small, big, ld_big, dP, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, g.Cb, rest, st, e0, e1, V, tune.s3w);
    if (rc != PG_OK) return rc;
    return pg_wino2_b2s(big, ld_big, P, nullptr, dsmall, ld_dsmall, g.N, g.Hb, g.Wb, g.Hs, g.Ws, g.Ca, g.Cb, PG_ACT_NONE, rest, st, e2,
                        e3, V, nullptr, nullptr, Uext, u_valid, tune.s3);
}

}  // extern "C"
