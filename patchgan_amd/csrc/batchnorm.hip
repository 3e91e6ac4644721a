// batchnorm.hip -- BatchNorm2d (affine, tracked running statistics; unet.py:20,55 and disc.py:32,42 with norm_layer=nn.BatchNorm2d)
// + activation + dropout, forward / backward, and the running-statistics update.  fp32 NHWC tensors (channel slices: any `ld`).
//
// Statistics are per (segment, channel) over the N_s * HW pixels of a SEGMENT: a run of N / nseg consecutive samples.  nseg = 2 is the
// discriminator step's one pass over din[2N], which the reference runs as two calls (trainer.py:97,99): each half is normalised with
// its own batch statistics, forward and backward.
//
// Same structure as InstanceNorm's kernels (norm_act.hip) and the same per-element helpers (norm_elem.h): fp64 partial sums per (sample, pixel chunk, channel) -- from the producing
// conv's epilogue where it emits them (pg_conv_extras.part), else from a statistics pass -- merged in a fixed order (no floating-point
// atomics: bit-reproducible), then a vectorised apply pass.  Where InstanceNorm's chunk plan would not split a plane (planes under 512
// pixels) a call is one kernel (a workgroup owns a group of channels of every segment and walks its pixels three times).
//
// coef[(s*C + c)*4 + {0,1,2,3}] = (mean, rstd, scale = weight*rstd, shift = bias - mean*scale): the forward is z = x*scale + shift,
// the backward reads (mean, rstd, scale) again.  bstat[(s*C + c)*2 + {0,1}] = (batch mean, unbiased batch variance) in fp64: what
// pg_batchnorm_update_running folds into the running statistics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "patchgan_hip.h"
#include "pg_common.h"
#include "norm_elem.h"

namespace {

// the incoming gradient of one element after dropout and the activation: dz = (g1 + g2) * keep/(1-p) * act'(x*scale + shift)
__device__ __forceinline__ float bn_dz(float g, float x, float scale, float shift, int act, float drop_p, float keep_scale,
                                       uint64_t seed, uint64_t e) {
    if (drop_p > 0.f) g = pg_dropout_keep(seed, e, drop_p) ? g * keep_scale : 0.f;
    return g * pg_norm_act_grad(__fadd_rn(__fmul_rn(x, scale), shift), act);
}

// ---- one kernel per call (planes under 512 pixels): grid (channel groups), the segments one after the other
template <int VEC>
__global__ __launch_bounds__(256) void k_bn_fwd_small(const float* __restrict__ y, int ld_y, float* __restrict__ out, int ld_out,
                                                      const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ coef,
                                                      double* __restrict__ bstat, int Ns, int HW, int C, int nseg, int G, int act,
                                                      float eps, float drop_p, uint64_t seed) {
    __shared__ double red[VEC][256];
    const int tid = threadIdx.x, cu = tid % G, pl = tid / G, PL = 256 / G;
    const int c0 = (blockIdx.x * G + cu) * VEC;
    const bool on = c0 < C;
    const int M = Ns * HW;
    const float keep_scale = 1.f / (1.f - drop_p);
    for (int s = 0; s < nseg; ++s) {
        const long p0 = (long)s * M;
        double acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.0;
        if (on)
            for (int p = pl; p < M; p += PL) {
                const Vec<VEC> v = vload<VEC>(y + (p0 + p) * ld_y + c0);
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] += (double)v.v[k];
            }
#pragma unroll
        for (int k = 0; k < VEC; ++k) red[k][tid] = acc[k];
        lane_tree<VEC>(red, tid, G);
        double mean[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) mean[k] = red[k][cu] / (double)M;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.0;
        if (on)
            for (int p = pl; p < M; p += PL) {
                const Vec<VEC> v = vload<VEC>(y + (p0 + p) * ld_y + c0);
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const double d = (double)v.v[k] - mean[k];
                    acc[k] += d * d;
                }
            }
#pragma unroll
        for (int k = 0; k < VEC; ++k) red[k][tid] = acc[k];
        lane_tree<VEC>(red, tid, G);
        float sc[VEC], sh[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const double var = red[k][cu] / (double)M;
            const double rstd = 1.0 / sqrt(var + (double)eps);
            const float wk = on ? w[c0 + k] : 0.f, bk = on ? b[c0 + k] : 0.f;
            sc[k] = (float)((double)wk * rstd);
            sh[k] = (float)((double)bk - mean[k] * (double)sc[k]);
            if (on && pl == 0) {
                float* q = coef + ((long)s * C + c0 + k) * 4;
                q[0] = (float)mean[k];
                q[1] = (float)rstd;
                q[2] = sc[k];
                q[3] = sh[k];
                if (bstat) {
                    bstat[((long)s * C + c0 + k) * 2 + 0] = mean[k];
                    bstat[((long)s * C + c0 + k) * 2 + 1] = var * (double)M / (double)(M - 1);
                }
            }
        }
        __syncthreads();
        if (!on) continue;
        for (int p = pl; p < M; p += PL) {
            const Vec<VEC> v = vload<VEC>(y + (p0 + p) * ld_y + c0);
            Vec<VEC> o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float a = pg_act(__fadd_rn(__fmul_rn(v.v[k], sc[k]), sh[k]), act);
                if (drop_p > 0.f) a = pg_dropout_keep(seed, (uint64_t)(p0 + p) * C + c0 + k, drop_p) ? a * keep_scale : 0.f;
                o.v[k] = a;
            }
            vstore<VEC>(out + (p0 + p) * ld_out + c0, o);
        }
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void k_bn_bwd_small(const float* __restrict__ g1, int ld_g1, const float* __restrict__ g2, int ld_g2,
                                                      const float* __restrict__ y, int ld_y, const float* __restrict__ coef,
                                                      float* __restrict__ dy, int ld_dy, float* __restrict__ dw, float* __restrict__ db,
                                                      int Ns, int HW, int C, int nseg, int G, int train, int act, float drop_p,
                                                      uint64_t seed) {
    __shared__ double red[2 * VEC][256];
    const int tid = threadIdx.x, cu = tid % G, pl = tid / G, PL = 256 / G;
    const int c0 = (blockIdx.x * G + cu) * VEC;
    const bool on = c0 < C;
    const int M = Ns * HW;
    const float keep_scale = 1.f / (1.f - drop_p);
    double tw[VEC], tb[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) tw[k] = tb[k] = 0.0;
    for (int s = 0; s < nseg; ++s) {
        const long p0 = (long)s * M;
        float mf[VEC], rs[VEC], sc[VEC], sh[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float* q = coef + ((long)s * C + (on ? c0 + k : 0)) * 4;
            mf[k] = q[0]; rs[k] = q[1]; sc[k] = q[2]; sh[k] = q[3];
        }
        auto dz_of = [&](long gp, Vec<VEC>& xh, Vec<VEC>& dz) {
            const Vec<VEC> v = vload<VEC>(y + gp * ld_y + c0);
            Vec<VEC> g = vload<VEC>(g1 + gp * ld_g1 + c0);
            if (g2) {
                const Vec<VEC> h = vload<VEC>(g2 + gp * ld_g2 + c0);
#pragma unroll
                for (int k = 0; k < VEC; ++k) g.v[k] += h.v[k];
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                dz.v[k] = bn_dz(g.v[k], v.v[k], sc[k], sh[k], act, drop_p, keep_scale, seed, (uint64_t)gp * C + c0 + k);
                xh.v[k] = (v.v[k] - mf[k]) * rs[k];
            }
        };
        double s1[VEC], s2[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) s1[k] = s2[k] = 0.0;
        if (on)
            for (int p = pl; p < M; p += PL) {
                Vec<VEC> xh, dz;
                dz_of(p0 + p, xh, dz);
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    s1[k] += (double)dz.v[k];
                    s2[k] += (double)dz.v[k] * (double)xh.v[k];
                }
            }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            red[k][tid] = s1[k];
            red[VEC + k][tid] = s2[k];
        }
        lane_tree<2 * VEC>(red, tid, G);
        float cdz[VEC], cx[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            tb[k] += red[k][cu];
            tw[k] += red[VEC + k][cu];
            cdz[k] = train ? (float)(red[k][cu] / (double)M) : 0.f;
            cx[k] = train ? (float)(red[VEC + k][cu] / (double)M) : 0.f;
        }
        __syncthreads();
        if (!on) continue;
        for (int p = pl; p < M; p += PL) {
            Vec<VEC> xh, dz, o;
            dz_of(p0 + p, xh, dz);
#pragma unroll
            for (int k = 0; k < VEC; ++k) o.v[k] = sc[k] * (dz.v[k] - cdz[k] - xh.v[k] * cx[k]);
            vstore<VEC>(dy + (p0 + p) * ld_dy + c0, o);
        }
    }
    if (on && pl == 0 && dw) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            dw[c0 + k] = (float)tw[k];
            db[c0 + k] = (float)tb[k];
        }
    }
}

// ---- chunked path (planes of >= 512 pixels): partial sums per (sample, chunk, channel), fixed-order merge, apply
// FWD: (sum x, sum x^2).  BWD: (sum dz, sum dz * xhat) with the forward's coefficients of the sample's segment.
template <int VEC, bool BWD, bool HG2>
__global__ __launch_bounds__(256) void k_bn_partial(const float* __restrict__ y, int ld_y, const float* __restrict__ g1, int ld_g1,
                                                    const float* __restrict__ g2, int ld_g2, const float* __restrict__ coef,
                                                    double* __restrict__ part, int Ns, int HW, int C, int G, int ppc, int act,
                                                    float drop_p, uint64_t seed) {
    __shared__ double red[2 * VEC][256];
    const int tid = threadIdx.x, cu = tid % G, pl = tid / G, PL = 256 / G;
    const int c0 = (blockIdx.x * G + cu) * VEC;
    const int chunk = blockIdx.y, nchunk = gridDim.y, n = blockIdx.z;
    const bool on = c0 < C;
    const long nb = (long)n * HW;
    const int p_begin = chunk * ppc, p_end = min(HW, p_begin + ppc);
    float mf[VEC], rs[VEC], sc[VEC], sh[VEC];
    if (BWD) {
        const int s = n / Ns;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float* q = coef + ((long)s * C + (on ? c0 + k : 0)) * 4;
            mf[k] = q[0]; rs[k] = q[1]; sc[k] = q[2]; sh[k] = q[3];
        }
    }
    const float keep_scale = 1.f / (1.f - drop_p);
    double s1[VEC], s2[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) s1[k] = s2[k] = 0.0;
    auto accumulate = [&](long gp, const Vec<VEC>& v, Vec<VEC> g, const Vec<VEC>& h) {
        if (!BWD) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const double d = (double)v.v[k];
                s1[k] += d;
                s2[k] += d * d;
            }
        } else {
            if (HG2) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) g.v[k] += h.v[k];
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float dz = bn_dz(g.v[k], v.v[k], sc[k], sh[k], act, drop_p, keep_scale, seed, (uint64_t)gp * C + c0 + k);
                s1[k] += (double)dz;
                s2[k] += (double)dz * (double)((v.v[k] - mf[k]) * rs[k]);
            }
        }
    };
    if (on) {
        constexpr int UNR = 4;
        int pix = p_begin + pl;
        for (; pix + (UNR - 1) * PL < p_end; pix += UNR * PL) {
            Vec<VEC> v[UNR], g[UNR], h[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const long gp = nb + pix + u * PL;
                v[u] = vload<VEC>(y + gp * ld_y + c0);
                if (BWD) {
                    g[u] = vload<VEC>(g1 + gp * ld_g1 + c0);
                    if (HG2) h[u] = vload<VEC>(g2 + gp * ld_g2 + c0);
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) accumulate(nb + pix + u * PL, v[u], g[u], h[u]);
        }
        for (; pix < p_end; pix += PL) {
            const long gp = nb + pix;
            Vec<VEC> v = vload<VEC>(y + gp * ld_y + c0), g, h;
            if (BWD) {
                g = vload<VEC>(g1 + gp * ld_g1 + c0);
                if (HG2) h = vload<VEC>(g2 + gp * ld_g2 + c0);
            }
            accumulate(gp, v, g, h);
        }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        red[k][tid] = s1[k];
        red[VEC + k][tid] = s2[k];
    }
    lane_tree<2 * VEC>(red, tid, G);
    if (on && pl == 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            double* o = part + (((long)n * nchunk + chunk) * C + c0 + k) * 2;
            o[0] = red[k][cu];
            o[1] = red[VEC + k][cu];
        }
    }
}

// Merge of the partials of every (segment, channel): the rows (sample, chunk) of a segment are contiguous; 16 lanes per channel each
// add every 16th row in row order, then a fixed LDS tree.  Workgroup = 16 channels, all segments (the weight gradients are their sum).
// FWD: coef / bstat.  BWD: bcoef[(s*C + c)*2] = (sum dz / M, sum dz*xhat / M) (zero in eval mode), dw / db (may be NULL).
constexpr int MERGE_CW = 16;
template <bool BWD>
__global__ __launch_bounds__(256) void k_bn_merge(const double* __restrict__ part, int nchunk, int Ns, int nseg, int HW, int C,
                                                  float eps, const float* __restrict__ w, const float* __restrict__ b,
                                                  float* __restrict__ coef, double* __restrict__ bstat, float* __restrict__ bcoef,
                                                  float* __restrict__ dw, float* __restrict__ db, int train) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x, cc = tid % MERGE_CW, r = tid / MERGE_CW, R = 256 / MERGE_CW;
    const int c = blockIdx.x * MERGE_CW + cc;
    const bool on = c < C;
    const int rows = Ns * nchunk;
    const double M = (double)Ns * HW;
    double tw = 0.0, tb = 0.0;
    for (int s = 0; s < nseg; ++s) {
        double s1 = 0.0, s2 = 0.0;
        if (on) {
            const double2* p2 = reinterpret_cast<const double2*>(part) + (long)s * rows * C + c;
            for (int row = r; row < rows; row += R) {
                const double2 v = p2[(long)row * C];
                s1 += v.x;
                s2 += v.y;
            }
        }
        red[0][tid] = s1;
        red[1][tid] = s2;
        lane_tree<2>(red, tid, MERGE_CW);
        if (on && r == 0) {
            const double t1 = red[0][cc], t2 = red[1][cc];
            if (!BWD) {
                const double mean = t1 / M;
                double var = t2 / M - mean * mean;
                var = var < 0.0 ? 0.0 : var;
                const double rstd = 1.0 / sqrt(var + (double)eps);
                const float sc = (float)((double)w[c] * rstd);
                float* q = coef + ((long)s * C + c) * 4;
                q[0] = (float)mean;
                q[1] = (float)rstd;
                q[2] = sc;
                q[3] = (float)((double)b[c] - mean * (double)sc);
                if (bstat) {
                    bstat[((long)s * C + c) * 2 + 0] = mean;
                    bstat[((long)s * C + c) * 2 + 1] = var * M / (M - 1.0);
                }
            } else {
                bcoef[((long)s * C + c) * 2 + 0] = train ? (float)(t1 / M) : 0.f;
                bcoef[((long)s * C + c) * 2 + 1] = train ? (float)(t2 / M) : 0.f;
                tb += t1;
                tw += t2;
            }
        }
        __syncthreads();
    }
    if (BWD && on && r == 0 && dw) {
        dw[c] = (float)tw;
        db[c] = (float)tb;
    }
}

// ---- split form (nn.SyncBatchNorm under data parallelism): a collective sits between the reduce and the rest, so the LOCAL fp64
// moments of every (segment, channel) leave in a caller-owned buffer mom[(s*C + c)*2 + {0,1}], and the coefficients / the backward
// apply are formed from the all-reduced moments and the GLOBAL count.  FWD: (sum x, sum x^2).  BWD: (sum dz, sum dz * xhat).
// Planes the chunk plan does not split: one launch, the first pass of the one-workgroup kernels above (any count >= 1).
template <int VEC, bool BWD>
__global__ __launch_bounds__(256) void k_bn_mom_small(const float* __restrict__ y, int ld_y, const float* __restrict__ g1, int ld_g1,
                                                      const float* __restrict__ g2, int ld_g2, const float* __restrict__ coef,
                                                      double* __restrict__ mom, float* __restrict__ dw, float* __restrict__ db, int Ns,
                                                      int HW, int C, int nseg, int G, int act, float drop_p, uint64_t seed) {
    __shared__ double red[2 * VEC][256];
    const int tid = threadIdx.x, cu = tid % G, pl = tid / G, PL = 256 / G;
    const int c0 = (blockIdx.x * G + cu) * VEC;
    const bool on = c0 < C;
    const int M = Ns * HW;
    const float keep_scale = 1.f / (1.f - drop_p);
    double tw[VEC], tb[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) tw[k] = tb[k] = 0.0;
    for (int s = 0; s < nseg; ++s) {
        const long p0 = (long)s * M;
        float mf[VEC], rs[VEC], sc[VEC], sh[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            mf[k] = rs[k] = sc[k] = sh[k] = 0.f;
            if (BWD) {
                const float* q = coef + ((long)s * C + (on ? c0 + k : 0)) * 4;
                mf[k] = q[0]; rs[k] = q[1]; sc[k] = q[2]; sh[k] = q[3];
            }
        }
        double s1[VEC], s2[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) s1[k] = s2[k] = 0.0;
        if (on)
            for (int p = pl; p < M; p += PL) {
                const long gp = p0 + p;
                const Vec<VEC> v = vload<VEC>(y + gp * ld_y + c0);
                if (!BWD) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const double d = (double)v.v[k];
                        s1[k] += d;
                        s2[k] += d * d;
                    }
                } else {
                    Vec<VEC> g = vload<VEC>(g1 + gp * ld_g1 + c0);
                    if (g2) {
                        const Vec<VEC> h = vload<VEC>(g2 + gp * ld_g2 + c0);
#pragma unroll
                        for (int k = 0; k < VEC; ++k) g.v[k] += h.v[k];
                    }
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const float dz = bn_dz(g.v[k], v.v[k], sc[k], sh[k], act, drop_p, keep_scale, seed, (uint64_t)gp * C + c0 + k);
                        s1[k] += (double)dz;
                        s2[k] += (double)dz * (double)((v.v[k] - mf[k]) * rs[k]);
                    }
                }
            }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            red[k][tid] = s1[k];
            red[VEC + k][tid] = s2[k];
        }
        lane_tree<2 * VEC>(red, tid, G);
        if (on && pl == 0) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                double* o = mom + ((long)s * C + c0 + k) * 2;
                o[0] = red[k][cu];
                o[1] = red[VEC + k][cu];
                tb[k] += red[k][cu];
                tw[k] += red[VEC + k][cu];
            }
        }
        __syncthreads();
    }
    if (BWD && on && pl == 0 && dw) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            dw[c0 + k] = (float)tw[k];
            db[c0 + k] = (float)tb[k];
        }
    }
}

// k_bn_merge's fixed-order sum of the partials of every (segment, channel), kept as moments.  BWD: dw / db (may be NULL) = the LOCAL
// sums over the segments (a data-parallel caller SUM-reduces the weight gradients itself).
template <bool BWD>
__global__ __launch_bounds__(256) void k_bn_mom_merge(const double* __restrict__ part, int nchunk, int Ns, int nseg, int C,
                                                      double* __restrict__ mom, float* __restrict__ dw, float* __restrict__ db) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x, cc = tid % MERGE_CW, r = tid / MERGE_CW, R = 256 / MERGE_CW;
    const int c = blockIdx.x * MERGE_CW + cc;
    const bool on = c < C;
    const int rows = Ns * nchunk;
    double tw = 0.0, tb = 0.0;
    for (int s = 0; s < nseg; ++s) {
        double s1 = 0.0, s2 = 0.0;
        if (on) {
            const double2* p2 = reinterpret_cast<const double2*>(part) + (long)s * rows * C + c;
            for (int row = r; row < rows; row += R) {
                const double2 v = p2[(long)row * C];
                s1 += v.x;
                s2 += v.y;
            }
        }
        red[0][tid] = s1;
        red[1][tid] = s2;
        lane_tree<2>(red, tid, MERGE_CW);
        if (on && r == 0) {
            mom[((long)s * C + c) * 2 + 0] = red[0][cc];
            mom[((long)s * C + c) * 2 + 1] = red[1][cc];
            tb += red[0][cc];
            tw += red[1][cc];
        }
        __syncthreads();
    }
    if (BWD && on && r == 0 && dw) {
        dw[c] = (float)tw;
        db[c] = (float)tb;
    }
}

// coef / bstat of k_bn_merge<false> from (all-reduced) forward moments and the count M they were summed over
__global__ void k_bn_coef_mom(const double* __restrict__ mom, double M, const float* __restrict__ w, const float* __restrict__ b,
                              float eps, float* __restrict__ coef, double* __restrict__ bstat, int C, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = i % C;
    const double mean = mom[(long)i * 2] / M;
    double var = mom[(long)i * 2 + 1] / M - mean * mean;
    var = var < 0.0 ? 0.0 : var;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const float sc = (float)((double)w[c] * rstd);
    float* q = coef + (long)i * 4;
    q[0] = (float)mean;
    q[1] = (float)rstd;
    q[2] = sc;
    q[3] = (float)((double)b[c] - mean * (double)sc);
    if (bstat) {
        bstat[(long)i * 2 + 0] = mean;
        bstat[(long)i * 2 + 1] = var * M / (M - 1.0);
    }
}

// bcoef of k_bn_merge<true> (training mode) from (all-reduced) backward moments: (sum dz / M, sum dz*xhat / M)
__global__ void k_bn_bcoef_mom(const double* __restrict__ mom, double M, float* __restrict__ bcoef, int n2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n2) bcoef[i] = (float)(mom[i] / M);
}

// Apply pass, grid (blocks per sample, N) as InstanceNorm's k_in_apply: where the channel units divide 256 a thread keeps one channel
// unit (its coefficients in registers) for the whole launch; otherwise the flat form within the sample.
// FWD: out = dropout(act(x*scale + shift)).  BWD: dy = scale * (dz - bcoef0 - xhat * bcoef1).
template <int VEC, bool BWD, bool HG2>
__global__ __launch_bounds__(256) void k_bn_apply(const float* __restrict__ y, int ld_y, const float* __restrict__ g1, int ld_g1,
                                                  const float* __restrict__ g2, int ld_g2, const float* __restrict__ coef,
                                                  const float* __restrict__ bcoef, float* __restrict__ out, int ld_out, int Ns, int HW,
                                                  int C, int act, float drop_p, uint64_t seed) {
    const int cq = C / VEC;
    const int n = blockIdx.y, s = n / Ns;
    const long nb = (long)n * HW;
    const float keep_scale = 1.f / (1.f - drop_p);
    const bool fixed = cq <= 256 && 256 % cq == 0;
    const int PL = fixed ? 256 / cq : 1;
    int c0 = fixed ? (int)(threadIdx.x % cq) * VEC : 0;
    float mf[VEC], rs[VEC], sc[VEC], sh[VEC], b0[VEC], b1[VEC];
    auto load_coef = [&]() {
        const float* q = coef + ((long)s * C + c0) * 4;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            mf[k] = q[4 * k]; rs[k] = q[4 * k + 1]; sc[k] = q[4 * k + 2]; sh[k] = q[4 * k + 3];
        }
        if (BWD) {
            const float* bq = bcoef + ((long)s * C + c0) * 2;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                b0[k] = bq[2 * k];
                b1[k] = bq[2 * k + 1];
            }
        }
    };
    if (fixed) load_coef();
    const int first = fixed ? blockIdx.x * PL + (int)(threadIdx.x / cq) : blockIdx.x * 256 + (int)threadIdx.x;
    const int step = fixed ? gridDim.x * PL : gridDim.x * 256;
    const int limit = fixed ? HW : HW * cq;
    auto one = [&](long gp, const Vec<VEC>& v, Vec<VEC> g, const Vec<VEC>& h) {
        Vec<VEC> o;
        if (!BWD) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float a = pg_act(__fadd_rn(__fmul_rn(v.v[k], sc[k]), sh[k]), act);
                if (drop_p > 0.f) a = pg_dropout_keep(seed, (uint64_t)gp * C + c0 + k, drop_p) ? a * keep_scale : 0.f;
                o.v[k] = a;
            }
        } else {
            if (HG2) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) g.v[k] += h.v[k];
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float dz = bn_dz(g.v[k], v.v[k], sc[k], sh[k], act, drop_p, keep_scale, seed, (uint64_t)gp * C + c0 + k);
                o.v[k] = sc[k] * (dz - b0[k] - (v.v[k] - mf[k]) * rs[k] * b1[k]);
            }
        }
        vstore<VEC>(out + gp * ld_out + c0, o);
    };
    int i = first;
    if (fixed) {
        constexpr int UNR = 4;
        for (; i + (UNR - 1) * step < limit; i += UNR * step) {
            Vec<VEC> v[UNR], g[UNR], h[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const long gp = nb + i + u * step;
                v[u] = vload<VEC>(y + gp * ld_y + c0);
                if (BWD) {
                    g[u] = vload<VEC>(g1 + gp * ld_g1 + c0);
                    if (HG2) h[u] = vload<VEC>(g2 + gp * ld_g2 + c0);
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) one(nb + i + u * step, v[u], g[u], h[u]);
        }
    }
    for (; i < limit; i += step) {
        int p = i;
        if (!fixed) {
            p = i / cq;
            c0 = (i - p * cq) * VEC;
            load_coef();
        }
        const long gp = nb + p;
        Vec<VEC> v = vload<VEC>(y + gp * ld_y + c0), g, h;
        if (BWD) {
            g = vload<VEC>(g1 + gp * ld_g1 + c0);
            if (HG2) h = vload<VEC>(g2 + gp * ld_g2 + c0);
        }
        one(gp, v, g, h);
    }
}

__global__ void k_bn_eval_coef(const float* __restrict__ rm, const float* __restrict__ rv, const float* __restrict__ w,
                               const float* __restrict__ b, int C, float eps, float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double rstd = 1.0 / sqrt((double)rv[c] + (double)eps);
    const float sc = (float)((double)w[c] * rstd);
    coef[c * 4 + 0] = rm[c];
    coef[c * 4 + 1] = (float)rstd;
    coef[c * 4 + 2] = sc;
    coef[c * 4 + 3] = (float)((double)b[c] - (double)rm[c] * (double)sc);
}

// running statistics of every BatchNorm layer of a network, `nslots` updates each in slot order (torch: running = (1 - momentum) *
// running + momentum * batch, evaluated in double and stored as float after every update), num_batches_tracked += nslots
struct BnUpdateArgs {
    pg_bn_update_item it[PG_BN_MAX_LAYERS];
};
__global__ void k_bn_update(BnUpdateArgs a, int nslots, float momentum) {
    const pg_bn_update_item& it = a.it[blockIdx.x];
    const double m = (double)momentum;
    for (int c = threadIdx.x; c < it.C; c += blockDim.x) {
        float rm = it.running_mean[c], rv = it.running_var[c];
        for (int s = 0; s < nslots; ++s) {
            const double* q = it.bstat + ((long)s * it.C + c) * 2;
            rm = (float)(m * q[0] + (1.0 - m) * (double)rm);
            rv = (float)(m * q[1] + (1.0 - m) * (double)rv);
        }
        it.running_mean[c] = rm;
        it.running_var[c] = rv;
    }
    if (threadIdx.x == 0) it.num_batches_tracked[0] += nslots;
}

struct BnPlan {
    int G, groups, nchunk, ppc;
    size_t part_bytes;
};
constexpr int BN_CHUNK_MIN = 512;      // planes below this many pixels are never chunked

// chunked plan: channel-group width G (<= 64 units), pixel chunks so that the grid has >= ~1024 workgroups -- InstanceNorm's chunk_plan
// (norm_act.hip) with its defaults, so that both norms choose the one-kernel or the chunked form of a layer alike: chunked iff nchunk > 1
BnPlan bn_plan(int N, int HW, int C, int vecw) {
    BnPlan p;
    const int units = C / vecw;
    int G = 1;
    while (G < 64 && G * 2 <= units) G *= 2;
    p.G = G;
    p.groups = (units + G - 1) / G;
    int nchunk = 1;
    if (HW >= BN_CHUNK_MIN) {
        long want = (1024 + (long)N * p.groups - 1) / ((long)N * p.groups);
        const long maxc = HW / ((256 / G) * 2);         // at least two pixels per lane per chunk
        if (want > maxc) want = maxc;
        if (want > 1024) want = 1024;
        nchunk = want < 1 ? 1 : (int)want;
    }
    p.ppc = (HW + nchunk - 1) / nchunk;
    p.nchunk = (HW + p.ppc - 1) / p.ppc;
    p.part_bytes = ((size_t)N * p.nchunk * C * 2 * sizeof(double) + 255) & ~(size_t)255;
    return p;
}

// channel units per workgroup of the one-kernel forms: as many as keeps >= 64 workgroups, at most 32
int bn_small_group(int units) {
    int G = 1;
    while (G < 32 && G * 2 <= units && (units + G * 2 - 1) / (G * 2) >= 64) G *= 2;
    return G;
}

inline dim3 bn_apply_grid(int N, int HW, int units) {
    const long per_sample = ((long)HW * units + 255) / 256;
    long gx = (4096 + N - 1) / N;
    if (gx > (per_sample + 3) / 4) gx = (per_sample + 3) / 4;
    if (gx < 1) gx = 1;
    return dim3((unsigned)gx, (unsigned)N);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

size_t bcoef_bytes(int nseg, int C) { return ((size_t)nseg * C * 2 * sizeof(float) + 255) & ~(size_t)255; }

// minm: the fewest pixels a segment may have (2 where batch statistics are formed, 1 in evaluation mode)
bool bad_geom(int N, int HW, int C, int nseg, int minm = 2) {
    return N <= 0 || HW <= 0 || C <= 0 || nseg < 1 || nseg > 2 || N % nseg != 0 || N > 65535 || (long)(N / nseg) * HW < minm;
}

}  // namespace

extern "C" {

size_t pg_batchnorm_workspace_bytes(int N, int HW, int C, int nseg) {
    if (bad_geom(N, HW, C, nseg, 1)) return 0;
    const BnPlan b = bn_plan(N, HW, C, 1);
    // fewer than 4 channels have no VEC 4 plan: its channel-group count is 0, and bn_plan divides by it
    const size_t a = C >= 4 ? bn_plan(N, HW, C, 4).part_bytes : 0;
    return std::max(a, b.part_bytes) + bcoef_bytes(nseg, C);
}

// One rule for the three entry points that take a workspace, whatever kernel the views select (the one-workgroup kernels of small
// planes use none of it): the caller passes what the query says, or the call is refused before anything is launched.
static bool ws_short(int N, int HW, int C, int nseg, const void* ws, size_t ws_bytes) {
    return !ws || ws_bytes < pg_batchnorm_workspace_bytes(N, HW, C, nseg);
}

int pg_batchnorm_stats(const float* y, int ld_y, const double* part, int chunks, const float* weight, const float* bias, float* coef,
                       double* bstat, int N, int HW, int C, int nseg, float eps, void* ws, size_t ws_bytes, void* stream) {
    if (bad_geom(N, HW, C, nseg) || !weight || !bias || !coef || ld_y < C) return PG_EINVAL;
    if (part ? chunks <= 0 : !y) return PG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int Ns = N / nseg;
    if (!part) {
        const bool vec = (C % 4 == 0) && (ld_y % 4 == 0) && al16(y);
        const BnPlan p = bn_plan(N, HW, C, vec ? 4 : 1);
        if (ws_short(N, HW, C, nseg, ws, ws_bytes)) return PG_EWORKSPACE;
        const dim3 grid(p.groups, p.nchunk, N);
        if (vec)
            hipLaunchKernelGGL((k_bn_partial<4, false, false>), grid, dim3(256), 0, st, y, ld_y, nullptr, 0, nullptr, 0, nullptr,
                               (double*)ws, Ns, HW, C, p.G, p.ppc, 0, 0.f, 0ull);
        else
            hipLaunchKernelGGL((k_bn_partial<1, false, false>), grid, dim3(256), 0, st, y, ld_y, nullptr, 0, nullptr, 0, nullptr,
                               (double*)ws, Ns, HW, C, p.G, p.ppc, 0, 0.f, 0ull);
        if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
        part = (const double*)ws;
        chunks = p.nchunk;
    }
    hipLaunchKernelGGL((k_bn_merge<false>), dim3((C + MERGE_CW - 1) / MERGE_CW), dim3(256), 0, st, part, chunks, Ns, nseg, HW, C, eps,
                       weight, bias, coef, bstat, (float*)nullptr, (float*)nullptr, (float*)nullptr, 1);
    return pg_launch_status();
}

int pg_batchnorm_eval_coef(const float* running_mean, const float* running_var, const float* weight, const float* bias, int C,
                           float eps, float* coef, void* stream) {
    if (!running_mean || !running_var || !weight || !bias || !coef || C <= 0) return PG_EINVAL;
    hipLaunchKernelGGL(k_bn_eval_coef, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, running_mean, running_var, weight,
                       bias, C, eps, coef);
    return pg_launch_status();
}

int pg_batchnorm_act_apply(const float* y, int ld_y, float* out, int ld_out, const float* coef, int N, int HW, int C, int nseg,
                           int act, float drop_p, uint64_t seed, void* stream) {
    if (!y || !out || !coef || N <= 0 || HW <= 0 || C <= 0 || nseg < 1 || nseg > 2 || N % nseg || N > 65535) return PG_EINVAL;
    if (ld_y < C || ld_out < C || drop_p < 0.f || drop_p >= 1.f || act < 0 || act > PG_ACT_SIGMOID) return PG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int Ns = N / nseg;
    const bool vec = (C % 4 == 0) && (ld_y % 4 == 0) && (ld_out % 4 == 0) && al16(y) && al16(out);
    if (vec)
        hipLaunchKernelGGL((k_bn_apply<4, false, false>), bn_apply_grid(N, HW, C / 4), dim3(256), 0, st, y, ld_y, nullptr, 0, nullptr, 0,
                           coef, nullptr, out, ld_out, Ns, HW, C, act, drop_p, seed);
    else
        hipLaunchKernelGGL((k_bn_apply<1, false, false>), bn_apply_grid(N, HW, C), dim3(256), 0, st, y, ld_y, nullptr, 0, nullptr, 0,
                           coef, nullptr, out, ld_out, Ns, HW, C, act, drop_p, seed);
    return pg_launch_status();
}

int pg_batchnorm_act_fwd(const float* y, int ld_y, float* out, int ld_out, const float* weight, const float* bias, float* coef,
                         double* bstat, int N, int HW, int C, int nseg, int act, float eps, float drop_p, uint64_t seed, void* ws,
                         size_t ws_bytes, void* stream) {
    if (bad_geom(N, HW, C, nseg) || !y || !out || !weight || !bias || !coef || ld_y < C || ld_out < C) return PG_EINVAL;
    if (drop_p < 0.f || drop_p >= 1.f || act < 0 || act > PG_ACT_SIGMOID) return PG_EINVAL;
    if (ws_short(N, HW, C, nseg, ws, ws_bytes)) return PG_EWORKSPACE;
    const bool vec = (C % 4 == 0) && (ld_y % 4 == 0) && (ld_out % 4 == 0) && al16(y) && al16(out);
    if (bn_plan(N, HW, C, vec ? 4 : 1).nchunk > 1) {          // (the decision of pg_instnorm_act_fwd_t for the same views)
        const int rc = pg_batchnorm_stats(y, ld_y, nullptr, 0, weight, bias, coef, bstat, N, HW, C, nseg, eps, ws, ws_bytes, stream);
        if (rc) return rc;
        return pg_batchnorm_act_apply(y, ld_y, out, ld_out, coef, N, HW, C, nseg, act, drop_p, seed, stream);
    }
    hipStream_t st = (hipStream_t)stream;
    const int Ns = N / nseg;
    if (vec) {
        const int units = C / 4, G = bn_small_group(units);
        hipLaunchKernelGGL(k_bn_fwd_small<4>, dim3((units + G - 1) / G), dim3(256), 0, st, y, ld_y, out, ld_out, weight, bias, coef,
                           bstat, Ns, HW, C, nseg, G, act, eps, drop_p, seed);
    } else {
        const int G = bn_small_group(C);
        hipLaunchKernelGGL(k_bn_fwd_small<1>, dim3((C + G - 1) / G), dim3(256), 0, st, y, ld_y, out, ld_out, weight, bias, coef, bstat,
                           Ns, HW, C, nseg, G, act, eps, drop_p, seed);
    }
    return pg_launch_status();
}

int pg_batchnorm_act_bwd(const float* g1, int ld_g1, const float* g2, int ld_g2, const float* y, int ld_y, const float* coef,
                         float* dy, int ld_dy, float* dweight, float* dbias, int N, int HW, int C, int nseg, int train, int act,
                         float drop_p, uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    if (bad_geom(N, HW, C, nseg, train ? 2 : 1) || !g1 || !y || !coef || !dy || ld_g1 < C || ld_y < C || ld_dy < C || (g2 && ld_g2 < C))
        return PG_EINVAL;
    if ((!dweight) != (!dbias) || drop_p < 0.f || drop_p >= 1.f || act < 0 || act > PG_ACT_SIGMOID) return PG_EINVAL;
    if (ws_short(N, HW, C, nseg, ws, ws_bytes)) return PG_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int Ns = N / nseg;
    const int tr = train ? 1 : 0;
    const bool vec = (C % 4 == 0) && (ld_g1 % 4 == 0) && (ld_y % 4 == 0) && (ld_dy % 4 == 0) && al16(g1) && al16(y) && al16(dy) &&
                     (!g2 || ((ld_g2 % 4 == 0) && al16(g2)));
    const BnPlan p = bn_plan(N, HW, C, vec ? 4 : 1);
    if (p.nchunk > 1) {
        double* part = (double*)ws;
        float* bcoef = (float*)((char*)ws + p.part_bytes);
        const dim3 grid(p.groups, p.nchunk, N);
#define BN_GO(K, V, GRID, ...)                                                                        \
        do {                                                                                          \
            if (g2) hipLaunchKernelGGL((K<V, true, true>), GRID, dim3(256), 0, st, __VA_ARGS__);      \
            else hipLaunchKernelGGL((K<V, true, false>), GRID, dim3(256), 0, st, __VA_ARGS__);        \
        } while (0)
        if (vec) BN_GO(k_bn_partial, 4, grid, y, ld_y, g1, ld_g1, g2, ld_g2, coef, part, Ns, HW, C, p.G, p.ppc, act, drop_p, seed);
        else BN_GO(k_bn_partial, 1, grid, y, ld_y, g1, ld_g1, g2, ld_g2, coef, part, Ns, HW, C, p.G, p.ppc, act, drop_p, seed);
        if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
        hipLaunchKernelGGL((k_bn_merge<true>), dim3((C + MERGE_CW - 1) / MERGE_CW), dim3(256), 0, st, (const double*)part, p.nchunk, Ns,
                           nseg, HW, C, 0.f, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (double*)nullptr, bcoef,
                           dweight, dbias, tr);
        if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
        if (vec) BN_GO(k_bn_apply, 4, bn_apply_grid(N, HW, C / 4), y, ld_y, g1, ld_g1, g2, ld_g2, coef, bcoef, dy, ld_dy, Ns, HW, C, act, drop_p, seed);
        else BN_GO(k_bn_apply, 1, bn_apply_grid(N, HW, C), y, ld_y, g1, ld_g1, g2, ld_g2, coef, bcoef, dy, ld_dy, Ns, HW, C, act, drop_p, seed);
#undef BN_GO
        return pg_launch_status();
    }
    if (vec) {
        const int units = C / 4, G = bn_small_group(units);
        hipLaunchKernelGGL(k_bn_bwd_small<4>, dim3((units + G - 1) / G), dim3(256), 0, st, g1, ld_g1, g2, ld_g2, y, ld_y, coef, dy, ld_dy,
                           dweight, dbias, Ns, HW, C, nseg, G, tr, act, drop_p, seed);
    } else {
        const int G = bn_small_group(C);
        hipLaunchKernelGGL(k_bn_bwd_small<1>, dim3((C + G - 1) / G), dim3(256), 0, st, g1, ld_g1, g2, ld_g2, y, ld_y, coef, dy, ld_dy,
                           dweight, dbias, Ns, HW, C, nseg, G, tr, act, drop_p, seed);
    }
    return pg_launch_status();
}

// ---- split form: moments -> (the caller's all-reduce of mom) -> coefficients / backward apply.  One workspace rule for the three
// entry points that take one: pg_batchnorm_workspace_bytes of the LOCAL geometry.
int pg_batchnorm_moments_fwd(const float* y, int ld_y, const double* part, int chunks, double* mom, int N, int HW, int C, int nseg,
                             void* ws, size_t ws_bytes, void* stream) {
    if (bad_geom(N, HW, C, nseg, 1) || !mom || ld_y < C) return PG_EINVAL;
    if (part ? chunks <= 0 : !y) return PG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int Ns = N / nseg;
    if (!part) {
        if (ws_short(N, HW, C, nseg, ws, ws_bytes)) return PG_EWORKSPACE;
        const bool vec = (C % 4 == 0) && (ld_y % 4 == 0) && al16(y);
        const BnPlan p = bn_plan(N, HW, C, vec ? 4 : 1);
        if (p.nchunk == 1) {
            if (vec) {
                const int units = C / 4, G = bn_small_group(units);
                hipLaunchKernelGGL((k_bn_mom_small<4, false>), dim3((units + G - 1) / G), dim3(256), 0, st, y, ld_y, nullptr, 0, nullptr,
                                   0, nullptr, mom, nullptr, nullptr, Ns, HW, C, nseg, G, 0, 0.f, 0ull);
            } else {
                const int G = bn_small_group(C);
                hipLaunchKernelGGL((k_bn_mom_small<1, false>), dim3((C + G - 1) / G), dim3(256), 0, st, y, ld_y, nullptr, 0, nullptr, 0,
                                   nullptr, mom, nullptr, nullptr, Ns, HW, C, nseg, G, 0, 0.f, 0ull);
            }
            return pg_launch_status();
        }
        const dim3 grid(p.groups, p.nchunk, N);
        if (vec)
            hipLaunchKernelGGL((k_bn_partial<4, false, false>), grid, dim3(256), 0, st, y, ld_y, nullptr, 0, nullptr, 0, nullptr,
                               (double*)ws, Ns, HW, C, p.G, p.ppc, 0, 0.f, 0ull);
        else
            hipLaunchKernelGGL((k_bn_partial<1, false, false>), grid, dim3(256), 0, st, y, ld_y, nullptr, 0, nullptr, 0, nullptr,
                               (double*)ws, Ns, HW, C, p.G, p.ppc, 0, 0.f, 0ull);
        if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
        part = (const double*)ws;
        chunks = p.nchunk;
    }
    hipLaunchKernelGGL((k_bn_mom_merge<false>), dim3((C + MERGE_CW - 1) / MERGE_CW), dim3(256), 0, st, part, chunks, Ns, nseg, C, mom,
                       (float*)nullptr, (float*)nullptr);
    return pg_launch_status();
}

int pg_batchnorm_coef_from_moments(const double* mom, double count, const float* weight, const float* bias, float eps, float* coef,
                                   double* bstat, int C, int nseg, void* stream) {
    if (!mom || !weight || !bias || !coef || C <= 0 || nseg < 1 || nseg > 2 || !(count > 1.0)) return PG_EINVAL;
    const int n = nseg * C;
    hipLaunchKernelGGL(k_bn_coef_mom, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, mom, count, weight, bias, eps, coef,
                       bstat, C, n);
    return pg_launch_status();
}

int pg_batchnorm_moments_bwd(const float* g1, int ld_g1, const float* g2, int ld_g2, const float* y, int ld_y, const float* coef,
                             double* mom, float* dweight, float* dbias, int N, int HW, int C, int nseg, int act, float drop_p,
                             uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    if (bad_geom(N, HW, C, nseg, 1) || !g1 || !y || !coef || !mom || ld_g1 < C || ld_y < C || (g2 && ld_g2 < C)) return PG_EINVAL;
    if ((!dweight) != (!dbias) || drop_p < 0.f || drop_p >= 1.f || act < 0 || act > PG_ACT_SIGMOID) return PG_EINVAL;
    if (ws_short(N, HW, C, nseg, ws, ws_bytes)) return PG_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int Ns = N / nseg;
    const bool vec = (C % 4 == 0) && (ld_g1 % 4 == 0) && (ld_y % 4 == 0) && al16(g1) && al16(y) && (!g2 || ((ld_g2 % 4 == 0) && al16(g2)));
    const BnPlan p = bn_plan(N, HW, C, vec ? 4 : 1);
    if (p.nchunk == 1) {
        if (vec) {
            const int units = C / 4, G = bn_small_group(units);
            hipLaunchKernelGGL((k_bn_mom_small<4, true>), dim3((units + G - 1) / G), dim3(256), 0, st, y, ld_y, g1, ld_g1, g2, ld_g2, coef,
                               mom, dweight, dbias, Ns, HW, C, nseg, G, act, drop_p, seed);
        } else {
            const int G = bn_small_group(C);
            hipLaunchKernelGGL((k_bn_mom_small<1, true>), dim3((C + G - 1) / G), dim3(256), 0, st, y, ld_y, g1, ld_g1, g2, ld_g2, coef, mom,
                               dweight, dbias, Ns, HW, C, nseg, G, act, drop_p, seed);
        }
        return pg_launch_status();
    }
    double* part = (double*)ws;
    const dim3 grid(p.groups, p.nchunk, N);
#define BN_GO(V, ...)                                                                                            \
    do {                                                                                                         \
        if (g2) hipLaunchKernelGGL((k_bn_partial<V, true, true>), grid, dim3(256), 0, st, __VA_ARGS__);          \
        else hipLaunchKernelGGL((k_bn_partial<V, true, false>), grid, dim3(256), 0, st, __VA_ARGS__);            \
    } while (0)
    if (vec) BN_GO(4, y, ld_y, g1, ld_g1, g2, ld_g2, coef, part, Ns, HW, C, p.G, p.ppc, act, drop_p, seed);
    else BN_GO(1, y, ld_y, g1, ld_g1, g2, ld_g2, coef, part, Ns, HW, C, p.G, p.ppc, act, drop_p, seed);
#undef BN_GO
    if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
    hipLaunchKernelGGL((k_bn_mom_merge<true>), dim3((C + MERGE_CW - 1) / MERGE_CW), dim3(256), 0, st, (const double*)part, p.nchunk, Ns,
                       nseg, C, mom, dweight, dbias);
    return pg_launch_status();
}

int pg_batchnorm_bwd_apply(const float* g1, int ld_g1, const float* g2, int ld_g2, const float* y, int ld_y, const float* coef,
                           const double* mom, double count, float* dy, int ld_dy, int N, int HW, int C, int nseg, int act,
                           float drop_p, uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    if (bad_geom(N, HW, C, nseg, 1) || !g1 || !y || !coef || !mom || !dy || ld_g1 < C || ld_y < C || ld_dy < C || (g2 && ld_g2 < C))
        return PG_EINVAL;
    if (!(count > 1.0) || drop_p < 0.f || drop_p >= 1.f || act < 0 || act > PG_ACT_SIGMOID) return PG_EINVAL;
    if (ws_short(N, HW, C, nseg, ws, ws_bytes)) return PG_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int Ns = N / nseg;
    const bool vec = (C % 4 == 0) && (ld_g1 % 4 == 0) && (ld_y % 4 == 0) && (ld_dy % 4 == 0) && al16(g1) && al16(y) && al16(dy) &&
                     (!g2 || ((ld_g2 % 4 == 0) && al16(g2)));
    float* bcoef = (float*)ws;
    const int n2 = nseg * C * 2;
    hipLaunchKernelGGL(k_bn_bcoef_mom, dim3((n2 + 255) / 256), dim3(256), 0, st, mom, count, bcoef, n2);
    if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
#define BN_GO(V, GRID, ...)                                                                                      \
    do {                                                                                                         \
        if (g2) hipLaunchKernelGGL((k_bn_apply<V, true, true>), GRID, dim3(256), 0, st, __VA_ARGS__);            \
        else hipLaunchKernelGGL((k_bn_apply<V, true, false>), GRID, dim3(256), 0, st, __VA_ARGS__);              \
    } while (0)
    if (vec) BN_GO(4, bn_apply_grid(N, HW, C / 4), y, ld_y, g1, ld_g1, g2, ld_g2, coef, bcoef, dy, ld_dy, Ns, HW, C, act, drop_p, seed);
    else BN_GO(1, bn_apply_grid(N, HW, C), y, ld_y, g1, ld_g1, g2, ld_g2, coef, bcoef, dy, ld_dy, Ns, HW, C, act, drop_p, seed);
#undef BN_GO
    return pg_launch_status();
}

int pg_batchnorm_update_running(int n, const pg_bn_update_item* items, int nslots, float momentum, void* stream) {
    if (n <= 0 || n > PG_BN_MAX_LAYERS || !items || nslots <= 0 || !(momentum >= 0.f && momentum <= 1.f)) return PG_EINVAL;
    BnUpdateArgs a;
    for (int i = 0; i < n; ++i) {
        const pg_bn_update_item& it = items[i];
        if (!it.bstat || !it.running_mean || !it.running_var || !it.num_batches_tracked || it.C <= 0) return PG_EINVAL;
        a.it[i] = it;
    }
    hipLaunchKernelGGL(k_bn_update, dim3(n), dim3(256), 0, (hipStream_t)stream, a, nslots, momentum);
    return pg_launch_status();
}

}  // extern "C"
