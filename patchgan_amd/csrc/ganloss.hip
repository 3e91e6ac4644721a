// ganloss.hip -- GAN objectives on the discriminator's patch map (least squares, hinge, BCE with logits): value and gradient seed of up
// to PG_GAN_MAX_TERMS terms in one launch.  The gradient of every kind is elementwise, so a term needs no reduction pass in front of
// its gradient pass: one workgroup per term sums and writes in the same sweep.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "patchgan_hip.h"
#include "pg_common.h"

namespace {

constexpr int GAN_SINGLE_THREADS = 1024;      // the one-launch path: one workgroup of 16 waves per term
constexpr long GAN_SINGLE_MAX = 16384;        // ... up to 16 elements per lane (cfg2's 16 x 30 x 30 map: 14 400)
constexpr int GAN_SLAB_THREADS = 256;         // the partial-slab path: 4096 elements per workgroup, at most GAN_SLAB_MAX_BLOCKS per term
constexpr long GAN_SLAB_ELEMS = 4096;
constexpr long GAN_SLAB_MAX_BLOCKS = 1024;

struct GanTerms {
    pg_gan_term t[PG_GAN_MAX_TERMS];
};

__host__ __device__ inline long gan_slab_blocks(long n) {
    const long b = (n + GAN_SLAB_ELEMS - 1) / GAN_SLAB_ELEMS;
    return b > GAN_SLAB_MAX_BLOCKS ? GAN_SLAB_MAX_BLOCKS : b;
}

// e(d) and de/dd of one element, fp32 (patchgan_hip.h states the expressions).  Comparisons, not fmaxf: a NaN must come out as a NaN.
__device__ __forceinline__ void gan_elem(float d, int kind, float target, float& e, float& dedd) {
    if (kind == PG_GAN_LSGAN) {
        const float a = d - target;
        e = a * a;
        dedd = 2.f * a;
    } else if (kind == PG_GAN_HINGE_D) {
        const bool real = target != 0.f;
        const float a = real ? 1.f - d : 1.f + d;
        const bool nan = a != a;
        e = (a > 0.f || nan) ? a : 0.f;
        dedd = nan ? a : (a > 0.f ? (real ? -1.f : 1.f) : 0.f);
    } else if (kind == PG_GAN_HINGE_G) {
        e = -d;
        dedd = d != d ? d : -1.f;
    } else {
        const float ex = expf(-fabsf(d));
        const float pos = d > 0.f ? d : 0.f;
        e = (pos - d * target) + log1pf(ex);
        const float s = d >= 0.f ? 1.f / (1.f + ex) : ex / (1.f + ex);
        dedd = s - target;
    }
}

// grid (blocks per term, terms).  part == nullptr: one workgroup per term, which writes the term's value; otherwise workgroup (x, y)
// takes the elements x * T + tid, + nb * T, ... of term y (nb = gan_slab_blocks(n) workgroups, the others leave at once) and writes its
// partial sum to part[y * part_stride + x].
__global__ __launch_bounds__(GAN_SINGLE_THREADS) void k_gan_loss(GanTerms T, double* __restrict__ part, long part_stride) {
    __shared__ double red[GAN_SINGLE_THREADS];
    const pg_gan_term t = T.t[blockIdx.y];
    const long nb = part ? gan_slab_blocks(t.n) : 1;
    if ((long)blockIdx.x >= nb) return;          // (uniform over the workgroup: ahead of every barrier)
    const int tid = threadIdx.x, nt = blockDim.x;
    const float sf = (float)t.scale;
    double s = 0.0;
    for (long i = (long)blockIdx.x * nt + tid; i < t.n; i += nb * nt) {
        float e, dedd;
        gan_elem(t.d[(size_t)i * t.ld], t.kind, t.target, e, dedd);
        s += (double)e;
        if (t.g) t.g[(size_t)i * t.ld_g] = sf * dedd;
    }
    red[tid] = s;
    for (int off = nt >> 1; off > 0; off >>= 1) {
        __syncthreads();
        if (tid < off) red[tid] += red[tid + off];
    }
    if (tid == 0) {
        if (part)
            part[(long)blockIdx.y * part_stride + blockIdx.x] = red[0];
        else
            *t.value = (float)(t.scale * red[0]);
    }
}

// one wave per term: the term's workgroup partials, lane l taking l, l + 64, ... in index order, then a halving tree
__global__ __launch_bounds__(64) void k_gan_loss_combine(GanTerms T, const double* __restrict__ part, long part_stride) {
    __shared__ double red[64];
    const pg_gan_term t = T.t[blockIdx.x];
    const long nb = gan_slab_blocks(t.n);
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long b = tid; b < nb; b += 64) s += part[(long)blockIdx.x * part_stride + b];
    red[tid] = s;
    for (int off = 32; off > 0; off >>= 1) {
        __syncthreads();
        if (tid < off) red[tid] += red[tid + off];
    }
    if (tid == 0) *t.value = (float)(t.scale * red[0]);
}

// -> 0: the one-launch path, > 0: doubles of workspace per term on the partial-slab path, < 0: a bad list
long gan_check(int nterms, const pg_gan_term* terms) {
    if (!terms || nterms <= 0 || nterms > PG_GAN_MAX_TERMS) return -1;
    long stride = 0;
    for (int k = 0; k < nterms; ++k) {
        const pg_gan_term& t = terms[k];
        if (!t.d || !t.value || t.n <= 0 || t.ld < 1 || (t.g && t.ld_g < 1)) return -1;
        if (t.kind < PG_GAN_LSGAN || t.kind > PG_GAN_BCE_LOGITS) return -1;
        if (t.kind == PG_GAN_HINGE_D && !(t.target == 0.f || t.target == 1.f)) return -1;
        if (t.n > GAN_SINGLE_MAX) stride = std::max(stride, gan_slab_blocks(t.n));
    }
    if (stride > 0)          // one path per call: every term's partials then have a slab of the same length
        for (int k = 0; k < nterms; ++k) stride = std::max(stride, gan_slab_blocks(terms[k].n));
    return stride;
}

}  // namespace

extern "C" {

int pg_gan_loss_max_terms(void) { return PG_GAN_MAX_TERMS; }

long pg_gan_loss_single_max(void) { return GAN_SINGLE_MAX; }

long pg_gan_loss_workspace_bytes(int nterms, const pg_gan_term* terms) {
    const long stride = gan_check(nterms, terms);
    return stride > 0 ? stride * nterms * (long)sizeof(double) : 0;
}

int pg_gan_loss(int nterms, const pg_gan_term* terms, void* ws, long ws_bytes, void* stream) {
    const long stride = gan_check(nterms, terms);
    if (stride < 0) return PG_EINVAL;
    GanTerms T;
    for (int k = 0; k < PG_GAN_MAX_TERMS; ++k) T.t[k] = terms[k < nterms ? k : 0];
    if (stride == 0) {
        hipLaunchKernelGGL(k_gan_loss, dim3(1, nterms), dim3(GAN_SINGLE_THREADS), 0, (hipStream_t)stream, T, (double*)nullptr, 0L);
        return pg_launch_status();
    }
    if (!ws || ((uintptr_t)ws & 7) || ws_bytes < stride * nterms * (long)sizeof(double)) return PG_EINVAL;
    hipLaunchKernelGGL(k_gan_loss, dim3((unsigned)stride, nterms), dim3(GAN_SLAB_THREADS), 0, (hipStream_t)stream, T, (double*)ws, stride);
    if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
    hipLaunchKernelGGL(k_gan_loss_combine, dim3(nterms), dim3(64), 0, (hipStream_t)stream, T, (const double*)ws, stride);
    return pg_launch_status();
}

}  // extern "C"
