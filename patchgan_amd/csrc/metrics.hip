// metrics.hip -- the integer counts every segmentation score is made of (IoU, Dice, precision, recall, pixel accuracy), accumulated on
// the device beside the loss reductions: a K x K confusion matrix of prediction against target plus the number of ignored pixels.
// One HBM-bound pass over N*HW pixels (2 * C * 4 bytes per pixel); integer sums only, so the result does not depend on the order in
// which workgroups arrive -- deterministic, and exactly what NumPy counts.
//
//   C == 1 : q = (p >= threshold), t = (y >= 0.5)                                  K = 2, nothing ignored
//   C  > 1 : q = first index of max p[0..C), t = first index of max y[0..C)          K = C
//            (strict `>` scan from channel 0: numpy.argmax, k_tiles_blend); a pixel whose largest y is <= 0 carries no listed label
//            and only adds 1 to counts[K*K]
//   counts[t*K + q] += 1
//
// Per workgroup: a table of 32-bit counters in LDS (ds_add_u32, no return value), moved to the 64-bit global words with one integer
// atomicAdd per non-zero counter when the workgroup is done.  The binary case does not touch LDS per pixel: three wave ballots and four
// popcounts per trip, kept in registers (64 colliding LDS adds otherwise).  A workgroup adds at most 256 per trip, so its table is
// moved out every EPOCH_TRIPS trips (2^22 * 256 = 2^30 < 2^32): a 32-bit counter cannot wrap whatever N * HW is.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "patchgan_hip.h"
#include "pg_common.h"

namespace {

constexpr int MAX_C = 32;
constexpr int MAX_WORDS = MAX_C * MAX_C + 1;
constexpr long EPOCH_TRIPS = 1L << 22;

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool vec_ok(const void* q, int ld) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0 && (ld & 3) == 0; }

// first index of the maximum of v[0..C) and the maximum itself (numpy.argmax on finite values)
template <typename V>
__device__ __forceinline__ int first_max(const V& v, int C, float& best) {
    best = v[0];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
        const float x = v[c];
        if (x > best) {
            best = x;
            bi = c;
        }
    }
    return bi;
}

// CT: 1 = binary, 4 = four classes (16-byte loads where a view allows them), 0 = any other class count (loads by element)
template <int CT>
__global__ __launch_bounds__(256) void k_seg_confusion(const float* __restrict__ p, int ld_p, const float* __restrict__ y, int ld_y,
                                                       long npix, int C, float thr, unsigned long long* __restrict__ counts) {
    __shared__ unsigned int tab[MAX_WORDS];
    const int tid = threadIdx.x;
    const int K = CT == 1 ? 2 : (CT == 4 ? 4 : C);
    const int words = K * K + 1;
    const long stride = (long)gridDim.x * 256;
    const long trips = (npix + stride - 1) / stride;      // the same for every thread: the ballots below see whole waves
    const bool vp = CT == 4 && vec_ok(p, ld_p), vy = CT == 4 && vec_ok(y, ld_y);
    for (long trip0 = 0; trip0 < trips; trip0 += EPOCH_TRIPS) {
        const long trip1 = trip0 + EPOCH_TRIPS < trips ? trip0 + EPOCH_TRIPS : trips;
        for (int i = tid; i < words; i += 256) tab[i] = 0u;
        __syncthreads();
        unsigned int n01 = 0, n10 = 0, n11 = 0, nv = 0;      // binary: per-wave counts (wave-uniform values)
        for (long trip = trip0; trip < trip1; ++trip) {
            // (four pixels per thread with their loads issued ahead of the counts measured the same: 18.0 us at 8 x 512^2 x 4 either way)
            const long pix = trip * stride + (long)blockIdx.x * 256 + tid;
            const bool valid = pix < npix;
            if (CT == 1) {
                bool q = false, t = false;
                if (valid) {
                    q = p[(size_t)pix * ld_p] >= thr;
                    t = y[(size_t)pix * ld_y] >= 0.5f;
                }
                const unsigned long long bq = __ballot(q), bt = __ballot(t), bv = __ballot(valid);
                n11 += __popcll(bq & bt);
                n01 += __popcll(bq & ~bt);
                n10 += __popcll(bt & ~bq);
                nv += __popcll(bv);
            } else if (valid) {
                const float* pp = p + (size_t)pix * ld_p;
                const float* yp = y + (size_t)pix * ld_y;
                int q, t;
                float pmax, ymax;
                if (CT == 4) {      // (a slice of a wider pixel -- the mask channels of the discriminator input -- is read by element)
                    const f4 pv = vp ? *reinterpret_cast<const f4*>(pp) : f4{pp[0], pp[1], pp[2], pp[3]};
                    const f4 yv = vy ? *reinterpret_cast<const f4*>(yp) : f4{yp[0], yp[1], yp[2], yp[3]};
                    q = first_max(pv, 4, pmax);
                    t = first_max(yv, 4, ymax);
                } else {
                    q = first_max(pp, C, pmax);
                    t = first_max(yp, C, ymax);
                }
                atomicAdd(&tab[ymax > 0.f ? t * K + q : K * K], 1u);
            }
        }
        if (CT == 1 && (tid & 63) == 0) {
            // counts[t*2 + q]
            if (nv - n01 - n10 - n11) atomicAdd(&tab[0], nv - n01 - n10 - n11);
            if (n01) atomicAdd(&tab[1], n01);
            if (n10) atomicAdd(&tab[2], n10);
            if (n11) atomicAdd(&tab[3], n11);
        }
        __syncthreads();
        for (int i = tid; i < words; i += 256) {
            const unsigned int v = tab[i];
            if (v) atomicAdd(&counts[i], (unsigned long long)v);
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

int pg_seg_confusion_max_c(void) { return MAX_C; }

int pg_seg_confusion(const float* p, int ld_p, const float* y, int ld_y, int N, int HW, int C, float threshold,
                     unsigned long long* counts, void* stream) {
    if (!p || !y || !counts || N <= 0 || HW <= 0 || C <= 0 || C > MAX_C || ld_p < C || ld_y < C) return PG_EINVAL;
    const long npix = (long)N * HW;
    long b = (npix + 255) / 256;
    if (b > 512) b = 512;
    const dim3 grid((int)b), block(256);
    if (C == 1)
        hipLaunchKernelGGL(k_seg_confusion<1>, grid, block, 0, (hipStream_t)stream, p, ld_p, y, ld_y, npix, C, threshold, counts);
    else if (C == 4)
        hipLaunchKernelGGL(k_seg_confusion<4>, grid, block, 0, (hipStream_t)stream, p, ld_p, y, ld_y, npix, C, threshold, counts);
    else
        hipLaunchKernelGGL(k_seg_confusion<0>, grid, block, 0, (hipStream_t)stream, p, ld_p, y, ld_y, npix, C, threshold, counts);
    return pg_launch_status();
}

}  // extern "C"
