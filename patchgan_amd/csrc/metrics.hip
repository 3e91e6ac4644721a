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

// ---- per-class prediction histograms (pg_seg_hist): the confusion counts at EVERY threshold k / bins from one pass -----------------
// Word (c*2 + t)*bins + b counts the pixels of channel c with one-vs-rest label t whose prediction falls into bin b; p * bins is exact
// in fp32 for a power-of-two bin count, so floor(p * bins) >= k exactly when p >= k / bins.  The per-workgroup table of 32-bit counters
// is DYNAMIC LDS of 2 * C * bins words (no static LDS beside it: the base stays 16-byte aligned); it moves to the 64-bit global words
// as k_seg_confusion's does, under the same epoch scheme.
//
// Contention: sigmoid / softmax outputs saturate, so most lanes of a wave want bin 0 or bin bins-1 of one (channel, label) pair.  Those
// adds never reach LDS lane by lane: per channel three ballots (label, first bin, last bin) and four scalar popcounts count the wave's
// pixels in the four extreme (label, bin) cells, as the binary path of k_seg_confusion counts its four cells.  For one and four
// channels the counts stay in wave-uniform registers until the epoch ends (one lane then adds them to the table); for any other channel
// count four lanes add them to the table once per channel and trip.  Only the lanes of the bins in between issue a ds_add of 1 each.
// (A first version selected a leader lane per counter in vector code, ~60 VALU instructions per channel and pixel where this one
// has ~15; the time on cfg4's views did not change with it.)
constexpr int HIST_MIN_BINS = 16, HIST_MAX_BINS = 1024;
constexpr int HIST_MAX_WORDS = 8192;      // C * bins: 2 * 8192 counters of 4 bytes = 64 KiB of LDS, two workgroups per CU
constexpr int HIST_FLUSH_BUDGET = 1 << 19;      // workgroups x counters: bounds the 64-bit global atomics of the flush

__device__ __forceinline__ int hist_bin(float x, int bins, float fbins) {
    int b = x >= 1.f ? bins - 1 : (x <= 0.f ? 0 : (int)(x * fbins));
    return b < 0 ? 0 : (b > bins - 1 ? bins - 1 : b);      // (NaN is unspecified, but never an index outside the table)
}

// One channel of one trip, called by whole waves: lanes with `on` count their (label t, bin b) in `tab` (2 * bins words: [t][b]) if the
// bin lies in between; the wave's pixels in the first / last bin are added to n[0..4): [first bin, label 0], [first, 1], [last, 0], [last, 1].
__device__ __forceinline__ void hist_add(unsigned int* tab, bool on, bool t, int b, int bins, unsigned int (&n)[4]) {
    const bool lo = on && b == 0, hi = on && b == bins - 1;
    const unsigned long long bt = __ballot(t), b0 = __ballot(lo), bl = __ballot(hi);
    n[0] += (unsigned int)__popcll(b0 & ~bt);
    n[1] += (unsigned int)__popcll(b0 & bt);
    n[2] += (unsigned int)__popcll(bl & ~bt);
    n[3] += (unsigned int)__popcll(bl & bt);
    if (on && !lo && !hi) atomicAdd(&tab[(t ? bins : 0) + b], 1u);
}

// The four extreme cells of one channel, from one lane (n wave-uniform).
__device__ __forceinline__ void hist_add_extremes(unsigned int* tab, int bins, const unsigned int (&n)[4]) {
    if (n[0]) atomicAdd(&tab[0], n[0]);
    if (n[1]) atomicAdd(&tab[bins], n[1]);
    if (n[2]) atomicAdd(&tab[bins - 1], n[2]);
    if (n[3]) atomicAdd(&tab[2 * bins - 1], n[3]);
}

// CT as in k_seg_confusion.  hist: C * 2 * bins + 1 words, the last one counts the ignored pixels.
// Workgroups of 512: the flush costs workgroups x counters global atomics, so a table is shared by many waves, and 256 such workgroups
// still put 8 waves on every CU.  (Measured on cfg4's views at 256 bins, us: 64 workgroups of 256 with one pixel per trip 129, 128 of
// 256 with four pixels loaded ahead 57, 256 of 1024 66, 256 of 512 44 -- against 23 for k_seg_confusion on 512 of 256; cfg2's views: 12.0,
// 11.1, 9.8, 10.0 against 9.8.  EXPERIMENTS.md.)  A workgroup adds at most 512 to a counter per trip: the epoch is 2^21 trips.
constexpr int HIST_THREADS = 512;
constexpr long HIST_EPOCH_TRIPS = EPOCH_TRIPS * 256 / HIST_THREADS;      // 2^21 trips x 512 = 2^30 < 2^32

template <int CT>
__global__ __launch_bounds__(HIST_THREADS) void k_seg_hist(const float* __restrict__ p, int ld_p, const float* __restrict__ y, int ld_y,
                                                           long npix, int C, int bins, unsigned long long* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) unsigned int htab[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int Cn = CT ? CT : C;
    const int words = 2 * Cn * bins;
    const float fbins = (float)bins;
    const long stride = (long)gridDim.x * HIST_THREADS;
    const long trips = (npix + stride - 1) / stride;      // the same for every thread: the ballots below see whole waves
    const bool vp = CT == 4 && vec_ok(p, ld_p), vy = CT == 4 && vec_ok(y, ld_y);
    // (the workgroups move their tables out at about the same time: each starts at another word)
    const int rot = (int)(((long)blockIdx.x * HIST_THREADS) % words);
    for (long trip0 = 0; trip0 < trips; trip0 += HIST_EPOCH_TRIPS) {
        const long trip1 = trip0 + HIST_EPOCH_TRIPS < trips ? trip0 + HIST_EPOCH_TRIPS : trips;
        for (int i = tid; i < words; i += HIST_THREADS) htab[i] = 0u;
        __syncthreads();
        unsigned int nign = 0;      // ignored pixels of this wave (a wave-uniform value; at most 64 per trip)
        unsigned int next[CT ? CT : 1][4] = {};      // CT 1 / 4: this wave's pixels in the extreme cells of every channel (wave-uniform)
        for (long trip = trip0; trip < trip1; ++trip) {
            const long pix = trip * stride + (long)blockIdx.x * HIST_THREADS + tid;
            const bool valid = pix < npix;
            if (CT == 1) {
                float pv = 0.f, yv = 0.f;
                if (valid) {
                    pv = p[(size_t)pix * ld_p];
                    yv = y[(size_t)pix * ld_y];
                }
                hist_add(htab, valid, yv >= 0.5f, hist_bin(pv, bins, fbins), bins, next[0]);
            } else if (CT == 4) {
                f4 pv = {0.f, 0.f, 0.f, 0.f}, yv = {0.f, 0.f, 0.f, 0.f};
                if (valid) {
                    const float* pp = p + (size_t)pix * ld_p;
                    const float* yp = y + (size_t)pix * ld_y;
                    pv = vp ? *reinterpret_cast<const f4*>(pp) : f4{pp[0], pp[1], pp[2], pp[3]};
                    yv = vy ? *reinterpret_cast<const f4*>(yp) : f4{yp[0], yp[1], yp[2], yp[3]};
                }
                float ymax;
                const int t = first_max(yv, 4, ymax);
                const bool keep = valid && ymax > 0.f;
                nign += (unsigned int)__popcll(__ballot(valid && !keep));
#pragma unroll
                for (int c = 0; c < 4; ++c) hist_add(htab + c * 2 * bins, keep, t == c, hist_bin(pv[c], bins, fbins), bins, next[c]);
            } else {
                const float* pp = p + (size_t)(valid ? pix : 0) * ld_p;
                float ymax = 0.f;
                int t = 0;
                if (valid) t = first_max(y + (size_t)pix * ld_y, C, ymax);
                const bool keep = valid && ymax > 0.f;
                nign += (unsigned int)__popcll(__ballot(valid && !keep));
                for (int c = 0; c < C; ++c) {
                    const float x = keep ? pp[c] : 0.f;
                    unsigned int n[4] = {};
                    hist_add(htab + c * 2 * bins, keep, t == c, hist_bin(x, bins, fbins), bins, n);
                    if (lane < 4) {      // lane k adds cell k: [k & 1 ? label 1 : 0][k & 2 ? last bin : first]
                        const unsigned int v = lane == 0 ? n[0] : (lane == 1 ? n[1] : (lane == 2 ? n[2] : n[3]));
                        if (v) atomicAdd(&htab[c * 2 * bins + ((lane & 1) ? bins : 0) + ((lane & 2) ? bins - 1 : 0)], v);
                    }
                }
            }
        }
        if (CT && lane == 0) {
#pragma unroll
            for (int c = 0; c < (CT ? CT : 1); ++c) hist_add_extremes(htab + c * 2 * bins, bins, next[c]);
        }
        __syncthreads();
        for (int j = tid; j < words; j += HIST_THREADS) {
            int i = j + rot;
            if (i >= words) i -= words;
            const unsigned int v = htab[i];
            if (v) atomicAdd(&hist[i], (unsigned long long)v);
        }
        if (lane == 0 && nign) atomicAdd(&hist[words], (unsigned long long)nign);
        __syncthreads();
    }
}

}  // namespace

extern "C" {

int pg_seg_hist_max_words(void) { return HIST_MAX_WORDS; }

int pg_seg_hist(const float* p, int ld_p, const float* y, int ld_y, int N, int HW, int C, int bins, unsigned long long* hist,
                void* stream) {
    if (!p || !y || !hist || N <= 0 || HW <= 0 || C <= 0 || C > MAX_C || ld_p < C || ld_y < C) return PG_EINVAL;
    if (bins < HIST_MIN_BINS || bins > HIST_MAX_BINS || (bins & (bins - 1)) != 0 || C * bins > HIST_MAX_WORDS) return PG_EINVAL;
    const long npix = (long)N * HW;
    const int words = 2 * C * bins;
    // every workgroup ends with up to `words` global atomics: a large table gets fewer workgroups (256 up to 2048 counters, 32 at 16384)
    long cap = HIST_FLUSH_BUDGET / words;
    cap = cap > 256 ? 256 : (cap < 32 ? 32 : cap);
    long b = (npix + HIST_THREADS - 1) / HIST_THREADS;
    if (b > cap) b = cap;
    const dim3 grid((int)b), block(HIST_THREADS);
    const size_t lds = (size_t)words * sizeof(unsigned int);
    if (C == 1)
        hipLaunchKernelGGL(k_seg_hist<1>, grid, block, lds, (hipStream_t)stream, p, ld_p, y, ld_y, npix, C, bins, hist);
    else if (C == 4)
        hipLaunchKernelGGL(k_seg_hist<4>, grid, block, lds, (hipStream_t)stream, p, ld_p, y, ld_y, npix, C, bins, hist);
    else
        hipLaunchKernelGGL(k_seg_hist<0>, grid, block, lds, (hipStream_t)stream, p, ld_p, y, ld_y, npix, C, bins, hist);
    return pg_launch_status();
}

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
