// diffaug.hip -- differentiable augmentation of the discriminator's inputs: the per-sample parameter table, the map and its adjoint.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "patchgan_hip.h"
#include "pg_common.h"

namespace {

constexpr int AUG_THREADS = 256;
constexpr uint64_t AUG_GOLD = 0x9e3779b97f4a7c15ULL;
constexpr uint64_t AUG_DOMAIN = 0x6469666661756721ULL;      // "diffaug!": keeps the stream apart from dropout's at an equal seed

// draw k of global sample s at step t of stream `seed` (patchgan_hip.h states the same expression)
__device__ __forceinline__ uint64_t aug_sample_key(uint64_t seed, uint64_t t, uint64_t s) {
    const uint64_t h0 = pg_mix64((seed ^ AUG_DOMAIN) + AUG_GOLD * (t + 1));
    return pg_mix64(h0 + AUG_GOLD * (s + 1));
}
__device__ __forceinline__ uint64_t aug_draw(uint64_t key, uint64_t k) { return pg_mix64(key + AUG_GOLD * (k + 1)); }

// One workgroup: every lane reads the step count, a strided loop over the samples writes the rows, and behind a barrier (every read of
// the counter is done) one lane stores t + 1.
__global__ __launch_bounds__(AUG_THREADS) void k_diffaug_params(uint64_t seed, unsigned long long* __restrict__ counter, uint64_t step,
                                                                int policy, long sample0, int N, int H, int W, int* __restrict__ params) {
    const uint64_t t = counter ? (uint64_t)*counter : step;
    const int my = H / 8, mx = W / 8, ch = H / 2, cw = W / 2;
    for (int n = threadIdx.x; n < N; n += AUG_THREADS) {
        const uint64_t key = aug_sample_key(seed, t, (uint64_t)(sample0 + n));
        int flip = 0, ty = 0, tx = 0, top = 0, left = 0, bh = 0, bw = 0;
        if (policy & PG_AUG_FLIP) flip = (int)(aug_draw(key, 0) >> 63);
        if (policy & PG_AUG_TRANSLATION) {
            ty = (int)((aug_draw(key, 1) >> 32) % (uint64_t)(2 * my + 1)) - my;
            tx = (int)((aug_draw(key, 2) >> 32) % (uint64_t)(2 * mx + 1)) - mx;
        }
        if (policy & PG_AUG_CUTOUT) {
            const int oy = (int)((aug_draw(key, 3) >> 32) % (uint64_t)(H + 1));
            const int ox = (int)((aug_draw(key, 4) >> 32) % (uint64_t)(W + 1));
            top = oy - ch / 2;
            left = ox - cw / 2;
            bh = ch;
            bw = cw;
        }
        int* row = params + (size_t)n * 8;
        row[0] = flip;
        row[1] = ty;
        row[2] = tx;
        row[3] = top;
        row[4] = left;
        row[5] = bh;
        row[6] = bw;
        row[7] = 0;
    }
    if (counter) {
        __syncthreads();
        if (threadIdx.x == 0) *counter = (unsigned long long)(t + 1);
    }
}

// The map T and its adjoint as ONE output-stationary move.  A workgroup takes chunks of AUG_THREADS consecutive pixels of one sample
// (lanes along w, then h), so the sample and its table row are uniform for the chunk: the row is read once per chunk, not per lane.
//   forward  (ADJ = false): out = dst pixel (h, w); in the box -> 0; (hs, ws) = (h - ty, w - tx) outside -> 0; flipped: ws = W-1-ws; src[hs, ws]
//   adjoint  (ADJ = true):  out = dsrc pixel (hs, w0); ws = flipped ? W-1-w0 : w0; (h, w) = (hs + ty, ws + tx) outside -> 0; in the box -> 0; g[h, w]
// T is an injective partial map of pixels, so the adjoint is a gather as well: every output element is written once, a copy or +0.
// VEC: pixels of C / 4 16-byte pieces (bases 16-byte aligned, ld and C multiples of 4); otherwise C scalars per pixel.
template <bool ADJ, bool VEC>
__global__ __launch_bounds__(AUG_THREADS) void k_diffaug_move(const float* __restrict__ in, int ld_in, float* __restrict__ out, int ld_out,
                                                             const int* __restrict__ params, int H, int W, int C, unsigned chunks_per_sample,
                                                             unsigned nchunks) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const unsigned HW = (unsigned)H * (unsigned)W;
    for (unsigned chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const unsigned n = chunk / chunks_per_sample;
        const unsigned p = (chunk - n * chunks_per_sample) * AUG_THREADS + threadIdx.x;
        const int* row = params + (size_t)n * 8;
        const int flip = row[0];
        const long ty = row[1], tx = row[2], top = row[3], left = row[4], bh = row[5], bw = row[6];
        if (p >= HW) continue;
        const int h = (int)(p / (unsigned)W), w = (int)(p - (unsigned)h * (unsigned)W);
        long hi, wi, hb, wb;          // the pixel read, and the pixel of the AUGMENTED frame the box test looks at
        if (ADJ) {
            const long ws = flip ? (long)(W - 1 - w) : (long)w;
            hi = h + ty;
            wi = ws + tx;
            hb = hi;
            wb = wi;
        } else {
            hi = h - ty;
            const long ws = w - tx;
            wi = flip ? (long)(W - 1) - ws : ws;
            hb = h;
            wb = w;
        }
        const bool ok = hi >= 0 && hi < H && wi >= 0 && wi < W && !(hb >= top && hb < top + bh && wb >= left && wb < left + bw);
        const float* ip = in + ((size_t)n * HW + (ok ? (size_t)hi * W + (size_t)wi : 0)) * ld_in;
        float* op = out + ((size_t)n * HW + p) * ld_out;
        if (VEC) {
            for (int q = 0; q < C; q += 4) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (ok) v = *reinterpret_cast<const f32x4*>(ip + q);
                *reinterpret_cast<f32x4*>(op + q) = v;
            }
        } else {
            for (int c = 0; c < C; ++c) op[c] = ok ? ip[c] : 0.f;
        }
    }
}

int move_check(const float* in, int ld_in, const float* out, int ld_out, const int* params, int N, int H, int W, int C) {
    if (!in || !out || !params || N <= 0 || H <= 0 || W <= 0 || C <= 0 || ld_in < C || ld_out < C) return PG_EINVAL;
    const long npix = (long)N * H * W;
    if (npix >= 0x7fffffffL) return PG_EINVAL;
    if ((((uintptr_t)in | (uintptr_t)out) & 3) || ((uintptr_t)params & 3)) return PG_EINVAL;
    // the byte ranges from the first element to the last channel of the last pixel must not intersect
    const uintptr_t a0 = (uintptr_t)in, a1 = a0 + (((size_t)npix - 1) * ld_in + C) * sizeof(float);
    const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (((size_t)npix - 1) * ld_out + C) * sizeof(float);
    if (a0 < b1 && b0 < a1) return PG_EINVAL;
    return PG_OK;
}

template <bool ADJ>
int move_launch(const float* in, int ld_in, float* out, int ld_out, const int* params, int N, int H, int W, int C, void* stream) {
    const int rc = move_check(in, ld_in, out, ld_out, params, N, H, W, C);
    if (rc != PG_OK) return rc;
    const unsigned HW = (unsigned)H * (unsigned)W;
    const unsigned cps = (HW + AUG_THREADS - 1) / AUG_THREADS;
    const unsigned long long total = (unsigned long long)cps * (unsigned)N;
    if (total >= 0x7fffffffULL) return PG_EINVAL;
    const unsigned nchunks = (unsigned)total;
    const unsigned grid = nchunks < 8192u ? nchunks : 8192u;          // capped and grid-strided (optim_layout.hip: blocks_for)
    const bool vec = (C & 3) == 0 && (ld_in & 3) == 0 && (ld_out & 3) == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL((k_diffaug_move<ADJ, true>), dim3(grid), dim3(AUG_THREADS), 0, (hipStream_t)stream, in, ld_in, out, ld_out, params,
                           H, W, C, cps, nchunks);
    else
        hipLaunchKernelGGL((k_diffaug_move<ADJ, false>), dim3(grid), dim3(AUG_THREADS), 0, (hipStream_t)stream, in, ld_in, out, ld_out, params,
                           H, W, C, cps, nchunks);
    return pg_launch_status();
}

}  // namespace

extern "C" {

int pg_diffaug_params(uint64_t seed, unsigned long long* counter, uint64_t step, int policy, long sample0, int N, int H, int W, int* params,
                      void* stream) {
    if (!params || N <= 0 || H <= 0 || W <= 0 || sample0 < 0 || policy < 0 || policy > (PG_AUG_FLIP | PG_AUG_TRANSLATION | PG_AUG_CUTOUT))
        return PG_EINVAL;
    if (((uintptr_t)params & 3) || ((uintptr_t)counter & 7)) return PG_EINVAL;
    hipLaunchKernelGGL(k_diffaug_params, dim3(1), dim3(AUG_THREADS), 0, (hipStream_t)stream, seed, counter, step, policy, sample0, N, H, W,
                       params);
    return pg_launch_status();
}

int pg_diffaug_fwd(const float* src, int ld_src, float* dst, int ld_dst, const int* params, int N, int H, int W, int C, void* stream) {
    return move_launch<false>(src, ld_src, dst, ld_dst, params, N, H, W, C, stream);
}

int pg_diffaug_bwd(const float* g, int ld_g, float* dsrc, int ld_dsrc, const int* params, int N, int H, int W, int C, void* stream) {
    return move_launch<true>(g, ld_g, dsrc, ld_dsrc, params, N, H, W, C, stream);
}

}  // extern "C"
