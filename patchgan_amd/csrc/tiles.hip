// tiles.hip -- tiled inference around the generator forward (reference patchgan/infer.py:14-68): cut an image into
// overlapping size x size tiles straight into the NHWC batch the generator kernels read (n_crop), and overlap-average the
// predicted tiles back into the image frame with the optional threshold and the class argmax (build_mask).  HBM-bound:
// 8 B per gathered element; the blend reads 4 B per tile element and writes 8 B per mask element.
//
// Tile k along an axis of `extent` pixels starts at  s = k*eff - max(k*eff + size - extent, 0),  eff = int(overlap*size),
// k < ceil(extent / eff)  (infer.py:20-31).  Tiles are numbered row-major, j * nx + i (the reference's j*ncropsy + i is
// the same number for the square images it supports).  The blend adds the tiles covering a pixel in that order into a
// double, divides by the cover count, compares >= threshold in double (threshold > 0) -- the reference's arithmetic and
// order, so the result is bit-identical to it.
//
// pg_tiles_gather_tta / pg_tiles_blend_win add what the reference lacks: K flipped / transposed variants of every tile as further
// samples of the batch, and a weighted average under a separable window with the variants read back through the inverse map.  The
// windowed blend's arithmetic is fixed (one rounded product per weight and per term, one rounded sum, no contraction) so that a
// NumPy loop reproduces it bit for bit; with a window of ones and K = 1 it is k_tiles_blend's acc / cnt.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "patchgan_hip.h"
#include "pg_common.h"

namespace {

__device__ __forceinline__ int tile_start(int k, int eff, int size, int extent) {
    const int s = k * eff, over = s + size - extent;
    return over > 0 ? s - over : s;
}

__global__ void k_tiles_gather(const float* __restrict__ img, int C, int H, int W, int size, int eff, int ny, int nx,
                               float* __restrict__ tiles, int ld) {
    const long total = (long)ny * nx * size * size * C;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C);
        long r = idx / C;
        const int x = (int)(r % size);
        r /= size;
        const int y = (int)(r % size);
        const int t = (int)(r / size);
        const int j = t / nx, i = t - j * nx;
        const int sy = tile_start(j, eff, size, H), sx = tile_start(i, eff, size, W);
        tiles[(((long)t * size + y) * size + x) * ld + c] = img[((long)c * H + sy + y) * W + sx + x];
    }
}

__global__ void k_tiles_blend(const float* __restrict__ tiles, int ld, int C, int size, int eff, int ny, int nx, int H,
                              int W, double thr, double* __restrict__ mask, long long* __restrict__ amax) {
    const long total = (long)H * W;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int h = (int)(idx / W), w = (int)(idx - (long)h * W);
        double best = 0.0;
        int bi = 0;
        for (int c = 0; c < C; ++c) {
            double acc = 0.0, cnt = 0.0;
            for (int j = 0; j < ny; ++j) {
                const int sy = tile_start(j, eff, size, H);
                if (h < sy || h >= sy + size) continue;
                for (int i = 0; i < nx; ++i) {
                    const int sx = tile_start(i, eff, size, W);
                    if (w < sx || w >= sx + size) continue;
                    acc += (double)tiles[(((long)(j * nx + i) * size + (h - sy)) * size + (w - sx)) * ld + c];
                    cnt += 1.0;
                }
            }
            double v = acc / cnt;
            if (thr > 0.0) v = (v >= thr) ? 1.0 : 0.0;
            if (mask) mask[((long)c * H + h) * W + w] = v;
            if (c == 0 || v > best) {      // first maximum, like numpy.argmax
                best = v;
                bi = c;
            }
        }
        if (amax) amax[idx] = bi;
    }
}

int grid_for(long total) {
    long b = (total + 255) / 256;
    if (b > 16384) b = 16384;
    return (int)(b < 1 ? 1 : b);
}

// ---- test-time augmentation and windowed blend ---------------------------------------------------------------------------------
// Variant k < K of a tile is  transpose (k & 4), then flip rows (k & 2), then flip columns (k & 1)  of the [C, size, size] tile, and
// sits at sample k * T + t of the batch (T = ny * nx).  Position (y, x) of the variant is position tta_src(k, size, y, x) of the tile;
// the same three steps undone in reverse order take position (ty, tx) of the tile to position tta_dst(k, size, ty, tx) of the variant.
__device__ __forceinline__ void tta_src(int k, int size, int y, int x, int& ty, int& tx) {
    const int xx = (k & 1) ? size - 1 - x : x, yy = (k & 2) ? size - 1 - y : y;
    ty = (k & 4) ? xx : yy;
    tx = (k & 4) ? yy : xx;
}

__device__ __forceinline__ void tta_dst(int k, int size, int ty, int tx, int& y, int& x) {
    const int yy = (k & 4) ? tx : ty, xx = (k & 4) ? ty : tx;
    y = (k & 2) ? size - 1 - yy : yy;
    x = (k & 1) ? size - 1 - xx : xx;
}

__global__ void k_tiles_gather_tta(const float* __restrict__ img, int C, int H, int W, int size, int eff, int ny, int nx, int K,
                                   float* __restrict__ tiles, int ld) {
    const int T = ny * nx;
    const long total = (long)K * T * size * size * C;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C);
        long r = idx / C;
        const int x = (int)(r % size);
        r /= size;
        const int y = (int)(r % size);
        const int s = (int)(r / size);          // sample k * T + t
        const int k = s / T, t = s - k * T;
        const int j = t / nx, i = t - j * nx;
        const int sy = tile_start(j, eff, size, H), sx = tile_start(i, eff, size, W);
        int ty, tx;
        tta_src(k, size, y, x, ty, tx);
        tiles[(((long)s * size + y) * size + x) * ld + c] = img[((long)c * H + sy + ty) * W + sx + tx];
    }
}

// First and last tile of an axis that can cover one of the pixels p0..p1 (starts are monotone, so the covering tiles are contiguous):
// every tile before `lo` ends at or before p0, every tile after `hi` starts past p1.  Taken once per workgroup for its patch (scalar
// divisions); a thread still tests each tile of [lo, hi] against its own pixel (duplicates at the clamped end all cover or all miss;
// with eff > size there are gaps).
__device__ __forceinline__ void cover_range(int p0, int p1, int eff, int size, int extent, int n, int& lo, int& hi) {
    const int m = p0 - size + 1;              // a tile covering p0 or a later pixel starts at m or later
    lo = m > 0 ? (m + eff - 1) / eff : 0;
    hi = p1 >= extent - size ? n - 1 : p1 / eff;
    if (hi > n - 1) hi = n - 1;
}

// A workgroup of 256 threads blends a 16 x 16 patch of the image, one pixel per thread: rows of 16 pixels whichever way a variant is
// read, so the transposed variants touch 64-byte runs like the plain ones.  (A 64 x 4 patch -- a wave per row of 64 pixels, the
// coalescing of k_tiles_blend -- measured no faster for the variants read along rows: EXPERIMENTS.md.)
constexpr int PW = 16, PH = 16;

__global__ void __launch_bounds__(PW * PH)
k_tiles_blend_win(const float* __restrict__ tiles, int ld, int C, int size, int eff, int ny, int nx, int H, int W, int K,
                  const double* __restrict__ win, double thr, double* __restrict__ mask, long long* __restrict__ amax) {
#pragma clang fp contract(off)
    const long T = (long)ny * nx;
    const int dy = threadIdx.x / PW, dx = threadIdx.x % PW;
    const int w0 = blockIdx.x * PW, w = w0 + dx;            // grid.x covers the width; grid.y strides over the patch rows
    int i0, i1;
    cover_range(w0, min(w0 + PW, W) - 1, eff, size, W, nx, i0, i1);
    for (long h0 = (long)blockIdx.y * PH; h0 < H; h0 += (long)gridDim.y * PH) {
        const int h = (int)h0 + dy;
        int j0, j1;
        cover_range((int)h0, min((int)h0 + PH, H) - 1, eff, size, H, ny, j0, j1);
        if (h >= H || w >= W) continue;
        double best = 0.0;
        int bi = 0;
        for (int c = 0; c < C; ++c) {
            double acc = 0.0, wsum = 0.0;
            for (int j = j0; j <= j1; ++j) {
                const int sy = tile_start(j, eff, size, H);
                if (h < sy || h >= sy + size) continue;
                for (int i = i0; i <= i1; ++i) {
                    const int sx = tile_start(i, eff, size, W);
                    if (w < sx || w >= sx + size) continue;
                    const double wgt = win[h - sy] * win[w - sx];
                    const long t = (long)j * nx + i;
                    for (int k = 0; k < K; ++k) {
                        int y, x;
                        tta_dst(k, size, h - sy, w - sx, y, x);
                        const double term = wgt * (double)tiles[(((k * T + t) * size + y) * size + x) * ld + c];
                        acc = acc + term;
                        wsum = wsum + wgt;
                    }
                }
            }
            double v = acc / wsum;
            if (thr > 0.0) v = (v >= thr) ? 1.0 : 0.0;
            if (mask) mask[((long)c * H + h) * W + w] = v;
            if (c == 0 || v > best) {      // first maximum, like numpy.argmax
                best = v;
                bi = c;
            }
        }
        if (amax) amax[(long)h * W + w] = bi;
    }
}

bool tta_ok(int K) { return K == 1 || K == 2 || K == 4 || K == 8; }

}  // namespace

extern "C" {

int pg_tiles_count(int extent, int size, int eff) {
    if (extent < size || size <= 0 || eff <= 0) return 0;
    return (extent + eff - 1) / eff;
}

int pg_tiles_gather(const float* image, int C, int H, int W, int size, int eff, float* tiles, int ld, void* stream) {
    const int ny = pg_tiles_count(H, size, eff), nx = pg_tiles_count(W, size, eff);
    if (!image || !tiles || C <= 0 || ld < C || ny <= 0 || nx <= 0) return PG_EINVAL;
    const long total = (long)ny * nx * size * size * C;
    hipLaunchKernelGGL(k_tiles_gather, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, image, C, H, W, size, eff, ny,
                       nx, tiles, ld);
    return pg_launch_status();
}

int pg_tiles_blend(const float* tiles, int ld, int C, int size, int eff, int H, int W, double threshold, double* mask,
                   long long* argmax, void* stream) {
    const int ny = pg_tiles_count(H, size, eff), nx = pg_tiles_count(W, size, eff);
    if (!tiles || (!mask && !argmax) || C <= 0 || ld < C || ny <= 0 || nx <= 0) return PG_EINVAL;
    hipLaunchKernelGGL(k_tiles_blend, dim3(grid_for((long)H * W)), dim3(256), 0, (hipStream_t)stream, tiles, ld, C, size, eff,
                       ny, nx, H, W, threshold, mask, argmax);
    return pg_launch_status();
}

int pg_tiles_tta_max(void) { return 8; }

int pg_tiles_gather_tta(const float* image, int C, int H, int W, int size, int eff, int K, float* tiles, int ld, void* stream) {
    const int ny = pg_tiles_count(H, size, eff), nx = pg_tiles_count(W, size, eff);
    if (!image || !tiles || C <= 0 || ld < C || !tta_ok(K) || ny <= 0 || nx <= 0) return PG_EINVAL;
    const long total = (long)K * ny * nx * size * size * C;
    hipLaunchKernelGGL(k_tiles_gather_tta, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, image, C, H, W, size, eff, ny,
                       nx, K, tiles, ld);
    return pg_launch_status();
}

int pg_tiles_blend_win(const float* tiles, int ld, int C, int size, int eff, int H, int W, int K, const double* window,
                       double threshold, double* mask, long long* argmax, void* stream) {
    const int ny = pg_tiles_count(H, size, eff), nx = pg_tiles_count(W, size, eff);
    if (!tiles || !window || (!mask && !argmax) || C <= 0 || ld < C || !tta_ok(K) || ny <= 0 || nx <= 0) return PG_EINVAL;
    const unsigned gx = ((unsigned)W + PW - 1) / PW, gy = ((unsigned)H + PH - 1) / PH;
    hipLaunchKernelGGL(k_tiles_blend_win, dim3(gx, gy > 65535u ? 65535u : gy), dim3(PW * PH), 0, (hipStream_t)stream, tiles, ld, C, size,
                       eff, ny, nx, H, W, K, window, threshold, mask, argmax);
    return pg_launch_status();
}

}  // extern "C"
