// spectral.hip -- spectral normalisation of the discriminator's conv weights (torch.nn.utils.spectral_norm, one power iteration):
// pg_spectral_fwd / pg_spectral_bwd over a list of layers (include/patchgan_hip.h).
//
// A layer's weight is the PACKED block P[16 taps][Cout][Cin]; torch's matrix is Wm[o][ci*16 + tap] = P[tap][o][ci].  u (Cout) and v
// (Cin*16) are stored in torch's order, so a packed column (tap, ci) is element ci*16 + tap of v: the kernels do that arithmetic.
//
// Every phase is a launch of its own over ALL layers (an item's workgroups are the range [block0[i], block0[i+1]) of the grid), phases
// hand partial sums on through the workspace, and no workgroup reads what another wrote in the same launch.  Every sum is fp64 in an
// order fixed by the shapes alone (per lane in index order, lanes by halving distances 32 .. 1, waves in order, partials in order), no
// atomics: equal inputs give equal bits.  Each stored result is one rounding of an fp64 expression of fp32 values.
//   forward   k_sn_wtu    (iterate)  tpart[rc][tap*Cin + ci] = sum over the rows o of chunk rc of P[tap][o][ci] * u[o]
//             k_sn_v      (iterate)  t = sum_rc tpart, v[ci*16 + tap] = (float)(t / max(|t|, eps))            one workgroup per layer
//             k_sn_wv                spart[tap][o] = sum_ci P[tap][o][ci] * v[ci*16 + tap]                    one wave per row
//             k_sn_u                 s = sum_tap spart; iterate: u[o] = (float)(s / max(|s|, eps)); sigma = (float)(sum_o u[o] * s[o])
//             k_sn_scale             w_hat = (float)(W / sigma) per layer, and the floats of `flat` between the layers' blocks copied
//   backward  k_sn_dot               cpart[b] = partial sums of <dW_hat, W_hat>
//             k_sn_map               c = sum_b cpart[b]; g = (float)((g - c * u[o] * v[ci*16 + tap]) / sigma) in place
#include "pg_common.h"

namespace {

constexpr int SN_THREADS = 256;
constexpr int SN_V_THREADS = 1024;  // k_sn_v
constexpr int SN_ROWS_T = 64;       // rows of one k_sn_wtu workgroup (16 per wave)
constexpr int SN_ROWS_S = 32;       // rows of one k_sn_wv workgroup (8 per wave)
constexpr int SN_EW_BLOCKS = 256;   // workgroups per layer of the elementwise / dot launches (at most: one per CU for the largest layer)
constexpr double SN_EPS = 1e-12;

struct SnArgs {
    pg_spectral_item it[PG_SN_MAX_LAYERS];
    long ws_off[PG_SN_MAX_LAYERS];        // the item's first double in the workspace
    int block0[PG_SN_MAX_LAYERS + 1];
    int n;
};

struct SnCopy {          // the floats of `flat` outside every item's block: at most n + 1 gaps (multiples of 4 floats)
    const float* src;
    float* dst;
    long off[PG_SN_MAX_LAYERS + 1], len[PG_SN_MAX_LAYERS + 1];
    int n, block0;
};

__device__ __forceinline__ int sn_item(const SnArgs& a, int bid) {
    int i = 0;
    while (i + 1 < a.n && bid >= a.block0[i + 1]) ++i;
    return i;
}

__device__ __forceinline__ double sn_wave_sum(double a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    return a;          // (lane 0 holds the sum)
}

// the sum over the NW waves of the workgroup, returned to every thread; `part` is reused by the next call (hence the leading barrier)
template <int NW = SN_THREADS / 64>
__device__ __forceinline__ double sn_block_sum(double a, double* part) {
    a = sn_wave_sum(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    double s = part[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += part[w];
    return s;
}

__host__ __device__ inline int sn_rc(int Cout) { return (Cout + SN_ROWS_T - 1) / SN_ROWS_T; }
// workspace of one item, in doubles: tpart [rc][16*Cin] | spart [16][Cout] | cpart [SN_EW_BLOCKS]
__host__ __device__ inline long sn_ws_t(const pg_spectral_item& it) { return (long)sn_rc(it.Cout) * 16 * it.Cin; }
__host__ __device__ inline long sn_ws_s(const pg_spectral_item& it) { return 16L * it.Cout; }
__host__ __device__ inline long sn_ws_doubles(const pg_spectral_item& it) { return sn_ws_t(it) + sn_ws_s(it) + SN_EW_BLOCKS; }

// V = 4: Cin % 4 == 0 and a 16-byte-aligned block, rows read as float4 along ci; V = 1: any Cin
template <int V>
__device__ __forceinline__ void sn_wtu_body(const pg_spectral_item& it, double* __restrict__ tpart, int lb) {
    __shared__ double red[SN_THREADS / 64][64 * 4];
    const int a = it.Cout, b = it.Cin;
    const int cc_n = (b + 64 * V - 1) / (64 * V), rc_n = sn_rc(a);
    const int cc = lb % cc_n, rc = (lb / cc_n) % rc_n, tap = lb / (cc_n * rc_n);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ci = (cc * 64 + lane) * V;
    const int o_end = min(a, (rc + 1) * SN_ROWS_T);
    const float* P = it.W + (size_t)tap * a * b;
    double acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.0;
    if (ci < b) {
        for (int o = rc * SN_ROWS_T + wave; o < o_end; o += SN_THREADS / 64) {
            const double uo = it.u[o];
            if constexpr (V == 4) {
                const float4 w = *reinterpret_cast<const float4*>(P + (size_t)o * b + ci);
                acc[0] += (double)w.x * uo;
                acc[1] += (double)w.y * uo;
                acc[2] += (double)w.z * uo;
                acc[3] += (double)w.w * uo;
            } else {
                acc[0] += (double)P[(size_t)o * b + ci] * uo;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) red[wave][lane * V + j] = acc[j];
    __syncthreads();
    if (wave == 0 && ci < b) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int k = lane * V + j;
            tpart[(size_t)rc * 16 * b + (size_t)tap * b + ci + j] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
        }
    }
}

__global__ __launch_bounds__(SN_THREADS) void k_sn_wtu(SnArgs a, double* __restrict__ ws) {
    const int i = sn_item(a, blockIdx.x);
    const pg_spectral_item& it = a.it[i];
    double* tpart = ws + a.ws_off[i];
    const int lb = blockIdx.x - a.block0[i];
    if ((it.Cin & 3) == 0) sn_wtu_body<4>(it, tpart, lb);
    else sn_wtu_body<1>(it, tpart, lb);
}

// one workgroup per iterating layer (of 1024 threads: the chunk sums are a chain of dependent loads per column, measured 49 us with 256)
__global__ __launch_bounds__(SN_V_THREADS) void k_sn_v(SnArgs a, const double* __restrict__ ws) {
    __shared__ double part[SN_V_THREADS / 64];
    const int i = blockIdx.x;
    const pg_spectral_item& it = a.it[i];
    if (!it.iterate) return;
    const double* tpart = ws + a.ws_off[i];
    const int b = it.Cin, K = 16 * b, rc_n = sn_rc(it.Cout);
    double acc = 0.0;
    for (int k = threadIdx.x; k < K; k += SN_V_THREADS) {
        double t = 0.0;
        for (int r = 0; r < rc_n; ++r) t += tpart[(size_t)r * K + k];
        acc += t * t;
    }
    const double nrm = sqrt(sn_block_sum<SN_V_THREADS / 64>(acc, part));
    const double d = nrm > SN_EPS ? nrm : SN_EPS;
    for (int k = threadIdx.x; k < K; k += SN_V_THREADS) {
        double t = 0.0;
        for (int r = 0; r < rc_n; ++r) t += tpart[(size_t)r * K + k];          // (the same sum in the same order)
        const int tap = k / b, ci = k - tap * b;
        it.v[ci * 16 + tap] = (float)(t / d);
    }
}

template <int V>
__device__ __forceinline__ void sn_wv_body(const pg_spectral_item& it, double* __restrict__ spart, int lb) {
    const int a = it.Cout, b = it.Cin;
    const int rc_n = (a + SN_ROWS_S - 1) / SN_ROWS_S;
    const int rc = lb % rc_n, tap = lb / rc_n;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int o_end = min(a, (rc + 1) * SN_ROWS_S);
    const float* P = it.W + (size_t)tap * a * b;
    const float* v = it.v + tap;
    for (int o = rc * SN_ROWS_S + wave; o < o_end; o += SN_THREADS / 64) {
        double acc = 0.0;
        for (int ci = lane * V; ci < b; ci += 64 * V) {
            if constexpr (V == 4) {
                const float4 w = *reinterpret_cast<const float4*>(P + (size_t)o * b + ci);
                acc += ((double)w.x * (double)v[ci * 16] + (double)w.y * (double)v[(ci + 1) * 16]) +
                       ((double)w.z * (double)v[(ci + 2) * 16] + (double)w.w * (double)v[(ci + 3) * 16]);
            } else {
                acc += (double)P[(size_t)o * b + ci] * (double)v[ci * 16];
            }
        }
        acc = sn_wave_sum(acc);
        if (lane == 0) spart[(size_t)tap * a + o] = acc;
    }
}

__global__ __launch_bounds__(SN_THREADS) void k_sn_wv(SnArgs a, double* __restrict__ ws) {
    const int i = sn_item(a, blockIdx.x);
    const pg_spectral_item& it = a.it[i];
    double* spart = ws + a.ws_off[i] + sn_ws_t(it);
    const int lb = blockIdx.x - a.block0[i];
    if ((it.Cin & 3) == 0) sn_wv_body<4>(it, spart, lb);
    else sn_wv_body<1>(it, spart, lb);
}

__device__ __forceinline__ double sn_s(const double* __restrict__ spart, int a, int o) {
    double s = 0.0;
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) s += spart[(size_t)tap * a + o];
    return s;
}

// one workgroup per layer
__global__ __launch_bounds__(SN_THREADS) void k_sn_u(SnArgs a, const double* __restrict__ ws) {
    __shared__ double part[SN_THREADS / 64];
    const int i = blockIdx.x;
    const pg_spectral_item& it = a.it[i];
    const double* spart = ws + a.ws_off[i] + sn_ws_t(it);
    const int A = it.Cout;
    double d = 1.0;
    if (it.iterate) {
        double acc = 0.0;
        for (int o = threadIdx.x; o < A; o += SN_THREADS) {
            const double s = sn_s(spart, A, o);
            acc += s * s;
        }
        const double nrm = sqrt(sn_block_sum(acc, part));
        d = nrm > SN_EPS ? nrm : SN_EPS;
    }
    double acc = 0.0;
    for (int o = threadIdx.x; o < A; o += SN_THREADS) {
        const double s = sn_s(spart, A, o);
        float uo;
        if (it.iterate) {
            uo = (float)(s / d);
            it.u[o] = uo;
        } else {
            uo = it.u[o];
        }
        acc += (double)uo * s;          // sigma = u^T (Wm v) with the u just stored
    }
    const double sigma = sn_block_sum(acc, part);
    if (threadIdx.x == 0) *it.sigma = (float)sigma;
}

__global__ __launch_bounds__(SN_THREADS) void k_sn_scale(SnArgs a, SnCopy c) {
    if ((int)blockIdx.x >= c.block0) {
        // the floats between the weight blocks (biases, norm parameters, alignment padding): copied as they are
        const long stride = (long)(gridDim.x - c.block0) * SN_THREADS;
        const long first = (long)(blockIdx.x - c.block0) * SN_THREADS + threadIdx.x;
        for (int g = 0; g < c.n; ++g) {
            const float4* s = reinterpret_cast<const float4*>(c.src + c.off[g]);
            float4* d = reinterpret_cast<float4*>(c.dst + c.off[g]);
            const long n4 = c.len[g] >> 2;
            for (long e = first; e < n4; e += stride) d[e] = s[e];
        }
        return;
    }
    const int i = sn_item(a, blockIdx.x);
    const pg_spectral_item& it = a.it[i];
    const double sigma = *it.sigma;
    const long n4 = 4L * it.Cout * it.Cin;
    const long stride = (long)(a.block0[i + 1] - a.block0[i]) * SN_THREADS;
    const float4* s = reinterpret_cast<const float4*>(it.W);
    float4* d = reinterpret_cast<float4*>(it.w_hat);
    for (long e = (long)(blockIdx.x - a.block0[i]) * SN_THREADS + threadIdx.x; e < n4; e += stride) {
        const float4 w = s[e];
        float4 r;
        // (a correctly rounded fp32 quotient: fp64 holds the quotient of two floats to more than twice their precision)
        r.x = (float)((double)w.x / sigma);
        r.y = (float)((double)w.y / sigma);
        r.z = (float)((double)w.z / sigma);
        r.w = (float)((double)w.w / sigma);
        d[e] = r;
    }
}

__global__ __launch_bounds__(SN_THREADS) void k_sn_dot(SnArgs a, const float* __restrict__ grad, double* __restrict__ ws) {
    __shared__ double part[SN_THREADS / 64];
    const int i = sn_item(a, blockIdx.x);
    const pg_spectral_item& it = a.it[i];
    const int lb = blockIdx.x - a.block0[i];
    const long n4 = 4L * it.Cout * it.Cin;
    const long stride = (long)(a.block0[i + 1] - a.block0[i]) * SN_THREADS;
    const float4* g = reinterpret_cast<const float4*>(grad + it.g_off);
    const float4* w = reinterpret_cast<const float4*>(it.w_hat);
    double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
    for (long e = (long)lb * SN_THREADS + threadIdx.x; e < n4; e += stride) {
        const float4 gg = g[e], ww = w[e];
        ax += (double)gg.x * (double)ww.x;
        ay += (double)gg.y * (double)ww.y;
        az += (double)gg.z * (double)ww.z;
        aw += (double)gg.w * (double)ww.w;
    }
    const double sum = sn_block_sum((ax + ay) + (az + aw), part);
    if (threadIdx.x == 0) ws[a.ws_off[i] + sn_ws_t(it) + sn_ws_s(it) + lb] = sum;
}

__global__ __launch_bounds__(SN_THREADS) void k_sn_map(SnArgs a, float* __restrict__ grad, const double* __restrict__ ws) {
    const int i = sn_item(a, blockIdx.x);
    const pg_spectral_item& it = a.it[i];
    const int nb = a.block0[i + 1] - a.block0[i];
    const double* cpart = ws + a.ws_off[i] + sn_ws_t(it) + sn_ws_s(it);
    double c = 0.0;
    for (int j = 0; j < nb; ++j) c += cpart[j];          // (every thread: the same partials in the same order)
    const double sigma = *it.sigma;
    const int A = it.Cout, b = it.Cin;
    const long ab = (long)A * b, n4 = 4L * ab;
    const long stride = (long)nb * SN_THREADS;
    float4* g = reinterpret_cast<float4*>(grad + it.g_off);
    for (long e = (long)(blockIdx.x - a.block0[i]) * SN_THREADS + threadIdx.x; e < n4; e += stride) {
        const float4 gg = g[e];
        float in[4] = {gg.x, gg.y, gg.z, gg.w}, out[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long q = e * 4 + j;
            const int tap = (int)(q / ab);
            const int r = (int)(q - (long)tap * ab);
            const int o = r / b, ci = r - o * b;
            out[j] = (float)(((double)in[j] - (c * (double)it.u[o]) * (double)it.v[ci * 16 + tap]) / sigma);
        }
        g[e] = make_float4(out[0], out[1], out[2], out[3]);
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline int ew_blocks(const pg_spectral_item& it) {
    const long b = (4L * it.Cout * it.Cin + SN_THREADS - 1) / SN_THREADS;
    return (int)(b < SN_EW_BLOCKS ? b : SN_EW_BLOCKS);
}

bool bad_items(int n, const pg_spectral_item* items) {
    if (n <= 0 || n > PG_SN_MAX_LAYERS || !items) return true;
    for (int i = 0; i < n; ++i) {
        const pg_spectral_item& it = items[i];
        if (it.Cout <= 0 || it.Cin <= 0 || it.Cout > (1 << 16) || it.Cin > (1 << 16)) return true;
        if (!it.W || !it.w_hat || !it.u || !it.v || !it.sigma || !al16(it.W) || !al16(it.w_hat)) return true;
        if (it.g_off < 0 || (it.g_off & 3)) return true;
    }
    return false;
}

long ws_doubles(int n, const pg_spectral_item* items, long* off) {
    long total = 0;
    for (int i = 0; i < n; ++i) {
        if (off) off[i] = total;
        total += sn_ws_doubles(items[i]);
    }
    return total;
}

bool bad_ws(int n, const pg_spectral_item* items, const void* ws, long ws_bytes) {
    return !ws || ((uintptr_t)ws & 7) || ws_bytes < ws_doubles(n, items, nullptr) * (long)sizeof(double);
}

void fill_args(SnArgs& a, int n, const pg_spectral_item* items) {
    a.n = n;
    for (int i = 0; i < n; ++i) a.it[i] = items[i];
    ws_doubles(n, items, a.ws_off);
}

}  // namespace

extern "C" {

long pg_spectral_workspace_bytes(int n, const pg_spectral_item* items) {
    if (n <= 0 || n > PG_SN_MAX_LAYERS || !items) return 0;
    for (int i = 0; i < n; ++i)
        if (items[i].Cout <= 0 || items[i].Cin <= 0 || items[i].Cout > (1 << 16) || items[i].Cin > (1 << 16)) return 0;
    return ws_doubles(n, items, nullptr) * (long)sizeof(double);
}

int pg_spectral_fwd(int n, const pg_spectral_item* items, const float* flat, float* eff, long nflat, void* ws, long ws_bytes,
                    void* stream) {
    if (bad_items(n, items) || bad_ws(n, items, ws, ws_bytes)) return PG_EINVAL;
    SnCopy c;
    c.src = flat;
    c.dst = eff;
    c.n = 0;
    if (flat || eff) {
        // the copy of everything between the layers' blocks: the items are the blocks of `flat` in ascending order, w_hat the same
        // offsets of `eff`
        if (!flat || !eff || nflat <= 0 || (nflat & 3) || !al16(flat) || !al16(eff)) return PG_EINVAL;
        long pos = 0;
        for (int i = 0; i < n; ++i) {
            const pg_spectral_item& it = items[i];
            const intptr_t d = (intptr_t)it.W - (intptr_t)flat;
            const long off = (long)(d / (intptr_t)sizeof(float)), len = 16L * it.Cout * it.Cin;
            if (d < 0 || off < pos || off + len > nflat || it.w_hat != eff + off) return PG_EINVAL;
            if (off > pos) c.off[c.n] = pos, c.len[c.n] = off - pos, ++c.n;
            pos = off + len;
        }
        if (nflat > pos) c.off[c.n] = pos, c.len[c.n] = nflat - pos, ++c.n;
    }
    hipStream_t st = (hipStream_t)stream;
    double* wsd = (double*)ws;
    SnArgs a;
    fill_args(a, n, items);
    bool any_iter = false;
    int nb = 0;
    for (int i = 0; i < n; ++i) {
        const pg_spectral_item& it = items[i];
        a.block0[i] = nb;
        if (it.iterate) {
            any_iter = true;
            const int V = (it.Cin & 3) == 0 ? 4 : 1;
            nb += 16 * sn_rc(it.Cout) * ((it.Cin + 64 * V - 1) / (64 * V));
        }
    }
    a.block0[n] = nb;
    if (any_iter) {
        // (a non-iterating item has no workgroups: sn_item skips an empty range)
        hipLaunchKernelGGL(k_sn_wtu, dim3(nb), dim3(SN_THREADS), 0, st, a, wsd);
        if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
        hipLaunchKernelGGL(k_sn_v, dim3(n), dim3(SN_V_THREADS), 0, st, a, (const double*)wsd);
        if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
    }
    nb = 0;
    for (int i = 0; i < n; ++i) {
        a.block0[i] = nb;
        nb += 16 * ((items[i].Cout + SN_ROWS_S - 1) / SN_ROWS_S);
    }
    a.block0[n] = nb;
    hipLaunchKernelGGL(k_sn_wv, dim3(nb), dim3(SN_THREADS), 0, st, a, wsd);
    if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
    hipLaunchKernelGGL(k_sn_u, dim3(n), dim3(SN_THREADS), 0, st, a, (const double*)wsd);
    if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
    nb = 0;
    for (int i = 0; i < n; ++i) {
        a.block0[i] = nb;
        nb += ew_blocks(items[i]);
    }
    a.block0[n] = nb;
    c.block0 = nb;
    hipLaunchKernelGGL(k_sn_scale, dim3(nb + (c.n ? 4 : 0)), dim3(SN_THREADS), 0, st, a, c);
    return pg_launch_status();
}

int pg_spectral_bwd(int n, const pg_spectral_item* items, float* grad, long ngrad, void* ws, long ws_bytes, void* stream) {
    if (bad_items(n, items) || bad_ws(n, items, ws, ws_bytes) || !grad || !al16(grad) || ngrad <= 0) return PG_EINVAL;
    for (int i = 0; i < n; ++i)
        if (items[i].g_off + 16L * items[i].Cout * items[i].Cin > ngrad) return PG_EINVAL;
    SnArgs a;
    fill_args(a, n, items);
    int nb = 0;
    for (int i = 0; i < n; ++i) {
        a.block0[i] = nb;
        nb += ew_blocks(items[i]);
    }
    a.block0[n] = nb;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sn_dot, dim3(nb), dim3(SN_THREADS), 0, st, a, (const float*)grad, (double*)ws);
    if (hipGetLastError() != hipSuccess) return PG_ELAUNCH;
    hipLaunchKernelGGL(k_sn_map, dim3(nb), dim3(SN_THREADS), 0, st, a, grad, (const double*)ws);
    return pg_launch_status();
}

}  // extern "C"
