// norm_elem.h -- the per-element vocabulary the InstanceNorm (norm_act.hip) and BatchNorm (batchnorm.hip) kernels share: a lane's
// VEC channels of one pixel, their loads and stores on fp32 / bf16 tensors, the derivative of the post-norm activation and the
// fixed-order LDS reduction over a workgroup's pixel lanes.  Included by those two files only; everything is file-local to each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "patchgan_hip.h"

namespace {

template <int VEC>
struct Vec {
    float v[VEC];
};

// Pointer to an fp32 or a bf16 activation tensor (bf16 storage mode); arithmetic in ELEMENTS.  Statistics, partial
// sums and all arithmetic stay fp32 / fp64 either way: a bf16 tensor is widened on load and rounded (RNE) on store.
struct TPtr {
    const char* p;
    int bf;
    __host__ __device__ TPtr operator+(long n) const { return TPtr{p + n * (bf ? 2 : 4), bf}; }
    __host__ __device__ explicit operator bool() const { return p != nullptr; }
};
inline TPtr tp(const void* p, bool bf) { return TPtr{(const char*)p, bf ? 1 : 0}; }

__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ unsigned short f2bf(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }

// VEC channels of an fp32 tensor: 16-byte accesses for VEC = 4 (two for VEC = 8), a scalar for VEC = 1
template <int VEC>
__device__ __forceinline__ Vec<VEC> vload(const float* p) {
    Vec<VEC> r;
    if constexpr (VEC == 8) {
        const float4 f = *reinterpret_cast<const float4*>(p), h = *reinterpret_cast<const float4*>(p + 4);
        r.v[0] = f.x; r.v[1] = f.y; r.v[2] = f.z; r.v[3] = f.w;
        r.v[4] = h.x; r.v[5] = h.y; r.v[6] = h.z; r.v[7] = h.w;
    } else if constexpr (VEC == 4) {
        const float4 f = *reinterpret_cast<const float4*>(p);
        r.v[0] = f.x; r.v[1] = f.y; r.v[2] = f.z; r.v[3] = f.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int VEC>
__device__ __forceinline__ void vstore(float* p, const Vec<VEC>& r) {
    if constexpr (VEC == 8) {
        *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
        *reinterpret_cast<float4*>(p + 4) = make_float4(r.v[4], r.v[5], r.v[6], r.v[7]);
    } else if constexpr (VEC == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
        *p = r.v[0];
    }
}

// KD: the storage type where the instantiation knows it (0 fp32, 1 bf16; -1 = read t.bf at run time).  VEC = 8 is bf16 by construction
// (v8_ok in norm_act.hip).  A known type leaves no branch around the access, so the loads of an unrolled loop are issued back to back.
template <int VEC, int KD = -1>
__device__ __forceinline__ Vec<VEC> vload(TPtr t) {
    Vec<VEC> r;
    const bool is_bf = (VEC == 8 || KD == 1) ? true : (KD == 0 ? false : (bool)t.bf);
    if (is_bf) {
        if constexpr (VEC == 8) {          // 16 bytes per lane on a bf16 tensor
            const uint4 u = *reinterpret_cast<const uint4*>(t.p);
            r.v[0] = __uint_as_float(u.x << 16); r.v[1] = __uint_as_float(u.x & 0xffff0000u);
            r.v[2] = __uint_as_float(u.y << 16); r.v[3] = __uint_as_float(u.y & 0xffff0000u);
            r.v[4] = __uint_as_float(u.z << 16); r.v[5] = __uint_as_float(u.z & 0xffff0000u);
            r.v[6] = __uint_as_float(u.w << 16); r.v[7] = __uint_as_float(u.w & 0xffff0000u);
        } else if constexpr (VEC == 4) {
            const uint2 u = *reinterpret_cast<const uint2*>(t.p);
            r.v[0] = __uint_as_float(u.x << 16); r.v[1] = __uint_as_float(u.x & 0xffff0000u);
            r.v[2] = __uint_as_float(u.y << 16); r.v[3] = __uint_as_float(u.y & 0xffff0000u);
        } else {
            r.v[0] = bf2f(*reinterpret_cast<const unsigned short*>(t.p));
        }
    } else {
        r = vload<VEC>(reinterpret_cast<const float*>(t.p));
    }
    return r;
}
template <int VEC, int KD = -1>
__device__ __forceinline__ void vstore(TPtr t, const Vec<VEC>& r) {
    char* q = const_cast<char*>(t.p);
    const bool is_bf = (VEC == 8 || KD == 1) ? true : (KD == 0 ? false : (bool)t.bf);
    if (is_bf) {
        if constexpr (VEC == 8) {
            uint4 u;
            u.x = (unsigned)f2bf(r.v[0]) | ((unsigned)f2bf(r.v[1]) << 16);
            u.y = (unsigned)f2bf(r.v[2]) | ((unsigned)f2bf(r.v[3]) << 16);
            u.z = (unsigned)f2bf(r.v[4]) | ((unsigned)f2bf(r.v[5]) << 16);
            u.w = (unsigned)f2bf(r.v[6]) | ((unsigned)f2bf(r.v[7]) << 16);
            *reinterpret_cast<uint4*>(q) = u;
        } else if constexpr (VEC == 4) {
            uint2 u;
            u.x = (unsigned)f2bf(r.v[0]) | ((unsigned)f2bf(r.v[1]) << 16);
            u.y = (unsigned)f2bf(r.v[2]) | ((unsigned)f2bf(r.v[3]) << 16);
            *reinterpret_cast<uint2*>(q) = u;
        } else {
            *reinterpret_cast<unsigned short*>(q) = f2bf(r.v[0]);
        }
    } else {
        vstore<VEC>(reinterpret_cast<float*>(q), r);
    }
}

// derivative of the post-norm activation evaluated at the normalised value z
__device__ __forceinline__ float pg_norm_act_grad(float z, int act) {
    switch (act) {
        case PG_ACT_LEAKY: return z > 0.f ? 1.f : 0.2f;
        case PG_ACT_RELU: return z > 0.f ? 1.f : 0.f;
        case PG_ACT_TANH: { float t = tanhf(z); return 1.f - t * t; }
        case PG_ACT_SIGMOID: { float t = 1.f / (1.f + expf(-z)); return t * (1.f - t); }
        default: return 1.f;
    }
}

// tree-reduce red[k][tid] over the pixel-lane dim (tid = pl*G + cu); result in red[k][cu]
template <int NK>
__device__ __forceinline__ void lane_tree(double (*red)[256], int tid, int G) {
    const int PL = 256 / G;
    for (int off = PL >> 1; off > 0; off >>= 1) {
        __syncthreads();
        if (tid < off * G) {
#pragma unroll
            for (int k = 0; k < NK; ++k) red[k][tid] += red[k][tid + off * G];
        }
    }
    __syncthreads();
}

}  // namespace
