/*
 * oracle/refshim/cuda_runtime.h -- just enough of the CUDA device language to run the
 * reference's kernels on the host, one host call per GPU thread.
 *
 * TEST INFRASTRUCTURE ONLY.  This header is found in place of the CUDA toolkit's when
 * the reference's .cu files are compiled by g++ (oracle/Makefile, target `ref`).  It is
 * written from the CUDA C++ Programming Guide, not from the oracle: it must NOT include
 * oracle_common.h, or the comparison of the two texture paths would prove nothing.
 *
 * What the reference leaves open stays a parameter here: the launch shape and, per
 * texture, the address mode and the filter variant.
 */
#ifndef MFSR_REFSHIM_CUDA_RUNTIME_H
#define MFSR_REFSHIM_CUDA_RUNTIME_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

/* ---- qualifiers: host functions and host globals ------------------------------------ */
#define __global__
#define __device__
#define __host__
#define __constant__
#define __shared__          /* `extern __shared__ T name[];` names a host array the wrapper file defines */
#define __restrict__ __restrict
#define __forceinline__ inline

/* ---- vector types (no over-alignment: test buffers are views at arbitrary offsets) -- */
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct uint3 { unsigned int x, y, z; };
struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

static inline float2 make_float2(float x, float y) { float2 v; v.x = x; v.y = y; return v; }
static inline float3 make_float3(float x, float y, float z) { float3 v; v.x = x; v.y = y; v.z = z; return v; }
static inline float4 make_float4(float x, float y, float z, float w) { float4 v; v.x = x; v.y = y; v.z = z; v.w = w; return v; }
static inline int2 make_int2(int x, int y) { int2 v; v.x = x; v.y = y; return v; }

/* ---- launch indices: one set per host thread ---------------------------------------- */
inline thread_local uint3 threadIdx = {0, 0, 0};
inline thread_local uint3 blockIdx = {0, 0, 0};
inline thread_local dim3 blockDim;
inline thread_local dim3 gridDim;

/* ---- math: a float operand reaches the float overload, as in device code ------------ */
using std::isnan;
using std::isfinite;
using std::isinf;
using std::exp;
using std::log;
using std::pow;
using std::sqrt;
using std::sin;
using std::cos;
using std::atan2;
using std::fabs;
using std::floor;
using std::ceil;
static inline int min(int a, int b) { return b < a ? b : a; }
static inline int max(int a, int b) { return a < b ? b : a; }
static inline unsigned int min(unsigned int a, unsigned int b) { return b < a ? b : a; }
static inline unsigned int max(unsigned int a, unsigned int b) { return a < b ? b : a; }
static inline float min(float a, float b) { return fminf(a, b); }
static inline float max(float a, float b) { return fmaxf(a, b); }

/* ---- textures ----------------------------------------------------------------------- */
enum { REFSHIM_ADDR_CLAMP = 0, REFSHIM_ADDR_MIRROR = 1 };
enum { REFSHIM_FILTER_EXACT = 0, REFSHIM_FILTER_FIXED8 = 1 };

/* A pitched 2-D array of float / float2 / float4 texels, normalised coordinates, linear
 * filtering.  cudaTextureObject_t carries the address of one of these. */
struct refshim_tex {
    const void* ptr;
    int pitch;      /* bytes */
    int w, h;       /* texels */
    int address;    /* REFSHIM_ADDR_* */
    int filter;     /* REFSHIM_FILTER_* */
};
typedef unsigned long long cudaTextureObject_t;

namespace refshim {

/* Programming Guide, "Texture Fetching": mirror mode maps x to frac(x) when floor(x) is
 * even and to 1 - frac(x) when it is odd; clamp mode clamps the texel index. */
inline float address_coord(float u, int mode)
{
    if (mode != REFSHIM_ADDR_MIRROR) return u;
    float period = floorf(u);
    float fr = u - period;
    bool odd = false;
    if (fabsf(period) < 4.0e18f) odd = (((long long)period) & 1LL) != 0;
    return odd ? 1.0f - fr : fr;
}

struct axis { int lo, hi; float frac; };

/* Linear filtering along one axis: xB = u*N - 0.5, i = floor(xB), weight = frac(xB); the two
 * texel indices are clamped to the array.  A coordinate that is not finite reads texel 0
 * (CUDA leaves it open; DESIGN.md "Canonical semantics"). */
inline axis locate(float u, int n, int mode, int filter)
{
    float xb = address_coord(u, mode) * (float)n - 0.5f;
    if (!std::isfinite(xb)) xb = 0.0f;
    float cell = floorf(xb);
    axis r;
    r.frac = xb - cell;
    if (filter == REFSHIM_FILTER_FIXED8) r.frac = floorf(r.frac * 256.0f + 0.5f) / 256.0f; /* 8 fractional bits */
    float last = (float)(n - 1);
    r.lo = (int)fminf(fmaxf(cell, 0.0f), last);
    r.hi = (int)fminf(fmaxf(cell + 1.0f, 0.0f), last);
    return r;
}

/* tex(x,y) = (1-a)(1-b) T[i,j] + a(1-b) T[i+1,j] + (1-a)b T[i,j+1] + ab T[i+1,j+1] */
inline float blend(float t00, float t10, float t01, float t11, float a, float b)
{
    return (1.0f - a) * (1.0f - b) * t00 + a * (1.0f - b) * t10 + (1.0f - a) * b * t01 + a * b * t11;
}

template <int C>
inline void fetch(cudaTextureObject_t obj, float u, float v, float* out)
{
    const refshim_tex* t = reinterpret_cast<const refshim_tex*>(static_cast<uintptr_t>(obj));
    axis ax = locate(u, t->w, t->address, t->filter);
    axis ay = locate(v, t->h, t->address, t->filter);
    const float* r0 = reinterpret_cast<const float*>(static_cast<const char*>(t->ptr) + (size_t)t->pitch * (size_t)ay.lo);
    const float* r1 = reinterpret_cast<const float*>(static_cast<const char*>(t->ptr) + (size_t)t->pitch * (size_t)ay.hi);
    for (int c = 0; c < C; c++)
        out[c] = blend(r0[C * ax.lo + c], r0[C * ax.hi + c], r1[C * ax.lo + c], r1[C * ax.hi + c], ax.frac, ay.frac);
}

inline void barrier();   /* refshim_launch.h */

} // namespace refshim

template <class T> T tex2D(cudaTextureObject_t obj, float u, float v);
template <> inline float tex2D<float>(cudaTextureObject_t obj, float u, float v)
{
    float o[1];
    refshim::fetch<1>(obj, u, v, o);
    return o[0];
}
template <> inline float2 tex2D<float2>(cudaTextureObject_t obj, float u, float v)
{
    float o[2];
    refshim::fetch<2>(obj, u, v, o);
    return make_float2(o[0], o[1]);
}
template <> inline float4 tex2D<float4>(cudaTextureObject_t obj, float u, float v)
{
    float o[4];
    refshim::fetch<4>(obj, u, v, o);
    return make_float4(o[0], o[1], o[2], o[3]);
}

static inline void __syncthreads() { refshim::barrier(); }

/* ---- host runtime calls of the reference's demo code: declared so that it compiles; it is
 *      never called (there is no device) ------------------------------------------------- */
typedef int cudaError_t;
enum { cudaSuccess = 0, cudaErrorNoDevice = 100 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };
static inline cudaError_t cudaSetDevice(int) { return cudaErrorNoDevice; }
static inline cudaError_t cudaMalloc(void** p, size_t) { *p = nullptr; return cudaErrorNoDevice; }
static inline cudaError_t cudaFree(void*) { return cudaSuccess; }
static inline cudaError_t cudaMemcpy(void*, const void*, size_t, cudaMemcpyKind) { return cudaErrorNoDevice; }
static inline cudaError_t cudaGetLastError() { return cudaErrorNoDevice; }
static inline cudaError_t cudaDeviceSynchronize() { return cudaErrorNoDevice; }
static inline const char* cudaGetErrorString(cudaError_t) { return "no CUDA device: host execution shim"; }

#endif
