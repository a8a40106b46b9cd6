// hsr_lane_io.h — four-wide plane access of the streaming helper units (internal, not part of the C ABI), stated ONCE for
// hsr_frame_export.hip, hsr_keyframe_pack.hip, hsr_replay.hip and hsr_tsdf.hip: a lane takes V consecutive values of a planar array,
// V = 4 with one vector access and V = 1 for the tail and for callers whose pointers are off the vector path's alignment.  Here are
// the vector types, hsr_load<V> / hsr_store<V> between a plane and a lane's V registers, the 0..1 clamp with the 8-bit colour code
// that follows it, and the host's alignment test that chooses between the two widths.  Every device function is
// __device__ __forceinline__, so the including file's flags (-ffp-contract=off where the Makefile says so) apply to the inlined code.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// ---- vector types ----------------------------------------------------------------------------------------------------------------------
// A plane of N % 4 != 0 values puts the next plane off the vector's natural alignment: the _aN types are declared with the ELEMENT's
// alignment (4 for float and int, 8 for int64, 2 for the 16-bit codes, 1 for four 8-bit codes in a dword) and the compiler picks an
// access global memory takes at that alignment — it takes a 16-byte access at any dword.
typedef float hsr_f4 __attribute__((ext_vector_type(4)));
typedef int hsr_i4 __attribute__((ext_vector_type(4)));
typedef long long hsr_l2 __attribute__((ext_vector_type(2)));
typedef unsigned short hsr_h4 __attribute__((ext_vector_type(4)));
typedef hsr_f4 hsr_f4_a4 __attribute__((aligned(4)));
typedef hsr_i4 hsr_i4_a4 __attribute__((aligned(4)));
typedef hsr_l2 hsr_l2_a8 __attribute__((aligned(8)));
typedef hsr_h4 hsr_h4_a2 __attribute__((aligned(2)));
typedef unsigned hsr_u32_a1 __attribute__((aligned(1)));

// ---- V values of one plane from p on, into registers -----------------------------------------------------------------------------------
template <int V> __device__ __forceinline__ void hsr_load(const float* __restrict__ p, float (&v)[V]);
template <> __device__ __forceinline__ void hsr_load<1>(const float* __restrict__ p, float (&v)[1]) { v[0] = *p; }
template <> __device__ __forceinline__ void hsr_load<4>(const float* __restrict__ p, float (&v)[4])
{
    const hsr_f4 t = *reinterpret_cast<const hsr_f4_a4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <int V> __device__ __forceinline__ void hsr_load(const int* __restrict__ p, int (&v)[V]);
template <> __device__ __forceinline__ void hsr_load<1>(const int* __restrict__ p, int (&v)[1]) { v[0] = *p; }
template <> __device__ __forceinline__ void hsr_load<4>(const int* __restrict__ p, int (&v)[4])
{
    const hsr_i4 t = *reinterpret_cast<const hsr_i4_a4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <int V> __device__ __forceinline__ void hsr_load(const long long* __restrict__ p, long long (&v)[V]);
template <> __device__ __forceinline__ void hsr_load<1>(const long long* __restrict__ p, long long (&v)[1]) { v[0] = *p; }
template <> __device__ __forceinline__ void hsr_load<4>(const long long* __restrict__ p, long long (&v)[4])
{
    const hsr_l2 a = reinterpret_cast<const hsr_l2_a8*>(p)[0], b = reinterpret_cast<const hsr_l2_a8*>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}
template <int V> __device__ __forceinline__ void hsr_load(const uint8_t* __restrict__ p, unsigned (&v)[V]);
template <> __device__ __forceinline__ void hsr_load<1>(const uint8_t* __restrict__ p, unsigned (&v)[1]) { v[0] = *p; }
template <> __device__ __forceinline__ void hsr_load<4>(const uint8_t* __restrict__ p, unsigned (&v)[4])
{
    const unsigned t = *reinterpret_cast<const hsr_u32_a1*>(p);
    v[0] = t & 255u; v[1] = (t >> 8) & 255u; v[2] = (t >> 16) & 255u; v[3] = t >> 24;
}
template <int V> __device__ __forceinline__ void hsr_load(const uint16_t* __restrict__ p, unsigned (&v)[V]);
template <> __device__ __forceinline__ void hsr_load<1>(const uint16_t* __restrict__ p, unsigned (&v)[1]) { v[0] = *p; }
template <> __device__ __forceinline__ void hsr_load<4>(const uint16_t* __restrict__ p, unsigned (&v)[4])
{
    const hsr_h4 t = *reinterpret_cast<const hsr_h4_a2*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

// ---- and back --------------------------------------------------------------------------------------------------------------------------
template <int V> __device__ __forceinline__ void hsr_store(float* __restrict__ p, const float (&v)[V]);
template <> __device__ __forceinline__ void hsr_store<1>(float* __restrict__ p, const float (&v)[1]) { *p = v[0]; }
template <> __device__ __forceinline__ void hsr_store<4>(float* __restrict__ p, const float (&v)[4])
{
    hsr_f4 t;
    t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
    *reinterpret_cast<hsr_f4_a4*>(p) = t;
}
template <int V> __device__ __forceinline__ void hsr_store(int* __restrict__ p, const int (&v)[V]);
template <> __device__ __forceinline__ void hsr_store<1>(int* __restrict__ p, const int (&v)[1]) { *p = v[0]; }
template <> __device__ __forceinline__ void hsr_store<4>(int* __restrict__ p, const int (&v)[4])
{
    hsr_i4 t;
    t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
    *reinterpret_cast<hsr_i4_a4*>(p) = t;
}
template <int V> __device__ __forceinline__ void hsr_store(uint8_t* __restrict__ p, const unsigned (&v)[V]);
template <> __device__ __forceinline__ void hsr_store<1>(uint8_t* __restrict__ p, const unsigned (&v)[1]) { *p = (uint8_t)v[0]; }
template <> __device__ __forceinline__ void hsr_store<4>(uint8_t* __restrict__ p, const unsigned (&v)[4])
{
    *reinterpret_cast<hsr_u32_a1*>(p) = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;      // every code is below 256
}
template <int V> __device__ __forceinline__ void hsr_store(uint16_t* __restrict__ p, const unsigned (&v)[V]);
template <> __device__ __forceinline__ void hsr_store<1>(uint16_t* __restrict__ p, const unsigned (&v)[1]) { *p = (uint16_t)v[0]; }
template <> __device__ __forceinline__ void hsr_store<4>(uint16_t* __restrict__ p, const unsigned (&v)[4])
{
    hsr_h4 t;
    t.x = (unsigned short)v[0]; t.y = (unsigned short)v[1]; t.z = (unsigned short)v[2]; t.w = (unsigned short)v[3];
    *reinterpret_cast<hsr_h4_a2*>(p) = t;
}
template <int V> __device__ __forceinline__ void hsr_store(long long* __restrict__ p, const unsigned (&v)[V]);
template <> __device__ __forceinline__ void hsr_store<1>(long long* __restrict__ p, const unsigned (&v)[1]) { *p = (long long)v[0]; }
template <> __device__ __forceinline__ void hsr_store<4>(long long* __restrict__ p, const unsigned (&v)[4])
{
    hsr_l2 a, b;
    a.x = (long long)v[0]; a.y = (long long)v[1]; b.x = (long long)v[2]; b.y = (long long)v[3];
    reinterpret_cast<hsr_l2_a8*>(p)[0] = a;
    reinterpret_cast<hsr_l2_a8*>(p)[1] = b;
}

// ---- a 0..1 value as an 8-bit colour ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float hsr_clamp01(float x) { return x > 0.f ? (x < 1.f ? x : 1.f) : 0.f; }      // a NaN fails x > 0
// the code as a float, 0.0f .. 255.0f, for the caller to convert to the integer type it stores; rintf: to nearest, halves to even
__device__ __forceinline__ float hsr_colour_code(float x) { return rintf(hsr_clamp01(x) * 255.0f); }

// ---- host: may a pointer take the V = 4 accesses? --------------------------------------------------------------------------------------
// a: a power of two, what the unit's vector path needs of that pointer
inline bool hsr_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }      // NULL is aligned
