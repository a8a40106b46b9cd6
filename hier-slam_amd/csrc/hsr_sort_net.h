// hsr_sort_net.h — the register bitonic networks of the per-tile sort and the way a lane moves its run of composites, keys and values
// (hsr_sort.hip; tools/micro/sort_net.hip runs every instantiation against std::sort before the library does).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The per-tile sort addresses its arrays through pointers QUALIFIED as global.  On the speculative path they are carved out of an
// integer (hsr_bin_resolve), so hipcc knows no address space for them and every access went out as a FLAT one — and while a FLAT
// access is pending every wait, whatever it is for, waits for everything (the same finding as hsr_render_fwd.hip's list words).
typedef __attribute__((address_space(1))) uint64_t sg_u64;
typedef __attribute__((address_space(1))) uint32_t sg_u32;
typedef uint64_t sn_u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t sn_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t sn_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) sn_u64x2 sg_u64x2;
typedef __attribute__((address_space(1))) sn_u32x2 sg_u32x2;
typedef __attribute__((address_space(1))) sn_u32x4 sg_u32x4;

// How a step whose partner is another lane of the SAME wave (tid ^ m, m < 64) gets the partner's composites:
//   SN_LDS     : two rows of 16 bytes through the exchange buffer, a wave-level fence on either side;
//   SN_BPERMUTE: __shfl_xor per dword (ds_bpermute_b32);
//   SN_SWIZZLE : ds_swizzle_b32 (bit mode, xor mask) for m < 32, v_permlane32_swap for m = 32: no LDS memory, no fence;
//   SN_DPP     : no LDS instruction at all: DPP moves for m < 16 (quad_perm for 1 and 2; row_half_mirror + quad_perm [3,2,1,0] = lane ^ 4;
//                row_mirror + row_half_mirror = lane ^ 8), v_permlane16_swap for 16, v_permlane32_swap for 32;
//   SN_MIX     : DPP quad_perm for m = 1 and 2 (one move per dword), SN_SWIZZLE for the rest.
// The step across waves always goes through the buffer and its two workgroup barriers.  hsr_sort.hip picks the form (TS_XCH) from the
// timings of tools/micro/sort_net.hip; the others stay here so that the comparison can be run again.
enum { SN_LDS = 0, SN_BPERMUTE = 1, SN_SWIZZLE = 2, SN_DPP = 3, SN_MIX = 4 };

template <int CTRL>
__device__ __forceinline__ uint32_t sn_dpp(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}

template <int M>
__device__ __forceinline__ uint32_t sn_swizzle_xor(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1f | (M << 10));
}

template <int XCH>
__device__ __forceinline__ uint32_t sn_partner_dword(uint32_t v, int m, int lane)
{
    if (XCH == SN_BPERMUTE) return (uint32_t)__shfl_xor((int)v, m);
    // DPP controls: quad_perm [1,0,3,2], [2,3,0,1], [3,2,1,0]; row_mirror (lane ^ 15 within 16), row_half_mirror (lane ^ 7 within 8)
    constexpr int QP_1032 = 0xB1, QP_2301 = 0x4E, QP_3210 = 0x1B, ROW_MIRROR = 0x140, ROW_HALF_MIRROR = 0x141;
    if (XCH == SN_DPP || XCH == SN_MIX) {
        switch (m) {
        case 1: return sn_dpp<QP_1032>(v);
        case 2: return sn_dpp<QP_2301>(v);
        default: break;
        }
    }
    if (XCH == SN_DPP) {
        switch (m) {
        case 4: return sn_dpp<QP_3210>(sn_dpp<ROW_HALF_MIRROR>(v));      // lane ^ 7 ^ 3
        case 8: return sn_dpp<ROW_HALF_MIRROR>(sn_dpp<ROW_MIRROR>(v));   // lane ^ 15 ^ 7
        case 16: {
            // old = src = v: the first result holds the even rows of 16 lanes in both rows of a pair, the second the odd rows
            const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
            return (lane & 16) ? r[0] : r[1];
        }
        default: break;   // 32: below
        }
    }
    switch (m) {
    case 1: return sn_swizzle_xor<1>(v);
    case 2: return sn_swizzle_xor<2>(v);
    case 4: return sn_swizzle_xor<4>(v);
    case 8: return sn_swizzle_xor<8>(v);
    case 16: return sn_swizzle_xor<16>(v);
    default: {
        // old = src = v: the first result holds lanes 0..31 of v in both halves, the second lanes 32..63
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return lane < 32 ? r[1] : r[0];
    }
    }
}

// NT threads (2 or 4 waves) sort N = NT * E composites held E per thread; buf: E / 2 rows of NT x 16 bytes.
// Thread tid holds elements E * tid .. E * tid + E - 1; a step with stride j >= E exchanges with thread tid ^ (j / E).
template <int E, int NT, int XCH = SN_LDS>
__device__ __forceinline__ void net_bitonic(uint64_t (&x)[E], int tid, ulonglong2* buf)
{
    constexpr int N = NT * E;
#pragma unroll
    for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j < E) {
                // in registers: one 64-bit compare and four selects per compare-exchange
#pragma unroll
                for (int r = 0; r < E; r++) {
                    if ((r & j) == 0) {
                        const bool up = k < E ? ((r & k) == 0) : (((E * tid) & k) == 0);
                        const uint64_t a = x[r], b = x[r + j];
                        const bool sw = (a > b) == up;
                        x[r] = sw ? b : a;
                        x[r + j] = sw ? a : b;
                    }
                }
            } else {
                const int m = j / E;                   // partner thread = tid ^ m
                const bool cross = m >= 64;            // partner in another wave: one step of the network at two waves, three at four
                const bool keep_min = ((tid & m) == 0) == (((E * tid) & k) == 0);
                // keep_min ? min(a, y) : max(a, y), written as ONE compare: ((a < y) == keep_min) ? a : y.  Exact, because the
                // composites (depth bits, Gaussian index) of a tile are unique, so a != y unless both are pads — and pads are all
                // ~0, where either side is the same value.  (min / max as two ternaries cost two 64-bit compares and three
                // selects per dword: half of the network's vector instructions.)
                if (cross || XCH == SN_LDS) {
#pragma unroll
                    for (int q = 0; q < E / 2; q++) buf[q * NT + tid] = make_ulonglong2(x[2 * q], x[2 * q + 1]);
                    if (cross) {
                        __syncthreads();
                    } else {
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    }
#pragma unroll
                    for (int q = 0; q < E / 2; q++) {
                        const ulonglong2 y = buf[q * NT + (tid ^ m)];
                        const uint64_t a0 = x[2 * q], a1 = x[2 * q + 1];
                        x[2 * q] = ((a0 < y.x) == keep_min) ? a0 : y.x;
                        x[2 * q + 1] = ((a1 < y.y) == keep_min) ? a1 : y.y;
                    }
                    // the next exchange's stores stay behind these loads
                    if (cross) {
                        __syncthreads();
                    } else {
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < E; r++) {
                        const uint64_t a = x[r];
                        const uint32_t ylo = sn_partner_dword<XCH>((uint32_t)a, m, tid & 63);
                        const uint32_t yhi = sn_partner_dword<XCH>((uint32_t)(a >> 32), m, tid & 63);
                        const uint64_t y = ((uint64_t)yhi << 32) | ylo;
                        x[r] = ((a < y) == keep_min) ? a : y;
                    }
                }
            }
        }
    }
}

// A lane's run of E composites, elements e0 .. e0 + E - 1 (e0 = E * tid) of the n the tile holds, from seg = the tile's segment.
// 16-byte loads where the run lies wholly inside the tile and the segment starts on a 16-byte boundary (the arrays are 256-aligned, so
// that is an even first index r0); element by element, pads beyond n, at the ragged end and for odd starts.
template <int E>
__device__ __forceinline__ void sn_load_run(const sg_u64* seg, bool seg_even, int e0, int n, uint64_t (&x)[E])
{
    if (seg_even && e0 + E <= n) {
        const sg_u64x2* p = reinterpret_cast<const sg_u64x2*>(seg + e0);
#pragma unroll
        for (int q = 0; q < E / 2; q++) {
            const sn_u64x2 v = p[q];
            x[2 * q] = v.x;
            x[2 * q + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int r = 0; r < E; r++) x[r] = e0 + r < n ? seg[e0 + r] : ~0ull;
    }
}

// The sorted run back as the reference's pairs: key = tile | depth bits, value = Gaussian index.  Keys in 16-byte stores under the
// same condition as the loads; values in 16-byte stores when the run's first value is 16-byte aligned too (8-byte ones at E = 2).
template <int E>
__device__ __forceinline__ void sn_store_run(sg_u64* kseg, sg_u32* vseg, int r0, int e0, int n, uint64_t tile_hi, const uint64_t (&x)[E])
{
    const bool whole = e0 + E <= n;
    if (whole && (r0 & 1) == 0) {
        sg_u64x2* p = reinterpret_cast<sg_u64x2*>(kseg + e0);
#pragma unroll
        for (int q = 0; q < E / 2; q++) {
            sn_u64x2 v;
            v.x = tile_hi | (x[2 * q] >> 32);
            v.y = tile_hi | (x[2 * q + 1] >> 32);
            p[q] = v;
        }
    } else {
#pragma unroll
        for (int r = 0; r < E; r++)
            if (e0 + r < n) kseg[e0 + r] = tile_hi | (x[r] >> 32);
    }
    constexpr int VA = E >= 4 ? 4 : 2;   // values per store
    if (whole && ((r0 + e0) & (VA - 1)) == 0) {
        if constexpr (E >= 4) {
            sg_u32x4* p = reinterpret_cast<sg_u32x4*>(vseg + e0);
#pragma unroll
            for (int q = 0; q < E / 4; q++) {
                sn_u32x4 v;
                v.x = (uint32_t)x[4 * q];
                v.y = (uint32_t)x[4 * q + 1];
                v.z = (uint32_t)x[4 * q + 2];
                v.w = (uint32_t)x[4 * q + 3];
                p[q] = v;
            }
        } else {
            sn_u32x2 v;
            v.x = (uint32_t)x[0];
            v.y = (uint32_t)x[1];
            *reinterpret_cast<sg_u32x2*>(vseg + e0) = v;
        }
    } else {
#pragma unroll
        for (int r = 0; r < E; r++)
            if (e0 + r < n) vseg[e0 + r] = (uint32_t)x[r];
    }
}
