// hsr_bwd_tile.h — what the two matrix-core backward tile kernels (hsr_render_bwd_q.hip, hsr_render_bwd_sub.hip) share around their
// visit loops and flushes.  Inlined code and text only: no kernel, no LDS of its own.
#pragma once
#include "hsr_tile_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// orders the LDS accesses of ONE wave (stores before it are visible to the wave's loads after it); no workgroup barrier
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the MFMA B operand: G transposed through LDS ----
// Lane l brings 16 channels gv[0..15] of its pixel and leaves with B[m] = G[pixel lane 4m + (l>>4)][channel l&15], m = 0..15.  The panel
// (64 x 17 words) is private to the wave: a wave-level fence orders its LDS stores and loads, the four waves do not have to meet (they
// would wait for the slowest wave's 30-odd global loads twice per channel group).  A macro for the reason given below.
#define HSR_BWD_TRANSPOSE_B(panel, lane, gv, B)                                                                                            \
    _Pragma("unroll") for (int c = 0; c < 16; c++) panel[lane * 17 + c] = gv[c];                                                          \
    wave_lds_fence();                                                                                                                      \
    _Pragma("unroll") for (int m = 0; m < 16; m++) B[m] = panel[(4 * m + (lane >> 4)) * 17 + (lane & 15)];                                \
    wave_lds_fence()

// ---- software-pipelined staging of a batch's splats ----
// Thread t holds, in registers, the splat it will stage in the NEXT batch (the inputs of its 48-byte record and its sub-block mask) and
// the id of the one after that: each was requested a whole batch of blending before it is used, and is waited for once, at the top of
// the batch that stages it (HSR_SETTLE_STAGING).
//
// These are macros, not functions: the two kernels sit at a register step, and hipcc schedules and allocates them differently as soon as
// any of this text is reached through a call — even a force-inlined one, even a bare struct of these registers (the early
// simplification passes see the kernel before the callee is inlined).  Expanded in place, both kernels compile to the instructions
// they had when each carried its own copy.  The macros use the kernel's `a` (RenderBwdArgs), `range` (the tile's list) and `t`.
//
// HSR_BWD_STAGING_DECLARE(): the registers and their loaders.  The loads are unconditional and clamped, and the id of the batch after
// next is requested before the next batch's records: see render_fwd_kernel (a load inside a divergent `if`, or into a register the
// loads before it took their addresses from, is waited for where it is issued — and the (rec == NULL) fallback kept three of these
// values in a scratch slot).  a.rec is never NULL.  fetch_mask: the forward's staging phase left the 16-bit sub-block mask of every
// list entry it staged in a.masks (the backward stages a subset of those entries: it stops at the tile's largest n_contrib): one 4-byte
// load per entry instead of ~460 instructions of subblock_mask.
#define HSR_BWD_STAGING_DECLARE()                                                                                                          \
    int id_next = 0, id_cur = 0;                                                                                                           \
    float2 p_xy = {0, 0};                                                                                                                  \
    float4 p_co = {0, 0, 0, 0};                                                                                                            \
    float p_r = 0, p_g = 0, p_b = 0, p_d = 0;                                                                                              \
    uint32_t p_mask = 0u;                                                                                                                  \
    const int n_list = (int)(range.y - range.x);                                                                                           \
    auto fetch_id = [&](int hi) -> int { return (int)a.point_list[range.x + min(max(hi - 1 - t, 0), max(n_list - 1, 0))]; };               \
    auto fetch_mask = [&](int hi) -> uint32_t { return a.masks[range.x + min(max(hi - 1 - t, 0), max(n_list - 1, 0))]; };                  \
    auto load_record = [&](int id_of) {                                                                                                    \
        const size_t id = (size_t)id_of;                                                                                                   \
        id_cur = id_of;                                                                                                                    \
        const float4* rec = a.rec + 4 * id;                                                                                                \
        const float4 r0 = rec[0], r2 = rec[2];                                                                                             \
        p_co = rec[1];                                                                                                                     \
        p_xy = make_float2(r0.x, r0.y);                                                                                                    \
        p_d = r0.z;                                                                                                                        \
        p_r = r2.x; p_g = r2.y; p_b = r2.z;                                                                                                \
    }
// before the first batch, which ends at list position hi_all
#define HSR_BWD_STAGING_PRIME(hi_all, BATCH)                                                                                               \
    if (n_list > 0) {                                                                                                                      \
        const int id0 = fetch_id(hi_all);                                                                                                  \
        id_next = fetch_id(hi_all - BATCH);                                                                                                \
        load_record(id0);                                                                                                                  \
        p_mask = fetch_mask(hi_all);                                                                                                       \
    }
// after the second barrier of the batch that ends at hi: its records are in LDS, the registers take the next batch's (its ids were
// requested a whole batch ago)
#define HSR_BWD_STAGING_ADVANCE(hi, BATCH)                                                                                                 \
    {                                                                                                                                      \
        int id_use = id_next;                                                                                                              \
        asm volatile("" : "+v"(id_use));                                                                                                   \
        id_next = fetch_id(hi - 2 * BATCH);                                                                                                \
        load_record(id_use);                                                                                                               \
        p_mask = fetch_mask(hi - BATCH);                                                                                                   \
    }
// the 48-byte staged record { x, y, A', B' | r, g, b, depth | C', opacity, B'/2, - } into s_ent[i .. i + 2]: ONE address computation per visit
#define HSR_BWD_STORE_RECORD(s_ent, i)                                                                                                     \
    s_ent[(i)] = make_float4(p_xy.x, p_xy.y, (-0.5f * HSR_LOG2E) * p_co.x, -HSR_LOG2E * p_co.y);                                             \
    s_ent[(i) + 1] = make_float4(p_r, p_g, p_b, p_d);                                                                                        \
    s_ent[(i) + 2] = make_float4((-0.5f * HSR_LOG2E) * p_co.z, p_co.w, (-0.5f * HSR_LOG2E) * p_co.y, 0.f)
// Makes the staging registers "used": hipcc waits for their loads where this stands.  It stands ONCE per batch, right behind the batch's
// top barrier and in front of everything that issues an atomic there (loads, stores and atomics retire through one in-order counter:
// a wait placed behind fresh atomics sits them out too).  What the wait does cover is the wave's own last flush of the batch before,
// whose atomics have had the barrier to retire in.
// It used to stand inside the chunk loop, in front of the first flush, so that the wait would cover no atomic at all.  hipcc does not
// leave it there: a loop that holds atomics but no loads and uses a register whose load is pending gets the counter flushed in its
// PREHEADER (the waitcnt pass's rule for such loops), i.e. every wave waited for the gathers a few dozen instructions after it had
// requested them, once per batch, and blended nothing meanwhile.  Hence no staging register may be touched between
// HSR_BWD_STAGING_ADVANCE and the next batch's top barrier — not by a copy either, which is why ADVANCE hands the id over through an
// opaque copy: without it the register allocator rotates id_next with a move at the head of the batch loop, in front of the barrier,
// and that move waits for all but the last four atomics of the batch.
#define HSR_SETTLE_STAGING()                                                                                                   \
    asm volatile("" ::"v"(id_next), "v"(p_xy.x), "v"(p_xy.y), "v"(p_co.x), "v"(p_co.y), "v"(p_co.z), "v"(p_co.w), "v"(p_r), "v"(p_g), \
                 "v"(p_b), "v"(p_d), "v"(p_mask))

// wave-uniform iteration count of a chunk: the longest of the four groups' visit lists, from the ballot of (row, group) touches
// (readfirstlane: the loop counter then lives in a scalar register, not in a VALU down-counter)
__device__ __forceinline__ int longest_group_list(uint64_t ball)
{
    return __builtin_amdgcn_readfirstlane(max(max(__popc((uint32_t)ball & 0xFFFFu), __popc((uint32_t)(ball >> 16) & 0xFFFFu)),
                                              max(__popc((uint32_t)(ball >> 32) & 0xFFFFu), __popc((uint32_t)(ball >> 48)))));
}
