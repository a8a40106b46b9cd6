// hsr_map_export.hip — device export of the Gaussian map as the body of a PLY file: packed 68-byte (SH) or 59-byte (RGB8) records, the
// RGB8 colour given, looked up per class label or looked up per tree tuple of the per-level labels, all in one launch (gfx950),
// DESIGN.md §7 row 10.  See include/ext/hsr_map_export.h for the rules, step by step, and the reference lines
// (scripts/export_ply_semantic_tree.py:201-382).
//   map_export_kernel<REC, WIDE> : a workgroup of MB = 256 lanes takes MB consecutive Gaussians (128 or 64 where the logit rows are long,
//       below).  The kernel moves bytes; its one arithmetic expression is f_dc = (rgb - 0.5f) / C0f.
//       in   each map array's span of the workgroup is contiguous ([256,3] floats = 3072 bytes, ...): it is read FLAT, lane t taking the
//            16 bytes at 16 t (WIDE) or the dwords at 4 t, 4 (t + MB), .. (narrow), and each dword is scattered to its record in LDS —
//            never one row per lane, which for 12-byte rows is three strided dword loads.  The loads of all arrays and of the wave's
//            logit rows are issued before the first is used: a workgroup waits for memory once, not once per array.
//       tree the [P,K] logits are the largest input.  A wave stages the contiguous span of its 64 rows (64 K floats, 16 bytes per lane,
//            sixteen loads in flight) into LDS rows of pitch K | 1 dwords: odd, so that lane r reading its own row r * pitch + c hits
//            bank (r * pitch + c) % 32, distinct over the 32 lanes of a half wave.  Every lane then runs the passes of the label rule
//            (hsr_tree.h's hsr_softmax_argmax) on its row in LDS.  A SIMD spends four cycles on a wave's instruction however few lanes are live,
//            so the rows are never dealt to fewer lanes: the workgroup shrinks instead, to the most of 4, 2 and 1 waves
//            whose records and 64 rows each fit in 64 KB (beside 59-byte records K <= 48, K <= 112 — K = 102 runs two waves — and
//            K <= 240).  Longer rows are not staged: each lane reads its own from global memory, a run of 964 bytes or more.
//       out  the records are assembled in LDS at their packed offsets (59-byte records put floats at odd addresses: the LDS takes
//            unaligned dword stores) and the workgroup's MB * stride contiguous bytes, a multiple of 16, leave as 16-byte stores
//            (WIDE) or 1-byte stores (narrow); the last workgroup writes cnt * stride bytes, the last P * stride % 16 of them singly.
// WIDE is chosen on the host: `out` and every array the call reads 16-byte aligned (every span starts at a multiple of 64 Gaussians, and
// so on 16 bytes).  No scratch, no atomics.
// Compiled with -ffp-contract=off: no rule of the header has a fused multiply-add.
#include <math.h>

#include "hsr_common.h"
#include "hsr_tree.h"
#include "../../include/hsr_eval.h"
#include "../../include/ext/hsr_map_export.h"

namespace {

constexpr int LDS_BYTES = 65536;      // the most a workgroup takes
constexpr int STAGE_LOADS = 16;       // loads a lane has in flight while staging rows
constexpr float C0F = (float)0.28209479177387814;

typedef unsigned u4 __attribute__((ext_vector_type(4)));

template <int REC> struct Layout;
template <> struct Layout<HSR_MAP_RECORD_SH> { static constexpr int STRIDE = 68, COLOUR = 24, OPACITY = 36, SCALE = 40, ROT = 52; };
template <> struct Layout<HSR_MAP_RECORD_RGB8> { static constexpr int STRIDE = 59, COLOUR = 24, OPACITY = 27, SCALE = 31, ROT = 43; };
template <> struct Layout<HSR_MAP_RECORD_NONE> { static constexpr int STRIDE = 0, COLOUR = 0, OPACITY = 0, SCALE = 0, ROT = 0; };

// one dword into the records at byte `off`: aligned in 68-byte records, at any byte in 59-byte ones
template <int REC> __device__ __forceinline__ void put32(unsigned char* rec, unsigned off, unsigned v)
{
    if (REC == HSR_MAP_RECORD_SH)
        *reinterpret_cast<unsigned*>(rec + off) = v;
    else
        __builtin_memcpy(rec + off, &v, 4);
}

// A lane's share of the workgroup's span of n <= 4 * MB dwords at src, every dword loaded once.  Two steps, so that a kernel can issue
// the loads of all its spans before it uses the first: fetch() loads, scatter() hands f(e, bits) every element e the lane holds.
// WIDE: the 16 bytes at 16 t, and for t < n % 4 one of the last dwords; narrow: the dwords t, t + MB, t + 2 MB, t + 3 MB.
struct Fetched {
    u4 q;
    unsigned tail;
};

template <bool WIDE> __device__ __forceinline__ Fetched fetch(const void* __restrict__ src_, unsigned n, unsigned t, unsigned MB)
{
    const unsigned* __restrict__ src = static_cast<const unsigned*>(src_);
    Fetched d = {};
    if (WIDE) {
        const unsigned n4 = n >> 2;
        if (t < n4) d.q = reinterpret_cast<const u4*>(src)[t];
        if (4 * n4 + t < n) d.tail = src[4 * n4 + t];
    } else {
        if (t < n) d.q.x = src[t];
        if (t + MB < n) d.q.y = src[t + MB];
        if (t + 2 * MB < n) d.q.z = src[t + 2 * MB];
        if (t + 3 * MB < n) d.q.w = src[t + 3 * MB];
    }
    return d;
}

template <bool WIDE, class F> __device__ __forceinline__ void scatter(const Fetched& d, unsigned n, unsigned t, unsigned MB, F f)
{
    if (WIDE) {
        const unsigned n4 = n >> 2;
        if (t < n4) { f(4 * t, d.q.x); f(4 * t + 1, d.q.y); f(4 * t + 2, d.q.z); f(4 * t + 3, d.q.w); }
        if (4 * n4 + t < n) f(4 * n4 + t, d.tail);
    } else {
        if (t < n) f(t, d.q.x);
        if (t + MB < n) f(t + MB, d.q.y);
        if (t + 2 * MB < n) f(t + 2 * MB, d.q.z);
        if (t + 3 * MB < n) f(t + 3 * MB, d.q.w);
    }
}

// the per-level labels of Gaussian g (its logits behind `at`), out_labels, and the tuple's colour into record `local`
template <int REC, class At>
__device__ __forceinline__ void tree_gaussian(const hsr_map_export_job& job, At at, int g, int local, unsigned char* rec)
{
    int idx = 0, begin = 0;
    for (int l = 0; l < job.L; l++) {
        const int size = job.sizes[l];      // a wave-uniform index into the kernel arguments: scalar loads, no scratch
        const int lab = hsr_softmax_argmax([&](int i) { return at(begin + i); }, size);
        if (job.out_labels) job.out_labels[(size_t)l * job.P + g] = lab;
        idx = idx * size + lab;
        begin += size;
    }
    if (REC == HSR_MAP_RECORD_RGB8) {
        const uint8_t* __restrict__ row = job.table + 3 * (size_t)idx;
        unsigned char* c = rec + local * Layout<REC>::STRIDE + Layout<REC>::COLOUR;
        c[0] = row[0]; c[1] = row[1]; c[2] = row[2];
    }
}

// a wave stages n dwords at src (whole rows of K) into buf, rows of `pitch` dwords; V dwords per lane and load, STAGE_LOADS loads in
// flight.  A lane keeps the (row, column) of its next element and steps it by the 64 V elements between two of its loads: one
// division per call, none per element.
template <int V> __device__ __forceinline__ void stage_rows(const unsigned* __restrict__ src, unsigned n, unsigned K, unsigned pitch,
                                                            unsigned* buf, unsigned lane)
{
    constexpr unsigned STEP = 64 * V;      // elements a wave takes per load
    const unsigned nv = n / V;
    const unsigned dr = STEP / K, dc = STEP - dr * K;
    unsigned row = (V * lane) / K, col = V * lane - row * K;
    for (unsigned i = lane; i < nv; i += STAGE_LOADS * 64) {
        unsigned v[STAGE_LOADS][V];
#pragma unroll
        for (int u = 0; u < STAGE_LOADS; u++) {
            if (i + 64 * u < nv) {
                if constexpr (V == 4) {
                    const u4 q = reinterpret_cast<const u4*>(src)[i + 64 * u];
                    v[u][0] = q.x; v[u][1] = q.y; v[u][2] = q.z; v[u][3] = q.w;
                } else {
                    v[u][0] = src[i + 64 * u];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < STAGE_LOADS; u++) {
            if (i + 64 * u < nv) {
                unsigned rr = row, cc = col;
#pragma unroll
                for (int k = 0; k < V; k++) {
                    buf[rr * pitch + cc] = v[u][k];
                    if (++cc == K) { cc = 0; rr++; }
                }
            }
            col += dc; row += dr;
            if (col >= K) { col -= K; row++; }
        }
    }
    for (unsigned e = V * nv + lane; e < n; e += 64) {      // V = 4: the last n % 4 dwords
        const unsigned r = e / K;
        buf[r * pitch + (e - r * K)] = src[e];
    }
}

// blockDim.x = MB = 256, 128 or 64: the Gaussians of a workgroup, one per lane
template <int REC, bool WIDE>
__global__ __launch_bounds__(256) void map_export_kernel(hsr_map_export_job job, int pitch)      // pitch 0: rows not staged
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    using Lay = Layout<REC>;
    constexpr int STRIDE = Lay::STRIDE;
    const unsigned t = threadIdx.x, MB = blockDim.x, lane = t & 63, w = t >> 6;
    const int g0 = blockIdx.x * MB;
    const int cnt = min((int)MB, job.P - g0);      // >= 1: the grid is ceil(P / MB)
    const unsigned n1 = cnt, n3 = cnt * 3, n4 = cnt * 4;
    unsigned char* rec = lds;
    const bool tree = REC == HSR_MAP_RECORD_NONE || (REC == HSR_MAP_RECORD_RGB8 && job.colour == HSR_MAP_COLOUR_TREE);
    const unsigned K = (unsigned)job.K;
    unsigned* buf = reinterpret_cast<unsigned*>(lds + MB * STRIDE) + w * (unsigned)(64 * pitch);      // this wave's staged rows
    const int row0 = g0 + 64 * (int)w;                 // the wave's first Gaussian
    const int rows = min(64, job.P - row0);            // those of its 64 the map has: may be <= 0 in the last workgroup

    // every load of the map arrays first, then the wave's rows of logits, then the uses: one round trip to memory, not one per array
    Fetched means = {}, normals = {}, opacity = {}, scales = {}, rot = {}, rgb = {};
    unsigned given_word = 0, given_byte[3] = {0, 0, 0};
    int label = -1;
    if (REC != HSR_MAP_RECORD_NONE) {
        means = fetch<WIDE>(job.means3D + (size_t)g0 * 3, n3, t, MB);
        if (job.normals) normals = fetch<WIDE>(job.normals + (size_t)g0 * 3, n3, t, MB);
        opacity = fetch<WIDE>(job.logit_opacities + g0, n1, t, MB);
        scales = job.S == 1 ? fetch<WIDE>(job.log_scales + g0, n1, t, MB) : fetch<WIDE>(job.log_scales + (size_t)g0 * 3, n3, t, MB);
        rot = fetch<WIDE>(job.unnorm_rotations + (size_t)g0 * 4, n4, t, MB);
        if (REC == HSR_MAP_RECORD_SH) {
            rgb = fetch<WIDE>(job.rgb_colors + (size_t)g0 * 3, n3, t, MB);
        } else if (job.colour == HSR_MAP_COLOUR_GIVEN) {      // n3 bytes: WIDE, the dword at 4 t and one of the last n3 % 4 bytes
            const uint8_t* __restrict__ src = job.colours + (size_t)g0 * 3;
            if (WIDE) {
                if (t < n3 >> 2) given_word = reinterpret_cast<const unsigned*>(src)[t];
                if ((n3 & ~3u) + t < n3) given_byte[0] = src[(n3 & ~3u) + t];
            } else {
#pragma unroll
                for (int k = 0; k < 3; k++)
                    if (t + k * MB < n3) given_byte[k] = src[t + k * MB];
            }
        } else if (job.colour == HSR_MAP_COLOUR_LABELS) {
            if ((int)t < cnt) label = job.labels[g0 + t];
        }
    }
    if (tree && pitch > 0 && rows > 0)
        stage_rows<WIDE ? 4 : 1>(reinterpret_cast<const unsigned*>(job.semantic) + (size_t)row0 * K, (unsigned)rows * K, K, (unsigned)pitch, buf,
                                 lane);

    if (REC != HSR_MAP_RECORD_NONE) {
        scatter<WIDE>(means, n3, t, MB, [&](unsigned e, unsigned v) {
            const unsigned g = e / 3;
            put32<REC>(rec, g * STRIDE + 4 * (e - 3 * g), v);
        });
        if (job.normals) {
            scatter<WIDE>(normals, n3, t, MB, [&](unsigned e, unsigned v) {
                const unsigned g = e / 3;
                put32<REC>(rec, g * STRIDE + 12 + 4 * (e - 3 * g), v);
            });
        } else if ((int)t < cnt) {
            put32<REC>(rec, t * STRIDE + 12, 0u); put32<REC>(rec, t * STRIDE + 16, 0u); put32<REC>(rec, t * STRIDE + 20, 0u);
        }
        scatter<WIDE>(opacity, n1, t, MB, [&](unsigned e, unsigned v) { put32<REC>(rec, e * STRIDE + Lay::OPACITY, v); });
        if (job.S == 1) {
            scatter<WIDE>(scales, n1, t, MB, [&](unsigned e, unsigned v) {
                put32<REC>(rec, e * STRIDE + Lay::SCALE, v); put32<REC>(rec, e * STRIDE + Lay::SCALE + 4, v);
                put32<REC>(rec, e * STRIDE + Lay::SCALE + 8, v);
            });
        } else {
            scatter<WIDE>(scales, n3, t, MB, [&](unsigned e, unsigned v) {
                const unsigned g = e / 3;
                put32<REC>(rec, g * STRIDE + Lay::SCALE + 4 * (e - 3 * g), v);
            });
        }
        scatter<WIDE>(rot, n4, t, MB, [&](unsigned e, unsigned v) { put32<REC>(rec, (e >> 2) * STRIDE + Lay::ROT + 4 * (e & 3), v); });
        if (REC == HSR_MAP_RECORD_SH) {
            scatter<WIDE>(rgb, n3, t, MB, [&](unsigned e, unsigned v) {
                const unsigned g = e / 3;
                const float f_dc = (__uint_as_float(v) - 0.5f) / C0F;
                put32<REC>(rec, g * STRIDE + Lay::COLOUR + 4 * (e - 3 * g), __float_as_uint(f_dc));
            });
        } else if (job.colour == HSR_MAP_COLOUR_GIVEN) {
            auto put = [&](unsigned e, unsigned byte) {
                const unsigned g = e / 3;
                rec[g * STRIDE + Lay::COLOUR + (e - 3 * g)] = (unsigned char)byte;
            };
            if (WIDE) {
                if (t < n3 >> 2) {
                    put(4 * t, given_word & 255u); put(4 * t + 1, (given_word >> 8) & 255u); put(4 * t + 2, (given_word >> 16) & 255u);
                    put(4 * t + 3, given_word >> 24);
                }
                if ((n3 & ~3u) + t < n3) put((n3 & ~3u) + t, given_byte[0]);
            } else {
#pragma unroll
                for (int k = 0; k < 3; k++)
                    if (t + k * MB < n3) put(t + k * MB, given_byte[k]);
            }
        } else if (job.colour == HSR_MAP_COLOUR_LABELS) {
            if ((int)t < cnt) {
                unsigned r = 0, g = 0, b = 0;
                if (label >= 0 && label < job.n) {
                    const uint8_t* __restrict__ row = job.table + 3 * (size_t)label;
                    r = row[0]; g = row[1]; b = row[2];
                }
                unsigned char* c = rec + t * STRIDE + Lay::COLOUR;
                c[0] = (unsigned char)r; c[1] = (unsigned char)g; c[2] = (unsigned char)b;
            }
        }
    }

    if (tree) {
        if (pitch > 0) {
            __syncthreads();
            if ((int)lane < rows) {
                const float* __restrict__ x = reinterpret_cast<const float*>(buf) + lane * (unsigned)pitch;
                tree_gaussian<REC>(job, [&](int i) { return x[i]; }, row0 + (int)lane, (int)t, rec);
            }
        } else if ((int)t < cnt) {      // rows too long to stage: each lane reads its own
            const float* __restrict__ x = job.semantic + (size_t)(g0 + t) * K;
            tree_gaussian<REC>(job, [&](int i) { return x[i]; }, g0 + (int)t, (int)t, rec);
        }
    }

    if (REC != HSR_MAP_RECORD_NONE) {
        __syncthreads();
        const unsigned bytes = (unsigned)cnt * STRIDE;
        unsigned char* __restrict__ dst = job.out + (size_t)g0 * STRIDE;
        unsigned done = 0;
        if (WIDE) {
            done = bytes & ~15u;
            for (unsigned i = t; i < bytes >> 4; i += MB) reinterpret_cast<u4*>(dst)[i] = reinterpret_cast<const u4*>(rec)[i];
        }
        for (unsigned b = done + t; b < bytes; b += MB) dst[b] = rec[b];
    }
}

template <int REC>
int launch(const hsr_map_export_job& job, bool wide, int waves, int pitch, size_t lds, hipStream_t stream)
{
    const int MB = 64 * waves;
    const unsigned grid = (unsigned)((job.P + MB - 1) / MB);
    if (wide)
        map_export_kernel<REC, true><<<grid, MB, lds, stream>>>(job, pitch);
    else
        map_export_kernel<REC, false><<<grid, MB, lds, stream>>>(job, pitch);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int hsr_map_export(const hsr_map_export_job* job_, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!job_) {
        hsr_set_error("map_export: job is NULL");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const hsr_map_export_job& j = *job_;
    if (j.P < 0 || j.P > HSR_MAP_EXPORT_MAX_P) {
        hsr_set_error("map_export: P must be 0..%d; got %d", HSR_MAP_EXPORT_MAX_P, j.P);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (j.record < HSR_MAP_RECORD_SH || j.record > HSR_MAP_RECORD_NONE) {
        hsr_set_error("map_export: unknown record %d", j.record);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const bool records = j.record != HSR_MAP_RECORD_NONE;
    bool tree = !records;
    bool wide = true;
    const bool empty = j.P == 0;      // the pointers of empty arrays may be NULL
    if (!records && !j.out_labels && !empty) {
        hsr_set_error("map_export: record NONE without out_labels");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (records) {
        if (j.S != 1 && j.S != 3) {
            hsr_set_error("map_export: S must be 1 or 3; got %d", j.S);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        if (!empty && (!j.means3D || !j.unnorm_rotations || !j.logit_opacities || !j.log_scales || !j.out ||
                       (j.record == HSR_MAP_RECORD_SH && !j.rgb_colors))) {
            hsr_set_error("map_export: record %d: NULL means3D, rgb_colors, unnorm_rotations, logit_opacities, log_scales or out", j.record);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        wide = aligned16(j.means3D) && aligned16(j.unnorm_rotations) && aligned16(j.logit_opacities) && aligned16(j.log_scales) &&
               aligned16(j.normals) && aligned16(j.out) && (j.record != HSR_MAP_RECORD_SH || aligned16(j.rgb_colors));
    }
    if (j.record == HSR_MAP_RECORD_RGB8) {
        if (j.colour < HSR_MAP_COLOUR_GIVEN || j.colour > HSR_MAP_COLOUR_TREE) {
            hsr_set_error("map_export: unknown colour %d", j.colour);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        tree = j.colour == HSR_MAP_COLOUR_TREE;
        if (j.colour == HSR_MAP_COLOUR_GIVEN) {
            if (!j.colours && !empty) {
                hsr_set_error("map_export: colour GIVEN: NULL colours");
                return HSR_ERR_INVALID_ARGUMENT;
            }
            wide = wide && aligned16(j.colours);
        } else {
            if ((j.colour == HSR_MAP_COLOUR_LABELS && !j.labels && !empty) || !j.table) {
                hsr_set_error("map_export: colour %d: NULL labels or table", j.colour);
                return HSR_ERR_INVALID_ARGUMENT;
            }
            if (j.n < 1) {
                hsr_set_error("map_export: a table of %d rows; it takes at least 1", j.n);
                return HSR_ERR_INVALID_ARGUMENT;
            }
        }
    }
    if (tree) {
        if (!j.semantic && !empty) {
            hsr_set_error("map_export: the tree labels need semantic; it is NULL");
            return HSR_ERR_INVALID_ARGUMENT;
        }
        if (j.L < 1 || j.L > HSR_EVAL_MAX_LEVELS) {
            hsr_set_error("map_export: L must be 1..%d; got %d", HSR_EVAL_MAX_LEVELS, j.L);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        const hsr_tree_extent e = hsr_parse_tree_levels(j.L, j.sizes, nullptr);
        if (e.bad_level >= 0) {
            hsr_set_error("map_export: level %d has %d classes", e.bad_level, j.sizes[e.bad_level]);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        if (e.sum > j.K) {
            hsr_set_error("map_export: the levels need %lld columns, K is %d", e.sum, j.K);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        if (records && e.prod != j.n) {
            hsr_set_error("map_export: the levels need a table of %lld rows, n is %d", e.prod, j.n);
            return HSR_ERR_INVALID_ARGUMENT;
        }
        wide = wide && aligned16(j.semantic);
    }
    if (empty) return HSR_OK;

    // The workgroup: 4, 2 or 1 waves of 64 Gaussians, the most whose records and 64 staged rows each fit in 64 KB together, so that every
    // lane has a row (K <= 48 / 112 / 240 beside 59-byte records).  Longer rows are not staged (pitch 0).
    const int stride = j.record == HSR_MAP_RECORD_SH ? 68 : j.record == HSR_MAP_RECORD_RGB8 ? 59 : 0;
    int waves = 4, pitch = 0;
    if (tree) {
        pitch = j.K | 1;
        const size_t per_wave = (size_t)64 * stride + (size_t)256 * pitch;
        if (per_wave > LDS_BYTES)
            pitch = 0;
        else if (per_wave * 4 > LDS_BYTES)
            waves = per_wave * 2 <= LDS_BYTES ? 2 : 1;
    }
    const size_t lds = (size_t)waves * (64 * stride + (size_t)256 * pitch);
    if (j.record == HSR_MAP_RECORD_SH) return launch<HSR_MAP_RECORD_SH>(j, wide, waves, pitch, lds, stream);
    if (j.record == HSR_MAP_RECORD_RGB8) return launch<HSR_MAP_RECORD_RGB8>(j, wide, waves, pitch, lds, stream);
    return launch<HSR_MAP_RECORD_NONE>(j, wide, waves, pitch, lds, stream);
}
