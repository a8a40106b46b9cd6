// hsr_mesh_clean.hip — the connected components of a triangle mesh and the removal of some of them (gfx950):
// include/surface/hsr_mesh_clean.h states the rules, and the rules alone define the results; this file only divides the work.  Integer
// work only: there is no floating-point operation here, so the file needs no -ffp-contract=off (csrc/Makefile).
//
// Components, four launches on the stream and no host read in between:
//   init    : init_kernel — parent[v] = v, count[v] = 0; out_label IS the parent array.
//   hook    : hook_kernel — a face per lane; a valid face unites (a, b) and (b, c).  unite() finds both roots and links the LARGER under
//             the smaller with one compare-and-swap on the larger root's own slot, so parent[x] <= x always and a finished component's
//             root is its smallest index.  One pass over the edges suffices (ECL-CC; Jayanti and Tarjan): there is no outer loop.
//             EVERY access to parent[] in this launch is a relaxed agent-scope atomic (ld / st / cas below): the eight XCDs have private
//             L2s and every CU its own L1, and a plain load could return a stale parent[x] == x for ever.  After a compare-and-swap that
//             another lane won, the walk continues from the value it returned (never a re-read), so each retry strictly descends.  find()
//             writes parent[x] = parent[parent[x]] on its way (path splitting: one extra store a step, no extra load); the value
//             written is an ancestor of x, which keeps both invariants.  Vertices sorted by edge key make long chains: without the
//             store the four launches took 2.02 ms instead of 1.23 ms on the 1.17 M-face room (EXPERIMENTS.md §23).
//   flatten : flatten_kernel — a vertex per lane: label[v] = root(v), in place.  Lanes of this launch read slots that other lanes of
//             it write, so the accesses stay relaxed atomics; whichever value a read returns, the old parent or the root, is an
//             ancestor, and the root's own slot never changes: the result does not depend on the interleaving.
//   count   : count_kernel — a face per lane: count[label[a]] += 1, the lanes of a wave that share a label adding once.  This is a
//             launch of its own because it reads label[a] of ANOTHER lane's vertex: in one launch with the flatten it could read a
//             slot before its lane had flattened it and count the face at an inner node.  The two-launch split costs no scratch, where
//             a second label array would (the entry point takes none).
// The belt: every walk counts its steps against a cap derived from V that cannot be reached while parent[x] <= x holds (each step
// strictly descends); a lane that reaches it stores -1 to count[] and stops, and count_kernel adds nothing to a negative entry (the
// header's gave_up rule).  No lane waits for another workgroup's progress and nothing spins.
//
// Select, an order-preserving compaction in three phases (hsr_block.h), six launches behind one memset of the marks:
//   face_count_kernel (kept faces per block; marks the vertices they use) -> vertex_count_kernel (marked vertices per block) ->
//   scan_kernel (ONE workgroup: both lists of counts to exclusive offsets, the totals to out_counts) -> vertex_scatter_kernel
//   (out_source, and the mark of a kept vertex becomes its new index) -> face_scatter_kernel (out_faces through the new indices).
// No workgroup polls another.  Every loop bound can be read here: none but the scan's ceil(n / 1024) trips and the wave loop of
// count_kernel (at most 64 trips: each retires a lane).
#include "hsr_common.h"
#include "hsr_block.h"
#include "../../include/surface/hsr_mesh_clean.h"

namespace {

constexpr int TB = HSR_MESH_CLEAN_BLOCK;      // one item a lane: a block of the compaction is a workgroup
static_assert(TB == 256, "hsr_block256_count and hsr_block_rank<4> below are for 256 threads");

typedef unsigned long long u64;

__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the value the slot held: `expect` when the exchange was made
__device__ __forceinline__ int cas(int* p, int expect, int desired)
{
    __hip_atomic_compare_exchange_strong(p, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;
}

__device__ __forceinline__ bool valid_face(int V, int a, int b, int c)
{
    return (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V;
}

// the root above x.  Every trip moves to a strictly smaller index (parent[x] <= x, and p != x here), so there are at most x trips;
// `steps` counts them against `cap`, and false means the cap was reached (never, while the invariant holds).
__device__ __forceinline__ bool find(int* parent, int& x, u64& steps, u64 cap)
{
    int p = ld(parent + x);
    while (p != x) {
        if (++steps > cap) return false;
        const int g = ld(parent + p);
        if (g != p) st(parent + x, g);      // an ancestor of x, and <= p <= x
        x = p;
        p = g;
    }
    return true;
}

// false: gave up
__device__ __forceinline__ bool unite(int* parent, int a, int b, u64 cap)
{
    u64 steps = 0;
    if (!find(parent, a, steps, cap) || !find(parent, b, steps, cap)) return false;
    while (a != b) {
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = cas(parent + hi, hi, lo);
        if (old == hi) break;      // linked: hi was a root and now hangs under lo < hi
        // another lane linked hi first, under old < hi: go on from there.  lo may have stopped being a root as well; then it is the
        // larger side of a later trip and its own compare-and-swap says so.  Either way max(a, b) has strictly decreased.
        if (++steps > cap) return false;
        a = old;
        b = lo;
        if (!find(parent, a, steps, cap)) return false;
    }
    return true;
}

__global__ __launch_bounds__(TB) void init_kernel(int V, int* __restrict__ parent, int* __restrict__ count)
{
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    if (i >= (long long)V) return;
    parent[i] = (int)i;
    count[i] = 0;
}

__global__ __launch_bounds__(TB) void hook_kernel(int V, int F, const int* __restrict__ faces, int* parent, int* count)
{
    const long long f = (long long)blockIdx.x * TB + threadIdx.x;
    if (f >= (long long)F) return;
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    if (!valid_face(V, a, b, c)) return;
    const u64 cap = 2ull * (u64)V + HSR_MESH_CLEAN_SLACK;
    if (!(unite(parent, a, b, cap) && unite(parent, b, c, cap))) st(count + a, -1);
}

__global__ __launch_bounds__(TB) void flatten_kernel(int V, int* label, int* count)
{
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    if (i >= (long long)V) return;
    int x = (int)i;
    u64 steps = 0;
    const u64 cap = (u64)V + HSR_MESH_CLEAN_SLACK;
    for (int p = ld(label + x); p != x; p = ld(label + x)) {
        if (++steps > cap) { st(count + i, -1); return; }
        x = p;
    }
    if (x != (int)i) st(label + i, x);
}

__global__ __launch_bounds__(TB) void count_kernel(int V, int F, const int* __restrict__ faces, const int* __restrict__ label, int* count)
{
    const long long f = (long long)blockIdx.x * TB + threadIdx.x;
    int r = -1;
    if (f < (long long)F) {
        const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        if (valid_face(V, a, b, c)) r = label[a];
    }
    // the lanes of the wave that share a label add once.  Each trip retires at least its leader: at most 64 trips
    const int lane = threadIdx.x & 63;
    bool todo = (unsigned)r < (unsigned)V;      // a label is in 0..V-1 (flatten wrote it)
    for (u64 left = __ballot(todo); left != 0; left = __ballot(todo)) {
        const int leader = __ffsll((long long)left) - 1;
        const int r0 = __shfl(r, leader);
        const u64 same = __ballot(todo && r == r0);
        if (lane == leader && count[r0] >= 0)      // a negative entry is a gave-up mark of an earlier launch: it stays
            __hip_atomic_fetch_add(count + r0, (int)__popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (r == r0) todo = false;
    }
}

// ---- select ------------------------------------------------------------------------------------------------------------------------
// is face f kept?  Its three indices come back in a, b, c
__device__ __forceinline__ bool kept_face(int V, int F, long long f, const int* __restrict__ faces, const int* __restrict__ label,
                                          const uint8_t* __restrict__ keep, int& a, int& b, int& c)
{
    if (f >= (long long)F) return false;
    a = faces[3 * (size_t)f]; b = faces[3 * (size_t)f + 1]; c = faces[3 * (size_t)f + 2];
    if (!valid_face(V, a, b, c)) return false;
    const int r = label[a];
    return (unsigned)r < (unsigned)V && keep[r] != 0;
}

__global__ __launch_bounds__(TB) void face_count_kernel(int V, int F, const int* __restrict__ faces, const int* __restrict__ label,
                                                        const uint8_t* __restrict__ keep, int* __restrict__ remap, unsigned* __restrict__ fcount)
{
    __shared__ unsigned s4[4];
    int a, b, c;
    const bool k = kept_face(V, F, (long long)blockIdx.x * TB + threadIdx.x, faces, label, keep, a, b, c);
    if (k) { remap[a] = 1; remap[b] = 1; remap[c] = 1; }      // the same value from every lane that names the vertex
    const unsigned n = hsr_block256_count(k, s4);
    if (threadIdx.x == 0) fcount[blockIdx.x] = n;
}

__global__ __launch_bounds__(TB) void vertex_count_kernel(int V, const int* __restrict__ remap, unsigned* __restrict__ vcount)
{
    __shared__ unsigned s4[4];
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    const unsigned n = hsr_block256_count(i < (long long)V && remap[i] != 0, s4);
    if (threadIdx.x == 0) vcount[blockIdx.x] = n;
}

__global__ __launch_bounds__(1024) void scan_kernel(int nfb, unsigned* __restrict__ fcount, int nvb, unsigned* __restrict__ vcount,
                                                    long long* __restrict__ out_counts)
{
    __shared__ unsigned s17[17];
    const unsigned nf = hsr_block1024_exclusive_scan(nfb, fcount, s17);
    __syncthreads();      // s17 is read by every thread before the second scan stores to it
    const unsigned nv = hsr_block1024_exclusive_scan(nvb, vcount, s17);
    if (threadIdx.x == 0) { out_counts[0] = (long long)nf; out_counts[1] = (long long)nv; out_counts[2] = 0; }
}

__global__ __launch_bounds__(TB) void vertex_scatter_kernel(int V, int* __restrict__ remap, const unsigned* __restrict__ voff, int* __restrict__ out_source)
{
    __shared__ unsigned s_w[4];
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    const bool k = i < (long long)V && remap[i] != 0;
    const unsigned dst = voff[blockIdx.x] + hsr_block_rank<4>(k, s_w);      // < V' <= V
    if (k) { out_source[dst] = (int)i; remap[i] = (int)dst; }
}

__global__ __launch_bounds__(TB) void face_scatter_kernel(int V, int F, const int* __restrict__ faces, const int* __restrict__ label,
                                                          const uint8_t* __restrict__ keep, const int* __restrict__ remap,
                                                          const unsigned* __restrict__ foff, int* __restrict__ out_faces)
{
    __shared__ unsigned s_w[4];
    int a, b, c;
    const bool k = kept_face(V, F, (long long)blockIdx.x * TB + threadIdx.x, faces, label, keep, a, b, c);
    const size_t dst = (size_t)foff[blockIdx.x] + hsr_block_rank<4>(k, s_w);      // < F' <= F
    if (k) { out_faces[3 * dst] = remap[a]; out_faces[3 * dst + 1] = remap[b]; out_faces[3 * dst + 2] = remap[c]; }
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
unsigned blocks_of(int n) { return (unsigned)(((long long)n + TB - 1) / TB); }

struct Scratch { size_t remap, fcount, vcount, end; };

Scratch scratch_layout(int V, int F)
{
    Scratch l;
    l.remap = 0;
    l.fcount = align16(sizeof(int) * (size_t)V);
    l.vcount = l.fcount + align16(sizeof(unsigned) * (size_t)blocks_of(F));
    l.end = l.vcount + align16(sizeof(unsigned) * (size_t)blocks_of(V)) + 16;
    return l;
}

}  // namespace

extern "C" int hsr_mesh_components(int V, int F, const int* faces, int* out_label, int* out_face_count, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 0 || F < 0) {
        hsr_set_error("mesh_components: invalid sizes V=%d F=%d (both >= 0)", V, F);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (F > 0 && !faces) {
        hsr_set_error("mesh_components: faces is required with F > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (V > 0 && (!out_label || !out_face_count)) {
        hsr_set_error("mesh_components: out_label and out_face_count are required with V > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (V == 0) return HSR_OK;
    init_kernel<<<blocks_of(V), TB, 0, stream>>>(V, out_label, out_face_count);
    HSR_HIP_CHECK(hipGetLastError());
    if (F == 0) return HSR_OK;
    hook_kernel<<<blocks_of(F), TB, 0, stream>>>(V, F, faces, out_label, out_face_count);
    HSR_HIP_CHECK(hipGetLastError());
    flatten_kernel<<<blocks_of(V), TB, 0, stream>>>(V, out_label, out_face_count);
    HSR_HIP_CHECK(hipGetLastError());
    count_kernel<<<blocks_of(F), TB, 0, stream>>>(V, F, faces, out_label, out_face_count);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}

extern "C" size_t hsr_mesh_select_scratch_bytes(int V, int F)
{
    if (V < 0 || F < 0) return 0;
    return scratch_layout(V, F).end;
}

extern "C" int hsr_mesh_select(int V, int F, const int* faces, const int* label, const uint8_t* keep_by_label, int* out_faces, int* out_source,
                               int64_t* out_counts, void* scratch, size_t scratch_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 0 || F < 0) {
        hsr_set_error("mesh_select: invalid sizes V=%d F=%d (both >= 0)", V, F);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (F > 0 && (!faces || !out_faces)) {
        hsr_set_error("mesh_select: faces and out_faces are required with F > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (V > 0 && (!label || !keep_by_label || !out_source)) {
        hsr_set_error("mesh_select: label, keep_by_label and out_source are required with V > 0");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    if (!out_counts) {
        hsr_set_error("mesh_select: out_counts is required");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    const Scratch l = scratch_layout(V, F);
    if (!scratch || scratch_bytes < l.end || (reinterpret_cast<uintptr_t>(scratch) & 15) != 0) {
        hsr_set_error("mesh_select: the scratch must hold %zu bytes (hsr_mesh_select_scratch_bytes) and be 16-byte aligned; %zu given%s", l.end,
                      scratch_bytes, scratch ? "" : " (NULL)");
        return HSR_ERR_INVALID_ARGUMENT;
    }
    char* base = reinterpret_cast<char*>(scratch);
    int* remap = reinterpret_cast<int*>(base + l.remap);
    unsigned* fcount = reinterpret_cast<unsigned*>(base + l.fcount);
    unsigned* vcount = reinterpret_cast<unsigned*>(base + l.vcount);
    const unsigned nfb = blocks_of(F), nvb = blocks_of(V);      // <= 2^23
    if (V > 0) HSR_HIP_CHECK(hipMemsetAsync(remap, 0, sizeof(int) * (size_t)V, stream));
    if (nfb > 0) {
        face_count_kernel<<<nfb, TB, 0, stream>>>(V, F, faces, label, keep_by_label, remap, fcount);
        HSR_HIP_CHECK(hipGetLastError());
    }
    if (nvb > 0) {
        vertex_count_kernel<<<nvb, TB, 0, stream>>>(V, remap, vcount);
        HSR_HIP_CHECK(hipGetLastError());
    }
    scan_kernel<<<1, 1024, 0, stream>>>((int)nfb, fcount, (int)nvb, vcount, reinterpret_cast<long long*>(out_counts));
    HSR_HIP_CHECK(hipGetLastError());
    if (nvb > 0) {
        vertex_scatter_kernel<<<nvb, TB, 0, stream>>>(V, remap, vcount, out_source);
        HSR_HIP_CHECK(hipGetLastError());
    }
    if (nfb > 0) {
        face_scatter_kernel<<<nfb, TB, 0, stream>>>(V, F, faces, label, keep_by_label, remap, fcount, out_faces);
        HSR_HIP_CHECK(hipGetLastError());
    }
    return HSR_OK;
}
