// Micro program for the register networks of the per-tile sort (hier-slam_amd/csrc/hsr_sort_net.h), to be run BEFORE the library first
// runs with a changed network: a wrong exchange can pair the high word of one composite with the low word of another and so invent a
// Gaussian index, which the render kernels must never see.
//
// 1. Correctness: every instantiation the library uses (E = 2, 4, 8 on two waves; E = 8 on four) and every exchange variant, through the
//    same load / network / store helpers as the library, against std::sort on the host.  Inputs: random, ascending, descending, all-equal
//    depth with shuffled indices; lengths 1, 2, 3 and every edge of the network (N/2 - 1, N/2, N/2 + 1, N - 1, N) plus ragged ones; segment
//    starts even (16-byte loads and stores) and odd (element-wise).  Guard words around every segment must come back untouched.
// 2. Cycles per tile of the exchange variants for steps inside a wave: SN_LDS, SN_BPERMUTE, SN_SWIZZLE, SN_DPP, SN_MIX; the headline's shape
//    (3 225 tiles of 263..448 entries, E = 4) and the four-wave E = 8 network (1 025..2 048 entries).
// Prints one JSON line per measurement and "ok" at the end; exit status 1 at the first mismatch or HIP error.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I hier-slam_amd/csrc tools/micro/sort_net.hip -o tools/micro/sort_net
// Run under a time limit of its own: timeout -k 10 120 tools/micro/sort_net
#include "hsr_sort_net.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#define CHECK(expr)                                                                              \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            printf("{\"error\": \"%s: %s\"}\n", #expr, hipGetErrorString(e__));                  \
            exit(1);                                                                             \
        }                                                                                        \
    } while (0)

// One tile per NT threads (two tiles per 256-thread workgroup at NT = 128, as tile_sort_pair_kernel), segment of tile i = [start[i], start[i] + len[i])
template <int E, int NT, int XCH>
__global__ void __launch_bounds__(256, 7) net_kernel(int T, const int* __restrict__ start, const int* __restrict__ len, uint64_t* keys, uint32_t* vals,
                                                     unsigned long long* ticks)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[(256 / NT) * (E / 2) * NT * 16];
    constexpr int PER = 256 / NT;
    const int sub = threadIdx.x / NT, tid = threadIdx.x % NT;
    const int tile = blockIdx.x * PER + sub;
    int r0 = 0, n = 0;
    if (tile < T) { r0 = start[tile]; n = len[tile]; }
    ulonglong2* buf = reinterpret_cast<ulonglong2*>(s_raw) + sub * ((E / 2) * NT);
    sg_u64* const kg = (sg_u64*)keys;
    sg_u32* const vg = (sg_u32*)vals;
    uint64_t x[E];
    sn_load_run<E>(kg + r0, (r0 & 1) == 0, E * tid, n, x);
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    net_bitonic<E, NT, XCH>(x, tid, buf);
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    sn_store_run<E>(kg + r0, vg + r0, r0, E * tid, n, (uint64_t)tile << 32, x);
    if (ticks && (threadIdx.x & 63) == 0) ticks[blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;
}

static const uint64_t GUARD_K = 0xDEADBEEFCAFEF00Dull;
static const uint32_t GUARD_V = 0xABCD1234u;

struct Case { int n; int kind; int odd; };   // kind: 0 random, 1 ascending, 2 descending, 3 equal depth + shuffled indices

template <int E, int NT, int XCH>
static int check(const char* name)
{
    constexpr int N = E * NT;
    std::vector<int> lens = {1, 2, 3, N / 2 - 1, N / 2, N / 2 + 1, N - 1, N, N / 2 + 2, N / 2 + 3, N - 2, N - 3, N - 5, N / 2 + E + 1, 5, 7};
    std::vector<Case> cases;
    for (int n : lens)
        if (n >= 1 && n <= N)
            for (int kind = 0; kind < 4; kind++)
                for (int odd = 0; odd < 2; odd++) cases.push_back({n, kind, odd});
    const int T = (int)cases.size();
    std::vector<int> start(T), len(T);
    std::vector<uint64_t> hk;
    std::vector<std::vector<uint64_t>> want(T);
    std::mt19937_64 rng(12345u + E * 131 + NT);
    // layout: [4 guards] segment [guards up to the next even / odd start]
    for (int i = 0; i < T; i++) {
        for (int g = 0; g < 4; g++) hk.push_back(GUARD_K);
        if ((int)(hk.size() & 1) != cases[i].odd) hk.push_back(GUARD_K);
        start[i] = (int)hk.size();
        len[i] = cases[i].n;
        std::vector<uint32_t> idx(cases[i].n);
        for (int e = 0; e < cases[i].n; e++) idx[e] = 1000u + 3u * e;           // unique indices
        if (cases[i].kind == 0 || cases[i].kind == 3) std::shuffle(idx.begin(), idx.end(), rng);
        for (int e = 0; e < cases[i].n; e++) {
            uint32_t d;
            if (cases[i].kind == 0) d = (uint32_t)(rng() % 50u) + 0x3f800000u;   // few depths: ties decided by the index half
            else if (cases[i].kind == 1) d = 0x3f800000u + e;
            else if (cases[i].kind == 2) d = 0x7f7fffffu - e;
            else d = 0x40000000u;
            hk.push_back(((uint64_t)d << 32) | idx[e]);
        }
        want[i].assign(hk.end() - cases[i].n, hk.end());
        std::sort(want[i].begin(), want[i].end());
    }
    for (int g = 0; g < 8; g++) hk.push_back(GUARD_K);
    const size_t R = hk.size();
    std::vector<uint32_t> hv(R, GUARD_V);
    uint64_t* dk; uint32_t* dv; int *ds, *dl;
    CHECK(hipMalloc(&dk, R * 8)); CHECK(hipMalloc(&dv, R * 4)); CHECK(hipMalloc(&ds, T * 4)); CHECK(hipMalloc(&dl, T * 4));
    CHECK(hipMemcpy(dk, hk.data(), R * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dv, hv.data(), R * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(ds, start.data(), T * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dl, len.data(), T * 4, hipMemcpyHostToDevice));
    constexpr int PER = 256 / NT;
    net_kernel<E, NT, XCH><<<(T + PER - 1) / PER, 256>>>(T, ds, dl, dk, dv, nullptr);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<uint64_t> gk(R);
    std::vector<uint32_t> gv(R);
    CHECK(hipMemcpy(gk.data(), dk, R * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(gv.data(), dv, R * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(dk)); CHECK(hipFree(dv)); CHECK(hipFree(ds)); CHECK(hipFree(dl));
    std::vector<char> inside(R, 0);
    int bad = 0;
    for (int i = 0; i < T && !bad; i++)
        for (int e = 0; e < len[i]; e++) {
            const size_t p = (size_t)start[i] + e;
            inside[p] = 1;
            const uint64_t wk = ((uint64_t)i << 32) | (want[i][e] >> 32);
            const uint32_t wv = (uint32_t)want[i][e];
            if (gk[p] != wk || gv[p] != wv) {
                printf("{\"net\": \"%s\", \"mismatch\": {\"n\": %d, \"kind\": %d, \"odd_start\": %d, \"element\": %d, \"key\": \"%016llx\", \"want_key\": \"%016llx\", "
                       "\"val\": %u, \"want_val\": %u}}\n", name, len[i], cases[i].kind, cases[i].odd, e, (unsigned long long)gk[p], (unsigned long long)wk, gv[p], wv);
                bad = 1;
                break;
            }
        }
    for (size_t p = 0; p < R && !bad; p++)
        if (!inside[p] && (gk[p] != GUARD_K || gv[p] != GUARD_V)) {
            printf("{\"net\": \"%s\", \"guard_overwritten_at\": %zu}\n", name, p);
            bad = 1;
        }
    printf("{\"net\": \"%s\", \"E\": %d, \"threads\": %d, \"cases\": %d, \"result\": \"%s\"}\n", name, E, NT, T, bad ? "MISMATCH" : "equal to std::sort");
    return bad;
}

template <int E, int NT, int XCH>
static void timing(const char* name, int T, int lo, int hi)
{
    std::mt19937_64 rng(777);
    std::vector<int> start(T), len(T);
    std::vector<uint64_t> hk;
    for (int i = 0; i < T; i++) {
        start[i] = (int)hk.size();
        len[i] = lo + (int)(rng() % (uint64_t)(hi - lo + 1));
        for (int e = 0; e < len[i]; e++) hk.push_back(((uint64_t)(0x3f800000u + (uint32_t)(rng() % 100000u)) << 32) | (uint32_t)(i * 4096 + e));
    }
    const size_t R = hk.size();
    constexpr int PER = 256 / NT;
    const int blocks = (T + PER - 1) / PER;
    uint64_t* dk; uint32_t* dv; int *ds, *dl; unsigned long long* dt;
    CHECK(hipMalloc(&dk, R * 8)); CHECK(hipMalloc(&dv, R * 4)); CHECK(hipMalloc(&ds, T * 4)); CHECK(hipMalloc(&dl, T * 4));
    CHECK(hipMalloc(&dt, (size_t)blocks * 4 * 8));
    CHECK(hipMemcpy(ds, start.data(), T * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dl, len.data(), T * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int rep = 0; rep < 12; rep++) {
        CHECK(hipMemcpy(dk, hk.data(), R * 8, hipMemcpyHostToDevice));   // composites again: the kernel sorts in place
        CHECK(hipEventRecord(e0));
        net_kernel<E, NT, XCH><<<blocks, 256>>>(T, ds, dl, dk, dv, dt);
        CHECK(hipEventRecord(e1));
        CHECK(hipGetLastError());
        CHECK(hipEventSynchronize(e1));
        float t;
        CHECK(hipEventElapsedTime(&t, e0, e1));
        if (rep >= 2) ms.push_back(t);
    }
    std::vector<unsigned long long> h((size_t)blocks * 4);
    CHECK(hipMemcpy(h.data(), dt, h.size() * 8, hipMemcpyDeviceToHost));
    std::sort(h.begin(), h.end());
    std::sort(ms.begin(), ms.end());
    // s_memtime counts at 100 MHz on gfx950
    printf("{\"net\": \"%s\", \"E\": %d, \"threads\": %d, \"tiles\": %d, \"entries\": [%d, %d], \"network_memtime_ticks_per_wave_median\": %llu, "
           "\"launch_us_min\": %.2f, \"launch_us_median\": %.2f, \"launch_us_max\": %.2f}\n", name, E, NT, T, lo, hi, h[h.size() / 2], ms.front() * 1e3,
           ms[ms.size() / 2] * 1e3, ms.back() * 1e3);
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
    CHECK(hipFree(dk)); CHECK(hipFree(dv)); CHECK(hipFree(ds)); CHECK(hipFree(dl)); CHECK(hipFree(dt));
}

int main()
{
    int bad = 0;
#define ALL(XCH, NAME)                                                                     \
    bad = bad || check<2, 128, XCH>(NAME) || check<4, 128, XCH>(NAME) || check<8, 128, XCH>(NAME) || check<8, 256, XCH>(NAME);
    ALL(SN_LDS, "lds")
    ALL(SN_BPERMUTE, "bpermute")
    ALL(SN_SWIZZLE, "swizzle+permlane32")
    ALL(SN_DPP, "dpp+permlane16/32")
    ALL(SN_MIX, "dpp(1,2)+swizzle+permlane32")
    if (bad) return 1;
    for (int round = 0; round < 2; round++) {
        timing<4, 128, SN_LDS>("lds", 3225, 263, 448);
        timing<4, 128, SN_BPERMUTE>("bpermute", 3225, 263, 448);
        timing<4, 128, SN_SWIZZLE>("swizzle+permlane32", 3225, 263, 448);
        timing<4, 128, SN_DPP>("dpp+permlane16/32", 3225, 263, 448);
        timing<4, 128, SN_MIX>("dpp(1,2)+swizzle+permlane32", 3225, 263, 448);
        timing<8, 256, SN_LDS>("lds", 3225, 1025, 2048);
        timing<8, 256, SN_BPERMUTE>("bpermute", 3225, 1025, 2048);
        timing<8, 256, SN_SWIZZLE>("swizzle+permlane32", 3225, 1025, 2048);
        timing<8, 256, SN_DPP>("dpp+permlane16/32", 3225, 1025, 2048);
        timing<8, 256, SN_MIX>("dpp(1,2)+swizzle+permlane32", 3225, 1025, 2048);
    }
    printf("ok\n");
    return 0;
}
