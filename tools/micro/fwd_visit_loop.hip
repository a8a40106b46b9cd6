// Micro-benchmark: what does a trip of the forward's visit loop cost, and what does staging it by hand buy?  (EXPERIMENTS.md §10n; the
// forward's counterpart of visit_loop.hip.)  Reproduces the K = 26 trip of render_fwd_kernel (hsr_render_fwd.hip, the per-lane kernels)
// on synthetic LDS contents of the kernel's own layout — 240 staged entries and the dummy: a 32-byte record and a 112-byte feature row
// each, sixteen byte lists of stride 260 — with the list byte, the record, the alpha chain with v_exp_f32, the contribution mask and the
// skip branch, the seven 16-byte row reads, the fifteen packed FMAs and the selects for T, T_out, the last slot and the median slot.
// Template flags select the form of the loop, a sum of (the kernel ships 1 + 4 + 8 = 13, and 15 at K = 16):
//   0 the straight loop as hipcc schedules it;  1 the record a trip ahead and the list byte two;  2 the alpha stage a trip ahead as well;
//   4 the row reads in two groups, each with its FMAs behind it;  8 no skip branch.
// It runs at 1..4 workgroups of four waves per CU (LDS padding sets the occupancy) and prints one JSON line per (variant, occupancy) with
// shader cycles per trip and wave (clock64, the counter tools/trace_fwd.py reads).  Twenty-six idle registers stand for the staging
// registers the kernel keeps across the loop.
// Build: hipcc --offload-arch=gfx950 -O3 fwd_visit_loop.hip -o fwd_visit_loop
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int KC = 26, RW = 28, NQ = RW / 4, BATCH = 240, LSTRIDE = 260;
constexpr int TRIPS = 64;   // per repetition: opacity 0.01, so T ends near 0.53 and crosses nothing twice

template <int F>
__global__ void __launch_bounds__(256, 4) k(float* out, unsigned long long* cyc, int iters, int pad_words)
{
    extern __shared__ float4 s_dyn[];
    __shared__ float4 s_rec[(BATCH + 1) * 2];
    __shared__ float4 s_row[(BATCH + 1) * NQ];
    __shared__ uint8_t s_sublist[16 * LSTRIDE];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, sb = wv * 4 + (lane >> 4);
    // records: centres within two pixels of the 16x16 tile's middle, a wide isotropic conic (pre-scaled as the kernel stages it), opacity
    // 0.01: every pixel is reached by every entry (alpha >= 1/255) and nothing finishes
    for (int i = t; i < BATCH; i += 256) {
        const float sig2 = 400.f, l2e = 1.44269504f;
        s_rec[2 * i] = make_float4(6.f + 0.017f * i, 9.f - 0.013f * i, -0.5f * l2e / sig2, 0.f);
        s_rec[2 * i + 1] = make_float4(-0.5f * l2e / sig2, 0.01f, 0.3f + 0.001f * i, 0.6f - 0.001f * i);
        for (int q = 0; q < NQ; q++) s_row[i * NQ + q] = make_float4(0.01f * q, 0.02f * q + 0.001f * i, 0.5f, 0.25f + 0.01f * q);
    }
    if (t < 2) s_rec[2 * BATCH + t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < NQ) s_row[BATCH * NQ + t] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = t; i < 16 * LSTRIDE; i += 256) {
        const int b = i / LSTRIDE, l = i % LSTRIDE;
        // every 32nd trip of a wave is one no lane contributes to (all four groups on the dummy): the kernel's 2 %
        s_sublist[i] = (uint8_t)((l < TRIPS && (l & 31) != 17) ? (l * 13 + b * 7) % BATCH : BATCH);
    }
    if (pad_words > 0 && t == 0) s_dyn[0] = make_float4(0, 0, 0, 0);
    __syncthreads();
    float pfx = (float)(lane & 3) + 4.f * ((lane >> 4) & 1) + 0.5f, pfy = (float)((lane >> 2) & 3) + 4.f * wv + 0.5f;
    asm volatile("" : "+v"(pfx), "+v"(pfy));
    float park[KC];   // the staging registers of the next batch
#pragma unroll
    for (int c = 0; c < KC; c++) {
        park[c] = 0.001f * (c + lane);
        asm volatile("" : "+v"(park[c]));
    }
    float S[KC];
#pragma unroll
    for (int c = 0; c < KC; c++) S[c] = 0.f;
    float C0 = 0, C1 = 0, C2 = 0, Dd = 0;
    int last_acc = 0, med_acc = 0;
    const uint8_t* list = s_sublist + sb * LSTRIDE;
    const int m = __builtin_amdgcn_readfirstlane(iters >= 0 ? TRIPS : 0);   // a run-time trip count, as in the kernel

    auto alpha_of = [&](const float4& g, const float2& co, float& alpha) -> bool {
        const float dx = g.x - pfx, dy = g.y - pfy;
        const float power2 = fmaf(co.x, dy * dy, fmaf(g.w, dx * dy, g.z * (dx * dx)));
        alpha = fminf(0.99f, co.y * __builtin_amdgcn_exp2f(power2));
        return power2 <= 0.0f && alpha >= 1.0f / 255.0f;
    };
    auto read_rec = [&](int slot, float4& g, float2& co) {
        g = s_rec[2 * slot];
        co = *reinterpret_cast<const float2*>(&s_rec[2 * slot + 1]);
    };

    unsigned long long total = 0;
    for (int rep = 0; rep < iters; rep++) {
        float T = 1.0f, T_out = 1.0f;
        int last_rel = -1, med_rel = -1;
        asm volatile("" : "+v"(T), "+v"(T_out), "+v"(last_rel), "+v"(med_rel));
        const long long t0 = clock64();
        if constexpr (F == 0) {
            // the kernel's loop before it was staged: plain C++ as hipcc schedules it, with the skip branch
            int j = (int)list[0];
            for (int kk = 0; kk < m; kk++) {
                const int j_next = (int)list[kk + 1];
                const float4 g = s_rec[2 * j];
                const float4 h4 = s_rec[2 * j + 1];
                const float2 co = make_float2(h4.x, h4.y);
                const float dx = g.x - pfx, dy = g.y - pfy;
                const float power2 = fmaf(co.x, dy * dy, fmaf(g.w, dx * dy, g.z * (dx * dx)));
                const float alpha = fminf(0.99f, co.y * __builtin_amdgcn_exp2f(power2));
                const bool reach = power2 <= 0.0f && alpha >= 1.0f / 255.0f;
                const float test_T = T * (1.0f - alpha);
                const bool low = test_T < 0.0001f;
                const bool contrib = reach && !low;
                const float w = contrib ? alpha * T : 0.f;
                if (__ballot(contrib) == 0ull) {
                    T = reach ? 0.0f : T;
                    j = j_next;
                    continue;
                }
                C0 = fmaf(h4.z, w, C0);
                C1 = fmaf(h4.w, w, C1);
                const float4* row = &s_row[j * NQ];
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const float4 f = row[q];
                    const float fv[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int c = 4 * q + i;
                        if (c < KC) S[c < KC ? c : 0] = fmaf(fv[i], w, S[c < KC ? c : 0]);
                        else if (c == KC) C2 = fmaf(fv[i], w, C2);
                        else Dd = fmaf(fv[i], w, Dd);
                    }
                }
                const float T_was = T_out;
                T_out = contrib ? test_T : T_out;
                med_rel = (T_was > 0.5f && T_out < 0.5f) ? j : med_rel;
                last_rel = contrib ? j : last_rel;
                T = reach ? (low ? 0.0f : test_T) : T;
                j = j_next;
            }
        } else {
            // hsr_render_fwd.hip's staged loop, with its stages behind flags
            constexpr int Q1 = (F & 4) ? (NQ - 1) / 2 : NQ;
            int j = (int)list[0], j1 = (int)list[1];
            float4 g;
            float2 co;
            read_rec(j, g, co);
            float alpha = 0.f;
            bool reach = false;
            if constexpr ((F & 2) != 0) reach = alpha_of(g, co, alpha);
            for (int kk = 0; kk < m; kk++) {
                if constexpr ((F & 2) == 0) reach = alpha_of(g, co, alpha);
                const float test_T = T * (1.0f - alpha);
                const bool low = test_T < 0.0001f;
                const bool contrib = reach && !low;
                const float w = contrib ? alpha * T : 0.f;
                const int j2 = (int)list[kk + 2];
                read_rec(j1, g, co);
                const bool any = (F & 8) != 0 || __ballot(contrib) != 0ull;
                const float4* row = &s_row[j * NQ];
                float4 f[NQ];
                float2 rg = make_float2(0.f, 0.f);
                if (any) {
                    rg = reinterpret_cast<const float2*>(&s_rec[2 * j + 1])[1];
#pragma unroll
                    for (int q = 0; q < Q1; q++) f[q] = row[q];
                }
                float alpha_n = 0.f;
                bool reach_n = false;
                if constexpr ((F & 2) != 0) reach_n = alpha_of(g, co, alpha_n);
                if (any) {
                    C0 = fmaf(rg.x, w, C0);
                    C1 = fmaf(rg.y, w, C1);
                    auto blend = [&](int q) {
                        const float fv[4] = {f[q].x, f[q].y, f[q].z, f[q].w};
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int c = 4 * q + i;
                            if (c < KC) S[c < KC ? c : 0] = fmaf(fv[i], w, S[c < KC ? c : 0]);
                            else if (c == KC) C2 = fmaf(fv[i], w, C2);
                            else Dd = fmaf(fv[i], w, Dd);
                        }
                    };
                    if constexpr (Q1 < NQ) {
#pragma unroll
                        for (int q = 0; q < Q1; q++) blend(q);
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int q = Q1; q < NQ; q++) f[q] = row[q];
#pragma unroll
                        for (int q = Q1; q < NQ; q++) blend(q);
                    } else {
#pragma unroll
                        for (int q = 0; q < NQ; q++) blend(q);
                    }
                    const float T_was = T_out;
                    T_out = contrib ? test_T : T_out;
                    med_rel = (T_was > 0.5f && T_out < 0.5f) ? j : med_rel;
                    last_rel = contrib ? j : last_rel;
                }
                T = reach ? (low ? 0.0f : test_T) : T;
                if constexpr ((F & 2) != 0) {
                    alpha = alpha_n;
                    reach = reach_n;
                }
                j = j1;
                j1 = j2;
            }
        }
        total += (unsigned long long)(clock64() - t0);
        last_acc += last_rel;
        med_acc += med_rel;
        C0 += T + T_out;
    }
    if (lane == 0) cyc[blockIdx.x * 4 + wv] = total;
    float acc = C0 + C1 + C2 + Dd + (float)last_acc + (float)med_acc;
#pragma unroll
    for (int c = 0; c < KC; c++) acc += S[c] + park[c];
    out[blockIdx.x * 256 + t] = acc;
}

template <int F>
void run(const char* name, int wg_per_cu, int cus)
{
    const int blocks = cus * wg_per_cu, iters = 200;
    float* out;
    unsigned long long* cyc;
    CK(hipMalloc(&out, sizeof(float) * blocks * 256));
    CK(hipMalloc(&cyc, sizeof(unsigned long long) * blocks * 4));
    // static LDS of the kernel: 7 712 + 26 992 + 4 160 B = 38 864 B; pad so that exactly wg_per_cu workgroups fit a CU's 160 KB
    const int per_wg = 160 * 1024 / wg_per_cu;
    int dyn = per_wg - 38864 - 256;
    if (dyn < 0 || wg_per_cu == 4) dyn = 0;
    CK(hipFuncSetAttribute((const void*)k<F>, hipFuncAttributeMaxDynamicSharedMemorySize, dyn));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    k<F><<<blocks, 256, dyn>>>(out, cyc, 5, dyn / 4);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    k<F><<<blocks, 256, dyn>>>(out, cyc, iters, dyn / 4);
    CK(hipEventRecord(e1));
    CK(hipDeviceSynchronize());
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> h(blocks * 4);
    CK(hipMemcpy(h.data(), cyc, sizeof(unsigned long long) * blocks * 4, hipMemcpyDeviceToHost));
    std::sort(h.begin(), h.end());
    const double med = (double)h[h.size() / 2] / ((double)iters * TRIPS);
    printf("{\"variant\": \"%s\", \"flags\": %d, \"wg_per_cu\": %d, \"cycles_per_trip_per_wave\": %.1f, \"kernel_ms\": %.4f, \"err\": \"%s\"}\n", name, F,
           wg_per_cu, med, ms, hipGetErrorString(hipGetLastError()));
    fflush(stdout);
    CK(hipFree(out));
    CK(hipFree(cyc));
}

int main()
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) {
        fprintf(stderr, "no device\n");
        return 1;
    }
    const int cus = prop.multiProcessorCount;
    for (int w = 1; w <= 4; w++) {
        run<0>("straight", w, cus);
        run<1>("record + list byte ahead", w, cus);
        run<3>("+ alpha stage ahead", w, cus);
        run<5>("record ahead, rows in two groups", w, cus);
        run<7>("+ alpha stage ahead, rows in two groups", w, cus);
        run<9>("record ahead, no skip branch", w, cus);
        run<11>("+ alpha stage ahead, no skip branch", w, cus);
        run<13>("record ahead, rows in two groups, no skip branch", w, cus);
        run<15>("+ alpha stage ahead, rows in two groups, no skip branch", w, cus);
    }
    return 0;
}
