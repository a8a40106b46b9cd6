// hsr_optim.hip — the optimizer step (gfx950): one Adam step over a table of tensors in one launch, and the tracking loop's best-pose
// bookkeeping (include/hsr_optim.h).
//
// Adam is a pure stream: 16 bytes read (p, g, m, v) and 12 written (p, m, v) per element, a dozen flops.  One launch covers up to
// HSR_ADAM_MAX_TENSORS tensors: the table travels by value in the kernel arguments, and the blocks are handed out to the tensors in
// proportion to numel (at least one per non-empty tensor), so one block never spans two tensors and needs no per-element lookup.
// Inside a tensor each thread takes float4s with a grid-stride loop when p, g, m and v are all 16-byte aligned (the usual case);
// views at odd float offsets (grads of the multi-GPU exchange bucket, rows of an odd P) take the scalar loop.  No LDS, no atomics.
//
// The arithmetic reproduces torch's foreach Adam (the default on a HIP device) bit for bit: the same operation order, fp32
// throughout, and the fused multiply-adds exactly where torch's own kernels have them.  The file is built with
// -ffp-contract=off so that the compiler adds no other contraction; the fmaf() calls below are the only ones.
#include "hsr_common.h"
#include "../../include/hsr_optim.h"
#include <cmath>

namespace {

constexpr int AB = 256;            // threads per block
constexpr int MAX_BLOCKS = 2048;   // grid cap per launch: 8 blocks of 256 per CU on 256 CUs

struct AdamLaunch {
    hsr_adam_tensor t[HSR_ADAM_MAX_TENSORS];
    int block_start[HSR_ADAM_MAX_TENSORS + 1];   // blocks [block_start[j], block_start[j+1]) serve tensor j
    int n;
};

struct AdamScalars {
    float step_size, bc2_sqrt, eps, w1, beta2, omb2;
};

// torch's lerp (ATen/native/Lerp.h) with the weight as a float scalar
__device__ __forceinline__ float adam_lerp(float m, float g, float w)
{
    return fabsf(w) < 0.5f ? fmaf(w, g - m, m) : g - (g - m) * (1.0f - w);
}

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamScalars& s)
{
    m = adam_lerp(m, g, s.w1);                 // _foreach_lerp_(exp_avgs, grads, 1 - beta1)
    v = v * s.beta2;                           // _foreach_mul_(exp_avg_sqs, beta2)
    v = fmaf(s.omb2, g * g, v);                // _foreach_addcmul_(exp_avg_sqs, grads, grads, 1 - beta2)
    float d = sqrtf(v);                        // _foreach_sqrt(exp_avg_sqs)
    d = d / s.bc2_sqrt;                        // _foreach_div_(., bias_correction2_sqrt)
    d = d + s.eps;                             // _foreach_add_(., eps)
    p = fmaf(s.step_size, m / d, p);           // _foreach_addcdiv_(params, exp_avgs, ., step_size)
}

__global__ __launch_bounds__(AB) void adam_step_kernel(const AdamLaunch args)
{
    int j = 0;
    while (j + 1 < args.n && (int)blockIdx.x >= args.block_start[j + 1]) j++;
    const hsr_adam_tensor& t = args.t[j];
    const AdamScalars s{t.step_size, t.bc2_sqrt, t.eps, t.one_minus_beta1, t.beta2, t.one_minus_beta2};
    const int64_t first = (int64_t)(blockIdx.x - args.block_start[j]) * AB + threadIdx.x;
    const int64_t stride = (int64_t)(args.block_start[j + 1] - args.block_start[j]) * AB;
    const int64_t n = t.numel;
    float* __restrict__ P = t.param;
    const float* __restrict__ G = t.grad;
    float* __restrict__ M = t.exp_avg;
    float* __restrict__ V = t.exp_avg_sq;
    int64_t scalar_from = 0;
    if ((((uintptr_t)P | (uintptr_t)G | (uintptr_t)M | (uintptr_t)V) & 15) == 0) {
        const int64_t n4 = n >> 2;
        for (int64_t i = first; i < n4; i += stride) {
            float4 p = reinterpret_cast<const float4*>(P)[i];
            const float4 g = reinterpret_cast<const float4*>(G)[i];
            float4 m = reinterpret_cast<const float4*>(M)[i];
            float4 v = reinterpret_cast<const float4*>(V)[i];
            adam_elem(p.x, g.x, m.x, v.x, s);
            adam_elem(p.y, g.y, m.y, v.y, s);
            adam_elem(p.z, g.z, m.z, v.z, s);
            adam_elem(p.w, g.w, m.w, v.w, s);
            reinterpret_cast<float4*>(P)[i] = p;
            reinterpret_cast<float4*>(M)[i] = m;
            reinterpret_cast<float4*>(V)[i] = v;
        }
        scalar_from = n4 << 2;
    }
    for (int64_t i = scalar_from + first; i < n; i += stride) {
        float p = P[i], m = M[i], v = V[i];
        adam_elem(p, G[i], m, v, s);
        P[i] = p;
        M[i] = m;
        V[i] = v;
    }
}

// one wave: the compare on every lane (all read the same two scalars), the copies on lanes 0..3 / 0..2
__global__ void keep_best_kernel(int T, int time_idx, const float* __restrict__ loss, float* __restrict__ best_loss,
                                 const float* __restrict__ rots, const float* __restrict__ trans, float* __restrict__ cand_rots,
                                 float* __restrict__ cand_trans)
{
    const float l = *loss;
    if (!(l < *best_loss)) return;             // a NaN loss keeps the old candidate, as Python's `<` does
    const int k = threadIdx.x;
    if (k < 4) cand_rots[k] = rots[(int64_t)k * T + time_idx];
    if (k < 3) cand_trans[k] = trans[(int64_t)k * T + time_idx];
    if (k == 0) *best_loss = l;
}

}  // namespace

extern "C" size_t hsr_adam_table_entry_bytes(void) { return sizeof(hsr_adam_tensor); }

extern "C" int hsr_adam_step(int n, const hsr_adam_tensor* table, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || (n > 0 && !table)) {
        hsr_set_error("adam_step: n=%d (>= 0) or NULL table", n);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    for (int i = 0; i < n; i++) {
        const hsr_adam_tensor& t = table[i];
        if (t.numel < 0 || (t.numel > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq))) {
            hsr_set_error("adam_step: entry %d has numel=%lld or a NULL pointer", i, (long long)t.numel);
            return HSR_ERR_INVALID_ARGUMENT;
        }
    }
    for (int base = 0; base < n; base += HSR_ADAM_MAX_TENSORS) {
        const int cnt = n - base < HSR_ADAM_MAX_TENSORS ? n - base : HSR_ADAM_MAX_TENSORS;
        // blocks wanted per tensor at one float4 per thread, scaled down to the grid cap in proportion to numel
        int64_t want[HSR_ADAM_MAX_TENSORS], total = 0;
        for (int i = 0; i < cnt; i++) {
            want[i] = (table[base + i].numel + 4 * AB - 1) / (4 * AB);
            total += want[i];
        }
        if (total == 0) continue;
        AdamLaunch a;
        a.n = cnt;
        int blocks = 0;
        for (int i = 0; i < cnt; i++) {
            a.t[i] = table[base + i];
            a.block_start[i] = blocks;
            int64_t nb = want[i];
            if (total > MAX_BLOCKS && nb > 0) {
                nb = nb * MAX_BLOCKS / total;
                if (nb < 1) nb = 1;
            }
            blocks += (int)nb;
        }
        for (int i = cnt; i <= HSR_ADAM_MAX_TENSORS; i++) a.block_start[i] = blocks;
        for (int i = cnt; i < HSR_ADAM_MAX_TENSORS; i++) a.t[i] = hsr_adam_tensor{};
        adam_step_kernel<<<blocks, AB, 0, stream>>>(a);
        HSR_HIP_CHECK(hipGetLastError());
    }
    return HSR_OK;
}

extern "C" int hsr_track_keep_best(int T, int time_idx, const float* loss, float* best_loss, const float* cam_unnorm_rots,
                                   const float* cam_trans, float* cand_rots, float* cand_trans, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (T < 1 || time_idx < 0 || time_idx >= T || !loss || !best_loss || !cam_unnorm_rots || !cam_trans || !cand_rots || !cand_trans) {
        hsr_set_error("track_keep_best: T=%d time_idx=%d (0..T-1) or a NULL pointer", T, time_idx);
        return HSR_ERR_INVALID_ARGUMENT;
    }
    keep_best_kernel<<<1, 64, 0, stream>>>(T, time_idx, loss, best_loss, cam_unnorm_rots, cam_trans, cand_rots, cand_trans);
    HSR_HIP_CHECK(hipGetLastError());
    return HSR_OK;
}
