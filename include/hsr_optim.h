/*
 * hsr_optim.h — C ABI of the optimizer step (libhsr_rast.so): one Adam step over many tensors in one launch, and the tracking loop's
 * best-pose bookkeeping on the device.
 *
 * What it replaces in the reference (scripts/hierslam.py):
 *   optimizer.step()   torch.optim.Adam (:411-417, :1757), called once per tracking and mapping iteration (:1852, :2053, :2055).  On a
 *                      HIP device torch runs its foreach path: lerp, mul, addcmul, sqrt, div, add and addcdiv, seven passes over the
 *                      map, one with a map-sized temporary.  hsr_adam_step reads p, g, m, v and writes p, m, v once.
 *   best candidate     `if loss < current_min_loss:` and the two column copies (:1855-1860), a host synchronisation per tracking
 *                      iteration.  hsr_track_keep_best is one small launch that never reads anything back.
 *
 * Arithmetic (fp32, per element, the order of torch's default foreach non-capturable Adam; expression forms in DESIGN.md §7 row 6):
 *   m = lerp(m, g, 1-beta1)                 (|1-beta1| < 0.5: m + w*(g-m) as one fma; else g - (g-m)*(1-w))
 *   v = v*beta2;  v = v + (1-beta2)*(g*g)   (the second as one fma)
 *   d = sqrt(v) / bc2_sqrt + eps
 *   p = p + step_size*(m/d)                 (one fma)
 * Denormals are kept.  lr == 0 still updates m and v and writes p + (-0)*x: NaN and inf propagate exactly as in torch.
 *
 * All tensor pointers are DEVICE pointers to dense fp32 data; tables are HOST arrays passed by value in the kernel arguments (no
 * host-to-device copy).  Everything runs on `stream`; no allocation, no host synchronisation.  Errors: <0 and hsr_last_error()
 * (hsr_rasterizer.h).
 */
#ifndef HSR_OPTIM_H_INCLUDED
#define HSR_OPTIM_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* entries per launch; hsr_adam_step splits a longer table into several launches */
#define HSR_ADAM_MAX_TENSORS 32

/* One tensor of an Adam step.  The scalars are what torch's foreach path computes on the host, in double, cast to float:
 * step_size = (lr / (1 - beta1^step)) * -1, bc2_sqrt = (1 - beta2^step)^0.5, one_minus_beta1 = 1 - beta1, one_minus_beta2 = 1 - beta2.
 * param / grad / exp_avg / exp_avg_sq: numel floats each, no two of them overlapping.  Any float alignment: the kernel uses 16-byte
 * accesses where all four pointers are 16-byte aligned and scalar ones otherwise.  numel == 0 is legal. */
typedef struct hsr_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    float step_size;
    float bc2_sqrt;
    float eps;
    float one_minus_beta1;
    float beta2;
    float one_minus_beta2;
} hsr_adam_tensor;

/* sizeof(hsr_adam_tensor), for bindings that lay the struct out themselves */
size_t hsr_adam_table_entry_bytes(void);

/* One Adam step over the n tensors of `table` (HOST array): ceil(n / HSR_ADAM_MAX_TENSORS) launches, blocks of 256 threads handed to
 * the tensors of a launch in proportion to numel.  n == 0 does nothing. */
int hsr_adam_step(int n, const hsr_adam_tensor* table, void* stream);

/* The tracking loop's candidate rule (scripts/hierslam.py:1855-1860) as one launch: if *loss < *best_loss (a NaN loss never is),
 * *best_loss = *loss and column time_idx of cam_unnorm_rots [1,4,T] and cam_trans [1,3,T] (contiguous) is copied into
 * cand_rots [4] and cand_trans [3]; otherwise nothing is written.  loss, best_loss: fp32 scalars on the device. */
int hsr_track_keep_best(int T, int time_idx, const float* loss, float* best_loss, const float* cam_unnorm_rots, const float* cam_trans,
                        float* cand_rots, float* cand_trans, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HSR_OPTIM_H_INCLUDED */
