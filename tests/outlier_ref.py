"""The ignore_outlier_depth_loss branch of the reference's get_loss* (scripts/hierslam.py:909-937) restated in torch, runnable on the
CPU: the oracle of include/ext/hsr_loss_outlier.h (tests/test_loss_outlier_cpu.py, tests/test_gpu_loss_outlier.py).

    depth_error = torch.abs(curr_data['depth'] - depth) * (curr_data['depth'] > 0)        :911
    mask = (depth_error < 10*depth_error.median())                                      :912
    mask = mask & (curr_data['depth'] > 0)                                              :913
    mask = mask & ~torch.isnan(depth)  [& (silhouette > sil_thres)]                     :909, :916-919
    losses['depth'] = torch.abs(curr_data['depth'] - depth)[mask].sum() | .mean()       :925 (tracking) | :927 (mapping)
    losses['im'] = torch.abs(curr_data['im'] - im)[torch.tile(mask, (3, 1, 1))].sum()   :932-935 (tracking, with the flag on: always masked)

reject=False leaves the factor of :912 out of the mask (median and threshold are still reported): the mask of hsr_loss_tracking_* (include/hsr_losses.h).
"""
import torch

W_DEPTH, W_IM = 1.0, 0.5      # the reference's tracking weights (configs/replica/hierslam_semantic_run.py)


def rank_rule(values):
    """torch.median's element as the header states it: NaN if any value is NaN, else the element of 0-based rank (n - 1) // 2 in
    ascending order (the LOWER of the two middle values for an even n)"""
    v = values.reshape(-1)
    if torch.isnan(v).any():
        return torch.tensor(float("nan"), dtype=v.dtype)
    return v.sort().values[(v.numel() - 1) // 2]


def outlier_mask(depth, gt_depth, silhouette=None, sil_thres=0.99, reject=True):
    """(median, threshold, mask) of :909-919 for fp32 [H,W] maps; median and threshold are fp32 0-dim tensors as torch computes them"""
    err = torch.abs(gt_depth - depth) * (gt_depth > 0)
    median = err.median()
    threshold = 10 * median
    mask = (gt_depth > 0) & ~torch.isnan(depth)
    if reject:
        mask = (err < threshold) & mask
    if silhouette is not None:
        mask = mask & (silhouette > sil_thres)
    return median, threshold, mask.detach()


def outlier_ref(depth, gt_depth, im=None, gt_im=None, silhouette=None, sil_thres=0.99, reject=True):
    """median, threshold, mask, and both terms summed in float64 over that mask (from the fp32 inputs); `count` selected pixels.
    depth / gt_depth / silhouette: [H,W]; im / gt_im: [3,H,W] or None"""
    median, threshold, mask = outlier_mask(depth, gt_depth, silhouette, sil_thres, reject)
    out = {"median": median, "threshold": threshold, "mask": mask, "count": int(mask.sum()),
           "depth_sum": float((gt_depth.double() - depth.double()).abs()[mask].sum())}
    if im is not None:
        out["colour_sum"] = float((gt_im.double() - im.double()).abs()[torch.tile(mask[None], (3, 1, 1))].sum())
    return out


def autograd_tracking(depth, gt_depth, im, gt_im, silhouette, sil_thres, upstream, reject=True):
    """torch autograd of the tracking form (:925, :935, weights W_DEPTH / W_IM) in fp32: (d loss / d im, d loss / d depth) of
    upstream * loss.  Where the depth is NaN torch's abs backward gives 0 * sign(NaN) = NaN off the mask; the caller decides."""
    d, a = depth.clone().requires_grad_(True), im.clone().requires_grad_(True)
    _m, _t, mask = outlier_mask(d.detach(), gt_depth, silhouette, sil_thres, reject)
    loss = W_DEPTH * torch.abs(gt_depth - d)[mask].sum() + W_IM * torch.abs(gt_im - a)[torch.tile(mask[None], (3, 1, 1))].sum()
    (loss * upstream).backward()
    return a.grad, d.grad


def autograd_mapping(depth, gt_depth, upstream, reject=True):
    """torch autograd of the mapping form's depth term (:927) in fp32: (mean, d (upstream * mean) / d depth)"""
    d = depth.clone().requires_grad_(True)
    _m, _t, mask = outlier_mask(d.detach(), gt_depth, reject=reject)
    loss = torch.abs(gt_depth - d)[mask].mean()
    (loss * upstream).backward()
    return loss.detach(), d.grad
