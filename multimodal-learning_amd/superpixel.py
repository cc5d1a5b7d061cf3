"""Superpixel attention masks of the MIA-2023 stage-1 trainer, reference
"MIA 2023/stage1_multi_modal_teacher/train_test_MT_SP_Masking.py":42-102 (`superpixel_attention_mask`).

Built here: everything after the input gradients exist (:77-98) - the per-superpixel aggregation of the image gradient
(the reference moves a one-hot [B, N, H*W] tensor to the HOST and runs the bmm there), the top-`Path_K` superpixel mask
and the top-`Omic_K` omic mask - as two kernels (csrc/superpixel.hip).  NOT built: the gradients themselves (:45-75
need an eval-mode backward down to the image, i.e. a stem dgrad kernel, which the distillation hot path never needs).

The label maps themselves: `slic_segment` (csrc/slic.hip), the role of the reference loader's `fast_slic` call."""
import torch

from . import ops
from ._lib import lib, check, ptr, stream, require_cuda


def slic_num_labels(H, W, num_components):
    """N = gy * gx <= num_components, the number of labels `slic_segment` produces for H x W tiles (host only)."""
    N = lib().ph_slic_num_labels(int(H), int(W), int(num_components))
    if N < 1:
        raise ValueError(f"no SLIC grid for {H} x {W} tiles and num_components={num_components}: needs 1 <= K, tiles of "
                         "1..8192 pixels a side, no more grid cells than pixels along an axis and at most 2048 labels")
    return N


def slic_connect(labels_i16, num_labels, min_size, out=None, chunk=None):
    """The connectivity pass of `slic_segment` on its own (csrc/slic.hip): labels_i16 int16
    [n, H, W] (device) with labels in [0, num_labels) -> int16 [n, H, W] in which every 4-connected component that is not
    the largest of its label, has fewer than `min_size` pixels and does not start at pixel (0, 0) carries the final label
    of the component above (in row 0: left of) its first pixel.  `out` may be `labels_i16` itself.  The store is walked
    in chunks of `chunk` tiles (default: a workspace of about 256 MB); tiles are independent."""
    t = require_cuda(labels_i16, "labels_i16")
    if t.dtype != torch.int16 or t.dim() != 3 or t.shape[0] < 1 or not t.is_contiguous():
        raise RuntimeError("labels_i16 must be a contiguous int16 [n, H, W] tensor")
    n, H, W = t.shape
    if not (1 <= H <= 8192 and 1 <= W <= 8192) or not (1 <= int(num_labels) <= 2048) or int(min_size) < 1:
        raise ValueError("needs tiles of 1..8192 pixels a side, 1 <= num_labels <= 2048 and min_size >= 1")
    if out is None:
        out = torch.empty_like(t)
    elif tuple(out.shape) != (n, H, W) or out.dtype != torch.int16 or not out.is_contiguous() or out.device != t.device:
        raise RuntimeError("out must be a contiguous int16 [n, H, W] tensor on the labels' device")
    if chunk is None:
        chunk = max(1, (256 << 20) // (8 * H * W))
    chunk = max(1, min(int(chunk), n, 65535))
    ws = torch.empty(lib().ph_slic_connect_workspace_bytes(chunk, H, W, int(num_labels)), device=t.device, dtype=torch.uint8)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        check(lib().ph_slic_connect(ptr(t[lo:]), ptr(out[lo:]), m, H, W, int(num_labels), int(min_size), ptr(ws), stream()),
              "ph_slic_connect")
    return out


def slic_min_size(H, W, num_labels, min_size_factor=0.25):
    """min_size of the connectivity pass: floor(min_size_factor * ((H W) // N)), at least 1."""
    return max(1, int(float(min_size_factor) * ((int(H) * int(W)) // int(num_labels))))


def slic_segment(tiles_u8, num_components, compactness=10, iters=10, out=None, chunk=None, enforce_connectivity=False,
                 min_size_factor=0.25):
    """SLIC superpixels on the device (csrc/slic.hip): tiles_u8 [n, H, W, 3] uint8 (device) ->
    (labels int16 [n, H, W] in [0, N), N).  The role of `fast_slic.Slic(num_components, compactness).iterate` in the
    reference's loader (data_loaders_MT_SP.py:303-304) - the same interface, an all-integer definition of its own, not
    bit parity.  The store is walked in chunks of `chunk` tiles (default: a workspace of about 256 MB); tiles are
    segmented independently, so the result does not depend on the chunking.  `out`: int16 [n, H, W] to fill.
    `enforce_connectivity`: run `slic_connect` over the maps in place with min_size = floor(min_size_factor * ((H W) // N)),
    at least 1 (0.25: fast_slic's default factor); off by default, and then the maps are those of the segmentation alone."""
    t = require_cuda(tiles_u8, "tiles_u8")
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or t.shape[0] < 1:
        raise RuntimeError("tiles_u8 must be uint8 [n, H, W, 3]")
    t = t.contiguous()
    n, H, W, _ = t.shape
    N = slic_num_labels(H, W, num_components)
    if not (0 <= int(compactness) <= 1024) or int(iters) < 1:
        raise ValueError("compactness must lie in 0..1024 and iters be at least 1")
    if enforce_connectivity and not float(min_size_factor) >= 0.0:
        raise ValueError("min_size_factor must not be negative")
    if out is None:
        out = torch.empty(n, H, W, device=t.device, dtype=torch.int16)
    elif tuple(out.shape) != (n, H, W) or out.dtype != torch.int16 or not out.is_contiguous() or out.device != t.device:
        raise RuntimeError("out must be a contiguous int16 [n, H, W] tensor on the tiles' device")
    if chunk is None:
        chunk = max(1, (256 << 20) // (4 * H * W))
    chunk = max(1, min(int(chunk), n))
    ws = torch.empty(lib().ph_slic_workspace_bytes(chunk, H, W, int(num_components)), device=t.device, dtype=torch.uint8)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        check(lib().ph_slic(ptr(t[lo:]), ptr(out[lo:]), m, H, W, int(num_components), int(compactness), int(iters), ptr(ws),
                            stream()), "ph_slic")
    if enforce_connectivity:
        slic_connect(out, N, slic_min_size(H, W, N, min_size_factor), out=out, chunk=chunk)
    return out, N


def rgb_to_lab8(rgb_u8):
    """The colour step of `slic_segment` on its own: uint8 [..., 3] sRGB (device) -> uint8 [..., 3] 8-bit CIELAB
    (L * 255 / 100, a + 128, b + 128)."""
    t = require_cuda(rgb_u8, "rgb_u8")
    if t.dtype != torch.uint8 or t.shape[-1] != 3 or t.numel() == 0:
        raise RuntimeError("rgb_u8 must be uint8 [..., 3]")
    t = t.contiguous()
    npix = t.numel() // 3
    words = torch.empty(npix, device=t.device, dtype=torch.int32)
    ws = torch.empty(lib().ph_slic_workspace_bytes(1, 1, 1, 1), device=t.device, dtype=torch.uint8)
    check(lib().ph_slic_lab(ptr(t), ptr(words), npix, ptr(ws), stream()), "ph_slic_lab")
    return words.view(torch.uint8).view(npix, 4)[:, :3].reshape(t.shape)


def superpixel_topk_mask(x_path_grad, sp_mask, path_k, num_superpixels=None, return_mean=False):
    """x_path_grad [B, C, H, W] float, sp_mask [B, H, W] integer labels -> [B, H, W] float mask of the `path_k`
    superpixels with the largest mean gradient (:77-93).  `num_superpixels` (labels are < it) avoids the device->host
    read of sp_mask.max() that F.one_hot does in the reference."""
    g = ops._f32(require_cuda(x_path_grad, "x_path_grad").detach()).contiguous()
    sp = sp_mask.to(g.device).long().contiguous()
    B, C, H, W = g.shape
    if tuple(sp.shape) != (B, H, W):
        raise RuntimeError("sp_mask must be [B, H, W]")
    N = int(num_superpixels) if num_superpixels is not None else int(sp.max().item()) + 1
    mask = torch.empty(B, H, W, device=g.device, dtype=torch.float32)
    mean = torch.empty(B, N, device=g.device, dtype=torch.float32) if return_mean else None
    check(lib().ph_superpixel_mask(ptr(g), ptr(sp), ptr(mask), ptr(mean), B, C, H, W, N, int(path_k), stream()),
          "ph_superpixel_mask")
    return (mask, mean) if return_mean else mask


def omic_topk_mask(x_omic_grad, omic_k):
    """x_omic_grad [B, D] -> float mask of the entries >= the omic_k-th largest of their row (:96)."""
    g = ops._f32(require_cuda(x_omic_grad, "x_omic_grad").detach()).contiguous()
    B, D = g.shape
    mask = torch.empty_like(g)
    check(lib().ph_topk_threshold_mask(ptr(g), ptr(mask), B, D, int(omic_k), stream()), "ph_topk_threshold_mask")
    return mask


def apply_mask(x, mask):
    """x * (1 - mask) with the mask broadcast over the channel axis (:201-202): x [B, C, H, W] with mask [B, H, W], or
    x [B, D] with mask [B, D]."""
    x = ops._f32(require_cuda(x, "x")).contiguous()
    mask = ops._f32(mask.to(x.device)).contiguous()
    B = x.shape[0]
    C = x.shape[1] if x.dim() == 4 else 1
    P = mask[0].numel()
    out = torch.empty_like(x)
    check(lib().ph_apply_mask(ptr(x), ptr(mask), ptr(out), B, C, P, stream()), "ph_apply_mask")
    return out


def masks_from_input_gradients(opt, x_path_grad, x_omic_grad, sp_mask, num_superpixels=None):
    """The tail of superpixel_attention_mask (:77-101): returns (x_path_super_mask, x_omic_super_mask), both float."""
    return (superpixel_topk_mask(x_path_grad, sp_mask, opt.Path_K, num_superpixels), omic_topk_mask(x_omic_grad, opt.Omic_K))


def superpixel_attention_mask(opt, optimizer, model, x_path, x_grph, x_omic, sp_mask, grade, device, num_superpixels=None):
    """The reference's function, same signature (:42-102): switch `model` to eval mode, take the gradient of the fused
    branch's NLL with respect to the image and the omic vector (eval-mode backward of the trunk down to the image:
    `ph_resnet_backward_input`), build the two masks, switch back to train mode.  Unlike the reference this does not
    leave the eval-mode cost's parameter gradients in `.grad` (the trainer zeroes them before its own backward)."""
    dev = torch.device(device)
    x_path_adv = ops._f32(x_path.detach().to(dev)).clone().requires_grad_(True)            # :46-49
    x_omic_adv = ops._f32(x_omic.detach().to(dev)).clone().requires_grad_(True)
    grade = grade.to(dev)
    model.eval()                                                                           # :62
    try:
        out = model(x_path=x_path_adv, x_grph=x_grph, x_omic=x_omic_adv)                  # :63
        pred = out[5]
        if not pred.requires_grad:
            raise RuntimeError("the fused prediction does not depend on the inputs (cut_fuse_grad?): the reference's "
                               "gradient hooks would never fire either")
        cost = ops.NLLFn.apply(pred, grade, float(pred.shape[0]))                          # :66
        x_path_grad, x_omic_grad = torch.autograd.grad(cost, [x_path_adv, x_omic_adv])     # :67-75
        masks = masks_from_input_gradients(opt, x_path_grad, x_omic_grad, sp_mask, num_superpixels)
    finally:
        model.train()                                                                      # :99
    return masks
