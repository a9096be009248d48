"""`iou3d_cuda` -- the pybind module of mmdet3d/ops/iou3d (src/iou3d.cpp:44-232), on the C ABI,
with the reference's argument lists and in-place outputs:

    boxes_overlap_bev_gpu(boxes_a, boxes_b, ans_overlap)
    boxes_iou_bev_gpu(boxes_a, boxes_b, ans_iou)
    nms_gpu(boxes, keep, nms_overlap_thresh, device_id) -> num_out
    nms_normal_gpu(boxes, keep, nms_overlap_thresh, device_id) -> num_out

`boxes` of the two NMS calls are already sorted by the caller (iou3d_utils.nms_gpu does that)
and `keep` is a CPU long tensor, as in the reference; the count these two return is the one
host read on this path.  The mask and its reduction stay on the device.
"""
import torch

from .. import kernels as K


def _check_input(**ts):
    for name, t in ts.items():
        if not t.is_cuda:
            raise RuntimeError("%s must be a CUDAtensor" % name)
        if not t.is_contiguous():
            raise RuntimeError("%s must be contiguous" % name)


def boxes_overlap_bev_gpu(boxes_a, boxes_b, ans_overlap):
    """iou3d.cpp:50-71: ans_overlap[M, N] <- overlap areas of (M, 5) x (N, 5) xyxyr boxes."""
    _check_input(boxes_a=boxes_a, boxes_b=boxes_b, ans_overlap=ans_overlap)
    with torch.cuda.device(boxes_a.device):
        ans_overlap.copy_(K.boxes_overlap_bev(boxes_a, boxes_b))
    return 1


def boxes_iou_bev_gpu(boxes_a, boxes_b, ans_iou):
    """iou3d.cpp:73-93: ans_iou[M, N] <- BEV IoU."""
    _check_input(boxes_a=boxes_a, boxes_b=boxes_b, ans_iou=ans_iou)
    with torch.cuda.device(boxes_a.device):
        ans_iou.copy_(K.boxes_iou_bev(boxes_a, boxes_b))
    return 1


def _nms(kind, boxes, keep, thresh, device_id):
    _check_input(boxes=boxes)
    if keep.is_cuda or keep.dtype != torch.long or not keep.is_contiguous():
        raise RuntimeError("keep must be a contiguous CPU long tensor")
    n = boxes.shape[0]
    if keep.numel() < n:
        raise RuntimeError("keep holds %d entries for %d boxes" % (keep.numel(), n))
    with torch.cuda.device(device_id):
        offsets = torch.tensor([0, n], dtype=torch.int32).to(boxes.device, non_blocking=True)
        th = torch.full((1,), float(thresh), dtype=torch.float32, device=boxes.device)
        kept, num = K.nms_segments(kind, boxes.float().contiguous(), offsets, th, n)
        num_out = int(num[0])
        keep[:num_out] = kept[0, :num_out].cpu()
    return num_out


def nms_gpu(boxes, keep, nms_overlap_thresh, device_id):
    """iou3d.cpp:95-147: rotated NMS of sorted (N, 5) xyxyr boxes; keep[:num_out] <- kept rows."""
    return _nms("rotate", boxes, keep, nms_overlap_thresh, device_id)


def nms_normal_gpu(boxes, keep, nms_overlap_thresh, device_id):
    """iou3d.cpp:149-201: the same with the axis-aligned IoU of (x1, y1, x2, y2)."""
    return _nms("normal", boxes, keep, nms_overlap_thresh, device_id)
