"""Cropping a case to its non-zero region ON THE DEVICE: `preprocessing/cropping.py` (reference preprocessing/cropping.py:23-116,
139-150) with the same names and signatures, on device tensors.  numpy inputs are uploaded; results stay on the device.

  create_nonzero_mask   `mt_nonzero_mask` (any channel != 0, numpy's rule on the bit pattern) + `mt_fill_holes3d`
                        (scipy.ndimage.binary_fill_holes with its default structure: the 6-connected background components that
                        touch no face of the volume are filled; the union-find labelling of `mt_cc_label3d` does the work);
  crop_to_nonzero       the two above, ONE device-to-host read of the seven box integers `mt_fill_holes3d` reduces, then
                        `mt_crop_nonzero`: data and segmentation of the box in one pass.

There is no CPU labelling here: without a HIP device every function raises (the host path is `cropping.py`).  The data must be
float32 (what `load_case_from_list_of_files` returns), a given seg float32 too."""
import numpy as np
import torch

from .. import ops
from .cropping import get_case_identifier, load_case_from_list_of_files  # noqa: F401  (same public names as cropping.py)


def _no_device():
    raise RuntimeError("multitalent_amd: cropping to the non-zero region runs on a HIP device only; there is no CPU fallback "
                       "(the host path is preprocessing/cropping.py)")


def _to_device(a, dtype=None):
    """numpy array or tensor -> contiguous device tensor (uploaded when it is not there yet); `dtype` is required, not converted to."""
    if torch.is_tensor(a):
        if not a.is_cuda:
            if not torch.cuda.is_available():
                _no_device()
            a = a.cuda()
    else:
        if not torch.cuda.is_available():
            _no_device()
        a = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if dtype is not None and a.dtype != dtype:
        raise TypeError("device cropping: %s expected, got %s" % (dtype, a.dtype))
    return a.contiguous()


def _filled_mask(data):
    """data: [C, D, H, W] float32 device tensor -> (uint8 mask [D, H, W] with the holes filled, int32 device tensor [7]: box + count)."""
    assert data.dim() == 4, "data must have shape (C, X, Y, Z)"
    ops.crop_check_shape(data.shape[1:])
    with torch.cuda.device(data.device):
        return ops.fill_holes3d(ops.nonzero_mask(data))


def create_nonzero_mask(data):
    """cropping.py:23-29 -> bool device tensor [D, H, W]."""
    assert len(data.shape) == 4, "data must have shape (C, X, Y, Z)"
    return _filled_mask(_to_device(data, torch.float32))[0].view(torch.bool)


def fill_holes(mask):
    """scipy.ndimage.binary_fill_holes(mask) for a 3-D volume with the default structure -> bool device tensor; `mask` is left as it is."""
    ops.crop_check_shape(mask.shape)
    m = _to_device(mask)
    with torch.cuda.device(m.device):
        return ops.fill_holes3d((m != 0).to(torch.uint8))[0].view(torch.bool)


def get_bbox_from_mask(mask, outside_value=0):
    """cropping.py:32-40 -> [[lo, hi], ...] of Python ints, hi exclusive; an empty mask raises ValueError like np.min of nothing."""
    m = _to_device(mask) != outside_value
    bbox = []
    for a in range(m.dim()):
        along = m.any(dim=tuple(i for i in range(m.dim()) if i != a)) if m.dim() > 1 else m
        idx = torch.nonzero(along).flatten()
        if idx.numel() == 0:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")
        bbox.append([int(idx[0]), int(idx[-1]) + 1])
    return bbox


def crop_to_bbox(image, bbox):
    return _to_device(image)[tuple(slice(b[0], b[1]) for b in bbox)]


def crop_to_nonzero(data, seg=None, nonzero_label=-1):
    """cropping.py:84-116 -> (data, seg, bbox): device tensors of the box (data float32 bit for bit; seg int64 without a given seg,
    float32 with one, as on the host path) and the box as [[lo, hi]] * 3 of Python ints.  An all-zero volume raises ValueError."""
    data = _to_device(data, torch.float32)
    seg = _to_device(seg, torch.float32) if seg is not None else None
    mask, box = _filled_mask(data)
    b = [int(i) for i in box.cpu()]                       # the one read-back of the case
    if b[6] == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")     # the host's np.min of nothing
    with torch.cuda.device(data.device):
        out, seg_out = ops.crop_nonzero(data, mask, b[:6], seg, nonzero_label)
    if seg is None:
        seg_out = seg_out.to(torch.int64)                 # the host's mask.astype(int)
    return out, seg_out, [[b[0], b[1]], [b[2], b[3]], [b[4], b[5]]]


class ImageCropper(object):
    @staticmethod
    def crop(data, properties, seg=None):
        data, seg, bbox = crop_to_nonzero(data, seg, nonzero_label=-1)                # cropping.py:139-150
        properties["crop_bbox"] = bbox
        # np.unique(seg), int64 or (with a seg file) float32: the device reduces the volume to its distinct BIT PATTERNS, numpy
        # applies its own rules for -0.0 and NaN to those few values
        u = torch.unique(seg.view(torch.int32) if seg.dtype == torch.float32 else seg).cpu().numpy()
        properties['classes'] = np.unique(u.view(np.float32) if seg.dtype == torch.float32 else u)
        seg.masked_fill_(seg < -1, 0)
        properties["size_after_cropping"] = tuple(int(i) for i in data[0].shape)
        return data, seg, properties

    @staticmethod
    def crop_from_list_of_files(data_files, seg_file=None):
        data, seg, properties = load_case_from_list_of_files(data_files, seg_file)
        return ImageCropper.crop(data, properties, seg)
