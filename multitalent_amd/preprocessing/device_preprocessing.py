"""Pre-processing on the device: resampling a cropped volume and its label map to the plan's spacing, the
intensity normalisation schemes and the sampled class locations — GenericPreprocessor.resample_and_normalize and _run_internal
(preprocessing.py:226-353) with resample_patient / resample_data_or_seg (preprocessing.py:38-197).

Data (order 3, separate z with order 0): skimage.transform.resize(order=3, mode='edge', anti_aliasing=False) is
scipy.ndimage.zoom(order=3, mode='nearest', grid_mode=True): the volume is edge-padded by 12 voxels, spline-prefiltered and
sampled at x = (o + 0.5) * in/out - 0.5.  Here: replicate padding (torch glue), `mt_spline_prefilter3`, `mt_affine_sample` (cubic,
diagonal matrix).  The prefilter initialises with mirror boundaries where scipy uses its 'nearest' rule; twelve voxels of edge
padding damp the difference to z^12 = 1.4e-7.
Labels (order 1, separate z with order 0): batchgenerators' resize_segmentation — per label the order-1 resize of its indicator,
ascending labels overwrite where it reaches 0.5 — is `mt_affine_sample` mode 11 on a volume edge-padded by one voxel.
Normalisation: `mt_masked_moments` (per-case mean / sd in double) and `mt_intensity_normalize` (one fused in-place pass).
Class locations: `mt_label_counts` / `mt_label_locations`; the host draws the reference's random ranks, the device resolves them.
Other orders (`resample_data_or_seg`, `resample_patient`: data at order 0, 1, 3 with order_z 0, 1, 3; labels at order 0, 1 with order_z
0, 1 — what GenericPreprocessor_linearResampling and Preprocessor3DDifferentResampling ask for) run on the resize unit, csrc/resize.hip:
`mt_resize_prefilter3` (scipy's 'nearest' edge rule in closed form, no padded copy), `mt_resize` (one order per axis, the
anisotropic axis addressed by its stride), `mt_resize_labels`, `mt_resize_labels_axis`.  `resample_data` / `resample_seg` above keep
their launches.
The crop to the non-zero region in front of this is `device_cropping.py` (also on the device); file I/O stays with the caller."""
import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..inference.segmentation_export import get_do_separate_z, get_lowres_axis
from ..training.data_augmentation.spatial import affine_sample

NPAD = 12


def _zoom3(x, new_shape, planar):
    """x: [1, C, D, H, W] device tensor -> [1, C, *new_shape]; planar: per-slice 2D resize (new_shape[0] == D)."""
    D, H, W = (int(i) for i in x.shape[2:])
    pad = (NPAD, NPAD, NPAD, NPAD, 0, 0) if planar else (NPAD,) * 6
    xp = F.pad(x, pad, mode='replicate')
    m = np.zeros((1, 12), dtype=np.float32)
    sc = [1.0 if planar else D / new_shape[0], H / new_shape[1], W / new_shape[2]]
    m[0, 0], m[0, 4], m[0, 8] = sc
    m[0, 9:] = [0 if planar else D / 2. - 0.5 + NPAD, H / 2. - 0.5 + NPAD, W / 2. - 0.5 + NPAD]
    return affine_sample(xp, m, tuple(int(i) for i in new_shape), 3, cval=0.0, planar=planar)


def resample_data(data, new_shape, axis=None, do_separate_z=False):
    """resample_data_or_seg(data, new_shape, is_seg=False, axis, order=3, do_separate_z, order_z=0) for a [C, X, Y, Z] volume."""
    assert data.is_cuda and data.dim() == 4
    shape = tuple(int(i) for i in data.shape[1:])
    new_shape = tuple(int(i) for i in new_shape)
    if shape == new_shape:
        return data
    x = data.float()
    if not do_separate_z:
        return _zoom3(x[None].contiguous(), new_shape, planar=False)[0]
    assert len(axis) == 1, "only one anisotropic axis supported"
    ax = int(axis[0])
    perm = [0, 1 + ax] + [1 + i for i in range(3) if i != ax]                 # anisotropic axis first: slices
    inv = [perm.index(i) for i in range(4)]
    xs = x.permute(perm).contiguous()
    ns = [new_shape[ax]] + [new_shape[i] for i in range(3) if i != ax]
    out = _zoom3(xs[None], (xs.shape[1], ns[1], ns[2]), planar=True)[0]        # order 3 in-plane, slice by slice
    if xs.shape[1] != ns[0]:                                                  # order 0 along the anisotropic axis
        o = torch.arange(ns[0], device=x.device, dtype=torch.float64)
        idx = torch.floor((o + 0.5) * (xs.shape[1] / ns[0]) - 0.5 + 0.5).clamp_(0, xs.shape[1] - 1).long()
        out = out.index_select(1, idx)
    return out.permute(inv).contiguous()


def resampling_plan(shape, original_spacing, target_spacing, force_separate_z=None, separate_z_anisotropy_threshold=3):
    """resample_patient's decisions (preprocessing.py:67-95): -> (new_shape, do_separate_z, axis)."""
    shape = np.array(shape)
    new_shape = np.round(((np.array(original_spacing) / np.array(target_spacing)).astype(float) * shape)).astype(int)
    if force_separate_z is not None:
        sep, axis = force_separate_z, (get_lowres_axis(original_spacing) if force_separate_z else None)
    elif get_do_separate_z(original_spacing, separate_z_anisotropy_threshold):
        sep, axis = True, get_lowres_axis(original_spacing)
    elif get_do_separate_z(target_spacing, separate_z_anisotropy_threshold):
        sep, axis = True, get_lowres_axis(target_spacing)
    else:
        sep, axis = False, None
    if axis is not None and len(axis) != 1:
        sep = False
    return new_shape, sep, axis


def _resize_stage(x, out_shape, order, is_seg):
    """One resize_fn call of the reference over the axes of x [C, X, Y, Z] (float32, contiguous) that change: skimage's resize at
    `order` for data and for labels at order 0, batchgenerators' resize_segmentation for labels at order 1."""
    if tuple(x.shape[1:]) == tuple(out_shape):
        return x
    if is_seg and order == 1:
        return ops.resize_labels(x, out_shape)
    axes = sum(1 << (2 - a) for a in range(3) if order == 3 and x.shape[1 + a] != out_shape[a])        # mask: bit 0 is the last axis
    return ops.resize(ops.resize_prefilter3(x, axes) if axes else x, out_shape, (order,) * 3)


def resample_data_or_seg(data, new_shape, is_seg, axis=None, order=3, do_separate_z=False, order_z=0):
    """The reference's resample_data_or_seg (preprocessing.py:109-197) for a [C, X, Y, Z] device tensor, on the resize unit
    (csrc/resize.hip).  Data: order 0, 1 or 3 with order_z 0, 1 or 3 (skimage's resize as scipy.ndimage.zoom(mode='nearest',
    grid_mode=True), the z pass as map_coordinates(mode='nearest')).  Labels: order 0 or 1 (resize_segmentation) with order_z 0 or 1
    (per label, strictly above one half); a label order of 3 is not on this path.  With do_separate_z every slice across `axis` is
    resized on its own, whichever of the three axes that is (addressed by strides, nothing is permuted), then the axis is resampled
    with order_z; the intermediate is float32, which for float32 input is the reference's own rounding.  The result has the dtype
    of the input; an input that already has `new_shape` is returned as it is."""
    if not torch.is_tensor(data) or not data.is_cuda:
        raise RuntimeError("multitalent_amd: device pre-processing runs on a HIP device only; there is no CPU fallback")
    assert data.dim() == 4, "data must be (c, x, y, z)"
    assert len(new_shape) == data.dim() - 1
    order, order_z = int(order), int(order_z)
    if is_seg:
        if order not in (0, 1) or order_z not in (0, 1):
            raise NotImplementedError("label maps are resampled with order 0 or 1 (order_z 0 or 1) on this path, got order %d / order_z %d"
                                      % (order, order_z))
    elif order not in ops.RESIZE_ORDERS or order_z not in ops.RESIZE_ORDERS:
        raise NotImplementedError("data is resampled with order 0, 1 or 3 on this path, got order %d / order_z %d" % (order, order_z))
    shape = tuple(int(i) for i in data.shape[1:])
    new_shape = tuple(int(i) for i in new_shape)
    if shape == new_shape:
        return data
    x = data.float().contiguous()
    if do_separate_z:
        assert len(axis) == 1, "only one anisotropic axis supported"
        ax = int(axis[0])
        mid = tuple(shape[a] if a == ax else new_shape[a] for a in range(3))
        out = _resize_stage(x, mid, order, is_seg)
        if shape[ax] != new_shape[ax]:
            if is_seg and order_z != 0:
                out = ops.resize_labels_axis(out, ax, new_shape[ax])
            else:
                if order_z == 3:
                    out = ops.resize_prefilter3(out, 1 << (2 - ax), out=None if out is x else out)
                out = ops.resize(out, new_shape, tuple(order_z if a == ax else 0 for a in range(3)))
    else:
        out = _resize_stage(x, new_shape, order, is_seg)
    return out.to(data.dtype)


def resample_patient(data, seg, original_spacing, target_spacing, order_data=3, order_seg=0, force_separate_z=False,
                     order_z_data=0, order_z_seg=0, separate_z_anisotropy_threshold=3):
    """The reference's resample_patient (preprocessing.py:38-106) for device tensors [C, X, Y, Z] (either may be None):
    -> (data, seg) at round(original_spacing / target_spacing * shape).  force_separate_z: None decides by the anisotropy of the
    spacings, True / False forces it."""
    assert not ((data is None) and (seg is None))
    if data is not None:
        assert data.dim() == 4, "data must be c x y z"
    if seg is not None:
        assert seg.dim() == 4, "seg must be c x y z"
    shape = (data if data is not None else seg).shape[1:]
    new_shape, sep, axis = resampling_plan(shape, original_spacing, target_spacing, force_separate_z, separate_z_anisotropy_threshold)
    data_reshaped = resample_data_or_seg(data, new_shape, False, axis, order_data, sep, order_z=order_z_data) if data is not None else None
    seg_reshaped = resample_data_or_seg(seg, new_shape, True, axis, order_seg, sep, order_z=order_z_seg) if seg is not None else None
    return data_reshaped, seg_reshaped


def _to_device(x):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("multitalent_amd: device pre-processing runs on a HIP device only; there is no CPU fallback")
        x = x.cuda()
    return x


def resample_and_normalize_ct(data, original_spacing, target_spacing, intensityproperties, force_separate_z=None,
                              separate_z_anisotropy_threshold=3):
    """data: [C, X, Y, Z] (already cropped and transposed) numpy or device tensor; every modality is normalised with the "CT"
    scheme (clip to the training set's 0.5 / 99.5 percentiles, subtract its mean, divide by its sd).  Returns a device tensor."""
    data = _to_device(data)
    data = torch.nan_to_num(data.float(), nan=0.0, posinf=None, neginf=None) if torch.isnan(data).any() else data.float()
    new_shape, sep, axis = resampling_plan(data.shape[1:], original_spacing, target_spacing, force_separate_z,
                                           separate_z_anisotropy_threshold)
    out = resample_data(data, new_shape, axis, sep)
    if out is data:
        out = data.clone()
    for c in range(out.shape[0]):
        ip = intensityproperties[c]
        out[c].clamp_(float(ip['percentile_00_5']), float(ip['percentile_99_5'])).sub_(float(ip['mean'])).div_(float(ip['sd']))
    return out


def _zoom_seg(x, new_shape, planar):
    """x: [1, C, D, H, W] label maps -> [1, C, *new_shape] by the per-label order-1 rule; one voxel of edge padding keeps every
    sampling coordinate (o + 0.5) * in/out - 0.5 >= -0.5 inside the padded volume (the reference's mode='edge')."""
    D, H, W = (int(i) for i in x.shape[2:])
    xp = F.pad(x, (1, 1, 1, 1, 0, 0) if planar else (1,) * 6, mode='replicate')
    m = np.zeros((1, 12), dtype=np.float32)
    m[0, 0], m[0, 4], m[0, 8] = 1.0 if planar else D / new_shape[0], H / new_shape[1], W / new_shape[2]
    m[0, 9:] = [0 if planar else D / 2. - 0.5 + 1, H / 2. - 0.5 + 1, W / 2. - 0.5 + 1]
    return affine_sample(xp, m, tuple(int(i) for i in new_shape), 1, cval=0.0, is_seg=True, planar=planar)


def resample_seg(seg, new_shape, axis=None, do_separate_z=False):
    """resample_data_or_seg(seg, new_shape, is_seg=True, axis, order=1, do_separate_z, order_z=0) for a [C, X, Y, Z] label map:
    result 0, then the labels in ascending order overwrite where the order-1 interpolation of their indicator is >= 0.5 (so -1
    stays only where no label >= 0 reaches 0.5); with separate z that rule per slice, then order 0 along the anisotropic axis."""
    if not seg.is_cuda:
        raise RuntimeError("multitalent_amd: device pre-processing runs on a HIP device only; there is no CPU fallback")
    assert seg.dim() == 4
    shape = tuple(int(i) for i in seg.shape[1:])
    new_shape = tuple(int(i) for i in new_shape)
    if shape == new_shape:
        return seg
    x = seg.float()
    if not do_separate_z:
        return _zoom_seg(x[None].contiguous(), new_shape, planar=False)[0]
    assert len(axis) == 1, "only one anisotropic axis supported"
    ax = int(axis[0])
    perm = [0, 1 + ax] + [1 + i for i in range(3) if i != ax]
    inv = [perm.index(i) for i in range(4)]
    xs = x.permute(perm).contiguous()
    ns = [new_shape[ax]] + [new_shape[i] for i in range(3) if i != ax]
    out = xs if tuple(xs.shape[2:]) == (ns[1], ns[2]) else _zoom_seg(xs[None], (xs.shape[1], ns[1], ns[2]), planar=True)[0]
    if xs.shape[1] != ns[0]:
        o = torch.arange(ns[0], device=x.device, dtype=torch.float64)
        idx = torch.floor((o + 0.5) * (xs.shape[1] / ns[0]) - 0.5 + 0.5).clamp_(0, xs.shape[1] - 1).long()
        out = out.index_select(1, idx)
    return out.permute(inv).contiguous()


def normalize(data, seg, schemes, use_mask, intensityproperties):
    """The normalisation loop of resample_and_normalize (preprocessing.py:273-310), in place on the [C, X, Y, Z] float32 device
    tensor `data`; seg: [Cs, X, Y, Z] float32 (its last channel carries the -1 of the non-zero mask) or None when no modality uses
    the mask.  schemes / use_mask: per modality.  The per-case means and sds are formed in double on the device (the reference
    takes them in float32) and never visit the host."""
    assert data.is_cuda and data.dtype == torch.float32 and data.is_contiguous() and data.dim() == 4
    assert len(schemes) == len(data), "self.normalization_scheme_per_modality must have as many entries as data has modalities"
    assert len(use_mask) == len(data), "self.use_nonzero_mask must have as many entries as data has modalities"
    m = None
    if any(use_mask):
        assert seg is not None, "use_mask_for_norm needs the segmentation (its -1 marks the region outside the non-zero mask)"
        m = seg[-1].float().contiguous()
        assert tuple(m.shape) == tuple(data.shape[1:])
    for c, scheme in enumerate(schemes):
        mc = m if use_mask[c] else None
        if scheme in ("CT", "CT2"):
            assert intensityproperties is not None, "ERROR: if there is a CT then we need intensity properties"
            ip = intensityproperties[c]
            lo, hi = float(ip['percentile_00_5']), float(ip['percentile_99_5'])
            if scheme == "CT":
                ops.intensity_normalize(data[c], (lo, hi), float(ip['mean']), float(ip['sd']), seg=mc)
            else:
                st = ops.masked_moments(data[c:c + 1], ops.MOMENTS_OPEN_RANGE, lo=[lo], hi=[hi])
                ops.intensity_normalize(data[c], (lo, hi), stats=st[0], seg=mc)
        elif scheme == 'noNorm':
            pass
        elif mc is not None:
            st = ops.masked_moments(data[c:c + 1], ops.MOMENTS_SEG_GE0, seg=mc)
            ops.intensity_normalize(data[c], stats=st[0], eps=1e-8, seg=mc)
        else:
            st = ops.masked_moments(data[c:c + 1], ops.MOMENTS_ALL)
            ops.intensity_normalize(data[c], stats=st[0], eps=1e-8)
    return data


NUM_LOCATION_SAMPLES = 10000
MIN_PERCENT_COVERAGE = 0.01


def draw_class_ranks(counts, seed=1234):
    """The random stream of _run_internal (preprocessing.py:338-351) on the voxel counts alone: one RandomState(seed) per case,
    classes visited in order, an empty class draws nothing.  -> per class the drawn ranks into np.argwhere(seg == c), or None."""
    rndst = np.random.RandomState(seed)
    ranks = []
    for n in counts:
        n = int(n)
        if n == 0:
            ranks.append(None)
            continue
        k = max(min(NUM_LOCATION_SAMPLES, n), int(np.ceil(n * MIN_PERCENT_COVERAGE)))
        ranks.append(rndst.choice(n, k, replace=False))
    return ranks


def class_locations(seg, all_classes):
    """properties['class_locations'] of _run_internal for the [X, Y, Z] float32 device label map `seg`: {c: int64 [k, 3] numpy array
    of sampled voxel coordinates, or [] for a class without voxels}, element for element the reference's.  The counts come back
    from the device, the host draws the ranks, the device resolves them to coordinates."""
    all_classes = list(all_classes)
    if len(all_classes) == 0:
        return {}
    counts_dev, index = ops.label_counts(seg.contiguous(), all_classes)
    counts = counts_dev.cpu().numpy()
    ranks = draw_class_ranks(counts)
    drawn = [(i, r) for i, r in enumerate(ranks) if r is not None]
    locs = {}
    if drawn:
        qslot = np.concatenate([np.full(len(r), i, dtype=np.int32) for i, r in drawn])
        qrank = np.concatenate([r.astype(np.int64) for _, r in drawn])
        out = ops.label_locations(index, qslot, qrank, total=int(counts.sum())).cpu().numpy()
        assert out.min() >= 0, "class_locations: a rank fell outside its class (counts and label map disagree)"
        pos = 0
        for i, r in drawn:
            locs[i] = out[pos:pos + len(r)]
            pos += len(r)
    return {c: (locs[i] if i in locs else []) for i, c in enumerate(all_classes)}
