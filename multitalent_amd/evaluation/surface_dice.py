"""`normalized_surface_dice` with the reference's signature (reference evaluation/surface_dice.py:20-56) on the device path of
evaluation/evaluator.py: borders by erosion, exact distances to the other border (`mt_surface_distances`), the distances within the
tolerance counted where they lie (`mt_sd_count_within`), the reference's formula on the two integers that come back.

As the reference's docstring says of itself, this is NOT the surface Dice of the official surface-distance package (area-weighted
surface elements); the two are not comparable.

Differences from the reference: 3-D volumes only; an empty or full mask gives NaN (the reference raises inside medpy); without a
HIP device it raises, there is no host path."""
import numpy as np

from .evaluator import NSD_METRIC, evaluate_case


def _mask(x):
    """non-zero -> 1: a uint8 numpy array, or a uint8 tensor where x is a tensor"""
    try:
        import torch
        if torch.is_tensor(x):
            return (x != 0).to(torch.uint8)
    except ImportError:
        pass
    return (np.asarray(x) != 0).astype(np.uint8)


def normalized_surface_dice(a, b, threshold, spacing=None, connectivity=1):
    """a, b: volumes [z, y, x] of one shape, numpy arrays or device tensors of any integer or bool type; non-zero is the mask.
    threshold: the tolerance in mm (a distance equal to it counts); spacing: mm per voxel along (z, y, x), None = 1 mm;
    connectivity: 1..3 of the erosion structure.  Symmetric in a and b up to the rounding of one float64 sum."""
    assert tuple(a.shape) == tuple(b.shape), "a and b must have the same shape. a.shape= %s, b.shape= %s" % (tuple(a.shape),
                                                                                                             tuple(b.shape))
    res = evaluate_case(_mask(a), _mask(b), [1], advanced=True, advanced_metrics=[NSD_METRIC], voxel_spacing=spacing,
                        connectivity=connectivity, nsd_threshold=threshold)
    return res['1'][NSD_METRIC]
