"""Network topology from a patch size and a spacing (reference experiment_planning/common_utils.py:50-155, 232-270): how often each
axis is pooled, the pooling and convolution kernel of every stage, and the patch size padded to what the poolings divide.

The plans these functions produce are compared with the reference's for equality, so every value is formed by the same numpy
and Python operations in the same order, including their types (`num_pool_per_axis` holds numpy integers from
`get_pool_and_conv_props_poolLateV2` and Python integers from `get_pool_and_conv_props`; `np.ceil` turns the running size into a
float).  All of it is host arithmetic on three numbers per axis."""
from copy import deepcopy

import numpy as np


def get_shape_must_be_divisible_by(net_numpool_per_axis):
    return 2 ** np.array(net_numpool_per_axis)


def pad_shape(shape, must_be_divisible_by):
    """`shape` rounded up, axis by axis, to a multiple of `must_be_divisible_by` -> int array."""
    if not isinstance(must_be_divisible_by, (tuple, list, np.ndarray)):
        must_be_divisible_by = [must_be_divisible_by] * len(shape)
    else:
        assert len(must_be_divisible_by) == len(shape)
    new_shp = []
    for s, m in zip(shape, must_be_divisible_by):
        up = s + m - s % m
        new_shp.append(up - m if s % m == 0 else up)
    return np.array(new_shp).astype(int)


def get_network_numpool(patch_size, maxpool_cap=999, min_feature_map_size=4):
    """floor(log2(edge / min_feature_map_size)) per axis, capped."""
    numpool = np.floor([np.log(i / min_feature_map_size) / np.log(2) for i in patch_size]).astype(int)
    return [min(i, maxpool_cap) for i in numpool]


def get_pool_and_conv_props_poolLateV2(patch_size, min_feature_map_size, max_numpool, spacing):
    """The base planner's rule: every axis is pooled as often as its edge allows, the axes with fewer poolings join LATE; an axis
    convolves with 1 until its spacing has come within a factor 2 of the coarsest spacing.
    -> num_pool_per_axis, pool kernels per stage, conv kernels per stage (+ the bottleneck's), padded patch size, divisors."""
    reach = max(deepcopy(spacing))
    dim = len(patch_size)
    num_pool_per_axis = get_network_numpool(patch_size, max_numpool, min_feature_map_size)
    pool_kernels, conv_kernels = [], []
    net_numpool = max(num_pool_per_axis)
    current_spacing = spacing
    for p in range(net_numpool):
        reached = [current_spacing[i] / reach > 0.5 for i in range(dim)]
        pool = [2 if num_pool_per_axis[i] + p >= net_numpool else 1 for i in range(dim)]
        conv = [3] * dim if all(reached) else [1 if reached[i] else 3 for i in range(dim)]
        pool_kernels.append(pool)
        conv_kernels.append(conv)
        current_spacing = [i * j for i, j in zip(current_spacing, pool)]
    conv_kernels.append([3] * dim)
    must_be_divisible_by = get_shape_must_be_divisible_by(num_pool_per_axis)
    return num_pool_per_axis, pool_kernels, conv_kernels, pad_shape(patch_size, must_be_divisible_by), must_be_divisible_by


def get_pool_and_conv_props(spacing, patch_size, min_feature_map_size, max_numpool):
    """The v2.1 rule: pooling follows the spacing.  Each round pools the axes whose spacing is within a factor 2 of the finest one
    and whose edge is still at least 2 * min_feature_map_size; the conv kernel is 3 on the largest group of axes whose spacings
    are within a factor 2 of one another and 1 elsewhere.  Same five results as above."""
    dim = len(spacing)
    current_spacing = deepcopy(list(spacing))
    current_size = deepcopy(list(patch_size))
    pool_kernels, conv_kernels = [], []
    num_pool_per_axis = [0] * dim
    while True:
        min_spacing = min(current_spacing)
        valid = [i for i in range(dim) if current_spacing[i] / min_spacing < 2]
        axes = []
        for a in range(dim):
            mine = current_spacing[a]
            partners = [i for i in range(dim) if current_spacing[i] / mine < 2 and mine / current_spacing[i] < 2]
            if len(partners) > len(axes):
                axes = partners
        conv = [3 if i in axes else 1 for i in range(dim)]
        valid = [i for i in valid if current_size[i] >= 2 * min_feature_map_size]
        valid = [i for i in valid if num_pool_per_axis[i] < max_numpool]
        if len(valid) == 0:
            break
        pool = [1] * dim
        for v in valid:
            pool[v] = 2
            num_pool_per_axis[v] += 1
            current_spacing[v] *= 2
            current_size[v] = np.ceil(current_size[v] / 2)
        pool_kernels.append(pool)
        conv_kernels.append(conv)
    must_be_divisible_by = get_shape_must_be_divisible_by(num_pool_per_axis)
    patch_size = pad_shape(patch_size, must_be_divisible_by)
    conv_kernels.append([3] * dim)
    return num_pool_per_axis, pool_kernels, conv_kernels, patch_size, must_be_divisible_by
