"""Shared by the dataset-conversion tests (not a test module): the golden data of tools/oracle_gen/make_golden_dataset_conversion.py
and a numpy restatement of what one voxel of `copy_and_convert_segmentation` becomes."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = ('uint8', 'int8', 'int16', 'uint16', 'int32', 'uint32', 'float32', 'float64')
SLOTS, UNLISTED = 1023, 0xffff


def golden():
    with open(os.path.join(HERE, 'golden', 'dataset_conversion.json')) as f:
        return json.load(f), np.load(os.path.join(HERE, 'golden', 'dataset_conversion.npz'))


def pairs(labels_in, labels_out):
    """[(input label, output)] in the order the reference assigns them."""
    return [(int(ii), int(o)) for i, o in zip(labels_in, labels_out) for ii in (i if hasattr(i, '__len__') else (i,))]


def np_table(labels_in, labels_out):
    t = np.full(SLOTS, UNLISTED, dtype=np.uint16)
    for ii, o in pairs(labels_in, labels_out):
        if ii > 0:
            t[ii] = o
    return t


def np_convert(vol, labels_in, labels_out):
    """-> (uint8 volume, number of unexpected voxels, the smallest unexpected value or None).  vol is widened to float64, which is
    exact for every stored type; a voxel counts only above 1e-20 (NaN does not), later pairs overwrite earlier ones."""
    v = np.asarray(vol).astype(np.float64)
    with np.errstate(invalid='ignore'):
        positive = v > 1e-20
    out = np.zeros(v.shape, dtype=np.uint8)
    listed = np.zeros(v.shape, dtype=bool)
    for ii, o in pairs(labels_in, labels_out):
        m = positive & (v == ii)
        out[m] = o
        listed |= m
    unexpected = positive & ~listed
    n = int(unexpected.sum())
    return out, n, (float(v[unexpected].min()) if n else None)


def np_slot(values):
    """mt_label_slot of csrc/label_class.h: -1 zero, -2 unexpected, else the table slot."""
    v = np.asarray(values).astype(np.float64)
    with np.errstate(invalid='ignore'):
        positive = v > 1e-20
        integral = positive & (v <= SLOTS - 1) & (np.floor(v) == v)
    slot = np.where(positive, -2, -1).astype(np.int32)
    slot[integral] = v[integral].astype(np.int32)
    return slot
