"""Golden vectors for cropping to the non-zero region: the REAL reference's nnunet/preprocessing/cropping.py `crop_to_nonzero`
(:84-116, with create_nonzero_mask / get_bbox_from_mask / crop_to_bbox underneath) run on CPU in the build container on small
seeded volumes.  Nothing is substituted besides the import shim for the third-party packages this image lacks (the function
itself needs numpy and scipy only).

Cases (all <= 40 x 48 x 56): one and two channels, with and without a float32 seg, interior holes, a cavity open to a face of the
volume, a shell whose only leak is diagonal, a zero border on every side / on one side / on none, and NaN, +-inf, -0.0 and
denormal voxels (in data and seg).  Per case: data, seg (dtype kept; absent without one), and the reference's outputs out_data,
out_seg (dtype kept: int64 without a seg, float32 with one), bbox.  Intensities are small integers (plus the special values) so
that the file compresses.

Writes tests/golden/cropping.npz.  Run: python tools/oracle_gen/make_golden_cropping.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_import
ref_import.install()

from nnunet.preprocessing.cropping import crop_to_nonzero                         # the reference itself


def ellipsoid(shape, centre, radii):
    g = np.ogrid[tuple(slice(0, s) for s in shape)]
    return sum(((g[a] - centre[a]) / radii[a]) ** 2 for a in range(3)) <= 1


def body(rng, shape, margin, zero_frac):
    """an elliptic body of integer intensities with `zero_frac` zero voxels inside it, `margin` zero voxels around it"""
    c = [(s - 1) / 2 for s in shape]
    r = [max((s - 1) / 2 - m, 0.5) for s, m in zip(shape, margin)]
    inside = ellipsoid(shape, c, r)
    v = rng.integers(-900, 900, shape).astype(np.float32)
    v[v == 0] = 7
    v[rng.random(shape) < zero_frac] = 0
    v[~inside] = 0
    return v


def shell(shape, lo, hi):
    """a one-voxel box shell between the corners lo and hi (inclusive)"""
    m = np.zeros(shape, bool)
    m[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
    m[lo[0] + 1:hi[0], lo[1] + 1:hi[1], lo[2] + 1:hi[2]] = False
    return m


def seg_for(rng, data, classes=4):
    s = rng.integers(0, classes, data.shape[1:]).astype(np.float32)
    s[rng.random(s.shape) < 0.5] = 0
    return s[None]


def make_cases():
    rng = np.random.default_rng(20240607)
    cases = {}
    # 1: one channel, holes inside the body, a zero border on every side, no seg
    cases['holes_border'] = (body(rng, (24, 30, 28), (3, 4, 2), 0.05)[None], None)
    # 2: two channels (the second shifted, so the union matters), float32 seg
    a, b = body(rng, (20, 26, 33), (2, 3, 5), 0.3), np.roll(body(rng, (20, 26, 33), (4, 3, 5), 0.3), 2, axis=2)
    d = np.stack([a, b])
    cases['two_channels_seg'] = (d, seg_for(rng, d))
    # 3: a shell with a closed cavity, a second one whose cavity has a face-connected channel to the outside, and a third that
    #    touches the volume's face so that its cavity is open there
    m = shell((30, 40, 36), (3, 4, 5), (12, 15, 16)) | shell((30, 40, 36), (15, 20, 4), (26, 33, 15))
    m[20, 33, 9] = False                                                          # the channel
    m |= shell((30, 40, 36), (4, 5, 22), (13, 18, 35 + 1))                        # open at w = 35
    cases['cavities'] = ((m * 5.0).astype(np.float32)[None], None)
    # 4: non-zero on every face (the box is the whole volume), interior holes, seg
    d = rng.integers(1, 50, (1, 17, 19, 23)).astype(np.float32)
    d[0, 3:9, 4:11, 5:14][rng.random((6, 7, 9)) < 0.6] = 0
    cases['no_border_seg'] = (d, seg_for(rng, d))
    # 5: special values.  NaN, +-inf and a denormal are non-zero, -0.0 is zero; the same in the seg's `== 0`
    d = np.zeros((2, 12, 14, 18), np.float32)
    d[0, 3:9, 4:10, 5:13] = rng.integers(1, 9, (6, 6, 8))
    d[0, 4:8, 5:9, 6:12] = -0.0                                                   # a cavity of negative zeros: filled
    d[0, 1, 7, 7] = np.nan
    d[1, 10, 2, 3] = np.float32(1e-45)
    d[1, 6, 12, 16] = np.inf
    d[0, 6, 1, 1] = -np.inf
    d[1, 0, 0, 0] = -0.0
    d[0, 5, 6, 8] = np.nan                                                        # inside the cavity
    s = seg_for(rng, d, 3)
    s[0, 2, 3, 4], s[0, 1, 1, 1], s[0, 10, 12, 16] = -0.0, np.nan, np.float32(1e-45)
    cases['special_values_seg'] = (d, s)
    # 6: the largest shape, 2 % zeros inside the body, no seg
    cases['large'] = (body(rng, (40, 48, 56), (5, 2, 7), 0.02)[None], None)
    # 7: a zero border on the low side of every axis only; seg
    d = np.zeros((1, 16, 21, 25), np.float32)
    d[0, 4:, 6:, 3:] = body(rng, (12, 15, 22), (0, 0, 0), 0.1)
    d[0, -1, -1, -1] = 3
    cases['low_border_seg'] = (d, seg_for(rng, d))
    # 8: a shell whose only leak is diagonal (an edge voxel removed: the cavity and the outside share no face there) - filled
    m = shell((14, 15, 16), (2, 2, 2), (10, 11, 12))
    m[2, 2, 5] = False
    cases['diagonal_leak'] = ((m * 2.0).astype(np.float32)[None], None)
    return cases


def main():
    out = {}
    names = []
    for name, (data, seg) in make_cases().items():
        assert data.dtype == np.float32 and max(data.shape[1:]) <= 56
        od, os_, bbox = crop_to_nonzero(data.copy(), None if seg is None else seg.copy(), nonzero_label=-1)
        names.append(name)
        out[name + '/data'] = data
        if seg is not None:
            out[name + '/seg'] = seg
        out[name + '/out_data'] = np.ascontiguousarray(od)
        out[name + '/out_seg'] = np.ascontiguousarray(os_)
        out[name + '/bbox'] = np.asarray(bbox, dtype=np.int64)
        print(name, data.shape, 'seg' if seg is not None else 'no seg', '->', bbox, os_.dtype, np.unique(os_)[:6])
    out['names'] = np.array(names)
    path = os.path.join(ROOT, 'tests', 'golden', 'cropping.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
