"""Golden vectors for the training-case pre-processing on the device: the REAL reference's GenericPreprocessor._run_internal
(preprocessing.py:323-359) on small synthetic cropped cases, with skimage.transform.resize substituted by the delegate it has used
since skimage 0.19 (scipy.ndimage.zoom(order, mode='nearest', grid_mode=True)) and batchgenerators' resize_segmentation (third
party, absent here) restated from its published algorithm.  Writes tests/golden/train_preprocess.npz: per case the cropped input,
the written `data` array, the class locations, the "fragile" voxels of the label resampling (some label's interpolated one-hot
weight within 1e-4 of 0.5: the float32 weights of the device may fall on the other side there), and, for the per-case schemes,
the same output with float64 moments together with the reference's own deviation from it.
Run: python tools/oracle_gen/make_golden_train_preprocess.py"""
import io, os, pickle, sys, tempfile, zipfile
import numpy as np
from scipy import ndimage
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import
ref_import.install()
import nnunet.preprocessing.preprocessing as pre

FRAGILE_EPS = 1e-4
MAX_FRAGILE_SHARE = 0.10
_weights = []          # the resized indicator of every label of every label resample of the running case, in call order


def resize(img, shape, order, mode='edge', anti_aliasing=False, **kw):
    assert mode == 'edge' and not anti_aliasing
    img = np.asarray(img, dtype=float)
    return ndimage.zoom(img, [n / o for n, o in zip(shape, img.shape)], order=order, mode='nearest', grid_mode=True)


def resize_segmentation(segmentation, new_shape, order=3):
    """Restatement of batchgenerators.augmentations.utils.resize_segmentation (batchgenerators>=0.23): order 0 resizes the label
    map itself; otherwise every label's indicator is resized and the labels, in ascending order, overwrite where it is >= 0.5."""
    tpe = segmentation.dtype
    assert len(segmentation.shape) == len(new_shape), "new shape must have same dimensionality as segmentation"
    if order == 0:
        return resize(segmentation.astype(float), new_shape, order, mode="edge", clip=True, anti_aliasing=False).astype(tpe)
    reshaped = np.zeros(new_shape, dtype=segmentation.dtype)
    for c in np.unique(segmentation):
        w = resize((segmentation == c).astype(float), new_shape, order, mode="edge", clip=True, anti_aliasing=False)
        _weights.append(w)
        reshaped[w >= 0.5] = c
    return reshaped


pre.resize = resize
pre.resize_segmentation = resize_segmentation
pre.pickle = pickle

IP = {0: {'mean': 63.44, 'sd': 175.48, 'percentile_00_5': -927.0, 'percentile_99_5': 275.0},
      1: {'mean': -12.5, 'sd': 210.25, 'percentile_00_5': -640.0, 'percentile_99_5': 410.0}}
GEOM = {'iso_up': ((18, 22, 20), (1.5, 1.2, 1.2), (1.0, 0.8, 0.9)),
        'iso_down': ((24, 26, 22), (0.8, 0.8, 0.8), (1.5, 1.4, 1.3)),
        'sepz': ((7, 24, 22), (5.0, 0.9, 0.9), (2.5, 1.2, 1.2)),
        'sepz_same': ((9, 20, 18), (4.0, 0.7, 0.7), (4.0, 1.0, 1.0)),
        'identity': ((8, 9, 10), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))}
ALL_CLASSES = [1, 2, 3, 4, 5, 7]            # 7 never occurs; label 1 is the large class of `big`
# name, geometry, schemes per modality, use_mask_for_norm per modality.  Masked cases use geometries whose -1 / 0 border has no
# fragile voxel (asserted below).
CASES = [('iso_up_ct2_mask', 'iso_up', ['CT2'], [True]),
         ('iso_down_ct_zscore', 'iso_down', ['CT', 'nonCT'], [False, False]),
         ('sepz_ct_mask_ct2_mask', 'sepz', ['CT', 'CT2'], [True, True]),
         ('sepz_zscore_mask_nonorm_mask', 'sepz', ['nonCT', 'noNorm'], [True, True]),
         ('sepz_same_nonorm', 'sepz_same', ['noNorm'], [False]),
         ('identity_zscore_mask', 'identity', ['nonCT'], [True]),
         ('big_ct2', 'big', ['CT2'], [False])]
GEOM['big'] = ((26, 26, 26), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))       # 17576 voxels, label 1 on more than 10000 of them


def new_shape_of(shape, sp0, sp1):
    return np.round((np.array(sp0) / np.array(sp1)).astype(float) * np.array(shape)).astype(int)


def slab_width(n_in, n_out, from_end):
    """Smallest width >= 2 of a -1 slab whose border no output coordinate (o + 0.5) * in/out - 0.5 meets half-way."""
    x = (np.arange(n_out) + 0.5) * n_in / n_out - 0.5
    for w in range(2, 7):
        border = (n_in - w - 0.5) if from_end else (w - 0.5)
        if np.abs(x - border).min() > 1e-3:
            return w
    raise AssertionError((n_in, n_out))


def blocky_labels(rs, shape, new_shape, big):
    """Label map with labels -1..5 in blocks: -1 on two border slabs (the outside of the non-zero mask), 0 background, boxes of
    1..5 (label 1 fills most of the `big` case)."""
    seg = np.zeros(shape, dtype=np.float32)
    if big:
        seg[:] = 1
    for lab in ([2, 3, 4, 5] if big else [1, 2, 3, 4, 5]):
        for _ in range(2):
            lo = [rs.randint(0, max(1, n - 3)) for n in shape]
            sz = [rs.randint(2, max(3, n // (5 if big else 2))) for n in shape]
            seg[lo[0]:lo[0] + sz[0], lo[1]:lo[1] + sz[1], lo[2]:lo[2] + sz[2]] = lab
    seg[:, :slab_width(shape[1], new_shape[1], False), :] = -1
    seg[:, :, shape[2] - slab_width(shape[2], new_shape[2], True):] = -1
    return seg


def run_reference(name, data, seg, props, schemes, masks, sp1, float64_moments):
    g = pre.GenericPreprocessor({i: s for i, s in enumerate(schemes)}, {i: m for i, m in enumerate(masks)}, [0, 1, 2], IP)
    if float64_moments:
        # the same loop with the per-case moments in double: data[c] is float32, so widen it around the normalisation only
        orig = pre.resample_patient

        def widened(*a, **k):
            d, s = orig(*a, **k)
            return d.astype(np.float64), s
        pre.resample_patient = widened
    del _weights[:]
    try:
        with tempfile.TemporaryDirectory() as tmp:
            src, dst = os.path.join(tmp, 'cropped'), os.path.join(tmp, 'stage0')
            os.makedirs(src); os.makedirs(dst)
            np.savez_compressed(os.path.join(src, name + '.npz'), data=np.vstack((data, seg)))
            with open(os.path.join(src, name + '.pkl'), 'wb') as f:
                pickle.dump(props, f)
            with open(os.path.join(src, 'dataset_properties.pkl'), 'wb') as f:
                pickle.dump({'all_classes': ALL_CLASSES}, f)
            g._run_internal(np.array(sp1), name, dst, src, None, ALL_CLASSES)
            out = np.load(os.path.join(dst, name + '.npz'))['data']
            with open(os.path.join(dst, name + '.pkl'), 'rb') as f:
                out_props = pickle.load(f)
    finally:
        if float64_moments:
            pre.resample_patient = orig
    return out, out_props, list(_weights)


def main():
    rs = np.random.RandomState(11)
    rec = {}
    names = []
    for name, geom, schemes, masks in CASES:
        shape, sp0, sp1 = GEOM[geom]
        data = np.stack([ndimage.gaussian_filter(rs.randn(*shape), 1.0) * 600 + 50 for _ in schemes]).astype(np.float32)
        seg = blocky_labels(rs, shape, new_shape_of(shape, sp0, sp1), geom == 'big')[None]
        props = {'original_spacing': np.array(sp0), 'valid_regions': [[1, 2], [3]], 'valid_labels': [1, 2, 3, 4, 5],
                 'crop_bbox': [[0, n] for n in shape]}
        out, out_props, weights = run_reference(name, data, seg, dict(props), schemes, masks, sp1, False)
        out64, _, _ = run_reference(name, data, seg, dict(props), schemes, masks, sp1, True)
        assert np.array_equal(out[-1], out64[-1])
        new_shape = out.shape[1:]
        # fragile voxels of the label resample.  Separate z: the weights are per slice; they pass through the same order-0 gather.
        fragile = np.zeros(new_shape, dtype=bool)
        fragile_mask = np.zeros(new_shape, dtype=bool)                     # the same for the -1 indicator alone
        if weights:
            labels = list(np.unique(seg))
            per_slice = weights[0].ndim == 2
            n_lab = len(labels)
            if per_slice:
                # the slices' label sets differ: recompute the indicator weights per slice and label
                idx = np.clip(np.floor((np.arange(new_shape[0]) + 0.5) * (shape[0] / new_shape[0]) - 0.5 + 0.5).astype(int), 0, shape[0] - 1)
                for o, z in enumerate(idx):
                    for c in np.unique(seg[0, z]):
                        w = resize((seg[0, z] == c).astype(float), new_shape[1:], 1)
                        fragile[o] |= np.abs(w - 0.5) <= FRAGILE_EPS
                        if c == -1:
                            fragile_mask[o] |= np.abs(w - 0.5) <= FRAGILE_EPS
            else:
                assert len(weights) == n_lab
                for c, w in zip(labels, weights):
                    fragile |= np.abs(w - 0.5) <= FRAGILE_EPS
                    if c == -1:
                        fragile_mask |= np.abs(w - 0.5) <= FRAGILE_EPS
        share = float(fragile.mean())
        assert share <= MAX_FRAGILE_SHARE, (name, share)
        if any(masks):
            assert not fragile_mask.any(), (name, int(fragile_mask.sum()))
        dev64 = float(np.abs(out[:-1].astype(np.float64) - out64[:-1].astype(np.float64)).max())
        rec[name + '/data'] = data; rec[name + '/seg'] = seg.astype(np.int8)
        rec[name + '/out'] = out.astype(np.float32)
        # the output with float64 moments, as its (tiny) difference from `out`: out64 = out[:-1] + d64 to about 1e-10
        rec[name + '/d64'] = (out64[:-1].astype(np.float64) - out[:-1].astype(np.float64)).astype(np.float16)
        rec[name + '/dev64'] = np.array(dev64)
        rec[name + '/fragile'] = np.packbits(fragile)
        rec[name + '/spacing'] = np.array(list(sp0) + list(sp1))
        rec[name + '/schemes'] = np.array(schemes); rec[name + '/masks'] = np.array(masks)
        for c in ALL_CLASSES:
            locs = out_props['class_locations'][c]
            rec['%s/loc%d' % (name, c)] = np.zeros((0, 3), dtype=np.int64) if len(locs) == 0 else locs
        assert len(out_props['class_locations'][7]) == 0
        assert tuple(out_props['size_after_resampling']) == tuple(new_shape)
        assert out_props['valid_regions'] == props['valid_regions'] and out_props['valid_labels'] == props['valid_labels']
        names.append(name)
        print(name, data.shape, '->', out.shape, 'fragile %.4f' % share, 'float32-vs-float64 moments %.3g' % dev64,
              [len(out_props['class_locations'][c]) for c in ALL_CLASSES])
    assert max(len(rec['%s/loc1' % n]) for n in names) == 10000
    rec['names'] = np.array(names); rec['all_classes'] = np.array(ALL_CLASSES)
    rec['ip'] = np.array([[IP[c][k] for k in ('mean', 'sd', 'percentile_00_5', 'percentile_99_5')] for c in (0, 1)])
    dst = os.path.normpath(os.path.join(HERE, '..', '..', 'tests', 'golden', 'train_preprocess.npz'))
    with zipfile.ZipFile(dst, 'w', zipfile.ZIP_DEFLATED) as z:           # fixed member dates: the file is reproducible byte for byte
        for k in sorted(rec):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(rec[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print('wrote', dst, os.path.getsize(dst) // 1024, 'KiB')


if __name__ == '__main__':
    main()
