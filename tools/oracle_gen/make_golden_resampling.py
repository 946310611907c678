"""Golden vectors for the resize unit: the REAL reference's resample_data_or_seg (preprocessing.py:109-197) for data and for label
maps, and `_run_internal` of GenericPreprocessor_linearResampling and Preprocessor3DDifferentResampling, on small float32 cases.
The substitutions are those of make_golden_train_preprocess.py: skimage.transform.resize is the delegate it has used since skimage
0.19 (scipy.ndimage.zoom(order, mode='nearest', grid_mode=True)), batchgenerators' resize_segmentation is restated from its
published algorithm.  Writes tests/golden/resampling.npz.

Per label case the "fragile" voxels are recorded: a voxel is fragile if a weight that decides it is within 1e-4 of one half — a
label's interpolated indicator of the in-plane / 3D stage at order 1, the linear weight of the z pass at order_z 1 — or if it reads a
stage-1 voxel that is.  The device forms these weights in its own order of operations and may fall on the other side there.  Order 0
has no such voxels: its coordinate is the same sequence of double operations in scipy and on the device, ties included.  Fragile
voxels must leave at least 0.90 of every case (the bound of test_train_preprocess_gpu.py).
Run: python tools/oracle_gen/make_golden_resampling.py"""
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
        reshaped[w >= 0.5] = c
    return reshaped


pre.resize = resize
pre.resize_segmentation = resize_segmentation
pre.pickle = pickle

IP = {0: {'mean': 63.44, 'sd': 175.48, 'percentile_00_5': -927.0, 'percentile_99_5': 275.0},
      1: {'mean': -12.5, 'sd': 210.25, 'percentile_00_5': -640.0, 'percentile_99_5': 410.0}}
# name: shape, original spacing, target spacing -> new shape (asserted), separate z, its axis
GEOM = {'up': ((9, 20, 18), (4.0, 0.7, 0.7), (2.77, 0.52, 0.505), (13, 27, 25), True, 0),
        'double': ((5, 12, 12), (5.0, 1.0, 1.0), (2.5, 0.5, 0.5), (10, 24, 24), True, 0),
        'mixed': ((7, 24, 22), (5.0, 0.9, 0.9), (2.5, 1.2, 1.17), (14, 18, 17), True, 0),
        'iso_down': ((24, 26, 22), (0.8, 0.8, 0.8), (1.5, 1.4, 1.3), (13, 15, 14), False, None),
        'axis_last': ((20, 18, 9), (0.7, 0.7, 4.0), (0.52, 0.505, 2.77), (27, 25, 13), True, 2),
        'z_same': ((9, 20, 18), (4.0, 0.7, 0.7), (4.0, 0.52, 0.505), (9, 27, 25), True, 0)}
DATA_ORDERS = [(1, 0), (3, 3), (3, 1), (0, 0)]
SEG_ORDERS = [(1, 1), (1, 0), (0, 0)]
ALL_CLASSES = [1, 2, 3, 4, 5, 7]            # 7 never occurs
# name, class, geometry, schemes per modality, use_mask_for_norm per modality
CASES = [('diff_up_ct', 'Preprocessor3DDifferentResampling', 'up', ['CT'], [False]),
         ('diff_mixed_ct2_mask', 'Preprocessor3DDifferentResampling', 'mixed', ['CT2'], [True]),
         ('diff_axis_last_zscore_nonorm', 'Preprocessor3DDifferentResampling', 'axis_last', ['nonCT', 'noNorm'], [False, False]),
         ('diff_iso_down_ct_mask', 'Preprocessor3DDifferentResampling', 'iso_down', ['CT'], [True]),
         ('lin_up_ct', 'GenericPreprocessor_linearResampling', 'up', ['CT'], [False]),
         ('lin_iso_down_zscore_mask', 'GenericPreprocessor_linearResampling', 'iso_down', ['nonCT'], [True]),
         ('lin_z_same_ct2', 'GenericPreprocessor_linearResampling', 'z_same', ['CT2'], [False])]


def coord(n_in, n_out):
    return (np.arange(n_out) + 0.5) * (float(n_in) / n_out) - 0.5


def slab_width(n_in, n_out, from_end):
    """Smallest width >= 2 of a -1 slab whose border no output coordinate (o + 0.5) * in/out - 0.5 meets half-way."""
    x = coord(n_in, n_out)
    for w in range(2, 7):
        border = (n_in - w - 0.5) if from_end else (w - 0.5)
        if np.abs(x - border).min() > 1e-3:
            return w
    raise AssertionError((n_in, n_out))


def blocky_labels(rs, shape, new_shape, sep_axis):
    """Labels -1..5 in blocks: -1 on two border slabs (the outside of the non-zero mask) across two axes that are not the separately
    resampled one, 0 background, boxes of 1..5."""
    seg = np.zeros(shape, dtype=np.float32)
    for lab in (1, 2, 3, 4, 5):
        for _ in range(2):
            lo = [rs.randint(0, max(1, n - 3)) for n in shape]
            sz = [rs.randint(2, max(3, n // 2)) for n in shape]
            seg[lo[0]:lo[0] + sz[0], lo[1]:lo[1] + sz[1], lo[2]:lo[2] + sz[2]] = lab
    a, b = [i for i in range(3) if i != (0 if sep_axis is None else sep_axis)]
    sl = [slice(None)] * 3
    sl[a] = slice(0, slab_width(shape[a], new_shape[a], False))
    seg[tuple(sl)] = -1
    sl = [slice(None)] * 3
    sl[b] = slice(shape[b] - slab_width(shape[b], new_shape[b], True), None)
    seg[tuple(sl)] = -1
    return seg


def stage_fragile(seg, new_shape, order, only=None):
    """Fragile voxels of one resize_fn call on the label map `seg` (2D or 3D); only: restrict to that label's indicator."""
    fragile = np.zeros(new_shape, dtype=bool)
    if tuple(seg.shape) == tuple(new_shape):
        return fragile
    if order == 0:
        return fragile
    for c in (np.unique(seg) if only is None else [only]):
        fragile |= np.abs(resize((seg == c).astype(float), new_shape, order) - 0.5) <= FRAGILE_EPS
    return fragile


def label_fragile(seg, new_shape, sep, axis, order, order_z, only=None):
    """seg: [X, Y, Z] -> fragile voxels of resample_data_or_seg(seg[None], new_shape, True, [axis], order, sep, order_z)."""
    shape = seg.shape
    if tuple(shape) == tuple(new_shape):
        return np.zeros(new_shape, dtype=bool)
    if not sep:
        return stage_fragile(seg, new_shape, order, only)
    new_2d = [new_shape[a] for a in range(3) if a != axis]
    f1 = np.stack([stage_fragile(np.take(seg, s, axis=axis), new_2d, order, only) for s in range(shape[axis])], axis)
    if shape[axis] == new_shape[axis]:
        return f1
    x = np.clip(coord(shape[axis], new_shape[axis]), 0, shape[axis] - 1)
    i0 = np.floor(x).astype(int)
    t = x - i0
    i1 = np.minimum(i0 + 1, shape[axis] - 1)
    if order_z == 0:
        idx = np.clip(np.floor(coord(shape[axis], new_shape[axis]) + 0.5).astype(int), 0, shape[axis] - 1)
        return np.take(f1, idx, axis=axis)
    else:
        f = (np.take(f1, i0, axis=axis) & np.reshape(t < 1, [-1 if a == axis else 1 for a in range(3)])) | \
            (np.take(f1, i1, axis=axis) & np.reshape(t > 0, [-1 if a == axis else 1 for a in range(3)]))
    return f | np.reshape(np.abs(t - 0.5) <= FRAGILE_EPS, [-1 if a == axis else 1 for a in range(3)])


def run_reference(cls_name, name, data, seg, props, schemes, masks, sp1, float64_moments):
    g = getattr(pre, cls_name)({i: s for i, s in enumerate(schemes)}, {i: m for i, m in enumerate(masks)}, [0, 1, 2], IP)
    if float64_moments:
        orig = pre.resample_patient

        def widened(*a, **k):
            d, s = orig(*a, **k)
            return d.astype(np.float64), s
        pre.resample_patient = widened
    try:
        with tempfile.TemporaryDirectory() as tmp:
            src, dst = os.path.join(tmp, 'cropped'), os.path.join(tmp, 'stage0')
            os.makedirs(src); os.makedirs(dst)
            np.savez_compressed(os.path.join(src, name + '.npz'), data=np.vstack((data, seg)))
            with open(os.path.join(src, name + '.pkl'), 'wb') as f:
                pickle.dump(props, f)
            g._run_internal(np.array(sp1), name, dst, src, None, ALL_CLASSES)
            out = np.load(os.path.join(dst, name + '.npz'))['data']
            with open(os.path.join(dst, name + '.pkl'), 'rb') as f:
                out_props = pickle.load(f)
    finally:
        if float64_moments:
            pre.resample_patient = orig
    return out, out_props


def main():
    rs = np.random.RandomState(23)
    rec = {}
    # ---- resample_data_or_seg alone
    inputs = {}
    for gname, (shape, sp0, sp1, new_shape, sep, axis) in GEOM.items():
        got = np.round((np.array(sp0) / np.array(sp1)).astype(float) * np.array(shape)).astype(int)
        assert tuple(got) == new_shape, (gname, got)
        data = np.stack([ndimage.gaussian_filter(rs.randn(*shape), 1.0) * 600 + 50 for _ in range(2)]).astype(np.float32)
        seg = blocky_labels(rs, shape, new_shape, axis)[None]
        inputs[gname] = (data, seg)
        rec['geom/%s/data' % gname] = data
        rec['geom/%s/seg' % gname] = seg.astype(np.int8)
        rec['geom/%s/spacing' % gname] = np.array(list(sp0) + list(sp1))
        rec['geom/%s/new_shape' % gname] = np.array(new_shape)
        rec['geom/%s/axis' % gname] = np.array(-1 if axis is None else axis)
        ax = None if axis is None else [axis]
        for order, order_z in DATA_ORDERS:
            out = pre.resample_data_or_seg(data[:1], new_shape, False, ax, order, sep, order_z)
            assert out.dtype == np.float32 and out.shape == (1,) + new_shape
            rec['data/%s/%d%d' % (gname, order, order_z)] = out
        for order, order_z in SEG_ORDERS:
            out = pre.resample_data_or_seg(seg, new_shape, True, ax, order, sep, order_z)
            assert out.dtype == np.float32 and np.array_equal(out, np.round(out))
            fragile = label_fragile(seg[0], new_shape, sep, axis, order, order_z)
            share = float(fragile.mean())
            assert share <= MAX_FRAGILE_SHARE, (gname, order, order_z, share)
            rec['seg/%s/%d%d' % (gname, order, order_z)] = out.astype(np.int8)
            rec['fragile/%s/%d%d' % (gname, order, order_z)] = np.packbits(fragile)
            print(gname, 'labels', (order, order_z), shape, '->', new_shape, 'fragile %.4f' % share, 'labels', np.unique(out))
    # ---- the two preprocessors
    names = []
    for name, cls_name, gname, schemes, masks in CASES:
        shape, sp0, sp1, new_shape, sep, axis = GEOM[gname]
        data, seg = inputs[gname][0][:len(schemes)], inputs[gname][1]
        props = {'original_spacing': np.array(sp0), 'valid_regions': [[1, 2], [3]], 'valid_labels': [1, 2, 3, 4, 5],
                 'crop_bbox': [[0, n] for n in shape]}
        out, out_props = run_reference(cls_name, name, data, seg, dict(props), schemes, masks, sp1, False)
        out64, _ = run_reference(cls_name, name, data, seg, dict(props), schemes, masks, sp1, True)
        assert np.array_equal(out[-1], out64[-1]) and out.shape[1:] == new_shape
        order_seg, order_z_seg = (1, 1) if cls_name == 'Preprocessor3DDifferentResampling' else (1, 0)
        assert np.array_equal(out[-1], rec['seg/%s/%d%d' % (gname, order_seg, order_z_seg)][0])
        fragile = label_fragile(seg[0], new_shape, sep, axis, order_seg, order_z_seg)
        if any(masks):
            fm = label_fragile(seg[0], new_shape, sep, axis, order_seg, order_z_seg, only=-1)
            assert not fm.any(), (name, int(fm.sum()))
        dev64 = float(np.abs(out[:-1].astype(np.float64) - out64[:-1].astype(np.float64)).max())
        rec[name + '/out'] = out[:-1].astype(np.float32)              # the label channel apart, as int8
        assert np.array_equal(out[-1], out[-1].astype(np.int8))
        rec[name + '/out_seg'] = out[-1].astype(np.int8)
        rec[name + '/d64'] = (out64[:-1].astype(np.float64) - out[:-1].astype(np.float64)).astype(np.float16)
        rec[name + '/dev64'] = np.array(dev64)
        rec[name + '/fragile'] = np.packbits(fragile)
        rec[name + '/schemes'] = np.array(schemes); rec[name + '/masks'] = np.array(masks)
        rec[name + '/class'] = np.array(cls_name); rec[name + '/geom'] = np.array(gname)
        for c in ALL_CLASSES:
            locs = out_props['class_locations'][c]
            rec['%s/loc%d' % (name, c)] = np.zeros((0, 3), dtype=np.int64) if len(locs) == 0 else locs
        assert len(out_props['class_locations'][7]) == 0
        assert tuple(out_props['size_after_resampling']) == tuple(new_shape)
        names.append(name)
        print(name, data.shape, '->', out.shape, 'fragile %.4f' % fragile.mean(), 'float32-vs-float64 moments %.3g' % dev64,
              [len(out_props['class_locations'][c]) for c in ALL_CLASSES])
    rec['names'] = np.array(names); rec['geoms'] = np.array(list(GEOM)); rec['all_classes'] = np.array(ALL_CLASSES)
    rec['data_orders'] = np.array(DATA_ORDERS); rec['seg_orders'] = np.array(SEG_ORDERS)
    rec['ip'] = np.array([[IP[c][k] for k in ('mean', 'sd', 'percentile_00_5', 'percentile_99_5')] for c in (0, 1)])
    dst = os.path.normpath(os.path.join(HERE, '..', '..', 'tests', 'golden', 'resampling.npz'))
    with zipfile.ZipFile(dst, 'w', zipfile.ZIP_DEFLATED) as z:           # fixed member dates: the file is reproducible byte for byte
        for k in sorted(rec):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(rec[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print('wrote', dst, os.path.getsize(dst) // 1024, 'KiB')


if __name__ == '__main__':
    main()
