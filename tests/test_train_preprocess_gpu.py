"""Training-case pre-processing on the device against the REAL reference's GenericPreprocessor._run_internal
(tools/oracle_gen/make_golden_train_preprocess.py; skimage.resize substituted by its scipy.ndimage.zoom delegate,
resize_segmentation restated): the label map resampled per label with order 1, every normalisation scheme with and without
use_mask_for_norm, the sampled class locations, and the written files read back through the training loader.
Bounds: labels are compared outside the golden's "fragile" voxels (an interpolated one-hot weight within 1e-4 of 0.5; the device
forms the weights in float32), which must leave at least 0.90 of each case; data within 2e-4 (the bound of test_preprocess_gpu.py
for the CT path) + 2 x the reference's own recorded deviation between float32 and float64 moments; class locations are identical.
The kernels are also checked against numpy alone."""
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_preprocess.npz')
CASES = ['iso_up_ct2_mask', 'iso_down_ct_zscore', 'sepz_ct_mask_ct2_mask', 'sepz_zscore_mask_nonorm_mask', 'sepz_same_nonorm',
         'identity_zscore_mask', 'big_ct2']


def _golden():
    z = np.load(G)
    assert list(z['names']) == CASES
    ip = {c: dict(zip(('mean', 'sd', 'percentile_00_5', 'percentile_99_5'), (float(v) for v in z['ip'][c]))) for c in (0, 1)}
    return z, ip, [int(c) for c in z['all_classes']]


def _preprocessor(z, ip, name):
    from multitalent_amd.preprocessing.preprocessing import GenericPreprocessor
    schemes, masks = [str(s) for s in z[name + '/schemes']], [bool(m) for m in z[name + '/masks']]
    return GenericPreprocessor(dict(enumerate(schemes)), dict(enumerate(masks)), [0, 1, 2], ip), masks


def _fragile(z, name, shape):
    return np.unpackbits(z[name + '/fragile'])[:int(np.prod(shape))].reshape(shape).astype(bool)


@pytest.mark.parametrize("name", CASES)
def test_resample_seg_matches_reference_outside_fragile_voxels(dev, name):
    from multitalent_amd.preprocessing import device_preprocessing as dp
    z, _, _ = _golden()
    sp = z[name + '/spacing']
    seg = torch.from_numpy(z[name + '/seg'].astype(np.float32)).to(dev)
    new_shape, sep, axis = dp.resampling_plan(seg.shape[1:], sp[:3], sp[3:])
    out = dp.resample_seg(seg, new_shape, axis, sep).cpu().numpy()
    ref = z[name + '/out'][-1:]
    assert out.shape == ref.shape and out.dtype == np.float32
    keep = ~_fragile(z, name, ref.shape[1:])
    print(name, 'compared share %.4f' % keep.mean(), 'mismatches outside fragile', int((out[0] != ref[0])[keep].sum()),
          'inside', int((out[0] != ref[0])[~keep].sum()))
    assert keep.mean() >= 0.90
    assert np.array_equal(out[0][keep], ref[0][keep])


@pytest.mark.parametrize("name", CASES)
def test_training_case_matches_reference(dev, name):
    z, ip, all_classes = _golden()
    g, masks = _preprocessor(z, ip, name)
    sp = z[name + '/spacing']
    props = {'original_spacing': sp[:3].copy(), 'valid_regions': [[1, 2], [3]], 'valid_labels': [1, 2, 3, 4, 5]}
    all_data, out_props = g.preprocess_training_case(z[name + '/data'], z[name + '/seg'].astype(np.float32), props, sp[3:], all_classes)
    assert all_data.is_cuda and all_data.dtype == torch.float32
    out, ref = all_data.cpu().numpy(), z[name + '/out']
    assert out.shape == ref.shape
    keep = ~_fragile(z, name, ref.shape[1:])
    assert np.array_equal(out[-1][keep], ref[-1][keep])
    bound = 2e-4 + 2 * float(z[name + '/dev64'])
    for c in range(len(ref) - 1):
        d = np.abs(out[c] - ref[c])
        d64 = np.abs(out[c].astype(np.float64) - (ref[c].astype(np.float64) + z[name + '/d64'][c].astype(np.float64)))
        sel = keep if masks[c] else np.ones_like(keep)
        print(name, 'channel', c, 'max |device - reference| %.3g (float64-moment reference %.3g), bound %.3g' % (d[sel].max(), d64[sel].max(), bound))
        assert d[sel].max() <= bound, (c, d[sel].max(), bound)
    assert tuple(out_props['size_after_resampling']) == tuple(ref.shape[1:])
    assert np.array_equal(np.asarray(out_props['spacing_after_resampling']), sp[3:])
    assert out_props['valid_regions'] == [[1, 2], [3]] and out_props['valid_labels'] == [1, 2, 3, 4, 5]
    # class locations: the device's own label map differs from the golden's on fragile voxels at most, so resolve them on the golden's
    from multitalent_amd.preprocessing import device_preprocessing as dp
    locs = dp.class_locations(torch.from_numpy(np.ascontiguousarray(ref[-1])).to(dev), all_classes)
    assert list(locs.keys()) == all_classes
    for c in all_classes:
        want = z['%s/loc%d' % (name, c)]
        if len(want) == 0:
            assert isinstance(locs[c], list) and locs[c] == []
        else:
            assert isinstance(locs[c], np.ndarray) and locs[c].dtype == np.int64 and locs[c].shape == want.shape
            assert np.array_equal(locs[c], want)
    if not (out[-1] != ref[-1]).any():
        for c in all_classes:
            assert np.array_equal(np.asarray(out_props['class_locations'][c]).reshape(-1, 3), z['%s/loc%d' % (name, c)])


def test_run_writes_what_the_loader_reads(dev, tmp_path):
    from multitalent_amd.training.dataloading.dataset_loading import DataLoader3D, load_dataset
    z, ip, all_classes = _golden()
    name = 'sepz_ct_mask_ct2_mask'
    g, _ = _preprocessor(z, ip, name)
    src, dst = tmp_path / 'cropped', tmp_path / 'out'
    src.mkdir()
    sp = z[name + '/spacing']
    for case in ('a_000', 'a_001'):
        np.savez_compressed(src / (case + '.npz'), data=np.vstack((z[name + '/data'], z[name + '/seg'].astype(np.float32))))
        with open(src / (case + '.pkl'), 'wb') as f:
            pickle.dump({'original_spacing': sp[:3].copy(), 'valid_regions': [[1, 2], [3]], 'valid_labels': [1, 2, 3], 'note': case}, f)
    with open(src / 'dataset_properties.pkl', 'wb') as f:
        pickle.dump({'all_classes': all_classes}, f)
    g.run([sp[3:], sp[3:] * 2], str(src), str(dst), 'nnUNetData_plans', num_threads=2)
    assert sorted(os.listdir(dst)) == ['nnUNetData_plans_stage0', 'nnUNetData_plans_stage1']
    ref = z[name + '/out']
    keep = ~_fragile(z, name, ref.shape[1:])
    ds = load_dataset(str(dst / 'nnUNetData_plans_stage0'))
    assert list(ds.keys()) == ['a_000', 'a_001']
    for case, entry in ds.items():
        arr = np.load(entry['data_file'])['data']
        assert arr.dtype == np.float32 and arr.shape == ref.shape
        assert np.array_equal(arr[-1][keep], ref[-1][keep])
        p = entry['properties']
        assert p['note'] == case and p['valid_regions'] == [[1, 2], [3]] and p['valid_labels'] == [1, 2, 3]
        assert tuple(p['size_after_resampling']) == tuple(ref.shape[1:])
        assert set(p['class_locations'].keys()) == set(all_classes) and len(p['class_locations'][7]) == 0
        for c in all_classes:
            for x, y, zz in np.asarray(p['class_locations'][c]).reshape(-1, 3)[:50]:
                assert arr[-1, x, y, zz] == c
    # _run_internal alone writes the same case
    one = tmp_path / 'single'
    one.mkdir()
    g._run_internal(sp[3:], 'a_000', str(one), str(src), None, all_classes)
    assert np.array_equal(np.load(one / 'a_000.npz')['data'], np.load(ds['a_000']['data_file'])['data'])
    np.random.seed(3)
    patch = (8, 12, 12)
    batch = next(DataLoader3D(ds, patch, patch, 2, oversample_foreground_percent=1.0))
    assert batch['data'].shape == (2, 2) + patch and batch['seg'].shape == (2, 1) + patch
    assert all((s > 0).any() for s in batch['seg'])                         # forced foreground: the patch holds the chosen voxel
    assert len(os.listdir(dst / 'nnUNetData_plans_stage1')) == 4


def test_previously_unsupported_schemes_return(dev):
    """`{0: 'nonCT'}` and `use_mask_for_norm={0: True}` raised NotImplementedError before."""
    from multitalent_amd.preprocessing.preprocessing import GenericPreprocessor
    rs = np.random.RandomState(0)
    data = (rs.randn(1, 10, 12, 14) * 40 + 100).astype(np.float32)
    seg = np.zeros((1, 10, 12, 14), dtype=np.float32)
    seg[:, :, :3] = -1
    ip = {0: {'mean': 100.0, 'sd': 40.0, 'percentile_00_5': 0.0, 'percentile_99_5': 200.0}}
    props = {'original_spacing': np.array([1.0, 1.0, 1.0])}
    d, s, _ = GenericPreprocessor({0: 'nonCT'}, {0: False}, [0, 1, 2], ip).resample_and_normalize(data.copy(), np.array([1.0, 1.0, 1.0]),
                                                                                                  dict(props), seg.copy())
    want = (data - data.mean(dtype=np.float64)) / (data.std(dtype=np.float64) + 1e-8)
    assert isinstance(d, np.ndarray) and np.abs(d - want).max() < 1e-5 and np.array_equal(s, seg)
    d, s, _ = GenericPreprocessor({0: 'CT'}, {0: True}, [0, 1, 2], ip).resample_and_normalize(data.copy(), np.array([1.0, 1.0, 1.0]),
                                                                                              dict(props), seg.copy())
    want = (np.clip(data, 0.0, 200.0) - np.float32(100.0)) / np.float32(40.0)
    want[seg < 0] = 0
    assert np.array_equal(d, want)                                          # the same float32 operations in the same order


def _moments_np(x, sel):
    v = x.astype(np.float64)[sel]
    return (float(sel.sum()), float(v.mean()), float(v.std())) if sel.any() else (0.0, np.nan, np.nan)


def test_masked_moments_against_numpy(dev):
    from multitalent_amd import ops
    rs = np.random.RandomState(5)
    shape = (2, 37, 41, 43)                                                 # 65231 voxels per channel: not a multiple of 4
    x = (rs.randn(*shape) * 5 - 900).astype(np.float32)
    x[1] = x[1] * 3 + 2000
    seg = (rs.randint(0, 3, shape[1:]) - 1).astype(np.float32)
    xd, sd = torch.from_numpy(x).to(dev), torch.from_numpy(seg).to(dev)
    lo, hi = [-903.0, -705.0], [-895.0, -690.0]
    runs = []
    for _ in range(2):
        runs.append([ops.masked_moments(xd, ops.MOMENTS_ALL).cpu().numpy(),
                     ops.masked_moments(xd, ops.MOMENTS_SEG_GE0, seg=sd).cpu().numpy(),
                     ops.masked_moments(xd, ops.MOMENTS_OPEN_RANGE, lo=lo, hi=hi).cpu().numpy(),
                     ops.masked_moments(xd, ops.MOMENTS_OPEN_RANGE, lo=[5e3, 5e3], hi=[6e3, 6e3]).cpu().numpy()])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()                                   # bit-equal from run to run
    got_all, got_seg, got_rng, got_empty = runs[0]
    for c in range(2):
        wants = [_moments_np(x[c], np.ones(shape[1:], bool)), _moments_np(x[c], seg >= 0),
                 _moments_np(x[c], (x[c].astype(np.float64) > lo[c]) & (x[c].astype(np.float64) < hi[c]))]
        for got, want in zip((got_all, got_seg, got_rng), wants):
            assert got[c, 0] == want[0] and want[0] > 1000
            rel = [abs(got[c, k] - want[k]) / abs(want[k]) for k in (1, 2)]
            print('channel', c, 'relative error of mean, sd:', rel)
            assert max(rel) <= 1e-12
        assert got_empty[c, 0] == 0 and np.isnan(got_empty[c, 1]) and np.isnan(got_empty[c, 2])


def test_intensity_normalize_is_numpy_float32(dev):
    from multitalent_amd import ops
    rs = np.random.RandomState(6)
    x = (rs.randn(33, 35, 37) * 300 + 50).astype(np.float32)               # 42735 voxels: odd
    seg = (rs.randint(0, 3, x.shape) - 1).astype(np.float32)
    m, s = np.float32(63.44), np.float32(175.48)
    want = (np.clip(x, np.float32(-500), np.float32(400)) - m) / s
    got = ops.intensity_normalize(torch.from_numpy(x).to(dev), (-500.0, 400.0), 63.44, 175.48).cpu().numpy()
    assert np.array_equal(got, want)
    want[seg < 0] = 0
    got = ops.intensity_normalize(torch.from_numpy(x).to(dev), (-500.0, 400.0), 63.44, 175.48, seg=torch.from_numpy(seg).to(dev)).cpu().numpy()
    assert np.array_equal(got, want)
    xd = torch.from_numpy(x).to(dev)
    st = ops.masked_moments(xd[None], ops.MOMENTS_ALL)
    mean, sd = np.float32(x.astype(np.float64).mean()), np.float32(x.astype(np.float64).std())
    assert float(st[0, 1]) == pytest.approx(x.astype(np.float64).mean(), rel=1e-12)
    want = (x - np.float32(st[0, 1].item())) / (np.float32(st[0, 2].item()) + np.float32(1e-8))
    got = ops.intensity_normalize(xd, stats=st[0], eps=1e-8).cpu().numpy()
    assert np.array_equal(got, want) and abs(float(mean) - float(st[0, 1])) < 1e-4 and abs(float(sd) - float(st[0, 2])) < 1e-4


def test_label_locations_against_argwhere_256(dev):
    from multitalent_amd import ops
    from multitalent_amd.preprocessing import device_preprocessing as dp
    rs = np.random.RandomState(8)
    seg = np.zeros((256, 256, 256), dtype=np.float32)
    seg[20:150, 30:140, 40:160] = 3                                         # 1 716 000 voxels: the 1 % rule gives k = 17160
    seg[100:130, 100:135, 150:200] = 300                                    # a label above 255, cutting into label 3
    seg[rs.randint(0, 256, 4000), rs.randint(0, 256, 4000), rs.randint(0, 256, 4000)] = 17     # scattered single voxels
    seg[:, :, 250:] = -1
    all_classes = [17, 3, 9, 300]                                           # 9 is absent
    sd = torch.from_numpy(seg).to(dev)
    counts, index = ops.label_counts(sd, all_classes)
    want_counts = [int((seg == c).sum()) for c in all_classes]
    assert counts.cpu().tolist() == want_counts and want_counts[1] > 1500000 and want_counts[2] == 0
    ranks = dp.draw_class_ranks(want_counts)
    assert len(ranks[1]) == int(np.ceil(0.01 * want_counts[1])) >= 15000 and ranks[2] is None
    a = dp.class_locations(sd, all_classes)
    b = dp.class_locations(sd, all_classes)
    rndst = np.random.RandomState(1234)
    for c in all_classes:
        locs = np.argwhere(seg == c)
        if len(locs) == 0:
            assert a[c] == [] and b[c] == []
            continue
        k = max(min(10000, len(locs)), int(np.ceil(len(locs) * 0.01)))
        want = locs[rndst.choice(len(locs), k, replace=False)]
        assert a[c].dtype == np.int64 and a[c].shape == want.shape and np.array_equal(a[c], want)
        assert a[c].tobytes() == b[c].tobytes()
    # every rank of a class, and ranks beyond the count
    n = want_counts[3]
    q = np.arange(n + 2, dtype=np.int64)
    out = ops.label_locations(index, np.full(n + 2, 3, dtype=np.int32), q).cpu().numpy()
    assert np.array_equal(out[:n], np.argwhere(seg == 300)) and (out[n:] == -1).all()


def test_label_locations_over_more_units_than_scan_threads(dev):
    """301 units of 8192 voxels, the last one 5 voxels long: every thread of the scan's workgroup owns up to two units, and the
    threads beyond unit 300 none."""
    from multitalent_amd import ops
    rs = np.random.RandomState(12)
    V = 8192 * 300 + 5
    density = np.linspace(0.02, 0.9, V) * (np.arange(V) // 8192 % 7 != 3)    # rising along the volume, some units empty
    seg = np.where(rs.rand(V) < density, rs.randint(1, 4, V), rs.randint(-1, 1, V)).astype(np.float32).reshape(1, 1, V)
    seg[0, 0, -1] = 2
    all_classes = [2, 3, 1]
    counts, index = ops.label_counts(torch.from_numpy(seg).to(dev), all_classes)
    want_counts = [int((seg == c).sum()) for c in all_classes]
    assert counts.cpu().tolist() == want_counts and min(want_counts) > 100000
    for slot, c in enumerate(all_classes):
        locs = np.argwhere(seg == c)
        rank = np.unique(np.concatenate([np.arange(0, len(locs), 7), [len(locs) - 1]]))
        out = ops.label_locations(index, np.full(len(rank), slot, dtype=np.int32), rank, total=sum(want_counts)).cpu().numpy()
        assert np.array_equal(out, locs[rank]), c


def test_label_counts_rejects_bad_arguments(dev):
    from multitalent_amd import ops
    seg = torch.zeros((4, 4, 4), device=dev)
    with pytest.raises(ValueError):
        ops.label_counts(seg, list(range(256)))
    with pytest.raises(ValueError):
        ops.label_counts(seg, [1, -1])
    with pytest.raises(ValueError, match="int32"):
        ops.label_counts(torch.zeros(1, device=dev).expand(1290, 1291, 1291), [1])
