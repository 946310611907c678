"""Cropping to the non-zero region on the device (mt_nonzero_mask, mt_fill_holes3d, mt_crop_nonzero; preprocessing/device_cropping.py).
Everything is exact: the hole filling against scipy.ndimage.binary_fill_holes, the mask against numpy, the crop against the real
reference's outputs (tests/golden/cropping.npz), and `preprocess_test_case` against the host cropper feeding the same kernels."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def golden_cases():
    g = np.load(os.path.join(HERE, 'golden', 'cropping.npz'))
    for name in [str(n) for n in g['names']]:
        yield name, {k: g[name + '/' + k] for k in ('data', 'seg', 'out_data', 'out_seg', 'bbox') if name + '/' + k in g.files}


def shell(shape, lo, hi):
    m = np.zeros(shape, bool)
    m[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
    m[lo[0] + 1:hi[0], lo[1] + 1:hi[1], lo[2] + 1:hi[2]] = False
    return m


def serpentine_cavity(shape, open_end):
    """A solid block with one cavity that snakes through every 8x16x16 brick: rows of zeros along w on every second (d, h), joined
    alternately at their ends, planes joined at (h, w) = (1, 1).  `open_end` carries it on to the face w = 0."""
    D, H, W = shape
    m = np.ones(shape, bool)
    for d in range(1, D - 1, 2):
        rows = list(range(1, H - 1, 2))
        for k, h in enumerate(rows):
            m[d, h, 1:W - 1] = False
            if k + 1 < len(rows):
                m[d, h + 1, W - 2 if k % 2 == 0 else 1] = False
        if d + 2 < D - 1:
            m[d + 1, 1, 1] = False
    if open_end:
        m[1, 1, 0] = False
    return m


def fill_cases():
    rng = np.random.default_rng(7)
    yield 'empty', np.zeros((9, 20, 33), bool)
    yield 'full', np.ones((9, 20, 33), bool)
    one = np.zeros((11, 13, 17), bool)
    one[5, 6, 7] = True
    yield 'one voxel', one
    yield '1x1x1 set', np.ones((1, 1, 1), bool)
    yield '1x1x1 clear', np.zeros((1, 1, 1), bool)
    for shape in ((1, 7, 9), (5, 1, 8), (6, 9, 1)):                  # an axis of 1: every voxel is on a face, nothing is filled
        m = rng.random(shape) < 0.6
        m[tuple(s // 2 for s in shape)] = False
        yield 'axis of one %s' % (shape,), m
    ring = np.zeros((1, 9, 9), bool)
    ring[0, 2:7, 2:7] = True
    ring[0, 4, 4] = False
    yield 'ring in a single slice', ring
    for shape, dens in (((9, 17, 19), 0.2), ((23, 37, 41), 0.5), ((40, 37, 50), 0.69), ((17, 33, 65), 0.8), ((8, 16, 16), 0.9),
                        ((31, 48, 47), 0.6931)):
        yield 'random %s density %g' % (shape, dens), rng.random(shape) < dens
    big = rng.random((72, 130, 150)) < 0.69                          # the background at the percolation density of 6-connectivity
    yield 'random 72x130x150 density 0.69', big
    closed = shell((20, 30, 40), (3, 4, 5), (15, 24, 33))
    yield 'closed shell', closed
    ch = closed.copy()
    ch[3, 12, 20] = False                                            # a face voxel of the shell: a channel to the outside
    yield 'shell with a channel', ch
    dg = closed.copy()
    dg[3, 4, 17] = False                                             # an edge voxel: the cavity and the outside share no face
    yield 'shell with a diagonal leak', dg
    yield 'cavity touching a volume face', shell((20, 30, 40), (3, 4, 5), (15, 24, 40))
    nested = shell((30, 36, 44), (2, 2, 2), (27, 33, 41)) | shell((30, 36, 44), (8, 9, 10), (20, 25, 30))
    nested[13:16, 15:19, 18:22] = True                               # and a solid core inside the inner cavity
    yield 'shell inside cavity inside shell', nested
    yield 'serpentine cavity', serpentine_cavity((21, 45, 50), False)
    yield 'serpentine cavity open to a face', serpentine_cavity((21, 45, 50), True)


def numpy_box(filled):
    idx = np.where(filled)
    return [int(v) for i in idx for v in (i.min(), i.max() + 1)], int(filled.sum())


def check_fill(name, m):
    from scipy.ndimage import binary_fill_holes
    from multitalent_amd import ops
    from multitalent_amd.preprocessing import device_cropping as dc
    want = binary_fill_holes(m)
    dev = torch.from_numpy(m.astype(np.uint8) * 3).cuda()             # any non-zero value is foreground
    out, box = ops.fill_holes3d(dev.clone())
    out2, box2 = ops.fill_holes3d(dev.clone())
    got = out.cpu().numpy()
    assert got.dtype == np.uint8 and got.max(initial=0) <= 1, name
    assert np.array_equal(got.astype(bool), want), '%s: %d voxels differ' % (name, int((got.astype(bool) != want).sum()))
    assert torch.equal(out, out2) and torch.equal(box, box2), name + ': two runs differ'
    b = [int(i) for i in box.cpu()]
    n = int(want.sum())
    assert b[6] == n, name
    if n:
        assert (b[:6], b[6]) == numpy_box(want), name
    keep = torch.from_numpy(m).cuda()
    pub = dc.fill_holes(keep)                                        # the public function: bool in, bool out, input untouched
    assert pub.dtype == torch.bool and np.array_equal(pub.cpu().numpy(), want) and np.array_equal(keep.cpu().numpy(), m), name
    if n:
        assert dc.get_bbox_from_mask(pub) == [[b[0], b[1]], [b[2], b[3]], [b[4], b[5]]], name


def test_fill_holes_equals_scipy():
    names = []
    for name, m in fill_cases():
        check_fill(name, m)
        names.append(name)
    assert len(names) == 23
    with pytest.raises(ValueError):
        from multitalent_amd.preprocessing import device_cropping as dc
        dc.get_bbox_from_mask(torch.zeros((3, 4, 5), dtype=torch.bool, device='cuda'))


def test_fill_holes_numpy_input_is_uploaded_and_left_alone():
    from scipy.ndimage import binary_fill_holes
    from multitalent_amd.preprocessing import device_cropping as dc
    m = shell((12, 14, 16), (2, 2, 2), (9, 11, 13))
    keep = m.copy()
    out = dc.fill_holes(m)
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), binary_fill_holes(keep)) and np.array_equal(m, keep)


def test_fill_holes_body_like_volume():
    """180 x 512 x 512: an elliptic body with 2 % zero voxels inside it and zeros outside (the volume of tools/bench_cropping.py)."""
    from scipy.ndimage import binary_fill_holes
    from multitalent_amd import ops
    rng = np.random.default_rng(3)
    D, H, W = 180, 512, 512
    z, y, x = np.ogrid[:D, :H, :W]
    m = (((z - 90) / 85.0) ** 2 + ((y - 256) / 200.0) ** 2 + ((x - 250) / 230.0) ** 2 <= 1) & (rng.random((D, H, W)) >= 0.02)
    want = binary_fill_holes(m)
    dev = torch.from_numpy(m.view(np.uint8)).cuda()
    out, box = ops.fill_holes3d(dev.clone())
    out2, box2 = ops.fill_holes3d(dev.clone())
    assert torch.equal(out, out2) and torch.equal(box, box2)
    got = out.cpu().numpy().astype(bool)
    assert np.array_equal(got, want), int((got != want).sum())
    b = [int(i) for i in box.cpu()]
    assert (b[:6], b[6]) == numpy_box(want)


def test_fill_holes_argument_checks():
    from multitalent_amd import ops
    m = torch.zeros((4, 5, 6), dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match="workspace"):
        ops.fill_holes3d(m, ws=torch.empty(4 * 5 * 6 * 4, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        ops.fill_holes3d(torch.zeros((4, 5), dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError, match="int32"):
        ops.crop_check_shape((2048, 1024, 1025))
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.fill_holes3d(torch.zeros((4, 5, 6), dtype=torch.uint8))


SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-45, -1e-45, 0.0, 1.0, -2.5, 1.1754944e-38], dtype=np.float32)


def special_data(rng, C, V):
    d = np.zeros((C, V), np.float32)
    pick = rng.random((C, V))
    d[pick < 0.25] = rng.standard_normal(int((pick < 0.25).sum())).astype(np.float32)
    sp = (pick >= 0.25) & (pick < 0.4)
    d[sp] = SPECIALS[rng.integers(0, len(SPECIALS), int(sp.sum()))]
    return d


@pytest.mark.parametrize('C', [1, 2, 4])
def test_nonzero_mask_equals_numpy(C):
    from multitalent_amd import ops
    rng = np.random.default_rng(10 + C)
    with np.errstate(invalid='ignore'):
        for V in (1, 3, 5, 63, 1021, 4099, 70001):
            for doff, moff in ((0, 0), (1, 3), (3, 1), (2, 2)):          # data starts doff floats, mask moff bytes after an aligned address
                d = special_data(rng, C, V)
                want = (d != 0).any(axis=0)
                base = torch.zeros(C * V + 8, dtype=torch.float32, device='cuda')
                view = base[doff:doff + C * V].view(C, V)
                view.copy_(torch.from_numpy(d))
                assert np.array_equal(bits(view.cpu().numpy()), bits(d))      # the copy kept -0.0, the denormals and the NaNs
                mbase = torch.full((V + 16,), 77, dtype=torch.uint8, device='cuda')
                mask = mbase[moff:moff + V]
                ops.nonzero_mask(view, mask)
                got = mbase.cpu().numpy()
                assert np.array_equal(got[moff:moff + V], want.astype(np.uint8)), (C, V, doff, moff)
                assert (got[:moff] == 77).all() and (got[moff + V:] == 77).all(), (C, V, doff, moff)


@pytest.mark.parametrize('C', [1, 2, 4])
def test_create_nonzero_mask_equals_the_host(C):
    from multitalent_amd.preprocessing import cropping, device_cropping as dc
    rng = np.random.default_rng(20 + C)
    with np.errstate(invalid='ignore'):
        for shape in ((5, 7, 9), (1, 1, 1), (12, 17, 31)):               # odd voxel counts
            d = special_data(rng, C, int(np.prod(shape))).reshape((C,) + shape)
            keep = d.copy()
            got = dc.create_nonzero_mask(d)
            assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == shape
            assert np.array_equal(got.cpu().numpy(), cropping.create_nonzero_mask(d))
            assert np.array_equal(bits(d), bits(keep))
            assert torch.equal(dc.create_nonzero_mask(torch.from_numpy(d).cuda()), got)


def test_crop_to_nonzero_equals_the_reference():
    from multitalent_amd.preprocessing import device_cropping as dc
    n = 0
    for name, c in golden_cases():
        seg = c.get('seg')
        for on_device in (False, True):
            di = torch.from_numpy(c['data']).cuda() if on_device else c['data'].copy()
            si = None if seg is None else (torch.from_numpy(seg).cuda() if on_device else seg.copy())
            d, s, bbox = dc.crop_to_nonzero(di, si, nonzero_label=-1)
            assert d.is_cuda and s.is_cuda and d.dtype == torch.float32, name
            assert bbox == c['bbox'].tolist() and all(type(v) is int for b in bbox for v in b), name
            dn, sn = d.cpu().numpy(), s.cpu().numpy()
            assert dn.shape == c['out_data'].shape and np.array_equal(bits(dn), bits(c['out_data'])), name
            assert sn.dtype == c['out_seg'].dtype and sn.shape == c['out_seg'].shape, name
            if sn.dtype == np.float32:
                assert np.array_equal(bits(sn), bits(c['out_seg'])), name
            else:
                assert np.array_equal(sn, c['out_seg']), name
            if not on_device:                                            # inputs are left as they were
                assert np.array_equal(bits(di), bits(c['data'])) and (seg is None or np.array_equal(bits(si), bits(seg))), name
        n += 1
    assert n == 8


def test_crop_to_nonzero_other_labels_and_two_seg_channels():
    """nonzero_label other than -1, and a seg with two channels: the mask broadcasts over them as on the host."""
    from multitalent_amd.preprocessing import cropping, device_cropping as dc
    c = dict(golden_cases())['two_channels_seg']
    seg2 = np.concatenate([c['seg'], np.roll(c['seg'], 3, axis=2)])
    for seg, label in ((None, -7), (seg2, -3), (c['seg'], 2.5)):
        hd, hs, hb = cropping.crop_to_nonzero(c['data'].copy(), None if seg is None else seg.copy(), nonzero_label=label)
        d, s, bbox = dc.crop_to_nonzero(c['data'], seg, nonzero_label=label)
        assert bbox == hb and np.array_equal(bits(d.cpu().numpy()), bits(hd))
        sn = s.cpu().numpy()
        assert sn.dtype == hs.dtype and np.array_equal(sn, hs)


def test_crop_to_nonzero_all_zero_raises():
    from multitalent_amd.preprocessing import cropping, device_cropping as dc
    z = np.zeros((2, 5, 6, 7), np.float32)
    z[1, 2, 3, 4] = -0.0
    with pytest.raises(ValueError):
        cropping.crop_to_nonzero(z.copy())
    with pytest.raises(ValueError):
        dc.crop_to_nonzero(z)
    with pytest.raises(ValueError):
        dc.crop_to_nonzero(torch.from_numpy(z).cuda(), torch.zeros((1, 5, 6, 7), device='cuda'))
    with pytest.raises(TypeError):
        dc.crop_to_nonzero(z.astype(np.float64))


def test_image_cropper_equals_the_host():
    from multitalent_amd.preprocessing import cropping, device_cropping as dc
    for name, c in golden_cases():
        seg = c.get('seg')
        if seg is not None:
            seg = seg.copy()
            seg[0, 1, 2, 3] = -4.0                                       # `seg[seg < -1] = 0` after `classes` was taken
        hd, hs, hp = cropping.ImageCropper.crop(c['data'].copy(), {}, None if seg is None else seg.copy())
        d, s, p = dc.ImageCropper.crop(c['data'].copy(), {}, None if seg is None else seg.copy())
        assert list(p) == list(hp) and p['crop_bbox'] == hp['crop_bbox'], name
        assert tuple(p['size_after_cropping']) == tuple(hp['size_after_cropping']), name
        assert p['classes'].dtype == hp['classes'].dtype, name
        assert np.array_equal(p['classes'], hp['classes'], equal_nan=p['classes'].dtype.kind == 'f'), name
        sn = s.cpu().numpy()
        assert sn.dtype == hs.dtype and np.array_equal(sn, hs, equal_nan=sn.dtype.kind == 'f'), name
        assert np.array_equal(bits(d.cpu().numpy()), bits(hd)), name


INTENSITY = {0: {'percentile_00_5': -950.0, 'percentile_99_5': 1100.0, 'mean': 60.0, 'sd': 310.0}}


def _ct_case(rng, shape):
    """a body of CT-like intensities with a zero border on every side (unequal margins), zero voxels inside it and one cavity"""
    D, H, W = shape
    z, y, x = np.ogrid[:D, :H, :W]
    body = ((z - D / 2 + 1) / (D / 2 - 3)) ** 2 + ((y - H / 2) / (H / 2 - 5)) ** 2 + ((x - W / 2 - 2) / (W / 2 - 6)) ** 2 <= 1
    vol = (rng.standard_normal(shape) * 300 + 40).astype(np.float32)
    vol[vol == 0] = 1.0
    vol[rng.random(shape) < 0.03] = 0
    vol[D // 2 - 2:D // 2 + 2, H // 2 - 3:H // 2 + 3, W // 2 - 4:W // 2 + 4] = 0
    vol[~body] = 0
    return vol


@pytest.mark.parametrize('transpose,spacing_xyz,with_seg', [((0, 1, 2), (0.9, 0.8, 2.5), False), ((0, 1, 2), (1.0, 1.0, 1.2), True),
                                                           ((2, 0, 1), (0.7, 0.8, 1.5), True)])
def test_preprocess_test_case_crops_on_the_device(tmp_path, monkeypatch, transpose, spacing_xyz, with_seg):
    import scipy.ndimage
    from multitalent_amd.preprocessing import cropping, preprocessing
    from multitalent_amd.preprocessing.device_preprocessing import resample_and_normalize_ct
    from multitalent_amd.utilities.nifti_io import write_image
    rng = np.random.default_rng(5)
    vol = _ct_case(rng, (28, 60, 52))
    f = str(tmp_path / 'case_0000.nii.gz')
    write_image(vol, f, spacing_xyz, (1.0, -2.0, 3.0))
    seg_file = None
    if with_seg:
        sg = rng.integers(0, 3, vol.shape).astype(np.uint8)
        sg[rng.random(vol.shape) < 0.6] = 0
        seg_file = str(tmp_path / 'case_seg.nii.gz')
        write_image(sg, seg_file, spacing_xyz, (1.0, -2.0, 3.0))
    target = [1.5, 1.0, 1.0]
    pre = preprocessing.GenericPreprocessor({0: 'CT'}, {0: False}, list(transpose), INTENSITY)

    # the host cropper first, feeding the same resampling kernels
    hd, hs, hp = cropping.ImageCropper.crop_from_list_of_files([f], seg_file)
    perm = (0, *[i + 1 for i in transpose])
    hdata, hseg, hprops = pre.resample_and_normalize(hd.transpose(perm), target, hp, hs.transpose(perm).copy(), None, return_device=True)
    assert tuple(hp['size_after_cropping']) != vol.shape                  # there was a border to cut
    assert not np.array_equal(scipy.ndimage.binary_fill_holes(vol != 0), vol != 0)      # and a hole to fill

    def boom(*a, **k):
        raise AssertionError("the host cropper was called")
    monkeypatch.setattr(cropping, 'create_nonzero_mask', boom)
    monkeypatch.setattr(cropping, 'binary_fill_holes', boom)
    monkeypatch.setattr(scipy.ndimage, 'binary_fill_holes', boom)

    for return_device in (True, False):
        data, seg, props = pre.preprocess_test_case([f], target, seg_file, return_device=return_device)
        assert list(props) == list(hprops)
        for k in hprops:
            a, b = props[k], hprops[k]
            if isinstance(b, np.ndarray):
                assert isinstance(a, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b), k
            else:
                assert a == b and type(a) is type(b), k
        if return_device:
            assert torch.is_tensor(data) and data.is_cuda and data.dtype == torch.float32 and torch.equal(data, hdata)
            assert torch.is_tensor(seg) and seg.is_cuda
            seg = seg.cpu().numpy()
        else:
            assert isinstance(data, np.ndarray) and data.dtype == np.float32 and np.array_equal(data, hdata.cpu().numpy())
            assert isinstance(seg, np.ndarray)
        assert seg.dtype == hseg.dtype == (np.float32 if with_seg else np.int64) and np.array_equal(seg, hseg)
        assert seg.shape[1:] == tuple(data.shape[1:])
