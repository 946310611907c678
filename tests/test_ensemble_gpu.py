"""`mt_ensemble_classify` against numpy, bit for bit, and the ensembling drivers against the REAL reference's output
(tests/golden/ensemble.npz from tools/oracle_gen/make_golden_ensemble.py).

The kernel's contract is numpy's `np.mean(float16_members, 0)`: float32 accumulation in member order, one IEEE division, one
round-to-nearest-even to float16 with subnormals kept; the label is decided on that rounded mean (argmax with the first maximum
winning, or the region thresholds painted in class order).  Everything is compared with `==`: no tolerance."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64                        # guard elements in front of and behind every output
OUT_FILL, GUARD_U8, GUARD_F16 = 7, 0xA5, 0x7BFF          # 0x7BFF = 65504.0, never a mean of probabilities


def make_members(K, C, shape, seed):
    """K float16 arrays [C, *shape]: softmax-like values, multiples of 1/8 (float16-equal means and means of exactly 0.5 occur),
    float16 subnormals and exact zeros; a voxel holds the same kind of value in every member."""
    rng = np.random.default_rng(seed)
    kind = rng.choice(4, size=shape, p=[0.4, 0.3, 0.2, 0.1])[None]
    out = []
    for _ in range(K):
        p = rng.random((C,) + shape, dtype=np.float32) ** 3
        p = (p / np.maximum(p.sum(0), 1e-6)).astype(np.float16)
        q = (rng.integers(0, 9, (C,) + shape) / 8.0).astype(np.float16)
        sub = rng.integers(0, 1024, (C,) + shape).astype(np.uint16).view(np.float16)
        z = np.where(rng.random((C,) + shape) < 0.6, 0.0, q).astype(np.float16)
        out.append(np.ascontiguousarray(np.where(kind == 0, p, np.where(kind == 1, q, np.where(kind == 2, sub, z))).astype(np.float16)))
    return out


def numpy_reference(members, order):
    """the reference's arithmetic (ensemble_predictions.py:28-30, segmentation_export.py:123-129)"""
    mean = np.mean(np.vstack([m[None] for m in members]), 0)
    assert mean.dtype == np.float16
    arg = mean.argmax(0).astype(np.uint8)
    reg = np.zeros(mean.shape[1:], dtype=np.uint8)
    for i, c in enumerate(order):
        reg[mean[i] > 0.5] = c
    return mean, arg, reg


def launch(members, shape, order, padded, offset, want_mean, full, lo, dev):
    """-> (labels [full] uint8, mean [C, *shape] float16 or None); asserts the guards and the pads of both outputs."""
    from multitalent_amd.inference.ensemble_predictions import ensemble_classify, padded_stride
    C = members[0].shape[0]
    V = int(np.prod(shape))
    cs = padded_stride(V) if padded else V
    views = []
    for m in members:
        buf = torch.zeros(8 + C * cs, dtype=torch.float16, device=dev)
        v = buf[offset:offset + C * cs]
        v.view(C, cs)[:, :V].copy_(torch.from_numpy(m.reshape(C, V)))
        views.append(v)
    nfull = int(np.prod(full))
    outbuf = torch.full((GUARD + nfull + GUARD,), GUARD_U8, dtype=torch.uint8, device=dev)
    out = outbuf[GUARD:GUARD + nfull].view(*full)
    out.fill_(OUT_FILL)
    mean = meanbuf = None
    if want_mean:
        meanbuf = torch.from_numpy(np.full(GUARD + C * cs + GUARD, GUARD_F16, dtype=np.uint16).view(np.float16)).to(dev)
        mean = meanbuf[GUARD:GUARD + C * cs]
    order_t = torch.tensor(order, dtype=torch.int32, device=dev) if order is not None else None
    ensemble_classify(views, C, shape, cs, out, lo, order_t, mean, cs)
    torch.cuda.synchronize()
    ob = outbuf.cpu().numpy()
    assert (ob[:GUARD] == GUARD_U8).all() and (ob[GUARD + nfull:] == GUARD_U8).all(), "guard bytes of the label volume were written"
    got_mean = None
    if want_mean:
        mb = meanbuf.cpu().numpy().view(np.uint16)
        assert (mb[:GUARD] == GUARD_F16).all() and (mb[GUARD + C * cs:] == GUARD_F16).all(), "guard elements of the mean were written"
        body = mb[GUARD:GUARD + C * cs].reshape(C, cs)
        assert (body[:, V:] == GUARD_F16).all(), "the pad behind a channel of the mean was written"
        got_mean = np.ascontiguousarray(body[:, :V]).view(np.float16).reshape((C,) + tuple(shape))
    return ob[GUARD:GUARD + nfull].reshape(full), got_mean


def expected_volume(lab, full, lo):
    e = np.full(full, OUT_FILL, dtype=np.uint8)
    e[lo[0]:lo[0] + lab.shape[0], lo[1]:lo[1] + lab.shape[1], lo[2]:lo[2] + lab.shape[2]] = lab
    return e


@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 5, 7), (8, 8, 8), (17, 31, 33)])
def test_kernel_equals_numpy(shape):
    dev = torch.device('cuda', 0)
    placements = [(tuple(s + e for s, e in zip(shape, (3, 4, 6))), (1, 2, 3)), (tuple(shape), (0, 0, 0))]
    for K in (1, 2, 3, 5, 16):
        for C in (1, 2, 5):
            members = make_members(K, C, shape, 1000 * K + 10 * C + shape[0])
            order = [3, 1, 4, 2, 9][:C]
            mean, arg, reg = numpy_reference(members, order)
            if shape == (17, 31, 33) and C == 5:
                srt = np.sort(mean.astype(np.float32), 0)
                assert int((srt[-1] == srt[-2]).sum()) > 0, "the input must hold a float16 tie of the two largest means"
                assert int(((mean != 0) & (np.abs(mean.astype(np.float32)) < 2.0 ** -14)).sum()) > 0, "and subnormal means"
            for regions in (False, True):
                for padded in (False, True):
                    for offset in (0, 1):
                        for want_mean in (False, True):
                            full, lo = placements[(int(padded) + offset + int(want_mean)) % 2]
                            what = "shape %s K %d C %d regions %d padded %d offset %d mean %d" % (shape, K, C, regions, padded, offset, want_mean)
                            lab, got = launch(members, shape, order if regions else None, padded, offset, want_mean, full, lo, dev)
                            assert np.array_equal(lab, expected_volume(reg if regions else arg, full, lo)), what
                            if want_mean:
                                assert np.array_equal(got.view(np.uint16), mean.view(np.uint16)), what
    # the same launch twice: identical; both placements of the widest configuration
    for full, lo in placements:
        a = launch(members, shape, None, True, 0, True, full, lo, dev)
        b = launch(members, shape, None, True, 0, True, full, lo, dev)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint16), b[1].view(np.uint16))
        assert np.array_equal(a[0], expected_volume(arg, full, lo)) and np.array_equal(a[1].view(np.uint16), mean.view(np.uint16))


def test_box_is_clipped_to_the_volume():
    """the insertion rule of mt_resample_classify: the offset lies inside the volume, the box is clipped to it"""
    dev = torch.device('cuda', 0)
    shape, full, lo = (5, 9, 11), (6, 8, 12), (2, 1, 4)
    members = make_members(3, 2, shape, 5)
    mean, arg, _ = numpy_reference(members, [1, 2])
    lab, got = launch(members, shape, None, True, 0, True, full, lo, dev)
    e = np.full(full, OUT_FILL, dtype=np.uint8)
    e[2:6, 1:8, 4:12] = arg[:4, :7, :8]
    assert np.array_equal(lab, e)
    assert np.array_equal(got.view(np.uint16), mean.view(np.uint16))          # the mean is the whole box


def test_bad_arguments_return_einval_without_a_launch():
    from multitalent_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    m = torch.zeros(4096, dtype=torch.float16, device=dev)
    out = torch.full((4, 4, 4), OUT_FILL, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(K, C, lo, full=(4, 4, 4)):
        ptrs = (ctypes.c_void_p * max(K, 1))(*([m.data_ptr()] * max(K, 1)))
        return lib.mt_ensemble_classify(ptrs, K, C, 2, 2, 2, 8, None, 0, out.data_ptr(), full[0], full[1], full[2], lo[0], lo[1], lo[2],
                                        None, 0, stream)

    assert call(2, 2, (1, 1, 1)) == 0
    torch.cuda.synchronize()
    assert int((out != OUT_FILL).sum()) == 8
    out.fill_(OUT_FILL)
    for K, C, lo in ((17, 2, (0, 0, 0)), (0, 2, (0, 0, 0)), (2, 256, (0, 0, 0)), (2, 0, (0, 0, 0)), (2, 2, (4, 0, 0)), (2, 2, (0, 0, 4)),
                     (2, 2, (0, -1, 0))):
        assert call(K, C, lo) == -1, (K, C, lo)                             # MT_EINVAL
        assert lib.mt_last_error()
    torch.cuda.synchronize()
    assert int((out != OUT_FILL).sum()) == 0, "a refused call must not launch"
    from multitalent_amd.inference.ensemble_predictions import ensemble_classify
    with pytest.raises(ValueError):
        ensemble_classify([m] * 17, 2, (2, 2, 2), 8, out, (0, 0, 0))


# ---- drivers against the golden -----------------------------------------------------------------------------------------------

def golden():
    return np.load(os.path.join(HERE, 'golden', 'ensemble.npz')), json.load(open(os.path.join(HERE, 'golden', 'ensemble.json')))


def case_properties(name, c, meta):
    sp = tuple(meta['spacing_zyx'])
    p = dict(list_of_data_files=['/raw/imagesTs/' + name + '_0000.nii.gz'], original_spacing=np.array(sp), spacing_after_resampling=np.array(sp),
             size_after_cropping=np.array(c['shape']), original_size_of_raw_data=np.array(c['full']),
             crop_bbox=[[c['lo'][i], c['lo'][i] + c['shape'][i]] for i in range(3)], itk_spacing=tuple(sp[::-1]),
             itk_origin=tuple(meta['origin']), itk_direction=tuple(np.eye(3).ravel()))
    if c['regions_class_order'] is not None:
        p['regions_class_order'] = list(c['regions_class_order'])
    return p


def write_members(z, meta, root):
    for f in meta['folders']:
        os.makedirs(os.path.join(root, f))
        for name, c in meta['cases'].items():
            np.savez_compressed(os.path.join(root, f, name + '.npz'), softmax=z['a/%s/%s' % (f, name)])
            with open(os.path.join(root, f, name + '.pkl'), 'wb') as fh:
                pickle.dump(case_properties(name, c, meta), fh)
    return [os.path.join(root, f) for f in meta['folders']]


def test_merge_matches_reference(tmp_path):
    from multitalent_amd.inference.ensemble_predictions import main, merge
    from multitalent_amd.utilities.nifti_io import read_image
    z, meta = golden()
    meta = meta['a']
    assert meta['equal_top2'] > 0
    folders = write_members(z, meta, str(tmp_path))
    pp = str(tmp_path / 'pp_merge.json')
    json.dump(meta['postprocessing'], open(pp, 'w'))
    out = str(tmp_path / 'merged')
    merge(folders, out, 2, override=True, postprocessing_file=pp, store_npz=True)
    assert json.load(open(os.path.join(out, 'pp_merge.json'))) == meta['postprocessing']
    for name, c in meta['cases'].items():
        raw = os.path.join(out, 'not_postprocessed', name)
        img = read_image(raw + '.nii.gz')
        seg = np.asarray(img.array)
        assert seg.dtype == np.uint8 and np.array_equal(seg, z['a/merged/%s/seg' % name]), name
        assert np.allclose(img.spacing, meta['spacing_zyx'][::-1]) and np.allclose(img.origin, meta['origin'])
        mean = np.load(raw + '.npz')['softmax']
        ref = z['a/merged/%s/mean' % name]
        assert mean.dtype == np.float16 and mean.shape == ref.shape and np.array_equal(mean.view(np.uint16), ref.view(np.uint16)), name
        props = pickle.load(open(raw + '.pkl', 'rb'))
        assert isinstance(props, list) and len(props) == len(folders)
        assert all(list(p['size_after_cropping']) == c['shape'] and p.get('regions_class_order') == c['regions_class_order'] for p in props)
        post = read_image(os.path.join(out, name + '.nii.gz'))
        assert np.array_equal(np.asarray(post.array), z['a/merged/%s/seg_pp' % name]), name
        assert np.allclose(post.spacing, meta['spacing_zyx'][::-1]) and np.allclose(post.origin, meta['origin'])
    # override=False keeps what is there
    f = os.path.join(out, 'not_postprocessed', 'caseA.nii.gz')
    before = os.stat(f).st_mtime_ns
    merge(folders, out, 2, override=False, postprocessing_file=pp, store_npz=True)
    assert os.stat(f).st_mtime_ns == before
    # the command line, without a postprocessing file: masks straight into the output folder, nothing else
    out2 = str(tmp_path / 'merged_cli')
    main(['-f'] + folders + ['-o', out2, '-t', '3'])
    assert sorted(os.listdir(out2)) == sorted(n + '.nii.gz' for n in meta['cases'])
    for name in meta['cases']:
        assert np.array_equal(np.asarray(read_image(os.path.join(out2, name + '.nii.gz')).array), z['a/merged/%s/seg' % name])


def test_model_selection_merge_matches_reference(tmp_path):
    from multitalent_amd.evaluation.model_selection.ensemble import merge
    from multitalent_amd.utilities.nifti_io import read_image
    z, meta = golden()
    f0, f1 = meta['b']['members']
    write_members(z, meta['a'], str(tmp_path))
    for name in meta['a']['cases']:
        o = str(tmp_path / ('msel_' + name + '.nii.gz'))
        args = (str(tmp_path / f0 / (name + '.npz')), str(tmp_path / f1 / (name + '.npz')), str(tmp_path / f0 / (name + '.pkl')), o)
        merge(args)
        img = read_image(o)
        assert np.array_equal(np.asarray(img.array), z['b/%s/seg' % name]), name
        assert np.allclose(img.spacing, meta['a']['spacing_zyx'][::-1]) and np.allclose(img.origin, meta['a']['origin'])
        before = os.stat(o).st_mtime_ns
        merge(args)                                                       # an existing file is kept (:28)
        assert os.stat(o).st_mtime_ns == before
