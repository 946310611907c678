"""Cropping to the non-zero region, host side (no GPU): the C ABI entries of the device cropper, no host fallback behind
`preprocessing/device_cropping.py`, and the host restatement `preprocessing/cropping.py` against the real reference's outputs
(tests/golden/cropping.npz from tools/oracle_gen/make_golden_cropping.py) - which pins the fixture the GPU tests compare with."""
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = {'mt_nonzero_mask': 'int', 'mt_fill_holes3d': 'int', 'mt_fill_holes3d_workspace': 'size_t', 'mt_crop_nonzero': 'int'}


def golden_cases():
    g = np.load(os.path.join(HERE, 'golden', 'cropping.npz'))
    for name in [str(n) for n in g['names']]:
        yield name, {k: g[name + '/' + k] for k in ('data', 'seg', 'out_data', 'out_seg', 'bbox') if name + '/' + k in g.files}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_header_and_signatures_declare_the_cropping_entries():
    from multitalent_amd import _lib
    txt = open(os.path.join(HERE, '..', 'include', 'mtseg.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for name, ret in ENTRIES.items():
        assert re.search(r'\b%s\s+%s\s*\(' % (ret, name), txt), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
    assert _lib.MT_ABI_VERSION == 4 and _lib.load().mt_abi_version() == 4


def test_workspace_query_and_argument_checks_need_no_device():
    """The size query is host arithmetic: 4 bytes per voxel (rounded up to 16) + 16.  Shapes beyond the int32 index range and a null
    pointer are refused before anything is launched."""
    from multitalent_amd import _lib
    lib = _lib.load()
    assert lib.mt_fill_holes3d_workspace(3, 5, 7) == ((3 * 5 * 7 * 4 + 15) // 16) * 16 + 16
    assert lib.mt_fill_holes3d_workspace(512, 512, 512) == 4 * 512 ** 3 + 16
    assert lib.mt_fill_holes3d_workspace(0, 5, 7) == 0
    assert lib.mt_fill_holes3d(None, 4, 4, 4, None, None, 0, None) == -1          # MT_EINVAL
    assert b'null pointer' in lib.mt_last_error()
    assert lib.mt_fill_holes3d(16, 2048, 2048, 1024, 16, 16, 1 << 40, None) == -1  # (never dereferenced) 2^32 voxels
    assert b'int32' in lib.mt_last_error()
    assert lib.mt_fill_holes3d(16, 8, 8, 8, 16, 16, 100, None) == -2                # MT_EWORKSPACE
    assert lib.mt_nonzero_mask(None, 1, 10, None, None) == -1


def test_no_host_fallback_without_a_device(monkeypatch):
    import torch
    from multitalent_amd.preprocessing import device_cropping as dc
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    data = np.zeros((1, 6, 7, 8), np.float32)
    data[0, 2:4, 2:5, 3:6] = 1.0
    seg = np.ones((1, 6, 7, 8), np.float32)
    keep_d, keep_s = data.copy(), seg.copy()
    mask = data[0] != 0
    for call in (lambda: dc.create_nonzero_mask(data), lambda: dc.fill_holes(mask), lambda: dc.get_bbox_from_mask(mask),
                 lambda: dc.crop_to_bbox(data[0], [[0, 2], [0, 2], [0, 2]]), lambda: dc.crop_to_nonzero(data, seg),
                 lambda: dc.crop_to_nonzero(data), lambda: dc.ImageCropper.crop(data, {}, seg),
                 lambda: dc.crop_to_nonzero(torch.from_numpy(data))):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
    assert np.array_equal(data, keep_d) and np.array_equal(seg, keep_s)


def test_host_cropper_reproduces_the_reference():
    """preprocessing/cropping.py == the reference on every golden case: data bit for bit, seg values and dtype, bbox."""
    from multitalent_amd.preprocessing.cropping import crop_to_nonzero
    n = 0
    for name, c in golden_cases():
        seg = c.get('seg')
        d, s, bbox = crop_to_nonzero(c['data'].copy(), None if seg is None else seg.copy(), nonzero_label=-1)
        assert np.asarray(bbox).tolist() == c['bbox'].tolist(), name
        assert d.dtype == np.float32 and d.shape == c['out_data'].shape and np.array_equal(bits(d), bits(c['out_data'])), name
        assert s.dtype == c['out_seg'].dtype and s.shape == c['out_seg'].shape, name
        if s.dtype == np.float32:
            assert np.array_equal(bits(s), bits(c['out_seg'])), name
        else:
            assert np.array_equal(s, c['out_seg']), name
        n += 1
    assert n == 8


def test_golden_cases_cover_what_they_claim():
    cases = dict(golden_cases())
    assert any('seg' in c for c in cases.values()) and any('seg' not in c for c in cases.values())
    assert {c['data'].shape[0] for c in cases.values()} == {1, 2}
    sp = cases['special_values_seg']['data']
    assert np.isnan(sp).any() and np.isinf(sp).any() and (sp == np.float32(1e-45)).any() and np.signbit(sp[sp == 0]).any()
    assert cases['no_border_seg']['bbox'].tolist() == [[0, s] for s in cases['no_border_seg']['data'].shape[1:]]
    assert all(max(c['data'].shape[1:]) <= 56 for c in cases.values())
    assert os.path.getsize(os.path.join(HERE, 'golden', 'cropping.npz')) < 1 << 20
