"""The device gzip encoder (csrc/deflate.hip through ops.deflate_gzip) against its restatement (deflate_host.py), byte for byte,
and the writers built on it: utilities.nifti_io.write_image for a device label map and the exporter."""
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_host as H  # noqa: E402

CHUNKS = (64, 1000, 1024)
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'export.npz')


def test_over_int32_max_is_refused_before_any_launch():
    """the argument check alone: nothing is allocated, the pointers are never followed"""
    import ctypes as C
    from multitalent_amd import _lib
    lib = _lib.load()
    fake, hist = C.c_void_p(4096), C.c_void_p(8192)
    pre = (C.c_uint8 * 352)()
    for npay, npre in ((2 ** 31, 0), (2 ** 31 - 352, 352), (2 ** 40, 0)):
        assert lib.mt_deflate_tokenize(fake, npay, pre, npre, 65536, fake, 1 << 40, hist, None) == -1                # MT_EINVAL
        assert b'INT32_MAX' in lib.mt_last_error()
        assert lib.mt_deflate_emit(fake, npay, pre, npre, 65536, fake, fake, 100, fake, 1 << 40, fake, 1 << 40, None) == -1
        assert lib.mt_deflate_workspace(npay + npre, 65536) == 0 and lib.mt_deflate_bound(npay + npre, 65536) == 0
    assert lib.mt_deflate_workspace(2 ** 31 - 1, 65536) > 2 ** 31 and lib.mt_deflate_workspace(100, 16) == 0
    assert lib.mt_deflate_tokenize(fake, 100, pre, 0, 16, fake, 1 << 40, hist, None) == -1                           # chunk below the minimum
    assert lib.mt_deflate_tokenize(fake, 100, pre, 513, 64, fake, 1 << 40, hist, None) == -1                          # prefix above the maximum
    assert lib.mt_deflate_tokenize(fake, 100, pre, 0, 64, fake, 16, hist, None) == -2                                 # MT_EWORKSPACE


def _encode(dev, x, npre, chunk):
    import torch
    from multitalent_amd import ops
    x = bytes(x)
    pay = torch.from_numpy(np.frombuffer(x[npre:], dtype=np.uint8).copy()).to(dev)
    return ops.deflate_gzip(pay, x[:npre], chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", CHUNKS)
def test_device_equals_restatement(dev, chunk):
    bad = []
    for name, x in H.cases(chunk).items():
        want = H.gzip_member(x, chunk)
        for npre in sorted({0, min(len(x), 352), min(len(x), 5)}):
            got = _encode(dev, x, npre, chunk)
            if got != want:
                bad.append((name, npre, len(got), len(want), next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), -1)))
    assert not bad, "(case, prefix bytes, bytes got, bytes wanted, first difference): %s" % bad


@pytest.fixture(scope='module')
def big():
    x = bytes(np.random.RandomState(9).randint(0, 256, 352).astype(np.uint8)) + H.SIZE_INPUTS['labels']().tobytes()
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [65536, 1024])
def test_large_label_map(dev, big, chunk):
    """64 x 96 x 300 voxels behind a 352-byte prefix: 29 chunks of 16 tiles at the product's chunk size, 1801 chunks at 1024"""
    import torch
    from multitalent_amd import ops
    assert ops.DEFLATE_CHUNK == 65536
    want = H.gzip_member(big, chunk)
    vol = torch.from_numpy(np.frombuffer(big[352:], dtype=np.uint8).copy()).to(dev).reshape(64, 96, 300)
    got = ops.deflate_gzip(vol, big[:352], chunk)
    assert got == want and gzip.decompress(got) == big
    assert ops.deflate_gzip(vol, big[:352], chunk) == got                      # two calls, identical bytes
    # a payload that is not dword aligned, and a compressed stream that needs the second read-back
    odd = torch.empty(len(big) - 352 + 3, dtype=torch.uint8, device=dev)[3:].copy_(vol.reshape(-1))
    head = ops._DEFLATE_HEAD
    try:
        ops._DEFLATE_HEAD = 1000
        assert ops.deflate_gzip(odd, big[:352], chunk) == want
    finally:
        ops._DEFLATE_HEAD = head


@pytest.mark.gpu
def test_encoder_refuses_what_it_does_not_serve(dev):
    import torch
    from multitalent_amd import ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.deflate_gzip(torch.zeros(10, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        ops.deflate_gzip(torch.zeros(10, dtype=torch.int16, device=dev))
    with pytest.raises(ValueError, match="limits"):
        ops.deflate_gzip(torch.zeros(10, dtype=torch.uint8, device=dev), bytes(513))


@pytest.mark.gpu
def test_write_image_from_the_device(dev, tmp_path):
    """a device label map written as .nii.gz reads back like today's `_write_nifti` file of the same input"""
    import torch
    from multitalent_amd.utilities.nifti_io import Image, _write_nifti, read_image, write_image
    arr = H.label_map((9, 33, 41), seed=4)
    d = (np.cos(0.3), -np.sin(0.3), 0, np.sin(0.3), np.cos(0.3), 0, 0, 0, 1)
    geo = ((0.8, 0.9, 2.5), (1.0, -2.0, 3.0), d)
    f_dev, f_host = str(tmp_path / 'dev.nii.gz'), str(tmp_path / 'host.nii.gz')
    write_image(torch.from_numpy(arr).to(dev), f_dev, *geo)
    _write_nifti(Image(arr, *geo), f_host)
    assert gzip.open(f_dev).read() == gzip.open(f_host).read()                # header and voxels, byte for byte
    a, b = read_image(f_dev), read_image(f_host)
    assert np.asarray(a.array).dtype == np.uint8 and np.array_equal(np.asarray(a.array), arr) and np.array_equal(np.asarray(b.array), arr)
    assert np.allclose(a.spacing, b.spacing, rtol=0, atol=0) and np.allclose(a.origin, b.origin, rtol=0, atol=0)
    assert np.allclose(a.direction, b.direction, rtol=0, atol=0) and np.allclose(a.spacing, geo[0], rtol=1e-6)
    with pytest.raises(TypeError):                                            # no silent copy of other device tensors to the host
        write_image(torch.from_numpy(arr).to(dev).short(), f_dev, *geo)


@pytest.mark.gpu
def test_exporter_writes_from_the_device(dev, tmp_path, monkeypatch):
    from test_export import _case
    from multitalent_amd import ops
    from multitalent_amd.inference import segmentation_export as se
    from multitalent_amd.utilities.nifti_io import read_image
    probs, props, order, force, _ = _case(np.load(G), 'iso_regions')
    props = dict(props, itk_spacing=(0.8, 0.9, 2.5), itk_origin=(1.0, -2.0, 3.0), itk_direction=tuple(np.eye(3).ravel()))
    before = se.resample_and_classify(probs, props, order, 1, force, 0).cpu().numpy()
    calls = []
    real = ops.deflate_gzip
    monkeypatch.setattr(ops, 'deflate_gzip', lambda *a, **k: calls.append(1) or real(*a, **k))
    out = str(tmp_path / 'a.nii.gz')
    ret = se.save_segmentation_nifti_from_softmax(probs, out, props, 1, order, None, None, None, None, force, 0, verbose=False)
    assert isinstance(ret, np.ndarray) and ret.dtype == np.uint8 and np.array_equal(ret, before) and len(calls) == 1
    im = read_image(out)
    assert np.array_equal(np.asarray(im.array), ret) and np.allclose(im.spacing, (0.8, 0.9, 2.5)) and np.allclose(im.origin, (1.0, -2.0, 3.0))
    dev_ret = se.export_label_map_device(probs, str(tmp_path / 'b.nii.gz'), props, 1, order, None, force, 0)
    assert dev_ret.is_cuda and np.array_equal(dev_ret.cpu().numpy(), before) and len(calls) == 2
    assert open(out, 'rb').read() == open(str(tmp_path / 'b.nii.gz'), 'rb').read()
    # a host post-processing function needs the host array: the host writer is used, as before
    flip = lambda s: (s.max() - s).astype(s.dtype)                            # noqa: E731
    post, raw = str(tmp_path / 'post.nii.gz'), str(tmp_path / 'raw.nii.gz')
    ret2 = se.save_segmentation_nifti_from_softmax(probs, post, props, 1, order, flip, (), None, raw, force, 0, verbose=False)
    assert len(calls) == 2 and np.array_equal(ret2, flip(before))
    assert np.array_equal(np.asarray(read_image(post).array), ret2) and np.array_equal(np.asarray(read_image(raw).array), before)
