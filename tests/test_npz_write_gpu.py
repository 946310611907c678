"""The device DEFLATE encoder at a period, as raw and segmented streams (ops.deflate_raw / deflate_segments), against its restatement
(deflate_period_host.py) byte for byte; the .npz writer built on it (utilities/npz_io.save_npz_device) against numpy; and the four
product paths that used to copy whole volumes to the host for np.savez_compressed."""
import os
import pickle
import sys
import zipfile
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import deflate_period_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
CHUNKS = (64, 1000, 1024)
GUARD = 64


def _payload(dev, data, offset=0):
    """the bytes as a uint8 device tensor between guard bytes (returned too, to be checked), `offset` bytes off a 256-byte boundary"""
    import torch
    buf = torch.full((GUARD + offset + len(data) + GUARD,), 0xa5, dtype=torch.uint8, device=dev)
    view = buf[GUARD + offset:GUARD + offset + len(data)]
    if len(data):
        view.copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()))
    return buf, view


def _first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


@pytest.mark.parametrize("period", H.PERIODS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_raw_stream_equals_restatement(dev, chunk, period):
    from multitalent_amd import ops
    bad = []
    for name, x in H.cases(chunk, period).items():
        wants = {final: H.raw(x, chunk, period, final) for final in (True, False)}
        for npre in sorted({0, min(len(x), 5), min(len(x), 128)}):
            for final in ((True, False) if npre in (0, 128) else (True,)):
                want = wants[final]
                buf, pay = _payload(dev, x[npre:], offset=1 if name in ('elements', 'ragged') else 0)
                got = ops.deflate_raw(pay, x[:npre], chunk, period, final)
                again = ops.deflate_raw(pay, x[:npre], chunk, period, final)
                if got != want or again != got:
                    bad.append((name, npre, final, len(got[0]), len(want[0]), _first_difference(got[0], want[0]), got[1:], want[1:]))
                elif final:
                    assert H.inflate(got[0]) == x and got[1] == zlib.crc32(x)
                assert bool((buf[:GUARD] == 0xa5).all()) and bool((buf[-GUARD:] == 0xa5).all())
    assert not bad, "(case, prefix bytes, final, bytes got, wanted, first difference, (crc, n) got, wanted): %s" % bad


@pytest.fixture(scope='module')
def softmax():
    return H.softmax_volume()


def test_softmax_volume_at_the_product_chunk(dev, softmax):
    """3 x 8 x 24 x 40 float16 probabilities with saturated regions behind their .npy header: 64 KiB chunks of 16 tiles; as a float16
    tensor (the encoder sees any contiguous tensor as bytes), with period 2 and, for comparison, 1"""
    import torch
    from multitalent_amd import ops
    assert ops.DEFLATE_CHUNK == 65536 and ops.DEFLATE_SEGMENT == 1 << 30 and ops.DEFLATE_SEGMENT % ops.DEFLATE_CHUNK == 0
    t = torch.from_numpy(softmax).to(dev)
    pre = H.npy_prefix(softmax)
    x = pre + softmax.tobytes()
    sizes = {}
    for period in (2, 1):
        want = H.raw(x, 65536, period)
        got = ops.deflate_raw(t, pre, period=period)
        assert got == want and ops.deflate_raw(t, pre, period=period) == got and H.inflate(got[0]) == x
        sizes[period] = len(got[0])
    assert (softmax == 1).mean() > 0.2 and sizes[2] < sizes[1]                 # matches at the element size are what makes it small


def test_segments_concatenate(dev):
    from multitalent_amd import ops
    rs = np.random.RandomState(5)
    x = np.repeat(rs.randint(0, 5, 2500).astype(np.float16), rs.randint(1, 8, 2500))[:10000].tobytes()
    assert len(x) == 20000
    for period, prefix, chunk in ((2, 0, 65536), (2, 128, 1024), (4, 5, 1000), (1, 0, 64)):
        buf, pay = _payload(dev, x[prefix:])
        seg = ops.deflate_segments(pay, x[:prefix], chunk, period, segment_bytes=5000)
        bodies = list(seg)
        want, crc, n = H.segments(x, chunk, period, 5000)
        assert len(bodies) == 4 and bodies == want and (seg.crc, seg.n, seg.compressed) == (crc, 20000, sum(len(b) for b in want))
        assert H.inflate(b''.join(bodies)) == x and seg.crc == zlib.crc32(x)
    with pytest.raises(ValueError, match="segments"):
        ops.deflate_segments(pay, bytes(128), 1024, 2, segment_bytes=100)


def test_encoder_refuses_what_it_does_not_serve(dev):
    import ctypes as C
    import torch
    from multitalent_amd import _lib, ops
    lib = _lib.load()
    fake, pre = C.c_void_p(4096), (C.c_uint8 * 8)()
    for period in (0, 3, 5, 16, -1):                                           # refused on the arguments alone: nothing is followed
        assert lib.mt_deflate_tokenize_period(fake, 100, pre, 0, 64, period, fake, 1 << 40, fake, None) == -1
        assert b'period' in lib.mt_last_error()
        assert lib.mt_deflate_emit_period(fake, 100, pre, 0, 64, period, 1, fake, fake, 100, fake, 1 << 40, fake, 1 << 40, None) == -1
    assert lib.mt_deflate_tokenize_period(fake, 2 ** 31, pre, 0, 65536, 2, fake, 1 << 40, fake, None) == -1
    with pytest.raises(ValueError, match="period"):
        ops.deflate_raw(torch.zeros(10, dtype=torch.float16, device=dev), period=3)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.deflate_raw(torch.zeros(10, dtype=torch.float16))
    with pytest.raises(ValueError, match="contiguous"):
        ops.deflate_raw(torch.zeros(10, 4, dtype=torch.float16, device=dev)[:, :2])


# ---- the writer ------------------------------------------------------------------------------------------------------------------

def _special(dtype, shape, seed):
    """values with subnormals, negative zero, infinities and constant stretches among them"""
    rs = np.random.RandomState(seed)
    a = rs.randn(*shape).astype(dtype)
    flat = a.reshape(-1)
    if a.dtype.kind == 'f':
        tiny = np.finfo(dtype).tiny
        flat[::7] = tiny / 4
        flat[1::11] = -0.0
        flat[2::13] = np.inf
        flat[len(flat) // 2:len(flat) // 2 + len(flat) // 4] = 1.0
    return a


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture
def guarded(monkeypatch):
    """guard bytes around every workspace and output buffer of the encoder; checked when the test is over"""
    import torch
    from multitalent_amd import ops
    made = []

    def alloc(nbytes, device):
        buf = torch.full((256 + nbytes + 256,), 0xa5, dtype=torch.uint8, device=device)
        made.append(buf)
        return buf[256:256 + nbytes]
    monkeypatch.setattr(ops, '_deflate_alloc', alloc)
    yield made
    assert made and all(bool((b[:256] == 0xa5).all()) and bool((b[-256:] == 0xa5).all()) for b in made)


@pytest.mark.parametrize("force", [False, True])
def test_writer_files_load_with_numpy(dev, tmp_path, force, guarded):
    import torch
    from multitalent_amd.utilities.npz_io import save_npz_device
    arrays = {'softmax': _special(np.float16, (3, 5, 7, 9), 0), 'data': _special(np.float32, (2, 8, 8, 8), 1),
              'wide': _special(np.float64, (3, 11), 2), 'labels': np.random.RandomState(3).randint(0, 4, (6, 50)).astype(np.uint8),
              'idx': np.arange(-40, 40, dtype=np.int64).reshape(8, 10) // 7, 'none': np.zeros((0, 3), np.float32)}
    padded = torch.full((3, 256), 0.25, dtype=torch.float16, device=dev)
    padded[:, :210] = torch.from_numpy(_special(np.float16, (3, 210), 4)).to(dev)
    view = padded[:, :210].unflatten(1, (5, 6, 7))                             # the padded-stride rows of the ensemble's mean
    assert not view.is_contiguous()
    tensors = {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
    f = save_npz_device(str(tmp_path / 'all'), _force_zip64=force, view=view, **tensors)
    assert f == str(tmp_path / 'all.npz') and os.listdir(str(tmp_path)) == ['all.npz']
    arrays['view'] = view.cpu().numpy()
    with np.load(f) as z:
        assert sorted(z.files) == sorted(arrays)
        for k, a in arrays.items():
            assert z[k].dtype == a.dtype and z[k].shape == a.shape and np.array_equal(_bits(z[k]), _bits(a)), k
    with zipfile.ZipFile(f) as z:
        assert z.testzip() is None and sorted(z.namelist()) == sorted(k + '.npy' for k in arrays)
        assert all(i.compress_type == zipfile.ZIP_DEFLATED and i.flag_bits == 0 for i in z.infolist())
    assert (b'PK\x06\x06' in open(f, 'rb').read()) == force
    # more than one segment per member, small chunks: the same arrays
    g = save_npz_device(str(tmp_path / 'seg.npz'), _chunk=1024, _segment_bytes=1000, **tensors)
    with np.load(g) as z:
        for k in tensors:
            assert np.array_equal(_bits(z[k]), _bits(arrays[k])), k
    with pytest.raises(TypeError, match="not written"):
        save_npz_device(str(tmp_path / 'bad.npz'), x=torch.zeros(4, dtype=torch.bfloat16, device=dev))
    with pytest.raises(TypeError, match="not written"):
        save_npz_device(str(tmp_path / 'bad.npz'), x=torch.zeros(4, dtype=torch.bool, device=dev))
    assert sorted(os.listdir(str(tmp_path))) == ['all.npz', 'seg.npz']


def test_file_size_against_numpy(dev, tmp_path):
    """the caps are the restatement's ratios (test_npz_write_cpu.test_size_against_numpy) x 1.1, rounded up to one decimal"""
    import torch
    from test_npz_write_cpu import SIZE_CAPS
    from multitalent_amd.utilities.npz_io import save_npz_device
    for name, make in H.SIZE_INPUTS.items():
        a = make()
        ours, theirs = str(tmp_path / (name + '_dev.npz')), str(tmp_path / (name + '_np.npz'))
        save_npz_device(ours, data=torch.from_numpy(a).to(dev))
        np.savez_compressed(theirs, data=a)
        assert np.array_equal(_bits(np.load(ours)['data']), _bits(a))
        ratio = os.path.getsize(ours) / os.path.getsize(theirs)
        print("%s: %d bytes against numpy's %d: %.3f (cap %.1f)" % (name, os.path.getsize(ours), os.path.getsize(theirs), ratio, SIZE_CAPS[name]))
        assert os.path.getsize(ours) == H.npz_member_size(a) + (30 + 8) + (46 + 8) + 22 and ratio <= SIZE_CAPS[name]


# ---- the drivers: nothing reaches np.savez_compressed ------------------------------------------------------------------------------

@pytest.fixture
def no_host_compression(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("np.savez_compressed: a device result was copied to the host to be compressed")
    monkeypatch.setattr(np, 'savez_compressed', boom)


def _small_softmax(dev, shape=(3, 6, 10, 14), seed=0):
    import torch
    return torch.softmax(6 * torch.from_numpy(np.random.RandomState(seed).randn(*shape).astype(np.float32)).to(dev), 0)


def test_exporter_stores_probabilities_from_the_device(dev, tmp_path, no_host_compression):
    from multitalent_amd.inference import segmentation_export as se
    p = _small_softmax(dev)
    props = {'size_after_cropping': (8, 12, 16), 'original_spacing': np.array([1.0, 1.0, 1.0]),
             'spacing_after_resampling': np.array([1.3, 1.2, 1.1])}
    want = se.resample_softmax(p.float(), (8, 12, 16), -1).cpu().numpy().astype(np.float16)         # what the host path stored
    npz = str(tmp_path / 'case.npz')
    ret = se._softmax_for_export(p, dict(props), 1, None, npz, None, 0)
    assert ret.is_cuda and ret.shape == p.shape
    got = np.load(npz)['softmax']
    assert got.dtype == np.float16 and got.shape == (3, 8, 12, 16) and np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert pickle.load(open(npz[:-4] + '.pkl', 'rb'))['size_after_cropping'] == (8, 12, 16)
    # a host array is uploaded for the resampling as before and stored from the device too
    se._softmax_for_export(p.cpu().numpy(), dict(props), 1, [1, 2, 3], str(tmp_path / 'host.npz'), None, 0)
    assert np.array_equal(np.load(str(tmp_path / 'host.npz'))['softmax'].view(np.uint16), want.view(np.uint16))


def test_merge_files_stores_the_mean_from_the_device(dev, tmp_path, monkeypatch):
    from multitalent_amd.inference.ensemble_predictions import merge_files, merge_on_device
    from multitalent_amd.utilities.nifti_io import read_image
    from test_ensemble_gpu import golden, write_members
    z, meta = golden()
    folders = write_members(z, meta['a'], str(tmp_path))
    monkeypatch.setattr(np, 'savez_compressed', lambda *a, **k: pytest.fail("np.savez_compressed was called"))
    for name, c in meta['a']['cases'].items():
        out = str(tmp_path / (name + '.nii.gz'))
        merge_files([os.path.join(f, name + '.npz') for f in folders], [os.path.join(f, name + '.pkl') for f in folders], out, True, True)
        mean, ref = np.load(out[:-7] + '.npz')['softmax'], z['a/merged/%s/mean' % name]
        assert mean.dtype == np.float16 and mean.shape == ref.shape and np.array_equal(mean.view(np.uint16), ref.view(np.uint16)), name
        assert np.array_equal(np.asarray(read_image(out).array), z['a/merged/%s/seg' % name])
        assert zipfile.ZipFile(out[:-7] + '.npz').testzip() is None
    # the new form of merge_on_device: the mean as a device view, the old form as a host array, the same values
    arrays = [z['a/%s/%s' % (f, name)] for f in meta['a']['folders']]
    from test_ensemble_gpu import case_properties
    p = case_properties(name, meta['a']['cases'][name], meta['a'])
    _, m_dev = merge_on_device(arrays, p, None, want_mean=True, mean_on_device=True)
    _, m_host = merge_on_device(arrays, p, None, want_mean=True)
    assert m_dev.is_cuda and isinstance(m_host, np.ndarray) and np.array_equal(m_dev.cpu().numpy().view(np.uint16), m_host.view(np.uint16))


def test_model_selection_merge_needs_no_host_compression(dev, tmp_path, monkeypatch):
    from multitalent_amd.evaluation.model_selection.ensemble import merge
    from multitalent_amd.utilities.nifti_io import read_image
    from test_ensemble_gpu import golden, write_members
    z, meta = golden()
    f0, f1 = meta['b']['members']
    write_members(z, meta['a'], str(tmp_path))
    monkeypatch.setattr(np, 'savez_compressed', lambda *a, **k: pytest.fail("np.savez_compressed was called"))
    for name in meta['a']['cases']:
        o = str(tmp_path / ('msel_' + name + '.nii.gz'))
        merge((str(tmp_path / f0 / (name + '.npz')), str(tmp_path / f1 / (name + '.npz')), str(tmp_path / f0 / (name + '.pkl')), o))
        assert np.array_equal(np.asarray(read_image(o).array), z['b/%s/seg' % name]), name


def test_preprocessor_writes_the_case_from_the_device(dev, tmp_path, monkeypatch):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from multitalent_amd.preprocessing.preprocessing import GenericPreprocessor
    rs = np.random.RandomState(0)
    data = (rs.randn(1, 8, 12, 16) * 40 + 100).astype(np.float32)
    seg = rs.randint(0, 3, (1, 8, 12, 16)).astype(np.float32)
    seg[:, :, :3] = -1
    src, dst = tmp_path / 'cropped', tmp_path / 'stage0'
    src.mkdir(), dst.mkdir()
    np.savez_compressed(src / 'c.npz', data=np.vstack((data, seg)))
    with open(src / 'c.pkl', 'wb') as f:
        pickle.dump({'original_spacing': np.array([1.0, 1.0, 1.0])}, f)
    ip = {0: {'mean': 100.0, 'sd': 40.0, 'percentile_00_5': 0.0, 'percentile_99_5': 200.0}}
    g = GenericPreprocessor({0: 'CT'}, {0: False}, [0, 1, 2], ip)
    target = np.array([1.0, 1.0, 1.0])
    d, s, props = g.load_cropped(str(src), 'c')
    want, _ = g.preprocess_training_case(d, s, props, target, [1, 2], None)
    want = want.cpu().numpy().astype(np.float32, copy=False)                   # what the host path handed to numpy's writer
    monkeypatch.setattr(np, 'savez_compressed', lambda *a, **k: pytest.fail("np.savez_compressed was called"))
    assert g._run_case(target, 'c', str(dst), str(src), None, [1, 2], None) is None
    got = np.load(dst / 'c.npz')['data']
    assert got.dtype == np.float32 and got.shape == (2, 8, 12, 16) and np.array_equal(_bits(got), _bits(want))
    assert set(pickle.load(open(dst / 'c.pkl', 'rb'))['class_locations']) == {1, 2}
    # with an executor the case is encoded here and the executor is handed compressed bytes only
    other = tmp_path / 'stage1'
    other.mkdir()
    seen = []

    class Writer(ThreadPoolExecutor):
        def submit(self, fn, *a):
            seen.extend(x for x in a if torch.is_tensor(x) or isinstance(x, np.ndarray))
            return ThreadPoolExecutor.submit(self, fn, *a)
    with Writer(max_workers=1) as w:
        g._run_case(target, 'c', str(other), str(src), None, [1, 2], w).result()
    assert not seen and np.array_equal(_bits(np.load(other / 'c.npz')['data']), _bits(want))


@pytest.mark.parametrize("with_seg", [True, False])
def test_cropper_writes_the_case_from_the_device(dev, tmp_path, monkeypatch, with_seg):
    from multitalent_amd.preprocessing.device_cropping import ImageCropper
    from multitalent_amd.preprocessing import cropping
    from multitalent_amd.utilities.nifti_io import write_image
    rs = np.random.RandomState(1)
    vol = np.zeros((8, 12, 16), np.float32)
    vol[1:7, 2:11, 3:12] = rs.randn(6, 9, 9).astype(np.float32) + 3
    files = [str(tmp_path / 'case_0000.nii.gz')]
    write_image(vol, files[0], (0.8, 0.9, 2.5))
    seg_file = None
    if with_seg:
        seg_file = str(tmp_path / 'case.nii.gz')
        write_image(rs.randint(0, 3, vol.shape).astype(np.uint8), seg_file, (0.8, 0.9, 2.5))
    hd, hs, hp = cropping.ImageCropper.crop_from_list_of_files(files, seg_file)          # the host cropper: vstack((data, seg))
    want = np.vstack((np.asarray(hd), np.asarray(hs)))
    monkeypatch.setattr(np, 'savez_compressed', lambda *a, **k: pytest.fail("np.savez_compressed was called"))
    out = tmp_path / 'out'
    ImageCropper(1, str(out)).load_crop_save(files + [seg_file], 'case')
    got = np.load(out / 'case.npz')['data']
    assert got.dtype == want.dtype and got.shape == want.shape == (2, 6, 9, 9) and np.array_equal(_bits(got), _bits(want))
    assert pickle.load(open(out / 'case.pkl', 'rb'))['crop_bbox'] == hp['crop_bbox']
    ImageCropper(2, str(tmp_path / 'run')).run_cropping([files + [seg_file]])
    assert np.array_equal(_bits(np.load(tmp_path / 'run' / 'case.npz')['data']), _bits(want))
