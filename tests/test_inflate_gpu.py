"""The device INFLATE decoder (csrc/inflate.hip through ops.inflate_raw) against its restatement (inflate_host.py): bytes, CRC, units
and chain positions on every kind of stream, statuses on damaged ones, guard bytes around input, workspace and output; the readers
built on it (utilities.npz_io.load_npz_device, utilities.nifti_io.read_image_device) against numpy and the host reader; and the
drivers that used to inflate on the host, with np.load and gzip.open taken away."""
import gzip
import os
import pickle
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import deflate_period_host as P  # noqa: E402
import inflate_host as I  # noqa: E402

GUARD = 256


def test_bad_arguments_are_refused_before_any_launch():
    """the argument checks alone: nothing is allocated, the pointers are never followed"""
    import ctypes as C
    from multitalent_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)
    assert lib.mt_inflate_workspace(0) == 0 and lib.mt_inflate_workspace(2 ** 31) == 0 and lib.mt_inflate_workspace(-5) == 0
    n = 100000
    cap, spans, blocks = n // 5 + 2, n // 6 + 2, -(-n // 4096)
    al = lambda v: (v + 15) & ~15                                              # noqa: E731
    assert lib.mt_inflate_workspace(n) == 64 + al(4 * blocks) + 3 * al(4 * cap) + 16 * cap + al(8 * cap) + 16 * spans
    assert [lib.mt_inflate_workspace_part(n, k) for k in range(4)] == [64 + al(4 * blocks), 64 + al(4 * blocks) + al(4 * cap) + 16 * cap, cap, 0]
    assert lib.mt_inflate_workspace_part(0, 0) == 0
    for args in ((fake, 0, 65536, 1, -1, fake, 1 << 40), (fake, 2 ** 31, 65536, 1, -1, fake, 1 << 40), (fake, 100, 0, 1, -1, fake, 1 << 40),
                 (fake, 100, 2 ** 30 + 1, 1, -1, fake, 1 << 40), (None, 100, 65536, 1, -1, fake, 1 << 40), (fake, 100, 65536, 1, -1, None, 1 << 40),
                 (fake, 100, 65536, 1, -1, C.c_void_p(4100), 1 << 40)):
        assert lib.mt_inflate_scan(*args, None) == -1, args                    # MT_EINVAL
    assert lib.mt_inflate_scan(fake, 100, 65536, 1, -1, fake, 16, None) == -2  # MT_EWORKSPACE
    assert lib.mt_inflate_write(fake, 100, fake, 1 << 40, 23, 0, fake, 10, None) == -1          # more units than 100 bytes can hold
    assert lib.mt_inflate_write(fake, 100, fake, 1 << 40, 1, 19, fake, 10, None) == -1
    assert lib.mt_inflate_write(fake, 100, fake, 16, 1, 0, fake, 10, None) == -2
    assert lib.mt_inflate_write(fake, 100, fake, 1 << 40, 1, 0, None, 10, None) == -1
    assert lib.mt_inflate_crc(fake, 100, 8, fake, None) == -1 and lib.mt_inflate_crc(fake, -1, 65536, fake, None) == -1
    assert lib.mt_inflate_crc(None, 100, 65536, fake, None) == -1


@pytest.fixture(scope='module')
def streams():
    """every stream of the CPU test with what the restatement makes of it, computed once"""
    out = {}
    for name, (body, x, final) in I.streams().items():
        data, crc, info = I.inflate(body, final=final)
        assert data == x
        out[name] = (body, x, final, crc, info)
    return out


@pytest.fixture
def guarded(monkeypatch):
    """guard bytes around every workspace and output buffer of the decoder; checked when the test is over"""
    import torch
    from multitalent_amd import ops
    made = []

    def alloc(nbytes, device):
        buf = torch.full((GUARD + nbytes + GUARD,), 0xa5, dtype=torch.uint8, device=device)
        made.append(buf)
        return buf[GUARD:GUARD + nbytes]
    monkeypatch.setattr(ops, '_deflate_alloc', alloc)
    yield made
    assert made and all(bool((b[:GUARD] == 0xa5).all()) and bool((b[-GUARD:] == 0xa5).all()) for b in made)


def _input(dev, body, offset=1):
    """the stream as a device tensor `offset` bytes off a 256-byte boundary, between guard bytes -> (whole buffer, view)"""
    import torch
    buf = torch.full((GUARD + offset + len(body) + GUARD,), 0xa5, dtype=torch.uint8, device=dev)
    view = buf[GUARD + offset:GUARD + offset + len(body)]
    view.copy_(torch.from_numpy(np.frombuffer(bytes(body), dtype=np.uint8).copy()))
    return buf, view


def _input_guards_ok(buf, n, offset=1):
    return bool((buf[:GUARD + offset] == 0xa5).all()) and bool((buf[GUARD + offset + n:] == 0xa5).all())


@pytest.mark.gpu
def test_inflate_raw_equals_restatement(dev, streams, guarded):
    from multitalent_amd import ops
    bad = []
    for name, (body, x, final, crc, ref) in streams.items():
        buf, comp = _input(dev, body, 1 + len(name) % 3)
        got = []
        for _ in range(2):
            out, c, info = ops.inflate_raw(comp, final=final, want_starts=True)
            got.append((out.cpu().numpy().tobytes(), c, info['units'], info['candidates'], info['spans'], info['bytes'],
                        info['starts'].cpu().tolist()))
        want = (x, crc, len(ref['units']), len(ref['candidates']), ref['spans'], len(x), ref['units'])
        if got[0] != want or got[1] != want or not _input_guards_ok(buf, len(body), 1 + len(name) % 3):
            first = next((i for i, (a, b) in enumerate(zip(got[0][0], x)) if a != b), -1)
            bad.append((name, len(body), got[0][1:6], want[1:6], first, got[0] == got[1]))
    assert not bad, "(stream, bytes, got, wanted (crc, units, candidates, spans, bytes), first difference, repeatable): %s" % bad


@pytest.mark.gpu
@pytest.mark.parametrize("period", P.PERIODS)
def test_round_trip_on_the_device(dev, period, guarded):
    """ops.deflate_raw / deflate_segments, then ops.inflate_raw, at the product's chunk of 64 KiB"""
    import torch
    from multitalent_amd import ops
    soft = P.softmax_volume((3, 16, 32, 48))
    case = P.training_case((2, 8, 24, 40))
    assert soft.nbytes > 2 * ops.DEFLATE_CHUNK and ops.INFLATE_UNIT_LIMIT == 16 * ops.DEFLATE_CHUNK
    for name, arr in (('softmax', soft), ('case', case)):
        t = torch.from_numpy(arr).to(dev)
        prefix = P.npy_prefix(arr)
        body, crc, n = ops.deflate_raw(t, prefix, ops.DEFLATE_CHUNK, period)
        x = prefix + arr.tobytes()
        out, c, info = ops.inflate_raw(_input(dev, body)[1], n_out=n)
        assert out.cpu().numpy().tobytes() == x and c == crc == zlib.crc32(x) and info['bytes'] == n == len(x), name
        assert 1 <= info['units'] <= -(-n // ops.DEFLATE_CHUNK)
    pay = torch.from_numpy(np.frombuffer(case.tobytes()[:20000], dtype=np.uint8).copy()).to(dev)
    seg = ops.deflate_segments(pay, b'', 1000, period, segment_bytes=5000)
    bodies = list(seg)
    assert len(bodies) == 4
    out, c, info = ops.inflate_raw(_input(dev, b''.join(bodies))[1], n_out=20000)
    assert out.cpu().numpy().tobytes() == case.tobytes()[:20000] and c == seg.crc and info['units'] >= 4
    out, c, info = ops.inflate_raw(_input(dev, bodies[0])[1], n_out=5000, final=False)      # one open segment on its own
    assert out.cpu().numpy().tobytes() == case.tobytes()[:5000]


@pytest.mark.gpu
def test_malformed_streams_give_their_status(dev, guarded):
    """each damaged stream was built and its status pinned on the CPU (test_inflate_cpu.py); here the device is only compared"""
    from multitalent_amd import ops
    cases = dict(I.malformed())
    x = np.repeat(np.random.RandomState(0).randint(0, 256, 40000).astype(np.uint8), 10).tobytes()
    cases['plain_zlib'] = (zlib.compress(x)[2:-4], {'unit_limit': 65536})
    cases['markers_only'] = (I.MARKER * 50, {})
    got, want = {}, {}
    for name, (body, kw) in cases.items():
        want[name] = I.scan(body, **kw)['status']
        buf, comp = _input(dev, body)
        try:
            ops.inflate_raw(comp, n_out=kw.get('n_expect'), unit_limit=kw.get('unit_limit', ops.INFLATE_UNIT_LIMIT))
            got[name] = (I.OK, None)
        except (ops.InflateForeign, IOError) as e:
            got[name] = (e.info['status'], type(e))
        assert _input_guards_ok(buf, len(body)), name
    assert {k: v[0] for k, v in got.items()} == want
    assert want['plain_zlib'] == I.TOO_LONG and want['markers_only'] == I.FOREIGN and I.OK not in want.values()
    for name, (status, kind) in got.items():
        assert kind is (ops.InflateForeign if status in (I.FOREIGN, I.TOO_LONG) else OSError), name


# ---- the readers -------------------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.gpu
def test_load_npz_device(dev, tmp_path, guarded):
    import torch
    from multitalent_amd.utilities.npz_io import load_npz_device, save_npz_device
    rs = np.random.RandomState(5)
    arrays = {'softmax': P.softmax_volume((3, 8, 24, 40)), 'data': P.training_case((2, 8, 24, 40)),
              'wide': rs.randn(3, 11).astype(np.float64) * (rs.rand(3, 11) > 0.5), 'labels': rs.randint(0, 4, (6, 50)).astype(np.uint8),
              'idx': np.arange(-40, 40, dtype=np.int64).reshape(8, 10) // 7, 'none': np.zeros((0, 3), np.float32),
              'noise': np.frombuffer(rs.bytes(140000), dtype=np.uint8).copy()}
    f = save_npz_device(str(tmp_path / 'dev.npz'), **{k: torch.from_numpy(v).to(dev) for k, v in arrays.items()})
    with np.load(f) as z:
        for key, a in arrays.items():
            st = {}
            t = load_npz_device(f, key, dev, stages=st)
            assert st['path'] == 'device' and t.is_cuda and tuple(t.shape) == a.shape and str(t.dtype) == 'torch.' + a.dtype.name, key
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(z[key])) and np.array_equal(_bits(z[key]), _bits(a)), key
            assert load_npz_device(f, key, dev, fallback=False).shape == t.shape
    with pytest.raises(KeyError):
        load_npz_device(f, 'missing', dev)
    # files of other writers: a stream without restart points (longer than the unit limit) and a stored member take the host path
    big = np.repeat(rs.randint(0, 200, 150000).astype(np.uint8), 10).reshape(1500, 1000)
    g, h = str(tmp_path / 'numpy.npz'), str(tmp_path / 'stored.npz')
    np.savez_compressed(g, big=big, small=arrays['idx'])
    np.savez(h, big=big)
    for fname in (g, h):
        st = {}
        t = load_npz_device(fname, 'big', dev, stages=st)
        assert st['path'] == 'host' and np.array_equal(t.cpu().numpy(), big)
        with pytest.raises(ValueError, match="not read on the device"):
            load_npz_device(fname, 'big', dev, fallback=False)
    st = {}                                                                    # a short zlib stream is one unit: decoded where it is
    assert np.array_equal(load_npz_device(g, 'small', dev, stages=st).cpu().numpy(), arrays['idx']) and st['path'] == 'device'
    fo = str(tmp_path / 'fortran.npz')
    np.savez_compressed(fo, a=np.asfortranarray(arrays['idx']))
    st = {}
    assert np.array_equal(load_npz_device(fo, 'a', dev, stages=st).cpu().numpy(), arrays['idx']) and st['path'] == 'host'
    # a valid member of another writer that the unit rules refuse (sync flushes keep the dictionary): zlib reads it, as before
    small = big.reshape(-1)[:200000].reshape(200, 1000)
    sy = P.npy_prefix(small) + small.tobytes()
    from multitalent_amd.utilities.npz_io import HostBodies, write_npz_members
    body = I.zlib_sync_flushed(sy, 6, 30000)
    assert I.scan(body)['status'] == I.BAD
    s = write_npz_members(str(tmp_path / 'sync.npz'), [('a', len(sy), HostBodies([body], zlib.crc32(sy)))])
    st = {}
    assert np.array_equal(load_npz_device(s, 'a', dev, stages=st).cpu().numpy(), small) and st['path'] == 'host'
    with pytest.raises(IOError, match="damaged"):
        load_npz_device(s, 'a', dev, fallback=False)
    # one flipped payload byte: the CRC-32 of the zip header catches what the stream's structure does not
    from multitalent_amd.utilities.npz_io import locate_member
    m = locate_member(f, 'noise')
    blob = bytearray(open(f, 'rb').read())
    body = bytes(blob[m['offset']:m['offset'] + m['csize']])
    spans = [s for u in I.scan(body)['units'] for s in I.decode_unit(body, u)['spans']]
    assert spans, "random bytes are stored"
    blob[m['offset'] + spans[0][0] + 7] ^= 0x20
    bad = str(tmp_path / 'flipped.npz')
    open(bad, 'wb').write(bytes(blob))
    with pytest.raises(IOError, match="CRC-32"):
        load_npz_device(bad, 'noise', dev)
    assert np.array_equal(_bits(load_npz_device(bad, 'softmax', dev).cpu().numpy()), _bits(arrays['softmax']))       # the others are whole


@pytest.mark.gpu
def test_read_image_device(dev, tmp_path, guarded):
    import torch
    from multitalent_amd.utilities import nifti_io as N
    rs = np.random.RandomState(4)
    arr = np.repeat(rs.randint(0, 5, (9, 33, 6)).astype(np.uint8), 7, axis=2)[:, :, :41]
    geo = ((0.8, 0.9, 2.5), (1.0, -2.0, 3.0), (np.cos(0.3), -np.sin(0.3), 0, np.sin(0.3), np.cos(0.3), 0, 0, 0, 1))
    f = str(tmp_path / 'dev.nii.gz')
    N.write_label_map_device(torch.from_numpy(arr).to(dev), f, *geo)
    ref = N._read_nifti(f)
    st = {}
    vox, spacing, origin, direction = N.read_image_device(f, dev, st)
    assert st['path'] == 'device' and vox.is_cuda and vox.dtype == torch.uint8 and np.array_equal(vox.cpu().numpy(), ref.array)
    assert np.array_equal(ref.array, arr) and spacing == ref.spacing and origin == ref.origin and direction == ref.direction
    # a host-written int16 volume (one zlib stream, short enough to be one unit) and one with a slope: the host path decides the values
    vol = rs.randint(-300, 900, (5, 6, 7)).astype(np.int16)
    g = str(tmp_path / 'host.nii.gz')
    N._write_nifti(N.Image(vol, *geo), g)
    st = {}
    vox, spacing, _, _ = N.read_image_device(g, dev, st)
    assert st['path'] == 'device' and vox.dtype == torch.int16 and np.array_equal(vox.cpu().numpy(), vol) and spacing == N._read_nifti(g).spacing
    raw = bytearray(gzip.open(g).read())
    raw[112:120] = np.array([2.0, 1.0], '<f4').tobytes()                      # scl_slope, scl_inter
    open(g, 'wb').write(gzip.compress(bytes(raw)))
    st = {}
    vox, _, _, _ = N.read_image_device(g, dev, st)
    assert st['path'] == 'host' and np.array_equal(vox.cpu().numpy(), vol.astype(np.float64) * 2 + 1)
    # a valid .nii.gz of another writer whose sync flushes (pigz does this) the unit rules refuse: the host reader reads it, as before
    vol2 = np.repeat(rs.randint(0, 5, (12, 40, 10)).astype(np.int16), 5, axis=2)
    h = str(tmp_path / 'sync.nii.gz')
    N._write_nifti(N.Image(vol2, *geo), h)
    plain = gzip.open(h).read()
    body = I.zlib_sync_flushed(plain, 6, 5000)
    assert I.scan(body)['status'] == I.BAD
    from multitalent_amd.utilities import deflate_host
    open(h, 'wb').write(deflate_host.gzip_member(body, zlib.crc32(plain), len(plain)))
    st = {}
    vox, spacing, _, _ = N.read_image_device(h, dev, st)
    assert st['path'] == 'host' and np.array_equal(vox.cpu().numpy(), vol2) and spacing == N._read_nifti(h).spacing
    blob = bytearray(open(f, 'rb').read())
    blob[-6] ^= 1                                                             # the CRC-32 of the trailer
    open(f, 'wb').write(bytes(blob))
    with pytest.raises(IOError, match="CRC-32"):
        N.read_image_device(f, dev)


# ---- the drivers: nothing reaches np.load or gzip.open -------------------------------------------------------------------------------

@pytest.fixture
def no_host_inflate(monkeypatch):
    """armed by calling it: from then on np.load and gzip.open raise"""
    def arm():
        def boom(*a, **k):
            raise AssertionError("a file this package wrote was inflated on the host")
        monkeypatch.setattr(np, 'load', boom)
        monkeypatch.setattr(gzip, 'open', boom)
    return arm


@pytest.mark.gpu
def test_ensemble_reads_its_members_on_the_device(dev, tmp_path, no_host_inflate):
    import torch
    from multitalent_amd.inference.ensemble_predictions import _load_case, merge_files
    from multitalent_amd.utilities.npz_io import save_npz_device
    from test_ensemble_gpu import golden, write_members
    z, meta = golden()
    folders = write_members(z, meta['a'], str(tmp_path))
    name = sorted(meta['a']['cases'])[0]
    files, pkls = [os.path.join(f, name + '.npz') for f in folders], [os.path.join(f, name + '.pkl') for f in folders]
    host_out = str(tmp_path / 'host.nii.gz')
    merge_files(files, pkls, host_out, True, True)                              # numpy-written members: the fallback inside the reader
    for f, folder in zip(files, meta['a']['folders']):
        save_npz_device(f, softmax=torch.from_numpy(z['a/%s/%s' % (folder, name)]).to(dev))
    want_seg, want_mean = open(host_out, 'rb').read(), open(host_out[:-7] + '.npz', 'rb').read()
    no_host_inflate()
    arrays, props, order = _load_case(files, pkls)
    assert all(torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float16 for a in arrays)
    out = str(tmp_path / 'dev.nii.gz')
    merge_files(files, pkls, out, True, True)
    assert open(out, 'rb').read() == want_seg and open(out[:-7] + '.npz', 'rb').read() == want_mean


@pytest.mark.gpu
def test_case_cache_fills_from_npz_on_the_device(dev, tmp_path, no_host_inflate):
    import torch
    from multitalent_amd.training.dataloading.device_loading import DeviceCaseCache
    from multitalent_amd.utilities.npz_io import save_npz_device
    case = P.training_case((3, 8, 24, 40))
    case[-1] = np.round(case[-1])
    f = save_npz_device(str(tmp_path / 'case.npz'), data=torch.from_numpy(case).to(dev))
    entry = {'data_file': f, 'properties': {'k': 1}}
    host = DeviceCaseCache(dev, 1 << 30).admit(entry, all_data=case)
    no_host_inflate()
    cache = DeviceCaseCache(dev, 1 << 30)
    res = cache.admit(entry)
    assert res is not None and cache.used_bytes == DeviceCaseCache.case_bytes(case.shape) and res.shape == case.shape[1:]
    assert res.data.dtype == torch.float32 and res.seg.dtype == torch.int16 and res.data.is_contiguous() and res.seg.is_contiguous()
    assert torch.equal(res.data, host.data) and torch.equal(res.seg, host.seg) and np.array_equal(_bits(res.data.cpu().numpy()), _bits(case[:-1]))
    assert DeviceCaseCache(dev, 1000).admit(entry) is None


@pytest.mark.gpu
def test_device_loader_admits_npz_cases_without_a_host_inflate(dev, tmp_path, no_host_inflate):
    """DeviceDataLoader3D.generate_train_batch on cases that exist as .npz only: every case fits the cache, so each is admitted
    through the device reader from plan_batch, and the batches are the host loader's"""
    import torch
    import device_loading_cases as DC
    from multitalent_amd.training.dataloading import dataset_loading as dl
    from multitalent_amd.training.dataloading.device_loading import DeviceCaseCache, DeviceDataLoader3D
    from multitalent_amd.utilities.npz_io import save_npz_device
    DC.write_synthetic(str(tmp_path))
    ds = dl.load_dataset(str(tmp_path))
    ps, B = DC.SYNTH_PATCH, 5
    kw = dict(oversample_foreground_percent=0.5, pad_mode='edge', memmap_mode='r')
    np.random.seed(11)
    host = dl.DataLoader3D(ds, ps, ps, B, False, **kw)
    want = [next(host) for _ in range(2)]
    for e in ds.values():                                                       # .npz only, written by the device writer
        arr = np.load(e['data_file'][:-4] + '.npy')
        os.remove(e['data_file'][:-4] + '.npy')
        save_npz_device(e['data_file'], data=torch.from_numpy(arr).to(dev))
    cache = DeviceCaseCache(dev, 1 << 30)
    small = DeviceCaseCache(dev, 1000)
    no_host_inflate()
    np.random.seed(11)
    loader = DeviceDataLoader3D(ds, ps, ps, B, False, cache=cache, **kw)
    drawn = set()
    for w in want:
        b = loader.generate_train_batch()
        drawn.update(str(k) for k in w['keys'])
        assert [str(k) for k in b['keys']] == [str(k) for k in w['keys']]
        assert np.array_equal(b['data'].cpu().numpy(), w['data']) and np.array_equal(b['seg'].cpu().numpy(), w['seg'])
    assert len(cache) == len(drawn) and cache.used_bytes == sum(DeviceCaseCache.case_bytes((3,) + cache.get(f).shape) for f in cache.resident_files())
    # a case that cannot stay is refused from its header: nothing is inflated anywhere (np.load would raise)
    e = next(iter(ds.values()))
    assert not small.room_for(e) and small.admit(e) is None and cache.room_for(e)


@pytest.mark.gpu
def test_preprocessor_and_analyzer_read_the_cropped_case_on_the_device(dev, tmp_path, no_host_inflate):
    import torch
    from multitalent_amd.experiment_planning.DatasetAnalyzer import DatasetAnalyzer
    from multitalent_amd.preprocessing.preprocessing import GenericPreprocessor
    from multitalent_amd.utilities.npz_io import save_npz_device
    rs = np.random.RandomState(0)
    data = (rs.randn(1, 8, 12, 16) * 40 + 100).astype(np.float32)
    seg = rs.randint(0, 3, (1, 8, 12, 16)).astype(np.float32)
    seg[:, :, :3] = -1
    both = np.vstack((data, seg))
    host, src = tmp_path / 'host', tmp_path / 'cropped'
    host.mkdir(), src.mkdir()
    np.savez_compressed(host / 'c.npz', data=both)
    save_npz_device(str(src / 'c.npz'), data=torch.from_numpy(both).to(dev))
    for d in (host, src):
        with open(d / 'c.pkl', 'wb') as f:
            pickle.dump({'original_spacing': np.array([1.0, 1.0, 1.0])}, f)
    g = GenericPreprocessor({0: 'CT'}, {0: False}, [0, 1, 2], {0: {'mean': 100.0, 'sd': 40.0, 'percentile_00_5': 0.0, 'percentile_99_5': 200.0}})
    target = np.array([1.0, 1.0, 1.0])
    want, _ = g.preprocess_training_case(data.copy(), seg.copy(), {'original_spacing': np.array([1.0, 1.0, 1.0])}, target, [1, 2], None)

    class A(DatasetAnalyzer):                                                   # the reads alone: no dataset.json is needed for them
        def __init__(self, folder):
            self.folder_with_cropped_data = folder
    want_case = np.load(host / 'c.npz')['data']
    no_host_inflate()
    d, s, props = g.load_cropped(str(src), 'c')
    assert torch.is_tensor(d) and d.is_cuda and d.dtype == torch.float32 and tuple(s.shape) == (1, 8, 12, 16)
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(data)) and np.array_equal(_bits(s.cpu().numpy()), _bits(seg))
    got, _ = g.preprocess_training_case(d, s, props, target, [1, 2], None)
    assert torch.equal(got, want)
    a = A(str(src))._load_case_device('c')
    assert a.is_cuda and np.array_equal(_bits(a.cpu().numpy()), _bits(want_case))
    assert torch.equal(DatasetAnalyzer._float32_on_device(a[-1]), DatasetAnalyzer._float32_on_device(want_case[-1]))


@pytest.mark.gpu
def test_load_remove_save_reads_the_label_map_on_the_device(dev, tmp_path, no_host_inflate):
    import torch
    from multitalent_amd.postprocessing.connected_components import load_remove_save
    from multitalent_amd.utilities import nifti_io as N
    rs = np.random.RandomState(3)
    arr = np.zeros((10, 20, 24), np.uint8)
    arr[1:6, 2:12, 3:14] = 1
    arr[7:9, 15:18, 18:22] = 1                                                 # a second, smaller component of class 1
    arr[2:4, 14:19, 2:9] = 2
    arr[rs.rand(*arr.shape) > 0.995] = 0
    geo = ((0.8, 0.9, 2.5), (1.0, -2.0, 3.0), tuple(np.eye(3).ravel()))
    dev_in, host_in = str(tmp_path / 'dev_in.nii.gz'), str(tmp_path / 'host_in.nii.gz')
    N.write_label_map_device(torch.from_numpy(arr).to(dev), dev_in, *geo)
    N._write_nifti(N.Image(arr, *geo), host_in)
    host_out, dev_out = str(tmp_path / 'host_out.nii.gz'), str(tmp_path / 'dev_out.nii.gz')
    want = load_remove_save(host_in, host_out, [1, 2])
    want_file = open(host_out, 'rb').read()
    no_host_inflate()
    got = load_remove_save(dev_in, dev_out, [1, 2])
    assert got == want and got[0][1] is not None and open(dev_out, 'rb').read() == want_file
