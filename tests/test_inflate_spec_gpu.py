"""The device decoder for DEFLATE streams without restart points (csrc/inflate_spec.hip through ops.inflate_stream) against its
restatement (inflate_spec_host.py): bytes, CRC, candidates, chain and statuses on every stream of the CPU test, guard bytes around
input, workspaces and output; the readers' second route on files of other writers (numpy, gzip, sync-flushed bodies) against np.load
and the host reader; and the call sites that inherit it, with np.load and gzip.open taken away."""
import gzip
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import inflate_host as I  # noqa: E402
import inflate_spec_host as S  # noqa: E402

GUARD = 256
ANY_SPAN = 1 << 30
CHUNKS = {'long_matches': (256, 4096), 'false_candidates': (64, 256), 'last_byte': (64, 256), 'ct_l6_m1': (64, 256)}


def test_bad_arguments_are_refused_before_any_launch():
    """the argument checks alone: nothing is allocated, the pointers are never followed"""
    import ctypes as C
    from multitalent_amd import _lib
    lib = _lib.load()
    fake, big = C.c_void_p(4096), 1 << 40
    for n, chunk in ((0, 8192), (2 ** 31, 8192), (-5, 8192), (100, 32), (100, 1 << 21), (100, 3000)):
        assert lib.mt_inflate_spec_workspace(n, chunk) == 0 and lib.mt_inflate_spec_workspace_part(n, chunk, 0) == 0
    n, chunk = 100000, 256
    nch = -(-n // chunk)
    al = lambda v: (v + 15) & ~15                                              # noqa: E731
    assert lib.mt_inflate_spec_workspace(n, chunk) == 64 + al(4 * nch) + al(8 * nch) + al(8 * (nch + 1)) + al(24 * (nch + 1)) \
        + 2 * al(4 * (nch + 1)) + al(8 * (nch + 1))
    assert lib.mt_inflate_spec_workspace_part(n, chunk, 2) == nch + 1 and lib.mt_inflate_spec_workspace_part(n, chunk, 3) == 0
    assert lib.mt_inflate_spec_write_workspace(3, 2, 1000) == 2000 + 3 * 32768 + 2 * 16
    assert lib.mt_inflate_spec_write_workspace(-1, 0, 10) == 0 and lib.mt_inflate_spec_write_workspace(1, 0, -1) == 0
    good = (fake, 100, 64, 1 << 30, 4096, -1, 7, fake, big)
    assert lib.mt_inflate_spec_scan(*good[:7], fake, 16, None) == -2           # MT_EWORKSPACE
    for k, v in ((1, 0), (1, 2 ** 31), (2, 100), (2, 32), (2, 1 << 21), (3, 0), (3, 2 ** 30 + 1), (4, 0), (6, 0), (6, 8), (0, None), (7, None),
                 (7, C.c_void_p(4100))):
        args = list(good)
        args[k] = v
        assert lib.mt_inflate_spec_scan(*args, None) == -1, (k, v)             # MT_EINVAL
    write = (fake, 100, 64, fake, big, 1, 0, fake, big, fake, 10, 7)
    assert lib.mt_inflate_spec_write(*write[:4], 16, *write[5:], None) == -2
    assert lib.mt_inflate_spec_write(*write[:8], 16, *write[9:], None) == -2
    for k, v in ((1, 0), (2, 100), (5, 4), (5, -1), (6, 22), (6, -1), (10, -1), (11, 0), (11, 8), (0, None), (3, None), (7, None), (9, None),
                 (3, C.c_void_p(4100)), (7, C.c_void_p(4104))):
        args = list(write)
        args[k] = v
        assert lib.mt_inflate_spec_write(*args, None) == -1, (k, v)


@pytest.fixture(scope='module')
def streams():
    """every stream of the CPU test with what the restatement makes of it at the chunk sizes it is run at, computed once"""
    out = {}
    for name, (body, x) in S.streams().items():
        hits, blocks = S.accepted(body), {}
        for chunk in CHUNKS.get(name, (256,)):
            data, crc, info = S.inflate(body, chunk, span_limit=ANY_SPAN, hits=hits, blocks=blocks)
            assert data == x
            out[name, chunk] = (body, x, crc, info)
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
def test_inflate_stream_equals_restatement(dev, streams, guarded):
    from multitalent_amd import ops
    bad = []
    for (name, chunk), (body, x, crc, ref) in streams.items():
        off = 1 + len(name) % 3
        buf, comp = _input(dev, body, off)
        got = []
        for _ in range(2):
            out, c, info = ops.inflate_stream(comp, chunk=chunk, span_limit=ANY_SPAN, want_starts=True)
            got.append((out.cpu().numpy().tobytes(), c, info['units'], info['spans'], info['bytes'], info['shortest_unit'], info['max_reach'],
                        info['positions'].cpu().tolist(), info['starts'].cpu().tolist()))
        want = (x, crc, len(ref['units']), ref['spans'], len(x), ref['shortest_unit'], ref['max_reach'], ref['candidates'], ref['units'])
        if got[0] != want or got[1] != want or not _input_guards_ok(buf, len(body), off):
            first = next((i for i, (a, b) in enumerate(zip(got[0][0], x)) if a != b), -1)
            bad.append((name, chunk, len(body), got[0][1:7], want[1:7], got[0][7] == want[7], got[0][8] == want[8], first, got[0] == got[1]))
    assert not bad, ("(stream, chunk, bytes, got, wanted (crc, units, spans, bytes, shortest unit, reach), same candidates, same chain, "
                     "first difference, repeatable): %s" % bad)


@pytest.mark.gpu
def test_expected_size_and_default_span_limit(dev, streams, guarded):
    from multitalent_amd import ops
    body, x, crc, ref = streams['ct_l6_m8', 256]
    out, c, info = ops.inflate_stream(_input(dev, body)[1], n_out=len(x), chunk=4096)
    assert out.cpu().numpy().tobytes() == x and c == crc and info['status'] == 'OK'
    with pytest.raises(ops.InflateForeign):                                     # 64 chunks of 64 bytes do not reach the second block
        ops.inflate_stream(_input(dev, body)[1], chunk=64)
    with pytest.raises(ValueError):
        ops.inflate_stream(_input(dev, body)[1], chunk=100)


@pytest.mark.gpu
def test_damaged_streams_give_their_status(dev, guarded):
    """each damaged stream was built and its status pinned on the CPU (test_inflate_spec_cpu.py); here the device is only compared"""
    from multitalent_amd import ops
    got, want = {}, {}
    for name, (body, chunk, kw, data) in S.malformed().items():
        ref, ref_crc, info = S.inflate(body, chunk, **kw)
        want[name] = info['status']
        buf, comp = _input(dev, body)
        try:
            out, crc, _ = ops.inflate_stream(comp, n_out=kw.get('n_expect'), chunk=chunk, **({'span_limit': kw['span_limit']} if 'span_limit' in kw else {}))
            got[name] = S.OK
            assert out.cpu().numpy().tobytes() == ref == data and crc == ref_crc, name
        except (ops.InflateForeign, IOError) as e:
            got[name] = e.info['status']
            assert type(e) is (ops.InflateForeign if got[name] == S.TOO_LONG else OSError), name
        assert _input_guards_ok(buf, len(body)), name
    assert got == want and sorted(set(want.values())) == sorted([S.OK, S.TOO_LONG, S.BAD, S.CORRUPT, S.SIZE])


# ---- the readers -------------------------------------------------------------------------------------------------------------------
# The shipped threshold (ops.INFLATE_SPEC_MIN_OUT, 64 MiB) is a measured break-even of two routes that give the same bytes, not a
# limit of the decoder.  A dozen files of that size would cost these tests half a minute of host zlib, so the tests below set it to
# TEST_MIN_OUT and write files just above and under that; test_the_shipped_threshold_decides_the_route reads one file at the real value.
TEST_MIN_OUT = 8 << 20


@pytest.fixture
def min_out(monkeypatch):
    from multitalent_amd import ops
    assert ops.INFLATE_SPEC_MIN_OUT >= TEST_MIN_OUT > 2 << 20
    monkeypatch.setattr(ops, 'INFLATE_SPEC_MIN_OUT', TEST_MIN_OUT)
    return TEST_MIN_OUT


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _ct_volume(shape, seed, noise_tail=0):
    """CT-like int16 values; `noise_tail` incompressible bytes at the end, which every DEFLATE writer stores"""
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    v = (np.repeat(rs.randint(-300, 900, n // 3 + 1), 3)[:n] + rs.randint(0, 3, n)).astype(np.int16)
    if noise_tail:
        v[-noise_tail // 2:] = np.frombuffer(rs.bytes(noise_tail), dtype=np.int16)
    return v.reshape(shape)


def _npz_with_body(fname, key, stream, body):
    from multitalent_amd.utilities.npz_io import HostBodies, write_npz_members
    return write_npz_members(fname, [(key, len(stream), HostBodies([body], zlib.crc32(stream)))])


@pytest.mark.gpu
def test_load_npz_device_reads_other_writers_members(dev, tmp_path, guarded, min_out):
    from multitalent_amd import ops
    from multitalent_amd.utilities.npz_io import load_npz_device, locate_member, npy_header
    shape = (min_out // 2 // (64 * 64) + 1, 64, 64)           # int16: just above the threshold
    vol = _ct_volume(shape, 1, noise_tail=200000)
    assert min_out <= vol.nbytes <= min_out + 64 * 64 * 2
    f = str(tmp_path / 'numpy.npz')
    np.savez_compressed(f, data=vol, small=vol[:200])
    st = {}
    t = load_npz_device(f, 'data', dev, stages=st)
    assert st['path'] == 'device' and st['route'] == 'speculative' and t.is_cuda and tuple(t.shape) == shape
    with np.load(f) as z:
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(z['data']))
    assert load_npz_device(f, 'data', dev, fallback=False).shape == t.shape
    st = {}                                                                     # under the threshold: the host, as before
    assert np.array_equal(load_npz_device(f, 'small', dev, stages=st).cpu().numpy(), vol[:200]) and st['path'] == 'host'
    assert 1 << 20 < vol[:200].nbytes < min_out
    # one flipped byte of the noise at the end, which zlib has stored: the structure is whole, the CRC-32 of the zip header tells
    stream = npy_header(vol.dtype, vol.shape) + vol.tobytes()
    m = locate_member(f, 'data')
    blob = bytearray(open(f, 'rb').read())
    end = m['offset'] + m['csize']
    assert bytes(blob[end - 1000:end]) == stream[-1000:]
    blob[end - 500] ^= 0x20
    bad = str(tmp_path / 'flipped.npz')
    open(bad, 'wb').write(bytes(blob))
    with pytest.raises(IOError, match="CRC-32"):
        load_npz_device(bad, 'data', dev)
    # a sync-flushed body (the dictionary survives every flush) and a Z_FIXED one (no block starts to find)
    s = _npz_with_body(str(tmp_path / 'sync.npz'), 'data', stream, I.zlib_sync_flushed(stream, 6, 128 << 10))
    st = {}
    t = load_npz_device(s, 'data', dev, stages=st)
    assert (st['path'], st['route']) == ('device', 'speculative') and np.array_equal(_bits(t.cpu().numpy()), _bits(vol))
    x = _npz_with_body(str(tmp_path / 'fixed.npz'), 'data', stream, S.deflate(stream, 6, 8, zlib.Z_FIXED))
    st = {}
    t = load_npz_device(x, 'data', dev, stages=st)
    assert st['path'] == 'host' and 'route' not in st and np.array_equal(_bits(t.cpu().numpy()), _bits(vol))
    with pytest.raises(ValueError, match="not read on the device"):
        load_npz_device(x, 'data', dev, fallback=False)


@pytest.mark.gpu
def test_the_shipped_threshold_decides_the_route(dev, tmp_path):
    """one numpy-written member just above ops.INFLATE_SPEC_MIN_OUT and one just under it (long runs, so that zlib is quick)"""
    from multitalent_amd import ops
    from multitalent_amd.utilities.npz_io import load_npz_device, npy_header
    rs = np.random.RandomState(3)
    n = ops.INFLATE_SPEC_MIN_OUT // 2
    over = np.repeat(rs.randint(-300, 900, n // 16 + 1).astype(np.int16), 16)[:n]
    under = over[:n - 256]
    assert len(npy_header(over.dtype, over.shape)) + over.nbytes >= ops.INFLATE_SPEC_MIN_OUT > len(npy_header(under.dtype, under.shape)) + under.nbytes
    f = str(tmp_path / 'numpy.npz')
    np.savez_compressed(f, over=over, under=under)
    for key, arr, want in (('over', over, ('device', 'speculative')), ('under', under, ('host', None))):
        st = {}
        t = load_npz_device(f, key, dev, stages=st)
        assert (st['path'], st.get('route')) == want and np.array_equal(t.cpu().numpy(), arr), key


def _nifti_blob(arr, geo):
    from multitalent_amd.utilities import nifti_io as N
    return N._nifti_header(arr.shape, arr.dtype, *geo) + arr.tobytes()


GEO = ((0.8, 0.9, 2.5), (1.0, -2.0, 3.0), (1, 0, 0, 0, 1, 0, 0, 0, 1))


@pytest.mark.gpu
def test_read_image_device_reads_other_writers_files(dev, tmp_path, guarded, min_out):
    import torch
    from multitalent_amd import ops
    from multitalent_amd.utilities import deflate_host
    from multitalent_amd.utilities import nifti_io as N
    shape = (min_out // 2 // (64 * 64) + 1, 64, 64)
    vol = _ct_volume(shape, 2, noise_tail=200000)
    plain = _nifti_blob(vol, GEO)
    f = str(tmp_path / 'gzip6.nii.gz')
    open(f, 'wb').write(gzip.compress(plain, 6))
    ref = N._read_nifti(f)
    st = {}
    vox, spacing, origin, direction = N.read_image_device(f, dev, st)
    assert (st['path'], st['route']) == ('device', 'speculative') and vox.dtype == torch.int16
    assert np.array_equal(vox.cpu().numpy(), ref.array) and np.array_equal(ref.array, vol)
    assert spacing == ref.spacing and origin == ref.origin and direction == ref.direction
    h = str(tmp_path / 'sync.nii.gz')                                           # as pigz writes: a sync flush every 128 KiB
    open(h, 'wb').write(deflate_host.gzip_member(I.zlib_sync_flushed(plain, 6, 128 << 10), zlib.crc32(plain), len(plain)))
    st = {}
    vox, _, _, _ = N.read_image_device(h, dev, st)
    assert (st['path'], st['route']) == ('device', 'speculative') and np.array_equal(vox.cpu().numpy(), vol)
    blob = bytearray(open(f, 'rb').read())
    assert bytes(blob[-1008:-8]) == plain[-1000:]                               # stored noise in front of the trailer
    blob[-500] ^= 0x20
    open(f, 'wb').write(bytes(blob))
    with pytest.raises(IOError, match="CRC-32"):
        N.read_image_device(f, dev)
    x = str(tmp_path / 'fixed.nii.gz')
    open(x, 'wb').write(deflate_host.gzip_member(S.deflate(plain, 6, 8, zlib.Z_FIXED), zlib.crc32(plain), len(plain)))
    small = str(tmp_path / 'small.nii.gz')
    open(small, 'wb').write(gzip.compress(_nifti_blob(vol[:400], GEO), 6))
    for fname, want in ((x, vol), (small, vol[:400])):
        st = {}
        vox, _, _, _ = N.read_image_device(fname, dev, st)
        assert st['path'] == 'host' and 'route' not in st and np.array_equal(vox.cpu().numpy(), want)


# ---- the call sites: nothing reaches np.load or gzip.open ------------------------------------------------------------------------------

@pytest.fixture
def no_host_inflate(monkeypatch):
    """armed by calling it: from then on np.load and gzip.open raise"""
    def arm():
        def boom(*a, **k):
            raise AssertionError("a file of another writer was inflated on the host")
        monkeypatch.setattr(np, 'load', boom)
        monkeypatch.setattr(gzip, 'open', boom)
    return arm


@pytest.mark.gpu
def test_case_cache_admits_a_numpy_written_case(dev, tmp_path, no_host_inflate, min_out):
    import torch
    from multitalent_amd import ops
    from multitalent_amd.training.dataloading.device_loading import DeviceCaseCache
    rs = np.random.RandomState(6)
    shape = (3, 12, 256, 256)
    case = (np.repeat(rs.randn(3 * 12 * 256 * 64).astype(np.float32), 4) * 40).reshape(shape)
    case[-1] = np.round(case[-1] / 40).clip(-1, 2)
    assert case.nbytes >= min_out
    f = str(tmp_path / 'case.npz')
    np.savez_compressed(f, data=case)
    entry = {'data_file': f, 'properties': {'k': 1}}
    host = DeviceCaseCache(dev, 1 << 30).admit(entry, all_data=case)
    no_host_inflate()
    cache = DeviceCaseCache(dev, 1 << 30)
    res = cache.admit(entry)
    assert res is not None and res.shape == shape[1:] and torch.equal(res.data, host.data) and torch.equal(res.seg, host.seg)
    assert np.array_equal(_bits(res.data.cpu().numpy()), _bits(case[:-1]))


@pytest.mark.gpu
def test_merge_files_reads_numpy_written_members(dev, tmp_path, no_host_inflate, min_out):
    """members above the threshold, written by np.savez_compressed as the reference writes them, merge to the same files as the
    same members written by the device writer"""
    import pickle
    import torch
    from multitalent_amd import ops
    from multitalent_amd.inference.ensemble_predictions import merge_files
    from multitalent_amd.utilities.npz_io import save_npz_device
    from test_ensemble_gpu import case_properties
    rs = np.random.RandomState(9)
    shape = (24, 240, 256)
    meta = {'spacing_zyx': [2.5, 0.9, 0.8], 'origin': [1.0, -2.0, 3.0]}
    c = {'shape': list(shape), 'full': list(shape), 'lo': [0, 0, 0], 'regions_class_order': None}
    members = []
    for m in range(2):
        logits = np.repeat(rs.randint(0, 16, (3, 24, 240, 64)), 4, axis=3).astype(np.float32)
        e = np.exp(logits / 4)
        members.append((e / e.sum(0)).astype(np.float16))
    assert members[0].nbytes >= min_out
    sets = {}
    for kind in ('device', 'numpy'):
        files, pkls = [], []
        for m, soft in enumerate(members):
            d = tmp_path / ('%s_m%d' % (kind, m))
            d.mkdir()
            if kind == 'device':
                save_npz_device(str(d / 'case.npz'), softmax=torch.from_numpy(soft).to(dev))
            else:
                np.savez_compressed(str(d / 'case.npz'), softmax=soft)
            with open(d / 'case.pkl', 'wb') as fh:
                pickle.dump(case_properties('case', c, meta), fh)
            files.append(str(d / 'case.npz'))
            pkls.append(str(d / 'case.pkl'))
        sets[kind] = (files, pkls)
    no_host_inflate()
    outs = {}
    for kind, (files, pkls) in sets.items():
        out = str(tmp_path / (kind + '.nii.gz'))
        merge_files(files, pkls, out, True, True)
        outs[kind] = (open(out, 'rb').read(), open(out[:-7] + '.npz', 'rb').read())
    assert outs['numpy'] == outs['device']


@pytest.mark.gpu
def test_evaluate_case_reads_gzip_label_files_on_the_device(dev, tmp_path, no_host_inflate, min_out):
    from multitalent_amd import ops
    from multitalent_amd.evaluation.evaluator import evaluate_case
    rs = np.random.RandomState(12)
    shape = (min_out // (256 * 256) + 1, 256, 256)
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    maps = []
    for shift in (0, 3):
        a = np.zeros(shape, np.uint8)
        a[(z - 40) ** 2 + (y - 100 - shift) ** 2 + (x - 90) ** 2 < 30 ** 2] = 1
        a[(z - 90) ** 2 + (y - 60) ** 2 + (x - 170 + shift) ** 2 < 25 ** 2] = 2
        a[rs.rand(*shape) > 0.9995] = 3
        maps.append(a)
    files = []
    for k, a in enumerate(maps):
        files.append(str(tmp_path / ('labels%d.nii.gz' % k)))
        open(files[-1], 'wb').write(gzip.compress(_nifti_blob(a, GEO), 6))
    want = evaluate_case(maps[0], maps[1], [1, 2, 3, (1, 2)])
    no_host_inflate()
    got = evaluate_case(files[0], files[1], [1, 2, 3, (1, 2)])
    assert got['test'] == files[0] and got['reference'] == files[1]
    for label in ('1', '2', '3', '(1, 2)'):
        assert got[label] == want[label], label
