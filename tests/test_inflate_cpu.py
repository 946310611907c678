"""The restatement of the device INFLATE decoder (inflate_host.py) against zlib, and the host halves of the readers built on the
decoder (the zip member locator, the gzip header parser, the .npy header): no GPU."""
import gzip
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_period_host as P  # noqa: E402
import inflate_host as I  # noqa: E402


def _zlib(body):
    d = zlib.decompressobj(-15)
    return d.decompress(bytes(body)) + d.flush()


@pytest.fixture(scope='module')
def streams():
    return I.streams()


def test_restatement_equals_zlib_on_every_stream(streams):
    """periods {1, 2, 4, 8} x chunks {64, 1000, 1024}, concatenated open bodies, segments, zlib streams cut by Z_FULL_FLUSH"""
    assert len(streams) == 4 * 3 * len(P.cases(64, 1)) + 1 + 4 + 12 + 1
    bad = []
    for name, (body, x, final) in streams.items():
        out, crc, info = I.inflate(body, final=final)
        want = _zlib(body) if final else x
        if info['status'] != I.OK or out != want or out != x or crc != zlib.crc32(x) or info['total'] != len(x):
            bad.append((name, info['status'], len(body)))
    assert not bad, bad


def test_streams_hold_every_block_type_and_far_distances(streams):
    """what the zlib streams are there for: fixed and stored blocks inside units, several units, a match that needs a far read"""
    kinds = set()
    for name, (body, x, final) in streams.items():
        if name.startswith('zlib'):
            info = I.scan(body)
            assert len(info['units']) >= 3
            for u in info['units']:
                kinds.add((body[u] >> 1) & 3)                           # the type of each unit's first block
    assert kinds == {0, 1, 2}
    far = [max(r['max_distance'] for r in I.scan(streams['zlib_l%d_f%s' % (l, f)][0])['results'].values()) for l in (1, 6, 9) for f in (4096, 40000)]
    print(far)
    assert min(far[0::2]) > 258 and max(far[0::2]) <= 4096 and min(far[1::2]) > 16384      # beside and beyond the decoder's 4 KiB ring


def test_open_stream_needs_final_false(streams):
    body, x, _ = streams['open_bodies']
    assert I.scan(body, final=True)['status'] == I.CORRUPT and I.scan(body, final=False)['status'] == I.OK


def test_planted_markers_are_ignored(streams):
    """restart markers inside stored chunks, followed by a plausible stored header or an empty final block: the candidates they
    make fail, or decode and are never reached; the chain holds the three true units"""
    body, x, _ = streams['planted']
    info = I.scan(body)
    out, _, _ = I.inflate(body)
    assert out == x == _zlib(body)
    res, units = info['results'], set(info['units'])
    failed = [c for c in info['candidates'] if res[c]['status'] != I.OK]
    unreferenced = [c for c in info['candidates'] if res[c]['status'] == I.OK and c not in units]
    print(len(info['candidates']), len(failed), len(unreferenced), len(units))
    assert (len(info['candidates']), len(failed), len(unreferenced), len(units)) == (8, 3, 2, 3)
    assert all(body[c - 4:c] == I.MARKER for c in info['candidates'][1:])


def test_plain_zlib_stream_is_too_long():
    x = np.repeat(np.random.RandomState(0).randint(0, 256, 40000).astype(np.uint8), 10).tobytes()
    assert len(x) == 400000
    body = zlib.compress(x)[2:-4]
    assert _zlib(body) == x
    info = I.scan(body, unit_limit=65536)
    assert info['status'] == I.TOO_LONG and info['units'] == []
    assert I.scan(body, unit_limit=400000)['status'] == I.OK             # one unit, when it is allowed to be that long


def test_malformed_statuses():
    """the statuses the GPU test compares the device against"""
    want = {'cut_header': I.BAD, 'cut_token': I.BAD, 'cut_marker': I.BAD, 'cut_stored': I.BAD, 'flipped_nlen': I.BAD,
            'oversubscribed': I.BAD, 'distance_before_unit': I.BAD, 'wrong_size': I.SIZE, 'no_last_block': I.CORRUPT}
    got = {name: I.scan(body, **kw)['status'] for name, (body, kw) in I.malformed().items()}
    assert got == want
    for name, (body, kw) in I.malformed().items():                       # and zlib refuses them too (but the size, which it is not told)
        if name in ('wrong_size',):
            continue
        d = zlib.decompressobj(-15)
        try:
            d.decompress(body)
            assert not d.eof, name
        except zlib.error:
            pass


def test_sync_flushed_stream_is_valid_but_refused_by_the_unit_rules():
    """why the readers hand BAD / CORRUPT to the host reader and do not call the file damaged"""
    x = b'restart points and dictionary ' * 400
    body = I.zlib_sync_flushed(x)
    assert _zlib(body) == x and body.count(I.MARKER) >= 3
    info = I.scan(body)
    assert info['status'] == I.BAD and info['results'][0]['status'] == I.OK       # the first unit decodes, the second reaches before it


def test_too_many_candidates_is_foreign():
    body = I.MARKER * 50
    assert len(I.candidates(body)) == 50 and I.candidate_capacity(len(body)) == 42
    assert I.scan(body)['status'] == I.FOREIGN


# ---- the host halves of the readers ----
def test_gzip_header_parser():
    from multitalent_amd.utilities.nifti_io import gzip_payload
    x = b'restart points ' * 40
    body = zlib.compress(x)[2:-4]
    trailer = struct.pack('<II', zlib.crc32(x), len(x))
    plain = gzip.compress(x)
    p, n, crc, isize = gzip_payload(plain)
    assert (p, crc, isize) == (10, zlib.crc32(x), len(x)) and _zlib(plain[p:p + n]) == x
    buf = io.BytesIO()
    with gzip.GzipFile('volume.nii', 'wb', fileobj=buf, mtime=0) as f:  # FNAME
        f.write(x)
    named = buf.getvalue()
    p, n, crc, isize = gzip_payload(named)
    assert named[3] & 8 and p == 10 + len('volume.nii') + 1 and _zlib(named[p:p + n]) == x
    extra = b'\x1f\x8b\x08' + bytes([4 | 8 | 16 | 2]) + bytes(6) + struct.pack('<H', 5) + b'AB\x01\x00\x07' + b'n\0' + b'c\0' + b'\x12\x34'
    p, n, crc, isize = gzip_payload(extra + body + trailer)
    assert p == len(extra) and n == len(body) and (crc, isize) == (zlib.crc32(x), len(x))
    assert gzip.decompress(extra[:-2] + struct.pack('<H', zlib.crc32(extra[:-2]) & 0xffff) + body + trailer) == x
    assert I.gzip_payload(extra + body + trailer) == (p, n, crc, isize)
    for bad in (b'', plain[:12], b'PK' + plain[2:], extra[:14] + trailer):
        with pytest.raises(IOError):
            gzip_payload(bad)
    # the device writer's format: the header deflate_host writes, the restated body
    from multitalent_amd.utilities import deflate_host as H
    raw, c, k = P.raw(x, 64, 1)
    member = H.gzip_member(raw, c, k)
    p, n, crc, isize = gzip_payload(member)
    assert member[p:p + n] == raw and (crc, isize) == (zlib.crc32(x), len(x)) and gzip.decompress(member) == x


def test_zip_member_locator_and_npy_header(tmp_path):
    from multitalent_amd.utilities import npz_io
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    b = np.asfortranarray(np.arange(6, dtype=np.int16).reshape(2, 3))
    f = str(tmp_path / 'host.npz')
    np.savez_compressed(f, data=a, other=b)
    blob = open(f, 'rb').read()
    for key, arr in (('data', a), ('other', b)):
        m = npz_io.locate_member(f, key)
        assert m['method'] == 8 and m['flags'] & 8 == 0
        assert I.zip_member(blob, key + '.npy') == (m['method'], m['offset'], m['csize'], m['usize'], m['crc'])
        stream = _zlib(blob[m['offset']:m['offset'] + m['csize']])
        assert len(stream) == m['usize'] and zlib.crc32(stream) == m['crc']
        shape, fortran, dtype, hbytes = npz_io.parse_npy_header(stream[:4096])
        assert shape == arr.shape and dtype == arr.dtype and fortran == (key == 'other') and hbytes % 16 == 0
        assert stream[hbytes:] == arr.tobytes('A')
        assert npz_io.parse_npy_header(stream[:11]) is None and npz_io.npy_header_bytes(stream[:12]) == hbytes
        out, crc, info = I.inflate(blob[m['offset']:m['offset'] + m['csize']])
        assert out == stream and crc == m['crc']
    with pytest.raises(KeyError):
        npz_io.locate_member(f, 'missing')
    assert npz_io.peek_npy_header(f, 'data') == (a.shape, False, a.dtype) and npz_io.peek_npy_header(f, 'other') == (b.shape, True, b.dtype)
    assert npz_io.peek_npy_header(f, 'missing') is None
    g = str(tmp_path / 'stored.npz')
    np.savez(g, data=a)
    assert npz_io.locate_member(g, 'data')['method'] == 0 and npz_io.peek_npy_header(g, 'data') == (a.shape, False, a.dtype)
    # the device writer's format, restated: the member is found where write_npz_members put it, Zip64 or not
    x = P.npy_prefix(a) + a.tobytes()
    for force in (False, True):
        h = npz_io.write_npz_members(str(tmp_path / ('dev%d.npz' % force)), [('data', len(x), npz_io.HostBodies([P.raw(x, 64, 4)[0]], zlib.crc32(x)))],
                                     _force_zip64=force)
        m = npz_io.locate_member(h, 'data')
        body = open(h, 'rb').read()[m['offset']:m['offset'] + m['csize']]
        out, crc, info = I.inflate(body, n_expect=m['usize'])
        assert out == x and crc == m['crc'] == zlib.crc32(x) and 2 <= len(info['units']) <= len(P.split(x, 64))
        assert np.array_equal(np.load(h)['data'], a)
    with pytest.raises(IOError):
        npz_io.parse_npy_header(b'\x93NUMPY\x01\x00' + struct.pack('<H', 6) + b'{bad}\n' + bytes(20))


def test_nifti_parser_is_the_reader_s(tmp_path):
    """`_parse_nifti`, factored out of `_read_nifti`, sees what it saw"""
    from multitalent_amd.utilities import nifti_io as N
    arr = np.random.RandomState(2).randint(0, 7, (5, 6, 7)).astype(np.int16)
    geo = ((0.8, 0.9, 2.5), (1.0, -2.0, 3.0), (np.cos(0.3), -np.sin(0.3), 0, np.sin(0.3), np.cos(0.3), 0, 0, 0, 1))
    f = str(tmp_path / 'a.nii.gz')
    N._write_nifti(N.Image(arr, *geo), f)
    im = N._read_nifti(f)
    dt, shape, off, slope, inter, spacing, origin, direction = N._parse_nifti(gzip.open(f).read()[:352], f)
    assert (dt, shape, off) == (np.dtype('<i2'), arr.shape, 352) and not N._is_scaled(slope, inter)
    assert np.array_equal(im.array, arr) and im.array.dtype == np.int16
    assert im.spacing == tuple(spacing) and im.origin == tuple(origin) and im.direction == tuple(direction)
    assert np.allclose(im.spacing, geo[0], rtol=1e-6) and np.allclose(im.origin, geo[1]) and np.allclose(im.direction, geo[2], atol=1e-6)
