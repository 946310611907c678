"""The period / raw-stream / segment restatement (deflate_period_host.py) and the .npz container (utilities/npz_io), without a
device: what the device encoder is compared with byte for byte (test_npz_write_gpu.py) is itself valid DEFLATE, equals the
period-1 restatement where they overlap, and the hand-written zip structures load with numpy and zipfile."""
import os
import sys
import zipfile
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_host as H1  # noqa: E402
import deflate_period_host as H  # noqa: E402

CHUNKS = (64, 1000, 1024)


@pytest.mark.parametrize("period", H.PERIODS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_restatement_round_trips(chunk, period):
    for name, x in H.cases(chunk, period).items():
        for c in H1.split(x, chunk):
            toks = H.tokenize(c, period)
            assert H.expand(toks, period) == c, name
            assert all(3 <= t[1] <= 258 for t in toks if isinstance(t, tuple))
        body, crc, n = H.raw(x, chunk, period)
        assert H.inflate(body) == x and crc == zlib.crc32(x) and n == len(x), name


def test_token_stream_is_the_one_the_issue_describes():
    # constant float16 1.0: no two neighbouring bytes are equal, every byte from the third on equals the one 2 in front
    x = np.full(300, 1.0, np.float16).tobytes()
    assert H.tokenize(x, 1) == list(x)
    assert H.tokenize(x, 2) == [0x00, 0x3c, ('m', 258), ('m', 258), ('m', 82)]
    assert H.tokenize(x, 4) == [0x00, 0x3c, 0x00, 0x3c, ('m', 258), ('m', 258), ('m', 80)]
    # remainders of 0, 1, 2 and 3 positions behind k matches of 258
    for period in H.PERIODS:
        for k in (258, 516):
            for r in (0, 1, 2, 3):
                toks = H.tokenize(H.stretch(period, k + r), period)
                m = [t for t in toks if isinstance(t, tuple)]
                assert m == [('m', 258)] * (k // 258) + ([('m', 3)] if r == 3 else []), (period, k, r)
                assert len(toks) == len(m) + 2 * (period + 3) + period + (r if r < 3 else 0)
    # a length that is no multiple of the period, and fewer bytes than the period
    assert H.tokenize(b'\x01\x02\x03\x04' * 3 + b'\x01\x02', 4) == [1, 2, 3, 4, ('m', 10)]
    assert H.tokenize(b'\x07\x07\x07', 4) == [7, 7, 7] and H.tokenize(b'', 8) == []


@pytest.mark.parametrize("chunk", CHUNKS)
def test_period_one_final_is_the_label_map_stream(chunk):
    for name, x in H1.cases(chunk).items():
        assert H.tokenize(x[:chunk], 1) == H1.tokenize(x[:chunk]), name
        assert H.raw_chunks(x, chunk, 1, True) == H1.deflate_chunks(x, chunk), name
        want = H1.gzip_member(x, chunk)
        body, crc, n = H.raw(x, chunk, 1)
        assert want[10:-8] == body and want[-8:] == crc.to_bytes(4, 'little') + (n & 0xffffffff).to_bytes(4, 'little')


@pytest.mark.parametrize("period", H.PERIODS)
def test_segments_concatenate_and_their_crc_joins(period):
    rs = np.random.RandomState(period)
    x = np.repeat(rs.randint(0, 5, 20000 // (4 * period) + 1).astype(np.uint8), 4 * period).tobytes()[:20000]
    for segment, chunk in ((5000, 65536), (5000, 1024), (7001, 1000), (20000, 64), (30000, 1024)):
        bodies, crc, n = H.segments(x, chunk, period, segment)
        assert len(bodies) == -(-20000 // segment) and n == 20000
        assert H.inflate(b''.join(bodies)) == x and crc == zlib.crc32(x)
        done = 0
        for k, b in enumerate(bodies):                            # every piece alone is whole bytes of whole blocks; only the last ends
            d = zlib.decompressobj(-15)
            piece = d.decompress(b)
            assert piece == x[done:done + segment] and d.eof == (k == len(bodies) - 1) and not d.unused_data
            done += len(piece)
    # the distance symbol of period 8 carries its extra bit: 7 and 8 share symbol 5
    assert H.inflate(H.raw(bytes(range(8)) * 40, 1024, 8)[0]) == bytes(range(8)) * 40


def test_product_tables_carry_the_period():
    from multitalent_amd.utilities import deflate_host as P
    for period in H.PERIODS:
        x = H.stretch(period, 519) + bytes(range(256))
        toks = [H.tokenize(x, period)]
        ll_hist, d_hist = H.histograms(toks, period)
        assert sum(d_hist) == d_hist[P.distance_symbol(period)[0]] == 3
        ll_lens, d_lens, hval, hbits, table = P.build_tables(ll_hist, d_hist, period=period)
        ll, d = H1.canonical(ll_lens), H1.canonical(d_lens)
        assert format(hval, '0%db' % hbits)[::-1] == H1.block_header(ll_lens, d_lens)
        for length in (3, 10, 258):
            e = int(table[P.TOKEN_MATCH0 + length - 3])
            assert (e != 0) == (length in (3, 258))               # 519 positions: two matches of 258 and one of 3
            if e:
                want = H.token_bits([('m', length)], ll, d, period)[:-len(ll[256])]
                assert e >> 48 == len(want) <= 48 and format(e & (2 ** 48 - 1), '0%db' % len(want))[::-1] == want
    assert P.build_tables(ll_hist, d_hist)[4].tolist() == P.build_tables(ll_hist, d_hist, period=1)[4].tolist()
    with pytest.raises(ValueError):
        P.build_tables(ll_hist, d_hist, period=3)


def _host_member(arr):
    """a member whose body host zlib made: the container knows nothing about who compressed"""
    from multitalent_amd.utilities.npz_io import HostBodies, npy_header
    stream = npy_header(arr.dtype, arr.shape) + arr.tobytes()
    assert stream[:128] == H.npy_prefix(arr) and len(H.npy_prefix(arr)) % 64 == 0
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(stream) + c.flush()
    return len(stream), HostBodies([body[:100], body[100:]], zlib.crc32(stream))


@pytest.mark.parametrize("force", [False, True])
def test_container_loads_with_numpy_and_zipfile(tmp_path, force):
    from multitalent_amd.utilities.npz_io import write_npz_members
    a = H.softmax_volume((3, 5, 7, 9))
    b = np.arange(-7, 23, dtype=np.int64).reshape(5, 6)
    f = write_npz_members(str(tmp_path / 'case'), [('softmax',) + _host_member(a), ('other',) + _host_member(b)], _force_zip64=force)
    assert f == str(tmp_path / 'case.npz') and os.listdir(str(tmp_path)) == ['case.npz']
    with np.load(f) as z:
        assert sorted(z.files) == ['other', 'softmax']
        assert z['softmax'].dtype == np.float16 and np.array_equal(z['softmax'].view(np.uint16), a.view(np.uint16))
        assert z['other'].dtype == np.int64 and np.array_equal(z['other'], b)
    with zipfile.ZipFile(f) as z:
        assert z.testzip() is None and z.namelist() == ['softmax.npy', 'other.npy']
        info = z.getinfo('softmax.npy')
        assert info.compress_type == zipfile.ZIP_DEFLATED and info.file_size == 128 + a.nbytes and info.flag_bits == 0
        assert info.CRC == zlib.crc32(H.npy_prefix(a) + a.tobytes())
    raw = open(f, 'rb').read()
    assert (b'PK\x06\x06' in raw) == force and (b'PK\x06\x07' in raw) == force
    assert raw[4:6] == ((45).to_bytes(2, 'little') if force else (20).to_bytes(2, 'little'))


def test_writer_refuses_host_arrays_and_other_dtypes(tmp_path):
    import torch
    from multitalent_amd.utilities.npz_io import save_npz_device
    with pytest.raises(TypeError, match="device tensor"):
        save_npz_device(str(tmp_path / 'a.npz'), data=np.zeros(3))
    with pytest.raises(TypeError, match="device tensor"):
        save_npz_device(str(tmp_path / 'a.npz'), data=torch.zeros(3))
    assert os.listdir(str(tmp_path)) == []


# file bytes of the GPU test's inputs against numpy's own writer, measured here with the restatement; the GPU test caps
# the device writer's files at these ratios x 1.1, rounded up to one decimal
SIZE_RATIOS = {'softmax': 1.044, 'case': 1.066}
SIZE_CAPS = {'softmax': 1.2, 'case': 1.2}                             # 1.044 x 1.1 = 1.148, 1.066 x 1.1 = 1.173


def test_size_against_numpy():
    import io
    for name, make in H.SIZE_INPUTS.items():
        a = make()
        f = io.BytesIO()
        np.savez_compressed(f, data=a)
        ours = H.npz_member_size(a) + (30 + 8) + (46 + 8) + 22        # member + local and central header of 'data.npy' + end record
        ratio = ours / len(f.getvalue())
        print("%s: %d bytes against numpy's %d: %.3f" % (name, ours, len(f.getvalue()), ratio))
        assert ratio < 1.5 and ratio < SIZE_CAPS[name] and abs(ratio - SIZE_RATIOS[name]) < 0.1 * SIZE_RATIOS[name], (name, ratio)
