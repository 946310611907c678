"""The gzip encoder of the label-map writer, without a device: the restatement in deflate_host.py (which the device output must
equal byte for byte, test_deflate_gpu.py) produces streams every inflater accepts, small enough to be worth having, and the host
pieces the product shares with it (code lengths, header, token table, CRC combine, the NIfTI header) are what they claim."""
import gzip
import hashlib
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_host as H  # noqa: E402

from multitalent_amd.utilities import deflate_host as P  # noqa: E402

CHUNKS = (64, 1000, 1024)
PRODUCT_CHUNK = 65536
cases = H.cases


@pytest.mark.parametrize("chunk", CHUNKS)
def test_round_trip_and_trailer(chunk):
    for name, x in cases(chunk).items():
        g = H.gzip_member(x, chunk)
        assert gzip.decompress(g) == x, name
        assert zlib.decompress(g[10:-8], -15) == x, name                    # the raw DEFLATE stream on its own
        assert g[:10] == b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff', name    # mtime 0: same input, same file
        assert struct.unpack('<II', g[-8:]) == (zlib.crc32(x), len(x) & 0xffffffff), name
        assert len(g) - 18 <= H.workspace_bound(len(x), chunk), name
    rnd = cases(chunk)['random']
    assert len(H.gzip_member(rnd, chunk)) - 18 == H.workspace_bound(len(rnd), chunk)      # random bytes: every chunk stored


@pytest.mark.parametrize("chunk", CHUNKS)
def test_chunks_are_independent_and_byte_aligned(chunk):
    """the stream is the concatenation of the chunk outputs; every chunk but the last ends with the empty stored block"""
    x = cases(chunk)['3chunk+7']
    parts = H.deflate_chunks(x, chunk)
    assert len(parts) == 4 and b''.join(parts) == H.gzip_member(x, chunk)[10:-8]
    for p in parts[:-1]:
        assert p[-4:] == b'\x00\x00\xff\xff'
    x = cases(chunk)['straddle']                                           # no match reaches back across the boundary:
    toks = [H.tokenize(c) for c in H.split(x, chunk)]                       # the second chunk starts with a literal of its own
    assert toks[1][0] == 2 and sum(t[1] if isinstance(t, tuple) else 1 for t in toks[0]) == chunk


def test_tokeniser_on_runs():
    m = lambda n: ('m', n)                                                  # noqa: E731
    want = {2: [3, 3], 3: [3, 3, 3], 4: [3, m(3)], 258: [3, m(257)], 259: [3, m(258)], 260: [3, m(258), 3], 261: [3, m(258), 3, 3],
            262: [3, m(258), m(3)], 516: [3, m(258), m(257)], 517: [3, m(258), m(258)], 518: [3, m(258), m(258), 3]}
    for r, toks in want.items():
        assert H.tokenize(b'\x07' + b'\x03' * r + b'\x09') == [7] + toks + [9], r


def test_crc_combine_against_zlib():
    rs = np.random.RandomState(3)
    for chunk, last in ((64, 1), (64, 63), (1000, 7), (1024, 1024), (65536, 12345)):
        parts = [rs.bytes(chunk) for _ in range(3)] + [rs.bytes(last)]
        whole = zlib.crc32(b''.join(parts))
        assert P.crc32_join([zlib.crc32(p) for p in parts], chunk, last) == whole
        crc = zlib.crc32(parts[0])
        for p in parts[1:]:
            crc = H.crc_combine(crc, zlib.crc32(p), len(p))
        assert crc == whole
    assert P.crc32_join([zlib.crc32(b'')], 64, 0) == 0 and P.crc32_combine(123, 0, 0) == 123
    a, b = rs.bytes(77), rs.bytes(5)
    assert P.crc32_combine(zlib.crc32(a), zlib.crc32(b), 5) == H.crc_combine(zlib.crc32(a), zlib.crc32(b), 5) == zlib.crc32(a + b)


def kraft(lens):
    return sum(2.0 ** -b for b in lens if b)


def test_code_lengths_are_limited_and_complete():
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])                                       # plain Huffman would be 39 deep
    rs = np.random.RandomState(0)
    for freqs, limit in ((fib, 15), (fib[:19], 7), ([0] * 10 + fib + [0] * 5, 15), (list(rs.randint(0, 50, 286)), 15),
                         ([1] * 286, 15), ([5, 0, 0, 9], 15), (list(rs.randint(0, 3, 19)), 7)):
        lens = P.code_lengths(freqs, limit)
        assert len(lens) == len(freqs) and max(lens) <= limit
        assert all((b > 0) == (f > 0) for b, f in zip(lens, freqs))
        assert kraft(lens) == 1.0                                            # complete: inflaters refuse an incomplete code
    assert P.code_lengths([0, 0, 7, 0], 15) == [1, 0, 1, 0]                 # a lone symbol gets a partner
    assert P.code_lengths([0, 0, 0], 15) == [1, 1, 0]
    assert P.code_lengths([9] + [0] * 29, 15, at_least_two=False) == [1] + [0] * 29        # the distance alphabet may be degenerate
    assert P.code_lengths([0] * 30, 15, at_least_two=False) == [0] * 30
    # a more frequent symbol never has a longer code
    lens = P.code_lengths(fib, 15)
    assert all(lens[i] >= lens[i + 1] for i in range(2, len(fib) - 1))


def test_degenerate_distance_alphabet_is_accepted():
    """matches only ever use distance code 0: one code of one bit (Kraft sum 1/2), and none at all without a match"""
    for x in (bytes(1000), b'abc' * 5, b''):
        toks = [H.tokenize(c) for c in H.split(x, 1024)]
        ll, d = H.histograms(toks)
        d_lens = P.code_lengths(d, 15, at_least_two=False)
        assert kraft(d_lens) in (0.5, 0.0) and (kraft(d_lens) == 0.5) == any(isinstance(t, tuple) for t in toks[0])
        bits = '1' + H.block_header(P.code_lengths(ll, 15), d_lens) + H.token_bits(toks[0], H.canonical(P.code_lengths(ll, 15)), H.canonical(d_lens))
        assert zlib.decompress(H.pack(bits), -15) == x                       # forced dynamic block, no stored fallback


@pytest.mark.parametrize("name", ['zeros', 'label_map', 'all_bytes', 'random'])
def test_product_tables_equal_the_restatement(name):
    """what ops.deflate_gzip hands the emit kernel (utilities/deflate_host: header bits, token table) against the bit strings here"""
    x = cases(1024)[name]
    toks = [H.tokenize(c) for c in H.split(x, 1024)]
    ll_hist, d_hist = H.histograms(toks)
    ll_lens, d_lens, hval, hbits, table = P.build_tables(ll_hist, d_hist)
    header = H.block_header(ll_lens, d_lens)
    assert len(header) == hbits <= 8192 and int(header[::-1], 2) == hval
    ll, d = H.canonical(ll_lens), H.canonical(d_lens)

    def entry(bits):
        return int(bits[::-1], 2) | (len(bits) << 48)

    for b in range(256):
        assert int(table[b]) == (entry(ll[b]) if b in ll else 0)
    assert int(table[P.TOKEN_EOB]) == entry(ll[256])
    for length in range(3, 259):
        s, eb, ev = H.length_code(length)
        assert (s, eb, ev) == P.length_symbol(length)
        want = entry(ll[s] + H._lsb(ev, eb) + d[0]) if s in ll else 0
        assert int(table[P.TOKEN_MATCH0 + length - 3]) == want
        assert (int(table[P.TOKEN_MATCH0 + length - 3]) >> 48) <= 48


def _parent_nifti_header(arr, spacing, origin, direction):
    """the header lines of `_write_nifti` as they stood before `_nifti_header` was factored out of it, kept verbatim"""
    from multitalent_amd.utilities.nifti_io import _CODES, _LPS, _matrix_to_quaternion
    nz, ny, nx = arr.shape
    sp = np.array(spacing, dtype=np.float64)
    Rras = _LPS @ np.array(direction, dtype=np.float64).reshape(3, 3)
    t = _LPS @ np.array(origin, dtype=np.float64)
    b, c, d, qfac = _matrix_to_quaternion(Rras)
    hdr = bytearray(348)
    struct.pack_into('<i', hdr, 0, 348)
    struct.pack_into('<8h', hdr, 40, 3, nx, ny, nz, 1, 1, 1, 1)
    struct.pack_into('<hh', hdr, 70, _CODES[arr.dtype.name], arr.dtype.itemsize * 8)
    struct.pack_into('<8f', hdr, 76, qfac, sp[0], sp[1], sp[2], 0, 0, 0, 0)
    struct.pack_into('<3f', hdr, 108, 352.0, 1.0, 0.0)
    hdr[123] = 2
    struct.pack_into('<2h', hdr, 252, 1, 1)
    struct.pack_into('<6f', hdr, 256, b, c, d, t[0], t[1], t[2])
    M = Rras * sp
    for r in range(3):
        struct.pack_into('<4f', hdr, 280 + 16 * r, M[r, 0], M[r, 1], M[r, 2], t[r])
    hdr[344:348] = b'n+1\0'
    return bytes(hdr) + b'\0\0\0\0'


def test_nifti_header_bytes_unchanged(tmp_path):
    """the digests are those of the files the parent commit's `_write_nifti` wrote for these inputs"""
    from multitalent_amd.utilities.nifti_io import Image, _nifti_header, _write_nifti
    arr = np.random.RandomState(5).randint(0, 5, (5, 7, 11)).astype(np.uint8)
    d = (np.cos(0.3), -np.sin(0.3), 0, np.sin(0.3), np.cos(0.3), 0, 0, 0, 1)
    geo = ((0.8, 0.9, 2.5), (1.0, -2.0, 3.0), d)
    for a, g, digest in ((arr, geo, '03c809558ed1801ac4a1194d1005aae94aace8e7f6afbbe765868a94d688b936'),
                         (arr.astype(np.int16), ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1, 0, 0, 0, 1, 0, 0, 0, 1)),
                          '12f5abae9676cdd5d9927b5275839af89dd7cc99a11f5e4e051c14f1cd490d13')):
        f = str(tmp_path / 'a.nii')
        _write_nifti(Image(a, *g), f)
        raw = open(f, 'rb').read()
        assert raw == _parent_nifti_header(a, *g) + a.tobytes() and hashlib.sha256(raw).hexdigest() == digest
        assert _nifti_header(a.shape, a.dtype, *g) == raw[:352]
        fz = str(tmp_path / 'a.nii.gz')
        _write_nifti(Image(a, *g), fz)
        assert gzip.open(fz).read() == raw


SIZE_INPUTS = H.SIZE_INPUTS


@pytest.mark.parametrize("name", sorted(SIZE_INPUTS))
def test_size_against_gzip_level_1(name):
    """A correct but useless encoder (all literals, all stored) passes every round trip: the file must also be small.  Measured
    (DESIGN §6v): 0.30, 0.49, 0.49 of gzip level 1 for zeros, ball, labels; the cap is 2."""
    x = bytes(352) + SIZE_INPUTS[name]().tobytes()
    g = H.gzip_member(x, PRODUCT_CHUNK)
    assert gzip.decompress(g) == x
    ref = len(gzip.compress(x, 1))
    print("%s: %d bytes, gzip level 1 %d, ratio %.3f" % (name, len(g), ref, len(g) / ref))
    assert len(g) <= 2 * ref
