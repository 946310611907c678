"""A Python restatement of the device INFLATE decoder (csrc/inflate.hip through ops.inflate_raw), written from RFC 1951,
include/mtseg.h and DESIGN.md §6y, not from the kernels: candidates, the decoding of one unit with its statuses and stored spans,
the chain from position 0, and the file framing the readers parse (zip member, gzip member).

A UNIT starts at a byte position, decodes consecutive blocks and ends behind an empty stored block (the next unit starts at the
following byte) or at a block with BFINAL.  `scan` is what mt_inflate_scan leaves in its head, `inflate` what ops.inflate_raw
returns."""
import struct
import zlib

OK, FOREIGN, TOO_LONG, BAD, CORRUPT, SIZE = 'OK', 'FOREIGN', 'TOO_LONG', 'BAD', 'CORRUPT', 'SIZE'
MARKER = b'\x00\x00\xff\xff'
MIN_UNIT = 5                        # an empty stored block on a byte boundary
UNIT_LIMIT = 16 * 65536
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


def candidates(comp):
    """position 0 and every position inside the stream that follows an occurrence of 00 00 ff ff, ascending"""
    comp, out, i = bytes(comp), [0], 0
    while True:
        i = comp.find(MARKER, i)
        if i < 0:
            return out
        if i + 4 < len(comp):
            out.append(i + 4)
        i += 1


def candidate_capacity(n):
    return n // MIN_UNIT + 2


class _Bits(object):
    """the stream from byte `start`, lowest bit first; bytes behind the end read as zero, `overrun` tells when they were used"""

    def __init__(self, comp, start):
        self.comp, self.n, self.pos = comp, len(comp), 8 * start

    def peek(self, k):
        b = self.pos >> 3
        return (int.from_bytes(self.comp[b:b + 4], 'little') >> (self.pos & 7)) & ((1 << k) - 1)

    def get(self, k):
        v = self.peek(k)
        self.pos += k
        return v

    def align(self):
        self.pos = (self.pos + 7) & ~7

    @property
    def overrun(self):
        return self.pos > 8 * self.n


class _Code(object):
    """a canonical Huffman code from its lengths; None when they are over-subscribed.  An incomplete set is accepted: a bit
    pattern that is no code fails when it is met."""

    def __init__(self, lens):
        self.count = [0] * 16
        for l in lens:
            self.count[l] += 1
        left, self.ok = 1, True
        for l in range(1, 16):
            left = 2 * left - self.count[l]
            if left < 0:
                self.ok = False
                return
        self.symbols = [s for l in range(1, 16) for s, v in enumerate(lens) if v == l]

    def decode(self, bits, maxlen=15):
        """-> symbol, or -1 when the next `maxlen` bits start no code; consumes the code's bits"""
        v = bits.peek(maxlen)
        code = first = index = 0
        for l in range(1, maxlen + 1):
            code |= v & 1
            v >>= 1
            c = self.count[l]
            if code - c < first:
                bits.pos += l
                return self.symbols[index + code - first]
            index, first, code = index + c, (first + c) << 1, code << 1
        return -1


def _length(sym, bits):
    if sym < 265:
        return sym - 254
    if sym == 285:
        return 258
    eb = (sym - 261) >> 2
    return 3 + ((4 + ((sym - 265) & 3)) << eb) + bits.get(eb)


def _distance(sym, bits):
    if sym < 4:
        return sym + 1
    eb = (sym >> 1) - 1
    return 1 + ((2 + (sym & 1)) << eb) + bits.get(eb)


def _dynamic_codes(bits):
    hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
    if hlit > 286 or hdist > 30:
        return None
    cl = [0] * 19
    for k in range(hclen):
        cl[ORDER[k]] = bits.get(3)
    code = _Code(cl)
    if bits.overrun or not code.ok:
        return None
    lens, prev = [], 0
    while len(lens) < hlit + hdist:
        s = code.decode(bits, 7)
        if s < 0:
            return None
        if s < 16:
            lens.append(s)
            prev = s
        else:
            if s == 16:
                if not lens:
                    return None
                val, rep = prev, 3 + bits.get(2)
            elif s == 17:
                val, rep = 0, 3 + bits.get(3)
            else:
                val, rep = 0, 11 + bits.get(7)
            if len(lens) + rep > hlit + hdist:
                return None
            lens += [val] * rep
            prev = val
        if bits.overrun:
            return None
    if lens[256] == 0:
        return None
    return lens[:hlit], lens[hlit:]


def decode_unit(comp, start, unit_limit=UNIT_LIMIT):
    """-> dict: status (OK, BAD, TOO_LONG), end (byte position behind the unit), final, data (the unit's bytes, stored blocks
    included), spans [(source position, offset in the unit's output, length)] of its non-empty stored blocks, max_distance."""
    comp = bytes(comp)
    bits, out, spans, huff = _Bits(comp, start), bytearray(), [], 0
    res = {'status': BAD, 'end': start, 'final': False, 'spans': spans, 'max_distance': 0}

    def done(status, end=None):
        res.update(status=status, data=bytes(out), end=start if end is None else end)
        return res

    while True:
        final = res['final'] = bool(bits.get(1))
        kind = bits.get(2)
        if kind == 3 or bits.overrun:
            return done(BAD)
        if kind == 0:
            bits.align()
            length, nlen = bits.get(16), bits.get(16)
            data = bits.pos >> 3
            if length ^ nlen != 0xffff or bits.overrun or data + length > len(comp):
                return done(BAD)
            if length == 0:
                return done(OK, data)
            spans.append((data, len(out), length))
            out += comp[data:data + length]
            bits.pos = 8 * (data + length)
            if final:
                return done(OK, data + length)
            continue
        if kind == 1:
            ll_lens, d_lens = FIXED_LL, FIXED_D
        else:
            got = _dynamic_codes(bits)
            if got is None:
                return done(BAD)
            ll_lens, d_lens = got
        ll, d = _Code(ll_lens), _Code(d_lens)
        if not ll.ok or not d.ok:
            return done(BAD)
        while True:
            sym = ll.decode(bits)
            if sym < 0 or sym > 285:
                return done(BAD)
            if sym < 256:
                out.append(sym)
                huff += 1
            elif sym == 256:
                if bits.overrun:
                    return done(BAD)
                break
            else:
                length = _length(sym, bits)
                dsym = d.decode(bits)
                if dsym < 0 or dsym > 29:
                    return done(BAD)
                dist = _distance(dsym, bits)
                if dist > len(out):
                    return done(BAD)                    # it would reach in front of the unit
                res['max_distance'] = max(res['max_distance'], dist)
                for _ in range(length):
                    out.append(out[-dist])
                huff += length
            if bits.overrun:
                return done(BAD)
            if huff > unit_limit:
                return done(TOO_LONG)
        if final:
            bits.align()
            return done(OK, bits.pos >> 3)


def scan(comp, unit_limit=UNIT_LIMIT, final=True, n_expect=None):
    """-> dict: status, candidates, results (candidate position -> decode_unit's dict, for every candidate), units (the start
    positions of the chain), total.  The chain follows end -> start from 0; it takes the status of a failed candidate on its
    way, and is CORRUPT when an end is no candidate or the stream does not end at its last byte (with BFINAL when final)."""
    comp = bytes(comp)
    cands = candidates(comp)
    info = {'candidates': cands, 'results': {}, 'units': [], 'total': 0}
    if len(cands) > candidate_capacity(len(comp)):
        info['status'] = FOREIGN
        return info
    results = info['results'] = {c: decode_unit(comp, c, unit_limit) for c in cands}
    pos, status = 0, None
    while status is None:
        r = results.get(pos)
        if r is None:
            status = CORRUPT
        elif r['status'] != OK:
            status = r['status']
        else:
            info['units'].append(pos)
            info['total'] += len(r['data'])
            pos = r['end']
            if r['final']:
                status = OK if pos == len(comp) else CORRUPT
            elif pos == len(comp):
                status = CORRUPT if final else OK
    if status == OK and n_expect is not None and info['total'] != n_expect:
        status = SIZE
    info['status'] = status
    return info


def inflate(comp, unit_limit=UNIT_LIMIT, final=True, n_expect=None):
    """-> (bytes or None, crc, info) as ops.inflate_raw returns them where it does not raise"""
    info = scan(comp, unit_limit, final, n_expect)
    if info['status'] != OK:
        return None, None, info
    out = b''.join(info['results'][u]['data'] for u in info['units'])
    info['spans'] = sum(len(info['results'][u]['spans']) for u in info['units'])
    return out, zlib.crc32(out), info


# ---- file framing ----
def gzip_payload(blob):
    """one gzip member -> (offset of the raw DEFLATE stream, its length, CRC-32, ISIZE); FEXTRA, FNAME, FCOMMENT and FHCRC are
    honoured (RFC 1952)"""
    blob = bytes(blob)
    if len(blob) < 18 or blob[:2] != b'\x1f\x8b' or blob[2] != 8:
        raise IOError("not a gzip member with a DEFLATE stream")
    flags, p = blob[3], 10
    if flags & 4:
        p += 2 + struct.unpack('<H', blob[p:p + 2])[0]
    for bit in (8, 16):
        if flags & bit:
            p = blob.index(b'\0', p) + 1
    if flags & 2:
        p += 2
    crc, isize = struct.unpack('<II', blob[-8:])
    return p, len(blob) - 8 - p, crc, isize


def zip_member(blob, name):
    """-> (method, data offset, compressed size, size, CRC-32) of member `name`, from the central directory and the local header"""
    import io
    import zipfile
    info = zipfile.ZipFile(io.BytesIO(bytes(blob))).getinfo(name)
    o = info.header_offset
    sig, nlen, elen = blob[o:o + 4], *struct.unpack('<HH', blob[o + 26:o + 30])
    assert sig == b'PK\x03\x04'
    return info.compress_type, o + 30 + nlen + elen, info.compress_size, info.file_size, info.CRC


# ---- the streams the CPU and GPU tests share ----
def zlib_flushed(x, level, every):
    """a raw zlib stream of x with a Z_FULL_FLUSH behind every `every` bytes"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    out = b''
    for i in range(0, len(x), every):
        out += c.compress(x[i:i + every]) + c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


def zlib_sync_flushed(x, level=6, every=3000):
    """a valid raw zlib stream that the unit rules refuse: Z_SYNC_FLUSH (and pigz by default) puts the empty stored block behind
    every piece but keeps the dictionary, so the matches of the second 'unit' reach in front of it"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return b''.join(c.compress(x[i:i + every]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(x), every)) + c.flush()


def mixed_bytes(n=24000, seed=3):
    """text, zeros and random bytes: zlib answers with fixed, dynamic and stored blocks and distances up to 32 KiB"""
    import numpy as np
    rs = np.random.RandomState(seed)
    words = [b'unit', b'chain', b'stored', b'block', b'marker', b'candidate', b'the', b'of', b'wave', b' ', b'\n']
    text = b' '.join(words[i] for i in rs.randint(0, len(words), n // 8))
    far = rs.bytes(300)
    x = text[:n // 3] + bytes(n // 6) + far + rs.bytes(n // 4) + text[:2000] + bytes(20000) + far + text[n // 5:n // 3]
    return x


def planted(seed=7):
    """-> (x, chunk, marks): 300 zeros, 6000 random bytes that hold a restart marker at each of `marks` — followed by a plausible
    stored header (00 10 00 ef ff) or by an empty final stored block (01 00 00 ff ff) — and 700 float16 ones.  Written with
    deflate_period_host.raw at a chunk of 1000, the random part becomes stored chunks with the markers inside.
    At period 2 the stream has 8 candidates: position 0; the two true restart points, behind the Huffman-coded first and in
    front of the Huffman-coded last chunk; the marks at 1300, 2500 and 4000, which lie in stored chunks (those at 100 and 5990 lie
    in the first and the last chunk, which are Huffman-coded because of the zeros and ones beside them, so their bytes do not
    appear in the stream); and one more behind each of the two planted empty final blocks (marks 1300 and 4000), whose own
    00 00 ff ff is a marker too.  The two that follow a planted final block
    decode it and are never reached; the two behind those and the one on the planted stored header run into random bytes and fail."""
    import numpy as np
    rs = np.random.RandomState(seed)
    r = bytearray(rs.bytes(6000))
    marks = (100, 1300, 2500, 4000, 5990)
    tails = (b'\x00\x10\x00\xef\xff', b'\x01\x00\x00\xff\xff', b'\x00\x10\x00\xef\xff', b'\x01\x00\x00\xff\xff', b'\x00\x10\x00\xef\xff')
    for m, t in zip(marks, tails):
        r[m:m + 4 + len(t)] = MARKER + t
    return bytes(300) + bytes(r) + np.ones(700, np.float16).tobytes(), 1000, marks


def streams():
    """name -> (raw DEFLATE stream, the bytes it holds, final): every kind of stream the decoder serves"""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import deflate_period_host as P
    out = {}
    for period in P.PERIODS:
        for chunk in (64, 1000, 1024):
            for name, x in P.cases(chunk, period).items():
                out['p%d_c%d_%s' % (period, chunk, name)] = (P.raw(x, chunk, period)[0], bytes(x), True)
    x = P.cases(1000, 2)['elements'] + P.cases(1000, 2)['random'] + P.cases(1000, 2)['zeros']
    out['open_bodies'] = (b''.join(P.raw(x[i:i + 2500], 1000, 2, False)[0] for i in range(0, len(x), 2500)), x, False)
    for p in P.PERIODS:
        out['segments_p%d' % p] = (b''.join(P.segments(x, 1000, p, 3000)[0]), x, True)
    m = mixed_bytes()
    for level in (1, 6, 9):
        for every in (64, 1000, 4096):
            out['zlib_l%d_f%d' % (level, every)] = (zlib_flushed(m, level, every), m, True)
        out['zlib_l%d_f40000' % level] = (zlib_flushed(m, level, 40000), m, True)     # units with matches further than the LDS ring
    px, chunk, _ = planted()
    out['planted'] = (P.raw(px, chunk, 2)[0], px, True)
    return out


def malformed():
    """name -> (stream, kwargs of scan / inflate_raw): damaged streams; the CPU test pins each one's status"""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import deflate_period_host as P
    import numpy as np
    rs = np.random.RandomState(11)
    x = np.repeat(rs.randint(0, 5, 400).astype(np.uint8), rs.randint(1, 9, 400)).tobytes() + rs.bytes(1500) + bytes(900)
    good = P.raw(x, 1000, 1)[0]
    first = decode_unit(good, 0)
    out = {}
    for name, cut in (('cut_header', 9), ('cut_token', first['end'] - 12), ('cut_marker', first['end'] - 2)):
        out[name] = (good[:cut], {})
    stored = P.raw(rs.bytes(3000), 1000, 1)[0]                          # three stored chunks
    out['cut_stored'] = (stored[:1500], {})
    flipped = bytearray(stored)
    flipped[3] ^= 0x10
    out['flipped_nlen'] = (bytes(flipped), {})
    # a dynamic header whose code-length code is over-subscribed: BFINAL 1, type 2, HLIT 0, HDIST 0, HCLEN 15 (19 lengths), all 1
    bits = '1' + '01' + '00000' + '00000' + '1111' + '100' * 19
    out['oversubscribed'] = (int(bits[::-1], 2).to_bytes((len(bits) + 7) // 8, 'little') + bytes(8), {})
    # a fixed block that starts with a match: length 3 (symbol 257: 0000001), distance 1 (00000)
    bits = '1' + '10' + '0000001' + '00000' + '0000000'
    out['distance_before_unit'] = (int(bits[::-1], 2).to_bytes((len(bits) + 7) // 8, 'little'), {})
    out['wrong_size'] = (good, {'n_expect': len(x) + 1})
    out['no_last_block'] = (P.raw(x, 1000, 1, False)[0], {})
    return out
