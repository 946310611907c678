"""A Python restatement of the device decoder for DEFLATE streams WITHOUT restart points (csrc/inflate_spec.hip through
ops.inflate_stream), written from RFC 1951, zlib's acceptance rules for a dynamic header, include/mtseg.h and DESIGN.md §6ab, not from
the kernels: the search for block starts, units that start at bit positions and hold markers, the chain from bit 0, the windows and the
resolve.

A UNIT starts at a candidate (a bit position), decodes consecutive blocks and ends at the first block end that is a candidate's
position, or at a block with BFINAL.  A match source r bytes in front of the unit (1 <= r <= 32768) is the marker 0x8000 | (32768 - r).
`scan` is what mt_inflate_spec_scan leaves in its head, `inflate` what ops.inflate_stream returns where it does not raise."""
import zlib
from array import array

import numpy as np

import inflate_host as I

OK, TOO_LONG, BAD, CORRUPT, SIZE = I.OK, I.TOO_LONG, I.BAD, I.CORRUPT, I.SIZE
WIN = 32768
UNIT_LIMIT = 1 << 30
SPAN_CHUNKS = 64


# ---- search ----
def _bits_at(comp, p):
    b = I._Bits(comp, 0)
    b.pos = p
    return b


def accept(comp, p):
    """is bit position p the header of a non-final dynamic block that zlib's inflate would accept?"""
    bits = _bits_at(comp, p)
    if bits.get(1) != 0 or bits.get(2) != 2:
        return False
    hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
    if hlit > 286 or hdist > 30:
        return False
    cl = [0] * 19
    for k in range(hclen):
        cl[I.ORDER[k]] = bits.get(3)
    if sum(1 << (7 - l) for l in cl if l) != 1 << 7:                      # the code-length code is complete
        return False
    code = I._Code(cl)
    lens, prev = [], 0
    while len(lens) < hlit + hdist:
        s = code.decode(bits, 7)
        if s < 0:
            return False
        if s < 16:
            lens.append(s)
            prev = s
            continue
        if s == 16:
            if not lens:
                return False
            val, rep = prev, 3 + bits.get(2)
        elif s == 17:
            val, rep = 0, 3 + bits.get(3)
        else:
            val, rep = 0, 11 + bits.get(7)
        if len(lens) + rep > hlit + hdist:
            return False
        lens += [val] * rep
        prev = val
    if bits.overrun or lens[256] == 0:                                    # no header bit behind the input; an end-of-block code
        return False
    for part in (lens[:hlit], lens[hlit:]):
        kraft = sum(1 << (15 - l) for l in part if l)
        if kraft > 1 << 15:                                               # over-subscribed
            return False
        if kraft < 1 << 15 and max(part) > 1:                             # incomplete: only a code of one-bit lengths passes
            return False
    return True


def accepted(comp):
    """every bit position p > 0 of the stream at which `accept` holds, ascending (the three header bits are tested with numpy first)"""
    comp = bytes(comp)
    bits = np.unpackbits(np.frombuffer(comp, dtype=np.uint8), bitorder='little')
    head = (bits[:-2] == 0) & (bits[1:-1] == 0) & (bits[2:] == 1)        # BFINAL 0, BTYPE 2 (lowest bit first)
    return [int(p) for p in np.flatnonzero(head) if p > 0 and accept(comp, int(p))]


def candidates(comp, chunk, hits=None):
    """bit 0, and per chunk of `chunk` compressed bytes the first accepted bit position p > 0 in it, ascending"""
    hits = accepted(comp) if hits is None else hits
    out, seen = [0], set()
    for p in hits:
        k = (p >> 3) // chunk
        if k not in seen:
            seen.add(k)
            out.append(p)
    return out


# ---- blocks (decoded once per start position, whatever unit they end up in) ----
def decode_block(comp, bit):
    """-> dict: kind (0 stored, 1 fixed, 2 dynamic), final, status (OK or BAD), end (bit position behind the block), and for a stored
    block src / len, for a coded one tokens (a literal 0..255, or -(length << 16 | distance)) with the bit position behind each, and
    last_overran: the last token's bits lie behind the input"""
    n = len(comp)
    bits = _bits_at(comp, bit)
    final, kind = bool(bits.get(1)), bits.get(2)
    b = {'kind': kind, 'final': final, 'status': BAD, 'end': bit, 'tokens': [], 'at': [], 'last_overran': False, 'src': 0, 'len': 0}
    if kind == 3 or bits.overrun:
        return b
    if kind == 0:
        bits.align()
        length, nlen = bits.get(16), bits.get(16)
        data = bits.pos >> 3
        if length ^ nlen != 0xffff or bits.overrun or data + length > n:
            return b
        b.update(status=OK, src=data, len=length, end=8 * (data + length))
        return b
    if kind == 1:
        ll_lens, d_lens = I.FIXED_LL, I.FIXED_D
    else:
        got = I._dynamic_codes(bits)
        if got is None:
            return b
        ll_lens, d_lens = got
    ll, d = I._Code(ll_lens), I._Code(d_lens)
    if not ll.ok or not d.ok:
        return b
    tokens, at = b['tokens'], b['at']
    while True:
        sym = ll.decode(bits)
        if sym < 0 or sym > 285:
            return b
        if sym == 256:
            if not bits.overrun:
                b.update(status=OK, end=bits.pos)
            return b
        if sym < 256:
            tokens.append(sym)
        else:
            length = I._length(sym, bits)
            dsym = d.decode(bits)
            if dsym < 0 or dsym > 29:
                return b
            tokens.append(-((length << 16) | I._distance(dsym, bits)))
        at.append(bits.pos)
        if bits.overrun:
            b['last_overran'] = True
            return b


def decode_unit(comp, start, is_candidate, unit_limit, span_limit, blocks):
    """-> dict: status (OK, BAD, TOO_LONG, CORRUPT), end (bit position), final, sym (array('H')), spans [(source byte, offset in the
    unit, length)], reach (the farthest a match reaches in front of the unit), matches [(offset in the unit, distance)]"""
    n = len(comp)
    span_bits = 8 * n + 64 if span_limit > n else 8 * span_limit
    sym, spans, matches = array('H'), [], []
    res = {'status': BAD, 'end': start, 'final': False, 'sym': sym, 'spans': spans, 'reach': 0, 'matches': matches}
    bit = start
    while True:
        b = blocks.get(bit)
        if b is None:
            b = blocks[bit] = decode_block(comp, bit)
        res['final'] = b['final']
        if b['kind'] == 0 or b['kind'] == 3:
            if b['status'] != OK:
                return res
            if b['len']:
                spans.append((b['src'], len(sym), b['len']))
                sym.extend(comp[b['src']:b['src'] + b['len']])
        else:
            last = len(b['tokens']) - 1
            for k, (t, tb) in enumerate(zip(b['tokens'], b['at'])):
                if t >= 0:
                    sym.append(t)
                else:
                    length, dist, pos = (-t) >> 16, (-t) & 0xffff, len(sym)
                    if dist > pos:
                        if start == 0:                                    # nothing lies in front of bit 0
                            res['status'] = CORRUPT
                            return res
                        res['reach'] = max(res['reach'], dist - pos)
                    matches.append((pos, dist))
                    first = min(length, dist)
                    if dist <= pos:
                        piece = sym[pos - dist:pos - dist + first]
                    else:
                        piece = array('H', (0x8000 | (WIN + q) for q in range(pos - dist, min(0, pos - dist + first))))
                        piece.extend(sym[0:pos - dist + first] if pos - dist + first > 0 else array('H'))
                    while len(piece) < length:
                        piece.extend(piece[:length - len(piece)])
                    sym.extend(piece)
                if k == last and b['last_overran']:
                    return res
                if len(sym) > unit_limit or tb - start > span_bits:
                    res['status'] = TOO_LONG
                    return res
            if b['status'] != OK:
                return res
        end = b['end']
        if len(sym) > unit_limit or end - start > span_bits:
            res['status'] = TOO_LONG
            return res
        if b['final']:
            res.update(status=OK, end=(end + 7) & ~7)
            return res
        if is_candidate(end):
            res.update(status=OK, end=end)
            return res
        bit = end


def scan(comp, chunk, unit_limit=UNIT_LIMIT, span_limit=None, n_expect=None, hits=None, blocks=None):
    """-> dict: status, candidates (bit positions), results (candidate -> decode_unit's dict, for every candidate), units (the start
    positions of the chain), total, max_reach, shortest_unit.  The chain follows end -> start from bit 0; it takes the status of a failed
    candidate on its way and is CORRUPT when the last unit is not final or does not end at the last byte."""
    comp = bytes(comp)
    span_limit = SPAN_CHUNKS * chunk if span_limit is None else span_limit
    cands = candidates(comp, chunk, hits)
    cset = set(cands[1:])
    blocks = {} if blocks is None else blocks
    results = {c: decode_unit(comp, c, cset.__contains__, unit_limit, span_limit, blocks) for c in cands}
    info = {'candidates': cands, 'results': results, 'units': [], 'total': 0, 'max_reach': 0, 'shortest_unit': 0}
    pos, status = 0, None
    while status is None:
        r = results.get(pos)
        if r is None:
            status = CORRUPT
        elif r['status'] != OK:
            status = r['status']
        else:
            info['units'].append(pos)
            info['total'] += len(r['sym'])
            pos = r['end']
            if r['final']:
                status = OK if pos == 8 * len(comp) else CORRUPT
    sizes = [len(results[u]['sym']) for u in info['units']]
    if sizes:
        info['shortest_unit'] = min(sizes)
        info['max_reach'] = max(results[u]['reach'] for u in info['units'])
    if status == OK and n_expect is not None and info['total'] != n_expect:
        status = SIZE
    info['status'] = status
    return info


def resolve(info):
    """windows and bytes of a chain with status OK -> (bytes or None when a marker points in front of the stream, the largest number
    of windows a byte was carried through before a marker read it)"""
    prev = np.zeros(WIN, np.uint8)
    origin = np.full(WIN, -1, np.int64)                                   # the unit each window byte was decoded in; -1: invalid
    out, hops = [], 0
    for k, u in enumerate(info['units']):
        sym = np.frombuffer(info['results'][u]['sym'], dtype=np.uint16) if len(info['results'][u]['sym']) else np.zeros(0, np.uint16)
        mark = sym >= 0x8000
        m = (sym & 0x7fff).astype(np.int64)
        if mark.any():
            if (origin[m[mark]] < 0).any():
                return None, hops
            hops = max(hops, int((k - origin[m[mark]]).max()))
        data = np.where(mark, prev[m], sym.astype(np.uint8)).astype(np.uint8)
        org = np.where(mark, origin[m], k)
        out.append(data.tobytes())
        prev, origin = np.concatenate((prev, data))[-WIN:], np.concatenate((origin, org))[-WIN:]
    return b''.join(out), hops


def inflate(comp, chunk, unit_limit=UNIT_LIMIT, span_limit=None, n_expect=None, hits=None, blocks=None):
    """-> (bytes or None, crc, info) as ops.inflate_stream returns them where it does not raise; info['hops'] as `resolve` counts"""
    info = scan(comp, chunk, unit_limit, span_limit, n_expect, hits, blocks)
    if info['status'] != OK:
        return None, None, info
    out, info['hops'] = resolve(info)
    if out is None:
        info['status'] = CORRUPT
        return None, None, info
    info['spans'] = sum(len(info['results'][u]['spans']) for u in info['units'])
    return out, zlib.crc32(out), info


def block_starts(comp):
    """[(bit position, kind, final)] of every block of a valid stream, by decoding it from bit 0"""
    comp, out, bit = bytes(comp), [], 0
    while True:
        b = decode_block(comp, bit)
        assert b['status'] == OK, bit
        out.append((bit, b['kind'], b['final']))
        if b['final']:
            return out
        bit = b['end']


# ---- a writer for hand-made blocks: what zlib never emits (distance 32768, a match in front of the stream) ----
class BitWriter(object):
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, k):
        self.v |= value << self.n
        self.n += k

    def code(self, value, k):
        """a Huffman code: its bits go out highest first"""
        for i in range(k - 1, -1, -1):
            self.put((value >> i) & 1, 1)

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, 'little')


def _canonical(lens):
    codes, code = {}, 0
    for l in range(1, 16):
        for s, v in enumerate(lens):
            if v == l:
                codes[s] = (code, l)
                code += 1
        code <<= 1
    return codes


_LL_LENS = [8] * 226 + [9] * 60                                           # complete: 226 / 256 + 60 / 512 = 1
_D_LENS = [4] * 2 + [5] * 28                                              # complete: 2 / 16 + 28 / 32 = 1
_CL_LENS = [0] * 19
for _s in (4, 5, 8, 9):
    _CL_LENS[_s] = 2


def put_stored(w, data, final=False):
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put(len(data) ^ 0xffff, 16)
    for c in data:
        w.put(c, 8)


def put_dynamic(w, tokens, final=False):
    """tokens: a byte value, or (length, distance); one dynamic block with a fixed, complete pair of codes"""
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(286 - 257, 5)
    w.put(30 - 1, 5)
    w.put(12 - 4, 4)                                                      # the order reaches symbol 4 with its 12th entry
    for k in range(12):
        w.put(_CL_LENS[I.ORDER[k]], 3)
    cl = _canonical(_CL_LENS)
    for l in _LL_LENS + _D_LENS:
        w.code(*cl[l])
    ll, d = _canonical(_LL_LENS), _canonical(_D_LENS)
    for t in list(tokens) + [256]:
        if not isinstance(t, tuple):
            w.code(*ll[t])
            continue
        length, dist = t
        s = 285 if length == 258 else next(s for s in range(284, 256, -1) if I._length(s, _Zero()) <= length)
        w.code(*ll[s])
        w.put(length - I._length(s, _Zero()), 0 if s < 265 or s == 285 else (s - 261) >> 2)
        ds = next(s for s in range(29, -1, -1) if I._distance(s, _Zero()) <= dist)
        w.code(*d[ds])
        w.put(dist - I._distance(ds, _Zero()), 0 if ds < 4 else (ds >> 1) - 1)


class _Zero(object):
    """extra bits that read as zero: the base value of a length or distance symbol"""

    def get(self, k):
        return 0


# ---- the streams the CPU and GPU tests share ----
def ct_bytes(n_values, seed=0):
    """CT-like int16 data: values repeated three times with a little noise on them"""
    rs = np.random.RandomState(seed)
    return (np.repeat(rs.randint(-300, 900, n_values), 3) + rs.randint(0, 3, 3 * n_values)).astype(np.int16).tobytes()


def deflate(x, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(x) + c.flush()


def false_candidates_stream():
    ct = ct_bytes(15000, 1)
    inner = deflate(ct, 6, 1)
    x = ct[:30000] + inner + ct[30000:60000]
    return deflate(x, 6), x


def exact_window_stream():
    """hand-made dynamic blocks: 32768 + 10 literals, then matches at distance exactly 32768 whose sources lie in front of the second
    block (zlib itself never looks back farther than 32768 - 262), then one literal in a final block"""
    rs = np.random.RandomState(8)
    head = rs.randint(0, 200, WIN + 10).astype(np.uint8).tobytes()
    w = BitWriter()
    put_dynamic(w, list(head))
    put_dynamic(w, [(258, WIN), (100, WIN), 7, (3, WIN)])
    put_dynamic(w, [9], final=True)
    x = bytearray(head)
    for length in (258, 100):
        for _ in range(length):
            x.append(x[-WIN])
    x.append(7)
    for _ in range(3):
        x.append(x[-WIN])
    return w.bytes(), bytes(x) + b'\x09'


def last_byte_stream():
    """a stored block of 58 bytes puts the header of a dynamic block at byte 63: in the last byte of the first 64-byte chunk"""
    w = BitWriter()
    data = bytes(range(58))
    put_stored(w, data)
    assert w.n == 8 * 63
    put_dynamic(w, list(b'abcabc') + [(20, 3), (30, 40)], final=False)
    put_dynamic(w, [1, 2, 3], final=True)
    x = bytearray(data + b'abcabc')
    for length, dist in ((20, 3), (30, 40)):
        for _ in range(length):
            x.append(x[-dist])
    return w.bytes(), bytes(x) + bytes([1, 2, 3])


def streams():
    """name -> (raw DEFLATE stream, the bytes it holds)"""
    out = {}
    ct = ct_bytes(16000, 0)                                               # 96 000 bytes
    for level in (1, 6, 9):
        out['ct_l%d_m8' % level] = (deflate(ct, level, 8), ct)
        out['ct_l%d_m1' % level] = (deflate(ct[:60000], level, 1), ct[:60000])
    rs = np.random.RandomState(2)
    motif = bytes(rs.randint(0, 64, 32500).astype(np.uint8))              # (zlib looks back 32768 - 262 bytes at the most)
    out['motif'] = (deflate(motif * 4, 6, 3), motif * 4)                   # blocks of 511 symbols
    out['exact_window'] = exact_window_stream()
    runs = bytes(3000000) + bytes(np.repeat(rs.randint(0, 256, 40).astype(np.uint8), 900))
    x = ct[:20000] + runs + ct[20000:40000]
    out['long_matches'] = (deflate(x, 6, 1), x)                           # blocks of 127 symbols: 32 766 zeros from some 30 bytes
    noise = rs.bytes(70000)
    out['noise'] = (deflate(noise), noise)
    mixed = ct[:20000] + noise[:40000] + ct[20000:60000] + noise[1000:1400] + ct[60000:96000]
    out['noise_between'] = (deflate(mixed), mixed)
    for name, strategy in (('fixed', zlib.Z_FIXED), ('huffman_only', zlib.Z_HUFFMAN_ONLY), ('rle', zlib.Z_RLE)):
        out[name] = (deflate(ct[:60000], 6, 8, strategy), ct[:60000])
    m = I.mixed_bytes()
    out['sync_flushed'] = (I.zlib_sync_flushed(m, 6, 3000), m)
    out['full_flushed'] = (I.zlib_flushed(m, 6, 1000), m)
    out['false_candidates'] = false_candidates_stream()
    out['last_byte'] = last_byte_stream()
    out['short'] = (deflate(b'a stream that is shorter than one chunk ' * 2), b'a stream that is shorter than one chunk ' * 2)
    out['one_final_block'] = (deflate(ct[:3000]), ct[:3000])
    return out


def malformed():
    """name -> (stream, chunk, kwargs of scan / inflate_stream, bytes or None): damaged streams; the CPU test pins each one's status.
    bytes: what a stream with status OK decodes to (its CRC-32 then differs from the original's)"""
    out, big = {}, {'span_limit': 1 << 30}
    ct = ct_bytes(16000, 0)
    good = deflate(ct, 6)
    starts = block_starts(good)
    assert len(starts) >= 3 and starts[1][1] == 2
    flipped = bytearray(good)
    flipped[(starts[1][0] + 4) >> 3] ^= 1 << ((starts[1][0] + 4) & 7)     # a bit of HLIT in the second block's header
    out['flipped_header'] = (bytes(flipped), 256, big, None)
    noise = np.random.RandomState(2).bytes(70000)
    stored = bytearray(deflate(noise))
    stored[1000] ^= 0x20
    bad_noise = bytearray(noise)
    bad_noise[1000 - 5] ^= 0x20                                           # the first stored block's data starts at byte 5
    out['flipped_payload'] = (bytes(stored), 256, big, bytes(bad_noise))
    out['truncated'] = (good[:len(good) // 2], 256, big, None)
    # a fixed block that starts with a match: length 3 (symbol 257: 0000001), distance 1 (00000)
    bits = '1' + '10' + '0000001' + '00000' + '0000000'
    out['before_stream_unit0'] = (int(bits[::-1], 2).to_bytes((len(bits) + 7) // 8, 'little'), 64, {}, None)
    w = BitWriter()
    put_dynamic(w, list(range(100)))
    put_dynamic(w, [(10, 200), 5])
    put_dynamic(w, [6], final=True)
    out['before_stream_unit1'] = (w.bytes(), 64, big, None)
    out['wrong_size'] = (good, 256, dict(big, n_expect=len(ct) + 1), None)
    fixed = deflate(ct[:60000], 6, 8, zlib.Z_FIXED)
    out['fixed_over_span_limit'] = (fixed, 64, {}, None)
    return out
