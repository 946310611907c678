"""A numpy / Python restatement of the device gzip encoder (csrc/deflate.hip + ops.deflate_gzip), written from the format
description in DESIGN.md §6v and RFC 1951/1952, not from the kernels: tokeniser, histograms, block header, bit packing, chunk
framing and CRC combine.  Only the code-LENGTH construction is imported from the product (utilities/deflate_host.code_lengths):
it is host code there too, and a second Huffman builder would pin nothing but its own tie-breaking.

`gzip_member(x, chunk)` is what `ops.deflate_gzip(payload, prefix, chunk)` must return byte for byte for x = prefix + payload."""
import struct
import zlib

import numpy as np

from multitalent_amd.utilities.deflate_host import code_lengths

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def length_code(length):
    """RFC 1951's length table, by search: -> (symbol, extra bits, extra value)."""
    k = max(i for i in range(29) if LEN_BASE[i] <= length)
    return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def tokenize(x):
    """One chunk -> list of tokens: an int 0..255 is a literal, ('m', L) a match of length L at distance 1.
    Every maximal run of equal bytes is: its first byte as a literal, then matches of 258 while 258 bytes remain, then the rest
    as one match when it is 3 or longer, as literals when it is 1 or 2."""
    x = np.frombuffer(bytes(x), dtype=np.uint8)
    n = len(x)
    if n == 0:
        return []
    starts = np.concatenate(([0], np.flatnonzero(x[1:] != x[:-1]) + 1))
    ends = np.concatenate((starts[1:], [n]))
    out = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        b = int(x[s])
        out.append(b)
        rest = e - s - 1
        out.extend([('m', 258)] * (rest // 258))
        rest %= 258
        if rest >= 3:
            out.append(('m', rest))
        else:
            out.extend([b] * rest)
    return out


def histograms(chunks_tokens):
    """-> (286 literal/length counts, 30 distance counts) of the whole file: every chunk ends with one end-of-block symbol."""
    ll, d = [0] * 286, [0] * 30
    for toks in chunks_tokens:
        for t in toks:
            if isinstance(t, tuple):
                ll[length_code(t[1])[0]] += 1
                d[0] += 1
            else:
                ll[t] += 1
        ll[256] += 1
    return ll, d


def canonical(lens):
    """RFC 1951 §3.2.2: shorter codes first, within a length in symbol order; -> {symbol: code as a bit STRING, first bit first}."""
    code, out = 0, {}
    for bits in range(1, max(lens) + 1):
        for s, b in enumerate(lens):
            if b == bits:
                out[s] = format(code, '0%db' % bits)
                code += 1
        code <<= 1
    return out


def _lsb(value, bits):
    return format(value, '0%db' % bits)[::-1] if bits else ''


def block_header(ll_lens, d_lens):
    """the dynamic-block header after BFINAL as a bit string: BTYPE, HLIT, HDIST, HCLEN, code-length code, coded lengths."""
    hlit = max(257, max(i for i, b in enumerate(ll_lens) if b) + 1)
    hdist = max([1] + [i + 1 for i, b in enumerate(d_lens) if b])
    seq = list(ll_lens[:hlit]) + list(d_lens[:hdist])
    items, i = [], 0                                    # (symbol, extra bits, extra value)
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        run, v = j - i, seq[i]
        if v == 0:
            while run >= 11:
                r = min(run, 138); items.append((18, 7, r - 11)); run -= r
            if run >= 3:
                items.append((17, 3, run - 3)); run = 0
        else:
            items.append((v, 0, 0)); run -= 1
            while run >= 3:
                r = min(run, 6); items.append((16, 2, r - 3)); run -= r
        items += [(v, 0, 0)] * run
        i = j
    freq = [0] * 19
    for s, _, _ in items:
        freq[s] += 1
    cl_lens = code_lengths(freq, 7)
    cl = canonical(cl_lens)
    hclen = max(4, max(k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]))
    bits = _lsb(2, 2) + _lsb(hlit - 257, 5) + _lsb(hdist - 1, 5) + _lsb(hclen - 4, 4)
    bits += ''.join(_lsb(cl_lens[CL_ORDER[k]], 3) for k in range(hclen))
    bits += ''.join(cl[s] + _lsb(ev, eb) for s, eb, ev in items)
    return bits


def token_bits(toks, ll, d):
    parts = []
    for t in toks:
        if isinstance(t, tuple):
            s, eb, ev = length_code(t[1])
            parts.append(ll[s] + _lsb(ev, eb) + d[0])
        else:
            parts.append(ll[t])
    parts.append(ll[256])
    return ''.join(parts)


def pack(bits):
    """bit string, first bit first -> bytes (DEFLATE fills each byte from its least significant bit), zero padded."""
    a = np.frombuffer(bits.encode(), dtype=np.uint8) - ord('0')
    return np.packbits(a, bitorder='little').tobytes()


def stored_size(n):
    return n + 5 * max(1, -(-n // 65535))


def stored_blocks(x, final):
    out, blocks = b'', [x[i:i + 65535] for i in range(0, len(x), 65535)] or [b'']
    for k, b in enumerate(blocks):
        out += bytes([1 if (final and k == len(blocks) - 1) else 0]) + struct.pack('<HH', len(b), len(b) ^ 0xffff) + b
    return out


def split(x, chunk):
    return [x[i:i + chunk] for i in range(0, len(x), chunk)] or [b'']


def deflate_chunks(x, chunk):
    """-> list of the chunks' encoded bytes.  A chunk is one dynamic block (the file's one code table) followed, except in the
    last chunk, by an empty stored block that byte-aligns it; or stored blocks when those are smaller."""
    x = bytes(x)
    chunks = split(x, chunk)
    toks = [tokenize(c) for c in chunks]
    ll_hist, d_hist = histograms(toks)
    ll_lens, d_lens = code_lengths(ll_hist, 15), code_lengths(d_hist, 15, at_least_two=False)
    ll, d = canonical(ll_lens), canonical(d_lens)
    header = block_header(ll_lens, d_lens)
    out = []
    for k, (c, t) in enumerate(zip(chunks, toks)):
        final = k == len(chunks) - 1
        bits = ('1' if final else '0') + header + token_bits(t, ll, d)
        if not final:
            bits += '000'
            bits += '0' * (-len(bits) % 8) + _lsb(0, 16) + _lsb(0xffff, 16)
        enc = pack(bits)
        out.append(stored_blocks(c, final) if stored_size(len(c)) < len(enc) else enc)
    return out


# ---- CRC-32 of a concatenation: crc(a + b) = crc(a) * x^(8 len(b)) mod P  xor  crc(b), in the reflected bit order ----
POLY = 0xedb88320


def _mulmod(a, b):
    """product of two reflected 32-bit polynomials modulo the CRC polynomial (bit 31 = x^0)."""
    p = 0
    for k in range(32):
        if (a >> (31 - k)) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def _xpow(nbits):
    r, sq = 1 << 31, 1 << 30                                # x^0, x^1
    while nbits:
        if nbits & 1:
            r = _mulmod(r, sq)
        sq = _mulmod(sq, sq)
        nbits >>= 1
    return r


def crc_combine(crc1, crc2, len2):
    return _mulmod(crc1, _xpow(8 * len2)) ^ crc2


def gzip_member(x, chunk):
    x = bytes(x)
    parts = split(x, chunk)
    crc = zlib.crc32(parts[0])
    for p in parts[1:]:
        crc = crc_combine(crc, zlib.crc32(p), len(p))
    return (b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff' + b''.join(deflate_chunks(x, chunk))
            + struct.pack('<II', crc, len(x) & 0xffffffff))


def workspace_bound(n, chunk):
    """the most bytes the DEFLATE stream of n input bytes can take: every chunk stored."""
    full, last = divmod(n, chunk)
    return full * stored_size(chunk) + (stored_size(last) if last or not full else 0)


# ---- the inputs the CPU and GPU tests share ----
def label_map(shape, labels=4, seed=0):
    """nested / neighbouring ellipsoids with labels 1..labels on a zero background, uint8 [z, y, x]."""
    rs = np.random.RandomState(seed)
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing='ij')
    out = np.zeros(shape, dtype=np.uint8)
    for lab in range(1, labels + 1):
        c = [rs.uniform(0.25, 0.75) * s for s in shape]
        r = [max(1.0, rs.uniform(0.15, 0.35) * s) for s in shape]
        out[((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0] = lab
    return out


def ball(shape):
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) - (s - 1) / 2.0 for s in shape], indexing='ij')
    r = 0.4 * min(shape)
    return (z * z + y * y + x * x <= r * r).astype(np.uint8)


RUNS = (2, 3, 258, 259, 260, 261, 516, 517, 518)


def cases(chunk):
    rs = np.random.RandomState(chunk)
    out = {'len%d' % n: bytes(rs.randint(0, 2, n).astype(np.uint8)) for n in (0, 1, 2, 3)}
    for name, n in (('chunk-1', chunk - 1), ('chunk', chunk), ('chunk+1', chunk + 1), ('3chunk+7', 3 * chunk + 7)):
        out[name] = np.repeat(rs.randint(0, 4, n // 5 + 1).astype(np.uint8), 5)[:n].tobytes()
    for r in RUNS:
        out['run%d' % r] = b'\x07' + b'\x03' * r + b'\x09\x09'
    out['straddle'] = b'\x01' * (chunk - 100 if chunk > 100 else chunk - 10) + b'\x02' * 300 + b'\x01' * 5
    out['all_bytes'] = bytes(range(256))
    out['zeros'] = bytes(2 * chunk + 300)
    out['random'] = rs.bytes(3 * chunk + 7)
    out['label_map'] = bytes(rs.randint(0, 256, 352).astype(np.uint8)) + label_map((5, 7, 300)).tobytes()
    return out


SIZE_INPUTS = {'zeros': lambda: np.zeros((64, 96, 300), np.uint8), 'ball': lambda: ball((64, 96, 300)),
               'labels': lambda: label_map((64, 96, 300))}
