"""Host side of the device gzip / DEFLATE encoder (csrc/deflate.hip, ops.deflate_gzip, ops.deflate_raw): everything that is small
and serial.

The device tokenises the byte stream and counts the DEFLATE symbols (286 literal/length + 30 distance counters); from those
counts this module builds ONE length-limited Huffman code per file, the dynamic-block header that announces it and the table of
ready-made token bit patterns the emit kernel looks up; after the emit it joins the per-chunk CRC-32s (`crc32_combine`, which
Python's zlib does not expose) and frames the gzip member.  Pure Python / numpy, no device, no file I/O."""
import struct

import numpy as np

LL_SYMBOLS, D_SYMBOLS, EOB = 286, 30, 256
MAX_BITS, MAX_CL_BITS = 15, 7
MIN_MATCH, MAX_MATCH = 3, 258
# index space of the token table: a literal byte b -> b, a match of length L at the call's one distance -> 256 + (L - 3), end of block -> 512
TOKEN_MATCH0, TOKEN_EOB, TOKEN_SLOTS = 256, 512, 513
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
GZIP_HEADER = b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff'          # deflate, no flags, mtime 0, no extra flags, OS unknown
MAX_INPUT = 2 ** 31 - 1


def length_symbol(length):
    """match length 3..258 -> (literal/length symbol 257..285, number of extra bits, extra value)  (RFC 1951 §3.2.5)."""
    if length == MAX_MATCH:
        return 285, 0, 0
    v = length - MIN_MATCH
    if v < 8:
        return 257 + v, 0, 0
    e = v.bit_length() - 3
    return 261 + 4 * e + ((v >> e) & 3), e, v & ((1 << e) - 1)


def code_lengths(freqs, max_bits, at_least_two=True):
    """Huffman code lengths (0 = unused) of an alphabet with the given counts, none longer than `max_bits`.

    Plain Huffman (ties broken by symbol index, so the result is a pure function of the counts); when the tree is deeper than
    `max_bits` the lengths are re-dealt from a Kraft-exact length census, the most frequent symbols getting the shortest codes.
    The code is complete (Kraft sum exactly 1) whenever two or more symbols are coded.  `at_least_two`: an alphabet with fewer
    than two used symbols gets dummy symbols (the lowest unused indices) so that its code is complete too — inflaters refuse an
    incomplete literal/length or code-length code; with False a single used symbol gets one bit and no used symbol gives all
    zeros, which is what DEFLATE allows for the distance alphabet."""
    freqs = [int(f) for f in freqs]
    n = len(freqs)
    used = [s for s in range(n) if freqs[s] > 0]
    if at_least_two:
        s = 0
        while len(used) < 2:
            if s not in used:
                used.append(s)
            s += 1
        used.sort()
    lens = [0] * n
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    import heapq
    # (count, tie, node); leaves carry their symbol as tie so that equal counts merge in index order
    heap = [(freqs[s], s, s) for s in used]
    heapq.heapify(heap)
    parent = {}
    nxt = n
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        parent[a[2]] = nxt
        parent[b[2]] = nxt
        heapq.heappush(heap, (a[0] + b[0], nxt, nxt))
        nxt += 1
    depth = {}
    for s in used:
        d, node = 0, s
        while node in parent:
            node = parent[node]
            d += 1
        depth[s] = d
    if max(depth.values()) > max_bits:
        census = [0] * (max_bits + 1)
        for d in depth.values():
            census[min(d, max_bits)] += 1
        total = sum(census[i] << (max_bits - i) for i in range(1, max_bits + 1))
        while total != 1 << max_bits:                       # over-subscribed: lengthen one short code, pair it with a max-length one
            census[max_bits] -= 1
            for i in range(max_bits - 1, 0, -1):
                if census[i]:
                    census[i] -= 1
                    census[i + 1] += 2
                    break
            total -= 1
        order = sorted(used, key=lambda s: (-freqs[s], s))
        k = 0
        for bits in range(1, max_bits + 1):
            for _ in range(census[bits]):
                depth[order[k]] = bits
                k += 1
    for s in used:
        lens[s] = depth[s]
    return lens


def canonical_codes(lens):
    """code lengths -> the canonical codes of RFC 1951 §3.2.2 (as integers, most significant bit first)."""
    max_bits = max(lens) if len(lens) else 0
    count = [0] * (max_bits + 2)
    for b in lens:
        count[b] += 1
    count[0] = 0
    nxt, code = [0] * (max_bits + 2), 0
    for b in range(1, max_bits + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, b in enumerate(lens):
        if b:
            out[s] = nxt[b]
            nxt[b] += 1
    return out


def _reverse(code, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def _rle_code_lengths(seq):
    """the code-length sequence -> [(symbol 0..18, extra bits, extra value)] with the repeat codes 16, 17, 18."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, 7, r - 11))
                run -= r
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
            out.extend([(0, 0, 0)] * run)
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, 2, r - 3))
                run -= r
            out.extend([(v, 0, 0)] * run)
        i = j
    return out


def dynamic_header(ll_lens, d_lens):
    """-> (value, nbits): the bits of a dynamic block's header AFTER its BFINAL bit, first bit in bit 0: BTYPE = 2, HLIT, HDIST,
    HCLEN, the code-length code and the two run-length coded length tables (RFC 1951 §3.2.7)."""
    hlit = max(257, max(s for s in range(LL_SYMBOLS) if ll_lens[s]) + 1)
    hdist = max([1] + [s + 1 for s in range(D_SYMBOLS) if d_lens[s]])
    items = _rle_code_lengths(list(ll_lens[:hlit]) + list(d_lens[:hdist]))
    cl_freq = [0] * 19
    for s, _, _ in items:
        cl_freq[s] += 1
    cl_lens = code_lengths(cl_freq, MAX_CL_BITS)
    cl_codes = canonical_codes(cl_lens)
    hclen = max(4, max(k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]))
    value, nbits = 0, 0

    def put(v, b):
        nonlocal value, nbits
        value |= v << nbits
        nbits += b

    put(2, 2)
    put(hlit - 257, 5)
    put(hdist - 1, 5)
    put(hclen - 4, 4)
    for k in range(hclen):
        put(cl_lens[CL_ORDER[k]], 3)
    for s, eb, ev in items:
        put(_reverse(cl_codes[s], cl_lens[s]), cl_lens[s])
        put(ev, eb)
    return value, nbits


PERIODS = (1, 2, 4, 8)


def distance_symbol(period):
    """the one match distance of a call -> (distance symbol, number of extra bits, extra value)  (RFC 1951 §3.2.5): distances 1..4
    are the symbols 0..3, distance 8 is the upper half of symbol 5 (7..8, one extra bit)."""
    if period not in PERIODS:
        raise ValueError("the encoder matches at a distance of 1, 2, 4 or 8 bytes, not %r" % (period,))
    return (5, 1, 1) if period == 8 else (period - 1, 0, 0)


def token_table(ll_lens, d_lens, period=1):
    """-> uint64[TOKEN_SLOTS]: per token its bits (first bit in bit 0, Huffman codes already reversed, extra bits behind their code,
    the code of the distance `period` with its extra bit behind a match) in the low 48 bits and their number in the bits above.  A
    token that does not occur has no code and an entry of 0."""
    ll_codes, d_codes = canonical_codes(ll_lens), canonical_codes(d_lens)
    tab = np.zeros(TOKEN_SLOTS, dtype=np.uint64)

    def entry(v, b):
        return np.uint64(v | (b << 48))

    for b in list(range(256)) + [EOB]:
        if ll_lens[b]:
            tab[TOKEN_EOB if b == EOB else b] = entry(_reverse(ll_codes[b], ll_lens[b]), ll_lens[b])
    ds, deb, dev = distance_symbol(period)
    if d_lens[ds]:
        dist = (_reverse(d_codes[ds], d_lens[ds]) | (dev << d_lens[ds]), d_lens[ds] + deb)
        for length in range(MIN_MATCH, MAX_MATCH + 1):
            s, eb, ev = length_symbol(length)
            if ll_lens[s]:
                v, b = _reverse(ll_codes[s], ll_lens[s]), ll_lens[s]
                v |= ev << b
                b += eb
                v |= dist[0] << b
                b += dist[1]
                tab[TOKEN_MATCH0 + length - MIN_MATCH] = entry(v, b)
    return tab


def build_tables(ll_hist, d_hist, period=1):
    """the device's two histograms -> (ll_lens, d_lens, header value, header bits, token table); period: the match distance of
    the call that counted them (mt_deflate_tokenize_period)."""
    ll_lens = code_lengths(ll_hist, MAX_BITS)
    d_lens = code_lengths(d_hist, MAX_BITS, at_least_two=False)
    value, nbits = dynamic_header(ll_lens, d_lens)
    return ll_lens, d_lens, value, nbits, token_table(ll_lens, d_lens, period)


# ---- CRC-32 (IEEE 802.3, reflected, polynomial 0xedb88320) of a concatenation from the CRCs of its parts ----
def _gf2_times(mat, vec):
    s, k = 0, 0
    while vec:
        if vec & 1:
            s ^= mat[k]
        vec >>= 1
        k += 1
    return s


def _gf2_square(mat):
    return [_gf2_times(mat, mat[k]) for k in range(32)]


def crc32_shift_operator(nbytes):
    """the 32 x 32 GF(2) matrix (32 column words) that advances a CRC register over `nbytes` zero bytes."""
    op = [0xedb88320] + [1 << k for k in range(31)]        # one zero BIT
    op = _gf2_square(_gf2_square(_gf2_square(op)))         # one zero byte
    result = [1 << k for k in range(32)]
    while nbytes:
        if nbytes & 1:
            result = [_gf2_times(op, result[k]) for k in range(32)]
        nbytes >>= 1
        if nbytes:
            op = _gf2_square(op)
    return result


def crc32_combine(crc1, crc2, len2, op=None):
    """zlib.crc32(a + b) from crc1 = zlib.crc32(a), crc2 = zlib.crc32(b) and len2 = len(b); `op` = crc32_shift_operator(len2)."""
    if len2 == 0:
        return crc1
    return _gf2_times(op if op is not None else crc32_shift_operator(len2), crc1) ^ crc2


def crc32_join(crcs, chunk, last_len):
    """the CRC of the whole stream from its per-chunk CRCs: all chunks have `chunk` bytes but the last, which has `last_len`."""
    crcs = [int(c) for c in crcs]
    crc = crcs[0]
    if len(crcs) > 1:
        op = crc32_shift_operator(chunk)
        for c in crcs[1:-1]:
            crc = crc32_combine(crc, c, chunk, op)
        crc = crc32_combine(crc, crcs[-1], last_len)
    return crc


def chunk_count(n, chunk):
    return max(1, -(-n // chunk))


def gzip_member(deflate_stream, crc, n):
    return GZIP_HEADER + bytes(deflate_stream) + struct.pack('<II', crc & 0xffffffff, n & 0xffffffff)
