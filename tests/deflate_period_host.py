"""A numpy / Python restatement of the period / raw-stream / segment forms of the device DEFLATE encoder (csrc/deflate.hip through
ops.deflate_raw and ops.deflate_segments) and of the .npz member built on them, written from include/mtseg.h, DESIGN.md §6w and
RFC 1951, not from the kernels.  The pieces that do not depend on the period (canonical codes, the block header, bit packing, stored
blocks, the CRC combine) are deflate_host.py's; from the product only the code-LENGTH construction is used, as there.

`raw(x, chunk, period, final)` is what `ops.deflate_raw(payload, prefix, chunk, period, final)` must return for x = prefix + payload;
`segments(x, chunk, period, segment)` the bodies of `ops.deflate_segments`."""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deflate_host import (_lsb, block_header, canonical, crc_combine, length_code, pack, split, stored_blocks,  # noqa: E402
                          stored_size)
from multitalent_amd.utilities.deflate_host import code_lengths  # noqa: E402

PERIODS = (1, 2, 4, 8)
DIST = {1: (0, ''), 2: (1, ''), 4: (3, ''), 8: (5, '1')}            # distance -> (symbol, its extra bits): 8 is the upper half of 7..8


def tokenize(x, period):
    """One chunk -> list of tokens: an int 0..255 is a literal, ('m', L) a match of length L at distance `period`.
    Position p is in a run when p >= period and x[p] == x[p - period].  Every maximal stretch of such positions is matches of 258
    while 258 positions remain, then the rest as one match when it is 3 or longer and as its 1 or 2 literals otherwise; every other
    position is a literal."""
    x = np.frombuffer(bytes(x), dtype=np.uint8)
    n = len(x)
    inrun = np.zeros(n, dtype=bool)
    if n > period:
        inrun[period:] = x[period:] == x[:-period]
    out, p = [], 0
    while p < n:
        if not inrun[p]:
            out.append(int(x[p]))
            p += 1
            continue
        q = p
        while q < n and inrun[q]:
            q += 1
        rest = q - p
        out.extend([('m', 258)] * (rest // 258))
        rest %= 258
        if rest >= 3:
            out.append(('m', rest))
        else:
            out.extend(int(v) for v in x[q - rest:q])
        p = q
    return out


def expand(toks, period):
    """the bytes a token list stands for (what an inflater makes of it)"""
    out = bytearray()
    for t in toks:
        if isinstance(t, tuple):
            for _ in range(t[1]):
                out.append(out[-period])
        else:
            out.append(t)
    return bytes(out)


def histograms(chunks_tokens, period):
    ll, d = [0] * 286, [0] * 30
    for toks in chunks_tokens:
        for t in toks:
            if isinstance(t, tuple):
                ll[length_code(t[1])[0]] += 1
                d[DIST[period][0]] += 1
            else:
                ll[t] += 1
        ll[256] += 1
    return ll, d


def token_bits(toks, ll, d, period):
    ds, dextra = DIST[period]
    parts = []
    for t in toks:
        if isinstance(t, tuple):
            s, eb, ev = length_code(t[1])
            parts.append(ll[s] + _lsb(ev, eb) + d[ds] + dextra)
        else:
            parts.append(ll[t])
    parts.append(ll[256])
    return ''.join(parts)


def raw_chunks(x, chunk, period=1, final=True):
    """-> list of the chunks' encoded bytes: one dynamic block each under the call's one code table, every chunk but a final call's
    last one byte-aligned by an empty stored block; stored blocks where those are smaller."""
    x = bytes(x)
    chunks = split(x, chunk)
    toks = [tokenize(c, period) for c in chunks]
    ll_hist, d_hist = histograms(toks, period)
    ll_lens, d_lens = code_lengths(ll_hist, 15), code_lengths(d_hist, 15, at_least_two=False)
    ll, d = canonical(ll_lens), (canonical(d_lens) if any(d_lens) else {})
    header = block_header(ll_lens, d_lens)
    out = []
    for k, (c, t) in enumerate(zip(chunks, toks)):
        last = final and k == len(chunks) - 1
        bits = ('1' if last else '0') + header + token_bits(t, ll, d, period)
        if not last:
            bits += '000'
            bits += '0' * (-len(bits) % 8) + _lsb(0, 16) + _lsb(0xffff, 16)
        enc = pack(bits)
        out.append(stored_blocks(c, last) if stored_size(len(c)) < len(enc) else enc)
    return out


def crc_of_chunks(x, chunk):
    parts = split(bytes(x), chunk)
    crc = zlib.crc32(parts[0])
    for p in parts[1:]:
        crc = crc_combine(crc, zlib.crc32(p), len(p))
    return crc


def raw(x, chunk, period=1, final=True):
    """-> (body, crc, n) as ops.deflate_raw returns them"""
    return b''.join(raw_chunks(x, chunk, period, final)), crc_of_chunks(x, chunk), len(bytes(x))


def segments(x, chunk, period, segment):
    """-> (list of bodies, crc, n) as ops.deflate_segments yields them: the stream in pieces of `segment` bytes, each its own call
    (its own code table), only the last final; the CRC joined from the pieces' CRCs."""
    x = bytes(x)
    parts = split(x, segment)
    bodies, crc = [], 0
    for k, p in enumerate(parts):
        body, c, _ = raw(p, chunk, period, k == len(parts) - 1)
        bodies.append(body)
        crc = crc_combine(crc, c, len(p)) if k else c
    return bodies, crc, len(x)


def inflate(body):
    d = zlib.decompressobj(-15)
    out = d.decompress(bytes(body)) + d.flush()
    assert d.eof and not d.unused_data
    return out


# ---- the .npz member: a .npy v1.0 header (numpy's own) in front of the array's bytes, matched at the element size ----
def npy_prefix(arr):
    import io
    f = io.BytesIO()
    np.lib.format.write_array_header_1_0(f, np.lib.format.header_data_from_array_1_0(np.ascontiguousarray(arr)))
    return f.getvalue()


def npz_member_size(arr, chunk=65536):
    """compressed bytes of the member `arr` becomes in the device writer's file"""
    a = np.ascontiguousarray(arr)
    return len(raw(npy_prefix(a) + a.tobytes(), chunk, a.dtype.itemsize, True)[0])


# ---- the inputs the CPU and GPU tests share ----
def softmax_volume(shape=(3, 8, 24, 40), sharp=6.0, seed=0):
    """float16 class probabilities [C, X, Y, Z] with saturated regions: smooth logits, scaled so that most voxels round to exactly
    0.0 / 1.0 in float16 and the class borders keep graded values."""
    rs = np.random.RandomState(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, s) for s in shape[1:]], indexing='ij')
    logits = np.stack([sharp * 8 * (np.cos(3 * (g[0] + 0.4 * c)) + np.sin(2 * g[1] - c) + g[2] * (c - 1)) + 0.01 * rs.randn(*shape[1:])
                       for c in range(shape[0])])
    e = np.exp(logits - logits.max(0))
    return (e / e.sum(0)).astype(np.float16)


def training_case(shape=(2, 8, 24, 40), seed=1):
    """float32 [C + 1, X, Y, Z]: normal data that is zero outside a mask, and a label channel of small integers (and -1) as floats"""
    rs = np.random.RandomState(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, s) for s in shape[1:]], indexing='ij')
    r = np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)
    out = np.zeros(shape, dtype=np.float32)
    for c in range(shape[0] - 1):
        out[c] = np.where(r < 0.8, rs.randn(*shape[1:]), 0.0)
    out[-1] = np.where(r < 0.3, 2.0, np.where(r < 0.6, 1.0, np.where(r < 0.8, 0.0, -1.0)))
    return out


SIZE_INPUTS = {'softmax': softmax_volume, 'case': training_case}


def stretch(period, k, seed=0):
    """bytes with one in-run stretch of exactly k positions between literals that match nothing"""
    rs = np.random.RandomState(seed + k)
    unit = bytes(rs.randint(1, 200, period).astype(np.uint8))
    body = (unit * (k // period + 2))[:period + k]
    head = bytes(range(200, 200 + period + 3))
    tail = bytes(range(220, 220 + period + 3))
    return head + body + tail


def cases(chunk, period):
    rs = np.random.RandomState(1000 * period + chunk)
    out = {'empty': b'', 'below_period': bytes(rs.randint(0, 3, period - 1).astype(np.uint8)) if period > 1 else b'\x05',
           'zeros': bytes(2 * chunk + 300),
           'half_one': np.full(chunk + 77, 1.0, np.float16).tobytes(),
           'random': rs.bytes(3 * chunk + 7),
           'ragged': (np.repeat(rs.randint(0, 4, 50).astype(np.uint8), 8 * period)).tobytes()[:50 * 8 * period - 1 - (period > 2)]}
    for k in (258, 516):
        for r in (0, 1, 2, 3):
            out['stretch%d' % (k + r)] = stretch(period, k + r)
    # a stretch over the 4096-byte tile edge (when the chunk has one) and one over the chunk edge, where it must split
    unit = bytes(rs.randint(1, 250, period).astype(np.uint8))
    out['tile_edge'] = rs.bytes(4096 - 40) + (unit * 400)[:90] + rs.bytes(33)
    out['chunk_edge'] = rs.bytes(max(chunk - 130, 3)) + (unit * 400)[:300] + rs.bytes(9)
    elems = np.frombuffer(rs.bytes(8 * 6), dtype=np.uint8).reshape(6, 8)[:, :period]
    out['elements'] = np.repeat(elems, rs.randint(1, 40, 6), axis=0).tobytes() * 3
    return out
