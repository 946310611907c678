"""The restatement of the decoder for streams without restart points (inflate_spec_host.py) against zlib, on the CPU: every stream at
three chunk sizes, the search on every true block start, pinned candidate lists, the property each stream exists for, and the pinned
status of every damaged stream.  tests/test_inflate_spec_gpu.py compares the device with the same restatement."""
import os
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_host as I  # noqa: E402
import inflate_spec_host as S  # noqa: E402

CHUNKS = (64, 256, 4096)
ANY_SPAN = 1 << 30                  # the span limit is a condition of its own (test_fixed_stream_over_the_span_limit_is_too_long)

# stream -> {chunk: (candidates, CRC-32 of their decimal positions joined by commas)}; written down from a run of this file
PINS = {
 'ct_l1_m8': {64: (2, 759703912), 256: (2, 759703912), 4096: (2, 759703912)},
 'ct_l1_m1': {64: (259, 1102493698), 256: (181, 3081080261), 4096: (14, 3698713980)},
 'ct_l6_m8': {64: (2, 2973308707), 256: (2, 2973308707), 4096: (2, 2973308707)},
 'ct_l6_m1': {64: (118, 1661671293), 256: (108, 2237035594), 4096: (12, 4114964884)},
 'ct_l9_m8': {64: (2, 2973308707), 256: (2, 2973308707), 4096: (2, 2973308707)},
 'ct_l9_m1': {64: (130, 49642902), 256: (117, 2177318230), 4096: (12, 4193066393)},
 'motif': {64: (62, 3987476411), 256: (62, 3987476411), 4096: (8, 2460396720)},
 'exact_window': {64: (2, 283534693), 256: (2, 283534693), 4096: (2, 283534693)},
 'long_matches': {64: (136, 1565185271), 256: (74, 3559447370), 4096: (10, 624496159)},
 'noise': {64: (1, 4108050209), 256: (1, 4108050209), 4096: (1, 4108050209)},
 'noise_between': {64: (2, 1979284403), 256: (2, 1979284403), 4096: (2, 1979284403)},
 'fixed': {64: (1, 4108050209), 256: (1, 4108050209), 4096: (1, 4108050209)},
 'huffman_only': {64: (3, 1601896106), 256: (3, 1601896106), 4096: (3, 1601896106)},
 'rle': {64: (3, 1699957227), 256: (3, 1699957227), 4096: (3, 1699957227)},
 'sync_flushed': {64: (9, 2738353858), 256: (7, 842254367), 4096: (4, 2640735784)},
 'full_flushed': {64: (13, 1276176849), 256: (13, 1276176849), 4096: (3, 1441127490)},
 'false_candidates': {64: (51, 1272960503), 256: (48, 1642883341), 4096: (8, 3367213527)},
 'last_byte': {64: (2, 1370864160), 256: (2, 1370864160), 4096: (2, 1370864160)},
 'short': {64: (1, 4108050209), 256: (1, 4108050209), 4096: (1, 4108050209)},
 'one_final_block': {64: (1, 4108050209), 256: (1, 4108050209), 4096: (1, 4108050209)},
}


@pytest.fixture(scope='module')
def decoded():
    """name -> (stream, bytes, accepted positions, {chunk: (out, crc, info)}), every stream decoded once per chunk size"""
    out = {}
    for name, (body, x) in S.streams().items():
        hits, blocks = S.accepted(body), {}
        out[name] = (body, x, hits, {c: S.inflate(body, c, span_limit=ANY_SPAN, hits=hits, blocks=blocks) for c in CHUNKS})
    return out


def _pin(cands):
    return len(cands), zlib.crc32(','.join(str(c) for c in cands).encode())


def test_restatement_equals_zlib(decoded):
    for name, (body, x, _, by_chunk) in decoded.items():
        assert zlib.decompressobj(-15).decompress(body) == x, name
        for chunk, (out, crc, info) in by_chunk.items():
            assert info['status'] == S.OK and out == x and crc == zlib.crc32(x), (name, chunk, info['status'])
            assert info['total'] == len(x) and info['units'][0] == 0 and set(info['units']) <= set(info['candidates'])


def test_every_true_dynamic_block_start_is_accepted(decoded):
    seen = 0
    for name, (body, x, hits, _) in decoded.items():
        true = [bit for bit, kind, final in S.block_starts(body) if kind == 2 and not final and bit > 0]
        assert set(true) <= set(hits), name
        seen += len(true)
    assert seen > 500


def test_candidate_lists_are_pinned(decoded):
    got = {name: {c: _pin(by_chunk[c][2]['candidates']) for c in CHUNKS} for name, (_, _, _, by_chunk) in decoded.items()}
    assert got == PINS, got


def test_short_blocks_give_many_units_and_chained_windows(decoded):
    """memLevel 1: blocks of 127 symbols, fixed ones among them, units far shorter than the window"""
    for level in (1, 6, 9):
        body, x, hits, by_chunk = decoded['ct_l%d_m1' % level]
        kinds = [kind for _, kind, _ in S.block_starts(body)]
        assert kinds.count(2) > 100 and kinds.count(1) > 20
        info = by_chunk[256][2]
        assert len(info['units']) >= 20 and info['shortest_unit'] < 1000 and info['hops'] >= 2
        body8, _, _, by8 = decoded['ct_l%d_m8' % level]
        assert len(by8[256][2]['units']) >= 2 and by8[256][2]['max_reach'] > 20000


def test_maximum_distance_crosses_a_unit_start(decoded):
    info = decoded['exact_window'][3][256][2]
    assert len(info['units']) == 2 and info['max_reach'] == S.WIN
    second = info['results'][info['units'][1]]
    assert second['sym'][0] == 0x8000 and second['matches'][0] == (0, S.WIN)  # the first symbol names the oldest byte of the window
    info = decoded['motif'][3][256][2]
    assert len(info['units']) > 20 and info['max_reach'] > 32000            # zlib's own farthest distance is 32768 - 262


def test_long_matches_blow_a_unit_up(decoded):
    body, x, _, by_chunk = decoded['long_matches']
    info = by_chunk[4096][2]
    big = [(len(info['results'][u]['sym']), (info['results'][u]['end'] - u + 7) // 8) for u in info['units']]
    assert any(out > 1 << 20 and comp < 4096 for out, comp in big), big
    assert any(dist == 1 for u in info['units'] for _, dist in info['results'][u]['matches'])


def test_stored_blocks(decoded):
    body, x, hits, by_chunk = decoded['noise']
    assert all(kind == 0 for _, kind, _ in S.block_starts(body)) and hits == []
    for chunk in CHUNKS:
        info = by_chunk[chunk][2]
        assert info['candidates'] == [0] and info['units'] == [0] and info['spans'] == len(S.block_starts(body))
    body, x, hits, by_chunk = decoded['noise_between']
    starts = S.block_starts(body)
    kinds = [kind for _, kind, _ in starts]
    at = kinds.index(0)
    assert at > 0 and starts[at][0] % 8 != 0                                # a stored block behind a block end inside a byte
    info = by_chunk[256][2]
    assert info['spans'] >= 2
    hit = 0                                                                 # a later match whose source lies in stored bytes
    offset = 0
    stored = []
    for u in info['units']:
        stored += [(offset + o, offset + o + n) for _, o, n in info['results'][u]['spans']]
        hit += sum(1 for pos, dist in info['results'][u]['matches'] if any(a <= offset + pos - dist < b for a, b in stored))
        offset += len(info['results'][u]['sym'])
    assert hit > 0


def test_streams_without_dynamic_headers(decoded):
    body, x, hits, by_chunk = decoded['fixed']
    assert all(kind == 1 for _, kind, _ in S.block_starts(body)) and hits == [] and by_chunk[64][2]['units'] == [0]
    info = decoded['huffman_only'][3][256][2]
    assert all(not info['results'][u]['matches'] for u in info['units']) and info['max_reach'] == 0
    info = decoded['rle'][3][256][2]
    assert {d for u in info['units'] for _, d in info['results'][u]['matches']} == {1} and info['max_reach'] <= 1


def test_fixed_stream_over_the_span_limit_is_too_long():
    body, chunk, kw, _ = S.malformed()['fixed_over_span_limit']
    assert len(body) > S.SPAN_CHUNKS * chunk
    assert S.scan(body, chunk)['status'] == S.TOO_LONG and S.scan(body, 4096)['status'] == S.OK


def test_flushed_streams_are_read(decoded):
    """the restart-point decoder calls the sync-flushed stream BAD (the dictionary survives the flush); this one reads both"""
    assert I.scan(decoded['sync_flushed'][0])['status'] == I.BAD and I.scan(decoded['full_flushed'][0])['status'] == I.OK
    assert decoded['sync_flushed'][3][256][2]['max_reach'] > 0 and decoded['full_flushed'][3][256][2]['max_reach'] == 0
    assert len(decoded['sync_flushed'][3][256][2]['units']) > 3


def test_false_candidates_are_never_chained(decoded):
    body, x, hits, by_chunk = decoded['false_candidates']
    true = {bit for bit, _, _ in S.block_starts(body)}
    assert 0 in [kind for _, kind, _ in S.block_starts(body)], "zlib stores part of the inner stream"
    for chunk in CHUNKS:
        out, crc, info = by_chunk[chunk]
        false = [c for c in info['candidates'] if c not in true]
        assert false and not set(false) & set(info['units']) and out == x
        if chunk == 64:
            assert len(false) > 40 and any(info['results'][c]['status'] == S.OK for c in false)
            assert any(info['results'][c]['status'] != S.OK for c in false)


def test_edge_conditions(decoded):
    body, x, hits, by_chunk = decoded['last_byte']
    assert hits == [8 * 63] and by_chunk[64][2]['units'] == [0, 8 * 63]     # the header starts in the last byte of the first chunk
    assert by_chunk[64][2]['results'][8 * 63]['end'] == 8 * len(body)
    body, x, hits, by_chunk = decoded['short']
    assert len(body) < 64 and all(by_chunk[c][2]['units'] == [0] for c in CHUNKS)
    assert [final for _, _, final in S.block_starts(decoded['one_final_block'][0])] == [True]


def test_damaged_streams_have_their_status():
    want = {'flipped_header': S.BAD, 'flipped_payload': S.OK, 'truncated': S.BAD, 'before_stream_unit0': S.CORRUPT,
            'before_stream_unit1': S.CORRUPT, 'wrong_size': S.SIZE, 'fixed_over_span_limit': S.TOO_LONG}
    got = {}
    for name, (body, chunk, kw, data) in S.malformed().items():
        out, crc, info = S.inflate(body, chunk, **kw)
        got[name] = info['status']
        if name == 'flipped_payload':                                       # only the CRC-32 of the file tells
            good = S.streams()['noise'][1]
            assert out == data != good and crc != zlib.crc32(good)
        if name == 'before_stream_unit1':                                   # the chain is whole; the marker fails when it is resolved
            assert len(info['units']) == 2 and info['results'][info['units'][1]]['reach'] == 200
        d = zlib.decompressobj(-15)
        try:
            d.decompress(body)
            whole = d.eof
        except zlib.error:
            whole = False
        assert whole == (name in ('flipped_payload', 'wrong_size', 'fixed_over_span_limit')), name    # zlib's own verdict
    assert got == want
