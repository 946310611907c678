"""Shared by tests/test_conv_dispatch_cpu.py and tools/record_dispatch.py (not a test module).

The forward / backward-data dispatch tables: which kernel `mt_conv3d_fwd` and `mt_conv3d_bwd_data_strided` take for a problem and what
the queries over that decision answer (chunk size, pack layout, statistics partials, storage types, fused norm-backward statistics).
Two tables, FWD and BWDD, in the form of bwdw_dispatch_cases (whose hash, thinning and fake-address helpers they use): every row is a
valid problem with fake, non-null pointers of chosen alignment, the MAJOR axes are crossed in full, and every major row appears once with
the MINOR axes at their defaults and once with a hash-drawn combination.  EXTRA adds the rows the thinning misses.
"""
import ctypes as C

from bwdw_dispatch_cases import MT_F32, MT_BF16, MT_F16, SEL_OFF, SEL_FORCE, _BASE, _ALIGN_OFF, _src, thinned, ask  # noqa: F401

SEL_WINO, SEL_M16, SEL_X16, SEL_TAPSPLIT = 0, 2, 4, 6

# (K, S, P, dil, placed): `placed` = a stride-1 sub-convolution of a transposed-convolution backward-data, written at every second
# position of a stored volume twice the size (osD/osH/osW = 2, offset 1)
GEOS = [((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((3, 3, 3), (2, 2, 2), (1, 1, 1), 1, False),
        ((3, 3, 3), (1, 2, 2), (1, 1, 1), 1, False), ((2, 2, 2), (2, 2, 2), (0, 0, 0), 1, False), ((1, 2, 2), (1, 2, 2), (0, 0, 0), 1, False),
        ((1, 1, 1), (1, 1, 1), (0, 0, 0), 1, False), ((3, 3, 1), (1, 1, 1), (1, 1, 0), 1, False), ((3, 3, 3), (1, 1, 1), (1, 1, 1), 2, False),
        ((2, 2, 2), (1, 1, 1), (0, 0, 0), 1, True)]
CHANNELS = [((1,), 30), ((30,), 30), ((30, 30), 30), ((60,), 32), ((16,), 64), ((320,), 320), ((31,), 30)]     # (channels per source, Cout)
SIZES = [(3, 6, 6), (6, 24, 24), (48, 192, 192), (2, 9, 20)]                                                   # output size
BATCH = [1, 2]
DTYPES = [MT_F32, MT_BF16, MT_F16]
MMA = [0, 1]
ALIGN = ['ok', 'odd_cs', 'base4', 'base2']          # odd channel stride; base = 4 mod 8; base = 2 mod 4


class Table:
    """One dispatch table: axes, rows and the library's answers (the interface tools/record_dispatch.py records)."""

    def __init__(self, prefix, major, minor, minor_default, extra, columns, families, problem, query):
        self.PREFIX, self.MAJOR, self.MINOR, self.MINOR_DEFAULT, self.EXTRA = prefix, major, minor, minor_default, extra
        self.COLUMNS, self.FAMILIES, self.problem, self.query = columns, families, problem, query

    def rows(self):
        return thinned(self.MAJOR, self.MINOR, self.MINOR_DEFAULT, self.EXTRA)

    def family(self, name):
        stem = name.split('<')[0]
        return stem if stem in self.FAMILIES else None


def _name(fn, p):
    buf = C.create_string_buffer(128)
    rc = fn(C.byref(p), buf, 128)
    return buf.value.decode() if rc == 0 else '<rc %d>' % rc


def _dst_ptr(slot, align):
    return _BASE + slot * 0x10000000 + _ALIGN_OFF[align]


# ---- forward: mt_conv3d_fwd
def _sel(shift):
    return [SEL_OFF << shift, SEL_FORCE << shift]


FWD_MINOR = [[None, 0.01, 1.5],                                                                  # lazy-activation slope of the sources
             ALIGN, ALIGN,                                                                       # sources, destination
             [0] + _sel(SEL_WINO) + _sel(SEL_M16) + _sel(SEL_X16) + _sel(SEL_TAPSPLIT),
             [0, 3],                                                                             # max_workgroups
             [False, True],                                                                      # stats_part
             [False, True],                                                                      # bstats (sets stats_part too)
             [False, True]]                                                                      # csplit = Cout / 2 with out1
FWD_MINOR_DEFAULT = (None, 'ok', 'ok', 0, 0, False, False, False)

_G333, _G133, _GS2, _GS122, _G222, _G122, _G111, _G331, _GDIL, _GPLACED = GEOS
_D = FWD_MINOR_DEFAULT
# rows the thinning misses (tools/record_dispatch.py --table conv --census N), and the pair of planes around the packed-offset limit of the
# persistent Winograd kernel: (5 Hi + 5) Wi + 17 < 2^20 holds for 400 x 522 and fails for 400 x 524
FWD_EXTRA = [
    ((_G333, ((30,), 30), (4, 400, 522), 1, MT_F32, MT_F32, 0), _D),
    ((_G333, ((30,), 30), (4, 400, 524), 1, MT_F32, MT_F32, 0), _D),
    ((_G333, ((30,), 30), (4, 400, 522), 1, MT_F32, MT_F32, 0), (None, 'ok', 'ok', 0, 0, False, True, False)),
    ((_G333, ((30,), 30), (4, 400, 524), 1, MT_F32, MT_F32, 0), (None, 'ok', 'ok', 0, 0, False, True, False)),
    # FAST geometry with strided placement and two destinations: neither the fast nor the runtime-geometry kernel -> conv_fwd_kernel<.., true>
    ((((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, True), ((30,), 30), (3, 6, 6), 1, MT_F32, MT_F32, 0), (None, 'ok', 'ok', 0, 0, False, False, True)),
    ((_G333, ((16,), 64), (2, 9, 20), 1, 0, 0, 1), (None, 'ok', 'base2', 8, 3, True, False, True)),    # conv_bf16_kernel<32, 4, 2, 2, 1, 4, 3, 0, 0, 1>
    ((_G133, ((30,), 30), (2, 9, 20), 2, 1, 2, 1), (0.01, 'base4', 'odd_cs', 8, 3, False, True, False)),    # conv_bf16_kernel<32, 4, 2, 4, 1, 4, 1, 1, 1, 1>
    ((_G333, ((16,), 64), (2, 9, 20), 2, 1, 1, 1), (None, 'base4', 'base2', 8, 0, True, True, True)),    # conv_bf16_kernel<32, 4, 2, 4, 1, 4, 3, 1, 1, 1>
    # the 2 x 4 x 16 tile of conv_fast_kernel with staging width 1 and 2: eight (or one) input channels on a grid too small for the wide tile
    ((((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((8,), 8), (2, 4, 16), 1, 0, 0, 1), (None, 'base4', 'odd_cs', 40, 3, False, False, True)),    # conv_fast_kernel<16, 2, 2, 1, 1>
    ((((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((1,), 30), (2, 4, 16), 1, 0, 0, 0), (0.01, 'ok', 'ok', 66, 0, True, True, True)),    # conv_fast_kernel<16, 2, 2, 1, 3>
    ((((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((8,), 8), (2, 4, 16), 1, 0, 0, 1), (0.01, 'ok', 'ok', 66, 3, False, True, True)),    # conv_fast_kernel<16, 2, 2, 2, 1>
]


def fwd_problem(major, minor):
    """(mt_conv3d_t,) of one forward row."""
    from multitalent_amd._lib import mt_conv3d_t
    (K, S, Pd, dil, placed), (cins, cout), out, N, xdt, odt, mma = major
    lazy, align_x, align_o, select, max_wgs, stats, bstats, split = minor
    p = mt_conv3d_t()
    p.nsrc = len(cins)
    for i, c in enumerate(cins):
        _src(p.src[i], i, c, xdt, lazy, align_x)
    p.N = N
    p.Do, p.Ho, p.Wo = out
    # the stored input whose zero-inserted (dil) extent the taps cover
    p.Di, p.Hi, p.Wi = [max(1, ((o - 1) * s + k - 2 * q - 1) // dil + 1) for o, s, k, q in zip(out, S, K, Pd)]
    p.dilD = p.dilH = p.dilW = dil
    p.KD, p.KH, p.KW = K
    p.SD, p.SH, p.SW = S
    p.PD, p.PH, p.PW = Pd
    p.Cin, p.Cout = sum(cins), cout
    p.wpack = _BASE + 0xa0000000
    p.out0, p.ocs0, p.odtype = _dst_ptr(4, align_o), ((cout + 1) | 1) if align_o == 'odd_cs' else cout, odt
    p.csplit = cout
    if split:
        p.csplit, p.out1, p.ocs1 = cout // 2, _dst_ptr(5, align_o), p.ocs0
    if stats or bstats:
        p.stats_part = _BASE + 0xb0000000
    if bstats:
        b = p.bstats
        b.y, b.mean, b.rstd, b.ycs, b.c0, b.C, b.slope = _BASE + 0xc0000000, _BASE + 0xc8000000, _BASE + 0xc9000000, cout, 0, cout, 0.01
    if placed:
        p.OD, p.OH, p.OW = [2 * o for o in out]
        p.osD = p.osH = p.osW = 2
        p.ooD = p.ooH = p.ooW = 1
    else:
        p.OD, p.OH, p.OW = out
        p.osD = p.osH = p.osW = 0
    p.mma, p.select, p.max_workgroups = mma, select, max_wgs
    return (p,)


def fwd_query(lib, p):
    r = C.byref(p)
    return (_name(lib.mt_conv3d_kernel_name, p), int(lib.mt_conv3d_ck(r)), int(lib.mt_conv3d_pack_layout(r)), int(lib.mt_conv3d_stats_blocks(r)),
            int(lib.mt_conv3d_io_supported(r)), int(lib.mt_conv3d_bwd_stats_supported(r)))


FWD = Table('', [GEOS, CHANNELS, SIZES, BATCH, DTYPES, DTYPES, MMA], FWD_MINOR, FWD_MINOR_DEFAULT, FWD_EXTRA,
            [('ck', 'int16'), ('pack_layout', 'uint8'), ('stats_blocks', 'int32'), ('io_supported', 'uint8'), ('bwd_stats_supported', 'uint8')],
            ['conv_stem_kernel', 'conv_wino8p_kernel', 'conv_wino8pb_kernel', 'conv_fast_kernel', 'conv_tapsplit_kernel', 'conv_fast_strided_kernel',
             'conv_bf16_kernel', 'conv_x16_kernel', 'conv_gather_kernel', 'conv_rt_kernel', 'conv_fwd_kernel'],
            fwd_problem, fwd_query)


# ---- strided backward-data: mt_conv3d_bwd_data_strided (p carries the FORWARD geometry, src[0] = dY, out0 = dX)
BWDD_GEOS = [_GS2, _GS122, _G333]                    # the last one is refused
BWDD_MINOR = [ALIGN, [0] + _sel(SEL_M16) + _sel(SEL_TAPSPLIT)]
BWDD_MINOR_DEFAULT = ('ok', 0)
BWDD_EXTRA = []


def bwdd_problem(major, minor):
    from multitalent_amd._lib import mt_conv3d_t
    (K, S, Pd, dil, _), (cins, cout), out, N, ydt, xdt, mma = major
    align_y, select = minor
    cin = sum(cins)
    p = mt_conv3d_t()
    p.nsrc = 1
    _src(p.src[0], 0, cout, ydt, None, align_y)
    p.N = N
    p.Do, p.Ho, p.Wo = out
    p.Di, p.Hi, p.Wi = [max(1, (o - 1) * s + k - 2 * q) for o, s, k, q in zip(out, S, K, Pd)]
    p.dilD = p.dilH = p.dilW = dil
    p.KD, p.KH, p.KW = K
    p.SD, p.SH, p.SW = S
    p.PD, p.PH, p.PW = Pd
    p.Cin, p.Cout, p.csplit = cin, cout, cout
    p.wpack = _BASE + 0xa0000000
    p.out0, p.ocs0, p.odtype = _dst_ptr(4, 'ok'), cin, xdt
    p.OD, p.OH, p.OW = out
    p.mma, p.select = mma, select
    return (p,)


def bwdd_query(lib, p):
    r = C.byref(p)
    return (_name(lib.mt_conv3d_bwd_data_strided_kernel_name, p), int(lib.mt_conv3d_bwd_data_strided_supported(r)),
            int(lib.mt_conv3d_bwd_data_strided_pack_layout(r)), int(lib.mt_conv3d_bwd_data_strided_io_supported(r)))


BWDD = Table('bwdd_', [BWDD_GEOS, CHANNELS, SIZES, BATCH, DTYPES, DTYPES, MMA], BWDD_MINOR, BWDD_MINOR_DEFAULT, BWDD_EXTRA,
             [('supported', 'uint8'), ('pack_layout', 'uint8'), ('io_supported', 'uint8')],
             ['conv_bwdd_strided_kernel', 'conv_bwdd_strided_ks_kernel'], bwdd_problem, bwdd_query)
# every instance launch_bwdd_strided can pick, per depth stride
BWDD_INSTANCES = ['conv_bwdd_strided_ks_kernel<%d, 2, 2>', 'conv_bwdd_strided_kernel<%d, 2, 2, 4, true, 1, 1>',
                  'conv_bwdd_strided_kernel<%d, 2, 2, 2, true, 0, 1>', 'conv_bwdd_strided_kernel<%d, 2, 2, 2, true, 0, 0>',
                  'conv_bwdd_strided_kernel<%d, 2, 2, 2, false, 0, 0>', 'conv_bwdd_strided_kernel<%d, 2, 2, 1, false, 0, 0>']
