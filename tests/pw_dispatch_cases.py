"""Shared by tests/test_pw_dispatch_cpu.py and tools/record_dispatch.py (not a test module).

The pointwise and head-backward dispatch tables: which kernel instance `mt_pointwise_fwd` and `mt_head_bwd` launch for a problem, with
which grid and store form, and what the queries over that decision answer.  Two tables, FWD and HB, in the form of conv_dispatch_cases
(whose Table they are) over the hash, thinning and fake-address helpers of bwdw_dispatch_cases: the MAJOR axes are crossed in full,
every major row appears once with the MINOR axes at their defaults and once with a hash-drawn combination, EXTRA adds the rows the
thinning misses.  Nothing in either decision reads the device's compute-unit count (head_bwd_waves caps at a constant 256 x 16 waves,
the grids are functions of the problem), so the table holds on any device.
"""
import ctypes as C

from bwdw_dispatch_cases import MT_F32, MT_BF16, MT_F16, _BASE, _src
from conv_dispatch_cases import Table, _name

DTYPES = [MT_F32, MT_BF16, MT_F16]
SLOPES = [None, 0.01, 1.0, -0.5, 2.0]              # lazy activation of the source: None = plain, else scale / shift set with this slope

# ---- forward: mt_pointwise_fwd
# (input stride, output stride, scatter, stored input one voxel larger than the base grid)
GEOS = [((1, 1, 1), (1, 1, 1), 0, False), ((1, 1, 1), (2, 2, 2), 0, False), ((1, 1, 1), (1, 2, 2), 0, False), ((1, 1, 1), (1, 1, 2), 0, False),
        ((2, 2, 2), (1, 1, 1), 0, False), ((1, 1, 1), (2, 2, 2), 1, False), ((1, 1, 1), (1, 1, 1), 0, True)]
G_UNIT, G_T8, G_T4, G_T2, G_PROJ, G_SCATTER, G_DI = GEOS
CIN = [8, 20, 30, 32, 47, 60, 64, 320, 1040]       # 1040 exceeds PW_MAXC: refused
COUT = [1, 2, 4, 5, 14, 30, 32, 33, 47, 64, 65, 320]
MMA = [0, 1]
# base grids: Wb % 32 zero (then Vb % 32 is zero too) | Wb % 32 and Vb % 32 non-zero | Wb % 32 non-zero, Vb % 32 zero | rows longer than 32
BASES = [(2, 3, 32), (2, 3, 5), (4, 4, 6), (3, 5, 40)]
OCS = ['dense', 'mult4', 'odd']                    # Cout | the next multiple of 4 above Cout | odd
OUT_ALIGN = [16, 8, 4]                             # bytes
SRC_CS = [0, 6]                                    # src.cs - Cin
SRC_ALIGN = [8, 4, 2]
FWD_MINOR = [BASES, OCS, OUT_ALIGN, SRC_CS, SRC_ALIGN, SLOPES, [0, 1], [False, True], [1, 2]]    # .., accumulate, stats_part, N
FWD_MINOR_DEFAULT = ((2, 3, 32), 'dense', 16, 0, 8, None, 0, False, 1)
_D = FWD_MINOR_DEFAULT
# rows the thinning misses (tools/record_dispatch.py --table pw --census N)
FWD_EXTRA = [
    # eight taps with statistics, the only way to pw_fast_kernel<8, ...>: the shape of the GPU test, plain and as the M16 form
    ((G_T8, 20, 14, MT_F32, MT_F32, 0), ((2, 3, 5), 'dense', 16, 0, 8, None, 0, True, 2)),
    ((G_T8, 20, 14, MT_F16, MT_F16, 1), ((2, 3, 5), 'dense', 16, 0, 8, 0.01, 0, True, 2)),
    # a 33..64-channel head whose voxel count is no multiple of 32 falls back to two channel tiles of pw_fast_kernel<1, ...>
    ((G_UNIT, 30, 47, MT_F32, MT_F32, 0), ((3, 5, 7), 'dense', 16, 0, 8, 0.01, 0, False, 1)),
]


def _ocs(kind, cout):
    return {'dense': cout, 'mult4': (cout + 4) & ~3, 'odd': (cout + 1) | 1}[kind]


def fwd_problem(major, minor):
    """(mt_pointwise_t,) of one forward row."""
    from multitalent_amd._lib import mt_pointwise_t
    (si, so, scatter, bigger), cin, cout, xdt, odt, mma = major
    base, ocs, out_align, dcs, src_align, slope, accumulate, stats, N = minor
    p = mt_pointwise_t()
    _src(p.src, 0, cin, xdt, slope, 'ok')
    p.src.cs = cin + dcs
    p.src.ptr = p.src.ptr + (src_align % 8)
    p.N = N
    p.Db, p.Hb, p.Wb = base
    p.Di, p.Hi, p.Wi = [b * s + (1 if bigger else 0) for b, s in zip(base, si)]
    p.siD, p.siH, p.siW = si
    p.soD, p.soH, p.soW = so
    p.Cin, p.Cout = cin, cout
    p.wpack = _BASE + 0xa0000000
    p.out, p.ocs, p.odtype = _BASE + 0x40000000 + (out_align % 16), _ocs(ocs, cout), odt
    p.accumulate, p.scatter, p.mma = accumulate, scatter, mma
    if stats:
        p.stats_part = _BASE + 0xb0000000
    return (p,)


def fwd_query(lib, p):
    r = C.byref(p)
    shape = (C.c_int32 * 4)()
    rc = int(lib.mt_pointwise_launch_shape(r, shape))
    return (_name(lib.mt_pointwise_kernel_name, p), rc, shape[0], shape[1], shape[2], shape[3], int(lib.mt_pointwise_pack_layout(r)),
            int(lib.mt_pointwise_io_supported(r)), int(lib.mt_pointwise_stats_blocks(r)))


FWD = Table('', [GEOS, CIN, COUT, DTYPES, DTYPES, MMA], FWD_MINOR, FWD_MINOR_DEFAULT, FWD_EXTRA,
            [('rc', 'int16'), ('grid_x', 'int32'), ('grid_y', 'int32'), ('grid_z', 'int32'), ('wide', 'uint8'), ('pack_layout', 'uint8'),
             ('io_supported', 'uint8'), ('stats_blocks', 'int32')],
            ['pw_fast_kernel', 'pw_head_kernel', 'pw_narrow_kernel'], fwd_problem, fwd_query)
# every instance mt_pointwise_fwd can pick: (source, destination) storage pairs of mt_pointwise_io_supported
_PAIRS = [(MT_F32, MT_F32), (MT_F32, MT_BF16), (MT_BF16, MT_BF16), (MT_BF16, MT_F32), (MT_F16, MT_F16), (MT_F16, MT_F32)]
FWD_INSTANCES = (['pw_fast_kernel<%d, %d, %d, false>' % ((nt,) + pr) for nt in (1, 2, 4, 8) for pr in _PAIRS] +
                 ['pw_fast_kernel<%d, %d, %d, true>' % (nt, MT_F16, MT_F16) for nt in (2, 4, 8)] +
                 ['pw_head_kernel<%d, false>' % xs for xs in DTYPES] + ['pw_head_kernel<%d, true>' % MT_F16] +
                 ['pw_narrow_kernel<%d, %d>' % (cin, xs) for cin in (30, 32) for xs in DTYPES])


# ---- head backward: mt_head_bwd
HB_N = [1, 2, 3, 1025]                             # 1025 exceeds HN_BLOCKS
HB_V = [33, 777, 2051, 4096]
HB_CIN = [8, 30, 32, 60, 64, 65]                   # 65 is refused
HB_COUT = [1, 2, 3, 4, 5, 47, 64, 65]
HB_DX = [MT_F32, MT_BF16]
STRIDE = ['dense', 'sliced', 'odd']                # C | C + 2 | odd
HB_MINOR = [STRIDE, STRIDE, STRIDE, SLOPES]        # x, dY, dX channel strides; lazy activation of x
HB_MINOR_DEFAULT = ('dense', 'dense', 'dense', None)
HB_EXTRA = []


def _stride(kind, c):
    return {'dense': c, 'sliced': c + 2, 'odd': (c + 1) | 1}[kind]


def hb_problem(major, minor):
    """(mt_src_t x, dycs, N, V, Cin, Cout, dxcs, dxdtype) of one head-backward row."""
    from multitalent_amd._lib import mt_src_t
    N, V, cin, cout, xdt, dxdt = major
    xcs, dycs, dxcs, slope = minor
    x = _src(mt_src_t(), 0, cin, xdt, slope, 'ok')
    x.cs = _stride(xcs, cin)
    return x, _stride(dycs, cout), N, V, cin, cout, _stride(dxcs, cin), dxdt


def hb_query(lib, x, dycs, N, V, cin, cout, dxcs, dxdt):
    buf, done = C.create_string_buffer(128), C.c_int(-1)
    rc = int(lib.mt_head_bwd_kernel_name(C.byref(x), dycs, N, V, cin, cout, dxcs, dxdt, buf, 128, C.byref(done)))
    return (buf.value.decode() if rc == 0 else '<rc %d>' % rc, rc, done.value, int(lib.mt_head_bwd_supported(cin, cout)),
            int(lib.mt_head_bwd_io_supported(x.dtype, x.cs, dxdt, dxcs, cin, cout)), int(lib.mt_head_bwd_workspace(N, V, cin, cout)))


HB = Table('hb_', [HB_N, HB_V, HB_CIN, HB_COUT, DTYPES, HB_DX], HB_MINOR, HB_MINOR_DEFAULT, HB_EXTRA,
           [('rc', 'int16'), ('dbias_done', 'int8'), ('supported', 'uint8'), ('io_supported', 'uint8'), ('workspace', 'int64')],
           ['head_bwd_kernel', 'head_bwd_narrow_kernel'], hb_problem, hb_query)
_HB_PAIRS = [(MT_F32, MT_F32), (MT_BF16, MT_BF16), (MT_F16, MT_BF16)]
HB_INSTANCES = (['head_bwd_kernel<%d, %d, %d, %s>' % ((nci,) + pr + (st,)) for nci in (1, 2) for pr in _HB_PAIRS for st in ('true', 'false')] +
                ['head_bwd_narrow_kernel<%d, %d, %d, %d>' % ((cin, nco) + pr) for cin in (30, 32) for nco in (2, 4) for pr in _HB_PAIRS])
