"""Shared by tests/test_bwdw_dispatch_cpu.py, tests/conv_dispatch_cases.py and tools/record_dispatch.py (not a test module).

The backward-weight dispatch table: which kernel `mt_conv3d_bwd_weight` takes for a problem, how much workspace the query asks for and
whether the storage types are served.  `cases()` yields the problems as (mt_conv3d_t, mt_src_t) pairs whose pointers are fake, non-null
addresses of chosen alignment — the three queries read the descriptors and never dereference them — and `query()` asks the library.

The problems are a thinned product of the axes below.  The MAJOR axes (geometry, channels, output size, batch, storage types, mma)
are crossed in full; every major row appears once with the MINOR axes (lazy activations, alignment, select word, max_workgroups) at
their defaults and once with a minor combination drawn by a fixed integer hash of the row number, so the table does not depend on any
random-number generator.  `EXTRA` adds rows for kernel names a uniform sample of the full product reaches but this thinning would miss.
"""
import ctypes as C
import itertools

import numpy as np

MT_F32, MT_BF16, MT_F16 = 0, 1, 2
SEL_OFF, SEL_FORCE = 1, 2
SEL_BWDW_WINO, SEL_BWDW_TR16, SEL_BWDW_CW = 8, 10, 12

# (K, S, P): the nine compile-time geometries of the tiled kernels (kBwGeos, same order) and one that matches none
GEOS = [((3, 3, 3), (1, 1, 1), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (1, 2, 2), (1, 1, 1)),
        ((2, 2, 2), (2, 2, 2), (0, 0, 0)), ((1, 2, 2), (1, 2, 2), (0, 0, 0)), ((1, 1, 1), (1, 1, 1), (0, 0, 0)),
        ((1, 3, 3), (1, 1, 1), (0, 1, 1)), ((1, 1, 1), (2, 2, 2), (0, 0, 0)), ((1, 1, 1), (1, 2, 2), (0, 0, 0)),
        ((3, 3, 1), (1, 1, 1), (1, 1, 0))]
CHANNELS = [((1,), 30), ((30,), 30), ((30, 30), 30), ((60,), 32), ((320,), 320), ((31,), 30)]      # (channels per X source, Cout)
SIZES = [(3, 6, 6), (6, 24, 24), (48, 192, 192), (2, 9, 20)]                                        # output (= dY) size
BATCH = [1, 2, 17]
DTYPES = [MT_F32, MT_BF16, MT_F16]
MMA = [0, 1]
MAJOR = [GEOS, CHANNELS, SIZES, BATCH, DTYPES, DTYPES, MMA]

LAZY_X = [None, 0.01, 1.5]                          # slope of a lazily activated X (scale / shift set), None = plain
LAZY_Y = [False, True]
ALIGN = ['ok', 'odd_cs', 'base4', 'base2']          # odd channel stride; base = 4 mod 8; base = 2 mod 4
SELECT = [0, SEL_OFF << SEL_BWDW_WINO, SEL_FORCE << SEL_BWDW_WINO, SEL_OFF << SEL_BWDW_TR16, SEL_FORCE << SEL_BWDW_TR16,
          1 << SEL_BWDW_CW, 2 << SEL_BWDW_CW, 3 << SEL_BWDW_CW]
MAX_WGS = [0, 3]
MINOR = [LAZY_X, LAZY_Y, ALIGN, ALIGN, SELECT, MAX_WGS]
MINOR_DEFAULT = (None, False, 'ok', 'ok', 0, 0)

FAMILIES = {'stem': 'conv_bwdw_stem_kernel', 'generic': 'conv_bwdw_kernel', 'gemm': 'bwdw_gemm_kernel', 'tr16': 'conv_bwdw_tr16_kernel',
            'wino': 'conv_bwdw_wino_kernel', 'march': 'conv_bwdw_march_kernel', 'march16': 'conv_bwdw_march16_kernel',
            'fast16': 'conv_bwdw_fast16_kernel', 'fast': 'conv_bwdw_fast_kernel'}


def family(name):
    """'conv_bwdw_fast_kernel<1, 1, 1, 1, 1, 1>' -> 'fast'"""
    stem = name.split('<')[0]
    for fam, kernel in FAMILIES.items():
        if stem == kernel:
            return fam
    return None


def _mix(i):
    """A fixed 32-bit integer hash (the finaliser of MurmurHash3)."""
    i &= 0xffffffff
    i ^= i >> 16
    i = (i * 0x85ebca6b) & 0xffffffff
    i ^= i >> 13
    i = (i * 0xc2b2ae35) & 0xffffffff
    return i ^ (i >> 16)


def _pick(axes, h):
    out = []
    for ax in axes:
        out.append(ax[h % len(ax)])
        h //= len(ax)
    return tuple(out)


def thinned(major_axes, minor_axes, minor_default, extra):
    """[(major, minor)]: the full product of the major axes, each row once with the default minor and once with a hash-drawn one."""
    out = []
    n_minor = 1
    for ax in minor_axes:
        n_minor *= len(ax)
    for i, major in enumerate(itertools.product(*major_axes)):
        out.append((major, minor_default))
        out.append((major, _pick(minor_axes, _mix(i) % n_minor)))
    out.extend(extra)
    return out


def census_rows(t, n):
    """n (major, minor) rows drawn by the fixed hash from the FULL product of the axes of a table t (tools/record_dispatch.py --census)."""
    axes = t.MAJOR + t.MINOR
    total = 1
    for ax in axes:
        total *= len(ax)
    for i in range(n):
        pick = _pick(axes, (_mix(i) * 0x100000000 + _mix(i + 0x9e3779b9)) % total)
        yield pick[:len(t.MAJOR)], pick[len(t.MAJOR):]


def _first_diff(rows, got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    if bad.size == 0:
        return None
    i = int(bad[0])
    return "%d rows differ; first is row %d %r: got %r, recorded %r" % (bad.size, i, rows[i], got[i], want[i])


# (major, minor) rows beyond the thinned product (see the module docstring)
EXTRA = []
PREFIX = ''                                                         # of this table's keys in its .npz
COLUMNS = [('workspace', 'int64'), ('io_supported', 'uint8')]       # what query() returns after the kernel name


def rows():
    """[(major, minor)] of the table, in its fixed order."""
    return thinned(MAJOR, MINOR, MINOR_DEFAULT, EXTRA)


_BASE = 0x7f0000000000          # fake device addresses, 256-byte aligned, never dereferenced
_ALIGN_OFF = {'ok': 0, 'odd_cs': 0, 'base4': 4, 'base2': 2}


def _src(s, slot, nch, dtype, lazy_slope, align):
    s.ptr = _BASE + slot * 0x10000000 + _ALIGN_OFF[align]
    s.C = nch
    s.cs = ((nch + 1) | 1) if align == 'odd_cs' else nch
    s.dtype = dtype
    s.slope = 0.0
    if lazy_slope is not None:
        s.scale, s.shift, s.slope = _BASE + 0x80000000 + slot * 0x1000, _BASE + 0x90000000 + slot * 0x1000, lazy_slope
    return s


def problem(major, minor):
    """The (mt_conv3d_t, mt_src_t) pair of one row."""
    from multitalent_amd._lib import mt_conv3d_t, mt_src_t
    (K, S, Pd), (cins, cout), (Do, Ho, Wo), N, xdt, ydt, mma = major
    lazy_x, lazy_y, align_x, align_y, select, max_wgs = minor
    p = mt_conv3d_t()
    p.nsrc = len(cins)
    for i, c in enumerate(cins):
        _src(p.src[i], i, c, xdt, lazy_x, align_x)
    p.N, p.Do, p.Ho, p.Wo = N, Do, Ho, Wo
    p.Di, p.Hi, p.Wi = [max(1, (o - 1) * s + k - 2 * q) for o, s, k, q in zip((Do, Ho, Wo), S, K, Pd)]
    p.dilD = p.dilH = p.dilW = 1
    p.KD, p.KH, p.KW = K
    p.SD, p.SH, p.SW = S
    p.PD, p.PH, p.PW = Pd
    p.Cin, p.Cout, p.csplit = sum(cins), cout, cout
    p.OD, p.OH, p.OW = Do, Ho, Wo
    p.osD = p.osH = p.osW = 1
    p.mma, p.select, p.max_workgroups = mma, select, max_wgs
    y = _src(mt_src_t(), 4, cout, ydt, 0.01 if lazy_y else None, align_y)
    return p, y


def cases():
    for major, minor in rows():
        yield problem(major, minor)


def query(lib, p, y):
    """(kernel name, workspace bytes, io_supported) of one problem; a failing name query reads '<rc N>'."""
    buf = C.create_string_buffer(128)
    rc = lib.mt_conv3d_bwd_weight_kernel_name(C.byref(p), C.byref(y), buf, 128)
    name = buf.value.decode() if rc == 0 else '<rc %d>' % rc
    return name, int(lib.mt_conv3d_bwd_weight_workspace(C.byref(p))), int(lib.mt_conv3d_bwd_weight_io_supported(C.byref(p), C.byref(y)))


def query_all(lib, pairs=None):
    """names (list of str), workspace (list of int), io (list of int) over `pairs` (default: the table's rows)."""
    names, ws, io = [], [], []
    for p, y in (cases() if pairs is None else pairs):
        n, w, s = query(lib, p, y)
        names.append(n), ws.append(w), io.append(s)
    return names, ws, io


def ask(lib, t):
    """names and {column: list} over the rows of a table t (this module, or a conv_dispatch_cases.Table): what tools/record_dispatch.py saves."""
    names, cols = [], {k: [] for k, _ in t.COLUMNS}
    for major, minor in t.rows():
        got = t.query(lib, *t.problem(major, minor))
        names.append(got[0])
        for (k, _), v in zip(t.COLUMNS, got[1:]):
            cols[k].append(v)
    return names, cols
