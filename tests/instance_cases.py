"""Shared by tests/test_instance_cases_cpu.py and tests/test_kernel_instances_gpu.py (not a test module).

Which problems run every kernel instance the five dispatch tables name (conv_dispatch_cases.FWD / BWDD, bwdw_dispatch_cases,
pw_dispatch_cases.FWD / HB) on real memory.  `cases(table)` lists (table, major, minor, expected_name): for every coverage key (kernel
name x the alignment axes of the table) the cheapest launchable row of the RECORDED table whose fp64 reference costs at most COST_CAP
multiply-adds, then the hand-written INSTANCE_EXTRA rows for instances no such row reaches.  UNLAUNCHABLE names instances every row of
which the library refuses to launch; UNREACHED names launchable instances with no problem under the cap.
"""
import os

import numpy as np

import bwdw_dispatch_cases as BC
import conv_dispatch_cases as CC
import pw_dispatch_cases as PC
from bwdw_dispatch_cases import MT_F32, MT_BF16, MT_F16

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# multiply-adds of the fp64 reference of one case: the largest case test_conv_fwd runs (2 x 16 -> 64 at 24 x 48 x 64, 3x3x3)
COST_CAP = 5 * 10 ** 9


class _Bwdw:
    """bwdw_dispatch_cases in the form of a conv_dispatch_cases.Table."""
    PREFIX, COLUMNS, MAJOR, MINOR, EXTRA = BC.PREFIX, BC.COLUMNS, BC.MAJOR, BC.MINOR, BC.EXTRA
    rows, problem, query = staticmethod(BC.rows), staticmethod(BC.problem), staticmethod(BC.query)


# table -> (Table, golden file)
TABLES = {'fwd': (CC.FWD, 'conv_dispatch.npz'), 'bwdd': (CC.BWDD, 'conv_dispatch.npz'), 'bwdw': (_Bwdw, 'bwdw_dispatch.npz'),
          'pw': (PC.FWD, 'pw_dispatch.npz'), 'hb': (PC.HB, 'pw_dispatch.npz')}
ORDER = ['fwd', 'bwdd', 'bwdw', 'pw', 'hb']


def _prod(v):
    out = 1
    for x in v:
        out *= int(x)
    return out


def cost(table, major, minor):
    """Multiply-adds of the reference: N Do Ho Wo Cin Cout KD KH KW (pointwise: voxels x taps x Cin x Cout)."""
    if table in ('fwd', 'bwdd'):
        (K, _, _, _, _), (cins, cout), out, N = major[:4]
        return N * _prod(out) * sum(cins) * cout * _prod(K)
    if table == 'bwdw':
        (K, _, _), (cins, cout), out, N = major[:4]
        return N * _prod(out) * sum(cins) * cout * _prod(K)
    if table == 'pw':
        (_, so, scatter, _), cin, cout = major[:3]
        return minor[8] * _prod(minor[0]) * (1 if scatter else _prod(so)) * cin * cout
    N, V, cin, cout = major[:4]
    return N * V * cin * cout


def recorded(table):
    """(rows, names, {column: array}) of the recorded table."""
    t, fname = TABLES[table]
    z = np.load(os.path.join(GOLDEN, fname))
    names = [str(n) for n in z[t.PREFIX + 'names'][z[t.PREFIX + 'name']]]
    return t.rows(), names, {k: z[t.PREFIX + k] for k, _ in t.COLUMNS}


def launches(table, cols, i, major, minor, name):
    """Whether the library launches row i of the recorded table: the *_io_supported / supported / rc columns, and what the launch
    requires beyond them (mt_conv3d_fwd: bstats only on a kernel that computes them; strided output placement only on conv_rt_kernel
    and without statistics)."""
    if name.startswith('<rc'):
        return False
    ok = bool(cols['io_supported'][i])
    if table == 'fwd' and minor[6]:
        ok = ok and bool(cols['bwd_stats_supported'][i])
    if table == 'fwd' and major[0][4]:
        ok = ok and name.startswith('conv_rt_kernel') and not minor[5] and not minor[6]
    if 'supported' in cols and table != 'hb':          # (mt_head_bwd_supported says where the fused kernel is FASTER, not where it launches)
        ok = ok and bool(cols['supported'][i])
    if 'rc' in cols:
        ok = ok and int(cols['rc'][i]) == 0
    return ok


def key(table, name, major, minor, cols, i):
    """The coverage key of a row: the instance and the alignment / stride axes its loads and stores depend on."""
    if table == 'fwd':
        return (name, minor[1], minor[2])
    if table == 'bwdd':
        return (name, minor[0])
    if table == 'bwdw':
        return (name, minor[2], minor[3])
    if table == 'pw':
        return (name, int(cols['wide'][i]), minor[1], minor[2], minor[3], minor[4])
    return (name, minor[0], minor[1], minor[2])


def valid_addresses(table, major, minor):
    """False for rows whose fake addresses are no valid addresses of the element type: a 2-byte base offset needs 16-bit storage."""
    if table == 'fwd':
        return (minor[1] != 'base2' or major[4] != MT_F32) and (minor[2] != 'base2' or major[5] != MT_F32)
    if table == 'bwdd':
        return minor[0] != 'base2' or major[4] != MT_F32
    if table == 'bwdw':
        return (minor[2] != 'base2' or major[4] != MT_F32) and (minor[3] != 'base2' or major[5] != MT_F32)
    if table == 'pw':
        return minor[4] != 2 or major[3] != MT_F32
    return True


# (table, major, minor, expected name): instances no launchable row of the recorded table under the cap reaches.  Found on the CPU by a
# seeded random search over the table's axes, widened by small channel counts (8, 16, 20, 32), small sizes and select words that force or
# exclude two families at once, asking the library with the table's own fwd_problem / fwd_query; the cheapest launchable hit per name.
INSTANCE_EXTRA = [
    ('fwd', (((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((16,), 30), (2, 4, 16), 1, 0, 0, 1), (None, 'ok', 'odd_cs', 24, 3, True, False, False), 'conv_bf16_kernel<16, 4, 2, 2, 1, 4, 1, 0, 0, 1>'),
    ('fwd', (((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((20,), 40), (3, 6, 6), 2, 1, 1, 1), (None, 'ok', 'ok', 8, 3, False, False, False), 'conv_bf16_kernel<16, 4, 2, 4, 1, 4, 1, 1, 1, 1>'),
    ('fwd', (((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((16,), 16), (2, 4, 16), 1, 2, 2, 1), (None, 'ok', 'ok', 24, 3, False, False, False), 'conv_bf16_kernel<16, 4, 2, 4, 1, 4, 1, 2, 2, 2>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((32,), 32), (2, 4, 16), 1, 1, 1, 1), (None, 'ok', 'ok', 8, 3, True, False, False), 'conv_bf16_kernel<16, 4, 2, 4, 1, 4, 3, 1, 1, 1>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((16,), 16), (2, 4, 16), 1, 2, 2, 1), (None, 'ok', 'ok', 8, 0, True, False, False), 'conv_bf16_kernel<16, 4, 2, 4, 1, 4, 3, 2, 2, 2>'),
    ('fwd', (((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((16,), 16), (2, 9, 20), 1, 0, 0, 1), (None, 'ok', 'ok', 8, 3, True, False, False), 'conv_bf16_kernel<32, 4, 2, 2, 1, 4, 1, 0, 0, 1>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((16,), 16), (2, 9, 20), 1, 0, 0, 1), (0.01, 'ok', 'ok', 8, 3, True, False, True), 'conv_bf16_kernel<32, 4, 2, 2, 1, 4, 3, 0, 0, 1>'),
    ('fwd', (((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((32,), 32), (2, 9, 20), 1, 1, 1, 1), (0.01, 'ok', 'ok', 40, 0, False, False, False), 'conv_bf16_kernel<32, 4, 2, 4, 1, 4, 1, 1, 1, 1>'),
    ('fwd', (((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((16,), 16), (2, 9, 20), 1, 2, 2, 1), (0.01, 'ok', 'ok', 8, 3, True, False, True), 'conv_bf16_kernel<32, 4, 2, 4, 1, 4, 1, 2, 2, 2>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((32,), 64), (2, 9, 20), 1, 1, 1, 1), (0.01, 'ok', 'ok', 8, 3, True, False, True), 'conv_bf16_kernel<32, 4, 2, 4, 1, 4, 3, 1, 1, 1>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((16,), 16), (2, 9, 20), 2, 2, 2, 1), (0.01, 'ok', 'ok', 24, 0, True, False, False), 'conv_bf16_kernel<32, 4, 2, 4, 1, 4, 3, 2, 2, 2>'),
    ('fwd', (((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((16,), 16), (4, 8, 32), 1, 0, 0, 1), (0.01, 'ok', 'ok', 24, 3, True, False, True), 'conv_bf16_kernel<32, 4, 4, 2, 1, 4, 1, 0, 0, 1>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((16,), 16), (4, 8, 32), 2, 0, 0, 1), (None, 'ok', 'ok', 24, 3, False, False, False), 'conv_bf16_kernel<32, 4, 4, 2, 1, 4, 3, 0, 0, 1>'),
    ('fwd', (((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((16, 16), 32), (4, 16, 32), 1, 1, 1, 1), (0.01, 'ok', 'ok', 24, 0, False, False, False), 'conv_bf16_kernel<32, 4, 4, 4, 1, 4, 1, 1, 1, 1>'),
    ('fwd', (((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((32,), 64), (4, 8, 32), 1, 2, 2, 1), (None, 'ok', 'ok', 24, 3, True, False, False), 'conv_bf16_kernel<32, 4, 4, 4, 1, 4, 1, 2, 2, 2>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((16, 16), 32), (4, 8, 32), 1, 1, 1, 1), (None, 'ok', 'ok', 8, 0, False, False, True), 'conv_bf16_kernel<32, 4, 4, 4, 1, 4, 3, 1, 1, 1>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((16,), 30), (4, 8, 32), 2, 2, 2, 1), (None, 'ok', 'ok', 24, 3, False, False, False), 'conv_bf16_kernel<32, 4, 4, 4, 1, 4, 3, 2, 2, 2>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((8,), 8), (2, 4, 16), 1, 0, 0, 0), (0.01, 'ok', 'base4', 32, 0, True, False, True), 'conv_fast_kernel<16, 2, 2, 2, 3>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((8,), 8), (1, 8, 32), 1, 0, 0, 1), (None, 'ok', 'ok', 66, 3, True, False, False), 'conv_fast_kernel<32, 4, 2, 2, 3>'),
    ('fwd', (((3, 3, 3), (1, 2, 2), (1, 1, 1), 1, False), ((16,), 16), (2, 9, 20), 1, 1, 0, 1), (None, 'ok', 'ok', 65, 0, False, False, False), 'conv_fast_strided_kernel<1, 2, 2, 4, true, 1, 0, 1>'),
    ('fwd', (((3, 3, 3), (1, 2, 2), (1, 1, 1), 1, False), ((16, 16), 32), (3, 6, 6), 1, 1, 1, 1), (None, 'ok', 'ok', 65, 0, False, False, False), 'conv_fast_strided_kernel<1, 2, 2, 4, true, 1, 1, 1>'),
    ('fwd', (((3, 3, 3), (1, 2, 2), (1, 1, 1), 1, False), ((32,), 32), (2, 4, 16), 1, 2, 0, 1), (None, 'ok', 'ok', 66, 3, True, False, False), 'conv_fast_strided_kernel<1, 2, 2, 4, true, 2, 0, 2>'),
    ('fwd', (((3, 3, 3), (1, 2, 2), (1, 1, 1), 1, False), ((16,), 16), (2, 4, 16), 2, 2, 2, 1), (0.01, 'ok', 'ok', 64, 3, False, False, False), 'conv_fast_strided_kernel<1, 2, 2, 4, true, 2, 2, 2>'),
    ('fwd', (((3, 3, 3), (2, 2, 2), (1, 1, 1), 1, False), ((8,), 8), (2, 4, 16), 1, 0, 0, 0), (None, 'ok', 'ok', 66, 3, False, False, False), 'conv_fast_strided_kernel<2, 2, 2, 2, false, 0, 0, 1>'),
    ('fwd', (((3, 3, 3), (2, 2, 2), (1, 1, 1), 1, False), ((16,), 64), (3, 6, 6), 1, 1, 0, 1), (0.01, 'ok', 'ok', 66, 0, True, False, False), 'conv_fast_strided_kernel<2, 2, 2, 4, true, 1, 0, 1>'),
    ('fwd', (((3, 3, 3), (2, 2, 2), (1, 1, 1), 1, False), ((16,), 16), (2, 9, 20), 1, 1, 1, 1), (0.01, 'ok', 'ok', 65, 0, True, False, False), 'conv_fast_strided_kernel<2, 2, 2, 4, true, 1, 1, 1>'),
    ('fwd', (((3, 3, 3), (2, 2, 2), (1, 1, 1), 1, False), ((16,), 16), (3, 6, 6), 1, 2, 0, 1), (0.01, 'ok', 'ok', 66, 3, True, False, False), 'conv_fast_strided_kernel<2, 2, 2, 4, true, 2, 0, 2>'),
    ('fwd', (((3, 3, 3), (2, 2, 2), (1, 1, 1), 1, False), ((30,), 30), (3, 6, 6), 1, 2, 2, 1), (0.01, 'ok', 'ok', 65, 0, True, False, False), 'conv_fast_strided_kernel<2, 2, 2, 4, true, 2, 2, 2>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((16,), 16), (3, 6, 6), 1, 0, 0, 0), (0.01, 'ok', 'ok', 2, 0, True, False, True), 'conv_wino8p_kernel'),
    ('fwd', (((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((16,), 16), (4, 16, 32), 2, 1, 1, 1), (None, 'ok', 'ok', 40, 3, False, False, False), 'conv_x16_kernel<1, 1>'),
    ('fwd', (((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((16,), 16), (8, 16, 64), 1, 2, 2, 1), (0.01, 'ok', 'ok', 40, 3, False, False, False), 'conv_x16_kernel<1, 2>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((16, 16), 32), (4, 8, 32), 1, 1, 1, 1), (0.01, 'ok', 'ok', 8, 3, True, False, False), 'conv_x16_kernel<3, 1>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((20,), 40), (4, 16, 32), 1, 2, 2, 1), (None, 'ok', 'ok', 40, 3, True, False, False), 'conv_x16_kernel<3, 2>'),
    # rows of the recorded table reach these only with bstats set on a kernel that refuses it
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((16,), 16), (1, 8, 32), 1, 0, 0, 1), (0.01, 'ok', 'ok', 8, 0, False, False, False), 'conv_bf16_kernel<16, 4, 2, 2, 1, 4, 3, 0, 0, 1>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((1,), 30), (2, 4, 16), 1, 0, 0, 0), (None, 'ok', 'ok', 8, 3, True, False, True), 'conv_fast_kernel<16, 2, 2, 1, 3>'),
    ('fwd', (((1, 3, 3), (1, 1, 1), (0, 1, 1), 1, False), ((8,), 8), (2, 4, 16), 1, 0, 0, 1), (0.01, 'ok', 'ok', 65, 0, False, False, False), 'conv_fast_kernel<16, 2, 2, 2, 1>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((1,), 30), (1, 8, 32), 1, 0, 0, 1), (0.01, 'ok', 'odd_cs', 2, 0, False, False, True), 'conv_fast_kernel<32, 4, 2, 1, 3>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 1, False), ((8,), 8), (3, 6, 6), 1, 0, 0, 1), (0.01, 'ok', 'ok', 128, 3, True, False, True), 'conv_fast_kernel<8, 2, 2, 2, 3>'),
    ('fwd', (((3, 3, 3), (1, 1, 1), (1, 1, 1), 2, False), ((1,), 30), (2, 4, 16), 1, 0, 0, 1), (None, 'ok', 'ok', 2, 0, False, False, True), 'conv_fwd_kernel<16, 2, 2, 16, false>'),
]
_GATHER16 = 'conv_io_served refuses fp16 on either side of conv_gather_kernel, and a 16-bit destination whose pairs are not aligned'
# table -> {name: reason}: every row of the recorded table that carries the name has io_supported == 0
UNLAUNCHABLE = {
    'fwd': {'conv_gather_kernel<4, 0, 2>': _GATHER16, 'conv_gather_kernel<4, 1, 2>': _GATHER16, 'conv_gather_kernel<4, 1, 2, true>': _GATHER16,
            'conv_gather_kernel<4, 2, 0>': _GATHER16, 'conv_gather_kernel<4, 2, 1>': _GATHER16, 'conv_gather_kernel<4, 2, 2>': _GATHER16,
            'conv_fwd_kernel<8, 2, 2, 16, true>': 'mt_conv3d_fwd refuses strided output placement on every kernel but conv_rt_kernel',
            # (3x3x3 stride 1 pad 1 reaches the generic kernel only with strided output placement: without it conv_fast_kernel or a
            # specialised kernel always serves it)
            },
    'bwdd': {},
    # the name carries dY's type; mt_conv3d_bwd_weight_io_supported takes the stem kernel with an fp32 or bf16 gradient only
    'bwdw': {'conv_bwdw_stem_kernel<2>': 'the stem kernel is instantiated for fp32 and bf16 dY; an fp16 dY is refused before the launch'},
    'pw': {}, 'hb': {}}
# table -> {name: (major, minor, multiply-adds)}: launchable, the smallest problem known is above the cap (at most two per table)
UNREACHED = {
    'fwd': {'conv_fwd_kernel<16, 2, 2, 8, false>': ((CC.GEOS[2], ((60,), 32), (48, 192, 192), 1, MT_F32, MT_F32, 0), CC.FWD_MINOR_DEFAULT, 91729428480)},
    'bwdd': {}, 'bwdw': {}, 'pw': {}, 'hb': {}}

_cache = {}


def cases(table):
    """[(table, major, minor, expected_name)]: one per coverage key, cheapest first-seen row, then this table's INSTANCE_EXTRA."""
    if table in _cache:
        return _cache[table]
    rows, names, cols = recorded(table)
    best = {}
    for i, ((major, minor), name) in enumerate(zip(rows, names)):
        if not launches(table, cols, i, major, minor, name) or not valid_addresses(table, major, minor):
            continue
        c = cost(table, major, minor)
        if c > COST_CAP:
            continue
        k = key(table, name, major, minor, cols, i)
        if k not in best or c < best[k][0]:
            best[k] = (c, i)
    out = [(table,) + rows[i] + (names[i],) for _, i in sorted(best.values(), key=lambda ci: ci[1])]
    out += [c for c in INSTANCE_EXTRA if c[0] == table]
    _cache[table] = out
    return out


def case_id(case):
    table, major, minor, name = case
    return '%s-%s-%s' % (name.replace(' ', ''), '_'.join(str(a) for a in _flat(major)), '_'.join(str(a) for a in _flat(minor)))


def _flat(v):
    for a in v:
        if isinstance(a, (tuple, list)):
            for b in _flat(a):
                yield b
        else:
            yield a


# ---- real memory ---------------------------------------------------------------------------------------------------------------------
# Everything below needs torch (and, to launch, a device); the selection above does not.
_PATTERN = -123.456          # prefill of destination neighbours and of the gaps of the placed form (compared as bits)
_BIG = {MT_F32: 1e30, MT_BF16: 1e30, MT_F16: 65504.0}          # source neighbours: large and finite, a leaked read is a gross error
_ROUND = {MT_BF16: 2.0 ** -9, MT_F16: 2.0 ** -12}              # one store to a 16-bit destination (store_rounding)


def _tdt(dt):
    import torch
    return {MT_F32: torch.float32, MT_BF16: torch.bfloat16, MT_F16: torch.float16}[dt]


def _bits(t):
    import torch
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


class Slab:
    """`rows` x `C` channel slice (row stride `cs` elements, first byte at `off` modulo 16) of a wider, 256-byte-aligned allocation the
    test owns.  written: the rows a launch may write (None = all): the placed form and the scatter write a subset."""

    def __init__(self, rows, C, cs, dt, off=0, written=None):
        import torch
        self.dtype = _tdt(dt)
        self.es = 4 if dt == MT_F32 else 2
        assert off % self.es == 0 and cs >= C
        self.front = (256 + off) // self.es
        self.rows, self.C, self.cs, self.written = rows, C, cs, written
        self.n = self.front + rows * cs + 256 // self.es
        self.host = torch.empty(self.n, dtype=self.dtype)
        self.dev = None

    def view(self, t):
        return t.as_strided((self.rows, self.C), (self.cs, 1), self.front)

    def mask(self):
        import torch
        m = torch.zeros(self.n, dtype=torch.bool)
        if self.written is None:
            self.view(m)[:] = True
        else:
            self.view(m)[self.written] = True
        return m

    def fill(self, outside, inside):
        """inside: a [rows (written), C] tensor, or a scalar"""
        self.host.fill_(outside)
        if self.written is None:
            self.view(self.host)[:] = inside
        else:
            self.view(self.host)[self.written] = inside
        return self

    def upload(self, dev):
        self.dev = self.host.to(dev)
        assert self.dev.data_ptr() % 256 == 0 or not self.dev.is_cuda
        return self.dev.data_ptr() + self.front * self.es

    def values(self, t=None):
        """[rows (written), C] float64 of the slice of t (default: the prefill)"""
        v = self.view(self.host if t is None else t)
        return (v if self.written is None else v[self.written]).double()


def _source(g, rows, C, cs, dt, off, amp=1.0):
    import torch
    return Slab(rows, C, cs, dt, off).fill(_BIG[dt], (amp * torch.randn((rows, C), generator=g)).to(_tdt(dt)))


def _dest(g, rows, C, cs, dt, off, accumulate=False, written=None):
    import torch
    s = Slab(rows, C, cs, dt, off, written)
    n = rows if written is None else len(written)
    return s.fill(_PATTERN, torch.randn((n, C), generator=g).to(_tdt(dt)) if accumulate else float('nan'))


def _lazy(g, N, C, slope):
    """(scale slab, shift slab) [N][C] of a lazily activated operand, or None; their neighbours are the identity (1, 0)"""
    import torch
    if slope is None:
        return None
    return (Slab(N, C, C, MT_F32).fill(1.0, torch.rand((N, C), generator=g) + 0.5), Slab(N, C, C, MT_F32).fill(0.0, 0.3 * torch.randn((N, C), generator=g)))


def _activated(slab, lazy, slope, N):
    """[N, V, C] float64 of an operand as the kernels stage it: widened exactly, the lazy activation lrelu(x scale + shift) in fp32 (one fma)"""
    import torch
    x = slab.values().reshape(N, -1, slab.C)
    if lazy is None:
        return x
    sc, sh = lazy[0].values()[:, None, :], lazy[1].values()[:, None, :]
    t = (x * sc + sh).float()                    # the fp64 sum rounded once = the fma
    return torch.where(t > 0, t, t * torch.tensor(slope, dtype=torch.float32)).double()


def _rnd(x, dt):
    """float64 x rounded to the product type dt (None: exact)"""
    return x if dt is None else x.float().to(_tdt(dt)).double()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from multitalent_amd import _lib as L
    return L


def _pack(w, C0, C1, Cout, K, strides, ck, layout):
    from multitalent_amd import ops
    return ops.pack_conv_weights(w, C0, C1, Cout, K, strides, False, ck, layout=layout)


def _placed_rows(N, O, o, stride, offset):
    """row indices of the logical positions `o` written at o * stride + offset of a stored volume O, all N samples"""
    import torch
    idx = [torch.arange(n) * s + off for n, s, off in zip(o, stride, offset)]
    r = (idx[0][:, None, None] * O[1] + idx[1][None, :, None]) * O[2] + idx[2][None, None, :]
    return (torch.arange(N)[:, None] * (O[0] * O[1] * O[2]) + r.reshape(1, -1)).reshape(-1)


def materialise(table, major, minor, dev, seed):
    """The struct(s) the table's problem() builds with every fake address replaced by device memory this call owns (offsets modulo 16
    bytes, channel strides and storage types kept) and seeded contents.  Returns the dict launch(), reference() and check() take."""
    import torch
    g = torch.Generator().manual_seed(1000 + seed)
    return {'fwd': _mat_fwd, 'bwdd': _mat_bwdd, 'bwdw': _mat_bwdw, 'pw': _mat_pw, 'hb': _mat_hb}[table](major, minor, dev, g, seed)


def _conv_sources(p, n, N, V, dev, g, lazy_slope, T):
    T['src'], T['lazy'] = [], []
    for i in range(n):
        s = p.src[i]
        slab = _source(g, N * V, s.C, s.cs, s.dtype, s.ptr % 16)
        s.ptr = slab.upload(dev)
        lz = _lazy(g, N, s.C, lazy_slope)
        if lz is not None:
            s.scale, s.shift = lz[0].upload(dev), lz[1].upload(dev)
        T['src'].append(slab)
        T['lazy'].append(lz)


def _mat_fwd(major, minor, dev, g, seed):
    import ctypes as C
    import torch
    L = _lib()
    lib = L.load()
    (p,) = CC.fwd_problem(major, minor)
    (K, S, Pd, dil, placed), (cins, cout), out, N, xdt, odt, mma = major
    lazy, _, _, _, _, stats, bstats, split = minor
    T = {'p': p, 'slope': lazy, 'N': N}
    _conv_sources(p, len(cins), N, p.Di * p.Hi * p.Wi, dev, g, lazy, T)
    O = (p.OD, p.OH, p.OW)
    written = _placed_rows(N, O, out, (2, 2, 2), (1, 1, 1)) if placed else None
    rows = N * O[0] * O[1] * O[2]
    T['dst'] = {}
    d0 = _dest(g, rows, p.csplit, p.ocs0, odt, p.out0 % 16, bool(p.accumulate), written)
    p.out0 = d0.upload(dev)
    T['dst']['out0'] = d0
    if split:
        d1 = _dest(g, rows, cout - p.csplit, p.ocs1, odt, p.out1 % 16, bool(p.accumulate), written)
        p.out1 = d1.upload(dev)
        T['dst']['out1'] = d1
    T['bias'] = Slab(1, cout, cout, MT_F32).fill(1e30, torch.randn((1, cout), generator=g))
    p.bias = T['bias'].upload(dev)
    if bstats:
        b = p.bstats
        V = out[0] * out[1] * out[2]
        T['by'] = _source(g, N * V, b.C, b.ycs, MT_F32, 0)
        T['bmean'] = Slab(N, b.C, b.C, MT_F32).fill(0.0, 0.5 * torch.randn((N, b.C), generator=g))
        T['brstd'] = Slab(N, b.C, b.C, MT_F32).fill(1.0, torch.rand((N, b.C), generator=g) + 0.5)
        b.y, b.mean, b.rstd = T['by'].upload(dev), T['bmean'].upload(dev), T['brstd'].upload(dev)
    r = C.byref(p)
    T['layout'], ck = int(lib.mt_conv3d_pack_layout(r)), int(lib.mt_conv3d_ck(r))
    cin = sum(cins)
    T['w'] = torch.randn((cout, cin) + tuple(K), generator=g) / float(np.sqrt(cin * _prod(K)))
    from multitalent_amd import ops
    wd = T['w'].to(dev).contiguous()
    T['wpack'] = _pack(wd, cins[0], cins[1] if len(cins) > 1 else 0, cout, K, ops.conv_weight_strides(wd), ck, T['layout'])
    p.wpack = T['wpack'].data_ptr()
    if stats or bstats:
        nsb = int(lib.mt_conv3d_stats_blocks(r))
        T['nsb'] = nsb
        T['dst']['stats'] = Slab(N * nsb, 2 * cout, 2 * cout, MT_F32).fill(_PATTERN, float('nan'))
        p.stats_part = T['dst']['stats'].upload(dev)
    T['bstats_served'] = bool(bstats) and bool(lib.mt_conv3d_bwd_stats_supported(r))
    T['name'] = CC._name(lib.mt_conv3d_kernel_name, p)
    T['launches'] = bool(lib.mt_conv3d_io_supported(r)) and (not bstats or T['bstats_served']) and (
        not placed or (T['name'].startswith('conv_rt_kernel') and not stats and not bstats))
    return T


def _mat_bwdd(major, minor, dev, g, seed):
    import ctypes as C
    import torch
    lib = _lib().load()
    (p,) = CC.bwdd_problem(major, minor)
    (K, S, Pd, dil, _), (cins, cout), out, N, ydt, xdt, mma = major
    cin = sum(cins)
    T = {'p': p, 'slope': None, 'N': N}
    _conv_sources(p, 1, N, _prod(out), dev, g, None, T)
    d0 = _dest(g, N * p.Di * p.Hi * p.Wi, cin, p.ocs0, xdt, p.out0 % 16)
    p.out0 = d0.upload(dev)
    T['dst'] = {'out0': d0}
    r = C.byref(p)
    T['layout'] = int(lib.mt_conv3d_bwd_data_strided_pack_layout(r))
    T['w'] = torch.randn((cout, cin) + tuple(K), generator=g) / float(np.sqrt(cin * _prod(K)))
    from multitalent_amd import ops
    wd = T['w'].to(dev).contiguous()
    T['wpack'] = _pack(wd, cout, 0, cin, K, ops.conv_weight_strides(wd, as_bwd_data=True), 16, T['layout'])
    p.wpack = T['wpack'].data_ptr()
    T['name'] = CC._name(lib.mt_conv3d_bwd_data_strided_kernel_name, p)
    T['launches'] = bool(lib.mt_conv3d_bwd_data_strided_supported(r)) and bool(lib.mt_conv3d_bwd_data_strided_io_supported(r))
    return T


def _mat_bwdw(major, minor, dev, g, seed):
    import ctypes as C
    import torch
    lib = _lib().load()
    p, y = BC.problem(major, minor)
    (K, S, Pd), (cins, cout), out, N, xdt, ydt, mma = major
    lazy_x, lazy_y = minor[0], minor[1]
    T = {'p': p, 'y': y, 'slope': lazy_x, 'yslope': 0.01 if lazy_y else None, 'N': N}
    _conv_sources(p, len(cins), N, p.Di * p.Hi * p.Wi, dev, g, lazy_x, T)
    T['ysrc'] = _source(g, N * _prod(out), cout, y.cs, ydt, y.ptr % 16)
    y.ptr = T['ysrc'].upload(dev)
    T['ylazy'] = _lazy(g, N, cout, T['yslope'])
    if T['ylazy'] is not None:
        y.scale, y.shift = T['ylazy'][0].upload(dev), T['ylazy'][1].upload(dev)
    cin = sum(cins)
    T['accumulate'] = seed % 3 == 1
    T['dst'] = {'dw': _dest(g, 1, cout * cin * _prod(K), cout * cin * _prod(K), MT_F32, 0, T['accumulate'])}
    T['dwptr'] = T['dst']['dw'].upload(dev)
    T['ws_bytes'] = int(lib.mt_conv3d_bwd_weight_workspace(C.byref(p)))
    T['ws'] = torch.empty(T['ws_bytes'] // 4 + 16, device=dev)
    T['name'] = BC.query(lib, p, y)[0]
    T['launches'] = bool(lib.mt_conv3d_bwd_weight_io_supported(C.byref(p), C.byref(y)))
    return T


def _mat_pw(major, minor, dev, g, seed):
    import ctypes as C
    import torch
    lib = _lib().load()
    (p,) = PC.fwd_problem(major, minor)
    (si, so, scatter, bigger), cin, cout, xdt, odt, mma = major
    base, _, _, _, _, slope, accumulate, stats, N = minor
    T = {'p': p, 'slope': slope, 'N': N}
    s = p.src
    T['src'] = [_source(g, N * p.Di * p.Hi * p.Wi, cin, s.cs, xdt, s.ptr % 16)]
    s.ptr = T['src'][0].upload(dev)
    T['lazy'] = [_lazy(g, N, cin, slope)]
    if slope is not None:
        s.scale, s.shift = T['lazy'][0][0].upload(dev), T['lazy'][0][1].upload(dev)
    O = tuple(b * t for b, t in zip(base, so))
    written = _placed_rows(N, O, base, so, (0, 0, 0)) if scatter else None
    d = _dest(g, N * _prod(O), cout, p.ocs, odt, p.out % 16, bool(accumulate), written)
    p.out = d.upload(dev)
    T['dst'] = {'out': d}
    T['bias'] = Slab(1, cout, cout, MT_F32).fill(1e30, torch.randn((1, cout), generator=g))
    p.bias = T['bias'].upload(dev)
    r = C.byref(p)
    T['layout'] = int(lib.mt_pointwise_pack_layout(r))
    taps = (1, 1, 1) if scatter else tuple(so)
    T['w'] = torch.randn((cin, cout) + taps, generator=g) / float(np.sqrt(cin))          # nn.ConvTranspose3d layout
    from multitalent_amd import ops
    wd = T['w'].to(dev).contiguous()
    T['wpack'] = _pack(wd, cin, 0, cout, taps, ops.conv_weight_strides(wd, transposed_layout=True), ops.POINTWISE_CK, T['layout'])
    p.wpack = T['wpack'].data_ptr()
    if stats:
        nsb = int(lib.mt_pointwise_stats_blocks(r))
        T['nsb'] = nsb
        T['dst']['stats'] = Slab(N * nsb, 2 * cout, 2 * cout, MT_F32).fill(_PATTERN, float('nan'))
        p.stats_part = T['dst']['stats'].upload(dev)
    q = PC.fwd_query(lib, p)
    T['name'], T['wide'] = q[0], q[5]
    T['launches'] = q[1] == 0 and bool(q[7])
    return T


def _mat_hb(major, minor, dev, g, seed):
    import ctypes as C
    import torch
    lib = _lib().load()
    x, dycs, N, V, cin, cout, dxcs, dxdt = PC.hb_problem(major, minor)
    slope = minor[3]
    T = {'x': x, 'slope': slope, 'N': N, 'args': (dycs, N, V, cin, cout, dxcs, dxdt)}
    T['src'] = [_source(g, N * V, cin, x.cs, x.dtype, 0)]
    x.ptr = T['src'][0].upload(dev)
    T['lazy'] = [_lazy(g, N, cin, slope)]
    if slope is not None:
        x.scale, x.shift = T['lazy'][0][0].upload(dev), T['lazy'][0][1].upload(dev)
    T['dy'] = _source(g, N * V, cout, dycs, MT_F32, 0)
    T['dyptr'] = T['dy'].upload(dev)
    T['acc_dx'], T['acc_dw'] = seed % 2 == 1, seed % 3 == 1
    T['dst'] = {'dx': _dest(g, N * V, cin, dxcs, dxdt, 0, T['acc_dx']),
                'dw': _dest(g, 1, cout * cin, cout * cin, MT_F32, 0, T['acc_dw']),
                'dbias': _dest(g, 1, cout, cout, MT_F32, 0, T['acc_dw'])}
    T['dxptr'], T['dwptr'], T['dbptr'] = [T['dst'][k].upload(dev) for k in ('dx', 'dw', 'dbias')]
    T['w'] = torch.randn((cout, cin, 1, 1, 1), generator=g) / float(np.sqrt(cin))
    from multitalent_amd import ops
    wd = T['w'].to(dev).contiguous()
    T['wpack'] = _pack(wd, cout, 0, cin, (1, 1, 1), ops.conv_weight_strides(wd, as_bwd_data=True), ops.POINTWISE_CK, 1)
    T['ws_bytes'] = int(lib.mt_head_bwd_workspace(N, V, cin, cout))
    T['ws'] = torch.empty(T['ws_bytes'] // 4 + 16, device=dev)
    q = PC.hb_query(lib, x, dycs, N, V, cin, cout, dxcs, dxdt)
    T['name'], T['dbias_done'] = q[0], q[2]
    T['launches'] = q[1] == 0 and bool(q[4])
    return T


def launch(table, T):
    """The launch through the C ABI, synchronised."""
    import ctypes as C
    import torch
    L = _lib()
    lib = L.load()
    st = _stream()
    if table == 'fwd':
        L.check(lib.mt_conv3d_fwd(C.byref(T['p']), st), 'conv3d_fwd')
    elif table == 'bwdd':
        L.check(lib.mt_conv3d_bwd_data_strided(C.byref(T['p']), st), 'conv3d_bwd_data_strided')
    elif table == 'bwdw':
        p = T['p']
        k3, kk = p.KD * p.KH * p.KW, p.KH * p.KW
        L.check(lib.mt_conv3d_bwd_weight(C.byref(p), C.byref(T['y']), T['dwptr'], k3, p.Cin * k3, kk, p.KW, 1, int(T['accumulate']),
                                         T['ws'].data_ptr(), T['ws_bytes'], st), 'conv3d_bwd_weight')
    elif table == 'pw':
        L.check(lib.mt_pointwise_fwd(C.byref(T['p']), st), 'pointwise_fwd')
    else:
        dycs, N, V, cin, cout, dxcs, dxdt = T['args']
        done = C.c_int(-1)
        L.check(lib.mt_head_bwd(C.byref(T['x']), T['dyptr'], dycs, N, V, cin, cout, T['wpack'].data_ptr(), T['dxptr'], dxcs, dxdt, int(T['acc_dx']),
                                T['dwptr'], 1, cin, T['dbptr'], int(T['acc_dw']), C.byref(done), T['ws'].data_ptr(), T['ws_bytes'], st), 'head_bwd')
        T['done'] = done.value
    torch.cuda.synchronize()


# ---- fp64 references -------------------------------------------------------------------------------------------------------------------
_PRODUCT = {1: None, 0: None, 2: None, 3: MT_BF16, 4: MT_F16}                       # pack layout -> type the instance multiplies in
_BWDW_BF16 = ('bwdw_gemm_kernel', 'conv_bwdw_tr16_kernel', 'conv_bwdw_march16_kernel', 'conv_bwdw_fast16_kernel')


def product_type(table, T):
    """The 16-bit type the instance rounds its matrix operands to, or None (fp32 products)."""
    if table == 'bwdw':
        return MT_BF16 if T['name'].split('<')[0] in _BWDW_BF16 else None
    if table == 'hb':
        return None
    return _PRODUCT[T['layout']]


def _ncdhw(x, N, dims):
    return x.reshape((N,) + tuple(dims) + (x.shape[-1],)).permute(0, 4, 1, 2, 3).contiguous()


def _rows(y):
    """NCDHW -> [N V, C]"""
    return y.permute(0, 2, 3, 4, 1).reshape(-1, y.shape[1])


def _conv_input(T, pt, dims):
    import torch
    N = T['N']
    return torch.cat([_ncdhw(_rnd(_activated(s, lz, T['slope'], N), pt), N, dims) for s, lz in zip(T['src'], T['lazy'])], 1)


def _stored(ref, slab):
    """ref + the prior contents of an accumulating destination"""
    prior = slab.values()
    return ref if bool(prior.isnan().all()) else ref + prior


def reference(table, major, minor, T):
    """{destination: [rows, C] float64} of the case, plain torch on the CPU in float64 (see the module docstring of the GPU test)."""
    import torch
    import torch.nn.functional as F
    pt = product_type(table, T)
    N = T['N']
    R = {}
    if table == 'fwd':
        p = T['p']
        (K, S, Pd, dil, placed), (cins, cout), out = major[:3]
        x = _conv_input(T, pt, (p.Di, p.Hi, p.Wi))
        need = [(o - 1) * s + k - 2 * q for o, s, k, q in zip(out, S, K, Pd)]          # extent of the (zero-inserted) virtual input
        xv = torch.zeros((N, x.shape[1]) + tuple(need), dtype=torch.float64)
        cnt = [min(d, (n - 1) // dil + 1) for n, d in zip(need, (p.Di, p.Hi, p.Wi))]          # stored samples inside the virtual extent
        xv[:, :, :(cnt[0] - 1) * dil + 1:dil, :(cnt[1] - 1) * dil + 1:dil, :(cnt[2] - 1) * dil + 1:dil] = x[:, :, :cnt[0], :cnt[1], :cnt[2]]
        y = F.conv3d(xv, _rnd(T['w'].double(), pt), T['bias'].values().reshape(-1), stride=S, padding=Pd)
        assert tuple(y.shape[2:]) == tuple(out), (y.shape, out)
        y = _rows(y)
        R['out0'] = _stored(y[:, :p.csplit], T['dst']['out0'])
        if 'out1' in T['dst']:
            R['out1'] = _stored(y[:, p.csplit:], T['dst']['out1'])
    elif table == 'bwdd':
        p = T['p']
        (K, S, Pd, dil, _), (cins, cout), out = major[:3]
        dy = _conv_input(T, pt, out)
        dx = F.conv_transpose3d(dy, _rnd(T['w'].double(), pt), None, stride=S, padding=Pd)
        assert tuple(dx.shape[2:]) == (p.Di, p.Hi, p.Wi), dx.shape
        R['out0'] = _rows(dx)
    elif table == 'bwdw':
        p = T['p']
        (K, S, Pd), (cins, cout), out = major[:3]
        x = _conv_input(T, pt, (p.Di, p.Hi, p.Wi))
        dy = _ncdhw(_rnd(_activated(T['ysrc'], T['ylazy'], T['yslope'], N), pt), N, out)
        w = torch.zeros((cout, sum(cins)) + tuple(K), dtype=torch.float64, requires_grad=True)
        F.conv3d(x, w, None, stride=S, padding=Pd).backward(dy)
        R['dw'] = _stored(w.grad.reshape(1, -1), T['dst']['dw'])
    elif table == 'pw':
        p = T['p']
        (si, so, scatter, bigger), cin, cout = major[:3]
        base = minor[0]
        a = _rnd(_activated(T['src'][0], T['lazy'][0], T['slope'], N), pt).reshape(N, p.Di, p.Hi, p.Wi, cin)
        a = a[:, ::si[0], ::si[1], ::si[2]][:, :base[0], :base[1], :base[2]]
        w = _rnd(T['w'].double(), pt)
        y = torch.einsum('ndhwi,ioabc->ndahbwco', a, w) + T['bias'].values().reshape(-1)
        kd, kh, kw = w.shape[2:]
        y = y.reshape(N * base[0] * kd * base[1] * kh * base[2] * kw, cout)             # scatter: one tap, the written rows in order
        R['out'] = _stored(y, T['dst']['out'])
    else:
        dycs, N, V, cin, cout, dxcs, dxdt = T['args']
        xa = _activated(T['src'][0], T['lazy'][0], T['slope'], N).reshape(N * V, cin)
        dy = T['dy'].values()
        w2 = T['w'].double().reshape(cout, cin)
        R['dx'] = _stored(dy @ w2, T['dst']['dx'])
        R['dw'] = _stored((dy.t() @ xa).reshape(1, -1), T['dst']['dw'])
        R['dbias'] = _stored(dy.sum(0).reshape(1, -1), T['dst']['dbias'])
    return R


def value_bound(table, T, name):
    """relerr bound of the instance's values: the family's existing bound (a 16-bit destination adds store_rounding())."""
    stem = name.split('<')[0]
    if product_type(table, T) is not None:
        b = 1e-4
    elif table in ('bwdw', 'hb') or stem in ('conv_wino8p_kernel', 'conv_wino8pb_kernel'):
        b = 2e-5
    else:
        b = 1e-5
    return b


def store_rounding(dst_dtype_code, ref):
    """The rounding of one store to a 16-bit destination, as an absolute error: round-to-nearest-even moves a value of the binade
    [2^e, 2^(e+1)) by at most half an ulp = 2^-9 (bf16) or 2^-12 (fp16) of the binade's UPPER end, so the scale the figure is relative to
    is max |ref| rounded up to a power of two (relative to max |ref| itself the half ulp reaches 2^-8 / 2^-11 just above a power of two)."""
    if dst_dtype_code not in _ROUND:
        return 0.0
    m = float(ref.abs().max())
    return _ROUND[dst_dtype_code] * (2.0 ** np.ceil(np.log2(m)) if m > 0 else 0.0)


def relerr(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def check(table, major, minor, T, R):
    """Everything the launch must have done, and nothing else.  Returns the measured figures (for the log)."""
    import torch
    figures = {}
    name = T['name']
    # sources unchanged, every byte
    srcs = list(T['src']) + [s for lz in T['lazy'] if lz is not None for s in lz]
    srcs += [T[k] for k in ('bias', 'by', 'bmean', 'brstd', 'ysrc', 'dy') if k in T]
    srcs += list(T.get('ylazy') or [])
    for s in srcs:
        assert torch.equal(_bits(s.dev.cpu()), _bits(s.host)), '%s: a source changed' % name
    got = {}
    for k, s in T['dst'].items():
        back = s.dev.cpu()
        m = s.mask()
        assert torch.equal(_bits(back)[~m], _bits(s.host)[~m]), '%s: %s written outside its slice (%d elements)' % (
            name, k, int((_bits(back)[~m] != _bits(s.host)[~m]).sum()))
        got[k] = s.values(back)
    for k, ref in R.items():
        if k == 'dbias' and not T.get('done'):
            continue                                  # not produced by this instance (the caller sums dY): its prefill is checked below
        g = got[k]
        assert not bool(g.isnan().any()), '%s: NaN left in %s' % (name, k)
        s = T['dst'][k]
        code = MT_F32 if s.es == 4 else (MT_BF16 if s.dtype == torch.bfloat16 else MT_F16)
        figures[k] = relerr(g, ref)
        bound = value_bound(table, T, name) + store_rounding(code, ref) / (float(ref.abs().max()) + 1e-12)
        print('%s %s relerr %.3e (bound %.3e)' % (name, k, figures[k], bound))
        assert figures[k] < bound, (name, k, figures[k], bound)
    if table == 'hb':
        assert T['done'] == T['dbias_done'], (name, T['done'], T['dbias_done'])
        if not T['done']:
            assert torch.equal(_bits(T['dst']['dbias'].dev.cpu()), _bits(T['dst']['dbias'].host)), '%s: dbias written although not done' % name
    if 'stats' in T['dst']:
        _check_stats(table, major, T, R, got, name)
    return figures


def _check_stats(table, major, T, R, got, name):
    """statistics partials summed over blocks, with the tolerances of test_conv_fwd and of
    test_winograd_backward_data_emits_norm_backward_statistics"""
    import torch
    N = T['N']
    p = T['p']
    cout = p.Cout
    part = got['stats']
    assert not bool(part.isnan().any()), '%s: statistics partials left unwritten' % name
    sums = part.reshape(N, T['nsb'], cout, 2).sum(1)
    keys = ['out0', 'out1'] if table == 'fwd' else ['out']
    keys = [k for k in keys if k in R]
    # the values as stored: the device's own output where the destination is 16-bit (checked against the reference above)
    is16 = T['dst'][keys[0]].es == 2
    o = torch.cat([(got[k] if is16 else R[k]).reshape(N, -1, R[k].shape[1]) for k in keys], 2)          # [N, V, Cout]
    V = o.shape[1]
    if T.get('bstats_served'):
        b = p.bstats
        y = T['by'].values().reshape(N, V, b.C)
        zh = ((y.float() - T['bmean'].values().float()[:, None, :]) * T['brstd'].values().float()[:, None, :]).double()
        gch = o[:, :, b.c0:b.c0 + b.C]
        dz = torch.where(zh > 0, gch, gch * float(np.float32(b.slope)))          # gamma = 1, beta = 0: z = zhat
        A, B = dz.sum(1), (dz * zh).sum(1)
        scale = float(dz.abs().sum(1).max())
        ea, eb = float((sums[:, b.c0:b.c0 + b.C, 0] - A).abs().max()), float((sums[:, b.c0:b.c0 + b.C, 1] - B).abs().max())
        print('%s bstats A %.3e B %.3e (scale %.3e)' % (name, ea, eb, scale))
        assert ea < 1e-5 * scale and eb < 3e-5 * scale, (name, ea, eb, scale)
        other = torch.ones(cout, dtype=torch.bool)
        other[b.c0:b.c0 + b.C] = False
        assert not bool(other.any()) or float(sums[:, other].abs().max()) == 0.0, name
        return
    s0, s1 = o.sum(1), (o * o).sum(1)
    print('%s stats sum %.3e sumsq %.3e' % (name, float((sums[..., 0] - s0).abs().max()), float(((sums[..., 1] - s1).abs() / s1.abs().clamp_min(1e-30)).max())))
    assert np.allclose(sums[..., 0].numpy(), s0.numpy(), rtol=1e-4, atol=1e-3 * np.sqrt(V)), name
    assert np.allclose(sums[..., 1].numpy(), s1.numpy(), rtol=1e-4), name


def run_case(case, dev, seed):
    """materialise, pin the instance name on the real addresses, launch, compare with the fp64 reference."""
    table, major, minor, expected = case
    T = materialise(table, major, minor, dev, seed)
    assert T['name'] == expected, (T['name'], expected)
    assert T['launches'], expected
    launch(table, T)
    return check(table, major, minor, T, reference(table, major, minor, T))
