"""Shared by tests/test_datapath_cases_cpu.py and tests/test_datapath_kernels_gpu.py (not a test module).

The units that move and reduce case data on real memory against numpy: named cases and references for the entry points of
csrc/preproc.hip, csrc/analyze.hip, csrc/crop.hip, csrc/loader.hip and csrc/select.hip.  numpy only; nothing here touches a device
or the library.  The launch geometry (8 blocks per CU, the thread counts, MT_PP_UNIT, the scan width, the chunk sizes) is read out of
the sources by `geometry()`, and every size that depends on the grid cap is computed from it for a CU count that the caller passes:
the CPU test evaluates the table at 256 CUs, the GPU test at the device's own count.

A case is `Case(id, entry, p)`: p holds the few numbers that define it, `build(case, geo)` makes its host inputs from a seed that is
the case's id (or from a closed form) together with the reference results.  `instances(case)` names the kernels and template
instances the entry point launches for it (the census of the CPU test).

References.  Everything except the moments is bit-exact against the numpy expression of the operation the unit's header cites:
 * mt_intensity_normalize: np.clip, `- mean`, `/ (sd + eps)`, `[seg < 0] = 0`, all in float32 (a NaN result is compared as "NaN on
   both sides": numpy does not specify a payload);
 * mt_label_counts / _locations: np.flatnonzero(slot == s) per slot, slot = the table entry of an integral label in [0, L);
 * mt_fg_sample_*: data[c][seg > 0][::stride][:out_cs] as bit patterns;
 * mt_label_presence: the set of integral values in [-1, 1022], a flag for anything else;
 * mt_label_convert: label_class.h's rule in numpy (zero | listed integer | unexpected), count and smallest unexpected value;
 * mt_nonzero_mask / mt_crop_nonzero: `!= 0` and slices, `seg[(seg == 0) & (mask == 0)] = label`;
 * mt_patch_gather: np.pad of the intersection box ('constant' / 'edge'); a patch that misses its source has no intersection to pad
   (np.pad refuses an empty array in 'edge' mode): there the documented meaning holds, every coordinate clamped into the source;
 * mt_seg_narrow: astype(int16) where the value is representable, the flag where not;
 * mt_select_kth*: the rank-th of the sorted KEYS of select.hip's header (bits ^ (sign ? all ones : sign bit)), turned back into bits.
For mt_masked_moments the count is exact; mean and sd come from math.fsum (correctly rounded sums of the float64-converted selection;
the centred squares are float64 products, each within 2^-52 of its value) and the bound is relative to the data:
|mean - ref| <= MOMENT_BOUND max|x| and |sd - ref| <= MOMENT_BOUND max(max|x|, ref), max|x| over the finite selected voxels.  A selection that
holds a NaN or an infinity has numpy's non-finite result (NaN, +-inf) and is compared as such.

The SEL_FLUSH_ITERS loop of sel_hist_kernel makes a second round only after 2^20 iterations of one block (2^30 per-block additions):
out of reach of a test of seconds, and left alone.
"""
import collections
import math
import os
import re

import numpy as np

GUARD = 64                         # elements on each side of a destination
F32_SENTINEL_BITS = 0x7fc0dead     # a NaN that no kernel produces
INT_SENTINEL = -12345
BYTE_SENTINEL = 0x77
MOMENT_BOUND = 1e-12

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'multitalent_amd', 'csrc')
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mtseg.h')
UNITS = ('preproc.hip', 'analyze.hip', 'crop.hip', 'loader.hip', 'select.hip')
MOMENTS_ALL, MOMENTS_SEG_GE0, MOMENTS_OPEN_RANGE = 0, 1, 2
PAD_CONSTANT, PAD_EDGE = 0, 1
NOSLOT = 255
LABEL_DTYPES = collections.OrderedDict((('uint8', 0), ('int8', 1), ('int16', 2), ('uint16', 3), ('int32', 4), ('uint32', 5), ('float32', 6),
                                        ('float64', 7)))
LABEL_CTYPES = {'uint8': 'uint8_t', 'int8': 'int8_t', 'int16': 'int16_t', 'uint16': 'uint16_t', 'int32': 'int32_t', 'uint32': 'uint32_t',
                'float32': 'float', 'float64': 'double'}
LABEL_SLOTS, LABEL_UNLISTED = 1023, 0xffff

Case = collections.namedtuple('Case', 'id entry p')


def rng(*key):
    """a generator seeded by the key's text (the same in every process)"""
    return np.random.RandomState(sum((i + 1) * ord(ch) for i, ch in enumerate(repr(key))) % (2 ** 31))


def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r'#define\s+%s\s+\(?(\d+)' % name, text)
    assert m, name
    return int(m.group(1))


Geo = collections.namedtuple('Geo', 'cus cap wave unit scan_threads threads maxranks max_src chunk chunk64')


def geometry(cus):
    """the launch geometry out of the sources, for a device of `cus` compute units"""
    stream, common, head = read('stream_common.h'), read('mt_common.h'), open(INCLUDE).read()
    m = re.search(r'mt_stream_cap\(\)\s*\{\s*return\s+mt_device_cus\(mt_current_device\(\)\)\s*\*\s*(\d+);', stream)
    assert m, 'mt_stream_cap'
    threads = {}
    for unit, name in (('preproc.hip', 'PP_THREADS'), ('analyze.hip', 'AN_THREADS'), ('crop.hip', 'CR_THREADS'), ('loader.hip', 'LD_THREADS'),
                       ('select.hip', 'SEL_THREADS')):
        threads[unit] = _define(read(unit), name)
    m2 = re.search(r'constexpr int VT = sizeof\(T\) == 8 \? (\d+) : (\d+)', read('analyze.hip'))
    assert m2, 'label_convert chunk'
    return Geo(cus=cus, cap=cus * int(m.group(1)), wave=_define(common, 'MT_WAVE'), unit=_define(head, 'MT_PP_UNIT'),
               scan_threads=_define(stream, 'MT_SCAN_THREADS'), threads=threads, maxranks=_define(read('select.hip'), 'SEL_MAXRANKS'),
               max_src=_define(head, 'MT_PATCH_MAX_SRC'), chunk=int(m2.group(2)), chunk64=int(m2.group(1)))


def kernels_in_sources():
    """{unit: [names of its __global__ functions]}"""
    out = {}
    for unit in UNITS:
        out[unit] = re.findall(r'__global__\s+(?:__launch_bounds__\(\w+\)\s+)?void\s+(\w+)\s*\(', read(unit))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def f32(bits_):
    return np.asarray(bits_, dtype=np.uint32).view(np.float32)


NAN32 = f32([0x7fc00000])[0]
DENORM_NEG = f32([0x80000001])[0]      # -1e-45
DENORM_POS = f32([0x00000001])[0]      # 1e-45


# ================================================================================================================================
# A. mt_masked_moments
def quad_trip(geo, unit='preproc.hip'):
    """elements a full grid of the quad loops covers in one trip"""
    return geo.cap * geo.threads[unit] * 4


def moments_cases(geo):
    out = []
    for pred in (MOMENTS_ALL, MOMENTS_SEG_GE0, MOMENTS_OPEN_RANGE):
        for V in (1, 2, 3, 4, 5, 1027):
            out.append(Case('mom-p%d-V%d' % (pred, V), 'mt_masked_moments', dict(pred=pred, V=V, C=1, kind='ct')))
        for C in (3, 16):
            out.append(Case('mom-p%d-C%d-V1027' % (pred, C), 'mt_masked_moments', dict(pred=pred, V=1027, C=C, kind='ct')))
        out.append(Case('mom-p%d-trip2' % pred, 'mt_masked_moments', dict(pred=pred, V=quad_trip(geo) + 1027, C=1, kind='ct', trip2=True)))
        for kind in ('nan', 'pinf', 'ninf', 'bothinf') + (('empty',) if pred != MOMENTS_ALL else ()):
            out.append(Case('mom-p%d-%s' % (pred, kind), 'mt_masked_moments', dict(pred=pred, V=1027, C=2, kind=kind)))
    out.append(Case('mom-p2-on-the-bounds', 'mt_masked_moments', dict(pred=MOMENTS_OPEN_RANGE, V=1027, C=2, kind='bounds')))
    out.append(Case('mom-p2-infinite-range', 'mt_masked_moments', dict(pred=MOMENTS_OPEN_RANGE, V=1027, C=2, kind='infrange')))
    out.append(Case('mom-p1-seg-edges', 'mt_masked_moments', dict(pred=MOMENTS_SEG_GE0, V=1027, C=2, kind='segedges')))
    out.append(Case('mom-p0-near-zero-mean', 'mt_masked_moments', dict(pred=MOMENTS_ALL, V=1027, C=1, kind='zeromean')))
    return out


def moments_build(c, geo):
    p, r = c.p, rng(c.id)
    V, C, kind = p['V'], p['C'], p['kind']
    data = (r.standard_normal((C, V)) * 5 - 900).astype(np.float32)
    seg = r.choice(np.array([-1, 0, 1, 2], np.float32), size=V, p=[0.4, 0.3, 0.2, 0.1])
    if V <= 5:
        seg[0] = 1                                      # something is selected
    lo, hi = np.full(C, -903.0) + np.arange(C) * 0.125, np.full(C, -897.0) + np.arange(C) * 0.125
    if V <= 5:
        lo[:], hi[:] = -950.0, -850.0
    if kind == 'zeromean':
        data = (r.standard_normal((C, V)) * 1000).astype(np.float32)
        data -= np.float32(data.astype(np.float64).mean())
    if kind in ('nan', 'pinf', 'ninf', 'bothinf'):
        lo[:], hi[:] = -np.inf, np.inf                  # the open range leaves +-inf and NaN out, as numpy's x[(x > lo) & (x < hi)]
        at = r.choice(V, 6, replace=False)
        seg[at[:4]] = 1
        seg[at[4:]] = -1                                # two of them are masked away
        vals = {'nan': [np.nan] * 6, 'pinf': [np.inf] * 6, 'ninf': [-np.inf] * 6, 'bothinf': [np.inf, -np.inf] * 3}[kind]
        data[0, at] = vals                              # channel 1 stays finite
    if kind == 'empty':
        seg[:] = -1
        lo[:], hi[:] = 5.0, 6.0
    if kind == 'bounds':
        lo[:], hi[:] = -903.0, -897.0
        data[:, ::7] = -903.0
        data[:, 3::7] = -897.0
        data[:, 5::7] = np.nextafter(np.float32(-903.0), np.float32(0))
        data[:, 6::7] = np.nextafter(np.float32(-897.0), np.float32(-1000))
    if kind == 'infrange':
        lo[:], hi[:] = -np.inf, np.inf
        data[0, ::11] = np.inf
        data[1, ::13] = -np.inf
        data[0, 5::17] = np.nan
    if kind == 'segedges':
        seg = r.choice(np.array([-0.0, np.nan, DENORM_NEG, np.inf, -1.0, 2.0, DENORM_POS, -np.inf], np.float32), size=V)
    refs = []
    for ch in range(C):
        x = data[ch]
        with np.errstate(invalid='ignore'):
            sel = np.ones(V, bool) if p['pred'] == MOMENTS_ALL else (seg >= 0) if p['pred'] == MOMENTS_SEG_GE0 else \
                (x.astype(np.float64) > lo[ch]) & (x.astype(np.float64) < hi[ch])
        refs.append(moments_ref(x[sel]) + (sel,))
    return dict(data=data, seg=seg, lo=lo, hi=hi, V=V, C=C, refs=refs)


def moments_ref(x):
    """(count, mean, sd, max|x| of the finite part) of a float32 selection"""
    x = np.asarray(x, np.float64)
    n = x.size
    fin = x[np.isfinite(x)]
    scale = float(np.abs(fin).max()) if fin.size else 0.0
    if n == 0:
        return 0, float('nan'), float('nan'), scale
    if fin.size != n:                                   # numpy's own non-finite result
        with np.errstate(invalid='ignore'):
            return n, float(x.mean()), float(x.std()), scale
    mean = math.fsum(x) / n
    d = x - mean
    return n, mean, math.sqrt(math.fsum(d * d) / n), scale


def moments_close(got, ref, scale, sd_ref=None):
    """(within the bound, error / scale) for a mean (sd_ref None) or an sd; non-finite references are matched in kind"""
    if not math.isfinite(ref):
        same = (math.isnan(ref) and math.isnan(got)) or got == ref
        return same, 0.0
    s = scale if sd_ref is None else max(scale, sd_ref)
    if not math.isfinite(got):
        return False, float('inf')
    err = abs(got - ref)
    return err <= MOMENT_BOUND * s, (err / s if s else (0.0 if err == 0 else float('inf')))


# ================================================================================================================================
# B. mt_intensity_normalize
def normalize_cases(geo):
    out = []
    i = 0
    for V in (1, 3, 1027, quad_trip(geo) + 1027):
        for clip, lo, hi in ((0, 0., 0.), (1, -950., -850.), (1, -900.5, -900.5)):
            for masked in (0, 1):
                stats = i % 2                            # host mean / sd and device stats in turn
                i += 1
                name = 'norm-V%s-c%d%s-m%d-%s' % (V if V <= 1027 else 'trip2', clip, 'eq' if clip and lo == hi else '', masked, 'dev' if stats else 'host')
                out.append(Case(name,
                                'mt_intensity_normalize', dict(V=V, clip=clip, lo=lo, hi=hi, masked=masked, stats=stats, kind='ct',
                                                               trip2=V > 1027)))
    for clip in (0, 1):
        for stats in (0, 1):
            out.append(Case('norm-nonfinite-c%d-%s' % (clip, 'dev' if stats else 'host'), 'mt_intensity_normalize',
                            dict(V=1027, clip=clip, lo=-950., hi=-850., masked=1, stats=stats, kind='nonfinite')))
    out.append(Case('norm-zero-mean-unit-sd', 'mt_intensity_normalize', dict(V=1027, clip=1, lo=-1., hi=1., masked=1, stats=0, kind='unit')))
    return out


def normalize_build(c, geo):
    p, r = c.p, rng(c.id)
    V = p['V']
    data = (r.standard_normal(V) * 60 - 900).astype(np.float32)
    seg = r.choice(np.array([-1, 0, 1], np.float32), size=V, p=[0.3, 0.4, 0.3])
    mean, sd = -897.25, 61.5
    if p['kind'] in ('nonfinite', 'unit'):
        special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, DENORM_POS, DENORM_NEG, f32([0x007fffff])[0], f32([0xffc00001])[0]], np.float32)
        data[::3] = special[np.arange(data[::3].size) % special.size]
        seg[:] = np.array([-0.0, np.nan, DENORM_NEG, 1.0, -1.0, 0.0, -np.inf], np.float32)[np.arange(V) % 7]
        seg = np.roll(seg, 1) if p['clip'] else seg
    if p['kind'] == 'unit':
        mean, sd = 0.0, 1.0                              # eps 0: signed zeros and denormals come through as they are
    eps = 0.0 if p['kind'] == 'unit' else 1e-8
    stats = np.array([V, mean + 1e-9, sd + 1e-9], np.float64)      # doubles that are no float32: the kernel rounds them once
    m32, s32 = (np.float32(stats[1]), np.float32(stats[2])) if p['stats'] else (np.float32(mean), np.float32(sd))
    with np.errstate(invalid='ignore', over='ignore'):
        x = data.copy()
        if p['clip']:
            x = np.clip(x, np.float32(p['lo']), np.float32(p['hi']))
        x = (x - m32) / (s32 + np.float32(eps))
        if p['masked']:
            x[seg < 0] = 0
    assert x.dtype == np.float32
    return dict(data=data, seg=seg, mean=float(m32) if not p['stats'] else 0.0, sd=float(s32) if not p['stats'] else 0.0, stats=stats, eps=eps,
                ref=x)


def same_float_results(got, ref):
    """bit-identical, or NaN on both sides"""
    return (bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref))


# ================================================================================================================================
# C. mt_label_counts / mt_label_locations
NSLOT_LADDER = (1, 63, 64, 65, 128, 129, 192, 193, 255)
V_LADDER = (1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193)


def unit_trip(geo):
    """units a full grid of the one-wave-per-unit loops covers in one trip"""
    return geo.cap * (geo.threads['preproc.hip'] // geo.wave)


def big_V(geo):
    """cap x 4 + 2 units: a whole unit and a short one that only a second trip reaches"""
    return (unit_trip(geo) + 1) * geo.unit + 1029


def label_cases(geo):
    out = []
    for n in NSLOT_LADDER:
        out.append(Case('lab-slots%d' % n, 'mt_label_locations', dict(kind='slots', nslots=n, V=5 * geo.unit + 5, cap=0)))
    for V in V_LADDER + (2 * geo.unit + 5,):
        out.append(Case('lab-V%d' % V, 'mt_label_locations', dict(kind='mix', nslots=3, V=V, cap=0)))
    for units in (geo.scan_threads + 1, 2 * geo.scan_threads + 1):
        out.append(Case('lab-units%d' % units, 'mt_label_locations', dict(kind='mix', nslots=3, V=(units - 1) * geo.unit + 100, cap=0)))
    out.append(Case('lab-capacity-one-short', 'mt_label_locations', dict(kind='mix', nslots=3, V=2 * geo.unit + 5, cap=-1)))
    out.append(Case('lab-many-queries', 'mt_label_locations', dict(kind='mix', nslots=3, V=geo.unit + 1, cap=0,
                                                                   nq=geo.cap * geo.threads['preproc.hip'] + 77)))
    out.append(Case('lab-trip2', 'mt_label_locations', dict(kind='big', nslots=3, V=big_V(geo), cap=0, trip2=True)))
    return out


def shape3(V):
    """a [D, H, W] with D H W = V and, where V allows, three axes longer than 1"""
    w = max(d for d in range(1, 98) if V % d == 0)
    h = max(d for d in range(1, 90) if (V // w) % d == 0)
    return V // (w * h), h, w


def slot_of(seg, table, L, nslots):
    """pp_slot: the table entry of an integral label in [0, L) when it is a slot below nslots, else NOSLOT"""
    f = np.asarray(seg, np.float64)
    with np.errstate(invalid='ignore'):
        ok = (f >= 0) & (f < L) & (f == np.floor(f))
    lab = np.where(ok, f, 0).astype(np.int64)
    s = table[lab].astype(np.int64)
    return np.where(ok & (s < nslots), s, NOSLOT).astype(np.uint8)


def big_seg(V, geo, r):
    """sparse closed form (every 997th voxel, classes in turn) and a dense end: the last whole unit and the short one behind it"""
    seg = np.zeros(V, np.float32)
    at = np.arange(0, V, 997)
    seg[at] = 1 + (at // 997) % 3
    last = ((V - 1) // geo.unit - 1) * geo.unit
    seg[last:] = r.randint(-1, 4, V - last)
    return seg


def label_build(c, geo):
    p, r = c.p, rng(c.id)
    V, nslots, kind = p['V'], p['nslots'], p['kind']
    if kind == 'slots':
        L = nslots + 2
        perm = r.permutation(L)
        if perm[0] == 0:
            perm[[0, 1]] = perm[[1, 0]]                  # -0.0 and 0 are label 0: keep it off the class that is moved below
        table = np.full(L, 255, np.uint8)
        table[perm[:nslots]] = np.arange(nslots)
        table[perm[nslots]] = min(nslots, 255)           # a slot that is no class; perm[nslots + 1] stays 255 inside the table
        body = np.repeat(perm[:nslots], 7 + np.arange(nslots)).astype(np.float32)          # every class, each count its own
        junk = np.array([0.5, -1, L, np.nan, 1e9, perm[nslots], perm[nslots + 1], -0.0, -2.5, np.inf], np.float32)
        seg = np.concatenate([body, junk[np.arange(V - body.size) % junk.size]])
        r.shuffle(seg)
        l0 = np.float32(perm[0])                         # class of slot 0: all of it into the last 64-voxel round of unit 1
        src = np.flatnonzero(seg == l0)
        assert src.size <= geo.wave
        dst = 2 * geo.unit - 1 - np.arange(src.size)
        keep = seg[dst].copy()
        seg[dst] = seg[src]
        seg[src[~np.isin(src, dst)]] = keep[~np.isin(dst, src)]
    elif kind == 'mix':
        L = 5
        table = np.array([1, 255, 0, 2, 7], np.uint8)   # label 1 is listed as 255, label 4 as a slot beyond nslots
        vals = np.array([-1, 0, 1, 2, 3, 4, 5, 0.5, -0.0, np.nan, 1e9], np.float32)
        seg = vals[r.choice(vals.size, size=V, p=[.2, .2, .05, .2, .2, .03, .03, .03, .02, .02, .02])]
    else:
        L = 4
        table = np.array([255, 0, 1, 2], np.uint8)
        seg = big_seg(V, geo, r)
    slot = slot_of(seg, table, L, nslots)
    order = [np.flatnonzero(slot == s) for s in range(nslots)]
    counts = np.array([o.size for o in order], np.int64)
    total = int(counts.sum())
    idx = np.concatenate(order).astype(np.int32) if total else np.zeros(0, np.int32)
    cap = max(1, total + p['cap']) if total else 1
    base = np.concatenate([[0], np.cumsum(counts)])
    # queries: every rank of every class with -1, count, count + 1 (small cases), else the ends and a draw
    qs, qr = [], []
    for s in range(-1, nslots + 1):
        n = int(counts[s]) if 0 <= s < nslots else 3
        ranks = np.arange(-1, n + 2) if V <= 6 * geo.unit else \
            np.unique(np.concatenate([[-1, 0, 1, n // 2, n - 2, n - 1, n, n + 1], r.randint(0, max(n, 1), 500)]))
        qs.append(np.full(ranks.size, s, np.int32))
        qr.append(ranks.astype(np.int64))
    qslot, qrank = np.concatenate(qs), np.concatenate(qr)
    if p.get('nq'):
        rep = -(-p['nq'] // qslot.size)
        qslot, qrank = np.tile(qslot, rep)[:p['nq']], np.tile(qrank, rep)[:p['nq']]
    D, H, W = shape3(V)
    out = np.full((qslot.size, 3), -1, np.int64)
    okq = (qslot >= 0) & (qslot < nslots) & (qrank >= 0)
    pos = base[np.clip(qslot, 0, nslots - 1)] + qrank
    okq &= (pos < base[np.clip(qslot, 0, nslots - 1) + 1]) & (pos < cap)
    lin = idx[pos[okq]].astype(np.int64)
    out[okq] = np.stack(np.unravel_index(lin, (D, H, W)), 1)
    return dict(seg=seg, table=table, L=L, nslots=nslots, V=V, shape=(D, H, W), slot=slot, counts=counts, idx=idx, cap=cap, total=total,
                qslot=qslot, qrank=qrank, out=out)


# ================================================================================================================================
# D. mt_fg_sample_count / _gather
def fg_cases(geo):
    out = []
    for V in V_LADDER + (2 * geo.unit + 5,):
        for stride in (1, 7):
            out.append(Case('fg-V%d-s%d' % (V, stride), 'mt_fg_sample_gather', dict(V=V, C=1, stride=stride, cs=0, kind='mix')))
    for units in (geo.scan_threads + 1, 2 * geo.scan_threads + 1):
        out.append(Case('fg-units%d' % units, 'mt_fg_sample_gather', dict(V=(units - 1) * geo.unit + 100, C=1, stride=10, cs=0, kind='mix')))
    for stride in (1, 2, 7, 10, geo.unit - 1, geo.unit, geo.unit + 1, 'n', 'n+1', 2 ** 31, 2 ** 40):
        for cs in ((0, 3, -2) if stride in (1, 7, 10) else (0,)):
            out.append(Case('fg-stride%s-cs%+d' % (stride, cs), 'mt_fg_sample_gather', dict(V=3 * geo.unit + 5, C=1, stride=stride, cs=cs, kind='dense')))
    out.append(Case('fg-C16', 'mt_fg_sample_gather', dict(V=geo.unit + 77, C=16, stride=7, cs=0, kind='mix')))
    out.append(Case('fg-trip2', 'mt_fg_sample_gather', dict(V=big_V(geo), C=1, stride=10, cs=0, kind='big', trip2=True)))
    return out


def fg_build(c, geo):
    p, r = c.p, rng(c.id)
    V, C, kind = p['V'], p['C'], p['kind']
    if kind == 'big':
        seg = big_seg(V, geo, r)
        data = np.arange(V, dtype=np.uint32).view(np.float32).reshape(1, V)          # the bit pattern of a voxel is its index
    else:
        vals = np.array([0, 1, 2, -1, 0.5, DENORM_POS, -0.0, np.nan, np.inf, -np.inf, DENORM_NEG], np.float32)
        pr = [.3, .2, .1, .1, .05, .05, .05, .05, .04, .03, .03] if kind == 'mix' else [.05, .5, .2, .05, .05, .05, .02, .02, .02, .02, .02]
        seg = vals[r.choice(vals.size, size=V, p=pr)]
        data = r.randint(0, 2 ** 32, (C, V), dtype=np.uint64).astype(np.uint32)
        data[:, ::5] |= 0x7f800001                                                  # NaN payloads of both signs
        data = data.view(np.float32)
    with np.errstate(invalid='ignore'):
        sel = seg > 0
    n = int(sel.sum())
    stride = {'n': max(n, 1), 'n+1': n + 1}.get(p['stride'], p['stride'])
    full = [bits(data[ch])[sel][::stride] for ch in range(C)]
    due = len(full[0])
    cs = max(1, max(due, 1) + p['cs'])
    ref = np.stack([f[:cs] for f in full])
    nan = np.array([int(((f & 0x7fffffff) > 0x7f800000).sum()) for f in ref], np.int64)
    return dict(data=data, seg=seg, V=V, C=C, sel=sel, n=n, stride=stride, cs=cs, ref=ref, nan=nan)


# ================================================================================================================================
# E. mt_label_presence
BAD_LABELS = (0.5, 1023.0, -2.0, float('nan'), float('inf'), float('-inf'), -1.5)


def presence_ref(seg):
    f = np.asarray(seg, np.float64)
    with np.errstate(invalid='ignore'):
        ok = (f >= -1) & (f <= 1022) & (f == np.floor(f))
    bitmap = np.zeros(32, np.uint32)
    for lab in np.unique(f[ok]).astype(np.int64):
        bitmap[(lab + 1) >> 5] |= np.uint32(1 << ((lab + 1) & 31))
    return bitmap, int((~ok).any())


def presence_cases(geo):
    out = [Case('pres-each-label-alone', 'mt_label_presence', dict(kind='each')),
           Case('pres-all-1024', 'mt_label_presence', dict(kind='all', V=1027)),
           Case('pres-runs', 'mt_label_presence', dict(kind='runs', V=4 * 4099 + 3)),
           Case('pres-trip2', 'mt_label_presence', dict(kind='trip2', V=quad_trip(geo, 'analyze.hip') + 1027, trip2=True))]
    return out


def presence_build(c, geo):
    p, r = c.p, rng(c.id)
    if p['kind'] == 'each':
        seg = np.arange(-1, 1023, dtype=np.float32)
        return dict(seg=seg, refs=[presence_ref(seg[i:i + 1]) for i in range(seg.size)])
    V = p['V']
    if p['kind'] == 'all':
        seg = np.arange(-1, 1026, dtype=np.float32) % 1023
        seg[:1024] = np.arange(-1, 1023)
        r.shuffle(seg)
    elif p['kind'] == 'runs':
        seg = np.repeat(np.array([5, 7, 5, 1022, -1], np.float32), V // 5 + 1)[:V]
    else:
        seg = np.ones(V, np.float32)
        seg[quad_trip(geo, 'analyze.hip') + 4 * 17 + 2] = 900          # a quad that only a second trip reads
        seg[-1] = 33                                                   # and the scalar tail
    return dict(seg=seg, V=V, ref=presence_ref(seg), second=quad_trip(geo, 'analyze.hip') + 4 * 101 + 1)


# ================================================================================================================================
# F. mt_label_convert
def convert_cases(geo):
    out = [Case('conv-%s-V1027' % d, 'mt_label_convert', dict(dtype=d, chunks=0, V=1027)) for d in LABEL_DTYPES]
    for d in ('uint8', 'int16', 'int32', 'float64'):
        out.append(Case('conv-%s-trip2' % d, 'mt_label_convert', dict(dtype=d, chunks=geo.cap * geo.threads['analyze.hip'] + 3, trip2=True)))
    return out


def convert_table():
    t = np.full(LABEL_SLOTS, LABEL_UNLISTED, np.uint16)
    t[1:10] = (np.arange(1, 10) * 29) % 256
    t[100] = 0
    return t


def convert_ref(x, table):
    """label_class.h in numpy: (out uint8, count of unexpected voxels, smallest unexpected value as the bits of its double, or all ones)"""
    v = np.asarray(x).astype(np.float64)
    with np.errstate(invalid='ignore'):
        pos = v > 1e-20
        integral = pos & (v <= LABEL_SLOTS - 1) & (v == np.floor(v))
    lab = np.where(integral, v, 0).astype(np.int64)
    listed = integral & (table[lab] != LABEL_UNLISTED)
    out = np.where(listed, table[lab], 0).astype(np.uint8)
    bad = pos & ~listed
    key = int(bits(np.array([v[bad].min()]))[0]) if bad.any() else 0xffffffffffffffff
    return out, int(bad.sum()), key


def convert_build(c, geo):
    p, r = c.p, rng(c.id)
    dt = np.dtype(p['dtype'])
    vt = geo.chunk64 if dt.itemsize == 8 else geo.chunk
    head, tail = 1, 5
    V = p['V'] if not p['chunks'] else head + p['chunks'] * vt + tail
    listed = np.array([0, 1, 2, 3, 9, 100, 0, 0], np.int64)
    x = listed[r.randint(0, listed.size, V)].astype(dt)
    lim = 127 if p['dtype'] == 'int8' else 255
    bad = np.array([lim, lim - 20, 50], np.int64).astype(dt)           # unlisted labels every type can hold
    if p['chunks']:                                                    # only behind the first trip, and in the tail
        second = head + geo.cap * geo.threads['analyze.hip'] * vt
        x[second + 5] = bad[0]
        x[second + vt + 1] = bad[1]
        x[-2] = bad[2]
    else:
        at = r.choice(V, 40, replace=False)
        x[at] = bad[np.arange(40) % 3]
        if dt.kind == 'f':
            x[at[:6]] = [0.5, np.nan, np.inf, 1e-20, 1023, -3]
        elif dt.kind == 'i':
            x[at[:2]] = [-1, np.iinfo(dt).min]
    table = convert_table()
    out, cnt, key = convert_ref(x, table)
    return dict(x=x, V=V, head=head, table=table, out=out, count=cnt, key=key, dtype=p['dtype'])


# ================================================================================================================================
# G. mt_nonzero_mask
def mask_cases(geo):
    g = geo.cap * geo.threads['crop.hip']
    return [Case('mask-%s' % where, 'mt_nonzero_mask', dict(where=where, nquad=3 * g + 100, trip2=True)) for where in ('third-stride', 'last-q1', 'tail')]


def mask_build(c, geo):
    p = c.p
    g = geo.cap * geo.threads['crop.hip']
    head, tail = 1, 2
    V = head + 4 * p['nquad'] + tail
    data = np.zeros((2, V), np.float32)
    data[0, 5::9] = -0.0                                 # zero by numpy's rule
    special = f32([0x7fc00000, 0x00000001, 0x80000001, 0x3f800000, 0xff800000])
    if p['where'] == 'third-stride':
        at = head + 4 * (2 * g) + np.arange(0, 4 * g, 37)
    elif p['where'] == 'last-q1':
        at = head + 4 * (3 * g) + np.arange(0, 400, 3)
    else:
        at = np.array([0, V - 2, V - 1])
    data[np.arange(at.size) % 2, at] = special[np.arange(at.size) % special.size]
    return dict(data=data, V=V, head=head, ref=(data != 0).any(0).astype(np.uint8), at=at)


# ================================================================================================================================
# H. mt_crop_nonzero
def crop_boxes(shape):
    D, H, W = shape
    full = [0, D, 0, H, 0, W]
    out = [('whole', full), ('one-voxel-corner', [0, 1, 0, 1, 0, 1]), ('one-voxel-inside', [D // 2, D // 2 + 1, H // 2, H // 2 + 1, W // 2, W // 2 + 1]),
           ('one-voxel-far-corner', [D - 1, D, H - 1, H, W - 1, W])]
    for a, n in enumerate(shape):
        b = list(full)
        b[2 * a], b[2 * a + 1] = n // 2, n // 2 + 1
        out.append(('thin-axis%d' % a, b))
        lo = [1, D - 1, 1, H - 1, 1, W - 1]
        lo[2 * a] = 0
        out.append(('touches-low-face%d' % a, lo))
        hi = [1, D - 1, 1, H - 1, 1, W - 1]
        hi[2 * a + 1] = n
        out.append(('touches-high-face%d' % a, hi))
    return out


def crop_cases(geo):
    out = []
    k = 0
    for shape in ((3, 5, 7), (17, 33, 65)):
        for name, box in crop_boxes(shape):
            for seg_mode in (0, 1):
                k += 1
                cs = (1, 3)[(k // 2) % 2]
                label = ((-1, 0, 5) if seg_mode == 0 else (-1.0, 2.5, 'nan'))[(k // 2) % 3]
                out.append(Case('crop%d-%dx%dx%d-%s' % ((seg_mode,) + shape + (name,)), 'mt_crop_nonzero',
                                dict(shape=shape, box=box, seg_mode=seg_mode, CS=cs if seg_mode else 0, label=label, C=1 + (k // 2 + seg_mode) % 2)))
    d = -(-(geo.cap * geo.threads['crop.hip'] + 1) // (96 * 94)) + 1        # a box of d x 96 x 94 voxels: more than one trip of the grid
    big, box = (d + 1, 96, 96), [1, d + 1, 0, 96, 1, 95]
    for seg_mode in (0, 1):
        out.append(Case('crop%d-trip2' % seg_mode, 'mt_crop_nonzero', dict(shape=big, box=box, seg_mode=seg_mode, CS=seg_mode,
                                                                           label=-1 if not seg_mode else 'nan',
                                                                           C=1, trip2=True)))
    return out


def crop_ref(data, mask, seg, box, label):
    """slices of the box; seg (float32 [CS, ...]) gets `label` where it is zero outside the mask, without seg an int8 map of the mask"""
    sl = (slice(box[0], box[1]), slice(box[2], box[3]), slice(box[4], box[5]))
    out = np.ascontiguousarray(data[(slice(None),) + sl])
    if seg is None:
        return out, np.where(mask[sl] != 0, 0, label).astype(np.int8)
    s = np.ascontiguousarray(seg[(slice(None),) + sl]).copy()
    with np.errstate(invalid='ignore'):
        s[(s == 0) & np.broadcast_to(mask[sl][None] == 0, s.shape)] = label
    return out, s


def crop_build(c, geo):
    p, r = c.p, rng(c.id)
    D, H, W = p['shape']
    C, CS = p['C'], p['CS']
    data = r.randint(0, 2 ** 32, (C, D, H, W), dtype=np.uint64).astype(np.uint32).view(np.float32)
    mask = (r.uniform(size=(D, H, W)) < 0.5).astype(np.uint8) * r.randint(1, 256, (D, H, W)).astype(np.uint8)      # any non-zero byte is 'inside'
    label = NAN32 if p['label'] == 'nan' else p['label']
    seg = None
    if p['seg_mode']:
        vals = np.array([0.0, -0.0, 1.0, 2.0, -1.0, np.nan, DENORM_POS], np.float32)
        seg = vals[r.randint(0, vals.size, (CS, D, H, W))]
    b = p['box']
    out, seg_out = crop_ref(data, mask, seg, b, label)
    return dict(data=data, mask=mask, seg=seg, box=np.array(b, np.int32), out=out, seg_out=seg_out, label=float(label))


# ================================================================================================================================
# I. mt_patch_gather
PATCH_WIDTHS = (1, 2, 3, 4, 5, 7, 8)


def gather_cases(geo):
    out = []
    for pw in PATCH_WIDTHS:
        for pad in (PAD_CONSTANT, PAD_EDGE):
            out.append(Case('gather-16src-PW%d-pad%d' % (pw, pad), 'mt_patch_gather', dict(n=geo.max_src, C=1 + pw % 2 * 2, P=(3, 4, pw), pad=pad, kind='many',
                                                                                           fill='nan' if pw % 2 else -1.0)))
    for pad in (PAD_CONSTANT, PAD_EDGE):
        out.append(Case('gather-1src-pad%d' % pad, 'mt_patch_gather', dict(n=1, C=3, P=(5, 6, 12), pad=pad, kind='one', fill=-1.0)))
        qw = -(-(geo.cap * geo.threads['loader.hip'] // 2 + 1) // (64 * 64)) + 1
        out.append(Case('gather-trip2-pad%d' % pad, 'mt_patch_gather', dict(n=2, C=1, P=(64, 64, 4 * qw), pad=pad, kind='big', fill='nan', trip2=True)))
    return out


def gather_sources(c, geo):
    """[(shape, lb)] of the case's samples"""
    p = c.p
    PD, PH, PW = p['P']
    if p['kind'] == 'one':
        return [((4, 9, 13), (-1, 2, 2))]            # the quad at w = 8 reads z = 10 .. 13: its last voxel is the first one outside
    if p['kind'] == 'big':
        return [((40, 70, PW - 10), (-5, -3, -4)), ((70, 40, PW + 3), (3, -20, 6))]
    out = []
    for j in range(p['n']):
        shape = (1 + j % 4, 2 + (j * 3) % 5, 1 + j % 5)                 # widths 1 .. 5 in turn
        lb = [(-1, 0, 1)[j % 3], (0, -2, 1)[(j // 3) % 3], (-1, 0, 1, -2)[j % 4]]
        if 4 <= j < 10:                                                 # wholly outside, on each axis and side
            a, side = (j - 4) // 2, (j - 4) % 2
            lb[a] = shape[a] + 1 if side else -p['P'][a] - 1
        out.append((shape, tuple(lb)))
    return out


def gather_index(n, lb, P, pad):
    """per axis: source coordinate of every patch coordinate (clamped) and whether it lies inside"""
    s = lb + np.arange(P)
    return np.clip(s, 0, n - 1), (s >= 0) & (s < n)


def gather_ref_sample(data, seg, lb, P, pad, fill):
    """np.pad of the intersection box; data [C, sx, sy, sz] float32, seg [sx, sy, sz] int16 -> ([C, PD, PH, PW], [PD, PH, PW]) float32"""
    shape = seg.shape
    lo = [max(0, lb[a]) for a in range(3)]
    hi = [min(shape[a], lb[a] + P[a]) for a in range(3)]
    fillv = np.float32(fill)
    if any(h <= l for l, h in zip(lo, hi)):                           # no intersection: nothing to pad
        sout = np.full(P, fillv, np.float32)
        if pad == PAD_CONSTANT:
            return np.zeros((data.shape[0],) + tuple(P), np.float32), sout
        ix = [gather_index(shape[a], lb[a], P[a], pad)[0] for a in range(3)]
        return data[:, ix[0][:, None, None], ix[1][None, :, None], ix[2][None, None, :]], sout
    sl = tuple(slice(l, h) for l, h in zip(lo, hi))
    width = [(lo[a] - lb[a], lb[a] + P[a] - hi[a]) for a in range(3)]
    d = data[(slice(None),) + sl]
    dout = np.pad(d, [(0, 0)] + width, 'constant', constant_values=0) if pad == PAD_CONSTANT else np.pad(d, [(0, 0)] + width, 'edge')
    s = seg[sl].astype(np.float32)
    inside = np.pad(np.ones(s.shape, bool), width, 'constant', constant_values=False)
    sout = np.where(inside, np.pad(s, width, 'constant', constant_values=0), fillv)
    return dout, sout


def gather_build(c, geo):
    p, r = c.p, rng(c.id)
    fill = NAN32 if p['fill'] == 'nan' else np.float32(p['fill'])
    srcs, dref, sref = [], [], []
    for j, (shape, lb) in enumerate(gather_sources(c, geo)):
        data = r.randint(0, 2 ** 32, (p['C'],) + shape, dtype=np.uint64).astype(np.uint32).view(np.float32)      # any bit pattern: a copy
        seg = r.randint(-32768, 32768, shape).astype(np.int16)
        d, s = gather_ref_sample(data, seg, lb, p['P'], p['pad'], fill)
        srcs.append(dict(data=data, seg=seg, shape=shape, lb=lb, data_off=1 + j % 3, seg_off=1 + 2 * (j % 2)))
        dref.append(d)
        sref.append(s)
    return dict(srcs=srcs, data_ref=np.stack(dref), seg_ref=np.stack(sref), fill=float(fill))


# ================================================================================================================================
# J. mt_seg_narrow
NARROW_BAD = (32768.5, -32768.5, 32768.0, -32769.0, 0.5, float('nan'), float('inf'), float('-inf'))


def narrow_cases(geo):
    V = quad_trip(geo, 'loader.hip') + 1027
    out = [Case('narrow-good-V%s' % (v if v != V else 'trip2'), 'mt_seg_narrow', dict(V=v, bad=None, where=None, trip2=v == V)) for v in (1, 3, 4, 1027, V)]
    for i, bad in enumerate(NARROW_BAD):
        for where in ('quad', 'tail', 'trip2'):
            out.append(Case('narrow-bad%d-%s' % (i, where), 'mt_seg_narrow', dict(V=V if where == 'trip2' else 1027, bad=bad, where=where,
                                                                                  trip2=where == 'trip2')))
    return out


def narrow_build(c, geo):
    p, r = c.p, rng(c.id)
    V = p['V']
    seg = r.randint(-32768, 32768, V).astype(np.float32)
    edge = np.array([-32768, 32767, 0.0, -0.0, -1, 1], np.float32)
    seg[:min(V, 6)] = edge[:min(V, 6)]
    seg[-min(V, 6):] = edge[::-1][-min(V, 6):]
    if V > 1027:
        t = quad_trip(geo, 'loader.hip')
        seg[t:t + 6] = edge
    good = np.ones(V, bool)
    if p['bad'] is not None:
        at = {'quad': 4 * 50 + 2, 'tail': V - 1, 'trip2': quad_trip(geo, 'loader.hip') + 4 * 33 + 1}[p['where']]
        seg[at] = p['bad']
        good[at] = False
    ref = np.where(good, seg, 0).astype(np.int16)
    return dict(seg=seg, V=V, good=good, ref=ref, flag=int(not good.all()))


# ================================================================================================================================
# K. mt_select_kth / mt_select_kth_f32
def select_cases(geo):
    out = []
    for width in (4, 8):
        n = geo.cap * geo.threads['select.hip'] * (16 // width) + 1027
        for off in (0, 1):
            for kind in ('spread', 'lastbyte'):
                out.append(Case('select-f%d-off%d-%s' % (8 * width, off, kind), 'mt_select_kth' + ('_f32' if width == 4 else ''),
                                dict(width=width, n=n, off=off, kind=kind, trip2=True)))
        out.append(Case('select-f%d-small' % (8 * width), 'mt_select_kth' + ('_f32' if width == 4 else ''),
                        dict(width=width, n=5, off=1, kind='spread')))
    return out


def select_key(b):
    """select.hip's header: the key orders as the numbers do, -0.0 before +0.0, NaNs by bit pattern at both ends"""
    sign = b.dtype.type(1) << b.dtype.type(8 * b.dtype.itemsize - 1)
    return b ^ np.where(b & sign, ~b.dtype.type(0), sign)


def select_unkey(k):
    sign = k.dtype.type(1) << k.dtype.type(8 * k.dtype.itemsize - 1)
    return k ^ np.where(k & sign, sign, ~k.dtype.type(0))


def select_build(c, geo):
    p, r = c.p, rng(c.id)
    n, width = p['n'], p['width']
    U = np.uint32 if width == 4 else np.uint64
    one = U(1)
    top = 8 * width - 1
    if p['kind'] == 'spread':                            # every bit pattern: NaNs of both signs, infinities, denormals, zeros
        b = (r.randint(0, 2 ** 32, n, dtype=np.uint64) | (r.randint(0, 2 ** 32, n, dtype=np.uint64) << np.uint64(32))).astype(U) if width == 8 else \
            r.randint(0, 2 ** 32, n, dtype=np.uint64).astype(U)
        expo = (U(0xff) << U(23)) if width == 4 else (U(0x7ff) << U(52))
        special = np.array([0, one << U(top), 1, (one << U(top)) | one, expo, expo | (one << U(top)), expo | one, expo | (one << U(top)) | one], U)
        if n > 16:
            b[8:n - 8:101] = special[np.arange(b[8:n - 8:101].size) % 8]
    else:                                                # one value but for the last byte
        base = U(0xc2f6e900) if width == 4 else U(0xc05edd2f1a9fbe00)
        b = base | r.randint(0, 256, n, dtype=np.uint64).astype(U)
    # the extremes of the key order sit in the head and the tail that block 0 reads by itself
    b[0] = ~U(0)                                         # -NaN, all ones: key 0
    b[-1] = U((1 << top) - 1)                            # +NaN, all ones below the sign: the largest key
    keys = np.sort(select_key(b))
    digit = (keys >> U(top - 7)).astype(np.int64)
    first = [int(np.searchsorted(digit, d)) for d in np.unique(digit)]
    if len(first) >= 8:
        eight = [first[i * (len(first) - 1) // 7] for i in range(8)]
    else:
        eight = [int(x) for x in np.linspace(0, n - 1, 8).astype(np.int64)]
    ranksets = [eight, [n // 3] * 8, [0, n - 1]] if n > 16 else [[0, n - 1], [2] * 8, list(range(n))]
    refs = [select_unkey(keys[np.array(rs)]) for rs in ranksets]
    return dict(bits=b, n=n, ranksets=ranksets, refs=refs, groups=len(set(int(digit[k]) for k in ranksets[0])))


# ================================================================================================================================
FAMILIES = collections.OrderedDict((
    ('moments', (moments_cases, moments_build)), ('normalize', (normalize_cases, normalize_build)), ('label', (label_cases, label_build)),
    ('fg', (fg_cases, fg_build)), ('presence', (presence_cases, presence_build)), ('convert', (convert_cases, convert_build)),
    ('mask', (mask_cases, mask_build)), ('crop', (crop_cases, crop_build)), ('gather', (gather_cases, gather_build)),
    ('narrow', (narrow_cases, narrow_build)), ('select', (select_cases, select_build))))


def cases(family, cus):
    return FAMILIES[family][0](geometry(cus))


def build(family, case, cus):
    return FAMILIES[family][1](case, geometry(cus))


def instances(case):
    """the kernels (with their template arguments) that the case's entry point launches"""
    e, p = case.entry, case.p
    if e == 'mt_masked_moments':
        return ['moments_kernel<%d,0>' % p['pred'], 'moments_kernel<%d,1>' % p['pred'], 'moments_finalize_kernel']
    if e == 'mt_intensity_normalize':
        return ['normalize_kernel']
    if e == 'mt_label_locations':                        # always behind mt_label_counts
        return ['label_units_kernel<false>', 'label_scan_kernel', 'label_base_kernel', 'label_units_kernel<true>', 'label_gather_kernel']
    if e == 'mt_fg_sample_gather':                       # always behind mt_fg_sample_count
        return ['fg_count_kernel', 'fg_scan_kernel', 'fg_gather_kernel']
    if e == 'mt_label_presence':
        return ['label_presence_kernel']
    if e == 'mt_label_convert':
        return ['label_convert_kernel<%s>' % LABEL_CTYPES[p['dtype']]]
    if e == 'mt_nonzero_mask':
        return ['nz_mask_kernel']
    if e == 'mt_crop_nonzero':
        return ['crop_kernel<%d>' % p['seg_mode']]
    if e == 'mt_patch_gather':
        return ['patch_gather_kernel']
    if e == 'mt_seg_narrow':
        return ['seg_narrow_kernel']
    if e in ('mt_select_kth', 'mt_select_kth_f32'):
        k = 'uint32_t' if p['width'] == 4 else 'uint64_t'
        return ['sel_init_kernel<%s>' % k, 'sel_hist_kernel<%s>' % k, 'sel_pick_kernel<%s>' % k]
    raise KeyError(e)


def launchable_instances():
    """every kernel of the five units, with every template argument its entry point can pass"""
    out = ['moments_kernel<%d,%d>' % (q, s) for q in range(3) for s in range(2)]
    out += ['moments_finalize_kernel', 'normalize_kernel', 'label_units_kernel<false>', 'label_units_kernel<true>', 'label_scan_kernel',
            'label_base_kernel', 'label_gather_kernel', 'fg_count_kernel', 'fg_scan_kernel', 'fg_gather_kernel', 'label_presence_kernel']
    out += ['label_convert_kernel<%s>' % t for t in LABEL_CTYPES.values()]
    out += ['nz_mask_kernel', 'crop_kernel<0>', 'crop_kernel<1>', 'patch_gather_kernel', 'seg_narrow_kernel']
    out += ['%s<%s>' % (k, t) for k in ('sel_init_kernel', 'sel_hist_kernel', 'sel_pick_kernel') for t in ('uint32_t', 'uint64_t')]
    return out
