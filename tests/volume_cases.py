"""Shared by tests/test_volume_cases_cpu.py and tests/test_volume_kernels_gpu.py (not a test module).

The label-volume and intensity units on real memory: named cases and references for the entry points of csrc/metrics.hip,
csrc/postproc.hip, csrc/intensity.hip and what tests/test_ensemble_gpu.py leaves open of csrc/ensemble.hip.  numpy and scipy only;
nothing here touches a device or the library.  The launch geometry (8 blocks per CU, the thread counts, the chunk sizes, the brick,
the 2^20 brick cap, the `* 4` of the rows and query grids) is read out of the sources by `geometry()`, and every size that depends on
the grid cap is computed from it for a CU count that the caller passes: the CPU test evaluates the table at 256 CUs, the GPU test at
the device's own count.  The closed forms of the large cases are checked against scipy at 1 CU, where they are small.

A case is `Case(id, entry, p)`; `build(family, case, cus)` makes its host inputs and the reference results, `instances(case)` names
the kernels and template instances its entry point launches, `second_trips(case, geo)` the stride loops it takes a second time.

References.
 * mt_seg_joint_hist: np.bincount(remap[t] * C + remap[r]), exact.
 * mt_surface_distances: borders from scipy's binary_erosion with generate_binary_structure(3, conn); the distance of a border voxel
   is the minimum over ALL border voxels of the other mask of sqrt((dz sz)^2 + (dy sy)^2 + (dx sx)^2), float64 in that order.  With
   dyadic spacings every product and sum is exact and the comparison is bit for bit; otherwise the bound is SD_ULPS = 2 ulp of the
   reference (three products, two sums, a square root, each within half an ulp with or without fusion).  stats: counts exact, max
   exact, sum within n 2^-52 sum of math.fsum.  Under a capacity below nA + nB the stored prefix is compared, the counts stay true,
   max and sum are those of the stored prefix per direction (an empty prefix has max 0 and sum 0).
 * mt_cc_label3d / mt_cc_remove: scipy.ndimage.label (default structure), every label mapped to the smallest linear index of its
   component, sizes from np.bincount, the removal rule of the header with Python floats.  Exact.
 * mt_fill_holes3d: scipy.ndimage.binary_fill_holes(mask != 0); bbox and count from numpy; at count 0 only the count.
 * mt_channel_stats: min / max exact (numpy's, NaN included); mean and sd from math.fsum of the float64-converted channel,
   |mean err| <= 1e-10 max|x|, |sd err| <= 1e-8 sd (the bounds of tests/test_intensity_gpu.py).  A channel with an infinity has numpy's
   min and max and a non-finite mean and sd; a channel with a NaN has four NaNs.
 * mt_intensity_apply: `apply_ref`, the float32 arithmetic of tests/intensity_restatement.py with the statistics as arguments (the CPU
   test shows the two agree bit for bit when the statistics are numpy's own).  SCALE, CONTRAST and RESTORE bit for bit; GAMMA by the
   measure of tests/test_intensity_gpu.py, max|got - f64| <= 4 max(max|f32 - f64|, ulp32(max|x|)).
 * mt_ensemble_classify: np.mean of the float16 members, np.argmax (the first NaN wins) or `> 0.5` painted in channel order with
   class_order & 255 (the label is a uint8).

Out of reach: `need = (V >> 30) + 1` of mt_seg_joint_hist wants a 1 GiB volume; nothing above INT32_MAX voxels can run.
"""
import collections
import math
import os
import re

import numpy as np

F32_SENTINEL_BITS = 0x7fc0dead
INT_SENTINEL = -12345
BYTE_SENTINEL = 0x77
SD_ULPS = 2
MEAN_BOUND, SD_BOUND, GAMMA_RATIO = 1e-10, 1e-8, 4.0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'multitalent_amd', 'csrc')
INCLUDE = os.path.join(ROOT, 'include', 'mtseg.h')
UNITS = ('metrics.hip', 'postproc.hip', 'intensity.hip', 'ensemble.hip')
OP_NONE, OP_SCALE, OP_CONTRAST, OP_GAMMA, OP_RESTORE = range(5)
OP_NAMES = {OP_SCALE: 'MT_INTENSITY_SCALE', OP_CONTRAST: 'MT_INTENSITY_CONTRAST', OP_GAMMA: 'MT_INTENSITY_GAMMA', OP_RESTORE: 'MT_INTENSITY_RESTORE'}
PRESERVE, NEGATE = 1, 2

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


def _match(text, pattern, what):
    m = re.search(pattern, text)
    assert m, what
    return int(m.group(1))


Geo = collections.namedtuple('Geo', 'cus cap mx_threads sd_chunk sd_rchunk lds_maxc brick cc_threads brick_cap rows_mul query_mul ia_threads '
                                    'ia_stat_quads ia_chunk ens_vox ens_max')


def geometry(cus):
    """the launch geometry out of the sources, for a device of `cus` compute units"""
    stream, mx, pp, ia, en, head = read('stream_common.h'), read('metrics.hip'), read('postproc.hip'), read('intensity.hip'), read('ensemble.hip'), \
        open(INCLUDE).read()
    per_cu = _match(stream, r'mt_stream_cap\(\)\s*\{\s*return\s+mt_device_cus\(mt_current_device\(\)\)\s*\*\s*(\d+);', 'mt_stream_cap')
    return Geo(cus=cus, cap=cus * per_cu, mx_threads=_define(mx, 'MX_THREADS'), sd_chunk=_define(mx, 'SD_CHUNK'), sd_rchunk=_define(mx, 'SD_RCHUNK'),
               lds_maxc=_define(mx, 'SH_LDS_MAXC'), brick=(_define(pp, 'CC_BD'), _define(pp, 'CC_BH'), _define(pp, 'CC_BW')),
               cc_threads=_define(pp, 'CC_THREADS'), brick_cap=1 << _match(pp, r'nb < \(1L << (\d+)\)', 'brick cap'),
               rows_mul=_match(mx, r'rgrid > cap_blocks \* (\d+)', 'rows grid'), query_mul=_match(mx, r'qgrid > cap_blocks \* (\d+)', 'query grid'),
               ia_threads=_define(ia, 'IA_THREADS'), ia_stat_quads=_define(ia, 'IA_STAT_QUADS'), ia_chunk=_define(ia, 'IA_CHUNK'),
               ens_vox=_define(en, 'MT_ENS_VOX'), ens_max=_define(head, 'MT_ENSEMBLE_MAX_MEMBERS'))


def kernels_in_sources():
    """{unit: [names of its __global__ functions]}"""
    out = {}
    for unit in UNITS:
        out[unit] = re.findall(r'__global__\s+(?:__launch_bounds__\(\w+\)\s+)?void\s+(\w+)\s*\(', read(unit))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def ulps64(got, ref):
    """|got - ref| in units of the reference's last place (finite float64 arrays)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.spacing(np.abs(ref))


# ================================================================================================================================
# A. mt_seg_joint_hist
def hist_split(a, b, V):
    """(head, vector, tail) voxel counts of mt_seg_joint_hist for pointers a and b bytes past a 16-byte boundary"""
    head = (16 - a) & 15
    head = min(head, V)
    if (b + head) & 15 == 0:
        nvec = (V - head) // 16
    else:
        head, nvec = 0, 0
    return head, 16 * nvec, V - head - 16 * nvec


def hist_trip(geo):
    return 16 * geo.mx_threads * geo.cap


def hist_cases(geo):
    out = [Case('hist-V%d' % V, 'mt_seg_joint_hist', dict(V=V, a=0, b=0, C=3, remap='id', fill='mix')) for V in (1, 15, 16, 17, 31)]
    for a in (0, 1, 15):
        for b in (0, 1, 15):
            h = (16 - a) & 15
            for V in sorted({5, max(h, 1), h + 16, h + 16 + 3, 100}):
                out.append(Case('hist-a%d-b%d-V%d' % (a, b, V), 'mt_seg_joint_hist', dict(V=V, a=a, b=b, C=4, remap='many', fill='mix')))
    out.append(Case('hist-head-clamped-to-V', 'mt_seg_joint_hist', dict(V=5, a=1, b=11, C=4, remap='many', fill='mix')))      # head 15 > V, ref + V aligned
    for C in (1, 2, 64, 65, 256):
        out.append(Case('hist-C%d' % C, 'mt_seg_joint_hist', dict(V=1003, a=3, b=3, C=C, remap='id', fill='all')))
    out.append(Case('hist-many-to-one', 'mt_seg_joint_hist', dict(V=1003, a=0, b=0, C=5, remap='many', fill='all')))
    out.append(Case('hist-zero-moved', 'mt_seg_joint_hist', dict(V=1003, a=2, b=2, C=7, remap='zero-moved', fill='all')))
    out.append(Case('hist-zero-moved-C65', 'mt_seg_joint_hist', dict(V=1003, a=2, b=2, C=65, remap='zero-moved', fill='all')))
    for remap in ('id', 'zero-moved'):
        out.append(Case('hist-background-%s' % remap, 'mt_seg_joint_hist', dict(V=1003, a=5, b=5, C=3, remap=remap, fill='zero')))
    for j in range(16):
        out.append(Case('hist-one-voxel-byte%d' % j, 'mt_seg_joint_hist', dict(V=64, a=0, b=0, C=3, remap='id', fill='one', at=16 + j, side=j % 2)))
    out.append(Case('hist-trip2', 'mt_seg_joint_hist', dict(V=hist_trip(geo) + 16 + 3, a=0, b=0, C=5, remap='many', fill='sparse', trip2=True)))
    return out


def hist_remap(kind, C):
    k = np.arange(256)
    if kind == 'id':
        return (k % C).astype(np.uint8)
    if kind == 'many':
        return ((k * 7 + 3) % C).astype(np.uint8)         # remap[0] = 3 % C
    r = (k % C).astype(np.uint8)
    r[0] = C - 1
    return r


def hist_build(c, geo):
    p, r = c.p, rng(c.id)
    V, C = p['V'], p['C']
    if p['fill'] == 'zero':
        t, q = np.zeros(V, np.uint8), np.zeros(V, np.uint8)
    elif p['fill'] == 'one':
        t, q = np.zeros(V, np.uint8), np.zeros(V, np.uint8)
        (q if p['side'] else t)[p['at']] = 2
    elif p['fill'] == 'sparse':
        t, q = np.zeros(V, np.uint8), np.zeros(V, np.uint8)
        at = np.arange(0, V, 4099)
        t[at], q[at[::2]] = 1 + at % 4, 2
        t[hist_trip(geo):], q[hist_trip(geo):] = r.randint(0, 5, V - hist_trip(geo)), r.randint(0, 5, V - hist_trip(geo))
    else:
        hi = 256 if p['fill'] == 'all' else 4
        t = (r.randint(0, hi, V) * (r.uniform(size=V) < 0.5)).astype(np.uint8)
        q = (r.randint(0, hi, V) * (r.uniform(size=V) < 0.5)).astype(np.uint8)
    remap = hist_remap(p['remap'], C)
    ref = np.bincount(remap[t].astype(np.int64) * C + remap[q], minlength=C * C).astype(np.int64)
    return dict(t=t, r=q, V=V, C=C, remap=remap, ref=ref)


# ================================================================================================================================
# B. mt_surface_distances
DYADIC = ((1.0, 0.5, 2.5), (0.75, 1.0, 0.5), (2.5, 0.75, 1.0))
RAGGED = (0.8, 0.7, 3.3)


def is_dyadic(sp):
    return all(float(s * 4).is_integer() for s in sp)


def sd_cases(geo):
    E = 'mt_surface_distances'
    out = []
    for conn in (1, 2, 3):
        out.append(Case('sd-conn%d' % conn, E, dict(kind='blobs', shape=(7, 9, 11), conn=conn, sp=DYADIC[conn - 1])))
        out.append(Case('sd-conn%d-ragged' % conn, E, dict(kind='blobs', shape=(7, 9, 11), conn=conn, sp=RAGGED)))
    for shape in ((1, 9, 11), (7, 1, 11), (7, 9, 1), (1, 1, 13), (1, 1, 1)):
        out.append(Case('sd-%dx%dx%d' % shape, E, dict(kind='blobs', shape=shape, conn=1 + sum(shape) % 3, sp=DYADIC[0])))
    for W in (63, 64, 65, 129):
        out.append(Case('sd-far-words-W%d' % W, E, dict(kind='far', shape=(2, 3, W), conn=1, sp=(100.0, 100.0, 0.5))))
    out.append(Case('sd-left-right-tie', E, dict(kind='tie', shape=(1, 1, 9), conn=1, sp=DYADIC[0])))
    out.append(Case('sd-test-empty', E, dict(kind='blobs', shape=(5, 6, 7), conn=1, sp=DYADIC[0], empty='t')))
    out.append(Case('sd-ref-empty', E, dict(kind='blobs', shape=(5, 6, 7), conn=2, sp=DYADIC[0], empty='r')))
    out.append(Case('sd-both-empty', E, dict(kind='blobs', shape=(5, 6, 7), conn=1, sp=DYADIC[0], empty='tr')))
    out.append(Case('sd-joint-member', E, dict(kind='blobs', shape=(7, 9, 11), conn=1, sp=DYADIC[2], member=(2, 3))))
    for n, shape, drop in ((4095, (2, 1024, 2), 1), (4096, (2, 1024, 2), 0), (4097, (3, 683, 2), 1), (8193, (17, 241, 2), 1)):
        out.append(Case('sd-n%d' % n, E, dict(kind='planes', shape=shape, drop=drop, conn=1, sp=DYADIC[1], n=n)))
    for name in ('1', 'nA-1', 'nA', 'nA+1', 'n-1', 'n'):
        out.append(Case('sd-capacity-%s' % name, E, dict(kind='blobs', shape=(7, 9, 11), conn=1, sp=DYADIC[0], capacity=name, seed='sd-capacity')))
    out.append(Case('sd-capacity-4097-of-8193', E, dict(kind='planes', shape=(17, 241, 2), drop=1, conn=1, sp=DYADIC[1], n=8193, capacity=4097)))
    rows = 4 * geo.rows_mul * geo.cap
    # the reduce chunks are counted per direction: a second trip of sd_reduce1_kernel needs D H, not 2 D H, above 4096 cap
    for name, dh in (('rows', rows + 5), ('query', geo.mx_threads * geo.query_mul * geo.cap // 2 + 3), ('reduce', geo.sd_rchunk * geo.cap + 3)):
        H = 64 if name == 'rows' else 2048
        out.append(Case('sd-loop-%s' % name, E, dict(kind='loop', shape=(-(-dh // H), H, 2), conn=1, sp=(2.5, 0.75, 0.5), trip2=name)))
    return out


def sd_borders(mask, conn):
    from scipy import ndimage
    if not mask.any():
        return np.zeros_like(mask)
    return mask ^ ndimage.binary_erosion(mask, ndimage.generate_binary_structure(3, conn))


def sd_brute(ba, bb, sp):
    """for every border voxel of ba, in linear order, the distance to the nearest voxel of bb (float64, the written order)"""
    pa, pb = np.argwhere(ba).astype(np.float64), np.argwhere(bb).astype(np.float64)
    if pb.shape[0] == 0:
        return np.full(pa.shape[0], np.inf)
    out = np.empty(pa.shape[0])
    for i in range(0, pa.shape[0], 512):
        d = pa[i:i + 512, None, :] - pb[None, :, :]
        tz, ty, tx = d[..., 0] * sp[0], d[..., 1] * sp[1], d[..., 2] * sp[2]
        out[i:i + 512] = np.sqrt((tz * tz + ty * ty + tx * tx).min(1))
    return out


def sd_volumes(c, geo):
    """(test, ref, member) of the case"""
    p = c.p
    r = rng(p.get('seed', c.id))
    shape = p['shape']
    member = np.zeros(256, np.uint8)
    member[list(p.get('member', range(1, 256)))] = 1
    if p['kind'] == 'blobs':
        def blob(lo_frac):
            m = r.uniform(size=shape) < 0.3
            lo = [int(n * lo_frac) for n in shape]
            m[lo[0]:lo[0] + max(1, shape[0] // 2), lo[1]:lo[1] + max(1, shape[1] // 2), lo[2]:lo[2] + max(1, shape[2] // 2)] = True
            return m
        lab = p.get('member', (1,))
        t = np.where(blob(0.1), r.choice(lab, size=shape), r.choice([0, 9], size=shape) if 'member' in p else 0).astype(np.uint8)
        q = np.where(blob(0.4), r.choice(lab, size=shape), r.choice([0, 9], size=shape) if 'member' in p else 0).astype(np.uint8)
        if 'member' in p:
            member[9] = 0
        if 't' in p.get('empty', ''):
            t[:] = 0
        if 'r' in p.get('empty', ''):
            q[:] = 0
    elif p['kind'] == 'far':
        W = shape[2]
        t, q = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
        t[0, 0, 0] = t[1, 2, W - 1] = 1
        q[0, 0, W - 1] = q[1, 2, 0] = 1
    elif p['kind'] == 'tie':
        t, q = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
        t[0, 0, 4] = 1
        q[0, 0, 2] = q[0, 0, 6] = 1
    else:                                                # planes / loop: test is the plane x = 0, ref the plane x = 1
        t, q = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
        t[:, :, 0], q[:, :, 1] = 1, 1
        if p.get('drop'):
            q[0, 0, 1] = 0
    return t, q, member


def sd_build(c, geo):
    p = c.p
    t, q, member = sd_volumes(c, geo)
    sp = p['sp']
    if p['kind'] == 'loop':                              # closed form: every voxel is a border voxel at distance sx
        assert sp[2] <= sp[0] and sp[2] <= sp[1]
        n = int(t.sum())
        return dict(t=t, r=q, member=member, sp=sp, conn=p['conn'], nA=n, nB=n, capacity=2 * n, out=None, value=sp[2], dyadic=True)
    ba, bb = sd_borders(member[t] != 0, p['conn']), sd_borders(member[q] != 0, p['conn'])
    nA, nB = int(ba.sum()), int(bb.sum())
    out = np.concatenate([sd_brute(ba, bb, sp), sd_brute(bb, ba, sp)])
    cap = p.get('capacity', 'n')
    capacity = cap if isinstance(cap, int) else max(1, {'1': 1, 'nA-1': nA - 1, 'nA': nA, 'nA+1': nA + 1, 'n-1': nA + nB - 1, 'n': nA + nB}[cap])
    return dict(t=t, r=q, member=member, sp=sp, conn=p['conn'], nA=nA, nB=nB, capacity=capacity, out=out, ba=ba, bb=bb, dyadic=is_dyadic(sp))


def sd_stats_ref(stored, nA, nB, capacity):
    """(count, max, fsum) per direction of the stored prefix"""
    a, b = stored[:min(nA, capacity)], stored[nA:min(nA + nB, capacity)]
    return [(n, float(x.max()) if x.size else 0.0, math.fsum(x)) for n, x in ((nA, a), (nB, b))]


# ================================================================================================================================
# C. mt_cc_label3d / mt_cc_remove
def cc_ref(mask):
    """(labels, sizes, (components, largest)) from scipy's labelling"""
    from scipy import ndimage
    lab, n = ndimage.label(mask)
    flat = lab.ravel()
    V = flat.size
    labels, sizes = np.full(V, -1, np.int32), np.zeros(V, np.int32)
    if n:
        _, first = np.unique(flat, return_index=True)
        first = first[1:] if flat.min() == 0 else first              # label 0 is the background
        lut = np.concatenate([[-1], first]).astype(np.int32)
        labels = lut[flat]
        sizes[first] = np.bincount(flat, minlength=n + 1)[1:]
    return labels, sizes, (n, int(sizes.max()) if n else 0)


def remove_ref(seg, labels, sizes, largest, vpv, use_min, min_size):
    """the header's rule with Python floats -> (seg after, largest removed count)"""
    out, removed = seg.ravel().copy(), 0
    max_size = float(largest) * vpv
    for root in np.flatnonzero(sizes):
        cnt = int(sizes[root])
        size = float(cnt) * vpv
        if size != max_size and (not use_min or size < min_size):
            out[labels == root] = 0
            removed = max(removed, cnt)
    return out.reshape(seg.shape), removed


def column_runs(n):
    """closed form of the long columns: runs of 7 voxels every 11 -> (mask, labels, sizes, (components, largest))"""
    i = np.arange(n, dtype=np.int64)
    mask = (i % 11) < 7
    labels = np.where(mask, i - i % 11, -1).astype(np.int32)
    sizes = np.zeros(n, np.int32)
    starts = np.arange(0, n, 11)
    sizes[starts] = np.minimum(7, n - starts)
    return mask, labels, sizes, (starts.size, 7)


def cc_cases(geo):
    E = 'mt_cc_label3d'
    bd, bh, bw = geo.brick
    out = []
    for axis, b in enumerate(geo.brick):
        for n in (1, b - 1, b, b + 1, 2 * b + 1):
            shape = [bd + 1, bh + 1, bw + 1]
            shape[axis] = n
            out.append(Case('cc-axis%d-%d' % (axis, n), E, dict(kind='random', shape=tuple(shape), member=(1,))))
    for kind in ('faces', 'corner', 'diagonal', 'comb', 'serpentine', 'full', 'empty'):
        out.append(Case('cc-%s' % kind, E, dict(kind=kind, shape=(2 * bd, 2 * bh, 2 * bw), member=(1,))))
    for name, member in (('255', (255,)), ('1-2', (1, 2)), ('0', (0,))):
        out.append(Case('cc-member-%s' % name, E, dict(kind='random', shape=(bd + 1, bh + 1, bw + 1), member=member)))
    out.append(Case('cc-column-d', E, dict(kind='column', shape=(bd * geo.brick_cap + 9, 1, 1), member=(1,), trip2=True)))
    out.append(Case('cc-column-w', E, dict(kind='column', shape=(1, 1, bw * geo.brick_cap + 17), member=(1,), trip2=True)))
    out.append(Case('cc-flat-trip2', E, dict(kind='random', shape=(geo.cap + 1, 16, 16), member=(1,), trip2=True, remove=(1.0, 1, 40.0))))
    R = 'mt_cc_remove'
    out.append(Case('rm-three-tied', R, dict(kind='lines', shape=(6, 7, 9), member=(1,), sizes=(5, 5, 5, 3, 2, 1), remove=(0.3, 0, 0.0))))
    for name, k in (('at', 0), ('above', 1), ('below', -1)):
        out.append(Case('rm-min-size-%s-3x0.3' % name, R, dict(kind='lines', shape=(6, 7, 9), member=(1,), sizes=(5, 5, 4, 3, 3, 2, 1), remove=(0.3, 1, ('c', 3, k)))))
    out.append(Case('rm-large-min-size', R, dict(kind='lines', shape=(6, 7, 9), member=(1,), sizes=(6, 4, 3, 2), remove=(0.3, 1, 1e9))))
    out.append(Case('rm-all-kept', R, dict(kind='lines', shape=(6, 7, 9), member=(1,), sizes=(4, 4, 4), remove=(2.0, 1, 100.0))))
    out.append(Case('rm-one-component', R, dict(kind='lines', shape=(6, 7, 9), member=(1,), sizes=(7,), remove=(1.0, 0, 0.0))))
    out.append(Case('rm-empty', R, dict(kind='empty', shape=(6, 7, 9), member=(1,), remove=(1.0, 1, 5.0))))
    return out


def cc_volume(c, geo):
    p, r = c.p, rng(c.id)
    shape, kind = p['shape'], p['kind']
    bd, bh, bw = geo.brick
    m = np.zeros(shape, bool)
    if kind == 'random':
        seg = r.choice(np.array([0, 1, 2, 255], np.uint8), size=shape, p=[0.35, 0.45, 0.1, 0.1])
        return seg
    if kind == 'faces':                                  # three components, each across exactly one face
        m[bd - 2:bd + 2, 3, 3] = m[3, bh - 2:bh + 2, 7] = m[5, 5, bw - 2:bw + 2] = True
    elif kind == 'corner':                               # round a brick corner through face neighbours only
        m[bd - 1, bh - 1, bw - 1] = m[bd, bh - 1, bw - 1] = m[bd, bh, bw - 1] = m[bd, bh, bw] = True
    elif kind == 'diagonal':                             # two voxels that touch only diagonally across each face: six components
        m[3, bh - 1, 5] = m[3, bh, 6] = m[bd - 1, 2, 2] = m[bd, 3, 2] = m[6, 9, bw - 1] = m[7, 9, bw] = True
    elif kind == 'comb':
        m[0, 0, 0:bw:2], m[0, 1, 0:bw] = True, True      # teeth, then the spine in a later row
        m[0, 4, 0:bw], m[0, 5, 1:bw:2] = True, True      # the spine first
        m[2, 8, 0:bw] = True
        m[3, 8, 0:bw:3] = True                           # teeth in the next slice
        m[5, 3, 0] = m[5, 3, 4] = True
        m[5, 4, 0:5] = True                              # a U
        m[6, 12, 2:9], m[7, 12, 2], m[7, 12, 8] = True, True, True        # a U through the previous slice
        m[1, 10, 0:bw:2] = True                          # teeth that nothing joins
    elif kind == 'serpentine':                           # a snake through every other slice of one brick, the slices joined at one corner
        for d in range(0, bd, 2):
            for h in range(bh):
                if h % 2 == 0:
                    m[d, h, 0:bw] = True
                else:
                    m[d, h, bw - 1 if (h // 2) % 2 == 0 else 0] = True
            m[d + 1, bh - 1, bw - 1 if ((bh - 1) // 2) % 2 == 0 else 0] = True
    elif kind == 'full':
        m[:] = True
    elif kind == 'lines':                                # components of the given sizes: straight lines along w, two rows apart
        rows = [(d, h) for d in range(0, shape[0], 2) for h in range(0, shape[1], 2)]
        for (d, h), n in zip(rows, p['sizes']):
            m[d, h, 1:1 + n] = True
    return m.astype(np.uint8)


def cc_build(c, geo):
    p = c.p
    member = np.zeros(256, np.uint8)
    member[list(p['member'])] = 1
    if p['kind'] == 'column':
        mask, labels, sizes, stats = column_runs(int(np.prod(p['shape'])))
        seg = mask.astype(np.uint8).reshape(p['shape'])
    else:
        seg = cc_volume(c, geo)
        labels, sizes, stats = cc_ref(member[seg] != 0)
    d = dict(seg=seg, member=member, labels=labels, sizes=sizes, stats=stats)
    if 'remove' in p:
        vpv, use_min, ms = p['remove']
        if isinstance(ms, tuple):                        # the product c * vpv itself, or the double above / below it
            prod = float(ms[1]) * vpv
            ms = prod if ms[2] == 0 else float(np.nextafter(prod, np.inf if ms[2] > 0 else -np.inf))
        d['remove'] = (vpv, use_min, ms)
        d['seg_after'], d['removed'] = remove_ref(seg, labels, sizes, stats[1], vpv, use_min, ms)
    return d


# ================================================================================================================================
# D. mt_fill_holes3d
def fh_cases(geo):
    E = 'mt_fill_holes3d'
    bd, bh, bw = geo.brick
    big = (2 * bd + 2, 2 * bh + 2, 2 * bw + 2)
    out = [Case('fh-%s' % k, E, dict(kind=k, shape=big if k != 'one-brick' else (6, 9, 10), off=0, vals=(1,)))
           for k in ('one-brick', 'eight-bricks', 'tunnel', 'diagonal-leak', 'two-cavities', 'zeros', 'ones', 'box-on-the-faces')]
    for axis in range(3):
        shape = [5, 7, 9]
        shape[axis] = 1
        out.append(Case('fh-axis%d-of-1' % axis, E, dict(kind='random', shape=tuple(shape), off=0, vals=(1,))))
    for name, vals in (('01', (1,)), ('0-255', (255,)), ('0-7-200', (7, 200))):
        out.append(Case('fh-values-%s' % name, E, dict(kind='random', shape=(7, 8, 9), off=0, vals=vals)))
    for off in (0, 1, 8):
        for shape in ((4, 4, 5), (3, 3, 9), (5, 5, 7)):
            out.append(Case('fh-off%d-Vmod16-%d' % (off, np.prod(shape) % 16), E, dict(kind='random', shape=shape, off=off, vals=(3,))))
    out.append(Case('fh-alternating-chunk', E, dict(kind='alternating', shape=(3, 3, 16), off=0, vals=(1,))))
    out.append(Case('fh-column', E, dict(kind='column', shape=(bd * geo.brick_cap + 9, 1, 1), off=0, vals=(7,), trip2=True)))
    n = 1
    while 2 * n * n + 6 * n < geo.cc_threads * geo.cap:      # the W faces of (3, n, n) are numbered beyond 256 cap: only a second trip marks them
        n += 1
    out.append(Case('fh-faces-trip2', E, dict(kind='late-face', shape=(3, n, n), off=0, vals=(1,), trip2=True)))
    out.append(Case('fh-fill-trip2', E, dict(kind='shell', shape=(-(-(16 * geo.cc_threads * geo.cap + 1) // 4096) + 1, 64, 64), off=0, vals=(1,), trip2=True)))
    return out


def fh_build(c, geo, full=True):
    from scipy import ndimage
    p, r = c.p, rng(c.id)
    shape, kind = p['shape'], p['kind']
    D, H, W = shape
    bd, bh, bw = geo.brick
    m = np.zeros(shape, bool)
    closed = None
    if kind == 'one-brick':
        m[1:5, 1:8, 1:9] = True
        m[2:4, 2:7, 2:8] = False
    elif kind == 'eight-bricks':
        m[bd - 3:bd + 4, bh - 3:bh + 4, bw - 3:bw + 4] = True
        m[bd - 2:bd + 3, bh - 2:bh + 3, bw - 2:bw + 3] = False
    elif kind == 'tunnel':                               # the cavity reaches the face d = 0 through one voxel
        m[2:bd + 4, 2:bh + 4, 2:bw + 4] = True
        m[3:bd + 3, 3:bh + 3, 3:bw + 3] = False
        m[0:3, 5, 5] = False
    elif kind == 'diagonal-leak':                        # an edge voxel of the shell is missing: open only diagonally
        m[2:bd + 4, 2:bh + 4, 2:bw + 4] = True
        m[3:bd + 3, 3:bh + 3, 3:bw + 3] = False
        m[2, 2, 5] = False
    elif kind == 'two-cavities':
        m[1:6, 1:6, 1:6] = m[bd:bd + 6, bh:bh + 6, bw:bw + 6] = True
        m[2:5, 2:5, 2:5] = m[bd + 1:bd + 5, bh + 1:bh + 5, bw + 2:bw + 4] = False
    elif kind == 'ones':
        m[:] = True
    elif kind == 'box-on-the-faces':
        m[:] = True
        m[1:-1, 1:-1, 1:-1] = False
    elif kind == 'random':
        m = r.uniform(size=shape) < 0.75
    elif kind == 'shell':                                # a hollow box one voxel inside the volume: the result is the solid box
        m[1:-1, 1:-1, 1:-1] = True
        m[2:-2, 2:-2, 2:-2] = False
        closed = np.zeros(shape, np.uint8)
        closed[1:-1, 1:-1, 1:-1] = 1
    elif kind == 'alternating':
        m[:] = True
        m[1, 1, 0:16:2] = False                          # w = 0 lies on a face (outside), w = 2 .. 14 are cavities
        m[1, 1, 15] = False                              # and the row ends on a face again
    elif kind == 'column':
        m[:, 0, 0] = (np.arange(D) % 11) < 7
        closed = m.astype(np.uint8)
    elif kind == 'late-face':                            # solid but for a cavity and a tunnel that reaches only the face w = W - 1
        m[:] = True
        m[1, 5, 5] = False
        m[1, H // 2, W - 5:] = False
        closed = m.astype(np.uint8)
        closed[1, 5, 5] = 1
    vals = np.array(p['vals'], np.uint8)
    mask = np.where(m, vals[r.randint(0, vals.size, shape)], 0).astype(np.uint8)
    V = int(np.prod(shape))
    ref = ndimage.binary_fill_holes(mask != 0).astype(np.uint8) if closed is None or (full and V <= 200000) else closed
    if closed is not None:
        assert ref is closed or np.array_equal(ref, closed), c.id
    nz = np.nonzero(ref)
    count = int(nz[0].size)
    bbox = [int(v) for a in nz for v in (a.min(), a.max() + 1)] if count else [0] * 6
    return dict(mask=mask, ref=ref, bbox=bbox, count=count)


# ================================================================================================================================
# E. mt_channel_stats
def stats_trip(geo):
    return 4 * geo.ia_threads * geo.ia_stat_quads * geo.cap


SPECIAL = ('constant', 'mean1e4-sd1e-2', 'denormals', 'pinf', 'ninf', 'bothinf', 'nan-first', 'nan-later', 'nan-and-inf', 'plain')


def stats_cases(geo):
    E = 'mt_channel_stats'
    out = [Case('stats-V%d' % V, E, dict(NC=1, V=V, active='all', kind='plain')) for V in (1, 2, 3, 4, 5, 7, 1023, 1024, 1025)]
    out += [Case('stats-odd-V%d-NC3' % V, E, dict(NC=3, V=V, active='all', kind='plain')) for V in (7, 1025)]
    for NC in (1, 64, 65, 130):
        out.append(Case('stats-NC%d' % NC, E, dict(NC=NC, V=37, active='all', kind='plain')))
    for bit in (0, 63, 64, 129):
        out.append(Case('stats-only-channel-%d' % bit, E, dict(NC=130, V=37, active=(bit,), kind='plain')))
    out.append(Case('stats-chunk-edges', E, dict(NC=130, V=37, active=(0, 63, 64, 129), kind='plain')))
    out.append(Case('stats-none-active', E, dict(NC=65, V=37, active=(), kind='plain')))
    out.append(Case('stats-special', E, dict(NC=len(SPECIAL), V=1025, active='all', kind='special')))
    out.append(Case('stats-special-V3', E, dict(NC=len(SPECIAL), V=3, active='all', kind='special')))
    out.append(Case('stats-trip2', E, dict(NC=1, V=stats_trip(geo) + 5, active='all', kind='plain', trip2=True)))
    return out


def stats_ref(x):
    """(min, max, mean, sd, max|x| of the finite part): numpy's min / max, math.fsum moments; numpy's own values when not finite"""
    x64 = np.asarray(x, np.float64)
    fin = x64[np.isfinite(x64)]
    scale = float(np.abs(fin).max()) if fin.size else 0.0
    with np.errstate(invalid='ignore'):
        lo, hi = float(np.min(x)), float(np.max(x))
        if fin.size != x64.size:
            return lo, hi, float(x64.mean()), float(x64.std()), scale
    n = x64.size
    mean = math.fsum(x64) / n
    d = x64 - mean
    return lo, hi, mean, math.sqrt(math.fsum(d * d) / n), scale


def stats_build(c, geo):
    p, r = c.p, rng(c.id)
    NC, V = p['NC'], p['V']
    x = (r.standard_normal((NC, V)) * (1 + np.arange(NC)[:, None] % 5) + (np.arange(NC)[:, None] % 7 - 3) * 10).astype(np.float32)
    if p['kind'] == 'special':
        for ch, kind in enumerate(SPECIAL):
            at = min(V - 1, 517)
            if kind == 'constant':
                x[ch] = 3.0
            elif kind == 'mean1e4-sd1e-2':
                x[ch] = (1e4 + 1e-2 * r.standard_normal(V)).astype(np.float32)
            elif kind == 'denormals':
                x[ch] = (r.randint(1, 2 ** 23, V).astype(np.uint32) | (r.randint(0, 2, V).astype(np.uint32) << 31)).view(np.float32)
            elif kind == 'pinf':
                x[ch, at] = np.inf
            elif kind == 'ninf':
                x[ch, at] = -np.inf
            elif kind == 'bothinf':
                x[ch, at], x[ch, 0] = np.inf, -np.inf
            elif kind == 'nan-first':
                x[ch, 0] = np.nan
            elif kind == 'nan-later':
                x[ch, at] = np.nan
            elif kind == 'nan-and-inf':
                x[ch, 0], x[ch, at] = np.inf, np.nan
    active = np.ones(NC, np.uint8) if p['active'] == 'all' else np.zeros(NC, np.uint8)
    if p['active'] != 'all':
        active[list(p['active'])] = 1
    refs = [stats_ref(x[ch]) if active[ch] else None for ch in range(NC)]
    return dict(x=x, NC=NC, V=V, active=active, refs=refs)


# ================================================================================================================================
# F. mt_intensity_apply
def apply_trip(geo):
    return 4 * geo.ia_threads * geo.cap


def apply_ref(x, op, flags, a, b, st, st2, dtype=np.float32):
    """the arithmetic of tests/intensity_restatement.py (brightness_one, contrast_one, gamma_one) in `dtype`, the statistics (min, max,
    mean, sd) given.  That module computes its statistics from the array itself, and the kernel reads them from device memory, so its
    functions cannot be called with the statistics a launch really used: this is their arithmetic with the statistics as arguments.
    tests/test_volume_cases_cpu.py::test_apply_reference_is_the_restatement holds the two together bit for bit (float32 and float64,
    every op and flag); change one and that test says so."""
    f = dtype
    x = x.astype(f)
    if op == OP_NONE:
        return x
    if op == OP_SCALE:
        return x * f(a)
    mn, mx, mean, sd = (f(v) for v in st)
    if op == OP_CONTRAST:
        y = (x - mean) * f(a) + mean
        return np.clip(y, mn, mx) if flags & PRESERVE else y
    neg = bool(flags & NEGATE)
    if neg:
        x, mn, mx, mean = -x, -mx, -mn, -mean
    if op == OP_GAMMA:
        rge = mx - mn
        with np.errstate(invalid='ignore', divide='ignore'):
            y = np.power((x - mn) / (rge + f(b)), f(a)) * rge + mn
    else:
        mean1, sd1 = f(st2[2]), f(st2[3])
        if neg:
            mean1 = -mean1
        y = (x - mean1) / (sd1 + f(1e-8)) * sd + mean
    return -y if neg else y


ALL_OPS = ((OP_SCALE, 0, 1.25, 0.0), (OP_NONE, 0, 0.0, 0.0), (OP_CONTRAST, 0, 0.75, 0.0), (OP_CONTRAST, PRESERVE, 1.25, 0.0), (OP_GAMMA, 0, 0.7, 1e-7),
           (OP_GAMMA, NEGATE, 1.5, 1e-7), (OP_RESTORE, 0, 0.0, 0.0), (OP_RESTORE, NEGATE, 0.0, 0.0), (OP_NONE, 0, 0.0, 0.0))


def apply_cases(geo):
    E = 'mt_intensity_apply'
    out = []
    for V in (1, 3, 4, 5, 1025):
        for mode in ('device', 'hand'):
            out.append(Case('apply-all-ops-V%d-%s' % (V, mode), E, dict(V=V, records=ALL_OPS, stats=mode, kind='plain')))
    slots = {0: (OP_SCALE, 0, 0.8, 0.0), 63: (OP_CONTRAST, PRESERVE, 1.25, 0.0), 64: (OP_GAMMA, NEGATE, 0.7, 1e-7), 129: (OP_RESTORE, 0, 0.0, 0.0)}
    out.append(Case('apply-slots-0-63-64-129', E, dict(V=37, records=tuple(slots.get(i, (OP_NONE, 0, 0.0, 0.0)) for i in range(130)), stats='device', kind='plain')))
    out.append(Case('apply-constant-channel', E, dict(V=1025, records=((OP_GAMMA, 0, 0.7, 1e-7), (OP_GAMMA, NEGATE, 0.0, 1e-7), (OP_RESTORE, 0, 0.0, 0.0),
                                                                         (OP_RESTORE, NEGATE, 0.0, 0.0), (OP_CONTRAST, PRESERVE, 1.25, 0.0)),
                                                      stats='device', kind='constant')))
    out.append(Case('apply-gamma-exponents', E, dict(V=1025, records=tuple((OP_GAMMA, fl, a, 1e-7) for a in (0.0, 1.0, 0.7, 1.5) for fl in (0, NEGATE)),
                                                     stats='hand', kind='plain')))
    out.append(Case('apply-preserve-range-clamps', E, dict(V=1025, records=((OP_CONTRAST, PRESERVE, 1.25, 0.0), (OP_CONTRAST, 0, 1.25, 0.0),
                                                                              (OP_CONTRAST, PRESERVE, 3.0, 0.0)), stats='hand', kind='plain')))
    four = ((OP_SCALE, 0, 1.25, 0.0), (OP_CONTRAST, PRESERVE, 1.25, 0.0), (OP_GAMMA, NEGATE, 0.7, 1e-7), (OP_RESTORE, 0, 0.0, 0.0))
    # 1024 cap + 3 elements are 256 cap quads: one trip of the quad loop and a tail; the second trip starts with one quad more
    out.append(Case('apply-V1024cap+3', E, dict(V=apply_trip(geo) + 3, records=four[:2], stats='hand', kind='plain', trip2=True)))
    out.append(Case('apply-trip2', E, dict(V=apply_trip(geo) + 4 + 3, records=four, stats='hand', kind='plain', trip2=True)))
    return out


def np_stats(x, dtype=np.float64):
    x = x.astype(dtype)
    return np.array([x.min(), x.max(), x.mean(), x.std()], np.float64)


def apply_build(c, geo):
    """x, x2 (the stream stats2 is taken on), records and, for hand-written statistics, stats and stats2 as doubles that are no
    float32 values; the reference is `apply_expected`, evaluated with the statistics the launch really read"""
    p, r = c.p, rng(c.id)
    NC, V = len(p['records']), p['V']
    shift = ((np.arange(NC) % 5) - 2)[:, None] * 3.0
    x = (r.standard_normal((NC, V)) * (1 + np.arange(NC)[:, None] % 3) + shift).astype(np.float32)
    x2 = (r.standard_normal((NC, V)) * 0.5 + shift + 0.25).astype(np.float32)
    if p['kind'] == 'constant':
        x[:], x2[:] = np.float32(3.0), np.float32(-1.5)
    d = dict(x=x, x2=x2, NC=NC, V=V, records=p['records'])
    if p['stats'] == 'hand':
        d['stats'] = np.stack([np_stats(x[ch]) for ch in range(NC)])
        d['stats2'] = np.stack([np_stats(x2[ch]) for ch in range(NC)])
    return d


def apply_expected(d, stats, stats2):
    """per channel (float32 reference, float64 reference) for the statistics given (doubles; the kernel rounds them to float32 once)"""
    out = []
    for ch, (op, flags, a, b) in enumerate(d['records']):
        s32, t32 = stats[ch].astype(np.float32), stats2[ch].astype(np.float32)
        r32 = apply_ref(d['x'][ch], op, flags, a, b, s32, t32, np.float32)
        r64 = apply_ref(d['x'][ch], op, flags, a, b, stats[ch], stats2[ch], np.float64)
        assert r32.dtype == np.float32
        out.append((r32, r64))
    return out


def gamma_ratio(got, r32, r64, x):
    """max|got - f64| over max(max|f32 - f64|, ulp32(max|x|)): the measure of tests/test_intensity_gpu.py"""
    base = max(float(np.abs(r32.astype(np.float64) - r64).max()), float(np.spacing(np.float32(np.abs(x).max()))))
    return float(np.abs(got.astype(np.float64) - r64).max()) / base


# ================================================================================================================================
# G. mt_ensemble_classify: what tests/test_ensemble_gpu.py leaves open
def ens_trip(geo):
    return geo.ens_vox * 256 * geo.cap


def ens_cases(geo):
    E = 'mt_ensemble_classify'
    out = [Case('ens-trip2', E, dict(K=2, C=2, shape=(-(-(ens_trip(geo) + 1) // (64 * 64)), 64, 64), regions=0, wide=True, out_off=0, kind='plain', trip2=True)),
           Case('ens-K16-C255-V9', E, dict(K=geo.ens_max, C=255, shape=(1, 1, 9), regions=0, wide=True, out_off=0, kind='plain'))]
    for wide in (True, False):
        for out_off in (0, 4, 1):                        # one 8-byte store, two 4-byte stores, bytewise
            out.append(Case('ens-order-255-256-%s-out%d' % ('wide' if wide else 'narrow', out_off), E,
                            dict(K=2, C=3, shape=(2, 3, 16), regions=1, order=(255, 256, 515), wide=wide, out_off=out_off, kind='plain', mean=True)))
            if out_off != 4:
                out.append(Case('ens-nan-%s-out%d' % ('wide' if wide else 'narrow', out_off), E,
                                dict(K=2, C=3, shape=(2, 3, 16), regions=0, wide=wide, out_off=out_off, kind='nan', mean=True)))
    out.append(Case('ens-nan-regions', E, dict(K=2, C=3, shape=(2, 3, 16), regions=1, order=(1, 2, 3), wide=True, out_off=0, kind='nan', mean=True)))
    return out


def ens_build(c, geo):
    p, r = c.p, rng(c.id)
    K, C, shape = p['K'], p['C'], p['shape']
    V = int(np.prod(shape))
    members = [(r.randint(0, 9, (C, V)) / 8.0).astype(np.float16) for _ in range(K)]
    if 'order' in p and p['kind'] == 'plain':            # two whole groups of the first class alone: every byte of a packed store carries it
        for m in members:
            m[0, :16], m[1:, :16] = 1.0, 0.0
    if p['kind'] == 'nan':
        members[0][0, 0::5] = np.nan                     # channel 0
        members[1][1, 1::5] = np.nan                     # a later channel
        members[0][2, 2::5] = np.nan                     # the last one
        members[1][1, 3::10], members[1][2, 3::10] = np.nan, np.nan       # two NaNs: the first wins
    with np.errstate(invalid='ignore'):
        mean = np.mean(np.vstack([m[None] for m in members]), 0)
        assert mean.dtype == np.float16
        if p['regions']:
            lab = np.zeros(V, np.uint8)
            for i, o in enumerate(p['order']):
                lab[mean[i] > 0.5] = o & 255
        else:
            lab = np.argmax(mean, 0).astype(np.uint8)
    return dict(members=members, mean=mean, lab=lab.reshape(shape), V=V)


# ================================================================================================================================
FAMILIES = collections.OrderedDict((('hist', (hist_cases, hist_build)), ('sd', (sd_cases, sd_build)), ('cc', (cc_cases, cc_build)),
                                    ('fh', (fh_cases, fh_build)), ('stats', (stats_cases, stats_build)), ('apply', (apply_cases, apply_build)),
                                    ('ens', (ens_cases, ens_build))))


def cases(family, cus):
    return FAMILIES[family][0](geometry(cus))


def build(family, case, cus, **kw):
    return FAMILIES[family][1](case, geometry(cus), **kw)


def instances(case):
    """the kernels (with their template arguments) that the case's entry point launches"""
    e, p = case.entry, case.p
    if e == 'mt_seg_joint_hist':
        return ['seg_hist_kernel<%s>' % ('true' if p['C'] <= 64 else 'false')]
    if e == 'mt_surface_distances':
        return ['sd_border_kernel', 'sd_scan_kernel', 'sd_compact_kernel', 'sd_rows_kernel', 'sd_query_kernel', 'sd_reduce1_kernel', 'sd_reduce2_kernel']
    label = ['cc_local_kernel<true>', 'cc_merge_kernel', 'cc_flatten_kernel', 'cc_count_kernel']
    if e == 'mt_cc_label3d':
        return label + (['cc_remove_kernel'] if 'remove' in p else [])
    if e == 'mt_cc_remove':                              # always behind mt_cc_label3d
        return label + ['cc_remove_kernel']
    if e == 'mt_fill_holes3d':
        return ['cc_local_kernel<false>', 'cc_merge_kernel', 'cc_flatten_kernel', 'fh_mark_kernel', 'fh_fill_kernel']
    if e == 'mt_channel_stats':
        return ['channel_stats_kernel', 'channel_stats_finalize_kernel'] if p['active'] == 'all' or p['active'] else []
    if e == 'mt_intensity_apply':
        return ['intensity_apply_kernel'] + sorted({'ia_run<%s>' % OP_NAMES[r[0]] for r in p['records'] if r[0] != OP_NONE}) + \
            (['channel_stats_kernel', 'channel_stats_finalize_kernel'] if p['stats'] == 'device' else [])
    if e == 'mt_ensemble_classify':
        return ['ensemble_classify_kernel<%s>' % ('true' if p['wide'] else 'false')]
    raise KeyError(e)


def launchable_instances():
    """every kernel of the four units, with every template argument its entry point can pass (ia_run is the per-op loop of
    intensity_apply_kernel: a device function, listed because each op is its own instantiation of the stride loop)"""
    out = ['seg_hist_kernel<true>', 'seg_hist_kernel<false>', 'sd_border_kernel', 'sd_scan_kernel', 'sd_compact_kernel', 'sd_rows_kernel',
           'sd_query_kernel', 'sd_reduce1_kernel', 'sd_reduce2_kernel', 'cc_local_kernel<true>', 'cc_local_kernel<false>', 'cc_merge_kernel',
           'cc_flatten_kernel', 'cc_count_kernel', 'cc_remove_kernel', 'fh_mark_kernel', 'fh_fill_kernel', 'channel_stats_kernel',
           'channel_stats_finalize_kernel', 'intensity_apply_kernel']
    out += ['ia_run<%s>' % n for n in OP_NAMES.values()]
    out += ['ensemble_classify_kernel<true>', 'ensemble_classify_kernel<false>']
    return out


STRIDE_LOOPS = ('seg_hist_kernel:vectors', 'cc_local_kernel<true>:bricks', 'cc_local_kernel<false>:bricks', 'cc_merge_kernel:bricks',
                'cc_flatten_kernel:voxels', 'cc_count_kernel:voxels', 'cc_remove_kernel:voxels', 'sd_rows_kernel:rows', 'sd_query_kernel:entries',
                'sd_reduce1_kernel:chunks', 'fh_mark_kernel:faces', 'fh_fill_kernel:chunks', 'channel_stats_kernel:quads',
                'mt_channel_stats:IA_CHUNK', 'mt_intensity_apply:IA_CHUNK', 'ensemble_classify_kernel:groups') + \
    tuple('ia_run<%s>:quads' % n for n in OP_NAMES.values())


def second_trips(case, geo):
    """the grid-, brick- and chunk-stride loops that make a second trip in this case, from its sizes"""
    e, p = case.entry, case.p
    out = []
    cdiv = lambda a, b: -(-a // b)
    if e == 'mt_seg_joint_hist':
        if hist_split(p['a'], p['b'], p['V'])[1] // 16 > geo.mx_threads * geo.cap:
            out.append('seg_hist_kernel:vectors')
    elif e == 'mt_surface_distances' and p['kind'] == 'loop':
        D, H, W = p['shape']
        if D * H > 4 * geo.rows_mul * geo.cap:
            out.append('sd_rows_kernel:rows')
        if 2 * D * H > geo.mx_threads * geo.query_mul * geo.cap:
            out.append('sd_query_kernel:entries')
        if cdiv(D * H, geo.sd_rchunk) > min(cdiv(2 * D * H, geo.sd_rchunk) + 1, geo.cap):
            out.append('sd_reduce1_kernel:chunks')
    elif e in ('mt_cc_label3d', 'mt_cc_remove', 'mt_fill_holes3d'):
        D, H, W = p['shape']
        V = D * H * W
        count = 'true' if e != 'mt_fill_holes3d' else 'false'
        if cdiv(D, geo.brick[0]) * cdiv(H, geo.brick[1]) * cdiv(W, geo.brick[2]) > geo.brick_cap:
            out += ['cc_local_kernel<%s>:bricks' % count, 'cc_merge_kernel:bricks']
        if V > geo.cc_threads * geo.cap:
            out.append('cc_flatten_kernel:voxels')
            if e != 'mt_fill_holes3d':
                out += ['cc_count_kernel:voxels'] + (['cc_remove_kernel:voxels'] if 'remove' in p else [])
        if e == 'mt_fill_holes3d':
            if 2 * (H * W + D * W + D * H) > geo.cc_threads * geo.cap:
                out.append('fh_mark_kernel:faces')
            if cdiv(V, 16) > geo.cc_threads * geo.cap:
                out.append('fh_fill_kernel:chunks')
    elif e == 'mt_channel_stats':
        if p['V'] // 4 > geo.ia_threads * geo.ia_stat_quads * geo.cap:
            out.append('channel_stats_kernel:quads')
        if p['active'] == 'all' and p['NC'] > geo.ia_chunk or p['active'] != 'all' and any(a >= geo.ia_chunk for a in p['active']):
            out.append('mt_channel_stats:IA_CHUNK')
    elif e == 'mt_intensity_apply':
        if p['V'] // 4 > geo.ia_threads * geo.cap:
            out += ['ia_run<%s>:quads' % OP_NAMES[r[0]] for r in p['records'] if r[0] != OP_NONE]
        if any(r[0] != OP_NONE for r in p['records'][geo.ia_chunk:]):
            out.append('mt_intensity_apply:IA_CHUNK')
            if p['stats'] == 'device':
                out.append('mt_channel_stats:IA_CHUNK')
    elif e == 'mt_ensemble_classify':
        if cdiv(int(np.prod(p['shape'])), geo.ens_vox) > 256 * geo.cap:
            out.append('ensemble_classify_kernel:groups')
    return out
