"""Shared by tests/test_spatial_cases_cpu.py and tests/test_spatial_kernels_gpu.py (not a test module).

The data side on real memory against float64: named cases and references for the six entry points of csrc/prep.hip, csrc/warp.hip and
csrc/sample_common.h — mt_affine_sample, mt_warp_sample, mt_spline_prefilter3, mt_gaussian_blur_axis, mt_gaussian_blur_axis_zero and
mt_downsample_seg_nearest.  numpy and scipy only; nothing here touches a device or the library.  test_spatial_cases_cpu.py checks the
references against scipy.ndimage and shows which branch every case reaches.

References.  The sampler: `sample_ref`, a plain float64 restatement of mt_sample_point (range check, nearest / linear / cubic stencil,
mirror rule, per-label rule), validated against map_coordinates(mode='constant') at every coordinate of every lattice case.  The
prefilter: ndimage.spline_filter1d per axis in the kernel's order (W, H, D), rounded to float32 after every pass.  The blurs:
ndimage.correlate1d in float64 with float64 weights of the float32 sigma ('reflect' / 'constant', cval 0).  The label pyramid:
ndimage.zoom(order=0, mode='nearest', grid_mode=True).

Bounds (none of them comes from what the kernels give).
 * sampler, lattice cases (every coordinate a multiple of 1/8, the same number in float64 on both sides): the set of cval outputs is
   identical, modes 0 and 11 are exact, mode 1 on small integers is bit-exact (dyadic weights: every product and partial sum is a
   multiple of 2^-9 below 2^24, exact in float32 in any order); mode 3 within CUBIC_BOUND = 2e-5 of the data range (float32 coefficients
   and weights, tests/test_spatial_gpu.py's bound).  No exclusions.
 * sampler, general position: outputs whose coordinate lies within EDGE_EPS of a face (every mode), of a .5 rounding tie (mode 0) or
   whose label indicator lies within EDGE_EPS of 0.5 (mode 11) are left out, at most EXCLUDE_CAP of a case; the rest: modes 0 / 11 exact,
   modes 1 / 3 within CUBIC_BOUND of the data range.
 * prefilter: on the same float32 input the kernel's pass and scipy's differ by the order of two double recursions and one float32
   rounding: |diff| <= 2^-23 |ref| + 1e-12 max|line| for every pass.  A call over several axes must be bit-identical to its own
   single-axis calls (W, H, D), each of which is held to that bound against scipy's pass over the same input; the free-running
   composition cannot be (an ulp that one pass rounds the other way is spread over a whole line by the next pass).
 * reflect blur: float32 weights, each off by at most 2^-24, double accumulation, one output rounding: 2^-22 max|src| per channel.
 * zero-padded blur: weights and accumulation in double, one rounding: 2^-23 |ref| + 1e-12 max|src|; three passes: 2e-6 of the range.
 * label pyramid: bit-exact.
"""
import collections
import functools

import numpy as np
from scipy import ndimage

GUARD = 64
SENTINEL = -7.25

# launch geometry of the kernels (test_spatial_cases_cpu.py reads the same numbers out of the sources)
BLOCK = 256
CAP_SAMPLE, CAP_PYRAMID, CAP_BLUR = 65536, 16384, 4096          # grid-stride caps: both samplers | label pyramid | reflect blur per channel
BLUR_MAXR = 32
ZB_MAXR, ZB_CHUNK, ZB_TL, ZB_RB, ZB_TW, ZB_RW = 64, 32, 64, 4, 256, 8

CUBIC_BOUND = 2e-5
CVAL = -37.0          # outside every case's data range (and no dyadic mean of small integers): 'is cval' and 'is outside' are the same set
EDGE_EPS = 1e-4
EXCLUDE_CAP = 0.01


def rng(*key):
    """a generator seeded by the key's text (the same in every process)"""
    return np.random.RandomState(sum((i + 1) * ord(ch) for i, ch in enumerate(repr(key))) % (2 ** 31))


def radius(sigma):
    """the kernels' (and scipy's) radius for truncate = 4, from the float32 sigma in double"""
    return int(4.0 * float(np.float32(sigma)) + 0.5)


# ================================================================================================================================
# A. the sampler
SampleCase = collections.namedtuple('SampleCase', 'id kind entry mode planar in_shape out_shape N C cval')
MODES = (0, 1, 3, 11)
LATTICE_SHAPES = ((1, 2, 3), (2, 3, 5), (3, 1, 4), (4, 5, 6))


def mirror(i, n):
    """mt_mirror: whole-sample symmetric index (period 2n - 2); n == 1 -> 0"""
    i = np.abs(np.asarray(i, dtype=np.int64))
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = i % period
    return np.where(i > n - 1, period - i, i)


def lattice_out_shape(in_shape, planar):
    """4 n + 1 outputs per axis: with a 1/4 step about the centre (n - 1) / 2 the coordinates run through [-0.5, n - 0.5]"""
    o = tuple(4 * n + 1 for n in in_shape)
    return ((in_shape[0],) + o[1:]) if planar else o


def lattice_mats(in_shape, planar):
    """three samples: the 1/4 lattice about the centre | an axis permutation with a flip | a shear with entries 2, 1, +-0.5, +-0.25.
    Every entry is in {0, +-1, +-0.5, +-0.25, 2}, every centre a multiple of 1/4."""
    c = np.array([(n - 1) / 2. for n in in_shape])
    q = np.floor(c * 4) / 4                                   # the centre itself where it is a multiple of 1/4, else 1/4 below
    m = np.zeros((3, 12), np.float32)
    m[0, :9] = np.diag([0.25, 0.25, 0.25]).reshape(-1)
    m[0, 9:] = c
    if planar:                                                # M acts on (h, w) only: swap and flip them
        m[1, :9] = np.array([[1, 0, 0], [0, 0, -0.25], [0, 0.5, 0]], np.float32).reshape(-1)
    else:
        m[1, :9] = np.array([[0, 0.25, 0], [0, 0, -0.5], [0.5, 0, 0]], np.float32).reshape(-1)
    m[1, 9:] = q + np.array([0.25, 0.0, 0.5])
    m[2, :9] = np.array([[0.5, 0, 0.25], [0.25, -0.25, 0], [1, 2, -0.5]], np.float32).reshape(-1) if not planar else \
        np.array([[2, 1, 0.5], [0, -0.25, 0.25], [0, 0.5, -0.25]], np.float32).reshape(-1)
    m[2, 9:] = q + np.array([0.0, 0.25, -0.25])
    return m


def general_mats(r, n, in_shape, planar):
    """tests/test_spatial_gpu.py's draw: identity, a rotation, rotation + anisotropic scaling, the same off-centre"""
    mats = np.zeros((n, 12), np.float32)
    for i in range(n):
        ax, ay, az = r.uniform(-0.6, 0.6, 3) if i else (0., 0., 0.)
        if planar:
            ay = az = 0.
        cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
        rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        m = (rx @ ry @ rz).T
        if i > 1:
            sc = r.uniform(0.7, 1.4, 3)
            if planar:
                sc[0] = 1.
            m = sc[:, None] * m
        ctr = np.array(in_shape) / 2. - 0.5 + (r.uniform(-4, 4, 3) if i > 2 else 0)
        mats[i, :9], mats[i, 9:] = m.reshape(-1), ctr
    return mats


def sample_cases():
    out = []
    for entry in ('affine', 'warp'):
        for mode in MODES:
            for planar in (0, 1):
                for shp in LATTICE_SHAPES:
                    out.append(SampleCase('%s-lat-m%d-%s-%dx%dx%d' % ((entry, mode, 'pl' if planar else '3d') + shp), 'lattice', entry, mode,
                                          planar, shp, lattice_out_shape(shp, planar), 3, 2, CVAL))
            out.append(SampleCase('%s-gen-m%d-3d' % (entry, mode), 'general', entry, mode, 0, (11, 13, 14), (9, 10, 11), 4, 2, CVAL))
        out.append(SampleCase('%s-gen-m3-pl' % entry, 'general', entry, 3, 1, (5, 13, 14), (5, 10, 11), 4, 2, CVAL))
    return out


def stride_cases():
    """more outputs than CAP_SAMPLE x 256 threads from a tiny input: the second trip of the grid-stride loop starts at od = 256, and the
    centre puts the inside of the volume on both sides of it"""
    out = [SampleCase('affine-stride-m%d' % m, 'stride', 'affine', m, 0, (2, 3, 4), (260, 256, 256), 1, 1, CVAL) for m in (0, 1)]
    out += [SampleCase('warp-stride-pl-m%d' % m, 'stride', 'warp', m, 1, (260, 3, 4), (260, 256, 256), 1, 1, CVAL) for m in (0, 1)]
    return out


def stride_mats(c):
    m = np.zeros((1, 12), np.float32)
    if c.planar:
        m[0, :9] = np.array([[1, 0, 0], [0, 0.25, 0], [0, 0, -0.25]], np.float32).reshape(-1)
        m[0, 9:] = [0, 1.0, 1.5]
    else:                                     # xd = 0.25 (od - 129.5) - 31.5: inside [0, 1] for od = 256 .. 259 only just; -31.25: od 255 .. 258
        m[0, :9] = np.diag([0.25, 0.25, -0.25]).reshape(-1)
        m[0, 9:] = [-31.25, 1.0, 1.5]
    return m


@functools.lru_cache(maxsize=None)
def sample_draw(c):
    """the operands of one case: src [N, C, D, H, W] float32, mats [N, 12] float32, and for mt_warp_sample field / alpha.  The dict is
    shared by every test of the case and never written."""
    r = rng('sample', c.id)
    shp = (c.N, c.C) + c.in_shape
    if c.mode == 11:
        src = r.randint(-1, 4, size=shp).astype(np.float32)
    elif c.mode == 1 and c.kind != 'general':
        src = r.randint(-8, 9, size=shp).astype(np.float32)
    else:
        src = r.randn(*shp).astype(np.float32)
    if c.kind == 'lattice':
        mats = lattice_mats(c.in_shape, c.planar)
    elif c.kind == 'stride':
        mats = stride_mats(c)
    else:
        mats = general_mats(r, c.N, c.in_shape, c.planar)
        if c.mode in (0, 11):                 # the identity sample would sit on the .5 ties of both rules (the lattice cases' subject)
            mats[:, 9:] += np.float32(0.013)
    d = dict(src=src, mats=mats, field=None, alpha=None)
    if c.entry == 'warp':
        fshape = ((c.N, 2) + c.out_shape[1:]) if c.planar else ((c.N, 3) + c.out_shape)
        if c.kind == 'general':
            field = ndimage.gaussian_filter(r.uniform(-1, 1, fshape), (0, 0) + (2.0,) * (len(fshape) - 2)).astype(np.float32)
            alpha = np.array([6.0, 0.0, 9.0, 3.5], np.float32)[:c.N]
        else:                                                 # multiples of 1/4 times a power of two: the displaced mesh stays on the lattice
            field = (r.randint(-3, 4, size=fshape) / 4.).astype(np.float32)
            alpha = np.array([4.0, 8.0, 0.0], np.float32)[:c.N]
        d['field'], d['alpha'] = field, alpha
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


def sample_coords(c, mats, field=None, alpha=None, n=0, od0=0, od1=None):
    """float64 input coordinates (xd, xh, xw), each [od1 - od0, OH, OW], of sample n's output slab — the kernels' expression on the
    float32 matrices, fields and alphas"""
    OD, OH, OW = c.out_shape
    od1 = OD if od1 is None else od1
    M = mats[n].astype(np.float64)
    od = np.arange(od0, od1, dtype=np.float64)[:, None, None]
    gd = od - 0.5 * (OD - 1) + np.zeros((1, OH, OW))
    gh = np.arange(OH, dtype=np.float64)[None, :, None] - 0.5 * (OH - 1) + np.zeros((od1 - od0, 1, OW))
    gw = np.arange(OW, dtype=np.float64)[None, None, :] - 0.5 * (OW - 1) + np.zeros((od1 - od0, OH, 1))
    if field is not None and float(alpha[n]) != 0.0:
        al = float(alpha[n])
        f = field[n].astype(np.float64)
        if c.planar:
            gh = gh + al * f[0][None]
            gw = gw + al * f[1][None]
        else:
            gd, gh, gw = gd + al * f[0, od0:od1], gh + al * f[1, od0:od1], gw + al * f[2, od0:od1]
    with np.errstate(invalid='ignore', over='ignore'):
        if c.planar:
            xd = od + np.zeros((1, OH, OW))
            xh = M[4] * gh + M[5] * gw + M[10]
            xw = M[7] * gh + M[8] * gw + M[11]
        else:
            xd = M[0] * gd + M[1] * gh + M[2] * gw + M[9]
            xh = M[3] * gd + M[4] * gh + M[5] * gw + M[10]
            xw = M[6] * gd + M[7] * gh + M[8] * gw + M[11]
    return xd, xh, xw


def inside_mask(in_shape, xd, xh, xw):
    D, H, W = in_shape
    with np.errstate(invalid='ignore'):
        return (xd >= 0) & (xd <= D - 1) & (xh >= 0) & (xh <= H - 1) & (xw >= 0) & (xw <= W - 1)


def _cubic_weights(t):
    return np.stack([(1 - t) ** 3 / 6., (4 - 6 * t * t + 3 * t ** 3) / 6., (1 + 3 * t + 3 * t * t - 3 * t ** 3) / 6., t ** 3 / 6.])


def sample_ref(vol, xd, xh, xw, mode, cval, planar=False, od=None):
    """mt_sample_point in float64.  vol: [C, D, H, W] (mode 3: the prefiltered coefficients); coordinates of any common shape S; od: the
    output slice index of every point (planar cubic sampling takes its slice from it) -> ([C] + S float64, inside mask).  Only the
    inside points are computed: the others are cval (mode 11: 0)."""
    vol = np.asarray(vol, dtype=np.float64)
    C, (D, H, W) = vol.shape[0], vol.shape[1:]
    ins = inside_mask((D, H, W), xd, xh, xw)
    out = np.full((C,) + xd.shape, 0.0 if mode == 11 else float(cval))
    if not ins.any():
        return out, ins
    a, b, e = xd[ins], xh[ins], xw[ins]
    if mode == 0:
        ia = np.minimum(np.floor(a + 0.5).astype(np.int64), D - 1)
        ib = np.minimum(np.floor(b + 0.5).astype(np.int64), H - 1)
        ie = np.minimum(np.floor(e + 0.5).astype(np.int64), W - 1)
        out[:, ins] = vol[:, ia, ib, ie]
        return out, ins
    if mode in (1, 11):
        d0, h0, w0 = np.floor(a).astype(np.int64), np.floor(b).astype(np.int64), np.floor(e).astype(np.int64)
        fd, fh, fw = a - d0, b - h0, e - w0
        d1, h1, w1 = mirror(d0 + 1, D), mirror(h0 + 1, H), mirror(w0 + 1, W)
        taps, wts = [], []
        for k in range(8):
            ia, ib, ie = (d1 if k & 4 else d0), (h1 if k & 2 else h0), (w1 if k & 1 else w0)
            taps.append(vol[:, ia, ib, ie])
            wts.append((fd if k & 4 else 1 - fd) * (fh if k & 2 else 1 - fh) * (fw if k & 1 else 1 - fw))
        taps, wts = np.stack(taps), np.stack(wts)                         # [8, C, P], [8, P]
        if mode == 1:
            out[:, ins] = (taps * wts[:, None]).sum(0)
            return out, ins
        best = np.zeros(taps.shape[1:])
        found = np.zeros(taps.shape[1:], bool)
        for k in range(8):                                    # the largest label whose indicator interpolates to >= 0.5
            s = ((taps == taps[k][None]) * wts[:, None]).sum(0)
            take = (s >= 0.5) & (~found | (taps[k] > best))
            best = np.where(take, taps[k], best)
            found |= take
        out[:, ins] = np.where(found, best, 0.0)
        return out, ins
    idx, wgt = [], []
    for x, n in ((a, D), (b, H), (e, W)):
        i0 = np.floor(x).astype(np.int64) - 1
        wgt.append(_cubic_weights(x - np.floor(x)))
        idx.append(np.stack([mirror(i0 + k, n) for k in range(4)]))
    if planar:                                                # slices are independent images: no D stencil
        sl = np.broadcast_to(od, xd.shape)[ins].astype(np.int64)
        idx[0] = np.stack([sl] * 4)
        wgt[0] = np.stack([np.zeros_like(a), np.ones_like(a), np.zeros_like(a), np.zeros_like(a)])
    acc = np.zeros((C, a.size))
    for i in range(4):
        for j in range(4):
            for k in range(4):
                acc += (wgt[0][i] * wgt[1][j] * wgt[2][k])[None] * vol[:, idx[0][i], idx[1][j], idx[2][k]]
    out[:, ins] = acc
    return out, ins


def prefilter_ref64(vol, planar):
    """float64 cubic B-spline coefficients of [.., D, H, W] as map_coordinates(order=3, mode='constant') computes them (mirror
    boundaries); planar: every D slice on its own"""
    out = np.asarray(vol, dtype=np.float64)
    for ax in ((-1, -2) if planar else (-1, -2, -3)):
        out = ndimage.spline_filter1d(out, 3, axis=ax, mode='mirror')
    return out


def sample_case_ref(c, d=None, mats=None, field=None, alpha=None):
    """the whole expected output [N, C, OD, OH, OW] float64 of a lattice / general case, with the inside mask and the coordinates"""
    d = sample_draw(c) if d is None else d
    mats = d['mats'] if mats is None else mats
    field = d['field'] if field is None else field
    alpha = d['alpha'] if alpha is None else alpha
    out = np.empty((c.N, c.C) + c.out_shape)
    ins = np.empty((c.N,) + c.out_shape, bool)
    coords = []
    od = np.arange(c.out_shape[0])[:, None, None]
    for n in range(c.N):
        xd, xh, xw = sample_coords(c, mats, field, alpha, n)
        vol = prefilter_ref64(d['src'][n], c.planar) if c.mode == 3 else d['src'][n]
        out[n], ins[n] = sample_ref(vol, xd, xh, xw, c.mode, c.cval, c.planar, od)
        coords.append((xd, xh, xw))
    return out, ins, coords


def general_exclusions(c, d, coords):
    """[N, OD, OH, OW] mask of the outputs a general-position case leaves out, from the reference coordinates alone"""
    ex = np.zeros((c.N,) + c.out_shape, bool)
    for n, xs in enumerate(coords):
        for x, size in list(zip(xs, c.in_shape))[1 if c.planar else 0:]:         # planar: xd is the slice index itself, exact on both sides
            ex[n] |= (np.abs(x) < EDGE_EPS) | (np.abs(x - (size - 1)) < EDGE_EPS)
            if c.mode == 0:
                ex[n] |= np.abs(x + 0.5 - np.round(x + 0.5)) < EDGE_EPS
        if c.mode == 11:
            for ch in range(c.C):
                for lab in np.unique(d['src'][n, ch]):
                    ind, _ = sample_ref((d['src'][n, ch:ch + 1] == lab).astype(np.float64), xs[0], xs[1], xs[2], 1, 0.0)
                    ex[n] |= np.abs(ind[0] - 0.5) < EDGE_EPS
    return ex


@functools.lru_cache(maxsize=None)
def stride_ref(c):
    """[1, 1, OD, OH, OW] float32 expected output of a grid-stride case, computed slab by slab"""
    d = sample_draw(c)
    out = np.empty((1, 1) + c.out_shape, np.float32)
    step = 20
    for od0 in range(0, c.out_shape[0], step):
        od1 = min(od0 + step, c.out_shape[0])
        xd, xh, xw = sample_coords(c, d['mats'], d['field'], d['alpha'], 0, od0, od1)
        ref, _ = sample_ref(d['src'][0], xd, xh, xw, c.mode, c.cval, c.planar, np.arange(od0, od1)[:, None, None])
        out[0, :, od0:od1] = ref
    out.setflags(write=False)
    return out


# ================================================================================================================================
# B. mt_spline_prefilter3
PrefilterCase = collections.namedtuple('PrefilterCase', 'id shape axes NC')
PF_LENGTHS = (1, 2, 3, 4, 21, 280, 600)
PF_AXIS = {1: 2, 2: 1, 4: 0}                                   # axes bit -> array axis of [D, H, W]


def prefilter_cases():
    out = []
    for bit in (1, 2, 4):
        for n in PF_LENGTHS:
            shp = [9, 10]
            shp.insert(PF_AXIS[bit], n)
            out.append(PrefilterCase('pf-a%d-n%d' % (bit, n), tuple(shp), bit, 3))
    out += [PrefilterCase('pf-a3-5x21x19', (5, 21, 19), 3, 3), PrefilterCase('pf-a3-7x280x13', (7, 280, 13), 3, 3),
            PrefilterCase('pf-a7-11x9x10', (11, 9, 10), 7, 3), PrefilterCase('pf-a7-280x10x9', (280, 10, 9), 7, 3)]
    return out


def prefilter_lines(c, bit):
    """number of lines of the pass along the axis of `bit`"""
    return c.NC * int(np.prod(c.shape)) // c.shape[PF_AXIS[bit]]


@functools.lru_cache(maxsize=None)
def prefilter_draw(c):
    r = rng('prefilter', c.id)
    x = r.randn(c.NC, *c.shape).astype(np.float32)
    x[1, ..., 0] += 5                          # something at the border
    x.setflags(write=False)
    return x


def prefilter_ref(c, x):
    """-> (float32 result, per-element max|line| of the last pass's input along its axis)"""
    cur = x
    linemax = np.zeros(x.shape)
    for bit in (1, 2, 4):
        if c.axes & bit:
            ax = 1 + PF_AXIS[bit]
            linemax = np.broadcast_to(np.abs(cur).max(axis=ax, keepdims=True), cur.shape).astype(np.float64)
            if cur.shape[ax] > 1:
                cur = ndimage.spline_filter1d(cur.astype(np.float64), 3, axis=ax, mode='mirror').astype(np.float32)
    return cur, linemax


def prefilter_bound(ref, linemax):
    return 2.0 ** -23 * np.abs(ref.astype(np.float64)) + 1e-12 * linemax


# ================================================================================================================================
# C. mt_gaussian_blur_axis (reflect)
BlurCase = collections.namedtuple('BlurCase', 'id shape axis sigmas')
RB_SIGMAS = (0.1, 0.0, 0.3, -1.0, 0.5, 1.0, 8.0, 0.7)         # r = 0 | copy | 1 | copy | 2 | 4 | 32 | 3 (4 sigma = 2.8: the + 0.5 decides)
RB_LENGTHS = (1, 2, 3, 19)
RB_REFUSED = (8.125, 8.2, 13.0, float('nan'), float('inf'))


def gauss_weights(sigma):
    """scipy's _gaussian_kernel1d for the float32 sigma, in double"""
    sg = float(np.float32(sigma))
    k = np.arange(-radius(sg), radius(sg) + 1, dtype=np.float64)
    w = np.exp(-0.5 * k * k / (sg * sg))
    return w / w.sum()


def reflect_blur_cases():
    out = []
    for axis in range(3):
        for n in RB_LENGTHS:
            shp = [5, 6]
            shp.insert(axis, n)
            out.append(BlurCase('rb-ax%d-n%d' % (axis, n), tuple(shp), axis, RB_SIGMAS))
    out.append(BlurCase('rb-stride-5x512x512', (5, 512, 512), 0, (1.0, 0.0)))
    return out


@functools.lru_cache(maxsize=None)
def blur_draw(c):
    r = rng('blur', c.id)
    x = (r.randn(len(c.sigmas), *c.shape) * 3 + 1).astype(np.float32)
    kind = getattr(c, 'data', 'randn')
    if kind == 'impulse':                                      # impulses at two opposite corners
        x[:] = 0
        x[:, 0, 0, 0] = 1.0
        x[:, -1, -1, -1] = -2.0
    elif kind == 'ramp':
        x[:] = (np.arange(c.shape[c.axis], dtype=np.float32) - 3.0).reshape([-1 if a == c.axis else 1 for a in range(3)])
    x.setflags(write=False)
    return x


def blur_ref(c, x, mode):
    """float64 correlate1d per channel along c.axis; channels with sigma <= 0 are copies -> float64 [NC, D, H, W]"""
    out = x.astype(np.float64)
    for ch, sg in enumerate(c.sigmas):
        if np.float32(sg) > 0:
            out[ch] = ndimage.correlate1d(x[ch].astype(np.float64), gauss_weights(sg), axis=c.axis, mode=mode, cval=0.0)
    return out


# ================================================================================================================================
# D. mt_gaussian_blur_axis_zero
ZeroCase = collections.namedtuple('ZeroCase', 'id shape axis sigmas data')
ZB_SIGMAS = (0.1, 0.3, 0.0, 0.5, 0.7, -2.0, 2.2, 15.9)         # r = 0 | 1 | copy | 2 | 3 | copy | 9 | 64
ZB_LENGTHS = (1, 2, 3, 5, 63, 64, 65, 67, 129)
ZB_WIDTHS = (1, 255, 256, 257, 300)


def many_sigmas(nc):
    """a distinct sigma per channel; a zero and a negative one in every chunk of ZB_CHUNK channels"""
    sg = [0.3 + 0.07 * ch for ch in range(nc)]
    for ch in range(nc):
        if ch % ZB_CHUNK == 5:
            sg[ch] = 0.0
        if ch % ZB_CHUNK == 11:
            sg[ch] = -1.0 - ch
    return tuple(sg)


def zero_blur_cases():
    out = []
    for n in ZB_LENGTHS:
        out.append(ZeroCase('zb-ax0-n%d-in1' % n, (n, 1, 1), 0, ZB_SIGMAS, 'randn'))
        out.append(ZeroCase('zb-ax0-n%d-in65' % n, (n, 5, 13), 0, ZB_SIGMAS, 'randn'))
        out.append(ZeroCase('zb-ax1-n%d-in1' % n, (3, n, 1), 1, ZB_SIGMAS, 'randn'))
        out.append(ZeroCase('zb-ax1-n%d-in65' % n, (3, n, 65), 1, ZB_SIGMAS, 'randn'))
    for w in ZB_WIDTHS:
        out.append(ZeroCase('zb-ax2-w%d-rows15' % w, (3, 5, w), 2, ZB_SIGMAS, 'randn'))
        out.append(ZeroCase('zb-ax2-w%d-rows1' % w, (1, 1, w), 2, ZB_SIGMAS, 'randn'))
    for axis, shp in ((0, (67, 5, 13)), (1, (3, 67, 65)), (2, (3, 5, 300))):
        out.append(ZeroCase('zb-ax%d-impulse' % axis, shp, axis, ZB_SIGMAS, 'impulse'))
        out.append(ZeroCase('zb-ax%d-ramp' % axis, shp, axis, ZB_SIGMAS, 'ramp'))
    for nc in (33, 70):
        for axis in range(3):
            out.append(ZeroCase('zb-ax%d-nc%d' % (axis, nc), (3, 5, 7), axis, many_sigmas(nc), 'randn'))
    return out


def zero_blur_bound(ref, x):
    return 2.0 ** -23 * np.abs(ref) + 1e-12 * np.abs(x).max()


def zero_blur_tiles(c):
    """tiles along the axis and across it, as mt_gaussian_blur_axis_zero cuts a channel"""
    D, H, W = c.shape
    if c.axis == 2:
        return (W + ZB_TW - 1) // ZB_TW, (D * H + ZB_RW - 1) // ZB_RW
    L, inner = (D, H * W) if c.axis == 0 else (H, W)
    return (L + ZB_TL - 1) // ZB_TL, (inner + 63) // 64


# ================================================================================================================================
# E. mt_downsample_seg_nearest
PyramidCase = collections.namedtuple('PyramidCase', 'id in_shape out_shape NC kind')
PY_PAIRS = ((1, 1), (1, 3), (3, 2), (6, 9), (7, 3), (37, 9), (5, 5))


def pyramid_cases():
    out = []
    for i in range(len(PY_PAIRS)):
        p = [PY_PAIRS[i], PY_PAIRS[(i + 2) % 7], PY_PAIRS[(i + 4) % 7]]
        out.append(PyramidCase('py-%s' % '-'.join('%dto%d' % q for q in p), tuple(q[0] for q in p), tuple(q[1] for q in p), 3,
                               'image' if i == 3 else 'labels'))
    out.append(PyramidCase('py-stride-2x3x4-to-130x180x180', (2, 3, 4), (130, 180, 180), 1, 'labels'))
    return out


@functools.lru_cache(maxsize=None)
def pyramid_draw(c):
    r = rng('pyramid', c.id)
    if c.kind == 'image':                      # non-integer image data with some voxels at exactly -1.0
        x = r.randn(c.NC, *c.in_shape).astype(np.float32)
        x[r.uniform(size=x.shape) < 0.2] = -1.0
    else:
        x = r.randint(-1, 4, size=(c.NC,) + c.in_shape).astype(np.float32)
    x.reshape(-1)[0] = -1.0
    x.setflags(write=False)
    return x


def pyramid_ref(c, x, remove_minus_one):
    out = np.empty((c.NC,) + c.out_shape, np.float32)
    for ch in range(c.NC):
        z = ndimage.zoom(x[ch], [o / i for o, i in zip(c.out_shape, c.in_shape)], order=0, mode='nearest', grid_mode=True)
        assert z.shape == c.out_shape and z.dtype == np.float32
        out[ch] = z
    if remove_minus_one:
        out[out == -1.0] = 0.0
    return out


def pyramid_index(n_in, n_out):
    """the kernel's source index of every output along one axis: floor((o + 0.5) * (in / out)), clamped"""
    f = float(n_in) / float(n_out)
    return np.clip(np.floor((np.arange(n_out, dtype=np.float64) + 0.5) * f).astype(np.int64), 0, n_in - 1)
