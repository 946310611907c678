"""The label-volume and intensity units on real memory against their references: every entry point of csrc/metrics.hip,
csrc/postproc.hip and csrc/intensity.hip, and what tests/test_ensemble_gpu.py leaves open of csrc/ensemble.hip, through the library's C
interface (ctypes: alignment, workspace and capacity are this file's to choose).  Cases, references and bounds are
tests/volume_cases.py (see its docstring), evaluated at the device's own CU count; tests/test_volume_cases_cpu.py checks the
references and what the cases reach.  Every destination and workspace starts as a sentinel between guard bytes; after a launch the
guards and every source are bit-identical, no sentinel is left where a value is due and every assigned element equals the reference.
Every figure is printed before it is asserted."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import volume_cases as VC

pytestmark = pytest.mark.gpu
GUARD_BYTE, GUARD_BYTES = 0xA5, 256
EINVAL, EWORKSPACE = -1, -2


def _ids(family):
    return [c.id for c in VC.cases(family, 256)]          # the ids do not depend on the CU count


@pytest.fixture(scope='module')
def env(dev):
    from multitalent_amd import _lib
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    tables = {f: {c.id: c for c in VC.cases(f, cus)} for f in VC.FAMILIES}
    print('VOLUME-FIG device compute-units %d grid-cap %d' % (cus, VC.geometry(cus).cap))
    return dict(dev=dev, lib=_lib.load(), _lib=_lib, cus=cus, geo=VC.geometry(cus), tables=tables)


def _case(env, family, cid, **kw):
    c = env['tables'][family][cid]
    trips = VC.second_trips(c, env['geo'])
    if c.p.get('trip2') and not c.id.startswith('apply-V1024cap'):
        assert trips, "the case does not reach a second trip on this device"
    return c, VC.build(family, c, env['cus'], **kw)


def stops_on_hip_error(fn):
    """A HIP error ends the whole run: nothing more is launched on a device that has faulted (as test_datapath_kernels_gpu)."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except BaseException as e:
            text = str(e)
            faulted = isinstance(e, RuntimeError) and any(s in text for s in ('rc=-3', 'HIP error', 'hipError', 'illegal memory', 'device-side'))
            if not faulted:
                try:
                    torch.cuda.synchronize()
                except Exception as e2:          # noqa: BLE001
                    faulted, text = True, str(e2)
            if faulted:
                pytest.exit('HIP error in %s: %s' % (fn.__name__, text), returncode=3)
            raise
    return run


def _fig(kernel, case_id, what, value):
    print('VOLUME-FIG %s %s %s %.3e' % (kernel, case_id, what, value))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sentinel(dtype, n):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.full(n, VC.F32_SENTINEL_BITS, np.uint32).view(np.float32)
    if dtype == np.float64:
        return np.full(n, 0x7ff8deaddeaddead, np.uint64).view(np.float64)
    if dtype.kind == 'i' and dtype.itemsize > 1:
        return np.full(n, VC.INT_SENTINEL, dtype)
    return np.full(n * dtype.itemsize, VC.BYTE_SENTINEL, np.uint8).view(dtype)


class Source(object):
    """an operand the kernel only reads, at a chosen byte offset from a 256-byte boundary; compared bit for bit afterwards"""

    def __init__(self, env, host, offset=0):
        self.host = np.ascontiguousarray(host)
        raw = self.host.reshape(-1).view(np.uint8)
        self.off, self.nbytes = GUARD_BYTES + offset, raw.size
        buf = np.full(self.off + raw.size + GUARD_BYTES, GUARD_BYTE, np.uint8)
        buf[self.off:self.off + raw.size] = raw
        self.image = torch.from_numpy(buf)
        self.dev = self.image.to(env['dev'])

    def ptr(self):
        return self.dev.data_ptr() + self.off

    def unchanged(self):
        return torch.equal(self.dev.cpu(), self.image)


class Guarded(object):
    """a destination of n elements of `dtype` at a chosen byte offset, sentinels inside and guard bytes around it; `init` for in-place kernels"""

    def __init__(self, env, dtype, n, offset=0, init=None):
        self.dtype, self.n = np.dtype(dtype), int(n)
        self.off, self.nbytes = GUARD_BYTES + offset, self.n * self.dtype.itemsize
        buf = np.full(self.off + self.nbytes + GUARD_BYTES, GUARD_BYTE, np.uint8)
        fill = _sentinel(dtype, self.n) if init is None else np.ascontiguousarray(init, dtype=self.dtype).reshape(-1)
        buf[self.off:self.off + self.nbytes] = fill.view(np.uint8)
        self.dev = torch.from_numpy(buf).to(env['dev'])

    def ptr(self):
        return self.dev.data_ptr() + self.off

    def guards_ok(self):
        d = self.dev
        return bool((d[:self.off] == GUARD_BYTE).all()) and bool((d[self.off + self.nbytes:] == GUARD_BYTE).all())

    def body(self, torch_dtype):
        """the destination on the device (large cases are reduced there)"""
        return self.dev[self.off:self.off + self.nbytes].view(torch_dtype)

    def fetch(self):
        assert self.guards_ok(), "guard bytes around a destination changed"
        return self.dev[self.off:self.off + self.nbytes].cpu().numpy().copy().view(self.dtype)

    def sentinels(self, got):
        """elements of got that still hold the sentinel"""
        return VC.bits(got) == VC.bits(_sentinel(self.dtype, got.size))

    def untouched(self):
        got = self.fetch()
        return bool(self.sentinels(got).all())


def _workspace(env, nbytes):
    return Guarded(env, np.uint8, max(int(nbytes), 16))


def _u8(values):
    return (ctypes.c_uint8 * len(values))(*[int(v) for v in values])


# ================================================================================================================================
# A. mt_seg_joint_hist
@pytest.mark.parametrize('cid', _ids('hist'))
@stops_on_hip_error
def test_seg_joint_hist(env, cid):
    """np.bincount of the remapped pairs, exact, at every pair of misalignments"""
    c, d = _case(env, 'hist', cid)
    lib, _lib = env['lib'], env['_lib']
    t, r = Source(env, d['t'], offset=c.p['a']), Source(env, d['r'], offset=c.p['b'])
    assert t.ptr() % 16 == c.p['a'] and r.ptr() % 16 == c.p['b']
    hist = Guarded(env, np.int64, d['C'] * d['C'])
    _lib.check(lib.mt_seg_joint_hist(t.ptr(), r.ptr(), d['V'], _u8(d['remap']), d['C'], hist.ptr(), _stream()), 'seg_joint_hist')
    torch.cuda.synchronize()
    got = hist.fetch()
    assert t.unchanged() and r.unchanged(), "mt_seg_joint_hist changed a source"
    _fig(VC.instances(c)[0], cid, 'wrong-cells', (got != d['ref']).sum())
    assert np.array_equal(got, d['ref']), (np.flatnonzero(got != d['ref'])[:8], got[got != d['ref']][:8], d['ref'][got != d['ref']][:8])


# ================================================================================================================================
# B. mt_surface_distances
_WORST = {}


def _worst(key, value):
    _WORST[key] = max(_WORST.get(key, 0.0), float(value))
    return _WORST[key]


def _surface(env, d, capacity, big=False):
    """`out` holds every entry there is (nA + nB), the call is given the case's capacity: what lies beyond it must stay sentinel"""
    lib, _lib = env['lib'], env['_lib']
    D, H, W = d['t'].shape
    t, r = Source(env, d['t'], offset=3), Source(env, d['r'], offset=5)
    sp = (ctypes.c_double * 3)(*d['sp'])
    wsn = lib.mt_surface_distances_workspace(D, H, W, capacity)
    assert wsn > 0
    out, stats, ws = Guarded(env, np.float64, max(capacity, d['nA'] + d['nB'])), Guarded(env, np.float64, 6), _workspace(env, wsn)
    _lib.check(lib.mt_surface_distances(t.ptr(), r.ptr(), D, H, W, _u8(d['member']), sp, d['conn'], out.ptr(), capacity, stats.ptr(), ws.ptr(), wsn,
                                        _stream()), 'surface_distances')
    torch.cuda.synchronize()
    assert ws.guards_ok(), "guard bytes around the workspace changed"
    assert t.unchanged() and r.unchanged(), "mt_surface_distances changed a source"
    return (out if big else out.fetch()), stats.fetch(), out


def _check_sd_stats(cid, st, stored, nA, nB, capacity):
    """counts exact; max exact and the maximum of the stored prefix; sum within n 2^-52 sum of math.fsum of what was stored"""
    ref = VC.sd_stats_ref(stored, nA, nB, capacity)
    for k, (n, mx, sm) in enumerate(ref):
        cnt, gmx, gsm = st[3 * k:3 * k + 3]
        stored_n = (min(nA, capacity), max(0, min(nA + nB, capacity) - nA))[k]
        bound = stored_n * 2.0 ** -52 * sm if math.isfinite(sm) else 0.0
        err = abs(gsm - sm) if math.isfinite(sm) else (0.0 if gsm == sm else math.inf)
        _fig('sd_reduce2_kernel', cid, 'dir%d-count-diff' % k, cnt - n)
        _fig('sd_reduce2_kernel', cid, 'dir%d-max-diff' % k, 0.0 if gmx == mx else math.inf)
        _fig('sd_reduce2_kernel', cid, 'dir%d-sum-err/bound' % k, err / bound if bound else (0.0 if err == 0 else math.inf))
        assert cnt == n and gmx == mx and err <= bound, (k, (cnt, gmx, gsm), (n, mx, sm))


@pytest.mark.parametrize('cid', [i for i in _ids('sd') if not i.startswith('sd-loop')])
@stops_on_hip_error
def test_surface_distances(env, cid):
    """the brute-force minimum over all border voxels: bit for bit with dyadic spacings, within 2 ulp otherwise; a capacity below
    nA + nB stores the prefix, leaves the rest and its guard alone, and keeps the counts true"""
    c, d = _case(env, 'sd', cid)
    nA, nB, capacity = d['nA'], d['nB'], d['capacity']
    stored = min(capacity, nA + nB)
    got, st, out = _surface(env, d, capacity)
    again, st2, _ = _surface(env, d, capacity)
    assert np.array_equal(VC.bits(got), VC.bits(again)) and np.array_equal(VC.bits(st), VC.bits(st2)), "two runs of mt_surface_distances differ"
    ref = d['out'][:stored]
    left = out.sentinels(got[:stored]).sum()
    stray = (~out.sentinels(got[stored:])).sum()
    _fig('sd_query_kernel', cid, 'sentinels-left', left)
    _fig('sd_compact_kernel', cid, 'writes-past-the-capacity', stray)
    assert left == 0 and stray == 0
    fin = np.isfinite(ref)
    assert np.array_equal(got[:stored][~fin], ref[~fin])                     # +inf where the other mask has no border voxel
    ulp = float(VC.ulps64(got[:stored][fin], ref[fin]).max()) if fin.any() else 0.0
    _fig('sd_query_kernel', cid, 'worst-ulp', ulp)
    _fig('sd_query_kernel', cid, 'worst-ulp-so-far-%s' % ('dyadic' if d['dyadic'] else 'ragged'), _worst(d['dyadic'], ulp))
    assert ulp <= (0 if d['dyadic'] else VC.SD_ULPS)
    _check_sd_stats(cid, st, got[:stored], nA, nB, capacity)
    if capacity < nA + nB:
        assert st[0] + st[3] > capacity                                       # what tells the caller that `out` is truncated


@pytest.mark.parametrize('cid', [i for i in _ids('sd') if i.startswith('sd-loop')])
@stops_on_hip_error
def test_surface_distances_loops(env, cid):
    """two facing planes: every entry is sx.  The second trips of the rows, query and reduce loops; `out` is reduced on the device"""
    c, d = _case(env, 'sd', cid)
    assert 'sd_%s%s_kernel:%s' % (c.p['trip2'], '1' if c.p['trip2'] == 'reduce' else '', {'rows': 'rows', 'query': 'entries', 'reduce': 'chunks'}[c.p['trip2']]) \
        in VC.second_trips(c, env['geo'])
    n = d['nA']
    out, st, _ = _surface(env, d, 2 * n, big=True)
    assert out.guards_ok()
    body = out.body(torch.float64)
    wrong = int((body != d['value']).sum())
    _fig('sd_query_kernel', cid, 'wrong-entries', wrong)
    assert wrong == 0
    tail = body[-5:].cpu().numpy()
    assert (tail == d['value']).all()
    for k in range(2):
        want = d['value'] * n                                                 # n sx: exact for a dyadic sx and n < 2^53
        _fig('sd_reduce2_kernel', cid, 'dir%d-sum-err' % k, abs(st[3 * k + 2] - want))
        assert st[3 * k] == n and st[3 * k + 1] == d['value'] and abs(st[3 * k + 2] - want) <= n * 2.0 ** -52 * want


# ================================================================================================================================
# C. mt_cc_label3d / mt_cc_remove
@pytest.mark.parametrize('cid', _ids('cc'))
@stops_on_hip_error
def test_cc_label_and_remove(env, cid):
    """scipy's labelling with every label mapped to its component's smallest index, exact; the removal rule with Python floats"""
    c, d = _case(env, 'cc', cid)
    lib, _lib = env['lib'], env['_lib']
    D, H, W = d['seg'].shape
    V = D * H * W
    seg = Source(env, d['seg'], offset=1)
    labels, sizes, stats = Guarded(env, np.int32, V), Guarded(env, np.int32, V), Guarded(env, np.int32, 2)
    _lib.check(lib.mt_cc_label3d(seg.ptr(), D, H, W, _u8(d['member']), labels.ptr(), sizes.ptr(), stats.ptr(), _stream()), 'cc_label3d')
    torch.cuda.synchronize()
    gl, gs, gst = labels.fetch(), sizes.fetch(), stats.fetch()
    assert seg.unchanged(), "mt_cc_label3d changed its source"
    _fig('cc_flatten_kernel', cid, 'wrong-labels', (gl != d['labels']).sum())
    _fig('cc_count_kernel', cid, 'wrong-sizes', (gs != d['sizes']).sum())
    _fig('cc_count_kernel', cid, 'stats-diff', abs(int(gst[0]) - d['stats'][0]) + abs(int(gst[1]) - d['stats'][1]))
    assert np.array_equal(gl, d['labels']), np.flatnonzero(gl != d['labels'])[:8]
    assert np.array_equal(gs, d['sizes']), np.flatnonzero(gs != d['sizes'])[:8]
    assert tuple(int(v) for v in gst) == d['stats']
    if 'remove' not in d:
        return
    vpv, use_min, min_size = d['remove']
    work, removed = Guarded(env, np.uint8, V, offset=3, init=d['seg']), Guarded(env, np.int32, 1)
    _lib.check(lib.mt_cc_remove(work.ptr(), D, H, W, labels.ptr(), sizes.ptr(), stats.ptr(), vpv, use_min, min_size, removed.ptr(), _stream()), 'cc_remove')
    torch.cuda.synchronize()
    after, rem = work.fetch(), int(removed.fetch()[0])
    _fig('cc_remove_kernel', cid, 'wrong-voxels', (after != d['seg_after'].ravel()).sum())
    _fig('cc_remove_kernel', cid, 'removed-diff', rem - d['removed'])
    assert np.array_equal(after, d['seg_after'].ravel()) and rem == d['removed']
    assert np.array_equal(labels.fetch(), gl) and np.array_equal(sizes.fetch(), gs) and np.array_equal(stats.fetch(), gst), "mt_cc_remove changed the labelling"


# ================================================================================================================================
# D. mt_fill_holes3d
@pytest.mark.parametrize('cid', _ids('fh'))
@stops_on_hip_error
def test_fill_holes(env, cid):
    """scipy's binary_fill_holes(mask != 0) as 0 / 1, the box and the count, exact, in place at every alignment of the mask"""
    c, d = _case(env, 'fh', cid, full=False)
    lib, _lib = env['lib'], env['_lib']
    D, H, W = d['mask'].shape
    V = D * H * W
    mask, bbox = Guarded(env, np.uint8, V, offset=c.p['off'], init=d['mask']), Guarded(env, np.int32, 7)
    assert mask.ptr() % 16 == c.p['off']
    wsn = lib.mt_fill_holes3d_workspace(D, H, W)
    ws = _workspace(env, wsn)
    _lib.check(lib.mt_fill_holes3d(mask.ptr(), D, H, W, bbox.ptr(), ws.ptr(), wsn, _stream()), 'fill_holes3d')
    torch.cuda.synchronize()
    assert ws.guards_ok(), "guard bytes around the workspace changed"
    got, box = mask.fetch(), bbox.fetch()
    _fig('fh_fill_kernel', cid, 'wrong-voxels', (got != d['ref'].ravel()).sum())
    _fig('fh_fill_kernel', cid, 'count-diff', int(box[6]) - d['count'])
    assert np.array_equal(got, d['ref'].ravel()), np.flatnonzero(got != d['ref'].ravel())[:8]
    assert int(box[6]) == d['count']
    if d['count']:
        assert box[:6].tolist() == d['bbox'], (box, d['bbox'])


# ================================================================================================================================
# E. mt_channel_stats
def _channel_stats(env, x_ptr, NC, V, active):
    lib, _lib = env['lib'], env['_lib']
    wsn = lib.mt_channel_stats_workspace(NC, V)
    stats, ws = Guarded(env, np.float64, 4 * NC), Guarded(env, np.uint8, wsn)
    _lib.check(lib.mt_channel_stats(x_ptr, NC, V, None if active is None else _u8(active), stats.ptr(), ws.ptr(), wsn, _stream()), 'channel_stats')
    torch.cuda.synchronize()
    assert ws.guards_ok(), "guard bytes around the workspace changed"
    return stats


@pytest.mark.parametrize('cid', _ids('stats'))
@stops_on_hip_error
def test_channel_stats(env, cid):
    """min and max exact, mean within 1e-10 max|x| and sd within 1e-8 sd of math.fsum; numpy's rule for infinities and NaNs; inactive
    rows keep their sentinel; the workspace is exactly what mt_channel_stats_workspace asks for"""
    c, d = _case(env, 'stats', cid)
    NC, V = d['NC'], d['V']
    x = Source(env, d['x'], offset=4)
    active = None if (c.p['active'] == 'all' and NC % 2) else d['active']
    st = _channel_stats(env, x.ptr(), NC, V, active)
    got = st.fetch()
    again = _channel_stats(env, x.ptr(), NC, V, active).fetch()
    assert x.unchanged(), "mt_channel_stats changed its source"
    assert np.array_equal(VC.bits(got), VC.bits(again)), "two runs of mt_channel_stats differ"
    got = got.reshape(NC, 4)
    same = lambda a, b: a == b or (math.isnan(a) and math.isnan(b))
    for ch in range(NC):
        r = d['refs'][ch]
        if r is None:
            assert st.sentinels(got[ch]).all(), "an inactive row was written"
            continue
        lo, hi, mean, sd, scale = r
        name = '%s/ch%d' % (cid, ch)
        _fig('channel_stats_kernel', name, 'min-diff', 0.0 if same(got[ch, 0], lo) else math.inf)
        _fig('channel_stats_kernel', name, 'max-diff', 0.0 if same(got[ch, 1], hi) else math.inf)
        assert same(got[ch, 0], lo) and same(got[ch, 1], hi), (got[ch], r)
        if math.isfinite(mean) and math.isfinite(sd):
            e_m = abs(got[ch, 2] - mean) / scale if scale else abs(got[ch, 2] - mean)
            e_s = abs(got[ch, 3] - sd) / sd if sd else (0.0 if got[ch, 3] == 0.0 else math.inf)      # a reference sd of 0 is met exactly
            _fig('channel_stats_finalize_kernel', name, 'mean-err/max|x|', e_m)
            _fig('channel_stats_finalize_kernel', name, 'sd-err/sd', e_s)
            _fig('channel_stats_finalize_kernel', name, 'worst-mean-err-so-far', _worst('mean', e_m))
            _fig('channel_stats_finalize_kernel', name, 'worst-sd-err-so-far', _worst('sd', e_s))
            assert e_m <= VC.MEAN_BOUND and e_s <= VC.SD_BOUND, (got[ch], r)
            assert sd != 0 or got[ch, 3] == 0.0, "a constant channel has sd 0 exactly"
        else:
            _fig('channel_stats_finalize_kernel', name, 'finite-moments', float(math.isfinite(got[ch, 2])) + float(math.isfinite(got[ch, 3])))
            assert not math.isfinite(got[ch, 2]) and not math.isfinite(got[ch, 3]), (got[ch], r)
            if np.isnan(d['x'][ch]).any():
                assert np.isnan(got[ch]).all(), (got[ch], r)


# ================================================================================================================================
# F. mt_intensity_apply
@pytest.mark.parametrize('cid', _ids('apply'))
@stops_on_hip_error
def test_intensity_apply(env, cid):
    """SCALE, CONTRAST and RESTORE bit for bit against the float32 restatement, GAMMA within four times what float32 loses; NONE
    channels bit-identical; statistics from mt_channel_stats on the same stream, or hand-written doubles"""
    c, d = _case(env, 'apply', cid)
    lib, _lib = env['lib'], env['_lib']
    NC, V = d['NC'], d['V']
    x, x2 = Guarded(env, np.float32, NC * V, offset=4, init=d['x']), Source(env, d['x2'], offset=12)
    if c.p['stats'] == 'device':
        s1, s2 = _channel_stats(env, x.ptr(), NC, V, None), _channel_stats(env, x2.ptr(), NC, V, None)
        stats, stats2 = s1.fetch().reshape(NC, 4), s2.fetch().reshape(NC, 4)
        p1, p2 = s1.ptr(), s2.ptr()
        if c.p['kind'] == 'constant':                    # the statistics the references are built from: exact for a constant channel
            for st, v in ((stats, d['x'][:, 0]), (stats2, d['x2'][:, 0])):
                _fig('channel_stats_finalize_kernel', cid, 'largest-sd-of-a-constant-channel', np.abs(st[:, 3]).max())
                assert (st[:, 3] == 0.0).all() and (st[:, 0] == v).all() and (st[:, 1] == v).all() and (st[:, 2] == v).all(), st
    else:
        s1, s2 = Source(env, d['stats']), Source(env, d['stats2'])
        stats, stats2, p1, p2 = d['stats'], d['stats2'], s1.ptr(), s2.ptr()
    rec = (_lib.mt_intensity_op_t * NC)(*[_lib.mt_intensity_op_t(op, fl, a, b) for op, fl, a, b in d['records']])
    _lib.check(lib.mt_intensity_apply(x.ptr(), NC, V, rec, p1, p2, _stream()), 'intensity_apply')
    torch.cuda.synchronize()
    got = x.fetch().reshape(NC, V)
    assert x2.unchanged() and (c.p['stats'] == 'device' or (s1.unchanged() and s2.unchanged())), "mt_intensity_apply changed a source"
    if c.p['stats'] == 'device':
        assert np.array_equal(VC.bits(s1.fetch()), VC.bits(stats.ravel())) and np.array_equal(VC.bits(s2.fetch()), VC.bits(stats2.ravel()))
    exp = VC.apply_expected(d, stats, stats2)
    for ch, (op, flags, a, b) in enumerate(d['records']):
        r32, r64 = exp[ch]
        name = '%s/ch%d-op%d-flags%d' % (cid, ch, op, flags)
        if op == VC.OP_NONE:
            assert np.array_equal(VC.bits(got[ch]), VC.bits(d['x'][ch])), "a channel without an op was written"
            continue
        assert np.isfinite(got[ch]).all(), name
        if op == VC.OP_GAMMA:
            ratio = VC.gamma_ratio(got[ch], r32, r64, d['x'][ch])
            _fig('ia_run<%s>' % VC.OP_NAMES[op], name, 'ratio', ratio)
            _fig('ia_run<%s>' % VC.OP_NAMES[op], name, 'worst-ratio-so-far', _worst('gamma', ratio))
            assert ratio <= VC.GAMMA_RATIO
        else:
            wrong = VC.bits(got[ch]) != VC.bits(r32)
            ulp = float((np.abs(got[ch].astype(np.float64) - r32) / np.spacing(np.abs(r32)).astype(np.float64))[wrong].max()) if wrong.any() else 0.0
            _fig('ia_run<%s>' % VC.OP_NAMES[op], name, 'worst-ulp', ulp)
            _fig('ia_run<%s>' % VC.OP_NAMES[op], name, 'mismatching-elements', wrong.sum())
            assert not wrong.any(), (np.flatnonzero(wrong)[:5], got[ch][wrong][:5], r32[wrong][:5])


# ================================================================================================================================
# G. mt_ensemble_classify
@pytest.mark.parametrize('cid', _ids('ens'))
@stops_on_hip_error
def test_ensemble_classify(env, cid):
    """np.argmax with the first NaN winning, `> 0.5` with NaN never above it, class_order & 255 on the 8-byte, the two 4-byte and the
    bytewise store; the float16 mean bit for bit (NaN for NaN) where the case asks for it"""
    c, d = _case(env, 'ens', cid)
    lib, _lib, p = env['lib'], env['_lib'], c.p
    K, C, (D, H, W), V = p['K'], p['C'], p['shape'], d['V']
    cs = -(-V // 8) * 8
    held = []
    for m in d['members']:
        pad = np.zeros((C, cs), np.float16)
        pad[:, :V] = m
        held.append(Source(env, pad, offset=0 if p['wide'] else 2))
    ptrs = (ctypes.c_void_p * K)(*[h.ptr() for h in held])
    assert all((h.ptr() % 16 == 0) == p['wide'] for h in held)
    order = Source(env, np.array(p['order'], np.int32)) if p['regions'] else None
    out = Guarded(env, np.uint8, V, offset=p['out_off'])
    assert out.ptr() % 8 == p['out_off']
    mean = Guarded(env, np.float16, C * cs, offset=0 if p['wide'] else 2) if p.get('mean') else None
    _lib.check(lib.mt_ensemble_classify(ptrs, K, C, D, H, W, cs, order.ptr() if order else None, p['regions'], out.ptr(), D, H, W, 0, 0, 0,
                                        mean.ptr() if mean else None, cs if mean else 0, _stream()), 'ensemble_classify')
    torch.cuda.synchronize()
    got = out.fetch()
    assert all(h.unchanged() for h in held) and (order is None or order.unchanged()), "mt_ensemble_classify changed a source"
    if mean is not None:
        gm = mean.fetch().reshape(C, cs)
        same = (VC.bits(gm[:, :V]) == VC.bits(d['mean'])) | (np.isnan(gm[:, :V]) & np.isnan(d['mean']))
        _fig(VC.instances(c)[0], cid, 'wrong-means', (~same).sum())
        assert same.all() and mean.sentinels(gm[:, V:].reshape(-1)).all()
    wrong = got != d['lab'].ravel()
    _fig(VC.instances(c)[0], cid, 'wrong-labels', wrong.sum())
    assert not wrong.any(), (np.flatnonzero(wrong)[:8], got[wrong][:8], d['lab'].ravel()[wrong][:8])


# ================================================================================================================================
# Refusals: the code comes back before any launch
@stops_on_hip_error
def test_refused_calls_launch_nothing(env):
    lib, _lib, dev = env['lib'], env['_lib'], env['dev']
    vol = Source(env, np.ones((4, 5, 6), np.uint8))
    member, remap, s = _u8([0] + [1] * 255), _u8([0] * 256), _stream()
    dst = dict(hist=Guarded(env, np.int64, 257 * 257), out=Guarded(env, np.float64, 256), sdstats=Guarded(env, np.float64, 6),
               labels=Guarded(env, np.int32, 120), sizes=Guarded(env, np.int32, 120), ccstats=Guarded(env, np.int32, 2), bbox=Guarded(env, np.int32, 7),
               stats=Guarded(env, np.float64, 8), lab=Guarded(env, np.uint8, 120))
    ws = _workspace(env, 1 << 20)
    sdn, fhn, csn = lib.mt_surface_distances_workspace(4, 5, 6, 256), lib.mt_fill_holes3d_workspace(4, 5, 6), lib.mt_channel_stats_workspace(2, 60)
    assert 0 < max(sdn, fhn, csn) < (1 << 20)
    assert lib.mt_surface_distances_workspace(4, 5, 6, 0) == 0 and lib.mt_fill_holes3d_workspace(0, 5, 6) == 0 and lib.mt_channel_stats_workspace(2, 0) == 0
    mask = Guarded(env, np.uint8, 120, init=np.zeros(120, np.uint8))
    x = Guarded(env, np.float32, 120, init=np.arange(120, dtype=np.float32))
    st = Source(env, np.ones(8))
    halves = Source(env, np.full((2, 128), 0.75, np.float16))
    sp = (ctypes.c_double * 3)(1.0, 1.0, 1.0)

    def rec(*ops):
        return (_lib.mt_intensity_op_t * len(ops))(*[_lib.mt_intensity_op_t(op, 0, 1.0, 0.0) for op in ops])

    def sd(conn, capacity, wsn):
        return lib.mt_surface_distances(vol.ptr(), vol.ptr(), 4, 5, 6, member, sp, conn, dst['out'].ptr(), capacity, dst['sdstats'].ptr(), ws.ptr(), wsn, s)

    def ens(bD, bW):
        ptrs = (ctypes.c_void_p * 2)(halves.ptr(), halves.ptr())
        return lib.mt_ensemble_classify(ptrs, 2, 1, 4, 5, 6, 128, None, 0, dst['lab'].ptr(), 4, 5, 6, bD, 0, bW, None, 0, s)

    calls = [('hist C=0', lambda: lib.mt_seg_joint_hist(vol.ptr(), vol.ptr(), 120, remap, 0, dst['hist'].ptr(), s), EINVAL),
             ('hist C=257', lambda: lib.mt_seg_joint_hist(vol.ptr(), vol.ptr(), 120, remap, 257, dst['hist'].ptr(), s), EINVAL),
             ('hist V=0', lambda: lib.mt_seg_joint_hist(vol.ptr(), vol.ptr(), 0, remap, 3, dst['hist'].ptr(), s), EINVAL),
             ('hist V<0', lambda: lib.mt_seg_joint_hist(vol.ptr(), vol.ptr(), -5, remap, 3, dst['hist'].ptr(), s), EINVAL),
             ('sd connectivity 0', lambda: sd(0, 256, sdn), EINVAL), ('sd connectivity 4', lambda: sd(4, 256, sdn), EINVAL),
             ('sd capacity 0', lambda: sd(1, 0, sdn), EINVAL), ('sd workspace one byte short', lambda: sd(1, 256, sdn - 1), EINVAL),
             ('cc D=0', lambda: lib.mt_cc_label3d(vol.ptr(), 0, 5, 6, member, dst['labels'].ptr(), dst['sizes'].ptr(), dst['ccstats'].ptr(), s), EINVAL),
             ('fh W=0', lambda: lib.mt_fill_holes3d(mask.ptr(), 4, 5, 0, dst['bbox'].ptr(), ws.ptr(), fhn, s), EINVAL),
             ('fh workspace one byte short', lambda: lib.mt_fill_holes3d(mask.ptr(), 4, 5, 6, dst['bbox'].ptr(), ws.ptr(), fhn - 1, s), EWORKSPACE),
             ('stats V=0', lambda: lib.mt_channel_stats(x.ptr(), 2, 0, None, dst['stats'].ptr(), ws.ptr(), csn, s), EINVAL),
             ('stats workspace one byte short', lambda: lib.mt_channel_stats(x.ptr(), 2, 60, None, dst['stats'].ptr(), ws.ptr(), csn - 1, s), EINVAL),
             ('apply unknown op', lambda: lib.mt_intensity_apply(x.ptr(), 2, 60, rec(VC.OP_SCALE, 5), st.ptr(), st.ptr(), s), EINVAL),
             ('apply op -1', lambda: lib.mt_intensity_apply(x.ptr(), 2, 60, rec(VC.OP_SCALE, -1), st.ptr(), st.ptr(), s), EINVAL),
             ('apply missing stats', lambda: lib.mt_intensity_apply(x.ptr(), 2, 60, rec(VC.OP_SCALE, VC.OP_CONTRAST), None, None, s), EINVAL),
             ('apply missing stats2', lambda: lib.mt_intensity_apply(x.ptr(), 2, 60, rec(VC.OP_SCALE, VC.OP_RESTORE), st.ptr(), None, s), EINVAL),
             ('ensemble offset d outside', lambda: ens(4, 0), EINVAL), ('ensemble offset w outside', lambda: ens(0, 6), EINVAL),
             ('ensemble offset negative', lambda: ens(0, -1), EINVAL)]
    for what, call, code in calls:
        rc = call()
        print('VOLUME-FIG refusal %s rc %d' % (what, rc))
        assert rc == code and lib.mt_last_error(), what
    torch.cuda.synchronize()
    for name, g in dst.items():
        assert g.untouched(), "a refused call wrote %s" % name
    assert ws.untouched(), "a refused call wrote the workspace"
    assert not mask.fetch().any() and np.array_equal(x.fetch(), np.arange(120, dtype=np.float32))
    assert vol.unchanged() and st.unchanged() and halves.unchanged()
