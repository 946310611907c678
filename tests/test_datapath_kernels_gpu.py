"""The data path on real memory against numpy: every entry point of csrc/preproc.hip, csrc/analyze.hip, csrc/crop.hip, csrc/loader.hip and
csrc/select.hip through the library's C interface (ctypes: alignment, workspace and capacity are this file's to choose).  Cases,
references and bounds are tests/datapath_cases.py (see its docstring), evaluated at the device's own CU count;
tests/test_datapath_cases_cpu.py checks the references and what the cases reach.  Every destination starts as a sentinel (NaN bits for
floats, -12345 / 0x77 for integers) between guard bytes; after a launch the guards and every source are bit-identical, no sentinel is
left where a value is due and every assigned byte equals the reference.  Every figure is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import datapath_cases as DC

pytestmark = pytest.mark.gpu
GUARD_BYTE, GUARD_BYTES = 0xA5, 256


def _ids(family):
    return [c.id for c in DC.cases(family, 256)]          # the ids do not depend on the CU count


@pytest.fixture(scope='module')
def env(dev):
    from multitalent_amd import _lib
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    tables = {f: {c.id: c for c in DC.cases(f, cus)} for f in DC.FAMILIES}
    return dict(dev=dev, lib=_lib.load(), _lib=_lib, cus=cus, geo=DC.geometry(cus), tables=tables)


def _case(env, family, cid):
    c = env['tables'][family][cid]
    return c, DC.build(family, c, env['cus'])


def stops_on_hip_error(fn):
    """A HIP error ends the whole run: nothing more is launched on a device that has faulted (as test_spatial_kernels_gpu)."""
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
    print('DATAPATH-FIG %s %s %s %.3e' % (kernel, case_id, what, value))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sentinel(dtype, n):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.full(n, DC.F32_SENTINEL_BITS, np.uint32).view(np.float32)
    if dtype == np.float64:
        return np.full(n, 0x7ff8deaddeaddead, np.uint64).view(np.float64)
    if dtype.kind == 'i' and dtype.itemsize > 1:
        return np.full(n, DC.INT_SENTINEL, dtype)
    return np.full(n * dtype.itemsize, DC.BYTE_SENTINEL, np.uint8).view(dtype)


class Source(object):
    """an operand the kernel only reads, at a chosen byte offset from a 256-byte boundary; compared bit for bit afterwards"""

    def __init__(self, env, host, offset=0):
        self.host = np.ascontiguousarray(host)
        raw = self.host.reshape(-1).view(np.uint8)
        self.off, self.nbytes = GUARD_BYTES + offset, raw.size
        buf = np.full(self.off + raw.size + GUARD_BYTES, GUARD_BYTE, np.uint8)
        buf[self.off:self.off + raw.size] = raw
        self.image = buf
        self.dev = torch.from_numpy(buf.copy()).to(env['dev'])

    def ptr(self):
        return self.dev.data_ptr() + self.off

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy(), self.image)


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

    def fetch(self):
        after = self.dev.cpu().numpy()
        assert (after[:self.off] == GUARD_BYTE).all() and (after[self.off + self.nbytes:] == GUARD_BYTE).all(), "guard bytes around a destination changed"
        return after[self.off:self.off + self.nbytes].copy().view(self.dtype)

    def sentinels(self, got):
        """elements of got that still hold the sentinel"""
        return DC.bits(got) == DC.bits(_sentinel(self.dtype, got.size))


def _workspace(env, nbytes):
    return Guarded(env, np.uint8, max(int(nbytes), 8))


# ================================================================================================================================
# A. mt_masked_moments
_WORST = {}


def _moments(env, d, pred):
    lib, _lib = env['lib'], env['_lib']
    C, V = d['C'], d['V']
    data, seg = Source(env, d['data'], offset=4), Source(env, d['seg'], offset=12)
    lo = (ctypes.c_double * C)(*d['lo'])
    hi = (ctypes.c_double * C)(*d['hi'])
    wsn = lib.mt_masked_moments_workspace(C, V)
    outs = []
    for _ in range(2):
        stats, ws = Guarded(env, np.float64, 3 * C), _workspace(env, wsn)
        _lib.check(lib.mt_masked_moments(data.ptr(), C, V, pred, seg.ptr(), lo, hi, stats.ptr(), ws.ptr(), wsn, _stream()), 'masked_moments')
        torch.cuda.synchronize()
        ws.fetch()
        outs.append(stats.fetch())
    assert data.unchanged() and seg.unchanged(), "mt_masked_moments changed a source"
    assert np.array_equal(DC.bits(outs[0]), DC.bits(outs[1])), "two runs of mt_masked_moments differ"
    return outs[0].reshape(C, 3)


@pytest.mark.parametrize('cid', _ids('moments'))
@stops_on_hip_error
def test_masked_moments(env, cid):
    """count exact; mean and sd within 1e-12 of the data's magnitude of the math.fsum reference; numpy's non-finite results in kind"""
    c, d = _case(env, 'moments', cid)
    geo = env['geo']
    if c.p.get('trip2'):
        beyond = DC.quad_trip(geo)
        assert d['V'] > beyond and all(r[4][beyond:].any() for r in d['refs']), "the case does not reach a second trip"
    got = _moments(env, d, c.p['pred'])
    worst = 0.0
    for ch, (n, mean, sd, scale, _) in enumerate(d['refs']):
        ok_m, e_m = DC.moments_close(got[ch, 1], mean, scale)
        ok_s, e_s = DC.moments_close(got[ch, 2], sd, scale, sd_ref=sd)
        _fig('moments_kernel<%d>' % c.p['pred'], cid, 'ch%d-count-diff' % ch, got[ch, 0] - n)
        _fig('moments_kernel<%d>' % c.p['pred'], cid, 'ch%d-mean-err/scale' % ch, e_m)
        _fig('moments_kernel<%d>' % c.p['pred'], cid, 'ch%d-sd-err/scale' % ch, e_s)
        worst = max(worst, e_m, e_s)
        assert got[ch, 0] == n, (got[ch], n)
        assert ok_m and ok_s, (got[ch], (n, mean, sd), scale)
    key = c.p['pred']
    _WORST[key] = max(_WORST.get(key, 0.0), worst)
    _fig('moments_kernel<%d>' % key, cid, 'worst-err/scale-so-far', _WORST[key])


# ================================================================================================================================
# B. mt_intensity_normalize
@pytest.mark.parametrize('cid', _ids('normalize'))
@stops_on_hip_error
def test_intensity_normalize(env, cid):
    """numpy's float32 expression bit for bit (NaN for NaN), in place between guards"""
    c, d = _case(env, 'normalize', cid)
    lib, _lib, p = env['lib'], env['_lib'], c.p
    V = d['data'].size
    if p.get('trip2'):
        beyond = DC.quad_trip(env['geo'])
        assert V > beyond and (DC.bits(d['ref'][beyond:]) != DC.bits(d['data'][beyond:])).any()
    x = Guarded(env, np.float32, V, offset=4, init=d['data'])
    seg = Source(env, d['seg'], offset=8)
    stats = Source(env, d['stats'])
    _lib.check(lib.mt_intensity_normalize(x.ptr(), V, p['clip'], p['lo'], p['hi'], d['mean'], d['sd'], stats.ptr() if p['stats'] else None, d['eps'],
                                          seg.ptr() if p['masked'] else None, _stream()), 'intensity_normalize')
    torch.cuda.synchronize()
    got = x.fetch()
    assert seg.unchanged() and stats.unchanged(), "mt_intensity_normalize changed a source"
    wrong = ~DC.same_float_results(got, d['ref'])
    _fig('normalize_kernel', cid, 'mismatching-voxels', wrong.sum())
    assert not wrong.any(), (np.flatnonzero(wrong)[:5], d['data'][wrong][:5], d['seg'][wrong][:5], got[wrong][:5], d['ref'][wrong][:5])


# ================================================================================================================================
# C. mt_label_counts / mt_label_locations
@pytest.mark.parametrize('cid', _ids('label'))
@stops_on_hip_error
def test_label_counts_and_locations(env, cid):
    """counts, the ordered index list (up to the capacity) and every queried location are np.flatnonzero(slot == s), bit for bit"""
    c, d = _case(env, 'label', cid)
    lib, _lib, geo = env['lib'], env['_lib'], env['geo']
    V, nslots, L = d['V'], d['nslots'], d['L']
    if c.p.get('trip2'):
        beyond = DC.unit_trip(geo) * geo.unit
        assert V > beyond + geo.unit and (d['slot'][beyond:beyond + geo.unit] != DC.NOSLOT).any() and (d['slot'][beyond + geo.unit:] != DC.NOSLOT).any()
    if c.p.get('nq'):
        assert d['qslot'].size > geo.cap * geo.threads['preproc.hip'] and (d['out'][geo.cap * geo.threads['preproc.hip']:] >= 0).any()
    seg, table = Source(env, d['seg'], offset=4), Source(env, d['table'], offset=3)
    wsn = lib.mt_label_counts_workspace(V, nslots)
    ws = _workspace(env, wsn)
    counts = Guarded(env, np.int64, nslots)
    _lib.check(lib.mt_label_counts(seg.ptr(), V, table.ptr(), L, nslots, counts.ptr(), ws.ptr(), wsn, _stream()), 'label_counts')
    torch.cuda.synchronize()
    got_counts = counts.fetch()
    _fig('label_units_kernel<false>', cid, 'wrong-counts', (got_counts != d['counts']).sum())
    bad = np.flatnonzero(got_counts != d['counts'])
    assert bad.size == 0, ('slots', bad, 'got', got_counts[bad], 'want', d['counts'][bad])
    if d['total'] == 0:
        ws.fetch()
        return
    D, H, W = d['shape']
    cap, nq = d['cap'], d['qslot'].size
    idx = Guarded(env, np.int32, cap, offset=4)
    qslot, qrank = Source(env, d['qslot'], offset=4), Source(env, d['qrank'], offset=8)
    out = Guarded(env, np.int64, 3 * nq, offset=8)
    _lib.check(lib.mt_label_locations(seg.ptr(), D, H, W, table.ptr(), L, nslots, ws.ptr(), wsn, idx.ptr(), cap, qslot.ptr(), qrank.ptr(), nq,
                                      out.ptr(), _stream()), 'label_locations')
    torch.cuda.synchronize()
    ws.fetch()
    got_idx, got_out = idx.fetch(), out.fetch().reshape(nq, 3)
    assert all(s.unchanged() for s in (seg, table, qslot, qrank)), "a label kernel changed a source"
    due = min(cap, d['total'])
    _fig('label_units_kernel<true>', cid, 'sentinels-left', idx.sentinels(got_idx[:due]).sum())
    _fig('label_units_kernel<true>', cid, 'wrong-indices', (got_idx[:due] != d['idx'][:due]).sum())
    _fig('label_gather_kernel', cid, 'wrong-locations', (got_out != d['out']).any(1).sum())
    assert np.array_equal(got_idx[:due], d['idx'][:due])
    assert np.array_equal(got_out, d['out'])
    if c.p['cap'] < 0:
        assert (d['out'][(d['qslot'] == nslots - 1) & (d['qrank'] == d['counts'][-1] - 1)] == -1).all()       # the query that falls past it


# ================================================================================================================================
# D. mt_fg_sample_count / _gather
@pytest.mark.parametrize('cid', _ids('fg'))
@stops_on_hip_error
def test_fg_sample(env, cid):
    """the count, data[c][seg > 0][::stride][:out_cs] as bit patterns, the NaN counts; a short out_cs truncates inside the guards"""
    c, d = _case(env, 'fg', cid)
    lib, _lib, geo = env['lib'], env['_lib'], env['geo']
    V, C, cs = d['V'], d['C'], d['cs']
    if c.p.get('trip2'):
        beyond = DC.unit_trip(geo) * geo.unit
        ranks = np.cumsum(d['sel']) - 1
        late = d['sel'] & (ranks % d['stride'] == 0)
        assert V > beyond + geo.unit and late[beyond:beyond + geo.unit].any() and late[beyond + geo.unit:].any()
    data, seg = Source(env, d['data'], offset=4), Source(env, d['seg'], offset=12)
    wsn = lib.mt_fg_sample_workspace(V)
    ws = _workspace(env, wsn)
    count = Guarded(env, np.int64, 1)
    _lib.check(lib.mt_fg_sample_count(seg.ptr(), V, count.ptr(), ws.ptr(), wsn, _stream()), 'fg_sample_count')
    torch.cuda.synchronize()
    got_n = int(count.fetch()[0])
    _fig('fg_count_kernel', cid, 'count-diff', got_n - d['n'])
    assert got_n == d['n']
    out, nan = Guarded(env, np.float32, C * cs, offset=4), Guarded(env, np.int64, C)
    _lib.check(lib.mt_fg_sample_gather(data.ptr(), C, V, seg.ptr(), d['stride'], ws.ptr(), wsn, out.ptr(), cs, nan.ptr(), _stream()), 'fg_sample_gather')
    torch.cuda.synchronize()
    ws.fetch()
    got = out.fetch().reshape(C, cs)
    assert data.unchanged() and seg.unchanged(), "mt_fg_sample_gather changed a source"
    due = d['ref'].shape[1]
    wrong = (DC.bits(got[:, :due]) != d['ref']).sum()
    stray = (~out.sentinels(got[:, due:].reshape(-1))).sum()
    _fig('fg_gather_kernel', cid, 'wrong-samples', wrong)
    _fig('fg_gather_kernel', cid, 'writes-past-the-samples', stray)
    assert wrong == 0 and stray == 0
    assert np.array_equal(nan.fetch(), d['nan'])


# ================================================================================================================================
# E. mt_label_presence
def _presence(env, seg_ptr, V, bitmap_ptr, flag_ptr):
    env['_lib'].check(env['lib'].mt_label_presence(seg_ptr, V, bitmap_ptr, flag_ptr, _stream()), 'label_presence')


@stops_on_hip_error
def test_label_presence_of_every_label_alone(env):
    """1024 launches of one voxel each: label l sets bit l + 1 of its own row and nothing else"""
    c, d = _case(env, 'presence', 'pres-each-label-alone')
    n = d['seg'].size
    seg = Source(env, d['seg'], offset=4)
    bitmap, flag = Guarded(env, np.uint32, 32 * n, offset=4), Guarded(env, np.int32, n, offset=4)
    for i in range(n):
        _presence(env, seg.ptr() + 4 * i, 1, bitmap.ptr() + 128 * i, flag.ptr() + 4 * i)
    torch.cuda.synchronize()
    got, gflag = bitmap.fetch().reshape(n, 32), flag.fetch()
    assert seg.unchanged()
    ref = np.stack([r[0] for r in d['refs']])
    _fig('label_presence_kernel', c.id, 'wrong-rows', (got != ref).any(1).sum())
    assert np.array_equal(got, ref) and not gflag.any()


@pytest.mark.parametrize('cid', _ids('presence')[1:])
@stops_on_hip_error
def test_label_presence(env, cid):
    """np.unique as a bitmap; in the second-trip case every bad value alone raises the flag and leaves the bitmap right"""
    c, d = _case(env, 'presence', cid)
    V = d['V']
    variants = [(None, d['ref'])]
    if c.p.get('trip2'):
        beyond = DC.quad_trip(env['geo'], 'analyze.hip')
        assert V > beyond and d['second'] >= beyond and (d['seg'][beyond:4 * (V // 4)] == 900).sum() == 1 and (d['seg'] == 900).sum() == 1
        for bad in DC.BAD_LABELS:
            s = d['seg'].copy()
            s[d['second']] = bad
            variants.append((bad, DC.presence_ref(s)))
    for bad, (ref_map, ref_flag) in variants:
        host = d['seg'].copy()
        if bad is not None:
            host[d['second']] = bad
            assert ref_flag == 1 and np.array_equal(ref_map, d['ref'][0])
        seg = Source(env, host, offset=4)
        bitmap, flag = Guarded(env, np.uint32, 32, offset=4), Guarded(env, np.int32, 1, offset=4)
        _presence(env, seg.ptr(), V, bitmap.ptr(), flag.ptr())
        torch.cuda.synchronize()
        got, gflag = bitmap.fetch(), int(flag.fetch()[0])
        assert seg.unchanged()
        _fig('label_presence_kernel', '%s/%s' % (cid, bad), 'wrong-words', (got != ref_map).sum())
        _fig('label_presence_kernel', '%s/%s' % (cid, bad), 'flag', gflag)
        assert np.array_equal(got, ref_map) and gflag == ref_flag, (bad, got, ref_map, gflag)


# ================================================================================================================================
# F. mt_label_convert
@pytest.mark.parametrize('cid', _ids('convert'))
@stops_on_hip_error
def test_label_convert(env, cid):
    """the table's uint8 for every voxel, the count of unexpected voxels and the smallest of them; a head of one element and a tail"""
    c, d = _case(env, 'convert', cid)
    lib, _lib, geo = env['lib'], env['_lib'], env['geo']
    x, V = d['x'], d['V']
    isz = x.dtype.itemsize
    if c.p.get('trip2'):
        vt = geo.chunk64 if isz == 8 else geo.chunk
        beyond = d['head'] + geo.cap * geo.threads['analyze.hip'] * vt
        bad = np.flatnonzero((x.astype(np.float64) > 1e-20) & (d['out'] == 0) & (x != 100))
        assert V > beyond and bad.size == d['count'] == 3 and bad.min() >= beyond
        assert lib.mt_label_convert_round(DC.LABEL_DTYPES[d['dtype']]) == beyond - d['head']
    src = Source(env, x, offset=16 - isz * d['head'])
    out, report = Guarded(env, np.uint8, V, offset=3), Guarded(env, np.uint64, 2)
    table = (ctypes.c_uint16 * DC.LABEL_SLOTS)(*d['table'])
    _lib.check(lib.mt_label_convert(src.ptr(), DC.LABEL_DTYPES[d['dtype']], V, table, out.ptr(), report.ptr(), _stream()), 'label_convert')
    torch.cuda.synchronize()
    got, rep = out.fetch(), report.fetch()
    assert src.unchanged()
    kernel = 'label_convert_kernel<%s>' % DC.LABEL_CTYPES[d['dtype']]
    _fig(kernel, cid, 'wrong-voxels', (got != d['out']).sum())
    _fig(kernel, cid, 'count-diff', int(rep[0]) - d['count'])
    assert np.array_equal(got, d['out']) and int(rep[0]) == d['count'] and int(rep[1]) == d['key'], (rep, d['count'], d['key'])


# ================================================================================================================================
# G. mt_nonzero_mask
@pytest.mark.parametrize('cid', _ids('mask'))
@stops_on_hip_error
def test_nonzero_mask(env, cid):
    c, d = _case(env, 'mask', cid)
    geo = env['geo']
    g = geo.cap * geo.threads['crop.hip']
    assert (d['V'] - d['head']) // 4 > 3 * g and d['ref'].sum() == d['at'].size
    data = Source(env, d['data'], offset=4)
    mask = Guarded(env, np.uint8, d['V'], offset=4 - d['head'])
    env['_lib'].check(env['lib'].mt_nonzero_mask(data.ptr(), 2, d['V'], mask.ptr(), _stream()), 'nonzero_mask')
    torch.cuda.synchronize()
    got = mask.fetch()
    assert data.unchanged()
    _fig('nz_mask_kernel', cid, 'wrong-bytes', (got != d['ref']).sum())
    assert np.array_equal(got, d['ref'])


# ================================================================================================================================
# H. mt_crop_nonzero
@pytest.mark.parametrize('cid', _ids('crop'))
@stops_on_hip_error
def test_crop_nonzero(env, cid):
    c, d = _case(env, 'crop', cid)
    lib, _lib, p = env['lib'], env['_lib'], c.p
    D, H, W = p['shape']
    if p.get('trip2'):
        assert d['out'][0].size > env['geo'].cap * env['geo'].threads['crop.hip']
    data, mask = Source(env, d['data'], offset=4), Source(env, d['mask'], offset=1)
    seg = Source(env, d['seg'], offset=8) if p['seg_mode'] else None
    box = (ctypes.c_int32 * 6)(*d['box'])
    out = Guarded(env, np.float32, d['out'].size, offset=4)
    seg_out = Guarded(env, d['seg_out'].dtype, d['seg_out'].size, offset=4 if p['seg_mode'] else 1)
    _lib.check(lib.mt_crop_nonzero(data.ptr(), p['C'], D, H, W, mask.ptr(), ctypes.cast(box, ctypes.c_void_p), out.ptr(), seg.ptr() if seg else None, p['CS'],
                                   seg_out.ptr(), d['label'], _stream()), 'crop_nonzero')
    torch.cuda.synchronize()
    got, got_seg = out.fetch(), seg_out.fetch()
    assert data.unchanged() and mask.unchanged() and (seg is None or seg.unchanged())
    kernel = 'crop_kernel<%d>' % p['seg_mode']
    _fig(kernel, cid, 'wrong-data-bits', (DC.bits(got) != DC.bits(d['out']).reshape(-1)).sum())
    _fig(kernel, cid, 'wrong-seg-bits', (DC.bits(got_seg) != DC.bits(d['seg_out']).reshape(-1)).sum())
    assert np.array_equal(DC.bits(got), DC.bits(d['out']).reshape(-1))
    assert np.array_equal(DC.bits(got_seg), DC.bits(d['seg_out']).reshape(-1))


# ================================================================================================================================
# I. mt_patch_gather
@pytest.mark.parametrize('cid', _ids('gather'))
@stops_on_hip_error
def test_patch_gather(env, cid):
    """np.pad of the intersection box for every sample of the launch, bit for bit"""
    c, d = _case(env, 'gather', cid)
    lib, _lib, geo, p = env['lib'], env['_lib'], env['geo'], c.p
    n, (PD, PH, PW) = len(d['srcs']), p['P']
    if p.get('trip2'):
        assert PD * PH * ((PW + 3) // 4) * n > geo.cap * geo.threads['loader.hip'] and PD * PH * ((PW + 3) // 4) > (geo.cap // n) * geo.threads['loader.hip']
    descs = (_lib.mt_patch_src_t * n)()
    held = []
    for j, s in enumerate(d['srcs']):
        a, b = Source(env, s['data'], offset=4 * s['data_off']), Source(env, s['seg'], offset=2 * s['seg_off'])
        held += [a, b]
        descs[j].data, descs[j].seg = a.ptr(), b.ptr()
        descs[j].shape[:], descs[j].lb[:] = s['shape'], s['lb']
    dout, sout = Guarded(env, np.float32, d['data_ref'].size, offset=4), Guarded(env, np.float32, d['seg_ref'].size, offset=12)
    _lib.check(lib.mt_patch_gather(descs, n, p['C'], PD, PH, PW, p['pad'], d['fill'], dout.ptr(), sout.ptr(), _stream()), 'patch_gather')
    torch.cuda.synchronize()
    gd, gs = dout.fetch(), sout.fetch()
    assert all(h.unchanged() for h in held), "mt_patch_gather changed a source"
    wd = (DC.bits(gd) != DC.bits(d['data_ref']).reshape(-1)).sum()
    ws_ = (DC.bits(gs) != DC.bits(d['seg_ref']).reshape(-1)).sum()
    _fig('patch_gather_kernel', cid, 'wrong-data-bits', wd)
    _fig('patch_gather_kernel', cid, 'wrong-label-bits', ws_)
    assert wd == 0 and ws_ == 0


# ================================================================================================================================
# J. mt_seg_narrow
@pytest.mark.parametrize('cid', _ids('narrow'))
@stops_on_hip_error
def test_seg_narrow(env, cid):
    """int16 bit for bit wherever the value is representable; the flag exactly when one is not"""
    c, d = _case(env, 'narrow', cid)
    V = d['V']
    if c.p.get('trip2'):
        beyond = DC.quad_trip(env['geo'], 'loader.hip')
        assert V > beyond and (c.p['bad'] is None or not d['good'][beyond:].all())
    seg = Source(env, d['seg'], offset=4)
    out, flag = Guarded(env, np.int16, V, offset=8), Guarded(env, np.int32, 1, init=[0])
    env['_lib'].check(env['lib'].mt_seg_narrow(seg.ptr(), V, out.ptr(), flag.ptr(), _stream()), 'seg_narrow')
    torch.cuda.synchronize()
    got, gflag = out.fetch(), int(flag.fetch()[0])
    assert seg.unchanged()
    wrong = (got != d['ref'])[d['good']].sum()
    _fig('seg_narrow_kernel', cid, 'wrong-representable-voxels', wrong)
    _fig('seg_narrow_kernel', cid, 'flag', gflag)
    assert wrong == 0 and gflag == d['flag']


# ================================================================================================================================
# K. mt_select_kth / mt_select_kth_f32
@pytest.mark.parametrize('cid', _ids('select'))
@stops_on_hip_error
def test_select_kth(env, cid):
    """the rank-th key of the sorted keys for three rank sets (eight first-digit groups, one rank eight times, both ends), run twice"""
    c, d = _case(env, 'select', cid)
    lib, _lib, geo, p = env['lib'], env['_lib'], env['geo'], c.p
    width, n = p['width'], d['n']
    if p.get('trip2'):
        assert n // (16 // width) > geo.cap * geo.threads['select.hip'] and d['groups'] == (8 if p['kind'] == 'spread' else 3)
    fn, wsn = (lib.mt_select_kth_f32, lib.mt_select_kth_f32_workspace(8)) if width == 4 else (lib.mt_select_kth, lib.mt_select_kth_workspace(8))
    x = Source(env, d['bits'], offset=width * p['off'])
    for ranks, ref in zip(d['ranksets'], d['refs']):
        rk = (ctypes.c_long * len(ranks))(*ranks)
        outs = []
        for _ in range(2):
            out, ws = Guarded(env, d['bits'].dtype, len(ranks), offset=width), _workspace(env, wsn)
            _lib.check(fn(x.ptr(), n, ctypes.cast(rk, ctypes.c_void_p), len(ranks), out.ptr(), ws.ptr(), wsn, _stream()), c.entry)
            torch.cuda.synchronize()
            ws.fetch()
            outs.append(out.fetch())
        _fig('sel_pick_kernel<%d>' % (8 * width), '%s/%d-ranks' % (cid, len(ranks)), 'wrong-ranks', (outs[0] != ref).sum())
        assert np.array_equal(outs[0], ref), (ranks, outs[0], ref)
        assert np.array_equal(outs[0], outs[1]), "two runs of %s differ" % c.entry
    assert x.unchanged()
