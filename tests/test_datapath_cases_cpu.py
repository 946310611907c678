"""tests/datapath_cases.py without a device: every reference against an independent statement of the same operation, and a census of
what the cases reach — every kernel and launchable template instance of the five units, every second trip at 256 CUs, class slots in
each of the four registers."""
import math
import re

import numpy as np
import pytest

import datapath_cases as DC

CUS = 256
GEO = DC.geometry(CUS)
ALL = [(f, c) for f in DC.FAMILIES for c in DC.cases(f, CUS)]


def fam(name):
    return DC.cases(name, CUS)


IDS = lambda c: c.id


def test_geometry_is_read_out_of_the_sources():
    assert GEO.cap == 8 * CUS and GEO.wave == 64 and GEO.unit == 8192 and GEO.scan_threads == 256 and GEO.maxranks == 8 and GEO.max_src == 16
    assert set(GEO.threads.values()) == {256} and (GEO.chunk, GEO.chunk64) == (16, 8)
    assert DC.geometry(304).cap == 8 * 304


def test_ids_are_unique_and_do_not_depend_on_the_cu_count():
    ids = [c.id for _, c in ALL]
    assert len(set(ids)) == len(ids)
    assert ids == [c.id for f in DC.FAMILIES for c in DC.cases(f, 304)]


def test_census_every_kernel_and_launchable_instance_has_a_case():
    reached = set()
    for _, c in ALL:
        reached.update(DC.instances(c))
    known = DC.launchable_instances()
    missing = [k for k in known if k not in reached]
    print('DATAPATH-CENSUS %d cases reach %d of %d instances' % (len(ALL), len(reached & set(known)), len(known)))
    assert not missing and reached <= set(known), (missing, reached - set(known))


def test_census_fails_on_a_kernel_the_table_does_not_know():
    names = {re.sub(r'<.*', '', k) for k in DC.launchable_instances()}
    in_sources = {k for ks in DC.kernels_in_sources().values() for k in ks}
    assert in_sources == names, (in_sources ^ names)
    # the template arguments the entry points pass
    pre, ana, crop, sel = DC.read('preproc.hip'), DC.read('analyze.hip'), DC.read('crop.hip'), DC.read('select.hip')
    assert sorted(set(re.findall(r'PP_LAUNCH\((MT_MOMENTS_\w+)\)', pre))) == ['MT_MOMENTS_ALL', 'MT_MOMENTS_OPEN_RANGE', 'MT_MOMENTS_SEG_GE0']
    assert set(re.findall(r'moments_kernel<PRED, (\d)>', pre)) == {'0', '1'}
    assert set(re.findall(r'label_units_kernel<(\w+)>', pre)) == {'false', 'true'}
    assert set(re.findall(r'lc_launch<(\w+)>', ana)) == set(DC.LABEL_CTYPES.values())
    assert set(re.findall(r'hipLaunchKernelGGL\(crop_kernel<(\d)>', crop)) == {'0', '1'}
    assert set(re.findall(r'sel_launch<(\w+)>', sel)) == {'uint32_t', 'uint64_t'}


def test_every_stride_loop_has_a_case_that_makes_a_second_trip():
    trip2 = {}
    for f, c in ALL:
        if c.p.get('trip2') or c.p.get('nq'):
            for k in DC.instances(c):
                trip2.setdefault(k, []).append(c.id)
    loops = [k for k in DC.launchable_instances() if not re.match(r'moments_finalize|label_scan|label_base|fg_scan|sel_init|sel_pick', k)]
    loops = [k for k in loops if not k.startswith('label_convert_kernel') or re.search(r'<(uint8_t|int16_t|int32_t|double)>', k)]   # one per item size
    assert all(k in trip2 for k in loops), [k for k in loops if k not in trip2]


# ---- moments ---------------------------------------------------------------------------------------------------------------------
def test_moments_numpy_meets_the_bound_on_every_case():
    """numpy's own float64 mean / std against the fsum reference: well inside 1e-12 of the data's magnitude"""
    worst = 0.0
    preds = set()
    for c in fam('moments'):
        d = DC.build('moments', c, CUS)
        preds.add(c.p['pred'])
        if c.p.get('trip2'):
            assert d['V'] > DC.quad_trip(GEO) and d['V'] % 4 and all(r[4][DC.quad_trip(GEO):].any() for r in d['refs'])
        for ch, (n, mean, sd, scale, sel) in enumerate(d['refs']):
            x = d['data'][ch][sel]
            assert n == sel.sum()
            if n == 0:
                assert math.isnan(mean) and math.isnan(sd)
                continue
            with np.errstate(invalid='ignore'):
                m, s = float(x.mean(dtype=np.float64)), float(x.astype(np.float64).std())
            ok_m, e_m = DC.moments_close(m, mean, scale)
            ok_s, e_s = DC.moments_close(s, sd, scale, sd_ref=sd)
            assert ok_m and ok_s, (c.id, ch, m, mean, s, sd)
            worst = max(worst, e_m, e_s)
    print('DATAPATH-FIG numpy moments worst-err/scale %.3e' % worst)
    assert preds == {0, 1, 2} and worst <= DC.MOMENT_BOUND / 100


def test_moments_cases_hold_their_edges():
    byid = {c.id: DC.build('moments', c, CUS) for c in fam('moments') if c.p['V'] <= 1027}
    d = byid['mom-p2-on-the-bounds']
    for ch in range(2):
        x, sel = d['data'][ch], d['refs'][ch][4]
        assert (x == d['lo'][ch]).any() and (x == d['hi'][ch]).any() and not sel[(x == d['lo'][ch]) | (x == d['hi'][ch])].any()
        assert sel[x == np.nextafter(np.float32(d['lo'][ch]), np.float32(0))].all()
    d = byid['mom-p1-seg-edges']
    sel, seg = d['refs'][0][4], d['seg']
    assert sel[DC.bits(seg) == 0x80000000].all() and not sel[np.isnan(seg)].any() and not sel[DC.bits(seg) == 0x80000001].any() and sel[seg == np.inf].all()
    for kind, want in (('nan', math.isnan), ('pinf', lambda v: v == math.inf), ('ninf', lambda v: v == -math.inf), ('bothinf', math.isnan)):
        for pred in (0, 1):
            n, mean, sd, _, _ = byid['mom-p%d-%s' % (pred, kind)]['refs'][0]
            assert want(mean) and math.isnan(sd), (kind, pred, mean, sd)
        assert math.isfinite(byid['mom-p2-%s' % kind]['refs'][0][1])          # the open range leaves them out
    for pred in (1, 2):
        assert byid['mom-p%d-empty' % pred]['refs'][0][:3] == (0,) + byid['mom-p%d-empty' % pred]['refs'][0][1:3] and \
            byid['mom-p%d-empty' % pred]['refs'][0][0] == 0
    assert {c.p['C'] for c in fam('moments')} >= {1, 3, 16} and {c.p['V'] for c in fam('moments')} >= {1, 2, 3, 4, 5, 1027}


# ---- normalize -------------------------------------------------------------------------------------------------------------------
def test_normalize_reference_keeps_nan_voxels_and_nan_seg():
    seen = set()
    for c in fam('normalize'):
        d = DC.build('normalize', c, CUS)
        p = c.p
        seen.add((p['clip'], p['masked'], p['stats'], p['lo'] == p['hi'] and p['clip'] == 1))
        if p.get('trip2'):
            assert d['data'].size > DC.quad_trip(GEO)
        if p['kind'] == 'ct':
            continue
        x, seg, ref = d['data'], d['seg'], d['ref']
        nanvox = np.isnan(x) & ~(seg < 0)
        assert nanvox.any() and np.isnan(ref[nanvox]).all()                  # a NaN passes the clip
        segnan = np.isnan(seg) & np.isfinite(x)
        assert segnan.any() and (ref[segnan] != 0).any()                     # a NaN in seg zeroes nothing
        assert (ref[seg < 0] == 0).all() and (DC.bits(seg) == 0x80000001).any() and (DC.bits(seg) == 0x80000000).any()
    assert {(0, 0), (0, 1), (1, 0), (1, 1)} <= {s[:2] for s in seen} and {0, 1} == {s[2] for s in seen} and any(s[3] for s in seen)
    d = DC.build('normalize', [c for c in fam('normalize') if c.id == 'norm-zero-mean-unit-sd'][0], CUS)
    keep = (np.abs(d['data']) <= 1) & ~(d['seg'] < 0)                         # (x - 0) / (1 + 0): bits unchanged, denormals and -0.0 included
    assert (DC.bits(d['ref'][keep]) == DC.bits(d['data'][keep])).all() and (DC.bits(d['data'][keep]) == 0x80000000).any() and \
        (DC.bits(d['data'][keep]) == 1).any()


# ---- labels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in fam('label') if c.p['V'] <= 6 * GEO.unit and not c.p.get('nq')], ids=IDS)
def test_label_reference_is_argwhere(case):
    d = DC.build('label', case, CUS)
    D, H, W = d['shape']
    seg3 = d['seg'].reshape(D, H, W)
    lab_of = {int(s): l for l, s in enumerate(d['table'][:d['L']]) if s < d['nslots']}
    assert sorted(lab_of) == list(range(d['nslots']))
    where = {s: np.argwhere(seg3 == np.float32(lab_of[s])) for s in range(d['nslots'])}
    for s in range(d['nslots']):
        assert len(where[s]) == d['counts'][s]
    for (s, r), o in zip(zip(d['qslot'], d['qrank']), d['out']):
        inside = 0 <= s < d['nslots'] and 0 <= r < d['counts'][s] and int(np.concatenate([[0], np.cumsum(d['counts'])])[s]) + r < d['cap']
        assert (o == (where[s][r] if inside else -1)).all(), (s, r, o)
    if case.p['kind'] == 'slots':
        assert (d['counts'] > 0).all() and len(set(d['counts'].tolist())) == d['nslots']
        first = np.flatnonzero(d['slot'] == 0)
        assert first.min() >= 2 * GEO.unit - GEO.wave and first.max() < 2 * GEO.unit          # slot 0 first appears in the last round of unit 1
        rounds = d['slot'][:5 * GEO.unit].reshape(-1, GEO.wave)
        assert max(len(set(r[r != DC.NOSLOT].tolist())) for r in rounds) >= min(d['nslots'], 3)


def test_label_cases_census():
    cs = fam('label')
    assert tuple(c.p['nslots'] for c in cs if c.p['kind'] == 'slots') == DC.NSLOT_LADDER
    d = DC.build('label', [c for c in cs if c.id == 'lab-slots255'][0], CUS)
    assert {int(s) // GEO.wave for s in np.unique(d['slot']) if s != DC.NOSLOT} == {0, 1, 2, 3}             # all four registers
    assert set(DC.V_LADDER + (2 * GEO.unit + 5,)) <= {c.p['V'] for c in cs}
    assert {-(-c.p['V'] // GEO.unit) for c in cs} >= {GEO.scan_threads + 1, 2 * GEO.scan_threads + 1, DC.unit_trip(GEO) + 2}
    d = DC.build('label', [c for c in cs if c.id == 'lab-V8193'][0], CUS)
    for v in (0.5, -1, 5, 1e9, 4, 1):                                         # fractional, negative, >= L, L - 1 beyond nslots, listed as 255
        assert (d['slot'][d['seg'] == np.float32(v)] == DC.NOSLOT).all() and (d['seg'] == np.float32(v)).any()
    assert (d['slot'][np.isnan(d['seg'])] == DC.NOSLOT).all() and (d['slot'][DC.bits(d['seg']) == 0x80000000] == 1).all()
    d = DC.build('label', [c for c in cs if c.id == 'lab-capacity-one-short'][0], CUS)
    assert d['cap'] == d['total'] - 1
    d = DC.build('label', [c for c in cs if c.id == 'lab-many-queries'][0], CUS)
    assert d['qslot'].size > GEO.cap * 256


def test_label_big_case_passes_the_unit_cap():
    c = [c for c in fam('label') if c.id == 'lab-trip2'][0]
    V = c.p['V']
    assert -(-V // GEO.unit) == GEO.cap * 4 + 2 and V % GEO.unit and V <= 2 ** 31 - 1
    assert [k.id for k in fam('fg') if k.p.get('trip2')] == ['fg-trip2'] and fam('fg')[-1].p['V'] == V


# ---- foreground samples ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in fam('fg') if c.p['V'] <= 3 * GEO.unit + 5], ids=IDS)
def test_fg_reference_is_the_ranked_walk(case):
    """voxel by voxel: the k-th selected voxel is written to k / stride when stride divides k"""
    d = DC.build('fg', case, CUS)
    seg, stride = d['seg'], d['stride']
    k, out = 0, []
    for v in range(d['V']):
        if seg[v] > 0:
            if k % stride == 0 and k // stride < d['cs']:
                out.append(v)
            k += 1
    assert k == d['n'] and d['ref'].shape == (d['C'], len(out))
    assert (d['ref'] == DC.bits(d['data'])[:, out]).all()
    assert (d['nan'] == np.isnan(d['data'][:, out]).sum(1)).all()


def test_fg_cases_census():
    cs = fam('fg')
    strides = {c.p['stride'] for c in cs}
    assert strides >= {1, 2, 7, 10, GEO.unit - 1, GEO.unit, GEO.unit + 1, 'n', 'n+1', 2 ** 31, 2 ** 40}
    assert {c.p['cs'] for c in cs} == {0, 3, -2} and {c.p['C'] for c in cs} == {1, 16}
    d = DC.build('fg', [c for c in cs if c.id == 'fg-V8193-s1'][0], CUS)
    seg, sel = d['seg'], d['sel']
    assert sel[seg == 0.5].all() and sel[DC.bits(seg) == 1].all() and sel[seg == np.inf].all() and (DC.bits(seg) == 1).any()
    assert not sel[DC.bits(seg) == 0x80000000].any() and not sel[np.isnan(seg)].any() and (d['nan'] > 0).all()
    d = DC.build('fg', [c for c in cs if c.id == 'fg-stride10-cs-2'][0], CUS)
    assert d['cs'] == -(-d['n'] // 10) - 2


# ---- presence, convert, narrow -----------------------------------------------------------------------------------------------------
def test_presence_reference_is_unique():
    for c in fam('presence')[1:]:
        d = DC.build('presence', c, CUS)
        labs = np.unique(d['seg']).astype(int)
        want = np.zeros(32, np.uint32)
        for l in labs:
            want[(l + 1) // 32] |= np.uint32(1) << np.uint32((l + 1) % 32)
        assert (d['ref'][0] == want).all() and d['ref'][1] == 0
    d = DC.build('presence', fam('presence')[0], CUS)
    assert all(int(sum(bin(w).count('1') for w in r[0])) == 1 and r[1] == 0 for r in d['refs']) and len(d['refs']) == 1024
    for bad in DC.BAD_LABELS:
        assert DC.presence_ref(np.array([3, bad], np.float32))[1] == 1
    t = [c for c in fam('presence') if c.p.get('trip2')][0]
    assert t.p['V'] > DC.quad_trip(GEO, 'analyze.hip')


def test_convert_reference_is_the_rule_voxel_by_voxel():
    for c in fam('convert'):
        d = DC.build('convert', c, CUS)
        if c.p.get('trip2'):
            vt = GEO.chunk64 if d['x'].dtype.itemsize == 8 else GEO.chunk
            assert (d['V'] - d['head']) // vt > GEO.cap * 256 and d['count'] == 3
            continue
        cnt, low = 0, None
        for v, o in zip(d['x'].tolist(), d['out'].tolist()):
            v = float(v)
            if not v > 1e-20:
                want = 0
            elif math.isfinite(v) and v == int(v) and v <= 1022 and d['table'][int(v)] != DC.LABEL_UNLISTED:
                want = int(d['table'][int(v)])
            else:
                want, cnt, low = 0, cnt + 1, v if low is None else min(low, v)
            assert o == want
        assert cnt == d['count'] > 0 and d['key'] == int(np.array([low], np.float64).view(np.uint64)[0])
    assert {c.p['dtype'] for c in fam('convert')} == set(DC.LABEL_DTYPES)


def test_narrow_reference():
    seen = set()
    for c in fam('narrow'):
        d = DC.build('narrow', c, CUS)
        g = d['good']
        assert (d['ref'][g].astype(np.float32) == d['seg'][g]).all() and d['flag'] == (c.p['bad'] is not None)
        assert {-32768, 32767} <= set(d['ref'][:6].tolist()) or d['V'] < 4
        seen.add((c.p['bad'] if c.p['bad'] == c.p['bad'] else 'nan', c.p['where']))
        if c.p.get('trip2'):
            assert d['V'] > DC.quad_trip(GEO, 'loader.hip') and d['V'] % 4
    assert len(seen) == 3 * len(DC.NARROW_BAD) + 1


# ---- mask, crop, gather ------------------------------------------------------------------------------------------------------------
def test_mask_cases_place_their_non_zeros():
    g = GEO.cap * 256
    for c in fam('mask'):
        d = DC.build('mask', c, CUS)
        q = (np.flatnonzero(d['ref']) - d['head']) // 4
        nquad = (d['V'] - d['head']) // 4
        assert nquad > 3 * g
        if c.p['where'] == 'third-stride':
            assert (q >= 2 * g).all() and (q < 3 * g).all()
        elif c.p['where'] == 'last-q1':
            assert (q >= 3 * g).all() and (q < nquad).all()
        else:
            assert set(np.flatnonzero(d['ref']).tolist()) == {0, d['V'] - 2, d['V'] - 1}
        assert (DC.bits(d['data']) == 0x80000000).any()


def test_crop_reference_is_the_host_cropper():
    """cropping.crop_to_nonzero on a volume whose non-zero region is the box: the same data, the same seg with -0.0 outside the mask"""
    from multitalent_amd.preprocessing import cropping
    r = DC.rng('host-crop')
    for label in (-1, 2.5):
        data = np.zeros((2, 6, 7, 8), np.float32)
        data[:, 1:5, 2:6, 1:7] = r.standard_normal((2, 4, 4, 6)) * (r.uniform(size=(2, 4, 4, 6)) < 0.6)
        data[0, 1, 2, 1] = data[1, 4, 5, 6] = 1.0
        seg = np.array([0.0, -0.0, 1.0, -1.0], np.float32)[r.randint(0, 4, (3, 6, 7, 8))]
        mask = cropping.create_nonzero_mask(data)
        bbox = cropping.get_bbox_from_mask(mask, 0)
        box = [b for ab in bbox for b in ab]
        assert box == [1, 5, 2, 6, 1, 7] and not mask[1:5, 2:6, 1:7].all()
        hd, hs, _ = cropping.crop_to_nonzero(data.copy(), seg.copy(), nonzero_label=label)
        out, seg_out = DC.crop_ref(data, mask.astype(np.uint8), seg, box, np.float32(label))
        assert np.array_equal(DC.bits(out), DC.bits(hd)) and np.array_equal(DC.bits(seg_out), DC.bits(hs))
        assert ((DC.bits(seg[:, 1:5, 2:6, 1:7]) == 0x80000000) & (mask[1:5, 2:6, 1:7] == 0)[None]).any()
    hd, hs, _ = cropping.crop_to_nonzero(data.copy(), None, nonzero_label=-1)
    out, seg_out = DC.crop_ref(data, mask.astype(np.uint8), None, box, -1)
    assert np.array_equal(seg_out[None], hs)


def test_crop_cases_census():
    cs = fam('crop')
    for shape in ((3, 5, 7), (17, 33, 65)):
        mine = [c for c in cs if c.p['shape'] == shape]
        boxes = {tuple(c.p['box']) for c in mine}
        D, H, W = shape
        assert (0, D, 0, H, 0, W) in boxes and any(all(b[2 * a + 1] - b[2 * a] == 1 for a in range(3)) for b in boxes)
        for a, n in enumerate(shape):
            assert any(b[2 * a + 1] - b[2 * a] == 1 and all(b[2 * k + 1] - b[2 * k] == shape[k] for k in range(3) if k != a) for b in boxes)
            assert any(b[2 * a] == 0 and b[2 * a + 1] < n for b in boxes) and any(b[2 * a] > 0 and b[2 * a + 1] == n for b in boxes)
        assert {c.p['seg_mode'] for c in mine} == {0, 1} and {c.p['CS'] for c in mine} == {0, 1, 3}
    assert {c.p['label'] for c in cs} >= {-1, 2.5, 'nan'}
    for c in cs:
        if c.p.get('trip2'):
            b = c.p['box']
            assert (b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4]) > GEO.cap * 256


@pytest.mark.parametrize('case', fam('gather'), ids=IDS)
def test_gather_reference_is_the_clamped_index(case):
    """np.pad of the intersection equals 'every coordinate clamped into the source' (edge) / 'zero outside' (constant), sample by sample"""
    d = DC.build('gather', case, CUS)
    P, pad = case.p['P'], case.p['pad']
    outside = set()
    for j, s in enumerate(d['srcs']):
        ix, ins = zip(*[DC.gather_index(s['shape'][a], s['lb'][a], P[a], pad) for a in range(3)])
        inside = ins[0][:, None, None] & ins[1][None, :, None] & ins[2][None, None, :]
        got = s['data'][:, ix[0][:, None, None], ix[1][None, :, None], ix[2][None, None, :]]
        if pad == DC.PAD_CONSTANT:
            got = np.where(inside[None], got, np.float32(0))
        assert np.array_equal(DC.bits(got), DC.bits(d['data_ref'][j]))
        lab = np.where(inside, s['seg'][ix[0][:, None, None], ix[1][None, :, None], ix[2][None, None, :]].astype(np.float32), np.float32(d['fill']))
        assert np.array_equal(DC.bits(lab), DC.bits(d['seg_ref'][j]))
        for a in range(3):
            if not ins[a].any():
                outside.add((a, s['lb'][a] < 0))
    if case.p['kind'] == 'many':
        assert outside == {(a, side) for a in range(3) for side in (False, True)}
        assert {s['shape'][2] for s in d['srcs']} == {1, 2, 3, 4, 5} and len({s['shape'] for s in d['srcs']}) >= 12
        assert {s['data_off'] for s in d['srcs']} == {1, 2, 3} and all(s['seg_off'] % 2 for s in d['srcs'])


def test_gather_cases_census():
    cs = fam('gather')
    assert {c.p['P'][2] for c in cs if c.p['kind'] == 'many'} == set(DC.PATCH_WIDTHS) and {c.p['pad'] for c in cs} == {0, 1}
    assert {c.p['n'] for c in cs} >= {1, GEO.max_src} and {c.p['C'] for c in cs} >= {1, 3} and {c.p['fill'] for c in cs} >= {'nan'}
    for c in cs:
        if c.p.get('trip2'):
            PD, PH, PW = c.p['P']
            assert PD * PH * ((PW + 3) // 4) > (GEO.cap // c.p['n']) * 256
    # full quads (four outputs) whose source run ends exactly at the source's last voxel, and one voxel beyond it
    ends = set()
    for c in cs:
        PW = c.p['P'][2]
        for shape, lb in DC.gather_sources(c, GEO):
            ends |= {lb[2] + w0 + 3 - (shape[2] - 1) for w0 in range(0, PW - 3, 4) if lb[2] + w0 >= 0}
    assert {0, 1} <= ends


# ---- select ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', fam('select'), ids=IDS)
def test_select_reference_is_sort_on_the_nan_free_part(case):
    d = DC.build('select', case, CUS)
    b = d['bits']
    F = np.float32 if case.p['width'] == 4 else np.float64
    x = b.view(F)
    keys = np.sort(DC.select_key(b))
    assert np.array_equal(DC.select_key(DC.select_unkey(keys)), keys)
    back = DC.select_unkey(keys).view(F)
    nn, np_ = int((np.isnan(x) & (b >> b.dtype.type(8 * b.itemsize - 1) == 1)).sum()), int(np.isnan(x).sum())
    mid = back[nn:back.size - (np_ - nn)]                                     # negative NaNs first, positive NaNs last
    assert not np.isnan(mid).any() and np.array_equal(mid, np.sort(x[~np.isnan(x)]))
    zeros = np.flatnonzero(mid == 0)
    if zeros.size > 1:
        assert np.all(np.diff(np.signbit(mid[zeros]).astype(int)) <= 0)       # -0.0 before +0.0
    for ranks, ref in zip(d['ranksets'], d['refs']):
        assert np.array_equal(ref, DC.select_unkey(keys[np.array(ranks)]))
    if case.p.get('trip2'):
        assert d['n'] // (16 // case.p['width']) > GEO.cap * 256 and d['groups'] == (8 if case.p['kind'] == 'spread' else 3) and len(set(d['ranksets'][1])) == 1
        assert d['ranksets'][2] == [0, d['n'] - 1] and case.p['off'] in (0, 1)
        assert int(d['refs'][2][0]) == int(b[0]) and int(d['refs'][2][1]) == int(b[-1])          # the extremes sit in the head and the tail
        if case.p['kind'] == 'spread':
            assert nn > 0 and np_ > nn and np.isinf(x).any() and (zeros.size > 1)
        else:
            assert len(set((b >> b.dtype.type(8)).tolist())) <= 3                # all bytes but the last agree (the two planted ends aside)
