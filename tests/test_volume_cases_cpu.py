"""tests/volume_cases.py without a device: every reference against an independent statement of the same operation (scipy's label,
binary_fill_holes, binary_erosion and distance_transform_edt, the medpy formulas of tests/evaluation_cases.py, np.bincount, numpy's
min / max / mean / std, tests/intensity_restatement.py), the inputs' own conditions (ties tie, capacities truncate, misalignments
leave a head, a vector part and a tail empty or not), and a census of what the cases reach: every kernel and launchable template
instance of the four units, and every grid-, brick- and chunk-stride loop a second time at 256 CUs."""
import math
import re

import numpy as np
import pytest
from scipy import ndimage

import intensity_restatement as IR
import volume_cases as VC

CUS = 256
GEO = VC.geometry(CUS)
ALL = [(f, c) for f in VC.FAMILIES for c in VC.cases(f, CUS)]
SMALL = 100000


def fam(name):
    return VC.cases(name, CUS)


def voxels(c):
    p = c.p
    return int(np.prod(p['shape'])) if 'shape' in p else p['V'] * p.get('NC', len(p.get('records', (0,))))


IDS = lambda c: c.id


def test_geometry_is_read_out_of_the_sources():
    g = GEO
    assert g.cap == 8 * CUS and g.mx_threads == 256 and g.sd_chunk == 2048 and g.sd_rchunk == 4096 and g.lds_maxc == 64
    assert g.brick == (8, 16, 16) and g.cc_threads == 256 and g.brick_cap == 2 ** 20 and (g.rows_mul, g.query_mul) == (4, 4)
    assert (g.ia_threads, g.ia_stat_quads, g.ia_chunk, g.ens_vox, g.ens_max) == (256, 4, 64, 8, 16)
    assert VC.geometry(304).cap == 8 * 304


def test_ids_are_unique_and_do_not_depend_on_the_cu_count():
    ids = [c.id for _, c in ALL]
    assert len(set(ids)) == len(ids)
    assert ids == [c.id for f in VC.FAMILIES for c in VC.cases(f, 304)]


def test_census_every_kernel_and_launchable_instance_has_a_case():
    reached = set()
    for _, c in ALL:
        reached.update(VC.instances(c))
    known = VC.launchable_instances()
    missing = [k for k in known if k not in reached]
    print('VOLUME-CENSUS %d cases reach %d of %d instances' % (len(ALL), len(reached & set(known)), len(known)))
    assert not missing and reached <= set(known), (missing, reached - set(known))


def test_census_fails_on_a_kernel_the_table_does_not_know():
    names = {re.sub(r'<.*', '', k) for k in VC.launchable_instances()} - {'ia_run'}
    in_sources = {k for ks in VC.kernels_in_sources().values() for k in ks}
    assert in_sources == names, (in_sources ^ names)
    assert [len(VC.kernels_in_sources()[u]) for u in VC.UNITS] == [8, 7, 3, 1]
    mx, pp, ia, en = (VC.read(u) for u in VC.UNITS)
    assert set(re.findall(r'hipLaunchKernelGGL\(seg_hist_kernel<(\w+)>', mx)) == {'true', 'false'}
    assert set(re.findall(r'cc_label_launches<(\w+)>\(', pp)) == {'true', 'false'}
    assert set(re.findall(r'hipLaunchKernelGGL\(ensemble_classify_kernel<(\w+)>', en)) == {'true', 'false'}
    assert sorted(set(re.findall(r'ia_run<(MT_INTENSITY_\w+)>\(', ia))) == sorted(VC.OP_NAMES.values())


def test_every_stride_loop_has_a_case_that_makes_a_second_trip():
    trips = {}
    for _, c in ALL:
        for k in VC.second_trips(c, GEO):
            trips.setdefault(k, []).append(c.id)
    for k in VC.STRIDE_LOOPS:
        print('VOLUME-CENSUS second trip of %s: %s' % (k, ', '.join(trips.get(k, []))))
    assert all(k in trips for k in VC.STRIDE_LOOPS), [k for k in VC.STRIDE_LOOPS if k not in trips]
    assert set(trips) <= set(VC.STRIDE_LOOPS)
    assert all(c.p.get('trip2') for _, c in ALL if voxels(c) > SMALL), "only the loop cases are large"


# ---- joint histogram ---------------------------------------------------------------------------------------------------------------
def test_hist_reference_is_a_loop_over_voxels():
    for c in fam('hist'):
        if c.p.get('trip2'):
            continue
        d = VC.build('hist', c, CUS)
        want = np.zeros((d['C'], d['C']), np.int64)
        for a, b in zip(d['t'].tolist(), d['r'].tolist()):
            want[d['remap'][a], d['remap'][b]] += 1
        assert np.array_equal(d['ref'], want.ravel()) and d['ref'].sum() == d['V'] and (d['remap'] < d['C']).all()


def test_hist_cases_hold_their_edges():
    cs = fam('hist')
    for a in (0, 1, 15):
        for b in (0, 1, 15):
            mine = [VC.hist_split(a, b, c.p['V']) for c in cs if (c.p['a'], c.p['b']) == (a, b) and c.p['fill'] == 'mix']
            if a == b:
                for part in range(3):
                    assert {bool(s[part]) for s in mine} >= ({False, True} if part else {a != 0}), (a, b, part, mine)
            else:
                assert all(s[0] == 0 and s[1] == 0 and s[2] for s in mine) and len(mine) >= 4
    assert VC.hist_split(1, 11, 5) == (5, 0, 0) and any((c.p['a'], c.p['b'], c.p['V']) == (1, 11, 5) for c in cs)
    assert {c.p['V'] for c in cs} >= {1, 15, 16, 17, 31} and {c.p['C'] for c in cs} >= {1, 2, 64, 65, 256}
    assert {c.p['at'] for c in cs if c.p['fill'] == 'one'} == set(range(16, 32))
    for c in cs:
        d = VC.build('hist', c, CUS) if not c.p.get('trip2') else None
        if c.p['fill'] == 'zero':
            assert not d['t'].any() and not d['r'].any() and d['ref'][int(d['remap'][0]) * (d['C'] + 1)] == d['V']
        if c.p['fill'] == 'one':
            assert int((d['t'] != 0).sum() + (d['r'] != 0).sum()) == 1
        if c.p['remap'] == 'zero-moved':
            assert d['remap'][0] != 0
        if c.p['remap'] == 'many' and d is not None:
            assert len(set(d['remap'].tolist())) < 256 and d['remap'][0] == 3 % d['C']
    t = [c for c in cs if c.p.get('trip2')][0]
    assert t.p['V'] == 16 * 256 * GEO.cap + 16 + 3
    d = VC.build('hist', t, CUS)
    assert d['t'][VC.hist_trip(GEO):].any() and d['r'][VC.hist_trip(GEO):].any() and d['ref'].sum() == d['V']


# ---- surface distances -------------------------------------------------------------------------------------------------------------
SD_SMALL = [c for c in fam('sd') if c.p['kind'] != 'loop']


@pytest.mark.parametrize('case', SD_SMALL, ids=IDS)
def test_sd_reference_is_the_distance_transform(case):
    """medpy's __surface_distances: distance_transform_edt(~border(other), sampling)[border(this)], to 1e-12 relative"""
    d = VC.build('sd', case, CUS)
    ba, bb = d['ba'], d['bb']
    assert (d['nA'], d['nB']) == (int(ba.sum()), int(bb.sum()))
    for this, other, got in ((ba, bb, d['out'][:d['nA']]), (bb, ba, d['out'][d['nA']:])):
        if not this.any():
            assert got.size == 0
        elif not other.any():
            assert np.isinf(got).all()
        else:
            want = ndimage.distance_transform_edt(~other, sampling=d['sp'])[this]
            assert got.shape == want.shape and np.allclose(got, want, rtol=1e-12, atol=0)
    # the border by its definition: a mask voxel with a structure neighbour outside the mask or outside the volume
    m = d['member'][d['t']] != 0
    st = ndimage.generate_binary_structure(3, d['conn'])
    pad = np.pad(m, 1)
    inner = np.ones_like(m)
    for dz, dy, dx in np.argwhere(st) - 1:
        inner &= pad[1 + dz:1 + dz + m.shape[0], 1 + dy:1 + dy + m.shape[1], 1 + dx:1 + dx + m.shape[2]]
    assert np.array_equal(ba, m & ~inner)


def test_sd_reference_gives_the_medpy_metrics():
    """hd, hd95, asd and assd of tests/evaluation_cases.py from the two direction lists of the reference"""
    import evaluation_cases as EC
    for cid in ('sd-conn1', 'sd-conn2', 'sd-conn3-ragged'):
        d = VC.build('sd', [c for c in SD_SMALL if c.id == cid][0], CUS)
        a, b = d['out'][:d['nA']], d['out'][d['nA']:]
        t, r = d['member'][d['t']] != 0, d['member'][d['r']] != 0
        args = (t, r, d['sp'], d['conn'])
        assert math.isclose(max(a.max(), b.max()), EC.hd(*args), rel_tol=1e-12)
        assert math.isclose(float(np.percentile(np.hstack((a, b)), 95)), EC.hd95(*args), rel_tol=1e-12)
        assert math.isclose(float(a.mean()), EC.asd(*args), rel_tol=1e-12)
        assert math.isclose(float(np.mean((a.mean(), b.mean()))), EC.assd(*args), rel_tol=1e-12)


def test_sd_cases_hold_their_edges():
    by = {c.id: c for c in fam('sd')}
    built = {i: VC.build('sd', by[i], CUS) for i in by if by[i].p['kind'] != 'loop'}
    assert {c.p['conn'] for c in by.values()} == {1, 2, 3}
    assert all(VC.is_dyadic(sp) for sp in VC.DYADIC) and not VC.is_dyadic(VC.RAGGED)
    for n in (4095, 4096, 4097, 8193):
        d = built['sd-n%d' % n]
        assert d['nA'] + d['nB'] == n == d['capacity']
    d = built['sd-left-right-tie']
    assert d['out'][0] == 2 * d['sp'][2] and d['nA'] == 1 and d['nB'] == 2
    for W in (63, 64, 65, 129):
        d = built['sd-far-words-W%d' % W]
        assert d['nA'] == d['nB'] == 2 and (d['out'] == (W - 1) * d['sp'][2]).all()
        assert (d['bb'][0, 0, :W - 1] == 0).all() and d['bb'][0, 0, W - 1] and d['ba'][0, 0, 0]           # the only set bit sits in the last word
    assert W // 64 == 2
    assert np.isinf(built['sd-ref-empty']['out']).all() and built['sd-ref-empty']['nB'] == 0 and built['sd-ref-empty']['nA'] > 0
    assert np.isinf(built['sd-test-empty']['out']).all() and built['sd-test-empty']['nA'] == 0
    assert built['sd-both-empty']['out'].size == 0
    d = built['sd-joint-member']
    assert d['member'].sum() == 2 and {2, 3, 9} <= set(np.unique(d['t']).tolist())
    caps = [built['sd-capacity-%s' % n] for n in ('1', 'nA-1', 'nA', 'nA+1', 'n-1', 'n')]
    nA, nB = caps[0]['nA'], caps[0]['nB']
    assert all((d['nA'], d['nB']) == (nA, nB) and np.array_equal(d['t'], caps[0]['t']) for d in caps) and nA > 2 and nB > 2
    assert [d['capacity'] for d in caps] == [1, nA - 1, nA, nA + 1, nA + nB - 1, nA + nB]
    assert all(d['capacity'] < nA + nB for d in caps[:-1])                                     # they really truncate
    d = built['sd-capacity-4097-of-8193']
    assert d['capacity'] == 4097 == GEO.sd_rchunk + 1 and d['nA'] + d['nB'] == 8193 and d['nA'] >= 4097
    s = VC.sd_stats_ref(d['out'][:4097], d['nA'], d['nB'], 4097)
    assert s[0][0] == d['nA'] and s[1] == (d['nB'], 0.0, 0.0)
    ragged = [built[i] for i in built if not built[i]['dyadic']]
    assert len(ragged) == 3 and all(d['sp'] == VC.RAGGED for d in ragged)


def test_sd_loop_closed_form_at_one_cu():
    """every voxel of the two planes is a border voxel at distance sx: against the brute-force reference where the case is small"""
    for c in VC.cases('sd', 1):
        if c.p['kind'] != 'loop':
            continue
        d = VC.build('sd', c, 1)
        t, q = d['t'], d['r']
        ba, bb = VC.sd_borders(t != 0, 1), VC.sd_borders(q != 0, 1)
        assert ba.sum() == d['nA'] == t.sum() and bb.sum() == d['nB']
        if d['nA'] <= 5000:
            assert (VC.sd_brute(ba, bb, d['sp']) == d['value']).all() and (VC.sd_brute(bb, ba, d['sp']) == d['value']).all()
    sizes = {c.p['trip2']: c.p['shape'] for c in fam('sd') if c.p['kind'] == 'loop'}
    assert all(max(s) <= 32766 and s[2] == 2 for s in sizes.values())
    assert sizes['rows'][0] * sizes['rows'][1] < sizes['query'][0] * sizes['query'][1] < sizes['reduce'][0] * sizes['reduce'][1]


# ---- connected components ----------------------------------------------------------------------------------------------------------
def flood_labels(mask):
    """6-connected flood fill in linear order: the component's smallest index is where it starts"""
    D, H, W = mask.shape
    lab = np.full(mask.shape, -1, np.int32)
    sizes = np.zeros(mask.size, np.int32)
    for start in np.flatnonzero(mask.ravel() & (lab.ravel() < 0)):
        s = np.unravel_index(start, mask.shape)
        if lab[s] >= 0:
            continue
        lab[s] = start
        stack, n = [s], 0
        while stack:
            z, y, x = stack.pop()
            n += 1
            for dz, dy, dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                v = (z + dz, y + dy, x + dx)
                if 0 <= v[0] < D and 0 <= v[1] < H and 0 <= v[2] < W and mask[v] and lab[v] < 0:
                    lab[v] = start
                    stack.append(v)
        sizes[start] = n
    return lab.ravel(), sizes


CC_SMALL = [c for c in fam('cc') if not c.p.get('trip2')]


@pytest.mark.parametrize('case', CC_SMALL, ids=IDS)
def test_cc_reference_is_a_flood_fill(case):
    d = VC.build('cc', case, CUS)
    mask = d['member'][d['seg']] != 0
    lab, sizes = flood_labels(mask)
    assert np.array_equal(lab, d['labels']) and np.array_equal(sizes, d['sizes'])
    assert d['stats'] == (int((sizes > 0).sum()), int(sizes.max()))
    assert np.array_equal(np.bincount(lab[lab >= 0], minlength=lab.size)[:lab.size] * (sizes > 0), sizes)
    if 'remove' in case.p:
        vpv, use_min, ms = d['remove']
        after = d['seg'].ravel().copy()
        for root in np.flatnonzero(sizes):
            size, largest = sizes[root] * vpv, d['stats'][1] * vpv            # np.int32 * float: the reference's own product
            if size != largest and (not use_min or size < ms):
                after[lab == root] = 0
        assert np.array_equal(after.reshape(d['seg'].shape), d['seg_after'])


def test_cc_cases_hold_their_edges():
    by = {c.id: VC.build('cc', c, CUS) for c in CC_SMALL}
    assert by['cc-faces']['stats'] == (3, 4) and by['cc-corner']['stats'] == (1, 4) and by['cc-diagonal']['stats'] == (6, 1)
    assert by['cc-full']['stats'] == (1, 16 * 32 * 32) and by['cc-empty']['stats'] == (0, 0)
    n, largest = by['cc-serpentine']['stats']
    assert n == 1 and largest == int(by['cc-serpentine']['seg'].sum()) > 500
    assert by['cc-comb']['stats'][0] == 5 + 8                                   # five joined shapes and eight loose teeth
    for axis, b in enumerate(GEO.brick):
        assert {c.p['shape'][axis] for c in CC_SMALL if c.id.startswith('cc-axis%d' % axis)} == {1, b - 1, b, b + 1, 2 * b + 1}
    assert by['cc-member-0']['stats'][0] > 0 and by['cc-member-1-2']['stats'] != by['cc-member-255']['stats']
    d = by['rm-three-tied']
    assert sorted(d['sizes'][d['sizes'] > 0].tolist()) == [1, 2, 3, 5, 5, 5] and d['removed'] == 3 and d['seg_after'].sum() == 15
    at, above, below = (by['rm-min-size-%s-3x0.3' % k] for k in ('at', 'above', 'below'))
    assert at['remove'][2] == 3 * 0.3 != 0.9 and below['remove'][2] < at['remove'][2] < above['remove'][2]
    assert (at['removed'], above['removed'], below['removed']) == (2, 3, 2)       # a size equal to the minimum is kept
    assert at['seg_after'].sum() == 5 + 5 + 4 + 3 + 3 and above['seg_after'].sum() == 5 + 5 + 4
    d = by['rm-large-min-size']
    assert d['removed'] == 4 and d['seg_after'].sum() == 6                       # several removed: the largest of them is reported
    assert by['rm-all-kept']['removed'] == 0 and np.array_equal(by['rm-all-kept']['seg_after'], by['rm-all-kept']['seg'])
    assert by['rm-one-component']['removed'] == 0 and by['rm-empty']['removed'] == 0 and by['rm-empty']['stats'] == (0, 0)


def test_cc_column_closed_form():
    mask, labels, sizes, stats = VC.column_runs(1000)
    ref = VC.cc_ref(mask.reshape(1000, 1, 1))
    assert np.array_equal(labels, ref[0]) and np.array_equal(sizes, ref[1]) and stats == ref[2]
    assert VC.column_runs(1006)[2][1001] == 5 and VC.cc_ref(VC.column_runs(1006)[0].reshape(1, 1, 1006))[1][1001] == 5
    for c in fam('cc'):
        if c.p['kind'] == 'column':
            D, H, W = c.p['shape']
            assert D * H * W in (8 * 2 ** 20 + 9, 16 * 2 ** 20 + 17)


# ---- fill holes ----------------------------------------------------------------------------------------------------------------------
def test_fh_reference_is_the_background_reached_from_the_faces():
    seen = 0
    for c in fam('fh'):
        if voxels(c) > SMALL:
            continue
        d = VC.build('fh', c, CUS)
        bg = d['mask'] == 0
        lab, sizes = VC.cc_ref(bg)[:2]
        lab = lab.reshape(bg.shape)
        face = np.zeros(bg.shape, bool)
        face[0], face[-1], face[:, 0], face[:, -1], face[:, :, 0], face[:, :, -1] = True, True, True, True, True, True
        outside = np.isin(lab, np.unique(lab[face & bg]))
        assert np.array_equal(d['ref'], (~(bg & outside)).astype(np.uint8)), c.id
        assert d['count'] == int(d['ref'].sum())
        if d['count']:
            z = np.argwhere(d['ref'])
            assert d['bbox'] == [v for a in range(3) for v in (int(z[:, a].min()), int(z[:, a].max()) + 1)]
        seen += 1
    assert seen >= 24


def test_fh_cases_hold_their_edges():
    by = {c.id: (c, VC.build('fh', c, CUS)) for c in fam('fh') if voxels(c) <= SMALL}
    filled = lambda i: int(by[i][1]['ref'].sum()) - int((by[i][1]['mask'] != 0).sum())
    assert filled('fh-one-brick') == 2 * 5 * 6 and filled('fh-eight-bricks') == 125 and filled('fh-tunnel') == 0 and filled('fh-diagonal-leak') > 0
    assert filled('fh-two-cavities') == 27 + 4 * 4 * 2 and by['fh-zeros'][1]['count'] == 0 and filled('fh-ones') == 0
    assert by['fh-box-on-the-faces'][1]['ref'].all() and filled('fh-box-on-the-faces') > 0
    assert all(filled('fh-axis%d-of-1' % a) == 0 and 1 in by['fh-axis%d-of-1' % a][0].p['shape'] for a in range(3))
    assert set(np.unique(by['fh-values-0-7-200'][1]['mask']).tolist()) == {0, 7, 200} and set(np.unique(by['fh-values-0-255'][1]['mask']).tolist()) == {0, 255}
    align = [(c.p['off'], int(np.prod(c.p['shape'])) % 16) for c, _ in by.values() if c.id.startswith('fh-off')]
    assert sorted(align) == [(o, m) for o in (0, 1, 8) for m in (0, 1, 15)]
    assert sum(filled(c.id) > 0 for c, _ in by.values() if c.id.startswith('fh-off')) >= 3
    c, d = by['fh-alternating-chunk']
    row = slice(64, 80)                                                          # one 16-voxel chunk of the fill kernel
    assert d['mask'].ravel()[row].tolist() == [0, 1] * 7 + [0, 0] and d['ref'].ravel()[row].tolist() == [0] + [1] * 13 + [0, 0]
    for c in fam('fh'):
        if c.p['kind'] == 'late-face':                    # the tunnel's only face voxel is numbered beyond the first trip of fh_mark_kernel
            D, H, W = c.p['shape']
            nD, nH, nW = H * W, D * W, D * H
            assert 2 * (nD + nH + nW) > 256 * GEO.cap and 2 * nD + 2 * nH + nW + (1 * H + H // 2) >= 256 * GEO.cap and D * H * W < 10 ** 6


def test_fh_closed_forms_at_one_cu():
    n = 0
    for c in VC.cases('fh', 1):
        if c.p['kind'] in ('shell', 'late-face') and voxels(c) <= SMALL:
            VC.build('fh', c, 1)                        # asserts closed form == scipy
            n += 1
    assert n == 2
    small = VC.Case('fh-column-small', 'mt_fill_holes3d', dict(kind='column', shape=(1000, 1, 1), off=0, vals=(7,)))
    d = VC.build('fh', small, 1)
    assert np.array_equal(d['ref'], (d['mask'] != 0).astype(np.uint8)) and d['count'] == int((np.arange(1000) % 11 < 7).sum())


# ---- channel statistics ------------------------------------------------------------------------------------------------------------
def test_stats_reference_against_numpy():
    worst_m = worst_s = 0.0
    for c in fam('stats'):
        if c.p.get('trip2'):
            continue
        d = VC.build('stats', c, CUS)
        for ch in range(d['NC']):
            r = d['refs'][ch]
            assert (r is None) == (not d['active'][ch])
            if r is None:
                continue
            x = d['x'][ch]
            with np.errstate(invalid='ignore'):
                lo, hi, mean, sd = float(x.min()), float(x.max()), float(x.astype(np.float64).mean()), float(x.astype(np.float64).std())
            same = lambda a, b: a == b or (math.isnan(a) and math.isnan(b))
            assert same(r[0], lo) and same(r[1], hi)
            if np.isfinite(x).all():
                worst_m, worst_s = max(worst_m, abs(mean - r[2]) / max(r[4], 1e-300)), max(worst_s, abs(sd - r[3]) / r[3] if r[3] else abs(sd))
            else:
                assert not math.isfinite(r[2]) and not math.isfinite(r[3])
                if np.isnan(x).any():
                    assert all(math.isnan(v) for v in r[:4])
    print('VOLUME-FIG numpy stats worst mean err / max|x| %.3e, worst sd err / sd %.3e' % (worst_m, worst_s))
    assert worst_m <= VC.MEAN_BOUND / 100 and worst_s <= VC.SD_BOUND / 100


def test_stats_cases_hold_their_edges():
    cs = fam('stats')
    assert {c.p['V'] for c in cs} >= {1, 2, 3, 4, 5, 7, 1023, 1024, 1025} and {c.p['NC'] for c in cs} >= {1, 64, 65, 130}
    assert {c.p['active'] for c in cs} >= {(0,), (63,), (64,), (129,), (0, 63, 64, 129), ()}
    assert any(c.p['NC'] > 1 and c.p['V'] % 2 for c in cs)
    d = VC.build('stats', [c for c in cs if c.id == 'stats-special'][0], CUS)
    k = {n: i for i, n in enumerate(VC.SPECIAL)}
    assert d['refs'][k['constant']][3] == 0.0 and abs(d['refs'][k['mean1e4-sd1e-2']][3] - 1e-2) < 2e-3
    assert 0 < np.abs(d['x'][k['denormals']]).max() < 1.2e-38 and d['refs'][k['denormals']][3] > 0
    assert np.isnan(d['x'][k['nan-first'], 0]) and not np.isnan(d['x'][k['nan-later'], 0]) and np.isnan(d['x'][k['nan-later']]).sum() == 1
    assert d['refs'][k['pinf']][1] == math.inf and math.isfinite(d['refs'][k['pinf']][0]) and d['refs'][k['pinf']][2] == math.inf
    assert d['refs'][k['bothinf']][:2] == (-math.inf, math.inf) and math.isnan(d['refs'][k['bothinf']][2])
    t = [c for c in cs if c.p.get('trip2')][0]
    assert t.p['V'] == 4096 * GEO.cap + 5


# ---- intensity apply -----------------------------------------------------------------------------------------------------------------
def test_apply_reference_is_the_restatement():
    """apply_ref with numpy's own float32 statistics equals tests/intensity_restatement.py bit for bit, in float32 and float64"""
    r = VC.rng('apply-vs-restatement')
    x = (r.standard_normal(1025) * 2 + 1).astype(np.float32)
    for dt in (np.float32, np.float64):
        st = VC.np_stats(x, dt)
        same = lambda a, b: a.dtype == b.dtype and np.array_equal(VC.bits(a), VC.bits(b))
        assert same(VC.apply_ref(x, VC.OP_SCALE, 0, 1.25, 0, None, None, dt), IR.brightness_one(x, 1.25, dt))
        for flags in (0, VC.PRESERVE):
            assert same(VC.apply_ref(x, VC.OP_CONTRAST, flags, 1.25, 0, st, None, dt), IR.contrast_one(x, 1.25, bool(flags), dt))
        for flags in (0, VC.NEGATE):
            for g in (0.7, 1.5):
                y = VC.apply_ref(x, VC.OP_GAMMA, flags, g, 1e-7, st, None, dt)
                assert same(y, IR.gamma_one(x, g, bool(flags), False, 1e-7, dt))
                yd = (-y if flags else y)                                     # the domain the restatement works in
                centred = yd - yd.mean()
                st2 = np.array([0, 0, -yd.mean() if flags else yd.mean(), centred.std()], np.float64)
                z = VC.apply_ref(y, VC.OP_RESTORE, flags, 0, 0, st, st2, dt)
                assert same(z, IR.gamma_one(x, g, bool(flags), True, 1e-7, dt)), (dt, flags, g)


def test_apply_cases_hold_their_edges():
    cs = {c.id: c for c in fam('apply')}
    combos = {(r[0], r[1]) for r in VC.ALL_OPS}
    assert combos == {(VC.OP_NONE, 0), (VC.OP_SCALE, 0), (VC.OP_CONTRAST, 0), (VC.OP_CONTRAST, VC.PRESERVE), (VC.OP_GAMMA, 0), (VC.OP_GAMMA, VC.NEGATE),
                      (VC.OP_RESTORE, 0), (VC.OP_RESTORE, VC.NEGATE)}
    assert {(c.p['V'], c.p['stats']) for c in cs.values() if c.p['records'] is VC.ALL_OPS} == {(V, m) for V in (1, 3, 4, 5, 1025) for m in ('device', 'hand')}
    rec = cs['apply-slots-0-63-64-129'].p['records']
    assert len(rec) == 130 and [i for i, r in enumerate(rec) if r[0] != VC.OP_NONE] == [0, 63, 64, 129] and len({rec[i][0] for i in (0, 63, 64, 129)}) == 4
    assert {r[2] for r in cs['apply-gamma-exponents'].p['records']} == {0.0, 1.0, 0.7, 1.5}
    d = VC.build('apply', cs['apply-preserve-range-clamps'], CUS)
    exp = VC.apply_expected(d, d['stats'], d['stats2'])
    lo, hi = np.float32(d['stats'][0][0]), np.float32(d['stats'][0][1])
    assert (exp[0][0] == lo).any() and (exp[0][0] == hi).any() and exp[1][0].min() < d['x'][1].min() and exp[1][0].max() > d['x'][1].max()
    d = VC.build('apply', cs['apply-constant-channel'], CUS)
    st, st2 = np.stack([VC.np_stats(v) for v in d['x']]), np.stack([VC.np_stats(v) for v in d['x2']])
    assert (st[:, 3] == 0).all() and (st[:, 0] == st[:, 1]).all()
    assert all(np.isfinite(r32).all() for r32, _ in VC.apply_expected(d, st, st2))
    assert cs['apply-V1024cap+3'].p['V'] == 1024 * GEO.cap + 3 and cs['apply-trip2'].p['V'] // 4 == 256 * GEO.cap + 1
    assert {r[0] for r in cs['apply-trip2'].p['records']} == {1, 2, 3, 4}


# ---- ensemble ------------------------------------------------------------------------------------------------------------------------
def test_ens_cases_hold_their_edges():
    cs = {c.id: c for c in fam('ens')}
    t = cs['ens-trip2'].p
    assert int(np.prod(t['shape'])) > 8 * 256 * GEO.cap and (t['K'], t['C']) == (2, 2) and int(np.prod(t['shape'])) % 8 == 0
    assert (cs['ens-K16-C255-V9'].p['K'], cs['ens-K16-C255-V9'].p['C']) == (16, 255)
    d = VC.build('ens', cs['ens-K16-C255-V9'], CUS)
    assert d['V'] == 9 and d['lab'].max() > 127
    for wide in ('wide', 'narrow'):
        for off in (0, 4, 1):
            d = VC.build('ens', cs['ens-order-255-256-%s-out%d' % (wide, off)], CUS)
            assert {0, 255, 3} >= set(np.unique(d['lab']).tolist()) >= {255, 3} and (d['mean'][1] > 0.5).any()
            want = np.zeros(d['V'], np.int64)
            for i, o in enumerate((255, 256, 515)):
                want[d['mean'][i].astype(np.float32) > 0.5] = o
            assert np.array_equal(d['lab'].ravel(), (want % 256).astype(np.uint8)) and (want == 256).any()
            assert (d['lab'].ravel()[:16] == 255).all()                           # label 255 in every byte of two packed stores
            if off == 4:
                continue
            d = VC.build('ens', cs['ens-nan-%s-out%d' % (wide, off)], CUS)
            mean, lab = d['mean'].astype(np.float32), d['lab'].ravel()
            nan = np.isnan(mean)
            assert nan[0].any() and (nan[1] & ~nan[0]).any() and (nan[2] & ~nan[0] & ~nan[1]).any() and (nan[1] & nan[2] & ~nan[0]).any()
            first = np.where(nan.any(0), nan.argmax(0), np.nan_to_num(mean, nan=-1).argmax(0))                # the first NaN, else the first maximum
            assert np.array_equal(lab, first.astype(np.uint8))
    d = VC.build('ens', cs['ens-nan-regions'], CUS)
    assert (d['lab'].ravel()[np.isnan(d['mean'].astype(np.float32)).all(0)] == 0).all()
