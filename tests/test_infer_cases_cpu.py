"""The case table of the prediction path (tests/infer_cases.py) without a GPU: every float64 reference against an independent statement
of the same operation, every head case's kernel instance by name (all eight are named), the axes the table promises per instance, the
sizes that reach the grid-stride loops / the large-LDS branch / the column loop, and the exclusion cap of the resampling cases for the
reference alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import infer_cases as IC
import mask_check


def test_unflip_is_torch_flip():
    t = torch.randn((2, 3, 4, 5, 6), generator=IC.gen('unflip')).double()
    for code in range(8):
        dims = [2 + i for i in range(3) if code & (1 << i)]
        assert torch.equal(IC.unflip(t, code), torch.flip(t, dims) if dims else t), code
        assert IC.bits(code) == tuple(2 + i in dims for i in range(3))


def _scipy_resample(p, oshape, sep):
    """resample_data_or_seg(is_seg=False, order 1, order_z 0) per channel with scipy alone (preprocessing.py:109-197): in-plane zoom of
    every slice, then map_coordinates order 0 along the separate axis at the coordinates of the same rule"""
    from scipy.ndimage import map_coordinates, zoom
    I = p.shape
    if sep < 0:
        return zoom(p, [o / i for o, i in zip(oshape, I)], order=1, mode='nearest', grid_mode=True)
    zf = [1.0 if ax == sep else oshape[ax] / I[ax] for ax in range(3)]
    q = zoom(p, zf, order=1, mode='nearest', grid_mode=True)
    assert q.shape == tuple(I[ax] if ax == sep else oshape[ax] for ax in range(3))
    grid = [np.arange(oshape[ax], dtype=np.float64) for ax in range(3)]
    grid[sep] = (grid[sep] + 0.5) * (I[sep] / oshape[sep]) - 0.5
    co = np.meshgrid(*grid, indexing='ij')
    return map_coordinates(q, co, order=0, mode='nearest')


@pytest.mark.parametrize('case', IC.resample_cases(), ids=lambda c: c.id)
def test_resample_reference_is_scipy_and_leaves_out_less_than_the_cap(case):
    p = IC.rs_probs(case).numpy()
    vals = IC.resample_values(p, case.oshape, case.sep)
    assert vals.shape == (case.C,) + case.oshape and vals.dtype == np.float64
    for ch in range(min(case.C, 6)):
        want = _scipy_resample(p[ch].astype(np.float64), case.oshape, case.sep)
        assert want.shape == case.oshape
        assert np.abs(vals[ch] - want).max() < 1e-12, (ch, float(np.abs(vals[ch] - want).max()))
    out = IC.resample_excluded(vals, case.order)
    print('%s: %.4f %% of the voxels within %g of a decision' % (case.id, 100.0 * out.mean(), IC.RS_MARGIN))
    assert out.mean() < IC.RS_MAX_OUT
    # the device form of the restatement (used for the large case) is the same arithmetic
    tv = IC.resample_values(torch.from_numpy(p), case.oshape, case.sep, xp=torch).numpy()
    assert np.array_equal(tv, vals)
    sl, box = IC.resample_box(case)
    assert all(s.stop <= f for s, f in zip(sl, case.full)) and all(b.stop >= 1 for b in box)


def test_resample_cases_reach_what_they_claim():
    cs = IC.resample_cases()
    want = [((5, 7, 9), (9, 16, 11), -1), ((4, 9, 13), (9, 5, 29), 0), ((9, 14, 16), (4, 5, 7), 1), ((4, 9, 13), (9, 20, 29), 2)]
    assert all(any((c.ishape, c.oshape, c.sep) == w for c in cs) for w in want)
    assert any(c.ishape == c.oshape for c in cs) and any(1 in c.ishape for c in cs)
    assert {c.C for c in cs} == {3, 5, 47} and any(c.order is None for c in cs) and any(c.order is not None for c in cs)
    for ax in range(3):                                         # the box clips in each dimension
        assert any(c.off[ax] + c.oshape[ax] > c.full[ax] for c in cs)
    assert any(all(c.off[ax] + c.oshape[ax] < c.full[ax] or c.off[ax] > 0 for ax in range(3)) for c in cs)
    L = IC.RS_LARGE
    _, box = IC.resample_box(L)
    assert L.C == 1 and int(np.prod([b.stop for b in box])) > 65536 * 256


def test_decision_rules_are_mask_check_decide():
    o5 = [3, 1, 4, 2, 5]
    for case in IC.norm_cases()[:-1]:
        d = IC.norm_draw(case)
        den = d['nb'] if d['nb'] is not None else torch.ones(case.V)
        probs = (d['agg'] / den).numpy()
        assert (probs == 0.5).any(), case.id
        if case.C > 1:
            srt = np.sort(probs, 0)
            assert (srt[-1] == srt[-2]).any(), case.id                      # exact ties are planted
        want = mask_check.decide(probs, case.order)
        assert np.array_equal(IC.decide_ref(probs, case.order), want.astype(np.int64)), case.id
    p = torch.rand((5, 4, 6, 7), generator=IC.gen('decide')).numpy()
    p[2, 1] = 0.5
    p[4, 2] = p[1, 2] = 0.99
    for order in (o5, None):
        assert np.array_equal(IC.decide_ref(p, order), mask_check.decide(p, order).astype(np.int64))
    # regions take the last channel above 0.5, argmax the first maximum
    one = np.array([0.9, 0.2, 0.9, 0.5, 0.3], np.float32).reshape(5, 1)
    assert IC.decide_ref(one, o5)[0] == 4 and IC.decide_ref(one, None)[0] == 0


def _name(lib, p, mirror):
    buf = C.create_string_buffer(128)
    rc = lib.mt_head_infer_kernel_name(C.byref(p), mirror, buf, 128)
    return rc, buf.value.decode()


def test_head_cases_name_all_eight_instances():
    from multitalent_amd import _lib
    lib = _lib.load()
    seen = set()
    for c in IC.head_cases():
        p = IC.head_problem(c)
        for mirror in (0, 1):
            rc, name = _name(lib, p, mirror)
            assert rc == 0 and name == IC.head_name(c, mirror), (c.id, rc, name)
            seen.add(name)
        vec, xs = IC.INST_ARGS[c.inst]
        if c.inst == 'd1':
            assert c.cs % 2 == 1 or p.src.ptr % 8 == 4
        elif c.inst == 'p2':
            assert c.cs % 2 == 0 and p.src.ptr % 8 == 0
        else:
            assert c.cs % 2 == 0 and p.src.ptr % 4 == 0
    assert seen == {'head_%s_accumulate_kernel<%d, %d>' % (k, v, x) for k in ('flip', 'mirror') for v, x in IC.INST_ARGS.values()}
    assert len(seen) == 8


def test_head_name_query_refuses_what_the_launches_refuse():
    from multitalent_amd import _lib
    lib = _lib.load()
    c = [c for c in IC.head_cases() if c.inst == 'f16'][0]
    p = IC.head_problem(c)
    assert _name(lib, p, 0)[0] == 0
    p.src.cs = c.cs + 1                                         # a 16-bit source at an odd channel stride
    assert _name(lib, p, 0)[0] == -1 and _name(lib, p, 1)[0] == -1
    p = IC.head_problem(c)
    p.src.ptr += 2
    assert _name(lib, p, 1)[0] == -1
    p = IC.head_problem(c)
    p.Cout = 65
    assert _name(lib, p, 0)[0] == -1
    p = IC.head_problem(c)
    p.soW = 2
    assert _name(lib, p, 0)[0] == -1
    p = IC.head_problem(c)
    p.src.dtype = 3
    assert _name(lib, p, 1)[0] == -1
    assert lib.mt_head_infer_kernel_name(C.byref(IC.head_problem(c)), 0, None, 0) == -1


def test_head_table_has_every_value_of_every_axis_for_every_instance():
    cases = IC.head_cases()
    assert len({c.id for c in cases}) == len(cases)
    for inst in IC.INSTANCES:
        cs = [c for c in cases if c.inst == inst]
        assert {(c.cin, c.cout) for c in cs} == set(IC.CC)
        assert {int(np.prod(c.shape)) for c in cs} == {105, 128, 129, 1155}
        assert {c.ns for c in cs} == {1, 2, 4, 8} and {c.sample0 for c in cs} == {0, 1}
        assert {f for c in cs for f in c.flips} == set(range(8))
        assert {f for c in cs for f in c.fflips} == set(range(8))
        assert {(c.aff, c.slope) for c in cs if c.aff} == {(True, 0.01), (True, 1.5)} and any(not c.aff for c in cs)
        assert {c.bias for c in cs} == {True, False}
        assert {(c.nonlin, c.spread) for c in cs} >= {(0, 0.0), (1, 0.0), (2, 0.0), (1, IC.SPREAD), (2, IC.SPREAD), (2, IC.SPREAD_WIDE)}
        assert {w for c in cs for w in c.fweights} == set(IC.WEIGHTS)
        assert {c.gauss for c in cs} == {True, False} and {c.nb for c in cs} == {True, False}
        assert {c.origin for c in cs} == set(IC.ORIGINS)
        if inst in ('f16', 'bf16'):
            assert any(c.cin == 30 and c.cs == 30 and c.c0 == 0 for c in cs)
            assert any(c.cin == 30 and c.cs == 34 and (c.c0 * 2) % 16 == 4 for c in cs)
    for c in cases:
        adims, o = IC.head_agg_geometry(c)
        assert all(o[i] + c.shape[i] <= adims[i] for i in range(3))
        if c.origin == 'corner':
            assert all(o[i] + c.shape[i] == adims[i] and o[i] > 0 for i in range(3))
        assert max(c.fsamples) < IC.head_N(c) and c.sample0 + c.ns <= IC.head_N(c)


def test_head_references_agree_with_a_plain_loop():
    """the float64 head reference against a per-voxel matrix product, and the spread case's range"""
    for c in [c for c in IC.head_cases() if c.inst == 'd1' and int(np.prod(c.shape)) <= 129][:3] + [c for c in IC.head_cases() if c.spread][:2]:
        d = IC.head_draw(c)
        lg = IC.head_logits(d['x'], d.get('scale'), d.get('shift'), c.slope, d['w'], d['b'])
        a = d['x'].double()
        if c.aff:
            t = a * d['scale'].double()[:, None, None, None, :] + d['shift'].double()[:, None, None, None, :]
            a = torch.maximum(t, torch.zeros_like(t)) + c.slope * torch.minimum(t, torch.zeros_like(t))
        want = a @ d['w'].double().reshape(c.cout, c.cin).t()
        if c.bias:
            want = want + d['b'].double()
        assert torch.allclose(lg, want.permute(0, 4, 1, 2, 3), rtol=1e-12, atol=1e-12)
        if c.spread:
            assert abs(float(lg.max()) - c.spread) < 1.0 and float(lg.min()) >= -c.spread - 1.0 and c.spread in (80.0, 100.0)
        buf = IC.head_buffer(c, d)
        assert torch.equal(buf[..., c.c0:c.c0 + c.cin], d['x']) and not torch.isnan(buf.float()).any()


def test_flip_accumulate_table():
    cs = IC.flipacc_cases()
    assert {c.C for c in cs} == set(IC.FA_C)
    assert {(c.shape[2], c.code >> 2) for c in cs} >= {(w, f) for w in IC.FA_W for f in (0, 1)}
    assert {c.code for c in cs} == set(range(8)) and {c.nonlin for c in cs} == {0, 1, 2}
    assert {c.nonlin for c in cs if c.spread == IC.SPREAD} == {1, 2} and any(c.nonlin == 2 and c.spread == IC.SPREAD_WIDE for c in cs)
    assert any(IC.flipacc_exact(c) for c in cs) and all(c.cs > c.C and c.c0 % 2 == 1 for c in cs)
    lds = lambda C_: 256 * (C_ | 1) * 4
    assert lds(47) <= 64 * 1024 < lds(64) and lds(159) <= 160 * 1024 < lds(160)
    assert any(c.C >= 64 and c.shape[2] > 256 and c.code & 4 for c in cs)
    for c in cs[:3]:
        d = IC.flipacc_draw(c)
        one, two = IC.flipacc_ref(c, d)
        dims = [1 + i for i in range(3) if c.code & (1 << i)]
        pred = IC.nonlin_ref(d['logits'].double(), c.nonlin, 3).permute(3, 0, 1, 2)
        assert torch.equal(one, c.weights[0] * (torch.flip(pred, dims) if dims else pred))


def test_large_cases_pass_their_block_caps():
    t = [c for c in IC.tile_cases() if c.C == 1 and int(np.prod(c.patch)) > 8192 * 256]
    assert len(t) == 1 and t[0].patch == (8, 512, 520)
    n = [c for c in IC.norm_cases() if c.V > 16384 * 256]
    assert len(n) == 1 and n[0].C == 1 and n[0].V == 16384 * 256 + 77
    assert {c.C for c in IC.norm_cases()} == {1, 5, 47}
    for c in IC.tile_cases():
        assert all(o + p <= a for o, p, a in zip(c.origin, c.patch, c.adims))
    e = IC.extract_cases()
    assert [len(c[4]) for c in e][:3] == [1, 9, 64] and any(c[3][1] * c[3][2] > 1024 for c in e)
    for _, _, vol, patch, tiles in e:
        assert all(o[i] + patch[i] <= vol[i] for o, _ in tiles for i in range(3))
