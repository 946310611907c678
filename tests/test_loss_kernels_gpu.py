"""Every case of tests/loss_cases.py on the device against its float64 reference: the MultiTalent loss kernels (forward on a NaN-filled
workspace of exactly mt_loss_workspace bytes, twice, bit-identical), the softmax Dice + CE instances, mt_multitalent_hard_stats (exact
counts, twice on the same garbage-filled workspace), mt_loss_combine and the optimizer kernels.  Every output lies between guards that
hold a sentinel: all of the view is overwritten, nothing outside it changes.  The bounds are those of loss_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import loss_cases as LC

pytestmark = pytest.mark.gpu
G, S = LC.GUARD, LC.SENTINEL
RAN = set()                        # kernel names the queries reported for the cases that ran
NRAN = [0]                         # MultiTalent and softmax cases that ran to their end
WORST = {}                         # worst err / bound per quantity (printed, and written where MT_LOSS_RATIOS names a file)


def _lib():
    from multitalent_amd import _lib
    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def _ratio(name, err, bound):
    r = float((err / bound).max()) if torch.is_tensor(err) else float(err / bound)
    WORST[name] = max(WORST.get(name, 0.0), r)
    path = os.environ.get('MT_LOSS_RATIOS')
    if path:
        with open(path, 'a') as f:
            f.write('%s %.4g\n' % (name, r))
    return r


def _view_buffer(dev, B, V, C_, cs, off, values=None):
    """flat fp32 buffer [G + off + B * V * cs + G] of SENTINEL with `values` [B, V, C] in the view's columns; -> (device, host copy)"""
    flat = torch.full((G + off + B * V * cs + G,), S)
    if values is not None:
        flat[G + off:G + off + B * V * cs].view(B, V, cs)[..., :C_] = values
    return flat.to(dev), flat


def _check_view(dbuf, host, B, V, C_, cs, off):
    """-> the view [B, V, C] of the device buffer (on the host); everything outside it is bit-identical to `host`"""
    got = dbuf.cpu()
    inner = got[G + off:G + off + B * V * cs].view(B, V, cs)
    assert torch.equal(got[:G + off], host[:G + off]) and torch.equal(got[G + off + B * V * cs:], host[G + off + B * V * cs:])
    if cs > C_:
        assert bool((inner[..., C_:] == S).all())                      # the neighbour channels of the wider buffer
    return inner[..., :C_]


def _words(vals, dev):
    return torch.tensor([LC.s64(v) for v in vals], dtype=torch.int64, device=dev)


def _guarded(dev, n, fill=S):
    t = torch.full((G + n + G,), S, device=dev)
    t[G:G + n] = fill
    return t


def _guards_intact(t, n):
    return bool((t[:G] == S).all()) and bool((t[G + n:] == S).all())


# ---- MultiTalent ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', LC.mt_cases(), ids=lambda c: c.id)
def test_multitalent_loss_case(dev, c):
    from multitalent_amd import ops
    lib, chk = _lib().load(), _lib().check
    d = LC.mt_draw(c)
    B, V, Cn = len(c.masks), c.V, c.C
    xbuf, _ = _view_buffer(dev, B, V, Cn, c.cs, c.off, d['x'])
    dbuf, dhost = _view_buffer(dev, B, V, Cn, c.dcs, c.off)
    target, valid, lut = d['labels'].to(dev), _words(d['masks'], dev), _words(d['lut'], dev)
    fwd = ops.multitalent_loss_fwd_kernel_name(c.cs, V, Cn)
    bwd = ops.multitalent_loss_bwd_kernel_name(xbuf.data_ptr() + 4 * (G + c.off), c.cs, dbuf.data_ptr() + 4 * (G + c.off), c.dcs, V, Cn)
    assert fwd[0] == c.fwd and bwd[0] == c.bwd, (fwd, bwd)
    RAN.update((fwd[0], bwd[0]))
    ws_bytes = ops.loss_workspace(B, V, Cn)
    assert ws_bytes % 4 == 0 and ws_bytes >= B * fwd[2] * Cn * 16
    runs = []
    for _ in range(2):
        ws = torch.full((ws_bytes // 4 + G,), S, device=dev)
        ws[:ws_bytes // 4] = float('nan')                            # a slot the kernels leave out shows in the sums
        stats = _guarded(dev, B * Cn * 4)
        chk(lib.mt_multitalent_loss_fwd(_p(xbuf, G + c.off), c.cs, _p(target), B, V, Cn, _p(valid), _p(lut), _p(stats, G), _p(ws), ws_bytes,
                                        _stream()), 'multitalent_loss_fwd')
        assert _guards_intact(stats, B * Cn * 4) and bool((ws[ws_bytes // 4:] == S).all())
        runs.append(stats[G:G + B * Cn * 4].cpu().view(B, Cn, 4))
    assert torch.equal(runs[0], runs[1])                             # (NaN != NaN: also says that no slot was left out)
    ref, dref = LC.mt_reference(d['x'], d['labels'], d['masks'], d['lut'], d['gstats'])
    got = runs[0].double()
    act = LC.mt_active(d['masks'], Cn)
    assert bool((got[act == 0] == 0).all())                          # exact zeros for the regions a sample does not carry
    err = (got - ref).abs()
    r1 = _ratio('mt_stats_project', err, LC.MT_STATS_RTOL * ref.abs() + LC.MT_STATS_ATOL)
    r2 = _ratio('mt_stats_chain', err, LC.sum_bound(ref, V, LC.mt_chain(c), LC.MT_TERM_REL, LC.MT_TERM_ABS) + 1e-300)
    print('%s: statistics err / bound %.3f (project) %.3f (chain %d)' % (c.id, r1, r2, LC.mt_chain(c)))
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)
    gst = d['gstats'].to(dev)
    chk(lib.mt_multitalent_loss_bwd(_p(xbuf, G + c.off), c.cs, _p(target), B, V, Cn, _p(valid), _p(lut), _p(gst), _p(dbuf, G + c.off), c.dcs,
                                    _stream()), 'multitalent_loss_bwd')
    dgot = _check_view(dbuf, dhost, B, V, Cn, c.dcs, c.off)
    assert bool((dgot != S).all())                                   # every element of the view is written
    dgot = dgot.double()
    assert bool((dgot[(act == 0)[:, None, :].expand(B, V, Cn)] == 0).all())
    r3 = _ratio('mt_grad_project', (dgot - dref).abs(), LC.MT_GRAD_RTOL * dref.abs() + LC.MT_GRAD_ATOL)
    print('%s: gradient err / bound %.3f' % (c.id, r3))
    assert r3 <= 1.0, r3
    NRAN[0] += 1


# ---- softmax -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', LC.sm_cases(), ids=lambda c: c.id)
def test_softmax_loss_case(dev, c):
    from multitalent_amd import ops
    lib, chk = _lib().load(), _lib().check
    d = LC.sm_draw(c)
    B, V, Cn = 2, c.V, c.C
    assert ops.softmax_dice_ce_kernel_name(Cn, False) == c.fwd and ops.softmax_dice_ce_kernel_name(Cn, True) == c.bwd
    RAN.update((c.fwd, c.bwd))
    xbuf, _ = _view_buffer(dev, B, V, Cn, c.cs, c.off, d['x'])
    dbuf, dhost = _view_buffer(dev, B, V, Cn, c.cs, c.off)
    target = d['labels'].to(dev)
    ws_bytes = ops.loss_workspace(B, V, Cn)
    runs = []
    for _ in range(2):
        ws = torch.full((ws_bytes // 4 + G,), S, device=dev)
        ws[:ws_bytes // 4] = float('nan')
        stats = _guarded(dev, B * Cn * 4)
        chk(lib.mt_softmax_dice_ce_fwd(_p(xbuf, G + c.off), c.cs, _p(target), B, V, Cn, _p(stats, G), _p(ws), ws_bytes, _stream()),
            'softmax_dice_ce_fwd')
        assert _guards_intact(stats, B * Cn * 4) and bool((ws[ws_bytes // 4:] == S).all())
        runs.append(stats[G:G + B * Cn * 4].cpu().view(B, Cn, 4))
    assert torch.equal(runs[0], runs[1])
    assert bool((runs[0][:, 1:, 0] == 0).all())                      # only slot (b, 0, 0) of the CE column: mt_loss_combine reads slot 0
    ref, dref = LC.sm_reference(d['x'], d['labels'], d['gstats'])
    err = (runs[0].double() - ref).abs()
    r1 = _ratio('sm_stats_project', err, LC.SM_STATS_REL * ref.abs() + LC.SM_STATS_ABS)
    r2 = _ratio('sm_stats_chain', err, LC.sum_bound(ref, V, LC.sm_chain(c), Cn + 6, Cn + 8))
    print('%s: statistics err / bound %.3f (project) %.3f (chain)' % (c.id, r1, r2))
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)
    gst = d['gstats'].to(dev)
    chk(lib.mt_softmax_dice_ce_bwd(_p(xbuf, G + c.off), c.cs, _p(target), B, V, Cn, _p(gst), _p(dbuf, G + c.off), c.cs, _stream()),
        'softmax_dice_ce_bwd')
    dgot = _check_view(dbuf, dhost, B, V, Cn, c.cs, c.off)
    assert bool((dgot != S).all())
    r3 = _ratio('sm_grad', float((dgot.double() - dref).abs().max()), LC.SM_GRAD * float(d['gstats'].abs().max()))
    print('%s: gradient err / bound %.3f' % (c.id, r3))
    assert r3 <= 1.0, r3
    NRAN[0] += 1


# ---- hard statistics -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', LC.hs_cases(), ids=lambda c: c.id)
def test_hard_stats_case(dev, c):
    lib, chk = _lib().load(), _lib().check
    d = LC.hs_draw(c)
    B, V, Cn = len(c.masks), c.V, c.C
    xbuf, _ = _view_buffer(dev, B, V, Cn, c.cs, 0, d['x'])
    target, valid, lut = d['labels'].to(dev), _words(d['masks'], dev), _words(d['lut'], dev)
    n = lib.mt_hard_stats_workspace(B, Cn)
    assert n == B * Cn * 3 * 8
    ws = torch.full((n // 8 + G,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=dev)             # garbage: the launcher zeroes its counters
    want = LC.hs_reference(d['x'], d['labels'], d['masks'], d['lut'])
    for _ in range(2):                                               # the second call finds the first call's counts in the workspace
        stats = _guarded(dev, B * Cn * 3)
        chk(lib.mt_multitalent_hard_stats(_p(xbuf, G), c.cs, _p(target), B, V, Cn, _p(valid), _p(lut), _p(stats, G), _p(ws), n, _stream()),
            'multitalent_hard_stats')
        assert _guards_intact(stats, B * Cn * 3) and bool((ws[n // 8:] == 0x5a5a5a5a5a5a5a5a).all())
        got = stats[G:G + B * Cn * 3].cpu().view(B, Cn, 3).numpy()
        assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), c.id
    assert LC.hs_left_out(d['x']) == 0


# ---- combination -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', LC.cb_cases(), ids=lambda c: c.id)
def test_loss_combine_case(dev, c):
    lib, chk = _lib().load(), _lib().check
    d = LC.cb_draw(c)
    L, B, Cn, k = c.L, c.B, c.C, d['k']
    consts = LC.CB_CONSTS[c.consts]
    n = L * B * Cn
    stats = d['stats'].to(dev)
    dice = stats.view(-1)[1:] if c.stride == 4 else (stats[..., 1:4] * k).contiguous()             # (doubling is exact)
    cek, dk = d['ce_coef'].to(dev), d['dice_coef'].to(dev)
    out3, gst = _guarded(dev, 3), _guarded(dev, n * 4)
    chk(lib.mt_loss_combine(_p(stats), _p(dice), c.stride, L, B, Cn, _p(cek), _p(dk), c.flags, c.c0, *[float(v) for v in consts], float(k),
                            _p(out3, G), _p(gst, G), _stream()), 'loss_combine')
    assert _guards_intact(out3, 3) and _guards_intact(gst, n * 4)
    g = gst[G:G + n * 4].cpu().view(L, B, Cn, 4)
    assert bool((g != S).all())                                      # all L * B * C * 4 slots
    (loss, ce, dc), gref = LC.cb_reference(d['stats'], k, d['ce_coef'], d['dice_coef'], c.flags, c.c0, consts)
    o = [float(v) for v in out3[G:G + 3].cpu()]
    M, MG = LC.COMBINE_VALUE_MULT * LC.U, LC.COMBINE_GRAD_MULT * LC.U
    rv = max(_ratio('combine_value', abs(o[1] - ce), M * abs(ce) + 1e-300), _ratio('combine_value', abs(o[2] - dc), M * abs(dc) + 1e-300),
             _ratio('combine_value', abs(o[0] - loss), M * (abs(ce) + abs(dc))))
    assert torch.equal(g[..., 0].double(), gref[..., 0])             # the CE column is the level's coefficient or 0, exactly
    err = (g.double() - gref).abs()[..., 1:]
    per_level = gref[..., 1:].abs().amax((1, 2, 3), keepdim=True)
    per_entry = (gref[..., 1].abs() + 2 * gref[..., 2].abs())[..., None]
    rg = max(_ratio('combine_grad_level', err, MG * per_level + 1e-300), _ratio('combine_grad_entry', err, MG * per_entry + 1e-300))
    print('%s: value err / bound %.3f (x %d U), gradient %.3f (x %d U)' % (c.id, rv, LC.COMBINE_VALUE_MULT, rg, LC.COMBINE_GRAD_MULT))
    assert rv <= 1.0 and rg <= 1.0, (rv, rg)
    assert torch.equal(g[..., 2], g[..., 3])
    if c.c0:
        assert bool((g[:, :, 0, 1:] == 0).all())
    if not c.flags & LC.OVER_B and c.consts == 'multitalent':        # the clamp branch: regions a sample does not carry
        flat, gflat = g.view(-1, 4), gref.view(-1, 4)
        rows = [i for i in d['rows']['zero'] + [d['rows']['below']] if i is not None and i % Cn >= c.c0]
        assert rows or n < 8
        for i in rows:
            want = -float(d['dice_coef'][i // (B * Cn)]) * k * 2.0 / LC.f32(1e-7)
            assert abs(float(flat[i, 1]) - want) <= 4 * LC.U * abs(want) and float(flat[i, 2]) == 0.0 and float(flat[i, 3]) == 0.0, i
            assert float(gflat[i, 2]) == 0.0
        i = d['rows']['above']
        if i is not None and i % Cn >= c.c0:                         # just above the clamp: the ratio's own gradient, fp and fn included
            assert float(flat[i, 2]) > 0.0 and abs(float(gflat[i, 1])) < 2.0 * k * float(d['dice_coef'][i // (B * Cn)]) / LC.f32(1e-7)


# ---- optimizer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', LC.ss_cases(), ids=lambda c: c.id)
def test_sumsq_case(dev, c):
    lib, chk = _lib().load(), _lib().check
    x = LC.ss_draw(c)
    xd = x.to(dev)
    assert xd.data_ptr() % 16 == 0
    nws = lib.mt_sumsq_workspace(c.n)
    ws = _guarded(dev, nws // 4, float('nan'))
    out = _guarded(dev, 1)
    for _ in range(2):
        chk(lib.mt_sumsq(_p(xd), c.n, _p(out, G), _p(ws, G), nws, _stream()), 'sumsq')
    assert _guards_intact(out, 1) and _guards_intact(ws, nws // 4) and torch.equal(xd.cpu(), x)
    got, ref = float(out[G]), LC.ss_reference(x)
    if c.big == 1e20:
        assert got == float('inf') and ref > 3.5e38                  # the fp32 sum of squares overflows, as the fp32 norm of torch does
    else:
        r = _ratio('sumsq', abs(got - ref), LC.SUMSQ_MULT * LC.U * ref)
        print('%s: err / bound %.3f' % (c.id, r))
        assert r <= 1.0, (got, ref)


def test_sumsq_refusals(dev):
    lib = _lib().load()
    x, out, ws = torch.zeros(64, device=dev), torch.zeros(1, device=dev), torch.zeros(1024, device=dev)
    assert lib.mt_sumsq(_p(x, 1), 32, _p(out), _p(ws), 4096, _stream()) == -1 and b'16-byte' in lib.mt_last_error()
    assert lib.mt_sumsq(_p(x), 32, _p(out), _p(ws), 4092, _stream()) == -2 and b'workspace' in lib.mt_last_error()
    assert lib.mt_sumsq(_p(x), 32, _p(out), _p(ws), 4096, _stream()) == 0 and float(out) == 0.0


@pytest.mark.parametrize('c', LC.sg_cases(), ids=lambda c: c.id)
def test_sgd_nesterov_case(dev, c):
    lib, chk = _lib().load(), _lib().check
    d = LC.sg_draw(c)
    n = c.n
    lr, wd, mom, mx = LC.SG_HP

    def place(t):                                                    # all three buffers one float into their allocations
        b = torch.full((1 + n + G,), S)
        b[1:1 + n] = t
        return b.to(dev)

    p, buf = place(d['p']), place(d['buf'])
    pref, bref = d['p'].double(), d['buf'].double()
    for step, mode in enumerate(c.steps):
        first = step == 0
        g = place(d['grads'][step])
        ss = LC.sg_sumsq(mode)
        ssd = None if ss is None else torch.tensor([ss], device=dev)
        chk(lib.mt_sgd_nesterov(_p(p, 1), _p(g, 1), _p(buf, 1), n, lr, wd, mom, int(first), _p(ssd) if ssd is not None else C.c_void_p(0), mx,
                                _stream()), 'sgd_nesterov')
        pref, bref = LC.sg_reference(pref, bref, d['grads'][step], first, ss)
        ph, bh, gh = p.cpu(), buf.cpu(), g.cpu()
        for t in (ph, bh, gh):
            assert float(t[0]) == S and bool((t[1 + n:] == S).all())
        assert torch.equal(gh[1:1 + n], d['grads'][step])            # the gradient is read only
        rp, rb = LC.relerr(ph[1:1 + n], pref), LC.relerr(bh[1:1 + n], bref)
        _ratio('sgd', max(rp, rb), LC.SGD_RELERR)
        print('%s step %d (%s): relerr p %.2e buf %.2e' % (c.id, step, mode, rp, rb))
        assert rp < LC.SGD_RELERR and rb < LC.SGD_RELERR, (step, rp, rb)
        pref, bref = ph[1:1 + n].double(), bh[1:1 + n].double()      # the next step starts from the stored fp32 values


def test_every_instance_ran():
    """after the cases above (file order): every name the queries can report was reported for a case that ran"""
    want = set(LC.SM_INSTANCES) | {'mt_loss_fwd_kernel', 'mt_loss_fwd_sparse_kernel', 'mt_loss_bwd_wide_kernel', 'mt_loss_bwd_flat_kernel',
                                   'mt_loss_bwd_kernel'}
    print('worst err / bound per quantity: %s' % ', '.join('%s %.3f' % kv for kv in sorted(WORST.items())))
    print(LC.bounds_text())
    assert RAN <= want
    if NRAN[0] == len(LC.mt_cases()) + len(LC.sm_cases()):          # (a selection or another order of the items: nothing to conclude)
        assert RAN == want, RAN ^ want
