"""Every dispatchable instance of the streaming norm / activation kernels (csrc/norm.hip) on real memory against float64: the cases,
the references and the derived bounds are tests/stream_cases.py (see its docstring); tests/test_stream_cases_cpu.py shows that the
cases reach every instance.  Outputs that are assigned start as NaN, outputs that are accumulated into start from random non-zero
values, and everything around an operand's view (other columns of a wider buffer, guard elements) must come back bit-identical."""
import ctypes as Ct

import pytest
import torch

import stream_cases as SC

pytestmark = pytest.mark.gpu

IDS = lambda c: c.id


@pytest.fixture(scope='module')
def env(dev):
    from multitalent_amd import _lib, ops
    return dev, _lib.load(), _lib, ops


def _p(t):
    return Ct.c_void_p(t.data_ptr()) if t is not None else None


class Operand(object):
    """an operand's flat buffer on the host (as drawn) and on the device"""

    def __init__(self, dev, case, op, vals=None, inside=None):
        self.case, self.op = case, op
        self.host, self.mask = SC.place(vals, case, op, inside=inside)
        self.dev = self.host.to(dev)
        assert self.dev.data_ptr() % 256 == 0
        self.cs = case.layout(op)[0]

    def addr(self):
        return self.case.addr(self.op, base=self.dev.data_ptr())

    def ptr(self):
        return Ct.c_void_p(self.addr())

    def fetch(self):
        """(the view [N, V, C] in the storage type, whether everything outside the view is bit-identical to what was uploaded)"""
        after = self.dev.cpu()
        width, c0, off = self.case.layout(self.op)
        c = self.case
        v = after[off:off + c.N * c.V * width].view(c.N, c.V, width)[:, :, c0:c0 + c.C].contiguous()
        return v, SC.untouched(self.host, after, self.mask)

    def unchanged(self):
        return _same_bits(self.host, self.dev.cpu())


def _same_bits(a, b):
    iv = {8: torch.int64, 4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


class Guarded(object):
    """a small fp32 vector followed by GUARD sentinels"""

    def __init__(self, dev, vals):
        self.n = vals.numel()
        self.host = torch.cat([vals.reshape(-1).float(), torch.full((SC.GUARD,), SC.SENTINEL)])
        self.dev = self.host.to(dev)

    def fetch(self, shape=None):
        after = self.dev.cpu()
        assert _same_bits(after[self.n:], self.host[self.n:]), "guard elements behind an output changed"
        return after[:self.n].reshape(shape) if shape is not None else after[:self.n]


def _maybe(dev, t):
    return t.to(dev) if t is not None else None


def _operands(dev, case, d, outputs=()):
    ops_ = {}
    for op in case.operands():
        src = {'res': 'y2'}.get(op, op)
        ops_[op] = Operand(dev, case, op, inside=float('nan')) if op in outputs else Operand(dev, case, op, vals=d[src])
    return ops_


def _real_instance(ops, case, X):
    assert SC.ask(ops, case, lambda op: X[op].addr()) == SC.claim(case), "the real addresses take another instance than the case claims"


@pytest.mark.parametrize('case', SC.by_family('bwd'), ids=IDS)
def test_inorm_lrelu_bwd_instance(env, case):
    dev, lib, _lib, ops = env
    d = SC.draw(case)
    N, V, C, o = case.N, case.V, case.C, case.opts
    X = _operands(dev, case, d)
    _real_instance(ops, case, X)
    mean, rstd, gamma, beta = d['mean'].to(dev), d['rstd'].to(dev), _maybe(dev, d['gamma']), _maybe(dev, d['beta'])
    dgamma = None if 'nodgb' in o else Guarded(dev, d['dgamma0'])                  # += : random non-zero start
    dbeta = None if 'nodgb' in o else Guarded(dev, d['dbeta0'])
    dbias = None if 'nodbias' in o else Guarded(dev, torch.full((C,), float('nan')))     # = : NaN start
    part = SC.bwd_partials(case, d) if 'part' in o else None
    partd = _maybe(dev, part)
    nbytes = lib.mt_inorm_bwd_workspace(N, V, C)
    ws = torch.full((nbytes // 4 + SC.GUARD,), SC.SENTINEL, device=dev)
    rc = lib.mt_inorm_lrelu_bwd(X['g'].ptr(), X['g'].cs, X['y'].ptr(), X['y'].cs, _p(mean), _p(rstd), _p(gamma), _p(beta), SC.SLOPE, N, V, C,
                                _p(dgamma.dev) if dgamma else None, _p(dbeta.dev) if dbeta else None, _p(dbias.dev) if dbias else None,
                                _p(partd), SC.PART_NBLK if part is not None else 0, C + SC.PART_PAD if part is not None else 0,
                                SC.PART_C0 if part is not None else 0, _p(ws), nbytes, case.gt, case.at, None)
    _lib.check(rc, case.id)
    torch.cuda.synchronize()
    dy, clean = X['g'].fetch()
    assert clean, "inorm_lrelu_bwd wrote outside the view of g"
    assert X['y'].unchanged() and bool((ws[nbytes // 4:] == SC.SENTINEL).all())
    assert part is None or _same_bits(part, partd.cpu())
    SC.check_bwd(case, d, part, dy, dgamma.fetch() if dgamma else None, dbeta.fetch() if dbeta else None, dbias.fetch() if dbias else None)


@pytest.mark.parametrize('case', SC.by_family('apply'), ids=IDS)
def test_inorm_lrelu_apply_instance(env, case):
    dev, lib, _lib, ops = env
    d = SC.draw(case)
    X = _operands(dev, case, d, outputs=('out',))
    _real_instance(ops, case, X)
    sc, sh, sc2, sh2 = (_maybe(dev, d[k]) for k in ('sc', 'sh', 'sc2', 'sh2'))
    res = X.get('res')
    rc = lib.mt_inorm_lrelu_apply(X['y'].ptr(), X['y'].cs, _p(sc), _p(sh), SC.SLOPE, res.ptr() if res else None, res.cs if res else 0, _p(sc2), _p(sh2),
                                  SC.SLOPE, X['out'].ptr(), X['out'].cs, case.N, case.V, case.C, case.at, None)
    _lib.check(rc, case.id)
    torch.cuda.synchronize()
    out, clean = X['out'].fetch()
    assert clean, "inorm_lrelu_apply wrote outside the view of out"
    assert X['y'].unchanged() and (res is None or res.unchanged())
    SC.check_apply(case, d, out)


def _lrelu_bwd_inputs(env, case):
    dev, lib, _lib, ops = env
    d = SC.draw(case)
    X = _operands(dev, case, d, outputs=('gcopy',))
    _real_instance(ops, case, X)
    return d, X, tuple(_maybe(dev, d[k]) for k in ('sc', 'sh', 'sc2', 'sh2'))


def _lrelu_bwd_outputs(case, d, X):
    want = SC.lbwd_ref(case, d)
    got, clean = X['g'].fetch()
    assert clean, "wrote outside the view of g"
    bad = got.view(torch.int16 if got.element_size() == 2 else torch.int32) != want.view(torch.int16 if want.element_size() == 2 else torch.int32)
    assert not bool(bad.any()), "%d elements of g differ from g | fl(g * slope), first at %s" % (int(bad.sum()), bad.nonzero()[0].tolist())
    if 'gcopy' in X:
        cp, clean = X['gcopy'].fetch()
        assert clean, "wrote outside the view of gcopy"
        assert _same_bits(cp, got)
    assert X['y'].unchanged() and ('y2' not in X or X['y2'].unchanged())
    return got


@pytest.mark.parametrize('case', SC.by_family('lbwd'), ids=IDS)
def test_lrelu_bwd_instance(env, case):
    dev, lib, _lib, ops = env
    d, X, (sc, sh, sc2, sh2) = _lrelu_bwd_inputs(env, case)
    y2, cp = X.get('y2'), X.get('gcopy')
    rc = lib.mt_lrelu_bwd(X['g'].ptr(), X['g'].cs, X['y'].ptr(), X['y'].cs, _p(sc), _p(sh), SC.SLOPE, y2.ptr() if y2 else None, y2.cs if y2 else 0,
                          _p(sc2), _p(sh2), SC.SLOPE, cp.ptr() if cp else None, cp.cs if cp else 0, case.N, case.V, case.C, case.gt, case.at, None)
    _lib.check(rc, case.id)
    torch.cuda.synchronize()
    _lrelu_bwd_outputs(case, d, X)


@pytest.mark.parametrize('case', SC.by_family('lstats'), ids=IDS)
def test_lrelu_bwd_stats_instance(env, case):
    dev, lib, _lib, ops = env
    d, X, (sc, sh, sc2, sh2) = _lrelu_bwd_inputs(env, case)
    y2, cp = X.get('y2'), X.get('gcopy')
    nblk = lib.mt_lrelu_bwd_stats_blocks(case.V, case.C)
    assert nblk == SC.nb_blocks(case.V)
    part = Guarded(dev, torch.full((case.N * nblk * case.C * 2,), float('nan')))
    mean, rstd = d['mean'].to(dev), d['rstd'].to(dev)
    rc = lib.mt_lrelu_bwd_stats(X['g'].ptr(), X['y'].ptr(), _p(sc), _p(sh), SC.SLOPE, y2.ptr() if y2 else None, _p(sc2), _p(sh2), SC.SLOPE,
                                cp.ptr() if cp else None, _p(mean), _p(rstd), _p(part.dev), case.N, case.V, case.C, case.gt, case.at, None)
    _lib.check(rc, case.id)
    torch.cuda.synchronize()
    got = _lrelu_bwd_outputs(case, d, X)
    SC.check_lstats(case, d, got, part.fetch((case.N, nblk, case.C, 2)))


@pytest.mark.parametrize('tag,N,V,C,dt,lay,accumulate', SC.CHANNEL_SUM_CASES, ids=[c[0] for c in SC.CHANNEL_SUM_CASES])
def test_channel_sum(env, tag, N, V, C, dt, lay, accumulate):
    dev, lib, _lib, ops = env
    case = SC.Case('csum', tag, N, V, C, (dt, dt), 'channel_sum_kernel', lay={'y': lay + (0,)})
    g = torch.Generator().manual_seed(41)
    x = SC.rnd(torch.randn((N, V, C), generator=g) + 0.25, dt)
    X = Operand(dev, case, 'y', vals=x)
    out0 = torch.randn(C, generator=g) + 3.0 if accumulate else torch.full((C,), float('nan'))
    out = Guarded(dev, out0)
    nbytes = lib.mt_channel_sum_workspace(N, V, C)
    ws = torch.empty(nbytes // 4 + 16, device=dev)
    _lib.check(lib.mt_channel_sum(X.ptr(), X.cs, N, V, C, _p(out.dev), accumulate, _p(ws), nbytes, dt, None), tag)
    torch.cuda.synchronize()
    assert X.unchanged()
    ref, mag = x.sum((0, 1)), x.abs().sum((0, 1))
    if accumulate:
        ref, mag = ref + out0.double(), mag + out0.double().abs()
    SC.sum_close(out.fetch(), ref, mag, SC.chain_strided(V) + SC.TAIL, 'channel_sum')


@pytest.mark.parametrize('nsb', SC.FINALIZE_NSB)
def test_inorm_finalize(env, nsb):
    """fp64 arithmetic on the same fp32 partials, with the clamp var < 0 -> 0; one channel is a constant whose partials give var <= 0"""
    dev, lib, _lib, ops = env
    N, C, per = 2, SC.FINALIZE_C, 16
    g = torch.Generator().manual_seed(100 + nsb)
    vals = torch.randn((N, nsb, C, per), generator=g, dtype=torch.float64) * 2 + 0.7
    cval, cch = SC.FINALIZE_CONST
    v = float(torch.tensor(cval, dtype=torch.float32))
    vals[:, :, cch] = v
    part = torch.stack([vals.sum(-1), (vals * vals).sum(-1)], -1).float().contiguous()          # [N][nsb][C][2]
    # the constant channel: every block's sum of squares is the fp32 number just BELOW the exact per v^2 (a 48-bit number, exact in
    # double), as a conversion that rounds down gives it, so that E[x^2] - mean^2 < 0 by far more than any double rounding
    sq = torch.tensor(per * v * v, dtype=torch.float64)
    below = sq.float() if float(sq.float()) < float(sq) else torch.nextafter(sq.float(), torch.tensor(0.0))
    part[:, :, cch, 1] = below
    count = float(nsb * per)
    gamma = None if nsb == 255 else torch.rand(C, generator=g) + 0.5
    beta = None if nsb == 257 else torch.randn(C, generator=g)
    m, rs, scale, shift, raw = SC.finalize_ref(part, count, gamma, beta, 1e-5)
    assert bool((raw[:, cch] < -1e-6).all()) and bool((raw[:, :cch] > 0).all())
    outs = [Guarded(dev, torch.full((N * C,), float('nan'))) for _ in range(4)]
    partd, gd, bd = part.to(dev), _maybe(dev, gamma), _maybe(dev, beta)
    _lib.check(lib.mt_inorm_finalize(_p(partd), N, nsb, C, count, _p(gd), _p(bd), 1e-5,
                                     *[_p(o.dev) for o in outs], None), 'inorm_finalize')
    torch.cuda.synchronize()
    for o, ref, what in zip(outs, (m, rs, scale, shift), ('mean', 'rstd', 'scale', 'shift')):
        got = o.fetch((N, C)).double()
        assert bool(((got - ref).abs() <= 2.0 ** -23 * ref.abs()).all()), (what, float(((got - ref).abs() / ref.abs()).max()))
    assert abs(float(rs[0, cch]) - 1e-5 ** -0.5) < 1e-2          # the clamp: rstd = 1 / sqrt(eps)


@pytest.mark.parametrize('C,V', SC.TRANSPOSE_CASES)
def test_transposes(env, C, V):
    """NCDHW <-> NDHWC with a channel stride of C + 3 on the NDHWC side: bit-exact, nothing else written"""
    dev, lib, _lib, ops = env
    N, cs = 2, C + 3
    g = torch.Generator().manual_seed(7 * C + V)
    x = torch.randn((N, C, V), generator=g)
    case = SC.Case('tr', 't', N, V, C, (SC.F32, SC.F32), 'transpose', lay={'out': (cs, 2, 0), 'y': (cs, 1, 0)})
    # NCDHW -> NDHWC slice
    O = Operand(dev, case, 'out', inside=float('nan'))
    xd = x.to(dev)
    _lib.check(lib.mt_ncdhw_to_ndhwc(_p(xd), O.ptr(), N, C, V, cs, None), 'ncdhw_to_ndhwc')
    torch.cuda.synchronize()
    got, clean = O.fetch()
    assert clean and _same_bits(got, x.permute(0, 2, 1).contiguous())
    # NDHWC slice -> NCDHW
    I = Operand(dev, case, 'y', vals=x.permute(0, 2, 1).double())
    back = Guarded(dev, torch.full((N * C * V,), float('nan')))
    _lib.check(lib.mt_ndhwc_to_ncdhw(I.ptr(), cs, _p(back.dev), N, C, V, None), 'ndhwc_to_ncdhw')
    torch.cuda.synchronize()
    assert I.unchanged() and _same_bits(back.fetch((N, C, V)), x)
