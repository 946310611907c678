"""Thin torch-tensor wrappers over the C ABI (include/mtseg.h).

Everything here is plumbing: torch owns device memory and streams, the arithmetic happens in
libmtseg_hip.so.  Activations are NDHWC tensors [N, D, H, W, C] (possibly channel slices of a wider buffer), float32 or — the
storage of the mixed-precision mode — float16 (activations) / bfloat16 (gradients) (mt_src_t.dtype / odtype).  There is NO CPU fallback: tensors must live on a HIP device.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import mt_conv3d_t, mt_pointwise_t, mt_src_t


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _check_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("multitalent_amd ops require HIP device tensors (no CPU fallback)")


_DT_CODES = {torch.float32: _lib.MT_F32, torch.bfloat16: _lib.MT_BF16, torch.float16: _lib.MT_F16}


class Act:
    """A (lazy) activation: channel slice [c0, c0+C) of an NDHWC buffer `buf` [N,D,H,W,cs], read as
    lrelu_slope(buf*scale + shift) when scale is not None (InstanceNorm+LeakyReLU applied on load)."""

    __slots__ = ('buf', 'c0', 'C', 'scale', 'shift', 'slope', 'mean', 'rstd')

    def __init__(self, buf, c0=0, C=None, scale=None, shift=None, slope=1.0, mean=None, rstd=None):
        assert buf.dim() == 5 and buf.is_contiguous() and buf.dtype in _DT_CODES
        self.buf, self.c0 = buf, c0
        self.C = buf.shape[4] - c0 if C is None else C
        self.scale, self.shift, self.slope = scale, shift, float(slope)
        self.mean, self.rstd = mean, rstd

    @property
    def N(self): return self.buf.shape[0]

    @property
    def spatial(self): return tuple(self.buf.shape[1:4])

    @property
    def cs(self): return self.buf.shape[4]

    @property
    def V(self): return self.buf.shape[1] * self.buf.shape[2] * self.buf.shape[3]

    @property
    def dtype(self): return self.buf.dtype

    @property
    def dt(self):
        """storage type code of the C ABI (MT_F32 | MT_BF16 | MT_F16)"""
        return _DT_CODES[self.buf.dtype]

    def data_ptr(self):
        return self.buf.data_ptr() + self.buf.element_size() * self.c0

    def with_buf(self, buf, c0=0):
        """the same lazy activation over another buffer (a storage-type copy of the raw values)"""
        return Act(buf, c0=c0, C=self.C, scale=self.scale, shift=self.shift, slope=self.slope, mean=self.mean, rstd=self.rstd)

    def src(self):
        s = mt_src_t()
        s.ptr = self.data_ptr()
        s.cs = self.cs
        s.C = self.C
        s.dtype = self.dt
        s.scale = self.scale.data_ptr() if self.scale is not None else None
        s.shift = self.shift.data_ptr() if self.shift is not None else None
        s.slope = self.slope
        return s

    def dense(self):
        """Materialise to a plain [N,D,H,W,C] tensor with torch ops (test/debug helper only)."""
        x = self.buf[..., self.c0:self.c0 + self.C].float()
        if self.scale is not None:
            x = x * self.scale[:, None, None, None, :] + self.shift[:, None, None, None, :]
            x = torch.where(x > 0, x, x * self.slope)
        return x.contiguous()


def _triple(v):
    return tuple(int(i) for i in v) if isinstance(v, (list, tuple)) or hasattr(v, '__len__') else (int(v),) * 3


class ConvGeom:
    """Geometry of one convolution problem as the kernels see it."""

    def __init__(self, in_spatial, kernel, stride=(1, 1, 1), pad=None, dil=(1, 1, 1), out_spatial=None):
        self.inp = _triple(in_spatial)
        self.k = _triple(kernel)
        self.s = _triple(stride)
        self.p = tuple((k - 1) // 2 for k in self.k) if pad is None else _triple(pad)
        self.dil = _triple(dil)
        if out_spatial is None:
            out_spatial = tuple(((i - 1) * d + 1 + 2 * p - k) // s + 1
                                for i, d, p, k, s in zip(self.inp, self.dil, self.p, self.k, self.s))
        self.out = _triple(out_spatial)


# matrix input type given to every mt_conv3d_t built by fill_conv: 0 = fp32, 1 = bf16 inputs / fp32 accumulation.  The engine
# sets it on entry of pack / forward / backward (Engine.mma), so several engines with different modes can coexist.
_MMA = 0


def set_mma(mode):
    """DEFAULT matrix input type of fill_conv / fill_pointwise when their caller passes none (kernel-level tests and tools; the engine
    passes its own): 0 = fp32 (exact), 1 = bf16 inputs with fp32 accumulation.  Host-side convenience — the C ABI takes mt_conv3d_t.mma."""
    global _MMA
    _MMA = int(mode)


# ---- kernel selection (mt_conv3d_t.select / max_workgroups, ABI 4) ------------------------------------------------------------------
# The library keeps no process-wide switches: which kernel family serves a problem is a field of the problem.  What lives HERE is the
# default this process writes into the structs it builds — 0 (the library's policy) unless a test, an A/B tool (MT_SELECT) or
# set_option changes it.  The legacy option names of rounds 1-5 map onto the fields.
_SEL_SHIFT = {'conv_wino': 0, 'conv_bf16': 2, 'conv_x16': 4, 'conv_tapsplit': 6, 'bwdw_wino': 8, 'bwdw_tr16': 10, 'bwdw_cw': 12}
_SEL_ALIASES = {'wino': 'conv_wino', 'm16': 'conv_bf16', 'x16': 'conv_x16', 'tapsplit': 'conv_tapsplit'}
_select = 0
_caps = {}


def _sel_set(name, code):
    global _select
    sh = _SEL_SHIFT[name]
    _select = (_select & ~(3 << sh)) | ((code & 3) << sh)


def set_option(name, value):
    """Default kernel selection of the problems this process builds (tests, A/B tools).  Legacy names and values:
    conv_wino | conv_bf16 | conv_tapsplit: 0 never, 1 the library's policy, 2 wherever eligible; bwdw_wino: 0 | 1;
    conv_x16 | bwdw_tr16: 0 | 1 | n > 1 = wherever eligible with at most n workgroups (4096: no cap); wino_persist: n > 1 = at most n workers
    per output-channel tile; bwdw_cw: 4 (policy) | 2 | 1 | 104 (four tiles also on small problems)."""
    name = _SEL_ALIASES.get(name, name)
    value = int(value)
    if name == 'wino_persist':
        _caps.pop(name, None) if value <= 1 else _caps.__setitem__(name, value)
    elif name in ('conv_x16', 'bwdw_tr16'):
        _sel_set(name, 1 if value == 0 else 0 if value == 1 else (2 if name == 'conv_x16' else 0))
        _caps.pop(name, None) if value <= 1 or value >= 4096 else _caps.__setitem__(name, value)
    elif name == 'bwdw_cw':
        _sel_set(name, {4: 0, 1: 1, 2: 2, 104: 3}[value])
    elif name in _SEL_SHIFT:
        _sel_set(name, {0: 1, 1: 0, 2: 2}[value])
    else:
        raise ValueError("set_option: unknown option %r" % (name,))


def apply_selection(p):
    """Write the process default selection into an mt_conv3d_t that was built earlier (tests that keep ONE struct while they switch
    between kernel families)."""
    p.select = _select
    p.max_workgroups = min(_caps.values()) if _caps else 0
    return p


def options_are_default():
    return _select == _select_env and not _caps and _MMA == 0


def _parse_select_env():
    """MT_SELECT="x16=off,wino=force,tapsplit=off": the default selection of a whole process (A/B runs of bench.py: tools/ab_env.sh)."""
    for item in os.environ.get('MT_SELECT', '').replace(' ', '').split(','):
        if item:
            k, v = item.split('=')
            k = _SEL_ALIASES.get(k, k)
            if k == 'bwdw_cw':
                set_option(k, int(v))
            else:
                _sel_set(k, {'default': 0, 'off': 1, 'force': 2}[v])


def fill_conv(srcs, geom, Cout, wpack=None, bias=None, out0=None, out1=None, csplit=None, accumulate=False,
              stats_part=None, place=None, mma=None):
    """Build an mt_conv3d_t.  srcs: list of 1-2 Act; out0/out1: Act-like destination slices.
    place = (stored_spatial, out_stride, out_offset): logical output o is written at o*stride + offset."""
    p = mt_conv3d_t()
    p.mma = _MMA if mma is None else int(mma)
    p.select = _select
    p.max_workgroups = min(_caps.values()) if _caps else 0
    p.nsrc = len(srcs)
    for i, a in enumerate(srcs):
        p.src[i] = a.src()
    p.N = srcs[0].N
    p.Di, p.Hi, p.Wi = geom.inp
    p.dilD, p.dilH, p.dilW = geom.dil
    p.Do, p.Ho, p.Wo = geom.out
    p.KD, p.KH, p.KW = geom.k
    p.SD, p.SH, p.SW = geom.s
    p.PD, p.PH, p.PW = geom.p
    p.Cin = sum(a.C for a in srcs)
    p.Cout = Cout
    p.wpack = wpack.data_ptr() if wpack is not None else None
    p.bias = bias.data_ptr() if bias is not None else None
    if out0 is not None:
        p.out0 = out0.data_ptr()
        p.ocs0 = out0.cs
        p.odtype = out0.dt
    if out1 is not None:
        assert out0 is not None and out1.dt == out0.dt, "the two destinations of a convolution share one storage type"
        p.out1 = out1.data_ptr()
        p.ocs1 = out1.cs
    p.csplit = Cout if csplit is None else csplit
    p.accumulate = 1 if accumulate else 0
    p.stats_part = stats_part.data_ptr() if stats_part is not None else None
    if place is not None:
        (p.OD, p.OH, p.OW), (p.osD, p.osH, p.osW), (p.ooD, p.ooH, p.ooW) = place
    return p


def bwd_data_parity_classes(geom):
    """Backward-data of a strided conv (geometry `geom`) as one exact stride-1 convolution per parity class of the input
    position:  dX[S*m + par] = sum_j dY[m - pad' + j] * W[tmax - S*j]  over the taps t = tmax - S*j congruent to
    par + P (mod S).  Returns [(ConvGeom on dY, placement, tapmap)] for fill_conv / pack_conv_weights; classes without taps
    are omitted (their input positions receive no gradient from this conv)."""
    dims = []
    for d in range(3):
        K, S, P, Di = geom.k[d], geom.s[d], geom.p[d], geom.inp[d]
        opts = []
        for par in range(S):
            taps = [t for t in range(K) if (t - par - P) % S == 0]
            cnt = (Di - par + S - 1) // S
            if not taps or cnt <= 0:
                continue
            tmax = max(taps)
            opts.append(dict(par=par, k=len(taps), pad=(tmax - par - P) // S, tb=tmax, ts=-S, cnt=cnt, S=S))
        dims.append(opts)
    out = []
    for a in dims[0]:
        for b in dims[1]:
            for c in dims[2]:
                sel = (a, b, c)
                geomc = ConvGeom(geom.out, tuple(x['k'] for x in sel), (1, 1, 1), tuple(x['pad'] for x in sel),
                                 out_spatial=tuple(x['cnt'] for x in sel))
                place = (geom.inp, tuple(x['S'] for x in sel), tuple(x['par'] for x in sel))
                tapmap = [v for x in sel for v in (x['tb'], x['ts'])]
                out.append((geomc, place, tapmap))
    return out


def conv_ck(p):
    ck = _lib.load().mt_conv3d_ck(C.byref(p))
    if ck <= 0:
        raise RuntimeError("conv3d: no kernel configuration for this shape")
    return ck


def conv_pack_layout(p):
    return _lib.load().mt_conv3d_pack_layout(C.byref(p))


def conv_bwd_data_strided_pack_layout(p):
    return _lib.load().mt_conv3d_bwd_data_strided_pack_layout(C.byref(p))


def conv_kernel_name(p):
    buf = C.create_string_buffer(128)
    _lib.check(_lib.load().mt_conv3d_kernel_name(C.byref(p), buf, 128), 'conv3d_kernel_name')
    return buf.value.decode()


def conv_bwd_weight_kernel_name(p, y):
    buf = C.create_string_buffer(128)
    ys = y.src()
    _lib.check(_lib.load().mt_conv3d_bwd_weight_kernel_name(C.byref(p), C.byref(ys), buf, 128), 'conv3d_bwd_weight_kernel_name')
    return buf.value.decode()


def conv_bwd_data_strided_kernel_name(p):
    buf = C.create_string_buffer(128)
    _lib.check(_lib.load().mt_conv3d_bwd_data_strided_kernel_name(C.byref(p), buf, 128), 'conv3d_bwd_data_strided_kernel_name')
    return buf.value.decode()


def conv_stats_blocks(p):
    return _lib.load().mt_conv3d_stats_blocks(C.byref(p))


_pack_recorder = None      # list while an Engine records its per-step packing program (see Engine._pack)


class PackProgram:
    """All weight packings of one optimizer step as ONE launch (mt_pack_batched): the descriptors are recorded once from the
    ordinary pack_conv_weights calls and live in a device table; valid while the weight and destination buffers are."""

    def __init__(self, records, device):
        lib = _lib.load()
        sz = lib.mt_pack_desc_size()
        self.n = len(records)
        host = (C.c_uint8 * (sz * self.n))()
        self.keep = []
        for i, (w, out, args, tm) in enumerate(records):
            tmc = (C.c_int32 * 6)(*[int(t) for t in tm]) if tm is not None else None
            _lib.check(lib.mt_pack_desc_fill(C.cast(C.byref(host, i * sz), C.c_void_p), _ptr(w), _ptr(out), *args,
                                             C.cast(tmc, C.c_void_p) if tmc is not None else None), 'pack_desc_fill')
            self.keep.append((w, out))
        self.table = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(device)

    def run(self):
        _lib.check(_lib.load().mt_pack_batched(_ptr(self.table), self.n, _stream()), 'pack_batched')


def pack_conv_weights(w, C0, C1, Cout, kernel, strides, flip, ck, out=None, layout=1, tapmap=None):
    """strides = (s_ci, s_co, s_kd, s_kh, s_kw) element strides of `w` for W_eff[tap][ci][co].
    layout 1 = every MFMA kernel (mt_conv3d_fwd with ck = mt_conv3d_ck, mt_pointwise_fwd with ck = POINTWISE_CK)."""
    lib = _lib.load()
    _check_dev(w)
    n = C.c_size_t(0)
    kd, kh, kw = kernel
    tm = (C.c_int32 * 6)(*[int(i) for i in tapmap]) if tapmap is not None else None
    _lib.check(lib.mt_pack_conv_weights(None, None, C.byref(n), C0, C1, Cout, kd, kh, kw, *strides, int(flip), ck, layout, None, None), 'pack(query)')
    if out is None:
        out = torch.empty(n.value, dtype=torch.float32, device=w.device)
    assert out.numel() >= n.value
    if _pack_recorder is not None:
        _pack_recorder.append((w, out, (C0, C1, Cout, kd, kh, kw) + tuple(int(s) for s in strides) + (int(flip), ck, layout), tapmap))
        return out
    _lib.check(lib.mt_pack_conv_weights(_ptr(w), _ptr(out), C.byref(n), C0, C1, Cout, kd, kh, kw, *strides, int(flip), ck, layout,
                                        C.cast(tm, C.c_void_p) if tm is not None else None, _stream()), 'pack')
    return out


def conv_weight_strides(w, transposed_layout=False, as_bwd_data=False):
    """Element strides (s_ci, s_co, s_kd, s_kh, s_kw) for a contiguous nn.Conv3d weight [Cout,Cin,kd,kh,kw]
    (or nn.ConvTranspose3d weight [Cin,Cout,kd,kh,kw] when transposed_layout).  as_bwd_data swaps the
    roles of ci/co (the backward-data conv maps Cout channels back to Cin channels)."""
    k = w.shape[2] * w.shape[3] * w.shape[4]
    s_first, s_second = w.shape[1] * k, k  # strides of dim0 / dim1
    if not transposed_layout:
        s_co, s_ci = s_first, s_second
    else:
        s_ci, s_co = s_first, s_second
    if as_bwd_data:
        s_ci, s_co = s_co, s_ci
    return (s_ci, s_co, w.shape[3] * w.shape[4], w.shape[4], 1)


def conv3d_fwd(p):
    _lib.check(_lib.load().mt_conv3d_fwd(C.byref(p), _stream()), 'conv3d_fwd')


def conv_io_supported(p):
    return bool(_lib.load().mt_conv3d_io_supported(C.byref(p)))


def conv_bwd_data_strided_io_supported(p):
    return bool(_lib.load().mt_conv3d_bwd_data_strided_io_supported(C.byref(p)))


def conv_bwd_weight_io_supported(p, y):
    ys = y.src()
    return bool(_lib.load().mt_conv3d_bwd_weight_io_supported(C.byref(p), C.byref(ys)))


def pointwise_io_supported(p):
    return bool(_lib.load().mt_pointwise_io_supported(C.byref(p)))


def cast(src, dst, accumulate=False):
    """dst (+)= src between storage types (mt_cast); src / dst: Act over the raw values (channel slices allowed)."""
    assert src.N == dst.N and src.V == dst.V and src.C == dst.C
    _lib.check(_lib.load().mt_cast(C.c_void_p(src.data_ptr()), src.cs, src.dt, C.c_void_p(dst.data_ptr()), dst.cs, dst.dt,
                                   src.N * src.V, src.C, int(accumulate), _stream()), 'cast')


def conv3d_bwd_data_strided_supported(p):
    return bool(_lib.load().mt_conv3d_bwd_data_strided_supported(C.byref(p)))


def conv3d_bwd_data_strided(p):
    """dX of a strided 3x3x3 conv in one launch; p = FORWARD geometry with src[0] = dY, out0 = dX (see include/mtseg.h)."""
    _lib.check(_lib.load().mt_conv3d_bwd_data_strided(C.byref(p), _stream()), 'conv3d_bwd_data_strided')


def conv3d_bwd_weight_workspace(p):
    return _lib.load().mt_conv3d_bwd_weight_workspace(C.byref(p))


def conv3d_bwd_weight(p, y, dw, strides, accumulate, ws):
    ys = y.src()
    _lib.check(_lib.load().mt_conv3d_bwd_weight(C.byref(p), C.byref(ys), _ptr(dw), *strides, int(accumulate), _ptr(ws),
                                                ws.numel() * ws.element_size(), _stream()), 'conv3d_bwd_weight')


POINTWISE_CK = 16   # mt_pointwise_fwd takes weights packed with layout 1, ck 16


def fill_pointwise(src, base, in_spatial, si, so, Cout, wpack, bias, out, accumulate=False, stats_part=None, mma=0):
    p = mt_pointwise_t()
    p.src = src.src()
    p.N = src.N
    p.Db, p.Hb, p.Wb = base
    p.Di, p.Hi, p.Wi = in_spatial
    p.siD, p.siH, p.siW = si
    p.soD, p.soH, p.soW = so
    p.Cin = src.C
    p.Cout = Cout
    p.wpack = wpack.data_ptr()
    p.bias = bias.data_ptr() if bias is not None else None
    p.out = out.data_ptr()
    p.ocs = out.cs
    p.odtype = out.dt
    p.accumulate = 1 if accumulate else 0
    p.stats_part = stats_part.data_ptr() if stats_part is not None else None
    p.mma = int(mma)
    return p


def pointwise_pack_layout(p):
    return _lib.load().mt_pointwise_pack_layout(C.byref(p))


def pointwise_kernel_name(p):
    buf = C.create_string_buffer(128)
    _lib.check(_lib.load().mt_pointwise_kernel_name(C.byref(p), buf, 128), 'pointwise_kernel_name')
    return buf.value.decode()


def pointwise_launch_shape(p):
    """(grid x, y, z, store form `wide` 0 / 1 / 2) of the launch mt_pointwise_fwd makes for p."""
    shape = (C.c_int32 * 4)()
    _lib.check(_lib.load().mt_pointwise_launch_shape(C.byref(p), shape), 'pointwise_launch_shape')
    return tuple(shape)


def pointwise_fwd(p):
    _lib.check(_lib.load().mt_pointwise_fwd(C.byref(p), _stream()), 'pointwise_fwd')


def head_bwd_supported(Cin, Cout):
    return bool(_lib.load().mt_head_bwd_supported(int(Cin), int(Cout)))


def head_bwd(x, dy, wpack_bwd, dx, accumulate_dx, dw, s_ci, s_co, dbias, accumulate_dw, ws):
    """Fused backward of a 1x1x1 head: x = Act (head input, lazy), dy = Act over the dense gradient of the logits, dx = Act over the
    gradient buffer of the head's input.  Returns True when dbias was produced (see mt_head_bwd)."""
    lib = _lib.load()
    assert dy.dt == _lib.MT_F32, "mt_head_bwd reads the fp32 loss gradient"
    xs = x.src()
    done = C.c_int(0)
    _lib.check(lib.mt_head_bwd(C.byref(xs), C.c_void_p(dy.data_ptr()), dy.cs, x.N, x.V, x.C, dy.C, _ptr(wpack_bwd),
                               C.c_void_p(dx.data_ptr()), dx.cs, dx.dt, int(accumulate_dx), _ptr(dw), int(s_ci), int(s_co), _ptr(dbias),
                               int(accumulate_dw), C.byref(done), _ptr(ws), ws.numel() * ws.element_size(), _stream()), 'head_bwd')
    return bool(done.value)


def head_bwd_kernel_name(x, dy, dx):
    """(main kernel instance, dbias_done) of the launch head_bwd makes for these operands."""
    xs = x.src()
    buf, done = C.create_string_buffer(128), C.c_int(0)
    _lib.check(_lib.load().mt_head_bwd_kernel_name(C.byref(xs), dy.cs, x.N, x.V, x.C, dy.C, dx.cs, dx.dt, buf, 128, C.byref(done)),
               'head_bwd_kernel_name')
    return buf.value.decode(), bool(done.value)


def head_bwd_io_supported(x, dx, Cout):
    return bool(_lib.load().mt_head_bwd_io_supported(x.dt, x.cs, dx.dt, dx.cs, x.C, int(Cout)))


def head_bwd_workspace(N, V, Cin, Cout):
    return _lib.load().mt_head_bwd_workspace(int(N), int(V), int(Cin), int(Cout))


def pointwise_stats_blocks(p):
    return _lib.load().mt_pointwise_stats_blocks(C.byref(p))


def inorm_finalize(part, N, nsb, Cn, count, gamma, beta, eps, mean, rstd, scale, shift):
    _lib.check(_lib.load().mt_inorm_finalize(_ptr(part), N, nsb, Cn, float(count), _ptr(gamma), _ptr(beta), float(eps),
                                             _ptr(mean), _ptr(rstd), _ptr(scale), _ptr(shift), _stream()), 'inorm_finalize')


def inorm_lrelu_apply(y, out, res=None):
    """out = lrelu_slope(y*scale+shift [+ res as lazy act]) materialised; y/res/out are Act."""
    _lib.check(_lib.load().mt_inorm_lrelu_apply(
        C.c_void_p(y.data_ptr()), y.cs, _ptr(y.scale), _ptr(y.shift), y.slope,
        C.c_void_p(res.data_ptr()) if res is not None else None, res.cs if res is not None else 0,
        _ptr(res.scale) if res is not None else None, _ptr(res.shift) if res is not None else None,
        res.slope if res is not None else 1.0,
        C.c_void_p(out.data_ptr()), out.cs, y.N, y.V, y.C, _same_dt(y, out, res), _stream()), 'inorm_lrelu_apply')


def _same_dt(*acts):
    """the streaming kernels take ONE storage type for all their activation operands and one for all their gradient operands (the
    engine chooses them per resolution level)"""
    dts = {a.dt for a in acts if a is not None}
    if len(dts) != 1:
        raise RuntimeError("operands of a streaming kernel must share one storage type (got %s): convert with ops.cast" % sorted(dts))
    return dts.pop()


def inorm_bwd_workspace(N, V, Cn):
    return _lib.load().mt_inorm_bwd_workspace(N, V, Cn)


def inorm_lrelu_bwd(g, y, gamma, beta, dgamma, dbeta, dbias, ws, part=None, part_c0=0):
    """g (Act over the gradient buffer, in place -> dy); y: Act with mean/rstd/slope of the forward.  part: [N, nblk, cs, 2] first-pass
    partials written by the convolution that produced g (mt_conv3d_t.bstats), this layer's channels at columns part_c0 .."""
    if part is not None:
        assert part.dim() == 4 and part.shape[0] == y.N and part.shape[3] == 2 and part.is_contiguous()
    _lib.check(_lib.load().mt_inorm_lrelu_bwd(
        C.c_void_p(g.data_ptr()), g.cs, C.c_void_p(y.data_ptr()), y.cs, _ptr(y.mean), _ptr(y.rstd), _ptr(gamma), _ptr(beta),
        y.slope, y.N, y.V, y.C, _ptr(dgamma), _ptr(dbeta), _ptr(dbias), _ptr(part), int(part.shape[1]) if part is not None else 0,
        int(part.shape[2]) if part is not None else 0, int(part_c0), _ptr(ws), ws.numel() * ws.element_size(), g.dt, y.dt, _stream()),
        'inorm_lrelu_bwd')


def _addr(a):
    return C.c_void_p(int(a)) if a else C.c_void_p(0)


def inorm_lrelu_apply_kernel_name(y, ycs, res, rcs, out, ocs, N, V, Cn, dt):
    """The kernel instance mt_inorm_lrelu_apply launches.  y / res / out: ADDRESSES (int, 0 or None = NULL; only NULL-ness and alignment
    are read, nothing needs to stand behind them), dt: storage type code.  Same for the three queries below."""
    buf = C.create_string_buffer(128)
    _lib.check(_lib.load().mt_inorm_lrelu_apply_kernel_name(_addr(y), ycs, _addr(res), rcs, _addr(out), ocs, N, V, Cn, dt, buf, 128),
               'inorm_lrelu_apply_kernel_name')
    return buf.value.decode()


def inorm_lrelu_bwd_kernel_name(g, gcs, y, ycs, N, V, Cn, gdt, ydt, part=0, part_nblk=0, part_cs=0, part_c0=0, mean=64, rstd=64):
    """(name of the kernel that writes dy, whether the launcher's own reduction pass runs, threads per workgroup of the named kernel)"""
    buf = C.create_string_buffer(128)
    red, blk = C.c_int(-1), C.c_int(-1)
    _lib.check(_lib.load().mt_inorm_lrelu_bwd_kernel_name(_addr(g), gcs, _addr(y), ycs, _addr(mean), _addr(rstd), N, V, Cn, _addr(part), part_nblk,
                                                          part_cs, part_c0, gdt, ydt, buf, 128, C.byref(red), C.byref(blk)),
               'inorm_lrelu_bwd_kernel_name')
    return buf.value.decode(), bool(red.value), blk.value


def lrelu_bwd_kernel_name(g, gcs, y, ycs, y2, y2cs, gcopy, gcopycs, N, V, Cn, gdt, ydt):
    buf = C.create_string_buffer(128)
    _lib.check(_lib.load().mt_lrelu_bwd_kernel_name(_addr(g), gcs, _addr(y), ycs, _addr(y2), y2cs, _addr(gcopy), gcopycs, N, V, Cn, gdt, ydt,
                                                    buf, 128), 'lrelu_bwd_kernel_name')
    return buf.value.decode()


def lrelu_bwd_stats_kernel_name(g, y, y2, gcopy, N, V, Cn, gdt, ydt, mean=64, rstd=64, part=64):
    buf = C.create_string_buffer(128)
    _lib.check(_lib.load().mt_lrelu_bwd_stats_kernel_name(_addr(g), _addr(y), _addr(y2), _addr(gcopy), _addr(mean), _addr(rstd), _addr(part),
                                                          N, V, Cn, gdt, ydt, buf, 128), 'lrelu_bwd_stats_kernel_name')
    return buf.value.decode()


def conv_bwd_stats_supported(p):
    return bool(_lib.load().mt_conv3d_bwd_stats_supported(C.byref(p)))


def set_bwd_stats(p, y_act, gamma, beta, c0):
    """fused first pass of the InstanceNorm backward of `y_act`'s layer in the epilogue of the convolution p (the last writer of that
    layer's output gradient): see mt_bwd_stats_t.  The caller keeps the tensors alive and provides p.stats_part."""
    assert y_act.dt == _lib.MT_F32, "the fused norm-backward statistics read an fp32 y"
    b = p.bstats
    b.y, b.ycs, b.c0, b.C = y_act.buf.data_ptr() + 4 * y_act.c0, y_act.cs, int(c0), y_act.C
    b.mean, b.rstd = y_act.mean.data_ptr(), y_act.rstd.data_ptr()
    b.gamma = gamma.data_ptr() if gamma is not None else None
    b.beta = beta.data_ptr() if beta is not None else None
    b.slope = float(y_act.slope)


def channel_sum_workspace(N, V, Cn):
    return _lib.load().mt_channel_sum_workspace(N, V, Cn)


def channel_sum(x, out, accumulate, ws):
    _lib.check(_lib.load().mt_channel_sum(C.c_void_p(x.data_ptr()), x.cs, x.N, x.V, x.C, _ptr(out), int(accumulate), _ptr(ws),
                                          ws.numel() * ws.element_size(), x.dt, _stream()), 'channel_sum')


def loss_workspace(B, V, Cn):
    return _lib.load().mt_loss_workspace(B, V, Cn)


def multitalent_loss_fwd(logits, target, valid, lut, stats, ws):
    _lib.check(_lib.load().mt_multitalent_loss_fwd(C.c_void_p(logits.data_ptr()), logits.cs, _ptr(target), logits.N, logits.V,
                                                   logits.C, _ptr(valid), _ptr(lut), _ptr(stats), _ptr(ws),
                                                   ws.numel() * ws.element_size(), _stream()), 'multitalent_loss_fwd')


def multitalent_loss_bwd(logits, target, valid, lut, gstats, dlogits):
    _lib.check(_lib.load().mt_multitalent_loss_bwd(C.c_void_p(logits.data_ptr()), logits.cs, _ptr(target), logits.N, logits.V,
                                                   logits.C, _ptr(valid), _ptr(lut), _ptr(gstats),
                                                   C.c_void_p(dlogits.data_ptr()), dlogits.cs, _stream()),
               'multitalent_loss_bwd')


def multitalent_hard_stats(logits, target, valid, lut, stats):
    """stats [B, C, 3] = exact (tp, fp, fn) counts of sigmoid(logits) > 0.5 per valid region (online evaluation)."""
    lib = _lib.load()
    n = lib.mt_hard_stats_workspace(logits.N, logits.C)
    ws = torch.empty((n + 7) // 8, dtype=torch.int64, device=stats.device)
    _lib.check(lib.mt_multitalent_hard_stats(C.c_void_p(logits.data_ptr()), logits.cs, _ptr(target), logits.N, logits.V, logits.C,
                                             _ptr(valid), _ptr(lut), _ptr(stats), _ptr(ws), ws.numel() * 8, _stream()),
               'multitalent_hard_stats')


def softmax_dice_ce_fwd(logits, target, stats, ws):
    _lib.check(_lib.load().mt_softmax_dice_ce_fwd(C.c_void_p(logits.data_ptr()), logits.cs, _ptr(target), logits.N, logits.V,
                                                  logits.C, _ptr(stats), _ptr(ws), ws.numel() * ws.element_size(), _stream()),
               'softmax_dice_ce_fwd')


def softmax_dice_ce_bwd(logits, target, gstats, dlogits):
    _lib.check(_lib.load().mt_softmax_dice_ce_bwd(C.c_void_p(logits.data_ptr()), logits.cs, _ptr(target), logits.N, logits.V,
                                                  logits.C, _ptr(gstats),
                                                  C.c_void_p(dlogits.data_ptr()), dlogits.cs, _stream()), 'softmax_dice_ce_bwd')


LOSS_CE_ALL_CHANNELS, LOSS_DICE_OVER_BATCH = 1, 2


def loss_combine(stats, dice, dice_stride, ce_coef, dice_coef, flags, c0, smooth_num, smooth_den, den_eps, clamp_min, out3, gstats, dice_grad_scale=1.0):
    """stats / gstats [L, B, C, 4]; dice = data pointer tensor of the (tp, fp, fn) the ratios are formed from (see mtseg.h)."""
    L, B, Cn = stats.shape[:3]
    _lib.check(_lib.load().mt_loss_combine(_ptr(stats), C.c_void_p(dice.data_ptr()), int(dice_stride), L, B, Cn, _ptr(ce_coef),
                                           _ptr(dice_coef), int(flags), int(c0), float(smooth_num), float(smooth_den), float(den_eps),
                                           float(clamp_min), float(dice_grad_scale), _ptr(out3), _ptr(gstats), _stream()), 'loss_combine')


def multitalent_loss_fwd_kernel_name(cs, V, Cn):
    """(kernel multitalent_loss_fwd launches for logits of channel stride cs, voxels per workgroup, workgroups per sample)"""
    buf, vpb, nblk = C.create_string_buffer(128), C.c_long(0), C.c_int(0)
    _lib.check(_lib.load().mt_multitalent_loss_fwd_kernel_name(int(cs), int(V), int(Cn), buf, 128, C.byref(vpb), C.byref(nblk)),
               'multitalent_loss_fwd_kernel_name')
    return buf.value.decode(), vpb.value, nblk.value


def multitalent_loss_bwd_kernel_name(logits, cs, dlogits, dcs, V, Cn):
    """the same for multitalent_loss_bwd; logits / dlogits: base ADDRESSES (only their alignment is read)"""
    buf, vpb, nblk = C.create_string_buffer(128), C.c_long(0), C.c_int(0)
    _lib.check(_lib.load().mt_multitalent_loss_bwd_kernel_name(C.c_void_p(int(logits)), int(cs), C.c_void_p(int(dlogits)), int(dcs), int(V),
                                                               int(Cn), buf, 128, C.byref(vpb), C.byref(nblk)),
               'multitalent_loss_bwd_kernel_name')
    return buf.value.decode(), vpb.value, nblk.value


def softmax_dice_ce_kernel_name(Cn, backward):
    """the kernel instance softmax_dice_ce_fwd (backward False) / _bwd (True) launches for Cn classes"""
    buf = C.create_string_buffer(128)
    _lib.check(_lib.load().mt_softmax_dice_ce_kernel_name(int(Cn), int(bool(backward)), buf, 128), 'softmax_dice_ce_kernel_name')
    return buf.value.decode()


def sumsq(x, out, ws):
    _lib.check(_lib.load().mt_sumsq(_ptr(x), x.numel(), _ptr(out), _ptr(ws), ws.numel() * ws.element_size(), _stream()), 'sumsq')


def sumsq_workspace(n):
    return _lib.load().mt_sumsq_workspace(n)


def sgd_nesterov(p, g, buf, lr, wd, mom, first_step, sumsq_dev, max_norm):
    _lib.check(_lib.load().mt_sgd_nesterov(_ptr(p), _ptr(g), _ptr(buf), p.numel(), float(lr), float(wd), float(mom),
                                           int(first_step), _ptr(sumsq_dev), float(max_norm), _stream()), 'sgd_nesterov')


def flip_accumulate(logits, flips, nonlin, weight, acc, first):
    D, H, W = logits.spatial
    _lib.check(_lib.load().mt_flip_accumulate(C.c_void_p(logits.data_ptr()), logits.cs, D, H, W, logits.C, int(flips[0]),
                                              int(flips[1]), int(flips[2]), int(nonlin), float(weight), _ptr(acc), int(first),
                                              _stream()), 'flip_accumulate')


def head_flip_accumulate(p, sample, flips, nonlin, weight, acc, first):
    _lib.check(_lib.load().mt_head_flip_accumulate(C.byref(p), int(sample), int(flips[0]), int(flips[1]), int(flips[2]), int(nonlin),
                                                   float(weight), _ptr(acc), int(first), _stream()), 'head_flip_accumulate')


def head_mirror_accumulate(p, sample0, flips, nonlin, weight, gauss, agg, nb, agg_shape, origin):
    """flips: list of (fD, fH, fW) booleans, one per sample (the mirror combinations of ONE tile)."""
    fl = (C.c_int32 * len(flips))(*[int(f[0]) | (int(f[1]) << 1) | (int(f[2]) << 2) for f in flips])
    _lib.check(_lib.load().mt_head_mirror_accumulate(C.byref(p), int(sample0), len(flips), C.cast(fl, C.c_void_p), int(nonlin), float(weight),
                                                     _ptr(gauss), _ptr(agg), _ptr(nb), agg_shape[0], agg_shape[1], agg_shape[2],
                                                     origin[0], origin[1], origin[2], _stream()), 'head_mirror_accumulate')


def head_infer_kernel_name(p, mirror):
    """the kernel instance head_flip_accumulate (mirror False) / head_mirror_accumulate (mirror True) launches for p"""
    buf = C.create_string_buffer(128)
    _lib.check(_lib.load().mt_head_infer_kernel_name(C.byref(p), int(bool(mirror)), buf, 128), 'head_infer_kernel_name')
    return buf.value.decode()


def extract_tiles(vol, patch, tiles, out):
    """vol [C,X,Y,Z] device tensor; tiles: list of ((x0,y0,z0), (fD,fH,fW)); out [len(tiles), C, *patch] — see mt_extract_tiles."""
    _check_dev(vol, out)
    assert vol.is_contiguous() and out.is_contiguous() and vol.dtype == torch.float32 and out.dtype == torch.float32
    flat = []
    for (x0, y0, z0), f in tiles:
        flat += [int(x0), int(y0), int(z0), int(f[0]) | (int(f[1]) << 1) | (int(f[2]) << 2)]
    desc = (C.c_int32 * len(flat))(*flat)
    _lib.check(_lib.load().mt_extract_tiles(_ptr(vol), vol.shape[0], vol.shape[1], vol.shape[2], vol.shape[3], _ptr(out), len(tiles),
                                            patch[0], patch[1], patch[2], C.cast(desc, C.c_void_p), _stream()), 'extract_tiles')
    return out


def tile_accumulate(acc, gauss, Cn, patch, agg, nb, agg_shape, origin):
    _lib.check(_lib.load().mt_tile_accumulate(_ptr(acc), _ptr(gauss), Cn, patch[0], patch[1], patch[2], _ptr(agg), _ptr(nb),
                                              agg_shape[0], agg_shape[1], agg_shape[2], origin[0], origin[1], origin[2],
                                              _stream()), 'tile_accumulate')


def normalize_threshold(agg, nb, Cn, V, class_order, use_regions, seg):
    _lib.check(_lib.load().mt_normalize_threshold(_ptr(agg), _ptr(nb), Cn, V, _ptr(class_order), int(use_regions), _ptr(seg),
                                                  _stream()), 'normalize_threshold')


def ncdhw_to_ndhwc(x, out=None, out_act=None):
    """x [N,C,D,H,W] contiguous -> NDHWC.  Writes into out_act (Act slice) if given."""
    N, Cn = x.shape[0], x.shape[1]
    V = x.shape[2] * x.shape[3] * x.shape[4]
    if out_act is None:
        if out is None:
            out = torch.empty((N,) + tuple(x.shape[2:]) + (Cn,), dtype=torch.float32, device=x.device)
        out_act = Act(out)
    _lib.check(_lib.load().mt_ncdhw_to_ndhwc(_ptr(x), C.c_void_p(out_act.data_ptr()), N, Cn, V, out_act.cs, _stream()),
               'ncdhw_to_ndhwc')
    return out_act.buf


def ndhwc_to_ncdhw(a, out=None):
    N, Cn = a.N, a.C
    D, H, W = a.spatial
    if out is None:
        out = torch.empty((N, Cn, D, H, W), dtype=torch.float32, device=a.buf.device)
    _lib.check(_lib.load().mt_ndhwc_to_ncdhw(C.c_void_p(a.data_ptr()), a.cs, _ptr(out), N, Cn, a.V, _stream()), 'ndhwc_to_ncdhw')
    return out


def downsample_seg_nearest(seg, out_spatial, remove_minus_one=False, out=None):
    """seg: [B, C, D, H, W] float32 label maps (contiguous) -> [B, C, *out_spatial]; see mt_downsample_seg_nearest."""
    _check_dev(seg)
    assert seg.dim() == 5 and seg.dtype == torch.float32 and seg.is_contiguous()
    B, Cn, D, H, W = seg.shape
    if out is None:
        out = torch.empty((B, Cn) + tuple(int(i) for i in out_spatial), dtype=torch.float32, device=seg.device)
    _lib.check(_lib.load().mt_downsample_seg_nearest(_ptr(seg), B * Cn, D, H, W, _ptr(out), *[int(i) for i in out_spatial],
                                                    int(remove_minus_one), _stream()), 'downsample_seg_nearest')
    return out


# ---- the resize unit (csrc/resize.hip): volumes are [NC, D, H, W] float32, contiguous ------------------------------------------------
_RESIZE = "the resize unit runs"
RESIZE_ORDERS = (0, 1, 3)
RESIZE_MAX_ELEMENTS = 2 ** 31 - 1


def _resize_volume(x, who):
    if not torch.is_tensor(x) or x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("%s: a contiguous float32 [NC, D, H, W] tensor is expected" % who)
    _require_device(_RESIZE, x)
    return tuple(int(i) for i in x.shape)


def _resize_out(x, out, shape, who):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=x.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("%s: out must be a contiguous float32 tensor of shape %s on the input's device" % (who, tuple(shape)))
    return out


def resize_prefilter3(x, axes, out=None):
    """mt_resize_prefilter3: cubic B-spline coefficients of x [NC, D, H, W] along the axes of the mask (bit 0 W, bit 1 H, bit 2 D) for
    lines extended by their edge values (scipy's 'nearest').  out: None (a new tensor), x itself (in place) or another tensor."""
    NC, D, H, W = _resize_volume(x, "resize_prefilter3")
    out = _resize_out(x, out, (NC, D, H, W), "resize_prefilter3")
    _lib.check(_lib.load().mt_resize_prefilter3(_ptr(x), _ptr(out), NC, D, H, W, int(axes), _stream()), 'resize_prefilter3')
    return out


def resize(x, out_shape, orders, out=None):
    """mt_resize: x [NC, D, H, W] -> [NC, *out_shape] with one order (0, 1, 3) per axis; an axis of order 3 that changes must hold
    prefilter coefficients (resize_prefilter3), an axis that keeps its extent is copied and must not."""
    NC, D, H, W = _resize_volume(x, "resize")
    out_shape = tuple(int(i) for i in out_shape)
    orders = tuple(int(i) for i in orders)
    if len(out_shape) != 3 or len(orders) != 3:
        raise ValueError("resize: three output extents and three orders are expected, got %s and %s" % (out_shape, orders))
    out = _resize_out(x, out, (NC,) + out_shape, "resize")
    if out.data_ptr() == x.data_ptr():
        raise ValueError("resize: out must not be the input")
    _lib.check(_lib.load().mt_resize(_ptr(x), NC, D, H, W, _ptr(out), *out_shape, *orders, _stream()), 'resize')
    return out


def resize_labels(seg, out_shape, out=None):
    """mt_resize_labels: resize_segmentation(order 1) of label maps [NC, D, H, W] on the axes that change."""
    NC, D, H, W = _resize_volume(seg, "resize_labels")
    out_shape = tuple(int(i) for i in out_shape)
    if len(out_shape) != 3:
        raise ValueError("resize_labels: three output extents are expected, got %s" % (out_shape,))
    out = _resize_out(seg, out, (NC,) + out_shape, "resize_labels")
    _lib.check(_lib.load().mt_resize_labels(_ptr(seg), NC, D, H, W, _ptr(out), *out_shape, _stream()), 'resize_labels')
    return out


def resize_labels_axis(seg, axis, out_n, out=None):
    """mt_resize_labels_axis: the z pass of label maps [NC, D, H, W] along `axis` (0 D, 1 H, 2 W) to `out_n` elements."""
    NC, D, H, W = _resize_volume(seg, "resize_labels_axis")
    shape = [D, H, W]
    if int(axis) not in (0, 1, 2):
        raise ValueError("resize_labels_axis: axis is 0, 1 or 2, got %r" % (axis,))
    shape[int(axis)] = int(out_n)
    out = _resize_out(seg, out, (NC,) + tuple(shape), "resize_labels_axis")
    _lib.check(_lib.load().mt_resize_labels_axis(_ptr(seg), NC, D, H, W, int(axis), int(out_n), _ptr(out), _stream()), 'resize_labels_axis')
    return out


# ---- the data path: post-processing, cropping, training-case preprocessing, evaluation, dataset analysis -----------------------------
MAX_VOXELS = 2 ** 31 - 1         # int32 linear indices and ranks in every kernel of the data path
CC_MAX_VOXELS = CROP_MAX_VOXELS = LABEL_MAX_VOXELS = FG_MAX_VOXELS = MAX_VOXELS
_CC, _CROP = "connected-component post-processing runs", "cropping to the non-zero region runs"
_PRE, _EVAL, _AN = "training-case preprocessing runs", "the evaluation kernels run", "the dataset analysis kernels run"


def _require_device(what, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("multitalent_amd: %s on a HIP device only; there is no CPU fallback" % what)


def _volume_shape(shape, who, allow_empty):
    """A [D, H, W] shape within the int32 index range of the device labelling, checked on the shape alone (nothing is read or
    allocated).  who: "<unit>: <the volume that is expected>"."""
    shape = tuple(int(i) for i in shape)
    if len(shape) != 3 or (not allow_empty and min(shape) < 1):
        raise ValueError("%s is expected, got shape %s" % (who, shape))
    if shape[0] * shape[1] * shape[2] > MAX_VOXELS:
        raise ValueError("%s: %d voxels exceed the int32 index range of the device labelling"
                         % (who.split(':')[0], shape[0] * shape[1] * shape[2]))
    return shape


def _member_table(member):
    """256 host entries, non-zero = in the mask -> the byte table of the C ABI."""
    tab = np.zeros(256, dtype=np.uint8)
    tab[:] = np.asarray(member, dtype=bool).reshape(256)
    return tab


def cc_check_shape(shape):
    """Shape rules of mt_cc_label3d / mt_cc_remove."""
    return _volume_shape(shape, "connected components: a 3-D label volume [D, H, W]", True)


def cc_label3d(seg, member, labels=None, sizes=None, stats=None):
    """seg: [D, H, W] uint8 device tensor (contiguous); member: 256 host entries, non-zero = in the mask.
    -> (labels, sizes, stats) int32 device tensors [D, H, W], [D, H, W], [2] (see mt_cc_label3d).  Nothing is synchronised."""
    D, H, W = cc_check_shape(seg.shape)
    _require_device(_CC, seg)
    assert seg.dtype == torch.uint8 and seg.is_contiguous()
    tab = _member_table(member)
    if labels is None:
        labels = torch.empty((D, H, W), dtype=torch.int32, device=seg.device)
    if sizes is None:
        sizes = torch.empty((D, H, W), dtype=torch.int32, device=seg.device)
    if stats is None:
        stats = torch.empty(2, dtype=torch.int32, device=seg.device)
    _require_device(_CC, labels, sizes, stats)
    _lib.check(_lib.load().mt_cc_label3d(_ptr(seg), D, H, W, tab.ctypes.data_as(C.c_void_p), _ptr(labels), _ptr(sizes), _ptr(stats),
                                         _stream()), 'cc_label3d')
    return labels, sizes, stats


def cc_remove(seg, labels, sizes, stats, volume_per_voxel, min_size=None, removed=None):
    """In place on seg (uint8 device tensor [D, H, W]): zero every component of (labels, sizes, stats) from cc_label3d that
    the reference's rule removes (see mt_cc_remove).  -> `removed`, int32 device tensor [1]: the largest removed count."""
    D, H, W = cc_check_shape(seg.shape)
    _require_device(_CC, seg, labels, sizes, stats)
    assert seg.dtype == torch.uint8 and seg.is_contiguous()
    if removed is None:
        removed = torch.empty(1, dtype=torch.int32, device=seg.device)
    _lib.check(_lib.load().mt_cc_remove(_ptr(seg), D, H, W, _ptr(labels), _ptr(sizes), _ptr(stats), float(volume_per_voxel),
                                        0 if min_size is None else 1, 0.0 if min_size is None else float(min_size), _ptr(removed),
                                        _stream()), 'cc_remove')
    return removed


def crop_check_shape(shape):
    """Shape rules of mt_fill_holes3d / mt_crop_nonzero for a [D, H, W] volume."""
    return _volume_shape(shape, "cropping: a non-empty 3-D volume [D, H, W]", False)


def nonzero_mask(data, mask=None):
    """data: [C, ...] float32 device tensor (contiguous) -> uint8 device tensor data.shape[1:]: 1 where any channel is != 0
    (numpy's rule on the bit pattern, see mt_nonzero_mask).  `mask` may have any alignment.  Nothing is synchronised."""
    _require_device(_CROP, data)
    assert data.dtype == torch.float32 and data.is_contiguous() and data.dim() >= 2
    Cn = int(data.shape[0])
    V = int(data.numel()) // max(Cn, 1)
    if Cn < 1 or V < 1:
        raise ValueError("nonzero_mask: empty input of shape %s" % (tuple(data.shape),))
    if mask is None:
        mask = torch.empty(tuple(data.shape[1:]), dtype=torch.uint8, device=data.device)
    _require_device(_CROP, mask)
    assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() == V
    _lib.check(_lib.load().mt_nonzero_mask(_ptr(data), Cn, V, _ptr(mask), _stream()), 'nonzero_mask')
    return mask


def fill_holes3d(mask, bbox=None, ws=None):
    """In place on mask ([D, H, W] uint8 device tensor, contiguous): scipy.ndimage.binary_fill_holes(mask != 0) as 0 / 1.
    -> (mask, bbox): bbox int32 device tensor [7] = lo_d, hi_d, lo_h, hi_h, lo_w, hi_w (hi exclusive) and the number of set voxels
    (see mt_fill_holes3d).  ws: optional uint8 device scratch of at least fill_holes3d_workspace bytes.  Nothing is synchronised."""
    D, H, W = crop_check_shape(mask.shape)
    _require_device(_CROP, mask)
    assert mask.dtype == torch.uint8 and mask.is_contiguous()
    need = int(_lib.load().mt_fill_holes3d_workspace(D, H, W))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=mask.device)
    if bbox is None:
        bbox = torch.empty(7, dtype=torch.int32, device=mask.device)
    _require_device(_CROP, ws, bbox)
    assert bbox.dtype == torch.int32 and bbox.is_contiguous() and bbox.numel() == 7
    _lib.check(_lib.load().mt_fill_holes3d(_ptr(mask), D, H, W, _ptr(bbox), _ptr(ws), ws.numel() * ws.element_size(), _stream()),
               'fill_holes3d')
    return mask, bbox


def fill_holes3d_workspace(shape):
    D, H, W = crop_check_shape(shape)
    return int(_lib.load().mt_fill_holes3d_workspace(D, H, W))


def crop_nonzero(data, mask, box, seg=None, nonzero_label=-1):
    """data: [C, D, H, W] float32, mask: [D, H, W] uint8, seg: None or [CS, D, H, W] float32 — contiguous device tensors; box: six host
    ints lo_d, hi_d, lo_h, hi_h, lo_w, hi_w.  -> (data[:, box] bit for bit, seg): int8 [1, box] (0 inside the mask, nonzero_label
    outside) without `seg`, else float32 [CS, box] (see mt_crop_nonzero).  Nothing is synchronised."""
    D, H, W = crop_check_shape(mask.shape)
    _require_device(_CROP, data, mask)
    assert data.dtype == torch.float32 and data.is_contiguous() and data.dim() == 4 and tuple(data.shape[1:]) == (D, H, W)
    assert mask.dtype == torch.uint8 and mask.is_contiguous()
    b = np.ascontiguousarray(np.asarray(box, dtype=np.int64).reshape(6))
    dims = (D, D, H, H, W, W)
    if any(b[2 * a] < 0 or b[2 * a] >= b[2 * a + 1] or b[2 * a + 1] > dims[2 * a] for a in range(3)):
        raise ValueError("crop_nonzero: box %s outside the volume %s" % (b.tolist(), (D, H, W)))
    b = b.astype(np.int32)
    bs = (int(b[1] - b[0]), int(b[3] - b[2]), int(b[5] - b[4]))
    out = torch.empty((int(data.shape[0]),) + bs, dtype=torch.float32, device=data.device)
    if seg is None:
        if float(nonzero_label) != int(nonzero_label) or not -128 <= int(nonzero_label) <= 127:
            raise ValueError("crop_nonzero: nonzero_label %r is not an int8 value" % (nonzero_label,))
        seg_out = torch.empty((1,) + bs, dtype=torch.int8, device=data.device)
        seg_ptr, CS = None, 0
    else:
        _require_device(_CROP, seg)
        assert seg.dtype == torch.float32 and seg.is_contiguous() and seg.dim() == 4 and tuple(seg.shape[1:]) == (D, H, W)
        CS = int(seg.shape[0])
        seg_out = torch.empty((CS,) + bs, dtype=torch.float32, device=data.device)
        seg_ptr = _ptr(seg)
    _lib.check(_lib.load().mt_crop_nonzero(_ptr(data), int(data.shape[0]), D, H, W, _ptr(mask), b.ctypes.data_as(C.c_void_p), _ptr(out),
                                           seg_ptr, CS, _ptr(seg_out), float(nonzero_label), _stream()), 'crop_nonzero')
    return out, seg_out


MOMENTS_ALL, MOMENTS_SEG_GE0, MOMENTS_OPEN_RANGE = 0, 1, 2
MOMENTS_MAX_CHANNELS = 16
LABEL_MAX_CLASSES = 255


def masked_moments(data, pred=MOMENTS_ALL, seg=None, lo=None, hi=None, stats=None):
    """data: [C, ...] float32 device tensor (contiguous).  -> stats, float64 device tensor [C, 3] = count, mean, population sd of
    every channel over the voxels the predicate selects: all of them, those with seg >= 0 (seg: float32, data.shape[1:]), or those
    with lo[c] < x < hi[c] (host values); see mt_masked_moments.  Deterministic; nothing is synchronised."""
    _require_device(_PRE, data)
    assert data.dtype == torch.float32 and data.is_contiguous() and data.dim() >= 2
    Cn = int(data.shape[0])
    V = int(data.numel()) // max(Cn, 1)
    if not 1 <= Cn <= MOMENTS_MAX_CHANNELS or V < 1:
        raise ValueError("masked_moments: 1..%d non-empty channels are expected, got shape %s" % (MOMENTS_MAX_CHANNELS, tuple(data.shape)))
    seg_ptr = lo_ptr = hi_ptr = None
    if pred == MOMENTS_SEG_GE0:
        _require_device(_PRE, seg)
        assert seg.dtype == torch.float32 and seg.is_contiguous() and seg.numel() == V
        seg_ptr = _ptr(seg)
    elif pred == MOMENTS_OPEN_RANGE:
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), (Cn,)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), (Cn,)))
        lo_ptr, hi_ptr = lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)
    elif pred != MOMENTS_ALL:
        raise ValueError("masked_moments: unknown predicate %r" % (pred,))
    lib = _lib.load()
    ws = torch.empty(int(lib.mt_masked_moments_workspace(Cn, V)), dtype=torch.uint8, device=data.device)
    if stats is None:
        stats = torch.empty((Cn, 3), dtype=torch.float64, device=data.device)
    _require_device(_PRE, stats)
    assert stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() == Cn * 3
    _lib.check(lib.mt_masked_moments(_ptr(data), Cn, V, int(pred), seg_ptr, lo_ptr, hi_ptr, _ptr(stats), _ptr(ws), ws.numel(), _stream()),
               'masked_moments')
    return stats


def intensity_normalize(x, clip=None, mean=0.0, sd=1.0, stats=None, eps=0.0, seg=None):
    """In place on one channel x (float32 device tensor, contiguous): clip to `clip` = (lo, hi) when given, then
    (x - m) / (s + eps) in float32 with (m, s) = (mean, sd), or the (mean, sd) of `stats` (one float64 device triple of
    masked_moments); where `seg` (float32, same size) is not >= 0 the result is 0.  See mt_intensity_normalize."""
    _require_device(_PRE, x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0
    seg_ptr = stats_ptr = None
    if seg is not None:
        _require_device(_PRE, seg)
        assert seg.dtype == torch.float32 and seg.is_contiguous() and seg.numel() == x.numel()
        seg_ptr = _ptr(seg)
    if stats is not None:
        _require_device(_PRE, stats)
        assert stats.dtype == torch.float64 and stats.numel() == 3 and stats.is_contiguous()
        stats_ptr = _ptr(stats)
    lo, hi = (float(clip[0]), float(clip[1])) if clip is not None else (0.0, 0.0)
    _lib.check(_lib.load().mt_intensity_normalize(_ptr(x), x.numel(), 0 if clip is None else 1, lo, hi, float(mean), float(sd), stats_ptr,
                                                  float(eps), seg_ptr, _stream()), 'intensity_normalize')
    return x


_AUG = "the intensity augmentation runs"
INTENSITY_NONE, INTENSITY_SCALE, INTENSITY_CONTRAST, INTENSITY_GAMMA, INTENSITY_RESTORE = (
    _lib.MT_INTENSITY_NONE, _lib.MT_INTENSITY_SCALE, _lib.MT_INTENSITY_CONTRAST, _lib.MT_INTENSITY_GAMMA, _lib.MT_INTENSITY_RESTORE)
INTENSITY_PRESERVE_RANGE, INTENSITY_NEGATE = _lib.MT_INTENSITY_PRESERVE_RANGE, _lib.MT_INTENSITY_NEGATE
INTENSITY_OP_DTYPE = np.dtype([('op', np.int32), ('flags', np.int32), ('a', np.float32), ('b', np.float32)])     # mt_intensity_op_t


def _channel_batch(x, who):
    """(NC, V) of a contiguous float32 device batch: [N, C, D, H, W] (NC = N*C) or [NC, V]."""
    _require_device(_AUG, x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    if x.dim() not in (2, 5) or x.numel() == 0:
        raise ValueError("%s: a non-empty [N, C, D, H, W] or [NC, V] batch is expected, got shape %s" % (who, tuple(x.shape)))
    NC = int(x.shape[0]) if x.dim() == 2 else int(x.shape[0]) * int(x.shape[1])
    return NC, int(x.numel()) // NC


def channel_stats(x, active=None, stats=None):
    """x: [N, C, D, H, W] or [NC, V] float32 device batch (contiguous).  -> stats, float64 device tensor [NC, 4] = min, max, mean,
    population sd of every channel whose entry of the host array `active` (NC booleans; None = all) is set; the other rows of a
    given `stats` are left as they are.  One pass, deterministic; nothing is synchronised.  See mt_channel_stats."""
    NC, V = _channel_batch(x, 'channel_stats')
    act_ptr = None
    if active is not None:
        active = np.ascontiguousarray(np.asarray(active).reshape(-1) != 0, dtype=np.uint8)
        if active.size != NC:
            raise ValueError("channel_stats: %d activity flags for %d channels" % (active.size, NC))
        act_ptr = active.ctypes.data_as(C.c_void_p)
    if stats is None:
        stats = torch.empty((NC, 4), dtype=torch.float64, device=x.device)
    _require_device(_AUG, stats)
    assert stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() == NC * 4
    lib = _lib.load()
    ws = torch.empty(int(lib.mt_channel_stats_workspace(NC, V)), dtype=torch.uint8, device=x.device)
    _lib.check(lib.mt_channel_stats(_ptr(x), NC, V, act_ptr, _ptr(stats), _ptr(ws), ws.numel(), _stream()), 'channel_stats')
    return stats


def intensity_apply(x, records, stats=None, stats2=None):
    """In place on x ([N, C, D, H, W] or [NC, V] float32 device batch, contiguous): one op per channel from the host array `records`
    (NC entries of INTENSITY_OP_DTYPE: op INTENSITY_*, flags, a, b), its statistics from `stats` / `stats2` ([NC, 4] float64 device
    tensors of channel_stats, enqueued before on the same stream).  Nothing is synchronised.  See mt_intensity_apply."""
    NC, V = _channel_batch(x, 'intensity_apply')
    records = np.ascontiguousarray(np.asarray(records, dtype=INTENSITY_OP_DTYPE).reshape(-1))
    if records.size != NC:
        raise ValueError("intensity_apply: %d records for %d channels" % (records.size, NC))
    for s in (stats, stats2):
        if s is not None:
            _require_device(_AUG, s)
            assert s.dtype == torch.float64 and s.is_contiguous() and s.numel() == NC * 4
    _lib.check(_lib.load().mt_intensity_apply(_ptr(x), NC, V, records.ctypes.data_as(C.POINTER(_lib.mt_intensity_op_t)), _ptr(stats),
                                              _ptr(stats2), _stream()), 'intensity_apply')
    return x


class LabelIndex:
    """State between label_counts and label_locations: the label map, the label-to-slot table and the unit offsets."""

    def __init__(self, seg, table, nslots, counts, ws):
        self.seg, self.table, self.nslots, self.counts, self.ws = seg, table, nslots, counts, ws


def label_counts(seg, all_classes):
    """seg: [D, H, W] float32 label map (contiguous device tensor); all_classes: up to 255 distinct non-negative integer labels.
    -> (counts, index): counts[i] (int64 device tensor) = number of voxels with label all_classes[i]; `index` goes to
    label_locations.  See mt_label_counts.  Nothing is synchronised."""
    shape = tuple(int(i) for i in seg.shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("label_counts: a non-empty 3-D label map [D, H, W] is expected, got shape %s" % (shape,))
    if shape[0] * shape[1] * shape[2] > LABEL_MAX_VOXELS:
        raise ValueError("label_counts: %d voxels exceed the int32 index range of the device compaction" % (shape[0] * shape[1] * shape[2]))
    classes = [int(c) for c in all_classes]
    if not 1 <= len(classes) <= LABEL_MAX_CLASSES or min(classes) < 0 or len(set(classes)) != len(classes):
        raise ValueError("label_counts: 1..%d distinct non-negative labels are expected, got %s" % (LABEL_MAX_CLASSES, classes))
    if any(c != f for c, f in zip(classes, all_classes)):
        raise ValueError("label_counts: labels must be integers, got %s" % (list(all_classes),))
    _require_device(_PRE, seg)
    assert seg.dtype == torch.float32 and seg.is_contiguous()
    tab = np.full(max(classes) + 1, 255, dtype=np.uint8)
    tab[classes] = np.arange(len(classes), dtype=np.uint8)
    table = torch.from_numpy(tab).to(seg.device)
    lib = _lib.load()
    V = seg.numel()
    ws = torch.empty(int(lib.mt_label_counts_workspace(V, len(classes))), dtype=torch.uint8, device=seg.device)
    counts = torch.empty(len(classes), dtype=torch.int64, device=seg.device)
    _lib.check(lib.mt_label_counts(_ptr(seg), V, _ptr(table), table.numel(), len(classes), _ptr(counts), _ptr(ws), ws.numel(), _stream()),
               'label_counts')
    return counts, LabelIndex(seg, table, len(classes), counts, ws)


def label_locations(index, qslot, qrank, total=None):
    """index: from label_counts; qslot / qrank: equally long host or device integer arrays, query i asks for the qrank[i]-th voxel
    (C order) with label all_classes[qslot[i]].  -> int64 device tensor [n, 3] of coordinates = np.argwhere(seg == c)[rank]
    (-1 for a rank outside the count).  total: sum of the counts when the caller already has it on the host (sizes the scratch);
    otherwise it is read back here."""
    seg = index.seg
    qslot = torch.as_tensor(np.asarray(qslot) if not torch.is_tensor(qslot) else qslot).to(device=seg.device, dtype=torch.int32).contiguous()
    qrank = torch.as_tensor(np.asarray(qrank) if not torch.is_tensor(qrank) else qrank).to(device=seg.device, dtype=torch.int64).contiguous()
    assert qslot.dim() == 1 and qslot.shape == qrank.shape
    n = int(qslot.numel())
    out = torch.empty((n, 3), dtype=torch.int64, device=seg.device)
    if n == 0:
        return out
    if total is None:
        total = int(index.counts.sum().item())
    total = int(total)
    if total < 1:
        return out.fill_(-1)
    idx = torch.empty(total, dtype=torch.int32, device=seg.device)
    D, H, W = (int(i) for i in seg.shape)
    _lib.check(_lib.load().mt_label_locations(_ptr(seg), D, H, W, _ptr(index.table), index.table.numel(), index.nslots, _ptr(index.ws),
                                              index.ws.numel(), _ptr(idx), total, _ptr(qslot), _ptr(qrank), n, _ptr(out), _stream()),
               'label_locations')
    return out


SD_MAX_AXIS = 32766             # mt_surface_distances: int16 site offsets
SELECT_MAX_RANKS = 8


def seg_joint_hist(test, ref, remap, num_classes, hist=None):
    """test, ref: contiguous uint8 device tensors of the same shape (any number of axes); remap: 256 host entries in
    0..num_classes-1.  -> hist, int64 device tensor [num_classes, num_classes]: hist[i, j] = #{v : remap[test[v]] == i and
    remap[ref[v]] == j}, exact (see mt_seg_joint_hist).  Nothing is synchronised."""
    if tuple(test.shape) != tuple(ref.shape):
        raise ValueError("seg_joint_hist: shape mismatch: %s and %s" % (tuple(test.shape), tuple(ref.shape)))
    Cn = int(num_classes)
    if not 1 <= Cn <= 256:
        raise ValueError("seg_joint_hist: num_classes %d outside 1..256" % Cn)
    tab = np.asarray(remap).reshape(256)
    if tab.min() < 0 or tab.max() >= Cn:
        raise ValueError("seg_joint_hist: remap entries must lie in 0..%d" % (Cn - 1))
    tab = np.ascontiguousarray(tab, dtype=np.uint8)
    _require_device(_EVAL, test, ref)
    assert test.dtype == torch.uint8 and ref.dtype == torch.uint8 and test.is_contiguous() and ref.is_contiguous()
    if test.numel() == 0:
        raise ValueError("seg_joint_hist: empty volume")
    if hist is None:
        hist = torch.empty((Cn, Cn), dtype=torch.int64, device=test.device)
    _require_device(_EVAL, hist)
    assert hist.dtype == torch.int64 and hist.is_contiguous() and hist.numel() == Cn * Cn
    _lib.check(_lib.load().mt_seg_joint_hist(_ptr(test), _ptr(ref), test.numel(), tab.ctypes.data_as(C.c_void_p), Cn, _ptr(hist),
                                             _stream()), 'seg_joint_hist')
    return hist


def sd_check_shape(shape):
    """Shape rules of mt_surface_distances, checked on the shape alone."""
    shape = cc_check_shape(shape)
    if max(shape) > SD_MAX_AXIS:
        raise ValueError("surface distances: an axis of %s exceeds %d" % (shape, SD_MAX_AXIS))
    return shape


def surface_distances(test, ref, member, spacing=None, connectivity=1, capacity=None, out=None, stats=None, ws=None):
    """test, ref: [D, H, W] uint8 device tensors (contiguous); member: 256 host entries, non-zero = in the mask; spacing: None
    or (z, y, x).  -> (out, stats): out, fp64 device tensor [capacity] (default 2 * D*H*W, always enough; the number of mask
    voxels of both volumes suffices), holds sds(test->ref) then sds(ref->test); stats, fp64 device tensor [6] = (count, max, sum)
    per direction (see mt_surface_distances).  Nothing is synchronised."""
    D, H, W = sd_check_shape(test.shape)
    if tuple(ref.shape) != (D, H, W):
        raise ValueError("surface distances: shape mismatch: %s and %s" % (tuple(test.shape), tuple(ref.shape)))
    if connectivity not in (1, 2, 3):
        raise ValueError("surface distances: connectivity %r (1, 2 or 3)" % (connectivity,))
    sp = None
    if spacing is not None:
        sp = np.ascontiguousarray(np.asarray(spacing, dtype=np.float64).reshape(-1))
        if sp.shape != (3,) or not np.all(np.isfinite(sp)) or not np.all(sp > 0):
            raise ValueError("surface distances: spacing must be three positive numbers (z, y, x), got %r" % (spacing,))
    _require_device(_EVAL, test, ref)
    assert test.dtype == torch.uint8 and ref.dtype == torch.uint8 and test.is_contiguous() and ref.is_contiguous()
    tab = _member_table(member)
    if out is not None:
        capacity = out.numel()
    elif capacity is None:
        capacity = 2 * D * H * W
    capacity = max(1, int(capacity))
    if out is None:
        out = torch.empty(capacity, dtype=torch.float64, device=test.device)
    if stats is None:
        stats = torch.empty(6, dtype=torch.float64, device=test.device)
    lib = _lib.load()
    need = lib.mt_surface_distances_workspace(D, H, W, capacity)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=test.device)
    _require_device(_EVAL, out, stats, ws)
    assert out.dtype == torch.float64 and out.is_contiguous() and stats.dtype == torch.float64 and stats.numel() == 6
    _lib.check(lib.mt_surface_distances(_ptr(test), _ptr(ref), D, H, W, tab.ctypes.data_as(C.c_void_p),
                                        sp.ctypes.data_as(C.c_void_p) if sp is not None else C.c_void_p(0), int(connectivity),
                                        _ptr(out), capacity, _ptr(stats), _ptr(ws), ws.numel() * ws.element_size(), _stream()),
               'surface_distances')
    return out, stats


def surface_distances_workspace(shape, capacity):
    D, H, W = sd_check_shape(shape)
    return int(_lib.load().mt_surface_distances_workspace(D, H, W, max(1, int(capacity))))


def _select_kth(x, ranks, out, ws, dtype, name):
    what = _EVAL if name == 'select_kth' else _AN        # the unit each entry point belongs to
    ranks = [int(r) for r in ranks]
    n = int(x.numel())
    if x.dim() != 1 or n < 1:
        raise ValueError("%s: a non-empty 1-D tensor is expected, got shape %s" % (name, tuple(x.shape)))
    if not 1 <= len(ranks) <= SELECT_MAX_RANKS:
        raise ValueError("%s: %d ranks (1..%d)" % (name, len(ranks), SELECT_MAX_RANKS))
    if min(ranks) < 0 or max(ranks) >= n:
        raise ValueError("%s: ranks %s outside 0..%d" % (name, ranks, n - 1))
    _require_device(what, x)
    assert x.dtype == dtype and x.is_contiguous()
    lib = _lib.load()
    if out is None:
        out = torch.empty(len(ranks), dtype=dtype, device=x.device)
    if ws is None:
        ws = torch.empty(getattr(lib, 'mt_%s_workspace' % name)(len(ranks)), dtype=torch.uint8, device=x.device)
    _require_device(what, out, ws)
    assert out.dtype == dtype and out.is_contiguous() and out.numel() >= len(ranks)
    rk = (C.c_long * len(ranks))(*ranks)
    _lib.check(getattr(lib, 'mt_' + name)(_ptr(x), n, C.cast(rk, C.c_void_p), len(ranks), _ptr(out), _ptr(ws), ws.numel(), _stream()), name)
    return out


def select_kth(x, ranks, out=None, ws=None):
    """x: 1-D contiguous fp64 device tensor; ranks: up to 8 host ints in 0..len(x)-1.  -> fp64 device tensor [len(ranks)]: the
    ranks[r]-th smallest of x, an element of x (radix select on signed doubles, see mt_select_kth).  Nothing is synchronised."""
    return _select_kth(x, ranks, out, ws, torch.float64, 'select_kth')


SD_COUNT_MAX_TOLERANCES = 8


def sd_count_within(sds, n_tr, n_rt, tolerances, out=None):
    """sds: the 1-D contiguous fp64 device tensor surface_distances wrote (8-byte aligned; n_tr + n_rt <= len(sds)); tolerances: 1..8
    host numbers >= 0 (+inf allowed).  -> int64 device tensor [2, T]: how many of sds[:n_tr] (row 0) and of sds[n_tr:n_tr + n_rt]
    (row 1) are <= each tolerance, compared in fp64 (see mt_sd_count_within).  `out` is zeroed by the call.  Nothing is synchronised."""
    tol = np.ascontiguousarray(np.asarray(tolerances, dtype=np.float64).reshape(-1))
    n_tr, n_rt = int(n_tr), int(n_rt)
    if not 1 <= tol.size <= SD_COUNT_MAX_TOLERANCES:
        raise ValueError("sd_count_within: %d tolerances (1..%d)" % (tol.size, SD_COUNT_MAX_TOLERANCES))
    if not np.all(tol >= 0):                                    # False for NaN
        raise ValueError("sd_count_within: tolerances must be numbers >= 0, got %s" % (tol.tolist(),))
    if n_tr < 0 or n_rt < 0 or n_tr + n_rt < 1:
        raise ValueError("sd_count_within: bad segment lengths %d, %d" % (n_tr, n_rt))
    if sds.dim() != 1 or n_tr + n_rt > sds.numel():
        raise ValueError("sd_count_within: %d + %d distances do not fit a tensor of shape %s" % (n_tr, n_rt, tuple(sds.shape)))
    _require_device(_EVAL, sds)
    assert sds.dtype == torch.float64 and sds.is_contiguous()
    T = int(tol.size)
    if out is None:
        out = torch.empty((2, T), dtype=torch.int64, device=sds.device)
    _require_device(_EVAL, out)
    assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() == 2 * T
    _lib.check(_lib.load().mt_sd_count_within(_ptr(sds), n_tr, n_rt, tol.ctypes.data_as(C.c_void_p), T, _ptr(out), _stream()),
               'sd_count_within')
    return out.view(2, T)


FG_MAX_CHANNELS = 16
LABEL_PRESENCE_MIN, LABEL_PRESENCE_MAX = -1, 1022


class FgIndex:
    """State between fg_sample_count and fg_sample: the label map, the unit offsets and the foreground count."""

    def __init__(self, seg, ws, count):
        self.seg, self.ws, self.count, self._n = seg, ws, count, None

    @property
    def n(self):
        """The number of voxels with seg > 0 as a host int (the one read-back, made on first use)."""
        if self._n is None:
            self._n = int(self.count.item())
        return self._n


def fg_sample_count(seg):
    """seg: contiguous float32 device tensor (a label map, any shape).  -> FgIndex: `.count` (int64 device tensor [1]) = number of
    voxels with seg > 0, `.n` the same on the host; it goes to fg_sample.  See mt_fg_sample_count.  Nothing is synchronised here."""
    V = int(seg.numel())
    if V < 1:
        raise ValueError("fg_sample_count: an empty label map")
    if V > FG_MAX_VOXELS:
        raise ValueError("fg_sample_count: %d voxels exceed the int32 index range of the device compaction" % V)
    _require_device(_AN, seg)
    assert seg.dtype == torch.float32 and seg.is_contiguous()
    lib = _lib.load()
    ws = torch.empty(int(lib.mt_fg_sample_workspace(V)), dtype=torch.uint8, device=seg.device)
    count = torch.empty(1, dtype=torch.int64, device=seg.device)
    _lib.check(lib.mt_fg_sample_count(_ptr(seg), V, _ptr(count), _ptr(ws), ws.numel(), _stream()), 'fg_sample_count')
    return FgIndex(seg, ws, count)


def fg_sample(data, seg, stride=10, out=None, offset=0, index=None):
    """data: [C, ...] float32 device tensor (contiguous, 1..16 channels), seg: float32 label map with data.shape[1:] voxels.
    -> (samples, n, nan_counts): samples [C, m] = data[c][seg > 0][::stride] bit for bit, m = ceil(n / stride); n the number of
    foreground voxels (host int: the one read-back); nan_counts, int64 device tensor [C], the NaNs among each channel's samples.
    out: a float32 device tensor [C, capacity]: the samples go to out[:, offset:offset + m], of which `samples` is then a view.
    index: the FgIndex of fg_sample_count(seg) when the caller made that call already (to size `out`).  See mt_fg_sample_gather."""
    stride = int(stride)
    if stride < 1:
        raise ValueError("fg_sample: stride %d < 1" % stride)
    if data.dim() < 2:
        raise ValueError("fg_sample: data [C, ...] is expected, got shape %s" % (tuple(data.shape),))
    Cn = int(data.shape[0])
    V = int(seg.numel())
    if not 1 <= Cn <= FG_MAX_CHANNELS:
        raise ValueError("fg_sample: %d channels (1..%d)" % (Cn, FG_MAX_CHANNELS))
    if V < 1 or int(data.numel()) != Cn * V:
        raise ValueError("fg_sample: data %s and seg %s do not match" % (tuple(data.shape), tuple(seg.shape)))
    _require_device(_AN, data, seg)
    assert data.dtype == torch.float32 and data.is_contiguous()
    if index is None:
        index = fg_sample_count(seg)
    elif index.seg is not seg and (index.seg.data_ptr() != seg.data_ptr() or index.seg.numel() != V):
        raise ValueError("fg_sample: the index belongs to another label map")
    n = index.n
    m = (n + stride - 1) // stride
    offset = int(offset)
    if out is None:
        if offset != 0:
            raise ValueError("fg_sample: an offset needs `out`")
        out = torch.empty((Cn, m), dtype=torch.float32, device=data.device)
    _require_device(_AN, out)
    if out.dim() != 2 or int(out.shape[0]) != Cn or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("fg_sample: out must be a contiguous float32 tensor [%d, capacity]" % Cn)
    cap = int(out.shape[1])
    if offset < 0 or offset + m > cap:
        raise ValueError("fg_sample: %d samples at offset %d do not fit the capacity %d" % (m, offset, cap))
    nan_counts = torch.zeros(Cn, dtype=torch.int64, device=data.device)
    if m > 0:
        lib = _lib.load()
        _lib.check(lib.mt_fg_sample_gather(_ptr(data), Cn, V, _ptr(seg), stride, _ptr(index.ws), index.ws.numel(),
                                           C.c_void_p(out.data_ptr() + 4 * offset), cap, _ptr(nan_counts), _stream()), 'fg_sample_gather')
    return out[:, offset:offset + m], n, nan_counts


def select_kth_f32(x, ranks, out=None, ws=None):
    """x: 1-D contiguous float32 device tensor (any 4-byte aligned view); ranks: up to 8 host ints in 0..len(x)-1.
    -> float32 device tensor [len(ranks)]: the ranks[r]-th smallest of x, an element of x (radix select on signed floats, see
    mt_select_kth_f32).  Nothing is synchronised."""
    return _select_kth(x, ranks, out, ws, torch.float32, 'select_kth_f32')


def label_presence(seg, what='label map'):
    """seg: contiguous float32 device tensor holding integer labels in -1..1022.  -> sorted list of the labels that occur
    (np.unique(seg) as Python ints; one read-back of 33 words).  A non-integral value, a NaN or a label outside the range raises
    ValueError naming `what` (the case).  See mt_label_presence."""
    V = int(seg.numel())
    if V < 1:
        raise ValueError("label_presence: %s is empty" % what)
    _require_device(_AN, seg)
    assert seg.dtype == torch.float32 and seg.is_contiguous()
    buf = torch.empty(33, dtype=torch.int32, device=seg.device)
    _lib.check(_lib.load().mt_label_presence(_ptr(seg), V, _ptr(buf), C.c_void_p(buf.data_ptr() + 4 * 32), _stream()), 'label_presence')
    host = buf.cpu().numpy()
    if host[32] != 0:
        raise ValueError("label_presence: %s holds a value that is not an integer label in %d..%d (a fraction, a NaN or a label "
                         "outside the range); there is no host fallback" % (what, LABEL_PRESENCE_MIN, LABEL_PRESENCE_MAX))
    bits = np.unpackbits(host[:32].view(np.uint8), bitorder='little')
    return [int(b) - 1 for b in np.flatnonzero(bits)]


_CONV = "the label conversion of the dataset conversion runs"
LABEL_CONVERT_DTYPES = _lib.MT_LABEL_DTYPES


def label_convert_round(dtype):
    """The voxels one full round of mt_label_convert's grid-stride loop covers for a numpy dtype name on the current device."""
    return int(_lib.load().mt_label_convert_round(LABEL_CONVERT_DTYPES[np.dtype(dtype).name]))


def label_convert(seg, table, out=None):
    """seg: contiguous device tensor of a label volume in the type its file stores (uint8, int8, int16, uint16, int32, uint32,
    float32 or float64; any element-aligned view).  table: uint16 numpy array of MT_LABEL_SLOTS entries, the output 0..255 of every
    input label 0..1022 or MT_LABEL_UNLISTED (dataset_conversion.Task100_MultiTalent.label_table builds it).
    -> (uint8 device tensor of seg's shape, number of unexpected voxels, the smallest unexpected value as a float or None): a
    voxel above 1e-20 that is no listed label is unexpected and becomes 0 (one read-back of two words).  `out`: a contiguous uint8
    device tensor of as many elements to write into, of any alignment.  See mt_label_convert."""
    _require_device(_CONV, seg)
    name = str(seg.dtype).replace('torch.', '')
    if name not in LABEL_CONVERT_DTYPES:
        raise ValueError("label_convert: a %s volume is not converted on the device (cast int64 / uint64 to float64 first)" % name)
    table = np.ascontiguousarray(table)
    if table.dtype != np.uint16 or table.shape != (_lib.MT_LABEL_SLOTS,):
        raise ValueError("label_convert: the table must be uint16 [%d]" % _lib.MT_LABEL_SLOTS)
    V = int(seg.numel())
    if V < 1:
        raise ValueError("label_convert: the volume is empty")
    assert seg.is_contiguous()
    if out is None:
        out = torch.empty(seg.shape, dtype=torch.uint8, device=seg.device)
    _require_device(_CONV, out)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == V and out.device == seg.device
    report = torch.empty(2, dtype=torch.int64, device=seg.device)
    with torch.cuda.device(seg.device):
        _lib.check(_lib.load().mt_label_convert(_ptr(seg), LABEL_CONVERT_DTYPES[name], V, table.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                _ptr(out), _ptr(report), _stream()), 'label_convert')
    host = report.cpu().numpy()
    count = int(host[0])
    return out, count, (float(host[1:2].view(np.float64)[0]) if count else None)


_LOAD = "the patch gather of the device loader runs"
PAD_MODES = {'constant': _lib.MT_PAD_CONSTANT, 'edge': _lib.MT_PAD_EDGE}


def seg_narrow(seg, flag, out=None):
    """seg: contiguous float32 device tensor of integer labels -> the same labels as int16 (`out`, or a new tensor of seg's shape).
    flag: int32 device tensor of one element that the call sets to 1 when a value is not an integer of int16; the caller zeroes
    and reads it (one flag can watch several calls).  Nothing is synchronised.  See mt_seg_narrow."""
    _require_device(_LOAD, seg, flag)
    assert seg.dtype == torch.float32 and seg.is_contiguous() and flag.dtype == torch.int32 and flag.numel() >= 1
    if out is None:
        out = torch.empty(seg.shape, dtype=torch.int16, device=seg.device)
    assert out.dtype == torch.int16 and out.is_contiguous() and out.numel() == seg.numel() and out.is_cuda
    if seg.numel():
        _lib.check(_lib.load().mt_seg_narrow(_ptr(seg), int(seg.numel()), _ptr(out), _ptr(flag), _stream()), 'seg_narrow')
    return out


def patch_gather(sources, patch_size, pad_mode, data_out=None, seg_out=None, seg_fill=-1.0):
    """sources: per sample (data [C, sx, sy, sz] float32, seg [sx, sy, sz] int16, lb) with contiguous device tensors and the lower
    corner lb of the patch in that source's coordinates (may be negative).  -> (data [B, C, *patch] float32, seg [B, 1, *patch]
    float32): np.pad(crop, pad_mode) of the data (`constant` = 0, or `edge`) and the labels padded with seg_fill, bit for bit.
    One launch per MT_PATCH_MAX_SRC samples; nothing is synchronised.  data_out / seg_out: contiguous float32 device tensors of
    those shapes to write into.  See mt_patch_gather."""
    B, (PD, PH, PW) = len(sources), (int(i) for i in patch_size)
    if B < 1:
        raise ValueError("patch_gather: no samples")
    Cn = int(sources[0][0].shape[0])
    dev = sources[0][0].device
    descs = (_lib.mt_patch_src_t * B)()
    for j, (data, seg, lb) in enumerate(sources):
        _require_device(_LOAD, data, seg)
        if data.dtype != torch.float32 or seg.dtype != torch.int16 or not data.is_contiguous() or not seg.is_contiguous() \
                or data.dim() != 4 or data.shape[0] != Cn or tuple(data.shape[1:]) != tuple(seg.shape) or data.device != dev:
            raise ValueError("patch_gather: sample %d: data float32 [%d, x, y, z] and seg int16 [x, y, z], contiguous, on one device, "
                             "are expected; got %s %s and %s %s" % (j, Cn, data.dtype, tuple(data.shape), seg.dtype, tuple(seg.shape)))
        descs[j].data, descs[j].seg = data.data_ptr(), seg.data_ptr()
        for a in range(3):
            descs[j].shape[a], descs[j].lb[a] = int(seg.shape[a]), int(lb[a])
    if data_out is None:
        data_out = torch.empty((B, Cn, PD, PH, PW), dtype=torch.float32, device=dev)
    if seg_out is None:
        seg_out = torch.empty((B, 1, PD, PH, PW), dtype=torch.float32, device=dev)
    _require_device(_LOAD, data_out, seg_out)
    assert data_out.dtype == seg_out.dtype == torch.float32 and data_out.is_contiguous() and seg_out.is_contiguous()
    assert tuple(data_out.shape) == (B, Cn, PD, PH, PW) and tuple(seg_out.shape) == (B, 1, PD, PH, PW)
    lib, PV = _lib.load(), PD * PH * PW
    with torch.cuda.device(dev):
        for j0 in range(0, B, _lib.MT_PATCH_MAX_SRC):
            n = min(_lib.MT_PATCH_MAX_SRC, B - j0)
            part = C.cast(C.byref(descs, j0 * C.sizeof(_lib.mt_patch_src_t)), C.POINTER(_lib.mt_patch_src_t))
            _lib.check(lib.mt_patch_gather(part, n, Cn, PD, PH, PW, PAD_MODES[pad_mode], float(seg_fill),
                                           C.c_void_p(data_out.data_ptr() + 4 * j0 * Cn * PV), C.c_void_p(seg_out.data_ptr() + 4 * j0 * PV),
                                           _stream()), 'patch_gather')
    return data_out, seg_out


_WRITE = "the gzip encoder of the label-map writer runs"
DEFLATE_CHUNK = 65536
_DEFLATE_HEAD = 1 << 20


def deflate_gzip(payload, prefix=b'', chunk=DEFLATE_CHUNK, stages=None):
    """payload: contiguous uint8 device tensor (any shape, any alignment); prefix: host bytes that precede it in the stream (at
    most MT_DEFLATE_MAX_PREFIX, a file header).  -> bytes: one complete gzip member (mtime 0) of prefix + payload, a pure function
    of the bytes and `chunk` (the size of the independently encoded pieces).  Two launches' worth of device work around one host
    step: the symbol counts come back (316 words), utilities.deflate_host builds the code, the compressed bytes come back — with
    the chunk CRCs in the same copy when they fit 1 MiB, so a label map costs one small and one final read-back.  See
    mt_deflate_tokenize / mt_deflate_emit.  stages: a dict that receives the seconds spent in 'encode' and 'readback'."""
    from .utilities import deflate_host as H
    _require_device(_WRITE, payload)
    if payload.dtype != torch.uint8 or not payload.is_contiguous():
        raise ValueError("deflate_gzip: a contiguous uint8 device tensor is expected, got %s" % payload.dtype)
    body, crc, n = _deflate_call('deflate_gzip', payload, int(payload.numel()), bytes(prefix), int(chunk), None, True, stages)
    return H.gzip_member(body, crc, n)


def _deflate_alloc(nbytes, device):
    """workspace and output of one encoder call (the tests put guard bytes around them here)"""
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _deflate_call(who, payload, npay, prefix, chunk, period, final, stages):
    """One tokenize / emit pair over prefix + the npay bytes at payload's address -> (raw DEFLATE bytes, CRC-32, stream bytes).
    period None: the label-map entry points mt_deflate_tokenize / mt_deflate_emit (distance 1, final)."""
    import time
    from .utilities import deflate_host as H
    npre = len(prefix)
    n = npay + npre
    if n > H.MAX_INPUT:
        raise ValueError("%s: %d bytes; at most %d are encoded as one gzip member" % (who, n, H.MAX_INPUT))
    if period is not None and period not in H.PERIODS:
        raise ValueError("%s: a period of %r bytes; the encoder matches at a distance of 1, 2, 4 or 8" % (who, period))
    lib = _lib.load()
    t0 = time.perf_counter()
    with torch.cuda.device(payload.device):
        ws_bytes, out_bytes = int(lib.mt_deflate_workspace(n, chunk)), int(lib.mt_deflate_bound(n, chunk))
        if not ws_bytes or npre > _lib.MT_DEFLATE_MAX_PREFIX:
            raise ValueError("%s: chunk of %d bytes or prefix of %d bytes outside the encoder's limits" % (who, chunk, npre))
        ws = _deflate_alloc(ws_bytes, payload.device)
        hist = torch.empty(H.LL_SYMBOLS + H.D_SYMBOLS, dtype=torch.int32, device=payload.device)
        pre = (C.c_uint8 * max(npre, 1)).from_buffer_copy(prefix or b'\0')
        if period is None:
            _lib.check(lib.mt_deflate_tokenize(_ptr(payload), npay, pre, npre, chunk, _ptr(ws), ws_bytes, _ptr(hist), _stream()),
                       'deflate_tokenize')
        else:
            _lib.check(lib.mt_deflate_tokenize_period(_ptr(payload), npay, pre, npre, chunk, period, _ptr(ws), ws_bytes, _ptr(hist),
                                                      _stream()), 'deflate_tokenize_period')
        counts = hist.cpu().numpy().view(np.uint32)
        _, _, hval, hbits, table = H.build_tables(counts[:H.LL_SYMBOLS].tolist(), counts[H.LL_SYMBOLS:].tolist(), period or 1)
        header = np.frombuffer(hval.to_bytes(4 * ((hbits + 31) // 32), 'little'), dtype=np.uint32).copy()
        out = _deflate_alloc(out_bytes, payload.device)
        tab_p, hdr_p = table.ctypes.data_as(C.c_void_p), header.ctypes.data_as(C.c_void_p)
        if period is None:
            _lib.check(lib.mt_deflate_emit(_ptr(payload), npay, pre, npre, chunk, tab_p, hdr_p, hbits, _ptr(ws), ws_bytes, _ptr(out),
                                           out_bytes, _stream()), 'deflate_emit')
        else:
            _lib.check(lib.mt_deflate_emit_period(_ptr(payload), npay, pre, npre, chunk, period, 1 if final else 0, tab_p, hdr_p, hbits,
                                                  _ptr(ws), ws_bytes, _ptr(out), out_bytes, _stream()), 'deflate_emit_period')
        if stages is not None:
            torch.cuda.synchronize(payload.device)                  # (only when timed: the emit's device time counts as 'encode')
        t1 = time.perf_counter()
        nchunks = H.chunk_count(n, chunk)
        data = 8 + (4 * nchunks + 7) // 8 * 8                       # out: int64 total, uint32 crc[nchunks], pad, stream
        head = out[:min(out_bytes, data + _DEFLATE_HEAD)].cpu().numpy()
        total = int(head[:8].view(np.int64)[0])
        if not 0 <= total <= out_bytes - data:
            raise RuntimeError("%s: the device reported %d compressed bytes, the bound is %d" % (who, total, out_bytes - data))
        crcs = head[8:8 + 4 * nchunks].view(np.uint32)
        body = head[data:data + total].tobytes()
        if data + total > head.size:                                # more than 1 MiB of compressed bytes: a second copy
            body += out[head.size:data + total].cpu().numpy().tobytes()
    crc = H.crc32_join(crcs, chunk, n - (nchunks - 1) * chunk)
    if stages is not None:
        stages['encode'] = stages.get('encode', 0.0) + (t1 - t0)
        stages['readback'] = stages.get('readback', 0.0) + (time.perf_counter() - t1)
    return body, crc, n


DEFLATE_SEGMENT = 1 << 30


def _payload_bytes(who, payload):
    _require_device(_WRITE, payload)
    if not payload.is_contiguous():
        raise ValueError("%s: a contiguous device tensor is expected" % who)
    return int(payload.numel()) * int(payload.element_size())


def deflate_raw(payload, prefix=b'', chunk=DEFLATE_CHUNK, period=1, final=True, stages=None):
    """payload: any contiguous device tensor, seen as its bytes in memory order (any alignment); prefix: host bytes in front of them.
    -> (body, crc, n): the raw DEFLATE stream of prefix + payload with run-length matches at distance `period` (1, 2, 4 or 8: the
    element size), the CRC-32 and the number of uncompressed bytes.  final=False leaves the stream open and byte-aligned, so that
    the bodies of consecutive calls concatenate into one stream.  See mt_deflate_tokenize_period / mt_deflate_emit_period."""
    npay = _payload_bytes('deflate_raw', payload)
    return _deflate_call('deflate_raw', payload, npay, bytes(prefix), int(chunk), int(period), bool(final), stages)


class deflate_segments(object):
    """The raw DEFLATE stream of prefix + payload (as deflate_raw sees them) for a payload of any size, as a sequence of bodies: the
    stream is cut into segments of `segment_bytes` (a multiple of the chunk in production; the prefix counts into the first), every
    segment is one deflate_raw call with its own code table and only the last is final.  Iterate once; each body can be written
    and dropped before the next is encoded.  Afterwards .crc (joined across the segments), .n and .compressed are set."""

    def __init__(self, payload, prefix=b'', chunk=DEFLATE_CHUNK, period=1, segment_bytes=DEFLATE_SEGMENT, stages=None):
        self.npay, self.prefix = _payload_bytes('deflate_segments', payload), bytes(prefix)
        self.payload, self.chunk, self.period, self.segment, self.stages = payload, int(chunk), int(period), int(segment_bytes), stages
        if not len(self.prefix) < self.segment <= DEFLATE_SEGMENT:
            raise ValueError("deflate_segments: segments of %d bytes (more than the prefix, at most %d)" % (self.segment, DEFLATE_SEGMENT))
        self.n, self.crc, self.compressed = self.npay + len(self.prefix), None, None

    def __iter__(self):
        from .utilities import deflate_host as H
        flat = self.payload.reshape(-1).view(torch.uint8)
        crc, done, compressed, pre = 0, 0, 0, self.prefix
        while True:
            take = min(self.segment - len(pre), self.npay - done)
            last = done + take == self.npay
            body, c, k = _deflate_call('deflate_segments', flat[done:done + take], take, pre, self.chunk, self.period, last, self.stages)
            crc = H.crc32_combine(crc, c, k)
            done, compressed, pre = done + take, compressed + len(body), b''
            if last:
                self.crc, self.compressed = crc, compressed
            yield body
            if last:
                return


_READ = "the INFLATE decoder of the file readers runs"
INFLATE_UNIT_LIMIT = 16 * DEFLATE_CHUNK
INFLATE_CRC_PIECE = 1 << 20
INFLATE_STATUS = ('OK', 'FOREIGN', 'TOO_LONG', 'BAD', 'CORRUPT', 'SIZE')


class InflateForeign(Exception):
    """the stream is well-formed as far as it was looked at, but has no restart points the decoder can work from (too many
    candidates, or a unit that is longer than `unit_limit`): a file of another writer, which the host inflates"""


def _inflate_unit_starts(ws, n, units):
    """the chained units' start positions as a device int32 tensor, from the workspace of mt_inflate_scan"""
    lib = _lib.load()
    cand, ucand, cap = (int(lib.mt_inflate_workspace_part(n, k)) for k in range(3))
    return ws[cand:cand + 4 * cap].view(torch.int32)[ws[ucand:ucand + 4 * units].view(torch.int32).long()]


def inflate_raw(comp, n_out=None, unit_limit=INFLATE_UNIT_LIMIT, final=True, stages=None, want_starts=False):
    """comp: uint8 device tensor (1-D, contiguous, any alignment) holding one raw DEFLATE stream -> (uint8 device tensor of the
    decoded bytes, their CRC-32, info).  n_out: the size the caller expects (a different size is an IOError).  final=False
    accepts a stream that ends on a restart marker with no last block (ops.deflate_raw(..., final=False)).  The stream is decoded
    in parallel from its restart points (mt_inflate_scan / mt_inflate_write); one without them (more than `unit_limit` bytes in
    one unit) raises InflateForeign, a malformed one IOError.  info: {'status', 'units', 'candidates', 'spans', 'bytes'} and, with
    want_starts, 'starts': the units' start positions as a device tensor; stages receives the seconds spent in 'scan', 'write' and 'crc'."""
    import time
    from .utilities import deflate_host as H
    _require_device(_READ, comp)
    if comp.dtype != torch.uint8 or comp.dim() != 1 or not comp.is_contiguous():
        raise ValueError("inflate_raw: a contiguous 1-D uint8 device tensor is expected, got %s %s" % (comp.dtype, tuple(comp.shape)))
    n = int(comp.numel())
    lib = _lib.load()
    t0 = time.perf_counter()
    with torch.cuda.device(comp.device):
        ws_bytes = int(lib.mt_inflate_workspace(n))
        if not ws_bytes:
            raise ValueError("inflate_raw: %d compressed bytes; 1 .. 2^31 - 65 are decoded as one stream" % n)
        ws = _deflate_alloc(ws_bytes, comp.device)
        _lib.check(lib.mt_inflate_scan(_ptr(comp), n, int(unit_limit), 1 if final else 0, -1 if n_out is None else int(n_out),
                                       _ptr(ws), ws_bytes, _stream()), 'inflate_scan')
        head = ws[:24].cpu().numpy()
        status, units = int(head[:4].view(np.int32)[0]), int(head[4:8].view(np.int32)[0])
        total = int(head[8:16].view(np.int64)[0])
        cands, spans = int(head[16:20].view(np.int32)[0]), int(head[20:24].view(np.int32)[0])
        info = {'status': INFLATE_STATUS[status] if 0 <= status < len(INFLATE_STATUS) else status, 'units': units, 'candidates': cands,
                'spans': spans, 'bytes': total}
        t1 = time.perf_counter()
        if stages is not None:
            stages['scan'] = stages.get('scan', 0.0) + (t1 - t0)
        err = None
        if info['status'] in ('FOREIGN', 'TOO_LONG'):
            err = InflateForeign("inflate_raw: %s: %d candidates in %d bytes, unit limit %d" % (info['status'], cands, n, unit_limit))
        elif info['status'] == 'SIZE':
            err = IOError("inflate_raw: the stream holds %d bytes, %d were expected" % (total, n_out))
        elif info['status'] != 'OK':
            err = IOError("inflate_raw: the DEFLATE stream is damaged (%s)" % info['status'])
        if err is not None:
            err.info = info
            raise err
        if want_starts:
            info['starts'] = _inflate_unit_starts(ws, n, units)
        out = _deflate_alloc(total, comp.device)
        _lib.check(lib.mt_inflate_write(_ptr(comp), n, _ptr(ws), ws_bytes, units, spans, _ptr(out), total, _stream()), 'inflate_write')
        if stages is not None:
            torch.cuda.synchronize(comp.device)
            t2 = time.perf_counter()
            stages['write'] = stages.get('write', 0.0) + (t2 - t1)
        pieces = max(1, -(-total // INFLATE_CRC_PIECE))
        crcs = torch.empty(pieces, dtype=torch.int32, device=comp.device)
        _lib.check(lib.mt_inflate_crc(_ptr(out), total, INFLATE_CRC_PIECE, _ptr(crcs), _stream()), 'inflate_crc')
        crc = H.crc32_join(crcs.cpu().numpy().view(np.uint32), INFLATE_CRC_PIECE, total - (pieces - 1) * INFLATE_CRC_PIECE)
        if stages is not None:
            stages['crc'] = stages.get('crc', 0.0) + (time.perf_counter() - t2)
    return out, crc, info


INFLATE_SPEC_CHUNK = 4096                # compressed bytes per searched chunk (measured among 2 .. 64 KiB: DESIGN 6ab)
INFLATE_SPEC_MIN_OUT = 64 << 20          # expected output bytes from which the readers try inflate_stream (measured: DESIGN 6ab)
INFLATE_SPEC_SPAN_CHUNKS = 64            # a unit that consumes more chunks than this found no block starts: the host reads the file
INFLATE_SPEC_UNIT_LIMIT = 1 << 30
_SPEC_SCAN_STEPS = (('search', 1), ('size', 2), ('chain', 4))
_SPEC_WRITE_STEPS = (('symbols', 1), ('windows', 2), ('resolve', 4))


def inflate_stream(comp, n_out=None, chunk=INFLATE_SPEC_CHUNK, unit_limit=INFLATE_SPEC_UNIT_LIMIT, span_limit=None, stages=None,
                   want_starts=False):
    """comp: uint8 device tensor (1-D, contiguous, any alignment) holding one raw DEFLATE stream of ANY writer -> (uint8 device tensor
    of the decoded bytes, their CRC-32, info).  The stream is decoded in parallel from block starts that are searched in it
    (mt_inflate_spec_scan / mt_inflate_spec_write): bit 0 and, per `chunk` compressed bytes (a power of two, 64 .. 2^20), the first
    position at which a non-final dynamic block header is accepted.  n_out: the size the caller expects (another size is an IOError).
    A unit of more than `unit_limit` output bytes or `span_limit` compressed bytes (default: 64 chunks; a stream whose block starts
    are not found, such as a Z_FIXED one) raises InflateForeign, a malformed stream IOError, each with e.info.
    info: {'status', 'units', 'candidates', 'spans', 'bytes', 'shortest_unit', 'max_reach'} and, with want_starts, 'positions' and
    'starts': the bit positions of the candidates and of the units as device tensors.  stages (a dict) makes the call synchronise
    between its passes and receives the seconds of 'search', 'size', 'chain', 'symbols', 'windows', 'resolve' and 'crc'."""
    import time
    from .utilities import deflate_host as H
    _require_device(_READ, comp)
    if comp.dtype != torch.uint8 or comp.dim() != 1 or not comp.is_contiguous():
        raise ValueError("inflate_stream: a contiguous 1-D uint8 device tensor is expected, got %s %s" % (comp.dtype, tuple(comp.shape)))
    n, chunk = int(comp.numel()), int(chunk)
    span_limit = INFLATE_SPEC_SPAN_CHUNKS * chunk if span_limit is None else int(span_limit)
    lib = _lib.load()

    def timed(steps, call):
        """one call for all steps, or one per step with a synchronise behind it when the stages are wanted"""
        if stages is None:
            return call(sum(m for _, m in steps))
        for name, mask in steps:
            t = time.perf_counter()
            call(mask)
            torch.cuda.synchronize(comp.device)
            stages[name] = stages.get(name, 0.0) + (time.perf_counter() - t)

    with torch.cuda.device(comp.device):
        ws_bytes = int(lib.mt_inflate_spec_workspace(n, chunk))
        if not ws_bytes:
            raise ValueError("inflate_stream: %d compressed bytes in chunks of %d; 1 .. 2^31 - 65 bytes and a power of two in "
                             "64 .. 2^20 are decoded" % (n, chunk))
        ws = _deflate_alloc(ws_bytes, comp.device)
        timed(_SPEC_SCAN_STEPS, lambda m: _lib.check(lib.mt_inflate_spec_scan(
            _ptr(comp), n, chunk, int(unit_limit), span_limit, -1 if n_out is None else int(n_out), m, _ptr(ws), ws_bytes, _stream()),
            'inflate_spec_scan'))

        def head():
            h = ws[:32].cpu().numpy()
            i32 = h.view(np.int32)
            status = int(i32[0])
            return {'status': INFLATE_STATUS[status] if 0 <= status < len(INFLATE_STATUS) else status, 'units': int(i32[1]),
                    'bytes': int(h[8:16].view(np.int64)[0]), 'candidates': int(i32[4]), 'spans': int(i32[5]), 'max_reach': int(i32[6]),
                    'shortest_unit': int(h[28:32].view(np.uint32)[0])}

        def fail(info):
            if info['status'] == 'TOO_LONG':
                err = InflateForeign("inflate_stream: a unit of more than %d bytes or %d compressed bytes: %d candidates in %d bytes"
                                     % (unit_limit, span_limit, info['candidates'], n))
            elif info['status'] == 'SIZE':
                err = IOError("inflate_stream: the stream holds %d bytes, %d were expected" % (info['bytes'], n_out))
            else:
                err = IOError("inflate_stream: the DEFLATE stream is damaged (%s)" % info['status'])
            err.info = info
            return err

        info = head()
        if info['status'] != 'OK':
            raise fail(info)
        units, spans, total = info['units'], info['spans'], info['bytes']
        if want_starts:
            cand, ucand, cap = (int(lib.mt_inflate_spec_workspace_part(n, chunk, k)) for k in range(3))
            info['positions'] = ws[cand:cand + 8 * info['candidates']].view(torch.int64).clone()
            info['starts'] = info['positions'][ws[ucand:ucand + 4 * units].view(torch.int32).long()]
        ws2_bytes = int(lib.mt_inflate_spec_write_workspace(units, spans, total))
        ws2 = _deflate_alloc(ws2_bytes, comp.device)
        out = _deflate_alloc(total, comp.device)
        timed(_SPEC_WRITE_STEPS, lambda m: _lib.check(lib.mt_inflate_spec_write(
            _ptr(comp), n, chunk, _ptr(ws), ws_bytes, units, spans, _ptr(ws2), ws2_bytes, _ptr(out), total, m, _stream()),
            'inflate_spec_write'))
        t2 = time.perf_counter()
        pieces = max(1, -(-total // INFLATE_CRC_PIECE))
        crcs = torch.empty(pieces, dtype=torch.int32, device=comp.device)
        _lib.check(lib.mt_inflate_crc(_ptr(out), total, INFLATE_CRC_PIECE, _ptr(crcs), _stream()), 'inflate_crc')
        crc = H.crc32_join(crcs.cpu().numpy().view(np.uint32), INFLATE_CRC_PIECE, total - (pieces - 1) * INFLATE_CRC_PIECE)
        after = head()                                          # a marker that points in front of the stream is found while writing
        if after['status'] != 'OK':
            raise fail(dict(info, status=after['status']))
        if stages is not None:
            stages['crc'] = stages.get('crc', 0.0) + (time.perf_counter() - t2)
    return out, crc, info


_parse_select_env()
_select_env = _select
