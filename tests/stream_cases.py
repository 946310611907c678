"""The streaming norm / activation kernels of csrc/norm.hip, instance by instance (shared module of tests/test_stream_cases_cpu.py and
tests/test_stream_kernels_gpu.py; not a test).

STREAM_INSTANCES names every kernel instance the three choosing launchers (mt_inorm_lrelu_apply, mt_inorm_lrelu_bwd, mt_lrelu_bwd) and
mt_lrelu_bwd_stats can launch, as mt_*_kernel_name prints them.  CASES is the hand-written list of the smallest problems that reach each
of them at the shapes where such kernels go wrong: channel counts that leave lanes idle (G = C / VEC not dividing 256), bases that are
only 4- or 8-byte aligned, channel strides != C, C > 32 with C % 32 != 0, C / VEC > 256, the N * V == 2048 boundary of the one-launch
backward, every block size of it, every tier of the voxel-block size mt_vb(V), NULL operands, accumulating outputs.

A case says which instance it claims (name, own reduce pass, block size); the CPU test asks the library with fake addresses, the GPU
test asks again with the real ones.  An operand is a (width, c0, off) view of a flat buffer: element off + (n * V + v) * width + c0 + c;
dense tensors are (C, 0, 0), `off` moves the base by whole elements, width > C is a channel slice of a wider buffer.  Everything outside
the view (the other columns, the `off` elements in front, GUARD elements behind) holds SENTINEL and must be bit-identical afterwards.

References are the plain formulas in float64 on the exact stored values.  Comparisons:
  * lrelu_bwd (g, gcopy) and the transposes: bit-exact against g or fl32(g * slope), rounded once to the storage type;
  * fp32 apply: elementwise <= 4 u (|y sc| + |sh| + |residual term|), u = 2^-24 (fma, add, multiply by the slope: three roundings);
  * 16-bit apply and 16-bit dy: the rules of test_streaming_kernels_16bit (one ulp of the maximum and < 1 % differing; 2^-7 of the maximum);
  * sums: |got - ref| <= L u sum|terms| with L from the launch geometry (below);
  * fp32 dy: relerr < 5e-5 (test_instance_norm_fwd_bwd) and elementwise <= 8 u k (|dz| + |m1| + |zh m2|) + k (dm1 + |zh| dm2) with
    k = |gamma rstd| and dm1 / dm2 the error of the two means that the sum bound allows.

L: the longest chain of fp32 roundings between a stored operand and the fp32 number the kernel hands to its double-precision sums,
     L = TERM + CHAIN + TAIL.
TERM = 3 covers the term itself (zh = fl(fl(y - mean) * rstd): two; dz = fl(g * slope): one; the product dz * zh is rounded inside the
fma that adds it, which CHAIN counts).  TAIL = 2 covers the conversion of the double sum to float and the `+=` into dgamma / dbeta
(whose previous value is one of the terms).  CHAIN, the fp32 additions, per family (vb = mt_vb(V), nblk = ceil(V / vb)):
  * strided kernels (inorm_bwd_reduce / _apply, channel_sum): a thread adds every 8th voxel of its block, ceil(vb / 8) additions, then one
    thread adds the 8 rows: CHAIN = ceil(vb / 8) + 8;
  * dense fast kernels (inorm_bwd_fast, lrelu_bwd_stats): G = C / VEC, A = (256 / G) G active threads, nvec = V C / VEC vectors per sample,
    per = ceil(ceil(nvec / nblk) / A) A vectors per block: a thread adds per / A terms, then one thread adds the A / G threads of its channel
    group: CHAIN = per / A + A / G;
  * one-launch small kernel: a thread adds ceil(V / NT) terms (NT = block size), a wave butterfly adds six levels, the waves and the samples
    are added in double: CHAIN = ceil(V / NT) + 6;
  * external partials: the kernels add the given fp32 partials in double: CHAIN = 0 and TERM = 0.
Everything after those chains is summed in double (an error of 2^-53 per addition, which the bounds ignore)."""
import functools
import zlib

import torch

F32, BF16, F16 = 0, 1, 2
TDT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
ES = {F32: 4, BF16: 2, F16: 2}
ULP16 = {BF16: 2.0 ** -7, F16: 2.0 ** -10}
U = 2.0 ** -24
PAIRS = ((F32, F32), (F16, BF16), (BF16, BF16))       # (activations, gradients): the pairs the dense kernels are compiled for
ODD_PAIR = (F16, F32)                                 # fp16 y with an fp32 g: strided kernels only
SLOPE = 0.01                                          # passed as a float: the kernels multiply by fl32(0.01)
SLOPE32 = 0.009999999776482582                        # that value
GUARD = 64
SENTINEL = -768.0                                     # exact in fp32, bf16 and fp16
EPS_Z = 1e-4                                          # no pre-activation of a case is closer to 0 than this
NUDGE = 1e-2
FAKE_BASE = 1 << 20                                   # base address of every flat buffer in the CPU queries
MAX_REF_ELEMS = 5 * 10 ** 6
BIG_V = 2048 * 512 + 77
PART_NBLK, PART_PAD, PART_C0 = 5, 6, 4                # external partials: [N][5][C + 6][2], this layer at columns 4 ..


def _vecs(at):
    return (4, 2, 1) if at == F32 else (8, 4, 2)


def apply_fast(vec, at): return 'inorm_apply_fast_kernel<%d, %d>' % (vec, at)
def bwd_fast(vec, at, gt): return 'inorm_bwd_fast_kernel<%d, true, %d, %d>' % (vec, at, gt)
def bwd_small(at, gt): return 'inorm_bwd_small_kernel<%d, %d, %d>' % (4 if gt == F32 else 8, at, gt)
def lbwd_fast(vec, at, gt): return 'lrelu_bwd_fast_kernel<%d, %d, %d>' % (vec, at, gt)
def lstats(at, gt): return 'lrelu_bwd_stats_kernel<4, %d, %d>' % (at, gt)


APPLY_GENERIC, BWD_GENERIC, LBWD_GENERIC = 'inorm_apply_kernel', 'inorm_bwd_apply_kernel', 'lrelu_bwd_kernel'

STREAM_INSTANCES = {
    'apply': [apply_fast(v, at) for at in (F32, F16, BF16) for v in _vecs(at)] + [APPLY_GENERIC],
    'bwd': [bwd_small(at, gt) for at, gt in PAIRS] + [bwd_fast(v, at, gt) for at, gt in PAIRS for v in _vecs(at)] + [BWD_GENERIC],
    'lbwd': [lbwd_fast(v, at, gt) for at, gt in PAIRS for v in _vecs(at)] + [LBWD_GENERIC],
    'lstats': [lstats(at, gt) for at, gt in PAIRS],
}
assert [len(STREAM_INSTANCES[f]) for f in ('apply', 'bwd', 'lbwd', 'lstats')] == [10, 13, 10, 3]


# ---- launch geometry, restated ----------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def mt_vb(V):
    if V >= 2048 * 512:
        return 2048
    return max(32, cdiv(cdiv(V, 512), 32) * 32)


def nb_blocks(V):
    return cdiv(V, mt_vb(V))


TERM, TAIL = 3, 2


def chain_strided(V):
    return cdiv(mt_vb(V), 8) + 8


def chain_fast(V, C, vec):
    G = C // vec
    A = (256 // G) * G
    per = cdiv(cdiv(V * C // vec, nb_blocks(V)), A) * A
    return per // A + A // G


def chain_small(V, block):
    return cdiv(V, block) + 6


class Case(object):
    """fam: 'apply' | 'bwd' | 'lbwd' | 'lstats'.  lay: operand -> (width, c0, off), dense (C, 0, 0) where absent.  opts: see CASES."""

    def __init__(self, fam, tag, N, V, C, pair, name, reduce=None, block=256, lay=None, opts=(), seed=0, tail64=False):
        self.fam, self.N, self.V, self.C, self.name, self.reduce, self.block = fam, N, V, C, name, reduce, block
        self.at, self.gt = pair
        self.lay, self.opts, self.seed, self.tail64 = dict(lay or {}), frozenset(opts), seed, tail64
        self.base_id = '%s-%s-N%dV%dC%d-a%dg%d' % (fam, tag, N, V, C, self.at, self.gt)
        self.id = self.base_id + ('-part' if 'part' in self.opts else '')

    def layout(self, op):
        return self.lay.get(op, (self.C, 0, 0))

    def dtype(self, op):
        return self.at if op in ('y', 'y2', 'res', 'out') else self.gt

    def addr(self, op, base=FAKE_BASE):
        _, c0, off = self.layout(op)
        return base + (off + c0) * ES[self.dtype(op)]

    def operands(self):
        o = self.opts
        if self.fam == 'apply':
            return ['y', 'out'] + (['res'] if 'res' in o else [])
        if self.fam == 'bwd':
            return ['g', 'y']
        return ['g', 'y'] + (['y2'] if 'y2' in o else []) + (['gcopy'] if 'gcopy' in o else [])

    def vec(self):
        """elements per thread of the claimed instance (0: a strided kernel)"""
        return int(self.name.split('<')[1].split(',')[0]) if '<' in self.name else 0

    def chain(self):
        """CHAIN of the kernel that writes the partial sums of this case (module docstring)"""
        if 'small' in self.name:
            return chain_small(self.V, self.block)
        return chain_fast(self.V, self.C, self.vec()) if self.vec() else chain_strided(self.V)

    def ref_elems(self):
        return self.N * self.V * self.C


def _bwd(tag, N, V, C, pair, name, **kw):
    """a fast or strided backward case, with the launcher's own reduction and with external partials"""
    opts = tuple(kw.pop('opts', ()))
    return [Case('bwd', tag, N, V, C, pair, name, reduce=True, opts=opts, **kw),
            Case('bwd', tag, N, V, C, pair, name, reduce=False, opts=opts + ('part',), **kw)]


def _small(tag, N, V, C, pair, block, **kw):
    return [Case('bwd', tag, N, V, C, pair, bwd_small(*pair), reduce=False, block=block, **kw)]


def _strided(C, ops):
    """`g` at columns [3, 3 + C) of a buffer C + 5 wide, `y` in a buffer C + 2 wide; the other operands likewise off their buffers' edge"""
    lay = {'g': (C + 5, 3, 0), 'y': (C + 2, 0, 0), 'res': (C + 5, 3, 0), 'out': (C + 3, 1, 0), 'y2': (C + 1, 1, 0), 'gcopy': (C + 4, 2, 0)}
    return {k: v for k, v in lay.items() if k in ops}


def _off(n, ops):
    return {k: (None, 0, n) for k in ops}


def _cases():
    c = []
    FF = (F32, F32)
    # ---- norm backward, fp32 ------------------------------------------------------------------------------------------------------
    # opts: 'nogb' gamma = beta = NULL; 'nodbias'; 'nodgb' dgamma = dbeta = NULL — each once per form
    c += _bwd('g3', 2, 1100, 12, FF, bwd_fast(4, F32, F32))                                    # G = 3, A = 255
    c += _bwd('g5', 2, 1100, 10, FF, bwd_fast(2, F32, F32), opts=('nogb',))                    # G = 5, A = 255
    c += _bwd('g7', 2, 333, 7, FF, bwd_fast(1, F32, F32), opts=('nodbias',))                   # odd C; G = 7, A = 252
    c += _bwd('off4', 2, 1100, 16, FF, bwd_fast(1, F32, F32), lay=_off(1, 'gy'), opts=('nodgb',))   # base + 4 bytes
    c += _bwd('off8', 2, 1100, 16, FF, bwd_fast(2, F32, F32), lay=_off(2, 'gy'))               # base + 8 bytes
    c += _bwd('g256', 2, 1100, 1024, FF, bwd_fast(4, F32, F32))                                # G = 256: every thread its own group
    c += _bwd('n2049', 1, 2049, 8, FF, bwd_fast(4, F32, F32))                                  # N V = 2049: just not small
    c += _small('b256', 2, 96, 12, FF, 256, opts=('nogb',))
    c += _small('b512', 2, 300, 12, FF, 512, opts=('nodbias',))
    c += _small('b768', 2, 600, 12, FF, 768, opts=('nodgb',))
    c += _small('b1024', 2, 800, 12, FF, 1024)
    c += _small('n3', 3, 333, 20, FF, 512)
    c += _small('n2048', 2, 1024, 4, FF, 1024)                                                 # N V = 2048: still small
    c += _bwd('g257', 2, 77, 1028, FF, BWD_GENERIC, opts=('nogb',))                            # C / 4 = 257 groups: strided kernels
    c += _bwd('cs', 2, 333, 7, FF, BWD_GENERIC, lay=_strided(7, 'gy'), opts=('nodbias',))
    c += _bwd('cs', 2, 333, 33, FF, BWD_GENERIC, lay=_strided(33, 'gy'))                       # two channel rounds, the second of one lane
    c += _bwd('cs', 2, 200, 70, FF, BWD_GENERIC, lay=_strided(70, 'gy'), opts=('nodgb',))      # three rounds
    # ---- the tiers of mt_vb
    c += _bwd('vb64', 2, 20000, 4, FF, bwd_fast(4, F32, F32))                                  # vb 64, 313 blocks, the last of 32 voxels
    c += _bwd('vb64cs', 2, 20000, 4, FF, BWD_GENERIC, lay={'g': (6, 1, 0), 'y': (6, 0, 0)})
    c += _bwd('vb2048', 1, BIG_V, 4, FF, bwd_fast(4, F32, F32), tail64=True)                   # vb 2048, 513 blocks, the last of 77 voxels
    c += _bwd('vb2048cs', 1, BIG_V, 4, FF, BWD_GENERIC, lay={'g': (6, 1, 0), 'y': (6, 0, 0)}, tail64=True)
    # ---- norm backward, 16-bit
    for p in PAIRS[1:]:
        c += _bwd('v8', 2, 1100, 24, p, bwd_fast(8, *p))
        c += _bwd('v4', 2, 1100, 12, p, bwd_fast(4, *p), opts=('nogb',))
        c += _bwd('v2', 2, 1100, 10, p, bwd_fast(2, *p), opts=('nodbias',))
        c += _bwd('off4', 2, 1100, 16, p, bwd_fast(2, *p), lay=_off(2, 'gy'), opts=('nodgb',))    # base + 4 bytes
        c += _bwd('c7', 2, 333, 7, p, BWD_GENERIC)                                             # no 16-bit vector of one element
        c += _small('b256', 2, 96, 24, p, 256)
        c += _small('b512', 2, 300, 24, p, 512, opts=('nogb',))
        c += _small('b768', 2, 600, 24, p, 768, opts=('nodbias',))
        c += _small('b1024', 2, 800, 24, p, 1024, opts=('nodgb',))
    c += _bwd('odd', 2, 333, 24, ODD_PAIR, BWD_GENERIC)                                        # a pair the dense kernels are not compiled for
    # ---- apply.  opts: 'res' with a residual; 'noscale' scale = shift = NULL; 'norscale' rscale = rshift = NULL -------------------
    A = lambda tag, N, V, C, at, name, **kw: [Case('apply', tag, N, V, C, (at, at), name, **kw)]
    c += A('g3', 2, 1100, 12, F32, apply_fast(4, F32), opts=('res',))
    c += A('g5', 2, 1100, 10, F32, apply_fast(2, F32))
    c += A('g7', 2, 333, 7, F32, apply_fast(1, F32), opts=('res', 'norscale'))
    c += A('off4', 2, 1100, 16, F32, apply_fast(1, F32), lay=_off(1, ('y', 'out')), opts=('noscale',))
    c += A('off8', 2, 1100, 16, F32, apply_fast(2, F32), lay=_off(2, ('y', 'out', 'res')), opts=('res',))
    c += A('resoff', 2, 1100, 16, F32, apply_fast(1, F32), lay=_off(1, ('res',)), opts=('res',))     # only the residual is misaligned
    c += A('g256', 2, 300, 1024, F32, apply_fast(4, F32), opts=('res',))
    c += A('g257', 2, 77, 1028, F32, APPLY_GENERIC, opts=('res',))
    c += A('cs', 2, 333, 7, F32, APPLY_GENERIC, lay=_strided(7, ('y', 'out', 'res')), opts=('res',))
    c += A('cs', 2, 333, 33, F32, APPLY_GENERIC, lay=_strided(33, ('y', 'out')), opts=('noscale',))
    c += A('ocs', 2, 333, 12, F32, APPLY_GENERIC, lay=_strided(12, ('out',)))                        # only the destination is a slice
    c += A('vb64', 2, 20000, 4, F32, apply_fast(4, F32), opts=('res',))
    c += A('vb64cs', 2, 20000, 4, F32, APPLY_GENERIC, lay={'y': (6, 0, 0), 'out': (6, 2, 0)})
    for at in (F16, BF16):
        c += A('v8', 2, 1100, 24, at, apply_fast(8, at), opts=('res',))
        c += A('v4', 2, 1100, 12, at, apply_fast(4, at), opts=('res', 'norscale'))
        c += A('v2', 2, 1100, 10, at, apply_fast(2, at), opts=('noscale',))
        c += A('off4', 2, 1100, 16, at, apply_fast(2, at), lay=_off(2, ('y', 'out', 'res')), opts=('res',))
        c += A('c7', 2, 333, 7, at, APPLY_GENERIC, opts=('res',))
        c += A('cs', 2, 333, 33, at, APPLY_GENERIC, lay=_strided(33, ('y', 'out', 'res')), opts=('res',))
    # ---- lrelu_bwd.  opts: 'y2' second term; 'gcopy' ----------------------------------------------------------------------------------
    Lb = lambda tag, N, V, C, p, name, **kw: [Case('lbwd', tag, N, V, C, p, name, **kw)]
    c += Lb('g3', 2, 1100, 12, FF, lbwd_fast(4, F32, F32), opts=('y2', 'gcopy'))
    c += Lb('g5', 2, 1100, 10, FF, lbwd_fast(2, F32, F32))
    c += Lb('g7', 2, 333, 7, FF, lbwd_fast(1, F32, F32), opts=('y2',))
    c += Lb('off4', 2, 1100, 16, FF, lbwd_fast(1, F32, F32), lay=_off(1, ('gcopy',)), opts=('gcopy',))   # only the copy is misaligned
    c += Lb('off8', 2, 1100, 16, FF, lbwd_fast(2, F32, F32), lay=_off(2, ('g', 'y', 'y2')), opts=('y2',))
    c += Lb('g256', 2, 300, 1024, FF, lbwd_fast(4, F32, F32), opts=('y2', 'gcopy'))
    c += Lb('g257', 2, 77, 1028, FF, LBWD_GENERIC, opts=('gcopy',))
    c += Lb('cs', 2, 333, 7, FF, LBWD_GENERIC, lay=_strided(7, ('g', 'y', 'y2', 'gcopy')), opts=('y2', 'gcopy'))
    c += Lb('cs', 2, 333, 33, FF, LBWD_GENERIC, lay=_strided(33, ('g', 'y')))
    c += Lb('cpcs', 2, 333, 12, FF, LBWD_GENERIC, lay=_strided(12, ('gcopy',)), opts=('gcopy',))         # dense but for the strided copy
    c += Lb('vb64', 2, 20000, 4, FF, lbwd_fast(4, F32, F32), opts=('gcopy',))
    c += Lb('vb64cs', 2, 20000, 4, FF, LBWD_GENERIC, lay={'g': (6, 1, 0), 'y': (6, 0, 0)})
    for p in PAIRS[1:]:
        c += Lb('v8', 2, 1100, 24, p, lbwd_fast(8, *p), opts=('y2', 'gcopy'))
        c += Lb('v4', 2, 1100, 12, p, lbwd_fast(4, *p), opts=('gcopy',))
        c += Lb('v2', 2, 1100, 10, p, lbwd_fast(2, *p), opts=('y2',))
        c += Lb('off4', 2, 1100, 16, p, lbwd_fast(2, *p), lay=_off(2, ('g', 'y', 'gcopy')), opts=('gcopy',))
        c += Lb('c7', 2, 333, 7, p, LBWD_GENERIC, opts=('y2', 'gcopy'))
    c += Lb('odd', 2, 333, 24, ODD_PAIR, LBWD_GENERIC, opts=('y2', 'gcopy'))
    # ---- lrelu_bwd_stats (dense, 16-byte aligned, C % 4 == 0 only) ---------------------------------------------------------------
    for p in PAIRS:
        c += [Case('lstats', 'g1', 2, 1100, 4, p, lstats(*p), opts=('y2', 'gcopy')),
              Case('lstats', 'g3', 2, 1100, 12, p, lstats(*p), opts=('gcopy',)),
              Case('lstats', 'g256', 2, 300, 1024, p, lstats(*p), opts=('y2',))]
    for x in c:                                            # None in a layout = the channel count
        x.lay = {k: (x.C if w is None else w, c0, off) for k, (w, c0, off) in x.lay.items()}
    assert len({x.id for x in c}) == len(c)
    return c


CASES = _cases()
# mt_lrelu_bwd_stats_blocks returns 0 for these and the launch refuses them.  (Its third condition, V C 4 % 16 != 0, cannot be met by a
# shape that passes C % 4 == 0.)
LSTATS_REFUSED = [(1100, 6), (77, 1028), (1100, 1026)]


def by_family(fam):
    return [x for x in CASES if x.fam == fam]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def rnd(x, dt):
    """x rounded once to storage type dt, as float64"""
    return x.to(torch.float32).to(TDT[dt]).to(torch.float64)


def lrelu(t, s):
    return torch.where(t > 0, t, t * s)


def bc(t):
    return t[:, None, :].double()


def place(vals, case, op, inside=None):
    """the flat buffer of operand `op` with `vals` [N, V, C] (float64, representable) in its view, SENTINEL elsewhere; `inside` replaces
    the values (an output that starts as NaN).  Returns (flat tensor of the storage type, bool mask of the view)."""
    width, c0, off = case.layout(op)
    N, V, C = case.N, case.V, case.C
    flat = torch.full((off + N * V * width + GUARD,), SENTINEL, dtype=torch.float32)
    mask = torch.zeros(flat.shape, dtype=torch.bool)
    body = flat[off:off + N * V * width].view(N, V, width)
    body[:, :, c0:c0 + C] = float(inside) if inside is not None else vals.to(torch.float32)
    mask[off:off + N * V * width].view(N, V, width)[:, :, c0:c0 + C] = True
    return flat.to(TDT[case.dtype(op)]), mask


def view(flat, case, op):
    """[N, V, C] float64 view of an operand's flat buffer (a copy)"""
    width, c0, off = case.layout(op)
    return flat[off:off + case.N * case.V * width].view(case.N, case.V, width)[:, :, c0:c0 + case.C].to(torch.float64)


def untouched(before, after, mask):
    """everything outside the view is bit-identical"""
    iv = {4: torch.int32, 2: torch.int16}[before.element_size()]
    return torch.equal(before.view(iv)[~mask], after.view(iv)[~mask])


def _gen(case):
    return torch.Generator().manual_seed((zlib.crc32(case.base_id.encode()) + case.seed) & 0x7fffffff)


def _nudge(y, dt, z_of, dzdy):
    """move y by +-NUDGE (away from the sign change) where |z_of(y)| < EPS_Z, re-round, and require that none remains"""
    z = z_of(y)
    bad = z.abs() < EPS_Z
    if bool(bad.any()):
        step = torch.where((z >= 0) == (dzdy >= 0), NUDGE, -NUDGE)
        y = rnd(torch.where(bad, y + step, y), dt)
        z = z_of(y)
    assert not bool((z.abs() < EPS_Z).any()), "a pre-activation within %g of zero remains: choose another seed" % EPS_Z
    return y, int(bad.sum())


@functools.lru_cache(maxsize=4)
def _draw(base_id):
    case = next(x for x in CASES if x.base_id == base_id)
    g = _gen(case)
    N, V, C = case.N, case.V, case.C
    o = case.opts
    d = {'nudged': 0}
    y = rnd(torch.randn((N, V, C), generator=g) + 0.3, case.at)
    if case.fam == 'bwd':
        mean = y.mean(1).float()
        rstd = (1.0 / torch.sqrt(y.var(1, unbiased=False) + 1e-5)).float()
        gamma = None if 'nogb' in o else (torch.rand(C, generator=g) + 0.5)
        beta = None if 'nogb' in o else (torch.randn(C, generator=g) * 0.3)
        ga = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
        be = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)
        z_of = lambda yy: (yy - bc(mean)) * bc(rstd) * ga + be
        y, d['nudged'] = _nudge(y, case.at, z_of, (bc(rstd) * ga).expand(N, V, C))
        gg = torch.randn((N, V, C), generator=g)
        if case.tail64:
            gg[:, -77:] *= 64.0
        d.update(y=y, g=rnd(gg, case.gt), mean=mean, rstd=rstd, gamma=gamma, beta=beta, ga=ga, be=be,
                 dgamma0=torch.randn(C, generator=g) + 2.0, dbeta0=torch.randn(C, generator=g) - 2.0)
        return d
    # apply | lbwd | lstats: t = y sc + sh (+ lrelu(y2 sc2 + sh2, slope2))
    second = 'res' if case.fam == 'apply' else 'y2'
    has2 = second in o
    sc = None if 'noscale' in o else (torch.rand((N, C), generator=g) + 0.5)
    sh = None if 'noscale' in o else torch.randn((N, C), generator=g)
    sc2 = None if ('norscale' in o or not has2) else (torch.rand((N, C), generator=g) + 0.5)
    sh2 = None if ('norscale' in o or not has2) else torch.randn((N, C), generator=g)
    one, zero = torch.ones((N, C)), torch.zeros((N, C))
    s1, h1 = bc(sc if sc is not None else one), bc(sh if sh is not None else zero)
    s2, h2 = bc(sc2 if sc2 is not None else one), bc(sh2 if sh2 is not None else zero)
    term2 = torch.zeros((N, V, C), dtype=torch.float64)
    y2 = None
    if has2:
        y2 = rnd(torch.randn((N, V, C), generator=g), case.at)
        y2, n2 = _nudge(y2, case.at, lambda v: v * s2 + h2, s2.expand(N, V, C))          # the inner LeakyReLU (slope2) has a sign change too
        d['nudged'] += n2
        term2 = lrelu(y2 * s2 + h2, SLOPE32)
    y, n1 = _nudge(y, case.at, lambda v: v * s1 + h1 + term2, s1.expand(N, V, C))
    d['nudged'] += n1
    d.update(y=y, y2=y2, sc=sc, sh=sh, sc2=sc2, sh2=sh2, s1=s1, h1=h1, term2=term2, t=y * s1 + h1 + term2)
    if case.fam != 'apply':
        d['g'] = rnd(torch.randn((N, V, C), generator=g), case.gt)
    if case.fam == 'lstats':
        d['mean'] = y.mean(1).float()
        d['rstd'] = (1.0 / torch.sqrt(y.var(1, unbiased=False) + 1e-5)).float()
    return d


def draw(case):
    """the drawn, nudged inputs of a case (float64 values that are exactly representable in their storage types; shared by the variants
    of one problem and cached)"""
    return _draw(case.base_id)


# ---- references and comparisons (CPU, float64) ------------------------------------------------------------------------------------
def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def close_16bit(out, ref, dt):
    """the rule of test_streaming_kernels_16bit for a materialised 16-bit tensor against its float reference (not yet rounded): at most
    one ulp of the maximum apart, and fewer than 1 % of the elements differ from the rounded reference"""
    r = ref.to(torch.float32).to(TDT[dt]).to(torch.float32)
    d = (out.float() - r).abs().max()
    assert float(d) <= float(ref.abs().max()) * ULP16[dt], float(d)         # at most one ulp (fma vs mul+add before the rounding)
    assert float((out.float() != r).float().mean()) < 0.01


def sum_close(got, ref, abs_terms, L, what=''):
    """|got - ref| <= L u sum|terms|, elementwise over the channels"""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bound = L * U * abs_terms.double()
    assert torch.isfinite(got).all(), what
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: %.3g of the bound (L = %d)" % (what, worst, L))
    assert bool((err <= bound).all()), "%s: |got - ref| is %.3g of its bound L u sum|terms| (L = %d)" % (what, worst, L)
    return worst


def bwd_partials(case, d):
    """external first-pass partials [N][PART_NBLK][C + PART_PAD][2] in fp32 from float64 sums over PART_NBLK runs of voxels; the columns
    outside [PART_C0, PART_C0 + C) hold NaN"""
    assert PART_NBLK != nb_blocks(case.V)
    dz, zh = bwd_dz(case, d)
    part = torch.full((case.N, PART_NBLK, case.C + PART_PAD, 2), float('nan'), dtype=torch.float32)
    edges = [case.V * i // PART_NBLK for i in range(PART_NBLK + 1)]
    for i in range(PART_NBLK):
        sl = slice(edges[i], edges[i + 1])
        part[:, i, PART_C0:PART_C0 + case.C, 0] = dz[:, sl].sum(1).float()
        part[:, i, PART_C0:PART_C0 + case.C, 1] = (dz[:, sl] * zh[:, sl]).sum(1).float()
    return part


def bwd_dz(case, d):
    zh = (d['y'] - bc(d['mean'])) * bc(d['rstd'])
    z = zh * d['ga'] + d['be']
    return torch.where(z > 0, d['g'], d['g'] * SLOPE32), zh


def check_bwd(case, d, part, dy, dgamma, dbeta, dbias):
    """dy [N, V, C] as stored (any float dtype), dgamma / dbeta / dbias fp32 [C] or None as passed; part: the external partials or None"""
    N, V, C = case.N, case.V, case.C
    dz, zh = bwd_dz(case, d)
    if part is not None:
        p = part[:, :, PART_C0:PART_C0 + C].double()
        A, B = p[..., 0].sum(1), p[..., 1].sum(1)                  # the kernels' means come from the given partials
        SA, SB = p[..., 0].abs().sum(1), p[..., 1].abs().sum(1)
        L = TAIL
    else:
        A, B = dz.sum(1), (dz * zh).sum(1)
        SA, SB = dz.abs().sum(1), (dz * zh).abs().sum(1)
        L = TERM + case.chain() + TAIL
    k = d['ga'] * bc(d['rstd'])
    m1, m2 = bc(A / V), bc(B / V)
    ref = k * (dz - m1 - zh * m2)
    got = dy.double()
    assert torch.isfinite(got).all()
    if case.gt == F32:
        assert relerr(got, ref) < 5e-5, relerr(got, ref)
        dm1, dm2 = bc(L * U * SA / V), bc(L * U * SB / V)
        bound = 8 * U * k.abs() * (dz.abs() + m1.abs() + (zh * m2).abs()) + k.abs() * (dm1 + zh.abs() * dm2)
        bad = (got - ref).abs() > bound
        print("dy: relerr %.3g, elementwise %.3g of the bound" % (relerr(got, ref), float(((got - ref).abs() / bound).max())))
        assert not bool(bad.any()), "%d elements of dy beyond the elementwise bound, worst %.3g of it, first at %s" % (
            int(bad.sum()), float(((got - ref).abs() / bound).max()), bad.nonzero()[0].tolist())
    else:
        err = (got - ref).abs().max() / ref.abs().max()
        print("dy: %.3g of max |dy| (bound 2^-7)" % float(err))
        assert float(err) < 2 ** -7, float(err)
    if dgamma is not None:
        sum_close(dgamma, d['dgamma0'].double() + B.sum(0), d['dgamma0'].double().abs() + SB.sum(0), L, 'dgamma')
        sum_close(dbeta, d['dbeta0'].double() + A.sum(0), d['dbeta0'].double().abs() + SA.sum(0), L, 'dbeta')
    if dbias is not None:                                          # the sum of what was stored
        sum_close(dbias, got.sum((0, 1)), got.abs().sum((0, 1)), case.chain() + TAIL, 'dbias')


def apply_ref(case, d):
    """(reference float64, sum of the magnitudes the fp32 bound is made of)"""
    t = d['t']
    return lrelu(t, SLOPE32), (d['y'] * d['s1']).abs() + d['h1'].abs() + d['term2'].abs()


def check_apply(case, d, out):
    ref, mag = apply_ref(case, d)
    assert torch.isfinite(out.double()).all()
    if case.at == F32:
        bad = (out.double() - ref).abs() > 4 * U * mag
        print("apply: %.3g of the bound" % float(((out.double() - ref).abs() / (4 * U * mag)).max()))
        assert not bool(bad.any()), "%d elements beyond 4 u (|y sc| + |sh| + |res|), worst %.3g of it" % (
            int(bad.sum()), float(((out.double() - ref).abs() / (4 * U * mag)).max()))
    else:
        close_16bit(out, ref, case.at)


def lbwd_ref(case, d):
    """bit-exact: g where t > 0, else fl32(g * slope) rounded once to the storage type; as a tensor of the storage type"""
    g32 = d['g'].to(torch.float32)
    return torch.where(d['t'] > 0, g32, g32 * SLOPE32).to(TDT[case.gt])


def check_lstats(case, d, gout, part):
    """part [N, nblk, C, 2] fp32: the block partials of (sum g', sum g' zhat) over the stored g'"""
    gp = gout.double()
    zh = (d['y'] - bc(d['mean'])) * bc(d['rstd'])
    L = 2 + chain_fast(case.V, case.C, 4)                          # zh: two roundings; g' is a stored value; the partials stay fp32
    s = part.double().sum(1)
    assert part.shape[1] == nb_blocks(case.V)
    sum_close(s[..., 0], gp.sum(1), gp.abs().sum(1), L, 'stats A')
    sum_close(s[..., 1], (gp * zh).sum(1), (gp * zh).abs().sum(1), L, 'stats B')


# ---- the kernels without a choice: finalize, channel_sum, transposes ---------------------------------------------------------------
FINALIZE_NSB = (1, 255, 257, 600)
FINALIZE_C = 33
FINALIZE_CONST = (1000.1, 5)                   # channel 5 of every sample is this constant: its fp32 partials give var <= 0
TRANSPOSE_CASES = [(C, V) for C in (5, 33, 64) for V in (31, 32, 1000)]        # N = 2, destination / source stride C + 3
# (tag, N, V, C, storage type, (width, c0), accumulate)
CHANNEL_SUM_CASES = [('dense', 2, 1100, 12, F32, (12, 0), 0), ('acc', 2, 1100, 12, F32, (12, 0), 1), ('cs33', 2, 333, 33, F32, (38, 3), 1),
                     ('vb64', 2, 20000, 4, F32, (6, 1), 0), ('c70', 1, 77, 70, BF16, (70, 0), 0), ('cs7', 2, 333, 7, F16, (9, 2), 1)]


def finalize_ref(part, count, gamma, beta, eps):
    """float64 arithmetic on the same fp32 partials [N][nsb][C][2], with the clamp; gamma / beta float or None"""
    s = part.double().sum(1)
    m = s[..., 0] / count
    var = (s[..., 1] / count - m * m).clamp_min(0.0)
    rs = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    g = gamma.double() if gamma is not None else torch.ones(part.shape[2], dtype=torch.float64)
    b = beta.double() if beta is not None else torch.zeros(part.shape[2], dtype=torch.float64)
    return m, rs, g * rs, b - m * g * rs, s[..., 1] / count - m * m


# ---- the library's answer -----------------------------------------------------------------------------------------------------------
def ask(ops, case, addr=None):
    """(name, own reduce pass, block size) the library gives for a case; addr(op) -> address of an operand (default: the fake ones).
    The reduce flag and the block size are None for the families that have neither."""
    addr = addr or case.addr
    N, V, C = case.N, case.V, case.C
    w = lambda op: case.layout(op)[0]
    a = lambda op: addr(op) if op in case.operands() else 0
    if case.fam == 'apply':
        return ops.inorm_lrelu_apply_kernel_name(a('y'), w('y'), a('res'), w('res') if a('res') else 0, a('out'), w('out'), N, V, C, case.at), None, None
    if case.fam == 'bwd':
        part = dict(part=64, part_nblk=PART_NBLK, part_cs=C + PART_PAD, part_c0=PART_C0) if 'part' in case.opts else {}
        return ops.inorm_lrelu_bwd_kernel_name(a('g'), w('g'), a('y'), w('y'), N, V, C, case.gt, case.at, **part)
    if case.fam == 'lbwd':
        return ops.lrelu_bwd_kernel_name(a('g'), w('g'), a('y'), w('y'), a('y2'), w('y2') if a('y2') else 0, a('gcopy'), w('gcopy') if a('gcopy') else 0,
                                         N, V, C, case.gt, case.at), None, None
    return ops.lrelu_bwd_stats_kernel_name(a('g'), a('y'), a('y2'), a('gcopy'), N, V, C, case.gt, case.at), None, None


def claim(case):
    return (case.name, case.reduce, case.block) if case.fam == 'bwd' else (case.name, None, None)
