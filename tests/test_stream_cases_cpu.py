"""The cases of tests/test_stream_kernels_gpu.py are what they claim and are complete (no GPU): with the built library and fake
addresses every case resolves to the kernel instance, reduce flag and block size it names; the names the cases cover are exactly
STREAM_INSTANCES, and those are exactly the names the library gives over a fixed product of the axes its dispatch reads."""
import itertools

import pytest

import stream_cases as SC


@pytest.fixture(scope='module')
def ops():
    from multitalent_amd import ops
    return ops


def test_every_case_is_the_instance_it_claims(ops):
    for case in SC.CASES:
        assert SC.ask(ops, case) == SC.claim(case), case.id
        for op in case.operands():                    # a view keeps the alignment of its elements and stays inside its row
            width, c0, off = case.layout(op)
            assert c0 + case.C <= width and off >= 0 and case.addr(op) % SC.ES[case.dtype(op)] == 0, (case.id, op)


@pytest.mark.parametrize('fam', sorted(SC.STREAM_INSTANCES))
def test_the_cases_cover_every_instance(fam):
    covered = {c.name for c in SC.by_family(fam)}
    want = set(SC.STREAM_INSTANCES[fam])
    assert covered == want, (sorted(want - covered), sorted(covered - want))


def test_backward_variants_are_spread_over_the_forms():
    """every fast and strided backward case runs with its own reduction and with external partials; each NULL variant once per form"""
    bwd = SC.by_family('bwd')
    for c in bwd:
        if 'small' in c.name:
            assert c.reduce is False and 'part' not in c.opts
        else:
            twin = [x for x in bwd if x.base_id == c.base_id]
            assert sorted('part' in x.opts for x in twin) == [False, True] and all(x.reduce == ('part' not in x.opts) for x in twin), c.id
    for form in ('small', 'fast', 'apply'):
        for opt in ('nogb', 'nodbias', 'nodgb'):
            assert any(('inorm_bwd_' + form) in c.name and opt in c.opts for c in bwd), (form, opt)
    assert {c.block for c in bwd if 'small' in c.name and c.gt == SC.F32} == {256, 512, 768, 1024}
    assert {c.block for c in bwd if 'small' in c.name and c.gt == SC.BF16} == {256, 512, 768, 1024}


CENSUS_C = list(range(1, 41)) + [60, 120, 256, 257, 320, 1024, 1028]
CENSUS_V = [77, 96, 256, 257, 512, 513, 768, 769, 1023, 1024, 1025, 1100, 2047, 2048, 2049, 20000]
CENSUS_ALIGN = [2, 4, 8, 16]                       # bytes by which the base is off a 4 KiB boundary
CENSUS_PAIRS = list(SC.PAIRS) + [SC.ODD_PAIR]


def test_name_census_is_closed_and_complete(ops):
    """Over the product of channel counts, voxel counts around every threshold, base alignments, storage pairs, dense / strided operands,
    optional operands and external partials: the set of names per family is STREAM_INSTANCES, no more and no less."""
    seen = {f: set() for f in SC.STREAM_INSTANCES}
    small_blocks = set()
    for C, V, N, al, (at, gt), strided in itertools.product(CENSUS_C, CENSUS_V, (1, 2), CENSUS_ALIGN, CENSUS_PAIRS, (False, True)):
        if al % SC.ES[at] or al % SC.ES[gt]:
            continue                                 # not an address of such elements
        a = SC.FAKE_BASE + al
        cs = C + 2 if strided else C
        for opt in (0, a):
            seen['apply'].add(ops.inorm_lrelu_apply_kernel_name(a, cs, opt, cs, a, cs, N, V, C, at))
            seen['lbwd'].add(ops.lrelu_bwd_kernel_name(a, cs, a, cs, opt, cs, opt, cs, N, V, C, gt, at))
            name, red, blk = ops.inorm_lrelu_bwd_kernel_name(a, cs, a, cs, N, V, C, gt, at, part=opt, part_nblk=3, part_cs=C, part_c0=0)
            seen['bwd'].add(name)
            assert red == (opt == 0 and 'small' not in name), (name, red, C, V, N)
            if 'small' in name:
                small_blocks.add(blk)
                assert opt == 0 and N * V <= 2048 and blk == (1024 if V > 768 else 768 if V > 512 else 512 if V > 256 else 256)
            else:
                assert blk == 256
        if not strided and al == 16 and (at, gt) in SC.PAIRS and C % 4 == 0 and C <= 1024:
            seen['lstats'].add(ops.lrelu_bwd_stats_kernel_name(a, a, 0, 0, N, V, C, gt, at))
    for fam, names in seen.items():
        want = set(SC.STREAM_INSTANCES[fam])
        assert names == want, (fam, sorted(want - names), sorted(names - want))
    assert small_blocks == {256, 512, 768, 1024}


def test_stats_refuses_what_its_block_query_refuses(ops):
    from multitalent_amd import _lib
    lib = _lib.load()
    for V, C in SC.LSTATS_REFUSED:
        assert lib.mt_lrelu_bwd_stats_blocks(V, C) == 0
        with pytest.raises(RuntimeError, match=r'rc=-1\).*unsupported shape'):         # MT_EINVAL
            ops.lrelu_bwd_stats_kernel_name(SC.FAKE_BASE, SC.FAKE_BASE, 0, 0, 2, V, C, SC.F32, SC.F32)
        # the launch itself refuses before it touches a device (the addresses are never read)
        rc = lib.mt_lrelu_bwd_stats(SC.FAKE_BASE, SC.FAKE_BASE, None, None, 0.01, None, None, None, 1.0, None, 64, 64, 64, 2, V, C, SC.F32, SC.F32, None)
        assert rc == -1
    with pytest.raises(RuntimeError, match='16-byte aligned'):
        ops.lrelu_bwd_stats_kernel_name(SC.FAKE_BASE + 8, SC.FAKE_BASE, 0, 0, 2, 1100, 12, SC.F32, SC.F32)
    with pytest.raises(RuntimeError, match='storage types'):
        ops.lrelu_bwd_stats_kernel_name(SC.FAKE_BASE, SC.FAKE_BASE, 0, 0, 2, 1100, 12, SC.F32, SC.F16)


def test_geometry_restatement_matches_the_library():
    """mt_vb / nb_blocks as restated for the chain lengths: the library's block count at every V of the cases and at the tier edges"""
    from multitalent_amd import _lib
    lib = _lib.load()
    vs = {c.V for c in SC.CASES} | {1, 31, 32, 33, 16384, 16385, 32768, 32769, 2048 * 512 - 1, 2048 * 512, SC.BIG_V}
    for V in sorted(vs):
        assert lib.mt_lrelu_bwd_stats_blocks(V, 4) == SC.nb_blocks(V), V
        assert lib.mt_inorm_bwd_workspace(2, V, 4) == (2 * SC.nb_blocks(V) * 4 * 3 + 2 * 4 * 2) * 4
    assert SC.mt_vb(20000) == 64 and SC.nb_blocks(20000) == 313 and 20000 % 64 == 32
    assert SC.mt_vb(SC.BIG_V) == 2048 and SC.nb_blocks(SC.BIG_V) == 513
    for c in SC.by_family('bwd'):
        assert SC.nb_blocks(c.V) != SC.PART_NBLK


def test_references_are_small_and_no_preactivation_is_near_zero():
    """each case's float64 reference has at most MAX_REF_ELEMS elements per tensor; drawing a case nudges every element whose pre-activation
    is within EPS_Z of zero and asserts that none remains (the seed of a case is fixed: what passes here is what the GPU test draws)"""
    nudged = 0
    for case in SC.CASES:
        assert case.ref_elems() <= SC.MAX_REF_ELEMS, case.id
        nudged += SC.draw(case)['nudged']
    assert nudged > 0                              # the nudge is exercised
