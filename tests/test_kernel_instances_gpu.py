"""Every kernel instance the five dispatch tables name, run on real memory against float64.

tests/instance_cases.py picks, per table, the cheapest launchable problem for every (instance, operand alignment / channel stride)
combination of the recorded tables, plus hand-written rows for the instances no small table row reaches.  One item per case:

  * materialise: the struct the table's problem() builds with real device memory behind every pointer.  Each operand is a channel slice
    of a wider 256-byte-aligned allocation at the row's offset modulo 16 bytes and with the row's channel stride; source neighbours
    hold 1e30 (65504 for fp16), destination neighbours and the gaps of the placed / scattered forms a bit pattern, destinations NaN
    (or seeded prior contents where the launch accumulates).
  * the kernel-name query on the REAL addresses equals the recorded name.
  * launch through the C ABI.
  * values against plain torch on the CPU in float64 (F.conv3d, F.conv_transpose3d, autograd, matrix products) with the measure and
    the bounds the family's own tests use: relerr = max |got - ref| / max |ref| < 1e-5 (fp32 forward, backward-data, pointwise),
    2e-5 (fp32 backward-weight, head backward, Winograd), 1e-4 for the instances that multiply 16-bit operands, against the reference
    over operands rounded to that type (the lazy activation lrelu(x scale + shift) applied in fp32 first, as the kernels stage it);
    a 16-bit destination adds the rounding of one store: 2^-9 (bf16) or 2^-12 (fp16) of max |ref| rounded up to a power of two (half an
    ulp is that fraction of the upper end of the value's binade; instance_cases.store_rounding).
  * statistics partials summed over blocks (tolerances of test_conv_fwd), the fused norm-backward sums (tolerances of
    test_winograd_backward_data_emits_norm_backward_statistics), dbias, accumulation on prior contents.
  * nothing else moved: every byte of the destination allocations outside the slice is bit-identical to its prefill, no NaN is left
    inside, the sources are unchanged.
"""
import pytest

import instance_cases as IC

pytestmark = pytest.mark.gpu


def _run(case, dev, seed):
    """One case.  A HIP error ends the whole run: nothing more is launched on a device that has faulted.  The launch's own return code
    (MT_EHIP) and any later HIP error are caught by message; after every other failure the device is asked once more (a sticky error
    shows in the next synchronisation) before the next case may start."""
    import torch
    try:
        IC.run_case(case, dev, seed)
    except BaseException as e:
        text = str(e)
        faulted = isinstance(e, RuntimeError) and any(k in text for k in ('rc=-3', 'HIP error', 'hipError', 'illegal memory', 'device-side'))
        if not faulted:
            try:
                torch.cuda.synchronize()
            except Exception as e2:          # noqa: BLE001
                faulted, text = True, str(e2)
        if faulted:
            pytest.exit('HIP error in %s: %s' % (IC.case_id(case), text), returncode=3)
        raise


def _params(table):
    return [pytest.param(c, i, id=IC.case_id(c)) for i, c in enumerate(IC.cases(table))]


@pytest.mark.parametrize('case,seed', _params('fwd'))
def test_conv_fwd_instance(dev, case, seed):
    _run(case, dev, seed)


@pytest.mark.parametrize('case,seed', _params('bwdd'))
def test_conv_bwd_data_strided_instance(dev, case, seed):
    _run(case, dev, seed)


@pytest.mark.parametrize('case,seed', _params('bwdw'))
def test_conv_bwd_weight_instance(dev, case, seed):
    _run(case, dev, seed)


@pytest.mark.parametrize('case,seed', _params('pw'))
def test_pointwise_instance(dev, case, seed):
    _run(case, dev, seed)


@pytest.mark.parametrize('case,seed', _params('hb'))
def test_head_bwd_instance(dev, case, seed):
    _run(case, dev, seed)
