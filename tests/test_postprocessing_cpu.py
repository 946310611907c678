"""Connected-component postprocessing, host side (no GPU): postprocessing.json parsing against the reference's output
(tests/golden/postprocessing.json from tools/oracle_gen/make_golden_postprocessing.py), the C ABI entries, and no host
fallback of the labelling."""
import json
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_load_postprocessing_reads_the_reference_json(tmp_path):
    from multitalent_amd.postprocessing.connected_components import load_postprocessing
    meta = json.load(open(os.path.join(HERE, 'golden', 'postprocessing.json')))
    seen = set()
    for sc in meta['b']:
        pp = dict(sc['postprocessing'])
        # numpy >= 2 prints the reference's np.float64 sizes as "np.float64(x)", which its own literal_eval cannot read back
        pp['min_valid_object_sizes'] = re.sub(r'np\.float64\(([^)]*)\)', r'\1', pp['min_valid_object_sizes'])
        f = tmp_path / (sc['name'] + '.json')
        f.write_text(json.dumps(pp))
        fwc, mins = load_postprocessing(str(f))
        assert fwc == sc['postprocessing']['for_which_classes']
        if sc['advanced']:
            assert isinstance(mins, dict) and set(mins) == {1} and mins[1] == pytest.approx(204.32999304056173, rel=0, abs=0)
        else:
            assert mins is None
        seen.add(json.dumps(fwc))
    assert seen == {'[[1, 2]]', '[1]', '[[1]]'}
    f = tmp_path / 'no_sizes.json'
    f.write_text(json.dumps({'for_which_classes': [[1, 2], 3]}))
    assert load_postprocessing(str(f)) == ([[1, 2], 3], None)


def test_header_and_signatures_declare_the_cc_entries():
    from multitalent_amd import _lib
    txt = open(os.path.join(HERE, '..', 'include', 'mtseg.h')).read()
    for name in ('mt_cc_label3d', 'mt_cc_remove'):
        assert re.search(r'\bint\s+%s\s*\(' % name, txt), name
        assert name in _lib.SIGNATURES
    assert _lib.MT_ABI_VERSION == 4


def test_no_host_fallback_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the device path is tested in test_postprocessing_gpu.py")
    from multitalent_amd.postprocessing.connected_components import remove_all_but_the_largest_connected_component
    img = np.zeros((6, 7, 8), np.uint8)
    img[0, 0, 0] = img[5, 6, 7] = 1
    with pytest.raises(RuntimeError, match="HIP device only"):
        remove_all_but_the_largest_connected_component(img, [1], 1.0)
    assert img[0, 0, 0] == 1 and img[5, 6, 7] == 1
