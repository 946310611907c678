"""Golden numbers for the evaluation: the REAL reference's nnunet/evaluation/evaluator.py (`Evaluator`, `aggregate_scores`, :30-225,
:321-400) over its nnunet/evaluation/metrics.py, run on CPU in the build container on the four seeded label-volume pairs of
tests/evaluation_cases.py (`golden_case`: three labels plus the tuple label (1, 2, 3); label 3 is absent from one case, so NaN and
the nan-mean are exercised), with advanced=True and all four surface-distance metrics.

Substitutions for what this image lacks, at third-party seams:
  * `medpy.metric` (the reference's `from medpy import metric`) -> a module whose hd / hd95 / asd / assd are the scipy restatement
    of medpy's published algorithm in tests/evaluation_cases.py.  The surface-distance numbers are therefore UNPINNED against
    medpy itself: what is pinned is the reference's own code around it (NaN rules, keyword plumbing, aggregation, json layout);
  * SimpleITK, pandas' absence and batchgenerators' file helpers -> tools/oracle_gen/ref_import.py; `save_json` -> json.dump.
The plain `Evaluator` is used (arrays in, voxel_spacing passed explicitly); labels are given as the reference's dict form, which is
the one its tuple entries work with.

Writes only names, seeds, spacings and the resulting numbers to tests/golden/evaluation.json; the test rebuilds the volumes.
Run: python tools/oracle_gen/make_golden_evaluation.py"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ref_import
ref_import.install()

import evaluation_cases as EC

import batchgenerators.utilities.file_and_folder_operations as ffo


def _save_json(obj, file, indent=4, sort_keys=True):
    with open(file, 'w') as f:
        json.dump(obj, f, sort_keys=sort_keys, indent=indent)


ffo.save_json = _save_json
ffo.subfiles = lambda *a, **k: []
ffo.__all__ = list(ffo.__all__) + ['save_json', 'subfiles']

import nnunet.evaluation.metrics as ref_metrics
ref_metrics.metric = EC.as_medpy_metric_module()
import nnunet.evaluation.evaluator as ref_eval


def _clean(x):
    """json without NaN literals: NaN -> None"""
    if isinstance(x, dict):
        return {k: _clean(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_clean(v) for v in x]
    if isinstance(x, float) and np.isnan(x):
        return None
    return x


def main():
    labels = {l: str(l) for l in EC.GOLDEN_LABELS}
    out = {'shape': list(EC.GOLDEN_SHAPE), 'labels': [list(l) if isinstance(l, tuple) else l for l in EC.GOLDEN_LABELS],
           'advanced_metrics': EC.ADVANCED, 'runs': []}
    for connectivity in (1, 2):
        # one aggregate_scores call per spacing would split the mean: every case is run with ITS spacing through the
        # reference's evaluator, the cases' dicts are then aggregated by the reference's own loop via a second call below
        per_case = []
        for c in EC.GOLDEN_CASES:
            test, ref = EC.golden_case(c['seed'], c['absent'])
            ev = ref_eval.Evaluator(advanced_metrics=list(EC.ADVANCED))
            s = ref_eval.aggregate_scores([(test, ref)], evaluator=ev, labels=labels, num_threads=1, advanced=True,
                                          voxel_spacing=np.array(c['spacing']), connectivity=connectivity)
            per_case.append(s['all'][0])
        # all four cases in one call, one spacing for all (the keyword is per call in the reference), with the json written
        sp = EC.GOLDEN_CASES[0]['spacing']
        pairs = [EC.golden_case(c['seed'], c['absent']) for c in EC.GOLDEN_CASES]
        with tempfile.TemporaryDirectory() as d:
            jf = os.path.join(d, 'summary.json')
            ev = ref_eval.Evaluator(advanced_metrics=list(EC.ADVANCED))
            s = ref_eval.aggregate_scores(pairs, evaluator=ev, labels=labels, num_threads=2, json_output_file=jf, json_name='golden',
                                          json_task='T', advanced=True, voxel_spacing=np.array(sp), connectivity=connectivity)
            with open(jf) as f:
                summary = json.load(f)
        out['runs'].append({'connectivity': connectivity, 'cases': [dict(c) for c in EC.GOLDEN_CASES], 'per_case': _clean(per_case),
                            'joint_spacing': list(sp), 'joint': _clean({'all': s['all'], 'mean': s['mean']}),
                            'summary_keys': sorted(summary.keys()), 'summary_results_keys': sorted(summary['results'].keys())})
    dst = os.path.join(ROOT, 'tests', 'golden', 'evaluation.json')
    with open(dst, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', dst, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
    main()
