"""Golden numbers for the normalized surface Dice: the REAL reference's nnunet/evaluation/surface_dice.py
(`normalized_surface_dice`, :20-56), run on CPU in the build container on the eight mask pairs of tests/evaluation_cases.py
(`SCENARIOS`, the (37, 61, 83) grid), with connectivity 1, 2, 3, spacing (1, 1, 1) and (2.5, 0.8, 0.8) and the tolerances below.

Substitution at a third-party seam: `medpy.metric.binary.__surface_distances` (medpy is not in this image and is not vendored by
the reference) -> `surface_distances_scipy` of tests/evaluation_cases.py, the scipy restatement of medpy's published algorithm.
The numbers are therefore UNPINNED against medpy itself; what is pinned is the reference's own counting and formula.

Beside each value the file keeps what a test needs to compare integer counts: the border voxels per direction, the restated
distances <= the tolerance per direction, and `exempt`: how many restated distances lie within 1e-12 (relative) of the tolerance,
where a device distance that differs from scipy's in the last bits may fall on the other side.  With unit spacing (squared
distances are integers, both sides take the correctly rounded root) and at tolerance 0 (a zero offset is 0.0 on both sides) nothing
is exempt.  ASSERTED here: `exempt` never exceeds 1e-3 of a case's border voxels.

Writes names and numbers only to tests/golden/surface_dice.json; the test rebuilds the masks.
Run: python tools/oracle_gen/make_golden_surface_dice.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ref_import
ref_import.install()

import evaluation_cases as EC

import medpy.metric.binary as medpy_binary
setattr(medpy_binary, '__surface_distances', EC.surface_distances_scipy)
from nnunet.evaluation.surface_dice import normalized_surface_dice

SPACINGS = [(1.0, 1.0, 1.0), (2.5, 0.8, 0.8)]
CONNECTIVITIES = [1, 2, 3]
TOLERANCES = [0.0, 1.0, 2.0, 1.25, 2.6, 1000.0]              # the last one lies beyond every distance on this grid (asserted)
NEAR = 1e-12
EXEMPT_CAP = 1e-3


def main():
    out = {'grid': list(EC.GRID), 'spacings': [list(s) for s in SPACINGS], 'connectivities': CONNECTIVITIES,
           'tolerances': TOLERANCES, 'near': NEAR, 'exempt_cap': EXEMPT_CAP, 'cases': []}
    worst_exempt = 0
    for name, make in EC.SCENARIOS.items():
        a, b, _ = make()
        for conn in CONNECTIVITIES:
            for sp in SPACINGS:
                d_ab = EC.surface_distances_scipy(a, b, sp, conn)
                d_ba = EC.surface_distances_scipy(b, a, sp, conn)
                assert max(d_ab.max(), d_ba.max()) < TOLERANCES[-1]
                case = {'scenario': name, 'connectivity': conn, 'spacing': list(sp), 'n_tr': int(len(d_ab)), 'n_rt': int(len(d_ba)),
                        'by_tolerance': []}
                unit = all(s == 1.0 for s in sp)
                for tol in TOLERANCES:
                    value = float(normalized_surface_dice(a, b, tol, sp, conn))
                    exempt = [0, 0]
                    if not unit and tol > 0:
                        exempt = [int((np.abs(d - tol) <= NEAR * tol).sum()) for d in (d_ab, d_ba)]
                    assert sum(exempt) <= EXEMPT_CAP * (len(d_ab) + len(d_ba)), (name, conn, sp, tol, exempt)
                    worst_exempt = max(worst_exempt, sum(exempt))
                    case['by_tolerance'].append({'tolerance': tol, 'value': value, 'c_tr': int((d_ab <= tol).sum()),
                                                 'c_rt': int((d_ba <= tol).sum()), 'exempt': exempt})
                assert case['by_tolerance'][-1]['c_tr'] == case['n_tr'] and case['by_tolerance'][-1]['c_rt'] == case['n_rt']
                out['cases'].append(case)
    dst = os.path.join(ROOT, 'tests', 'golden', 'surface_dice.json')
    with open(dst, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', dst, os.path.getsize(dst), 'bytes;', len(out['cases']), 'cases; most exempt distances in a case:', worst_exempt)


if __name__ == '__main__':
    main()
