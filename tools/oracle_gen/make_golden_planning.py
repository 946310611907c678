"""Golden vectors for experiment planning: the REAL reference's planners (experiment_planning/experiment_planner_baseline_3DUNet.py,
..._v21.py, task_specific_planner/MultiTalent/MultiTalent_planner.py, alternative_experiment_planning/experiment_planner_residual_
3DUNet_v21.py and experiment_planner_pretrained.py), `common_utils.get_pool_and_conv_props*` and the two networks'
`compute_approx_vram_consumption`, run on synthetic fingerprints.  The batchgenerators file helpers the reference takes from its
star import (third party, absent here) are added below.  Writes tests/golden/planning.json in the codec of tests/planning_cases.py:

  fingerprints   per fingerprint: the case names and `dataset_properties`, the complete plans of the four planners (paths relative
                 to the cropped / preprocessed folder; the entries that repeat the fingerprint are stored as a mark, `compact_plans`) and the `use_nonzero_mask_for_norm` written into every case pickle;
  props          inputs and the five outputs of both `get_pool_and_conv_props*` over seeded (spacing, patch) pairs;
  vram           `compute_approx_vram_consumption` of Generic_UNet and FabiansUNet over seeded configurations;
  pretrained     the v2.1 plans of one fingerprint used as `-overwrite_plans` for another: the file name, and the entries in which
                 the file differs from the target's own v2.1 plan before the preprocessing and from the source's plan after it.

Run: python tools/oracle_gen/make_golden_planning.py"""
import contextlib, io, json, os, pickle, shutil, sys, tempfile
from collections import OrderedDict
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.normpath(os.path.join(HERE, '..', '..', 'tests')))
import make_golden_dataset_analysis as DA      # installs the reference import shim and subfiles, load_json, save_pickle, load_pickle
import batchgenerators.utilities.file_and_folder_operations as ffo
import planning_cases as PC
load_pickle = DA.load_pickle


def subdirs(folder, join=True, prefix=None, suffix=None, sort=True):
    """Restatement of batchgenerators' subdirs, as `subfiles` there."""
    res = [os.path.join(folder, i) if join else i for i in os.listdir(folder)
           if os.path.isdir(os.path.join(folder, i)) and (prefix is None or i.startswith(prefix)) and (suffix is None or i.endswith(suffix))]
    return sorted(res) if sort else res


def save_json(obj, file, indent=4, sort_keys=True):
    with open(file, 'w') as f:
        json.dump(obj, f, sort_keys=sort_keys, indent=indent)


ffo.subdirs, ffo.save_json, ffo.write_pickle = subdirs, save_json, DA.save_pickle
ffo.pickle, ffo.json, ffo.shutil = pickle, json, shutil
ffo.__all__ = sorted(set(ffo.__all__) | {'subdirs', 'save_json', 'write_pickle', 'pickle', 'json', 'shutil'})
from nnunet.experiment_planning.experiment_planner_baseline_3DUNet import ExperimentPlanner
from nnunet.experiment_planning.experiment_planner_baseline_3DUNet_v21 import ExperimentPlanner3D_v21
from nnunet.experiment_planning.task_specific_planner.MultiTalent.MultiTalent_planner import ExperimentPlanner3D_v21_MultiTalent
from nnunet.experiment_planning.alternative_experiment_planning.experiment_planner_residual_3DUNet_v21 import \
    ExperimentPlanner3DFabiansResUNet_v21
from nnunet.experiment_planning.alternative_experiment_planning.experiment_planner_pretrained import ExperimentPlanner3D_v21_Pretrained
from nnunet.experiment_planning import common_utils as ref_cu
from nnunet.network_architecture.generic_UNet import Generic_UNet
from nnunet.network_architecture.generic_modular_residual_UNet import FabiansUNet

PLANNERS = (ExperimentPlanner, ExperimentPlanner3D_v21, ExperimentPlanner3D_v21_MultiTalent, ExperimentPlanner3DFabiansResUNet_v21)


def synthetic(rs, n, shape, spacing, jitter, modalities, classes, reduction):
    """n cases: sizes and spacings near `shape` / `spacing` (each factor uniform in 1 +- jitter), size reductions near `reduction`."""
    dp = dict()
    dp['all_sizes'] = [tuple(int(max(4, round(s * (1 + jitter * rs.uniform(-1, 1))))) for s in shape) for _ in range(n)]
    dp['all_spacings'] = [np.array([s * (1 + jitter * rs.uniform(-1, 1)) for s in spacing]) for _ in range(n)]
    dp['all_classes'] = list(range(1, classes))
    dp['modalities'] = {i: m for i, m in enumerate(modalities)}
    dp['intensityproperties'] = None
    cases = ['case_%03d' % i for i in range(n)]
    dp['size_reductions'] = OrderedDict((c, float(min(1.0, reduction * (1 + 0.1 * rs.uniform(-1, 1))))) for c in cases)
    return {'cases': cases, 'dataset_properties': dp}


SYNTHETIC = OrderedDict([      # name: (seed, cases, shape, spacing, jitter, modalities, classes incl. background, size reduction)
    ('ct_large', (4, 12, (200, 512, 512), (2.5, 0.8, 0.8), 0.1, ['CT'], 3, 1.0)),
    ('ct_small', (1, 7, (60, 90, 70), (0.98, 0.98, 1.05), 0.02, ['CT'], 2, 0.9)),
    ('aniso', (4, 9, (12, 256, 216), (10.0, 1.5, 1.5), 0.3, ['MRI'], 4, 1.0)),
    ('brain4', (1, 10, (140, 170, 140), (1.0, 1.0, 1.0), 0.03, ['T1', 'T1ce', 'T2', 'noNorm'], 4, 0.4)),
    ('last_axis', (2, 8, (320, 320, 70), (0.7, 0.7, 3.0), 0.08, ['CT'], 14, 1.0)),
])


def fingerprints():
    fps = OrderedDict((k, synthetic(np.random.RandomState(v[0]), *v[1:])) for k, v in SYNTHETIC.items())
    fps['tiny'] = PC.toy_fingerprint(PC.TASK901)
    return fps


def run_planner(cls, fp, extra=()):
    """-> (file name of the plans, the plans with relative paths, the masks written into the case pickles)."""
    with tempfile.TemporaryDirectory() as cropped, tempfile.TemporaryDirectory() as out:
        PC.write_fingerprint_folder(cropped, fp)
        with contextlib.redirect_stdout(io.StringIO()):
            planner = cls(cropped, out, *extra)
            planner.plan_experiment()
        plans = load_pickle(planner.plans_fname)
        roots = {cropped: '<cropped>', out: '<preprocessed>'}
        return os.path.basename(planner.plans_fname), PC.relativize(plans, roots), PC.case_mask(cropped, fp['cases'])


def props_table(rs, n=200):
    rows = []
    for i in range(n):
        base = rs.choice([0.5, 0.7, 1.0, 1.5])
        spacing = [round(float(base * rs.choice([1, 1, 1.3, 1.9, 2.0, 2.1, 3.0, 4.5, 7.0]) * rs.uniform(0.95, 1.05)), 3) for _ in range(3)]
        patch = [int(rs.choice([5, 7, 8, 12, 16, 20, 24, 40, 56, 64, 96, 100, 128, 160, 192, 250])) for _ in range(3)]
        cap = int(rs.choice([999, 999, 5, 3]))
        late = ref_cu.get_pool_and_conv_props_poolLateV2(list(patch), 4, cap, np.array(spacing))
        v21 = ref_cu.get_pool_and_conv_props(np.array(spacing), list(patch), 4, cap)
        assert all(isinstance(r[3], np.ndarray) and isinstance(r[4], np.ndarray) for r in (late, v21))
        rows.append([' '.join(repr(i) for i in spacing), patch, cap, PC.pack_topology(late), PC.pack_topology(v21)])
    return rows


def vram_table(rs, n=24):
    rows = []
    for i in range(n):
        spacing = np.array([float(rs.choice([1.0, 2.0, 3.0, 5.0])), 1.0, float(rs.choice([1.0, 1.2]))])
        patch = [int(rs.choice([16, 32, 40, 64, 96, 128, 160, 192])) for _ in range(3)]
        pools_per_axis, pool_k, conv_k, shp, _ = ref_cu.get_pool_and_conv_props(spacing, patch, 4, 999)
        base, mx = int(rs.choice([30, 32, 24])), int(rs.choice([320, 512]))
        mods, classes, cps, ds = int(rs.randint(1, 5)), int(rs.randint(2, 40)), int(rs.choice([2, 3])), bool(rs.randint(2))
        plain = Generic_UNet.compute_approx_vram_consumption(shp, pools_per_axis, base, mx, mods, classes, pool_k, ds, cps)
        pk = [[1, 1, 1]] + pool_k
        enc = FabiansUNet.default_blocks_per_stage_encoder[:len(pk)]
        dec = FabiansUNet.default_blocks_per_stage_decoder[:len(pk) - 1]
        with contextlib.redirect_stdout(io.StringIO()):
            res = FabiansUNet.compute_approx_vram_consumption(shp, base, mx, mods, classes, pk, enc, dec, 2, 2)
        rows.append({'patch': [int(i) for i in shp], 'pools': PC.pack_kernels(pool_k), 'base': base, 'max': mx,
                     'modalities': mods, 'classes': classes, 'conv_per_stage': cps, 'deep_supervision': ds,
                     'plain': plain, 'plain_type': type(plain).__name__, 'residual': res})
    return rows


def pretrained_flow(source_fp, target_fp):
    with tempfile.TemporaryDirectory() as sc, tempfile.TemporaryDirectory() as so, \
            tempfile.TemporaryDirectory() as tc, tempfile.TemporaryDirectory() as to:
        PC.write_fingerprint_folder(sc, source_fp)
        PC.write_fingerprint_folder(tc, target_fp)
        with contextlib.redirect_stdout(io.StringIO()):
            src = ExperimentPlanner3D_v21(sc, so)
            src.plan_experiment()
            planner = ExperimentPlanner3D_v21_Pretrained(tc, to, src.plans_fname, 'GOLD')
            planner.plan_experiment()
            own = load_pickle(planner.plans_fname)
            planner.load_pretrained_plans()
        roots = {sc: '<source_cropped>', so: '<source_preprocessed>', tc: '<cropped>', to: '<preprocessed>'}
        source, final = load_pickle(src.plans_fname), load_pickle(planner.plans_fname)
        v21 = run_planner(ExperimentPlanner3D_v21, target_fp)[1]
        own = PC.relativize(own, roots)
        # before the preprocessing the file holds the target's own v2.1 plan under the new identifier; afterwards the source's plan
        own_differs = [k for k in own if PC.encode(own[k]) != PC.encode(v21[k])]
        differs = [k for k in final if PC.encode(final[k]) != PC.encode(source[k])]
        assert list(own) == list(v21) and list(final) == list(source)
        return {'fname': os.path.basename(planner.plans_fname), 'own_differs_from_v21': {k: own[k] for k in own_differs},
                'differs_from_source': {k: final[k] for k in differs}, 'preprocessor_name': planner.preprocessor_name,
                'transpose_forward': planner.transpose_forward}


def main():
    fps = fingerprints()
    gold = OrderedDict(fingerprints=OrderedDict())
    for name, fp in fps.items():
        rec = OrderedDict(cases=fp['cases'], dataset_properties=fp['dataset_properties'], planners=OrderedDict())
        for cls in (PLANNERS if name != 'tiny' else PLANNERS[1:2]):      # the toy task of the device tests: v2.1 only
            fname, plans, masks = run_planner(cls, fp)
            rec['planners'][cls.__name__] = {'fname': fname, 'plans': PC.compact_plans(plans, fp), 'case_mask': masks}
            st = plans['plans_per_stage']
            print(name, cls.__name__, 'stages', len(st), 'tf', plans['transpose_forward'],
                  [(list(s['patch_size']), s['batch_size'], list(np.round(s['current_spacing'], 3)), s['conv_kernel_sizes'][0],
                    len(s['pool_op_kernel_sizes']), bool(s['do_dummy_2D_data_aug'])) for s in st.values()],
                  plans['normalization_schemes'], plans['use_mask_for_norm'])
        gold['fingerprints'][name] = rec
    rs = np.random.RandomState(77)
    gold['props'] = props_table(rs)
    gold['vram'] = vram_table(rs)
    gold['pretrained'] = dict(source='ct_large', target='ct_small', **pretrained_flow(fps['ct_large'], fps['ct_small']))
    dst = PC.GOLDEN
    with open(dst, 'w') as f:
        json.dump(PC.encode(gold), f, separators=(',', ':'))
        f.write('\n')
    print('wrote', dst, os.path.getsize(dst) // 1024, 'KiB')


if __name__ == '__main__':
    main()
