"""Shared by the evaluation tests and tools/oracle_gen/make_golden_evaluation.py (not a test module).

* `surface_distances_scipy` and `hd / hd95 / asd / assd`: a restatement, with scipy, of medpy.metric.binary's published
  algorithm (`__surface_distances`: border = mask ^ binary_erosion(mask, generate_binary_structure(ndim, connectivity)),
  distances = distance_transform_edt(~border(reference), sampling)[border(result)]; hd = max of both directions' maxima,
  hd95 = numpy.percentile of both directions' distances, asd = mean of one direction, assd = mean of the two asd).  medpy is a
  third-party package the reference does not vendor: the tests are UNPINNED against medpy itself.
* `SCENARIOS`: the eight mask pairs of the surface-distance test on a (37, 61, 83) grid.
* `golden_case`: the seeded label-volume pairs behind tests/golden/evaluation.json."""
import types

import numpy as np

GRID = (37, 61, 83)
ADVANCED = ["Hausdorff Distance", "Hausdorff Distance 95", "Avg. Surface Distance", "Avg. Symmetric Surface Distance"]


def surface_distances_scipy(result, reference, voxelspacing=None, connectivity=1):
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    result = np.atleast_1d(np.asarray(result).astype(bool))
    reference = np.atleast_1d(np.asarray(reference).astype(bool))
    if voxelspacing is not None:
        voxelspacing = np.asarray(voxelspacing, dtype=np.float64) * np.ones(result.ndim)
    footprint = generate_binary_structure(result.ndim, connectivity)
    if 0 == np.count_nonzero(result):
        raise RuntimeError('The first supplied array does not contain any binary object.')
    if 0 == np.count_nonzero(reference):
        raise RuntimeError('The second supplied array does not contain any binary object.')
    result_border = result ^ binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ binary_erosion(reference, structure=footprint, iterations=1)
    dt = distance_transform_edt(~reference_border, sampling=voxelspacing)
    return dt[result_border]


def hd(result, reference, voxelspacing=None, connectivity=1):
    return max(surface_distances_scipy(result, reference, voxelspacing, connectivity).max(),
               surface_distances_scipy(reference, result, voxelspacing, connectivity).max())


def hd95(result, reference, voxelspacing=None, connectivity=1):
    hd1 = surface_distances_scipy(result, reference, voxelspacing, connectivity)
    hd2 = surface_distances_scipy(reference, result, voxelspacing, connectivity)
    return np.percentile(np.hstack((hd1, hd2)), 95)


def asd(result, reference, voxelspacing=None, connectivity=1):
    return surface_distances_scipy(result, reference, voxelspacing, connectivity).mean()


def assd(result, reference, voxelspacing=None, connectivity=1):
    return np.mean((asd(result, reference, voxelspacing, connectivity), asd(reference, result, voxelspacing, connectivity)))


def as_medpy_metric_module():
    """A module object with medpy.metric's four functions, for the reference's `from medpy import metric`."""
    m = types.ModuleType('medpy.metric')
    m.hd, m.hd95, m.asd, m.assd = hd, hd95, asd, assd
    return m


def ellipsoid(shape, centre, radii):
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return ((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 + ((x - centre[2]) / radii[2]) ** 2 <= 1


def _ellipsoids():
    return ellipsoid(GRID, (17, 28, 38), (9, 15, 20)), ellipsoid(GRID, (19, 32, 44), (8, 13, 22)), (2.5, 0.8, 0.8)


def _single_voxels():
    a, b = np.zeros(GRID, bool), np.zeros(GRID, bool)
    a[5, 10, 20] = True
    b[30, 50, 70] = True
    return a, b, (3, 1, 0.7)


def _boxes_on_faces():
    a, b = np.zeros(GRID, bool), np.zeros(GRID, bool)
    a[:12, :20, :30] = True
    b[20:, 35:, 50:] = True
    return a, b, None


def _plates():
    a, b = np.zeros(GRID, bool), np.zeros(GRID, bool)
    a[10, 5:50, 8:70] = True
    b[4:30, 30, 10:75] = True
    return a, b, (5, 1, 1)


def _shell_vs_solid():
    shell = ellipsoid(GRID, (18, 30, 41), (14, 24, 33)) & ~ellipsoid(GRID, (18, 30, 41), (10, 19, 27))
    return shell, ellipsoid(GRID, (18, 30, 41), (12, 21, 30)), (1.5, 1, 1)


def _nested():
    return ellipsoid(GRID, (18, 30, 41), (5, 8, 10)), ellipsoid(GRID, (18, 30, 41), (15, 26, 36)), (1, 1.25, 0.75)


def _two_components():
    a = ellipsoid(GRID, (10, 15, 20), (6, 9, 12)) | ellipsoid(GRID, (30, 52, 74), (3, 4, 5))
    b = ellipsoid(GRID, (11, 17, 22), (6, 9, 12)) | ellipsoid(GRID, (8, 50, 10), (3, 5, 5))
    return a, b, (2, 1, 1)


def _noise():
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(7)
    a = gaussian_filter(rng.standard_normal(GRID), sigma=3) > 0.02
    b = gaussian_filter(rng.standard_normal(GRID), sigma=3) > 0.02
    return a, b, (1, 0.5, 0.5)


SCENARIOS = {'ellipsoids': _ellipsoids, 'single_voxels': _single_voxels, 'boxes_on_faces': _boxes_on_faces, 'plates': _plates,
             'shell_vs_solid': _shell_vs_solid, 'nested': _nested, 'two_components': _two_components, 'noise': _noise}


def big_ellipsoids():
    shape = (192, 256, 256)
    return ellipsoid(shape, (96, 128, 128), (60, 90, 100)), ellipsoid(shape, (100, 120, 135), (64, 84, 96)), (2.5, 0.8, 0.8)


GOLDEN_SHAPE = (28, 44, 52)
GOLDEN_LABELS = [1, 2, 3, (1, 2, 3)]
GOLDEN_CASES = [dict(name='case_0', seed=11, spacing=(2.5, 0.8, 0.8), absent=None),
                dict(name='case_1', seed=12, spacing=(1.0, 1.0, 1.0), absent=None),
                dict(name='case_2', seed=13, spacing=(3.0, 1.5, 0.7), absent=3),
                dict(name='case_3', seed=14, spacing=(1.25, 0.9, 1.1), absent=None)]


def golden_case(seed, absent=None):
    """-> (test, reference) uint8 label volumes of GOLDEN_SHAPE: one ellipsoid per label 1..3, the reference's shifted and
    rescaled; `absent`: a label left out of both volumes."""
    rng = np.random.default_rng(seed)
    s = np.array(GOLDEN_SHAPE, dtype=np.float64)
    test, ref = np.zeros(GOLDEN_SHAPE, np.uint8), np.zeros(GOLDEN_SHAPE, np.uint8)
    anchors = ((0.3, 0.3, 0.3), (0.65, 0.6, 0.4), (0.4, 0.55, 0.75))
    for lab, a in zip((1, 2, 3), anchors):
        c = (np.array(a) + rng.uniform(-0.04, 0.04, 3)) * s
        r = rng.uniform(0.1, 0.17, 3) * s
        shift = rng.uniform(-2.5, 2.5, 3)
        scale = rng.uniform(0.85, 1.15, 3)
        if lab == absent:
            continue
        test[ellipsoid(GOLDEN_SHAPE, c, r)] = lab
        ref[ellipsoid(GOLDEN_SHAPE, c + shift, r * scale)] = lab
    return test, ref
