"""Helpers of the surface-metric tests (test_surface_metrics_emu.py on the CPU emulator, test_gpu_surface_metrics.py on the device): the
cases, the numpy / scipy reference (icl_amd.val_3D._surface_distances: MedPy 0.4.0's ``__surface_distances`` with ``sampling=spacing``,
np.percentile, .mean()) and the comparison of one record of ``ops.seg_surface_metrics`` with it.  The reference is never the code under test.

Tolerances (derived, not measured):
  * DYADIC spacings — (1, 1, 1), (1.5, 1.5, 2.0), (10, 1.25, 1.25), (0.78125, 0.78125, 5.0), (0.5, 0.5, 0.5) — at these extents every
    axis term and every sum is exact in double, whatever the order: hd95, hd and both NSD counts are BIT-EQUAL to the reference.
  * (0.7, 0.9, 1.3): scipy adds the axis terms in the order 0, 1, 2, the passes in the order 2, 1, 0.  Each d^2 carries at most five
    roundings per side (three squares after three products counted once each, two sums); the square root halves their relative size and
    adds one rounding; an order statistic of values each perturbed by at most eps moves by at most eps: hd95 and hd within relative 16 * 2^-53.
  * sums (asd_*, assd): n non-negative terms added in different orders, each term's root one ulp off at most: relative (n + 4) * 2^-52
    with n the number of border voxels of that direction; assd is the mean of the two, so the larger of the two bounds holds for it.
  * NSD with the non-dyadic spacing: tolerance 2.0, and the test first asserts ON THE REFERENCE's distances that none lies within
    relative 1e-9 of it; then the counts are equal.
"""
import numpy as np

from icl_amd.val_3D import _surface_distances, hd95_from_order_stats

DYADIC = [(1.0, 1.0, 1.0), (1.5, 1.5, 2.0), (10.0, 1.25, 1.25), (0.78125, 0.78125, 5.0)]
NON_DYADIC = (0.7, 0.9, 1.3)
NON_DYADIC_TOLERANCE = 2.0
U = 2.0 ** -53


def is_dyadic(spacing):
    return all(float(s * 2 ** 20).is_integer() for s in spacing)


def blob(shape, center, radii, rng=None, speckle=0.0):
    idx = np.indices(shape).astype(np.float64)
    r = sum(((idx[i] - center[i]) / radii[i]) ** 2 for i in range(3))
    m = r <= 1.0
    if rng is not None and speckle:
        m ^= rng.random(shape) < speckle
    return m


def ellipsoids(seed, shape=(19, 23, 17)):
    """Two overlapping ellipsoids with 3 % speckle, uint8 ground truth against int64 prediction."""
    rng = np.random.default_rng(seed)
    c = [s // 2 for s in shape]
    gt = blob(shape, c, (shape[0] / 3.2, shape[1] / 2.9, shape[2] / 3.4), rng, 0.03).astype(np.uint8)
    pred = blob(shape, (c[0] + 1, c[1] + 1, c[2] - 1), (shape[0] / 3.8, shape[1] / 3.3, shape[2] / 2.9), rng, 0.03).astype(np.int64)
    return gt, pred


def anisotropy_pair():
    """6 x 40 x 40 at (10, 1.25, 1.25): the prediction's voxel has a ground-truth voxel one slice away (and one pixel aside: 1.41 voxels,
    10.08 mm) and another eight pixels away in plane (8 voxels, 10 mm): the nearest feature in millimetres is not the nearest in voxels."""
    gt = np.zeros((6, 40, 40), np.uint8)
    pred = np.zeros((6, 40, 40), np.int64)
    pred[2, 20, 20] = 1
    gt[3, 21, 20] = 1
    gt[2, 20, 28] = 1
    return gt, pred


def disjoint_boxes():
    shape = (14, 16, 12)
    gt = blob(shape, (2, 3, 2), (2, 3, 2)).astype(np.uint8)
    pred = blob(shape, (11, 12, 9), (2, 3, 2)).astype(np.int64)
    return gt, pred


def slab_on_five_faces():
    shape = (12, 15, 10)
    gt = np.zeros(shape, np.uint8)
    gt[:5, :, :4] = 1
    pred = np.zeros(shape, np.int64)
    pred[:, 10:, :] = 1
    pred[0, 0, 0] = 1
    return gt, pred


def speckle_everywhere():
    rng = np.random.default_rng(21)
    shape = (15, 14, 13)
    return (rng.random(shape) < 0.3).astype(np.uint8), (rng.random(shape) < 0.25).astype(np.int64)


def single_voxels():
    gt = np.zeros((5, 6, 7), np.uint8)
    pred = np.zeros((5, 6, 7), np.int64)
    gt[3, 4, 5] = 1
    pred[1, 1, 1] = 1
    return gt, pred


def single_voxel_against_large():
    shape = (16, 14, 18)
    gt = blob(shape, (8, 7, 9), (7, 6, 8)).astype(np.int64)
    pred = np.zeros(shape, np.uint8)
    pred[3, 4, 5] = 1
    return gt, pred


def identical_maps():
    rng = np.random.default_rng(5)
    m = blob((13, 11, 9), (6, 5, 4), (5, 4, 3), rng, 0.05).astype(np.int64)
    return m, m.copy()


def three_points(near, far):
    """The prediction is the voxel at the origin, the ground truth two isolated voxels at the offsets ``near`` and ``far``: n = 3 border
    voxels, the sorted union of the squared distances is [d(near), d(near), d(far)] and k0 = floor(0.95 * 2) = 1, so the two order
    statistics are d(near)^2 and d(far)^2."""
    shape = tuple(max(a, b) + 2 for a, b in zip(near, far))
    gt = np.zeros(shape, np.uint8)
    pred = np.zeros(shape, np.int64)
    pred[0, 0, 0] = 1
    gt[tuple(near)] = 1
    gt[tuple(far)] = 1
    return gt, pred


def pass_order_square(offset, spacing):
    """The squared distance of one offset as the kernels form it: t = (double)delta * s, t * t per axis, added in the order 2, 1, 0."""
    t = [np.float64(o) * np.float64(s) for o, s in zip(offset, spacing)]
    return (t[2] * t[2] + t[1] * t[1]) + t[0] * t[0]


def four_class_maps():
    """Classes 1..4 (num_classes 5): 1 in both maps, 2 absent from the prediction, 3 absent from both, 4 absent from the ground truth."""
    rng = np.random.default_rng(11)
    shape = (15, 13, 11)
    gt = np.zeros(shape, np.uint8)
    pred = np.zeros(shape, np.int64)
    gt[blob(shape, (5, 5, 5), (4, 4, 3), rng, 0.02)] = 1
    pred[blob(shape, (6, 5, 4), (4, 3, 3), rng, 0.02)] = 1
    gt[blob(shape, (11, 9, 7), (2, 3, 3))] = 2
    pred[blob(shape, (11, 3, 8), (2, 2, 2))] = 4
    return gt, pred


CASES = {
    "anisotropy": anisotropy_pair, "disjoint_boxes": disjoint_boxes, "slab_on_five_faces": slab_on_five_faces,
    "speckle_everywhere": speckle_everywhere, "single_voxels": single_voxels, "single_voxel_against_large": single_voxel_against_large,
    "identical_maps": identical_maps,
}


class Reference:
    """The reference quantities of class c, formed once per (maps, class, spacing)."""

    def __init__(self, gt, pred, c, spacing):
        self.p, self.g = pred == c, gt == c
        self.np_, self.ng, self.inter = int(self.p.sum()), int(self.g.sum()), int((self.p & self.g).sum())
        self.valid = self.np_ > 0 and self.ng > 0
        if self.valid:
            self.a = _surface_distances(self.p, self.g, spacing)      # dP -> dG
            self.b = _surface_distances(self.g, self.p, spacing)      # dG -> dP
            self.union = np.sort(np.hstack((self.a, self.b)))
            self.hd95 = float(np.percentile(np.hstack((self.a, self.b)), 95))
            self.hd = float(max(self.a.max(), self.b.max()))


def assert_tolerance_is_clear(ref, tolerance):
    """Precondition on the INPUTS of an NSD comparison with a non-dyadic spacing: no reference distance within 1e-9 (relative) of tau."""
    d = np.hstack((ref.a, ref.b))
    assert not np.any(np.abs(d - tolerance) <= 1e-9 * tolerance), "choose another seed: a distance sits on the tolerance"


def check_record(cnt, val, ref, spacing, tolerance):
    """One row of ops.seg_surface_metrics (lists) against the reference, under the tolerances of this module's docstring."""
    cnt = [int(v) for v in cnt]
    val = [np.float64(v) for v in val]
    assert cnt[:3] == [ref.np_, ref.ng, ref.inter]
    if not ref.valid:
        assert all(v == -1.0 for v in val), val
        assert cnt[5] == 0 and cnt[6] == 0
        return
    na, nb = len(ref.a), len(ref.b)
    assert cnt[3:5] == [na, nb]
    n = na + nb
    k0 = int(np.floor((n - 1) * 0.95))
    hd95 = hd95_from_order_stats(n, val[0], val[1])
    hd = float(max(np.sqrt(val[2]), np.sqrt(val[3])))
    within = [int(np.count_nonzero(ref.a <= tolerance)), int(np.count_nonzero(ref.b <= tolerance))]
    if is_dyadic(spacing):
        assert np.sqrt(val[0]) == ref.union[k0] and np.sqrt(val[1]) == ref.union[k0 + 1]
        assert hd95 == ref.hd95 and hd == ref.hd
        assert np.sqrt(val[2]) == ref.a.max() and np.sqrt(val[3]) == ref.b.max()
        assert cnt[5:7] == within
    else:
        assert abs(hd95 - ref.hd95) <= 16 * U * ref.hd95, (hd95, ref.hd95)
        assert abs(hd - ref.hd) <= 16 * U * ref.hd, (hd, ref.hd)
        assert_tolerance_is_clear(ref, tolerance)
        assert cnt[5:7] == within
    for s, d, m in ((val[4], ref.a, na), (val[5], ref.b, nb)):
        want = float(d.sum())
        assert abs(float(s) - want) <= (m + 4) * 2 * U * want, (float(s), want, m)
        assert abs(float(s) / m - float(d.mean())) <= (m + 4) * 2 * U * float(d.mean())


def check_dict(rec, ref, spacing, tolerance):
    """One dict of surface_metrics_multiclass for a class present in both maps against the host restatements' quantities."""
    na, nb = len(ref.a), len(ref.b)
    apg, agp = float(ref.a.mean()), float(ref.b.mean())
    assert rec["dice"] == 2.0 * ref.inter / float(ref.np_ + ref.ng) and isinstance(rec["dice"], float)
    if is_dyadic(spacing):
        assert rec["hd95"] == ref.hd95 and rec["hd"] == ref.hd
    else:
        assert abs(rec["hd95"] - ref.hd95) <= 16 * U * ref.hd95 and abs(rec["hd"] - ref.hd) <= 16 * U * ref.hd
        assert_tolerance_is_clear(ref, tolerance)
    assert abs(rec["asd_pred_gt"] - apg) <= (na + 4) * 2 * U * apg
    assert abs(rec["asd_gt_pred"] - agp) <= (nb + 4) * 2 * U * agp
    want = float(np.mean((apg, agp)))
    assert abs(rec["assd"] - want) <= (max(na, nb) + 4) * 2 * U * want
    assert rec["nsd"] == float((np.count_nonzero(ref.a <= tolerance) + np.count_nonzero(ref.b <= tolerance)) / (na + nb))
    assert all(isinstance(rec[k], float) for k in rec)
