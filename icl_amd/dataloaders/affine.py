"""Host side of the affine stage (random rotation and zoom) that the device feeds share: the matrix, the keyword checks, the draws and
the ``affine_params`` block of a launch.  ``dataloaders/amos.py`` (``OnDeviceAugmentAMOS``, ``OnDeviceAugmentPosNeg``) and
``dataloaders/brats2019.py`` (``OnDeviceAugment``) both import from here; every name stays importable from ``dataloaders.amos`` as well."""
from __future__ import annotations

import ctypes
from typing import List, Sequence

import numpy as np

AFFINE_MAX_ENTRY = 16.0     # icl_volume_feed_affine refuses |M_ab| above this: |x| then stays far below 2^31 for every legal extent


def affine_matrix(theta: Sequence[float], zoom) -> np.ndarray:
    """``M = R_0(theta_0) @ R_1(theta_1) @ R_2(theta_2) @ diag(1 / z_0, 1 / z_1, 1 / z_2)`` in double: the 3x3 matrix that takes an
    OUTPUT offset from the patch centre to the SOURCE offset the affine stage samples.  ``R_a`` is the right-handed rotation about patch
    axis ``a`` (radians); ``zoom``: one number or three, ``z > 1`` magnifies the content."""
    t = np.asarray(theta, dtype=np.float64).reshape(-1)
    z = np.asarray(zoom, dtype=np.float64).reshape(-1)
    if z.size == 1:
        z = np.repeat(z, 3)
    if t.size != 3 or z.size != 3 or not np.isfinite(t).all() or not np.isfinite(z).all() or (z <= 0).any():
        raise ValueError(f"affine_matrix: three finite angles and one or three finite positive zooms expected, got {theta!r} and {zoom!r}")
    c, s = np.cos(t), np.sin(t)
    r0 = np.array([[1.0, 0.0, 0.0], [0.0, c[0], -s[0]], [0.0, s[0], c[0]]])
    r1 = np.array([[c[1], 0.0, s[1]], [0.0, 1.0, 0.0], [-s[1], 0.0, c[1]]])
    r2 = np.array([[c[2], -s[2], 0.0], [s[2], c[2], 0.0], [0.0, 0.0, 1.0]])
    return r0 @ r1 @ r2 @ np.diag(1.0 / z)


def _affine_arguments(affine_prob: float = 0.0, rotate_range=(0, 0, 0), zoom_range=(1.0, 1.0), zoom_isotropic: bool = True) -> tuple:
    """The affine keywords of ``draw_amos_params``, checked and in ``_draw_affine``'s order: the probability in [0, 1], three
    non-negative finite angles (one number means all three axes), ``0 < lo <= hi`` finite."""
    prob = float(affine_prob)
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"affine_prob {affine_prob!r} must be in [0, 1]")
    r = np.asarray(rotate_range, dtype=np.float64).reshape(-1)
    if r.size == 1:
        r = np.repeat(r, 3)
    if r.size != 3 or not np.isfinite(r).all() or (r < 0).any():
        raise ValueError(f"rotate_range {rotate_range!r} must be one or three non-negative finite angles (radians)")
    z = np.asarray(zoom_range, dtype=np.float64).reshape(-1)
    if z.size != 2 or not np.isfinite(z).all() or not 0.0 < z[0] <= z[1]:
        raise ValueError(f"zoom_range {zoom_range!r} must be (lo, hi) with 0 < lo <= hi")
    return prob, tuple(float(v) for v in r), (float(z[0]), float(z[1])), bool(zoom_isotropic)


def _draw_affine(rng, prob, rotate, zoom, isotropic) -> tuple:
    """Step 2a of ``draw_amos_params``: ``()`` for a sample without an affine, else the nine entries of ``M``, row-major."""
    if prob == 0 or not rng.rand() < prob:
        return ()
    theta = [rng.uniform(-rotate[a], rotate[a]) for a in range(3)]
    z = [rng.uniform(zoom[0], zoom[1]) for _ in range(1 if isotropic else 3)]
    return tuple(float(v) for v in affine_matrix(theta, z).reshape(-1))


def _affine_suffixes(who: str, params, base: int, expected: str) -> List[tuple]:
    """The affine suffix of every row, ``()`` or nine floats: a row has ``base`` values, or ``base + 9`` with a finite ``M`` whose
    entries are at most ``AFFINE_MAX_ENTRY`` in magnitude; anything else is a ``ValueError`` (``expected``: what the rows should be)."""
    out = []
    for j, row in enumerate(params):
        if len(row) == base:
            out.append(())
            continue
        if len(row) != base + 9:
            raise ValueError(f"{who}: {expected} ({base + 9} with an affine matrix); row {j} has {len(row)}")
        m = tuple(float(v) for v in row[base:])
        for e, v in enumerate(m):
            if not np.isfinite(v) or abs(v) > AFFINE_MAX_ENTRY:
                raise ValueError(f"{who}: parameter row {j}: affine matrix entry M[{e // 3}][{e % 3}] = {v} must be finite and at most "
                                 f"{AFFINE_MAX_ENTRY:g} in magnitude")
        out.append(m)
    return out


def _affine_block(suffixes: Sequence[tuple]):
    """``affine_params`` of one launch, ``[m][10]`` doubles = {flag, M row-major}, or None when no sample of it has an affine."""
    if not any(suffixes):
        return None
    flat = [v for m in suffixes for v in ((1.0, *m) if m else (0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0))]
    return (ctypes.c_double * len(flat))(*flat)
