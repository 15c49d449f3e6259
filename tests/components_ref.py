"""Cases and the scipy reference of the connected-component kernels (icl_amd/csrc/kernels/components.h), shared by
test_components_emu.py, test_components_host.py and test_gpu_components.py.  Every comparison is exact.

For a map, class c and connectivity k the reference is ``scipy.ndimage.label(map == c, generate_binary_structure(3, k))``.

Extents follow the kernels' tile (8 x 8 x 16 along axes 0, 1, 2): 2 T + 3 = 19 x 19 x 35 gives three tiles per axis with a ragged last
one, and no axis is longer than 64."""
import numpy as np
from scipy import ndimage

TILE = (8, 8, 16)
SHAPE = tuple(2 * t + 3 for t in TILE)      # (19, 19, 35)
CONNECTIVITIES = (1, 2, 3)


def structure(k):
    return ndimage.generate_binary_structure(3, k)


def squeeze3(m):
    """The 3-D map behind leading axes of length 1."""
    m = np.asarray(m)
    assert m.ndim >= 3 and all(s == 1 for s in m.shape[:-3])
    return m.reshape(m.shape[-3:])


class ClassReference:
    """scipy's components of ``map == c``: lab, n, sizes [n], first [n] (raster index of each component's first voxel)."""

    def __init__(self, m3, c, k):
        self.mask = m3 == c
        self.lab, self.n = ndimage.label(self.mask, structure(k))
        flat = self.lab.ravel()
        idx = np.nonzero(flat)[0]
        first = np.full(self.n + 1, flat.size, dtype=np.int64)
        np.minimum.at(first, flat[idx], idx)
        self.first = first[1:]
        self.sizes = np.bincount(flat, minlength=self.n + 1)[1:]
        # scipy numbers the components in raster order of their first voxel: np.argmax over its sizes is "the largest, the first among equals"
        assert np.all(np.diff(self.first) > 0)

    def expected_labels(self):
        out = np.zeros(self.lab.shape, dtype=np.int64)
        if self.n:
            out[self.mask] = self.first[self.lab[self.mask] - 1] + 1
        return out

    def record(self):
        if self.n == 0:
            return [0, 0, 0]
        big = int(np.argmax(self.sizes))
        return [self.n, int(self.sizes[big]), int(self.first[big]) + 1]


def check_labels(m, labels, counts, nc, k):
    """labels / counts (numpy) of ``ops.seg_components(m, nc, k)`` against scipy."""
    m3 = squeeze3(m).astype(np.int64)
    labels = np.asarray(labels)
    assert labels.dtype == np.int32 and labels.shape == np.asarray(m).shape
    l3 = squeeze3(labels).astype(np.int64)
    counts = np.asarray(counts)
    assert counts.shape == (nc - 1, 3) and counts.dtype == np.int64
    fg = (m3 >= 1) & (m3 < nc)
    assert np.all(l3[~fg] == 0)                       # background is 0
    assert np.all(l3[fg] > 0)
    for c in range(1, nc):
        ref = ClassReference(m3, c, k)
        dev, sci = l3[ref.mask], ref.lab[ref.mask]
        pairs = np.unique(dev * (ref.n + 1) + sci)      # the (device label, scipy label) pairs that occur
        assert len(pairs) == ref.n == len(np.unique(dev)) == len(np.unique(sci)), (c, k)      # a bijection
        assert np.array_equal(l3[ref.mask], ref.expected_labels()[ref.mask]), (c, k)      # label - 1 = the first voxel's raster index
        assert counts[c - 1].tolist() == ref.record(), (c, k, counts[c - 1].tolist(), ref.record())


def keep_reference(m, nc, k, keep_largest=True, min_size=0):
    """The filtered map, restated on scipy: the map's shape and dtype."""
    m = np.asarray(m)
    m3 = squeeze3(m).astype(np.int64)
    out = np.zeros(m3.shape, dtype=np.int64)
    for c in range(1, nc):
        ref = ClassReference(m3, c, k)
        if ref.n == 0:
            continue
        keep = ref.sizes >= min_size
        if keep_largest:
            only = np.zeros(ref.n, dtype=bool)
            only[int(np.argmax(ref.sizes))] = True
            keep &= only
        sel = ref.mask.copy()
        sel[ref.mask] = keep[ref.lab[ref.mask] - 1]
        out[sel] = c
    return out.reshape(m.shape).astype(m.dtype)


def check_filter(m, out, nc, k, keep_largest=True, min_size=0):
    out = np.asarray(out)
    want = keep_reference(m, nc, k, keep_largest, min_size)
    assert out.dtype == want.dtype and out.shape == want.shape
    assert np.array_equal(out, want), (nc, k, keep_largest, min_size)


# ---------------------------------------------------------------------------------------------------------------- cases: () -> (map, nc)

def serpentine():
    """One class-1 path, one voxel wide: rows along axis 2 on the even (axis 0, axis 1) lines, joined at alternating ends, the planes joined at
    alternating corners.  It crosses every tile face many times; it starts in the first tile and ends in the last."""
    n0, n1, n2 = SHAPE
    m = np.zeros(SHAPE, dtype=np.uint8)
    rows = list(range(0, n1, 2))
    for a in range(0, n0, 2):
        for r, b in enumerate(rows):
            m[a, b, :] = 1
            if r + 1 < len(rows):
                m[a, b + 1, n2 - 1 if r % 2 == 0 else 0] = 1
    end = (rows[-1], n2 - 1 if (len(rows) - 1) % 2 == 0 else 0)
    for g, a in enumerate(range(1, n0 - 1, 2)):
        b, c = end if g % 2 == 0 else (0, 0)
        m[a, b, c] = 1
    assert ndimage.label(m, structure(1))[1] == 1
    return m, 2


def checkerboard():
    i, j, k = np.indices(SHAPE)
    return ((i + j + k) % 2).astype(np.uint8), 2


def corner_and_edge():
    """Class 1: two blobs that touch only at the tile corner (8, 8, 16) — one component under connectivity 3 only; class 2: two that touch
    only across the tile edge (16, 16, .) — one component under connectivity 2 and 3."""
    m = np.zeros(SHAPE, dtype=np.uint8)
    m[6:8, 6:8, 14:16] = 1
    m[8:10, 8:10, 16:18] = 1
    m[14:16, 14:16, 4:6] = 2
    m[16:18, 16:18, 4:6] = 2
    return m, 3


def two_classes_face_to_face():
    m = np.ones(SHAPE, dtype=np.uint8)
    m[TILE[0]:] = 2
    return m, 3


def one_class():
    return np.ones(SHAPE, dtype=np.uint8), 2


def all_background():
    return np.zeros(SHAPE, dtype=np.uint8), 3


def _random(shape, nc, density, seed, dtype=np.uint8):
    rng = np.random.default_rng(seed)
    m = rng.integers(1, nc, size=shape) * (rng.random(shape) < density)
    return m.astype(dtype), nc


def line(axis):
    shape = [1, 1, 1]
    shape[axis] = SHAPE[2]
    return _random(tuple(shape), 3, 0.7, 40 + axis)


def ties(axis):
    shape = [1, 1, 1]
    shape[axis] = 5
    return np.array([1, 1, 0, 1, 1], dtype=np.uint8).reshape(shape), 2


def out_of_range_int64():
    m, nc = _random(SHAPE, 4, 0.6, 7, np.int64)
    rng = np.random.default_rng(8)
    r = rng.random(SHAPE)
    m[r < 0.1] = -3
    m[(r >= 0.1) & (r < 0.2)] = nc
    m[(r >= 0.2) & (r < 0.25)] = 2 ** 40 + 1      # low byte 1: not class 1
    return m, nc


def out_of_range_uint8():
    m, nc = _random(SHAPE, 4, 0.6, 9)
    rng = np.random.default_rng(10)
    r = rng.random(SHAPE)
    m[r < 0.15] = nc
    m[(r >= 0.15) & (r < 0.3)] = 255
    return m, nc


CASES = {
    "serpentine": serpentine,
    "checkerboard": checkerboard,
    "corner_and_edge": corner_and_edge,
    "two_classes_face_to_face": two_classes_face_to_face,
    "one_class": one_class,
    "all_background": all_background,
    "line_axis2": lambda: line(2),
    "line_axis1": lambda: line(1),
    "line_axis0": lambda: line(0),
    "ties_axis0": lambda: ties(0),
    "ties_axis1": lambda: ties(1),
    "ties_axis2": lambda: ties(2),
    "out_of_range_int64": out_of_range_int64,
    "out_of_range_uint8": out_of_range_uint8,
    "bool_map": lambda: (_random(SHAPE, 2, 0.5, 11)[0].astype(np.bool_), 2),
    "int64_map": lambda: _random(SHAPE, 4, 0.5, 12, np.int64),
    "leading_axis": lambda: (_random(SHAPE, 3, 0.4, 13, np.int64)[0][None], 3),
}
for _nc in (2, 4, 17):
    for _d in (0.2, 0.5, 0.8):
        CASES[f"random_nc{_nc}_d{int(_d * 10)}"] = (lambda nc=_nc, d=_d: _random(SHAPE, nc, d, 100 * nc + int(d * 10)))


def filter_settings(m, nc, k):
    """(keep_largest, min_size) pairs for a case: the defaults, no keep-largest with a threshold at exactly a component's size and one above
    it, and keep-largest with a threshold above the largest (the class vanishes)."""
    m3 = squeeze3(m).astype(np.int64)
    sizes = [ClassReference(m3, c, k).sizes for c in range(1, nc)]
    sizes = np.concatenate(sizes) if sizes else np.zeros(0, dtype=np.int64)
    s = int(np.sort(sizes)[len(sizes) // 2]) if len(sizes) else 1      # a size that occurs
    big = int(sizes.max()) if len(sizes) else 1
    return [(True, 0), (False, s), (False, s + 1), (True, big + 1), (True, big), (False, 0)]
