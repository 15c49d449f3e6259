"""Case table, references and checks of the pooling / resize / depth-to-space family (csrc/kernels/pool_resize.h and its launchers in
csrc/icl_abi.inc), shared by test_resample_emu.py (CPU emulation of the kernel sources) and test_gpu_resample.py (the MI355X): both
files run every entry of ``CHECKS`` and nothing else, so nothing asserted in one is missing in the other.

References, all computed on the CPU and once per case (``resize_ref`` is cached, nothing mutates what it returns):
  resize        F.interpolate(x.double(), size, mode="trilinear", align_corners) and its autograd gradient
  max-pool      F.max_pool3d in fp32, BIT FOR BIT (values, NaN positions and where the gradient goes)
  k2s2 deconv   F.conv_transpose3d in fp64
  lazy forms    the same op on torch.relu(torch.addcmul(shift, x, scale)) materialised in fp32 (deferred InstanceNorm + ReLU)

Error measure: max|got - ref64| / max|ref64|.

Bound of a resize case: MARGIN * e_torch + floor.  e_torch is the same measure of torch's own fp32 CPU result of that case — measured
against the reference, never against the code under test.  MARGIN = 4 covers a different association of the same at most 8 products
(forward) and of the separable passes (backward).  floor = (t + 8) * 2**-24 with t the largest number of terms summed into one element
(8 forward; backward the product over the axes of the largest number of outputs that touch one input index, from the fp64 tap table):
e_torch is exactly 0 where every weight is dyadic (identity, size-1 axes) while the kernels add in another order.

Bound of a k2s2 transposed convolution (true fp32 MFMA products, fp32 accumulation): the textbook forward error of a K-term dot product
in any summation order, |err| <= (K + 2) * 2**-24 * sum|a||b|, with the sum of absolute products taken from an fp64 evaluation on
|x|, |w| (K = cin forward, 8 cout for the input gradient, n d h w for the weight gradient).

Every check also asserts WHICH kernel ran (icl_last_resample_route); the table states the route each row is there for, and
``check_routes_complete`` that the rows together reach all 4 forward routes, the one-pass backward and the 4 axis kernels.

`python tests/resample_ref.py [--gpu]` prints the measured errors of every tolerance-checked case (profiles/resample_parity.md)."""
import ctypes
import functools
import itertools
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from icl_amd import _lib, ops  # noqa: E402
from icl_amd.utils.hashfill import synthetic_volume  # noqa: E402

U = 2.0 ** -24
MARGIN = 4.0
N, C = 2, 3
GUARD = 64            # floats of sentinel in front of and behind every buffer handed to the C ABI (keeps 16-byte alignment)
SENTINEL = 1234.5
_vp = ctypes.c_void_p

FWD_X4, FWD_X2 = "upsample2x_fwd_x4_kernel", "upsample2x_fwd_kernel"
FWD_QUAD, FWD_SCALAR = "trilinear_fwd_quad_kernel", "trilinear_fwd_kernel"
BWD_ONE = "upsample2x_bwd_kernel"
AXIS = {"t4": "resize_bwd_axis_t4_kernel", "lds": "resize_bwd_axis_x_lds_kernel", "i4": "resize_bwd_axis_i4_kernel",
        "s": "resize_bwd_axis_kernel"}
REQUIRED_ROUTES = {FWD_X4, FWD_X2, FWD_QUAD, FWD_SCALAR, BWD_ONE, *AXIS.values()}

MEASURED = []         # (case id, what, e_kernel, e_torch, bound) of every tolerance-checked quantity, in the order the checks ran


def passes(x, y, z):
    return f"x:{AXIS[x]}|y:{AXIS[y]}|z:{AXIS[z]}"


def route():
    return (_lib.lib().icl_last_resample_route() or b"").decode()


def backward_route(outputs, grads, leaf):
    """Runs autograd's backward and returns the route record as the backward's own thread sees it: the record is per thread, and autograd
    runs the backward of device tensors on a thread of its own.  A hook on ``leaf`` (an input of the operator under test) runs there, right
    after the operator's backward."""
    seen = []
    h = leaf.register_hook(lambda g: seen.append(route()))
    torch.autograd.backward(outputs, grads)
    h.remove()
    assert len(seen) == 1
    return seen[0]


def place(t, dev, off4=False):
    """A copy of CPU tensor ``t`` on ``dev``; off4: as a contiguous view 4 bytes into a larger buffer (not 16-byte, not 8-byte aligned)."""
    if not off4:
        return t.detach().clone().to(dev)
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def guarded(numel, dev, fill=SENTINEL):
    """(flat buffer of GUARD + numel + GUARD floats filled with ``fill``, its 16-byte aligned middle)."""
    flat = torch.full((numel + 2 * GUARD,), fill, dtype=torch.float32, device=dev)
    mid = flat[GUARD:GUARD + numel]
    assert mid.data_ptr() % 16 == 0
    return flat, mid


def guards_intact(flat, fill=SENTINEL):
    f = flat.cpu()
    return bool((f[:GUARD] == fill).all()) and bool((f[-GUARD:] == fill).all())


def err(got, ref64):
    return float((got.detach().double().cpu() - ref64).abs().max()) / max(float(ref64.abs().max()), 1e-300)


def note(case, what, e_kernel, e_torch, bound):
    MEASURED.append((case, what, e_kernel, e_torch, bound))
    assert e_kernel <= bound, f"{case} {what}: e_kernel {e_kernel:.3e} > bound {bound:.3e} (e_torch {e_torch:.3e})"


# ---- the fp64 tap table of one axis (ATen's area_pixel_compute_source_index) and what the floor of a case needs from it ---------------------

def axis_taps(n_in, n_out, align):
    o = np.arange(n_out, dtype=np.float64)
    if align:
        src = ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0) * o
    else:
        src = np.maximum(n_in / n_out * (o + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0
    return i0, i1, 1.0 - l1, l1


def max_fan_in(n_in, n_out, align):
    """Largest number of output indices that contribute (non-zero weight) to one input index."""
    i0, i1, l0, l1 = axis_taps(n_in, n_out, align)
    cnt = np.zeros(n_in, dtype=np.int64)
    for o in range(n_out):
        for i in {int(i0[o])} | ({int(i1[o])} if l1[o] != 0.0 else set()):
            cnt[i] += 1
    return int(cnt.max())


def floors(ins, outs, align):
    t_bwd = math.prod(max_fan_in(i, o, align) for i, o in zip(ins, outs))
    return (8 + 8) * U, (t_bwd + 8) * U


class ResizeRef:
    pass


@functools.lru_cache(maxsize=None)
def resize_ref(ins, outs, align, n=N, c=C):
    r = ResizeRef()
    r.x = synthetic_volume((n, c) + tuple(ins), 15)
    r.gy = synthetic_volume((n, c) + tuple(outs), 16)
    x64 = r.x.double().requires_grad_()
    y64 = F.interpolate(x64, size=list(outs), mode="trilinear", align_corners=align)
    y64.backward(r.gy.double())
    r.y64, r.gx64 = y64.detach(), x64.grad
    x32 = r.x.clone().requires_grad_()
    y32 = F.interpolate(x32, size=list(outs), mode="trilinear", align_corners=align)
    y32.backward(r.gy)
    r.e_torch_fwd, r.e_torch_bwd = err(y32, r.y64), err(x32.grad, r.gx64)
    f_fwd, f_bwd = floors(ins, outs, align)
    r.bound_fwd, r.bound_bwd = MARGIN * r.e_torch_fwd + f_fwd, MARGIN * r.e_torch_bwd + f_bwd
    return r


# ---- the resize table ---------------------------------------------------------------------------------------------------------------------------
# (input extents, output extents, forward route and backward route with align_corners False, the same with True, what the row is there for)
GEN_I4 = passes("i4", "t4", "t4")
ALL_S = passes("s", "s", "s")
RESIZE_ROWS = [
    ((4, 6, 8), (8, 12, 16), FWD_X4, BWD_ONE, FWD_QUAD, GEN_I4, "exact 2x: x4 forward, one-pass backward, depth shorter than kUpSeg"),
    ((9, 5, 4), (18, 10, 8), FWD_X4, BWD_ONE, FWD_QUAD, GEN_I4, "exact 2x: one full depth segment plus one plane, odd height"),
    ((5, 3, 6), (10, 6, 12), FWD_X2, ALL_S, FWD_QUAD, ALL_S, "exact 2x with wi % 4 != 0: 2-wide forward, three-pass scalar backward"),
    ((3, 5, 3), (6, 10, 6), FWD_SCALAR, ALL_S, FWD_SCALAR, ALL_S, "exact 2x, odd width: scalar forward"),
    ((4, 5, 5), (17, 17, 20), FWD_QUAD, passes("lds", "s", "s"), FWD_QUAD, passes("lds", "s", "s"),
     "x pass through LDS staging: rows * li = 867 * 5 >= 4096, 2 * 867 rows are 54 row blocks of 32 and a ragged one of 6"),
    ((6, 4, 8), (9, 7, 12), FWD_QUAD, GEN_I4, FWD_QUAD, GEN_I4, "quad forward; x pass i4; y and z passes t4"),
    ((2, 2, 4), (4, 40, 8), FWD_QUAD, GEN_I4, FWD_QUAD, GEN_I4, "y pass t4 with more than 8 taps per input, a count that is no multiple of 8"),
    ((12, 10, 16), (5, 4, 6), FWD_SCALAR, GEN_I4, FWD_SCALAR, GEN_I4, "downscale: scalar forward, i4 x pass with rscale > 1"),
    ((9, 7, 11), (4, 7, 23), FWD_SCALAR, ALL_S, FWD_SCALAR, ALL_S, "mixed down / identity / up axes: all scalar"),
    ((8, 8, 8), (1, 1, 1), FWD_SCALAR, GEN_I4, FWD_SCALAR, GEN_I4, "size-1 outputs (rscale == 0 under align_corners)"),
    ((1, 1, 1), (4, 6, 8), FWD_QUAD, ALL_S, FWD_QUAD, ALL_S, "size-1 inputs"),
    ((5, 6, 7), (5, 6, 7), FWD_SCALAR, ALL_S, FWD_SCALAR, ALL_S, "identity"),
]
# the first row with x (forward) and gy (backward) 4 bytes into a larger buffer: the misaligned fall-backs
MISALIGNED_ROW = ((4, 6, 8), (8, 12, 16), FWD_X2, GEN_I4, FWD_QUAD, GEN_I4, "first row, x and gy at a 4-byte offset")


def _shape_id(ins, outs):
    return "x".join(map(str, ins)) + "->" + "x".join(map(str, outs))


def check_resize(dev, row, align, off4=False):
    ins, outs = row[0], row[1]
    want_fwd, want_bwd = (row[4], row[5]) if align else (row[2], row[3])
    case = f"{_shape_id(ins, outs)} ac={int(align)}" + (" +4B" if off4 else "")
    r = resize_ref(ins, outs, align, N, C)
    x = place(r.x, dev, off4).requires_grad_()
    y = ops.trilinear_resize(x, outs, align_corners=align)
    assert route() == want_fwd, (case, route())
    note(case, "fwd", err(y, r.y64), r.e_torch_fwd, r.bound_fwd)
    got_bwd = backward_route([y], [place(r.gy, dev, off4)], x)
    assert got_bwd == want_bwd, (case, got_bwd)
    note(case, "bwd", err(x.grad, r.gx64), r.e_torch_bwd, r.bound_bwd)


def check_routes_complete(dev=None):
    """The routes the table states (each asserted against icl_last_resample_route by its row) cover every kernel of section 2."""
    named = set()
    for row in RESIZE_ROWS + [MISALIGNED_ROW]:
        for s in row[2:6]:
            named |= {p.split(":")[-1] for p in s.split("|")}
    assert named >= REQUIRED_ROUTES, sorted(REQUIRED_ROUTES - named)
    assert any(row[2] == FWD_X4 and row[3] == BWD_ONE for row in RESIZE_ROWS)
    assert all(row[4] in (FWD_QUAD, FWD_SCALAR) and row[5] != BWD_ONE for row in RESIZE_ROWS)      # align_corners: the generic kernels


# ---- strided forms through the C ABI: the forward writes, the backward reads, a channel slice of a concat buffer -------------------------------
# (inputs, outputs, align, leading channels, channels, forward route, backward route, what)
STRIDED_ROWS = [
    ((4, 6, 8), (8, 12, 16), False, 2, 3, FWD_X4, BWD_ONE, "bstride = (2 + c) S, S % 4 == 0: the exact-2x kernels on a slice"),
    ((6, 4, 8), (9, 7, 12), True, 2, 3, FWD_QUAD, GEN_I4, "bstride = (2 + c) S, S % 4 == 0: quad forward, i4 / t4 backward"),
    ((4, 5, 5), (17, 17, 20), False, 2, 3, FWD_QUAD, passes("lds", "s", "s"), "LDS-staged x pass reading a batch-strided slice"),
    ((2, 3, 3), (3, 5, 7), False, 1, 2, FWD_SCALAR, ALL_S, "bstride = 3 * 105, slice 105 floats in: neither a multiple of 4, all scalar"),
    ((2, 3, 4), (3, 5, 7), True, 1, 2, FWD_SCALAR, GEN_I4, "the same odd stride into the i4 x pass (scalar loads of gy, aligned workspace)"),
]


def check_strided(dev, row):
    ins, outs, align, lead, c, want_fwd, want_bwd, _ = row
    case = f"{_shape_id(ins, outs)} ac={int(align)} slice {lead}+{c}"
    L = _lib.lib()
    n = N
    r = resize_ref(ins, outs, align, n, c)
    s_out, s_in = math.prod(outs), math.prod(ins)
    bs = (lead + c) * s_out
    # forward into the slice [:, lead:] of a sentinel-filled buffer
    flat, mid = guarded(n * bs, dev)
    buf = mid.view(n, lead + c, *outs)
    x = place(r.x, dev)
    _lib.check(L.icl_trilinear_fwd(_vp(x.data_ptr()), _vp(buf[:, lead:].data_ptr()), n, c, *ins, *outs, bs, int(align), ops._stream(x)),
               "trilinear_fwd")
    assert route() == want_fwd, (case, route())
    note(case, "fwd", err(buf[:, lead:], r.y64), r.e_torch_fwd, r.bound_fwd)
    assert bool((buf[:, :lead].cpu() == SENTINEL).all()) and guards_intact(flat), case
    # backward out of the slice of a buffer that holds NaN everywhere else; gx and the workspace between guards
    gflat, gmid = guarded(n * bs, dev, float("nan"))
    gbuf = gmid.view(n, lead + c, *outs)
    gbuf[:, lead:] = r.gy.to(dev)
    xflat, xmid = guarded(n * c * s_in, dev)
    ws_floats = L.icl_trilinear_bwd_ws_bytes(n, c, *ins, *outs) // 4
    wflat, wmid = guarded(max(ws_floats, 4), dev)
    _lib.check(L.icl_trilinear_bwd(_vp(gbuf[:, lead:].data_ptr()), _vp(xmid.data_ptr()), _vp(wmid.data_ptr()), n, c, *ins, *outs, bs,
                                   int(align), ops._stream(x)), "trilinear_bwd")
    assert route() == want_bwd, (case, route())
    note(case, "bwd", err(xmid.view(n, c, *ins), r.gx64), r.e_torch_bwd, r.bound_bwd)
    assert guards_intact(xflat) and guards_intact(wflat), case


# ---- max-pool: bit for bit against torch, NaN and the gradient's target included -------------------------------------------------------------
POOL_X2, POOL_SCALAR = "maxpool2_fwd_x2_kernel", "maxpool2_fwd_kernel"
POOL_SHAPES = {                      # name: (shape, x at a 4-byte offset, forward route)
    "w8": ((2, 3, 4, 6, 8), False, POOL_X2),         # pooled width 4: two windows per thread
    "w6": ((2, 3, 4, 6, 6), False, POOL_SCALAR),     # pooled width 3
    "w8+4B": ((2, 3, 4, 6, 8), True, POOL_SCALAR),   # rows that are not 16-byte aligned
}
SLOT_PAIRS = list(itertools.combinations(range(8), 2))
POOL_FILLS = ["plain", "relu", "constant", "neg_inf"] + [f"nan{k}" for k in range(8)] + ["nan_pairs"]


def pool_input(shape, fill):
    """Hash-filled volume edited per 2x2x2 window; slot k of a window is (dz, dy, dx) = (k >> 2, (k >> 1) & 1, k & 1), the kernels' scan order."""
    n, c, d, h, w = shape
    x = synthetic_volume(shape, 13)
    wins = x.view(n * c, d // 2, 2, h // 2, 2, w // 2, 2).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, 8).clone()
    nw = wins.shape[0]
    nan = float("nan")
    if fill == "relu":
        wins = torch.relu(wins)                      # exact-zero ties
    elif fill == "constant":
        wins[::5] = 0.375                            # every slot of a window equal: the first wins
        wins[2::5] = 0.0
    elif fill == "neg_inf":
        wins[::7] = -float("inf")                    # nothing exceeds the start value: index 0, value -inf
        wins[3::7, :5] = -float("inf")
        wins[5::7, 1:] = -float("inf")
    elif fill.startswith("nan") and fill != "nan_pairs":
        k = int(fill[3:])
        wins[k::5, k] = nan                          # a stride of 5 meets every pooled x of a row of 4 or 3
    elif fill == "nan_pairs":
        assert nw > 3 * len(SLOT_PAIRS)
        for j, (a, b) in enumerate(SLOT_PAIRS):      # the LAST NaN in scan order takes the gradient
            wins[3 * j + 1, a] = nan
            wins[3 * j + 1, b] = nan
        wins[nw - 1] = nan
        wins[nw - 2, :7] = nan
    return wins.view(n * c, d // 2, h // 2, w // 2, 2, 2, 2).permute(0, 1, 4, 2, 5, 3, 6).reshape(shape).contiguous()


def same_bits_as_torch(got, want, what):
    got = got.detach().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaN positions differ ({int(torch.isnan(got).sum())} vs {int(torch.isnan(want).sum())})"
    assert torch.equal(torch.isinf(got), torch.isinf(want)), f"{what}: inf positions differ"
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want)), f"{what}: values differ"


def check_pool(dev, shape_name, fill):
    shape, off4, want = POOL_SHAPES[shape_name]
    xc = pool_input(shape, fill)
    x = place(xc, dev, off4).requires_grad_()
    y = ops.max_pool3d_2(x)
    assert route() == want, route()
    gyc = synthetic_volume(tuple(y.shape), 14)
    got_bwd = backward_route([y], [place(gyc, dev)], x)
    assert got_bwd == "maxpool2_bwd_kernel", got_bwd
    xr = xc.clone().requires_grad_()
    yr = F.max_pool3d(xr, 2)
    yr.backward(gyc)
    same_bits_as_torch(y, yr.detach(), "pooled")
    same_bits_as_torch(x.grad, xr.grad, "gradient")


def check_skip_and_pool(dev, w):
    """ops.skip_and_pool with the skip gradient a batch-strided channel slice of a concat gradient; ReLU-ed input (ties)."""
    xc = torch.relu(synthetic_volume((2, 3, 4, 6, w), 31))
    x = place(xc, dev).requires_grad_()
    skip, y = ops.skip_and_pool(x)
    assert route() == (POOL_X2 if w % 4 == 0 else POOL_SCALAR), route()
    gskc = synthetic_volume((2, 5, 4, 6, w), 32)
    gyc = synthetic_volume(tuple(y.shape), 33)
    got_bwd = backward_route([skip, y], [place(gskc, dev)[:, :3], place(gyc, dev)], x)
    assert got_bwd == ("maxpool2_bwd_add_x2_kernel" if w % 4 == 0 else "maxpool2_bwd_add_kernel"), got_bwd
    xr = xc.clone().requires_grad_()
    yr = F.max_pool3d(xr, 2)
    torch.autograd.backward([xr * 1.0, yr], [gskc[:, :3], gyc])
    same_bits_as_torch(y, yr.detach(), "pooled")
    same_bits_as_torch(x.grad, xr.grad, "gradient")


def check_pool_bwd_add_live(dev, w):
    """icl_maxpool2_bwd_add_live, n = 3, skip_live = 1: 9 planes of 24 (18) pooled outputs are ONE workgroup, whose threads below plane 3
    add the skip gradient and whose others must not load it: the addend's tail (and everything outside its channel slice) is NaN."""
    L = _lib.lib()
    n, c, live, lead = 3, 3, 1, 2
    d, h = 4, 6
    do, ho, wo = d // 2, h // 2, w // 2
    xc = torch.relu(synthetic_volume((n, c, d, h, w), 41))
    gyc = synthetic_volume((n, c, do, ho, wo), 42)
    addc = torch.full((n, lead + c, d, h, w), float("nan"))
    addc[:live, lead:] = synthetic_volume((live, c, d, h, w), 43)
    x, gy, add = place(xc, dev), place(gyc, dev), place(addc, dev)
    y = torch.empty((n, c, do, ho, wo), dtype=torch.float32, device=dev)
    idx = torch.empty(y.shape, dtype=torch.uint8, device=dev)
    st = ops._stream(x)
    _lib.check(L.icl_maxpool2_fwd(_vp(x.data_ptr()), _vp(y.data_ptr()), _vp(idx.data_ptr()), n * c, do, ho, wo, 2, st), "maxpool2_fwd")
    flat, mid = guarded(xc.numel(), dev)
    _lib.check(L.icl_maxpool2_bwd_add_live(_vp(gy.data_ptr()), _vp(idx.data_ptr()), _vp(add[:, lead:].data_ptr()), _vp(mid.data_ptr()), n, live,
                                           c, do, ho, wo, 2, add.stride(0), st), "maxpool2_bwd_add_live")
    assert route() == ("maxpool2_bwd_add_x2_kernel" if wo % 2 == 0 else "maxpool2_bwd_add_kernel"), route()
    assert (n * c * do * ho * wo) // (2 if wo % 2 == 0 else 1) <= 256      # one workgroup holds the boundary
    xr = xc.clone().requires_grad_()
    F.max_pool3d(xr, 2).backward(gyc)
    want = xr.grad.clone()
    want[:live] += addc[:live, lead:]
    same_bits_as_torch(mid.view(n, c, d, h, w), want, "gradient")
    assert not bool(torch.isnan(mid).any()) and guards_intact(flat)


def dyadic_ss(n, c, seed):
    """(scale, shift) pairs whose scale is a power of two: x * scale is exact, so the kernels' fma and torch's addcmul round once, alike."""
    scale = torch.tensor([0.5, 1.0, 2.0, 0.25])[torch.arange(n * c) % 4]
    shift = 0.3 * synthetic_volume((n * c,), seed)
    return torch.stack([scale, shift], 1).contiguous()


def materialise(t, ss):
    n, c = t.shape[:2]
    return torch.relu(torch.addcmul(ss[:, 1].view(n, c, 1, 1, 1), t, ss[:, 0].view(n, c, 1, 1, 1)))


def check_pool_norm(dev, w):
    """icl_maxpool2_fwd_norm (through ops.skip_and_pool on a LazyAct): pooling of relu(fma(t, scale, shift)) applied on load, against
    F.max_pool3d of the materialised tensor, forward and where the gradient goes."""
    tc = synthetic_volume((2, 3, 4, 6, w), 51)
    ssc = dyadic_ss(2, 3, 52)
    t = place(tc, dev).requires_grad_()
    _, y = ops.skip_and_pool(ops.LazyAct(t, place(ssc, dev)))
    assert route() == (POOL_X2 if w % 4 == 0 else POOL_SCALAR), route()
    gyc = synthetic_volume(tuple(y.shape), 53)
    # (autograd hands the unused skip output a zero gradient: the backward is the fused add, 0 + g)
    got_bwd = backward_route([y], [place(gyc, dev)], t)
    assert got_bwd == ("maxpool2_bwd_add_x2_kernel" if w % 4 == 0 else "maxpool2_bwd_add_kernel"), got_bwd
    m = materialise(tc, ssc).requires_grad_()
    yr = F.max_pool3d(m, 2)
    yr.backward(gyc)
    assert float((m == 0).float().mean()) > 0.1      # the ReLU made ties
    same_bits_as_torch(y, yr.detach(), "pooled")
    same_bits_as_torch(t.grad, m.grad, "gradient")


# ---- upsample2x_concat, either or both sources lazy ---------------------------------------------------------------------------------------------

def check_upsample_concat(dev, w, skip_lazy, deep_lazy):
    n, cs, cd, d, h = 2, 3, 5, 4, 6
    case = f"upcat w={w} lazy=({int(skip_lazy)},{int(deep_lazy)})"
    skc, dpc = synthetic_volume((n, cs, d, h, w), 17), synthetic_volume((n, cd, d // 2, h // 2, w // 2), 18)
    sssc, dssc = torch.stack([0.5 + 0.1 * synthetic_volume((n * cs,), 61).abs(), 0.2 * synthetic_volume((n * cs,), 62)], 1).contiguous(), \
        torch.stack([0.5 + 0.1 * synthetic_volume((n * cd,), 63).abs(), 0.2 * synthetic_volume((n * cd,), 64)], 1).contiguous()
    gyc = synthetic_volume((n, cs + cd, d, h, w), 19)
    sk, dp = place(skc, dev).requires_grad_(), place(dpc, dev).requires_grad_()
    y = ops.upsample2x_concat(ops.LazyAct(sk, place(sssc, dev)) if skip_lazy else sk, ops.LazyAct(dp, place(dssc, dev)) if deep_lazy else dp)
    up = FWD_X4 if (w // 2) % 4 == 0 else FWD_X2
    if skip_lazy or deep_lazy:
        assert route() == ("copy_rows_norm_kernel" if skip_lazy else "copy_rows_kernel") + "|" + up, route()
    else:
        assert route() == up, route()
    got_bwd = backward_route([y], [place(gyc, dev)], dp)
    assert got_bwd == (BWD_ONE if (w // 2) % 4 == 0 else ALL_S), got_bwd
    # the materialised composition: fp64 reference, torch's fp32 for e_torch
    skm = (materialise(skc, sssc) if skip_lazy else skc)
    dpm = (materialise(dpc, dssc) if deep_lazy else dpc)
    res = []
    for dt in (torch.float64, torch.float32):
        a, b = skm.to(dt).requires_grad_(), dpm.to(dt).requires_grad_()
        yr = torch.cat([a, F.interpolate(b, size=[d, h, w], mode="trilinear", align_corners=False)], 1)
        yr.backward(gyc.to(dt))
        res.append((yr.detach(), a.grad, b.grad))
    (y64, gs64, gd64), (y32, _, gd32) = res
    f_fwd, f_bwd = floors((d // 2, h // 2, w // 2), (d, h, w), False)
    e_t = err(y32, y64)
    note(case, "fwd", err(y, y64), e_t, MARGIN * e_t + f_fwd)
    e_t = err(gd32, gd64)
    note(case, "bwd deep", err(dp.grad, gd64), e_t, MARGIN * e_t + f_bwd)
    assert torch.equal(sk.grad.cpu(), gs64.float()), case      # the skip gradient is a slice of gy


# ---- ConvTranspose3d(kernel 2, stride 2) as a product + depth_to_space2 / space_to_depth2 --------------------------------------------------------

def max_dyn_lds():
    """kMaxDynLds of csrc/icl_abi.inc: the dynamic-LDS size above which a launcher raises the kernel's limit."""
    import re
    src = open(os.path.join(ROOT, "icl_amd", "csrc", "icl_abi.inc")).read()
    m = re.search(r"constexpr int kMaxDynLds = (\d+) \* 1024;", src)
    return int(m.group(1)) * 1024


def check_conv_transpose(dev, n, cin, dims, cout, cs, big):
    d, h, w = dims
    case = f"deconv {n}x{cin}x{d}x{h}x{w}->{cout}" + (f" +skip{cs}" if cs else "")
    lds = w * (cout * 8 + 2) * 4
    assert (lds > max_dyn_lds()) == big, (lds, max_dyn_lds())
    xc = synthetic_volume((n, cin, d, h, w), 14)
    wc = synthetic_volume((cin, cout, 2, 2, 2), 15) * 0.3
    skc = synthetic_volume((n, cs, 2 * d, 2 * h, 2 * w), 16) if cs else None
    gyc = synthetic_volume((n, cout + cs, 2 * d, 2 * h, 2 * w), 17)
    x, wt = place(xc, dev).requires_grad_(), place(wc, dev).requires_grad_()
    sk = place(skc, dev).requires_grad_() if cs else None
    y = ops.conv_transpose3d_k2s2(x, wt, sk)
    tag = "+big_lds" if big else "+lds"
    assert route() == "depth_to_space2_kernel" + tag, route()
    got_bwd = backward_route([y], [place(gyc, dev)], x)
    assert got_bwd == "space_to_depth2_kernel" + tag, got_bwd
    xr, wr = xc.double().requires_grad_(), wc.double().requires_grad_()
    yr = F.conv_transpose3d(xr, wr, stride=2)
    yr.backward(gyc[:, :cout].double())
    xa, wa = xc.double().abs().requires_grad_(), wc.double().abs().requires_grad_()
    ya = F.conv_transpose3d(xa, wa, stride=2)
    ya.backward(gyc[:, :cout].double().abs())
    for what, got, ref, mag, k in (("fwd", y[:, :cout], yr.detach(), ya.detach(), cin), ("bwd x", x.grad, xr.grad, xa.grad, 8 * cout),
                                   ("bwd w", wt.grad, wr.grad, wa.grad, n * d * h * w)):
        scale = float(ref.abs().max())
        note(case, what, err(got, ref), 0.0, (k + 2) * U * float(mag.abs().max()) / scale)
    if cs:
        assert torch.equal(y[:, cout:].detach().cpu(), skc) and torch.equal(sk.grad.cpu(), gyc[:, cout:]), case


# ---- the batch-split gradient (concat2_kernel), each half null in turn ---------------------------------------------------------------------------

def check_split_batch(dev, use):
    xc = synthetic_volume((3, 2, 4, 2, 6), 91)
    x = place(xc, dev).requires_grad_()
    a, b = ops.split_batch(x, 1)
    gac, gbc = synthetic_volume(tuple(a.shape), 92), synthetic_volume(tuple(b.shape), 93)
    if use == "first":
        loss = (a * place(gac, dev)).sum()
    elif use == "second":
        loss = (b * place(gbc, dev)).sum()
    else:
        loss = (a * place(gac, dev)).sum() + (b * place(gbc, dev)).sum()
    loss.backward()
    want = torch.cat([gac if use != "second" else torch.zeros_like(gac), gbc if use != "first" else torch.zeros_like(gbc)], 0)
    assert torch.equal(x.grad.cpu(), want)


# ---- every check, by id -----------------------------------------------------------------------------------------------------------------------------

def _checks():
    out = {"routes_complete": check_routes_complete}
    for row in RESIZE_ROWS:
        for align in (False, True):
            out[f"resize[{_shape_id(row[0], row[1])},ac={int(align)}]"] = functools.partial(check_resize, row=row, align=align)
    for align in (False, True):
        out[f"resize[{_shape_id(*MISALIGNED_ROW[:2])},ac={int(align)},+4B]"] = functools.partial(check_resize, row=MISALIGNED_ROW, align=align, off4=True)
    for row in STRIDED_ROWS:
        out[f"strided[{_shape_id(row[0], row[1])},ac={int(row[2])},{row[3]}+{row[4]}]"] = functools.partial(check_strided, row=row)
    for shape_name in POOL_SHAPES:
        for fill in POOL_FILLS:
            out[f"pool[{shape_name},{fill}]"] = functools.partial(check_pool, shape_name=shape_name, fill=fill)
    for w in (8, 6):
        out[f"skip_and_pool[w={w}]"] = functools.partial(check_skip_and_pool, w=w)
        out[f"pool_bwd_add_live[w={w}]"] = functools.partial(check_pool_bwd_add_live, w=w)
        out[f"pool_norm[w={w}]"] = functools.partial(check_pool_norm, w=w)
    for w in (8, 12):
        for sl, dl in ((False, False), (True, False), (False, True), (True, True)):
            out[f"upsample2x_concat[w={w},lazy={int(sl)}{int(dl)}]"] = functools.partial(check_upsample_concat, w=w, skip_lazy=sl, deep_lazy=dl)
    out["conv_transpose[2x5x3x4x5->3]"] = functools.partial(check_conv_transpose, n=2, cin=5, dims=(3, 4, 5), cout=3, cs=0, big=False)
    out["conv_transpose[2x5x3x4x5->3,skip]"] = functools.partial(check_conv_transpose, n=2, cin=5, dims=(3, 4, 5), cout=3, cs=2, big=False)
    out["conv_transpose[1x4x2x2x24->96,big_lds]"] = functools.partial(check_conv_transpose, n=1, cin=4, dims=(2, 2, 24), cout=96, cs=0, big=True)
    for use in ("both", "first", "second"):
        out[f"split_batch[{use}]"] = functools.partial(check_split_batch, use=use)
    return out


CHECKS = _checks()


def report(dev):
    for name, fn in CHECKS.items():
        fn(dev)
    lines = ["| case | what | e_kernel | e_torch | bound | e_kernel / bound |", "|---|---|---|---|---|---|"]
    for case, what, ek, et, b in MEASURED:
        lines.append(f"| `{case}` | {what} | {ek:.2e} | {et:.2e} | {b:.2e} | {ek / b:.2f} |")
    return "\n".join(lines)


if __name__ == "__main__":
    if "--gpu" in sys.argv:
        print(report(torch.device("cuda", 0)))
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
        from build_emu import build_emu
        _lib._use_library_for_tests(build_emu(), host_pointers=True)
        print(report("cpu"))
