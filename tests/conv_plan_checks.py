"""Checks of the forward convolution planner shared by the emulation suite (CPU tensors) and the device suite.

`check_pointer_fallbacks`: what a split-product launch decides from its POINTERS once the plan is made — with and without a slab
workspace, a y that is not 16-byte aligned, statistics asked where the plan wants a split.  n = 1, 32 -> 32 channels, the smallest volume
of each tile form; ICL_CONV_SPLIT_MIN=1 admits it and ICL_CONV_SPLIT_KSPLIT=2 makes the plan want two slices.  The return codes and kernel
names are those of the commit before the planner (run once on it, emulation and MI355X).  Where a kernel runs its result is compared with
torch's convolution, in the tolerance tests/test_kernels_emu.py has for the split-product kernels.

`launch_record`: the kernels, grids and output checksums of one layer shape at batch 2 (tests/test_gpu_conv_plan.py).
"""
import ctypes

import torch
import torch.nn.functional as F

from icl_amd import _lib, ops
from icl_amd.ops import _ptr, _stream
from icl_amd.utils.hashfill import hash_uniform_torch, synthetic_volume

# (cin, cout, cube edge): the layers of the U-Net and SwinUNETR decoders at batch 2, and two ragged ones
SHAPES = [(16, 16, 96), (32, 16, 96), (48, 16, 96), (48, 48, 96), (1, 16, 96),
          (16, 32, 48), (32, 32, 48), (96, 32, 48),
          (32, 64, 24), (64, 64, 24), (192, 64, 24), (64, 32, 24),
          (64, 128, 12), (128, 128, 12), (384, 128, 12), (128, 384, 12), (128, 64, 12),
          (128, 256, 6), (256, 256, 6), (256, 128, 6),
          (20, 24, 24), (16, 16, 20)]

# (d, h, w): (kernel with a slab, rc without one) — rows of 24 run unsplit without a slab, the other two exist for split launches only
FALLBACK_CASES = {
    (2, 8, 24): ("conv3d_bf16x3_fwd_kernel<2, 8, 60, flat24>", 0),
    (4, 4, 12): ("conv3d_bf16x3_fwd_kernel<2, 4, 60, flat12>", 1),
    (6, 6, 6): ("conv3d_bf16x3_fwd_kernel<2, 6, 60, flat6>", 1),
}


def _split_weights(L, wp, cin, cout):
    wsplit = torch.empty(L.icl_conv3d_split_ws_bytes(cin, cout) // 4, dtype=torch.float32, device=wp.device)
    arr, iarr = ctypes.c_void_p * 1, ctypes.c_int32 * 1
    _lib.check(L.icl_conv3d_split_weights_multi(arr(wp.data_ptr()), arr(wsplit.data_ptr()), iarr(cin), iarr(cout), 1, _stream(wp)), "split")
    return wsplit


def _name(L):
    return (L.icl_last_kernel_name() or b"").decode()


def check_pointer_fallbacks(monkeypatch, dev, d, h, w):
    kernel, rc_no_slab = FALLBACK_CASES[(d, h, w)]
    monkeypatch.setenv("ICL_CONV_SPLIT", "1")
    monkeypatch.setenv("ICL_CONV_SPLIT_MIN", "1")
    for k in ("ICL_CONV_SPLIT_FLAT", "ICL_CONV_SPLIT_FLAT12", "ICL_CONV_SPLIT_FLAT6", "ICL_CONV_SPLIT_KSPLIT_CUS"):
        monkeypatch.delenv(k, raising=False)
    L = _lib.lib()
    n, cin, cout, s = 1, 32, 32, d * h * w
    x = synthetic_volume((n, cin, d, h, w), 51).to(dev)
    wt = (synthetic_volume((cout, cin, 3, 3, 3), 52) * 0.2).to(dev)
    b = synthetic_volume((cout,), 53).to(dev)
    ref = F.conv3d(x.double().cpu(), wt.double().cpu(), b.double().cpu(), padding=1)
    tol = 2e-5 * float(ref.abs().max())
    wp = ops.pack_weights(wt, 0)
    wsplit = _split_weights(L, wp, cin, cout)
    shape = (n, cin, cout, d, h, w)

    def sentinel():      # a launch of another kernel, so that "nothing ran" shows in icl_last_kernel_name
        w1 = ops.pack_weights(wt[:, :, :1, :1, :1].contiguous(), 0)
        y1 = torch.empty((n, cout, d, h, w), device=dev)
        _lib.check(L.icl_conv3d_fwd(_ptr(x), _ptr(w1), None, _ptr(y1), None, n, cin, cout, d, h, w, 1, cin * s, cout * s, _stream(x)), "1x1x1")
        assert _name(L).startswith("conv3d_mfma_fwd_kernel<1, 2, 8, 4, ")
        return _name(L)

    def close(y):
        assert float((y.double().cpu() - ref).abs().max()) < tol

    # the unsplit plan: one tile, padded to one workgroup per XCD, each with a statistics slot; no slab
    monkeypatch.setenv("ICL_CONV_SPLIT_KSPLIT", "0")
    slots0 = L.icl_conv3d_fwd_stats_slots(*shape)
    assert slots0 == 8 and L.icl_conv3d_fwd_presplit_ws_bytes(*shape) == 0
    monkeypatch.setenv("ICL_CONV_SPLIT_KSPLIT", "2")
    kneed = L.icl_conv3d_fwd_presplit_ws_bytes(*shape)
    assert kneed == 2 * n * cout * s * 4 and L.icl_conv3d_fwd_stats_slots(*shape) == 0
    need = L.icl_conv3d_fwd_ws_bytes(*shape, 3)
    assert need == L.icl_conv3d_split_ws_bytes(cin, cout) + kneed
    slab = torch.empty(kneed // 4, device=dev)

    # 1. with a slab: the split launch
    nothing_ran = sentinel()
    y = torch.full((n, cout, d, h, w), float("nan"), device=dev)
    assert L.icl_conv3d_fwd_presplit_ws(_ptr(x), _ptr(wsplit), _ptr(b), _ptr(y), _ptr(slab), *shape, cin * s, cout * s, _stream(x)) == 0
    assert _name(L) == kernel
    close(y)
    y_split = y.clone()
    # 2. without one: rows of 24 run unsplit (other sums: close, not equal), the other tiles hand the call back
    nothing_ran = sentinel()
    y = torch.full((n, cout, d, h, w), float("nan"), device=dev)
    assert L.icl_conv3d_fwd_presplit(_ptr(x), _ptr(wsplit), _ptr(b), _ptr(y), *shape, cin * s, cout * s, _stream(x)) == rc_no_slab
    assert _name(L) == (kernel if rc_no_slab == 0 else nothing_ran)
    if rc_no_slab == 0:
        close(y)
        assert not torch.equal(y, y_split)
    else:
        assert bool(torch.isnan(y).all())
    # 3. fp32 weights given: they are split into the workspace and the slab lies behind them — the split launch, bit for bit
    nothing_ran = sentinel()
    ws = torch.empty(need // 4, device=dev)
    y = torch.full((n, cout, d, h, w), float("nan"), device=dev)
    assert L.icl_conv3d_fwd(_ptr(x), _ptr(wp), _ptr(b), _ptr(y), _ptr(ws), *shape, 3, cin * s, cout * s, _stream(x)) == 0
    assert _name(L) == kernel and torch.equal(y, y_split)
    # 4. y offset by 4 bytes: handed back (1), nothing launched, nothing written
    nothing_ran = sentinel()
    buf = torch.full((n * cout * s + 4,), float("nan"), device=dev)
    yo = buf[1:1 + n * cout * s]
    assert yo.data_ptr() % 16 == 4
    assert L.icl_conv3d_fwd_presplit_ws(_ptr(x), _ptr(wsplit), _ptr(b), _ptr(yo), _ptr(slab), *shape, cin * s, cout * s, _stream(x)) == 1
    assert _name(L) == nothing_ran and bool(torch.isnan(buf).all())
    # 5. statistics where the plan wants a split (this entry point brings no slab): rows of 24 run unsplit with the slots of the unsplit
    #    plan, the other tiles hand the call back
    nothing_ran = sentinel()
    stats = torch.full((n * cout, slots0, 3), float("nan"), device=dev)
    y = torch.full((n, cout, d, h, w), float("nan"), device=dev)
    assert L.icl_conv3d_fwd_presplit_stats(_ptr(x), _ptr(wsplit), _ptr(b), _ptr(y), _ptr(stats), *shape, cin * s, cout * s,
                                           _stream(x)) == rc_no_slab
    assert _name(L) == (kernel if rc_no_slab == 0 else nothing_ran)
    if rc_no_slab == 0:
        close(y)
        st = stats.double().cpu()        # (count, mean, M2) per (channel, workgroup): the counts add up to the volume
        assert not bool(torch.isnan(st).any()) and torch.equal(st[:, :, 0].sum(1), torch.full((n * cout,), float(s), dtype=torch.float64))
    else:
        assert bool(torch.isnan(y).all()) and bool(torch.isnan(stats).all())


# ---- the launches of one layer shape ---------------------------------------------------------------------------------------------

def checksum(t):
    """(int64 sum, xor) of the values' bit patterns, computed on the tensor's device"""
    b = t.contiguous().view(-1).view(torch.int32)
    total = int(b.sum(dtype=torch.int64))
    while b.numel() > 1:
        if b.numel() & 1:
            b = torch.cat([b, b.new_zeros(1)])
        half = b.numel() // 2
        b = b[:half] ^ b[half:]
    return [total, int(b[0])]


def _fill(numel, seed, dev, bound=1.0):
    return hash_uniform_torch(numel, seed, bound, device=dev)


def launch_record(dev, cin, cout, e, pool):
    """What the launcher does with cin -> cout @ e^3 at batch 2: the pre-split forward (with statistics where the plan has slots), the
    input gradient with n_live = 1 where icl_conv3d_fwd_live_ok allows it, the weight-gradient slabs with n_live 1 and 2.  Kernel
    names, slab counts, grids and the checksums of every output.  ``pool``: {"x": ..., "gy": ...} hash-filled buffers shared by the shapes."""
    L = _lib.lib()
    n, s = 2, e ** 3
    x = pool["x"][:n * cin * s].view(n, cin, e, e, e)
    gy = pool["gy"][:n * cout * s].view(n, cout, e, e, e)
    gy1 = gy.clone()
    gy1[1:] = 0
    wt = _fill(cout * cin * 27, 7, dev, (6.0 / (cin * 27)) ** 0.5).view(cout, cin, 3, 3, 3)
    wp, wpt = ops.pack_weights(wt, 0), ops.pack_weights(wt, 1)
    st = _stream(x)
    rec = {}

    def forward(tag, xin, wpk, ci, co, nl, live):
        """the entry-point choice of ops.conv3d_forward_raw on raw pointers"""
        y = torch.full((n, co, e, e, e), float("nan"), device=dev)
        out = {}
        rc = 1
        if ci % 16 == 0:
            wsplit = _split_weights(L, wpk, ci, co)
            slots = L.icl_conv3d_fwd_stats_slots(n, ci, co, e, e, e) if not live else 0
            kneed = L.icl_conv3d_fwd_presplit_ws_bytes(nl, ci, co, e, e, e)
            out["slots"], out["presplit_ws_bytes"] = slots, kneed
            if slots > 0:
                stats = torch.full((n * co, slots, 3), float("nan"), device=dev)
                rc = L.icl_conv3d_fwd_presplit_stats(_ptr(xin), _ptr(wsplit), None, _ptr(y), _ptr(stats), n, ci, co, e, e, e, ci * s, co * s, st)
                if rc == 0:
                    out["stats"] = checksum(stats)
            elif kneed:
                kws = torch.empty(kneed // 4, device=dev)
                rc = (L.icl_conv3d_fwd_presplit_ws_live(_ptr(xin), _ptr(wsplit), None, _ptr(y), _ptr(kws), n, nl, ci, co, e, e, e, ci * s, co * s, st)
                      if live else
                      L.icl_conv3d_fwd_presplit_ws(_ptr(xin), _ptr(wsplit), None, _ptr(y), _ptr(kws), n, ci, co, e, e, e, ci * s, co * s, st))
            else:
                rc = (L.icl_conv3d_fwd_presplit_live(_ptr(xin), _ptr(wsplit), None, _ptr(y), n, nl, ci, co, e, e, e, ci * s, co * s, st) if live
                      else L.icl_conv3d_fwd_presplit(_ptr(xin), _ptr(wsplit), None, _ptr(y), n, ci, co, e, e, e, ci * s, co * s, st))
            assert rc in (0, 1), rc
        out["presplit_rc"] = rc
        if rc == 1:      # not the split-product kernels: the fp32 pack
            need = L.icl_conv3d_fwd_ws_bytes(nl, ci, co, e, e, e, 3)
            ws = torch.empty(max(need // 4, 1), device=dev)
            out["fwd_ws_bytes"] = need
            rc = (L.icl_conv3d_fwd_live(_ptr(xin), _ptr(wpk), None, _ptr(y), _ptr(ws) if need else None, n, nl, ci, co, e, e, e, 3, ci * s, co * s, st)
                  if live else
                  L.icl_conv3d_fwd(_ptr(xin), _ptr(wpk), None, _ptr(y), _ptr(ws) if need else None, n, ci, co, e, e, e, 3, ci * s, co * s, st))
            assert rc == 0, rc
        out["kernel"] = _name(L)
        if live:
            out["live_kernel"] = (L.icl_last_live_fwd_kernel_name() or b"").decode()
        out["y"] = checksum(y)
        rec[tag] = out

    forward("forward", x, wp, cin, cout, n, False)
    rec["live_ok"] = L.icl_conv3d_fwd_live_ok(n, 1, cout, cin, e, e, e)
    if rec["live_ok"]:
        forward("dgrad_live1", gy1, wpt, cout, cin, 1, True)
    pe = L.icl_conv3d_packed_elems(cout, cin, 3, 0)
    for nl in (1, 2):
        ws = torch.full((max(L.icl_conv3d_wgrad_ws_bytes_live(n, nl, cin, cout, 3) // 4, 1),), float("nan"), device=dev)
        ns, a, b = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        rc = L.icl_conv3d_wgrad_slabs_live(_ptr(x), _ptr(gy if nl == 2 else gy1), _ptr(ws), n, nl, cin, cout, e, e, e, 3, cin * s, cout * s,
                                           ctypes.byref(ns), st)
        assert rc == 0 and 0 < ns.value * pe <= ws.numel(), (rc, ns.value)
        L.icl_last_wgrad_grid(ctypes.byref(a), ctypes.byref(b))
        rec[f"wgrad_live{nl}"] = {"kernel": _name(L), "nslabs": ns.value, "grid": [a.value, b.value], "slabs": checksum(ws[:ns.value * pe])}
    return rec
