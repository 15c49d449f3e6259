"""Call-trace pin of the convolution operators of icl_amd/ops.py, shared by the emulation suite (tests/test_conv_route.py, CPU tensors)
and the device suite (tests/test_gpu_conv_route.py).

`Recorder` stands in for the loaded library: every `icl_*` call is noted — entry point, every integer / float argument, pointers as
"null" / "ptr", the stream as "here" (the stream the case started on) / "other", the return value and `icl_last_kernel_name()` after the
call — and forwarded.  The launcher keeps that name per thread, so the first call a thread makes is preceded by a sentinel launch (a
1x1x1 convolution on sixteen voxels): no name is left over from an earlier test.  A plain entry point that has a `_live` sibling is
noted under the sibling's name with n_live = n (the two are the same call, include/icl_abi.inc), so which of them the operator picks
is not part of the pin.

`run_case` runs forward and backward of one case and returns {"trace": [...], "sums": checksums of y, gx, gw, gb}.  The goldens
(tests/golden/conv_route.json, conv_route_gpu.json) were recorded by tests/golden/make_golden_conv_route*.py on the commit BEFORE
`ops.plan_conv3d` existed; the tests compare for equality: same calls, same arguments, same kernels, same bits.

`forms_of` names what a trace reached (from the entry points it holds and the case's shape, never from the code under test); the
drivers assert that the goldens reach every name of `FORMS_EMU` / `FORMS_GPU`.
"""
import ctypes
import hashlib
import os
import threading

import torch

from conv_plan_checks import checksum
from icl_amd import _lib, ops
from icl_amd.utils.hashfill import synthetic_volume

SPLIT = {"ICL_CONV_SPLIT": "1", "ICL_CONV_SPLIT_MIN": "1"}
SWITCHES = ("ICL_CONV_", "ICL_WGRAD_", "ICL_LIVE_BATCH", "ICL_LAZY_NORM")
_QUIET = ("icl_last_kernel_name", "icl_last_error", "icl_last_live_fwd_kernel_name", "icl_last_wgrad_grid", "icl_abi_version")
_INTS = (ctypes.c_int, ctypes.c_int64, ctypes.c_uint32)
_FLOATS = (ctypes.c_float, ctypes.c_double)


def case(entry, n, cin, cout, d, h, w, ks=3, bias=True, zbg=False, xgrad=True, scope=False, lane=False, defer=False, k=None, p=0.0,
         patch=None, env=None):
    """entry: conv3d / conv3d_instance_norm_act / dropout_conv1x1 / conv1x1_lazy.  scope: second iteration of a StepScope with a
    PackedWeights cache (lane / defer: the weight-gradient lane is open / the slab sums are deferred).  k: live mark on gy.  patch:
    thresholds of ops moved for the case; env: environment switches (all ICL_CONV_* / ICL_WGRAD_* others are unset)."""
    return dict(entry=entry, n=n, cin=cin, cout=cout, d=d, h=h, w=w, ks=ks, bias=bias, zbg=zbg, xgrad=xgrad, scope=scope, lane=lane,
                defer=defer, k=k, p=p, patch=patch or {}, env=env or {})


def case_id(c):
    flags = "".join(f for f, on in (("b", c["bias"]), ("z", c["zbg"]), ("x", c["xgrad"]), ("S", c["scope"]), ("L", c["lane"]),
                                    ("D", c["defer"])) if on)
    extra = "".join(f"|{k}={v}" for k, v in sorted({**c["patch"], **c["env"]}.items()))
    return f"{c['entry']}|{c['n']}x{c['cin']}>{c['cout']}@{c['d']}.{c['h']}.{c['w']}|ks{c['ks']}|{flags}|k{c['k']}|p{c['p']}{extra}"


class Recorder:
    def __init__(self, real, here, sentinel):
        self._real, self._here, self._sentinel, self._primed, self.trace = real, here or 0, sentinel, set(), []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("icl_") or name in _QUIET:
            return fn
        types = _lib._SIGNATURES[name][1]
        live = name + "_live" if name + "_live" in _lib.EXPORTS else None
        first_int = next((i for i, t in enumerate(types) if t is ctypes.c_int), None)
        launches = _lib._SIGNATURES[name][0] is ctypes.c_int and types and types[-1] is ctypes.c_void_p

        def call(*args):
            assert len(args) == len(types), (name, len(args))
            noted = []
            for i, (a, t) in enumerate(zip(args, types)):
                if t in _INTS:
                    noted.append(int(a))
                    if live is not None and i == first_int:
                        noted.append(int(a))              # the `_live` sibling with n_live = n
                elif t in _FLOATS:
                    noted.append(float(a))
                else:
                    v = a.value if isinstance(a, ctypes.c_void_p) else a
                    if launches and i == len(types) - 1:
                        noted.append("here" if (v or 0) == self._here else "other")
                    else:
                        noted.append("null" if v is None or v == 0 else "ptr")
            if threading.get_ident() not in self._primed:
                self._primed.add(threading.get_ident())
                self._sentinel()
            rc = fn(*args)
            self.trace.append([live or name, noted, int(rc) if rc is not None else None, (self._real.icl_last_kernel_name() or b"").decode()])
            return rc
        return call


def _rand(shape, seed, dev, scale=1.0):
    return (synthetic_volume(tuple(shape), seed) * scale).to(dev)


def run_case(monkeypatch, dev, c):
    for key in [key for key in os.environ if key.startswith(SWITCHES)]:
        monkeypatch.delenv(key)
    for key, v in c["env"].items():
        monkeypatch.setenv(key, v)
    for key, v in c["patch"].items():
        monkeypatch.setattr(ops, key, v)
    n, cin, cout, d, h, w, ks = (c[f] for f in ("n", "cin", "cout", "d", "h", "w", "ks"))
    param = torch.nn.Parameter if c["scope"] else (lambda t: t.requires_grad_())
    x = _rand((n, cin, d, h, w), 61, dev).requires_grad_(c["xgrad"])
    wt = param(_rand((cout, cin, ks, ks, ks), 62, dev, (6.0 / (cin * ks ** 3)) ** 0.5))
    b = param(_rand((cout,), 63, dev, 0.1)) if c["bias"] else None
    ss = torch.stack([0.5 + 0.1 * _rand((n * cin,), 64, dev).abs(), 0.2 * _rand((n * cin,), 65, dev)], 1).contiguous()
    gy = _rand((n, cout, d, h, w), 66, dev)
    if c["k"] is not None:
        gy[c["k"]:] = 0

    def forward():
        if c["entry"] == "conv3d":
            return ops.conv3d(x, wt, b, zero_bias_grad=c["zbg"])
        if c["entry"] == "conv3d_instance_norm_act":
            return ops.conv3d_instance_norm_act(x, wt, b)
        if c["entry"] == "dropout_conv1x1":
            return ops.dropout_conv1x1(x, wt, b, c["p"], seed=91)
        assert c["entry"] == "conv1x1_lazy"
        return ops.conv1x1_lazy(ops.LazyAct(x, ss), wt, b, c["p"], seed=91)

    def iteration(rec=None):
        x.grad = wt.grad = None
        if b is not None:
            b.grad = None
        g = gy.clone()
        ops.mark_live(g, c["k"])
        y = forward()
        if rec is not None:
            rec.trace.append(["backward"])
        torch.autograd.backward([y], [g])
        return y

    real = _lib.lib()
    x1, y1, w1 = torch.zeros(64, device=dev), torch.zeros(64, device=dev), ops.pack_weights(torch.zeros((4, 4, 1, 1, 1), device=dev), 0)
    ws1 = torch.zeros(max(real.icl_conv3d_fwd_ws_bytes(1, 4, 4, 2, 2, 4, 1) // 4, 1), device=dev)

    def sentinel():
        _lib.check(real.icl_conv3d_fwd(ops._ptr(x1), ops._ptr(w1), None, ops._ptr(y1), ops._ptr(ws1), 1, 4, 4, 2, 2, 4, 1, 64, 64, ops._stream(x1)))
        assert (real.icl_last_kernel_name() or b"").decode().startswith("conv3d_mfma_fwd_kernel<1, ")
    here = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    rec = Recorder(real, here, sentinel)
    cache = ops.PackedWeights() if c["scope"] else None
    lane_was = ops.WgradLane.enabled
    try:
        if c["scope"]:
            with ops.StepScope.open(cache, deferrals=False):      # the first iteration packs per call and records the Parameters
                iteration()
            ops.WgradLane.enabled = c["lane"]
        _lib._lib = rec
        if c["scope"]:
            with ops.StepScope.open(cache, lane_open=c["lane"], deferrals=c["defer"]):
                y = iteration(rec)
                rec.trace.append(["close"])
        else:
            y = iteration(rec)
    finally:
        _lib._lib = real
        ops.WgradLane.enabled = lane_was
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    sums = {name: checksum(t.detach()) for name, t in (("y", y), ("gx", x.grad), ("gw", wt.grad), ("gb", None if b is None else b.grad))
            if t is not None}
    return {"trace": rec.trace, "sums": sums}


# ---- what a trace reached ---------------------------------------------------------------------------------------------------------

FORMS_FWD = ["fwd:tiny-volume-gemm", "fwd:channel-gemm", "fwd:small-1x1", "fwd:cin1", "fwd:presplit-stats", "fwd:presplit-slab",
             "fwd:presplit", "fwd:fp32-pack"]
FORMS_DGRAD = ["dgrad:channel-gemm", "dgrad:small-1x1", "dgrad:mfma"]
FORMS_WGRAD_INLINE = ["wgrad:rows", "wgrad:cin1", "wgrad:planes", "wgrad:product6", "wgrad:exchanged", "wgrad:deferred", "wgrad:direct"]
FORMS_WGRAD_LANE = [f + ":lane" for f in ("wgrad:product6", "wgrad:exchanged", "wgrad:deferred", "wgrad:direct")]
FORMS_GATE = ["gate:kept", "gate:dropped:channel-gemm", "gate:dropped:cin1", "gate:dropped:first-layer", "gate:dropped:flat6",
              "gate:dropped:1x1-mfma", "gate:dropped:live_ok"]
FORMS_FUSED = ["fused:dropout", "fused:lazy", "fused:lazy-dropout"]
FORMS_EMU = FORMS_FWD + FORMS_DGRAD + FORMS_WGRAD_INLINE + FORMS_GATE + FORMS_FUSED      # (the lane takes device tensors only)
FORMS_GPU = FORMS_EMU + FORMS_WGRAD_LANE


def forms_of(c, trace):
    cut = trace.index(["backward"])
    fwd = [t for t in trace[:cut] if len(t) == 4]
    bwd = [t for t in trace[cut:] if len(t) == 4]
    names_f, names_b = {t[0] for t in fwd}, {t[0] for t in bwd}
    out = set()
    mfma = ("icl_conv3d_fwd_presplit_ws_live", "icl_conv3d_fwd_presplit_live", "icl_conv3d_fwd_live")
    tiny = "icl_im2col3" in names_f
    if tiny:
        out.add("fwd:tiny-volume-gemm")
    elif "icl_gemm" in names_f:
        out.add("fwd:channel-gemm")
    if "icl_conv1x1_small_live" in names_f:
        out.add("fwd:small-1x1")
    if "icl_conv3d_cin1_fwd" in names_f:
        out.add("fwd:cin1")
    for name, form in (("icl_conv3d_fwd_presplit_stats", "fwd:presplit-stats"), ("icl_conv3d_fwd_presplit_ws_live", "fwd:presplit-slab"),
                       ("icl_conv3d_fwd_presplit_live", "fwd:presplit"), ("icl_conv3d_fwd_live", "fwd:fp32-pack")):
        if any(t[0] == name and t[2] == 0 for t in fwd):
            out.add(form)
    if "fwd:channel-gemm" in out and "icl_gemm" in names_b:
        out.add("dgrad:channel-gemm")
    if "icl_conv1x1_small_live" in names_b and c["entry"] in ("conv3d", "conv3d_instance_norm_act"):
        out.add("dgrad:small-1x1")
    if any(t[0] in mfma and t[2] == 0 for t in bwd):
        out.add("dgrad:mfma")

    def wgrad(form, launch):
        out.add(form + (":lane" if launch[1][-1] == "other" else ""))
    for t in bwd:
        ints = [a for a in t[1] if not isinstance(a, str)]
        if t[0] == "icl_conv1x1_wgrad_live":
            wgrad("wgrad:planes" if "icl_im2col3_planes" in names_b else "wgrad:rows", t)
        elif t[0] == "icl_conv3d_cin1_wgrad":
            wgrad("wgrad:cin1", t)
        elif t[0] == "icl_im2col3" and not tiny:
            wgrad("wgrad:product6", t)
        elif t[0] == "icl_conv3d_wgrad_slabs_live":
            wgrad("wgrad:deferred", t)
        elif t[0] == "icl_conv3d_wgrad_live":      # (n, n_live, channels of the first operand, of the second, ...)
            wgrad("wgrad:exchanged" if c["cin"] != c["cout"] and ints[2:4] == [c["cout"], c["cin"]] else "wgrad:direct", t)
    fused_b = {"icl_conv1x1_wgrad_dropout_live", "icl_conv1x1_wgrad_dropout_norm_live"} & names_b
    if "icl_conv1x1_dropout" in names_f or "icl_conv1x1_dropout_live" in names_f:
        out.add("fused:dropout")
    if "icl_conv1x1_dropout_norm" in names_f:
        out.add("fused:lazy-dropout" if c["p"] > 0 else "fused:lazy")
    if c["k"] is not None and not fused_b:
        live = [t for t in bwd if t[0].startswith("icl_conv") and t[0].endswith("_live") and not t[0].endswith("ws_bytes_live")]
        if any([a for a in t[1] if not isinstance(a, str)][1] == c["k"] for t in live):      # n_live is the second number
            out.add("gate:kept")
        elif "fwd:channel-gemm" in out:
            out.add("gate:dropped:channel-gemm")
        elif "fwd:cin1" in out:
            out.add("gate:dropped:cin1")
        elif c["cin"] == 1:
            out.add("gate:dropped:first-layer")
        elif "wgrad:product6" in out or "wgrad:product6:lane" in out:
            out.add("gate:dropped:flat6")
        elif c["ks"] == 1:
            out.add("gate:dropped:1x1-mfma")
        elif any(t[0] == "icl_conv3d_fwd_live_ok" and t[2] == 0 for t in bwd):
            out.add("gate:dropped:live_ok")
    return out


# ---- consumption of torch's CPU generator -------------------------------------------------------------------------------------------

def rng_states(dev):
    """sha256 of torch.get_rng_state() after each stochastic operator called without a seed, StepRNG off: dropout, drop_path,
    dropout_conv1x1 (fused and two-op form), conv1x1_lazy (p = 0 draws nothing, p > 0)."""
    assert ops.StepRNG.tensor is None
    torch.manual_seed(0)
    x = _rand((2, 16, 32, 32, 32), 71, dev)
    small = _rand((2, 16, 4, 4, 4), 72, dev)
    wt, b = _rand((2, 16, 1, 1, 1), 73, dev, 0.3), _rand((2,), 74, dev)
    ss = torch.stack([0.5 + 0.1 * _rand((32,), 75, dev).abs(), 0.2 * _rand((32,), 76, dev)], 1).contiguous()
    out = []

    def note(what):
        out.append([what, hashlib.sha256(torch.get_rng_state().numpy().tobytes()).hexdigest()])
    note("seeded")
    with torch.enable_grad():
        ops.dropout(small, 0.3)
        note("dropout")
        ops.drop_path(small, 0.3)
        note("drop_path")
        ops.dropout_conv1x1(x, wt, b, 0.3)
        note("dropout_conv1x1 fused")
        ops.dropout_conv1x1(small, wt, b, 0.3)
        note("dropout_conv1x1 two ops")
        ops.conv1x1_lazy(ops.LazyAct(x, ss), wt, b, 0.0)
        note("conv1x1_lazy p 0")
        ops.conv1x1_lazy(ops.LazyAct(x, ss), wt, b, 0.3)
        note("conv1x1_lazy p 0.3")
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

_ROWS1 = {"CONV1X1_WGRAD_MIN_VOXELS": 1}      # the thresholds tests/test_kernels_emu.py moves to reach the same forms
_GEMM = {"CONV1X1_GEMM_MIN_VOXELS": 4096}
_SWAP = {"WGRAD_SWAP_MIN_VOXELS": 1}
_KSPLIT = {**SPLIT, "ICL_CONV_SPLIT_KSPLIT": "3"}

CASES_EMU = [
    case("conv3d", 1, 128, 128, 3, 3, 3),                                          # tiny-volume GEMM
    case("conv3d_instance_norm_act", 1, 130, 128, 2, 3, 4),
    case("conv3d", 2, 20, 50, 10, 12, 20, ks=1),                                   # MFMA 1x1x1, rows reduction
    case("conv3d", 3, 20, 8, 4, 4, 8, ks=1, k=1),                                  # ... gate: 1x1x1 beyond 16 channels
    case("conv3d", 2, 20, 50, 10, 12, 20, ks=1, patch=_GEMM),                      # channel GEMM
    case("conv3d", 3, 20, 50, 4, 12, 30, ks=1, patch=_GEMM, k=2),
    case("conv3d", 2, 8, 2, 4, 4, 8, ks=1),                                        # small 1x1x1, direct weight gradient
    case("conv3d", 2, 8, 2, 4, 4, 8, ks=1, bias=False, xgrad=False),
    case("conv3d", 3, 8, 2, 4, 4, 8, ks=1, k=1),
    case("conv3d", 3, 16, 2, 8, 16, 16, ks=1, k=2),                                # small 1x1x1 with the rows reduction, live
    case("conv3d", 3, 1, 3, 4, 4, 8, ks=1, k=1),                                   # one input channel, 1x1x1: the first-layer clause
    case("conv3d", 2, 1, 16, 5, 7, 12, patch=_ROWS1),                              # shifted planes
    case("conv3d", 3, 1, 16, 5, 7, 12, patch=_ROWS1, k=2),
    case("conv3d", 2, 1, 16, 5, 7, 12),                                            # one input channel below the planes threshold
    case("conv3d", 2, 1, 16, 5, 9, 12, zbg=True, xgrad=False),                     # cin1 forward and weight gradient
    case("conv3d", 3, 1, 16, 5, 9, 12, zbg=True, xgrad=False, k=1),
    case("conv3d", 2, 1, 5, 2, 8, 8, xgrad=False),                                 # cin1 forward, bias gradient wanted: direct
    case("conv3d", 2, 1, 5, 2, 8, 8, xgrad=False, patch=_ROWS1),                   # ... planes
    case("conv3d", 1, 1, 16, 3, 6, 10, zbg=True, xgrad=False),                     # ... a width that is no multiple of 4
    case("conv3d", 2, 1, 16, 5, 9, 12, zbg=True, xgrad=False, env={"ICL_CONV_CIN1": "0"}),
    case("conv3d", 1, 16, 16, 3, 6, 10, zbg=True, xgrad=False),                    # no input gradient: the forward pack alone
    case("conv3d", 1, 48, 16, 8, 8, 16, zbg=True, patch=_SWAP),                    # exchanged roles
    case("conv3d", 1, 48, 16, 8, 8, 16, zbg=True, patch=_SWAP, env={"ICL_WGRAD_SWAP": "0"}),
    case("conv3d", 1, 48, 16, 8, 8, 16, patch=_SWAP),                              # ... refused by a wanted bias gradient
    case("conv3d", 1, 48, 16, 8, 8, 16, zbg=True),                                 # ... by the volume
    case("conv3d", 2, 3, 4, 8, 8, 8),                                              # fp32 pack
    case("conv3d", 2, 3, 4, 8, 8, 8, bias=False),
    case("conv3d", 2, 48, 32, 6, 6, 6, env=SPLIT),                                 # flat 6^3 forward, 6^3 product weight gradient
    case("conv3d", 3, 48, 32, 6, 6, 6, env=SPLIT, k=1),
    case("conv3d", 2, 48, 32, 6, 6, 6, env={**SPLIT, "ICL_CONV_SPLIT_FLAT6": "0"}),
    case("conv3d", 3, 16, 16, 4, 8, 16, env=SPLIT, k=1),                           # 3^3 split product, live
    case("conv3d", 3, 16, 16, 4, 8, 16, env=SPLIT, k=2),
    case("conv3d_instance_norm_act", 3, 4, 8, 3, 4, 8, env=SPLIT, k=1),
    case("conv3d", 3, 48, 32, 4, 4, 12, env=_KSPLIT, k=1),                         # split over the channel chunks: icl_conv3d_fwd_live_ok
    case("conv3d_instance_norm_act", 2, 16, 16, 8, 8, 16, scope=True, defer=True, env=SPLIT),      # statistics, deferred slabs
    case("conv3d_instance_norm_act", 2, 16, 16, 8, 8, 16, scope=True, env=SPLIT),
    case("conv3d_instance_norm_act", 1, 48, 32, 4, 4, 12, scope=True, defer=True, env=_KSPLIT),     # no slots: the slab launch
    case("conv3d", 2, 16, 16, 8, 8, 16, scope=True, defer=True, env=SPLIT),                         # pre-split without a slab
    case("conv3d", 2, 16, 16, 8, 8, 16, scope=True, defer=True, zbg=True, env=SPLIT),
    case("conv3d", 1, 32, 32, 2, 8, 24, scope=True, env=_KSPLIT),                                   # pre-split with a slab
    case("conv3d", 3, 16, 16, 4, 8, 16, scope=True, defer=True, zbg=True, env=SPLIT, k=1),
    case("conv3d", 2, 1, 16, 5, 9, 12, zbg=True, xgrad=False, scope=True, defer=True),
    case("conv3d", 2, 8, 2, 4, 4, 8, ks=1, scope=True, defer=True),
    case("dropout_conv1x1", 2, 16, 2, 32, 32, 32, ks=1, p=0.3),
    case("dropout_conv1x1", 3, 16, 2, 28, 28, 28, ks=1, p=0.3, k=1),
    case("dropout_conv1x1", 2, 16, 2, 4, 4, 8, ks=1, p=0.3),                      # not fusable: the two operators
    case("conv1x1_lazy", 2, 16, 2, 32, 32, 32, ks=1, p=0.0),
    case("conv1x1_lazy", 2, 16, 2, 32, 32, 32, ks=1, p=0.3),
    case("conv1x1_lazy", 3, 16, 2, 28, 28, 28, ks=1, p=0.0, k=2),
    case("conv1x1_lazy", 3, 16, 2, 28, 28, 28, ks=1, p=0.3, k=2, xgrad=False),
    case("conv1x1_lazy", 2, 16, 2, 4, 4, 8, ks=1, p=0.0),                         # not fusable: materialised
    case("conv1x1_lazy", 2, 16, 2, 4, 4, 8, ks=1, p=0.3),
]

# The device cases: the smallest volumes that reach each threshold unpatched, batch 2 (3 under a live mark).  (16 -> 16 @20^3 is not a
# volume of the split-product kernels — rows of 20 voxels —: it stays as the fp32 case whose live batch the launcher refuses, and
# 16 -> 16 @24^3 stands for the upper levels.)
_STEP = dict(scope=True, lane=True, defer=True)
CASES_GPU = [
    case("conv3d", 2, 16, 16, 20, 20, 20),
    case("conv3d", 3, 16, 16, 20, 20, 20, k=1),
    case("conv3d_instance_norm_act", 2, 16, 16, 24, 24, 24, **_STEP),                      # statistics from the epilogue
    case("conv3d", 2, 16, 16, 24, 24, 24, zbg=True, **_STEP),                              # pre-split, deferred slabs on the lane
    case("conv3d", 2, 16, 16, 24, 24, 24, zbg=True, scope=True, defer=True),               # ... in line
    case("conv3d", 2, 16, 16, 24, 24, 24, zbg=True, scope=True, lane=True),                # direct on the lane
    case("conv3d", 2, 16, 16, 24, 24, 24, zbg=True, scope=True),
    case("conv3d", 2, 16, 16, 24, 24, 24, scope=True, lane=True, defer=True),              # a bias gradient: direct
    case("conv3d", 3, 16, 16, 24, 24, 24, zbg=True, k=1, **_STEP),
    case("conv3d", 3, 16, 16, 24, 24, 24, k=2),
    case("conv3d_instance_norm_act", 2, 32, 64, 24, 24, 24, **_STEP),
    case("conv3d_instance_norm_act", 3, 32, 64, 24, 24, 24, k=1, **_STEP),
    case("conv3d_instance_norm_act", 3, 64, 32, 24, 24, 24, k=1, **_STEP),
    case("conv3d_instance_norm_act", 3, 64, 64, 24, 24, 24, k=1, **_STEP),
    case("conv3d_instance_norm_act", 3, 64, 64, 24, 24, 24, k=2, **_STEP),
    case("conv3d_instance_norm_act", 2, 128, 128, 12, 12, 12, **_STEP),                    # deep level: split over the channel chunks
    case("conv3d_instance_norm_act", 3, 128, 128, 12, 12, 12, k=1, **_STEP),
    case("conv3d_instance_norm_act", 3, 128, 128, 12, 12, 12, k=2, **_STEP),
    case("conv3d_instance_norm_act", 2, 256, 256, 6, 6, 6, **_STEP),                       # flat 6^3, the 6^3 product on the lane
    case("conv3d_instance_norm_act", 2, 256, 256, 6, 6, 6, scope=True, defer=True),
    case("conv3d_instance_norm_act", 3, 256, 256, 6, 6, 6, k=1, **_STEP),
    case("conv3d_instance_norm_act", 2, 128, 128, 4, 4, 4, **_STEP),                       # tiny-volume GEMM
    case("conv3d", 2, 128, 128, 4, 4, 4),
    case("conv3d", 2, 48, 16, 24, 24, 24, zbg=True, **_STEP),                              # exchanged roles on the lane
    case("conv3d", 2, 48, 16, 24, 24, 24, zbg=True, scope=True, defer=True),
    case("conv3d", 2, 48, 16, 24, 24, 24, **_STEP),                                        # ... refused by a wanted bias gradient
    case("conv3d", 3, 48, 16, 24, 24, 24, zbg=True, k=1, **_STEP),
    case("conv3d", 2, 1, 16, 64, 64, 64, zbg=True, xgrad=False),                           # cin1
    case("conv3d", 3, 1, 16, 64, 64, 64, zbg=True, xgrad=False, k=1),
    case("conv3d", 2, 1, 16, 64, 64, 64, xgrad=False),                                     # ... bias gradient wanted: planes
    case("conv3d", 2, 1, 16, 64, 64, 64, zbg=True),                                        # shifted planes
    case("conv3d", 3, 1, 16, 64, 64, 64, zbg=True, k=2),
    case("conv3d", 2, 1, 16, 32, 32, 32, zbg=True),                                        # ... below their threshold: direct
    case("conv3d", 2, 16, 2, 32, 32, 32, ks=1),                                            # small 1x1x1, rows reduction
    case("conv3d", 3, 16, 2, 32, 32, 32, ks=1, k=1),
    case("conv3d", 3, 16, 2, 8, 8, 8, ks=1, k=2),                                          # ... direct
    case("conv3d", 2, 32, 32, 32, 32, 32, ks=1),                                           # channel GEMM
    case("conv3d", 3, 32, 32, 32, 32, 32, ks=1, k=2),
    case("conv3d", 2, 32, 32, 16, 16, 16, ks=1),                                           # MFMA 1x1x1, rows reduction
    case("conv3d", 3, 32, 32, 16, 16, 16, ks=1, k=1),
    case("conv3d", 2, 32, 32, 8, 8, 8, ks=1),                                              # ... direct
    case("dropout_conv1x1", 2, 16, 2, 32, 32, 32, ks=1, p=0.3),
    case("dropout_conv1x1", 3, 16, 2, 32, 32, 32, ks=1, p=0.3, k=1),
    case("dropout_conv1x1", 2, 16, 2, 8, 8, 8, ks=1, p=0.3),
    case("conv1x1_lazy", 2, 16, 2, 32, 32, 32, ks=1, p=0.0),
    case("conv1x1_lazy", 2, 16, 2, 32, 32, 32, ks=1, p=0.3),
    case("conv1x1_lazy", 3, 16, 2, 32, 32, 32, ks=1, p=0.0, k=2),
    case("conv1x1_lazy", 3, 16, 2, 32, 32, 32, ks=1, p=0.3, k=2, xgrad=False),
    case("conv1x1_lazy", 2, 16, 2, 8, 8, 8, ks=1, p=0.3),
]


def record(monkeypatch_cls, dev, cases):
    """{case id: run_case(...)} with every case in a monkeypatch context of its own (the golden scripts)"""
    out = {}
    for c in cases:
        with monkeypatch_cls.context() as m:
            out[case_id(c)] = run_case(m, dev, c)
    return out
