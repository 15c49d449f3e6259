"""torch.autograd wrappers around the C-ABI HIP kernels (include/icl_hip.h).

PyTorch is plumbing here: tensors own the device memory, autograd owns the graph, the current
torch stream is handed to every launch.  All arithmetic happens in libicl_hip.so.
Each function cites the reference operator it replaces (paths relative to /root/reference/code).
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from .step_scope import BackwardEnd, DeferredBiasGrads, DeferredWgradReduce, FactoredGrads, ScopeField, StepScope, WgradLane  # noqa: F401

_vp = ctypes.c_void_p


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else _vp(t.data_ptr())


def _stream(t: torch.Tensor):
    if t.is_cuda:
        return _vp(torch.cuda.current_stream(t.device).cuda_stream)
    return None


def _require(*ts: Optional[torch.Tensor]):
    for t in ts:
        if t is None:
            continue
        if t.dtype not in (torch.float32, torch.uint8, torch.int64, torch.int32):
            raise TypeError(f"icl_amd: unsupported dtype {t.dtype}")
        if not t.is_cuda and not _lib.host_pointers_ok():
            raise RuntimeError("icl_amd: HIP kernels need device tensors (no CPU fallback)")


class SideStream:
    """Fork/join of the aligner heads onto a second HIP stream.

    The aligners (three calls, ~600 small launches forward+backward and the HBM-bound streaming of the 764 MB ``mlp2`` weights) need
    only the three deepest decoder maps; the rest of the decoder (the 48^3 / 96^3 convolutions, compute-bound on the matrix cores) does
    not depend on them.  ``with SideStream(inputs) as side:`` runs its body on a second stream ordered after everything queued on the
    current one; ``side.join(outputs)`` orders the current stream after it.  Autograd runs every backward node on the stream of its
    forward and synchronises across streams itself, so the aligner backward overlaps the backward of the upper decoder too; inside a
    captured step (ICLTrainer.capture) the two streams become parallel branches of the hipGraph.  Tensors crossing streams are
    recorded with the caching allocator (``record_stream``).  ``ICL_ALIGNER_STREAM=0`` (or a CPU tensor) runs the body in line."""
    enabled = os.environ.get("ICL_ALIGNER_STREAM", "1") != "0"
    # which branches take a lane: bit 0 the attention-map chains of sspa (own queries), bit 1 the guided levels of uscl (A/B runs:
    # with the three lanes 11.94 ms, only bit 0 13.95, only bit 1 13.62 on one box)
    lane_mask = 3
    lanes = int(os.environ.get("ICL_ALIGNER_LANES", "3"))   # further streams for the per-level branches inside the aligners (0: none)
    # Round 6: one more stream for the TOKEN side of the own-query aligner (1x1x1 projection, two LayerNorms, fc_kv of every level: needs
    # only the feature maps).  Forward: it runs beside the query chain, which waits for a level's k / v when it gets there.  Backward: the
    # token side of level i (130 us of 13,824-row kernels at 24^3) used to sit BETWEEN the chain's calls for levels i and i - 1 on the
    # aligner stream; on its own stream it runs beside them.  It forks from the step's stream (never from the aligner stream) and is
    # joined there: per captured graph every edge between forked streams keeps one direction (see join()).
    token_lane_on = os.environ.get("ICL_TOKEN_LANE", "1") != "0"
    _streams = {}
    _outer = None

    def __init__(self, inputs, lane: int = 0):
        """``lane`` 0 is the aligner stream itself; lanes 1..``SideStream.lanes`` carry branches forked from it (the attention-map
        chain of one resolution level: drop-path, LayerNorm, the token-axis ``mlp2``, the separable convolutions — independent of
        the query chain that links the levels, unet_3D_icl.py:209-222), so that the many small launches of the 6^3 / 12^3 levels
        and the HBM-bound 13,824^2 weight streams of the 24^3 level overlap instead of queueing behind each other.  A lane beyond
        ``SideStream.lanes`` runs its body in line on the current stream."""
        self.stream = None
        self.children, self.pending = [], []
        t0 = inputs[0]
        if SideStream.enabled and t0.is_cuda and torch.is_grad_enabled() and lane <= SideStream.lanes:
            dev = t0.device
            s = SideStream._streams.get((dev.index, lane))
            if s is None:
                s = SideStream._streams[(dev.index, lane)] = torch.cuda.Stream(device=dev)
            self.main = torch.cuda.current_stream(dev)
            s.wait_stream(self.main)
            self.tok = None
            if lane == 0:
                # the lanes fork from and join to the stream the aligner stream itself forks from (see join())
                for k in range(1, SideStream.lanes + 1):
                    sk = SideStream._streams.get((dev.index, k))
                    if sk is None:
                        sk = SideStream._streams[(dev.index, k)] = torch.cuda.Stream(device=dev)
                    sk.wait_stream(self.main)
                    self.children.append(sk)
            for t in inputs:
                t.record_stream(s)
            self.stream = s
            self._guard = torch.cuda.stream(s)

    @staticmethod
    def token_stream():
        """The token-side stream of the aligner block that is open on this thread, or None.  Forked from the step's stream on FIRST
        request (and joined there with the lanes): a block that never asks for it — nc = 16, SwinUNETR, whose aligners take the
        operator-by-operator path — captures no empty fork / join of it (a forked-but-unused token stream in the THIRD capture of a
        process made the replay of that graph crash inside hipGraphLaunch on ROCm 7.2: bench.py's default run, round 6)."""
        outer = SideStream._outer
        if outer is None or outer.stream is None or not SideStream.token_lane_on or SideStream.lanes <= 0:
            return None
        if outer.tok is None:
            dev = outer.stream.device
            sk = SideStream._streams.get((dev.index, "tok"))
            if sk is None:
                sk = SideStream._streams[(dev.index, "tok")] = torch.cuda.Stream(device=dev)
            sk.wait_stream(outer.main)
            outer.children.append(sk)
            outer.tok = sk
        return outer.tok

    def __enter__(self):
        if self.stream is not None:
            self._guard.__enter__()
            if self.children:
                SideStream._outer = self
        return self

    def __exit__(self, *a):
        if self.stream is not None:
            if SideStream._outer is self:
                SideStream._outer = None
            self._guard.__exit__(*a)

    def join(self, outputs):
        """Order the forking stream after this one.  A lane joined inside the aligner stream's block is NOT waited for there: the
        aligner stream's own join (to the stream everything forked from) waits for every lane — the lanes' results are consumed by the
        losses only, and a lane that the aligner stream waits on after it waited on the aligner stream is the two-way dependency
        between forked streams that a stream capture on ROCm 7.2 does not survive (trainer.capture)."""
        if self.stream is None:
            return
        outer = SideStream._outer
        if outer is not None and outer is not self:
            outer.pending.extend(outputs)
            return
        self.main.wait_stream(self.stream)
        for sk in self.children:
            self.main.wait_stream(sk)
        for t in list(outputs) + self.pending:
            t.record_stream(self.main)
        self.pending = []



class KernelTimer:
    """HIP-event timing of individual kernel launches on the stream they are launched on (bench.py roofline).
    Usage: ``with KernelTimer() as kt: step()``; ``kt.summary()`` -> {name: (launches, ms_total, flops, bytes)}."""

    active = None

    def __init__(self):
        self.records = []

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *a):
        KernelTimer.active = None

    def region(self, name, flops, nbytes, like):
        return _TimedRegion(self, name, flops, nbytes, like)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, fl, by in self.records:
            n, ms, f, b = out.get(name, (0, 0.0, 0.0, 0.0))
            out[name] = (n + 1, ms + e0.elapsed_time(e1), f + fl, b + by)
        return out


def event_bracket_overhead_us(device, reps: int = 40) -> float:
    """Median HIP-event duration of a bracket around a one-element fill kernel: what an event pair adds to the kernel it brackets on an
    otherwise idle stream (dispatch latency of the kernel packet behind the event packet).  bench.py reports it next to the raw numbers."""
    t = torch.zeros(1, device=device)
    s = torch.cuda.current_stream(device)
    vals = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        t.fill_(1.0)
        e1.record(s)
        torch.cuda.synchronize(device)
        vals.append(e0.elapsed_time(e1) * 1e3)
    vals.sort()
    return vals[len(vals) // 2]


class _TimedRegion:
    def __init__(self, kt, name, flops, nbytes, like):
        self.kt, self.name, self.flops, self.nbytes, self.like = kt, name, flops, nbytes, like

    def __enter__(self):
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e1 = torch.cuda.Event(enable_timing=True)
        self.e0.record(torch.cuda.current_stream(self.like.device))

    def __exit__(self, *a):
        self.e1.record(torch.cuda.current_stream(self.like.device))
        name = self.name
        if name.startswith("conv3d"):  # the launcher reports which template instantiation it picked
            kn = _lib.lib().icl_last_kernel_name()
            if kn:
                name = kn.decode()
        self.kt.records.append((name, self.e0, self.e1, self.flops, self.nbytes))


class _NullRegion:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NULL = _NullRegion()


def _timed(name, flops, nbytes, like):
    kt = KernelTimer.active
    if kt is None or not like.is_cuda:
        return _NULL
    return kt.region(name, flops, nbytes, like)


def _ws(nbytes: int, like: torch.Tensor) -> torch.Tensor:
    return torch.empty((max(int(nbytes), 4) + 3) // 4, dtype=torch.float32, device=like.device)


# --------------------------------------------------------------------------------------
# Conv3d (k=3 pad 1 or k=1), stride 1 — nn.Conv3d in networks/utils.py:104,107, unet_3D_icl.py:65
# --------------------------------------------------------------------------------------

def pack_weights(w: torch.Tensor, mode: int) -> torch.Tensor:
    L = _lib.lib()
    cout, cin, ks = w.shape[0], w.shape[1], w.shape[2]
    n = L.icl_conv3d_packed_elems(cout, cin, ks, mode)
    wp = torch.empty(n, dtype=torch.float32, device=w.device)
    _lib.check(L.icl_conv3d_pack_weights(_ptr(w), _ptr(wp), cout, cin, ks, mode, _stream(w)), "pack_weights")
    return wp


class _PackedEntry:
    """What a PackedWeights cache keeps per Parameter."""
    __slots__ = ("weight", "wp", "wpt", "valid", "split_fwd", "split_dgrad", "planes_valid", "wants_planes")

    def __init__(self, weight, wp, wpt):
        self.weight, self.wp, self.wpt, self.valid = weight, wp, wpt, False      # the Parameter, its two packs; valid: packed in this step
        self.split_fwd = self.split_dgrad = None                                 # the bf16 planes of wp / wpt,
        self.planes_valid = self.wants_planes = False      # ... split in this step; the weight has met a volume of the split-product kernels


class PackedWeights:
    """Step-level cache of the packed convolution weights (forward + dgrad layout).  The weights only change in the optimiser
    step, so a step scope brackets the iteration with ``begin_step()`` / ``end_step()`` of its owner's cache (``StepScope.open(packed)``):
    the first iteration packs per call (as a bare module does) and records which Parameters asked; every later ``begin_step()`` packs
    all of them in ONE launch into persistent buffers (fixed addresses: the launch is part of the captured hipGraph).  Else no cache."""
    current = ScopeField("packed")      # the cache of the open step

    def __init__(self):
        self.entries = {}     # id(parameter) -> _PackedEntry

    def begin_step(self):
        live = list(self.entries.values())
        if not live:
            return
        L = _lib.lib()
        n = len(live)
        arr, iarr = ctypes.c_void_p * n, ctypes.c_int32 * n
        _lib.check(L.icl_conv3d_pack_weights_multi(arr(*[e.weight.data_ptr() for e in live]), arr(*[e.wp.data_ptr() for e in live]),
                                                   arr(*[e.wpt.data_ptr() for e in live]), iarr(*[e.weight.shape[0] for e in live]),
                                                   iarr(*[e.weight.shape[1] for e in live]), iarr(*[e.weight.shape[2] for e in live]), n,
                                                   _stream(live[0].weight)), "pack_weights_multi")
        for e in live:
            e.valid = True
        # the three bf16 planes of every pack that can run on the split-product kernels (csrc/kernels/conv_bf16x3.h), again in one
        # launch: a convolution call then starts its kernel directly instead of a small split launch in front of it
        jobs = []
        for e in live:
            cout, cin = e.weight.shape[0], e.weight.shape[1]
            if e.weight.shape[2] != 3 or not e.wants_planes:      # only weights that have met a volume the split-product kernels take
                continue
            if e.split_fwd is None and e.split_dgrad is None:
                e.split_fwd, e.split_dgrad = (torch.empty(nb // 4, dtype=torch.float32, device=e.weight.device) if nb else None
                                              for nb in (L.icl_conv3d_split_ws_bytes(cin, cout), L.icl_conv3d_split_ws_bytes(cout, cin)))
            if e.split_fwd is not None:
                jobs.append((e.wp, e.split_fwd, cin, cout))
            if e.split_dgrad is not None:
                jobs.append((e.wpt, e.split_dgrad, cout, cin))
        if jobs:
            m = len(jobs)
            arr, iarr = ctypes.c_void_p * m, ctypes.c_int32 * m
            _lib.check(L.icl_conv3d_split_weights_multi(arr(*[j[0].data_ptr() for j in jobs]), arr(*[j[1].data_ptr() for j in jobs]),
                                                        iarr(*[j[2] for j in jobs]), iarr(*[j[3] for j in jobs]), m, _stream(live[0].weight)),
                       "split_weights_multi")
        for e in live:
            e.planes_valid = True

    def end_step(self):
        for e in self.entries.values():
            e.valid = e.planes_valid = False

    @staticmethod
    def _entry(weight):
        """(the cache of the open step, its entry for this very Parameter object); None for what does not exist."""
        cache = getattr(StepScope.current, "packed", None) if isinstance(weight, torch.nn.Parameter) else None
        e = cache.entries.get(id(weight)) if cache is not None else None
        return cache, (e if e is not None and e.weight is weight else None)

    @staticmethod
    def split_of(weight):
        """(fwd planes, dgrad planes) of a weight whose packs were split by this step's ``begin_step()``; (None, None) otherwise."""
        _, e = PackedWeights._entry(weight)
        return (e.split_fwd, e.split_dgrad) if e is not None and e.valid and e.planes_valid else (None, None)

    @staticmethod
    def get(weight):
        """(wp, wpt) of ``weight`` (contiguous [Cout, Cin, k, k, k]), packed now unless this step's begin_step() already did."""
        L = _lib.lib()
        cout, cin, ks = weight.shape[0], weight.shape[1], weight.shape[2]
        cache, e = PackedWeights._entry(weight)
        if e is None:
            e = _PackedEntry(weight, *(torch.empty(L.icl_conv3d_packed_elems(cout, cin, ks, mode), dtype=torch.float32, device=weight.device)
                                       for mode in (0, 1)))
            if cache is not None:
                cache.entries[id(weight)] = e
        if not e.valid:
            _lib.check(L.icl_conv3d_pack_weights_both(_ptr(weight), _ptr(e.wp), _ptr(e.wpt), cout, cin, ks, _stream(weight)), "pack_weights_both")
            e.valid, e.planes_valid = True, False       # packed by this call: the split planes are stale
        return e.wp, e.wpt

    @staticmethod
    def note_volume(weight, voxels: int):
        """Called by the convolution with the size of the volume it runs on: weights that meet a volume of the split-product
        kernels (>= 6^3 voxels — the launcher decides per shape — unless ICL_CONV_SPLIT_MIN says otherwise) get their bf16 planes from
        the next begin_step() on."""
        _, e = PackedWeights._entry(weight)
        if e is not None and voxels >= int(os.environ.get("ICL_CONV_SPLIT_MIN", 6 ** 3)):
            e.wants_planes = True


def conv3d_forward_raw(x, wp, bias, n, cin, cout, d, h, w, ks, x_bstride, y, y_bstride, wsplit=None, want_stats=False, n_live=None):
    """``wsplit``: the pack's bf16 planes when the step's PackedWeights.begin_step() has split them already.
    ``n_live`` (input gradients only; y dense): samples [0, n_live) are computed, samples [n_live, n) of y written as zeros; the plan,
    the workspaces and the FLOP / byte figures are those of a batch of n_live (the `_live` entry points: with n_live == n the plain ones).
    ``want_stats``: returns the InstanceNorm statistics of y — [n * cout, slots, 3] (count, mean, M2) summaries written by the
    convolution's epilogue (icl_conv3d_fwd_presplit_stats) — or None when this shape / path does not produce them."""
    L = _lib.lib()
    s = d * h * w
    assert n_live is None or not want_stats
    nl = n if n_live is None else n_live
    # algorithmic work of this launch: 2*taps*Cin*Cout FLOP per voxel; 4*(I+O+W) bytes
    flops = 2.0 * ks ** 3 * cin * cout * s * nl
    nbytes = 4.0 * (nl * s * (cin + cout) + ks ** 3 * cin * cout)
    need = L.icl_conv3d_fwd_ws_bytes(nl, cin, cout, d, h, w, ks)
    ws = _ws(need, x) if need else None
    ptrs, dims = (_ptr(x), _ptr(wsplit), _ptr(bias), _ptr(y)), (cin, cout, d, h, w, x_bstride, y_bstride, _stream(x))
    with _timed("conv3d_mfma_fwd_kernel", flops, nbytes, x):
        if want_stats and wsplit is not None and ks == 3 and os.environ.get("ICL_CONV_STATS", "1") != "0":
            slots = L.icl_conv3d_fwd_stats_slots(n, cin, cout, d, h, w)
            if slots > 0:
                stats = torch.empty((n * cout, slots, 3), dtype=torch.float32, device=x.device)
                rc = L.icl_conv3d_fwd_presplit_stats(*ptrs, _ptr(stats), n, *dims)
                if rc != 1:
                    _lib.check(rc, "conv3d_fwd_presplit_stats")
                    return stats
        if wsplit is not None and ks == 3:
            # deep levels (rows of 12 / 24 voxels): the launcher may split the channel chunks over workgroups and needs a slab workspace
            kneed = L.icl_conv3d_fwd_presplit_ws_bytes(nl, cin, cout, d, h, w)
            if kneed:
                kws = _ws(kneed, x)
                rc = L.icl_conv3d_fwd_presplit_ws_live(*ptrs, _ptr(kws), n, nl, *dims)
            else:
                rc = L.icl_conv3d_fwd_presplit_live(*ptrs, n, nl, *dims)
            if rc != 1:         # 1: this shape does not run on the split-product kernel -> the fp32 pack below
                _lib.check(rc, "conv3d_fwd_presplit_live")
                return
        _lib.check(L.icl_conv3d_fwd_live(_ptr(x), _ptr(wp), _ptr(bias), _ptr(y), _ptr(ws), n, nl, cin, cout, d, h, w, ks, x_bstride, y_bstride,
                                         _stream(x)), "conv3d_fwd_live")


@functools.lru_cache(maxsize=None)
def _cached_zeros(n: int, device: str) -> torch.Tensor:
    return torch.zeros(n, dtype=torch.float32, device=device)


# The route of a convolution call: everything that follows from shapes, flags, environment switches and the thresholds below is decided
# ONCE, by plan_conv3d, and carried from forward to backward as ctx.route.  What depends on pointers or on the state of
# the backward pass is decided where the call is made, as the C launcher does with its plans: the 16-byte alignment of dY for the
# one-input-channel weight gradient, a pre-split launch handing the call back (rc 1), icl_conv3d_fwd_stats_slots,
# DeferredWgradReduce.wants, WgradLane.wants / adoptable, the live mark of dY (live_of) and icl_conv3d_fwd_live_ok.

CONV1X1_WGRAD_MIN_VOXELS = 4096
FIRST_CONV_PLANES_MAX_K = 32      # Cin * 27 <= 32, i.e. one input channel
CONV1X1_GEMM_MIN_VOXELS = 65536
CONV1X1_SMALL_MAX_CHANNELS = 16       # 1x1x1 convolutions with <= 16 -> <= 16 channels below the GEMM threshold: icl_conv1x1_small
SMALL_CONV_MAX_VOXELS = 216      # 6^3
WGRAD_SWAP_MIN_VOXELS = 24 ** 3    # exchanged-roles weight gradient (_wgrad_exchanged): only where the split-product kernels run
SMALL_CONV_MIN_WEIGHTS = 128 * 128 * 27


class ConvRoute(NamedTuple):
    tiny: bool              # conv3d() and its fused forms run _conv3d_tiny_volume instead of _Conv3d (which takes `fwd` when called anyway)
    fwd: str                # "gemm" (channel GEMM) | "small" (<= 16-channel 1x1x1) | "cin1" | "mfma" (MFMA / split product)
    dgrad: Optional[str]    # "gemm" | "small" | "mfma"; None: the cin1 forward exists only where no input gradient is asked for
    wgrad: str              # "rows" | "planes" | "product6" | "exchanged" | "mfma" (deferred slabs or direct: decided at launch)
    wgrad_cin1: bool        # ... the one-input-channel kernel instead, where dY is 16-byte aligned
    dgrad_live: bool        # the form runs on the live samples of a marked dY; a form that does not reads the whole gradient
    wgrad_live: bool
    lane_ok: bool           # the weight gradient may run on the WgradLane beside the input gradient
    has_bias: bool
    zero_bias_grad: bool


def plan_conv3d(x_shape, w_shape, *, x_needs_grad: bool, has_bias: bool, zero_bias_grad: bool) -> ConvRoute:
    """The route of Conv3d of x [n, cin, d, h, w] with weight [cout, cin, k, k, k], k 3 (pad 1) or 1; thresholds and switches as they are now."""
    (n, cin, d, h, w), cout, ks = x_shape, w_shape[0], w_shape[2]
    s = d * h * w
    no_bias_grad = not has_bias or zero_bias_grad
    first = cin * 27 <= FIRST_CONV_PLANES_MAX_K
    # a whole 6^3 volume that the split-product kernel takes as ONE flat tile, split over the channel chunks (conv_bf16x3.h Bf3F6): the centre
    # block of the 3-D U-Net.  Forward and input gradient are one launch + a slab sum each; the weight gradient keeps the product form.
    flat6 = (ks == 3 and (d, h, w) == (6, 6, 6) and cin % 16 == 0 and cin >= 32 and ((cout + 15) // 16 * 16) % 32 == 0
             and os.environ.get("ICL_CONV_SPLIT", "1") != "0" and os.environ.get("ICL_CONV_SPLIT_FLAT6", "1") != "0"
             and os.environ.get("ICL_CONV_SPLIT_KSPLIT", "-1") != "0" and int(os.environ.get("ICL_CONV_SPLIT_MIN", 216)) <= 216)
    # <= 6^3 voxels with >= 128x128 channels: a skinny GEMM that streams the weights once, unless the flat 6^3 tile takes the volume
    tiny = ks == 3 and s <= SMALL_CONV_MAX_VOXELS and math.prod(w_shape) >= SMALL_CONV_MIN_WEIGHTS and not flat6
    small_ch = cin <= CONV1X1_SMALL_MAX_CHANNELS and cout <= CONV1X1_SMALL_MAX_CHANNELS and s % 4 == 0
    if ks == 1 and n * s >= CONV1X1_GEMM_MIN_VOXELS and not small_ch:
        fwd = dgrad = "gemm"
    elif ks == 1 and small_ch:
        fwd = dgrad = "small"
    elif (ks == 3 and cin == 1 and cout <= 16 and not x_needs_grad and 120 * (w + 2) <= 65536
          and os.environ.get("ICL_CONV_CIN1", "1") != "0"):
        fwd, dgrad = "cin1", None
    else:
        fwd = dgrad = "mfma"
    if ks == 1 and s % 4 == 0 and n * s >= CONV1X1_WGRAD_MIN_VOXELS:
        wgrad = "rows"
    elif ks == 3 and first and w % 4 == 0 and n * s >= CONV1X1_WGRAD_MIN_VOXELS * 64:
        wgrad = "planes"
    elif flat6:
        wgrad = "product6"
    elif (ks == 3 and no_bias_grad and cout == 16 and cin % 48 == 0 and h % 8 == 0 and d >= 8 and w % 4 == 0
          and s >= WGRAD_SWAP_MIN_VOXELS and os.environ.get("ICL_WGRAD_SWAP", "1") != "0"):
        wgrad = "exchanged"
    else:
        wgrad = "mfma"
    wgrad_cin1 = fwd == "cin1" and w % 4 == 0 and no_bias_grad
    # live batch: the 3^3 split-product / fp32 MFMA paths, the <= 16-channel 1x1x1 path and the rows reduction run on samples [0, k); the
    # channel GEMM, an MFMA 1x1x1 input gradient, the 6^3 product and a first-layer convolution in any form read the whole gradient
    return ConvRoute(tiny=tiny, fwd=fwd, dgrad=dgrad, wgrad=wgrad, wgrad_cin1=wgrad_cin1,
                     dgrad_live=dgrad == "small" or (dgrad == "mfma" and ks == 3),
                     wgrad_live=wgrad in ("rows", "exchanged", "mfma") and not first and not wgrad_cin1,
                     lane_ok=ks == 3 and x_needs_grad and not first, has_bias=has_bias, zero_bias_grad=zero_bias_grad)


class _Conv3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, route, want_stats=False):
        """want_stats: returns (y, stats) — stats = the InstanceNorm summaries of y from the convolution's epilogue, or an empty
        tensor when this call did not produce them (the normalisation then runs its own statistics pass)."""
        _require(x, weight, bias)
        x, weight = x.contiguous(), weight.contiguous()
        (n, cin, d, h, w), cout, ks = x.shape, weight.shape[0], weight.shape[2]
        assert weight.shape[1] == cin and weight.shape[2] == weight.shape[3] == weight.shape[4]
        s = d * h * w
        ctx.save_for_backward(x, weight)
        if ks == 3:
            WgradLane.note_use(weight)
        ctx.route, ctx.wpt, ctx.wsd = route, None, None
        y = torch.empty((n, cout, d, h, w), dtype=torch.float32, device=x.device)
        stats = wsf = None
        if route.fwd == "gemm":
            # 1x1x1 convolution with many channels on a big volume = one batched product  W [Cout,Cin] x x[b] [Cin,S]  on the
            # tiled fp32-MFMA kernel (csrc/kernels/gemm.h), reading the channel-major volume in place (k-strided B operand)
            gemm(weight, x, cout, s, cin, cin, s, True, False, out=y, ldc=s, bias=bias, act=16, batch=n, b_bstride=cin * s,
                 c_bstride=cout * s)       # act 16: the bias is indexed by the output row (= channel)
        elif route.fwd == "small":
            # <= 16 channels (the aligner's h -> h / h -> 1 maps, the `final` 16 -> num_classes convolution on 96^3 voxels): VALU
            # kernels on the natural weight layout, HBM-bound on big volumes
            _lib.check(_lib.lib().icl_conv1x1_small(_ptr(x), _ptr(weight), _ptr(bias), _ptr(y), n, cin, cout, s, cin, 1, _stream(x)),
                       "conv1x1_small")
        elif route.fwd == "cin1":
            # the first convolution of the backbones (one input channel): K = 27, an HBM stream of the output (csrc/kernels/conv_cin1.h)
            with _timed("conv_cin1_fwd_kernel", 2.0 * 27 * cout * s * n, 4.0 * n * s * (1 + cout), x):
                _lib.check(_lib.lib().icl_conv3d_cin1_fwd(_ptr(x), _ptr(weight), _ptr(bias), _ptr(y), n, cout, d, h, w, cin * s, cout * s,
                                                          _stream(x)), "conv3d_cin1_fwd")
        else:
            if ctx.needs_input_grad[0]:
                # the input gradient will need the flipped/transposed packing too: one launch for both, kept for backward
                wp, ctx.wpt = PackedWeights.get(weight)
                wsf, ctx.wsd = PackedWeights.split_of(weight)
                if ks == 3:
                    PackedWeights.note_volume(weight, s)
            else:
                wp = pack_weights(weight, 0)
            stats = conv3d_forward_raw(x, wp, bias, n, cin, cout, d, h, w, ks, cin * s, y, cout * s, wsplit=wsf, want_stats=want_stats)
        if not want_stats:
            return y
        ctx.set_materialize_grads(False)      # (no zero tensor — a fill launch per call — for the non-differentiable statistics output)
        if stats is None:
            stats = torch.empty(0, dtype=torch.float32, device=x.device)
        ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    def backward(ctx, gy, gstats=None):
        if gy is None:
            return None, None, None, None, None
        x, weight = ctx.saved_tensors
        route, gy = ctx.route, gy.contiguous()
        (n, cin, d, h, w), cout, ks = x.shape, weight.shape[0], weight.shape[2]
        # live batch: kept where both gradient forms of the route take one, and (3^3: the launcher splits the deep levels over the channel
        # chunks by the batch size) only where the live batch gets the full batch's kernels — its samples come out bit for bit
        k = live_of(gy, n)
        if k is not None and not (route.dgrad_live and route.wgrad_live
                                  and (ks != 3 or _lib.lib().icl_conv3d_fwd_live_ok(n, k, cout, cin, d, h, w))):
            k = None
        lane = route.lane_ok and WgradLane.wants(x, d * h * w) and ctx.needs_input_grad[1]
        if lane:
            WgradLane.fork_point(gy)      # where dY is complete, before the input gradient is queued on this stream
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _conv_dgrad(route, x, weight, gy, k, ctx.wpt, ctx.wsd)
        if ctx.needs_input_grad[1] or (route.has_bias and ctx.needs_input_grad[2]):
            gw, gb = _conv_wgrad(route, x, weight, gy, k, lane)
        return gx, gw, gb, None, None


def _conv_dgrad(route, x, weight, gy, k, wpt, wsd):
    (n, cin, d, h, w), cout, ks = x.shape, weight.shape[0], weight.shape[2]
    s = d * h * w
    gx = torch.empty_like(x)
    if route.dgrad == "gemm":      # (never under a live mark: k is None)
        # gx[b] [Cin,S] = W^T gy[b]: A = W read transposed (k-strided), B = gy[b] [Cout,S] (k-strided)
        gemm(weight, gy, cin, s, cout, cin, s, False, False, out=gx, ldc=s, batch=n, b_bstride=cout * s, c_bstride=cin * s)
    elif route.dgrad == "small":
        _lib.check(_lib.lib().icl_conv1x1_small_live(_ptr(gy), _ptr(weight), None, _ptr(gx), n, n if k is None else k, cout, cin, s, 1, cin,
                                                     _stream(x)), "conv1x1_small_live dgrad")
    else:
        conv3d_forward_raw(gy, wpt if wpt is not None else pack_weights(weight, 1), None, n, cout, cin, d, h, w, ks, cout * s, gx, cin * s,
                           wsplit=wsd, n_live=k)
    return mark_live(gx, k)


# The weight-gradient forms: f(L, x, weight, gy, gw, gb, dims, cost) writes gw (and gb where it is not None) from samples [0, nl) of x
# and dY; dims = (n, nl, cin, cout, d, h, w, ks, s), cost = (flops, bytes) of the launch for the KernelTimer.

def _wgrad_rows(L, x, weight, gy, gw, gb, dims, cost):
    """big-volume 1x1x1 convolution: HBM-bound channel-major reduction, rows split over many waves"""
    n, nl, cin, cout, d, h, w, ks, s = dims
    ws = _ws(L.icl_conv1x1_wgrad_ws_bytes(n, s, cin, cout), x)
    with _timed("conv1x1_wgrad_kernel", *cost, x):
        _lib.check(L.icl_conv1x1_wgrad_live(_ptr(x), _ptr(gy), _ptr(gw), _ptr(gb), _ptr(ws), n, nl, cin, cout, s, cin * s, cout * s,
                                            _stream(x)), "conv1x1_wgrad_live")


def _wgrad_cin1(L, x, weight, gy, gw, gb, dims, cost):
    n, nl, cin, cout, d, h, w, ks, s = dims
    ws = _ws(L.icl_conv3d_cin1_wgrad_ws_bytes(n, d, h), x)
    with _timed("conv_cin1_wgrad_kernel", *cost, x):
        _lib.check(L.icl_conv3d_cin1_wgrad(_ptr(x), _ptr(gy), _ptr(gw), _ptr(ws), n, cout, d, h, w, cin * s, cout * s, _stream(x)),
                   "conv3d_cin1_wgrad")


def _wgrad_planes(L, x, weight, gy, gw, gb, dims, cost):
    """first convolution (one input channel, big volume): 27 shifted planes + the reduction of _wgrad_rows over them; the implicit GEMM
    pads Cin to 16 and takes 300 us for 0.8 GFLOP (batch 2, 96^3), this takes ~130"""
    n, nl, cin, cout, d, h, w, ks, s = dims
    planes = torch.empty((n, cin * 27, s), dtype=torch.float32, device=x.device)
    _lib.check(L.icl_im2col3_planes(_ptr(x), _ptr(planes), n, cin, d, h, w, _stream(x)), "im2col3_planes")
    _wgrad_rows(L, planes, weight, gy, gw, gb, (n, n, cin * 27, cout, d, h, w, 1, s), cost)


def _wgrad_product6(L, x, weight, gy, gw, gb, dims, cost):
    """dW[cout][cin * 27] = dY^T [cout, n S] x im2col(x) [n S, cin * 27]: the tall / skinny product of ops.linear's weight gradient (the
    form _conv3d_tiny_volume gives it), here beside the split-product input gradient of the flat 6^3 tile"""
    n, nl, cin, cout, d, h, w, ks, s = dims
    cols = torch.empty((n * s, cin * 27), dtype=torch.float32, device=x.device)
    _lib.check(L.icl_im2col3(_ptr(x), _ptr(cols), n, cin, d, h, w, _stream(x)), "im2col3")
    g2 = gy.reshape(n, cout, s).transpose(1, 2).reshape(n * s, cout).contiguous()
    gw2, gb2 = _tall_atb(g2, cols, gb is not None)
    gw.copy_(gw2.view_as(gw))
    if gb is not None:
        gb.copy_(gb2)


def _wgrad_exchanged(L, x, weight, gy, gw, gb, dims, cost):
    """One cout block but three (or six, nine ...) cin blocks — up_concat1.conv1, 48 -> 16 @96^3, the U-Net's largest weight gradient:
    with the roles of x and dY exchanged, dW[co][ci][t] = sum_q dY[co][q - t] x[ci][q], the z-column kernel stages ONE halo'd dY block for
    three x blocks instead of one halo'd x block per dY block (matrix pipe 52 -> 68 %, profiles/r5_pmc_conv.md); the result comes out as
    [cin][cout] with mirrored taps and is written back by two tiny copies.  (Never with a bias gradient: plan_conv3d.)"""
    n, nl, cin, cout, d, h, w, ks, s = dims
    ws = _ws(L.icl_conv3d_wgrad_ws_bytes_live(n, nl, cout, cin, ks), x)
    gws = torch.empty((cin, cout, ks, ks, ks), dtype=torch.float32, device=x.device)
    with _timed("conv3d_mfma_wgrad_kernel", *cost, x):
        _lib.check(L.icl_conv3d_wgrad_live(_ptr(gy), _ptr(x), _ptr(gws), None, _ptr(ws), n, nl, cout, cin, d, h, w, ks, cout * s, cin * s,
                                           _stream(x)), "conv3d_wgrad (roles exchanged)")
    gw.copy_(gws.flip(2, 3, 4).transpose(0, 1))


def _wgrad_mfma(L, x, weight, gy, gw, gb, dims, cost):
    n, nl, cin, cout, d, h, w, ks, s = dims
    ws = _ws(L.icl_conv3d_wgrad_ws_bytes_live(n, nl, cin, cout, ks), x)
    with _timed("conv3d_mfma_wgrad_kernel", *cost, x):
        if gb is None and DeferredWgradReduce.wants(weight):
            # the slab sum is a leaf of the pass: queued, one launch for all of them when backward has ended
            ns = ctypes.c_int32(0)
            _lib.check(L.icl_conv3d_wgrad_slabs_live(_ptr(x), _ptr(gy), _ptr(ws), n, nl, cin, cout, d, h, w, ks, cin * s, cout * s,
                                                     ctypes.byref(ns), _stream(x)), "conv3d_wgrad_slabs")
            DeferredWgradReduce.defer(ws, gw, cout, cin, ks, ns.value, weight)
        else:
            _lib.check(L.icl_conv3d_wgrad_live(_ptr(x), _ptr(gy), _ptr(gw), _ptr(gb), _ptr(ws), n, nl, cin, cout, d, h, w, ks, cin * s, cout * s,
                                               _stream(x)), "conv3d_wgrad")


_WGRAD_FORMS = {"rows": _wgrad_rows, "cin1": _wgrad_cin1, "planes": _wgrad_planes, "product6": _wgrad_product6,
                "exchanged": _wgrad_exchanged, "mfma": _wgrad_mfma}


def _conv_wgrad(route, x, weight, gy, k, lane):
    """(gw, gb) by the route's weight-gradient form; ``lane``: on the WgradLane, which the caller forked where dY was complete."""
    (n, cin, d, h, w), cout, ks = x.shape, weight.shape[0], weight.shape[2]
    s, nl = d * h * w, n if k is None else k
    gw = torch.empty_like(weight)
    gb = gb_arg = torch.empty(cout, dtype=torch.float32, device=x.device) if route.has_bias else None
    if route.has_bias and route.zero_bias_grad:
        # the conv feeds an InstanceNorm: its output is invariant to the bias, so dL/dbias == 0 exactly (the reference holds ~1e-8 rounding
        # noise there); skip the reduction pass over dY.  The zero vector is a cached constant (nothing ever writes a non-zero into it), not a
        # fill kernel per layer and step; a fresh view, so that AccumulateGrad adopts it instead of cloning a tensor it sees other references
        # to.  Only inside a step bracket, where FusedSGD is the sole consumer; anywhere else every bias gets its own zero tensor.
        gb = _cached_zeros(cout, str(x.device)).view(cout) if getattr(StepScope.current, "packed", None) is not None else x.new_zeros(cout)
        gb_arg = None
    cost = (2.0 * ks ** 3 * cin * cout * s * nl, 4.0 * (nl * s * (cin + cout) + 2 * ks ** 3 * cin * cout))
    form = _WGRAD_FORMS["cin1" if route.wgrad_cin1 and gy.data_ptr() % 16 == 0 else route.wgrad]
    args = (_lib.lib(), x, weight, gy, gw, gb_arg, (n, nl, cin, cout, d, h, w, ks, s), cost)
    if lane:
        with WgradLane.on_lane(x, gy, gw, gb_arg):      # deep level: beside the input gradient instead of behind it
            form(*args)
        if not WgradLane.adoptable(weight):
            WgradLane.sync_to_current(gw)      # accumulated / hooked gradient: no race with the lane
    else:
        form(*args)
    return gw, gb


class _Im2Col3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require(x)
        x = x.contiguous()
        n, c, d, h, w = x.shape
        cols = torch.empty((n * d * h * w, c * 27), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().icl_im2col3(_ptr(x), _ptr(cols), n, c, d, h, w, _stream(x)), "im2col3")
        ctx.shape = (n, c, d, h, w)
        return cols

    @staticmethod
    def backward(ctx, g):
        n, c, d, h, w = ctx.shape
        g = g.contiguous()
        dx = torch.empty((n, c, d, h, w), dtype=torch.float32, device=g.device)
        _lib.check(_lib.lib().icl_col2im3(_ptr(g), _ptr(dx), n, c, d, h, w, _stream(g)), "col2im3")
        return dx


def _conv3d_tiny_volume(x, weight, bias):
    """3^3 convolution on <= 6^3 voxels with >= 128x128 channels: a skinny GEMM that streams the weights once
    (csrc/kernels/misc.h im2col3 / col2im3 + the weight-streaming / tiled products of csrc/kernels/gemm.h through ``linear``;
    dW through its tall/skinny paths)."""
    n, cin, d, h, w = x.shape
    cout = weight.shape[0]
    y = linear(_Im2Col3.apply(x), weight.flatten(1), bias, lane_wgrad=True)            # [n*S, cout]; dW beside the input gradient (WgradLane)
    return y.view(n, d * h * w, cout).permute(0, 2, 1).reshape(n, cout, d, h, w)


def _conv3d_routed(x, weight, bias, zero_bias_grad, want_stats=False, tiny_ok=True):
    """(y, the InstanceNorm statistics of y from the convolution's epilogue where they were asked for and produced, else None)"""
    route = plan_conv3d(x.shape, weight.shape, x_needs_grad=x.requires_grad, has_bias=bias is not None, zero_bias_grad=zero_bias_grad)
    if route.tiny and tiny_ok:
        return _conv3d_tiny_volume(x, weight, bias), None
    if not want_stats:
        return _Conv3d.apply(x, weight, bias, route), None
    y, stats = _Conv3d.apply(x, weight, bias, route, True)
    return y, (stats if stats.numel() else None)


def conv3d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
           zero_bias_grad: bool = False) -> torch.Tensor:
    """Conv3d, kernel 3 (pad 1) or 1 (pad 0), stride 1.  ``zero_bias_grad``: the caller guarantees the output goes
    straight into a mean-removing normalisation, so the bias gradient is identically zero."""
    return _conv3d_routed(x, weight, bias, zero_bias_grad)[0]


def conv3d_instance_norm_act(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: int = 1, eps: float = 1e-5):
    """Conv3d(k=3, pad=1) -> InstanceNorm3d(affine=False) -> act (1 = ReLU): the block of UnetConv3
    (/root/reference/code/networks/utils.py:104-106).  Where the convolution runs on the split-product kernels inside a trainer step,
    its epilogue hands the normalisation the per-(sample, channel) statistics and the stand-alone statistics pass is skipped; everywhere
    else this is conv3d followed by instance_norm_act."""
    y, stats = _conv3d_routed(x, weight, bias, True, True)
    return _NormAct.apply(y, None, None, None, None, 0, True, int(act), eps, 0.0, stats)


# --------------------------------------------------------------------------------------
# InstanceNorm3d / BatchNorm3d (+ReLU) — networks/utils.py:105-109, unet_3D_icl.py:325-340
# --------------------------------------------------------------------------------------

class _NormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, mode, use_batch_stats, act, eps, momentum, stats=None):
        """stats: [rows, slots, 3] (count, mean, M2) summaries of x written by its producer (conv3d_forward_raw) — the statistics
        pass over x is skipped."""
        _require(x, gamma, beta, running_mean, running_var)
        L = _lib.lib()
        x = x.contiguous()
        n, c = x.shape[0], x.shape[1]
        s = x.numel() // (n * c)
        groups = c if mode == 1 else n * c
        y = torch.empty_like(x)
        ws = _ws(L.icl_norm_ws_bytes(n, c, s), x)
        if use_batch_stats:
            mean = torch.empty(groups, dtype=torch.float32, device=x.device)
            rstd = torch.empty(groups, dtype=torch.float32, device=x.device)
            rm, rv = running_mean, running_var
        else:  # eval-mode BatchNorm: fixed statistics
            assert mode == 1 and running_mean is not None
            mean = running_mean.detach().clone()
            rstd = torch.empty(groups, dtype=torch.float32, device=x.device)
            _lib.check(L.icl_rstd_from_var(_ptr(running_var), _ptr(rstd), c, eps, _stream(x)), "rstd_from_var")
            rm = rv = None
        if stats is not None and use_batch_stats:
            assert mode == 0 and stats.shape[0] == n * c and stats.is_contiguous()
            _lib.check(L.icl_norm_fwd_given_stats(_ptr(x), None, _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv),
                                                  n, c, s, mode, act, eps, momentum, _ptr(stats), stats.shape[1], _stream(x)),
                       "norm_fwd_given_stats")
        else:
            _lib.check(L.icl_norm_fwd(_ptr(x), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv),
                                      n, c, s, mode, int(use_batch_stats), act, eps, momentum, _ptr(ws), _stream(x)), "norm_fwd")
        ctx.save_for_backward(x, mean, rstd, gamma, beta)
        ctx.cfg = (mode, int(use_batch_stats), act)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        mode, ubs, act = ctx.cfg
        L = _lib.lib()
        gy = gy.contiguous()
        n, c = x.shape[0], x.shape[1]
        s = x.numel() // (n * c)
        gx = torch.empty_like(x)
        dg = db = None
        if gamma is not None:
            dg = torch.empty_like(gamma)
            db = torch.empty_like(beta)
        k = live_of(gy, n) if (mode == 0 and gamma is None) else None      # instance statistics: per sample
        nl = n if k is None else k
        ws = _ws(L.icl_norm_ws_bytes(nl, c, s), x)
        _lib.check(L.icl_norm_bwd_live(_ptr(gy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(gx), _ptr(dg), _ptr(db), n, nl, c,
                                       s, mode, ubs, act, _ptr(ws), _stream(x)), "norm_bwd_live")
        return mark_live(gx, k), dg, db, None, None, None, None, None, None, None, None


def instance_norm_relu(x: torch.Tensor, relu: bool = True, eps: float = 1e-5) -> torch.Tensor:
    """InstanceNorm3d(affine=False, no running stats) [+ ReLU] fused."""
    return _NormAct.apply(x, None, None, None, None, 0, True, int(relu), eps, 0.0)


def instance_norm_act(x: torch.Tensor, act: int, eps: float = 1e-5) -> torch.Tensor:
    """InstanceNorm3d(affine=False) fused with act 0 none / 1 ReLU / 2 LeakyReLU(0.01) (MONAI UnetResBlock norm1+lrelu, norm3)."""
    return _NormAct.apply(x, None, None, None, None, 0, True, int(act), eps, 0.0)


# --------------------------------------------------------------------------------------
# Deferred InstanceNorm3d + ReLU (round 5) — Conv3d -> InstanceNorm3d -> ReLU of UnetConv3 (networks/utils.py:107-109) whose output
# feeds MaxPool3d, the skip concatenation, nn.Upsample or the `final` convolution (unet_3D_icl.py:41-53,116-117; utils.py:264,276)
# --------------------------------------------------------------------------------------

def _lazy_norm_min_voxels() -> int:
    """Smallest volume whose normalisation is deferred; ICL_LAZY_NORM=0 turns the deferral off (both read per call: the tests switch them)."""
    if os.environ.get("ICL_LAZY_NORM", "1") == "0":
        return 1 << 62
    return int(os.environ.get("ICL_LAZY_NORM_MIN", str(48 ** 3)))


class LazyAct:
    """A convolution output whose InstanceNorm + ReLU is deferred to its consumers.  ``t`` holds the RAW convolution output — in autograd
    terms it already IS the normalised activation (its gradient is the gradient of relu(norm(y)); `_NormActLazy.backward` turns it into
    the gradient of y) — and ``ss`` the per-(sample, channel) (scale, shift) pairs with which ``skip_and_pool``, ``upsample2x_concat`` and
    ``dropout_conv1x1`` / ``conv1x1_lazy`` apply relu(fma(t, scale, shift)) while they load it.  Never hand ``t`` to anything else:
    ``materialize()`` writes the normalised tensor out (one pass, what the non-deferred path always does).  Measured upper bound of not
    writing the 96^3 / 48^3 activations of a step: profiles/r5_skip_norm_fwd_upper_bound.txt."""
    __slots__ = ("t", "ss")

    def __init__(self, t: torch.Tensor, ss: torch.Tensor):
        self.t, self.ss = t, ss

    @property
    def shape(self):
        return self.t.shape

    def materialize(self) -> torch.Tensor:
        return _LazyMaterialize.apply(self.t, self.ss)


def materialized(x):
    return x.materialize() if isinstance(x, LazyAct) else x


class _NormActLazy(torch.autograd.Function):
    """(y, summaries) -> (y as the virtual normalised activation, ss).  Backward: InstanceNorm + ReLU backward exactly as _NormAct's."""

    @staticmethod
    def forward(ctx, y, stats, eps):
        _require(y, stats)
        L = _lib.lib()
        n, c = y.shape[0], y.shape[1]
        mean = torch.empty(n * c, dtype=torch.float32, device=y.device)
        rstd = torch.empty(n * c, dtype=torch.float32, device=y.device)
        ss = torch.empty((n * c, 2), dtype=torch.float32, device=y.device)
        _lib.check(L.icl_norm_finalize_stats(_ptr(stats), n, c, stats.shape[1], eps, _ptr(mean), _ptr(rstd), _ptr(ss), _stream(y)),
                   "norm_finalize_stats")
        ctx.save_for_backward(y, mean, rstd)
        ctx.mark_non_differentiable(ss)
        ctx.set_materialize_grads(False)
        return y.view_as(y), ss

    @staticmethod
    def backward(ctx, ga, gss=None):
        if ga is None:
            return None, None, None
        y, mean, rstd = ctx.saved_tensors
        L = _lib.lib()
        ga = ga.contiguous()
        n, c = y.shape[0], y.shape[1]
        s = y.numel() // (n * c)
        gy = torch.empty_like(y)
        k = live_of(ga, n)
        nl = n if k is None else k
        ws = _ws(L.icl_norm_ws_bytes(nl, c, s), y)
        _lib.check(L.icl_norm_bwd_live(_ptr(ga), _ptr(y), _ptr(mean), _ptr(rstd), None, None, _ptr(gy), None, None, n, nl, c, s, 0, 1, 1,
                                       _ptr(ws), _stream(y)), "norm_bwd_live")
        return mark_live(gy, k), None, None


class _LazyMaterialize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, ss):
        L = _lib.lib()
        n, c = t.shape[0], t.shape[1]
        s = t.numel() // (n * c)
        if s % 4:
            sc = ss[:, 0].reshape(n, c, *([1] * (t.dim() - 2)))
            sh = ss[:, 1].reshape(n, c, *([1] * (t.dim() - 2)))
            return torch.clamp_min(torch.addcmul(sh, t, sc), 0.0)
        out = torch.empty_like(t)
        _lib.check(L.icl_norm_apply(_ptr(t), _ptr(ss), _ptr(out), n, c, s, _stream(t)), "norm_apply")
        return out

    @staticmethod
    def backward(ctx, g):
        return g, None      # `t` already stands for the normalised activation in the autograd graph


def conv3d_instance_norm_act_lazy(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], eps: float = 1e-5):
    """``conv3d_instance_norm_act(..., act=1)`` returning a ``LazyAct`` when the convolution's epilogue produced the statistics and the
    volume is big enough for the normalisation pass to matter (>= 48^3 voxels), the normalised tensor otherwise."""
    s = x.shape[2] * x.shape[3] * x.shape[4]
    if weight.shape[2] != 3 or s < _lazy_norm_min_voxels() or s % 4 or not torch.is_grad_enabled():
        return conv3d_instance_norm_act(x, weight, bias, act=1, eps=eps)
    y, stats = _conv3d_routed(x, weight, bias, True, True, tiny_ok=False)
    if stats is None:
        return _NormAct.apply(y, None, None, None, None, 0, True, 1, eps, 0.0, None)
    av, ss = _NormActLazy.apply(y, stats, eps)
    return LazyAct(av, ss)


class _InstanceNormAddAct(torch.autograd.Function):
    """act(InstanceNorm3d(x) + res): the tail of MONAI UnetResBlock.forward in one pass (and one backward pass that
    produces both gx and gres)."""

    @staticmethod
    def forward(ctx, x, res, act, eps, stats=None):
        _require(x, res)
        L = _lib.lib()
        x, res = x.contiguous(), res.contiguous()
        assert x.shape == res.shape
        n, c = x.shape[0], x.shape[1]
        s = x.numel() // (n * c)
        y = torch.empty_like(x)
        mean = torch.empty(n * c, dtype=torch.float32, device=x.device)
        rstd = torch.empty(n * c, dtype=torch.float32, device=x.device)
        if stats is not None:       # the producing convolution's epilogue wrote the (count, mean, M2) summaries (conv3d_forward_raw)
            assert stats.shape[0] == n * c and stats.is_contiguous()
            _lib.check(L.icl_norm_fwd_given_stats(_ptr(x), _ptr(res), _ptr(y), _ptr(mean), _ptr(rstd), None, None, None, None, n, c, s, 0, act,
                                                  eps, 0.0, _ptr(stats), stats.shape[1], _stream(x)), "norm_fwd_given_stats")
        else:
            ws = _ws(L.icl_norm_ws_bytes(n, c, s), x)
            _lib.check(L.icl_norm_res_fwd(_ptr(x), _ptr(res), _ptr(y), _ptr(mean), _ptr(rstd), None, None, None, None, n, c, s, 0, 1, act,
                                          eps, 0.0, _ptr(ws), _stream(x)), "norm_res_fwd")
        ctx.save_for_backward(x, res, mean, rstd)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, gy):
        x, res, mean, rstd = ctx.saved_tensors
        L = _lib.lib()
        gy = gy.contiguous()
        n, c = x.shape[0], x.shape[1]
        s = x.numel() // (n * c)
        gx = torch.empty_like(x)
        gres = torch.empty_like(x)
        ws = _ws(L.icl_norm_ws_bytes(n, c, s), x)
        _lib.check(L.icl_norm_res_bwd(_ptr(gy), _ptr(x), _ptr(res), _ptr(mean), _ptr(rstd), None, None, _ptr(gx), _ptr(gres), None,
                                      None, n, c, s, 0, 1, ctx.act, _ptr(ws), _stream(x)), "norm_res_bwd")
        return gx, gres, None, None, None


def instance_norm_add_act(x: torch.Tensor, res: torch.Tensor, act: int = 2, eps: float = 1e-5) -> torch.Tensor:
    return _InstanceNormAddAct.apply(x, res, int(act), eps)


def conv3d_instance_norm_add_act(x: torch.Tensor, weight: torch.Tensor, res: torch.Tensor, act: int = 2, eps: float = 1e-5) -> torch.Tensor:
    """act(InstanceNorm3d(Conv3d(x)) + res): the second half of MONAI's UnetResBlock (swinunetr_icl.py:128-229), the convolution's
    epilogue handing the normalisation its statistics where it can (see conv3d_instance_norm_act)."""
    y, stats = _conv3d_routed(x, weight, None, True, True)
    return _InstanceNormAddAct.apply(y, res, int(act), eps, stats)


def batch_norm_relu(x, gamma, beta, running_mean, running_var, training: bool, relu: bool = True,
                    eps: float = 1e-5, momentum: float = 0.1) -> torch.Tensor:
    """BatchNorm3d (batch statistics + running-stat update in training, running stats in eval) [+ ReLU]."""
    return _NormAct.apply(x, gamma, beta, running_mean, running_var, 1, bool(training), int(relu), eps, momentum)


def batch_norm_act(x, gamma, beta, running_mean, running_var, training: bool, act: int,
                   eps: float = 1e-5, momentum: float = 0.1) -> torch.Tensor:
    """BatchNorm{2,3}d fused with act: 0 none, 1 ReLU, 2 LeakyReLU(0.01) (2-D ConvBlock, networks/unet_icl.py:46-54).
    A 4-D input [N,C,H,W] is normalised over (N,H,W) exactly like a 5-D one over (N,D,H,W)."""
    return _NormAct.apply(x, gamma, beta, running_mean, running_var, 1, bool(training), int(act), eps, momentum)


def _embed_2d_weight(weight: torch.Tensor) -> torch.Tensor:
    """[Co,Ci,3,3] -> [Co,Ci,3,3,3] with the 2-D stencil in the dz = 1 plane (autograd slices the gradient back).
    A 3x3 convolution of a D = 1 volume with this kernel and padding 1 is exactly the 2-D convolution."""
    co, ci, kh, kw = weight.shape
    if kh == 1:
        return weight.unsqueeze(2)
    w3 = weight.new_zeros((co, ci, 3, kh, kw))
    w3[:, :, 1] = weight
    return w3


def conv2d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, zero_bias_grad: bool = False) -> torch.Tensor:
    """nn.Conv2d k=3 pad 1 / k=1 on [N,C,H,W] (networks/unet_icl.py:46-52,82,173) through the 3-D MFMA kernels."""
    return conv3d(x.unsqueeze(2), _embed_2d_weight(weight), bias, zero_bias_grad).squeeze(2)


def depthwise_conv2d(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """Depthwise 3x3 (SeparableConv2d.depthwise, networks/unet_icl.py:100-103) on the 3-D stencil kernel."""
    return depthwise_conv3d(x.unsqueeze(2), _embed_2d_weight(weight)).squeeze(2)


# --------------------------------------------------------------------------------------
# MaxPool3d(2) — networks/unet_3D_icl.py:41-53
# --------------------------------------------------------------------------------------

class _MaxPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pd):
        _require(x)
        L = _lib.lib()
        x = x.contiguous()
        n, c, d, h, w = x.shape
        assert d % pd == 0 and h % 2 == 0 and w % 2 == 0, "max-pool kernels need even extents"
        y = torch.empty((n, c, d // pd, h // 2, w // 2), dtype=torch.float32, device=x.device)
        idx = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
        _lib.check(L.icl_maxpool2_fwd(_ptr(x), _ptr(y), _ptr(idx), n * c, d // pd, h // 2, w // 2, pd, _stream(x)), "maxpool2_fwd")
        ctx.save_for_backward(idx)
        ctx.pd = pd
        return y

    @staticmethod
    def backward(ctx, gy):
        (idx,) = ctx.saved_tensors
        L = _lib.lib()
        gy = gy.contiguous()
        n, c, d, h, w = gy.shape
        gx = torch.empty((n, c, d * ctx.pd, h * 2, w * 2), dtype=torch.float32, device=gy.device)
        _lib.check(L.icl_maxpool2_bwd(_ptr(gy), _ptr(idx), _ptr(gx), n * c, d, h, w, ctx.pd, _stream(gy)), "maxpool2_bwd")
        return gx, None


class _SkipAndPool(torch.autograd.Function):
    """(x, maxpool2(x)) for a tensor that feeds a skip connection AND the pooling of the next level: the backward adds the two
    gradients inside the pooling backward's pass (icl_maxpool2_bwd_add) instead of a pooling backward plus an autograd `add` over the
    full-resolution tensor.  The skip gradient may be a channel slice of a concat gradient (batch-strided view, _UpCat.backward)."""

    @staticmethod
    def forward(ctx, x):
        _require(x)
        L = _lib.lib()
        x = x.contiguous()
        n, c, d, h, w = x.shape
        assert d % 2 == 0 and h % 2 == 0 and w % 2 == 0, "max-pool kernels need even extents"
        y = torch.empty((n, c, d // 2, h // 2, w // 2), dtype=torch.float32, device=x.device)
        idx = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
        _lib.check(L.icl_maxpool2_fwd(_ptr(x), _ptr(y), _ptr(idx), n * c, d // 2, h // 2, w // 2, 2, _stream(x)), "maxpool2_fwd")
        ctx.save_for_backward(idx)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, gskip, gy):
        (idx,) = ctx.saved_tensors
        L = _lib.lib()
        n, c, d, h, w = idx.shape
        if gy is None:
            return gskip
        gy = gy.contiguous()
        gx = torch.empty((n, c, d * 2, h * 2, w * 2), dtype=torch.float32, device=gy.device)
        plane = 8 * d * h * w
        ok = (gskip is not None and gskip.dtype == torch.float32 and tuple(gskip.shape) == tuple(gx.shape)
              and gskip.stride()[1:] == (plane, 4 * h * w, 2 * w, 1) and gskip.stride(0) % 2 == 0 and gskip.data_ptr() % 8 == 0)
        if ok:
            # the mark stops here: a live-batch skip gradient meets the full pooling gradient.  Samples past the live batch take the
            # pooling gradient alone (no load of the skip addend, whose bytes there are zeros)
            k = live_of(gskip, n)
            if k is not None:
                _lib.check(L.icl_maxpool2_bwd_add_live(_ptr(gy), _ptr(idx), _vp(gskip.data_ptr()), _ptr(gx), n, k, c, d, h, w, 2,
                                                       gskip.stride(0), _stream(gy)), "maxpool2_bwd_add_live")
            else:
                _lib.check(L.icl_maxpool2_bwd_add(_ptr(gy), _ptr(idx), _vp(gskip.data_ptr()), _ptr(gx), n, c, d, h, w, 2, gskip.stride(0),
                                                  _stream(gy)), "maxpool2_bwd_add")
            return gx
        _lib.check(L.icl_maxpool2_bwd(_ptr(gy), _ptr(idx), _ptr(gx), n * c, d, h, w, 2, _stream(gy)), "maxpool2_bwd")
        return gx if gskip is None else gx + gskip


class _SkipAndPoolLazy(torch.autograd.Function):
    """_SkipAndPool on a deferred normalisation: the pooling reads the raw tensor and normalises on load; the skip output stays deferred."""

    @staticmethod
    def forward(ctx, t, ss):
        L = _lib.lib()
        n, c, d, h, w = t.shape
        y = torch.empty((n, c, d // 2, h // 2, w // 2), dtype=torch.float32, device=t.device)
        idx = torch.empty(y.shape, dtype=torch.uint8, device=t.device)
        _lib.check(L.icl_maxpool2_fwd_norm(_ptr(t), _ptr(ss), _ptr(y), _ptr(idx), n * c, d // 2, h // 2, w // 2, 2, _stream(t)), "maxpool2_fwd_norm")
        ctx.save_for_backward(idx)
        return t.view_as(t), y

    @staticmethod
    def backward(ctx, gskip, gy):
        return _SkipAndPool.backward(ctx, gskip, gy), None


def skip_and_pool(x):
    """Returns (x, MaxPool3d(2)(x)); use the FIRST output for the skip connection so that the backward can fuse the two gradients.
    ``x`` may be a ``LazyAct``: the skip output then is one too."""
    if isinstance(x, LazyAct):
        d, h, w = x.t.shape[2:]
        if d % 2 == 0 and h % 2 == 0 and w % 2 == 0 and x.t.is_contiguous():
            skip, pooled = _SkipAndPoolLazy.apply(x.t, x.ss)
            return LazyAct(skip, x.ss), pooled
        x = x.materialize()
    return _SkipAndPool.apply(x)


def max_pool3d_2(x: torch.Tensor) -> torch.Tensor:
    return _MaxPool2.apply(x, 2)


def max_pool2d_2(x: torch.Tensor) -> torch.Tensor:
    """nn.MaxPool2d(2) on [N,C,H,W] (networks/unet_icl.py:64), run as a D = 1 volume."""
    return _MaxPool2.apply(x.unsqueeze(2), 1).squeeze(2)


# --------------------------------------------------------------------------------------
# trilinear resize (align_corners=False) — networks/utils.py:264, utils/losses.py:263,292
# --------------------------------------------------------------------------------------

class _Trilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, align):
        _require(x)
        L = _lib.lib()
        x = x.contiguous()
        n, c, di, hi, wi = x.shape
        do, ho, wo = size
        y = torch.empty((n, c, do, ho, wo), dtype=torch.float32, device=x.device)
        _lib.check(L.icl_trilinear_fwd(_ptr(x), _ptr(y), n, c, di, hi, wi, do, ho, wo, c * do * ho * wo, align, _stream(x)),
                   "trilinear_fwd")
        ctx.in_shape = (n, c, di, hi, wi)
        ctx.align = align
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        gy = gy.contiguous()
        n, c, di, hi, wi = ctx.in_shape
        do, ho, wo = gy.shape[2:]
        gx = torch.empty(ctx.in_shape, dtype=torch.float32, device=gy.device)
        ws = _ws(L.icl_trilinear_bwd_ws_bytes(n, c, di, hi, wi, do, ho, wo), gy)
        _lib.check(L.icl_trilinear_bwd(_ptr(gy), _ptr(gx), _ptr(ws), n, c, di, hi, wi, do, ho, wo, c * do * ho * wo, ctx.align,
                                       _stream(gy)), "trilinear_bwd")
        return gx, None, None


def trilinear_resize(x: torch.Tensor, size: Sequence[int], align_corners: bool = False) -> torch.Tensor:
    return _Trilinear.apply(x, tuple(int(s) for s in size), int(bool(align_corners)))


def bilinear_resize(x: torch.Tensor, size: Sequence[int], align_corners: bool = False) -> torch.Tensor:
    """F.interpolate(mode='bilinear') / nn.Upsample(bilinear) on [N,C,H,W], run as a D = 1 volume."""
    return _Trilinear.apply(x.unsqueeze(2), (1, int(size[0]), int(size[1])), int(bool(align_corners))).squeeze(2)


class _UpCat(torch.autograd.Function):
    """cat([skip, upsample2x(deep)], 1) without materialising the upsampled tensor:
    the resize kernel writes straight into the channel slice of the concat buffer
    (UnetUp3_CT.forward, networks/utils.py:271-276)."""

    @staticmethod
    def forward(ctx, skip, deep):
        _require(skip, deep)
        L = _lib.lib()
        skip = skip.contiguous()
        deep = deep.contiguous()
        n, cs, d, h, w = skip.shape
        cd = deep.shape[1]
        assert deep.shape[0] == n and tuple(deep.shape[2:]) == (d // 2, h // 2, w // 2)
        s = d * h * w
        out = torch.empty((n, cs + cd, d, h, w), dtype=torch.float32, device=skip.device)
        _lib.check(L.icl_copy_rows(_ptr(skip), _ptr(out), n, cs * s, cs * s, (cs + cd) * s, _stream(skip)), "copy_rows")
        up_view = out[:, cs:]
        _lib.check(L.icl_trilinear_fwd(_ptr(deep), _vp(up_view.data_ptr()), n, cd, d // 2, h // 2, w // 2, d, h, w,
                                       (cs + cd) * s, 0, _stream(skip)), "trilinear_fwd")
        ctx.dims = (n, cs, cd, d, h, w)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        g = g.contiguous()
        n, cs, cd, d, h, w = ctx.dims
        s = d * h * w
        gskip = gdeep = None
        k = live_of(g, n)
        if ctx.needs_input_grad[0]:
            # a VIEW of the concat gradient, not a copy: the skip tensor also feeds the max-pool, so autograd adds this to the pooling
            # gradient right away (one strided read instead of a copy pass plus a read); a sole consumer makes it contiguous itself.
            # A view does not inherit the live-batch mark of its base: this one is marked explicitly (its tail is g's tail)
            gskip = mark_live(g[:, :cs], k)
        if ctx.needs_input_grad[1]:
            gdeep = torch.empty((n, cd, d // 2, h // 2, w // 2), dtype=torch.float32, device=g.device)
            gv = g[:, cs:]
            if k is not None:
                ws = _ws(L.icl_trilinear_bwd_ws_bytes(k, cd, d // 2, h // 2, w // 2, d, h, w), g)
                _lib.check(L.icl_trilinear_bwd_live(_vp(gv.data_ptr()), _ptr(gdeep), _ptr(ws), n, k, cd, d // 2, h // 2, w // 2, d, h, w,
                                                    (cs + cd) * s, 0, _stream(g)), "trilinear_bwd_live")
                mark_live(gdeep, k)
            else:
                ws = _ws(L.icl_trilinear_bwd_ws_bytes(n, cd, d // 2, h // 2, w // 2, d, h, w), g)
                _lib.check(L.icl_trilinear_bwd(_vp(gv.data_ptr()), _ptr(gdeep), _ptr(ws), n, cd, d // 2, h // 2, w // 2, d, h, w,
                                               (cs + cd) * s, 0, _stream(g)), "trilinear_bwd")
        return gskip, gdeep


class _UpCatLazy(torch.autograd.Function):
    """_UpCat with either source given as a deferred normalisation (raw tensor + (scale, shift), applied while it is copied / up-sampled
    into the concat buffer)."""

    @staticmethod
    def forward(ctx, skip, skip_ss, deep, deep_ss):
        L = _lib.lib()
        n, cs, d, h, w = skip.shape
        cd = deep.shape[1]
        out = torch.empty((n, cs + cd, d, h, w), dtype=torch.float32, device=skip.device)
        _lib.check(L.icl_upsample2x_concat_norm(_ptr(skip), _ptr(skip_ss), _ptr(deep), _ptr(deep_ss), _ptr(out), n, cs, cd, d, h, w,
                                                _stream(skip)), "upsample2x_concat_norm")
        ctx.dims = (n, cs, cd, d, h, w)
        return out

    @staticmethod
    def backward(ctx, g):
        ctx2 = ctx
        needs = ctx.needs_input_grad

        class _View:      # _UpCat.backward reads needs_input_grad[0] / [1] of (skip, deep)
            dims = ctx2.dims
            needs_input_grad = (needs[0], needs[2])
        gskip, gdeep = _UpCat.backward(_View, g)
        return gskip, None, gdeep, None


def upsample2x_concat(skip, deep) -> torch.Tensor:
    """cat([skip, upsample2x(deep)], 1); either argument may be a ``LazyAct`` (its normalisation is applied while it is read)."""
    if isinstance(skip, LazyAct) or isinstance(deep, LazyAct):
        st, dt = (skip.t if isinstance(skip, LazyAct) else skip), (deep.t if isinstance(deep, LazyAct) else deep)
        n, cs, d, h, w = st.shape
        ok = (d % 2 == 0 and h % 2 == 0 and w % 4 == 0 and tuple(dt.shape[2:]) == (d // 2, h // 2, w // 2) and dt.shape[0] == n
              and st.is_contiguous() and dt.is_contiguous() and st.dtype == torch.float32 and (st.is_cuda or _lib.host_pointers_ok()))
        if ok:
            return _UpCatLazy.apply(st, skip.ss if isinstance(skip, LazyAct) else None, dt, deep.ss if isinstance(deep, LazyAct) else None)
        skip, deep = materialized(skip), materialized(deep)
    return _UpCat.apply(skip, deep)


# --------------------------------------------------------------------------------------
# depthwise Conv3d 3^3 (groups = C, no bias) — SeparableConv3d.depthwise, unet_3D_icl.py:320-323
# --------------------------------------------------------------------------------------

class _DWConv3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        _require(x, weight)
        L = _lib.lib()
        x = x.contiguous()
        weight = weight.contiguous()
        n, c, d, h, w = x.shape
        assert tuple(weight.shape) == (c, 1, 3, 3, 3)
        y = torch.empty_like(x)
        _lib.check(L.icl_dwconv3_fwd(_ptr(x), _ptr(weight), _ptr(y), n, c, d, h, w, 0, _stream(x)), "dwconv3_fwd")
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        L = _lib.lib()
        gy = gy.contiguous()
        n, c, d, h, w = x.shape
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _lib.check(L.icl_dwconv3_fwd(_ptr(gy), _ptr(weight), _ptr(gx), n, c, d, h, w, 1, _stream(x)), "dwconv3_dgrad")
        if ctx.needs_input_grad[1]:
            gw = torch.empty_like(weight)
            ws = _ws(L.icl_dwconv3_wgrad_ws_bytes(n, c, d, h, w), x)
            _lib.check(L.icl_dwconv3_wgrad(_ptr(x), _ptr(gy), _ptr(gw), _ptr(ws), n, c, d, h, w, _stream(x)), "dwconv3_wgrad")
        return gx, gw


def depthwise_conv3d(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    return _DWConv3.apply(x, weight)


# --------------------------------------------------------------------------------------
# Dropout — nn.Dropout(p=0.3), unet_3D_icl.py:67-68
# --------------------------------------------------------------------------------------

def _mix32(x: int) -> int:
    """The 32-bit finaliser of csrc/kernels/misc.h (mix32), on the host."""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


class StepRNG:
    """Device-resident step counter for dropout under hipGraph replay: a captured launch bakes its scalar arguments in,
    so the per-step variation of the mask comes from this counter (incremented on the device at the end of every step and
    hashed into the seed by the kernel) and the per-call variation from a host-side call index that is identical in every
    replay.  The stream is keyed by ``torch.initial_seed()`` (so ``torch.manual_seed`` selects it) and by the data-parallel rank
    (every rank draws its own masks, as W independent reference processes would)."""
    tensor: Optional[torch.Tensor] = None
    calls = 0
    base = 0

    @classmethod
    def enable(cls, device, base_seed: Optional[int] = None, rank: Optional[int] = None):
        cls.tensor = torch.zeros(1, dtype=torch.int32, device=device)
        cls.calls = 0
        if base_seed is None:
            base_seed = torch.initial_seed()
        if rank is None:
            rank = torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
        cls.base = _mix32(_mix32(base_seed & 0xFFFFFFFF) ^ _mix32((base_seed >> 32) + 0x9E3779B1) ^ _mix32(rank + 0x85EBCA77))

    @classmethod
    def begin_step(cls):
        cls.calls = 0

    @classmethod
    def end_step(cls):
        if cls.tensor is not None:
            cls.tensor += 1

    @classmethod
    def next_seed(cls) -> int:
        """Seed of the next stochastic call of the step: a hash of (stream key, call index)."""
        seed = _mix32(cls.base ^ _mix32(cls.calls + 0x2545F491))
        cls.calls += 1
        return seed


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, seed_dev, group=1):
        _require(x)
        L = _lib.lib()
        x = x.contiguous()
        y = torch.empty_like(x)
        _lib.check(L.icl_drop_path(_ptr(x), _ptr(y), x.numel(), group, seed, p, _ptr(seed_dev), _stream(x)), "dropout")
        ctx.cfg = (p, seed, group)
        ctx.seed_dev = seed_dev
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        p, seed, group = ctx.cfg
        gy = gy.contiguous()
        gx = torch.empty_like(gy)
        _lib.check(L.icl_drop_path(_ptr(gy), _ptr(gx), gy.numel(), group, seed, p, _ptr(ctx.seed_dev), _stream(gy)), "dropout_bwd")
        return gx, None, None, None, None


class _DropPathAdd(torch.autograd.Function):
    """y = res + drop_path(x) in one kernel; ``res is x`` gives x + drop_path(x).  d/dres is the identity (the incoming gradient is
    handed on as is), d/dx the same per-sample mask applied to the gradient."""

    @staticmethod
    def forward(ctx, x, res, p, seed, seed_dev):
        _require(x, res)
        L = _lib.lib()
        x = x.contiguous()
        same = res is x or (res.data_ptr() == x.data_ptr() and res.shape == x.shape and res.is_contiguous())
        res = x if same else res.contiguous()
        assert res.shape == x.shape
        group = x.numel() // x.shape[0]
        y = torch.empty_like(x)
        _lib.check(L.icl_drop_path_add(_ptr(x), _ptr(res), _ptr(y), x.numel(), group, seed, p, _ptr(seed_dev), _stream(x)), "drop_path_add")
        ctx.cfg = (p, seed, group)
        ctx.seed_dev = seed_dev
        ctx.same = same
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        p, seed, group = ctx.cfg
        gx = None
        if ctx.same and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
            # x + drop_path(x) (the doubling of Class_Decoder, unet_3D_icl.py:264,266): both gradients belong to the same tensor —
            # gy + mask * gy in the forward kernel's one pass, handed back once, instead of a mask kernel plus an autograd add
            gy = gy.contiguous()
            gx = torch.empty_like(gy)
            _lib.check(L.icl_drop_path_add(_ptr(gy), _ptr(gy), _ptr(gx), gy.numel(), group, seed, p, _ptr(ctx.seed_dev), _stream(gy)),
                       "drop_path_add_bwd")
            return gx, None, None, None, None
        if ctx.needs_input_grad[0]:
            gy = gy.contiguous()
            gx = torch.empty_like(gy)
            _lib.check(L.icl_drop_path(_ptr(gy), _ptr(gx), gy.numel(), group, seed, p, _ptr(ctx.seed_dev), _stream(gy)), "drop_path_bwd")
        return gx, (gy if ctx.needs_input_grad[1] else None), None, None, None


def _step_seed(x, seed):
    seed_dev = None
    if seed is None:
        if StepRNG.tensor is not None and StepRNG.tensor.device == x.device:
            seed = StepRNG.next_seed()
            seed_dev = StepRNG.tensor
        else:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    return int(seed) & 0xFFFFFFFF, seed_dev


def _mix32_np(x):
    import numpy as np
    x = x.astype(np.uint32, copy=True)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def dropout_keep_mask(seed: int, numel: int, p: float, group: int = 1, step: Optional[int] = None, start: int = 0):
    """The keep / drop decisions of ``dropout_kernel`` / ``drop_apply`` (csrc/kernels/misc.h) restated on the host: a numpy bool array
    [numel], True where element i is kept.  ``seed``: the 32-bit seed handed to the kernel; ``step``: the value of the ``StepRNG`` device
    counter when one is in use (it is hashed into the seed as ``drop_seed`` does), None when the launch has no device counter;
    ``group``: elements per decision (``icl_drop_path``: one decision per sample); ``start``: index of the first element (the decisions
    of elements start .. start + numel - 1: a window of a tensor too large to enumerate).  Pure numpy, no GPU: the explicit mask against which
    every stochastic site — the in-kernel attention dropout included — is checked."""
    import numpy as np
    seed = int(seed) & 0xFFFFFFFF
    if step is not None:
        seed = _mix32(seed ^ _mix32((int(step) + 0x632BE5AB) & 0xFFFFFFFF))
    thresh = int(float(np.float32(p)) * 4294967296.0)      # (unsigned)((double)p * 2^32), p a C float
    i = np.arange(int(numel), dtype=np.uint64) + np.uint64(start)
    k = i // np.uint64(group) if group > 1 else i
    lo = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (k >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = _mix32_np(lo * np.uint32(0x9E3779B1) + np.uint32(seed)) ^ _mix32_np(hi + np.uint32((seed * 0x85EBCA77) & 0xFFFFFFFF))
    return h.astype(np.uint64) >= np.uint64(thresh)


def drop_path_add(res: torch.Tensor, x: torch.Tensor, p: float, training: bool = True, seed: Optional[int] = None) -> torch.Tensor:
    """res + DropPath(p)(x) — the residual update of a transformer block — as one kernel in training (a plain add otherwise).
    Same per-sample mask and seeding as ``drop_path``."""
    if p == 0.0 or not training:
        return res + x
    seed, seed_dev = _step_seed(x, seed)
    return _DropPathAdd.apply(x, res, float(p), seed, seed_dev)


def dropout(x: torch.Tensor, p: float, seed: Optional[int] = None) -> torch.Tensor:
    """Training-mode dropout.  Eager: the seed advances with torch's CPU generator (reproducible under manual_seed).
    With StepRNG enabled (graph capture): seed = call index, varied per step by the device-resident counter."""
    seed, seed_dev = _step_seed(x, seed)
    return _Dropout.apply(x, float(p), seed, seed_dev)


def _conv1x1_fusable(t, weight, also: bool) -> bool:
    """A 1x1x1 convolution of <= 16 -> <= 16 channels on a big volume that the fused dropout kernels take; ``also``: what the call site
    asks on top (dropout_conv1x1: autograd is recording; conv1x1_lazy: the raw tensor is contiguous)."""
    n, cin = t.shape[0], t.shape[1]
    s = t.numel() // max(n * cin, 1)
    return ((t.is_cuda or _lib.host_pointers_ok()) and weight.shape[2:].numel() == 1 and cin <= 16 and weight.shape[0] <= 16
            and s % 4 == 0 and n * s >= 65536 and also)


def _dropout_conv1x1_backward(ctx, x, weight, gy, needs, mask_dgrad, wgrad, what):
    """(gx, gw, gb) of _DropoutConv1x1 / _DropoutConv1x1Lazy.  ``needs``: (x, weight, bias) want a gradient; ``mask_dgrad``: the input
    gradient applies the dropout mask on its stores; ``wgrad``: the weight-gradient entry point, its operand pointers bound."""
    p, seed, has_bias = ctx.cfg
    L = _lib.lib()
    gy = gy.contiguous()
    n, cin, cout = x.shape[0], x.shape[1], weight.shape[0]
    s = x.numel() // (n * cin)
    gx = gw = gb = None
    k = live_of(gy, n)
    nl = n if k is None else k
    if needs[0]:
        gx = torch.empty_like(x)
        if mask_dgrad:
            _lib.check(L.icl_conv1x1_dropout_live(_ptr(gy), _ptr(weight), None, _ptr(gx), n, nl, cout, cin, s, 1, cin, 2, seed, p,
                                                  _ptr(ctx.seed_dev), _stream(x)), "conv1x1_dropout dgrad")
        else:
            _lib.check(L.icl_conv1x1_small_live(_ptr(gy), _ptr(weight), None, _ptr(gx), n, nl, cout, cin, s, 1, cin, _stream(x)),
                       "conv1x1_small dgrad")
        mark_live(gx, k)
    if needs[1] or (has_bias and needs[2]):
        gw = torch.empty_like(weight)
        gb = torch.empty(cout, dtype=torch.float32, device=x.device) if has_bias else None
        ws = _ws(L.icl_conv1x1_wgrad_ws_bytes(n, s, cin, cout), x)
        with _timed("conv1x1_wgrad_kernel", 2.0 * cin * cout * s * nl, 4.0 * nl * s * (cin + cout), x):
            _lib.check(wgrad(_ptr(gy), _ptr(gw), _ptr(gb), _ptr(ws), n, nl, cin, cout, s, cout * s, seed, p, _ptr(ctx.seed_dev), _stream(x)),
                       what)
    return gx, gw, gb


class _DropoutConv1x1(torch.autograd.Function):
    """conv1x1(dropout(x)) with the mask applied on the fly: forward (mask on the convolution's input loads), input gradient (mask on its
    stores) and weight gradient (mask on the x operand) each run as ONE pass — the dropped tensor never exists."""

    @staticmethod
    def forward(ctx, x, weight, bias, p, seed, seed_dev):
        _require(x, weight, bias)
        L = _lib.lib()
        x = x.contiguous()
        n, cin, cout = x.shape[0], x.shape[1], weight.shape[0]
        s = x.numel() // (n * cin)
        y = torch.empty((n, cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        _lib.check(L.icl_conv1x1_dropout(_ptr(x), _ptr(weight), _ptr(bias), _ptr(y), n, cin, cout, s, cin, 1, 1, seed, p, _ptr(seed_dev),
                                         _stream(x)), "conv1x1_dropout")
        ctx.save_for_backward(x, weight)
        ctx.cfg, ctx.seed_dev = (p, seed, bias is not None), seed_dev
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gx, gw, gb = _dropout_conv1x1_backward(ctx, x, weight, gy, ctx.needs_input_grad, True,
                                               lambda *a: _lib.lib().icl_conv1x1_wgrad_dropout_live(_ptr(x), *a), "conv1x1_wgrad_dropout")
        return gx, gw, gb, None, None, None


class _DropoutConv1x1Lazy(torch.autograd.Function):
    """_DropoutConv1x1 on a deferred normalisation: y = conv1x1(dropout(relu(fma(t, scale, shift)), p)) — InstanceNorm + ReLU, the dropout
    mask and the convolution in one pass over the raw tensor (p = 0: no mask); the weight gradient applies both on its x operand."""

    @staticmethod
    def forward(ctx, t, ss, weight, bias, p, seed, seed_dev):
        L = _lib.lib()
        n, cin, cout = t.shape[0], t.shape[1], weight.shape[0]
        s = t.numel() // (n * cin)
        y = torch.empty((n, cout) + tuple(t.shape[2:]), dtype=torch.float32, device=t.device)
        _lib.check(L.icl_conv1x1_dropout_norm(_ptr(t), _ptr(ss), _ptr(weight), _ptr(bias), _ptr(y), n, cin, cout, s, cin, 1, seed, p,
                                              _ptr(seed_dev), _stream(t)), "conv1x1_dropout_norm")
        ctx.save_for_backward(t, ss, weight)
        ctx.cfg, ctx.seed_dev = (p, seed, bias is not None), seed_dev
        return y

    @staticmethod
    def backward(ctx, gy):
        t, ss, weight = ctx.saved_tensors      # (gx: the gradient of the NORMALISED activation — what `t` stands for in the autograd graph)
        needs = ctx.needs_input_grad
        gx, gw, gb = _dropout_conv1x1_backward(ctx, t, weight, gy, (needs[0], needs[2], needs[3]), ctx.cfg[0] > 0.0,
                                               lambda *a: _lib.lib().icl_conv1x1_wgrad_dropout_norm_live(_ptr(t), _ptr(ss), *a),
                                               "conv1x1_wgrad_dropout_norm")
        return gx, None, gw, gb, None, None, None


def conv1x1_lazy(x, weight: torch.Tensor, bias: Optional[torch.Tensor], p: float = 0.0, seed: Optional[int] = None) -> torch.Tensor:
    """``conv3d(dropout(relu(norm(y)), p), weight, bias)`` for a 1x1x1 convolution whose input is a ``LazyAct`` — `final(dropout2(up1))`
    (unet_3D_icl.py:116-117) in one pass over the RAW output of up1's last convolution; p = 0: `final(up1)`.  Shapes the fused kernels do
    not take are materialised and run the ordinary operators."""
    if not isinstance(x, LazyAct):
        return dropout_conv1x1(x, weight, bias, p, seed) if p > 0.0 else conv3d(x, weight, bias)
    t = x.t
    if not _conv1x1_fusable(t, weight, t.is_contiguous()):
        a = x.materialize()
        return dropout_conv1x1(a, weight, bias, p, seed) if p > 0.0 else conv3d(a, weight, bias)
    seed, seed_dev = _step_seed(t, seed) if p > 0.0 else (int(seed or 0) & 0xFFFFFFFF, None)      # p = 0: no mask, no seed drawn
    return _DropoutConv1x1Lazy.apply(t, x.ss, weight.contiguous(), bias, float(p), seed, seed_dev)


def dropout_conv1x1(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], p: float, seed: Optional[int] = None) -> torch.Tensor:
    """``conv3d(dropout(x, p), weight, bias)`` for a 1x1x1 (or 1x1) convolution of <= 16 channels on a big volume — `final(dropout2(up1))` of
    the backbones (unet_3D_icl.py:67-68,117) — without materialising the dropped tensor.  Same seed protocol and the same mask as
    ``dropout`` (so the results are those of the two-op form, bit for bit); other shapes take the two-op form."""
    if not _conv1x1_fusable(x, weight, torch.is_grad_enabled()):
        return conv3d(dropout(x, p, seed), weight, bias)
    seed, seed_dev = _step_seed(x, seed)
    return _DropoutConv1x1.apply(x, weight, bias, float(p), seed, seed_dev)


def drop_path(x: torch.Tensor, p: float, seed: Optional[int] = None) -> torch.Tensor:
    """Per-sample stochastic depth (timm / MONAI DropPath): each sample of the batch keeps its branch with probability 1-p (scaled
    by 1/(1-p)) or drops it entirely — one kernel instead of empty + bernoulli_ + div + mul; same seeding scheme as ``dropout``."""
    seed, seed_dev = _step_seed(x, seed)
    return _Dropout.apply(x, float(p), seed, seed_dev, x.numel() // x.shape[0])


# --------------------------------------------------------------------------------------
# Aligner token ops (unet_3D_icl.py:244-315): LayerNorm, GELU and the prototype attention are HIP kernels
# (csrc/kernels/token.h); the Linear layers (incl. the 13,824^2 mlp2) run on csrc/kernels/gemm.h — the skinny mlp2 products
# stream the weight matrix once per launch (5.4-5.8 TB/s, profiles/), the others use the LDS-tiled fp32 MFMA product.
# --------------------------------------------------------------------------------------

LINEAR_WGRAD_MIN_ROWS = 2048
LINEAR_BWD_ONE_LAUNCH = True


def linear_forward_raw(x2: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0) -> torch.Tensor:
    """act(x2 W^T + b) for row-major x2 [rows, in], W [out, in] (csrc/kernels/gemm.h: weight streaming for <= 32 rows and
    >= 2^20 weights, LDS-tiled fp32 MFMA product otherwise)."""
    _require(x2, weight, bias)
    L = _lib.lib()
    rows, i = x2.shape
    o = weight.shape[0]
    y = torch.empty((rows, o), dtype=torch.float32, device=x2.device)
    need = L.icl_linear_ws_bytes(rows, i, o, 0)
    ws = _ws(need, x2) if need else None
    big = rows <= 32 and i * o >= (1 << 26)      # the 13,824^2 matrices: reported separately (bench.py roofline.mlp2_weight_stream)
    with _timed("linear_stream_fwd" if big else "linear_fwd", 2.0 * rows * i * o, 4.0 * (i * o if big else rows * (i + o) + i * o), x2):
        _lib.check(L.icl_linear_fwd(_ptr(x2), _ptr(weight), _ptr(bias), _ptr(y), _ptr(ws), rows, i, o, act, _stream(x2)), "linear_fwd")
    return y


def linear_dgrad_raw(g2: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """g2 W for row-major g2 [rows, out], W [out, in] -> [rows, in]."""
    _require(g2, weight)
    L = _lib.lib()
    rows, o = g2.shape
    i = weight.shape[1]
    gx = torch.empty((rows, i), dtype=torch.float32, device=g2.device)
    need = L.icl_linear_ws_bytes(rows, i, o, 1)
    ws = _ws(need, g2) if need else None
    big = rows <= 32 and i * o >= (1 << 26)
    with _timed("linear_stream_dgrad" if big else "linear_dgrad", 2.0 * rows * i * o, 4.0 * (i * o if big else rows * (i + o) + i * o), g2):
        _lib.check(L.icl_linear_dgrad(_ptr(g2), _ptr(weight), _ptr(gx), _ptr(ws), rows, i, o, _stream(g2)), "linear_dgrad")
    return gx


def gemm(a: torch.Tensor, b: torch.Tensor, m: int, n: int, k: int, lda: int, ldb: int, a_kcontig: bool, b_kcontig: bool,
         out: Optional[torch.Tensor] = None, ldc: Optional[int] = None, bias: Optional[torch.Tensor] = None, act: int = 0, batch: int = 1,
         a_bstride: int = 0, b_bstride: int = 0, c_bstride: int = 0) -> torch.Tensor:
    """C[b] = act(A[b] B[b] + bias) through icl_gemm (include/icl_hip.h): operands are described by their pitches, so transposed
    views are consumed in place (no transpose copies)."""
    _require(a, b, bias)
    L = _lib.lib()
    if out is None:
        out = torch.empty((batch, m, n) if batch > 1 else (m, n), dtype=torch.float32, device=a.device)
        ldc, c_bstride = n, m * n
    need = L.icl_gemm_ws_bytes(m, n, k, batch)
    ws = _ws(need, a) if need else None
    with _timed("gemm", 2.0 * batch * m * n * k, 4.0 * batch * (m * k + k * n + m * n), a):
        _lib.check(L.icl_gemm(_ptr(a), _ptr(b), _ptr(out), _ptr(bias), _ptr(ws), m, n, k, lda, ldb, ldc, int(a_kcontig), int(b_kcontig),
                              act, batch, a_bstride, b_bstride, c_bstride, _stream(a)), "gemm")
    return out


def _tall_atb(a: torch.Tensor, b: torch.Tensor, want_colsum: bool):
    """a^T b for row-major a [rows, A], b [rows, B] (-> [A, B]) and, optionally, the column sums of a (-> [A]).
    rows >= LINEAR_WGRAD_MIN_ROWS: csrc/kernels/linear_wgrad.h (rows split over many waves); otherwise the tiled product of
    csrc/kernels/gemm.h with both operands k-strided."""
    rows, A = a.shape
    B = b.shape[1]
    _require(a, b)
    L = _lib.lib()
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty((A, B), dtype=torch.float32, device=a.device)
    if rows < LINEAR_WGRAD_MIN_ROWS:
        need = L.icl_linear_ws_bytes(rows, B, A, 2)
        ws = _ws(need, a) if need else None
        with _timed("linear_wgrad_small", 2.0 * rows * A * B, 4.0 * (rows * (A + B) + A * B), a):
            _lib.check(L.icl_linear_wgrad_small(_ptr(a), _ptr(b), _ptr(out), _ptr(ws), rows, B, A, _stream(a)), "linear_wgrad_small")
        return out, (a.sum(0) if want_colsum else None)
    colsum = torch.empty(A, dtype=torch.float32, device=a.device) if want_colsum else None
    ws = _ws(L.icl_linear_wgrad_ws_bytes(rows, A, B), a)
    with _timed("linear_wgrad_kernel", 2.0 * rows * A * B, 4.0 * rows * (A + B), a):
        _lib.check(L.icl_linear_wgrad(_ptr(a), _ptr(b), _ptr(out), _ptr(colsum), _ptr(ws), rows, A, B, _stream(a)), "linear_wgrad")
    return out, colsum


class _Linear(torch.autograd.Function):
    """y = x W^T + b.  Forward and dx: csrc/kernels/gemm.h (fp32 MFMA; the weight is streamed once for skinny inputs); dW/db of TALL
    inputs (>= 2048 rows: the Swin token grids) use csrc/kernels/linear_wgrad.h, of short ones the k-strided tiled product."""

    @staticmethod
    def forward(ctx, x, weight, bias, owner=None, lane_wgrad=False):
        weight = weight.contiguous()
        x2 = x.reshape(-1, weight.shape[1]).contiguous()
        ctx.save_for_backward(x2, weight)
        ctx.lane_wgrad = bool(lane_wgrad)
        # the gradient is returned for `weight` as passed (a view of the convolution weight in _conv3d_tiny_volume): adoption is
        # decided on the Parameter behind it
        ctx.lane_param = owner.weight if owner is not None and getattr(owner, "weight", None) is not None else (
            weight._base if weight._base is not None else weight)
        if lane_wgrad:
            WgradLane.note_use(ctx.lane_param)
        ctx.has_bias = bias is not None
        # the Parameter behind the bias (for DeferredBiasGrads: all small bias gradients of a step reduced in one launch): the
        # owner's, or the argument itself when the caller passed a Parameter without naming its module
        ctx.bias_param = (owner.bias if (owner is not None and bias is not None and getattr(owner, "bias", None) is bias)
                          else (bias if isinstance(bias, torch.nn.Parameter) else None))
        ctx.x_shape = x.shape
        return linear_forward_raw(x2, weight, bias).view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x2, weight = ctx.saved_tensors
        o, i = weight.shape
        gx = gw = gb = None
        g2 = gy.reshape(-1, o).contiguous()
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        if need_b and ctx.bias_param is not None and g2.shape[0] < LINEAR_WGRAD_MIN_ROWS and DeferredBiasGrads.defer(ctx.bias_param, g2):
            need_b = False      # reduced with all the other bias gradients of the step (DeferredBiasGrads.flush)
        if ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and g2.shape[0] <= 32 and LINEAR_BWD_ONE_LAUNCH:
            # few rows (the aligner's query-side layers): input gradient and weight gradient in ONE launch — these layers sit on the
            # backward chains the step waits for, where a dependent launch costs 10-15 us (profiles/r4_timeline.md)
            _require(g2, weight, x2)
            L = _lib.lib()
            rows = g2.shape[0]
            gx2 = torch.empty((rows, i), dtype=torch.float32, device=g2.device)
            gw2 = torch.empty((o, i), dtype=torch.float32, device=g2.device)
            need = L.icl_linear_ws_bytes(rows, i, o, 1)
            ws = _ws(need, g2) if need else None
            rc = L.icl_linear_bwd_small(_ptr(g2), _ptr(weight), _ptr(x2), _ptr(gx2), _ptr(gw2), _ptr(ws), rows, i, o, _stream(g2))
            if rc == 0:
                return gx2.view(ctx.x_shape), gw2, (g2.sum(0) if need_b else None), None, None
            if rc != 1:      # 1: shapes that do not take that path
                _lib.check(rc, "linear_bwd_small")
        # the product form of a 6^3 convolution (conv3d on tiny volumes): its weight gradient goes to the lane of the deep levels' weight gradients
        lane = ctx.lane_wgrad and ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and not need_b and WgradLane.wants(g2, 0)
        if lane:
            WgradLane.fork_point(g2)
        if ctx.needs_input_grad[0]:
            gx = linear_dgrad_raw(g2, weight).view(ctx.x_shape)
        if ctx.needs_input_grad[1] or need_b:
            if ctx.needs_input_grad[1]:
                if lane:
                    with WgradLane.on_lane(g2, x2):
                        gw, gb = _tall_atb(g2, x2, False)
                    if not WgradLane.adoptable(ctx.lane_param):
                        WgradLane.sync_to_current(gw)
                else:
                    gw, gb = _tall_atb(g2, x2, need_b)
            elif need_b:
                gb = g2.sum(0)
        return gx, gw, gb, None, None


class _ConvTransposeGemm(torch.autograd.Function):
    """y[b, s, :] = sum_ci x[b, ci, s] W[ci, :] — the k2s2 transposed convolution as ONE batched product whose A operand is the
    channel-major activation itself (k-strided: no transpose copy); gx comes back channel-major, gW is summed over the batch."""

    @staticmethod
    def forward(ctx, x, w2):
        x = x.contiguous()
        w2 = w2.contiguous()
        b, cin = x.shape[0], x.shape[1]
        s = x.numel() // (b * cin)
        j = w2.shape[1]
        ctx.save_for_backward(x, w2)
        return gemm(x, w2, s, j, cin, s, j, False, False, batch=b, a_bstride=cin * s)        # [b, s, j]

    @staticmethod
    def backward(ctx, gy):
        x, w2 = ctx.saved_tensors
        gy = gy.contiguous()
        b, cin = x.shape[0], x.shape[1]
        s = x.numel() // (b * cin)
        j = w2.shape[1]
        gx = gw = None
        if ctx.needs_input_grad[0]:
            # gx[b][ci][s] = sum_j W[ci][j] gy[b][s][j]
            gx = torch.empty_like(x)
            gemm(w2, gy, cin, s, j, j, j, True, True, out=gx, ldc=s, batch=b, b_bstride=s * j, c_bstride=cin * s)
        if ctx.needs_input_grad[1]:
            # gW[ci][j] = sum_{b,s} x[b][ci][s] gy[b][s][j]: one product per sample, summed
            gw = torch.empty_like(w2)
            gemm(x, gy, cin, j, s, s, j, True, False, out=gw, ldc=j, batch=b, a_bstride=cin * s, b_bstride=s * j, c_bstride=0)
        return gx, gw


class _LinearFactored(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, owner):
        weight = weight.contiguous()
        x2 = x.reshape(-1, weight.shape[1]).contiguous()
        ctx.save_for_backward(x2, weight)
        ctx.owner = owner
        ctx.has_bias = bias is not None
        ctx.x_shape = x.shape
        return linear_forward_raw(x2, weight, bias).view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x2, weight = ctx.saved_tensors
        o, i = weight.shape
        g2 = gy.reshape(-1, o).contiguous()
        param = ctx.owner.weight
        gb = None
        if ctx.has_bias and ctx.needs_input_grad[2] and not (g2.shape[0] < LINEAR_WGRAD_MIN_ROWS
                                                             and DeferredBiasGrads.defer(getattr(ctx.owner, "bias", None), g2)):
            gb = g2.sum(0)
        scope = StepScope.current
        opt = scope.fused_optimizer if scope is not None else None
        if (opt is not None and ctx.needs_input_grad[0] and scope.factor_uses.get(id(param)) == 1
                and weight.data_ptr() == param.data_ptr() and opt.can_update_in_backward(param, g2.shape[0])):
            # input gradient from the old weight and the SGD step of the weight, one pass over the matrix
            return opt.update_in_backward(param, g2, x2).view(ctx.x_shape), None, gb, None
        gx = linear_dgrad_raw(g2, weight).view(ctx.x_shape) if ctx.needs_input_grad[0] else None
        if getattr(param, "_icl_factors", None) is None:
            param._icl_factors = []
        param._icl_factors.append((g2, x2))
        return gx, None, gb, None


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], owner=None, lane_wgrad: bool = False) -> torch.Tensor:
    """F.linear.  ``owner``: the module whose ``.weight`` this is — lets the gradient stay factored (see FactoredGrads)."""
    scope = StepScope.current
    if scope is not None and scope.factor_uses is not None:
        # every use of a weight in this step, whichever autograd path it takes below: the update-inside-backward of
        # _LinearFactored is only legal for a weight that is read exactly once per step
        key = id(owner.weight) if owner is not None and getattr(owner, "weight", None) is not None else id(weight)
        scope.factor_uses[key] = scope.factor_uses.get(key, 0) + 1
    if (owner is not None and FactoredGrads.enabled and weight.requires_grad and weight.numel() >= FactoredGrads.min_elems
            and x.numel() // x.shape[-1] <= FactoredGrads.max_rows
            and (x.numel() // x.shape[-1]) * (1 if scope is None else scope.world)
            <= (FactoredGrads.max_rows_gathered if scope is None else scope.max_rows_gathered)
            and weight.shape[1] % 4 == 0 and torch.is_grad_enabled()):
        return _LinearFactored.apply(x, weight, bias, owner)
    return _Linear.apply(x, weight, bias, owner, lane_wgrad)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        _require(x, weight, bias)
        L = _lib.lib()
        x = x.contiguous()
        c = x.shape[-1]
        rows = x.numel() // c
        y = torch.empty_like(x)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        _lib.check(L.icl_layernorm_fwd(_ptr(x), _ptr(weight), _ptr(bias), _ptr(y), _ptr(mean), _ptr(rstd), rows, c, eps, _stream(x)),
                   "layernorm_fwd")
        ctx.save_for_backward(x, weight, mean, rstd)
        both = isinstance(weight, torch.nn.Parameter) and isinstance(bias, torch.nn.Parameter)
        ctx.params = (weight, bias) if both and weight.requires_grad and bias.requires_grad else None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, mean, rstd = ctx.saved_tensors
        L = _lib.lib()
        gy = gy.contiguous()
        c = x.shape[-1]
        rows = x.numel() // c
        gx = torch.empty_like(x)
        dg = db = ws = None       # no-affine: F.layer_norm(x, [C]) (swinunetr_icl.py:1214)
        defer = False
        if weight is not None:
            ws = _ws(L.icl_layernorm_bwd_ws_bytes(rows, c), x)
            # inside ICLTrainer's step the chunk partials of all LayerNorm layers are summed by ONE launch at the end of backward
            # (DeferredBiasGrads.flush); elsewhere on the spot.  Either way in a fixed order: no float atomics.
            scope = StepScope.current
            defer = scope is not None and scope.bias_grads is not None and ctx.params is not None
            if not defer:
                dgb = torch.empty((2, c), dtype=torch.float32, device=x.device)
                dg, db = dgb[0], dgb[1]
        _lib.check(L.icl_layernorm_bwd(_ptr(gy), _ptr(x), _ptr(weight), _ptr(mean), _ptr(rstd), _ptr(gx), _ptr(dg), _ptr(db), _ptr(ws), rows, c,
                                       _stream(x)), "layernorm_bwd")
        if defer:
            part = ws[:(ws.numel() // (2 * c)) * 2 * c].view(2, -1, c)
            scope.bias_grads.append((ctx.params[0], part[0]))
            scope.bias_grads.append((ctx.params[1], part[1]))
            DeferredBiasGrads.note_producer(part)
            BackwardEnd.arm()
        return gx, dg, db, None


def layer_norm(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float = 1e-5) -> torch.Tensor:
    return _LayerNorm.apply(x, weight, bias, eps)


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require(x)
        L = _lib.lib()
        x = x.contiguous()
        y = torch.empty_like(x)
        _lib.check(L.icl_gelu_fwd(_ptr(x), _ptr(y), x.numel(), _stream(x)), "gelu_fwd")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        L = _lib.lib()
        gy = gy.contiguous()
        gx = torch.empty_like(x)
        _lib.check(L.icl_gelu_bwd(_ptr(gy), _ptr(x), _ptr(gx), x.numel(), _stream(x)), "gelu_bwd")
        return gx


def gelu(x: torch.Tensor) -> torch.Tensor:
    return _Gelu.apply(x)


# --------------------------------------------------------------------------------------
# SwinUNETR pieces (networks/swinunetr_icl.py)
# --------------------------------------------------------------------------------------

class _DepthToSpaceCat(torch.autograd.Function):
    """[depth_to_space(yt) | skip] along channels in one buffer: the GEMM result of the k2s2 transposed convolution is moved
    straight into the channel slice of the concat buffer MONAI's UnetrUpBlock builds (``torch.cat((out, skip), 1)``)."""

    @staticmethod
    def forward(ctx, yt, skip, dims):
        _require(yt, skip)
        L = _lib.lib()
        n, d, h, w, cout = dims
        yt = yt.contiguous()
        so = 8 * d * h * w
        cs = 0 if skip is None else skip.shape[1]
        out = torch.empty((n, cout + cs, 2 * d, 2 * h, 2 * w), dtype=torch.float32, device=yt.device)
        _lib.check(L.icl_depth_to_space2(_ptr(yt), _ptr(out), n, d, h, w, cout, (cout + cs) * so, _stream(yt)), "depth_to_space2")
        if cs:
            skip = skip.contiguous()
            _lib.check(L.icl_copy_rows(_ptr(skip), _vp(out[:, cout:].data_ptr()), n, cs * so, cs * so, (cout + cs) * so, _stream(yt)),
                       "copy_rows")
        ctx.dims = (n, d, h, w, cout, cs)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        n, d, h, w, cout, cs = ctx.dims
        g = g.contiguous()
        so = 8 * d * h * w
        gt = gskip = None
        if ctx.needs_input_grad[0]:
            gt = torch.empty((n, d * h * w, cout * 8), dtype=torch.float32, device=g.device)
            _lib.check(L.icl_space_to_depth2(_ptr(g), _ptr(gt), n, d, h, w, cout, (cout + cs) * so, _stream(g)), "space_to_depth2")
        if cs and ctx.needs_input_grad[1]:
            gskip = torch.empty((n, cs, 2 * d, 2 * h, 2 * w), dtype=torch.float32, device=g.device)
            _lib.check(L.icl_copy_rows(_vp(g[:, cout:].data_ptr()), _ptr(gskip), n, cs * so, (cout + cs) * so, cs * so, _stream(g)),
                       "copy_rows")
        return gt, gskip, None


def conv_transpose3d_k2s2(x: torch.Tensor, weight: torch.Tensor, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.ConvTranspose3d(cin, cout, kernel 2, stride 2, no bias) — MONAI UnetrUpBlock.transp_conv — optionally followed by
    ``torch.cat((up, skip), 1)``.  Kernel == stride, so the output voxels do not overlap:
    out[b, co, 2z+i, 2y+j, 2x+k] = sum_ci x[b, ci, z, y, x] * W[ci, co, i, j, k], i.e. ONE product
    [B*S, Cin] x [Cin, Cout*8] on the fp32 matrix cores (csrc/kernels/gemm.h, reading the channel-major activation in place)
    followed by a depth-to-space move (csrc/kernels/pool_resize.h) that writes straight into the concat buffer."""
    b, cin, d, h, w = x.shape
    cout = weight.shape[1]
    y = _ConvTransposeGemm.apply(x, weight.flatten(1))          # [B, S, Cout*8]
    return _DepthToSpaceCat.apply(y, skip, (b, d, h, w, cout))


class _GatherRows(torch.autograd.Function):
    """out[b, m] = src[b, idx[m]] (zero row for idx[m] < 0); ``idx_back`` is the index that undoes it (gradient = gather again)."""

    @staticmethod
    def forward(ctx, src, idx, idx_back):
        _require(src, idx, idx_back)
        L = _lib.lib()
        src = src.contiguous()
        b, s, c = src.shape
        m = idx.shape[0]
        assert idx_back.shape[0] == s
        out = torch.empty((b, m, c), dtype=torch.float32, device=src.device)
        _lib.check(L.icl_gather_rows(_ptr(src), _ptr(idx), _ptr(out), b, s, m, c, _stream(src)), "gather_rows")
        ctx.save_for_backward(idx, idx_back)
        return out

    @staticmethod
    def backward(ctx, g):
        idx, idx_back = ctx.saved_tensors
        L = _lib.lib()
        g = g.contiguous()
        b, m, c = g.shape
        s = idx_back.shape[0]
        gs = torch.empty((b, s, c), dtype=torch.float32, device=g.device)
        _lib.check(L.icl_gather_rows(_ptr(g), _ptr(idx_back), _ptr(gs), b, m, s, c, _stream(g)), "gather_rows")
        return gs, None, None


def gather_rows(src: torch.Tensor, idx: torch.Tensor, idx_back: torch.Tensor) -> torch.Tensor:
    """src [B, S, C] -> [B, M, C] with out[:, m] = src[:, idx[m]] (zeros where idx[m] < 0).  ``idx`` must reference every source
    row exactly once (a permutation with optional padding slots) and ``idx_back`` [S] must be its inverse."""
    return _GatherRows.apply(src, idx, idx_back)


# --------------------------------------------------------------------------------------
# Live batch (DESIGN.md §4.4 "Live batch"): "samples [0, k) of this gradient hold values, samples [k, n) are exactly zero" — in MEMORY too: the tail is
# always written, so a consumer that does not know the mark reads a correct gradient.  The unlabeled stream's logits enter the loss only
# as a detached target (utils/losses.py:294), so autograd hands _SplitBatch.backward no gradient for them; every Function of the upper
# decoder's backward (all per sample) then runs its kernels on the live samples and passes the mark on with its input gradient.
# --------------------------------------------------------------------------------------

_LIVE_ATTR = "_icl_live_batch"


def live_batch_enabled() -> bool:
    """ICL_LIVE_BATCH=0 (read per call): no mark is ever created — every backward launches what it launched without this."""
    return os.environ.get("ICL_LIVE_BATCH", "1") != "0"


def mark_live(t: Optional[torch.Tensor], k: Optional[int]):
    """Marks ``t`` (the caller has WRITTEN zeros to t[k:]) as live on samples [0, k); returns ``t``.  The mark is an attribute of this
    tensor object — a view, slice or copy of it does not carry it — and holds the tensor's version: an in-place write (autograd
    accumulating into the buffer) voids it.  k None / 0 / >= n: nothing to mark."""
    if t is None or k is None or t.dim() == 0 or not (0 < int(k) < t.shape[0]) or not live_batch_enabled():
        return t
    setattr(t, _LIVE_ATTR, (int(k), t._version))
    return t


def live_of(t: Optional[torch.Tensor], n: int) -> Optional[int]:
    """The live sample count of gradient ``t`` of a batch of ``n``, or None: full batch (no mark, a stale one, another leading dimension)."""
    m = getattr(t, _LIVE_ATTR, None) if t is not None else None
    if m is None or not live_batch_enabled():
        return None
    k, version = m
    if version != t._version or t.dim() == 0 or t.shape[0] != n or not (0 < k < n):
        return None
    return k


class _SplitBatch(torch.autograd.Function):
    """(x[:k], x[k:]) whose gradient is ONE concatenation; two Python slices cost two zero fills, two copies and an add.  A missing second
    half is the one producer of a live-batch mark (``mark_live``)."""

    @staticmethod
    def forward(ctx, x, k):
        ctx.k, ctx.n = int(k), x.shape[0]
        ctx.tail = tuple(x.shape[1:])
        ctx.set_materialize_grads(False)
        return x[:k], x[k:]

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None and gb is None:
            return None, None
        ref = ga if ga is not None else gb
        na, nb = ctx.k * math.prod(ctx.tail), (ctx.n - ctx.k) * math.prod(ctx.tail)
        ok = ref.dtype == torch.float32 and na % 4 == 0 and nb % 4 == 0 and (ref.is_cuda or _lib.host_pointers_ok())
        if ok:
            # one launch, whichever halves exist (a missing half is written as zeros)
            ga = ga.contiguous() if ga is not None else None
            gb = gb.contiguous() if gb is not None else None
            out = torch.empty((ctx.n,) + ctx.tail, dtype=torch.float32, device=ref.device)
            if all(t is None or t.data_ptr() % 16 == 0 for t in (ga, gb)):
                _lib.check(_lib.lib().icl_concat2(_ptr(ga), na, _ptr(gb), nb, _ptr(out), _stream(ref)), "concat2")
                return mark_live(out, ctx.k if gb is None else None), None
        live = ctx.k if (gb is None and ga is not None) else None
        if ga is None:
            ga = ref.new_zeros((ctx.k,) + ctx.tail)
        if gb is None:
            gb = ref.new_zeros((ctx.n - ctx.k,) + ctx.tail)
        return mark_live(torch.cat([ga, gb], 0), live), None


def cat_batch(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """torch.cat([a, b], 0) — without the copies when the two already ARE one batch: contiguous slices `v[:k]`, `v[k:]` of one tensor
    that need no gradient (the trainers split their batch that way, train_inherent_consistent_unet_3D_BraTS.py:103-104, and the ICL models
    run both streams as one batch): a view over both instead of two device copies at the head of every step."""
    if (a.dim() == b.dim() and a.shape[1:] == b.shape[1:] and a.dtype == b.dtype and a.device == b.device and a.is_contiguous()
            and b.is_contiguous() and not a.requires_grad and not b.requires_grad and a.numel() > 0 and b.numel() > 0
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.data_ptr() == a.data_ptr() + a.numel() * a.element_size()):
        return a.as_strided((a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), a.stride())
    return torch.cat([a, b], 0)


def split_batch(x: torch.Tensor, k: int):
    """x[:k], x[k:] (views) with a single-kernel gradient."""
    return _SplitBatch.apply(x, k)


class _GatherRowsDup(torch.autograd.Function):
    """Row gather whose index may repeat or omit source rows (PatchMerging); ``idx_back2`` [S, 2] lists for every source row the
    (at most two) output rows that read it, -1 where absent, so the gradient is again a deterministic gather."""

    @staticmethod
    def forward(ctx, src, idx, idx_back2):
        _require(src, idx, idx_back2)
        L = _lib.lib()
        src = src.contiguous()
        b, s, c = src.shape
        m = idx.shape[0]
        assert tuple(idx_back2.shape) == (s, 2)
        out = torch.empty((b, m, c), dtype=torch.float32, device=src.device)
        _lib.check(L.icl_gather_rows(_ptr(src), _ptr(idx), _ptr(out), b, s, m, c, _stream(src)), "gather_rows")
        ctx.save_for_backward(idx_back2)
        return out

    @staticmethod
    def backward(ctx, g):
        (idx_back2,) = ctx.saved_tensors
        L = _lib.lib()
        g = g.contiguous()
        b, m, c = g.shape
        s = idx_back2.shape[0]
        gs = torch.empty((b, s, c), dtype=torch.float32, device=g.device)
        _lib.check(L.icl_gather_rows_sum2(_ptr(g), _ptr(idx_back2), _ptr(gs), b, m, s, c, _stream(g)), "gather_rows_sum2")
        return gs, None, None


def gather_rows_dup(src: torch.Tensor, idx: torch.Tensor, idx_back2: torch.Tensor) -> torch.Tensor:
    """src [B, S, C] -> [B, M, C], out[:, m] = src[:, idx[m]]; every source row is read by at most two output rows, listed in
    ``idx_back2`` [S, 2] (int32, -1 = none)."""
    return _GatherRowsDup.apply(src, idx, idx_back2)


_RELPOS_INV = {}


def _relpos_inverse(index: torch.Tensor, n: int, table_rows: int):
    """(inv, offs) of ``relative_position_index[:n, :n]``: the padded positions i * npad + j sorted by table row (stable) and the
    row offsets — what icl_relpos_bias_bwd_sum walks to add the bias gradient in a fixed order.  Built once per (index buffer, n) on the
    host (a buffer that never changes); the first call must not happen under graph capture (every trainer warms up eagerly)."""
    key = (index.data_ptr(), int(index._version), n, table_rows, str(index.device))
    hit = _RELPOS_INV.get(key)
    if hit is None:
        if index.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("icl_amd window attention: the inverse of relative_position_index must be built before graph capture "
                               "(run one eager backward first)")
        npad = (n + 15) // 16 * 16
        idx = index[:n, :n].reshape(-1).to("cpu", torch.int64)
        order = torch.argsort(idx, stable=True)
        inv = ((order // n) * npad + order % n).to(torch.int32)
        offs = torch.zeros(table_rows + 1, dtype=torch.int64)
        offs[1:] = torch.cumsum(torch.bincount(idx, minlength=table_rows), 0)
        hit = _RELPOS_INV[key] = (inv.to(index.device), offs.to(torch.int32).to(index.device))
    return hit


class _WindowAttention(torch.autograd.Function):
    """One fused MFMA kernel per direction (csrc/kernels/winattn.h): scores, bias, shift mask, softmax and P@V never leave
    the CU; backward recomputes the scores from the saved log-sum-exp.  The relative-position bias is gathered from the
    table into the kernel's padded [heads, n, npad] layout by a small kernel (and its gradient scattered back)."""

    @staticmethod
    def forward(ctx, qkv, table, index, regions, heads, scale, attn_drop=0.0, seed=0, seed_dev=None):
        _require(qkv, table, index, regions)
        L = _lib.lib()
        qkv = qkv.contiguous()
        b_, n, c3 = qkv.shape
        c = c3 // 3
        dh = c // heads
        if c != heads * dh or dh not in (16, 32):
            raise ValueError("icl_amd window attention: head dim must be 16 (SwinUNETR) or 32 (2-D Swin-UNet)")
        if table.shape[1] != heads or index.dim() != 2 or index.shape[0] != index.shape[1] or n > index.shape[0]:
            raise ValueError("icl_amd window attention: table [T, heads] / index [N, N] with n <= N expected")
        table, index = table.contiguous(), index.contiguous()
        npad = (n + 15) // 16 * 16
        bias_pad = torch.empty((heads, n, npad), dtype=torch.float32, device=qkv.device)
        _lib.check(L.icl_relpos_bias_fwd(_ptr(table), _ptr(index), _ptr(bias_pad), n, heads, index.shape[0], _stream(qkv)), "relpos_bias_fwd")
        nw = regions.shape[0] if regions is not None else 1
        out = torch.empty((b_, n, c), dtype=torch.float32, device=qkv.device)
        lse = torch.empty((b_, heads, n), dtype=torch.float32, device=qkv.device)
        flops = 4.0 * b_ * heads * n * n * dh
        with _timed("window_attn_fwd_kernel", flops, 4.0 * (qkv.numel() + out.numel()), qkv):
            if attn_drop > 0.0:      # the dropout instantiations: the mask is regenerated in the kernels from (seed, index), never stored
                _lib.check(L.icl_window_attn_fwd_drop(_ptr(qkv), _ptr(bias_pad), _ptr(regions), _ptr(out), _ptr(lse), b_, n, heads, nw, dh,
                                                      scale, seed, attn_drop, _ptr(seed_dev), _stream(qkv)), "window_attn_fwd_drop")
            else:
                _lib.check(L.icl_window_attn_fwd(_ptr(qkv), _ptr(bias_pad), _ptr(regions), _ptr(out), _ptr(lse), b_, n, heads, nw, dh,
                                                 scale, _stream(qkv)), "window_attn_fwd")
        ctx.save_for_backward(qkv, bias_pad, index, regions, out, lse)
        ctx.cfg = (heads, scale, nw, table.shape[0], dh)
        ctx.drop = (attn_drop, seed)
        ctx.seed_dev = seed_dev
        return out

    @staticmethod
    def backward(ctx, gout):
        qkv, bias_pad, index, regions, out, lse = ctx.saved_tensors
        heads, scale, nw, trows, dh = ctx.cfg
        L = _lib.lib()
        gout = gout.contiguous()
        b_, n, _ = qkv.shape
        dqkv = torch.empty_like(qkv)
        need_table = ctx.needs_input_grad[1]
        chunks = L.icl_window_attn_bwd_chunks(b_, n, heads, nw, dh) if need_table else 0
        # one d(bias) slab per slice of windows (plain stores), summed in a fixed order below: no float atomics
        dbias = torch.empty((chunks,) + tuple(bias_pad.shape), dtype=torch.float32, device=qkv.device) if need_table else None
        flops = 14.0 * b_ * heads * n * n * dh
        attn_drop, seed = ctx.drop
        with _timed("window_attn_bwd_kernel", flops, 4.0 * (2 * qkv.numel() + 2 * out.numel()), qkv):
            if attn_drop > 0.0:
                _lib.check(L.icl_window_attn_bwd_drop(_ptr(qkv), _ptr(bias_pad), _ptr(regions), _ptr(out), _ptr(lse), _ptr(gout), _ptr(dqkv),
                                                      _ptr(dbias), b_, n, heads, nw, dh, scale, seed, attn_drop, _ptr(ctx.seed_dev),
                                                      _stream(qkv)), "window_attn_bwd_drop")
            else:
                _lib.check(L.icl_window_attn_bwd(_ptr(qkv), _ptr(bias_pad), _ptr(regions), _ptr(out), _ptr(lse), _ptr(gout), _ptr(dqkv),
                                                 _ptr(dbias), b_, n, heads, nw, dh, scale, _stream(qkv)), "window_attn_bwd")
        dtable = None
        if need_table:
            dtable = torch.empty((trows, heads), dtype=torch.float32, device=qkv.device)
            inv, offs = _relpos_inverse(index, n, trows)
            _lib.check(L.icl_relpos_bias_bwd_sum(_ptr(dbias), chunks, _ptr(inv), _ptr(offs), _ptr(dtable), trows, n, heads, _stream(qkv)),
                       "relpos_bias_bwd_sum")
        return dqkv, dtable, None, None, None, None, None, None, None


def window_attention(qkv: torch.Tensor, table: torch.Tensor, index: torch.Tensor, regions: Optional[torch.Tensor], heads: int,
                     scale: float, attn_drop: float = 0.0, seed: Optional[int] = None) -> torch.Tensor:
    """WindowAttention.forward core (swinunetr_icl.py:728-747).  qkv [B_, n, 3C] (q|k|v, each head-major); table
    ``relative_position_bias_table`` [T, heads] and index ``relative_position_index`` [343, 343] (the bias of a window with
    n tokens is table[index[:n, :n]] — also for clipped windows, as the reference does); regions int32 [nW, n] or None
    (tokens of one window attend to each other iff their region ids match: the 0/-100 mask).  Returns [B_, n, C].

    ``attn_drop`` > 0 (the caller passes 0 outside training): dropout on the soft-max probabilities (:742-747) inside the fused kernels,
    ``out = (keep * P / (1 - attn_drop)) @ v``.  The mask is the one ``dropout`` would draw on the reference's [B_, heads, n, n] attention
    tensor — ``dropout_keep_mask(seed, B_ * heads * n * n, attn_drop)`` — and is regenerated by the backward kernels; ``seed`` follows the
    protocol of ``dropout`` (None: ``StepRNG`` when enabled for the device, else torch's CPU generator).  ``attn_drop == 0`` draws no
    seed and launches exactly the kernels without dropout."""
    attn_drop = float(attn_drop)
    if attn_drop == 0.0:
        return _WindowAttention.apply(qkv, table, index, regions, heads, float(scale))
    if not 0.0 < attn_drop < 1.0:
        raise ValueError("icl_amd window attention: attn_drop must lie in [0, 1)")
    seed, seed_dev = _step_seed(qkv, seed)
    return _WindowAttention.apply(qkv, table, index, regions, heads, float(scale), attn_drop, seed, seed_dev)


def window_attention_keep_probe(like: torch.Tensor, base: int, count: int, seed: int, p: float, seed_dev: Optional[torch.Tensor] = None):
    """The keep decisions of the attention-dropout kernels for the flat indices base .. base + count - 1 of the attention tensor (bool
    tensor on the device of ``like``), drawn by the kernels' own hoisted form of the hash: the unit check of its 64-bit index handling
    (``base`` may exceed 2^32, which no model's attention tensor does) against ``dropout_keep_mask(..., start=base)``."""
    _require(like)
    out = torch.empty(count, dtype=torch.int32, device=like.device)
    _lib.check(_lib.lib().icl_window_attn_keep_probe(_ptr(out), int(base), int(count), int(seed) & 0xFFFFFFFF, float(p), _ptr(seed_dev),
                                                     _stream(like)), "window_attn_keep_probe")
    return out != 0


PROTO_ATTN_WS_MIN_TOKENS = 1024      # token axes from here on take icl_attn_bwd_ws with its dQ-share workspace (the tests move it)
MAX_CLASSES = 256      # the loss kernels (csrc/kernels/loss.h, kLossMaxNc) and the prototype attention (token.h, kAttnMaxClasses)


def _check_classes(nc: int, what: str) -> None:
    if not 1 <= nc <= MAX_CLASSES:
        raise ValueError(f"icl_amd {what}: {nc} classes; the training kernels take 1 .. {MAX_CLASSES} (ops.MAX_CLASSES)")


class _ProtoAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qh, kv, heads, scale):
        _require(qh, kv)
        L = _lib.lib()
        qh = qh.contiguous()
        kv = kv.contiguous()
        B, h, nc, d = qh.shape
        N = kv.shape[1]
        assert h == heads and kv.shape[2] == 2 * h * d
        _check_classes(nc, "prototype attention")
        logits = torch.empty((B, nc, h, N), dtype=torch.float32, device=qh.device)       # class-major: the layout the reference returns
        out = torch.empty((B, h, nc, d), dtype=torch.float32, device=qh.device)
        stats = torch.empty((B, h, nc, 2), dtype=torch.float32, device=qh.device)
        _lib.check(L.icl_attn_fwd(_ptr(qh), _ptr(kv), _ptr(logits), _ptr(out), _ptr(stats), B, h, nc, N, d, scale, _stream(qh)), "attn_fwd")
        ctx.save_for_backward(qh, kv, logits, stats, out)
        ctx.scale = scale
        return out, logits

    @staticmethod
    def backward(ctx, gout, glog):
        qh, kv, logits, stats, out = ctx.saved_tensors
        L = _lib.lib()
        B, h, nc, d = qh.shape
        N = kv.shape[1]
        gout = gout.contiguous() if gout is not None else None
        glog = glog.contiguous() if glog is not None else None
        gq = torch.empty_like(qh)
        gkv = torch.empty_like(kv)
        # dQ from the shares the dK / dV pass writes per 256-token chunk (long token axes: the row-per-workgroup dQ kernel is a latency
        # chain on the backward's query chain); short axes keep the two-kernel form (one launch fewer than shares + sum... the same count)
        ws = _ws(L.icl_attn_bwd_ws_bytes(B, h, nc, N, d), qh) if N >= PROTO_ATTN_WS_MIN_TOKENS else None
        _lib.check(L.icl_attn_bwd_ws(_ptr(qh), _ptr(kv), _ptr(logits), _ptr(stats), _ptr(out), _ptr(gout), _ptr(glog), _ptr(gq), _ptr(gkv),
                                     _ptr(ws), B, h, nc, N, d, ctx.scale, _stream(qh)), "attn_bwd")
        return gq, gkv, None, None


def prototype_attention(qh: torch.Tensor, kv: torch.Tensor, heads: int, scale: float):
    """qh [B,h,nc,d]; kv [B,N,2*h*d] laid out (k|v, head, d).  Returns (softmax(QK^T*scale) V  [B,h,nc,d],
    scaled pre-softmax logits [B,nc,h,N] — already in the layout of the reference's ``attn1.permute(0, 2, 1, 3)``)."""
    return _ProtoAttention.apply(qh, kv, heads, float(scale))


# --------------------------------------------------------------------------------------
# The aligner's query chain as fused stages (csrc/kernels/qchain.h; networks/unet_3D_icl.py:258-264, 283-297, 299-315, 220-222)
# --------------------------------------------------------------------------------------

class _QcStage(ctypes.Structure):      # include/icl_hip.h IclQcStage
    _fields_ = [("x", _vp), ("x_rows", ctypes.c_int), ("w", _vp), ("bias", _vp), ("y", _vp),
                ("R", ctypes.c_int), ("K", ctypes.c_int), ("N", ctypes.c_int), ("trans", ctypes.c_int), ("nc", ctypes.c_int),
                ("npw", ctypes.c_int), ("pro", ctypes.c_int), ("epi", ctypes.c_int),
                ("pa", _vp), ("pb", _vp), ("pc", _vp), ("pd", _vp), ("pro_dp", ctypes.c_int),
                ("so0", _vp), ("so1", _vp), ("so2", _vp), ("ea", _vp), ("eb", _vp),
                ("ea_r0", ctypes.c_int), ("ea_r1", ctypes.c_int), ("eb_r0", ctypes.c_int), ("eb_r1", ctypes.c_int),
                ("dp_seed", ctypes.c_uint32 * 2), ("dp_thresh", ctypes.c_uint32 * 2), ("dp_scale", ctypes.c_float * 2),
                ("dp_seed_dev", _vp), ("eps", ctypes.c_float)]


QC_PRO_NONE, QC_PRO_LN, QC_PRO_GELU, QC_PRO_LNBWD, QC_PRO_SCALE = range(5)
QC_EPI_NONE, QC_EPI_DP1, QC_EPI_RES_DP, QC_EPI_GELUBWD, QC_EPI_ADDROWS, QC_EPI_SUMB = range(6)
QCHAIN = os.environ.get("ICL_QCHAIN", "1") != "0"
QC_MAX_ROWS, QC_MAX_K, QC_ROWS_PER_PASS = 32, 1024, 8
# Rows up to which the aligner takes the fused chain.  The stages walk the rows in passes of eight, re-reading the workgroup's weight slice per
# pass: with nc = 16 (32 / 16 rows) the fused chain measured SLOWER than the operator-by-operator path whose products run on the MFMA stream
# kernel (15.58 against 15.30 ms per step, profiles/r6_qchain_ab.txt), so it is taken for one pass only (nc = 2: 4 / 2 rows); the kernels and
# their tests cover 32 rows.
QC_FUSE_MAX_ROWS = int(os.environ.get("ICL_QCHAIN_MAX_ROWS", str(QC_ROWS_PER_PASS)))


def _qc_stage(like, dp, *, y, R, K, N=0, trans=0, nc=1, x=None, x_rows=0, w=None, bias=None, pro=QC_PRO_NONE, epi=QC_EPI_NONE, pa=None,
              pb=None, pc=None, pd=None, pro_dp=0, so0=None, so1=None, so2=None, ea=None, eb=None, ea_rows=(0, 0), eb_rows=(0, 0), eps=1e-5):
    """One launch of icl_qchain_stage.  ``dp``: ((seed, thresh, scale) of site 0, of site 1, seed_dev tensor or None)."""
    st = _QcStage()
    st.x, st.x_rows, st.w, st.bias, st.y = _ptr(x), x_rows, _ptr(w), _ptr(bias), _ptr(y)
    st.R, st.K, st.N, st.trans, st.nc, st.npw = R, K, N, trans, nc, 0
    st.pro, st.epi, st.pro_dp = pro, epi, pro_dp
    st.pa, st.pb, st.pc, st.pd = _ptr(pa), _ptr(pb), _ptr(pc), _ptr(pd)
    st.so0, st.so1, st.so2 = _ptr(so0), _ptr(so1), _ptr(so2)
    st.ea, st.eb = _ptr(ea), _ptr(eb)
    st.ea_r0, st.ea_r1 = ea_rows
    st.eb_r0, st.eb_r1 = eb_rows
    for i in (0, 1):
        st.dp_seed[i], st.dp_thresh[i], st.dp_scale[i] = dp[i]
    st.dp_seed_dev = _ptr(dp[2])
    st.eps = eps
    _lib.check(_lib.lib().icl_qchain_stage(ctypes.byref(st), _stream(like)), "qchain_stage")


def _qc_wgrad(like, jobs):
    """jobs: (g, x, dw, db or None, rows, n, k, kind)."""
    n = len(jobs)
    arr, iarr = _vp * n, ctypes.c_int32 * n
    _lib.check(_lib.lib().icl_qchain_wgrad(arr(*[j[0].data_ptr() for j in jobs]), arr(*[j[1].data_ptr() for j in jobs]),
                                          arr(*[j[2].data_ptr() for j in jobs]), arr(*[(j[3].data_ptr() if j[3] is not None else None) for j in jobs]),
                                          iarr(*[j[4] for j in jobs]), iarr(*[j[5] for j in jobs]), iarr(*[j[6] for j in jobs]),
                                          iarr(*[j[7] for j in jobs]), n, _stream(like)), "qchain_wgrad")


def query_chain_ok(rows: int, c: int, hidden: int, nc: int, like: torch.Tensor) -> bool:
    return (QCHAIN and rows <= min(QC_MAX_ROWS, QC_FUSE_MAX_ROWS) and c % 8 == 0 and hidden % 4 == 0 and max(c, hidden) <= QC_MAX_K and nc <= 16
            and (like.is_cuda or _lib.host_pointers_ok()))


class _QueryAttend(torch.autograd.Function):
    """One resolution level of the aligner's query half as fused stages: LayerNorm(norm1_query) -> fc_q -> [read-out of softmax(q k^T) v]
    -> proj -> q + drop_path(q) -> LayerNorm(norm2) -> fc1 -> GELU -> fc2 -> q + drop_path(.) -> query_convs.
    Inputs: q_in [B or 1, nc, C] (a [1, nc, C] query is broadcast over the batch inside the first stage), kv [B, N, 2C] (fc_kv of the
    normalised tokens), cfg, the fourteen parameters.  Outputs: logits [B, nc, h, N], and with cfg['full'] the query after the block as
    its two batch halves q2[:ba], q2[ba:] (views of one buffer) and the query handed down a level [B, nc, C/2].  ``full`` False (the
    guided call of the 3-D models, whose updated queries nobody reads): fc_q and the logits only."""

    @staticmethod
    def forward(ctx, q_in, kv, cfg, n1w, n1b, fqw, fqb, pw, pb, n2w, n2b, f1w, f1b, f2w, f2b, qcw, qcb):
        L = _lib.lib()
        h, scale, ba, eps, dp, full = cfg["heads"], cfg["scale"], cfg["ba"], cfg["eps"], cfg["dp"], cfg["full"]
        q_in, kv = q_in.contiguous(), kv.contiguous()
        _require(q_in, kv, fqw)
        nc, C = q_in.shape[1], q_in.shape[2]
        B, N = kv.shape[0], kv.shape[1]
        R, d = B * nc, C // h
        dev = kv.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        xhat1, rstd1, n1, qf = new(R, C), new(R), new(R, C), new(R, C)
        _qc_stage(kv, dp, y=qf, R=R, K=C, N=C, nc=nc, x=q_in, x_rows=q_in.shape[0] * nc, w=fqw, bias=fqb, pro=QC_PRO_LN, pa=n1w, pb=n1b,
                  so0=xhat1, so1=rstd1, so2=n1, eps=eps)
        logits, a, stats = new(B, nc, h, N), new(R, C), new(B, h, nc, 2)
        # qf read as [B, h, nc, d] and the read-out written back as [B, nc, C]: the reference's reshape quirk (:287, :293) is a
        # reinterpretation of the same contiguous bytes
        _lib.check(L.icl_attn_fwd(_ptr(qf), _ptr(kv), _ptr(logits), _ptr(a), _ptr(stats), B, h, nc, N, d, scale, _stream(kv)), "attn_fwd")
        ctx.cfg, ctx.shape = cfg, (B, nc, C, N, tuple(q_in.shape))
        ctx.set_materialize_grads(False)      # an output nobody differentiates (the last level's hand-down, a discarded batch half) arrives as None
        if not full:
            ctx.save_for_backward(kv, logits, stats, a, qf, xhat1, rstd1, n1, n1w, fqw)
            return (logits,)
        H = f1w.shape[0]
        q1, xhat2, rstd2, n2, u, hh, q2, nxt = new(R, C), new(R, C), new(R), new(R, C), new(R, H), new(R, H), new(B, nc, C), new(B, nc, qcw.shape[0])
        _qc_stage(kv, dp, y=q1, R=R, K=C, N=C, nc=nc, x=a, w=pw, bias=pb, epi=QC_EPI_DP1)
        _qc_stage(kv, dp, y=u, R=R, K=C, N=H, nc=nc, x=q1, w=f1w, bias=f1b, pro=QC_PRO_LN, pa=n2w, pb=n2b, so0=xhat2, so1=rstd2, so2=n2, eps=eps)
        _qc_stage(kv, dp, y=q2, R=R, K=H, N=C, nc=nc, x=u, w=f2w, bias=f2b, pro=QC_PRO_GELU, so2=hh, epi=QC_EPI_RES_DP, ea=q1)
        _qc_stage(kv, dp, y=nxt, R=R, K=C, N=qcw.shape[0], nc=nc, x=q2, w=qcw, bias=qcb)
        ctx.save_for_backward(kv, logits, stats, a, qf, xhat1, rstd1, n1, n1w, fqw, q1, xhat2, rstd2, n2, u, hh, q2, n2w, pw, f1w, f2w, qcw)
        return logits, q2[:ba], q2[ba:], nxt

    @staticmethod
    def backward(ctx, glog, gq2a=None, gq2b=None, gnxt=None):
        L = _lib.lib()
        cfg = ctx.cfg
        h, scale, ba, dp, full = cfg["heads"], cfg["scale"], cfg["ba"], cfg["dp"], cfg["full"]
        B, nc, C, N, q_shape = ctx.shape
        R, d = B * nc, C // h
        sv = ctx.saved_tensors
        kv, logits, stats, a, qf, xhat1, rstd1, n1, n1w, fqw = sv[:10]
        dev = kv.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        jobs = []
        ga = None
        grads = [None] * 14
        if full and (gq2a is not None or gq2b is not None or gnxt is not None):
            q1, xhat2, rstd2, n2, u, hh, q2, n2w, pw, f1w, f2w, qcw = sv[10:]
            H = f1w.shape[0]
            gq2a = gq2a.contiguous() if gq2a is not None else None
            gq2b = gq2b.contiguous() if gq2b is not None else None
            dq2, g2, du, dn2, do, ga = new(R, C), new(R, C), new(R, H), new(R, C), new(R, C), new(R, C)
            add = dict(epi=QC_EPI_ADDROWS, ea=gq2a, ea_rows=(0, ba * nc), eb=gq2b, eb_rows=(ba * nc, R))
            if gnxt is not None:
                gnxt = gnxt.contiguous()
                _qc_stage(kv, dp, y=dq2, R=R, K=qcw.shape[0], N=C, trans=1, nc=nc, x=gnxt, w=qcw, **add)
            else:
                _qc_stage(kv, dp, y=dq2, R=R, K=C, trans=2, nc=nc, **add)
            # g2 = f1 * dq2 is fc2's output gradient; du = (g2 W2) * gelu'(u)
            _qc_stage(kv, dp, y=du, R=R, K=C, N=H, trans=1, nc=nc, x=dq2, w=f2w, pro=QC_PRO_SCALE, so2=g2, epi=QC_EPI_GELUBWD, ea=u)
            _qc_stage(kv, dp, y=dn2, R=R, K=H, N=C, trans=1, nc=nc, x=du, w=f1w)
            # do = (dq2 + LayerNorm'(dn2)) * (1 + f0) is proj's output gradient; ga = do Wp the read-out's
            _qc_stage(kv, dp, y=ga, R=R, K=C, N=C, trans=1, nc=nc, x=dn2, w=pw, pro=QC_PRO_LNBWD, pa=xhat2, pb=rstd2, pc=n2w, pd=dq2, pro_dp=1, so2=do)
            gpw, gpb, gn2w, gn2b, gf1w, gf1b, gf2w, gf2b = new(C, C), new(C), new(C), new(C), new(H, C), new(H), new(C, H), new(C)
            jobs += [(do, a, gpw, gpb, R, C, C, 0), (dn2, xhat2, gn2w, gn2b, R, C, C, 1), (du, n2, gf1w, gf1b, R, H, C, 0),
                     (g2, hh, gf2w, gf2b, R, C, H, 0)]
            grads[4:12] = [gpw, gpb, gn2w, gn2b, gf1w, gf1b, gf2w, gf2b]
            if gnxt is not None:
                gqcw, gqcb = new(qcw.shape[0], C), new(qcw.shape[0])
                jobs.append((gnxt, q2.view(R, C), gqcw, gqcb, R, qcw.shape[0], C, 0))
                grads[12:14] = [gqcw, gqcb]
        glog = glog.contiguous() if glog is not None else None
        gq, gkv = new(R, C), torch.empty_like(kv)
        ws = _ws(L.icl_attn_bwd_ws_bytes(B, h, nc, N, d), kv) if N >= PROTO_ATTN_WS_MIN_TOKENS else None
        _lib.check(L.icl_attn_bwd_ws(_ptr(qf), _ptr(kv), _ptr(logits), _ptr(stats), _ptr(a), _ptr(ga), _ptr(glog), _ptr(gq), _ptr(gkv),
                                     _ptr(ws), B, h, nc, N, d, scale, _stream(kv)), "attn_bwd")
        dn1 = new(R, C)
        _qc_stage(kv, dp, y=dn1, R=R, K=C, N=C, trans=1, nc=nc, x=gq, w=fqw)
        bcast = q_shape[0] == 1 and B > 1
        if bcast and R <= QC_ROWS_PER_PASS:
            gqin = new(1, nc, C)
            _qc_stage(kv, dp, y=gqin, R=R, K=C, trans=2, nc=nc, x=dn1, pro=QC_PRO_LNBWD, pa=xhat1, pb=rstd1, pc=n1w, epi=QC_EPI_SUMB)
        else:
            gqin = new(B, nc, C)
            _qc_stage(kv, dp, y=gqin, R=R, K=C, trans=2, nc=nc, x=dn1, pro=QC_PRO_LNBWD, pa=xhat1, pb=rstd1, pc=n1w)
            if bcast:
                gqin = gqin.sum(0, keepdim=True)
        gn1w, gn1b, gfqw, gfqb = new(C), new(C), new(C, C), new(C)
        jobs += [(dn1, xhat1, gn1w, gn1b, R, C, C, 1), (gq, n1, gfqw, gfqb, R, C, C, 0)]
        grads[0:4] = [gn1w, gn1b, gfqw, gfqb]
        _qc_wgrad(kv, jobs)
        return (gqin, gkv, None, *grads)


def query_attend(q_in, kv, heads, scale, ba, eps, dp, full, params):
    """See _QueryAttend.  ``params``: the fourteen parameter tensors in the Function's order."""
    cfg = dict(heads=int(heads), scale=float(scale), ba=int(ba), eps=float(eps), dp=dp, full=bool(full))
    return _QueryAttend.apply(q_in, kv, cfg, *params)


def drop_path_site(like, p: float, training: bool):
    """(seed, thresh, scale, seed_dev) of one drop-path site for the fused stages: the per-sample decision of ``drop_path`` (same hash, same
    seeding); an inactive site keeps everything at scale 1."""
    if p == 0.0 or not training:
        return (0, 0, 1.0), None
    seed, seed_dev = _step_seed(like, None)
    return (seed, int(p * 4294967296.0) & 0xFFFFFFFF, 1.0 / (1.0 - p)), seed_dev


# --------------------------------------------------------------------------------------
# Loss reductions (utils/losses.py L1-L5): one fused HIP pass per loss term, one more for its gradient
# --------------------------------------------------------------------------------------

LOSS_MAX_BLOCKS = 1024   # ICL_LOSS_MAX_BLOCKS (include/icl_hip.h)


class _FusedLoss(torch.autograd.Function):
    """(term0, term1) per icl_loss_fwd's mode table (include/icl_hip.h)."""

    @staticmethod
    def forward(ctx, a, target, weight, mode, a_is_prob):
        _require(a, target, weight)
        L = _lib.lib()
        a = a.contiguous()
        target = target.contiguous()
        B, nc = a.shape[0], a.shape[1]
        _check_classes(nc, "loss")
        S = a.numel() // (B * nc)
        hard = mode <= 1
        if hard:
            assert target.dtype == torch.int64 and target.numel() == B * S, "labels must be int64 [B, ...]"
        else:
            assert target.shape == a.shape and target.dtype == torch.float32
        stats = torch.empty((3 * nc + 1) * (1 + LOSS_MAX_BLOCKS), dtype=torch.float32, device=a.device)   # ICL_LOSS_STATS_FLOATS
        out = torch.empty(2, dtype=torch.float32, device=a.device)
        _lib.check(L.icl_loss_fwd(_ptr(a), None if hard else _ptr(target), _ptr(target) if hard else None, _ptr(weight),
                                  _ptr(stats), _ptr(out), B, nc, S, mode, int(a_is_prob), _stream(a)), "loss_fwd")
        ctx.save_for_backward(a, target, stats, weight)
        ctx.cfg = (mode, int(a_is_prob))
        ctx.set_materialize_grads(False)
        return out[0], out[1]      # two scalars: an unused one costs nothing in backward (no select_backward / zero fill)

    @staticmethod
    def backward(ctx, g0, g1):
        a, target, stats, weight = ctx.saved_tensors
        mode, aip = ctx.cfg
        L = _lib.lib()
        B, nc = a.shape[0], a.shape[1]
        S = a.numel() // (B * nc)
        hard = mode <= 1
        g0 = g0.contiguous() if g0 is not None else None
        g1 = g1.contiguous() if g1 is not None else None
        ga = torch.empty_like(a)
        _lib.check(L.icl_loss_bwd(_ptr(a), None if hard else _ptr(target), _ptr(target) if hard else None, _ptr(weight),
                                  _ptr(stats), _ptr(g0), _ptr(g1), _ptr(ga), B, nc, S, mode, aip, _stream(a)), "loss_bwd")
        return ga, None, None, None, None


class _LossJob(ctypes.Structure):      # include/icl_hip.h IclLossJob
    _fields_ = [("a", _vp), ("b", _vp), ("labels", _vp), ("weight", _vp), ("stats", _vp), ("out", _vp), ("gout0", _vp), ("gout1", _vp),
                ("ga", _vp), ("s", ctypes.c_int64), ("batch", ctypes.c_int), ("nc", ctypes.c_int), ("mode", ctypes.c_int),
                ("a_is_prob", ctypes.c_int)]


LOSS_MULTI_MAX = 12
LOSS_MULTI = os.environ.get("ICL_LOSS_MULTI", "1") != "0"


class _FusedLossMulti(torch.autograd.Function):
    """Several `_FusedLoss` terms — (a_j, target_j, mode_j) — in ONE statistics launch, one finalize launch and one gradient launch
    (icl_loss_fwd_multi / icl_loss_bwd_multi).  ``modes``: tuple of icl_loss_fwd modes; tensors: a_0, t_0, a_1, t_1, ...; returns
    (term0_0, term1_0, term0_1, term1_1, ...), each the 0-dim tensor `_FusedLoss` would have returned (bit-identical)."""

    @staticmethod
    def forward(ctx, modes, *tensors):
        L = _lib.lib()
        n = len(modes)
        assert 1 <= n <= LOSS_MULTI_MAX and len(tensors) == 2 * n
        a_s = [tensors[2 * j].contiguous() for j in range(n)]
        t_s = [tensors[2 * j + 1].contiguous() for j in range(n)]
        _require(*a_s, *t_s)
        dev = a_s[0].device
        nc = a_s[0].shape[1]
        _check_classes(nc, "loss")
        per = (3 * nc + 1) * (1 + LOSS_MAX_BLOCKS)
        stats = torch.empty((n, per), dtype=torch.float32, device=dev)
        out = torch.empty((n, 2), dtype=torch.float32, device=dev)
        jobs = (_LossJob * n)()
        for j in range(n):
            a, t, mode = a_s[j], t_s[j], modes[j]
            B = a.shape[0]
            S = a.numel() // (B * nc)
            hard = mode <= 1
            assert a.shape[1] == nc
            if hard:
                assert t.dtype == torch.int64 and t.numel() == B * S, "labels must be int64 [B, ...]"
            else:
                assert t.shape == a.shape and t.dtype == torch.float32
            q = jobs[j]
            q.a, q.b, q.labels, q.weight = a.data_ptr(), (None if hard else t.data_ptr()), (t.data_ptr() if hard else None), None
            q.stats, q.out = stats[j].data_ptr(), out[j].data_ptr()
            q.s, q.batch, q.nc, q.mode, q.a_is_prob = S, B, nc, mode, 0
        _lib.check(L.icl_loss_fwd_multi(jobs, n, _stream(a_s[0])), "loss_fwd_multi")
        ctx.save_for_backward(stats, *a_s, *t_s)
        ctx.modes = tuple(modes)
        ctx.set_materialize_grads(False)
        return tuple(out[j, k] for j in range(n) for k in (0, 1))

    @staticmethod
    def backward(ctx, *gs):
        L = _lib.lib()
        modes = ctx.modes
        n = len(modes)
        stats = ctx.saved_tensors[0]
        a_s, t_s = ctx.saved_tensors[1:1 + n], ctx.saved_tensors[1 + n:1 + 2 * n]
        nc = a_s[0].shape[1]
        gas = [None] * n
        keep = []
        live = [j for j in range(n) if ctx.needs_input_grad[1 + 2 * j] and (gs[2 * j] is not None or gs[2 * j + 1] is not None)]
        jobs = (_LossJob * max(len(live), 1))()
        for i, j in enumerate(live):
            a, t, mode = a_s[j], t_s[j], modes[j]
            B = a.shape[0]
            S = a.numel() // (B * nc)
            hard = mode <= 1
            g0 = gs[2 * j].contiguous() if gs[2 * j] is not None else None
            g1 = gs[2 * j + 1].contiguous() if gs[2 * j + 1] is not None else None
            keep += [g0, g1]
            gas[j] = torch.empty_like(a)
            q = jobs[i]
            q.a, q.b, q.labels, q.weight = a.data_ptr(), (None if hard else t.data_ptr()), (t.data_ptr() if hard else None), None
            q.stats, q.out = stats[j].data_ptr(), None
            q.gout0, q.gout1, q.ga = _ptr(g0), _ptr(g1), gas[j].data_ptr()
            q.s, q.batch, q.nc, q.mode, q.a_is_prob = S, B, nc, mode, 0
        if live:
            _lib.check(L.icl_loss_bwd_multi(jobs, len(live), _stream(a_s[0])), "loss_bwd_multi")
        res = [None]
        for j in range(n):
            res += [gas[j], None]
        return tuple(res)


def fused_losses(terms):
    """``terms``: list of (a, target, mode) with mode 1 = (cross-entropy, Dice(softmax)) on int64 labels, 2 = soft Dice against logits,
    3 = softmax MSE against logits (the targets of modes 2 / 3 are detached).  Returns the list of (term0, term1) pairs — one statistics
    launch, one finalize launch, one gradient launch for all of them when there are at most 12 with one class count (one class count is
    one class group of icl_loss_fwd_multi: <= 4, 5 .. 16 or 17 .. 256 classes)."""
    if not terms:
        return []
    ncs = {t[0].shape[1] for t in terms}
    if not LOSS_MULTI or len(terms) > LOSS_MULTI_MAX or len(ncs) != 1:
        return [_FusedLoss.apply(a, (t.long() if m <= 1 else t.detach()), None, m, False) for a, t, m in terms]
    flat = []
    for a, t, m in terms:
        flat += [a, (t.long() if m <= 1 else t.detach())]
    out = _FusedLossMulti.apply(tuple(m for _, _, m in terms), *flat)
    return [(out[2 * j], out[2 * j + 1]) for j in range(len(terms))]


class _CombineScalars(torch.autograd.Function):
    """out[j] = sum_i W[j][i] * terms[i] for 0-dim fp32 tensors ``terms``: one launch (icl_scalar_combine); backward one launch with
    W^T.  The scalar arithmetic between loss terms (trainer :105-112, losses.py "(a + b + c) / 3") as torch ops is a chain of
    one-element kernels, forward and backward."""

    @staticmethod
    def forward(ctx, W, *terms):
        n, m = len(terms), len(W)
        ts = [t if (t.dtype == torch.float32 and t.dim() == 0) else t.float().reshape(()) for t in terms]
        _require(*ts)
        out = torch.empty(m, dtype=torch.float32, device=ts[0].device)
        arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        flat = (ctypes.c_float * (m * n))(*[float(W[j][i]) for j in range(m) for i in range(n)])
        _lib.check(_lib.lib().icl_scalar_combine(arr, flat, n, m, _ptr(out), _stream(out)), "scalar_combine")
        ctx.W = W
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, gout):
        W, n = ctx.W, ctx.n
        m = len(W)
        gout = gout.contiguous()
        gin = torch.empty(n, dtype=torch.float32, device=gout.device)
        arr = (ctypes.c_void_p * m)(*[gout.data_ptr() + 4 * j for j in range(m)])
        flat = (ctypes.c_float * (n * m))(*[float(W[j][i]) for i in range(n) for j in range(m)])       # W^T, [n][m]
        _lib.check(_lib.lib().icl_scalar_combine(arr, flat, m, n, _ptr(gin), _stream(gin)), "scalar_combine_bwd")
        return (None,) + tuple(gin[i] for i in range(n))


def combine_scalars(terms, W) -> torch.Tensor:
    """[sum_i W[j][i] * terms[i] for j] as one fp32 vector; ``terms``: 0-dim tensors on one device, ``W``: nested Python floats
    (at most 16 x 16)."""
    return _CombineScalars.apply(tuple(tuple(float(v) for v in row) for row in W), *terms)


def _weight_tensor(weight, like):
    if weight is None:
        return None
    return torch.as_tensor(weight, dtype=torch.float32, device=like.device)


def dice_loss(inputs: torch.Tensor, labels: torch.Tensor, n_classes: int, softmax: bool = False, weight=None):
    """DiceLoss.forward (losses.py:218-231); labels [B, ...] integer class ids."""
    assert inputs.shape[1] == n_classes
    return _FusedLoss.apply(inputs, labels.long(), _weight_tensor(weight, inputs), 0, not softmax)[1]


def cross_entropy_dice_parts(logits: torch.Tensor, labels: torch.Tensor, n_classes: int):
    """(CrossEntropyLoss()(logits, labels), DiceLoss(softmax=True)(logits, labels)) from ONE pass over the logits."""
    assert logits.shape[1] == n_classes
    return _FusedLoss.apply(logits, labels.long(), None, 1, False)


def cross_entropy_dice(logits: torch.Tensor, labels: torch.Tensor, n_classes: int):
    """CE + Dice(softmax=True) — one AuxLoss3D term (losses.py:268-269)."""
    ce, dc = cross_entropy_dice_parts(logits, labels, n_classes)
    return ce + dc


def soft_dice_loss(a: torch.Tensor, b: torch.Tensor):
    """softmax_dice_loss (losses.py:42-59): per class 1-(2*sum(sa*sb)+eps)/(sum(sa)+sum(sb)+eps), mean over classes.
    Gradient flows to ``a`` only (the reference detaches the target, losses.py:294)."""
    return _FusedLoss.apply(a, b.detach(), None, 2, False)[1]


def softmax_mse(a: torch.Tensor, b: torch.Tensor):
    """mean((softmax(a,1) - softmax(b,1))^2) — one scale of softmax_mse_loss (losses.py:82-87); target detached."""
    return _FusedLoss.apply(a, b.detach(), None, 3, False)[0]


# --------------------------------------------------------------------------------------
# Voxel-wise losses (utils/losses.py: softmax_kl_loss :93-112, compute_kl_loss :334-346, the entropy functions :33-39, :62-65, :321-331,
# FocalLoss :149-183): csrc/kernels/loss_point.h — one pass and a one-block finalize forward, one pass backward, nothing kept between them
# --------------------------------------------------------------------------------------

def _class_axis(t: torch.Tensor, dim: int, what: str):
    """(outer, nc, inner) of a contiguous tensor whose class axis is ``dim``."""
    if t.dim() < 2:
        raise ValueError(f"icl_amd {what}: needs a class axis, got shape {tuple(t.shape)}")
    dim = dim % t.dim()
    nc = t.shape[dim]
    _check_classes(nc, what)
    outer = math.prod(t.shape[:dim])
    inner = math.prod(t.shape[dim + 1:])
    if outer * inner < 1:
        raise ValueError(f"icl_amd {what}: empty tensor {tuple(t.shape)}")
    return outer, nc, inner


def _point_ws(like: torch.Tensor) -> torch.Tensor:
    return torch.empty(LOSS_MAX_BLOCKS, dtype=torch.float32, device=like.device)      # ICL_POINT_LOSS_WS_FLOATS


class _SoftmaxKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, w_fwd, w_rev, dim):
        _require(a, b)
        assert a.shape == b.shape and a.dtype == torch.float32 and b.dtype == torch.float32, "softmax_kl: two fp32 tensors of one shape"
        a, b = a.contiguous(), b.contiguous()
        geo = _class_axis(a, dim, "softmax_kl")
        out, ws = torch.empty(1, dtype=torch.float32, device=a.device), _point_ws(a)
        _lib.check(_lib.lib().icl_kl_fwd(_ptr(a), _ptr(b), _ptr(ws), _ptr(out), *geo, w_fwd, w_rev, _stream(a)), "kl_fwd")
        ctx.save_for_backward(a, b)
        ctx.cfg = (geo, w_fwd, w_rev)
        ctx.set_materialize_grads(False)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None
        a, b = ctx.saved_tensors
        geo, w_fwd, w_rev = ctx.cfg
        g = g.contiguous()
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        gb = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.lib().icl_kl_bwd(_ptr(a), _ptr(b), _ptr(g), _ptr(ga), _ptr(gb), *geo, w_fwd, w_rev, _stream(a)), "kl_bwd")
        return ga, gb, None, None, None


def softmax_kl(a: torch.Tensor, b: torch.Tensor, w_fwd: float = 1.0, w_rev: float = 0.0, dim: int = 1) -> torch.Tensor:
    """w_fwd * mean KL(q || p) + w_rev * mean KL(p || q) with p = softmax(a, dim), q = softmax(b, dim); the mean is over ALL elements, as
    F.kl_div(log_softmax(a), softmax(b), reduction='mean') takes it (losses.py:106-110).  The gradient reaches ``b`` when, and only
    when, it requires one: the reference's softmax_kl_loss does not detach its target."""
    return _SoftmaxKL.apply(a, b, float(w_fwd), float(w_rev), int(dim))


class _Entropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, from_logits, scale, want_mean, want_map):
        _require(x)
        assert x.dtype == torch.float32, "entropy: fp32 input"
        x = x.contiguous()
        geo = _class_axis(x, 1, "entropy")
        mean = torch.empty(1, dtype=torch.float32, device=x.device) if want_mean else None
        emap = torch.empty((x.shape[0], 1) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device) if want_map else None
        ws = _point_ws(x) if want_mean else None
        _lib.check(_lib.lib().icl_entropy_fwd(_ptr(x), _ptr(ws), _ptr(mean), _ptr(emap), *geo,
                                              int(from_logits), scale, _stream(x)), "entropy_fwd")
        ctx.save_for_backward(x)
        ctx.cfg = (geo, int(from_logits), scale)
        ctx.set_materialize_grads(False)
        return (mean[0] if want_mean else None), emap

    @staticmethod
    def backward(ctx, gmean, gmap):
        if gmean is None and gmap is None:
            return None, None, None, None, None
        x, = ctx.saved_tensors
        geo, from_logits, scale = ctx.cfg
        gmean = gmean.contiguous() if gmean is not None else None
        gmap = gmap.contiguous() if gmap is not None else None
        gx = torch.empty_like(x)
        _lib.check(_lib.lib().icl_entropy_bwd(_ptr(x), _ptr(gmean), _ptr(gmap), _ptr(gx), *geo, from_logits, scale, _stream(x)),
                   "entropy_bwd")
        return gx, None, None, None, None


def entropy(p: torch.Tensor, from_logits: bool = False, scale: float = 1.0, want: str = "mean"):
    """H_v = -sum_c p_c log(p_c + 1e-6) over dim 1 of [B, nc, ...] probabilities (``from_logits``: of softmax(p, 1), fused), times
    ``scale`` (1, or 1 / log C for entropy_loss): want = "mean" the mean over the voxels (0-dim), "map" the [B, 1, ...] map, "both" the
    pair from one pass."""
    if want not in ("mean", "map", "both"):
        raise ValueError(f"icl_amd entropy: want = 'mean', 'map' or 'both', not {want!r}")
    mean, emap = _Entropy.apply(p, bool(from_logits), float(scale), want != "map", want != "mean")
    return mean if want == "mean" else (emap if want == "map" else (mean, emap))


class _Focal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, alpha, gamma, mean, dim):
        _require(logits, labels, alpha)
        assert logits.dtype == torch.float32, "focal_loss: fp32 logits"
        logits, labels = logits.contiguous(), labels.contiguous()
        geo = _class_axis(logits, dim, "focal_loss")
        assert labels.dtype == torch.int64 and labels.numel() == geo[0] * geo[2], "focal_loss: int64 labels, one per voxel"
        out, ws = torch.empty(1, dtype=torch.float32, device=logits.device), _point_ws(logits)
        _lib.check(_lib.lib().icl_focal_fwd(_ptr(logits), _ptr(labels), _ptr(alpha), _ptr(ws), _ptr(out), *geo, gamma,
                                            int(mean), _stream(logits)), "focal_fwd")
        ctx.save_for_backward(logits, labels, alpha)
        ctx.cfg = (geo, gamma, int(mean))
        ctx.set_materialize_grads(False)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None, None
        logits, labels, alpha = ctx.saved_tensors
        geo, gamma, mean = ctx.cfg
        g = g.contiguous()
        ga = torch.empty_like(logits)
        _lib.check(_lib.lib().icl_focal_bwd(_ptr(logits), _ptr(labels), _ptr(alpha), _ptr(g), _ptr(ga), *geo, gamma, mean,
                                            _stream(logits)), "focal_bwd")
        return ga, None, None, None, None, None


def focal_loss(logits: torch.Tensor, labels: torch.Tensor, gamma: float = 2.0, alpha: Optional[torch.Tensor] = None,
               size_average: bool = True) -> torch.Tensor:
    """FocalLoss.forward (losses.py:160-183): -alpha_y (1 - pt)^gamma log pt per voxel, pt = softmax(logits, 1)_y, mean or sum over the
    voxels.  ``logits`` [N, C, ...] or [M, C], ``labels`` int64 with one entry per voxel, ``alpha`` None or a float tensor of at least C
    entries on the logits' device.  (1 - pt)^gamma is a constant of the backward pass, as in the reference (pt from ``.data``).
    A label outside [0, C) indexes nothing — its voxel adds 0 to the value and to the gradient and still counts in the mean — where the
    reference's gather raises on the CPU."""
    if gamma < 0:
        raise ValueError(f"icl_amd focal_loss: gamma >= 0, not {gamma}")
    if alpha is not None:
        if alpha.numel() < logits.shape[1]:
            raise ValueError(f"icl_amd focal_loss: alpha has {alpha.numel()} entries for {logits.shape[1]} classes")
        alpha = alpha.detach().to(device=logits.device, dtype=torch.float32).contiguous()
    return _Focal.apply(logits, labels, alpha, float(gamma), bool(size_average), 1)


# --------------------------------------------------------------------------------------
# Validation metrics — cal_metric / calculate_metric_percase of every foreground class (val_3D.py:85-97, val_2D.py:10-22)
# --------------------------------------------------------------------------------------

_SEG_DTYPES = {torch.uint8: 1, torch.bool: 1, torch.int64: 8}


def seg_metrics_shape(t: torch.Tensor):
    """(n0, n1, n2, all_border) for a label map the metric kernels take: 3-D, or 3-D after leading axes of length 1 (the AMOS path scores
    [1, D, H, W] arrays: under the N-D connectivity-1 erosion such an axis makes every voxel of a class a surface voxel).  None otherwise."""
    shape = tuple(t.shape)
    if len(shape) < 3 or any(s != 1 for s in shape[:-3]):
        return None
    return shape[-3], shape[-2], shape[-1], int(len(shape) > 3)


def _seg_label_maps(who, *maps, exactly_3d=False):
    """What every ``seg_*`` entry does with its label maps (one, or pred and gt) first: the checks of shape, dtype and device, then
    (contiguous maps, (n0, n1, n2, all_border)).  ``who`` starts every message.  The entry's own argument checks follow, then
    ``_seg_workspace``."""
    first = maps[0]
    if len(maps) == 2 and first.shape != maps[1].shape:
        raise ValueError(f"{who}: shapes differ {tuple(first.shape)} vs {tuple(maps[1].shape)}")
    geo = seg_metrics_shape(first)
    if exactly_3d and first.dim() != 3:
        raise ValueError(f"{who}: needs a 3-D label map, got {tuple(first.shape)}")
    if geo is None:
        raise ValueError(f"{who}: needs a 3-D label map (leading axes of length 1 allowed), got {tuple(first.shape)}")
    for t in maps:
        if t.dtype not in _SEG_DTYPES:
            raise TypeError(f"{who}: unsupported label dtype {t.dtype}")
        if not t.is_cuda and not _lib.host_pointers_ok():
            raise RuntimeError("icl_amd: HIP kernels need device tensors (no CPU fallback)")
    if len(maps) == 2 and first.device != maps[1].device:
        raise ValueError(f"{who}: pred and gt on different devices")
    return [t.contiguous() for t in maps], geo


def _seg_workspace(who, ws_bytes, geo, num_classes, device):
    """The workspace of one ``seg_*`` call, sized by the entry's ``*_ws_bytes``, which also judges the shape and the class count."""
    nbytes = ws_bytes(*geo[:3], int(num_classes))
    if nbytes < 0:
        raise ValueError(f"{who}: shape {geo[:3]} / num_classes {num_classes} not supported (2 <= num_classes <= 256)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def seg_metrics(pred: torch.Tensor, gt: torch.Tensor, num_classes: int) -> torch.Tensor:
    """Per-class integer records of Dice and HD95 (include/icl_hip.h icl_seg_metrics): int64 [num_classes - 1, 6] on the device of the
    maps, row c - 1 = (|P|, |G|, |P & G|, n, s0, s1) for P = pred == c, G = gt == c; n = number of surface voxels of both, s0 / s1 the
    squared surface distances at ranks floor(0.95 (n - 1)) and the next one (-1 when P or G is empty).  Asynchronous on the current
    stream; the maps stay where they are.  Label dtypes: uint8 / bool (h5 labels) and int64 (argmax); pred and gt may differ."""
    L = _lib.lib()
    (pred, gt), geo = _seg_label_maps("seg_metrics", pred, gt)
    ws = _seg_workspace("seg_metrics", L.icl_seg_metrics_ws_bytes, geo, num_classes, pred.device)
    out = torch.empty((int(num_classes) - 1, 6), dtype=torch.int64, device=pred.device)
    _lib.check(L.icl_seg_metrics(_ptr(pred), _SEG_DTYPES[pred.dtype], _ptr(gt), _SEG_DTYPES[gt.dtype], *geo[:3], int(num_classes), geo[3],
                                 _ptr(out), _ptr(ws), _stream(pred)), "seg_metrics")
    return out


def seg_surface_metrics(pred: torch.Tensor, gt: torch.Tensor, num_classes: int, spacing, tolerance: float = 1.0):
    """Per-class records of the surface metrics with a voxel spacing (include/icl_hip.h icl_seg_surface_metrics): ``(counts, values)`` on
    the device of the maps.  ``counts`` int64 [num_classes - 1, 7], row c - 1 = (|P|, |G|, |P & G|, |dP|, |dG|, voxels of dP within
    ``tolerance`` of dG, voxels of dG within ``tolerance`` of dP); ``values`` float64 [num_classes - 1, 6] = (sq[k0], sq[k0 + 1] of the union
    of both directions' squared distances, max d^2 P -> G, max d^2 G -> P, sum d P -> G, sum d G -> P), -1 when P or G is empty.
    ``spacing``: three finite positive numbers (the voxel size along the three axes).  Always the floating-point path, also for spacing
    (1, 1, 1).  Asynchronous on the current stream.  The maps are exactly 3-D; label dtypes as ``seg_metrics``."""
    (pred, gt), (n0, n1, n2, _) = _seg_label_maps("seg_surface_metrics", pred, gt, exactly_3d=True)
    try:
        sp = [float(v) for v in spacing]
    except TypeError:
        raise ValueError(f"seg_surface_metrics: spacing must be three numbers, got {spacing!r}") from None
    if len(sp) != 3 or not all(math.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f"seg_surface_metrics: spacing must be three finite positive numbers, got {spacing!r}")
    tol = float(tolerance)
    if not (math.isfinite(tol) and tol >= 0):
        raise ValueError(f"seg_surface_metrics: tolerance must be finite and not negative, got {tolerance!r}")
    L = _lib.lib()
    ws = _seg_workspace("seg_surface_metrics", L.icl_seg_surface_ws_bytes, (n0, n1, n2), num_classes, pred.device)
    counts = torch.empty((int(num_classes) - 1, 7), dtype=torch.int64, device=pred.device)
    values = torch.empty((int(num_classes) - 1, 6), dtype=torch.float64, device=pred.device)
    _lib.check(L.icl_seg_surface_metrics(_ptr(pred), _SEG_DTYPES[pred.dtype], _ptr(gt), _SEG_DTYPES[gt.dtype], n0, n1, n2, int(num_classes),
                                         sp[0], sp[1], sp[2], tol, _ptr(counts), _ptr(values), _ptr(ws), _stream(pred)), "seg_surface_metrics")
    return counts, values


def _seg_components_args(who, label_map, num_classes, connectivity):
    """The checks ``seg_components`` and ``seg_filter_components`` share: (contiguous 3-D view, n0, n1, n2, workspace)."""
    (m,), (n0, n1, n2, _) = _seg_label_maps(who, label_map)
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity not in (1, 2, 3):
        raise ValueError(f"{who}: connectivity must be 1, 2 or 3, got {connectivity!r}")
    return m, n0, n1, n2, _seg_workspace(who, _lib.lib().icl_seg_components_ws_bytes, (n0, n1, n2), num_classes, m.device)


def seg_components(label_map: torch.Tensor, num_classes: int, connectivity: int = 1):
    """Connected components of every foreground class in one labelling (include/icl_hip.h icl_seg_components): ``(labels, counts)`` on the
    device of the map.  ``labels`` int32 of the map's shape: 0 on background, else 1 + the linear index of the component's first voxel
    in raster order; ``counts`` int64 [num_classes - 1, 3], row c - 1 = (components of class c, voxels in the largest, its label — 0
    when the class is absent; among equal sizes the component that starts first).  ``connectivity`` 1 / 2 / 3: 6 / 18 / 26 neighbours.
    Asynchronous on the current stream.  Label dtypes and shapes as ``seg_metrics`` (a leading axis of length 1 adds no neighbour)."""
    m, n0, n1, n2, ws = _seg_components_args("seg_components", label_map, num_classes, connectivity)
    labels = torch.empty(label_map.shape, dtype=torch.int32, device=m.device)
    counts = torch.empty((int(num_classes) - 1, 3), dtype=torch.int64, device=m.device)
    _lib.check(_lib.lib().icl_seg_components(_ptr(m), _SEG_DTYPES[m.dtype], n0, n1, n2, int(num_classes), connectivity, _ptr(labels),
                                             _ptr(counts), _ptr(ws), _stream(m)), "seg_components")
    return labels, counts


def seg_filter_components(label_map: torch.Tensor, num_classes: int, connectivity: int = 1, keep_largest: bool = True, min_size: int = 0,
                          out: torch.Tensor = None) -> torch.Tensor:
    """The label map with the voxels of every component that is not kept set to 0 (include/icl_hip.h icl_seg_filter_components), in the
    map's dtype and shape: a component is kept iff (not ``keep_largest`` or it is its class's largest; ties go to the one that starts
    first in raster order) and it has at least ``min_size`` voxels.  Labels outside 1..num_classes-1 are background and come out as 0.
    ``out``: a contiguous tensor of the map's shape, dtype and device to write into — it may be the map itself.  Asynchronous on the
    current stream."""
    m, n0, n1, n2, ws = _seg_components_args("seg_filter_components", label_map, num_classes, connectivity)
    if isinstance(min_size, bool) or not isinstance(min_size, int) or not 0 <= min_size < 2 ** 63:
        raise ValueError(f"seg_filter_components: min_size must be an integer >= 0, got {min_size!r}")
    if out is None:
        out = torch.empty_like(m)
    elif out.shape != label_map.shape or out.dtype != label_map.dtype or out.device != label_map.device or not out.is_contiguous():
        raise ValueError("seg_filter_components: out must be contiguous with the map's shape, dtype and device")
    _lib.check(_lib.lib().icl_seg_filter_components(_ptr(m), _SEG_DTYPES[m.dtype], n0, n1, n2, int(num_classes), connectivity,
                                                    1 if keep_largest else 0, min_size, _ptr(out), None, _ptr(ws), _stream(m)),
               "seg_filter_components")
    return out


# --------------------------------------------------------------------------------------
# 3-D sliding window of the validation loops (val_3D.py:18-73, :128-132; csrc/kernels/window.h)
# --------------------------------------------------------------------------------------

def _window_origins(origins):
    flat = [int(v) for o in origins for v in o]
    if len(flat) != 3 * len(origins):
        raise ValueError("window origins must be (o0, o1, o2) triples")
    return (ctypes.c_int32 * max(len(flat), 1))(*flat), len(origins)


def _window_flips(who, flips, n):
    """``flips`` of ``window_gather`` / ``window_accumulate`` as a host int32 array: one mirror mask 0..7 per origin."""
    masks = list(flips)
    if len(masks) != n:
        raise ValueError(f"{who}: {len(masks)} mirror masks for {n} windows")
    for m in masks:
        if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= 7:
            raise ValueError(f"{who}: a mirror mask must be an integer 0..7 (bit a: axis a of the window), got {m!r}")
    return (ctypes.c_int32 * max(n, 1))(*masks)


def window_gather(vol: torch.Tensor, origins, roi, pads, padded, out: Optional[torch.Tensor] = None, flips=None) -> torch.Tensor:
    """``stack([pad(vol)[:, o0:o0 + r0, o1:o1 + r1, o2:o2 + r2] for o in origins]).contiguous()`` in one launch, bit-equal
    (include/icl_hip.h icl_window_gather): vol fp32 [Cin, s0, s1, s2]; origins: up to 16 triples in the padded frame ``padded``, in which the
    volume starts at ``pads`` = (a0, a1, a2); voxels outside the volume read as 0.  Returns [n, Cin, r0, r1, r2] (``out`` when given: a contiguous tensor of
    that shape, e.g. a slice of a larger batch along its first axis).  ``flips``: one mirror mask 0..7 per origin (bit a set: the window is
    mirrored along its spatial axis a) — window w comes out as ``torch.flip`` of the above along the axes of ``flips[w]``, from the same
    launch (icl_window_gather_flipped); None: the plain kernel.  Asynchronous on the current stream."""
    _require(vol)
    if vol.dtype != torch.float32 or vol.dim() != 4:
        raise ValueError(f"window_gather: needs an fp32 [Cin, s0, s1, s2] volume, got {vol.dtype} {tuple(vol.shape)}")
    vol = vol.contiguous()
    arr, n = _window_origins(origins)
    r, a, p = [int(v) for v in roi], [int(v) for v in pads], [int(v) for v in padded]
    shape = (n, vol.shape[0], *r)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=vol.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != vol.device:
        raise ValueError(f"window_gather: out must be a contiguous fp32 {shape} tensor on the volume's device")
    if flips is None:
        _lib.check(_lib.lib().icl_window_gather(_ptr(vol), _ptr(out), arr, n, vol.shape[0], *vol.shape[1:], *a, *p, *r, _stream(vol)), "window_gather")
    else:
        fl = _window_flips("window_gather", flips, n)
        _lib.check(_lib.lib().icl_window_gather_flipped(_ptr(vol), _ptr(out), arr, fl, n, vol.shape[0], *vol.shape[1:], *a, *p, *r, _stream(vol)),
                   "window_gather_flipped")
    return out


def window_accumulate(logits: torch.Tensor, origins, score: torch.Tensor, weight: torch.Tensor, importance: Optional[torch.Tensor] = None,
                      softmax: bool = False, flips=None) -> None:
    """``score[:, window] += value`` and ``weight[window] += 1`` for every window of a batch, in the given order, in one launch
    (icl_window_accumulate): logits fp32 [n, C, r0, r1, r2] (n <= 16, C <= 256), score fp32 [C, p0, p1, p2] and weight fp32 [p0, p1, p2],
    updated in place.  ``softmax``: the value is softmax(logits, 1), else the logits.  ``importance`` fp32 [r0, r1, r2]: the value is
    multiplied by it first (rounded, then added) and ``weight[window] += importance``.  ``flips``: one mirror mask 0..7 per origin — the
    logits of window w were computed on the window mirrored along the axes of ``flips[w]`` and their value is mirrored back as it is read
    (``score[:, window] += flip(value, axes)``, icl_window_accumulate_flipped); the importance map is not mirrored.  None: the plain kernel."""
    _require(logits, score, weight, importance)
    if logits.dim() != 5 or score.dim() != 4 or weight.dim() != 3 or score.shape[0] != logits.shape[1] or score.shape[1:] != weight.shape:
        raise ValueError(f"window_accumulate: shapes {tuple(logits.shape)}, {tuple(score.shape)}, {tuple(weight.shape)}")
    for t in (logits, score, weight, importance):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"window_accumulate: fp32 only, got {t.dtype}")
    if not (score.is_contiguous() and weight.is_contiguous()):
        raise ValueError("window_accumulate: score and weight are updated in place and must be contiguous")
    if importance is not None:
        if importance.shape != logits.shape[2:]:
            raise ValueError(f"window_accumulate: importance map {tuple(importance.shape)} for windows {tuple(logits.shape[2:])}")
        importance = importance.contiguous()
    logits = logits.contiguous()
    arr, n = _window_origins(origins)
    if n != logits.shape[0]:
        raise ValueError(f"window_accumulate: {n} origins for {logits.shape[0]} windows")
    if flips is None:
        _lib.check(_lib.lib().icl_window_accumulate(_ptr(logits), _ptr(importance), _ptr(score), _ptr(weight), arr, n, logits.shape[1],
                                                    *weight.shape, *logits.shape[2:], int(bool(softmax)), _stream(score)), "window_accumulate")
    else:
        fl = _window_flips("window_accumulate", flips, n)
        _lib.check(_lib.lib().icl_window_accumulate_flipped(_ptr(logits), _ptr(importance), _ptr(score), _ptr(weight), arr, fl, n,
                                                            logits.shape[1], *weight.shape, *logits.shape[2:], int(bool(softmax)),
                                                            _stream(score)), "window_accumulate_flipped")


def window_finalize(score: torch.Tensor, weight: torch.Tensor, pads, size, return_score: bool = False, label: bool = True):
    """``argmax(score / weight, 0)`` cropped to the volume ``size`` = (s0, s1, s2) that starts at ``pads`` of the padded maps, in one pass
    (icl_window_finalize): int64 [s0, s1, s2]; with ``return_score`` also the cropped quotients, fp32 [C, s0, s1, s2].  Where nothing is
    cropped the quotients REPLACE the contents of ``score`` (division in place: no second class-by-volume tensor) and ``score`` itself is
    returned for them.  ``label=False`` (with ``return_score``): the quotients alone are computed and returned."""
    _require(score, weight)
    if score.dim() != 4 or weight.dim() != 3 or score.shape[1:] != weight.shape or score.dtype != torch.float32 or weight.dtype != torch.float32:
        raise ValueError(f"window_finalize: needs fp32 score [C, p0, p1, p2] and weight [p0, p1, p2], got {tuple(score.shape)}, {tuple(weight.shape)}")
    if not (label or return_score):
        raise ValueError("window_finalize: nothing to compute")
    if not (score.is_contiguous() and weight.is_contiguous()):
        raise ValueError("window_finalize: score and weight must be contiguous")
    a, s = [int(v) for v in pads], [int(v) for v in size]
    lab = torch.empty(s, dtype=torch.int64, device=score.device) if label else None
    quot = None
    if return_score:
        quot = score if tuple(s) == tuple(weight.shape) else torch.empty((score.shape[0], *s), dtype=torch.float32, device=score.device)
    _lib.check(_lib.lib().icl_window_finalize(_ptr(score), _ptr(weight), _ptr(lab), _ptr(quot), score.shape[0], *weight.shape, *a, *s,
                                              _stream(score)), "window_finalize")
    if not label:
        return quot
    return (lab, quot) if return_score else lab
