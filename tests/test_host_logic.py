"""CPU tests of host-side logic: sampler semantics (row f2), metric conventions (row f1), C-ABI export table,
checkpoint key filter (row f3), poly-LR schedule (T1)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_stream_sampler_matches_reference_semantics():
    from icl_amd.dataloaders.brats2019 import TwoStreamBatchSampler
    lab, unlab = list(range(0, 25)), list(range(25, 250))
    np.random.seed(1337)
    s = TwoStreamBatchSampler(lab, unlab, 4, 2)
    batches = list(s)
    assert len(batches) == len(s) == 12          # 25 // 2 primary batches per epoch, tail dropped
    seen = [i for b in batches for i in b[:2]]
    assert len(set(seen)) == 24 and all(i < 25 for i in seen)
    assert all(len(b) == 4 and all(i >= 25 for i in b[2:]) for b in batches)
    # the same numpy stream drives an independent restatement of the reference iteration (brats2019.py:208-217)
    np.random.seed(1337)
    prim = np.random.permutation(lab)
    sec = np.random.permutation(unlab)
    assert tuple(batches[0]) == (prim[0], prim[1], sec[0], sec[1])
    assert tuple(batches[5]) == (prim[10], prim[11], sec[10], sec[11])
    # rank sharding: W ranks together consume exactly the global batches
    glob = []
    np.random.seed(7)
    glob = list(TwoStreamBatchSampler(lab, unlab, 8, 4))
    shards = []
    for r in range(2):
        np.random.seed(7)
        shards.append(list(TwoStreamBatchSampler(lab, unlab, 8, 4, rank=r, world_size=2)))
    for g, a, b in zip(glob, shards[0], shards[1]):
        assert sorted(g[:4]) == sorted(a[:2] + b[:2]) and sorted(g[4:]) == sorted(a[2:] + b[2:])


def test_cal_metric_conventions_and_dice():
    from icl_amd.val_3D import binary_dice, binary_hd95, cal_metric
    z = np.zeros((8, 8, 8), bool)
    a = z.copy(); a[2:6, 2:6, 2:6] = True
    b = z.copy(); b[3:7, 2:6, 2:6] = True
    assert cal_metric(z, z) == (1, 0)                       # val_3D.py:96-97
    assert cal_metric(a, z) == (0, 373.128664) and cal_metric(z, a) == (0, 373.128664)
    d, h = cal_metric(a, b)
    assert abs(d - 2 * 48 / 128) < 1e-12 and abs(binary_dice(a, b) - 0.75) < 1e-12
    assert h == binary_hd95(b, a) == 1.0                    # the two cubes are shifted by one voxel


def test_c_abi_exports_every_declared_symbol():
    """include/icl_hip.h <-> libicl_hip.so <-> the ctypes table: no compute calls (no GPU here)."""
    from icl_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "icl_hip.h")).read()
    declared = set(re.findall(r"\b(icl_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    lib = ctypes.CDLL(build.build(verbose=False))
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, missing
    lib.icl_abi_version.restype = ctypes.c_int
    assert lib.icl_abi_version() == 1
    # bad arguments are rejected with a message, without touching a device
    lib.icl_last_error.restype = ctypes.c_char_p
    lib.icl_gelu_fwd.restype = ctypes.c_int
    assert lib.icl_gelu_fwd(None, None, ctypes.c_int64(0), None) == -1
    assert b"gelu_fwd" in lib.icl_last_error()


def test_product_path_fails_loudly_without_device_or_library(tmp_path, monkeypatch):
    from icl_amd import _lib, ops
    x = torch.zeros(1, 1, 4, 4, 4)
    assert not _lib.host_pointers_ok()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.instance_norm_relu(x)
    with pytest.raises(RuntimeError, match="not found"):
        _lib._load(str(tmp_path / "missing.so"))
    if not torch.cuda.is_available():
        from icl_amd.networks.net_factory_3d import net_factory_3d
        with pytest.raises(RuntimeError, match="no HIP device"):
            net_factory_3d("unet_3D_icl", 1, 2)


def test_checkpoint_filter_and_lr_schedule():
    from icl_amd.trainer import ICLConfig, backbone_state_dict
    from icl_amd.networks.unet_3D_icl import unet_3D_icl
    from oracle import icl_oracle as O
    m = unet_3D_icl(n_classes=2, in_channels=1, device="meta")
    sd = backbone_state_dict(m)
    assert list(sd.keys()) == [k for k, _ in O.backbone_shapes(2, 1)] and len(sd) == 38   # …BraTS.py:158-162
    assert abs(O.poly_lr(0.01, 0, 30000) - 0.01) < 1e-15 and O.poly_lr(0.01, 30000, 30000) == 0.0
    cfg = ICLConfig()
    assert cfg.base_lr * (1.0 - 100 / cfg.max_iterations) ** 0.9 == O.poly_lr(cfg.base_lr, 100, cfg.max_iterations)


def test_bench_self_launches_its_ranks_and_relays_rank0_json():
    """`python bench.py --gpus 2` (no launcher around it, the driver's N > 1 spelling without torch.distributed.run) starts its
    ranks as a child torch.distributed.run, rendezvous on 127.0.0.1; rank 0's JSON line is the last line of stdout and the return
    code is the launcher's.  The selftest mode runs the same launcher path and timing protocol on gloo with a sleep as the step."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
                        "--launcher-selftest"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["config"]["ranks"] == 2 and line["steps"] == 4
    assert line["ms_per_step"] >= 3.9        # MAX over ranks: the last rank sleeps 4 ms per step, rank 0 only 2 ms
    assert "torch.distributed.run" in r.stderr and "--nproc-per-node=2" in r.stderr
    # without enough devices the real mode refuses before anything is launched, naming the device count
    if torch.cuda.device_count() < 2:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and f"{torch.cuda.device_count()} HIP device(s)" in r.stderr and r.stdout.strip() == ""


@pytest.mark.timeout(900)
def test_no_kernel_of_the_library_keeps_a_crossed_packed_add(tmp_path):
    """Round 6: the instruction form behind the round-5 wrong result — `v_pk_add_f32 d, s0, s1 op_sel:[0,1]
    op_sel_hi:[1,0]` (halves crossed; in every case found the destination pair was also a source) — must not appear in ANY kernel of
    the library: the device assembly of the whole library, built with the flags of icl_amd/build.py, is scanned kernel by kernel.
    The mechanism of the loss is unreproduced outside the full step, so the form itself is banned."""
    import re
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this host")
    from icl_amd import build as icl_build
    csrc = os.path.join(ROOT, "icl_amd", "csrc")
    kernels, bad, procs = 0, [], []
    for src, extra in icl_build.UNITS:           # every translation unit of the library, with the flags it ships with; side by side
        out = tmp_path / (src + ".s")
        procs.append((out, subprocess.Popen([hipcc, *icl_build.FLAGS, *extra, "-I", csrc, "-S", "--cuda-device-only", "-o", str(out),
                                             os.path.join(csrc, src)], stderr=subprocess.DEVNULL)))
    for out, p in procs:
        assert p.wait() == 0, out
        text = out.read_text()
        for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
            kernels += 1
            for ln in m.group(2).splitlines():
                if "v_pk_add_f32" in ln and "op_sel:[0,1]" in ln and "op_sel_hi:[1,0]" in ln:
                    bad.append((m.group(1), ln.strip()))
    assert kernels >= 200, kernels          # the whole library was scanned (319 kernels with the forward convolution planner)
    assert not bad, bad[:4]


def test_layernorm_backward_keeps_its_bias_sums_out_of_packed_adds(tmp_path):
    """Round 5: with `b[k] += gv` packed into one `v_pk_add_f32 ... op_sel:[0,1] op_sel_hi:[1,0]` (halves crossed,
    destination pair = second source) layernorm_bwd_wgrad_kernel lost one row's term of dbeta in lanes 48..63 under concurrent streams.
    The source pins b[k] after every add; this checks what the compiler makes of it, on the device assembly of every instantiation the
    launcher uses: no packed add of that form, and the bias sums are plain v_add_f32."""
    import re
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this host")
    csrc = os.path.join(ROOT, "icl_amd", "csrc")
    sig = "(const float*, const float*, const float*, const float*, const float*, float*, float*, float*, long, int, long)"
    insts = [(1, 4), (2, 4), (4, 2), (8, 1), (16, 1)]          # icl_abi.inc ICL_LN_BW
    src = tmp_path / "ln.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "device_env_hip.h"\n#include "kernels/common.h"\n#include "kernels/token.h"\n'
                   + "".join(f"template __global__ void icl::layernorm_bwd_wgrad_kernel<{c}, {r}>{sig};\n" for c, r in insts))
    out = tmp_path / "ln.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", csrc, "-S", "--cuda-device-only", "-o", str(out), str(src)],
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    seen = 0
    for m in re.finditer(r"^(_ZN3icl26layernorm_bwd_wgrad_kernel\w+):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M):
        seen += 1
        body = m.group(2)
        crossed = [ln for ln in body.splitlines() if "v_pk_add_f32" in ln and "op_sel:[0,1] op_sel_hi:[1,0]" in ln]
        assert not crossed, (m.group(1), crossed[:2])
        assert body.count("v_add_f32") >= 8, m.group(1)
    assert seen == len(insts), seen
