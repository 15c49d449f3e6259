"""fp64 torch restatements with EXPLICIT masks of the stochastic SwinUNETR pieces (tests/test_swin_dropout.py on the emulator,
tests/test_gpu_swin_dropout.py on the device).  Every mask comes from ``ops.dropout_keep_mask`` — the host restatement of the
counter-based hash of csrc/kernels/misc.h — so the kernels are compared with a dense evaluation of the reference's formulas
(swinunetr_icl.py:742-749, :812, :869, :911-915) and not with themselves."""
import torch
import torch.nn.functional as F

from icl_amd import ops
from icl_amd.networks import swinunetr as SW

SITES = ("attn_drop", "proj_drop", "drop_path1", "mlp_drop1", "mlp_drop2", "drop_path2")      # the block's draw order


def keep(seed, shape, p, step=None):
    """Mask of an element-wise site over a tensor of ``shape`` (flat index = the kernel's element index), as float64 keep / (1 - p)."""
    n = 1
    for s in shape:
        n *= s
    m = torch.from_numpy(ops.dropout_keep_mask(seed, n, p, 1, step)).reshape(tuple(shape))
    return m.double() / (1.0 - p)


def attention_ref(qkv, table, index, regions, heads, scale, attn_keep=None):
    """WindowAttention.forward core (swinunetr_icl.py:728-747) in the dtype of ``qkv``; ``attn_keep`` [B_, heads, n, n] = keep / (1 - p)
    multiplies the soft-max probabilities (attn_drop, :742-747)."""
    b_, n, c3 = qkv.shape
    c = c3 // 3
    bias = table[index[:n, :n].reshape(-1)].reshape(n, n, heads).permute(2, 0, 1)
    q, k, v = qkv.view(b_, n, 3, heads, c // heads).permute(2, 0, 3, 1, 4).unbind(0)
    attn = (q * scale) @ k.transpose(-2, -1) + bias.unsqueeze(0)
    if regions is not None:
        nw = regions.shape[0]
        mask = (regions.unsqueeze(1) != regions.unsqueeze(2)).to(attn.dtype) * -100.0
        attn = (attn.view(b_ // nw, nw, heads, n, n) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, n, n)
    attn = attn.softmax(-1)
    if attn_keep is not None:
        attn = attn * attn_keep
    return (attn @ v).transpose(1, 2).reshape(b_, n, c)


def check_attention(dev, qkv, table, index, regions, heads, scale, gy, p, seed, rel_err, step=None):
    """ops.window_attention(attn_drop=p, seed) on ``dev`` against attention_ref in fp64 with the explicit mask: (output error, dqkv error,
    dtable error), each printed."""
    b_, n, _ = qkv.shape
    q = qkv.detach().to(dev).requires_grad_()
    t = table.detach().to(dev).requires_grad_()
    reg = regions.to(dev) if regions is not None else None
    y = ops.window_attention(q, t, index.to(dev), reg, heads, scale, attn_drop=p, seed=seed)
    y.backward(gy.to(dev))
    qr, tr = qkv.detach().double().requires_grad_(), table.detach().double().requires_grad_()
    yr = attention_ref(qr, tr, index, regions, heads, scale, keep(seed, (b_, heads, n, n), p, step))
    yr.backward(gy.double())
    errs = (rel_err(y.detach().cpu(), yr.detach()), rel_err(q.grad.cpu(), qr.grad), rel_err(t.grad.cpu(), tr.grad))
    print("window_attention dropout p=%g B_=%d n=%d heads=%d: out %.3g dqkv %.3g dtable %.3g" % ((p, b_, n, heads) + errs))
    return errs


def block_ref(P, x, regions, heads, window, shift, rates, masks):
    """SwinTransformerBlock.forward (swinunetr_icl.py:905-916) on channels-last ``x`` [b, d, h, w, c] in fp64.  P: the block's parameters by
    their state_dict names; rates = (drop, attn_drop, drop_path); masks: callable site -> shape -> keep / (1 - p) tensor.  Returns
    (out, x after the first residual)."""
    drop, attn_drop, drop_path = rates
    b, d, h, w, c = x.shape
    ws, ss = SW.get_window_size((d, h, w), window, shift)
    shifted = any(s > 0 for s in ss)
    n = ws[0] * ws[1] * ws[2]
    y = F.layer_norm(x, (c,), P["norm1.weight"], P["norm1.bias"], 1e-5)
    to_win, to_tok = SW.window_index((d, h, w), ws, ss if shifted else (0, 0, 0), "cpu")
    ypad = torch.cat([y.reshape(b, d * h * w, c), y.new_zeros(b, 1, c)], 1)      # slot -1 (padding) reads the zero row
    win = ypad[:, to_win.long()].reshape(-1, n, c)
    qkv = F.linear(win, P["attn.qkv.weight"], P["attn.qkv.bias"])
    b_ = qkv.shape[0]
    att = attention_ref(qkv, P["attn.relative_position_bias_table"], P["attn.relative_position_index"], regions if shifted else None, heads,
                        (c // heads) ** -0.5, masks("attn_drop", (b_, heads, n, n)) if attn_drop > 0 else None)
    o = F.linear(att, P["attn.proj.weight"], P["attn.proj.bias"])
    if drop > 0:
        o = o * masks("proj_drop", o.shape)
    part1 = o.reshape(b, -1, c)[:, to_tok.long()].reshape(b, d, h, w, c)
    x1 = x + (part1 * masks("drop_path1", (b,)).view(b, 1, 1, 1, 1) if drop_path > 0 else part1)
    z = F.gelu(F.linear(F.layer_norm(x1, (c,), P["norm2.weight"], P["norm2.bias"], 1e-5), P["mlp.linear1.weight"], P["mlp.linear1.bias"]))
    if drop > 0:
        z = z * masks("mlp_drop1", z.shape)
    z = F.linear(z, P["mlp.linear2.weight"], P["mlp.linear2.bias"])
    if drop > 0:
        z = z * masks("mlp_drop2", z.shape)
    return x1 + (z * masks("drop_path2", (b,)).view(b, 1, 1, 1, 1) if drop_path > 0 else z), x1


def base_seed_with_one_dropped(p, batch, site, step, n_sites=len(SITES)):
    """Smallest StepRNG base seed for which drop-path site ``site`` (index into the draw order) keeps at least one and drops at least one
    of ``batch`` samples at device-counter value ``step`` — found on the host with dropout_keep_mask."""
    for base in range(1, 4096):
        ops.StepRNG.enable("cpu", base_seed=base, rank=0)
        seeds = [ops.StepRNG.next_seed() for _ in range(n_sites)]
        m = ops.dropout_keep_mask(seeds[site], batch, p, 1, step)
        if m.any() and not m.all():
            return base
    raise AssertionError("no base seed found")


def check_block(dev, shift, grid, rel_err, c=32, heads=2, rates=(0.1, 0.1, 0.2), step=5):
    """One training-mode SwinTransformerBlock with all three rates on against block_ref with the masks rebuilt from the recorded seeds.
    Returns the dict of errors (output, input gradient, every parameter gradient) and whether the dropped sample's first residual is
    exactly the shortcut."""
    from icl_amd.utils.hashfill import synthetic_volume
    drop, attn_drop, drop_path = rates
    b = 2
    base = base_seed_with_one_dropped(drop_path, b, SITES.index("drop_path1"), step)
    torch.manual_seed(7)
    blk = SW.SwinTransformerBlock(c, heads, (7, 7, 7), shift, drop, attn_drop, drop_path, device=dev)
    with torch.no_grad():
        for k, t in blk.named_parameters():      # LayerNorm affine away from (1, 0), a bias table with some size
            if k.startswith("norm"):
                t.add_(0.2 * synthetic_volume(tuple(t.shape), 300 + len(k)).to(dev))
            if k.endswith("bias_table"):
                t.copy_(synthetic_volume(tuple(t.shape), 310).to(dev))
    blk.train()
    d, h, w = grid
    x = synthetic_volume((b, d, h, w, c), 301).to(dev).requires_grad_()
    gy = synthetic_volume((b, d, h, w, c), 302).to(dev)
    ws, ss = SW.get_window_size(grid, (7, 7, 7), shift)
    padded = [-(-g // s) * s for g, s in zip(grid, ws)]
    regions = SW.window_regions(padded, ws, ss, dev) if any(s > 0 for s in ss) else None
    seeds, x1_seen = [], []
    hook = blk.norm2.register_forward_hook(lambda m, inp, out: x1_seen.append(inp[0].detach().clone()))
    real = ops.StepRNG.next_seed.__func__
    try:
        ops.StepRNG.enable(dev, base_seed=base, rank=0)
        ops.StepRNG.tensor.fill_(step)

        def recording(cls):
            s = real(cls)
            seeds.append(s)
            return s
        ops.StepRNG.next_seed = classmethod(recording)
        ops.StepRNG.begin_step()
        y = blk(x, regions)
        y.backward(gy)
    finally:
        ops.StepRNG.next_seed = classmethod(real)
        ops.StepRNG.tensor = None
        hook.remove()
    assert len(seeds) == len(SITES), seeds
    by_site = dict(zip(SITES, seeds))
    rate = dict(attn_drop=attn_drop, proj_drop=drop, mlp_drop1=drop, mlp_drop2=drop, drop_path1=drop_path, drop_path2=drop_path)
    masks = lambda site, shape: keep(by_site[site], shape, rate[site], step)      # noqa: E731
    P = {k: v.detach().cpu().double().requires_grad_(v.is_floating_point() and k != "attn.relative_position_index")
         for k, v in blk.state_dict().items()}
    P["attn.relative_position_index"] = blk.attn.relative_position_index.cpu()
    xr = x.detach().cpu().double().requires_grad_()
    yr, x1r = block_ref(P, xr, regions.cpu() if regions is not None else None, heads, (7, 7, 7), shift, rates, masks)
    yr.backward(gy.cpu().double())
    errs = {"out": rel_err(y.detach().cpu(), yr.detach()), "x1": rel_err(x1_seen[0].cpu(), x1r.detach()), "dx": rel_err(x.grad.cpu(), xr.grad)}
    for k, t in blk.named_parameters():
        errs["d " + k] = rel_err(t.grad.cpu(), P[k].grad)
    for k, v in errs.items():
        print("block shift=%s grid=%s %-44s %.3g" % (shift, grid, k, v))
    m1 = ops.dropout_keep_mask(by_site["drop_path1"], b, drop_path, 1, step)
    dropped = [i for i in range(b) if not m1[i]]
    assert dropped and len(dropped) < b
    exact = all(torch.equal(x1_seen[0][i], x.detach()[i]) for i in dropped)
    kept_moved = all(not torch.equal(x1_seen[0][i], x.detach()[i]) for i in range(b) if m1[i])
    return errs, exact and kept_moved
