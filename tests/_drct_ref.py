"""References of DRCT for tests/test_drct_host.py and tests/test_gpu_drct.py (CPU only: torch and numpy, no library call).  Natural channel order and a real torch.cat:
nothing here knows of the engine's dense slab.

The network (the reference project has no such architecture and no DRCT source was at hand: this is the definition the project's issue tracker wrote out, which
include/innfer_amd.h and innfer_amd/architectures/DRCT_arch.py repeat).  C = embed_dim, gc = 32, 16 x 16 windows, s = upscale:

    forward(x):  reflect-pad right / bottom to multiples of 16; f = conv_first(x - mean); f = conv_after_body(norm(RDG_{R-1}(.. RDG_0(patch_embed.norm(f))))) + f;
                 conv_before_upsample + LeakyReLU(0.01); upsample (pixelshuffle); conv_last; + mean; crop
    RDG(x):      x_k = lrelu_0.2(adjust_k(swin_k(cat(x, x_1 .. x_{k-1}))))  k = 1 .. 4;   x_5 = adjust_5(swin_5(cat(x, x_1 .. x_4)));   return 0.2 x_5 + x
    swin_k(t):   on dim_k = C + 32 (k - 1) channels: t = t + proj(attn(norm1(t)));  t = t + fc2(GELU(fc1(norm2(t))));  attn: shift 8 for k = 2, 4 (-100 between region
                 labels of the rolled frame); softmax(q d^-0.5 k^T + B_h + M) v with table [961, nH_k]; nH_k and the MLP's hidden size are read off the state dict

forward64: that graph in float64 on the weights as given.  `fault` plants one mistake: 'no_shift', 'no_mask', 'no_cat' (x_k left out of the later blocks' input: zeros in
its place), 'lrelu5' (an activation behind adjust_5), 'no_res_scale' (x_5 + x).  stats['smax']: (head dim, max |S|) of every block.

forward_storage: the "fp16 storage model", the same graph in float64 with the engine's folds and roundings: weights rounded to fp16 (d^-0.5 folded into the q rows in float64
first), biases float32; rounded to fp16: the input, x - mean, every conv's and Linear's result (with its shortcut or activation inside the one rounding), every LayerNorm's
result, the unnormalised probabilities as the operand of P v (against the row's maximum) and o / sum, x_k, and 0.2 x_5 + x.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import _hat_ref as HR
from innfer_amd import synth

MEAN = HR.MEAN
GC = 32
QK_GAIN, TABLE, LAST_GAIN = 1.3, 8.0, 0.25


def head_rule(dim, num_heads):
    """The published rule as the issue states it: num_heads - (dim % num_heads)."""
    return num_heads - dim % num_heads


def shapes(in_chans=3, C=180, R=6, num_heads=6, mlp_ratio=2.0, s=4):
    """State-dict key -> shape of the parameters, written out from the definition above (compared with innfer_amd's drct_shapes by the host test)."""
    sh = {}

    def wb(k, *w):
        sh[k + ".weight"], sh[k + ".bias"] = tuple(w), (w[0],)
    wb("conv_first", C, in_chans, 3, 3)
    wb("patch_embed.norm", C)
    for i in range(R):
        for k in range(1, 6):
            dim = C + GC * (k - 1)
            b = f"layers.{i}.swin{k}."
            wb(b + "norm1", dim)
            sh[b + "attn.relative_position_bias_table"] = (961, head_rule(dim, num_heads))
            wb(b + "attn.qkv", 3 * dim, dim)
            wb(b + "attn.proj", dim, dim)
            wb(b + "norm2", dim)
            wb(b + "mlp.fc1", int(dim * mlp_ratio), dim)
            wb(b + "mlp.fc2", dim, int(dim * mlp_ratio))
            wb(f"layers.{i}.adjust{k}", GC if k < 5 else C, dim, 1, 1)
    wb("norm", C)
    wb("conv_after_body", C, C, 3, 3)
    wb("conv_before_upsample.0", 64, C, 3, 3)
    if s == 3:
        wb("upsample.0", 576, 64, 3, 3)
    else:
        for st in range(int(math.log2(s))):
            wb(f"upsample.{2 * st}", 256, 64, 3, 3)
    wb("conv_last", in_chans, 64, 3, 3)
    return sh


def fill(in_chans=3, C=180, R=6, num_heads=6, mlp_ratio=2.0, s=4, seed=0):
    """{key: float32 torch tensor} with HAT's scales (tests/_hat_ref.py fill); the q and k rows of every qkv times QK_GAIN, so that the scores of the wide heads spread
    (tests/test_drct_host.py asserts max |S| >= 4 in a wide-head block of every fixture)."""
    sd = {}
    for key, shp in shapes(in_chans, C, R, num_heads, mlp_ratio, s).items():
        ks = synth.key_seed(key, seed)
        if key.endswith("relative_position_bias_table"):
            v = synth.uniform(shp, ks, -TABLE, TABLE)
        elif key.endswith("weight") and len(shp) >= 2:
            b = float(np.sqrt(3.0 / np.prod(shp[1:])))
            v = synth.uniform(shp, ks, -b, b)
            if key.endswith("qkv.weight"):
                v[:2 * shp[1]] *= np.float32(QK_GAIN)
            if key.endswith("proj.weight") or key.endswith("mlp.fc2.weight"):
                v = v * np.float32(0.5)
            if key == "conv_last.weight":
                v = v * np.float32(LAST_GAIN)
        elif key.endswith("weight"):                   # LayerNorm
            v = synth.uniform(shp, ks, 0.5, 1.5)
        elif ".norm" in key or key.startswith("norm."):
            v = synth.uniform(shp, ks, -0.2, 0.2)
        else:
            v = synth.uniform(shp, ks, -0.1, 0.1)
        sd[key] = torch.from_numpy(np.ascontiguousarray(v, np.float32))
    return sd


def groups_of(sd):
    n = 0
    while f"layers.{n}.swin1.norm1.weight" in sd:
        n += 1
    return n


def buffers(sd):
    """The buffers a published checkpoint may carry beside its parameters: attn.relative_position_index on every block, attn_mask (sized for img_size 64) on the shifted."""
    out = {}
    for i in range(groups_of(sd)):
        for k in range(1, 6):
            out[f"layers.{i}.swin{k}.attn.relative_position_index"] = HR.index_sa()
            if k in (2, 4):
                out[f"layers.{i}.swin{k}.attn_mask"] = HR.shift_mask(64, 64).float()
    return out


def _forward(sd, x, s, storage, fault=None, stats=None):
    dt = torch.float64
    r16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t)
    w16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t.to(dt))
    W = lambda k: w16(sd[k + ".weight"])
    Bv = lambda k: sd[k + ".bias"].to(dt)
    norm = lambda k, t: r16(HR.layer_norm(t, sd[k + ".weight"].to(dt), sd[k + ".bias"].to(dt)))
    lin = lambda w, b, t: F.conv2d(t, w[:, :, None, None] if w.dim() == 2 else w, b, padding=(w.shape[-1] // 2 if w.dim() == 4 else 0))
    N, cin, H, Wd = x.shape
    mean32 = torch.tensor(MEAN if cin == 3 else (0.0,) * cin, dtype=torch.float32)
    mean = mean32.to(dt)[None, :, None, None]
    Hp, Wp = -(-H // 16) * 16, -(-Wd // 16) * 16
    x = r16(x.to(dt))
    x = F.pad(x, (0, Wp - Wd, 0, Hp - H), mode="reflect")
    x = r16(x - mean)
    f0 = r16(F.conv2d(x, sd["conv_first.weight"].to(dt), Bv("conv_first"), padding=1))          # (storage: the first conv keeps its fp32 weights)
    isa = HR.index_sa()
    M = HR.shift_mask(Hp, Wp)

    def swin(b, t, shift):
        dim = t.shape[1]
        nH = sd[b + "attn.relative_position_bias_table"].shape[1]
        d = dim // nH
        heads = lambda w: w.reshape(w.shape[0], w.shape[1], w.shape[2], nH, d).permute(0, 1, 3, 2, 4)          # [N, nW, T, C] -> [N, nW, nH, T, d]
        u = norm(b + "norm1", t)
        us = torch.roll(u, (-shift, -shift), (2, 3)) if shift else u
        wq, bq = sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"]
        if storage:                                     # d^-0.5 folded into the q rows in float64, one rounding to float32 (the engine's input), then fp16
            sc = torch.ones(3 * dim, dtype=dt)
            sc[:dim] = d ** -0.5
            qkv, qscale = r16(lin((wq.to(dt) * sc[:, None]).float().half().to(dt), (bq.to(dt) * sc).float().to(dt), us)), 1.0
        else:
            qkv, qscale = lin(wq.to(dt), bq.to(dt), us), d ** -0.5
        win = HR._windows(qkv)
        q, k, v = heads(win[..., :dim]) * qscale, heads(win[..., dim:2 * dim]), heads(win[..., 2 * dim:])
        S = q @ k.transpose(-1, -2) + HR.dense_table(sd[b + "attn.relative_position_bias_table"].to(dt), isa)
        if shift and fault != "no_mask":
            S = S + M[None, :, None]
        if stats is not None:
            stats.setdefault("smax", []).append((d, float((q @ k.transpose(-1, -2)).abs().max())))
        o = HR.softmax_pv(S, v, storage, r16)
        o = HR._unwindows(o.permute(0, 1, 3, 2, 4).reshape(N, -1, 256, dim), Hp, Wp)
        if shift:
            o = torch.roll(o, (shift, shift), (2, 3))
        t = r16(lin(W(b + "attn.proj"), Bv(b + "attn.proj"), o) + t)
        h = r16(F.gelu(lin(W(b + "mlp.fc1"), Bv(b + "mlp.fc1"), norm(b + "norm2", t))))
        return r16(lin(W(b + "mlp.fc2"), Bv(b + "mlp.fc2"), h) + t)

    t = norm("patch_embed.norm", f0)
    for i in range(groups_of(sd)):
        xs = [t]
        for k in range(1, 6):
            shift = 8 if k in (2, 4) and fault != "no_shift" else 0
            cat = torch.cat(xs if fault != "no_cat" else [xs[0]] + [torch.zeros_like(v) for v in xs[1:]], 1)
            y = lin(W(f"layers.{i}.adjust{k}"), Bv(f"layers.{i}.adjust{k}"), swin(f"layers.{i}.swin{k}.", cat, shift))
            if k < 5:
                xs.append(r16(F.leaky_relu(y, 0.2)))
            else:
                if fault == "lrelu5":
                    y = F.leaky_relu(y, 0.2)
                t = r16((1.0 if fault == "no_res_scale" else 0.2) * y + t)
    f = r16(lin(W("conv_after_body"), Bv("conv_after_body"), norm("norm", t)) + f0)
    y = r16(F.leaky_relu(lin(W("conv_before_upsample.0"), Bv("conv_before_upsample.0"), f), 0.01))
    for k in sorted(k[:-7] for k in sd if k.startswith("upsample.") and k.endswith(".weight")):
        y = F.pixel_shuffle(r16(lin(W(k), Bv(k), y)), 3 if s == 3 else 2)
    y = r16(lin(W("conv_last"), (sd["conv_last.bias"].to(dt) + mean32.to(dt)).float().to(dt) if storage else Bv("conv_last"), y))
    if not storage:
        y = y + mean
    return y[:, :, :H * s, :Wd * s]


def forward64(sd, x, s, fault=None, stats=None):
    return _forward(sd, x, s, False, fault, stats)


def forward_storage(sd, x, s):
    return _forward(sd, x, s, True)


codes, codes_within_one = HR.codes, HR.codes_within_one


# The network fixtures of both test files: (C, num_heads of the published rule, R, input shape, scale, the checkpoint carries the buffers, seed); mlp_ratio 2;
# the input is synth.uniform(shape, 7 + seed).
FIXTURES = {
    "C60 R2 x2 13x21 (padded)": (60, 6, 2, (1, 3, 13, 21), 2, True, 1),           # d 10, 23, 62, 26, 47: both attention kernels
    "C180 R1 x4 32x48": (180, 6, 1, (1, 3, 32, 48), 4, False, 2),                 # d 30, 53, 122, 46, 77: every G
    "C96 R1 x3 batch of two 19x26": (96, 4, 1, (2, 3, 19, 26), 3, True, 3),
}
_CASES = {}


def fixture_sd(name, with_buffers=None):
    C, nH, R, shape, s, stored, seed = FIXTURES[name]
    sd = fill(shape[1], C, R, nH, 2.0, s, seed)
    if stored if with_buffers is None else with_buffers:
        sd.update(buffers(sd))
    return sd


def case(name):
    """(state dict without buffers, input, float64 result, storage-model result, stats of the float64 forward) of a fixture, computed once per process, left unchanged."""
    if name not in _CASES:
        C, nH, R, shape, s, stored, seed = FIXTURES[name]
        sd = fixture_sd(name, False)
        x = torch.from_numpy(synth.uniform(shape, 7 + seed))
        st = {}
        _CASES[name] = (sd, x, forward64(sd, x, s, stats=st), forward_storage(sd, x, s), st)
    return _CASES[name]
