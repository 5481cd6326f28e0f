"""References of HAT for tests/test_hat_host.py and tests/test_gpu_hat.py (CPU only: torch and numpy, no library call).

The network (the reference project has no such architecture; no HAT source was at hand either: this is the definition the project's issue tracker wrote out, which
include/innfer_amd.h and innfer_amd/architectures/HAT_arch.py repeat).  With C = embed_dim, nH heads of d = C / nH, ws = 16, ows = 24, s = upscale:

    forward(x):  reflect-pad right / bottom to multiples of 16; f = conv_first(x - mean); f = conv_after_body(norm(RHAGs(patch_embed.norm(f)))) + f;
                 conv_before_upsample + LeakyReLU(0.01); upsample (pixelshuffle); conv_last; + mean; crop           (mean, img_range 1: as SwinIR)
    RHAG i:      t = conv(OCAB(HAB_{n-1}(... HAB_0(t)))) + t
    HAB j:       u = norm1(t);  t = t + proj(attn(u)) + conv_scale * CAB(u);  t = t + fc2(GELU(fc1(norm2(t))))
                 attn: window attention with ws 16, shift 8 for odd j; -100 between region labels of the rolled frame (rows / columns split at Hp - 16 and Hp - 8)
    CAB(u):      z = conv3x3(C -> C / compress_ratio) -> exact GELU -> conv3x3(-> C);  y = sigmoid(W2 relu(W1 mean_pixels(z) + b1) + b2);  CAB = z * y[channel]
                 -- the mean runs over the whole padded grid of ONE sample
    OCAB:        u = norm1(t); q, k, v = qkv(u) ([3][nH][d]); queries: the 16 x 16 windows; keys / values of window (wy, wx): nn.Unfold(24, stride 16, padding 4) of
                 k and v (zeros outside the grid: such a key's score is its bias alone and it takes part in the softmax); softmax(q d^-0.5 k^T + B) v;
                 t = t + proj(.);  t = t + fc2(GELU(fc1(norm2(t))))
    B (HAB):     table[idx_SA[i][j]][h], idx_SA the Swin index with ws 16;  B (OCAB): table[idx_OCA[i][j]][h],
                 idx_OCA[i][j] = (ry_j - ry_i - 7) * 39 + (rx_j - rx_i - 7), negative entries indexing the table from its end (the torch rule)

forward64: that graph in float64 on the weights as given.  `fault` plants one mistake (tests/test_hat_host.py: each must move the result by at least 10 x what fp16 storage
costs on some fixture): 'no_shift', 'no_mask', 'sa_bias_T', 'oca_bias_T', 'oca_skip' (overlap keys outside the grid left out of the softmax instead of zero), 'oca_origin'
(the overlapping window taken from (16 wy, 16 wx): the -4 forgotten), 'roll_sign', 'no_conv_scale' (the factor conv_scale left out: t + y z), 'sa_bias_T' / 'oca_bias_T'
(the bias read with the two tokens exchanged; for the 256 x 576 table: with rows and columns of both windows exchanged),
'pool_unpadded' (the channel attention's mean over the unpadded H x W), 'y_per_pixel' (the squeeze / excite applied to every pixel's own z instead of the pooled mean),
'ln_pad' (LayerNorm's statistics over the 64-padded channel count).

forward_storage: the "fp16 storage model", the same graph in float64 with the engine's folds and roundings -- SwinIR's (tests/_swinir_ref.py) and, for what HAT adds:
    rounded to fp16: GELU(cab.0), cab.2 (z: the pool reads the ROUNDED z), proj + shortcut, THEN that + conv_scale y z (two roundings, as the engine's two launches);
    the channel attention's 1x1 weights stay float32, y is not rounded; the unnormalised probabilities are rounded as the operand of P v (against the row's maximum).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from innfer_amd import synth

MEAN = (0.4488, 0.4371, 0.4040)
WS, OWS = 16, 24
QK_GAIN, TABLE, CA_GAIN, LAST_GAIN = 2.2, 8.0, 6.0, 0.25          # (over 256 / 576 keys SwinIR's 2.0 / 2.0 leave a third of the rows peaked; a larger QK_GAIN hides the zero-filled keys)


def shapes(in_chans=3, C=180, depths=(6,) * 6, nH=6, mlp_ratio=2.0, s=4, compress=3, squeeze=30):
    """State-dict key -> shape of the parameters, written out from the definition above (compared with innfer_amd's hat_shapes by the host test)."""
    hid, sh = int(C * mlp_ratio), {}

    def wb(k, *w):
        sh[k + ".weight"], sh[k + ".bias"] = tuple(w), (w[0],)
    wb("conv_first", C, in_chans, 3, 3)
    wb("patch_embed.norm", C)
    for i, depth in enumerate(depths):
        g = f"layers.{i}.residual_group."
        for j in range(depth):
            b = g + f"blocks.{j}."
            wb(b + "norm1", C)
            sh[b + "attn.relative_position_bias_table"] = (961, nH)
            wb(b + "attn.qkv", 3 * C, C)
            wb(b + "attn.proj", C, C)
            wb(b + "conv_block.cab.0", C // compress, C, 3, 3)
            wb(b + "conv_block.cab.2", C, C // compress, 3, 3)
            wb(b + "conv_block.cab.3.attention.1", C // squeeze, C, 1, 1)
            wb(b + "conv_block.cab.3.attention.3", C, C // squeeze, 1, 1)
            wb(b + "norm2", C)
            wb(b + "mlp.fc1", hid, C)
            wb(b + "mlp.fc2", C, hid)
        o = g + "overlap_attn."
        wb(o + "norm1", C)
        sh[o + "relative_position_bias_table"] = (1521, nH)
        wb(o + "qkv", 3 * C, C)
        wb(o + "proj", C, C)
        wb(o + "norm2", C)
        wb(o + "mlp.fc1", hid, C)
        wb(o + "mlp.fc2", C, hid)
        wb(f"layers.{i}.conv", C, C, 3, 3)
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


def index_sa():
    r, c = torch.arange(256) // 16, torch.arange(256) % 16
    return (r[:, None] - r[None, :] + 15) * 31 + (c[:, None] - c[None, :] + 15)


def index_oca():
    qy, qx = torch.arange(256) // 16, torch.arange(256) % 16
    ky, kx = torch.arange(576) // 24, torch.arange(576) % 24
    return (ky[None, :] - qy[:, None] - 7) * 39 + (kx[None, :] - qx[:, None] - 7)


def buffers():
    """The two top-level buffers a published checkpoint carries beside its parameters."""
    return {"relative_position_index_SA": index_sa(), "relative_position_index_OCA": index_oca()}


def fill(in_chans=3, C=180, depths=(6,) * 6, nH=6, mlp_ratio=2.0, s=4, compress=3, squeeze=30, seed=0):
    """{key: float32 torch tensor}: SwinIR's scales (conv / Linear weights uniform +-sqrt(3 / fan_in); the q and k rows of every qkv times QK_GAIN and the bias tables uniform
    +-TABLE, so that softmax rows are far from uniform; LayerNorm weights in [0.5, 1.5], biases +-0.2; other biases +-0.1; proj and fc2 weights times 0.5; conv_last times
    LAST_GAIN) and, for the channel attention, both 1x1 weights times CA_GAIN, so that y moves with the pooled mean and spreads over (0, 1)."""
    sd = {}
    for key, shp in shapes(in_chans, C, depths, nH, mlp_ratio, s, compress, squeeze).items():
        ks = synth.key_seed(key, seed)
        if key.endswith("relative_position_bias_table"):
            v = synth.uniform(shp, ks, -TABLE, TABLE)
        elif key.endswith("weight") and len(shp) >= 2:
            b = float(np.sqrt(3.0 / np.prod(shp[1:])))
            v = synth.uniform(shp, ks, -b, b)
            if key.endswith("qkv.weight"):
                v[:2 * C] *= np.float32(QK_GAIN)
            if key.endswith("proj.weight") or key.endswith("mlp.fc2.weight"):
                v = v * np.float32(0.5)
            if ".attention." in key:
                v = v * np.float32(CA_GAIN)
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


def depths_of(sd):
    depths = []
    while f"layers.{len(depths)}.residual_group.blocks.0.norm1.weight" in sd:
        j = 0
        while f"layers.{len(depths)}.residual_group.blocks.{j}.norm1.weight" in sd:
            j += 1
        depths.append(j)
    return depths


def _windows(u):
    N, C, H, W = u.shape
    return u.reshape(N, C, H // 16, 16, W // 16, 16).permute(0, 2, 4, 3, 5, 1).reshape(N, (H // 16) * (W // 16), 256, C)


def _unwindows(w, H, W):
    N, _, _, C = w.shape
    return w.reshape(N, H // 16, W // 16, 16, 16, C).permute(0, 5, 1, 3, 2, 4).reshape(N, C, H, W)


def shift_mask(Hp, Wp):
    """[nW, 256, 256] float64: -100 where the region labels of the two tokens differ (the rolled frame's last 16 rows / columns split at 8)."""
    band = lambda n: torch.tensor([0 if r < n - 16 else (1 if r < n - 8 else 2) for r in range(n)])
    lab = (3 * band(Hp)[:, None] + band(Wp)[None, :]).double()[None, None]
    lw = _windows(lab)[0, :, :, 0]
    return torch.where(lw[:, :, None] != lw[:, None, :], -100.0, 0.0).double()


def layer_norm(t, g, b, fault=None):
    C = t.shape[1]
    x = t.permute(0, 2, 3, 1)
    if fault == "ln_pad" and C % 64:
        Cp = -(-C // 64) * 64
        mu = x.sum(-1, keepdim=True) / Cp
        var = (((x - mu) ** 2).sum(-1, keepdim=True) + (Cp - C) * mu ** 2) / Cp
        y = (x - mu) / torch.sqrt(var + 1e-5) * g + b
    else:
        y = F.layer_norm(x, (C,), g, b, 1e-5)
    return y.permute(0, 3, 1, 2)


def dense_table(table, index):
    """[rows, nH] table and [q, k] index (negative entries from the end) -> [nH, q, k]."""
    return table[index.reshape(-1)].reshape(index.shape[0], index.shape[1], -1).permute(2, 0, 1)


def overlap_kv(t, origin=-4):
    """[N, C, Hp, Wp] -> [N, nW, 576, C]: the 24 x 24 pixels from (16 wy + origin, 16 wx + origin) of every window, zeros outside the grid, and [nW, 576] bool: inside."""
    N, C, Hp, Wp = t.shape
    lo, hi = -origin, 24 - 16 + origin
    p = F.pad(t, (lo, hi, lo, hi))
    inside = F.pad(torch.ones(1, 1, Hp, Wp, dtype=t.dtype), (lo, hi, lo, hi))
    unf = lambda a: F.unfold(a, 24, stride=16).reshape(a.shape[0], a.shape[1], 576, -1).permute(0, 3, 2, 1)
    return unf(p), unf(inside)[0, :, :, 0] > 0


def softmax_pv(S, v, storage, r16):
    if storage:
        e = torch.exp(S - S.amax(-1, keepdim=True))
        return r16((r16(e) @ v) / e.sum(-1, keepdim=True))
    return torch.softmax(S, -1) @ v


def _forward(sd, x, s, conv_scale, storage, fault=None, stats=None, idx=None):
    dt = torch.float64
    r16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t)
    w16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t.to(dt))
    W = lambda k: w16(sd[k + ".weight"])
    Bv = lambda k: sd[k + ".bias"].to(dt)
    norm = lambda k, t: r16(layer_norm(t, sd[k + ".weight"].to(dt), sd[k + ".bias"].to(dt), fault))
    lin = lambda w, b, t: F.conv2d(t, w[:, :, None, None] if w.dim() == 2 else w, b, padding=(w.shape[-1] // 2 if w.dim() == 4 else 0))
    N, cin, H, Wd = x.shape
    C = sd["conv_first.weight"].shape[0]
    nH = sd["layers.0.residual_group.blocks.0.attn.relative_position_bias_table"].shape[1]
    d = C // nH
    mean32 = torch.tensor(MEAN if cin == 3 else (0.0,) * cin, dtype=torch.float32)
    mean = mean32.to(dt)[None, :, None, None]
    Hp, Wp = -(-H // 16) * 16, -(-Wd // 16) * 16
    x = r16(x.to(dt))
    x = F.pad(x, (0, Wp - Wd, 0, Hp - H), mode="reflect")
    x = r16(x - mean)
    f0 = r16(F.conv2d(x, sd["conv_first.weight"].to(dt), Bv("conv_first"), padding=1))          # (storage: the first conv keeps its fp32 weights)
    isa, ioca = (index_sa(), index_oca()) if idx is None else idx
    M = shift_mask(Hp, Wp)

    def qkv_of(k, u):
        wq, bq = sd[k + ".weight"], sd[k + ".bias"]
        if storage:                                     # d^-0.5 folded into the q rows in float32, then the one rounding of the weights
            sc = torch.ones(3 * C, dtype=torch.float32)
            sc[:C] = float(np.float32(d ** -0.5))
            return r16(lin((wq * sc[:, None]).half().to(dt), (bq * sc).to(dt), u)), 1.0
        return lin(wq.to(dt), bq.to(dt), u), d ** -0.5

    def heads(w):                                       # [N, nW, T, C] -> [N, nW, nH, T, d]
        return w.reshape(w.shape[0], w.shape[1], w.shape[2], nH, d).permute(0, 1, 3, 2, 4)

    def mlp(b, t):
        h = r16(F.gelu(lin(W(b + "mlp.fc1"), Bv(b + "mlp.fc1"), norm(b + "norm2", t))))
        return r16(lin(W(b + "mlp.fc2"), Bv(b + "mlp.fc2"), h) + t)

    t = norm("patch_embed.norm", f0)
    for i, depth in enumerate(depths_of(sd)):
        short = t
        g = f"layers.{i}.residual_group."
        for j in range(depth):
            b = g + f"blocks.{j}."
            shift = 8 if j % 2 and fault != "no_shift" else 0
            u = norm(b + "norm1", t)
            # the conv block on the UNSHIFTED u
            zc = r16(F.gelu(lin(W(b + "conv_block.cab.0"), Bv(b + "conv_block.cab.0"), u)))
            z = r16(lin(W(b + "conv_block.cab.2"), Bv(b + "conv_block.cab.2"), zc))
            a = b + "conv_block.cab.3.attention."
            w1, b1, w2, b2 = sd[a + "1.weight"].to(dt), sd[a + "1.bias"].to(dt), sd[a + "3.weight"].to(dt), sd[a + "3.bias"].to(dt)
            if fault == "y_per_pixel":
                pooled = z
            elif fault == "pool_unpadded":
                pooled = z[:, :, :H, :Wd].mean((2, 3), keepdim=True)
            else:
                pooled = z.mean((2, 3), keepdim=True)
            y = torch.sigmoid(F.conv2d(F.relu(F.conv2d(pooled, w1, b1)), w2, b2))
            us = torch.roll(u, (-shift, -shift), (2, 3)) if shift else u
            qkv, qscale = qkv_of(b + "attn.qkv", us)
            win = _windows(qkv)                           # [N, nW, 256, 3 C]
            q, k, v = heads(win[..., :C]) * qscale, heads(win[..., C:2 * C]), heads(win[..., 2 * C:])
            Bh = dense_table(sd[b + "attn.relative_position_bias_table"].to(dt), isa)
            S = q @ k.transpose(-1, -2) + (Bh.transpose(-1, -2) if fault == "sa_bias_T" else Bh)
            if shift and fault != "no_mask":
                S = S + M[None, :, None]
            if stats is not None:
                stats.setdefault("pmax", []).append(torch.softmax(S, -1).amax(-1).flatten())
            o = softmax_pv(S, v, storage, r16)
            o = _unwindows(o.permute(0, 1, 3, 2, 4).reshape(N, -1, 256, C), Hp, Wp)
            if shift:
                o = torch.roll(o, (-shift, -shift) if fault == "roll_sign" else (shift, shift), (2, 3))
            t = r16(lin(W(b + "attn.proj"), Bv(b + "attn.proj"), o) + t)
            t = r16(t + (1.0 if fault == "no_conv_scale" else conv_scale) * y * z)
            t = mlp(b, t)
        o_ = g + "overlap_attn."
        u = norm(o_ + "norm1", t)
        qkv, qscale = qkv_of(o_ + "qkv", u)
        q = heads(_windows(qkv[:, :C])) * qscale
        kw, inside = overlap_kv(qkv[:, C:], 0 if fault == "oca_origin" else -4)          # [N, nW, 576, 2 C]
        k, v = heads(kw[..., :C]), heads(kw[..., C:])
        Bh = dense_table(sd[o_ + "relative_position_bias_table"].to(dt), ioca)
        if fault == "oca_bias_T":                       # the table read with query and key positions exchanged: B[i][j] of the key's position inside the central 16 x 16
            Bh = dense_table(sd[o_ + "relative_position_bias_table"].to(dt), ioca.reshape(16, 16, 24, 24).permute(1, 0, 3, 2).reshape(256, 576))
        S = q @ k.transpose(-1, -2) + Bh
        if fault == "oca_skip":
            S = S.masked_fill(~inside[None, :, None, None, :], float("-inf"))
        if stats is not None:
            stats.setdefault("pmax", []).append(torch.softmax(S, -1).amax(-1).flatten())
        o = softmax_pv(S, v, storage, r16)
        o = _unwindows(o.permute(0, 1, 3, 2, 4).reshape(N, -1, 256, C), Hp, Wp)
        t = r16(lin(W(o_ + "proj"), Bv(o_ + "proj"), o) + t)
        t = mlp(o_, t)
        t = r16(lin(W(f"layers.{i}.conv"), Bv(f"layers.{i}.conv"), t) + short)
    f = r16(lin(W("conv_after_body"), Bv("conv_after_body"), norm("norm", t)) + f0)
    y = r16(F.leaky_relu(lin(W("conv_before_upsample.0"), Bv("conv_before_upsample.0"), f), 0.01))
    for k in sorted(k[:-7] for k in sd if k.startswith("upsample.") and k.endswith(".weight")):
        y = F.pixel_shuffle(r16(lin(W(k), Bv(k), y)), 3 if s == 3 else 2)
    y = r16(lin(W("conv_last"), (sd["conv_last.bias"] + mean32).to(dt) if storage else Bv("conv_last"), y))
    if not storage:
        y = y + mean
    return y[:, :, :H * s, :Wd * s]


def forward64(sd, x, s, conv_scale, fault=None, stats=None, idx=None):
    return _forward(sd, x, s, conv_scale, False, fault, stats, idx)


def forward_storage(sd, x, s, conv_scale):
    return _forward(sd, x, s, conv_scale, True)


def peaked_share(sd, x, s, conv_scale):
    """Share of softmax rows (all blocks, windows, heads) whose largest probability exceeds 0.5, in the float64 forward."""
    st = {}
    forward64(sd, x, s, conv_scale, stats=st)
    return float((torch.cat(st["pmax"]) > 0.5).double().mean())


def codes(y):
    """tensor2np's uint8 codes of a planar result (clip(255 y), round half to even), channel order left alone."""
    return torch.round((255.0 * y.double()).clamp(0, 255)).to(torch.int16)


def codes_within_one(y, ref):
    return float(((codes(y) - codes(ref)).abs() <= 1).double().mean())


# The network fixtures of both test files: (C, nH, depths, input shape, scale, compress_ratio, squeeze_factor, conv_scale, the checkpoint carries the index buffers, seed);
# mlp_ratio 2; the input is synth.uniform(shape, 7 + seed).
FIXTURES = {
    "C60 [2] x2 16x16 cs1": (60, 6, (2,), (1, 3, 16, 16), 2, 3, 30, 1.0, True, 1),
    "C60 [1,1] x4 13x21 (padded) cs1": (60, 6, (1, 1), (1, 3, 13, 21), 4, 3, 30, 1.0, True, 2),
    "C180 [2] x3 32x48 cs0.01": (180, 6, (2,), (1, 3, 32, 48), 3, 3, 30, 0.01, True, 3),
    "C144 [2] x2 batch of two 19x26 cs1 (formula indices)": (144, 6, (2,), (2, 3, 19, 26), 2, 24, 24, 1.0, False, 4),
    "C60 [2] x2 48x48 cs1": (60, 6, (2,), (1, 3, 48, 48), 2, 3, 30, 1.0, True, 5),
}
_CASES = {}


def fixture_sd(name, with_buffers=None):
    C, nH, depths, shape, s, cr, sq, cs, stored, seed = FIXTURES[name]
    sd = fill(shape[1], C, depths, nH, 2.0, s, cr, sq, seed)
    if stored if with_buffers is None else with_buffers:
        sd.update(buffers())
    return sd


def case(name):
    """(state dict without buffers, input, float64 result, storage-model result) of a fixture, computed once per process and left unchanged."""
    if name not in _CASES:
        C, nH, depths, shape, s, cr, sq, cs, stored, seed = FIXTURES[name]
        sd = fixture_sd(name, False)
        x = torch.from_numpy(synth.uniform(shape, 7 + seed))
        _CASES[name] = (sd, x, forward64(sd, x, s, cs), forward_storage(sd, x, s, cs))
    return _CASES[name]
