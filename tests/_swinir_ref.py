"""References of SwinIR for tests/test_swinir_host.py and tests/test_gpu_swinir.py (CPU only: torch and numpy, no library call).

The network (the reference project has no such architecture; this is the published definition, KAIR / BasicSR swinir_arch.py, written out from its text):

    SwinIR(img_size, patch_size 1, in_chans 3, embed_dim C, depths, num_heads nH, window_size 8, mlp_ratio, qkv_bias, patch_norm, upscale s, img_range 1, upsampler, resi_connection)
    forward(x):   reflect-pad right / bottom to multiples of 8; x = x - mean; f = conv_first(x); f = conv_after_body(norm(RSTBs(patch_embed.norm(f)))) + f; tail; + mean;
                  crop to s H x s W.    mean = (0.4488, 0.4371, 0.4040) for three channels, else zeros.  Tokens are pixels; LayerNorm(C): biased variance, eps 1e-5, affine.
    RSTB i:       t = conv(blocks(t)) + t;   conv = Conv2d(C, C, 3, 1, 1) ('1conv') or Conv2d(C, C/4, 3), LeakyReLU(0.2), Conv2d(C/4, C/4, 1), LeakyReLU(0.2), Conv2d(C/4, C, 3)
    block j:      t = t + proj(attn(norm1(t)));  t = t + fc2(GELU(fc1(norm2(t))))  (exact GELU);  shift = 4 for odd j, whatever the input's size
    attn(u):      u' = roll(u, (-shift, -shift)); 8 x 8 windows, token i = pixel (i // 8, i % 8); qkv(u') split [3][nH][d]; per window and head
                  S = (q d^-0.5) k^T + B_h + M, P = softmax(S), o = P v;  B_h[i][j] = table[(ri - rj + 7) 15 + (ci - cj + 7)][h];  M (shift only) = -100 where the labels
                  3 a(r) + b(c) of the two tokens' pixels in the rolled frame differ (a(r) = 0 for r < Hp - 8, 1 for r < Hp - 4, else 2);  heads concatenated, projected,
                  windows reassembled, rolled back by (+shift, +shift)
    tails:        pixelshuffle: conv_before_upsample.0 (C -> 64) + LeakyReLU(0.01); per factor 2 Conv2d(64, 256) + PixelShuffle(2) (s 3: Conv2d(64, 576) + PixelShuffle(3));
                  conv_last.  pixelshuffledirect: upsample.0 = Conv2d(C, s^2 out) + PixelShuffle(s).  nearest+conv: conv_before_upsample.0 + LeakyReLU(0.01);
                  lrelu(conv_up1(nearest2x)); s 4: lrelu(conv_up2(nearest2x)); conv_last(lrelu(conv_hr)), those lrelu with slope 0.2

forward64: that graph in float64 on the weights as given.  `fault` plants one mistake (tests/test_swinir_host.py: each must move the result by far more than fp16 storage does):
    'no_shift' no cyclic shift (and no mask), 'no_mask', 'no_bias', 'bias_T' (B_h transposed), 'roll_sign' (the roll back with the wrong sign), 'ln_pad' (LayerNorm's
    statistics taken over the 64-padded channel count, the pad channels counted as zeros).

forward_storage: the "fp16 storage model" -- the same graph in float64 with the engine's folds and roundings:
    folds, each in float32 before the weights' one rounding to fp16: d^-0.5 into the q rows of attn.qkv and their bias; + mean into the bias of the last conv
    (pixelshuffledirect: of upsample.0, once per phase); - mean is the first conv's input map: its operand is fp16(x - mean), the zero padding behind it;
    weights: every conv / Linear weight rounded to fp16 EXCEPT conv_first's (the engine's first conv multiplies fp32 weights as fp16 pairs); biases, LayerNorm affines
    and the bias table stay float32;
    rounded to fp16 (the input and every launch's stored result): the input; x - mean; conv_first; every LayerNorm; q, k, v; the UNNORMALISED probabilities
    exp(S - max) as the operand of P v (the sum in the denominator is taken over the unrounded ones); o = (P v) / sum; proj + shortcut; GELU(fc1); fc2 + shortcut; every
    conv of an RSTB's `conv` (after its LeakyReLU / with its shortcut); conv_after_body + shortcut; every conv of the tail after its activation; the result.
Its distance from forward64 is what fp16 storage costs a case; the engine differs from it in the fp32 order of summation, the fp32 statistics, softmax in fp32 and the
erf approximation only.

fill: conv and Linear weights uniform +-sqrt(3 / fan_in) seeded by synth.key_seed(key, seed); the q and k rows of attn.qkv times QK_GAIN and the bias table uniform +-TABLE
(so that row softmaxes are far from uniform: tests/test_swinir_host.py prints the share of rows whose largest p exceeds 0.5); LayerNorm weights uniform in [0.5, 1.5], their
biases +-0.2; every other bias +-0.1; attn.proj and mlp.fc2 weights times 0.5 (the token stream keeps its scale over a group); the last conv's weight times LAST_GAIN[upsampler] so that
the result spans about -0.2 .. 1.2 around the mean (both clips of the uint8 store are exercised).  The input is synth.uniform in [0, 1).
With this fill the storage model alone is 7.3e-4 .. 1.6e-3 from float64 on the fixtures below, every uint8 code within +-1; the results span -0.43 .. 1.44; 52 - 67 % of the
softmax rows have a largest probability above 0.5; a planted fault moves the float64 result by 35 (LayerNorm's pad channels) to 257 (the roll back) times the storage
model's error on its worst fixture (tests/test_swinir_host.py prints the figures of every fixture).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from innfer_amd import synth

MEAN = (0.4488, 0.4371, 0.4040)
QK_GAIN, TABLE = 2.0, 2.0
LAST_GAIN = {"pixelshuffledirect": 0.18, "pixelshuffle": 0.25, "nearest+conv": 1.2}


def shapes(in_chans=3, C=180, depths=(6,) * 6, nH=6, mlp_ratio=2.0, s=4, upsampler="pixelshuffle", resi="1conv"):
    """State-dict key -> shape of the parameters, written out from the definition above (compared with innfer_amd's swinir_shapes by the host test)."""
    hid, sh = int(C * mlp_ratio), {}

    def wb(k, *w):
        sh[k + ".weight"], sh[k + ".bias"] = tuple(w), (w[0],)

    def resi_conv(k):
        if resi == "3conv":
            wb(k + ".0", C // 4, C, 3, 3); wb(k + ".2", C // 4, C // 4, 1, 1); wb(k + ".4", C, C // 4, 3, 3)
        else:
            wb(k, C, C, 3, 3)
    wb("conv_first", C, in_chans, 3, 3)
    wb("patch_embed.norm", C)
    for i, depth in enumerate(depths):
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            wb(b + "norm1", C)
            sh[b + "attn.relative_position_bias_table"] = (225, nH)
            wb(b + "attn.qkv", 3 * C, C)
            wb(b + "attn.proj", C, C)
            wb(b + "norm2", C)
            wb(b + "mlp.fc1", hid, C)
            wb(b + "mlp.fc2", C, hid)
        resi_conv(f"layers.{i}.conv")
    wb("norm", C)
    resi_conv("conv_after_body")
    if upsampler == "pixelshuffledirect":
        wb("upsample.0", s * s * in_chans, C, 3, 3)
        return sh
    wb("conv_before_upsample.0", 64, C, 3, 3)
    if upsampler == "pixelshuffle":
        if s == 3:
            wb("upsample.0", 576, 64, 3, 3)
        else:
            for st in range(int(math.log2(s))):
                wb(f"upsample.{2 * st}", 256, 64, 3, 3)
    else:
        wb("conv_up1", 64, 64, 3, 3)
        if s == 4:
            wb("conv_up2", 64, 64, 3, 3)
        wb("conv_hr", 64, 64, 3, 3)
    wb("conv_last", in_chans, 64, 3, 3)
    return sh


def position_index():
    r, c = torch.arange(64) // 8, torch.arange(64) % 8
    return (r[:, None] - r[None, :] + 7) * 15 + (c[:, None] - c[None, :] + 7)


def buffers(sd, img_size=64):
    """The two buffers a published checkpoint carries beside its parameters: attn.relative_position_index on every block, attn_mask (sized for img_size) on the odd ones."""
    out = {}
    nw = (img_size // 8) ** 2
    for k in sd:
        if k.endswith("attn.relative_position_bias_table"):
            b = k[:-len("attn.relative_position_bias_table")]
            out[b + "attn.relative_position_index"] = position_index()
            if int(b.split(".")[-2]) % 2:
                out[b + "attn_mask"] = torch.zeros(nw, 64, 64)
    return out


def fill(in_chans=3, C=180, depths=(6,) * 6, nH=6, mlp_ratio=2.0, s=4, upsampler="pixelshuffle", resi="1conv", seed=0):
    """{key: float32 torch tensor} of the network (see the module docstring for the scales)."""
    sd = {}
    last = "upsample.0.weight" if upsampler == "pixelshuffledirect" else "conv_last.weight"
    for key, shp in shapes(in_chans, C, depths, nH, mlp_ratio, s, upsampler, resi).items():
        ks = synth.key_seed(key, seed)
        if key.endswith("relative_position_bias_table"):
            v = synth.uniform(shp, ks, -TABLE, TABLE)
        elif key.endswith("weight") and len(shp) >= 2:
            b = float(np.sqrt(3.0 / np.prod(shp[1:])))
            v = synth.uniform(shp, ks, -b, b)
            if key.endswith("attn.qkv.weight"):
                v[:2 * C] *= np.float32(QK_GAIN)
            if key.endswith("attn.proj.weight") or key.endswith("mlp.fc2.weight"):
                v = v * np.float32(0.5)
            if key == last:
                v = v * np.float32(LAST_GAIN[upsampler])
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
    return u.reshape(N, C, H // 8, 8, W // 8, 8).permute(0, 2, 4, 3, 5, 1).reshape(N, (H // 8) * (W // 8), 64, C)


def _unwindows(w, H, W):
    N, _, _, C = w.shape
    return w.reshape(N, H // 8, W // 8, 8, 8, C).permute(0, 5, 1, 3, 2, 4).reshape(N, C, H, W)


def shift_mask(Hp, Wp):
    """[nW, 64, 64] float64: -100 where the region labels of the two tokens differ (the rolled frame's last 8 rows / columns split at 4)."""
    band = lambda n: torch.tensor([0 if r < n - 8 else (1 if r < n - 4 else 2) for r in range(n)])
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


def _forward(sd, x, s, upsampler, storage, fault=None, stats=None):
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
    Hp, Wp = -(-H // 8) * 8, -(-Wd // 8) * 8
    x = r16(x.to(dt))
    x = F.pad(x, (0, Wp - Wd, 0, Hp - H), mode="reflect")
    x = r16(x - mean)
    f0 = r16(F.conv2d(x, sd["conv_first.weight"].to(dt), Bv("conv_first"), padding=1))          # (storage: the first conv keeps its fp32 weights)
    idx = position_index().reshape(-1)
    M = shift_mask(Hp, Wp)

    def resi(k, t, short):
        if k + ".0.weight" in sd:
            a = r16(F.leaky_relu(lin(W(k + ".0"), Bv(k + ".0"), t), 0.2))
            a = r16(F.leaky_relu(lin(W(k + ".2"), Bv(k + ".2"), a), 0.2))
            return r16(lin(W(k + ".4"), Bv(k + ".4"), a) + short)
        return r16(lin(W(k), Bv(k), t) + short)

    t = norm("patch_embed.norm", f0)
    for i, depth in enumerate(depths_of(sd)):
        short = t
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            shift = 4 if j % 2 and fault != "no_shift" else 0
            u = norm(b + "norm1", t)
            if shift:
                u = torch.roll(u, (-shift, -shift), (2, 3))
            wq, bq = sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"]
            if storage:                                     # d^-0.5 folded into the q rows in float32, then the one rounding of the weights
                sc = torch.ones(3 * C, dtype=torch.float32)
                sc[:C] = float(np.float32(d ** -0.5))
                wq, bq, qscale = (wq * sc[:, None]).half().to(dt), (bq * sc).to(dt), 1.0
            else:
                wq, bq, qscale = wq.to(dt), bq.to(dt), d ** -0.5
            qkv = r16(lin(wq, bq, u))
            win = _windows(qkv).reshape(N, -1, 64, 3, nH, d).permute(3, 0, 1, 4, 2, 5)          # [3, N, nW, nH, 64, d]
            q, k, v = win[0] * qscale, win[1], win[2]
            S = q @ k.transpose(-1, -2)
            if fault != "no_bias":
                Bh = sd[b + "attn.relative_position_bias_table"].to(dt)[idx].reshape(64, 64, nH).permute(2, 0, 1)
                S = S + (Bh.transpose(-1, -2) if fault == "bias_T" else Bh)
            if shift and fault != "no_mask":
                S = S + M[None, :, None]
            if stats is not None:
                stats.setdefault("pmax", []).append(torch.softmax(S, -1).amax(-1).flatten())
            if storage:
                e = torch.exp(S - S.amax(-1, keepdim=True))
                o = r16((r16(e) @ v) / e.sum(-1, keepdim=True))
            else:
                o = torch.softmax(S, -1) @ v
            o = _unwindows(o.permute(0, 1, 3, 2, 4).reshape(N, -1, 64, C), Hp, Wp)
            if shift:
                o = torch.roll(o, (-shift, -shift) if fault == "roll_sign" else (shift, shift), (2, 3))
            t = r16(lin(W(b + "attn.proj"), Bv(b + "attn.proj"), o) + t)
            h = r16(F.gelu(lin(W(b + "mlp.fc1"), Bv(b + "mlp.fc1"), norm(b + "norm2", t))))
            t = r16(lin(W(b + "mlp.fc2"), Bv(b + "mlp.fc2"), h) + t)
        t = resi(f"layers.{i}.conv", t, short)
    f = resi("conv_after_body", norm("norm", t), f0)
    fold = (lambda k: (sd[k + ".bias"] + (mean32.repeat_interleave(s * s) if k == "upsample.0" else mean32)).to(dt)) if storage else Bv
    if upsampler == "pixelshuffledirect":
        y = F.pixel_shuffle(r16(lin(W("upsample.0"), fold("upsample.0"), f)), s)
    else:
        y = r16(F.leaky_relu(lin(W("conv_before_upsample.0"), Bv("conv_before_upsample.0"), f), 0.01))
        if upsampler == "pixelshuffle":
            for k in sorted(k[:-7] for k in sd if k.startswith("upsample.") and k.endswith(".weight")):
                y = F.pixel_shuffle(r16(lin(W(k), Bv(k), y)), 3 if s == 3 else 2)
        else:
            y = r16(F.leaky_relu(lin(W("conv_up1"), Bv("conv_up1"), F.interpolate(y, scale_factor=2, mode="nearest")), 0.2))
            if s == 4:
                y = r16(F.leaky_relu(lin(W("conv_up2"), Bv("conv_up2"), F.interpolate(y, scale_factor=2, mode="nearest")), 0.2))
            y = r16(F.leaky_relu(lin(W("conv_hr"), Bv("conv_hr"), y), 0.2))
        y = r16(lin(W("conv_last"), fold("conv_last"), y))
    if not storage:
        y = y + mean
    return y[:, :, :H * s, :Wd * s]


def forward64(sd, x, s, upsampler, fault=None, stats=None):
    return _forward(sd, x, s, upsampler, False, fault, stats)


def forward_storage(sd, x, s, upsampler):
    return _forward(sd, x, s, upsampler, True)


def peaked_share(sd, x, s, upsampler):
    """Share of softmax rows (all blocks, windows, heads) whose largest probability exceeds 0.5, in the float64 forward."""
    st = {}
    forward64(sd, x, s, upsampler, stats=st)
    return float((torch.cat(st["pmax"]) > 0.5).double().mean())


def codes(y):
    """tensor2np's uint8 codes of a planar result (clip(255 y), round half to even), channel order left alone."""
    return torch.round((255.0 * y.double()).clamp(0, 255)).to(torch.int16)


def codes_within_one(y, ref):
    return float(((codes(y) - codes(ref)).abs() <= 1).double().mean())


# The network fixtures of both test files: (C, nH, depths, input shape, upsampler, scale, resi, seed); mlp_ratio 2; the input is synth.uniform(shape, 7 + seed).
FIXTURES = {
    "C60 [2,2] direct x2 16x24": (60, 6, (2, 2), (1, 3, 16, 24), "pixelshuffledirect", 2, "1conv", 1),
    "C60 [2,2] direct x4 13x21 (padded)": (60, 6, (2, 2), (1, 3, 13, 21), "pixelshuffledirect", 4, "1conv", 2),
    "C180 [2] pixelshuffle x4 16x16": (180, 6, (2,), (1, 3, 16, 16), "pixelshuffle", 4, "1conv", 3),
    "C180 [2] pixelshuffle x3 9x17": (180, 6, (2,), (1, 3, 9, 17), "pixelshuffle", 3, "1conv", 4),
    "C240 [2] 3conv nearest+conv x4 16x24": (240, 8, (2,), (1, 3, 16, 24), "nearest+conv", 4, "3conv", 5),
    "C64 [2] nearest+conv x2 8x8": (64, 2, (2,), (1, 3, 8, 8), "nearest+conv", 2, "1conv", 6),
    "C60 [2] batch of two pixelshuffle x2 19x26": (60, 6, (2,), (2, 3, 19, 26), "pixelshuffle", 2, "1conv", 7),
}
_CASES = {}


def fixture_sd(name):
    C, nH, depths, shape, ups, s, resi, seed = FIXTURES[name]
    return fill(shape[1], C, depths, nH, 2.0, s, ups, resi, seed)


def case(name):
    """(state dict, input, float64 result, storage-model result) of a fixture, computed once per process and left unchanged."""
    if name not in _CASES:
        C, nH, depths, shape, ups, s, resi, seed = FIXTURES[name]
        sd = fixture_sd(name)
        x = torch.from_numpy(synth.uniform(shape, 7 + seed))
        _CASES[name] = (sd, x, forward64(sd, x, s, ups), forward_storage(sd, x, s, ups))
    return _CASES[name]
