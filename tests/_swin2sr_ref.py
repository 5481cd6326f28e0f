"""References of Swin2SR for tests/test_swin2sr_host.py and tests/test_gpu_swin2sr.py (CPU only: torch and numpy, no library call; helpers shared with _swinir_ref).

The network (the reference project has no such architecture; this is the published definition, network_swin2sr.py, written out from its text).  Everything not named here
is SwinIR's, exactly as in _swinir_ref: the reflect pad to multiples of 8, x - mean, conv_first, patch_embed.norm, RSTB = conv(blocks(t)) + t ('1conv' / '3conv'), the final
norm, conv_after_body + f, the tails, + mean, the crop, shift 4 for odd j whatever the input's size, the -100 mask between the region labels of the rolled frame.

    block j:   t = t + norm1(proj(attn(t)))          -- the norm comes AFTER the branch ("res-post-norm"); attn reads t itself
               t = t + norm2(fc2(GELU(fc1(t))))      -- exact GELU; LayerNorm(C), eps 1e-5, affine
    attn(t):   t' = roll(t, (-shift, -shift)); 8 x 8 windows; qkv = Linear(C, 3C, bias=False)(t') + cat(q_bias, zeros(C), v_bias)     -- k has NO bias
               per head h:  S = (q^ k^^T) * tau_h + B_h + M;   q^ = q / max(||q||_2, 1e-12), k^ likewise (over the d channels of the head)
               tau_h = exp(min(logit_scale[h], ln 100));   P = softmax(S);  o = P v;  heads concatenated, proj, windows back, roll back.  There is no d^-0.5.
    B_h:       rows of a table T[225][nH] = cpb_mlp(coords):  cpb_mlp = Linear(2, hidden, bias) -> ReLU -> Linear(hidden, nH, no bias)
               coords[a*15 + b] = (g(a - 7), g(b - 7)),  g(c) = sign(c) * log2(|8 c / 7| + 1) / 3        (a: row offset, b: column offset)
               B_h[i][j] = 16 * sigmoid(T[(ri - rj + 7) * 15 + (ci - cj + 7)][h])                          for tokens i = 8 ri + ci, j = 8 rj + cj
    parameters per block: attn.logit_scale [nH, 1, 1], attn.cpb_mlp.0.weight [hidden, 2], .0.bias [hidden], attn.cpb_mlp.2.weight [nH, hidden], attn.q_bias [C], attn.v_bias [C],
               attn.qkv.weight [3C, C], attn.proj.*, norm1.*, norm2.*, mlp.fc1.*, mlp.fc2.* -- NO attn.relative_position_bias_table and NO attn.qkv.bias
    buffers a checkpoint may carry: attn.relative_coords_table [1, 15, 15, 2] (authoritative when present: it feeds cpb_mlp instead of the formula),
               attn.relative_position_index [64, 64], attn_mask

forward64: that graph in float64 on the weights as given (coords: a stored relative_coords_table, else the formula).  `fault` plants one mistake
(tests/test_swin2sr_host.py: each must move the result by far more than fp16 storage does):
    'no_qk_norm' (the plain dot product times tau), 'no_clamp' (tau = exp(logit_scale)), 'pre_norm' (SwinIR's order -- norm in front of each branch -- with these weights),
    'no_sigmoid' (the MLP's raw output as the bias), 'k_bias' (q_bias also added to k), 'coords_linear' (g(c) = c / 7), and SwinIR's 'no_shift', 'no_mask', 'bias_T',
    'roll_sign', 'ln_pad'.

forward_storage: SwinIR's "fp16 storage model" with this graph's roundings:
    weights: every conv / Linear weight rounded to fp16 except conv_first's; attn.qkv WITHOUT a fold; biases (cat(q_bias, 0, v_bias) among them) and LayerNorm affines float32;
    the bias table is the float32 the shell builds (float64 evaluation, one rounding); tau float32;
    rounded to fp16: the input; x - mean; conv_first; patch_embed.norm and norm; q, k, v as stored; the norms ||q||, ||k|| and S are NOT rounded; the unnormalised
    probabilities as the operand of P v (the sum over the unrounded ones); o; u = proj; t + LN(u) ONCE; GELU(fc1); u = fc2; t + LN(u) once; everything else as SwinIR's.

fill: SwinIR's scales (conv / Linear weights uniform +-sqrt(3 / fan_in), the q and k rows of attn.qkv times QK_GAIN, LayerNorm weights in [0.5, 1.5] and biases +-0.2, other
biases +-0.1, the last conv times LAST_GAIN) and: logit_scale spread evenly over LOGIT[0] .. LOGIT[1] across the heads with a small seeded jitter (tau from about 3 to
beyond the clamp at 100: at least one head on each side of ln 100 in every fixture); cpb_mlp.0.weight uniform +-CPB_W0, its bias +-CPB_B0, cpb_mlp.2.weight uniform
+-CPB_W2 sqrt(3 / hidden) (B = 16 sigmoid(T) varies by several units across offsets); q_bias and v_bias uniform +-QV_BIAS.
Figures of this fill (tests/test_swin2sr_host.py prints them per fixture) are in that file's docstrings.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import _swinir_ref as SR
from _swinir_ref import LAST_GAIN, MEAN, codes, codes_within_one, depths_of, layer_norm, position_index, shift_mask  # noqa: F401
from innfer_amd import synth

QK_GAIN = 2.0
LOGIT = (1.2, 4.7)
CPB_W0, CPB_B0, CPB_W2 = 6.0, 1.0, 2.0
QV_BIAS = 1.0
LN100 = math.log(100.0)


def shapes(in_chans=3, C=180, depths=(6,) * 6, nH=6, mlp_ratio=2.0, s=4, upsampler="pixelshuffle", resi="1conv", cpb=512):
    """State-dict key -> shape of the parameters, written out from the definition above (compared with innfer_amd's swin2sr_shapes by the host test)."""
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
            sh[b + "attn.logit_scale"] = (nH, 1, 1)
            wb(b + "attn.cpb_mlp.0", cpb, 2)
            sh[b + "attn.cpb_mlp.2.weight"] = (nH, cpb)
            sh[b + "attn.q_bias"], sh[b + "attn.v_bias"] = (C,), (C,)
            sh[b + "attn.qkv.weight"] = (3 * C, C)
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


def coords_table(linear=False):
    """[225, 2] float64: row 15 a + b = (g(a - 7), g(b - 7))."""
    c = torch.arange(-7, 8, dtype=torch.float64)
    g = c / 7 if linear else torch.sign(c) * torch.log2((8 * c / 7).abs() + 1) / 3
    return torch.stack(torch.meshgrid(g, g, indexing="ij"), -1).reshape(225, 2)


def buffers(sd, img_size=64, coords=None):
    """The three buffers a published checkpoint carries beside its parameters: attn.relative_coords_table and attn.relative_position_index on every block, attn_mask
    (sized for img_size) on the odd ones."""
    out = {}
    nw = (img_size // 8) ** 2
    ct = (coords_table() if coords is None else coords).reshape(1, 15, 15, 2).float()
    for k in sd:
        if k.endswith("attn.logit_scale"):
            b = k[:-len("attn.logit_scale")]
            out[b + "attn.relative_coords_table"] = ct.clone()
            out[b + "attn.relative_position_index"] = position_index()
            if int(b.split(".")[-2]) % 2:
                out[b + "attn_mask"] = torch.zeros(nw, 64, 64)
    return out


def fill(in_chans=3, C=180, depths=(6,) * 6, nH=6, mlp_ratio=2.0, s=4, upsampler="pixelshuffle", resi="1conv", cpb=512, seed=0):
    """{key: float32 torch tensor} of the network (see the module docstring for the scales)."""
    sd = {}
    last = "upsample.0.weight" if upsampler == "pixelshuffledirect" else "conv_last.weight"
    for key, shp in shapes(in_chans, C, depths, nH, mlp_ratio, s, upsampler, resi, cpb).items():
        ks = synth.key_seed(key, seed)
        if key.endswith("attn.logit_scale"):
            base = np.linspace(LOGIT[0], LOGIT[1], nH, dtype=np.float32) if nH > 1 else np.float32([LOGIT[1]])
            v = (base + synth.uniform((nH,), ks, -0.1, 0.1)).reshape(shp)
        elif key.endswith("cpb_mlp.0.weight"):
            v = synth.uniform(shp, ks, -CPB_W0, CPB_W0)
        elif key.endswith("cpb_mlp.0.bias"):
            v = synth.uniform(shp, ks, -CPB_B0, CPB_B0)
        elif key.endswith("cpb_mlp.2.weight"):
            b = CPB_W2 * float(np.sqrt(3.0 / shp[1]))
            v = synth.uniform(shp, ks, -b, b)
        elif key.endswith("q_bias") or key.endswith("v_bias"):
            v = synth.uniform(shp, ks, -QV_BIAS, QV_BIAS)
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


def bias_table(sd, b, coords=None, fault=None):
    """[nH, 64, 64] float64 of block prefix `b`: 16 sigmoid(cpb_mlp(coords)) gathered by the position index."""
    xy = coords_table(fault == "coords_linear") if coords is None else coords.double().reshape(225, 2)
    hid = torch.relu(xy @ sd[b + "attn.cpb_mlp.0.weight"].double().T + sd[b + "attn.cpb_mlp.0.bias"].double())
    T = hid @ sd[b + "attn.cpb_mlp.2.weight"].double().T
    if fault != "no_sigmoid":
        T = 16.0 * torch.sigmoid(T)
    nH = T.shape[1]
    return T[position_index().reshape(-1)].reshape(64, 64, nH).permute(2, 0, 1)


def tau_of(sd, b, fault=None):
    ls = sd[b + "attn.logit_scale"].double().reshape(-1)
    return torch.exp(ls if fault == "no_clamp" else ls.clamp(max=LN100))


def _forward(sd, x, s, upsampler, storage, fault=None, stats=None, coords=None):
    dt = torch.float64
    r16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t)
    w16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t.to(dt))
    W = lambda k: w16(sd[k + ".weight"])
    Bv = lambda k: sd[k + ".bias"].to(dt)
    ln = lambda k, t: layer_norm(t, sd[k + ".weight"].to(dt), sd[k + ".bias"].to(dt), fault)
    lin = lambda w, b, t: F.conv2d(t, w[:, :, None, None] if w.dim() == 2 else w, b, padding=(w.shape[-1] // 2 if w.dim() == 4 else 0))
    N, cin, H, Wd = x.shape
    C = sd["conv_first.weight"].shape[0]
    nH = sd["layers.0.residual_group.blocks.0.attn.logit_scale"].shape[0]
    d = C // nH
    mean32 = torch.tensor(MEAN if cin == 3 else (0.0,) * cin, dtype=torch.float32)
    mean = mean32.to(dt)[None, :, None, None]
    Hp, Wp = -(-H // 8) * 8, -(-Wd // 8) * 8
    x = r16(x.to(dt))
    x = F.pad(x, (0, Wp - Wd, 0, Hp - H), mode="reflect")
    x = r16(x - mean)
    f0 = r16(F.conv2d(x, sd["conv_first.weight"].to(dt), Bv("conv_first"), padding=1))          # (storage: the first conv keeps its fp32 weights)
    M = shift_mask(Hp, Wp)

    def resi(k, t, short):
        if k + ".0.weight" in sd:
            a = r16(F.leaky_relu(lin(W(k + ".0"), Bv(k + ".0"), t), 0.2))
            a = r16(F.leaky_relu(lin(W(k + ".2"), Bv(k + ".2"), a), 0.2))
            return r16(lin(W(k + ".4"), Bv(k + ".4"), a) + short)
        return r16(lin(W(k), Bv(k), t) + short)

    def attn(b, u, shift):
        if shift:
            u = torch.roll(u, (-shift, -shift), (2, 3))
        qb, vb = sd[b + "attn.q_bias"].to(dt), sd[b + "attn.v_bias"].to(dt)
        bias = torch.cat([qb, qb if fault == "k_bias" else torch.zeros(C, dtype=dt), vb])
        qkv = r16(lin(W(b + "attn.qkv"), bias, u))
        win = SR._windows(qkv).reshape(N, -1, 64, 3, nH, d).permute(3, 0, 1, 4, 2, 5)          # [3, N, nW, nH, 64, d]
        q, k, v = win[0], win[1], win[2]
        tau, Bh = tau_of(sd, b, fault), bias_table(sd, b, coords, fault)
        if storage:
            tau, Bh = tau.float().to(dt), Bh.float().to(dt)
        if fault != "no_qk_norm":
            q = q / q.norm(dim=-1, keepdim=True).clamp(min=1e-12)
            k = k / k.norm(dim=-1, keepdim=True).clamp(min=1e-12)
        S = (q @ k.transpose(-1, -2)) * tau[:, None, None] + (Bh.transpose(-1, -2) if fault == "bias_T" else Bh)
        if shift and fault != "no_mask":
            S = S + M[None, :, None]
        if stats is not None:
            stats.setdefault("pmax", []).append(torch.softmax(S, -1).amax(-1).flatten())
        if storage:
            e = torch.exp(S - S.amax(-1, keepdim=True))
            o = r16((r16(e) @ v) / e.sum(-1, keepdim=True))
        else:
            o = torch.softmax(S, -1) @ v
        o = SR._unwindows(o.permute(0, 1, 3, 2, 4).reshape(N, -1, 64, C), Hp, Wp)
        if shift:
            o = torch.roll(o, (-shift, -shift) if fault == "roll_sign" else (shift, shift), (2, 3))
        return o

    t = r16(ln("patch_embed.norm", f0))
    for i, depth in enumerate(depths_of(sd)):
        short = t
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            shift = 4 if j % 2 and fault != "no_shift" else 0
            if fault == "pre_norm":
                t = t + lin(W(b + "attn.proj"), Bv(b + "attn.proj"), attn(b, ln(b + "norm1", t), shift))
                t = t + lin(W(b + "mlp.fc2"), Bv(b + "mlp.fc2"), F.gelu(lin(W(b + "mlp.fc1"), Bv(b + "mlp.fc1"), ln(b + "norm2", t))))
                continue
            u = r16(lin(W(b + "attn.proj"), Bv(b + "attn.proj"), attn(b, t, shift)))
            t = r16(t + ln(b + "norm1", u))
            h = r16(F.gelu(lin(W(b + "mlp.fc1"), Bv(b + "mlp.fc1"), t)))
            u = r16(lin(W(b + "mlp.fc2"), Bv(b + "mlp.fc2"), h))
            t = r16(t + ln(b + "norm2", u))
        t = resi(f"layers.{i}.conv", t, short)
    f = resi("conv_after_body", r16(ln("norm", t)), f0)
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


def forward64(sd, x, s, upsampler, fault=None, stats=None, coords=None):
    return _forward(sd, x, s, upsampler, False, fault, stats, coords)


def forward_storage(sd, x, s, upsampler, coords=None):
    return _forward(sd, x, s, upsampler, True, coords=coords)


def peaked_share(sd, x, s, upsampler):
    """Share of softmax rows (all blocks, windows, heads) whose largest probability exceeds 0.5, in the float64 forward."""
    st = {}
    forward64(sd, x, s, upsampler, stats=st)
    return float((torch.cat(st["pmax"]) > 0.5).double().mean())


# The network fixtures of both test files: (C, nH, depths, input shape, upsampler, scale, resi, cpb hidden, seed); mlp_ratio 2; the input is synth.uniform(shape, 7 + seed).
FIXTURES = {
    "C60 [2,2] direct x2 16x24": (60, 6, (2, 2), (1, 3, 16, 24), "pixelshuffledirect", 2, "1conv", 512, 1),
    "C60 [2] direct x4 13x21 (padded)": (60, 6, (2,), (1, 3, 13, 21), "pixelshuffledirect", 4, "1conv", 512, 2),
    "C180 [2] pixelshuffle x4 16x16": (180, 6, (2,), (1, 3, 16, 16), "pixelshuffle", 4, "1conv", 512, 3),
    "C180 [2] pixelshuffle x3 9x17": (180, 6, (2,), (1, 3, 9, 17), "pixelshuffle", 3, "1conv", 512, 4),
    "C240 nH8 [2] 3conv nearest+conv x4 16x24": (240, 8, (2,), (1, 3, 16, 24), "nearest+conv", 4, "3conv", 512, 5),
    "C64 nH2 [2] pixelshuffle x2 8x8": (64, 2, (2,), (1, 3, 8, 8), "pixelshuffle", 2, "1conv", 48, 6),
    "C60 [2] batch of two pixelshuffle x2 19x26": (60, 6, (2,), (2, 3, 19, 26), "pixelshuffle", 2, "1conv", 512, 7),
}
_CASES = {}


def fixture_sd(name):
    C, nH, depths, shape, ups, s, resi, cpb, seed = FIXTURES[name]
    return fill(shape[1], C, depths, nH, 2.0, s, ups, resi, cpb, seed)


def case(name):
    """(state dict, input, float64 result, storage-model result) of a fixture, computed once per process and left unchanged."""
    if name not in _CASES:
        C, nH, depths, shape, ups, s, resi, cpb, seed = FIXTURES[name]
        sd = fixture_sd(name)
        x = torch.from_numpy(synth.uniform(shape, 7 + seed))
        _CASES[name] = (sd, x, forward64(sd, x, s, ups), forward_storage(sd, x, s, ups))
    return _CASES[name]
