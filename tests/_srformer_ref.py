"""References of SRFormer for tests/test_srformer_host.py and tests/test_gpu_srformer.py (CPU only: torch and numpy, no library call).  The network is the one
include/innfer_amd.h writes down (SwinIR's skeleton, tests/_swinir_ref.py, around the permuted self-attention and the ConvFFN); nothing here knows of slabs or groups.

    psa(q, k, v, table, ws, shift, dt, model):  one attention over planar q [N, C, Hp, Wp] (ALREADY scaled) and k, v [N, C / 4, Hp, Wp] with real rolls, reshapes and
        permutes; model = the declared arithmetic (P rounded to fp16 in front of P v, the sum over the unrounded values).
    forward(.., storage): the graph in float64 on the weights as given / with the engine's folds (in float64, then the one rounding) and fp16 storage of the input
        and of every launch's result, as tests/_swinir_ref.py's; the depthwise launch stores fp16(h + GELU(dw(h))).
    fill: tests/_swinir_ref.py's scales; the q and k rows times QK_GAIN[ws] (so that max |q k^T| >= 4 on every fixture: tests/test_srformer_host.py checks it)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _swinir_ref as SR
from innfer_amd import synth
from innfer_amd.architectures.keys import srformer_shapes

QK_GAIN = 3.0


def fill(in_chans=3, C=180, depths=(6,) * 6, nH=6, mlp_ratio=2.0, s=4, upsampler="pixelshuffle", resi="1conv", ws=22, seed=0):
    sd = {}
    last = "upsample.0.weight" if upsampler == "pixelshuffledirect" else "conv_last.weight"
    for key, shp in srformer_shapes(in_chans, C, depths, nH, mlp_ratio, s, upsampler, resi, ws).items():
        ks = synth.key_seed(key, seed)
        if key.endswith("relative_position_bias_table"):
            v = synth.uniform(shp, ks, -SR.TABLE, SR.TABLE)
        elif key.endswith("weight") and len(shp) >= 2:
            b = float(np.sqrt(3.0 / np.prod(shp[1:])))
            v = synth.uniform(shp, ks, -b, b)
            if key.endswith("attn.q.weight"):
                v = v * np.float32(QK_GAIN)
            if key.endswith("attn.kv.weight"):
                v[:C // 4] *= np.float32(QK_GAIN)
            if key.endswith("attn.proj.weight") or key.endswith("mlp.fc2.weight"):
                v = v * np.float32(0.5)
            if key == last:
                v = v * np.float32(SR.LAST_GAIN[upsampler])
        elif key.endswith("weight"):
            v = synth.uniform(shp, ks, 0.5, 1.5)
        elif ".norm" in key or key.startswith("norm."):
            v = synth.uniform(shp, ks, -0.2, 0.2)
        else:
            v = synth.uniform(shp, ks, -0.1, 0.1)
        sd[key] = torch.from_numpy(np.ascontiguousarray(v, np.float32))
    return sd


def aligned_index(ws):
    pw = ws // 2
    r, c = torch.arange(ws * ws) // ws // 2, torch.arange(ws * ws) % ws // 2
    py, px = torch.arange(pw * pw) // pw, torch.arange(pw * pw) % pw
    return (r[:, None] - py[None, :] + pw - 1) * (2 * pw - 1) + (c[:, None] - px[None, :] + pw - 1)


def buffers(sd, ws):
    out = {}
    for k in sd:
        if k.endswith("attn.relative_position_bias_table"):
            b = k[:-len("attn.relative_position_bias_table")]
            out[b + "attn.aligned_relative_position_index"] = aligned_index(ws)
            if int(b.split(".")[-2]) % 2:
                out[b + "attn_mask"] = torch.zeros(4, ws * ws, ws * ws // 4)
    return out


def _win(u, ws):
    """[N, C, H, W] -> [N, nW, ws^2, C]"""
    N, C, H, W = u.shape
    return u.reshape(N, C, H // ws, ws, W // ws, ws).permute(0, 2, 4, 3, 5, 1).reshape(N, -1, ws * ws, C)


def shift_mask(Hp, Wp, ws):
    """[nW, ws^2, pw^2] float64: -100 where the label of the query (the rolled frame, slices (0, -ws), (-ws, -ws / 2), (-ws / 2, end)) differs from the label of the key
    (the half-resolution grid, slices (0, -pw), (-pw, -(pw // 2)), (-(pw // 2), end))."""
    pw = ws // 2

    def labels(H, W, win, sh):
        img, cnt = torch.zeros(1, 1, H, W, dtype=torch.float64), 0
        for hs in (slice(0, -win), slice(-win, -sh), slice(-sh, None)):
            for wsl in (slice(0, -win), slice(-win, -sh), slice(-sh, None)):
                img[:, :, hs, wsl] = cnt
                cnt += 1
        return _win(img, win)[0, :, :, 0]
    lq, lk = labels(Hp, Wp, ws, ws // 2), labels(Hp // 2, Wp // 2, pw, pw // 2)
    return torch.where(lq[:, :, None] != lk[:, None, :], -100.0, 0.0).double()


def psa(q, k, v, table, ws, shift, dt=torch.float64, model=False):
    """softmax(q k^T + B + M) v per window and head through the roll; q [N, C, Hp, Wp] scaled, k and v [N, C / 4, Hp, Wp], table [(2 pw - 1)^2, nH].  Returns ([N, C, Hp, Wp], max |q k^T|)."""
    N, C, Hp, Wp = q.shape
    nH, pw = table.shape[1], ws // 2
    d = C // nH
    q, k, v = (torch.roll(t.to(dt), (-shift, -shift), (2, 3)) if shift else t.to(dt) for t in (q, k, v))
    qw = _win(q, ws).reshape(N, -1, ws * ws, nH, d).permute(0, 1, 3, 2, 4)                       # [N, nW, nH, n, d]

    def keys(t):          # [N, C / 4, Hp, Wp] -> [N, nW, nH, pw^2, d]: (py, 2, px, 2, C / 4) -> (py, px, s, cc)
        w = _win(t, ws).reshape(N, -1, pw, 2, pw, 2, C // 4).permute(0, 1, 2, 4, 3, 5, 6).reshape(N, -1, pw * pw, nH, d)
        return w.permute(0, 1, 3, 2, 4)
    kw, vw = keys(k), keys(v)
    QK = qw @ kw.transpose(-1, -2)
    S = QK + table.to(dt)[aligned_index(ws).reshape(-1)].reshape(ws * ws, pw * pw, nH).permute(2, 0, 1)
    if shift:
        S = S + shift_mask(Hp, Wp, ws).to(dt)[None, :, None]
    if model:
        e = torch.exp(S - S.amax(-1, keepdim=True))
        o = (e.half().to(dt) @ vw) / e.sum(-1, keepdim=True)
    else:
        o = torch.softmax(S, -1) @ vw
    o = o.permute(0, 1, 3, 2, 4).reshape(N, Hp // ws, Wp // ws, ws, ws, C).permute(0, 5, 1, 3, 2, 4).reshape(N, C, Hp, Wp)
    if shift:
        o = torch.roll(o, (shift, shift), (2, 3))
    return o, float(QK.abs().max())


def dwconv5(h, w, b, dt=torch.float64):
    """h + GELU(depthwise 5 x 5 (h) + b): h [N, C, H, W], w [C, 1, 5, 5]"""
    h = h.to(dt)
    return h + F.gelu(F.conv2d(h, w.to(dt), b.to(dt), padding=2, groups=h.shape[1]))


def forward(sd, x, s, upsampler, ws, storage, stats=None):
    """storage False: the graph in float64 on the weights as given; True: the fp16 storage model."""
    dt = torch.float64
    r16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t)
    w16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t.to(dt))
    W = lambda k: w16(sd[k + ".weight"])
    Bv = lambda k: sd[k + ".bias"].to(dt)
    norm = lambda k, t: r16(SR.layer_norm(t, sd[k + ".weight"].to(dt), sd[k + ".bias"].to(dt)))
    lin = lambda w, b, t: F.conv2d(t, w[:, :, None, None] if w.dim() == 2 else w, b, padding=(w.shape[-1] // 2 if w.dim() == 4 else 0))
    N, cin, H, Wd = x.shape
    C = sd["conv_first.weight"].shape[0]
    nH = sd["layers.0.residual_group.blocks.0.attn.relative_position_bias_table"].shape[1]
    d = C // nH
    mean32 = torch.tensor(SR.MEAN if cin == 3 else (0.0,) * cin, dtype=torch.float32)
    mean = mean32.to(dt)[None, :, None, None]
    Hp, Wp = -(-H // ws) * ws, -(-Wd // ws) * ws
    x = r16(x.to(dt))
    x = F.pad(x, (0, Wp - Wd, 0, Hp - H), mode="reflect")
    x = r16(x - mean)
    f0 = r16(F.conv2d(x, sd["conv_first.weight"].to(dt), Bv("conv_first"), padding=1))

    def resi(k, t, short):
        if k + ".0.weight" in sd:
            a = r16(F.leaky_relu(lin(W(k + ".0"), Bv(k + ".0"), t), 0.2))
            a = r16(F.leaky_relu(lin(W(k + ".2"), Bv(k + ".2"), a), 0.2))
            return r16(lin(W(k + ".4"), Bv(k + ".4"), a) + short)
        return r16(lin(W(k), Bv(k), t) + short)

    t = norm("patch_embed.norm", f0)
    for i, depth in enumerate(SR.depths_of(sd)):
        short = t
        for j in range(depth):
            b = f"layers.{i}.residual_group.blocks.{j}."
            u = norm(b + "norm1", t)
            sc = d ** -0.5
            wq, bq = sd[b + "attn.q.weight"].to(dt) * sc, sd[b + "attn.q.bias"].to(dt) * sc          # (storage: folded in float64, then the one rounding)
            if storage:
                wq, bq = wq.half().to(dt), bq.float().to(dt)
            q = r16(lin(wq, bq, u))
            kv = r16(lin(W(b + "attn.kv"), Bv(b + "attn.kv"), u))
            o, smax = psa(q, kv[:, :C // 4], kv[:, C // 4:], sd[b + "attn.relative_position_bias_table"], ws, ws // 2 if j % 2 else 0, dt, model=storage)
            if stats is not None:
                stats["smax"] = max(stats.get("smax", 0.0), smax)
            t = r16(lin(W(b + "attn.proj"), Bv(b + "attn.proj"), r16(o)) + t)
            h = r16(F.gelu(lin(W(b + "mlp.fc1"), Bv(b + "mlp.fc1"), norm(b + "norm2", t))))
            z = r16(dwconv5(h, sd[b + "mlp.dwconv.depthwise_conv.0.weight"], sd[b + "mlp.dwconv.depthwise_conv.0.bias"]))
            t = r16(lin(W(b + "mlp.fc2"), Bv(b + "mlp.fc2"), z) + t)
        t = resi(f"layers.{i}.conv", t, short)
    f = resi("conv_after_body", norm("norm", t), f0)
    fold = (lambda k: (sd[k + ".bias"].double() + (mean32.double().repeat_interleave(s * s) if k == "upsample.0" else mean32.double())).float().to(dt)) if storage else Bv
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


# The network fixtures of both test files: (C, nH, depths, window, input shape, upsampler, scale, seed); mlp_ratio 2, '1conv'; the input is synth.uniform(shape, 7 + seed).
FIXTURES = {
    "C60 nH6 [2] ws16 direct x2 13x21": (60, 6, (2,), 16, (1, 3, 13, 21), "pixelshuffledirect", 2, 1),
    "C180 nH6 [2] ws22 pixelshuffle x4 44x66": (180, 6, (2,), 22, (1, 3, 44, 66), "pixelshuffle", 4, 2),
    "C96 nH4 [2] ws24 nearest+conv x4 batch of two 25x30": (96, 4, (2,), 24, (2, 3, 25, 30), "nearest+conv", 4, 3),
}


def fixture_sd(name):
    C, nH, depths, ws, shape, ups, s, seed = FIXTURES[name]
    return fill(shape[1], C, depths, nH, 2.0, s, ups, "1conv", ws, seed)


@functools.lru_cache(None)
def case(name):
    """(state dict, input, float64 result, storage-model result, max |q k^T|) of a fixture, computed once per process and left unchanged."""
    C, nH, depths, ws, shape, ups, s, seed = FIXTURES[name]
    sd, x, st = fixture_sd(name), torch.from_numpy(synth.uniform(shape, 7 + seed)), {}
    return sd, x, forward(sd, x, s, ups, ws, False, st), forward(sd, x, s, ups, ws, True), st["smax"]
