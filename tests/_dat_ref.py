"""Functional references of the pieces of a DAT block (Chen et al. 2023, "Dual Aggregation Transformer for Image Super-Resolution"), written from the definition of the
published dat_arch.py and not from engine code: every function works in the dtype it is given (float64 for the reference, float32 for a model's error estimate).

The window attention follows the published order of operations -- zero-pad q, k, v behind the Linear, roll, partition into the branch's windows, softmax(q k^T + B + M) v,
reverse, roll back, crop -- and builds the mask the published way (a label image, its window partition, pairwise differences), so that it checks the kernel's coordinate
formula instead of repeating it.
"""
import torch
import torch.nn.functional as F


def padded(H, W, s0, s1):
    m = max(s0, s1)
    return -(-H // m) * m, -(-W // m) * m


def windows(x, wh, ww):
    """[N, C, Hp, Wp] -> [N, nW, wh * ww, C], windows row-major, tokens row-major inside a window."""
    N, C, Hp, Wp = x.shape
    x = x.reshape(N, C, Hp // wh, wh, Wp // ww, ww).permute(0, 2, 4, 3, 5, 1)
    return x.reshape(N, (Hp // wh) * (Wp // ww), wh * ww, C)


def unwindows(w, Hp, Wp, wh, ww):
    """[N, nW, wh * ww, C] -> [N, C, Hp, Wp]."""
    N, _, _, C = w.shape
    x = w.reshape(N, Hp // wh, Wp // ww, wh, ww, C).permute(0, 5, 1, 3, 2, 4)
    return x.reshape(N, C, Hp, Wp)


def shift_mask(Hp, Wp, wh, ww, shy, shx):
    """[nW, T, T]: 0, or -100 between tokens of different regions of the rolled frame (calculate_mask of the published code)."""
    img = torch.zeros(1, 1, Hp, Wp)
    cnt = 0
    for hs in (slice(0, -wh), slice(-wh, -shy), slice(-shy, None)):
        for ws in (slice(0, -ww), slice(-ww, -shx), slice(-shx, None)):
            img[:, :, hs, ws] = cnt
            cnt += 1
    lab = windows(img, wh, ww)[0, :, :, 0]                                    # [nW, T]
    diff = lab[:, None, :] - lab[:, :, None]
    return torch.where(diff != 0, torch.tensor(-100.0), torch.tensor(0.0))


def branch_geometry(br, s0, s1, shifted):
    wh, ww = (s0, s1) if br == 0 else (s1, s0)
    return wh, ww, (wh // 2 if shifted else 0), (ww // 2 if shifted else 0)


def pad_keys(H, W, s0, s1, br, shifted):
    """[nW, T] bool: the tokens of every window of branch br whose stored pixel lies outside H x W."""
    Hp, Wp = padded(H, W, s0, s1)
    wh, ww, shy, shx = branch_geometry(br, s0, s1, shifted)
    inside = torch.zeros(1, 1, Hp, Wp)
    inside[:, :, :H, :W] = 1
    if shifted:
        inside = torch.roll(inside, (-shy, -shx), (2, 3))
    return windows(inside, wh, ww)[0, :, :, 0] == 0


def rect_attention(qkv, table, s0, s1, shifted, dt, model=False):
    """qkv: [3, N, nH, d, H, W] (q already scaled); table: [nH, T, T].  Returns ([N, nH, d, H, W] in dt, max |score|).
    model: the kernel's declared arithmetic -- the keys walked in blocks of 64 with a running maximum m and sum l, P rounded to fp16 in front of P v."""
    _, N, nH, d, H, W = qkv.shape
    Hp, Wp = padded(H, W, s0, s1)
    T = s0 * s1
    x = F.pad(qkv.to(dt).reshape(3 * N, nH * d, H, W), (0, Wp - W, 0, Hp - H)).reshape(3, N, nH, d, Hp, Wp)
    outs, smax = [], 0.0
    for br in (0, 1):
        wh, ww, shy, shx = branch_geometry(br, s0, s1, shifted)
        hs = slice(0, nH // 2) if br == 0 else slice(nH // 2, nH)
        nb = nH // 2
        xb = x[:, :, hs].reshape(3, N, nb * d, Hp, Wp)
        if shifted:
            xb = torch.roll(xb, (-shy, -shx), (3, 4))
        heads = lambda w: w.reshape(N, -1, T, nb, d).permute(0, 1, 3, 2, 4)          # [N, nW, T, C] -> [N, nW, nb, T, d]
        q, k, v = (heads(windows(xb[i], wh, ww)) for i in range(3))
        S = q @ k.transpose(-1, -2) + table[hs].to(dt)
        if shifted:
            S = S + shift_mask(Hp, Wp, wh, ww, shy, shx).to(dt)[None, :, None]
        smax = max(smax, float(S.abs().max()))
        if model:
            m = torch.full(S.shape[:-1] + (1,), -3.0e38, dtype=dt)
            l = torch.zeros_like(m)
            o = torch.zeros(S.shape[:-1] + (d,), dtype=dt)
            for b in range(0, T, 64):
                sb = S[..., b:b + 64]
                mn = torch.maximum(m, sb.amax(-1, keepdim=True))
                alpha = torch.exp(m - mn)
                e = torch.exp(sb - mn)
                l = l * alpha + e.sum(-1, keepdim=True)
                o = o * alpha + e.half().to(dt) @ v[..., b:b + 64, :]
                m = mn
            o = o / l
        else:
            o = torch.softmax(S, -1) @ v
        o = unwindows(o.permute(0, 1, 3, 2, 4).reshape(N, -1, T, nb * d), Hp, Wp, wh, ww)
        if shifted:
            o = torch.roll(o, (shy, shx), (2, 3))
        outs.append(o[:, :, :H, :W].reshape(N, nb, d, H, W))
    return torch.cat(outs, 1), smax


def channel_scores(q, k, temperature, dt):
    """q, k: [N, nH, d, H, W]; temperature [nH].  Returns (G [N, nH, d, d], sq [N, nH, d], sk, A [N, nH, d, d]) in dt: F.normalize over the pixels, q k^T, times the
    temperature, softmax over the last index."""
    N, nH, d = q.shape[:3]
    qf, kf = q.to(dt).reshape(N, nH, d, -1), k.to(dt).reshape(N, nH, d, -1)
    G = qf @ kf.transpose(-1, -2)
    sq, sk = (qf * qf).sum(-1), (kf * kf).sum(-1)
    qn = qf / torch.sqrt(sq).clamp_min(1e-12)[..., None]
    kn = kf / torch.sqrt(sk).clamp_min(1e-12)[..., None]
    A = torch.softmax((qn @ kn.transpose(-1, -2)) * temperature.to(dt)[None, :, None, None], -1)
    return G, sq, sk, A


def channel_apply(A, v):
    """A [N, nH, d, d], v [N, nH, d, H, W] -> [N, nH, d, H, W]."""
    N, nH, d, H, W = v.shape
    return (A @ v.to(A.dtype).reshape(N, nH, d, -1)).reshape(N, nH, d, H, W)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def dwconv(x, taps, bias):
    """x [N, C, H, W], taps [C, 3, 3], bias [C]: depthwise, zero padding."""
    return F.conv2d(x, taps[:, None].to(x.dtype), bias.to(x.dtype), padding=1, groups=x.shape[1])


def fold_bn(w, b, bn_w, bn_b, mean, var, eps=1e-5):
    """BatchNorm (eval) behind a conv / Linear with output channels on axis 0, folded into its weight and bias (float64)."""
    g = bn_w.double() / torch.sqrt(var.double() + eps)
    return w.double() * g.reshape(-1, *([1] * (w.dim() - 1))), (b.double() - mean.double()) * g + bn_b.double()


def excite_gelu(pooled, w1, b1, w2, b2):
    """pooled [N, C] -> sigmoid(W2 GELU(W1 pooled + b1) + b2) [N, C]."""
    dt = pooled.dtype
    return torch.sigmoid(gelu(pooled @ w1.to(dt).T + b1.to(dt)) @ w2.to(dt).T + b2.to(dt))


def spatial_gate(x, w1, b1, w2, b2):
    """x [N, C, H, W] -> sigmoid(w2 . GELU(W1 x + b1) + b2) [N, 1, H, W]."""
    dt = x.dtype
    h = gelu(torch.einsum("jc,nchw->njhw", w1.to(dt), x) + b1.to(dt)[None, :, None, None])
    return torch.sigmoid(torch.einsum("j,njhw->nhw", w2.to(dt), h) + b2)[:, None]


def aim_mix(x, y, gate, w1, b1, w2, b2):
    """out = X * gate[channel] + Y * s[pixel]: X the branch gated per channel (gate [N, C]), Y the one gated per pixel by spatial_gate(X)."""
    return x * gate.to(x.dtype)[:, :, None, None] + y * spatial_gate(x, w1, b1, w2, b2)


def layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(1, keepdim=True)
    var = x.var(1, unbiased=False, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g.to(x.dtype)[None, :, None, None] + b.to(x.dtype)[None, :, None, None]


# ------------------------------------------------------------------------------------------------ the whole network
# A functional forward of DAT written from the definition (include/innfer_amd.h, innfer_dat_create), in float64; next to it the fp16 storage model of the same forward:
# the same arithmetic with a rounding to fp16 wherever the engine stores a slab, the weights of the matrix-core convs rounded once (after the load-time folds, which the
# model repeats in float32 / float64 as the shell does).
import numpy as np                                      # noqa: E402

from innfer_amd import synth                            # noqa: E402
from innfer_amd.architectures.keys import dat_shapes    # noqa: E402

MEAN = (0.4488, 0.4371, 0.4040)
QK_GAIN, LAST_GAIN = 4.0, 0.25


def fill(in_chans=3, C=180, depths=(6,) * 6, nH=6, ef=4.0, s=4, upsampler="pixelshuffle", resi="1conv", seed=0):
    """{key: float32 torch tensor}: conv / Linear weights uniform +-sqrt(3 / fan_in) (the q and k rows of every qkv times QK_GAIN, so that softmax rows are far from uniform;
    proj and fc2 times 0.5; the interaction convs times 3, so that both gates spread over (0, 1); conv_last times LAST_GAIN); LayerNorm / BatchNorm weights in [0.5, 1.5],
    their biases +-0.2; running_mean +-0.25, running_var in [0.5, 1.5); temperature in [0.5, 3) with the last head negative; other biases +-0.1."""
    sd = {}
    shapes = dat_shapes(in_chans, C, depths, nH, ef, s, upsampler, resi)
    for key, shp in shapes.items():
        ks = synth.key_seed(key, seed)
        if key.endswith("num_batches_tracked"):
            sd[key] = torch.zeros((), dtype=torch.long)
            continue
        if key.endswith("temperature"):
            v = synth.uniform(shp, ks, 0.5, 3.0)
            v[-1] = -v[-1]
        elif key.endswith("running_mean"):
            v = synth.uniform(shp, ks, -0.25, 0.25)
        elif key.endswith("running_var"):
            v = synth.uniform(shp, ks, 0.5, 1.5)
        elif key.endswith("weight") and len(shp) >= 2:
            b = float(np.sqrt(3.0 / np.prod(shp[1:])))
            v = synth.uniform(shp, ks, -b, b)
            if key.endswith("qkv.weight"):
                v[:2 * C] *= np.float32(QK_GAIN)
            if key.endswith("proj.weight") or key.endswith("ffn.fc2.weight"):
                v = v * np.float32(0.5)
            if "_interaction." in key:
                v = v * np.float32(3.0)
            if key == "conv_last.weight":
                v = v * np.float32(LAST_GAIN)
        elif key.endswith("weight"):                   # LayerNorm / BatchNorm
            v = synth.uniform(shp, ks, 0.5, 1.5)
        elif "norm" in key or key[:-5] + ".running_mean" in shapes or (".pos." in key and key.endswith(".0.bias")):          # the biases of LayerNorm / BatchNorm
            v = synth.uniform(shp, ks, -0.2, 0.2)
        else:
            v = synth.uniform(shp, ks, -0.1, 0.1)
        sd[key] = torch.from_numpy(np.ascontiguousarray(v, np.float32))
    return sd


def depths_of(sd):
    depths = []
    while f"layers.{len(depths)}.blocks.0.norm1.weight" in sd:
        j = 0
        while f"layers.{len(depths)}.blocks.{j}.norm1.weight" in sd:
            j += 1
        depths.append(j)
    return depths


def published_shift(i, b):
    return (i % 2 == 0 and b > 0 and (b - 2) % 4 == 0) or (i % 2 != 0 and b % 4 == 0)


def pos_bias(sd, prefix, wh, ww):
    """[nH / 2, T, T] float64 from the DynamicPosBias MLP: rel = the integer offsets, dy-major; B[h][i][j] = pos(rel)[(ri - rj + wh - 1)(2 ww - 1) + (ci - cj + ww - 1)][h]."""
    dt = torch.float64
    f = lambda k: sd[prefix + k].to(dt)
    rel = torch.tensor([[dy, dx] for dy in range(1 - wh, wh) for dx in range(1 - ww, ww)], dtype=dt)
    x = rel @ f("pos_proj.weight").T + f("pos_proj.bias")
    for m in ("pos1", "pos2", "pos3"):
        x = F.layer_norm(x, (x.shape[-1],), f(m + ".0.weight"), f(m + ".0.bias"), 1e-5)
        x = F.relu(x) @ f(m + ".2.weight").T + f(m + ".2.bias")
    T = wh * ww
    out = torch.empty(x.shape[1], T, T, dtype=dt)
    for i in range(T):
        ri, ci = divmod(i, ww)
        rj, cj = torch.arange(T) // ww, torch.arange(T) % ww
        out[:, i, :] = x[(ri - rj + wh - 1) * (2 * ww - 1) + (ci - cj + ww - 1)].T
    return out


def _bn_eval(t, sd, k):
    dt = t.dtype
    f = lambda n: sd[k + n].to(dt)
    sh = (1, -1) + (1,) * (t.dim() - 2)
    return (t - f(".running_mean").reshape(sh)) / torch.sqrt(f(".running_var").reshape(sh) + 1e-5) * f(".weight").reshape(sh) + f(".bias").reshape(sh)


def _forward(sd, x, s, split, storage, shifted=None):
    dt = torch.float64
    r16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t)
    w16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t.to(dt))
    W = lambda k: w16(sd[k + ".weight"])
    Bv = lambda k: sd[k + ".bias"].to(dt)
    P = lambda k: sd[k].to(dt)
    norm = lambda k, t: r16(layer_norm(t, P(k + ".weight"), P(k + ".bias")))
    lin = lambda w, b, t: F.conv2d(t, w[:, :, None, None] if w.dim() == 2 else w, b, padding=(w.shape[-1] // 2 if w.dim() == 4 else 0))
    N, cin, H, Wd = x.shape
    C = sd["conv_first.weight"].shape[0]
    nH = 2 * sd["layers.0.blocks.0.attn.attns.0.pos.pos3.2.weight"].shape[0]
    d, s0, s1 = C // nH, split[0], split[1]
    hid = sd["layers.0.blocks.0.ffn.fc1.weight"].shape[0]
    mean32 = torch.tensor(MEAN if cin == 3 else (0.0,) * cin, dtype=torch.float32)
    mean = mean32.to(dt)[None, :, None, None]
    direct = "conv_last.weight" not in sd
    x = r16(r16(x.to(dt)) - mean)
    f0 = r16(F.conv2d(x, sd["conv_first.weight"].to(dt), Bv("conv_first"), padding=1))          # (storage: the first conv keeps its fp32 weights)

    def resi(k, t, short):
        if k + ".weight" in sd:
            return r16(lin(W(k), Bv(k), t) + short)
        a = r16(F.leaky_relu(lin(W(k + ".0"), Bv(k + ".0"), t), 0.2))
        a = r16(F.leaky_relu(lin(W(k + ".2"), Bv(k + ".2"), a), 0.2))
        return r16(lin(W(k + ".4"), Bv(k + ".4"), a) + short)

    def heads(t):                                       # [N, C, H, W] -> [N, nH, d, H, W]
        return t.reshape(N, nH, d, H, Wd)

    t = norm("before_RG.1", f0)
    for i, depth in enumerate(depths_of(sd)):
        short = t
        for j in range(depth):
            b = f"layers.{i}.blocks.{j}."
            u = norm(b + "norm1", t)
            wq, bq = sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"]
            if j % 2 == 0:
                if storage:                             # d^-0.5 folded into the q rows in float32, then the one rounding of the weights
                    sc = torch.ones(3 * C, dtype=torch.float32)
                    sc[:C] = float(np.float32(d ** -0.5))
                    qkv = r16(lin((wq * sc[:, None]).half().to(dt), (bq * sc).to(dt), u))
                else:
                    qkv = lin(wq.to(dt), bq.to(dt), u)
                    qkv = torch.cat([qkv[:, :C] * d ** -0.5, qkv[:, C:]], 1)
                table = torch.cat([pos_bias(sd, b + "attn.attns.0.pos.", s0, s1), pos_bias(sd, b + "attn.attns.1.pos.", s1, s0)])
                if storage:
                    table = table.float().to(dt)
                sh = published_shift(i, j) if shifted is None else (i, j) in shifted
                q3 = torch.stack([heads(qkv[:, :C]), heads(qkv[:, C:2 * C]), heads(qkv[:, 2 * C:])])
                if storage:
                    a = r16(_rect_storage(q3, table, s0, s1, sh, r16))
                else:
                    a = rect_attention(q3, table, s0, s1, int(sh), dt)[0]
                a = a.reshape(N, C, H, Wd)
            else:
                qkv = r16(lin(W(b + "attn.qkv"), bq.to(dt), u))
                q, k, v = heads(qkv[:, :C]), heads(qkv[:, C:2 * C]), heads(qkv[:, 2 * C:])
                A = channel_scores(q, k, P(b + "attn.temperature").reshape(nH), dt)[3]
                a = r16(channel_apply(A.float().to(dt) if storage else A, v)).reshape(N, C, H, Wd)
            v_img = qkv[:, 2 * C:]
            if storage:                                 # BatchNorm folded in float64, the result used as float32 parameters
                tw, tb = fold_bn(P(b + "attn.dwconv.0.weight").reshape(C, 3, 3), P(b + "attn.dwconv.0.bias"), P(b + "attn.dwconv.1.weight"), P(b + "attn.dwconv.1.bias"),
                                 P(b + "attn.dwconv.1.running_mean"), P(b + "attn.dwconv.1.running_var"))
                c = r16(gelu(dwconv(v_img, tw.float().to(dt), tb.float().to(dt))))
            else:
                c = gelu(_bn_eval(dwconv(v_img, P(b + "attn.dwconv.0.weight").reshape(C, 3, 3), P(b + "attn.dwconv.0.bias")), sd, b + "attn.dwconv.1"))
            X, Y = (a, c) if j % 2 == 0 else (c, a)
            ci, si = b + "attn.channel_interaction.", b + "attn.spatial_interaction."
            pooled = Y.mean((2, 3), keepdim=True)
            cm = lin(P(ci + "4.weight"), P(ci + "4.bias"), gelu(_bn_eval(lin(P(ci + "1.weight"), P(ci + "1.bias"), pooled), sd, ci + "2")))
            sm = lin(P(si + "3.weight"), P(si + "3.bias"), gelu(_bn_eval(lin(P(si + "0.weight"), P(si + "0.bias"), X), sd, si + "1")))
            mixed = r16(X * torch.sigmoid(cm) + Y * torch.sigmoid(sm))
            t = r16(lin(W(b + "attn.proj"), Bv(b + "attn.proj"), mixed) + t)
            h = r16(gelu(lin(W(b + "ffn.fc1"), Bv(b + "ffn.fc1"), norm(b + "norm2", t))))
            x1, x2 = h[:, :hid // 2], h[:, hid // 2:]
            g = dwconv(r16(layer_norm(x2, P(b + "ffn.sg.norm.weight"), P(b + "ffn.sg.norm.bias"))), P(b + "ffn.sg.conv.weight").reshape(hid // 2, 3, 3), P(b + "ffn.sg.conv.bias"))
            t = r16(lin(W(b + "ffn.fc2"), Bv(b + "ffn.fc2"), r16(x1 * g)) + t)
        t = resi(f"layers.{i}.conv", t, short)
    f = resi("conv_after_body", norm("norm", t), f0)
    if direct:
        bias = (sd["upsample.0.bias"] + mean32.repeat_interleave(s * s)).to(dt) if storage else Bv("upsample.0")
        y = F.pixel_shuffle(r16(lin(W("upsample.0"), bias, f)), s)
        return y if storage else y + mean
    y = r16(F.leaky_relu(lin(W("conv_before_upsample.0"), Bv("conv_before_upsample.0"), f), 0.01))
    for k in sorted(k[:-7] for k in sd if k.startswith("upsample.") and k.endswith(".weight")):
        y = F.pixel_shuffle(r16(lin(W(k), Bv(k), y)), 3 if s == 3 else 2)
    y = r16(lin(W("conv_last"), (sd["conv_last.bias"] + mean32).to(dt) if storage else Bv("conv_last"), y))
    return y if storage else y + mean


def _rect_storage(q3, table, s0, s1, sh, r16):
    """rect_attention with P rounded to fp16 in front of P v (the one rounding inside the kernel that the storage model keeps); the caller rounds the result."""
    dt = torch.float64
    _, N, nH, d, H, W = q3.shape
    Hp, Wp = padded(H, W, s0, s1)
    T = s0 * s1
    x = F.pad(q3.reshape(3 * N, nH * d, H, W), (0, Wp - W, 0, Hp - H)).reshape(3, N, nH, d, Hp, Wp)
    outs = []
    for br in (0, 1):
        wh, ww, shy, shx = branch_geometry(br, s0, s1, sh)
        hs = slice(0, nH // 2) if br == 0 else slice(nH // 2, nH)
        nb = nH // 2
        xb = x[:, :, hs].reshape(3, N, nb * d, Hp, Wp)
        if sh:
            xb = torch.roll(xb, (-shy, -shx), (3, 4))
        hd = lambda w: w.reshape(N, -1, T, nb, d).permute(0, 1, 3, 2, 4)
        q, k, v = (hd(windows(xb[i], wh, ww)) for i in range(3))
        S = q @ k.transpose(-1, -2) + table[hs]
        if sh:
            S = S + shift_mask(Hp, Wp, wh, ww, shy, shx).to(dt)[None, :, None]
        e = torch.exp(S - S.amax(-1, keepdim=True))
        o = (r16(e) @ v) / e.sum(-1, keepdim=True)
        o = unwindows(o.permute(0, 1, 3, 2, 4).reshape(N, -1, T, nb * d), Hp, Wp, wh, ww)
        if sh:
            o = torch.roll(o, (shy, shx), (2, 3))
        outs.append(o[:, :, :H, :W].reshape(N, nb, d, H, W))
    return torch.cat(outs, 1)


def forward64(sd, x, s, split, shifted=None):
    return _forward(sd, x, s, split, False, shifted)


def forward_storage(sd, x, s, split, shifted=None):
    return _forward(sd, x, s, split, True, shifted)


def codes(y):
    """tensor2np's uint8 codes of a planar result (clip(255 y), round half to even), channel order left alone."""
    return torch.round((255.0 * y.double()).clamp(0, 255)).to(torch.int16)


def codes_within_one(y, ref):
    return float(((codes(y) - codes(ref)).abs() <= 1).double().mean())


# The network fixtures: (C, nH, split, depths, expansion_factor, upsampler, resi_connection, scale, input shape, seed); the input is synth.uniform(shape, 7 + seed).
FIXTURES = {
    "C60 nH6 [8,16] [3,2] 3conv direct x2 20x44": (60, 6, (8, 16), (3, 2), 2.0, "pixelshuffledirect", "3conv", 2, (1, 3, 20, 44), 1),
    "C180 nH6 [8,32] [2] x4 40x72": (180, 6, (8, 32), (2,), 2.0, "pixelshuffle", "1conv", 4, (1, 3, 40, 72), 2),
    "C64 nH2 [8,16] [4] ef4 x3 batch of two 19x26": (64, 2, (8, 16), (4,), 4.0, "pixelshuffle", "1conv", 3, (2, 3, 19, 26), 3),
}
_CASES = {}


def fixture_sd(name):
    C, nH, split, depths, ef, ups, resi, s, shape, seed = FIXTURES[name]
    return fill(shape[1], C, depths, nH, ef, s, ups, resi, seed)


def case(name):
    """(state dict, input, float64 result, storage-model result) of a fixture, computed once per process and left unchanged."""
    if name not in _CASES:
        C, nH, split, depths, ef, ups, resi, s, shape, seed = FIXTURES[name]
        sd = fixture_sd(name)
        x = torch.from_numpy(synth.uniform(shape, 7 + seed))
        _CASES[name] = (sd, x, forward64(sd, x, s, split), forward_storage(sd, x, s, split))
    return _CASES[name]
