"""References of SPAN (Swift Parameter-free Attention Network) for tests/test_span_host.py and tests/test_gpu_span.py (CPU only: torch and numpy, no library call).

The network (the reference project has no such architecture; this is its definition):

    Conv3XC(ci, co, gain=2): sk = Conv2d(ci, co, 1), conv.0 = Conv2d(ci, ci gain, 1), conv.1 = Conv2d(ci gain, co gain, 3, padding=0), conv.2 = Conv2d(co gain, co, 1),
    eval_conv = Conv2d(ci, co, 3, padding=1), all with bias.  In eval mode it is ONE 3x3 zero-pad-1 conv, recomputed from sk and conv.* (`collapse`):
        W[o,i,y,x] = sum_{m,j} conv.2.w[o,m] conv.1.w[m,j,y,x] conv.0.w[j,i];   W[o,i,1,1] += sk.w[o,i]
        b[o]       = sum_m conv.2.w[o,m] (sum_{j,y,x} conv.1.w[m,j,y,x] conv.0.b[j] + conv.1.b[m]) + conv.2.b[o] + sk.b[o]
    the stored eval_conv.* is NOT the source of truth (`fill` puts noise there); a `deploy` dict has only eval_conv.* and those are used as given.

    SPAB(c): out1 = c1_r(x); out2 = c2_r(SiLU(out1)); out3 = c3_r(SiLU(out2)); out = (out3 + x) * (sigmoid(out3) - 0.5); returns (out, out1)      # out1 PRE-activation
    SPAN:    x = (x - mean) * img_range (only when norm; per channel, never added back); f0 = conv_1(x); b1 .. b5 = block_1 .. block_5;
             (b6, b5_2) = block_6(b5); out = PixelShuffle(s)(upsampler.0(conv_cat(cat[f0, conv_2(b6), b1, b5_2])))

forward64: that graph in float64 on the weights as given.
forward_storage: the "fp16 storage model" -- the same graph in float64 with the collapsed weights rounded to fp32 and then fp16 (bias fp32, as the engine keeps it), where
the input, the input map's result and every launch's stored output are each rounded to fp16: f0; per SPAB SiLU(out1), SiLU(out2), the gated result (block_6: out1 raw,
then SiLU of the ROUNDED out1 -- that activation is a pass of its own there); conv_2, conv_cat and upsampler.0's results.  Its distance from forward64 is what fp16 storage
costs a case; the engine differs from it in the fp32 order of summation and the hardware exponential / reciprocal only.

fill: every Conv3XC part and conv_cat / upsampler.0 from synth.uniform seeded by key, +-sqrt(3 / fan_in) (unit gain per part), biases +-0.1; then
  conv_1: sk and conv.2 (weights and biases) times 1 / 64 -- the (x - mean) * 255 input of range +-140 comes down to O(1) features (norm=False: times 2 instead);
  block convs: sk and conv.2 times G_BLOCK = 1.2, so that out3 spreads over both regimes of the gate although SiLU and the gate (|sigmoid - 0.5| < 0.5) shrink;
  upsampler.0: weight times 0.02 and bias set to 0.5 +- 0.1: the result stays an image.
Shares of out3 values (all six blocks, float64) with |out3| < 2 (unsaturated gate) / |out3| > 4 (saturated), printed by test_span_host.py for the fixtures:
    f 48 x4 32x32 seed 1: 0.39 / 0.33 | f 48 x2 31x33 seed 2: 0.33 / 0.41 | f 52 x3 17x9 seed 3: 0.36 / 0.37 | f 32 x1 8x8 seed 4: 0.48 / 0.22 |
    norm=False f 48 x2 20x24 seed 5: 0.48 / 0.24
(below G_BLOCK 1.0 every block after the first has all of out3 inside +-2; from about 1.3 on the features grow from block to block.)
The storage model alone against float64 on these fixtures: max |err| 5.1e-4 .. 1.2e-3, every uint8 code within +-1.
"""
import numpy as np
import torch
import torch.nn.functional as F

from innfer_amd import synth

MEAN = (0.4488, 0.4371, 0.4040)
G_BLOCK = 1.2


def units():
    return ["conv_1"] + [f"block_{i}.c{j}_r" for i in range(1, 7) for j in range(1, 4)] + ["conv_2"]


def shapes(num_in_ch=3, f=48, upscale=4, norm=True, deploy=False, gain=2):
    """State-dict key -> shape, written out from the definition above (compared with innfer_amd's span_shapes by the host test)."""
    s = {}
    for p in units():
        ci = num_in_ch if p == "conv_1" else f
        if not deploy:
            s[p + ".sk.weight"], s[p + ".sk.bias"] = (f, ci, 1, 1), (f,)
            s[p + ".conv.0.weight"], s[p + ".conv.0.bias"] = (ci * gain, ci, 1, 1), (ci * gain,)
            s[p + ".conv.1.weight"], s[p + ".conv.1.bias"] = (f * gain, ci * gain, 3, 3), (f * gain,)
            s[p + ".conv.2.weight"], s[p + ".conv.2.bias"] = (f, f * gain, 1, 1), (f,)
        s[p + ".eval_conv.weight"], s[p + ".eval_conv.bias"] = (f, ci, 3, 3), (f,)
    s["conv_cat.weight"], s["conv_cat.bias"] = (f, 4 * f, 1, 1), (f,)
    k = num_in_ch * upscale * upscale
    s["upsampler.0.weight"], s["upsampler.0.bias"] = (k, f, 3, 3), (k,)
    if not norm:
        s["no_norm"] = (1,)
    return s


def collapse(sd, p, dt=torch.float64):
    """(W [co, ci, 3, 3], b [co]) of Conv3XC `p` in eval mode: the two formulas above, in dtype dt."""
    g = lambda k: sd[f"{p}.{k}"].to(dt)
    w0, w1, w2 = g("conv.0.weight")[:, :, 0, 0], g("conv.1.weight"), g("conv.2.weight")[:, :, 0, 0]
    W = torch.einsum("om,mjyx,ji->oiyx", w2, w1, w0).clone()
    W[:, :, 1, 1] += g("sk.weight")[:, :, 0, 0]
    b = w2 @ (torch.einsum("mjyx,j->m", w1, g("conv.0.bias")) + g("conv.1.bias")) + g("conv.2.bias") + g("sk.bias")
    return W, b


def training_branch(sd, p, x):
    """Conv3XC's training forward in x's dtype: conv(F.pad(x, 1)) + sk(x) -- the pad is ZEROS in front of conv.0, so the ring carries conv.0.b."""
    g = lambda k: sd[f"{p}.{k}"].to(x.dtype)
    t = F.conv2d(F.pad(x, (1, 1, 1, 1)), g("conv.0.weight"), g("conv.0.bias"))
    t = F.conv2d(t, g("conv.1.weight"), g("conv.1.bias"))
    t = F.conv2d(t, g("conv.2.weight"), g("conv.2.bias"))
    return t + F.conv2d(x, g("sk.weight"), g("sk.bias"))


def fill(num_in_ch=3, f=48, upscale=4, seed=0, norm=True, deploy=False):
    """{key: float32 torch tensor} of the network (see the module docstring for the scales); deploy: the collapsed convs of the same network under eval_conv.*."""
    full = {}
    for k, shp in shapes(num_in_ch, f, upscale, norm, False).items():
        ks = synth.key_seed(k, seed)
        if k == "no_norm":
            v = np.zeros(shp, np.float32)
        elif len(shp) == 4:
            b = float(np.sqrt(3.0 / (shp[1] * shp[2] * shp[3])))
            v = synth.uniform(shp, ks, -b, b)
        else:
            v = synth.uniform(shp, ks, -0.1, 0.1)
        p = k.split(".sk.")[0] if ".sk." in k else k.split(".conv.2.")[0] if ".conv.2." in k else None
        if p == "conv_1":
            v = v * np.float32(1.0 / 64 if norm else 2.0)
        elif p is not None and p.startswith("block_"):
            v = v * np.float32(G_BLOCK)
        if k == "upsampler.0.weight":
            v = v * np.float32(0.02)
        if k == "upsampler.0.bias":
            v = v + np.float32(0.5)
        full[k] = torch.from_numpy(np.ascontiguousarray(v, np.float32))
    if not deploy:
        return full
    out = {}
    for k in shapes(num_in_ch, f, upscale, norm, True):
        if ".eval_conv." in k:
            W, b = collapse(full, k.split(".eval_conv.")[0])
            out[k] = (W if k.endswith("weight") else b).float()
        else:
            out[k] = full[k]
    return out


def _unit(sd, p, storage):
    dt = torch.float64
    if f"{p}.sk.weight" in sd:
        W, b = collapse(sd, p)
        W, b = W.float(), b.float()              # the host's collapse is rounded to fp32 at upload
    else:
        W, b = sd[f"{p}.eval_conv.weight"], sd[f"{p}.eval_conv.bias"]
    if storage:
        W = W.half()
    return W.to(dt), b.to(dt)


def _forward(sd, x, upscale, norm, img_range, mean, storage, stats):
    dt = torch.float64
    r16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t)
    conv = lambda t, p: F.conv2d(t, *_unit(sd, p, storage), padding=1)
    silu = lambda t: t * torch.sigmoid(t)
    x = r16(x.to(dt))
    if norm:
        m = torch.tensor(mean, dtype=torch.float32).to(dt)[None, :, None, None]
        x = r16(x * float(np.float32(img_range)) - (m * float(np.float32(img_range))).float().to(dt)) if storage else (x - torch.tensor(mean, dtype=dt)[None, :, None, None]) * img_range
    f0 = r16(conv(x, "conv_1"))
    t, keep = f0, {}
    for i in range(1, 7):
        o1 = conv(t, f"block_{i}.c1_r")
        if i == 6:
            keep["b5_2"] = r16(o1)
            a1 = r16(silu(keep["b5_2"]))         # a pass of its own on the stored (rounded) value
        else:
            a1 = r16(silu(o1))
        a2 = r16(silu(conv(a1, f"block_{i}.c2_r")))
        o3 = conv(a2, f"block_{i}.c3_r")
        if stats is not None:
            stats.append(o3.abs().flatten())
        t = r16((o3 + t) * (torch.sigmoid(o3) - 0.5))
        if i == 1:
            keep["b1"] = t
    c2 = r16(conv(t, "conv_2"))
    cat = torch.cat([f0, c2, keep["b1"], keep["b5_2"]], 1)
    wc, wu = sd["conv_cat.weight"], sd["upsampler.0.weight"]
    y = r16(F.conv2d(cat, (wc.half() if storage else wc).to(dt), sd["conv_cat.bias"].to(dt)))
    y = r16(F.conv2d(y, (wu.half() if storage else wu).to(dt), sd["upsampler.0.bias"].to(dt), padding=1))
    return F.pixel_shuffle(y, upscale)


def forward64(sd, x, upscale, norm=True, img_range=255.0, mean=MEAN, stats=None):
    return _forward(sd, x, upscale, norm, img_range, mean, False, stats)


def forward_storage(sd, x, upscale, norm=True, img_range=255.0, mean=MEAN):
    return _forward(sd, x, upscale, norm, img_range, mean, True, None)


def gate_shares(sd, x, upscale, norm=True):
    """(share of |out3| < 2, share of |out3| > 4) over the six blocks of the float64 forward."""
    st = []
    forward64(sd, x, upscale, norm, stats=st)
    a = torch.cat(st)
    return float((a < 2).double().mean()), float((a > 4).double().mean())


def codes(y):
    """tensor2np's uint8 codes of a planar result (clip(255 y), round half to even), channel order left alone."""
    return torch.round((255.0 * y.double()).clamp(0, 255)).to(torch.int16)


def codes_within_one(y, ref):
    return float(((codes(y) - codes(ref)).abs() <= 1).double().mean())
