"""References of BasicSR's SRVGGNetCompact for tests/test_compact_host.py and tests/test_gpu_compact.py (CPU only: torch and numpy, no library call).

The network (the reference project has no such architecture; this is its definition):

    body.0 = Conv2d(in, nf, 3, 1, 1), body.1 its activation; body.2i / 2i + 1 (i = 1 .. num_conv) Conv2d(nf, nf, 3, 1, 1) and its activation;
    body.<2 num_conv + 2> = Conv2d(nf, out * s^2, 3, 1, 1);     out = PixelShuffle(s)(body(x)) + F.interpolate(x, scale_factor=s, mode='nearest')

forward64: that graph in float64 on the weights as given.
forward_storage: the "fp16 storage model" -- the same graph in float64 with fp16-rounded conv weights (bias and slopes stay fp32, as the engine keeps them), where the
input, every layer's output (after its activation) and the final sum are each rounded to fp16: the roundings an fp16 engine with exact accumulation makes.  Its
distance from forward64 is what fp16 storage costs a case; the engine differs from it only in the fp32 order of summation.
fill: synth.uniform conv weights in +-sqrt(5.5 / fan_in), biases in +-0.1, PReLU slopes in [-0.25, 0.75) (negative, near-zero and positive slopes all occur); the
last conv's weight and bias are multiplied by 0.05, so the result stays an image (about [-0.14, 1.14] for inputs in [0, 1)).
"""
import numpy as np
import torch
import torch.nn.functional as F

from innfer_amd import synth


def shapes(num_in_ch=3, num_feat=64, num_conv=16, upscale=4, act_type="prelu"):
    """State-dict key -> shape, written out from the definition above (compared with innfer_amd's compact_shapes by the host test)."""
    s = {}
    cin = num_in_ch
    for i in range(num_conv + 1):
        s[f"body.{2 * i}.weight"], s[f"body.{2 * i}.bias"] = (num_feat, cin, 3, 3), (num_feat,)
        if act_type == "prelu":
            s[f"body.{2 * i + 1}.weight"] = (num_feat,)
        cin = num_feat
    k = num_in_ch * upscale * upscale
    s[f"body.{2 * num_conv + 2}.weight"], s[f"body.{2 * num_conv + 2}.bias"] = (k, num_feat, 3, 3), (k,)
    return s


def fill(num_in_ch=3, num_feat=64, num_conv=16, upscale=4, seed=0, act_type="prelu"):
    """{key: float32 torch tensor} of the network."""
    sd = {}
    last = f"body.{2 * num_conv + 2}."
    for k, shp in shapes(num_in_ch, num_feat, num_conv, upscale, act_type).items():
        ks = synth.key_seed(k, seed)
        if len(shp) == 4:
            b = float(np.sqrt(5.5 / (shp[1] * 9)))
            v = synth.uniform(shp, ks, -b, b)
        elif k.endswith(".bias"):
            v = synth.uniform(shp, ks, -0.1, 0.1)
        else:
            v = synth.uniform(shp, ks, -0.25, 0.75)
        if k.startswith(last):
            v = v * np.float32(0.05)
        sd[k] = torch.from_numpy(np.ascontiguousarray(v, np.float32))
    return sd


def _slope(sd, i, nf, act_type, dt):
    if act_type == "prelu":
        return sd[f"body.{i}.weight"].to(dt)
    return torch.full((nf,), 0.1 if act_type == "leakyrelu" else 0.0, dtype=dt)


def _forward(sd, x, num_conv, upscale, act_type, storage):
    dt = torch.float64
    r16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t)
    x = r16(x.to(dt))
    t = x
    for i in range(num_conv + 2):
        w, b = sd[f"body.{2 * i}.weight"], sd[f"body.{2 * i}.bias"]
        t = F.conv2d(t, r16(w.to(dt)), b.to(dt), padding=1)
        if i <= num_conv:
            a = _slope(sd, 2 * i + 1, w.shape[0], act_type, dt)
            t = torch.where(t >= 0, t, a[None, :, None, None] * t)
        t = r16(t)
    out = F.pixel_shuffle(t, upscale) + F.interpolate(x, scale_factor=upscale, mode="nearest")
    return r16(out)


def forward64(sd, x, num_conv, upscale, act_type="prelu"):
    return _forward(sd, x, num_conv, upscale, act_type, False)


def forward_storage(sd, x, num_conv, upscale, act_type="prelu"):
    return _forward(sd, x, num_conv, upscale, act_type, True)


def codes(y):
    """tensor2np's uint8 codes of a planar result (clip(255 y), round half to even), channel order left alone."""
    return torch.round((255.0 * y.double()).clamp(0, 255)).to(torch.int16)


def codes_within_one(y, ref):
    return float(((codes(y) - codes(ref)).abs() <= 1).double().mean())


def pad_features(sd, num_conv, nf_to):
    """The same network with num_feat zero-padded to nf_to: zero weights, zero bias, zero slope for the new features -- an exact restatement."""
    out = {}
    last = 2 * num_conv + 2
    for k, v in sd.items():
        i = int(k.split(".")[1])
        if v.dim() == 4:
            K = v.shape[0] if i == last else nf_to
            Cc = v.shape[1] if i == 0 else nf_to
            p = torch.zeros((K, Cc, 3, 3), dtype=v.dtype)
            p[:v.shape[0], :v.shape[1]] = v
        else:
            n = v.shape[0] if (i == last and k.endswith(".bias")) else nf_to
            p = torch.zeros((n,), dtype=v.dtype)
            p[:v.shape[0]] = v
        out[k] = p
    return out
