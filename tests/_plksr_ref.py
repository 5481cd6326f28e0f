"""References of RealPLKSR for tests/test_plksr_host.py and tests/test_gpu_plksr.py (CPU only: torch and numpy, no library call).

The network (the reference project has no such architecture; this is its definition):

    DCCM(dim):       Sequential(Conv2d(dim, 2 dim, 3, 1, 1), Mish(), Conv2d(2 dim, dim, 3, 1, 1))
    PLKConv2d(p, k): conv = Conv2d(p, p, k, 1, k // 2);  forward: x[:, :p] = conv(x[:, :p])  (the other channels pass through)
    EA(dim):         f = Sequential(Conv2d(dim, dim, 3, 1, 1), Sigmoid());  forward: x * f(x)
    PLKBlock:        channel_mixer = DCCM(dim); lk = PLKConv2d(int(dim * split_ratio), k); attn = EA(dim) or Identity (use_ea False);
                     refine = Conv2d(dim, dim, 1); norm = GroupNorm(norm_groups, dim)       (eps 1e-5, biased variance, per sample over (dim / groups) x H x W)
                     forward: norm(refine(attn(lk(channel_mixer(x))))) + x
    RealPLKSR(in_ch 3, out_ch 3, dim 64, n_blocks 28, upscaling_factor 4, kernel_size 17, split_ratio 0.25, use_ea True, norm_groups 4):
                     feats = Sequential(Conv2d(in_ch, dim, 3, 1, 1), n_blocks x PLKBlock, Dropout2d (no parameters), Conv2d(dim, out_ch s^2, 3, 1, 1))
                     forward: PixelShuffle(s)(feats(x) + repeat_interleave(x, s^2, dim=1))
    Mish(f) = f * tanh(softplus(f)) = f * (n^2 + 2 n) / (n^2 + 2 n + 2),  n = exp(f)

forward64: that graph in float64 on the weights as given.
forward_storage: the "fp16 storage model" -- the same graph in float64 with the conv weights rounded to fp16 (biases and the GroupNorm affine stay fp32, as the engine keeps
them), where the input and every launch's stored output are each rounded to fp16: feats.0; Mish(conv); the second DCCM conv; the PLK result on its 16 channels; the gated
result; refine; norm + skip; the last conv; the sum with the repeated input.  Its distance from forward64 is what fp16 storage costs a case; the engine differs from it in
the fp32 order of summation, the fp32 statistics and the hardware exponential / reciprocal only.

fill: every conv weight uniform +-sqrt(3 / fan_in) seeded by synth.key_seed(key, seed); channel_mixer.0 and attn.f.0 weights times 2; norm.weight uniform in [0.25, 0.75];
every bias and norm.bias +-0.1; the last conv's weight times 0.05; the input is synth.uniform in [0, 1).
With this fill (dim 64, k 17) the storage model alone is 8.1e-4 (3 blocks x4 32x32), 7.0e-4 (2 blocks x2 21x37), 6.9e-4 (2 blocks x3 9x17) and 2.2e-3 (28 blocks x4 24x24)
from float64, every uint8 code within +-1; the results span about -0.2 .. 1.2 (both clips of the uint8 store are exercised); about half of the Mish arguments lie inside
+-1 and 1 - 4 % below -3; 67 - 85 % of the gate arguments lie inside +-2 and up to 7 % beyond +-4 (tests/test_plksr_host.py prints the figures of every fixture).
"""
import numpy as np
import torch
import torch.nn.functional as F

from innfer_amd import synth


def shapes(in_ch=3, dim=64, n_blocks=28, scale=4, k=17, use_ea=True, p=16):
    """State-dict key -> shape, written out from the definition above (compared with innfer_amd's realplksr_shapes by the host test)."""
    s = {"feats.0.weight": (dim, in_ch, 3, 3), "feats.0.bias": (dim,)}
    for i in range(1, n_blocks + 1):
        b = f"feats.{i}."
        s[b + "channel_mixer.0.weight"], s[b + "channel_mixer.0.bias"] = (2 * dim, dim, 3, 3), (2 * dim,)
        s[b + "channel_mixer.2.weight"], s[b + "channel_mixer.2.bias"] = (dim, 2 * dim, 3, 3), (dim,)
        s[b + "lk.conv.weight"], s[b + "lk.conv.bias"] = (p, p, k, k), (p,)
        if use_ea:
            s[b + "attn.f.0.weight"], s[b + "attn.f.0.bias"] = (dim, dim, 3, 3), (dim,)
        s[b + "refine.weight"], s[b + "refine.bias"] = (dim, dim, 1, 1), (dim,)
        s[b + "norm.weight"], s[b + "norm.bias"] = (dim,), (dim,)
    kk = in_ch * scale * scale
    s[f"feats.{n_blocks + 2}.weight"], s[f"feats.{n_blocks + 2}.bias"] = (kk, dim, 3, 3), (kk,)
    return s


def fill(in_ch=3, dim=64, n_blocks=28, scale=4, k=17, use_ea=True, seed=0, p=16):
    """{key: float32 torch tensor} of the network (see the module docstring for the scales)."""
    sd = {}
    last = f"feats.{n_blocks + 2}.weight"
    for key, shp in shapes(in_ch, dim, n_blocks, scale, k, use_ea, p).items():
        ks = synth.key_seed(key, seed)
        if len(shp) == 4:
            b = float(np.sqrt(3.0 / (shp[1] * shp[2] * shp[3])))
            v = synth.uniform(shp, ks, -b, b)
            if key.endswith("channel_mixer.0.weight") or key.endswith("attn.f.0.weight"):
                v = v * np.float32(2.0)
            if key == last:
                v = v * np.float32(0.05)
        elif key.endswith("norm.weight"):
            v = synth.uniform(shp, ks, 0.25, 0.75)
        else:
            v = synth.uniform(shp, ks, -0.1, 0.1)
        sd[key] = torch.from_numpy(np.ascontiguousarray(v, np.float32))
    return sd


def mish(t):
    return t * torch.tanh(F.softplus(t))


def _forward(sd, x, scale, groups, storage, stats):
    dt = torch.float64
    r16 = (lambda t: t.half().to(dt)) if storage else (lambda t: t)
    w = lambda k: (sd[k + ".weight"].half() if storage else sd[k + ".weight"]).to(dt)
    b = lambda k: sd[k + ".bias"].to(dt)
    n_blocks = 0
    while f"feats.{n_blocks + 1}.channel_mixer.0.weight" in sd:
        n_blocks += 1
    x = r16(x.to(dt))
    t = r16(F.conv2d(x, w("feats.0"), b("feats.0"), padding=1))
    for i in range(1, n_blocks + 1):
        p = f"feats.{i}."
        f = F.conv2d(t, w(p + "channel_mixer.0"), b(p + "channel_mixer.0"), padding=1)
        if stats is not None:
            stats.setdefault("mish", []).append(f.flatten())
        u = r16(F.conv2d(r16(mish(f)), w(p + "channel_mixer.2"), b(p + "channel_mixer.2"), padding=1))
        wl = w(p + "lk.conv")
        pc, k = wl.shape[0], wl.shape[-1]
        u = torch.cat([r16(F.conv2d(u[:, :pc], wl, b(p + "lk.conv"), padding=k // 2)), u[:, pc:]], 1)
        if p + "attn.f.0.weight" in sd:
            g = F.conv2d(u, w(p + "attn.f.0"), b(p + "attn.f.0"), padding=1)
            if stats is not None:
                stats.setdefault("gate", []).append(g.flatten())
            u = r16(u * torch.sigmoid(g))
        u = r16(F.conv2d(u, w(p + "refine"), b(p + "refine")))
        t = r16(F.group_norm(u, groups, sd[p + "norm.weight"].to(dt), sd[p + "norm.bias"].to(dt), eps=1e-5) + t)
    last = f"feats.{n_blocks + 2}"
    y = r16(F.conv2d(t, w(last), b(last), padding=1))
    y = r16(y + torch.repeat_interleave(x, scale * scale, dim=1))
    return F.pixel_shuffle(y, scale)


def forward64(sd, x, scale, groups=4, stats=None):
    return _forward(sd, x, scale, groups, False, stats)


def forward_storage(sd, x, scale, groups=4):
    return _forward(sd, x, scale, groups, True, None)


def argument_shares(sd, x, scale, groups=4):
    """{'mish': (share of |f| < 1, share of f < -3), 'gate': (share of |g| < 2, share of |g| > 4) or None} over all blocks of the float64 forward."""
    st = {}
    forward64(sd, x, scale, groups, stats=st)
    m = torch.cat(st["mish"])
    out = {"mish": (float((m.abs() < 1).double().mean()), float((m < -3).double().mean())), "gate": None}
    if "gate" in st:
        g = torch.cat(st["gate"]).abs()
        out["gate"] = (float((g < 2).double().mean()), float((g > 4).double().mean()))
    return out


def codes(y):
    """tensor2np's uint8 codes of a planar result (clip(255 y), round half to even), channel order left alone."""
    return torch.round((255.0 * y.double()).clamp(0, 255)).to(torch.int16)


def codes_within_one(y, ref):
    return float(((codes(y) - codes(ref)).abs() <= 1).double().mean())


# The network fixtures of both test files: (n_blocks, scale, input shape, kernel_size, use_ea, seed); the input is synth.uniform(shape, 7 + seed).
FIXTURES = {
    "3 blocks x4 32x32": (3, 4, (1, 3, 32, 32), 17, True, 1),
    "2 blocks x2 21x37": (2, 2, (1, 3, 21, 37), 17, True, 2),
    "2 blocks x3 9x17": (2, 3, (1, 3, 9, 17), 17, True, 3),
    "2 blocks x1 8x8": (2, 1, (1, 3, 8, 8), 17, True, 4),
    "S (k 13, no EA) x2 20x24": (2, 2, (1, 3, 20, 24), 13, False, 5),
    "batch of two x2 19x26": (2, 2, (2, 3, 19, 26), 17, True, 6),
    "28 blocks x4 24x24": (28, 4, (1, 3, 24, 24), 17, True, 7),
}
_CASES = {}


def case(name):
    """(state dict, input, float64 result, storage-model result) of a fixture, computed once per process and left unchanged."""
    if name not in _CASES:
        nb, s, shape, k, ea, seed = FIXTURES[name]
        sd = fill(3, 64, nb, s, k, ea, seed)
        x = torch.from_numpy(synth.uniform(shape, 7 + seed))
        _CASES[name] = (sd, x, forward64(sd, x, s), forward_storage(sd, x, s))
    return _CASES[name]
