"""One SCPA block of PAN (PAN_arch.py:58-105, oracle/nets.py scpa_trunk) on the CPU (torch and numpy only, no library call): the references, the bounds and the cases
of tests/test_pan_scpa_cpu.py and tests/test_gpu_pan_scpa.py.

    A = lrelu(conv1_a x)   B = lrelu(conv1_b x)   a' = lrelu(k1 * A)   Y = (k3 * B) sigmoid(k2 B + bias)   b' = lrelu(k4 * Y)   out = conv3 [a' | b'] + x

block(x, w, dtype, rounding, fault)   the block by F.conv2d in `dtype`; returns the output BEFORE its storage rounding.
  rounding None     nothing is rounded on the way.
  rounding "fp16"   the declared roundings of pan_scpa_fused / pan_scpa_duo (csrc/pan_scpa.hip): A | B, a', Y and b' are rounded to fp16 where the five-launch schedule
                    stored them; the gate is formed before Y is rounded; sums and the gate in `dtype` (the kernels': fp32).
  rounding "split"  the declared arithmetic of pan_scpa_split (csrc/pan_scpa_split.hip): every tensor and weight a pair hi = fp16(v), lo' = fp16((v - hi) 2^11) 2^-11,
                    a product xh wh + xh wl' + xl' wh (the xl' wl' term is absent: conv(xh + xl', wh + wl') - conv(xl', wl')), the intermediates re-split where the fp16
                    kernel rounds.  Evaluated in float64: the MFMAs' fp32 sums are not modelled (2^-24-sized, inside the margin).
block_f64(c)        float64, nothing rounded, on the fp16-rounded x and the fp16-rounded weights (the k2 bias stays fp32).
figures(c)          per case: model64 = block(float64, "fp16") -- what the fp16 forms are held to --, e_model = max |block(float32, "fp16") - model64| (fp32 accumulation and
                    the rounding flips it causes in the intermediates: rare one-ulp16 flips of A / B / a' / Y / b', which the device makes elsewhere), exact = float64 with
                    the UNROUNDED fp32 weights -- what the split form is held to --, e_split = max |split model (its output pair included) - exact|, and trans.

Bounds, per element, never taken from a kernel (MARGIN = 8: what an emulation figure gets in every "held to float64" file of this project):
    fp16 forms   |got - model64| <= ulp16(max(|got|, |model64|)) / 2 + 8 e_model + trans
    split form   |got - exact|   <= 8 e_split + trans
trans: the gate's sigmoid runs on the hardware exponential and reciprocal (gate8: v_exp_f32 and v_rcp_f32, one ulp each; with the argument scaling 2^-21 absolute on
the sigmoid: tests/_conv_ref.py TRANS).  Y = c sigmoid(g) then moves by <= TRANS max|c|, c = k3 * B.  From Y to the output the map is conv3_b . lrelu . k4 with
|lrelu'| <= 1: an error eps in every Y value moves output channel o by at most eps sum_m |conv3[o][20 + m]| sum_{j, tap} |k4[m][j][tap]|.
trans = TRANS max|c| max_o (that sum) -- the largest |conv3| |k4| column gain of the case, 2e-6 .. 8e-5 here.

Faults (block(..., fault = name)): what tests/test_pan_scpa_cpu.py proves the bounds would see.  FAULTS lists them; fault_acts says where one can act at all.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from _conv_ref import TRANS, ulp16
from innfer_amd import synth

MARGIN = 8.0
NF, HALF = 40, 20
FAMILIES = ("flat", "live")
SHAPES = ((1, 4, 4), (1, 8, 32), (1, 9, 33), (2, 6, 40), (1, 16, 32), (1, 17, 33), (1, 50, 70), (3, 37, 45), (1, 273, 513))
BIG = (1, 273, 513)                                   # 306 tiles of 16 x 32, 595 of 8 x 32: more tiles than workgroups on a 256-CU part -- the next-tile prefetch
C8_SHAPES = ((1, 17, 33), (3, 37, 45), BIG)           # the compact-plane combinations
CPU_SHAPES = ((1, 17, 33), (1, 50, 70), (3, 37, 45))  # where the planted faults are measured
TILE_W, TILE_H = 32, 8                                # seams every 32 columns (every form), every 8 rows (forms 1, 2; form 0: every 16)
FAULTS = ("gate_half", "no_k2_bias", "k1_transposed", "relu_after_k1", "y_ring", "seam_col", "seam_row", "drop_b19", "swap_ab", "c8_stale", "prev_image", "k3c_for_k2")


@dataclass(frozen=True)
class Case:
    family: str
    N: int
    H: int
    W: int

    @property
    def seed(self):
        return 7000 + 97 * self.H + 13 * self.W + self.N + (500 if self.family == "live" else 0)

    def __str__(self):
        return f"{self.family}-{self.N}x{self.H}x{self.W}"


def cases(shapes=SHAPES):
    return [Case(fam, *s) for fam in FAMILIES for s in shapes]


def fault_acts(fault, c):
    """Whether the planted fault can change this case at all."""
    return {"seam_col": c.W > TILE_W, "seam_row": c.H > TILE_H, "prev_image": c.N > 1}.get(fault, True)


# ------------------------------------------------------------------------------------------------ operands
KEYS = ("c1a", "c1b", "k1", "k2", "k2b", "k3", "k4", "c3")
W_SHAPES = {"c1a": (HALF, NF, 1, 1), "c1b": (HALF, NF, 1, 1), "k1": (HALF, HALF, 3, 3), "k2": (HALF, HALF, 1, 1), "k2b": (HALF,), "k3": (HALF, HALF, 3, 3),
            "k4": (HALF, HALF, 3, 3), "c3": (NF, NF, 1, 1)}


@functools.lru_cache(maxsize=None)
def weights(family, seed=0):
    """fp32 torch-layout weights.  flat: +-1 / sqrt(fan_in) as synth.fill_state_dict, the k2 bias +-0.2 -- the networks' weights: the branch is a small correction to
    x and the gate is flat.  live: every conv x 2, k2 x 8, the k2 bias +-2: the gate spans its range and LeakyReLU's negative side carries weight."""
    w = {}
    for i, k in enumerate(KEYS):
        shp = W_SHAPES[k]
        if k == "k2b":
            b = 0.2 if family == "flat" else 2.0
        else:
            b = 1.0 / np.sqrt(shp[1] * shp[2] * shp[3])
            if family == "live":
                b *= 8.0 if k == "k2" else 2.0
        w[k] = torch.from_numpy(synth.uniform(shp, 0x5C9A00 + 16 * seed + i, -b, b))
    assert family in FAMILIES
    return w


def r16(t):
    """Round to fp16 (one rounding from the tensor's own precision), back in the tensor's dtype."""
    return torch.from_numpy(t.numpy().astype(np.float16)).to(t.dtype)


def weights16(family, seed=0):
    """What the fp16 kernels hold: every weight rounded to fp16, the k2 bias fp32."""
    return {k: (v if k == "k2b" else r16(v)) for k, v in weights(family, seed).items()}


@functools.lru_cache(maxsize=None)
def data(c):
    """x [N][40][H][W] float32 on the fp16 grid, uniform in +-1."""
    return r16(torch.from_numpy(synth.uniform((c.N, NF, c.H, c.W), c.seed, -1.0, 1.0)))


# ------------------------------------------------------------------------------------------------ the block
def split_pair(t):
    """t (float64) -> (hi, lo') with hi = fp16(t) and lo' = fp16((t - hi) 2^11) 2^-11, both as float64: the 22 bits the split planes carry."""
    hi = r16(t)
    return hi, r16((t - hi) * 2048.0) / 2048.0


def block(x, w, dtype=torch.float64, rounding=None, fault=None, parts=None):
    """See the head of the file.  x: [N][40][H][W]; w: the dict of weights() / weights16().  parts (a dict) receives c = k3 * B for trans."""
    assert rounding in (None, "fp16", "split") and (fault is None or fault in FAULTS)
    assert rounding != "split" or dtype == torch.float64
    w = {k: v.to(dtype) for k, v in w.items()}
    x = x.to(dtype)
    N, _, H, W = x.shape
    if fault == "prev_image" and N > 1:          # the images stacked into one tall frame: the rows above image n are image n - 1's last rows (no row check per image)
        tall = x.permute(1, 0, 2, 3).reshape(1, NF, N * H, W)
        y = block(tall, w, dtype, rounding, None)
        return y.reshape(NF, N, H, W).permute(1, 0, 2, 3).contiguous()
    if fault == "k1_transposed":
        w["k1"] = w["k1"].transpose(2, 3).contiguous()
    if fault == "no_k2_bias":
        w["k2b"] = torch.zeros_like(w["k2b"])
    if fault == "k3c_for_k2":
        w["k2"] = w["k3"][:, :, 1:2, 1:2].contiguous()
    if rounding == "split":
        ws = {k: (split_pair(v) if k != "k2b" else v) for k, v in w.items()}

        def conv(t, key, pad=0):                 # t: a pair
            (th, tl), (wh, wl) = t, ws[key]
            return F.conv2d(th + tl, wh + wl, None, padding=pad) - F.conv2d(tl, wl, None, padding=pad)
        rnd, val, xin = split_pair, (lambda t: t[0] + t[1]), split_pair(x)
        cat = lambda a, b: (torch.cat([a[0], b[0]], 1), torch.cat([a[1], b[1]], 1))
        zero_ch = lambda t, ch: (t[0].index_fill(1, torch.tensor([ch]), 0.0), t[1].index_fill(1, torch.tensor([ch]), 0.0))
        tmap = lambda f, t: tuple(f(u) for u in t)
    else:
        def conv(t, key, pad=0):
            return F.conv2d(t, w[key], None, padding=pad)
        rnd = r16 if rounding == "fp16" else (lambda t: t)
        val, xin, cat = (lambda t: t), x, (lambda a, b: torch.cat([a, b], 1))
        zero_ch = lambda t, ch: t.index_fill(1, torch.tensor([ch]), 0.0)
        tmap = lambda f, t: f(t)
    lrelu = lambda t: F.leaky_relu(t, 0.2)
    A = rnd(lrelu(conv(xin, "c1a")))
    B = rnd(lrelu(conv(xin, "c1b")))
    k1 = conv(A, "k1", 1)
    ap = rnd(F.relu(k1) if fault == "relu_after_k1" else lrelu(k1))
    ring = fault == "y_ring"                     # Y computed one pixel beyond the image from the zero-padded B and NOT zeroed there: k4 sees k3(B) sigmoid(bias) in its padding
    Bq = tmap(lambda u: F.pad(u, (1, 1, 1, 1)), B) if ring else B
    cc = conv(Bq, "k3", 1)
    g = conv(Bq, "k2") + w["k2b"].reshape(1, -1, 1, 1)
    if parts is not None:
        parts["c"] = cc
    gate = torch.full_like(g, 0.5) if fault == "gate_half" else torch.sigmoid(g)
    Y = rnd(cc * gate)
    k4 = lambda t: conv(t, "k4", 0 if ring else 1)
    if fault == "seam_col":
        bp = torch.cat([k4(tmap(lambda u: u[..., s:s + TILE_W], Y)) for s in range(0, W, TILE_W)], dim=3)
    elif fault == "seam_row":
        bp = torch.cat([k4(tmap(lambda u: u[:, :, s:s + TILE_H], Y)) for s in range(0, H, TILE_H)], dim=2)
    else:
        bp = k4(Y)
    bp = rnd(lrelu(bp))
    if fault == "drop_b19":
        bp = zero_ch(bp, 19)
    out = conv(cat(bp, ap) if fault == "swap_ab" else cat(ap, bp), "c3") + val(xin)
    if fault == "c8_stale":                      # channels 32 .. 39 (the compact plane) keep the block's input
        out = torch.cat([out[:, :32], x[:, 32:]], 1)
    if rounding == "split":
        out = val(split_pair(out))               # the pair the kernel stores, as innfer_pan_split_to_nchw joins it
    return out


def gain(w):
    """max_o sum_m |conv3[o][20 + m]| sum_{j, tap} |k4[m][j][tap]|: how far an error in every Y value can move an output value (head of the file)."""
    k4 = w["k4"].double().abs().sum(dim=(1, 2, 3))
    return float((w["c3"].double().abs()[:, HALF:, 0, 0] @ k4).max())


@functools.lru_cache(maxsize=None)
def figures(c):
    """-> dict(model64, e_model, exact, e_split, trans) of the case (tensors float64, read-only by convention: shared between the tests)."""
    x, w16, w32 = data(c), weights16(c.family), weights(c.family)
    parts = {}
    with torch.no_grad():
        model64 = block(x, w16, torch.float64, "fp16", parts=parts)
        model32 = block(x, w16, torch.float32, "fp16").double()
        exact = block(x, w32, torch.float64, None)
        split = block(x, w32, torch.float64, "split")
    trans = TRANS * float(parts["c"].abs().max()) * gain(w32)
    return dict(model64=model64, model32=model32, e_model=float((model32 - model64).abs().max()), exact=exact, e_split=float((split - exact).abs().max()), trans=trans)


def block_f64(c):
    with torch.no_grad():
        return block(data(c), weights16(c.family), torch.float64, None)


def bound16(c, got, ref=None):
    """The fp16 forms' bound, per element."""
    f = figures(c)
    ref = f["model64"] if ref is None else ref
    return ulp16(torch.maximum(got.abs().double(), ref.abs())) / 2 + MARGIN * f["e_model"] + f["trans"]


def bound_split(c):
    f = figures(c)
    return MARGIN * f["e_split"] + f["trans"]


# ------------------------------------------------------------------------------------------------ the memory layouts (include/innfer_amd.h), in numpy
def to_slab(x, in_c8=False, fill=0.0, rest=np.nan):
    """x [N][40][H][W] -> the two-group fp16 slab as a flat array of 2 npx 32 elements (group stride npx 32).  Two-group form: channels 40 .. 63 hold `fill`.
    Compact form: channels 32 .. 39 at group_stride + p 8, the other 24 npx elements of group 1 hold `rest`."""
    N, _, H, W = x.shape
    npx = N * H * W
    px = np.ascontiguousarray(x.permute(0, 2, 3, 1).reshape(npx, NF).numpy()).astype(np.float16)
    g1 = np.full(npx * 32, rest if in_c8 else fill, dtype=np.float16)
    if in_c8:
        g1[:npx * 8] = px[:, 32:].reshape(-1)
    else:
        g1.reshape(npx, 32)[:, :8] = px[:, 32:]
    return np.concatenate([px[:, :32].reshape(-1), g1])


def from_slab(s, N, H, W, out_c8=False):
    """-> (x [N][40][H][W] fp16 as a torch tensor, the other elements of group 1 as a flat fp16 array)."""
    npx = N * H * W
    g0, g1 = s[:npx * 32].reshape(npx, 32), s[npx * 32:npx * 64]
    if out_c8:
        c8, rest = g1[:npx * 8].reshape(npx, 8), g1[npx * 8:]
    else:
        c8, rest = g1.reshape(npx, 32)[:, :8], g1.reshape(npx, 32)[:, 8:].reshape(-1)
    px = np.concatenate([g0, c8], axis=1)
    return torch.from_numpy(np.ascontiguousarray(px.reshape(N, H, W, NF).transpose(0, 3, 1, 2))), rest


def to_split_planes(x):
    """x [N][40][H][W] float32 -> the split planes as 80 npx fp16 elements: [hi 0..31][hi 32..39][lo 0..31][lo 32..39], lo = fp16((x - hi) 2^11)."""
    N, _, H, W = x.shape
    npx = N * H * W
    px = np.ascontiguousarray(x.permute(0, 2, 3, 1).reshape(npx, NF).numpy()).astype(np.float32)
    hi = px.astype(np.float16)
    lo = ((px.astype(np.float64) - hi.astype(np.float64)) * 2048.0).astype(np.float16)
    return np.concatenate([hi[:, :32].reshape(-1), hi[:, 32:].reshape(-1), lo[:, :32].reshape(-1), lo[:, 32:].reshape(-1)])


def from_split_planes(s, N, H, W):
    """-> hi + 2^-11 lo, [N][40][H][W] float64."""
    npx = N * H * W
    s = s.astype(np.float64)
    hi = np.concatenate([s[:npx * 32].reshape(npx, 32), s[npx * 32:npx * 40].reshape(npx, 8)], axis=1)
    lo = np.concatenate([s[npx * 40:npx * 72].reshape(npx, 32), s[npx * 72:].reshape(npx, 8)], axis=1)
    return torch.from_numpy(np.ascontiguousarray((hi + lo / 2048.0).reshape(N, H, W, NF).transpose(0, 3, 1, 2)))


# ------------------------------------------------------------------------------------------------ the wiring: a PAN whose SCPA blocks show
SCPA_KEYS = {"c1a": "conv1_a.weight", "c1b": "conv1_b.weight", "k1": "k1.0.weight", "k2": "PACnv.k2.weight", "k2b": "PACnv.k2.bias", "k3": "PACnv.k3.weight",
             "k4": "PACnv.k4.weight", "c3": "conv3.weight"}
NET_FAULTS = FAULTS[:10]                              # the table of docs/KERNELS.md 3.5c (prev_image needs a batch, k3c_for_k2 is a single-launch fault)


def scale_scpa(sd, s):
    """Every conv of every SCPA block x s, k2 and its bias x 4 s (x 2 / x 8 is the `live` family)."""
    out = dict(sd)
    for k, v in sd.items():
        if ".PACnv.k2." in k:
            out[k] = v * (4.0 * s)
        elif k.startswith("SCPA_trunk.") and k.endswith(".weight"):
            out[k] = v * s
    return out


def pan_forward(sd, x, nb, fault=None, fp16=False):
    """oracle.pan_forward (nf 40, scale 4, self attention, nearest up-blocks) with the SCPA trunk through block() above, so that a fault can be planted in every
    block; fp16: a restatement with the fp16 engine's roundings -- block(rounding = "fp16") and every other tensor the engine stores as fp16 rounded where it is
    stored.  fault None, fp16 False is oracle.pan_forward itself (asserted in tests/test_pan_scpa_cpu.py)."""
    rnd = r16 if fp16 else (lambda t: t)
    if fp16:
        sd = {k: (r16(v) if v.dim() == 4 else v) for k, v in sd.items()}

    def conv(t, key, pad=0):
        return F.conv2d(t, sd[key + ".weight"], sd.get(key + ".bias"), padding=pad)
    x = rnd(x)
    fea = rnd(conv(x, "conv_first", 1))
    t = fea
    for b in range(nb):
        w = {k: sd[f"SCPA_trunk.{b}.{v}"] for k, v in SCPA_KEYS.items()}
        t = rnd(block(t, w, torch.float32, "fp16" if fp16 else None, fault))
    inp = rnd(fea + conv(t, "trunk_conv", 1))
    xp = F.max_pool2d(inp, 4, 4)
    B, C, h, w_ = xp.shape
    xv = xp.reshape(B, C, h * w_)
    f = F.conv1d(xv, sd["FSA.conv_f.weight"], sd["FSA.conv_f.bias"])
    g = F.conv1d(xv, sd["FSA.conv_g.weight"], sd["FSA.conv_g.bias"])
    hh = F.conv1d(xv, sd["FSA.conv_h.weight"], sd["FSA.conv_h.bias"])
    att = torch.softmax(torch.bmm(f.permute(0, 2, 1), g), dim=-1)
    out = torch.bmm(hh, att.permute(0, 2, 1)).reshape(B, C, h, w_)
    out = F.interpolate(out, size=(inp.shape[2], inp.shape[3]), mode="bicubic", align_corners=False)
    t = rnd(sd["FSA.gamma"] * out + inp)
    for u in range(2):
        i = 5 * u
        t = F.interpolate(t, scale_factor=2.0, mode="nearest")
        t = conv(t, f"upsample.{i + 1}", 1)                           # (the engine forms the gate from the fp32 sums: V is not stored)
        t = rnd(F.leaky_relu(t * torch.sigmoid(conv(rnd(t) if fp16 else t, f"upsample.{i + 2}.conv")), 0.2))
        t = rnd(conv(t, f"upsample.{i + 4}", 1))
    out = conv(t, "conv_last", 1)
    return rnd(out + F.interpolate(x, scale_factor=4.0, mode="bilinear", align_corners=True))


WIRING_SCALE = 2.75          # between x 2 (faults at 1e-3 .. 1e-2: below the fp16 bound) and x 3 (the fp16 restatement itself at 0.9 of the bound); see wiring()
NET_MAX, NET_MEAN, NET_FP32 = 1e-2, 1.5e-3, 1e-4          # the networks' bounds (tests/test_gpu_parity.py, tests/test_gpu_fp32_mode.py)


@functools.lru_cache(maxsize=None)
def wiring():
    """PAN nb = 4, seed 41, 50 x 70, the SCPA convs x WIRING_SCALE (k2 and its bias x 4 more): -> dict(sd, x, ref = oracle.pan_forward, lim = max(1, max|ref|),
    own = max |pan_forward above - ref|, faults = {name: (max, mean) change of the oracle with the fault in every block}, model = (max, mean) distance of the fp16
    restatement from the oracle).  The scale was picked on the CPU from these figures: (a) every fault of NET_FAULTS moves the oracle by >= 3 x the fp16 bound (max
    against 1e-2 lim or mean against 1.5e-3), (b) the restatement stays within a third of both.  x 2.5 fails (a) for y_ring (0.9 x), x 3 fails (b) (0.86)."""
    import oracle
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    net = get_network(get_network_G_config({"type": "pan", "nb": 4}, 4))
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = scale_scpa({k: torch.from_numpy(np.asarray(v)) for k, v in synth.fill_state_dict(shapes, 41).items()}, WIRING_SCALE)
    x = torch.from_numpy(synth.uniform((1, 3, 50, 70), 304))
    with torch.no_grad():
        ref = oracle.pan_forward(sd, x, nb=4, scale=4)
        own = (pan_forward(sd, x, 4) - ref).abs().max().item()
        faults = {}
        for f in NET_FAULTS:
            d = (pan_forward(sd, x, 4, f) - ref).abs()
            faults[f] = (d.max().item(), d.mean().item())
        d = (pan_forward(sd, x, 4, None, True) - ref).abs()
    return dict(sd=sd, x=x, ref=ref, lim=max(1.0, ref.abs().max().item()), own=own, faults=faults, model=(d.max().item(), d.mean().item()))


def assert_wiring_discriminates(wr):
    """Conditions (a) and (b) of wiring(); returns the printable figures."""
    bmax = NET_MAX * wr["lim"]
    assert wr["own"] <= 1e-5, wr["own"]
    lines = [f"fp16 restatement vs oracle: max {wr['model'][0]:.2e} ({wr['model'][0] / bmax:.2f} of the bound) mean {wr['model'][1]:.2e} ({wr['model'][1] / NET_MEAN:.2f})"]
    assert wr["model"][0] <= bmax / 3 and wr["model"][1] <= NET_MEAN / 3, lines[0]
    for f, (mx, mn) in wr["faults"].items():
        lines.append(f"{f} in every block: max {mx:.2e} ({mx / bmax:.1f} x the bound) mean {mn:.2e} ({mn / NET_MEAN:.1f} x)")
        assert max(mx / bmax, mn / NET_MEAN) >= 3.0 and mx >= 3.0 * NET_FP32 * wr["lim"], lines[-1]
    return lines
