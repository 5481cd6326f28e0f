"""float64 references and the one bound of tests/test_gpu_conv_forms.py (CPU only: torch and numpy, no library call).

The bound, for every element of a result the kernel stores as fp16:

    |got - ref| <= ulp16(max(|ref|, |got|)) / 2 + 8 * e32 + extra

  ulp16(v) = 2^(floor(log2 max(|v|, 2^-14)) - 10): the storage rounding, derived.
  e32      = max over the case of |F.conv2d in float32 on the CPU - the float64 reference| on the same fp16 operands, before the activation: what fp32 accumulation costs
             this case, measured against the reference and never against the kernel.
  8        = the margin docs/KERNELS.md gives an emulation figure (the device sums in another order).
  extra    = roundings / approximations the kernel makes on purpose, derived where they are used (TRANS per hardware tanh / sigmoid; the self gate's rounded v).

A result the kernel stores as fp32 has no storage rounding: its bound is 8 * e32 + extra (rounding=False).  That tightening is this file's own, and it is applied
only where the case has at least FEW values: e32 is a maximum over the case, and over a few dozen values (a 1 x 1 or 4 x 4 image) it understates what fp32
accumulation costs the operation -- the device reached 0.75 of 8 e32 on a 4 x 4 image against 0.34 on every case of >= 4096 values.  Smaller cases keep the bound
as it stands above.

References are plain torch in float64 on the fp16-rounded operands.  Two forms feed fp16 somewhere inside and the reference mirrors exactly that rounding:
  prefix_lrelu: the operand of input group g is fp16(max(s, 0.2f * s)), s = the fp32 running sum of groups 0 .. g (inputs are multiples of 2^-10, so s is exact);
  up-conv phases: Wt = fp16(float32 sum of the taps that meet the same source pixel) (up2x_phase_weights, compared bit for bit with the packer on the CPU).
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from innfer_amd import synth

# One hardware tanh / sigmoid (common.h fast_tanh / fast_sigmoid: v_exp_f32 and v_rcp_f32 are 1-ulp instructions; the argument scaling adds <= (|2x| + 1) 2^-24
# relative on e = exp(2x), and d/de of 1 - 2 / (1 + e) is 2 / (1 + e)^2 with e / (1 + e)^2 <= 1/4; with the final subtraction below 4.8e-7): 2^-21 absolute.
TRANS = 2.0 ** -21

FEW = 4096
MEASURED = {}          # family -> [largest e32, worst err / bound], filled by assert_within_fp16_rounding


def ulp16(v):
    m, e = torch.frexp(v.detach().abs().double().clamp_min(2.0 ** -14))      # v = m 2^e, m in [0.5, 1): floor(log2 v) = e - 1
    return torch.exp2((e - 11).double())


def assert_within_fp16_rounding(got, ref64, e32, extra=0, what="", family=None, rounding=True):
    """Every element of `got` within one fp16 rounding (+ 8 e32 + extra) of ref64; returns the worst err / bound."""
    got, ref64 = got.double(), ref64.double()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    bound = 8.0 * e32 + extra + (ulp16(torch.maximum(got.abs(), ref64.abs())) / 2 if rounding else 0.0)
    ratio = (got - ref64).abs() / bound
    worst = ratio.max().item() if ratio.numel() else 0.0
    if family is not None:
        m = MEASURED.setdefault(family, [0.0, 0.0])
        m[0], m[1] = max(m[0], e32), max(m[1], worst)
    print(f"[conv-forms] {family or '-'} | {what}: e32 {e32:.2e} worst err/bound {worst:.3f}")
    if not worst <= 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{what}: e32 {e32:.3e}, worst err / bound {worst:.3f} at {tuple(int(j) for j in i)}: got {got[i].item():.8g} ref {ref64[i].item():.8g} "
                             f"bound {(bound[i].item() if torch.is_tensor(bound) else bound):.3e}; {(ratio > 1).sum().item()} of {ratio.numel()} elements beyond the bound")
    return worst


# ------------------------------------------------------------------------------------------------ slabs
def to_slab(x, groups=None, fill=7.0):
    """[N, C, H, W] (C % 32 == 0) -> the blocked NHWC slab [groups, N, H, W, 32]; groups beyond C / 32 hold `fill`."""
    N, Cc, H, W = x.shape
    g = Cc // 32
    s = x.reshape(N, g, 32, H, W).permute(1, 0, 3, 4, 2).contiguous()
    if groups and groups > g:
        s = torch.cat([s, torch.full((groups - g, N, H, W, 32), fill, dtype=x.dtype)])
    return s


def from_slab(s):
    G, N, H, W, _ = s.shape
    return s.permute(1, 0, 4, 2, 3).reshape(N, G * 32, H, W)


# ------------------------------------------------------------------------------------------------ cases and their data
@dataclass(frozen=True)
class Case:
    form: str           # 3x3 | 1x1 | 7x7 | phases (ConvTranspose2d(4, 2, 1), planar) | upph (nearest 2x + 3x3 as four phases) | s2k4 | t2x | 7x1 | dil | shuffle
    N: int
    C: int
    K: int
    H: int              # the kernel's grid (3x3 with up: the upsampled size; phases / upph / t2x: the INPUT grid; s2k4: the OUTPUT grid)
    W: int
    seed: int = 0
    reflect: int = 0
    up: int = 0
    in_relu: int = 0
    prefix: int = 0     # 1x1: the running-sum operand
    k: int = 4          # t2x: kernel size 3 | 4
    dil: int = 1
    blo: float = -1.0   # biases uniform in [blo, 1)

    def __str__(self):
        f = "".join(f" {n}" for n in ("reflect", "up", "in_relu", "prefix") if getattr(self, n)) + (f" d{self.dil}" if self.dil > 1 else "")
        return f"{self.form} {self.C}->{self.K} {self.N}x{self.H}x{self.W}{f}"


TAPS = {"3x3": 9, "1x1": 1, "7x7": 49, "phases": 4, "upph": 9, "s2k4": 16, "t2x": 4, "7x1": 7, "dil": 9, "shuffle": 9}


@functools.lru_cache(maxsize=4)
def data(c):
    """x fp16 [N, C, Hs, Ws]; w float32 in the layout the form's packer takes (the values the kernel multiplies are fp16(w)); b float32 [K]."""
    s = 100 * c.seed
    Hs, Ws = (c.H // 2, c.W // 2) if c.up else (2 * c.H, 2 * c.W) if c.form == "s2k4" else (c.H, c.W)
    if c.prefix:            # multiples of 2^-10 in (-1, 1): the running sums over up to eight groups are exact in fp32 in any order
        x = torch.from_numpy(np.floor(synth.uniform((c.N, c.C, Hs, Ws), s + 1, -1023, 1024)) / 1024.0).half()
    else:
        x = torch.from_numpy(synth.uniform((c.N, c.C, Hs, Ws), s + 1, -1, 1)).half()
    shape = {"3x3": (c.K, c.C, 3, 3), "1x1": (c.K, c.C), "7x7": (c.K, c.C, 7, 7), "phases": (c.C, c.K, 4, 4), "upph": (c.K, c.C, 3, 3), "s2k4": (c.K, c.C, 4, 4),
             "t2x": (c.C, c.K, c.k, c.k), "7x1": (c.K, c.C, 7), "dil": (c.K, c.C, 3, 3), "shuffle": (c.K, c.C, 3, 3)}[c.form]
    taps = (c.k * c.k / 4.0) if c.form == "t2x" else TAPS[c.form]
    w = torch.from_numpy(synth.uniform(shape, s + 2, -1, 1) / np.float32(np.sqrt(taps * c.C)))
    b = torch.from_numpy(synth.uniform((c.K,), s + 3, c.blo, 1))
    return x, w, b


def up2x_phase_weights(w):
    """conv_pack_up2x_phases' fold, in its order of summation: w float32 [K][C][3][3] -> float32 [C][K][4][4], the ConvTranspose2d(4, 2, 1) that equals
    conv3x3(nearest2x(x)): kernel row ky collects the 3x3 rows 3: {0}, 1: {1, 2}, 2: {0, 1}, 0: {2}, columns alike."""
    R = ((2,), (1, 2), (0, 1), (0,))
    K, Cc = w.shape[:2]
    w = w.float()
    wt = torch.zeros(Cc, K, 4, 4, dtype=torch.float32)
    for ky in range(4):
        for kx in range(4):
            a = torch.zeros(K, Cc, dtype=torch.float32)
            for i in R[ky]:
                for j in R[kx]:
                    a = a + w[:, :, i, j]
            wt[:, :, ky, kx] = a.t()
    return wt


def phase_conv3x3_weights(wt):
    """ConvTranspose2d(4, 2, 1) weights [C][K][4][4] -> the ONE 3x3 conv of 4 K phase-major channels over the input grid (innfer_conv_args.planar_phases): channel
    (2a + b) K + c at tap (dy, dx) in {-1, 0, 1}^2 is wt[ci][c][ky][kx], ky = 1 (dy 0) / 3 (dy -1) for a = 0 and 0 (dy +1) / 2 (dy 0) for a = 1 (oy = 2 iy - 1 + ky)."""
    Cc, K = wt.shape[:2]

    def kof(a, d):
        return {0: 1, -1: 3}.get(d, -1) if a == 0 else {1: 0, 0: 2}.get(d, -1)
    w3 = torch.zeros(4 * K, Cc, 3, 3, dtype=wt.dtype)
    for ph in range(4):
        for t in range(9):
            ky, kx = kof(ph >> 1, t // 3 - 1), kof(ph & 1, t % 3 - 1)
            if ky >= 0 and kx >= 0:
                w3[ph * K:(ph + 1) * K, :, t // 3, t % 3] = wt[:, :, ky, kx].t()
    return w3


def operand(c, dt):
    """The tensor the kernel multiplies, as dtype dt."""
    x, _, _ = data(c)
    if c.prefix:
        G = c.C // 32
        run = torch.cumsum(x.float().reshape(c.N, G, 32, *x.shape[2:]), 1)                     # exact: multiples of 2^-10 below 8
        x = torch.maximum(run, torch.tensor(0.2, dtype=torch.float32) * run).half().reshape(x.shape)   # the loader's fmaxf(run, 0.2f * run), rounded to fp16
    x = x.to(dt)
    if c.in_relu:
        x = F.relu(x)
    if c.up:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return x


def conv(c, dt, w=None):
    """conv + bias of the case in dtype dt, on the fp16-rounded operands (w: other weights of the same layout, already rounded as the caller wants them)."""
    _, w0, b = data(c)
    w = (w0.half() if w is None else w).to(dt)
    x, b = operand(c, dt), b.to(dt)
    if c.form in ("3x3", "shuffle"):
        if c.reflect:
            x = F.pad(x, (1, 1, 1, 1), mode="reflect" if c.reflect == 1 else "replicate")
        return F.conv2d(x, w, b, padding=0 if c.reflect else 1)
    if c.form == "dil":
        return F.conv2d(x, w, b, padding=c.dil, dilation=c.dil)
    if c.form == "1x1":
        return F.conv2d(x, w[:, :, None, None], b)
    if c.form == "7x7":
        if c.reflect:
            x = F.pad(x, (3, 3, 3, 3), mode="reflect")
        return F.conv2d(x, w, b, padding=0 if c.reflect else 3)
    if c.form == "7x1":
        if c.reflect:
            x = F.pad(x, (0, 0, 3, 3), mode="reflect")
        return F.conv2d(x, w[:, :, :, None], b, padding=(0 if c.reflect else 3, 0))
    if c.form == "phases":
        return F.conv_transpose2d(x, w, b, stride=2, padding=1)
    if c.form == "t2x":
        return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1 if c.k == 3 else 0)
    if c.form == "upph":        # w here: the folded transposed-conv weights [C][K][4][4]
        return F.conv_transpose2d(x, w, b, stride=2, padding=1)
    if c.form == "s2k4":
        return F.conv2d(x, w, b, stride=2, padding=1)
    raise ValueError(c.form)


@functools.lru_cache(maxsize=4)
def pre(c):
    """(float64 conv + bias, e32) of the case, computed once and shared by every epilogue of it."""
    w = None
    if c.form == "upph":
        w = up2x_phase_weights(data(c)[1]).half()
    y64 = conv(c, torch.float64, w)
    e32 = (conv(c, torch.float32, w).double() - y64).abs().max().item()
    return y64, e32


def epilogue(y, act=0, outm=0, res1=None, s1=1.0, res2=None, s2=1.0):
    """The kernels' epilogue in y's dtype; returns (result, number of hardware tanh / sigmoid evaluations per value)."""
    n = 0
    if act in (4, 5):
        y = res1.to(y.dtype) * torch.sigmoid(y)
        n += 1
        return (F.leaky_relu(y, 0.2) if act == 4 else y), n
    if act == 1:
        y = F.leaky_relu(y, 0.2)
    elif act == 2:
        y = F.relu(y)
    elif act == 3:
        y, n = torch.tanh(y), n + 1
    elif act == 6:
        y, n = torch.sigmoid(y), n + 1
    if outm == 1:
        y, n = (torch.tanh(y) + 1) / 2, n + 1
    elif outm == 2:
        y, n = torch.tanh(y), n + 1
    elif outm == 3:
        y, n = torch.sigmoid(y), n + 1
    elif outm == 4:
        y = y.clamp(0, 1)
    if res1 is not None:
        y = y * s1 + res1.to(y.dtype)
    if res2 is not None:
        y = y * s2 + res2.to(y.dtype)
    return y, n


def residual(c, which, shape):
    return torch.from_numpy(synth.uniform(tuple(shape), 100 * c.seed + 10 + which, -1, 1)).half()


def gate_params(c):
    """The self gate's 32 x 32 matrix (float32; the kernel multiplies fp16(Wg)) and bias."""
    wg = torch.from_numpy(synth.uniform((32, 32), 100 * c.seed + 20, -1, 1) / np.float32(np.sqrt(32.0)))
    bg = torch.from_numpy(synth.uniform((32,), 100 * c.seed + 21, -1, 1))
    return wg, bg


def self_gate(c, y, e32, act):
    """out = act(v sigmoid(Wg v + bg)) with v = y kept in y's dtype, and -- for float64 y -- the allowance for the kernel's v = fp16(y): with eps_j = ulp16(v_j) / 2 + 8 e32
    the gate argument moves by at most sum_j |W_kj| eps_j, sigmoid' <= 1/4, so the output by at most eps_k + |v_k| / 4 * sum_j |W_kj| eps_j (act has slope <= 1);
    the hardware sigmoid adds TRANS |v_k|."""
    wg, bg = gate_params(c)
    W = wg.half().to(y.dtype)
    g = torch.einsum("kj,njhw->nkhw", W, y) + bg.to(y.dtype)[None, :, None, None]
    out = y * torch.sigmoid(g)
    out = F.leaky_relu(out, 0.2) if act == 1 else F.relu(out) if act == 2 else out
    eps = ulp16(y) / 2 + 8 * e32
    extra = eps + y.abs().double() / 4 * torch.einsum("kj,njhw->nkhw", W.abs().double(), eps) + TRANS * y.abs().double()
    return out, extra


# ------------------------------------------------------------------------------------------------ the uint8 image (tensor2np as the conv's epilogue)
def image_codes(y, denorm, round16):
    """tensor2np, step by step, on a planar [N, K, H, W] result: [round to fp16 (the fp16 forward's output dtype),] denormalise (v + 1) / 2 clipped to [0, 1],
    (255 v) clipped to [0, 255], rounded half to even, RGB -> BGR for 3 / 4 channels, HWC.  Returns (uint8 [N, H, W, K], float64 255 v before the rounding, same layout)."""
    v = y.half().to(y.dtype) if round16 else y
    u = y
    if denorm:
        v, u = ((v + 1) / 2).clamp(0, 1), ((u + 1) / 2).clamp(0, 1)
    v, u = (255 * v).clamp(0, 255), (255 * u).clamp(0, 255)
    K = y.shape[1]
    order = [2, 1, 0] + ([3] if K == 4 else []) if K >= 3 else list(range(K))
    codes = torch.round(v)[:, order].permute(0, 2, 3, 1).contiguous().to(torch.uint8)
    return codes, u.double()[:, order].permute(0, 2, 3, 1).contiguous(), y.double()[:, order].permute(0, 2, 3, 1).contiguous()


def assert_image_codes(got, y64, e32, denorm, round16, what="", family=None, cap=0.01):
    """Codes equal, except a difference of one code where the float64 value 255 v lies within 255 (ulp16 / 2 [only with round16: without it nothing is rounded to fp16]
    + 8 e32) [halved by the denormalisation] of a rounding boundary; at most `cap` of the values excused.  Returns the excused share."""
    ref, u, y = image_codes(y64, denorm, round16)
    assert got.shape == ref.shape and got.dtype == torch.uint8, (what, got.shape, ref.shape)
    d = got.to(torch.int16) - ref.to(torch.int16)
    win = 255.0 * ((ulp16(y) / 2 if round16 else 0.0) + 8 * e32) * (0.5 if denorm else 1.0)
    near = ((u - torch.floor(u)) - 0.5).abs() <= win
    bad = (d != 0) & ~((d.abs() == 1) & near)
    share = (d != 0).double().mean().item()
    if family is not None:
        m = MEASURED.setdefault(family, [0.0, 0.0])
        m[0], m[1] = max(m[0], e32), max(m[1], share / cap)
    print(f"[conv-forms] {family or '-'} | {what}: e32 {e32:.2e} codes differing {share:.5f} (cap {cap})")
    if bad.any() or share > cap:
        i = np.unravel_index(int(bad.double().argmax()), bad.shape)
        raise AssertionError(f"{what}: e32 {e32:.3e}; {int(bad.sum())} codes differ away from a rounding boundary (first at {tuple(int(j) for j in i)}: got {int(got[i])} "
                             f"ref {int(ref[i])}, 255 v = {u[i].item():.6f}), share of differing codes {share:.5f} (cap {cap})")
    return share
