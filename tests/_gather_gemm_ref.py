"""The gather GEMM's descriptor taken literally, in float64 (CPU only: torch and numpy, no library call), and the cases of tests/test_gpu_gather_gemm.py.

One launch of gg::gemm_gather (csrc/gather_gemm.h, innfer_gather_gemm) means, on the fp16-rounded operands,

    out[n, oy * os + ooy, ox * os + oox, g * g_outoff + co] = sum over t, ci of in[n, oy * stride + dy_t * m, ox * stride + dx_t * m, ci] * w[g][co, ci, t]

  m = 1 + g * g_tapmul (the group's tap multiplier); out-of-image taps are zero, or mirrored with reflect; with up the input is read through nearest 2x;
  g_phase: group g uses its own taps and writes (2 oy + (g >> 1), 2 ox + (g & 1)).

reference() builds it as an index gather plus matmul -- no F.conv2d -- and tests/test_gather_gemm_cpu.py checks it once against F.conv2d / F.conv_transpose2d / F.pad /
F.interpolate for every tap table below that stands for a torch operator.

Two kinds of data:
  exact   inputs and weights are integers in [-8, 8] / 8: products are multiples of 2^-6 and the longest sum of the cases (16 taps x 1024 channels) stays below 2^14,
          so every partial sum in any order is k * 2^-6 with |k| < 2^20 -- representable in fp32 (24 bits): the device must equal float64 BIT FOR BIT.
  random  synth.uniform, weights scaled by 1 / sqrt(taps * cin) as _conv_ref.data does: |got - ref| <= 8 * e32 for cases of >= FEW values (_conv_ref's bound for fp32
          results), e32 = the larger of two distances from float64 on the same operands: float32 F.conv2d on the CPU (the gathered operand as a 1x1 conv), and a
          float32 emulation of the kernel's accumulation order (one [M, 32] x [32, cout] product per k-step added in step order, split segments summed separately
          and added in split order).  Never measured against the kernel.
"""
import functools
from dataclasses import dataclass, field, replace

import numpy as np
import torch
import torch.nn.functional as F

from innfer_amd import synth

FEW = 4096
SENT = -3.0                 # what the raw buffer, its guards and the scratch hold before a launch
IN_GUARD = 1024.0           # the bands around the input slab: read by mistake, they show in every value
PAD_JUNK, GROUP_JUNK = 5.0, 7.0     # the slab's pad channels (cin .. cin_pad: the packer's zero weights cancel them) and the junk group behind the last chunk
MEASURED = {}               # family -> [largest e32, worst err / bound, exact cases]


# ------------------------------------------------------------------------------------------------ tap tables
def taps_conv(kh, kw, ph, pw, dil=1):
    """nn.Conv2d(kernel (kh, kw), padding (ph, pw), dilation dil): tap t = ky * kw + kx reads (oy * stride + ky * dil - ph, ...)."""
    return tuple((ky * dil - ph, kx * dil - pw) for ky in range(kh) for kx in range(kw))


T3 = taps_conv(3, 3, 1, 1)
T3_TF = taps_conv(3, 3, 0, 0)          # stride 2 with tensorflow's `same` on an even input: the pad is one row / column behind the image, offsets 0 .. 2
T4 = taps_conv(4, 4, 1, 1)
T7 = taps_conv(7, 7, 3, 3)
T7x1 = taps_conv(7, 1, 3, 0)
T1 = ((0, 0),)


def convt_phase_taps(k, a, b):
    """nn.ConvTranspose2d(k, stride 2, padding 1): output pixel (2 y + a, 2 x + b) = sum over the kernel rows ky with (a + 1 - ky) even of in[y + (a + 1 - ky) / 2] *
    w[ky] (oy = 2 iy - 1 + ky), columns alike.  Returns [(dy, dx, ky, kx)]."""
    def one(p):
        return [((p + 1 - kk) // 2, kk) for kk in range(k) if (p + 1 - kk) % 2 == 0]
    return [(dy, dx, ky, kx) for dy, ky in one(a) for dx, kx in one(b)]


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    family: str
    N: int
    Hin: int
    Win: int
    cin: int
    cout: int                   # per group
    taps: tuple                 # (dy, dx) per tap; g_phase: the four groups' lists back to back
    Ho: int
    Wo: int
    expect: tuple               # (tile shape, ksplit, seg, taps kept) the case was designed to reach
    stride: int = 1
    os: int = 1
    ooy: int = 0
    oox: int = 0
    up: int = 0
    reflect: int = 0
    ngroup: int = 1
    g_tapmul: int = 0
    g_outoff: int = 0
    g_phase: int = 0
    raw_stride: int = 0         # as passed (0 = cout_pad)
    cout_store: int = 0         # as passed (0 = min(raw_stride, cout_pad))
    raw_off: int = 0            # d_raw points this many floats into the pixel row (other writers' columns in front)
    scratch: str = "none"       # none | ample | short (one byte less than the split needs)
    seed: int = 1

    def __str__(self):
        return self.name

    @property
    def cin_pad(self): return (self.cin + 31) // 32 * 32
    @property
    def cout_pad(self): return (self.cout + 63) // 64 * 64
    @property
    def ntaps(self): return len(self.taps) // 4 if self.g_phase else len(self.taps)
    @property
    def Hfull(self): return self.Ho * self.os
    @property
    def Wfull(self): return self.Wo * self.os
    @property
    def row(self): return self.raw_stride if self.raw_stride > 0 else self.cout_pad          # floats per pixel of the raw buffer
    @property
    def store(self): return self.cout_store if self.cout_store > 0 else min(self.row, self.cout_pad)
    @property
    def values(self): return self.N * self.Ho * self.Wo * self.ngroup * self.store

    def group_taps(self, g):
        return self.taps[g * self.ntaps:(g + 1) * self.ntaps] if self.g_phase else self.taps

    def tapmul(self, g):
        return 1 + g * self.g_tapmul if self.ngroup > 1 and not self.g_phase else 1

    def origin(self, g):
        return ((g >> 1, g & 1) if self.g_phase else (self.ooy, self.oox))


def live_taps(c, g):
    """Brute force over every output pixel of the grid: does tap t of group g read an in-image pixel anywhere?"""
    m, out = c.tapmul(g), []
    hy, hx = (2 * c.Hin, 2 * c.Win) if c.up else (c.Hin, c.Win)
    for dy, dx in c.group_taps(g):
        hit = bool(c.reflect)
        for oy in range(c.Ho):
            for ox in range(c.Wo):
                iy, ix = oy * c.stride + dy * m, ox * c.stride + dx * m
                hit = hit or (0 <= iy < hy and 0 <= ix < hx)
        out.append(hit)
    return out


def kept_taps(c):
    """Per group, the indices of the taps the launch keeps: dead taps are dropped where the launch has one group, or four phase groups with EQUAL live counts (they share
    the k loop); groups of scaled taps keep everything."""
    ng = 4 if c.g_phase else 1
    if c.ngroup > 1 and not c.g_phase:
        return [list(range(c.ntaps))] * c.ngroup
    live = [live_taps(c, g) for g in range(ng)]
    cnt = [sum(l) for l in live]
    if cnt[0] > 0 and all(n == cnt[0] for n in cnt):
        return [[t for t in range(c.ntaps) if l[t]] for l in live]
    return [list(range(c.ntaps))] * ng


# ------------------------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=2)
def operands(c, kind):
    """x fp16 [N, Hin, Win, cin], w fp16 [groups, cout, cin, ntaps] (the values the kernel multiplies)."""
    G = c.ngroup
    xs, ws = (c.N, c.Hin, c.Win, c.cin), (G, c.cout, c.cin, c.ntaps)
    if kind == "exact":
        x = np.clip(np.floor(synth.uniform(xs, 100 * c.seed + 1, -8, 9)), -8, 8) / 8.0
        w = np.clip(np.floor(synth.uniform(ws, 100 * c.seed + 2, -8, 9)), -8, 8) / 8.0
    else:
        x = synth.uniform(xs, 100 * c.seed + 3, -1, 1)
        w = synth.uniform(ws, 100 * c.seed + 4, -1, 1) / np.float32(np.sqrt(c.ntaps * c.cin))
    return torch.from_numpy(np.asarray(x, np.float32)).half(), torch.from_numpy(np.asarray(w, np.float32)).half()


def input_slab(c, x, guard=4096):
    """The blocked-NHWC slab [chunk][N][Hin][Win][32] of x between guard bands of IN_GUARD, pad channels PAD_JUNK, a junk group behind the last chunk.
    Returns (flat fp16 tensor, offset of the first chunk in elements, group stride in elements)."""
    nch, gs = c.cin_pad // 32, c.N * c.Hin * c.Win * 32
    xp = torch.full((c.N, c.Hin, c.Win, c.cin_pad), PAD_JUNK, dtype=torch.float16)
    xp[..., :c.cin] = x
    body = xp.reshape(c.N, c.Hin, c.Win, nch, 32).permute(3, 0, 1, 2, 4).reshape(-1)
    band = torch.full((guard,), IN_GUARD, dtype=torch.float16)
    return torch.cat([band, body, torch.full((gs,), GROUP_JUNK, dtype=torch.float16), band]), guard, gs


# ------------------------------------------------------------------------------------------------ the reference
def gather(c, x, g):
    """The operand of group g: [M, ntaps, cin] in x's dtype, M = N * Ho * Wo -- the input pixel each tap reads, zero where it lies outside the image."""
    m = c.tapmul(g)
    oy, ox = torch.arange(c.Ho) * c.stride, torch.arange(c.Wo) * c.stride
    hy, hx = (2 * c.Hin, 2 * c.Win) if c.up else (c.Hin, c.Win)
    cols = []
    for dy, dx in c.group_taps(g):
        iy, ix = oy + dy * m, ox + dx * m
        if c.reflect:               # nn.ReflectionPad2d: the mirror without the border pixel
            iy = torch.where(iy < 0, -iy, torch.where(iy >= c.Hin, 2 * c.Hin - 2 - iy, iy))
            ix = torch.where(ix < 0, -ix, torch.where(ix >= c.Win, 2 * c.Win - 2 - ix, ix))
        vy, vx = (iy >= 0) & (iy < hy), (ix >= 0) & (ix < hx)
        sy, sx = iy.clamp(0, hy - 1), ix.clamp(0, hx - 1)
        if c.up:
            sy, sx = sy // 2, sx // 2
        blk = x[:, sy][:, :, sx] * (vy[:, None] & vx[None, :]).to(x.dtype)[None, :, :, None]
        cols.append(blk.reshape(-1, c.cin))
    return torch.stack(cols, 1)


def place(c, out, mask, g, y):
    """y [M, cout] of group g into the raw image out [N, Hfull, Wfull, row] (channels cout .. store are the zero rows of the padded panel)."""
    oy0, ox0 = c.origin(g)
    off = c.raw_off + g * c.g_outoff
    n = min(c.store, c.cout)
    blk = torch.zeros(c.N, c.Ho, c.Wo, c.store, dtype=out.dtype)
    blk[..., :n] = y.reshape(c.N, c.Ho, c.Wo, -1)[..., :n]
    out[:, oy0::c.os, ox0::c.os, off:off + c.store] = blk
    mask[:, oy0::c.os, ox0::c.os, off:off + c.store] = True


def width(c):
    """Floats per pixel of the buffer the case allocates: the row the launch addresses.  d_raw points raw_off columns into it; what the groups write stays inside."""
    assert c.raw_off + (0 if c.g_phase else (c.ngroup - 1) * c.g_outoff) + c.store <= c.row
    return c.row


def reference(c, x, w, dtype=torch.float64):
    """(raw image [N, Hfull, Wfull, width] in dtype, mask of the elements the launch writes)."""
    out = torch.zeros(c.N, c.Hfull, c.Wfull, width(c), dtype=dtype)
    mask = torch.zeros(out.shape, dtype=torch.bool)
    xd = x.to(dtype)
    for g in range(c.ngroup):
        A = gather(c, xd, g).reshape(-1, c.ntaps * c.cin)
        B = w[g].to(dtype).permute(2, 1, 0).reshape(c.ntaps * c.cin, c.cout)
        place(c, out, mask, g, A @ B)
    return out, mask


def conv32(c, x, w):
    """The same sums by float32 F.conv2d on the CPU: the gathered operand as the input of a 1x1 conv."""
    out = torch.zeros(c.N, c.Hfull, c.Wfull, width(c), dtype=torch.float32)
    mask = torch.zeros(out.shape, dtype=torch.bool)
    xf = x.float()
    for g in range(c.ngroup):
        A = gather(c, xf, g).reshape(-1, c.ntaps * c.cin)
        B = w[g].float().permute(0, 2, 1).reshape(c.cout, c.ntaps * c.cin)
        y = F.conv2d(A.t()[None, :, :, None].contiguous(), B[:, :, None, None])[0, :, :, 0].t()
        place(c, out, mask, g, y)
    return out


def emulate32(c, x, w, ksplit=None, seg=None, partials=False):
    """float32 in the kernel's order: the kept taps in order, each in 32-channel chunks -- one [M, 32] x [32, cout] product per k-step added in step order; the
    segments of a split launch summed separately, then added in split order.  partials: the list of the segments' raw images instead of their sum."""
    _, ks, sg, _ = c.expect
    ks, sg = ksplit or ks, seg or sg
    nch = c.cin_pad // 32
    keep = kept_taps(c)
    parts = [torch.zeros(c.N, c.Hfull, c.Wfull, width(c), dtype=torch.float32) for _ in range(ks)]
    mask = torch.zeros(parts[0].shape, dtype=torch.bool)
    xf = F.pad(x.float(), (0, c.cin_pad - c.cin))
    cp = replace(c, cin=c.cin_pad)
    for g in range(c.ngroup):
        A = gather(cp, xf, g)                                                   # [M, ntaps, cin_pad]
        B = F.pad(w[g].float(), (0, 0, 0, c.cin_pad - c.cin)).permute(2, 1, 0)      # [ntaps, cin_pad, cout]
        kg = keep[g if c.g_phase else 0]
        steps = [(t, ch) for t in kg for ch in range(nch)]
        for z in range(ks):
            acc = torch.zeros(A.shape[0], c.cout, dtype=torch.float32)
            lo, hi = (z * sg, min((z + 1) * sg, len(steps))) if ks > 1 else (0, len(steps))
            for t, ch in steps[lo:hi]:
                acc = acc + A[:, t, 32 * ch:32 * ch + 32] @ B[t, 32 * ch:32 * ch + 32]
            place(c, parts[z], mask, g, acc)
    if partials:
        return parts
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


@functools.lru_cache(maxsize=2)
def expected(c, kind):
    """(float64 raw image, mask, e32) of the case, computed once."""
    x, w = operands(c, kind)
    ref, mask = reference(c, x, w)
    if kind == "exact":
        return ref, mask, 0.0
    a = (conv32(c, x, w).double() - ref).abs().max().item()
    b = (emulate32(c, x, w).double() - ref).abs().max().item()
    print(f"[gather-gemm] {c.family} | {c}: e32 ingredients F.conv2d {a:.2e}, kernel-order emulation {b:.2e} (ratio {max(a, b) / max(min(a, b), 1e-30):.2f})")
    return ref, mask, max(a, b)


# ------------------------------------------------------------------------------------------------ the cases
def _c(name, family, N, Hin, Win, cin, cout, taps, Ho, Wo, expect, **kw):
    return Case(name, family, N, Hin, Win, cin, cout, tuple(taps), Ho, Wo, tuple(expect), **kw)


def _conv(name, family, N, H, W, cin, cout, taps, expect, stride=1, pad=None, **kw):
    """A conv whose output grid follows from the taps' reach: Ho = floor((H + lo + hi - span) / stride) + 1 with lo = -min(d), span = max(d) - min(d); `pad`
    overrides (lo_y, hi_y, lo_x, hi_x)."""
    dys, dxs = [t[0] for t in taps], [t[1] for t in taps]
    ly, hy, lx, hx = pad or (-min(dys), max(dys), -min(dxs), max(dxs))
    Ho, Wo = (H + ly + hy - (max(dys) - min(dys)) - 1) // stride + 1, (W + lx + hx - (max(dxs) - min(dxs)) - 1) // stride + 1
    return _c(name, family, N, H, W, cin, cout, taps, Ho, Wo, expect, stride=stride, **kw)


def _phase4(name, family, N, H, W, cin, cout, expect, **kw):
    """ConvTranspose2d(4, 2, 1) as the grouped launch of four phases."""
    taps = [(dy, dx) for ph in range(4) for dy, dx, _, _ in convt_phase_taps(4, ph >> 1, ph & 1)]
    return _c(name, family, N, H, W, cin, cout, taps, H, W, expect, os=2, ngroup=4, g_phase=1, **kw)


def _cases():
    L = []
    # 128 x 64 tile walk: M = 1, 127, 128, 129; batches whose tiles straddle images; cout_pad 64 / 128; cout 3 (raw_stride = cout_store = 4); cin 3, 32, 40, 96
    f = "tile walk"
    L += [_conv("3x3 40->64 1x1x1 (M 1)", f, 1, 1, 1, 40, 64, T3, (0, 1, 2, 1)),
          _conv("3x3 40->64 1x1x127 (M 127)", f, 1, 1, 127, 40, 64, T3, (0, 1, 6, 3)),
          _conv("3x3 40->64 1x8x16 (M 128)", f, 1, 8, 16, 40, 64, T3, (0, 1, 18, 9)),
          _conv("3x3 40->64 1x3x43 (M 129)", f, 1, 3, 43, 40, 64, T3, (0, 1, 18, 9)),
          _conv("3x3 3->3 3x5x7", f, 3, 5, 7, 3, 3, T3, (0, 1, 9, 9), raw_stride=4),
          _conv("3x3 3->3 300x5x7", f, 300, 5, 7, 3, 3, T3, (0, 1, 9, 9), raw_stride=4),
          _conv("3x3 96->128 5x5x7", f, 5, 5, 7, 96, 128, T3, (0, 1, 27, 9)),
          _conv("3x3 32->70 3x5x7", f, 3, 5, 7, 32, 70, T3, (0, 1, 9, 9), raw_stride=72)]
    # ring prologue: 1 .. 5 and 9 k-steps against the four stages and the three counted waits
    f = "ring prologue"
    L += [_conv(f"1x1 {32 * k}->64 2x5x7 ({k} steps)", f, 2, 5, 7, 32 * k, 64, T1, (0, 1, k, 1)) for k in (1, 2, 3, 4, 5)]
    L += [_conv("3x3 32->64 2x5x7 (9 steps)", f, 2, 5, 7, 32, 64, T3, (0, 1, 9, 9))]
    # tap tables at ragged sizes
    f = "tap tables"
    for H, W in ((5, 7), (9, 13)):
        L += [_conv(f"3x3 40->70 2x{H}x{W}", f, 2, H, W, 40, 70, T3, (0, 1, 18, 9)),
              _conv(f"3x3 s2 40->70 2x{H}x{W}", f, 2, H, W, 40, 70, T3, (0, 1, 18, 9), stride=2),
              _conv(f"3x3 s2 tf 40->70 2x{H}x{W}", f, 2, H, W, 40, 70, T3_TF, (0, 1, 18, 9), stride=2, pad=(0, 1, 0, 1)),
              _conv(f"4x4 s2 40->70 2x{H}x{W}", f, 2, H, W, 40, 70, T4, (0, 1, 32, 16), stride=2, pad=(1, 1, 1, 1)),
              _conv(f"7x7 40->70 2x{H}x{W}", f, 2, H, W, 40, 70, T7, (0, 1, 49, 49)),
              _conv(f"7x7 reflect 40->70 2x{H}x{W}", f, 2, H, W, 40, 70, T7, (0, 1, 49, 49), reflect=1),
              _conv(f"7x1 40->70 2x{H}x{W}", f, 2, H, W, 40, 70, T7x1, (0, 1, 14, 7)),
              _conv(f"7x1 reflect 40->70 2x{H}x{W}", f, 2, H, W, 40, 70, T7x1, (0, 1, 14, 7), reflect=1),
              _conv(f"3x3 reflect 40->70 2x{H}x{W}", f, 2, H, W, 40, 70, T3, (0, 1, 18, 9), reflect=1)]
    L += [_conv("3x3 s2 40->70 2x6x8 (even)", f, 2, 6, 8, 40, 70, T3, (0, 1, 18, 9), stride=2),
          _conv("3x3 s2 tf 40->70 2x6x8 (even)", f, 2, 6, 8, 40, 70, T3_TF, (0, 1, 18, 9), stride=2, pad=(0, 1, 0, 1)),
          _conv("4x4 s2 40->70 2x6x8 (even)", f, 2, 6, 8, 40, 70, T4, (0, 1, 32, 16), stride=2, pad=(1, 1, 1, 1)),
          _conv("3x3 reflect 40->64 32x2x2 (smallest)", f, 32, 2, 2, 40, 64, T3, (0, 1, 9, 9), reflect=1),
          _conv("7x7 reflect 40->64 4x4x4 (smallest)", f, 4, 4, 4, 40, 64, T7, (0, 1, 49, 49), reflect=1),
          _c("3x3 up 40->70 2x3x5 -> 6x10", f, 2, 3, 5, 40, 70, T3, 6, 10, (0, 1, 18, 9), up=1)]
    # dilated groups (PPON's fallback): eight convs of one input, taps scaled 1 .. 8, 32 channels each into a row wider than the eight of them
    f = "dilated groups"
    L += [_c(f"8 x 3x3 d1..8 64->32 2x{H}x{W}", f, 2, H, W, 64, 32, T3, H, W, (0, 1, 18, 9), ngroup=8, g_tapmul=1, g_outoff=32, cout_store=32, raw_stride=288)
          for H, W in ((9, 9), (5, 7), (17, 19))]
    # transposed convs: k = 3 as four single-phase launches (1 / 2 / 2 / 4 taps), k = 4 as the grouped launch
    f = "transposed"
    for H, W in ((1, 1), (1, 2), (2, 2), (3, 5), (8, 8)):
        for ph in range(4):
            a, b = ph >> 1, ph & 1
            tp = [(dy, dx) for dy, dx, _, _ in convt_phase_taps(3, a, b)]
            kept = (1 if a == 0 or H < 2 else 2) * (1 if b == 0 or W < 2 else 2)
            L.append(_c(f"convT k3 phase {a}{b} 40->64 {64 if H * W <= 4 else 2}x{H}x{W}", f, 64 if H * W <= 4 else 2, H, W, 40, 64, tp, H, W, (0, 1, 2 * kept, kept),
                        os=2, ooy=a, oox=b))
        kept = (1 if H < 2 else 2) * (1 if W < 2 else 2)
        L.append(_phase4(f"convT k4 phases 40->64 {16 if H * W <= 4 else 2}x{H}x{W}", f, 16 if H * W <= 4 else 2, H, W, 40, 64, (0, 1, 2 * kept, kept)))
    L.append(_c("phases with unequal live taps 40->64 4x2x3", f, 4, 2, 3, 40, 64, [(0, 0), (0, 1), (0, 0), (5, 0), (0, 0), (0, -1), (-7, 0), (0, 0)], 2, 3, (0, 1, 4, 2),
                os=2, ngroup=4, g_phase=1))
    # dead taps
    f = "dead taps"
    L += [_conv("4x4 s2 64->64 64x2x2 -> 1x1 (12 of 16 dropped)", f, 64, 2, 2, 64, 64, T4, (0, 1, 8, 4), stride=2, pad=(1, 1, 1, 1)),
          _conv("4x4 s2 64->64 16x4x4 -> 2x2 (none dropped)", f, 16, 4, 4, 64, 64, T4, (0, 1, 8, 16), stride=2, pad=(1, 1, 1, 1)),
          _phase4("convT k4 phases 64->64 16x1x1 (one tap per phase)", f, 16, 1, 1, 64, 64, (0, 1, 2, 1))]
    # split-K, tiny rule: 2x2 -> 1x1, 4 live taps
    f = "split-K tiny"
    L += [_conv(f"4x4 s2 {cin}->64 64x2x2 -> 1x1", f, 64, 2, 2, cin, 64, T4, e, stride=2, pad=(1, 1, 1, 1), scratch="ample")
          for cin, e in ((512, (0, 8, 8, 4)), (352, (0, 5, 9, 4)), (160, (0, 2, 10, 4)))]
    # split-K, general rule
    f = "split-K"
    L += [_conv(f"4x4 s2 {cin}->64 4x8x8 -> 4x4", f, 4, 8, 8, cin, 64, T4, e, stride=2, pad=(1, 1, 1, 1), scratch="ample")
          for cin, e in ((128, (0, 2, 32, 16)), (256, (0, 4, 32, 16)), (512, (0, 8, 32, 16)), (160, (0, 2, 40, 16)))]
    L += [_conv("3x3 480->64 1x8x8 (34 + 34 + 34 + 33)", f, 1, 8, 8, 480, 64, T3, (0, 4, 34, 9), scratch="ample"),
          _conv("3x3 480->64 1x5x13 (65 pixels: not split)", f, 1, 5, 13, 480, 64, T3, (0, 1, 34, 9), scratch="ample"),
          _conv("3x3 480->64 1x8x8, scratch one byte short", f, 1, 8, 8, 480, 64, T3, (0, 1, 34, 9), scratch="short"),
          _phase4("convT k4 phases 512->64 1x4x4 -> 8x8, split", f, 1, 4, 4, 512, 64, (0, 2, 32, 4), scratch="ample"),
          _conv("4x4 s2 128->3 342x8x8 -> 4x4, narrow row", f, 342, 8, 8, 128, 3, T4, (0, 2, 32, 16), stride=2, pad=(1, 1, 1, 1), scratch="ample", raw_stride=4),
          _conv("4x4 s2 128->64 4x8x8 -> 4x4, row wider than the store", f, 4, 8, 8, 128, 64, T4, (0, 2, 32, 16), stride=2, pad=(1, 1, 1, 1), scratch="ample",
                raw_stride=160, cout_store=64, raw_off=32)]
    # wide tiles
    f = "wide tiles"
    L += [_conv(f"3x3 64->{co} 1x{S}x{S}", f, 1, S, S, 64, co, T3, (sh, 1, 18, 9), **kw)
          for S, sh in ((127, 1), (181, 2)) for co, kw in ((512, {}), (510, dict(raw_stride=512, cout_store=512)))]
    L += [_phase4(f"convT k4 phases 512->{co} {N}x8x8 -> 16x16, split", f, N, 8, 8, 512, co, (sh, 2, 32, 4), scratch="ample")
          for co, N, sh in ((256, 64, 1), (512, 64, 2), (256, 1, 0), (512, 1, 0))]
    return L


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)
RANDOM_CASES = [c for c in CASES if c.values >= FEW]
# the random twins of the two largest layers cost a second of float64 matmul each and add no mechanism to their exact runs at the same shape: one width of each
RANDOM_CASES = [c for c in RANDOM_CASES if not (c.family == "wide tiles" and c.cout in (510,))]
