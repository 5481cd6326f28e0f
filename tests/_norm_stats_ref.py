"""Shared by test_norm_stats_cpu.py and test_gpu_norm_stats.py: the cases, the float64 reference and a numpy float32 emulation of the device arithmetic of the
fp16 engine's norm statistics -- the (count, mean, M2) records of csrc/conv3x3_stats_gate_rlds.h epilogue_stats and their merges in csrc/norm_stats.h
(combine_parts_kernel), resnet.hip (rn_post_slab_parts) and unet.hip (unet_post_slab_parts).

Record layout (what the emulation and the GPU test index by): the kernel's grid (the conv's output, or the INPUT grid of a transposed conv with its four output
phases) is cut into tiles of 16 x 32 pixels; each of a tile's 8 consumer waves owns 2 rows.  Record r of an image:
    r = ((tile_row * tile_cols + tile_col) * phases + phase) * 8 + wave,      part[((n * nper + r) * channels + c) * 3] = (count, mean, M2)
phase (a, b) = (ph >> 1, ph & 1) of a transposed conv is output pixel (2 y + a, 2 x + b) of grid pixel (y, x).

Data kinds (per case: operands rounded to fp16, bias fp32):
  a  zero-mean uniform input and weights;
  b  non-negative input |x| (as behind a ReLU), zero-mean weights;
  c  a non-negative input as in b (the images of a batch share 0.8 of their content), weights with a common positive offset per output channel, solved on the float64 reference so that |mean - bias| / std of every
     (image, channel) is 8 (asserted: within [6, 10]).  The offset sits on the taps that EVERY output pixel sees inside the image -- the centre tap of the
     3 x 3 and 7 x 1 kernels, the inner 2 x 2 taps of the 4 x 4 and transposed kernels.  On a tap that zero padding cuts off at the border the response's spread
     would be tied to the border's share of the image, which alone caps the ratio below 6 on the small grids (2.5 on a 3 x 3 transposed grid).
  d  characterisation only: a flat input in [0.4, 0.6] and the offset solved for a ratio of 30.
Every family has cases whose record count is no multiple of 32 (8, 72) except the transposed one, whose 4 phases x 8 waves make every count one.
A plane of one pixel has no spread (std = 0): there the ratio is not defined and not asserted; the case still runs."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

TH, TW, NCW, RPW = 16, 32, 8, 2          # tile rows / columns, consumer waves per tile, rows per wave
EPS = 1e-5                                # the networks' eps
CEILING = 2.0 ** -12                      # hard ceiling of the y metric: a quarter of an fp16 ulp
MARGIN = 8.0                              # working bound = MARGIN x the emulation's worst error on the same cases
KINDS = ("a", "b", "c")

# family: plain (3x3; opt = reflect_pad 0 zero / 1 reflect / 2 replicate), up (ConvTranspose2d(k, 2, 1); opt = k; H x W the INPUT grid),
# down (Conv2d(4, 2, 1); H x W the OUTPUT grid), col (7 x 1; opt = 1: reflected rows)
Case = namedtuple("Case", "family N C K H W opt")


def _plain_cases():
    out = []
    for (N, H, W) in [(1, 1, 1), (1, 2, 17), (1, 15, 31), (1, 16, 32), (2, 17, 33), (3, 33, 65), (1, 37, 70)]:
        for pad in (0, 1, 2):
            if pad == 1 and (H < 2 or W < 2):
                continue                   # ReflectionPad2d(1) needs two pixels
            out.append(Case("plain", N, 64, 64, H, W, pad))
    out.append(Case("plain", 2, 96, 128, 17, 33, 1))      # two channel groups: stats_cn = K = 128
    out.append(Case("plain", 1, 64, 64, 48, 65, 0))       # 72 records whose LAST one holds pixels (33 x 65 and 37 x 70 end in an empty wave): what the merges' rr < nper guards keep out
    return out


def _up_cases():
    out = [Case("up", 3, 64, 64, 3, 3, 4), Case("up", 1, 64, 128, 3, 3, 3), Case("up", 1, 64, 64, 9, 17, 4), Case("up", 2, 64, 64, 16, 32, 3),
           Case("up", 1, 64, 128, 17, 40, 4), Case("up", 2, 64, 64, 17, 40, 3)]
    i = 0
    for (H, W) in [(20, 1), (7, 5), (16, 16)]:             # grids at most 16 wide: two images per tile row; an odd N leaves a pair without its second image
        for N in (1, 2, 3):
            out.append(Case("up", N, 64, 128 if i % 4 == 3 else 64, H, W, 4 if i % 2 == 0 else 3))
            i += 1
    return out


def _down_cases():
    return [Case("down", N, 32, 64, H, W, 0) for (H, W) in [(8, 16), (5, 7), (17, 33), (16, 32)] for N in (1, 3)]


def _col_cases():
    return [Case("col", 1 + (i % 2), 32, 64, H, W, r) for i, (H, W, r) in enumerate((H, W, r) for H in (4, 16, 23) for W in (17, 40) for r in (0, 1))]


CASES = {"plain": _plain_cases(), "up": _up_cases(), "down": _down_cases(), "col": _col_cases()}
ALL_CASES = [c for f in ("plain", "up", "down", "col") for c in CASES[f]]
# kind d (ratio 30, characterisation only): one ragged multi-tile case per family
D_CASES = [Case("plain", 3, 64, 64, 33, 65, 0), Case("up", 2, 64, 64, 17, 40, 3), Case("down", 3, 32, 64, 17, 33, 0), Case("col", 2, 32, 64, 23, 40, 1)]


def case_id(c):
    return "%s-N%d-C%d-K%d-%dx%d-o%d" % c


def phases(c):
    return 4 if c.family == "up" else 1


def out_hw(c):
    return (2 * c.H, 2 * c.W) if c.family == "up" else (c.H, c.W)


def records_per_image(H, W, nph):
    return ((H + TH - 1) // TH) * ((W + TW - 1) // TW) * nph * NCW


# ------------------------------------------------------------------------------------------------ operands and the float64 reference
def conv64(c, x, w, b):
    """The conv of case c in float64: x, w float64 tensors (fp16-representable values), b float64 [K] or None.  [N, K, Ho, Wo]."""
    if c.family == "plain":
        xp = F.pad(x, (1, 1, 1, 1), mode=("constant", "reflect", "replicate")[c.opt])
        y = F.conv2d(xp, w)
    elif c.family == "up":
        y = F.conv_transpose2d(x, w, None, stride=2, padding=1, output_padding=1 if c.opt == 3 else 0)
    elif c.family == "down":
        y = F.conv2d(x, w, None, stride=2, padding=1)
    else:
        xp = F.pad(x, (0, 0, 3, 3), mode="reflect" if c.opt else "constant")
        y = F.conv2d(xp, w[:, :, :, None])
    return y if b is None else y + b.view(1, -1, 1, 1)


def _shapes(c):
    """(input shape, weight shape, output-channel axis of the weight, the offset pattern u of kinds c / d as a weight of ONE output channel)"""
    if c.family == "plain":
        u = torch.zeros(1, c.C, 3, 3, dtype=torch.float64)
        u[:, :, 1, 1] = 1
        return (c.N, c.C, c.H, c.W), (c.K, c.C, 3, 3), 0, u
    if c.family == "up":
        k = c.opt
        u = torch.zeros(c.C, 1, k, k, dtype=torch.float64)
        u[:, :, 1:3, 1:3] = 1              # tap k of a row reaches output row 2 i - 1 + k: taps 1 and 2 always land inside
        return (c.N, c.C, c.H, c.W), (c.C, c.K, k, k), 1, u
    if c.family == "down":
        u = torch.zeros(1, c.C, 4, 4, dtype=torch.float64)
        u[:, :, 1:3, 1:3] = 1              # tap k reads source row 2 o - 1 + k: taps 1 and 2 never leave the image
        return (c.N, c.C, 2 * c.H, 2 * c.W), (c.K, c.C, 4, 4), 0, u
    u = torch.zeros(1, c.C, 7, dtype=torch.float64)
    u[:, :, 3] = 1
    return (c.N, c.C, c.H, c.W), (c.K, c.C, 7), 0, u


def _solve_offset(c, x, w0, u, target):
    """Per output channel, the offset t with sqrt(min_n ratio * max_n ratio) = target, ratio = |mean| / std of conv(x, w0 + t u) per image (no bias)."""
    A = conv64(c, x, w0, None).flatten(2).numpy()                 # [N, K, P]
    B = conv64(c, x, u, None).flatten(2).numpy()                  # [N, 1, P]
    mA, mB = A.mean(2), B.mean(2)
    dA, dB = A - mA[..., None], B - mB[..., None]
    vA, vB, cAB = (dA * dA).mean(2), (dB * dB).mean(2), (dA * dB).mean(2)

    def g(t):                                                     # t [K]
        m = np.abs(mA + t * mB)
        v = np.maximum(vA + 2 * t * cAB + t * t * vB, 1e-300)
        r = m / np.sqrt(v)
        return np.sqrt(r.min(0) * r.max(0))
    lo, hi = np.full(A.shape[1], 1e-6), np.full(A.shape[1], 1e3)
    if A.shape[2] > 1 and not (g(hi) > target).all():
        raise AssertionError("%s: a ratio of %g is out of reach (limit %g)" % (case_id(c), target, g(hi).min()))
    for _ in range(80):
        mid = np.sqrt(lo * hi)
        up = g(mid) < target
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return np.sqrt(lo * hi) if A.shape[2] > 1 else np.full(A.shape[1], 0.05)


_Data = namedtuple("_Data", "x w b y mean var ratio")


@functools.lru_cache(maxsize=None)
def data(c, kind):
    """Operands and float64 reference of (case, kind), computed once: x, w (float32 tensors holding fp16 values), b float32 [K], y float64 [N, K, Ho, Wo] (bias
    included), mean / var (biased) float64 [N, K], ratio = |mean - bias| / std float64 [N, K] (inf where std = 0)."""
    xs, ws, kax, u = _shapes(c)
    seed = sum((i + 1) * 7919 * int(v) for i, v in enumerate(c[1:])) + 104729 * "abcd".index(kind) + 15485863 * ("plain", "up", "down", "col").index(c.family)
    rng = np.random.default_rng(seed)
    taps_c = float(np.prod(ws)) / c.K / (4.0 if c.family == "up" else 1.0)       # operands per output value
    x = rng.uniform(-1, 1, xs)
    if kind in "cd" and c.N > 1:
        # one offset per channel serves every image of the batch: the images share most of their content (0.8 of a common pattern, 0.2 their own), else the spread of
        # a 35-pixel plane's sample std between images (a factor 1.7 over 64 channels) does not fit into [6, 10]
        x = 0.8 * x[:1] + 0.2 * rng.uniform(-1, 1, xs)
    if kind in "bc":
        x = np.abs(x)
    elif kind == "d":
        x = 0.5 + 0.1 * x
    w = rng.uniform(-1, 1, ws) / math.sqrt(taps_c)
    b = rng.uniform(-0.5, 0.5, c.K)
    x = torch.from_numpy(x).half().double()
    w = torch.from_numpy(w).half().double()
    if kind in "cd":
        t = torch.from_numpy(_solve_offset(c, x, w, u, 8.0 if kind == "c" else 30.0))
        w = (w + u * t.view([-1 if i == kax else 1 for i in range(w.dim())])).half().double()
    b32 = torch.from_numpy(b).float()
    y = conv64(c, x, w, b32.double())
    mean = y.mean((2, 3))
    var = ((y - mean[..., None, None]) ** 2).mean((2, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (mean - b32.double()).abs().numpy() / np.sqrt(var.numpy())
    return _Data(x.float(), w.float(), b32, y, mean.numpy(), var.numpy(), ratio)


def affine(c, which):
    """(gamma, beta) float32 [K] of the norm layer behind case c, or (None, None): which = 0 none, 1 with"""
    if not which:
        return None, None
    rng = np.random.default_rng(4242 + c.K)
    return rng.uniform(0.5, 1.5, c.K).astype(np.float32), rng.uniform(-0.5, 0.5, c.K).astype(np.float32)


def alpha_shift64(mean, var, gamma=None, beta=None, eps=EPS):
    a = (1.0 if gamma is None else gamma.astype(np.float64)) / np.sqrt(var + eps)
    return a, (0.0 if beta is None else beta.astype(np.float64)) - mean * a


def y_error(alpha, shift, alpha64, shift64, xs):
    """The y metric: worst |y - y64| / max(1, |y64|, |x alpha64|) of y = x alpha + shift over the probe values xs [N, K, m] (float64; the channel's min,
    max and mean), alpha / shift as the device (or the emulation) gave them."""
    a, s = np.asarray(alpha, np.float64)[..., None], np.asarray(shift, np.float64)[..., None]
    a64, s64 = np.asarray(alpha64)[..., None], np.asarray(shift64)[..., None]
    y, y64 = xs * a + s, xs * a64 + s64
    return float((np.abs(y - y64) / np.maximum(1.0, np.maximum(np.abs(y64), np.abs(xs * a64)))).max())


def probes(y):
    """[N, K, 3]: min, max and mean of every (image, channel) plane of y [N, K, ...]"""
    f = y.reshape(y.shape[0], y.shape[1], -1)
    f = f.numpy() if isinstance(f, torch.Tensor) else f
    return np.stack([f.min(2), f.max(2), f.mean(2)], 2)


# ------------------------------------------------------------------------------------------------ records
def regions(c, y):
    """The 64-pixel region of every record: values [N, nper, K, 64] float64 (0 outside the image) and the validity mask [nper, 64] of y [N, K, Ho, Wo]
    (numpy float64) in the record order given at the top."""
    N, K = y.shape[:2]
    P = phases(c)
    if P == 4:
        v = np.stack([y[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)], 1)      # [N, P, K, H, W]
    else:
        v = y[:, None]
    ty, tx = (c.H + TH - 1) // TH, (c.W + TW - 1) // TW
    vp = np.zeros((N, P, K, ty * TH, tx * TW))
    vp[..., :c.H, :c.W] = v
    m = np.zeros((ty * TH, tx * TW), bool)
    m[:c.H, :c.W] = True
    vals = vp.reshape(N, P, K, ty, NCW, RPW, tx, TW).transpose(0, 3, 6, 1, 4, 2, 5, 7).reshape(N, ty * tx * P * NCW, K, RPW * TW)
    mask = np.broadcast_to(m.reshape(ty, NCW, RPW, tx, TW).transpose(0, 3, 1, 2, 4)[:, :, None], (ty, tx, P, NCW, RPW, TW)).reshape(ty * tx * P * NCW, RPW * TW)
    return vals, mask


def records64(vals, mask):
    """float64 (count [nper], mean [N, nper, K], M2 [N, nper, K]) of every record's region (mean 0 where the region is empty)"""
    cnt = mask.sum(1).astype(np.float64)
    mk = mask[None, :, None, :]
    mean = (vals * mk).sum(3) / np.maximum(cnt, 1)[None, :, None]
    M2 = (((vals - mean[..., None]) * mk) ** 2).sum(3)
    return cnt, mean, M2


def emulate_records(vals, mask, bias, cnt=None):
    """epilogue_stats in float32: the accumulators hold fp32(conv + bias); d = x - bias, s1 = sum d, s2 = sum d^2 over the wave's 64 values in sequence,
    mean = s1 * (1 / count), record = (count, bias + mean, max(s2 - s1 * mean, 0)).  [N, nper, K, 3] float32."""
    f = np.float32
    x = vals.astype(f)
    bl = np.asarray(bias, f)[None, None, :]
    s1 = np.zeros(x.shape[:3], f)
    s2 = np.zeros(x.shape[:3], f)
    for i in range(x.shape[3]):
        d = np.where(mask[None, :, None, i], x[..., i] - bl, f(0))
        s1 = s1 + d
        s2 = s2 + d * d
    cnt = (mask.sum(1) if cnt is None else cnt).astype(f)          # (cnt: a count other than the region's, for the planted faults of test_norm_stats_cpu.py)
    with np.errstate(divide="ignore"):
        inv = np.where(cnt > 0, f(1) / cnt, f(0)).astype(f)[None, :, None]
    mean = s1 * inv
    rec = np.empty(x.shape[:3] + (3,), f)
    rec[..., 0] = cnt[None, :, None]
    rec[..., 1] = bl + mean
    rec[..., 2] = np.maximum(s2 - s1 * mean, f(0))
    return rec


def _chan_merge(n, mu, m2, nb, mub, m2b):
    """norm::chan_merge in float32 on arrays (count 0: no-op)"""
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        tot = n + nb
        d = mub - mu
        mu2 = mu + d * (nb / tot)
        m22 = m2 + (m2b + d * d * (n * nb / tot))
    ok = nb > 0
    return np.where(ok, tot, n).astype(f), np.where(ok, mu2, mu).astype(f), np.where(ok, m22, m2).astype(f)


def emulate_merge(rec, lanes, merge=None):
    """The merges as the kernels write them, float32.  lanes = 32: combine_parts_kernel -- lane pl of a channel merges records pl, pl + 32, .. in order, then lanes
    1 .. 31 are merged into lane 0 in lane order.  lanes = 8: rn_post_slab_parts and unet_post_slab_parts (one merge order, written twice) -- lane lg takes, per trip
    r = lg, lg + 32, .., the records r, r + 8, r + 16, r + 24 below nper: every record = lg (mod 8) in rising order, then lanes 1 .. 7 into lane 0.
    rec [N, nper, K, 3] -> (count, mean, M2) [N, K] float32."""
    f = np.float32
    _chan_merge = merge or globals()["_chan_merge"]
    N, nper, K, _ = rec.shape
    steps = (nper + lanes - 1) // lanes
    pad = np.zeros((N, steps * lanes, K, 3), f)
    pad[:, :nper] = rec
    pad = pad.reshape(N, steps, lanes, K, 3)
    n, mu, m2 = (np.zeros((N, lanes, K), f) for _ in range(3))
    for s in range(steps):
        n, mu, m2 = _chan_merge(n, mu, m2, pad[:, s, :, :, 0], pad[:, s, :, :, 1], pad[:, s, :, :, 2])
    cn, cmu, cm2 = n[:, 0], mu[:, 0], m2[:, 0]
    for i in range(1, lanes):
        cn, cmu, cm2 = _chan_merge(cn, cmu, cm2, n[:, i], mu[:, i], m2[:, i])
    return cn, cmu, cm2


def alpha_shift32(mu, m2, HW, gamma=None, beta=None, eps=EPS):
    """bn_write in float32: alpha = (1 / sqrt(M2 / HW + eps)) * gamma, shift = beta - mean * alpha"""
    f = np.float32
    a = (f(1) / np.sqrt(m2 / f(HW) + f(eps), dtype=f)) * (f(1) if gamma is None else gamma.astype(f))
    return a.astype(f), ((f(0) if beta is None else beta.astype(f)) - mu * a).astype(f)


def record_error(rec, cnt, mean64, M264):
    """Worst error of the records' means, relative to max(1, |mean|), and of their M2, relative to max(1, M2), over the records that hold pixels"""
    has = cnt > 0
    r = np.asarray(rec, np.float64)[:, has]
    em = np.abs(r[..., 1] - mean64[:, has]) / np.maximum(1.0, np.abs(mean64[:, has]))
    e2 = np.abs(r[..., 2] - M264[:, has]) / np.maximum(1.0, M264[:, has])
    return float(max(em.max(), e2.max()))


_Ref = namedtuple("_Ref", "vals mask cnt mean M2 xs")


@functools.lru_cache(maxsize=None)
def reference_records(c, kind):
    """Of (case, kind), computed once: the records' regions (regions), their float64 (count, mean, M2) (records64) and the planes' probe values (probes)"""
    y = data(c, kind).y.numpy()
    vals, mask = regions(c, y)
    return _Ref(vals, mask, *records64(vals, mask), probes(y))


_Emu = namedtuple("_Emu", "y rec")


@functools.lru_cache(maxsize=None)
def emulation_error(c, kind):
    """The float32 emulation's error on (case, kind) against float64: y = the y metric, worst over the two merge orders, without and with gamma / beta;
    rec = record_error of the emulated records."""
    d = data(c, kind)
    vals, mask, cnt, m64, M264, xs = reference_records(c, kind)
    rec = emulate_records(vals, mask, d.b.numpy())
    HW = d.y.shape[2] * d.y.shape[3]
    worst = 0.0
    for lanes in (32, 8):
        _, mu, m2 = emulate_merge(rec, lanes)
        for which in (0, 1):
            g, bt = affine(c, which)
            a, s = alpha_shift32(mu, m2, HW, g, bt)
            a64, s64 = alpha_shift64(d.mean, d.var, g, bt)
            worst = max(worst, y_error(a, s, a64, s64, xs))
    return _Emu(worst, record_error(rec, cnt, m64, M264))


@functools.lru_cache(maxsize=None)
def working_bounds(family, kind):
    """(y bound, record bound) of a family and data kind: MARGIN x the emulation's worst error over that family's cases.  The margin covers what the
    emulation does not model: the kernel sums in-lane and then by butterfly, its accumulators carry the MFMA's fp32 rounding, the compiler may contract
    s2 - s1 * mean.  Never computed from the code under test."""
    es = [emulation_error(c, kind) for c in CASES[family]]
    return MARGIN * max(e.y for e in es), MARGIN * max(e.rec for e in es)


# ------------------------------------------------------------------------------------------------ the re-read kernels' data
def plane_data(N, C, HW, kind, seed):
    """[N, C, HW] float64 of fp16-representable values: kind a zero-mean uniform; kind c mean / std = 8 per plane (exactly before the fp16 rounding; HW = 1: no
    spread, a lone value)."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(-1, 1, (N, C, HW))
    if kind == "c":
        if HW > 1:
            z = z - z.mean(2, keepdims=True)
            z = z / np.sqrt((z * z).mean(2, keepdims=True))
        sd = rng.uniform(0.1, 0.4, (N, C, 1))
        z = sd * (8.0 + z)
    return torch.from_numpy(z).half().double().numpy()


def emulate_two_pass(x, seg=1024):
    """The re-read kernels (stats_kernel, stats_slab8_kernel, combine_kernel) in float32: per segment of 1024 pixels the mean and the sum of squared deviations from
    it, segments combined with  M2 = sum M2_s + sum n_s (mean_s - mean)^2.  x [N, C, HW] -> (mean, M2) float32 [N, C].  (numpy's float32 sums: a summation order of
    its own, as the kernels' lanes-then-waves order is.)"""
    f = np.float32
    x = x.astype(f)
    HW = x.shape[2]
    mus, m2s, ns = [], [], []
    for p0 in range(0, HW, seg):
        v = x[:, :, p0:p0 + seg]
        n = f(v.shape[2])
        mu = v.sum(2, dtype=f) / n
        dv = v - mu[..., None]
        mus.append(mu); m2s.append((dv * dv).sum(2, dtype=f)); ns.append(n)
    if len(ns) == 1:
        return mus[0], m2s[0]
    tot = np.zeros_like(mus[0])
    for mu, n in zip(mus, ns):
        tot = tot + mu * n
    mean = tot / f(HW)
    M2 = np.zeros_like(mean)
    for mu, m2, n in zip(mus, m2s, ns):
        dm = mu - mean
        M2 = M2 + (m2 + n * dm * dm)
    return mean.astype(f), M2.astype(f)
