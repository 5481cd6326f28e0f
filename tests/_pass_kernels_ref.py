"""float64 references, case lists and comparators for the pass kernels of the pix2pix UNet (csrc/unet.hip) and the CycleGAN ResNet (csrc/resnet.hip) -- the
launches between one conv and the next, reached one at a time through the entry points of ABI 123.  No GPU here: tests/test_pass_kernels_cpu.py holds these
references to the torch modules they restate and shows that the comparators catch planted faults; tests/test_gpu_pass_kernels.py holds the kernels to them.

The references are written from the module definitions, not from the kernels:
  nn.BatchNorm2d in training mode on one image (= nn.InstanceNorm2d): per (image, channel) mean and BIASED variance over H * W, eps 1e-5 ........ bn_alpha_shift
  nn.LeakyReLU(0.2) / nn.ReLU ..................................................................................................................... act
  nn.ReflectionPad2d(3) plus one ring of zeros: the (H + 8) x (W + 8) slab the last conv's sub-block form reads ................................... pad_index
  nn.Conv2d(C, 64, 4, 2, 1): the 16 * C window values of an output pixel, tap-major (channel (ky * 4 + kx) * C + c) ................................. unet_patch
  nn.ReflectionPad2d(3) + the kx taps of a 7 x 7 conv as channels (kx * C + c) ................................................................... row_patch
  a 7 x 7 kernel, zero-padded to 9 x 9, as nine 3 x 3 sub-blocks (sr, sc): out = tanh(b + sum Q[sr, sc] displaced by 3 (sr - 1), 3 (sc - 1)) ....... sum9

Bounds (none is taken from the code under test):
  pass_bound   |got - ref| <= ulp16(max(|ref|, |got|)) / 2 + 4 * 2^-24 * (|x alpha| + |shift| + |res|): the fp16 store's rounding, plus up to three fp32 roundings
               (the product, the sum, then the 0.2 of the LeakyReLU or the residual add), each at most 2^-24 of a magnitude no larger than that sum, whether or not
               the compiler contracts the multiply-add; 4 is the next power of two.  Where x is itself a float32 sum of ks split-K segments (unet_deep_post without
               statistics), each of its ks - 1 additions rounds once more, by at most 2^-24 of sum |segment|: + (ks - 1) * 2^-24 * |alpha| * sum |segment|.
  deep post with statistics: the project's y metric (tests/_norm_stats_ref.py) -- the error of y = x alpha + shift relative to max(1, |y|, |x alpha|), beyond the fp16
               store's 2^-11 -- held to MARGIN x e_emul of the (instantiation, kind), ceiling 2^-12; e_emul is the error of emulate_deep_post (float32, the kernel's
               order of operations) against float64.
  conv / tanh: ulp16 / 2 + 8 * e32 (+ 2^-21 for the hardware tanh, as tests/test_gpu_conv_forms.py), e32 = the error of the same computation in float32 on the CPU.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _norm_stats_ref as NS

EPS = NS.EPS
CEILING = NS.CEILING
MARGIN = NS.MARGIN
TANH_HW = 2.0 ** -21              # allowance for the hardware tanh (tests/test_gpu_conv_forms.py)


# ------------------------------------------------------------------------------------------------ layouts
def to_slab(x, fill=0.0):
    """[N, C, H, W] -> the fp16 blocked-NHWC slab [ceil(C / 32), N, H, W, 32]; channels beyond C hold `fill`"""
    x = torch.as_tensor(x)
    N, Cc, H, W = x.shape
    G = -(-Cc // 32)
    p = torch.full((N, G * 32, H, W), fill, dtype=torch.float16)
    p[:, :Cc] = x.half()
    return p.view(N, G, 32, H, W).permute(1, 0, 3, 4, 2).contiguous()


def from_slab(s):
    """[G, N, H, W, 32] -> [N, G * 32, H, W]"""
    G, N, H, W, _ = s.shape
    return s.permute(1, 0, 4, 2, 3).reshape(N, G * 32, H, W)


def to_rows(x, cpad, fill=float("nan")):
    """[N, C, HW] -> float32 rows [N, HW, cpad]; the padding columns hold `fill`"""
    x = torch.as_tensor(x)
    N, Cc, HW = x.shape
    r = torch.full((N, HW, cpad), fill, dtype=torch.float32)
    r[:, :, :Cc] = x.permute(0, 2, 1).float()
    return r


def bits16(t):
    return torch.as_tensor(t).contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ comparators
def ulp16(v):
    """Spacing of fp16 at |v| (float64 array): 2^-24 in the subnormal range, 2^(e - 10) for 2^e <= |v| < 2^(e + 1)"""
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(np.maximum(v, 2.0 ** -14))               # v = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, e - 1 - 10)


def act(v, a):
    """a: 0 none, 1 LeakyReLU(0.2), 2 ReLU"""
    return np.maximum(v, 0.2 * v) if a == 1 else np.maximum(v, 0.0) if a == 2 else v


def pass_ref(x, alpha, shift, a, res=None):
    """float64 act(x alpha + shift) [+ res] and the magnitude the fp32 roundings scale with; x [N, C, ...], alpha / shift broadcastable (None: 1 / 0)"""
    x = np.asarray(x, np.float64)
    xa = x * (1.0 if alpha is None else alpha)
    v = xa + (0.0 if shift is None else shift)
    mag = np.abs(xa) + np.abs(0.0 if shift is None else shift)
    ref = act(v, a)
    if res is not None:
        ref = ref + res
        mag = mag + np.abs(res)
    return ref, mag


def pass_bound(ref, got, mag, extra=0.0):
    return ulp16(np.maximum(np.abs(ref), np.abs(got))) / 2 + 4 * 2.0 ** -24 * mag + extra


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; NaN or inf in `got` counts as infinitely wrong"""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / bound).max())


def passes(got, ref, bound):
    return worst_ratio(got, ref, bound) <= 1.0


# ------------------------------------------------------------------------------------------------ norm statistics (BatchNorm2d.train() on one image == InstanceNorm2d)
def bn_alpha_shift(x, gamma=None, beta=None, eps=EPS):
    """x [N, C, HW] float64 -> alpha, shift [N, C]: norm(x) = x alpha + shift with the image's mean and biased variance"""
    mean, var = x.mean(2), ((x - x.mean(2, keepdims=True)) ** 2).mean(2)
    a = (1.0 if gamma is None else np.asarray(gamma, np.float64)) / np.sqrt(var + eps)
    return a, (0.0 if beta is None else np.asarray(beta, np.float64)) - mean * a


# ------------------------------------------------------------------------------------------------ gathers
def unet_pre_ref(x):
    """NCHW -> [N, H * W, 32]: channels beyond C zero"""
    N, Cc, H, W = x.shape
    o = torch.zeros(N, H * W, 32, dtype=x.dtype)
    o[:, :, :Cc] = x.reshape(N, Cc, H * W).permute(0, 2, 1)
    return o


def unet_patch(x, order="ky*4+kx"):
    """The windows of Conv2d(C, 64, 4, 2, 1) as a 64-channel image at half resolution: [N, 64, H / 2, W / 2], channel (ky * 4 + kx) * C + c =
    zero-padded x[c][2 oy - 1 + ky][2 ox - 1 + kx], zero beyond 16 * C.  (order "kx*4+ky": the deliberately wrong restatement of the CPU test.)"""
    N, Cc, H, W = x.shape
    u = F.unfold(x, 4, padding=1, stride=2).view(N, Cc, 4, 4, H // 2, W // 2)             # [n, c, ky, kx, oy, ox]
    if order != "ky*4+kx":
        u = u.transpose(2, 3)
    o = torch.zeros(N, 64, H // 2, W // 2, dtype=x.dtype)
    o[:, :16 * Cc] = u.permute(0, 2, 3, 1, 4, 5).reshape(N, 16 * Cc, H // 2, W // 2)
    return o


def unet_patch_weight(w):
    """[64, C, 4, 4] -> [64, 64] over unet_patch's channels"""
    K, Cc = w.shape[:2]
    o = torch.zeros(K, 64, dtype=w.dtype)
    o[:, :16 * Cc] = w.permute(0, 2, 3, 1).reshape(K, 16 * Cc)
    return o


def row_patch(x):
    """The row-patch slab of ReflectionPad2d(3) + a 7-wide kernel row: [N, 32, H, W], channel kx * C + c = reflect-padded x[c][y][x + kx - 3], zero beyond 7 * C"""
    N, Cc, H, W = x.shape
    p = F.pad(x, (3, 3, 0, 0), mode="reflect")
    o = torch.zeros(N, 32, H, W, dtype=x.dtype)
    for kx in range(7):
        o[:, kx * Cc:(kx + 1) * Cc] = p[:, :, :, kx:kx + W]
    return o


def reflect_index(n):
    """Source index of every position of ReflectionPad2d(3) along an axis of n: [n + 6]"""
    i = np.arange(n + 6) - 3
    return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))


def pad_ref(v, both=True, ring=0.0, row_off=0):
    """ReflectionPad2d(3) of v [N, C, H, W] plus one outer ring of `ring`: [N, C, H + 8, W + 8].  The faults of the CPU test: row_off = 1 mirrors the rows above
    the image about the wrong line (source row y at padded row 3 - y instead of 4 - y); both = False applies only the near mirror where a source row has two mirror targets (H in 4 .. 6) and leaves the far one at the fill."""
    v = np.asarray(v)
    N, Cc, H, W = v.shape
    iy, ix = reflect_index(H), reflect_index(W)
    if row_off:
        iy[:3] -= row_off
    o = np.full((N, Cc, H + 8, W + 8), ring, v.dtype)
    o[:, :, 1:-1, 1:-1] = v[:, :, iy][:, :, :, ix]
    if not both:
        for y in range(1, 4):
            if H - 4 <= y <= H - 2:                          # source row y is mirrored above AND below the image: drop the lower copy
                o[:, :, 2 * (H - 1) - y + 4, 1:-1] = -7.0
    return o


def sum9_ref(Q, bias, K, H, W, disp=3):
    """Q [N, 9 K, H + 8, W + 8] float64 -> the pre-activation [N, K, H, W]: bias + sum over (sr, sc) of Q[9 k + 3 sr + sc][y + 3 sr + 1][x + 3 sc + 1]
    (disp != 3: the fault of the CPU test, in sub-block (2, 1) only)"""
    N = Q.shape[0]
    o = np.broadcast_to(np.asarray(bias, np.float64)[None, :, None, None], (N, K, H, W)).copy()
    for sr in range(3):
        for sc in range(3):
            d = disp if (sr, sc) == (2, 1) else 3
            o += Q[:, sr * 3 + sc::9][:, :K, d * sr + 1:d * sr + 1 + H, 3 * sc + 1:3 * sc + 1 + W]
    return o


def sum9_weights(w7):
    """[K, C, 7, 7] -> the nine 3 x 3 sub-blocks of the kernel zero-padded to 9 x 9: [9 K, C, 3, 3], channel 9 k + 3 sr + sc"""
    K, Cc = w7.shape[:2]
    w9 = F.pad(w7, (1, 1, 1, 1))
    return w9.view(K, Cc, 3, 3, 3, 3).permute(0, 2, 4, 1, 3, 5).reshape(9 * K, Cc, 3, 3)       # [k, sr, r, sc, s] -> [k, sr, sc, c, r, s]


# ------------------------------------------------------------------------------------------------ unet_deep_post
DEEP_HW = (1, 2, 4, 5, 16, 17, 64, 65, 255, 256)
DEEP_C = (32, 64, 40)
DEEP_KS = (1, 2, 8, 9, 16, 17)
DEEP_N = (1, 3)
DEEP_MODES = ("train", "eval", "bias", "none")
DEEP_CPAD = 64


def deep_inst(HW):
    """(NPX, PL) of unet_deep_post for HW pixels per image, as unet.hip's launch chooses"""
    return (1, 1) if HW == 1 else (1, 4) if HW <= 4 else (1, 16) if HW <= 16 else (2, 32) if HW <= 64 else (8, 32)


@functools.lru_cache(maxsize=None)
def deep_data(N, Cc, HW, ks, kind):
    """ks float32 partial results [ks, N, HW, C] whose sum is plane data of `kind` (a: zero mean; c: mean / std = 8), and that float64 sum x [N, C, HW]"""
    seed = 5000 + 7 * HW + 31 * ks + 3 * Cc + N + (1000 if kind == "c" else 0)
    x = NS.plane_data(N, Cc, HW, kind, seed)
    rng = np.random.default_rng(seed + 1)
    p = (0.25 * rng.uniform(-1, 1, (ks, N, HW, Cc))).astype(np.float32)
    p[ks - 1] = (x.transpose(0, 2, 1) - p[:ks - 1].astype(np.float64).sum(0)).astype(np.float32)
    return p, p.astype(np.float64).sum(0).transpose(0, 2, 1)


def deep_params(Cc, mode):
    """(gamma, beta, ev_alpha, ev_shift) float32 [C] or None of a mode: train BN, eval (running statistics' transform), bias only (ones, bias), none"""
    rng = np.random.default_rng(77 + Cc)
    g, b = rng.uniform(0.5, 1.5, Cc).astype(np.float32), rng.uniform(-0.5, 0.5, Cc).astype(np.float32)
    if mode == "train":
        return g, b, None, None
    if mode == "eval":
        return None, None, g, b
    if mode == "bias":
        return None, None, np.ones(Cc, np.float32), b
    return None, None, None, None


def emulate_deep_post(p, HW, gamma, beta, drop_segment=None, drop_tail=False, drop_blocks=False):
    """unet_deep_post's train mode in float32 in the kernel's order: segments added in index order; a lane's pixels (pl, pl + PL, ..) summed in sequence; the PL
    lane sums added in lane order from 0; two-pass statistics.  p [ks, N, HW, C] float32 -> (x32 [N, C, HW], alpha, shift [N, C]) float32.
    The faults of the CPU test: drop_segment = z leaves segment z out; drop_tail leaves out what the 8-deep loop does not reach (z = 1 + 8 ((ks - 1) // 8) ..),
    drop_blocks what it does reach (z = 1 .. 8 ((ks - 1) // 8))."""
    f = np.float32
    ks = p.shape[0]
    NPX, PL = deep_inst(HW)
    tail0 = 1 + 8 * ((ks - 1) // 8)
    a = p[0].copy()
    for z in range(1, ks):
        if z == drop_segment or (drop_tail and z >= tail0) or (drop_blocks and z < tail0):
            continue
        a = (a + p[z]).astype(f)

    def lanes_sum(v):                                          # v [N, HW, C] -> [N, C]
        lane = np.zeros((PL,) + v[:, 0].shape, f)
        for i in range(NPX):
            for pl in range(PL):
                if pl + PL * i < HW:
                    lane[pl] = (lane[pl] + v[:, pl + PL * i]).astype(f)
        t = np.zeros_like(lane[0])
        for pl in range(PL):
            t = (t + lane[pl]).astype(f)
        return t
    mu = (lanes_sum(a) / f(HW)).astype(f)
    d = (a - mu[:, None, :]).astype(f)
    var = (lanes_sum((d * d).astype(f)) / f(HW)).astype(f)
    al = ((f(1) / np.sqrt(var + f(EPS), dtype=f)) * gamma).astype(f)
    sh = (beta - (mu * al).astype(f)).astype(f)
    return a.transpose(0, 2, 1), al, sh


def y_excess(got, x64, a64, s64, a):
    """The y metric on a stored fp16 result: what |got - act(y64)| exceeds the fp16 store's rounding by, relative to max(1, |y64|, |x alpha64|); worst over elements.
    got, x64 [N, C, HW]; a64, s64 [N, C]"""
    xa = x64 * a64[..., None]
    v = xa + s64[..., None]
    ref = act(v, a)
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    scale = np.maximum(1.0, np.maximum(np.abs(v), np.abs(xa)))
    return float((np.maximum(np.abs(got - ref) - 2.0 ** -11 * np.abs(ref) - 2.0 ** -24, 0.0) / scale).max())


def emul_error(p, x64, HW, gamma, beta):
    """e_emul of one case: the float32 emulation's y = x32 alpha32 + shift32 against float64, relative to max(1, |y64|, |x alpha64|), worst over elements"""
    x32, al, sh = emulate_deep_post(p, HW, gamma, beta)
    a64, s64 = bn_alpha_shift(x64, gamma, beta)
    y32 = (x32 * al[..., None]).astype(np.float32) + sh[..., None]
    xa = x64 * a64[..., None]
    y64 = xa + s64[..., None]
    return float((np.abs(y32.astype(np.float64) - y64) / np.maximum(1.0, np.maximum(np.abs(y64), np.abs(xa)))).max())


@functools.lru_cache(maxsize=None)
def deep_e_emul(inst, kind):
    """Worst e_emul over every case (HW, C, ks, N) of an instantiation, train mode, one data kind"""
    worst = 0.0
    for HW in DEEP_HW:
        if deep_inst(HW) != inst:
            continue
        for Cc in DEEP_C:
            g, b, _, _ = deep_params(Cc, "train")
            for ks in DEEP_KS:
                for N in DEEP_N:
                    p, x = deep_data(N, Cc, HW, ks, kind)
                    worst = max(worst, emul_error(p, x, HW, g, b))
    return worst


def deep_bound(inst, kind):
    return min(MARGIN * deep_e_emul(inst, kind), CEILING)


# ------------------------------------------------------------------------------------------------ first conv
FIRST_SHAPES = ((1, 2, 32), (1, 32, 32), (2, 6, 64), (3, 34, 96), (1, 16448, 32))
FIRST_C = (1, 3, 4)


@functools.lru_cache(maxsize=2)
def first_data(N, H, W, Cc, bias):
    """(x32, x, w16, b, ref, e32): x32 float32 [N, C, H, W] as the fp32 input holds it and x = its fp16 rounding (float32 again: what the fp16 input holds and
    what the kernel multiplies either way), w16 [64, C, 4, 4] (float32 holding fp16 values), b [64] float32 or None, the float64 conv of (x, w16, b) and e32"""
    g = torch.Generator().manual_seed(100 * H + W + 7 * Cc + N)
    x32 = torch.rand(N, Cc, H, W, generator=g).mul(2).sub(1)
    x = x32.half().float()
    w = torch.randn(64, Cc, 4, 4, generator=g).mul(0.3).half().float()
    b = torch.randn(64, generator=g).mul(0.5) if bias else None
    ref = F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=2, padding=1)
    e32 = (F.conv2d(x, w, b, stride=2, padding=1).double() - ref).abs().max().item()
    return x32, x, w, b, ref, e32
