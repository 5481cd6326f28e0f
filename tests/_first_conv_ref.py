"""float64 references, case lists and comparators for the launches every RRDBNet / SRResNet / SRVGGNetCompact forward starts with -- first_conv_mfma and
first_conv_mfma_prelu (csrc/conv_first.hip, conv_first_body.inc) -- and for the slab passes of csrc/net.hip between the convs (slab_upsample_nearest,
slab_pixel_shuffle, slab_input_map, slab_input_map_split), each reached alone through innfer_first_conv / innfer_slab_*.  No GPU here:
tests/test_first_conv_cpu.py holds these references to the torch modules they restate and shows that the comparators reject planted faults at cases of the GPU
test's own list; tests/test_gpu_first_conv.py holds the kernels to them.

Reference of the first conv: F.conv2d in float64 on the operands the kernel is given -- the fp32 weights unrounded, the input as stored -- + bias + act
(0 none, 1 LeakyReLU(0.2), 2 ReLU, 8 f >= 0 ? f : slope[c] f).  A uint8 image is np2tensor restated in numpy float32 (/255, channel flip, optional
((x - 0.5) * 2).clip(-1, 1), optional fp16 rounding): the separate pass is the contract, and the kernel must equal the planar launch on that tensor bit for bit.

e of a case = max(e32, e_split), both measured here against that reference, never against the kernel:
  e32      the error of a float32 F.conv2d (+ the activation in float32);
  e_split  the error of split_model, a numpy model of the arithmetic the kernel declares: w = wh + wl, x = xh + xl with fp16 heads and fp16 remainders (NOT scaled:
           below 2^-14 they are fp16 subnormals and must survive as such), wh xh + wl xh + wh xl accumulated in float32, the 2^-22 term wl xl dropped.

Bounds (none is taken from the code under test):
  fp16 store     |got - ref| <= ulp16(max(|ref|, |got|)) / 2 + 8 e           (the store's rounding + the margin an emulation figure gets in this project)
  split pair     read as hi + lo 2^-11:  8 e + pair_term,  pair_term(v) = ulp16(2^10 ulp16(v)) 2^-12: lo = fp16((f - hi) 2^11) with |f - hi| <= ulp16(f) / 2, so
                 |(f - hi) 2^11| <= 2^10 ulp16(f), its fp16 rounding errs by at most half an ulp16 of that, and the 2^-11 brings it back.  Taken at
                 max(|ref|, |got|) like the fp16 store's term: f may sit one binade above ref.
  slab_input_map        pass_bound of tests/_pass_kernels_ref.py
  slab_input_map_split  4 * 2^-24 * mag + pair_term
  slab_upsample_nearest, slab_pixel_shuffle: bit for bit.

Data kinds: A  x uniform in [-1, 1), w 0.2 N(0, 1);  B  x uniform in +-2^-4 and w 0.05 N(0, 1) -- every xl and every wl an fp16 subnormal, outputs ~1e-2 whose
fp16 ulp (2^-17) is below what lost low parts cost (~1e-5): the kind that makes them visible, most sharply in a split-output case;  U  uint8 images.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _pass_kernels_ref as P
from _pass_kernels_ref import bits16, from_slab, pass_bound, pass_ref, to_slab, ulp16, worst_ratio  # noqa: F401  (shared, not copied)

f16, f32, f64 = np.float16, np.float32, np.float64

FIRST_ROWS = 16                   # rows of a workgroup (conv_first.hip)
FIRST_HW = ((1, 1), (1, 17), (2, 16), (15, 63), (16, 64), (17, 65), (18, 15), (31, 33), (33, 130))
FIRST_C = (1, 3, 4, 7, 8)         # STEPS 1, 1, 2, 2, 3
FIRST_K = (32, 64)
ACTS = (0, 1, 2, 8)
Case = collections.namedtuple("Case", "K C H W N kind act")


def form(K, Cc, in_kind, act):
    """The instantiation first_conv_launch picks: (K, STEPS = ceil(9 in_nc / 32), FAST16 = planar fp16 input, PReLU); in_kind 'f16' | 'f32' | 'u8'"""
    return (K, -(-9 * Cc // 32), in_kind == "f16", act == 8)


ALL_FORMS = frozenset((K, st, fast, pre) for K in FIRST_K for st in (1, 2, 3) for fast in (False, True) for pre in (False, True))


def first_cases(K=None, Cc=None):
    """The GPU test's case list: every (K, in_nc) at every H x W; the activation, the data kind and the batch rotate so that each (K, in_nc) meets all four
    activations under both kinds, and N = 3 at every third case.  Each case is launched with planar fp16 AND planar fp32 input (case_forms)."""
    out = []
    for i, (k, c) in enumerate((k, c) for k in FIRST_K for c in FIRST_C):
        for j, (H, W) in enumerate(FIRST_HW):
            if (K is None or k == K) and (Cc is None or c == Cc):
                out.append(Case(k, c, H, W, 3 if (i + j) % 3 == 0 else 1, "AB"[(j // 4 + i) % 2], ACTS[(i + j) % 4]))
    return out


def case_forms(case):
    return {form(case.K, case.C, "f16", case.act), form(case.K, case.C, "f32", case.act)}


# ------------------------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=4)
def first_data(case):
    """(x32, x16, w, b, slope): x32 float32 [N, C, H, W] as the fp32 input holds it, x16 = its fp16 rounding (float32 again), w [K, C, 3, 3] and b [K] float32,
    slope [K] float32 in [-0.5, 0.5] with a 0 and a 1 among them (act 8; None otherwise)"""
    K, Cc, H, W, N, kind, a = case
    rng = np.random.default_rng(1000 * K + 100 * Cc + 7 * H + W + 13 * N + (50000 if kind == "B" else 0))
    sx, sw, sb = (1.0, 0.2, 0.3) if kind == "A" else (2.0 ** -4, 0.05, 0.01)
    x32 = rng.uniform(-sx, sx, (N, Cc, H, W)).astype(f32)
    w = (sw * rng.standard_normal((K, Cc, 3, 3))).astype(f32)
    b = (sb * rng.standard_normal(K)).astype(f32)
    slope = None
    if a == 8:
        slope = rng.uniform(-0.5, 0.5, K).astype(f32)
        slope[3], slope[K - 2] = 0.0, 1.0
    return x32, x32.astype(f16).astype(f32), w, b, slope


def u8_images(N, H, W, Cc, seed=0):
    """uint8 HWC images [N, H, W, C] with 0 and 255 among the values"""
    img = np.random.default_rng(4242 + seed + 100 * H + W + Cc).integers(0, 256, (N, H, W, Cc), dtype=np.uint8)
    img.reshape(-1)[:2] = (0, 255)
    return img


def np2tensor_np(img, normalize, round16, flip="np2tensor"):
    """np2tensor (utils/utils.py; oracle/convert.py) in numpy float32 on [N, H, W, C] uint8 -> [N, C, H, W] float32: / 255, BGR -> RGB (C % 3 == 0: reversed;
    C == 4: channels 0 and 2 swapped, alpha in place), optional [-1, 1] normalisation, optional rounding to fp16 (`.half()`).
    flip = "all4": the fault of the CPU test -- BGRA reversed as four channels."""
    t = (img.astype(f32) / f32(255)).transpose(0, 3, 1, 2)
    Cc = t.shape[1]
    if Cc % 3 == 0 or (Cc == 4 and flip == "all4"):
        t = t[:, ::-1]
    elif Cc == 4:
        t = t[:, [2, 1, 0, 3]]
    if normalize:
        t = np.clip((t - f32(0.5)) * f32(2), -1, 1)
    if round16:
        t = t.astype(f16).astype(f32)
    return np.ascontiguousarray(t, f32)


# ------------------------------------------------------------------------------------------------ references
def act_ref(v, a, slope=None):
    if a == 8:
        return np.where(v >= 0, v, np.asarray(slope, v.dtype)[None, :, None, None] * v)
    return P.act(v, a)


def conv_ref(x, w, b, a, slope=None):
    """float64 act(conv3x3(x, w) + b), zero padding 1; x [N, C, H, W], w [K, C, 3, 3] (any float type: taken as they are)"""
    r = F.conv2d(torch.as_tensor(x).double(), torch.as_tensor(w).double(), torch.as_tensor(b).double(), padding=1).numpy()
    return act_ref(r, a, None if slope is None else np.asarray(slope, f64))


def conv_f32(x, w, b, a, slope=None):
    """The same in float32 (e32)"""
    r = F.conv2d(torch.as_tensor(x), torch.as_tensor(w), torch.as_tensor(b), padding=1).numpy()
    if a == 1:
        return np.maximum(r, f32(0.2) * r)
    return act_ref(r, a, slope)


def patches(x, fault=None):
    """x [N, C, H, W] -> the zero-padded 3 x 3 windows [N, C, 3, 3, H, W]: element (r, s, y, x) = x[y + r - 1][x + s - 1].
    Faults: "top" -- the top-row mask missing, row -1 reads row 0; "strip" -- the right tap of the last column of a 16-column strip is taken 16 columns to
    the left (the neighbouring strip's lane)."""
    N, Cc, H, W = x.shape
    p = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    if fault == "top":
        p[:, :, 0, 1:-1] = x[:, :, 0]
    q = np.stack([np.stack([p[:, :, r:r + H, s:s + W] for s in range(3)], 2) for r in range(3)], 2)
    if fault == "strip":
        for xc in range(15, W - 1, 16):
            q[:, :, :, 2, :, xc] = q[:, :, :, 1, :, xc - 15]
    return q


def split16(v, flush=False):
    """fp16 head and fp16 remainder (float32 arrays); flush: remainders below 2^-14 (the fp16 subnormals) lost"""
    h = v.astype(f16).astype(f32)
    lo = (v - h).astype(f16).astype(f32)
    if flush:
        lo = np.where(np.abs(lo) < 2.0 ** -14, f32(0), lo)
    return h, lo


def split_model(x, w, b, a, slope=None, fault=None):
    """The arithmetic first_conv_mfma declares, in numpy: wh xh + wl xh + wh xl in float32 (+ bias, activation in float32) -> float32 [N, K, H, W] before the store.
    (An fp16-representable x has xl = 0: the planar fp16 input.)  Faults of the CPU test: "wl_xh", "xl_wh" (the term dropped), "flush" (subnormal low parts
    lost), "taps" (kernel rows and columns transposed), "top", "strip" (patches), "slope" (the slope of channel c ^ 4)."""
    N, Cc, H, W = x.shape
    K = w.shape[0]
    if fault == "taps":
        w = np.ascontiguousarray(w.transpose(0, 1, 3, 2))
    q = patches(x, fault).reshape(N, Cc * 9, H * W)
    wm = w.reshape(K, Cc * 9)
    xh, xl = split16(q, fault == "flush")
    wh, wl = split16(wm, fault == "flush")
    acc = np.matmul(wh, xh)
    if fault != "wl_xh":
        acc = acc + np.matmul(wl, xh)
    if fault != "xl_wh":
        acc = acc + np.matmul(wh, xl)
    v = (acc + b[None, :, None]).astype(f32).reshape(N, K, H, W)
    if a == 1:
        return np.maximum(v, f32(0.2) * v)
    if a == 8 and fault == "slope":
        slope = slope[np.arange(K) ^ 4]
    return act_ref(v, a, slope).astype(f32)


def to_pair(v):
    """float32 -> the (hi, lo) fp16 pair of the fp32-accurate mode: hi = fp16(v), lo = fp16((v - hi) 2^11)"""
    v = np.asarray(v, f32)
    hi = v.astype(f16)
    return hi, ((v - hi.astype(f32)) * f32(2048)).astype(f16)


def pair_value(hi, lo):
    """The pair read back: hi + lo 2^-11 (float64, exact)"""
    return np.asarray(hi, f64) + np.asarray(lo, f64) / 2048.0


def data_e(x, w, b, a, slope=None):
    """e = max(e32, e_split) of one conv on given operands"""
    ref = conv_ref(x, w, b, a, slope)
    return max(float(np.abs(conv_f32(x, w, b, a, slope).astype(f64) - ref).max()), float(np.abs(split_model(x, w, b, a, slope).astype(f64) - ref).max()))


_E = {}


def case_e(case, which):
    """e of a case on its fp16-representable image (which = 16) or its float32 image (32), cached"""
    key = (case, which)
    if key not in _E:
        x32, x16, w, b, slope = first_data(case)
        _E[key] = data_e(x16 if which == 16 else x32, w, b, case.act, slope)
    return _E[key]


# ------------------------------------------------------------------------------------------------ bounds
def store_bound(ref, got, e):
    return ulp16(np.maximum(np.abs(ref), np.abs(got))) / 2 + 8 * e


def pair_term(v):
    return ulp16(2.0 ** 10 * ulp16(v)) * 2.0 ** -12


def pair_bound(ref, got, e):
    return 8 * e + pair_term(np.maximum(np.abs(ref), np.abs(got)))


def map_split_bound(ref, got, mag):
    return 4 * 2.0 ** -24 * mag + pair_term(np.maximum(np.abs(ref), np.abs(got)))


# ------------------------------------------------------------------------------------------------ the exact passes
SLAB_GRIDS = ((1, 1), (3, 5), (7, 11))
UPSAMPLE_CASES = tuple((f, g) for f in (3, 2) for g in (1, 2))                  # (factor, groups)
SHUFFLE_CASES = ((32, 2), (64, 2), (64, 3))                                      # (nf, r)
MAP_C = (32, 64, 40)


def upsample_ref(x, f, fault=None):
    """Nearest-neighbour f x of [N, C, H, W]: out[Y][X] = x[Y // f][X // f] ("up": the fault, Y / f rounded up)"""
    N, Cc, H, W = x.shape
    iy = np.arange(H * f) // f
    if fault == "up":
        iy = np.minimum(-(-np.arange(H * f) // f), H - 1)
    return x[:, :, iy][:, :, :, np.arange(W * f) // f]


def shuffle_ref(x, r, fault=None):
    """nn.PixelShuffle(r): out[n, c, y r + i, x r + j] = x[n, c r^2 + i r + j, y, x] ("ij": the fault, i r + j transposed)"""
    N, Cr, H, W = x.shape
    v = x.reshape(N, Cr // (r * r), r, r, H, W)
    if fault == "ij":
        v = v.transpose(0, 1, 3, 2, 4, 5)
    return v.transpose(0, 1, 4, 2, 5, 3).reshape(N, Cr // (r * r), H * r, W * r)


def map_data(Cc, N, H, W, seed=0):
    """(x32 [N, C, H, W] float32, alpha [C] in +-[0.5, 1.5], shift [C] in [-0.5, 0.5])"""
    rng = np.random.default_rng(900 + Cc + 10 * N + 100 * H + W + seed)
    x = rng.normal(0.0, 1.5, (N, Cc, H, W)).astype(f32)
    al = (rng.uniform(0.5, 1.5, Cc) * rng.choice([-1.0, 1.0], Cc)).astype(f32)
    return x, al, rng.uniform(-0.5, 0.5, Cc).astype(f32)


# ------------------------------------------------------------------------------------------------ refusals: one launch-free call each
def refusals(L):
    """(what, return code, expected code) of calls the entry points must refuse before anything is uploaded or launched (no pointer is ever dereferenced)"""
    p, lib, big = 0x1000, L.lib, 1 << 40
    w = np.zeros((64, 8, 3, 3), f32).ctypes.data
    sl = np.zeros(64, f32).ctypes.data
    INV, UNS = L.ERR_INVALID, L.ERR_UNSUPPORTED

    def fc(i=p, dt=0, N=1, Cc=3, H=4, W=4, wt=w, K=64, a=0, s=None, d=p, gs=big, lo=0, d2=None, gs2=0, lo2=0):
        return lib.innfer_first_conv(i, dt, 0, 1, N, Cc, H, W, wt, None, K, a, s, d, gs, lo, d2, gs2, lo2, None)
    yield "first_conv: null input", fc(i=None), INV
    yield "first_conv: null weights", fc(wt=None), INV
    yield "first_conv: null slab", fc(d=None), INV
    yield "first_conv: dtype", fc(dt=3), INV
    yield "first_conv: shape", fc(H=0), INV
    yield "first_conv: group stride", fc(N=2, H=5, W=7, gs=2 * 5 * 7 * 32 - 1), INV
    yield "first_conv: second group stride", fc(N=2, H=5, W=7, d2=p, gs2=2 * 5 * 7 * 32 - 1), INV
    yield "first_conv: K 48", fc(K=48), UNS
    yield "first_conv: K 128", fc(K=128), UNS
    yield "first_conv: in_nc 0", fc(Cc=0), UNS
    yield "first_conv: in_nc 9", fc(Cc=9), UNS
    yield "first_conv: act 3", fc(a=3), UNS
    yield "first_conv: act 8 without slopes", fc(a=8), INV
    yield "first_conv: act 8 with a split output", fc(a=8, s=sl, lo=2 * big), UNS
    yield "first_conv: lo inside the hi slab", fc(gs=1 << 20, lo=1 << 20), INV
    yield "first_conv: lo for one slab only", fc(lo=2 * big, d2=p, gs2=big), INV
    for name, fn in (("slab_upsample_nearest", lib.innfer_slab_upsample_nearest), ("slab_pixel_shuffle", lib.innfer_slab_pixel_shuffle)):
        def sp(s=p, sg=big, d=p, dg=big, n=64 if "shuffle" in name else 2, N=2, H=3, W=5, f=2, lo=0):
            return fn(s, sg, d, dg, n, N, H, W, f, lo, None)
        yield name + ": null source", sp(s=None), INV
        yield name + ": null destination", sp(d=None), INV
        yield name + ": factor 0", sp(f=0), INV
        yield name + ": shape", sp(W=0), INV
        yield name + ": source group stride", sp(sg=2 * 3 * 5 * 32 - 1), INV
        yield name + ": destination group stride", sp(dg=2 * 3 * 5 * 4 * 32 - 1), INV
        yield name + ": lo inside the slab", sp(sg=1 << 20, dg=1 << 20, lo=1 << 20), INV
    yield "slab_pixel_shuffle: nf 36", lib.innfer_slab_pixel_shuffle(p, big, p, big, 36, 1, 3, 5, 2, 0, None), INV
    yield "slab_pixel_shuffle: nf 0", lib.innfer_slab_pixel_shuffle(p, big, p, big, 0, 1, 3, 5, 2, 0, None), INV
    yield "slab_upsample_nearest: groups 0", lib.innfer_slab_upsample_nearest(p, big, p, big, 0, 1, 3, 5, 2, 0, None), INV

    def im(s=p, d=p, gs=3200, lo=0, Cc=64, a=1):
        return lib.innfer_slab_input_map(s, d, gs, lo, Cc, None, None, a, None)
    yield "slab_input_map: null source", im(s=None), INV
    yield "slab_input_map: null destination", im(d=None), INV
    yield "slab_input_map: C 0", im(Cc=0), INV
    yield "slab_input_map: act 3", im(a=3), INV
    yield "slab_input_map: group of half a pixel", im(gs=3200 + 16), INV
    yield "slab_input_map: lo inside the slab", im(lo=2 * 3200 - 32), INV
