"""float64 references, float32 models and bounds of the small pointwise / gather kernels around PAN, PPON, the WBC UNet and the image filters (CPU only: torch and
numpy, no library call).  tests/test_glue_cpu.py checks this file against torch and plants faults in the models; tests/test_gpu_glue_kernels.py holds every launch to it.

Three kinds of function:
  *_ref    float64, torch.nn.functional or plain indexing on the stored operands (fp16 values, or the fp32 values as given): what a result is compared with.
  *_model  numpy in a chosen dtype, written in the KERNEL's order of operations.  In float32 its distance from the reference is e32 / e_model, the figure a bound is
           a multiple of; in float64 it must agree with the reference (the CPU test); with fault=... it is the stand-in a planted fault lives in.
  bounds   fp16 stores: ulp16(max(|ref|, |got|)) / 2 + 8 e32 + extra, through _conv_ref.assert_within_fp16_rounding; fp32 stores: 8 e32 + extra (rounding=False).
           extra is derived where it is used (u = 2^-24, one float32 rounding):
             wb_upadd, pt mode   ulp16(|up64|) / 2: the kernel rounds the upsampled value to fp16 before the add, as the reference network does
             ppon_axpy           u (|a x| + |a x + y|): two roundings, or one with the product kept exact (contraction)
             f32_prefix_lrelu    group k: (k + 1) u sum_{i <= k} |d_i|: k additions of a running sum below sum |d_i| and one rounding for the slope
             k_filter2d          kH kW u sum |k v|: the fmaf chain
             tanh / sigmoid      _conv_ref.TRANS per evaluation (device libm: 1 - 2 ulp)
Outputs with no float32 freedom (pan_pre, wb_pre, nearest upsampling, the slab pair, wb_upadd's tf mode) are compared bit for bit.

A model reads memory as the kernel does: planes are flattened and followed by PAST, so an index the kernel failed to clamp lands in the next row or behind the plane.
"""
import numpy as np
import torch
import torch.nn.functional as F

import _conv_ref as C

U = 2.0 ** -24
PAST = float("nan")          # what lies behind a tensor in the GPU tests: a NaN guard
f32, f64 = np.float32, np.float64
BORDERS = ("constant", "reflect", "replicate", "circular")


def ratio(got, ref64, e32, extra=0.0, rounding=True):
    """worst |got - ref| / bound under _conv_ref.assert_within_fp16_rounding's bound, without raising (a non-finite value: inf)"""
    got, ref64 = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(ref64)).double()
    if not torch.isfinite(got).all():
        return float("inf")
    extra = torch.as_tensor(np.asarray(extra)).double() if not np.isscalar(extra) else extra
    bound = 8.0 * e32 + extra + (C.ulp16(torch.maximum(got.abs(), ref64.abs())) / 2 if rounding else 0.0)
    return ((got - ref64).abs() / bound).max().item()


def bits_off(got, want):
    """a bit-for-bit comparator's miss in units of the smallest difference it can see: max |got - want| / (ulp16(want) / 2); 0 when every bit agrees"""
    got, want = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(want)).double()
    if not torch.isfinite(got).all():
        return float("inf")
    return ((got - want).abs() / (C.ulp16(want) / 2)).max().item()


def rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(tuple(shape), generator=g, dtype=torch.float32) * (hi - lo) + lo


def h16(a, dt):
    """round a model's result to fp16 as the kernel's store does, back in dt"""
    return np.asarray(a, f32).astype(np.float16).astype(dt)


# ------------------------------------------------------------------------------------------------ slabs
def to_group(x):
    """[N, C <= 32, H, W] -> one zero-padded group [N, H, W, 32]"""
    N, Cc, H, W = x.shape
    out = torch.zeros(N, H, W, 32, dtype=x.dtype)
    out[..., :Cc] = x.permute(0, 2, 3, 1)
    return out


def to_slab(x):
    """[N, C, H, W] -> [ceil(C / 32), N, H, W, 32], pad channels zero"""
    N, Cc, H, W = x.shape
    G = -(-Cc // 32)
    p = torch.zeros(N, G * 32, H, W, dtype=x.dtype)
    p[:, :Cc] = x
    return p.reshape(N, G, 32, H, W).permute(1, 0, 3, 4, 2).contiguous()


def from_slab(s):
    G, N, H, W, _ = s.shape
    return s.permute(1, 0, 4, 2, 3).reshape(N, G * 32, H, W)


# ------------------------------------------------------------------------------------------------ interpolation
def _flat(x, dt):
    x = np.asarray(x, dt)
    h, w = x.shape[-2:]
    fl = x.reshape(-1, h * w)
    return np.concatenate([fl, np.full((fl.shape[0], 2 * h * w + 2 * w + 4), PAST, dt)], 1), x.shape[:-2], h, w


def _src(n_out, n_in, align, f, dt, inv=None):
    d = np.arange(n_out).astype(dt)
    if align:
        src = (dt(n_in - 1) / dt(n_out - 1) if n_out > 1 else dt(0)) * d
    else:
        inv = dt(1.0) / dt(f) if inv is None else dt(inv)
        src = np.maximum(inv * (d + dt(0.5)) - dt(0.5), dt(0))
    i0 = src.astype(np.int64)
    return i0, src - i0.astype(dt)


def bilinear_model(x, Ho, Wo, align, f=None, dt=f32, inv=None, fault=None):
    """The bilinear kernels' arithmetic (pan_upsample, pan_final, wb_upadd's pt mode, gf_out_fast, f32_bilinear_up, f32_upadd): source index in dt, the second tap clamped
    at the last row / column, hy (hx v00 + lx v01) + ly (hx v10 + lx v11).  fault 'noclamp': the second tap is y0 + 1 / x0 + 1 whatever the size."""
    fl, lead, h, w = _flat(x, dt)
    y0, ly = _src(Ho, h, align, f, dt, inv)
    x0, lx = _src(Wo, w, align, f, dt, inv)
    y1, x1 = (y0 + 1, x0 + 1) if fault == "noclamp" else (y0 + (y0 < h - 1), x0 + (x0 < w - 1))
    at = lambda yy, xx: fl[:, yy[:, None] * w + xx[None, :]]
    hy, hx, ly, lx = (dt(1) - ly)[:, None], (dt(1) - lx)[None, :], ly[:, None], lx[None, :]
    out = hy * (hx * at(y0, x0) + lx * at(y0, x1)) + ly * (hx * at(y1, x0) + lx * at(y1, x1))
    assert out.dtype == dt
    return out.reshape(*lead, Ho, Wo)


def nearest_model(x, f, div=None):
    """out[y][x] = in[y / f][x / f] (div: the divisor a fault uses instead of f)"""
    fl, lead, h, w = _flat(x, np.asarray(x).dtype)
    d = div or f
    yy, xx = np.arange(f * h) // d, np.arange(f * w) // d
    return fl[:, yy[:, None] * w + xx[None, :]].reshape(*lead, f * h, f * w)


def upsample_ref(x, f, bilinear):
    """F.interpolate(scale_factor=f) in float64: 'bilinear' with align_corners=False, or 'nearest'"""
    x = x.double()
    return F.interpolate(x, scale_factor=float(f), mode="bilinear", align_corners=False) if bilinear else F.interpolate(x, scale_factor=float(f), mode="nearest")


def pan_final_ref(raw, x, scale):
    x = x.double()
    H, W = x.shape[-2:]
    return raw.double() + (F.interpolate(x, size=(H * scale, W * scale), mode="bilinear", align_corners=True) if scale > 1 else x)


def pan_final_model(raw, x, scale, dt=f32, fault=None):
    """raw + il in dt; fault 'align': align_corners=False's source index, 'noclamp' as bilinear_model"""
    H, W = x.shape[-2:]
    if scale == 1:
        return np.asarray(raw, dt) + np.asarray(x, dt)
    if fault == "align":
        il = bilinear_model(x, H * scale, W * scale, False, scale, dt)
    else:
        il = bilinear_model(x, H * scale, W * scale, True, None, dt, fault=fault)
    return np.asarray(raw, dt) + il


# ------------------------------------------------------------------------------------------------ PAN / PPON passes
def slab_pair_ref(x32):
    """hi = fp16(x), lo = fp16((x - hi) * 2^11): x - hi and the scaling are exact in float32, so the two roundings are all there is"""
    hi = x32.half()
    lo = ((x32 - hi.float()) * 2048.0).half()
    return hi, lo


def slab_pair_model(x32, scale=2048.0):
    x = np.asarray(x32, f32)
    hi = x.astype(np.float16)
    return hi, ((x - hi.astype(f32)) * f32(scale)).astype(np.float16)


def slab_pair_values(shape, seed):
    """0, fp16-exact values (lo = 0), |x| up to 4, and values whose low part is subnormal in fp16 ((x - hi) 2^11 below 2^-14)"""
    x = rand(shape, seed, -4.0, 4.0)
    fl = x.reshape(-1)
    fl[0::7] = 0.0
    fl[1::7] = fl[1::7].half().float()
    fl[2::7] = fl[2::7].half().float() * 2.0 ** -6 + rand((fl[2::7].numel(),), seed + 1, -1, 1) * 2.0 ** -27
    return x


def axpy_ref(x, y, a):
    return float(np.float32(a)) * x.double() + y.double()


def axpy_extra(x, y, a):
    ax = float(np.float32(a)) * x.double()
    return U * (ax.abs() + (ax + y.double()).abs())


def axpy_model(x, y, a, dt=f32, fault=None):
    a = dt(np.float32(1.0 if fault == "ignore_a" else a))
    return a * np.asarray(x, dt) + np.asarray(y, dt)


def prefix_lrelu_ref(t, groups):
    """t [N, groups * gc, hw]: group k <- LeakyReLU(0.2)(d_0 + .. + d_k) (PPON's cat(d1, d1 + d2, ..) -> act), slope float32(0.2); also the bound's extra"""
    N, Cc, hw = t.shape
    d = t.double().reshape(N, groups, Cc // groups, hw)
    run = torch.cumsum(d, 1)
    ref = torch.where(run > 0, run, float(np.float32(0.2)) * run)
    k = torch.arange(groups, dtype=torch.float64).view(1, groups, 1, 1)
    extra = (k + 1) * U * torch.cumsum(d.abs(), 1)
    return ref.reshape(N, Cc, hw), extra.reshape(N, Cc, hw)


def prefix_lrelu_model(t, groups, dt=f32, fault=None):
    """the kernel's loop; fault 'feedback': the activated value goes back into the running sum"""
    N, Cc, hw = t.shape
    d = np.asarray(t, dt).reshape(N, groups, Cc // groups, hw).copy()
    run = np.zeros_like(d[:, 0])
    for k in range(groups):
        run = run + d[:, k]
        d[:, k] = np.where(run > 0, run, dt(np.float32(0.2)) * run)
        if fault == "feedback":
            run = d[:, k]
    return d.reshape(N, Cc, hw)


def act_ref(v, act):
    """f32_act in v's dtype: 0 none, 1 LeakyReLU(float32(0.2)), 2 ReLU, 3 tanh, 4 sigmoid"""
    return [v, torch.where(v > 0, v, float(np.float32(0.2)) * v), F.relu(v), torch.tanh(v), torch.sigmoid(v)][act]


# ------------------------------------------------------------------------------------------------ WBC UNet passes
def wb_pre_ref(x):
    """[N, C, H, W] -> [N, H, W, 32]: channel kx * C + c of pixel (y, x) = in[c][y][x + kx - 3], zero outside the row and beyond 7 C channels"""
    return wb_pre_model(x)


def wb_pre_model(x, off=-3, order="kx*C+c"):
    x = torch.as_tensor(x)
    N, Cc, H, W = x.shape
    out = torch.zeros(N, H, W, 32, dtype=x.dtype)
    p = F.pad(x, (8, 8))
    for kx in range(7):
        for c in range(Cc):
            j = kx * Cc + c if order == "kx*C+c" else c * 7 + kx
            out[..., j] = p[:, c, :, 8 + kx + off:8 + kx + off + W]
    return out


def tf_up_ref(x):
    """tf_2xupsample_bilinear (WBCNet_arch.py:127-138) in x's dtype"""
    b, c, h, w = x.shape
    out = torch.zeros(b, c, 2 * h, 2 * w, dtype=x.dtype)
    out[:, :, ::2, ::2] = x
    p = F.pad(x, (0, 1, 0, 1), mode="replicate")
    out[:, :, 1::2, ::2] = (p[:, :, :-1, :-1] + p[:, :, 1:, :-1]) / 2
    out[:, :, ::2, 1::2] = (p[:, :, :-1, :-1] + p[:, :, :-1, 1:]) / 2
    out[:, :, 1::2, 1::2] = (p[:, :, :-1, :-1] + p[:, :, 1:, 1:]) / 2
    return out


def tf_up_model(x, dt=f32, fault=None):
    """the kernels' form: a = x[Y >> 1][X >> 1], b = its lower / right / diagonal neighbour clamped to the border, (a + b) / 2 where Y or X is odd.
    fault 'right': odd / odd takes the right neighbour; 'zero': a neighbour beyond the border reads zero"""
    x = np.asarray(x, dt)
    h, w = x.shape[-2:]
    Y, X = np.arange(2 * h), np.arange(2 * w)
    i, j = Y >> 1, X >> 1
    i2, j2 = np.where(Y & 1, np.minimum(i + 1, h - 1), i), np.where(X & 1, np.minimum(j + 1, w - 1), j)
    a = x[..., i[:, None], j[None, :]]
    if fault == "right":
        b = np.where((X & 1)[None, :] > 0, x[..., i[:, None], j2[None, :]], x[..., i2[:, None], j[None, :]])
    else:
        b = x[..., i2[:, None], j2[None, :]]
    if fault == "zero":
        out_y, out_x = (Y & 1) & (i + 1 > h - 1), (X & 1) & (j + 1 > w - 1)
        b = np.where((out_y[:, None] | out_x[None, :]) > 0, dt(0), b)
    odd = ((Y[:, None] | X[None, :]) & 1) > 0
    return np.where(odd, (a + b) / dt(2), a)


def upadd16_ref(src, skip, tf):
    """what the fp16 kernel is held to: pt mode (float64 reference, extra = ulp16(|up64|) / 2); tf mode: fp16(fp16(up) + skip), one value -- (a + b) / 2 is exact in float32"""
    if tf:
        up = tf_up_ref(src.float()).half()
        return (up.float() + skip.float()).half(), None
    up = upsample_ref(src, 2, True)
    return up + skip.double(), C.ulp16(up) / 2


def upadd16_model(src, skip, tf, fault=None):
    h, w = src.shape[-2:]
    up = tf_up_model(src, f32, fault) if tf else bilinear_model(src, 2 * h, 2 * w, False, 2, f32, fault=fault)
    return h16(h16(up, f32) + np.asarray(skip, f32), f32)


# ------------------------------------------------------------------------------------------------ guided filter
def _refl(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def gf_model(x, y, ks, eps, dt=f32, xhr=None, fault=None):
    """The guided-filter kernels in their order (gf_ab / gf_ab_r, then gf_out / gf_out_r or gf_out_fast), planes [P, H, W]: s += v * k tap by tap in (dy, dx) order, / sn;
    cov and var as differences; cov / (var + eps); the second box pass or the align_corners=True interpolation; mean_A x + mean_b.
    faults: 'replicate' (border), 'b_mean_y' (b = mean_y - A mean_y), 'no_eps', 'box_ks3' (the taps weigh float32(1 / 9) whatever ks; N keeps the window's own value)"""
    x, y = np.asarray(x, dt), np.asarray(y, dt)
    H, W = x.shape[-2:]
    r = ks // 2
    k = dt(np.float32(1.0 / (ks * ks)))
    kt = dt(np.float32(1.0 / 9.0)) if fault == "box_ks3" else k
    idx = (lambda i, n: np.clip(i, 0, n - 1)) if fault == "replicate" else _refl

    def box(*vs):
        s, sn = [np.zeros_like(vs[0]) for _ in vs], dt(0)
        for dy in range(-r, r + 1):
            iy = idx(np.arange(H) + dy, H)
            for dx in range(-r, r + 1):
                ix = idx(np.arange(W) + dx, W)
                for q, v in enumerate(vs):
                    s[q] = s[q] + v[:, iy[:, None], ix[None, :]] * kt
                sn = sn + k
        return [q / sn for q in s]
    with np.errstate(all="ignore"):          # (the 'no_eps' fault divides 0 by 0 on a flat plane)
        mx, my, mxy, mxx = box(x, y, x * y, x * x)
        cov, var = mxy - mx * my, mxx - mx * mx
        A = cov / (var + (dt(0) if fault == "no_eps" else dt(np.float32(eps))))
        B = my - A * (my if fault == "b_mean_y" else mx)
        if xhr is None:
            mA, mB = box(A, B)
            out = mA * x + mB
        else:
            xhr = np.asarray(xhr, dt)
            Hh, Wh = xhr.shape[-2:]
            out = bilinear_model(A, Hh, Wh, True, None, dt) * xhr + bilinear_model(B, Hh, Wh, True, None, dt)
    assert out.dtype == dt
    return out


def gf_ref(x, y, ks, eps, xhr=None):
    """guided_filter (utils.py:549-626) in float64 with torch: reflect-padded box means (N = 1 for a normalised box), eps the float32 value the kernel receives"""
    x, y = x.double()[:, None], y.double()[:, None]
    r = ks // 2
    box = lambda v: F.avg_pool2d(F.pad(v, (r, r, r, r), mode="reflect") if r else v, ks, 1)
    mx, my = box(x), box(y)
    A = (box(x * y) - mx * my) / (box(x * x) - mx * mx + float(np.float32(eps)))
    B = my - A * mx
    if xhr is None:
        return (box(A) * x + box(B))[:, 0]
    xhr = xhr.double()[:, None]
    up = lambda v: F.interpolate(v, size=xhr.shape[-2:], mode="bilinear", align_corners=True)
    return (up(A) * xhr + up(B))[:, 0]


def gf_operands(family, P, H, W, seed):
    """(x guidance, y input) float32 holding fp16 values: uniform noise | a flat plane | 1 + 2^-9 noise (the var cancellation) | a ramp"""
    n = rand((P, H, W), seed)
    yv = rand((P, H, W), seed + 1)
    if family == "noise":
        x = n
    elif family == "flat":
        x = torch.full((P, H, W), 0.75)
    elif family == "near1":
        x = 1.0 + n * 2.0 ** -9
    else:
        x = (torch.arange(H).view(1, H, 1) * 0.05 + torch.arange(W).view(1, 1, W) * 0.03 + torch.arange(P).view(P, 1, 1) * 0.01 - 0.5).float()
    return x.half().float(), yv.half().float()


GF_FAMILIES = ("noise", "flat", "near1", "ramp")


# ------------------------------------------------------------------------------------------------ filter2D
def _f2d_src(i, n, border, shift=0):
    inside = (i >= 0) & (i < n)
    if border == 1:
        o = np.where(i < 0, -i, 2 * n - 2 - i)
    elif border == 2:
        o = np.where(i < 0, 0, n - 1)
    elif border == 3:
        o = (i + shift) % n
    else:
        o = np.full_like(i, -1)
    return np.where(inside, i, o)


def f2d_model(x, k, pl, pt, border, dt=f32, fault=None):
    """k_filter2d: acc = fmaf(k[a][b], v, acc) over (a, b) in row order, v the border mode's source value (0 outside for constant).
    faults: 'swap' (pad_left / pad_top swapped), 'circ1' (circular source off by one), 'conv' (the kernel flipped: convolution)"""
    x, k = np.asarray(x, dt), np.asarray(k, dt)
    H, W = x.shape[-2:]
    kH, kW = k.shape
    if fault == "swap":
        pl, pt = min(pt, kW - 1), min(pl, kH - 1)
    if fault == "conv":
        k = k[::-1, ::-1]
    acc = np.zeros_like(x)
    for a in range(kH):
        sy = _f2d_src(np.arange(H) + a - pt, H, border, 1 if fault == "circ1" else 0)
        for b in range(kW):
            sx = _f2d_src(np.arange(W) + b - pl, W, border, 1 if fault == "circ1" else 0)
            v = np.where((sy[:, None] < 0) | (sx[None, :] < 0), dt(0), x[..., np.maximum(sy, 0)[:, None], np.maximum(sx, 0)[None, :]])
            acc = (f64(k[a, b]) * v.astype(f64) + acc.astype(f64)).astype(dt)          # fmaf: the product exact, one rounding
    return acc


def f2d_ref(x, k, pl, pt, border):
    """filter2D (utils.py:484-535) in float64: F.pad(x, (pl, pr, pt, pb), mode) then a cross-correlation; also sum |k v|, what the fmaf chain's bound scales with"""
    kH, kW = k.shape
    x, k = x.double()[:, None], k.double()[None, None]
    pad = lambda v: F.pad(v, (pl, kW - 1 - pl, pt, kH - 1 - pt), mode=BORDERS[border])
    return F.conv2d(pad(x), k)[:, 0], F.conv2d(pad(x.abs()), k.abs())[:, 0]


def f2d_kernel(kH, kW, seed):
    return rand((kH, kW), seed, -1, 1) / float(np.sqrt(kH * kW))


# ------------------------------------------------------------------------------------------------ what each family is judged by: (ref64, e32, extra)
def _e(model, ref):
    return float((torch.as_tensor(np.asarray(model, f64)) - ref).abs().max())


def judge_upsample(src, f):
    ref = upsample_ref(src, f, True)
    h, w = src.shape[-2:]
    return ref, _e(bilinear_model(src, f * h, f * w, False, f), ref), 0.0


def judge_final(raw, x, scale):
    ref = pan_final_ref(raw, x, scale)
    return ref, _e(pan_final_model(raw, x, scale), ref), 0.0


def judge_upadd_pt(src, skip, fp16):
    """fp16: the slab kernel (the upsampled value rounded to fp16 before the add); else the fp32 kernel"""
    up = upsample_ref(src, 2, True)
    h, w = src.shape[-2:]
    m = bilinear_model(src, 2 * h, 2 * w, False, 2)
    if fp16:
        return up + skip.double(), _e(m, up), C.ulp16(up) / 2
    ref = up + skip.double()
    return ref, _e(m + np.asarray(skip, f32), ref), 0.0


def judge_gf(x, y, ks, eps, xhr=None):
    ref = gf_ref(x, y, ks, eps, xhr)
    return ref, _e(gf_model(x, y, ks, eps, f32, xhr), ref), 0.0


def judge_f2d(x, k, pl, pt, border):
    ref, sabs = f2d_ref(x, k, pl, pt, border)
    return ref, _e(f2d_model(x, k, pl, pt, border), ref), k.shape[0] * k.shape[1] * U * sabs


# ------------------------------------------------------------------------------------------------ the case lists (h x w of the kernel's INPUT grid)
UPS_SIZES = ((1, 1), (1, 7), (7, 1), (5, 7), (17, 33))
FINAL_SIZES = ((1, 1), (1, 5), (5, 7), (16, 32))
UPADD_SIZES = ((1, 1), (1, 4), (3, 5), (8, 10))
GF_SIZES = ((2, 2), (5, 7), (17, 23))
F2D_KERNELS = ((1, 1, 0, 0), (3, 3, 1, 1), (1, 5, 2, 0), (5, 1, 0, 2), (4, 4, 1, 2), (4, 4, 2, 1), (5, 7, 3, 2))          # kH, kW, pad_left, pad_top
F2D_PLANES = ((2, 3), (7, 5), (17, 23))


def f2d_accepts(H, W, kH, kW, pl, pt, border):
    """F.pad's limits, as innfer_filter2d states them: a reflection needs pad < size, a circular pad <= size"""
    py, px = max(pt, kH - 1 - pt), max(pl, kW - 1 - pl)
    return not ((border == 1 and (py >= H or px >= W)) or (border == 3 and (py > H or px > W)))
