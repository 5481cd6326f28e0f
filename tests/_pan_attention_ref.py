"""PAN's FSA attention in numpy (CPU only: numpy and torch, no library call), and the cases of tests/test_pan_fsa_cpu.py and tests/test_gpu_pan_fsa.py.

    out[i][c] = sum_j softmax_j(f_i . g_j) h_j[c]          f, g: [Np][5], h: [Np][40], fp32, the biases added (one fp32 add, as the kernels add them)

exact(f, g, h)          the operation in float64.
model(f, g, h, split)   pan_attn_prep + pan_attention_mfma<split> (csrc/pan.hip): the kernel's DECLARED roundings in the kernel's key order, float64 everywhere else
                        (the MFMAs' fp32 sums, v_exp_f32 and the fp32 rescale are not modelled: 2^-24-sized, covered by the margin of 8):
  * f' = fp32(f * log2 e); f', g as fp16 pairs x = xh + xl' 2^-11, xl' = fp16((x - xh) * 2^11);
  * s = gh . fh + gh . fp16(fl' 2^-11) + gl' . fp16(fh 2^-11): the cross operands carry the 2^-11 in fp16, the 2^-22 term (gl' . fl') is absent;
  * keys in pairs of 64, in order; keys >= Np score -inf.  The first pair takes its own maximum as delta from m = 0 (negative where every score is), later pairs
    delta = max(pair max - m, 0) per query; m += delta, the accumulators and the sum are multiplied by 2^-delta;
  * p = rtz16(2^(s - m)) (round toward zero to fp16, denormals kept); h = fp16(h); o += p h, sum += p: the SAME rounded p in both;
  * split: pl = rtz16((2^(s - m) - p) * 2^11), h = hh + hl' 2^-11; o += p hh + 2^-11 (p hl' + pl hh), sum += p + 2^-11 pl (the pl hl' term is absent);
  * out = o / sum.
model(..., fault=...)   the same with one fault planted -- what tests/test_pan_fsa_cpu.py proves the sweep would see:
  perm            the keys of h permuted j ^ 4 within a pair against the keys of p (a wrong row -> key assignment of the score tiles);
  unmasked        the first padding key of a ragged pair admitted: score 0 (its g row is zero), value 0, counted in the sum;
  droptail        the ragged last 32-key block masked altogether;
  norescale       the maximum moves but the accumulators and the sum are not rescaled;
  first_pair_m0   the first pair's delta clamped at 0 like the later ones.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

CQ, C, ROW = 5, 40, 64                    # channels of f / g, of h, floats per fgh row
LOG2E = np.float32(1.44269504088896340736)
NP_SWEEP = (1, 2, 31, 32, 33, 64, 65, 96, 127, 129, 257, 513, 1057)
NP_BATCH = (33, 129, 513)                 # N = 3 here: each image bit-equal to its own N = 1 launch
FAMILIES = ("flat", "peaked", "ramp", "negative")
FAULTS = ("perm", "unmasked", "droptail", "norescale", "first_pair_m0")
MARGIN = 8.0                              # what an emulation figure gets in this project


@dataclass(frozen=True)
class Case:
    family: str
    Np: int
    seed: int

    def __str__(self):
        return f"{self.family}-{self.Np}"


def cases():
    """The sweep: every key count x every family, seeded.  The single list both test files iterate."""
    return [Case(fam, n, 1000 * (k + 1) + n) for k, fam in enumerate(FAMILIES) for n in NP_SWEEP]


def fault_acts(fault, c):
    """Whether the planted fault can change this case at all."""
    ragged = c.Np % 64 != 0
    return {"perm": c.Np >= 2, "unmasked": ragged, "droptail": c.Np % 32 != 0 and c.Np > 32, "norescale": c.Np > 64,
            "first_pair_m0": c.family == "negative"}[fault]


@functools.lru_cache(maxsize=None)
def operands(c):
    """(fgh rows [Np][64] fp32 with NaN in columns 50 .. 63, bf, bg, bh, f, g, h): the rows and biases the kernels take, and f / g / h = fp32(row + bias).
    |f|, |g| <= 6, h uniform in +-1 (the targets; the rows are target - bias rounded to fp32)."""
    r = np.random.default_rng(c.seed)
    n = c.Np
    if c.family == "flat":               # what the networks show: scores within +-0.45
        f, g = r.uniform(-0.3, 0.3, (n, CQ)), r.uniform(-0.3, 0.3, (n, CQ))
    elif c.family == "peaked":           # row spread of tens of nats: a handful of keys carry the row
        f, g = r.uniform(-4, 4, (n, CQ)), r.uniform(-4, 4, (n, CQ))
    elif c.family == "ramp":             # s_ij = b_i a_j, a ascending over +-6: b > 0 moves the maximum in every pair, b < 0 sets it in the first
        u = r.uniform(0.2, 1.0, CQ) * r.choice([-1.0, 1.0], CQ)
        u /= np.linalg.norm(u)
        a = np.linspace(-6.0, 6.0, n) if n > 1 else np.array([-6.0])
        b = r.uniform(-6, 6, n)
        b[0] = 0.0                       # one level row between the two regimes (every key weighs the same: a padding key let in shows as 1 / (Np + 1))
        f, g = b[:, None] * u[None, :], a[:, None] * u[None, :]
    elif c.family == "negative":         # every product in [-7.2, -1.8]: every score between -9 and -36 nats
        lo, hi = np.sqrt(9.0 / CQ) * 1.0005, np.sqrt(36.0 / CQ) * 0.9995
        f, g = r.uniform(lo, hi, (n, CQ)), -r.uniform(lo, hi, (n, CQ))
    else:
        raise ValueError(c.family)
    h = r.uniform(-1, 1, (n, C))
    bf, bg, bh = (r.uniform(-0.5, 0.5, k).astype(np.float32) for k in (CQ, CQ, C))
    rows = np.full((n, ROW), np.nan, dtype=np.float32)
    rows[:, :CQ] = (f - bf).astype(np.float32)
    rows[:, CQ:2 * CQ] = (g - bg).astype(np.float32)
    rows[:, 2 * CQ:2 * CQ + C] = (h - bh).astype(np.float32)
    f32 = rows[:, :CQ] + bf
    g32 = rows[:, CQ:2 * CQ] + bg
    h32 = rows[:, 2 * CQ:2 * CQ + C] + bh
    for a in (rows, bf, bg, bh, f32, g32, h32):
        a.setflags(write=False)
    return rows, bf, bg, bh, f32, g32, h32


def exact(f, g, h):
    """softmax(f g^T) h in float64 on the fp32 operands."""
    s = f.astype(np.float64) @ g.astype(np.float64).T
    p = np.exp(s - s.max(axis=1, keepdims=True))
    return (p @ h.astype(np.float64)) / p.sum(axis=1, keepdims=True)


def torch32(f, g, h):
    """The same by torch in float32 on the CPU (mm, softmax, mm), as float64."""
    tf, tg, th = (torch.from_numpy(np.array(a)) for a in (f, g, h))
    return (torch.softmax(tf @ tg.t(), dim=1) @ th).double().numpy()


def rtz16(x):
    """Round toward zero onto the fp16 grid (x >= 0, float64 in and out; denormals kept: the grid is 2^-24 below 2^-14)."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)                                   # x = mant * 2^e, mant in [0.5, 1)
    ulp = np.ldexp(1.0, np.maximum(e - 11, -24))
    return np.floor(x / ulp) * ulp


def _pair16(x):
    """x (fp32) -> (xh, xl') as float64 values of fp16 numbers: xh = fp16(x), xl' = fp16((x - xh) * 2^11), fp32 arithmetic in between."""
    xh = x.astype(np.float16)
    xl = ((x - xh.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return xh, xl


def model(f, g, h, split, fault=None):
    assert fault is None or fault in FAULTS
    n = f.shape[0]
    npair = (n + 63) // 64
    fs = (f * LOG2E).astype(np.float32)
    fh, fl = _pair16(fs)
    gh, gl = _pair16(g.astype(np.float32))
    k = np.float16(1.0 / 2048.0)
    fhx, flx = (fh * k).astype(np.float16), (fl * k).astype(np.float16)          # fp16 products: rounded where they fall under the normal range
    fh, fl, gh, gl, fhx, flx = (a.astype(np.float64) for a in (fh, fl, gh, gl, fhx, flx))
    hh, hl = _pair16(h.astype(np.float32))
    hh, hl = hh.astype(np.float64), hl.astype(np.float64)
    keys = npair * 64
    pad = lambda a: np.concatenate([a, np.zeros((keys - n,) + a.shape[1:])], axis=0)          # padding keys: zero rows (pan_attn_prep)
    gh, gl, hh, hl = pad(gh), pad(gl), pad(hh), pad(hl)
    one = pad(np.ones(n))
    live = np.arange(keys) < n
    if fault == "droptail" and n % 32 and n > 32:
        live = np.arange(keys) < n - n % 32
    if fault == "unmasked" and n % 64:
        live = np.arange(keys) < n + 1
        one[n] = 1.0
    m = np.zeros(n)
    acc, accx = np.zeros((n, C)), np.zeros((n, C))
    den, denx = np.zeros(n), np.zeros(n)
    for bp in range(npair):
        sl = slice(64 * bp, 64 * bp + 64)
        s = fh @ gh[sl].T + flx @ gh[sl].T + fhx @ gl[sl].T - m[:, None]
        s[:, ~live[sl]] = -np.inf
        bm = s.max(axis=1)
        delta = bm if (bp == 0 and fault != "first_pair_m0") else np.maximum(bm, 0.0)
        m = m + delta
        if fault != "norescale":
            r = np.exp2(-delta)
            acc *= r[:, None]; accx *= r[:, None]; den *= r; denx *= r
        e = np.exp2(s - delta[:, None])
        p = rtz16(e)
        vh, vl, on = hh[sl], hl[sl], one[sl]
        if fault == "perm":
            j = np.arange(64) ^ 4
            vh, vl = vh[j], vl[j]
        acc += p @ vh
        den += p @ on
        if split:
            pl = rtz16((e - p) * 2048.0)
            accx += p @ vl + pl @ vh
            denx += pl @ on
    if split:
        acc, den = acc + accx / 2048.0, den + denx / 2048.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return acc / den[:, None]


def err(a, ref):
    """max |a - ref|, inf where a is not finite."""
    d = np.abs(a - ref)
    return float("inf") if not np.isfinite(a).all() else float(d.max())


@functools.lru_cache(maxsize=None)
def figures(c):
    """(exact, e32, e_model non-split, e_model split) of the case, computed once and shared; the exact result is read-only."""
    _, _, _, _, f, g, h = operands(c)
    ref = exact(f, g, h)
    ref.setflags(write=False)
    return ref, err(torch32(f, g, h), ref), err(model(f, g, h, False), ref), err(model(f, g, h, True), ref)


def bound(c, form):
    """The bound of tests/test_gpu_pan_fsa.py on |device - exact| for the launch's form: never taken from the kernel."""
    _, e32, em, ems = figures(c)
    return MARGIN * (e32 if form == 0 else em if form == 1 else ems + e32)


def split_budget(f, g, h):
    """What the split form's declared roundings can cost against exact, from the number formats: the lo parts x - xh are <= 2^-12 |x| and are kept to fp16's 2^-11, and
    the lo . lo product is dropped, so a score is off by <= 5 F G (2 * 2^-23 + 2^-24) log2 units (F = max |f log2 e|, G = max |g|; + as much again for the scaled cross
    operands' denormal rounding, <= 2^-25 each against operands <= G, F); a softmax weight moves by <= ln 2 * that relatively, numerator and denominator each; p and h
    are kept to 22 bits (2^-21, truncated, and 2^-23) and their lo . lo term is 2^-23."""
    F, G, Hm = float(np.abs(f * LOG2E).max()), float(np.abs(g).max()), float(np.abs(h).max())
    ds = CQ * F * G * (2.0 ** -22 + 2.0 ** -24) + CQ * (F + G) * 2.0 ** -25
    return (2.0 * np.log(2.0) * ds + 2.0 ** -20) * Hm
