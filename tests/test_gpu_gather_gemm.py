"""The gather GEMM, one launch at a time, against float64 (needs an MI355X: `pytest -m gpu`).

gg::gemm_gather (csrc/gather_gemm.h) runs what the halo-tile kernel cannot express -- the pix2pix UNet's deep levels, every conv of the CycleGAN ResNet, the WBC
UNet, PPON's fallback dilated convs and c2, PAN's attention projections -- and until ABI 122 was seen only through those networks.  innfer_gather_gemm makes one
launch of it through the decision code of the five families (gg::decide); tests/_gather_gemm_ref.py holds the reference (the descriptor taken literally, float64, index
gather plus matmul), the two kinds of data and the cases.  Every case asserts

  1. info = the tile shape, ksplit, seg and kept taps the case was designed to reach (a later change of the heuristics fails here instead of moving the coverage);
  2. the values: exact data (integers / 8: every partial sum representable in fp32) equal float64 BIT FOR BIT; random data within 8 * e32 (cases of >= 4096 values);
  3. everything else keeps the sentinel: channels >= cout_store, the other phase positions of an os = 2 launch, other writers' columns of a shared row, the guards
     around the raw buffer and behind the scratch;
  4. a second run with another scratch fill gives identical bits;
  5. the case took a few seconds at the most, its reference included.

The input slab lies between bands of 1024.0 with a junk group behind its last chunk and finite junk in its pad channels: read by mistake, each shows in the values.

Split launches whose raw row is wider than cout_store (several GEMMs filling one row): until ABI 121 the in-call reduction ran over the whole row -- scratch nobody
wrote, stored over the neighbours' columns.  No network formed that launch (only the UNet passes scratch, with raw_stride == cout_store).  The reduction is now confined
to the channels the GEMM wrote; "row wider than the store" below is its test.

Measured on the MI355X (largest e32 of the family's random cases; worst err / (8 e32) over every element of them; exact cases, each bit-equal):

    family              e32        worst err / bound    exact cases
    tile walk           1.3e-06    0.068                8
    ring prologue       5.4e-07    0.076                6
    tap tables          9.0e-07    0.193                24
    dilated groups      1.9e-06    0.039                3
    transposed          5.8e-07    0.060                26
    dead taps           2.1e-07    0.143                3
    split-K tiny        1.5e-07    0.090                3
    split-K             5.2e-07    0.262                10
    wide tiles          2.7e-06    0.169                8

91 exact cases, every one bit-equal; the random cases stay below 0.27 of 8 e32 (the largest where a 135-step k loop runs unsplit).  keep_partials: the host's
float32 sum of the segments, in split order, equals the in-call reduction bit for bit on exact and random data.

"""
import ctypes as C
import time
from dataclasses import dataclass, replace

import numpy as np
import pytest
import torch

import _gather_gemm_ref as R

GUARD = 4096                # floats around the raw buffer and behind the scratch
SECONDS = 10.0              # "a few seconds": the whole check of a case, references and both launches
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -3


# ------------------------------------------------------------------------------------------------ arguments and the plan (no GPU)
def make_args(c, d_in=0, in_gs=0, d_packed=0, g_wbytes=0, d_raw=0, d_scratch=0, scratch_bytes=0, keep=0):
    import innfer_amd.lib as L
    return L.gather_gemm_args([t[0] for t in c.taps], [t[1] for t in c.taps], ntaps=c.ntaps,
                              d_in=d_in, in_group_stride=in_gs, cin_pad=c.cin_pad, d_packed=d_packed, cout_pad=c.cout_pad,
                              d_raw=d_raw, raw_stride=c.raw_stride, cout_store=c.cout_store,
                              N=c.N, Hin=c.Hin, Win=c.Win, Ho=c.Ho, Wo=c.Wo, stride=c.stride,
                              Hfull=c.Hfull, Wfull=c.Wfull, os=c.os, ooy=c.ooy, oox=c.oox, up=c.up, reflect=c.reflect,
                              ngroup=c.ngroup, g_wbytes=g_wbytes, g_outoff=c.g_outoff, g_tapmul=c.g_tapmul, g_phase=c.g_phase,
                              d_scratch=d_scratch, scratch_bytes=scratch_bytes, keep_partials=keep)


def scratch_bytes(c):
    """(bytes the case passes as scratch_bytes, bytes the split of the layer needs): `ample` passes exactly what the plan asks for, `short` one byte less."""
    import innfer_amd.lib as L
    if c.scratch == "none":
        return 0, 0
    need = L.gather_gemm_plan(make_args(c, d_scratch=1, scratch_bytes=1 << 40))["split_bytes"]
    return (need - 1 if c.scratch == "short" else max(need, 4096)), need


def plan(c):
    import innfer_amd.lib as L
    sb, _ = scratch_bytes(c)
    return L.gather_gemm_plan(make_args(c, d_scratch=1 if sb else 0, scratch_bytes=sb))


def pack(c, w):
    """The groups' panels back to back through innfer_pack_gather_gemm: (uint8 array, bytes per group)."""
    import innfer_amd.lib as L
    per = L.lib.innfer_gather_gemm_packed_bytes(c.cout, c.cin_pad, c.ntaps)
    assert per > 0
    out = np.zeros(per * w.shape[0], dtype=np.uint8)
    for g in range(w.shape[0]):
        wg = np.ascontiguousarray(w[g].float().numpy())
        L.check(L.lib.innfer_pack_gather_gemm(wg.ctypes.data, c.cout, c.cin, c.cin_pad, c.ntaps, out[g * per:].ctypes.data))
    return out, per


# ------------------------------------------------------------------------------------------------ one launch
@dataclass
class Result:
    rc: int
    info: tuple
    raw: np.ndarray             # float32, GUARD + N * Hfull * Wfull * row + GUARD
    scratch: np.ndarray         # float32 (the bytes passed, rounded up, + GUARD), or None


def launch_gpu(c, x, w, fill=R.SENT, keep=0, override=None, sb=None):
    """One innfer_gather_gemm of the case on cuda:0 (override: struct fields set after the case's own; sb: scratch bytes instead of the case's)."""
    import innfer_amd.lib as L
    dev = torch.device("cuda:0")
    slab, first, gs = R.input_slab(c, x)
    d_slab = slab.to(dev)
    panels, per = pack(c, w)
    d_w = torch.from_numpy(panels).to(dev)
    body = c.N * c.Hfull * c.Wfull * R.width(c)
    d_raw = torch.full((body + 2 * GUARD,), R.SENT, dtype=torch.float32, device=dev)
    if sb is None:
        sb, _ = scratch_bytes(c)
    d_scr = torch.full(((sb + 4) // 4 + GUARD,), fill, dtype=torch.float32, device=dev) if sb else None
    a = make_args(c, d_in=d_slab.data_ptr() + 2 * first, in_gs=gs, d_packed=d_w.data_ptr(), g_wbytes=per,
                  d_raw=d_raw.data_ptr() + 4 * (GUARD + c.raw_off), d_scratch=d_scr.data_ptr() if sb else 0, scratch_bytes=sb, keep=keep)
    for k, v in (override or {}).items():
        setattr(a, k, v)
    info = (C.c_int * 5)(*([-1] * 5))
    rc = L.lib.innfer_gather_gemm(C.byref(a), info, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return Result(rc, tuple(info), d_raw.cpu().numpy(), d_scr.cpu().numpy() if sb else None)


# ------------------------------------------------------------------------------------------------ the check
def check_case(c, kind, launch, measure=True):
    """The five assertions of the file's docstring on one case; `launch` makes the launch (the GPU's, or a CPU stand-in of the same output format)."""
    t0 = time.perf_counter()
    x, w = R.operands(c, kind)
    ref, mask, e32 = R.expected(c, kind)
    r = launch(c, x, w, fill=R.SENT)
    assert r.rc == OK, (str(c), r.rc)
    assert r.info[:4] == c.expect, f"{c}: the launch took (shape, ksplit, seg, taps) = {r.info[:4]}, the case was designed for {c.expect}"
    assert (r.raw[:GUARD] == R.SENT).all() and (r.raw[-GUARD:] == R.SENT).all(), f"{c}: the guards of the raw buffer were written"
    got = torch.from_numpy(r.raw[GUARD:-GUARD]).reshape(ref.shape)
    assert (got[~mask] == R.SENT).all(), f"{c}: {(got[~mask] != R.SENT).sum().item()} elements outside the launch's channels / phase / columns lost the sentinel"
    sb, need = scratch_bytes(c)
    if r.scratch is not None:
        used = need // 4 if r.info[1] > 1 else 0
        assert (r.scratch[used:] == R.SENT).all(), f"{c}: the scratch was written beyond the {r.info[1]} partial results"
    assert torch.isfinite(got[mask]).all(), f"{c}: non-finite values"
    err = (got.double() - ref).abs()[mask]
    if kind == "exact":
        assert (err == 0).all(), f"{c}: {(err != 0).sum().item()} of {err.numel()} values differ from float64 on exact data (largest difference {err.max().item():.4g})"
        worst = 0.0
    else:
        assert c.values >= R.FEW, f"{c}: {c.values} values understate e32"
        worst = (err.max() / (8 * e32)).item()
        print(f"[gather-gemm] {c.family} | {c}: e32 {e32:.2e} worst err/bound {worst:.3f}")
        assert worst <= 1.0, f"{c}: e32 {e32:.3e}, worst err / (8 e32) {worst:.3f}: {(err > 8 * e32).sum().item()} of {err.numel()} values beyond the bound"
    r2 = launch(c, x, w, fill=11.0)
    assert r2.rc == OK and np.array_equal(r.raw.view(np.uint32), r2.raw.view(np.uint32)), f"{c}: another scratch fill changed the result"
    took = time.perf_counter() - t0
    if measure:
        m = R.MEASURED.setdefault(c.family, [0.0, 0.0, 0])
        m[0], m[1], m[2] = max(m[0], e32), max(m[1], worst), m[2] + (kind == "exact")
    print(f"[gather-gemm] {c.family} | {c} ({kind}): {took:.2f} s")
    assert took <= SECONDS, f"{c}: {took:.1f} s"
    return r


# ------------------------------------------------------------------------------------------------ tests
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import innfer_amd.lib  # noqa: F401
    torch.zeros(1, device="cuda:0").cpu()       # the context exists before a case starts its clock
    return torch.device("cuda:0")


@gpu
@pytest.mark.parametrize("c", R.CASES, ids=str)
def test_exact_data_bit_for_bit(dev, c):
    check_case(c, "exact", launch_gpu)


@gpu
@pytest.mark.parametrize("c", R.RANDOM_CASES, ids=str)
def test_random_data_within_8_e32(dev, c):
    check_case(c, "random", launch_gpu)


SPLIT_CASES = [c for c in R.CASES if c.expect[1] > 1 and c.N * c.Ho * c.Wo <= 4096 and c.cout <= 256]


@gpu
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("c", SPLIT_CASES, ids=str)
def test_keep_partials_sum_equals_the_in_call_reduction(dev, c, kind):
    """keep_partials leaves the segments' partial results in scratch and d_raw untouched; their float32 sum on the host, in split order, is the in-call reduction's
    result bit for bit (the order the UNet's deep-level pass adds them in)."""
    x, w = R.operands(c, kind)
    _, mask, _ = R.expected(c, kind)
    c0 = replace(c, raw_off=0)                  # the partials lie in scratch from column 0: raw_off belongs to d_raw
    pmask = torch.roll(mask.reshape(-1), -c.raw_off).reshape(mask.shape)
    red = launch_gpu(c, x, w)
    kept = launch_gpu(c, x, w, keep=1)
    assert red.rc == OK and kept.rc == OK and kept.info[:4] == c.expect
    assert (kept.raw == R.SENT).all(), "keep_partials wrote d_raw"
    ks, n = c.expect[1], mask.numel()
    parts = torch.from_numpy(kept.scratch[:ks * n]).reshape(ks, *mask.shape)
    assert (parts[:, ~pmask] == R.SENT).all(), "a partial result was written outside the launch's channels"
    assert (kept.scratch[ks * n:] == R.SENT).all()
    acc = parts[0].clone()
    for z in range(1, ks):
        acc = acc + parts[z]
    got = torch.from_numpy(red.raw[GUARD:-GUARD]).reshape(mask.shape)
    assert np.array_equal(acc[pmask].numpy().view(np.uint32), got[mask].numpy().view(np.uint32))
    if kind == "exact":     # and every segment is the sum of its own k-steps (exact in fp32 on this data)
        for z, p in enumerate(R.emulate32(c0, x, w, partials=True)):
            assert torch.equal(p[pmask], parts[z][pmask]), f"segment {z}"


@gpu
@pytest.mark.parametrize("cout", [256, 512])
def test_a_batch_on_wide_split_tiles_equals_its_batch_1_launch(dev, cout):
    """64 images of 8 x 8 -> 16 x 16 take the 256 x 128 / 256 x 256 tiles at ksplit 2, tiles straddling images; the same layer at N = 1 takes 128 x 64 tiles.  The tile
    shape never changes an element's accumulation order: images 0 and 63 of the batch equal the N = 1 launch bit for bit (random data)."""
    big = next(c for c in R.CASES if c.family == "wide tiles" and c.g_phase and c.N == 64 and c.cout == cout)
    one = next(c for c in R.CASES if c.family == "wide tiles" and c.g_phase and c.N == 1 and c.cout == cout)
    x, w = R.operands(big, "random")
    x = x.clone()
    x[63] = x[0]
    rb, r1 = launch_gpu(big, x, w), launch_gpu(one, x[:1], w)
    assert rb.rc == OK and r1.rc == OK and rb.info[:4] == big.expect and r1.info[:4] == one.expect and rb.info[0] != r1.info[0]
    b = rb.raw[GUARD:-GUARD].reshape(64, -1).view(np.uint32)
    o = r1.raw[GUARD:-GUARD].view(np.uint32)
    assert np.array_equal(b[0], o) and np.array_equal(b[63], o)


BASE = next(c for c in R.CASES if c.name == "3x3 32->64 2x5x7 (9 steps)")
PHASE = next(c for c in R.CASES if c.name == "convT k4 phases 40->64 2x3x5")
REFUSALS = [
    ("raw_stride 6", BASE, dict(raw_stride=6), ERR_INVALID),
    ("raw_stride -4", BASE, dict(raw_stride=-4), ERR_INVALID),
    ("ntaps 0", BASE, dict(ntaps=0), ERR_INVALID),
    ("ntaps 50", BASE, dict(ntaps=50), ERR_INVALID),
    ("g_phase with two groups", PHASE, dict(ngroup=2), ERR_INVALID),
    ("g_phase with 13 taps per group", PHASE, dict(ntaps=13), ERR_INVALID),
    ("cout_store 6", BASE, dict(cout_store=6), ERR_INVALID),
    ("reflect 3x3 on a 1 x 7 image", replace(BASE, Hin=1, Ho=1, reflect=1), {}, ERR_UNSUPPORTED),
    ("reflect 7x7 on a 3 x 7 image", replace(BASE, Hin=3, Ho=3, taps=R.T7, reflect=1), {}, ERR_UNSUPPORTED),
]
TOO_BIG = replace(BASE, N=1, Hin=5793, Win=5793, Ho=5793, Wo=5793)       # 5793^2 pixels x 64 bytes >= 2^31 - 1: through the plan only, nothing allocated


@gpu
@pytest.mark.parametrize("what,c,override,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_launch_nothing(dev, what, c, override, code):
    import innfer_amd.lib as L
    x, w = R.operands(c, "exact")
    r = launch_gpu(c, x, w, override=override, sb=1 << 16)
    assert r.rc == code, (what, r.rc, L.last_error())
    assert (r.raw == R.SENT).all() and (r.scratch == R.SENT).all(), f"{what}: a refused launch wrote"


@gpu
def test_measured_table(dev):
    """Prints the table of the docstring from what the tests above measured (run the file as a whole)."""
    for fam, (e32, worst, n) in R.MEASURED.items():
        print(f"[gather-gemm-table] {fam:<20}{e32:<11.1e}{worst:<21.3f}{n}")
