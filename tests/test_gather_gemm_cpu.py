"""The gather GEMM's single-launch entry without a GPU: the packer, the plan, the reference of tests/_gather_gemm_ref.py and the check function of
tests/test_gpu_gather_gemm.py under a CPU stand-in with planted faults."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gather_gemm_ref as R
import test_gpu_gather_gemm as G
from innfer_amd import synth


# ------------------------------------------------------------------------------------------------ packer
def lds_image(w, cout, cin, cin_pad, ntaps):
    """The documented LDS image of the A operand: [channel tile][tap][chunk][64 rows][4 slots of 8]; slot s of row R holds channels 8 * (s ^ 2 * bit2(R)) .. + 7 of
    the chunk, out channel tile * 64 + R; padding is zero."""
    cots, nch = (cout + 63) // 64, cin_pad // 32
    wp = np.zeros((cots * 64, nch * 32, ntaps), np.float16)
    wp[:cout, :cin] = w.astype(np.float16)
    img = np.zeros((cots, ntaps, nch, 64, 4, 8), np.float16)
    for Rr in range(64):
        for s in range(4):
            cg = s ^ (2 * ((Rr >> 2) & 1))
            for ch in range(nch):
                img[:, :, ch, Rr, s, :] = wp[Rr::64, ch * 32 + cg * 8:ch * 32 + cg * 8 + 8, :].transpose(0, 2, 1)
    return img


@pytest.mark.parametrize("cout", [3, 64, 70])
@pytest.mark.parametrize("cin", [3, 32, 40])
@pytest.mark.parametrize("ntaps", [1, 9])
def test_packer_writes_the_documented_lds_image(cout, cin, ntaps):
    import innfer_amd.lib as L
    cin_pad = (cin + 31) // 32 * 32
    w = synth.uniform((cout, cin, ntaps), 7 + cout + cin, -1, 1)
    size = L.lib.innfer_gather_gemm_packed_bytes(cout, cin_pad, ntaps)
    assert size == (cout + 63) // 64 * ntaps * (cin_pad // 32) * 64 * 32 * 2
    got = np.full(size // 2, 9.0, np.float16)
    L.check(L.lib.innfer_pack_gather_gemm(w.ctypes.data, cout, cin, cin_pad, ntaps, got.ctypes.data))
    assert np.array_equal(got.view(np.uint16), lds_image(w, cout, cin, cin_pad, ntaps).reshape(-1).view(np.uint16))
    assert L.lib.innfer_gather_gemm_packed_bytes(cout, cin_pad + 1, ntaps) == 0 and L.lib.innfer_gather_gemm_packed_bytes(cout, cin_pad, 50) == 0
    assert L.lib.innfer_pack_gather_gemm(w.ctypes.data, cout, cin_pad + 1, cin_pad, ntaps, got.ctypes.data) == L.ERR_INVALID


# ------------------------------------------------------------------------------------------------ plan
def test_abi_revision():
    import innfer_amd.lib as L
    assert L.ABI_VERSION == 124 == L.lib.innfer_version()
    assert C.sizeof(L.GatherGemmArgs) % 8 == 0 and L.GatherGemmArgs.keep_partials.offset + 8 == C.sizeof(L.GatherGemmArgs)


@pytest.mark.parametrize("c", R.CASES, ids=str)
def test_every_case_plans_what_it_was_designed_for(c):
    p = G.plan(c)
    assert (p["shape"], p["ksplit"], p["seg"], p["taps"]) == c.expect
    sb, need = G.scratch_bytes(c)
    if p["ksplit"] > 1:
        assert need == p["ksplit"] * c.N * c.Hfull * c.Wfull * c.row * 4 <= sb
    assert p["taps"] == len(R.kept_taps(c)[0]), "kept taps against the brute-force enumeration over all output pixels"


def test_the_cases_reach_every_shape_split_and_prologue():
    shapes = {c.expect[0] for c in R.CASES}
    assert shapes == {0, 1, 2} and {(c.expect[0], c.expect[1] > 1) for c in R.CASES} >= {(0, True), (1, True), (2, True), (1, False), (2, False)}
    steps = {c.expect[3] * (c.cin_pad // 32) for c in R.CASES if c.expect[1] == 1}
    assert steps >= {1, 2, 3, 4, 5, 9}
    assert {c.expect[1] for c in R.CASES} >= {1, 2, 4, 5, 8}
    for c in R.RANDOM_CASES:
        assert c.values >= R.FEW
    assert {c.family for c in R.RANDOM_CASES} == {c.family for c in R.CASES}


@pytest.mark.parametrize("c", [c for c in R.CASES if c.Hin <= 17], ids=str)
def test_split_and_taps_do_not_depend_on_the_batch(c):
    """A batch equals its batch-1 forwards: ksplit, seg and the kept taps are the layer's, for any N with the scratch scaled by N; the tile shape may differ."""
    import innfer_amd.lib as L
    per_image = 8 * c.Hfull * c.Wfull * c.row * 4 if c.scratch == "ample" else 0
    seen = set()
    for N in (1, 2, 3, 16, 64):
        p = L.gather_gemm_plan(G.make_args(replace(c, N=N), d_scratch=1 if per_image else 0, scratch_bytes=N * per_image))
        seen.add((p["ksplit"], p["seg"], p["taps"]))
    assert len(seen) == 1
    if c.scratch != "short":
        assert seen == {c.expect[1:]}


PLAN_REFUSALS = G.REFUSALS + [("input beyond the 2 GiB buffer window", G.TOO_BIG, {}, G.ERR_UNSUPPORTED)]


@pytest.mark.parametrize("what,c,override,code", PLAN_REFUSALS, ids=[r[0] for r in PLAN_REFUSALS])
def test_plan_refuses_what_the_launch_refuses(what, c, override, code):
    import innfer_amd.lib as L
    a = G.make_args(c, d_scratch=1, scratch_bytes=1 << 30)
    for k, v in override.items():
        setattr(a, k, v)
    info = (C.c_int * 5)(*([-7] * 5))
    assert L.lib.innfer_gather_gemm_plan(C.byref(a), info) == code and L.last_error()
    assert list(info) == [-7] * 5
    if c is G.TOO_BIG:      # one row less fits the window
        assert L.gather_gemm_plan(G.make_args(replace(c, Hin=5792, Ho=5792)))["ksplit"] == 1


# ------------------------------------------------------------------------------------------------ reference
def _nchw(c, x):
    return x.double().permute(0, 3, 1, 2)


def _kernel(w, kh, kw):
    return w.double().reshape(w.shape[0], w.shape[1], kh, kw)


def _case(name):
    return next(c for c in R.CASES if c.name == name)


CROSS = [
    ("3x3 40->70 2x5x7", lambda x, w: F.conv2d(x, _kernel(w[0], 3, 3), padding=1)),
    ("3x3 40->70 2x9x13", lambda x, w: F.conv2d(x, _kernel(w[0], 3, 3), padding=1)),
    ("3x3 s2 40->70 2x5x7", lambda x, w: F.conv2d(x, _kernel(w[0], 3, 3), stride=2, padding=1)),
    ("3x3 s2 40->70 2x6x8 (even)", lambda x, w: F.conv2d(x, _kernel(w[0], 3, 3), stride=2, padding=1)),
    ("3x3 s2 tf 40->70 2x5x7", lambda x, w: F.conv2d(F.pad(x, (0, 1, 0, 1)), _kernel(w[0], 3, 3), stride=2)),
    ("3x3 s2 tf 40->70 2x6x8 (even)", lambda x, w: F.conv2d(F.pad(x, (0, 1, 0, 1)), _kernel(w[0], 3, 3), stride=2)),
    ("4x4 s2 40->70 2x5x7", lambda x, w: F.conv2d(x, _kernel(w[0], 4, 4), stride=2, padding=1)),
    ("4x4 s2 40->70 2x6x8 (even)", lambda x, w: F.conv2d(x, _kernel(w[0], 4, 4), stride=2, padding=1)),
    ("7x7 40->70 2x5x7", lambda x, w: F.conv2d(x, _kernel(w[0], 7, 7), padding=3)),
    ("7x7 reflect 40->70 2x9x13", lambda x, w: F.conv2d(F.pad(x, (3, 3, 3, 3), mode="reflect"), _kernel(w[0], 7, 7))),
    ("7x7 reflect 40->64 4x4x4 (smallest)", lambda x, w: F.conv2d(F.pad(x, (3, 3, 3, 3), mode="reflect"), _kernel(w[0], 7, 7))),
    ("7x1 40->70 2x5x7", lambda x, w: F.conv2d(x, _kernel(w[0], 7, 1), padding=(3, 0))),
    ("7x1 reflect 40->70 2x9x13", lambda x, w: F.conv2d(F.pad(x, (0, 0, 3, 3), mode="reflect"), _kernel(w[0], 7, 1))),
    ("3x3 reflect 40->70 2x5x7", lambda x, w: F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), _kernel(w[0], 3, 3))),
    ("3x3 reflect 40->64 32x2x2 (smallest)", lambda x, w: F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), _kernel(w[0], 3, 3))),
    ("3x3 up 40->70 2x3x5 -> 6x10", lambda x, w: F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), _kernel(w[0], 3, 3), padding=1)),
    ("4x4 s2 64->64 64x2x2 -> 1x1 (12 of 16 dropped)", lambda x, w: F.conv2d(x, _kernel(w[0], 4, 4), stride=2, padding=1)),
]


@pytest.mark.parametrize("name,op", CROSS, ids=[n for n, _ in CROSS])
def test_tap_tables_say_the_torch_operator(name, op):
    c = _case(name)
    x, w = R.operands(c, "random")
    ref, mask = R.reference(c, x, w)
    y = op(_nchw(c, x), w).permute(0, 2, 3, 1)
    assert y.shape == (c.N, c.Ho, c.Wo, c.cout)
    assert torch.allclose(ref[..., :c.cout], y, rtol=0, atol=1e-12)
    assert mask[..., :c.store].all() and not mask[..., c.store:].any() and (ref[..., c.cout:] == 0).all()


@pytest.mark.parametrize("H,W", [(9, 9), (5, 7), (17, 19)])
def test_dilated_groups_say_dilation_1_to_8(H, W):
    c = _case(f"8 x 3x3 d1..8 64->32 2x{H}x{W}")
    x, w = R.operands(c, "random")
    ref, mask = R.reference(c, x, w)
    for g in range(8):
        y = F.conv2d(_nchw(c, x), _kernel(w[g], 3, 3), padding=g + 1, dilation=g + 1).permute(0, 2, 3, 1)
        assert torch.allclose(ref[..., 32 * g:32 * g + 32], y, rtol=0, atol=1e-12)
    assert mask[..., :256].all() and not mask[..., 256:].any()
    if (H, W) == (5, 7):        # dilation 8 leaves the centre tap alone (at 9 x 9: for the centre pixel; every tap still meets a corner)
        assert sum(R.live_taps(c, 7)) == 1


@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 2), (3, 5), (8, 8)])
@pytest.mark.parametrize("k", [3, 4])
def test_phase_taps_say_conv_transpose2d(k, H, W):
    """ConvTranspose2d(4, 2, 1) as the grouped launch and (3, 2, 1, output_padding 1) as four single-phase launches: assembled, they are F.conv_transpose2d."""
    N, cin, cout = 2, 40, 64
    x = torch.from_numpy(synth.uniform((N, H, W, cin), 5, -1, 1)).half()
    wt = torch.from_numpy(synth.uniform((cin, cout, k, k), 6, -1, 1)).half()
    y = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), wt.double(), stride=2, padding=1, output_padding=1 if k == 3 else 0).permute(0, 2, 3, 1)
    tabs = [R.convt_phase_taps(k, ph >> 1, ph & 1) for ph in range(4)]
    assert [len(t) for t in tabs] == ([1, 2, 2, 4] if k == 3 else [4] * 4)
    ws = [torch.stack([wt[:, :, ky, kx].t() for _, _, ky, kx in t], 2) for t in tabs]          # [cout][cin][taps of the phase]
    if k == 4:
        c = R._phase4("x", "x", N, H, W, cin, cout, (0, 0, 0, 0))
        assert c.taps == next(q for q in R.CASES if q.g_phase and q.family == "transposed").taps
        ref, mask = R.reference(c, x, torch.stack(ws))
        assert mask.all()
    else:
        ref, mask = torch.zeros(N, 2 * H, 2 * W, cout, dtype=torch.float64), torch.zeros(N, 2 * H, 2 * W, cout, dtype=torch.bool)
        for ph, t in enumerate(tabs):
            c = R._c("x", "x", N, H, W, cin, cout, [(dy, dx) for dy, dx, _, _ in t], H, W, (0, 0, 0, 0), os=2, ooy=ph >> 1, oox=ph & 1)
            assert any(q.taps == c.taps and (q.ooy, q.oox) == (c.ooy, c.oox) and (q.Hin, q.Win) == (H, W) for q in R.CASES)
            r, m = R.reference(c, x, ws[ph][None])
            assert not (mask & m).any()
            ref, mask = ref + r, mask | m
        assert mask.all()
    assert torch.allclose(ref, y, rtol=0, atol=1e-12)


def test_exact_data_sums_are_exact_in_float32_in_any_order():
    """The premise of the bit-for-bit comparison, on the longest sum of the cases: every float32 partial sum, in several shuffled orders, equals float64."""
    c = max(R.CASES, key=lambda q: q.ntaps * q.cin)
    assert c.ntaps * c.cin == 16 * 512
    x, w = R.operands(c, "exact")
    for t in (x, w):
        assert (t.double() * 8 == torch.round(t.double() * 8)).all() and t.abs().max() == 1.0
    A = R.gather(c, x.double(), 0).reshape(-1, c.ntaps * c.cin)[:24]
    B = w[0].double().permute(2, 1, 0).reshape(c.ntaps * c.cin, c.cout)[:, :16]
    g = torch.Generator().manual_seed(3)
    for _ in range(4):
        perm = torch.randperm(A.shape[1], generator=g)
        prod = A[:, perm, None] * B[None, perm, :]
        run64 = torch.cumsum(prod, 1)
        run32 = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
        for k in range(0, A.shape[1], 64):                  # float32 running sums, term by term within blocks of 64 (cumsum) and block by block
            blk = torch.cumsum(prod[:, k:k + 64].float(), 1) + run32[:, None]
            assert torch.equal(blk.double(), run64[:, k:k + 64])
            run32 = blk[:, -1]
        assert run64.abs().max() < 2 ** 14
        assert torch.equal((A[:, perm].float() @ B[perm].float()).double(), A @ B)
    for q in R.CASES:       # no case sums more terms than this one
        assert q.ntaps * q.cin <= 16 * 1024


@pytest.mark.parametrize("name", ["3x3 96->128 5x5x7", "4x4 s2 512->64 4x8x8 -> 4x4", "3x3 480->64 1x8x8 (34 + 34 + 34 + 33)", "convT k4 phases 512->64 1x4x4 -> 8x8, split",
                                  "8 x 3x3 d1..8 64->32 2x9x9"])
def test_e32_ingredients_agree(name):
    """float32 F.conv2d and the float32 emulation of the kernel's order are two orders of the same sums: their distances from float64 agree within the margin the
    bound gives an order (8), and neither is zero."""
    c = _case(name)
    x, w = R.operands(c, "random")
    ref, mask = R.reference(c, x, w)
    a = (R.conv32(c, x, w).double() - ref).abs().max().item()
    b = (R.emulate32(c, x, w).double() - ref).abs().max().item()
    print(f"[gather-gemm] {c}: F.conv2d {a:.3e}, emulation {b:.3e}, factor {max(a, b) / min(a, b):.2f}")
    assert 0 < a and 0 < b and max(a, b) <= 8 * min(a, b)
    ex, ew = R.operands(c, "exact")
    assert torch.equal(R.emulate32(c, ex, ew).double(), R.reference(c, ex, ew)[0])


# ------------------------------------------------------------------------------------------------ the check function under a CPU stand-in
def standin(fault=None):
    """A float32 gather GEMM on the CPU in the entry's output format (loops over groups, segments, taps and chunks; info from the plan), optionally with one fault."""
    def shifted(c, xf, dy, dx):
        N, H, W, _ = xf.shape
        oy, ox = np.arange(c.Ho) * c.stride + dy, np.arange(c.Wo) * c.stride + dx
        if c.reflect:
            k = 0 if fault == "reflect" else 2
            oy = np.where(oy < 0, -oy, np.where(oy >= H, 2 * H - k - oy, oy))
            ox = np.where(ox < 0, -ox, np.where(ox >= W, 2 * W - k - ox, ox))
        s = 2 if c.up else 1
        iy, ix = np.broadcast_to(oy[:, None], (c.Ho, c.Wo)), np.broadcast_to(ox[None, :], (c.Ho, c.Wo))
        ok = (iy >= 0) & (iy < s * H) & (ix >= 0) & (ix < s * W)
        flat = (np.arange(N)[:, None, None] * H + iy[None] // s) * W + ix[None] // s
        if fault == "neighbour":        # the image bound forgotten: a padding tap reads whatever pixel the flat index lands on
            okn = np.broadcast_to((ix >= 0) & (ix < s * W), (N, c.Ho, c.Wo)) & (flat >= 0) & (flat < N * H * W)
        else:
            okn = np.broadcast_to(ok, (N, c.Ho, c.Wo))
        return xf.reshape(N * H * W, -1)[np.clip(flat, 0, N * H * W - 1)] * okn[..., None]

    def launch(c, x, w, fill=R.SENT, keep=0, **_):
        p = G.plan(c)
        ks, seg = p["ksplit"], p["seg"]
        raw = np.full(c.N * c.Hfull * c.Wfull * c.row + 2 * G.GUARD, R.SENT, np.float32)
        img = raw[G.GUARD:-G.GUARD].reshape(c.N, c.Hfull, c.Wfull, c.row)
        xf = np.zeros((c.N, c.Hin, c.Win, c.cin_pad), np.float32)
        xf[..., :c.cin] = x.float().numpy()
        if fault == "channels":
            xf[..., [3, 4]] = xf[..., [4, 3]]
        wf = np.zeros((w.shape[0], c.cout, c.cin_pad, c.ntaps), np.float32)
        wf[:, :, :c.cin] = w.float().numpy()
        keep_t = R.kept_taps(c)
        for g in range(c.ngroup):
            taps, m = c.group_taps(g), c.tapmul(g)
            steps = [(t, ch) for t in keep_t[g if c.g_phase else 0] for ch in range(c.cin_pad // 32)]
            if fault == "tap":
                steps = [s for s in steps if s[0] != steps[-1][0]]
            total = np.zeros((c.N, c.Ho, c.Wo, c.cout), np.float32)
            for z in range(ks):
                mine = steps[z * seg:(z + 1) * seg] if ks > 1 else steps
                if fault == "segment" and ks > 1:
                    mine = mine[:-1]
                acc = np.zeros_like(total)
                for t, ch in mine:
                    dy, dx = taps[t] if fault != "swap" else taps[t][::-1]
                    acc += shifted(c, xf[..., 32 * ch:32 * ch + 32], dy * m, dx * m) @ wf[g, :, 32 * ch:32 * ch + 32, t].T
                total = total + acc
            oy0, ox0 = c.origin(g)
            if fault == "quadrant":
                oy0, ox0 = ox0, oy0
            n, off = min(c.store, c.cout), c.raw_off + g * c.g_outoff
            store = c.store + (4 if fault == "sentinel" else 0)
            blk = np.zeros((c.N, c.Ho, c.Wo, store), np.float32)
            blk[..., :n] = total[..., :n]
            img[:, oy0::c.os, ox0::c.os, off:off + store] = blk
        sb, _ = G.scratch_bytes(c)
        return G.Result(0, tuple(p.values()), raw, np.full((sb + 4) // 4 + G.GUARD, R.SENT, np.float32) if sb else None)
    return launch


STANDIN_CASES = [c for c in R.CASES if c.family != "wide tiles" and c.N * c.Hin * c.Win * c.cin_pad * c.ntaps <= 1 << 21]


@pytest.mark.parametrize("c", STANDIN_CASES, ids=str)
def test_the_right_standin_passes_the_gpu_check(c):
    G.check_case(c, "exact", standin(), measure=False)


def test_the_right_standin_passes_on_random_data():
    for name in ("3x3 96->128 5x5x7", "4x4 s2 160->64 4x8x8 -> 4x4", "8 x 3x3 d1..8 64->32 2x9x9"):
        G.check_case(_case(name), "random", standin(), measure=False)


FAULTS = [
    ("tap", "3x3 40->70 2x5x7"), ("tap", "convT k4 phases 40->64 2x3x5"),
    ("swap", "3x3 40->70 2x5x7"), ("swap", "7x1 40->70 2x5x7"),
    ("segment", "4x4 s2 160->64 4x8x8 -> 4x4"), ("segment", "3x3 480->64 1x8x8 (34 + 34 + 34 + 33)"),
    ("quadrant", "convT k4 phases 40->64 2x3x5"), ("quadrant", "convT k3 phase 01 40->64 2x3x5"),
    ("reflect", "3x3 reflect 40->70 2x5x7"), ("reflect", "7x7 reflect 40->64 4x4x4 (smallest)"),
    ("channels", "3x3 40->70 2x5x7"), ("channels", "1x1 64->64 2x5x7 (2 steps)"),
    ("neighbour", "3x3 40->70 2x5x7"), ("neighbour", "4x4 s2 40->70 2x6x8 (even)"),
    ("sentinel", "8 x 3x3 d1..8 64->32 2x5x7"), ("sentinel", "4x4 s2 128->64 4x8x8 -> 4x4, row wider than the store"),
]


@pytest.mark.parametrize("fault,name", FAULTS, ids=[f"{f}: {n}" for f, n in FAULTS])
def test_planted_faults_fail_on_the_exact_data(fault, name):
    """One tap dropped; dy / dx swapped; the last step of a segment skipped; a phase in the wrong quadrant; reflection without the -2; channels 3 and 4 swapped; a
    neighbour image read where padding belongs; the sentinel overwritten beyond cout_store."""
    with pytest.raises(AssertionError):
        G.check_case(_case(name), "exact", standin(fault), measure=False)
