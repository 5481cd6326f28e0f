"""PAN's SCPA block kernels (csrc/pan_scpa.hip pan_scpa_fused<16> / pan_scpa_duo, csrc/pan_scpa_split.hip pan_scpa_split), one launch at a time, against float64
(needs an MI355X: `pytest -m gpu`).

The network tests do not hold these kernels: with synth.fill_state_dict weights the block's branch is a small correction to x and its gate is flat, so ten different
faults planted in EVERY block stay below every fp16 bound of the suite (the table in tests/test_pan_scpa_cpu.py), and up to 200 x 200 no workgroup takes a second
tile.  Here each launch runs alone through innfer_pan_scpa_block, which calls the launch functions the two forwards call.

Forms       every shape of tests/_pan_scpa_ref.py x {flat, live} x form 0 (pan_scpa_fused<16>), 1 (pan_scpa_duo), -1 (the forward's choice) against the float64 model
            with the kernels' declared fp16 roundings: |got - model64| <= ulp16 / 2 + 8 e_model + trans per element; x form 2 (pan_scpa_split) against exact float64:
            <= 8 e_split + trans.  No figure comes from a kernel; tests/test_pan_scpa_cpu.py proves that twelve planted faults miss both bounds by >= 10x.
            1 x 273 x 513 is the second-tile-per-workgroup case (the next-tile X prefetch): the test reads the CU count and asserts tiles > grid for every form.
Compact     forms 0 / 1, all four (in_c8, out_c8) combinations: the same values bit for bit as the two-group run; the 48 unused bytes per pixel keep their fill.
Guards      both slabs lie between guard bands (-3.0 around the output, NaN around the input and the blob), a sentinel group lies behind the output's last group, the output
            is 0xFF before the launch; the pad channels 40 .. 63 of a two-group output are zero (include/innfer_amd.h), everything else keeps its fill.
Bit-equal   form 0 = form 1 = form -1; N = 3 = three N = 1 launches, every form; a second launch over a poisoned output gives the same bits.
Conversions innfer_pan_split_from_nchw = the numpy layout bit for bit; to_nchw(from_nchw(x)) = x to the pair's 22 bits.
Refusals    every refused argument set returns its error and writes nothing.
Wiring      PAN nb = 4 whose SCPA convs are scaled until the block shows (tests/_pan_scpa_ref.py wiring()), fused_scpa in {1, 0, 6, 7, 3} fp16 and {1, 0} fp32 mode, against
            oracle.pan_forward at the networks' bounds; that every planted fault would miss those bounds by >= 3x is recomputed and asserted before the device runs.

Measured on the MI355X -- docs/KERNELS.md section 3.5c; test_report prints the table.
"""

import numpy as np
import pytest
import torch

import _pan_scpa_ref as R

pytestmark = pytest.mark.gpu

SENT = -3.0
GUARD = 4096                       # fp16 elements
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -3
MEASURED = {}                      # (form, family) -> [largest e_model / e_split, worst err / bound]
FORM_NAME = {0: "0 fused<16>", 1: "1 duo", -1: "-1 default", 2: "2 split"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def record(key, eref, ratio):
    m = MEASURED.setdefault(key, [0.0, 0.0])
    m[0], m[1] = max(m[0], eref), max(m[1], ratio)


_blobs = {}


def blob(dev, family, split):
    """The packed weights of the family on the device, NaN on both sides: -> (buffer, pointer to the blob)."""
    import innfer_amd.lib as L
    if (family, split) not in _blobs:
        w = {k: np.ascontiguousarray(v.numpy(), dtype=np.float32) for k, v in R.weights(family).items()}
        n = L.lib.innfer_pan_scpa_blob_bytes(split)
        assert n > 0 and n % 2 == 0 and (split == 0 or n == 2 * ((L.lib.innfer_pan_scpa_blob_bytes(0) + 255) // 256 * 256))
        h = np.zeros(n, dtype=np.uint8)
        rc = L.lib.innfer_pack_pan_scpa(*(w[k].ctypes.data for k in R.KEYS), split, h.ctypes.data)
        assert rc == OK, L.last_error()
        buf = np.full(2 * GUARD + n // 2, np.nan, dtype=np.float16)
        buf[GUARD:GUARD + n // 2] = h.view(np.float16)
        _blobs[(family, split)] = torch.from_numpy(buf).to(dev)
    d = _blobs[(family, split)]
    return d, d.data_ptr() + 2 * GUARD


def bits(a):
    return a.view(np.uint16) if isinstance(a, np.ndarray) else a.view(torch.int16)


def launch(dev, x, family, form, in_c8=0, out_c8=0, again=False):
    """One innfer_pan_scpa_block of x [N][40][H][W] (a float32 tensor on the fp16 grid; form 2: any float32) -> the result [N][40][H][W] (fp16 forms: a torch fp16
    tensor; form 2: hi + 2^-11 lo in float64) and the raw output elements.  Checks the guards, the sentinel group, the pad channels and the unused bytes.
    again: poisons the output and launches a second time; both results must have the same bits."""
    import innfer_amd.lib as L
    N, _, H, W = x.shape
    npx = N * H * W
    split = form == 2
    body_in = R.to_split_planes(x) if split else R.to_slab(x, bool(in_c8), fill=0.0, rest=np.nan)
    n_out = npx * 80 if split else npx * 64
    sent = 0 if split else npx * 32                                    # a sentinel group behind the output's last group
    h_in = np.full(2 * GUARD + body_in.size, np.nan, dtype=np.float16)
    h_in[GUARD:GUARD + body_in.size] = body_in
    d_in = torch.from_numpy(h_in).to(dev)
    d_out = torch.full((2 * GUARD + n_out + sent,), SENT, dtype=torch.float16, device=dev)
    _, p_blob = blob(dev, family, 1 if split else 0)
    runs = []
    for _ in range(2 if again else 1):
        d_out[GUARD:GUARD + n_out].view(torch.int16).fill_(-1)         # 0xFFFF
        rc = L.lib.innfer_pan_scpa_block(d_in.data_ptr() + 2 * GUARD, d_out.data_ptr() + 2 * GUARD, 0 if split else npx * 32, p_blob, N, H, W, form, in_c8, out_c8, stream())
        torch.cuda.synchronize()
        assert rc == OK, (rc, L.last_error())
        runs.append(d_out.cpu().numpy())
    what = f"{N}x{H}x{W} {family} form {form} c8 {in_c8}{out_c8}"
    o = runs[0]
    if again:
        assert np.array_equal(bits(o), bits(runs[1])), f"{what}: a second launch over a poisoned output gives other bits"
    assert (o[:GUARD] == SENT).all() and (o[GUARD + n_out:] == SENT).all(), f"{what}: the launch wrote outside its output (guards / sentinel group)"
    assert torch.equal(bits(d_in.cpu()), bits(torch.from_numpy(h_in))), f"{what}: the launch wrote to its input"
    raw = o[GUARD:GUARD + n_out]
    if split:
        got = R.from_split_planes(raw, N, H, W)
        assert torch.isfinite(got).all(), f"{what}: non-finite or unwritten values"
        return got, raw
    got, rest = R.from_slab(raw, N, H, W, bool(out_c8))
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite or unwritten values"
    if out_c8:
        assert (bits(rest) == 0xFFFF).all(), f"{what}: a compact output must leave the other 48 bytes per pixel of group 1 alone"
    else:
        assert (bits(rest) == 0).all(), f"{what}: the pad channels 40 .. 63 of a two-group output are written as zeros"
    return got, raw


def tiles_and_grid(dev, N, H, W, form):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    th = 16 if form == 0 else 8
    return N * ((H + th - 1) // th) * ((W + 31) // 32), (2 * cus if form in (1, -1) else cus)


# ------------------------------------------------------------------------------------------------ the forms against float64
@pytest.mark.parametrize("c", R.cases(), ids=str)
def test_block_vs_float64(dev, c):
    x, f = R.data(c), R.figures(c)
    if (c.N, c.H, c.W) == R.BIG:
        for form in (0, 1, -1, 2):
            tiles, grid = tiles_and_grid(dev, c.N, c.H, c.W, form)
            print(f"[pan-scpa] {c} form {form}: {tiles} tiles on {grid} workgroups")
            assert tiles > grid, f"form {form}: {tiles} tiles on {grid} workgroups -- no workgroup takes a second tile: the next-tile prefetch is not covered on this part"
    raws = {}
    for form in (0, 1, -1):
        got, raws[form] = launch(dev, x, c.family, form)
        g = got.double()
        ratio = ((g - f["model64"]).abs() / R.bound16(c, g)).max().item()
        print(f"[pan-scpa] {c} form {form}: e_model {f['e_model']:.2e} trans {f['trans']:.2e}; max err {(g - f['model64']).abs().max().item():.2e} worst err/bound {ratio:.3f}")
        record((FORM_NAME[form], c.family), f["e_model"], ratio)
        assert ratio <= 1.0, f"{c} form {form}: worst err / bound {ratio:.3f}"
    assert np.array_equal(bits(raws[0]), bits(raws[1])), f"{c}: pan_scpa_fused<16> and pan_scpa_duo differ in {(bits(raws[0]) != bits(raws[1])).sum()} elements"
    assert np.array_equal(bits(raws[1]), bits(raws[-1])), f"{c}: the default form is not form 1's bits"
    got, _ = launch(dev, x, c.family, 2)
    e, b = (got - f["exact"]).abs().max().item(), R.bound_split(c)
    print(f"[pan-scpa] {c} form 2: e_split {f['e_split']:.2e} trans {f['trans']:.2e}; max err {e:.2e} bound {b:.2e} err/bound {e / b:.3f} err/(8 e_split) {e / (R.MARGIN * f['e_split']):.3f}")
    record((FORM_NAME[2], c.family), f["e_split"], e / b)
    assert e <= b, f"{c} form 2: |device - exact| {e:.3e} > {b:.3e}"


# ------------------------------------------------------------------------------------------------ the compact plane
@pytest.mark.parametrize("c", R.cases(R.C8_SHAPES), ids=str)
def test_compact_plane_is_bit_equal(dev, c):
    x = R.data(c)
    for form in (0, 1):
        ref, _ = launch(dev, x, c.family, form)
        for in_c8, out_c8 in ((1, 0), (0, 1), (1, 1)):
            got, _ = launch(dev, x, c.family, form, in_c8, out_c8)
            assert torch.equal(bits(got), bits(ref)), f"{c} form {form} in_c8 {in_c8} out_c8 {out_c8}: {(bits(got) != bits(ref)).sum().item()} values differ from the two-group run"


# ------------------------------------------------------------------------------------------------ batches, relaunch
@pytest.mark.parametrize("family", R.FAMILIES)
def test_batch_images_equal_their_own_launches(dev, family):
    c = R.Case(family, 3, 37, 45)
    x = R.data(c)
    for form, c8 in ((0, 0), (1, 0), (-1, 0), (1, 1), (0, 1), (2, 0)):
        got, _ = launch(dev, x, family, form, c8, c8)
        for n in range(3):
            own, _ = launch(dev, x[n:n + 1].contiguous(), family, form, c8, c8)
            same = torch.equal(got[n:n + 1], own) if form == 2 else torch.equal(bits(got[n:n + 1].contiguous()), bits(own))
            assert same, f"{c} form {form} c8 {c8}: image {n} of the batch differs from its own launch"


@pytest.mark.parametrize("shape", [(1, 9, 33), (3, 37, 45), R.BIG], ids=str)
def test_second_launch_over_poisoned_output(dev, shape):
    c = R.Case("live", *shape)
    for form, c8 in ((0, 0), (1, 0), (1, 1), (2, 0)):
        launch(dev, R.data(c), c.family, form, c8, c8, again=True)


def test_split_form_with_full_precision_input(dev):
    """The cases above feed form 2 an x on the fp16 grid (its lo planes are zero).  Here x is unrounded float32: the input's lo planes carry weight.  `flat` only:
    an x rounded to fp16 moves the output by 2^-12 |x|, which the flat family's bound sees 50-fold (asserted); in `live` the hardware sigmoid's allowance times that
    family's gain (trans) is itself within 8x of an fp16 rounding of x, so the case would not discriminate there."""
    fam = "flat"
    x = torch.from_numpy(np.random.default_rng(1937).uniform(-1, 1, (2, 40, 19, 37)).astype(np.float32))
    w = R.weights(fam)
    parts = {}
    with torch.no_grad():
        exact = R.block(x, w, torch.float64, None, parts=parts)
        e_split = (R.block(x, w, torch.float64, "split") - exact).abs().max().item()
        dropped = (R.block(R.r16(x), w, torch.float64, None) - exact).abs().max().item()
    bound = R.MARGIN * e_split + R.TRANS * float(parts["c"].abs().max()) * R.gain(w)
    assert dropped > 10 * bound                             # an input whose lo planes were ignored would show
    got, _ = launch(dev, x, fam, 2)
    e = (got - exact).abs().max().item()
    print(f"[pan-scpa] {fam} 2x19x37 unrounded x, form 2: e_split {e_split:.2e}; max err {e:.2e} bound {bound:.2e} err/bound {e / bound:.3f} (lo planes dropped: {dropped / bound:.0f})")
    record((FORM_NAME[2] + ", fp32 x", fam), e_split, e / bound)
    assert e <= bound


# ------------------------------------------------------------------------------------------------ the split conversions
@pytest.mark.parametrize("shape", [(1, 4, 4), (2, 6, 40), (3, 37, 45)], ids=str)
def test_split_conversions(dev, shape):
    import innfer_amd.lib as L
    N, H, W = shape
    npx = N * H * W
    x = torch.from_numpy(np.random.default_rng(11 * H + W).uniform(-1, 1, (N, 40, H, W)).astype(np.float32))
    x[0, 0, 0, :4] = torch.tensor([0.0, 1.0, -2.0 ** -20, 1.0 + 2.0 ** -12])
    d_x = x.to(dev)
    d_pl = torch.full((2 * GUARD + npx * 80,), SENT, dtype=torch.float16, device=dev)
    assert L.lib.innfer_pan_split_from_nchw(d_x.data_ptr(), d_pl.data_ptr() + 2 * GUARD, N, H, W, stream()) == OK, L.last_error()
    d_back = torch.full((2 * GUARD + npx * 40,), SENT, dtype=torch.float32, device=dev)
    assert L.lib.innfer_pan_split_to_nchw(d_pl.data_ptr() + 2 * GUARD, d_back.data_ptr() + 4 * GUARD, N, H, W, stream()) == OK, L.last_error()
    torch.cuda.synchronize()
    pl, back = d_pl.cpu().numpy(), d_back.cpu()
    assert (pl[:GUARD] == SENT).all() and (pl[-GUARD:] == SENT).all() and (back[:GUARD] == SENT).all() and (back[-GUARD:] == SENT).all()
    want = R.to_split_planes(x)
    assert np.array_equal(bits(pl[GUARD:-GUARD]), bits(want)), f"{(bits(pl[GUARD:-GUARD]) != bits(want)).sum()} elements of the split planes differ from the documented layout"
    back = back[GUARD:-GUARD].reshape(N, 40, H, W).double()
    assert torch.equal(back, R.from_split_planes(want, N, H, W))                      # hi + 2^-11 lo is exact in fp32
    assert ((back - x.double()).abs() <= 2.0 ** -22 * x.double().abs() + 2.0 ** -36).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(dev):
    import innfer_amd.lib as L
    N, H, W = 1, 9, 33
    npx = N * H * W
    d_in = torch.zeros(npx * 80, dtype=torch.float16, device=dev)
    d_out = torch.full((npx * 80,), SENT, dtype=torch.float16, device=dev)
    d_f32 = torch.full((npx * 40,), SENT, dtype=torch.float32, device=dev)
    _, b16 = blob(dev, "flat", 0)
    _, b32 = blob(dev, "flat", 1)
    G = npx * 32
    i, o = d_in.data_ptr(), d_out.data_ptr()
    call = L.lib.innfer_pan_scpa_block
    for form, bl, g in ((0, b16, G), (1, b16, G), (-1, b16, G), (2, b32, 0)):
        assert call(None, o, g, bl, N, H, W, form, 0, 0, stream()) == ERR_INVALID
        assert call(i, None, g, bl, N, H, W, form, 0, 0, stream()) == ERR_INVALID
        assert call(i, o, g, None, N, H, W, form, 0, 0, stream()) == ERR_INVALID
        for n, h, w in ((0, H, W), (N, 0, W), (N, H, 0), (-1, H, W)):
            assert call(i, o, g, bl, n, h, w, form, 0, 0, stream()) == ERR_INVALID
    for form in (3, -2, 7):
        assert call(i, o, G, b16, N, H, W, form, 0, 0, stream()) == ERR_INVALID
    assert call(i, o, G - 1, b16, N, H, W, 0, 0, 0, stream()) == ERR_INVALID          # groups that overlap
    assert call(i, o, G, b32, N, H, W, 2, 0, 0, stream()) == ERR_INVALID              # the split form takes no group stride ..
    assert call(i, o, 0, b32, N, H, W, 2, 1, 0, stream()) == ERR_INVALID and call(i, o, 0, b32, N, H, W, 2, 0, 1, stream()) == ERR_INVALID          # .. and no compact plane
    for form in (0, 1, -1):                                                           # 2^25 pixels: 64 npx + 2 G beyond 32-bit byte offsets
        assert call(i, o, 1 << 30, b16, 1, 4096, 8192, form, 0, 0, stream()) == ERR_UNSUPPORTED
    assert call(i, o, 0, b32, 1, 4096, 4096, 2, 0, 0, stream()) == ERR_UNSUPPORTED      # 160 npx beyond 32-bit byte offsets
    for conv in (L.lib.innfer_pan_split_from_nchw, L.lib.innfer_pan_split_to_nchw):
        a, b = (d_f32.data_ptr(), o) if conv is L.lib.innfer_pan_split_from_nchw else (o, d_f32.data_ptr())
        assert conv(None, b, N, H, W, stream()) == ERR_INVALID and conv(a, None, N, H, W, stream()) == ERR_INVALID
        assert conv(a, b, 0, H, W, stream()) == ERR_INVALID and conv(a, b, N, 0, W, stream()) == ERR_INVALID and conv(a, b, N, H, 0, stream()) == ERR_INVALID
        assert conv(a, b, 1, 4096, 4096, stream()) == ERR_UNSUPPORTED
    assert L.lib.innfer_pack_pan_scpa(None, None, None, None, None, None, None, None, 0, None) == ERR_INVALID
    torch.cuda.synchronize()
    assert (d_out == SENT).all().item() and (d_f32 == SENT).all().item(), "a refused launch wrote"
    assert call(i, o, G, b16, N, H, W, -1, 0, 0, stream()) == OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the wiring
@pytest.mark.parametrize("fp32", [False, True], ids=["fp16", "fp32"])
def test_network_with_visible_scpa_blocks(dev, fp32):
    """PAN nb = 4, seed 41, 50 x 70, SCPA convs x 2.75 (k2 x 11): every schedule of the trunk against the oracle at the networks' bounds.  The five-launch schedule
    has no single-block entry (it lives on the network's conv list); this is where it, the blob packing from the state dict and the compact plane between the blocks
    are held to weights that show the block."""
    from innfer_amd.architectures import get_network
    from innfer_amd.utils.defaults import get_network_G_config
    wr = R.wiring()
    for line in R.assert_wiring_discriminates(wr):
        print("[pan-scpa] wiring:", line)
    ref, lim = wr["ref"], wr["lim"]
    net = get_network(get_network_G_config({"type": "pan", "nb": 4}, 4))
    net.load_state_dict(wr["sd"], strict=True)
    net = net.to(dev).eval()
    ys = {}
    for mode in ((1, 0) if fp32 else (1, 0, 6, 7, 3)):
        net.fused_scpa = mode
        if fp32:
            y = net(wr["x"].to(dev))
            assert y.dtype == torch.float32
            e = (y.cpu() - ref).abs().max().item()
            print(f"[pan-scpa] wiring fp32 mode, fused_scpa {mode}: max {e:.2e} (bound {R.NET_FP32 * lim:.2e})")
            record((f"network fp32 mode, fused_scpa {mode}", "x2.75"), 0.0, e / (R.NET_FP32 * lim))
            assert e < R.NET_FP32 * lim, (mode, e)
        else:
            y = net(wr["x"].to(dev).half())
            d = (y.float().cpu() - ref).abs()
            print(f"[pan-scpa] wiring fp16, fused_scpa {mode}: max {d.max().item():.2e} mean {d.mean().item():.2e} (bounds {R.NET_MAX * lim:.2e} / {R.NET_MEAN:.1e})")
            record((f"network fp16, fused_scpa {mode}", "x2.75"), 0.0, max(d.max().item() / (R.NET_MAX * lim), d.mean().item() / R.NET_MEAN))
            assert d.max().item() < R.NET_MAX * lim and d.mean().item() < R.NET_MEAN, (mode, d.max().item(), d.mean().item())
        ys[mode] = y
    d01 = (ys[1].float() - ys[0].float()).abs()
    print(f"[pan-scpa] wiring {'fp32 mode' if fp32 else 'fp16'}: one launch per block against the {'generic fp32 convs' if fp32 else 'five launches'}: max {d01.max().item():.2e}, "
          f"{(d01 > 0).float().mean().item():.3f} of the values differ")
    assert (d01 > 0).any(), "fused_scpa 0 and 1 gave the same bits: the schedule switch did not act"          # (other summation orders: the same bits would mean one schedule ran twice)
    if not fp32:
        assert torch.equal(ys[6], ys[7]) and torch.equal(ys[6], ys[1]) and torch.equal(ys[3], ys[1]), "the block kernel's forms / the compact plane change the network's bits"


def test_report():
    """The table of docs/KERNELS.md 3.5c: per form and family the largest e_model / e_split and the worst err / bound of this run."""
    print("\n[pan-scpa] form | family | largest e_model / e_split | worst err / bound")
    for (form, fam), (eref, ratio) in sorted(MEASURED.items(), key=lambda kv: tuple(map(str, kv[0]))):
        print(f"[pan-scpa] {form} | {fam} | {eref:.1e} | {ratio:.3f}")
