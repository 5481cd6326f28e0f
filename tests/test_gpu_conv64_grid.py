"""The 2 x 4 consumer grid of the 64-output slab convs (conv3x3_pc<4, 2, .., TMF | PC_GRID2>) against the 8 x 1 form, bit for bit (needs an MI355X: `pytest -m gpu`).

The grid splits a tile's 16 rows x 64 channels among the eight consumer waves as 4 row groups x 2 channel halves instead of 8 row groups, and loads the one memory
residual at the top of a tile's last chunk instead of the top of the epilogue.  Every accumulator sees the same MFMAs in the same order and the same epilogue
arithmetic, so the two forms must agree in every bit, guard bands and foreign channel groups included (torch.equal on the whole buffer).  innfer_conv3x3_f16_grid
launches either form on the same operands; one case is also held to float64 (the bound of tests/_conv_ref.py: ulp16 / 2 + 8 e32, e32 from the float32 CPU conv), so
that the new form is not only compared with its sibling; the network level compares innfer_net_set_consumer_grid 1 against 0 under every residual_lds mode.

Shapes: one tile (16 x 32), four ragged tiles (17 x 33), a frame smaller than a tile (5 x 7), 40 x 70 with N = 2 (laid out as an image canvas, a form the grid does
not have: both calls run the 8 x 1 kernel -- the selection must not break it), two images that are NOT a canvas (2 x 17 x 33, and 2 x 40 x 70 with a row range: n > 0
in the new form), and 272 x 512 = 272 tiles for 256 workgroups, where a workgroup's second tile issues its prefetch across the persistent loop.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _conv_ref as R
from _conv_ref import Case

pytestmark = pytest.mark.gpu

FILL, GUARD = -3.0, 4096
RES = ("none", "mem1", "lds1", "lds1+res2", "mem2")
SIZES = [(1, 16, 32), (1, 17, 33), (1, 5, 7), (2, 40, 70), (2, 17, 33)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class _Operands:
    """The device operands of one case, shared by every launch of it: input slab (+ a junk group), plane-order panels, bias, two residual slabs."""

    def __init__(self, dev, c):
        import innfer_amd.lib as L
        x, w, b = R.data(c)
        self.c, self.x = c, x
        self.xin = R.to_slab(x, c.C // 32 + 1).to(dev)
        wc = np.ascontiguousarray(w.numpy(), dtype=np.float32)
        packed = np.zeros(L.lib.innfer_conv3x3_packed_bytes(c.K, c.C), dtype=np.uint8)
        L.check(L.lib.innfer_pack_conv3x3_rows(wc.ctypes.data, c.K, c.C, 1, packed.ctypes.data))
        self.packed = torch.from_numpy(packed).to(dev)
        self.bias = b.to(dev)
        shape = (c.N, c.K, c.H, c.W)
        self.r = [R.residual(c, 1, shape), R.residual(c, 2, shape)]
        self.rs = [R.to_slab(r).to(dev) for r in self.r]


def _launch(dev, ops, grid, act=0, res="none", rows=None, s1=0.2, s2=0.2):
    """One launch through innfer_conv3x3_f16_grid; returns the whole buffer (guard bands, a foreign group behind the output) on the host."""
    import innfer_amd.lib as L
    c = ops.c
    g = c.N * c.H * c.W * 32
    numel = 3 * g                                             # the conv's two groups + one foreign group
    buf = torch.full((numel + 2 * GUARD,), FILL, dtype=torch.float16, device=dev)
    a = L.ConvArgs()
    a.d_in, a.in_group_stride, a.C = ops.xin.data_ptr(), g, c.C
    a.d_packed, a.d_bias = ops.packed.data_ptr(), ops.bias.data_ptr()
    a.d_out, a.out_group_stride, a.out_ch_off, a.K = buf.data_ptr() + GUARD * 2, g, 0, c.K
    a.N, a.H, a.W, a.act, a.plane_rows = c.N, c.H, c.W, act, 1
    if res in ("mem1", "mem2"):
        a.d_res1, a.res1_group_stride, a.res1_scale = ops.rs[0].data_ptr(), g, s1
    if res in ("lds1", "lds1+res2"):                          # x5 * 0.2 + x: the residual is the conv's own input groups 0, 1
        a.d_res1, a.res1_group_stride, a.res1_scale, a.res1_from_input = ops.xin.data_ptr(), g, s1, 1
    if res in ("mem2", "lds1+res2"):
        a.d_res2, a.res2_group_stride, a.res2_scale = ops.rs[1].data_ptr(), g, s2
    if rows:
        a.row_begin, a.row_end = rows
    rc = L.lib.innfer_conv3x3_f16_grid(C.byref(a), grid, None)
    torch.cuda.synchronize()
    assert rc == 0, (str(c), grid, act, res, rows, L.last_error())
    return buf.cpu()


def _same(dev, ops, **kw):
    new, old = _launch(dev, ops, 1, **kw), _launch(dev, ops, 0, **kw)
    what = f"{ops.c} {kw}"
    assert bool((old[:GUARD] == FILL).all()) and bool((old[-GUARD:] == FILL).all()), f"{what}: the 8 x 1 form wrote outside the output"
    assert bool((old[GUARD:-GUARD] != FILL).any()), f"{what}: nothing was written"
    assert torch.equal(new, old), f"{what}: {(new != old).sum().item()} of {new.numel()} values differ between the 2 x 4 and the 8 x 1 consumer grid"


@pytest.mark.parametrize("Cc", [64, 192])
def test_grid_equals_8x1_bit_for_bit(dev, Cc):
    """Every size x residual combination x activation (res1 from LDS exists for act 0 and C >= 96; elsewhere the launch takes res1 from memory, on both forms)."""
    for i, (N, H, W) in enumerate(SIZES):
        ops = _Operands(dev, Case("3x3", N, Cc, 64, H, W, seed=300 + i))
        for res in RES:
            for act in (0, 1, 2):
                _same(dev, ops, act=act, res=res)


@pytest.mark.parametrize("Cc", [64, 192])
def test_row_range_that_cuts_a_tile(dev, Cc):
    """Rows [5, 30) of 40: tiles start at row 5, the second one is cut at row 30 (a wave's row group partly outside); one image and a batch (no canvas with a row range)."""
    for N in (1, 2):
        ops = _Operands(dev, Case("3x3", N, Cc, 64, 40, 70, seed=310 + N))
        for res in RES:
            _same(dev, ops, act=0, res=res, rows=(5, 30))
        _same(dev, ops, act=1, res="mem1", rows=(3, 12))


def test_second_tile_of_a_workgroup(dev):
    """272 x 512 at C = 64: 272 tiles for 256 workgroups -- sixteen workgroups run a second tile, whose prefetch is issued inside the persistent loop."""
    ops = _Operands(dev, Case("3x3", 1, 64, 64, 272, 512, seed=320))
    for res, act in (("mem1", 0), ("mem2", 1), ("none", 2)):
        _same(dev, ops, act=act, res=res)


def test_grid_against_float64(dev):
    """C = 192, 17 x 33, res1 + res2 from memory on the 2 x 4 grid against the float64 conv and epilogue: |got - ref| <= ulp16 / 2 + 8 e32."""
    c = Case("3x3", 1, 192, 64, 17, 33, seed=330)
    ops = _Operands(dev, c)
    y64, e32 = R.pre(c)
    for act in (0, 1):
        raw = _launch(dev, ops, 1, act=act, res="mem2")
        got = R.from_slab(raw[GUARD:-GUARD].reshape(3, c.N, c.H, c.W, 32))
        assert bool((got[:, 64:] == FILL).all()), "the foreign group of the slab was written"
        ref, _ = R.epilogue(y64, act, 0, ops.r[0].double(), 0.2, ops.r[1].double(), 0.2)
        R.assert_within_fp16_rounding(got[:, :64], ref, e32, what=f"{c} 2 x 4 grid act {act} res1 + res2", family="3x3 64 outputs, 2 x 4 consumer grid")


def test_network_level_consumer_grid(dev):
    """RRDBNet (nb = 2) on 1 x 3 x 40 x 70: consumer_grid 1 against 0, bit for bit, with the dense blocks' residual from memory (0), from LDS at the RRDB ends (1)
    and from LDS everywhere (2)."""
    from innfer_amd import synth
    from innfer_amd.architectures.RRDBNet_arch import RRDBNet
    sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.rrdbnet_shapes(nb=2, scale=4), 7).items()}
    net = RRDBNet(3, 3, 64, 2, upscale=4)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    x = torch.from_numpy(synth.uniform((1, 3, 40, 70), 71)).to(dev).half()
    for mode in (0, 1, 2):
        net.residual_lds = mode
        ys = {}
        for grid in (1, 0):
            net.consumer_grid = grid
            ys[grid] = net(x).cpu()
        assert torch.isfinite(ys[0]).all() and ys[0].abs().max().item() > 0
        assert torch.equal(ys[1], ys[0]), f"residual_lds {mode}: {(ys[1] != ys[0]).sum().item()} values differ between consumer_grid 1 and 0"
