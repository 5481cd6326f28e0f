"""The workspace of the eight newer network engines held to poison and guards (needs an MI355X: `pytest -m gpu`): SRVGGNetCompact (kind 2), SPAN (3), RealPLKSR (4),
SwinIR (5), HAT (6), Swin2SR (7), DAT (8), DRCT (9).  No reference value is computed: every assertion is bit-equality (torch.equal on integer views), a fill check or a
status.  innfer_net_forward is driven through innfer_amd.lib with a workspace the test owns: one uint8 tensor of 2 x need bytes, need = innfer_net_workspace_bytes; the
forward gets the first half, the second half is the guard (as large as the workspace: an undercount of a whole region shows, not only a spill).  The result lies in a
buffer of its own between guard bands of 4096 elements (fill -3.0; 0xA5 for uint8), as in the single-launch tests.

1. Poison independence.  y0 with the workspace all 0x00; then all 0xFF (NaN as fp16 and as fp32); then all 0x7B (fp16 0x7B7B = 6.1e4, fp32 1.3e36: finite, huge).  The
   three results are bit-equal and finite.  fmaxf(NaN, x) = x and a compare-and-select drops NaN, so a running maximum or a ReLU hides a NaN it read -- the huge finite
   value shows there; NaN x 0 shows where huge x 0 does not.  Both patterns are needed.
2. Containment.  After every forward the guard half of the workspace and the result's guard bands hold their fill; the input is unchanged.
3. Refusal.  workspace_bytes = need - 1: INNFER_ERR_WORKSPACE, and workspace, guard and result keep their fill (nothing launched); the same with a NULL workspace
   (as found a NULL workspace was INNFER_ERR_INVALID; innfer_net_forward now answers a short and a missing workspace alike, as innfer_pan_attention does).
4. Shape sequences on one net through the Python module, which keeps `_ws` while it is large enough: the family's batch of two, then a smaller padded shape, then the
   batch again.  The small result equals that of a freshly built net that never saw another shape; the second large result equals the first; `_ws.data_ptr()` is
   asserted unchanged (the reuse is live).  Once as found and once with `_ws.fill_(0x7B)` between the forwards.
5. Batch tail.  N = 2 in a poisoned workspace, then N = 1 of sample 1 in the SAME workspace (now the stale bytes of the N = 2 layout): equal to y[1:].
1 - 3 run fp16 -> fp16 on every case and uint8 -> uint8 (the reflect pad reads HWC bytes, the crop writes codes) on one padded case per family.

What each family rests on, and what was found (MI355X):
    family   invariant the forward relies on                                                                                    outcome
    compact  two ping-pong slabs and the last conv's 32- / 64-channel slab; pad channels of nf < 64 come from zero weight rows  passed as found
    span     the concat slab f0 | conv_2 | b1 | b5_2 is written group by group before conv_cat reads it                         passed as found
    plksr    GroupNorm's records and affine (`tmp`) are written by the stats launch of the same block; [U0 | T0 | U1] groups      passed as found
    swinir   the qkv pad contract: "head_dim real channels, then zeros" must come from zero rows of the packed qkv slices         passed as found
             (d = 10 / 30 in a 32-group; a spare half slice when 3 nH is odd); pad channels of C = 60 / 180 / 240 in 64-slabs
    hat      as swinir on the 16-grid, plus zc / z / y / pool of the conv block and the channel attention's segment sums        passed as found
    swin2sr  as swinir; the cosine attention normalises q and k over the 32-group (a pad channel that is not zero enters)       passed as found
    dat      qkv pad contract for both attentions, the dwconv on the v groups, `pool` / `gram` / `amat` segment records,         passed as found
             x1 | x2 halves of the hidden slab with their own pad channels
    drct     the dense slab: no group is read by a product before it is written; rounded-up groups hold zeros of the launch    passed as found
             before (csrc/net.hip, the comment in front of the DRCT loop)
"""
import functools

import pytest
import torch

import _compact_ref as CR
import _dat_ref as DTR
import _drct_ref as DCR
import _hat_ref as HR
import _plksr_ref as PR
import _span_ref as SPR
import _swin2sr_ref as S2
import _swinir_ref as SR

pytestmark = pytest.mark.gpu

FILL, GUARD = -3.0, 4096
FILL_U8 = 0xA5                       # guard bands of a uint8 result, and the guard half of every workspace
PATTERNS = (0x00, 0xFF, 0x7B)        # the reference run, NaN (fp16 0xFFFF, fp32 0xFFFFFFFF), huge and finite (fp16 6.1e4, fp32 1.3e36)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ the nets
def _from_sd(sd, **extra):
    from innfer_amd.architectures import get_network
    from innfer_amd.run import infer_from_state_dict
    info = infer_from_state_dict({"params_ema": sd})
    net = get_network(dict(info["net_params"], **extra))
    net.load_state_dict(info["state_dict"], strict=True)
    return net


def _dat(name):
    from innfer_amd.architectures.DAT_arch import DAT
    Cc, nH, split, depths, ef, ups, resi, s, shape, seed = DTR.FIXTURES[name]
    net = DAT(in_chans=shape[1], embed_dim=Cc, split_size=list(split), depth=list(depths), num_heads=[nH] * len(depths), expansion_factor=ef, upscale=s, upsampler=ups,
              resi_connection=resi)
    net.load_state_dict(DTR.fixture_sd(name), strict=True)
    return net


def _plksr(name):
    nb, s, shape, k, ea, seed = PR.FIXTURES[name]
    return _from_sd(PR.fill(3, 64, nb, s, k, ea, seed))


# family -> {label: (builder of the net (state dict of an existing fixture), (N, H, W), seed of the input)}.  Shapes <= 48 x 48.  The first label with "u8" in its flags is
# the family's uint8 case, the one flagged "batch" its batch of two (the large shape of the sequences), the one flagged "small" gives the sequences' small padded shape.
CASES = {
    "compact": {
        "nf64 2 convs x4 13x21": (lambda: _from_sd(CR.fill(3, 64, 2, 4, seed=12)), (1, 13, 21), 12, "u8 small"),
        "nf64 1 conv x3 9x17": (lambda: _from_sd(CR.fill(3, 64, 1, 3, seed=11)), (1, 9, 17), 11, ""),
        "nf64 no nf->nf conv x1 9x17": (lambda: _from_sd(CR.fill(3, 64, 0, 1, seed=10)), (1, 9, 17), 10, ""),
        "nf24 2 convs x4 19x23": (lambda: _from_sd(CR.fill(3, 24, 2, 4, seed=32)), (1, 19, 23), 32, ""),
        "nf32 2 convs x2 batch of two 19x26": (lambda: _from_sd(CR.fill(3, 32, 2, 2, seed=31)), (2, 19, 26), 31, "batch"),
    },
    "span": {
        "f48 x4 13x21": (lambda: _from_sd(SPR.fill(3, 48, 4, 1)), (1, 13, 21), 1, "u8 small"),
        "f52 x3 9x17": (lambda: _from_sd(SPR.fill(3, 52, 3, 3)), (1, 9, 17), 3, ""),
        "f48 x2 norm=False 13x21": (lambda: _from_sd(SPR.fill(3, 48, 2, 5, False)), (1, 13, 21), 5, ""),
        "f48 x2 deploy batch of two 19x26": (lambda: _from_sd(SPR.fill(3, 48, 2, 6, True, True)), (2, 19, 26), 6, "batch"),          # (a deploy net uploads at once: the sequences build two)
    },
    "plksr": {
        "2 blocks k17 x2 13x21": (lambda: _plksr("2 blocks x2 21x37"), (1, 13, 21), 2, "u8 small"),
        "2 blocks k17 x3 9x17": (lambda: _plksr("2 blocks x3 9x17"), (1, 9, 17), 3, ""),
        "S (k 13, no EA) x2 13x21": (lambda: _plksr("S (k 13, no EA) x2 20x24"), (1, 13, 21), 5, ""),
        "2 blocks k17 x2 batch of two 19x26": (lambda: _plksr("batch of two x2 19x26"), (2, 19, 26), 6, "batch"),
    },
    "swinir": {
        "C60 [2,2] direct x2 16x24": (lambda: _from_sd(SR.fixture_sd("C60 [2,2] direct x2 16x24")), (1, 16, 24), 1, ""),
        "C60 [2,2] direct x4 13x21": (lambda: _from_sd(SR.fixture_sd("C60 [2,2] direct x4 13x21 (padded)")), (1, 13, 21), 2, "u8 small"),
        "C180 [2] pixelshuffle x4 16x16": (lambda: _from_sd(SR.fixture_sd("C180 [2] pixelshuffle x4 16x16")), (1, 16, 16), 3, ""),
        "C180 [2] pixelshuffle x3 9x17": (lambda: _from_sd(SR.fixture_sd("C180 [2] pixelshuffle x3 9x17")), (1, 9, 17), 4, ""),
        "C240 nH8 [2] 3conv nearest+conv x4 13x21": (lambda: _from_sd(SR.fixture_sd("C240 [2] 3conv nearest+conv x4 16x24")), (1, 13, 21), 5, ""),
        "C64 nH2 [2] nearest+conv x2 9x17": (lambda: _from_sd(SR.fixture_sd("C64 [2] nearest+conv x2 8x8")), (1, 9, 17), 6, ""),
        "C60 [2] pixelshuffle x2 batch of two 19x26": (lambda: _from_sd(SR.fixture_sd("C60 [2] batch of two pixelshuffle x2 19x26")), (2, 19, 26), 7, "batch"),
    },
    "hat": {
        "C60 [2] x2 16x16": (lambda: _from_sd(HR.fixture_sd("C60 [2] x2 16x16 cs1"), conv_scale=1.0), (1, 16, 16), 1, ""),
        "C60 [1,1] x4 13x21": (lambda: _from_sd(HR.fixture_sd("C60 [1,1] x4 13x21 (padded) cs1"), conv_scale=1.0), (1, 13, 21), 2, "u8 small"),
        "C180 [2] x3 32x48 cs0.01": (lambda: _from_sd(HR.fixture_sd("C180 [2] x3 32x48 cs0.01"), conv_scale=0.01), (1, 32, 48), 3, ""),
        "C144 [2] x2 batch of two 19x26": (lambda: _from_sd(HR.fixture_sd("C144 [2] x2 batch of two 19x26 cs1 (formula indices)"), conv_scale=1.0), (2, 19, 26), 4, "batch"),
    },
    "swin2sr": {
        "C60 [2,2] direct x2 16x24": (lambda: _from_sd(S2.fixture_sd("C60 [2,2] direct x2 16x24")), (1, 16, 24), 1, ""),
        "C60 [2] direct x4 13x21": (lambda: _from_sd(S2.fixture_sd("C60 [2] direct x4 13x21 (padded)")), (1, 13, 21), 2, "u8 small"),
        "C180 [2] pixelshuffle x4 16x16": (lambda: _from_sd(S2.fixture_sd("C180 [2] pixelshuffle x4 16x16")), (1, 16, 16), 3, ""),
        "C180 [2] pixelshuffle x3 9x17": (lambda: _from_sd(S2.fixture_sd("C180 [2] pixelshuffle x3 9x17")), (1, 9, 17), 4, ""),
        "C240 nH8 [2] 3conv nearest+conv x4 13x21": (lambda: _from_sd(S2.fixture_sd("C240 nH8 [2] 3conv nearest+conv x4 16x24")), (1, 13, 21), 5, ""),
        "C64 nH2 [2] pixelshuffle x2 9x17": (lambda: _from_sd(S2.fixture_sd("C64 nH2 [2] pixelshuffle x2 8x8")), (1, 9, 17), 6, ""),
        "C60 [2] pixelshuffle x2 batch of two 19x26": (lambda: _from_sd(S2.fixture_sd("C60 [2] batch of two pixelshuffle x2 19x26")), (2, 19, 26), 7, "batch"),
    },
    "dat": {        # (DAT runs on H x W itself: its windows pad inside the attention; 33 x 47 = 1551 pixels is a ragged second segment of the pool and the Gram)
        "C60 nH6 [8,16] [3,2] 3conv direct x2 20x44": (lambda: _dat("C60 nH6 [8,16] [3,2] 3conv direct x2 20x44"), (1, 20, 44), 1, ""),
        "C60 nH6 [8,16] [3,2] 3conv direct x2 13x21": (lambda: _dat("C60 nH6 [8,16] [3,2] 3conv direct x2 20x44"), (1, 13, 21), 1, "u8 small"),
        "C180 nH6 [8,32] [2] x4 33x47": (lambda: _dat("C180 nH6 [8,32] [2] x4 40x72"), (1, 33, 47), 2, ""),
        "C64 nH2 [8,16] [4] ef4 x3 batch of two 19x26": (lambda: _dat("C64 nH2 [8,16] [4] ef4 x3 batch of two 19x26"), (2, 19, 26), 3, "batch"),
    },
    "drct": {
        "C60 R2 x2 13x21": (lambda: _from_sd(DCR.fixture_sd("C60 R2 x2 13x21 (padded)")), (1, 13, 21), 1, "u8 small"),
        "C180 R1 x4 32x48": (lambda: _from_sd(DCR.fixture_sd("C180 R1 x4 32x48")), (1, 32, 48), 2, ""),
        "C96 R1 x3 batch of two 19x26": (lambda: _from_sd(DCR.fixture_sd("C96 R1 x3 batch of two 19x26")), (2, 19, 26), 3, "batch"),
    },
}
ALL = [pytest.param(f, k, id=f"{f}-{k}") for f, d in CASES.items() for k in d]
U8 = [pytest.param(f, k, id=f"{f}-{k}") for f, d in CASES.items() for k, v in d.items() if "u8" in v[3]]
BATCH = [pytest.param(f, k, id=f"{f}-{k}") for f, d in CASES.items() for k, v in d.items() if "batch" in v[3]]


def _build(dev, family, label):
    return CASES[family][label][0]().to(dev).eval()


@functools.lru_cache(maxsize=None)
def _shared_net(dev, family, label):
    """The net of a case, built once for the tests that own their workspace (the sequences build their own: they are about the net's `_ws`)."""
    return _build(dev, family, label)


def _input(dev, family, label, u8=False):
    from innfer_amd import synth
    _, (N, H, W), seed, _ = CASES[family][label]
    if u8:
        return torch.stack([torch.from_numpy(synth.image_u8(H, W, 3, 40 + seed + n)) for n in range(N)]).to(dev)          # [N, H, W, 3]
    return torch.from_numpy(synth.uniform((N, 3, H, W), 7 + seed)).to(dev).half()


# ------------------------------------------------------------------------------------------------ the harness
class Run:
    """innfer_net_forward of one net on a workspace and a result buffer of the test's: [workspace: need bytes | guard: need bytes], [guard | result | guard]."""

    def __init__(self, net, x):
        import innfer_amd.lib as L
        self.L, self.net, self.x = L, net, x
        self.u8 = x.dtype == torch.uint8
        # the module sets the handle's switches (precision, uint8 conversion, outm) as its forward does; its own workspace is let go at once
        (net.forward_u8 if self.u8 else net)(x)
        net.release_workspace()
        self.N, self.H, self.W = (x.shape[0], x.shape[1], x.shape[2]) if self.u8 else (x.shape[0], x.shape[2], x.shape[3])
        s = L.lib.innfer_net_scale(net._handle)
        self.shape = (self.N, self.H * s, self.W * s, net.out_nc) if self.u8 else (self.N, net.out_nc, self.H * s, self.W * s)
        self.numel = self.N * net.out_nc * self.H * s * self.W * s
        self.need = L.lib.innfer_net_workspace_bytes(net._handle, self.N, self.H, self.W)
        assert self.need > 0
        self.ws = torch.empty(2 * self.need, dtype=torch.uint8, device=x.device)
        self.out = torch.empty(self.numel + 2 * GUARD, dtype=x.dtype, device=x.device)
        self.x0 = x.clone()

    def fill(self, pattern):
        self.ws[:self.need].fill_(pattern)
        self.ws[self.need:].fill_(FILL_U8)
        self.out.fill_(FILL_U8 if self.u8 else FILL)

    def forward(self, x=None, ws_ptr=True, ws_bytes=None):
        """The status of one forward of x (default: the case's input; a batch's tail runs in the same workspace) after a synchronise."""
        L, x = self.L, self.x if x is None else x
        N = x.shape[0]
        dt = L.U8 if self.u8 else L.F16
        rc = L.lib.innfer_net_forward(self.net._handle, x.data_ptr(), dt, self.out.data_ptr() + GUARD * self.out.element_size(), dt, N, self.H, self.W,
                                      self.ws.data_ptr() if ws_ptr else None, self.need if ws_bytes is None else ws_bytes,
                                      torch.cuda.current_stream(x.device).cuda_stream)
        torch.cuda.synchronize()
        return rc

    def result(self, N=None):
        n = self.numel if N is None else self.numel // self.N * N
        shape = self.shape if N is None else (N,) + self.shape[1:]
        return self.out[GUARD:GUARD + n].clone().reshape(shape)

    def assert_contained(self, what, N=None):
        """The guard half of the workspace, the result's guard bands (and what lies behind a shorter batch's result) hold their fill; the input is unchanged."""
        n = self.numel if N is None else self.numel // self.N * N
        fill = FILL_U8 if self.u8 else FILL
        g = self.ws[self.need:] != FILL_U8
        assert not bool(g.any()), f"{what}: the forward wrote {int(g.sum())} bytes behind its workspace, the first at byte {int(g.nonzero()[0])} of {self.need} behind its end"
        assert bool((self.out[:GUARD] == fill).all()), f"{what}: the forward wrote in front of its result"
        assert bool((self.out[GUARD + n:] == fill).all()), f"{what}: the forward wrote behind its result"
        assert torch.equal(self.x, self.x0), f"{what}: the forward wrote to its input"

    def assert_untouched(self, what, pattern):
        assert bool((self.ws[:self.need] == pattern).all()), f"{what}: a refused forward wrote to its workspace"
        assert bool((self.ws[self.need:] == FILL_U8).all()), f"{what}: a refused forward wrote behind its workspace"
        assert bool((self.out == (FILL_U8 if self.u8 else FILL)).all()), f"{what}: a refused forward wrote to its result"
        assert torch.equal(self.x, self.x0), f"{what}: a refused forward wrote to its input"


def _bits(t):
    return t if t.dtype == torch.uint8 else t.view(torch.int16)


def _assert_same_bits(got, want, what, u8=False):
    """Bit equality; a failure names the count and the first differing coordinate (n, c, y, x): a pad-channel leak, a halo leak and a batch leak look different there."""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(_bits(got), _bits(want)):
        return
    ne = (_bits(got) != _bits(want)).cpu()
    i = [int(v) for v in ne.nonzero()[0]]
    n, c, y, x = (i[0], i[3], i[1], i[2]) if u8 else i
    rows = sorted({int(v) for v in ne.nonzero()[:, 1 if u8 else 2][:4096]})
    raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} values differ, the first at (n, c, y, x) = ({n}, {c}, {y}, {x}): {got[tuple(i)].item()} != {want[tuple(i)].item()}; "
                         f"rows {rows[0]} .. {rows[-1]} of {got.shape[1 if u8 else 2]}")


def _poison_and_containment(dev, family, label, u8):
    run = Run(_shared_net(dev, family, label), _input(dev, family, label, u8))
    y0 = None
    for pattern in PATTERNS:
        what = f"{family} {label}{' uint8' if u8 else ''}, workspace 0x{pattern:02X}"
        run.fill(pattern)
        rc = run.forward()
        assert rc == 0, (what, rc, run.L.last_error())
        run.assert_contained(what)
        y = run.result()
        if y0 is None:
            y0 = y
        _assert_same_bits(y, y0, f"{what} against workspace 0x00", u8)
        if not u8:
            assert bool(torch.isfinite(y).all()), f"{what}: the result is not finite"


# ------------------------------------------------------------------------------------------------ 1, 2: poison and containment
@pytest.mark.parametrize("family,label", ALL)
def test_poison_independence_and_containment(dev, family, label):
    _poison_and_containment(dev, family, label, False)


@pytest.mark.parametrize("family,label", U8)
def test_poison_independence_and_containment_u8(dev, family, label):
    _poison_and_containment(dev, family, label, True)


# ------------------------------------------------------------------------------------------------ 3: refusal
@pytest.mark.parametrize("family,label", ALL + [pytest.param(*p.values, id=p.id + "-u8") for p in U8])
def test_short_or_missing_workspace_is_refused(dev, family, label, request):
    u8 = request.node.callspec.id.endswith("-u8")
    run = Run(_shared_net(dev, family, label), _input(dev, family, label, u8))
    E = run.L.ERR_WORKSPACE
    run.fill(0x5C)
    rc = run.forward(ws_bytes=run.need - 1)
    assert rc == E and "workspace" in run.L.last_error(), (rc, run.L.last_error())
    run.assert_untouched(f"{family} {label}: one byte short", 0x5C)
    rc = run.forward(ws_ptr=False)
    assert rc == E, (rc, run.L.last_error())
    run.assert_untouched(f"{family} {label}: no workspace", 0x5C)
    rc = run.forward(ws_ptr=False, ws_bytes=0)
    assert rc == E, (rc, run.L.last_error())
    run.assert_untouched(f"{family} {label}: no workspace, no bytes", 0x5C)
    assert run.forward() == 0          # (and it is the size alone that was refused)
    run.assert_contained(f"{family} {label}: exactly the bytes asked for")


# ------------------------------------------------------------------------------------------------ 4: shape sequences on one net
@pytest.mark.parametrize("family", list(CASES))
def test_shape_sequence_reuses_the_workspace(dev, family):
    """batch of two -> small padded shape -> batch of two on ONE net object (the module keeps `_ws`: the small forward runs in the stale bytes of another layout) against a
    fresh net that only ever saw the small shape; then the same with 0x7B bytes put into `_ws` between the forwards."""
    from innfer_amd import synth
    big = next(k for k, v in CASES[family].items() if "batch" in v[3])
    _, (sn, sh, sw), seed, _ = next(v for v in CASES[family].values() if "small" in v[3])
    xb = _input(dev, family, big)
    xs = torch.from_numpy(synth.uniform((sn, 3, sh, sw), 90 + seed)).to(dev).half()
    want_s = _build(dev, family, big)(xs)
    net = _build(dev, family, big)
    for poison in (None, 0x7B):
        yb = net(xb)
        ptr, size = net._ws.data_ptr(), net._ws.numel()
        if poison is not None:
            net._ws.fill_(poison)
        ys = net(xs)
        assert net._ws.data_ptr() == ptr and net._ws.numel() == size, "the workspace was reallocated for the small shape: this test would not test reuse"
        what = f"{family} {big} -> 1x{sh}x{sw} -> batch" + ("" if poison is None else f", 0x{poison:02X} in between")
        _assert_same_bits(ys, want_s, f"{what}: the small shape after the large one against a fresh net")
        if poison is not None:
            net._ws.fill_(poison)
        yb2 = net(xb)
        assert net._ws.data_ptr() == ptr
        _assert_same_bits(yb2, yb, f"{what}: the large shape again")
        assert bool(torch.isfinite(ys).all()) and bool(torch.isfinite(yb2).all())


# ------------------------------------------------------------------------------------------------ 5: batch tail
@pytest.mark.parametrize("family,label", BATCH)
def test_batch_tail_in_the_same_poisoned_workspace(dev, family, label):
    """N = 2, then N = 1 of sample 1 in the same workspace -- poisoned in front of the batch, holding the batch's stale layout in front of the tail: equal to y[1:]."""
    run = Run(_shared_net(dev, family, label), _input(dev, family, label))
    tail = run.x[1:].contiguous()
    for pattern in PATTERNS[1:]:
        what = f"{family} {label}, workspace 0x{pattern:02X}"
        run.fill(pattern)
        assert run.forward() == 0, run.L.last_error()
        run.assert_contained(what)
        y = run.result()
        run.out.fill_(FILL)
        assert run.forward(tail) == 0, run.L.last_error()
        run.assert_contained(what + ", the tail", N=1)
        _assert_same_bits(run.result(N=1), y[1:], f"{what}: sample 1 alone against sample 1 of the batch")
