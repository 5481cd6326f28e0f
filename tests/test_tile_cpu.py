"""The stitched tile path (`-tile N -tile_pad P`), the part that needs no GPU: the lattice of the library (innfer_tile_plan) against a Python restatement of its
formulas and the invariants the stitch relies on, the owner as the kernels compute it (innfer_tile_owner) against its definition, the two flags, and the
refusals of Model(tile=, tile_pad=), which come before anything touches a device."""
import inspect

import numpy as np
import pytest

import innfer_amd.lib as L
from innfer_amd import run as R

AXES = list(range(1, 400)) + [1080, 1920, 2160, 3840, 4320, 7680]
TILES = (1, 2, 8, 32, 33, 64, 200, 512, 1024)
HALOS = (0, 1, 3, 8, 16)


def axis_plan(A, T, h):
    """(n, P, origins) of one axis, the issue's formulas written out."""
    if A <= T + 2 * h:
        return 1, A, [0]
    n = -(-(A - 2 * h) // T)
    P = -(-(A + 2 * h * (n - 1)) // n)
    S = P - 2 * h
    return n, P, [min(i * S, A - P) for i in range(n)]


def owners(A, org, h):
    """owner(y) for every y of the axis: the largest i with i == 0 or o_i + h <= y."""
    return np.maximum(np.searchsorted(np.asarray(org) + h, np.arange(A), side="right") - 1, 0)


@pytest.mark.parametrize("h", HALOS)
def test_tile_plan_equals_the_formulas_and_keeps_the_invariants(h):
    for T in TILES:
        for A in AXES:
            n, P, org = axis_plan(A, T, h)
            B = AXES[(AXES.index(A) * 7 + 3) % len(AXES)]                           # another length on the other axis: the axes are independent
            nb, Pb, orgb = axis_plan(B, T, h)
            assert L.tile_plan(A, B, T, h) == (P, Pb, org, orgb), (A, B, T, h)
            o = np.asarray(org)
            assert o[0] == 0 and o[-1] == A - P and np.all(np.diff(o) > 0), (A, T, h)       # strictly increasing, inside the image, the last one at the end
            assert P <= T + 2 * h and len(org) == n
            k = owners(A, org, h)
            off = np.arange(A) - o[k]
            assert np.all((0 <= off) & (off < P)), (A, T, h)                         # every pixel has an owner that holds it
            low_inner, high_inner = o[k] > 0, o[k] + P < A                           # tile edges that are not image edges
            assert np.all(off[low_inner] >= h) and np.all((P - 1 - off)[high_inner] >= h), (A, T, h)


@pytest.mark.parametrize("scale", (1, 2, 3, 4))
def test_tile_owner_closed_form_is_the_definition(scale):
    """What the stitch kernels compute per pixel (one division) against the definition, in output pixels."""
    for h in HALOS:
        for T in (1, 2, 8, 32, 33):
            for A in list(range(1, 90)) + [399]:
                _, P, org = axis_plan(A, T, h)
                k = owners(A, org, h)
                for X in range(scale * A):
                    assert L.tile_owner(A, T, h, X, scale) == (k[X // scale], scale * org[k[X // scale]]), (A, T, h, scale, X)
    for A, T, h in ((1080, 1024, 16), (3840, 512, 16), (7680, 512, 16)):
        _, P, org = axis_plan(A, T, h)
        k = owners(A, org, h)
        for X in range(0, scale * A, 7):
            assert L.tile_owner(A, T, h, X, scale) == (k[X // scale], scale * org[k[X // scale]])


def test_spot_values_and_refusals():
    assert L.tile_plan(50, 41, 32, 8)[::2] == (33, [0, 17])
    assert L.tile_plan(41, 50, 16, 4)[::2] == (19, [0, 11, 22])
    assert axis_plan(50, 32, 8) == (2, 33, [0, 17]) and axis_plan(41, 16, 4) == (3, 19, [0, 11, 22])
    ph, pw, ys, xs = L.tile_plan(4320, 7680, 512, 16)
    assert (ph, pw, len(ys), len(xs)) == (509, 542, 9, 15)
    assert L.tile_plan(1080, 1920, 1024, 16)[:2] == (556, 976)                       # balanced: two tiles of 556 rows, not one of 1056 and a sliver
    # the share of the image that runs through the network: 1.11 / 1.12 / 1.12 at 512 + 16, where the 200 / 0.5 chop runs 3.67 / 3.85 / 3.94
    for (H, W), want in (((1080, 1920), 1.11), ((2160, 3840), 1.12), ((4320, 7680), 1.12)):
        ph, pw, ys, xs = L.tile_plan(H, W, 512, 16)
        assert round(ph * pw * len(ys) * len(xs) / (H * W), 2) == want
    for bad in ((0, 5, 8, 1), (5, 0, 8, 1), (5, 5, 0, 1), (5, 5, 8, -1), (-3, 5, 8, 0)):
        with pytest.raises(ValueError):
            L.tile_plan(*bad)
    with pytest.raises(ValueError):
        L.tile_owner(50, 32, 8, 50)
    assert L.ABI_VERSION == 124 and all(hasattr(L.lib, f) for f in ("innfer_tile_plan", "innfer_tile_owner", "innfer_extract_tiles_rect",
                                                                    "innfer_extract_tiles_u8_rect", "innfer_stitch_tiles", "innfer_stitch_tiles_u8"))


def test_flags_parse_and_are_absent_by_default():
    p = R.build_parser()
    argv = ["-m", "4x_model.pth", "-i", "in", "-o", "out", "-cf"]
    plain = p.parse_args(argv)
    assert not hasattr(plain, "tile") and not hasattr(plain, "tile_pad")
    assert vars(plain) == dict(models="4x_model.pth", arch="infer", input="in", output="out", scale="-1", cf=True, comp=False, no_gpu=True,
                               no_fp16=True, norm=False)                            # the namespace of the reference's flags, as before
    ns = p.parse_args(argv + ["-tile", "512"])
    assert ns.tile == 512 and not hasattr(ns, "tile_pad")
    d = vars(ns)
    del d["tile"]
    assert d == vars(plain)
    ns = p.parse_args(["-m", "x", "-tile", "1024", "-tile_pad", "8", "-seamless", "tile", "-tta"])
    assert (ns.tile, ns.tile_pad, ns.seamless, ns.tta) == (1024, 8, "tile", True)
    assert p.parse_args(["-m", "x", "-tile", "0"]).tile == 0
    for bad in (["-tile"], ["-tile", "big"], ["-tile", "51.5"], ["-tile", "512", "-tile_pad", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv + bad)


@pytest.mark.parametrize("argv, match", [
    (["-a", "p2p_256", "-tile", "512"], "-tile 512 with 'p2p_256'"),                  # the presets that already run whole images
    (["-a", "wbc", "-tile", "0"], "-tile 0 with 'wbcunet'"),
    (["-tile", "16"], "tile must be"),
    (["-tile", "-512"], "tile must be"),
    (["-tile", "512", "-tile_pad", "-1"], "tile_pad must be"),
    (["-tile_pad", "8"], "-tile_pad is the halo of -tile"),
])
def test_main_refuses_before_it_loads_a_model(argv, match):
    with pytest.raises(ValueError, match=match):
        R.main(["-m", "no_such_model.pth"] + argv)


def test_model_arguments_are_checked_before_any_device_call():
    sig = inspect.signature(R.Model.__init__).parameters
    assert sig["tile"].default is None and sig["tile_pad"].default == 16
    assert list(inspect.signature(R.Model.tile_forward).parameters) == ["self", "data", "tile", "tile_pad"]
    for kw, match in ((dict(tile=16), "tile must be"), (dict(tile=31), "tile must be"), (dict(tile=-1), "tile must be"), (dict(tile=512.0), "tile must be"),
                      (dict(tile="512"), "tile must be"), (dict(tile=True), "tile must be"), (dict(tile=512, tile_pad=-1), "tile_pad must be"),
                      (dict(tile=512, tile_pad=1.5), "tile_pad must be"), (dict(tile_pad=None), "tile_pad must be"),
                      (dict(tile=512, chop=False), "chop=False"), (dict(tile=0, chop=False), "chop=False")):
        with pytest.raises(ValueError, match=match):
            R.Model("no_such_model.pth", "infer", 4, **kw)
        with pytest.raises(ValueError, match=match):                                   # ahead of the refusal of a CPU device, too
            R.Model("no_such_model.pth", "infer", 4, device="cpu", **kw)
    for kw in (dict(tile=None), dict(tile=0), dict(tile=32), dict(tile=512, tile_pad=0), dict(tile=1024, tile_pad=32)):
        with pytest.raises(FileNotFoundError):                                         # accepted: the next thing that happens is the read of the file
            R.Model("no_such_model.pth", "infer", 4, **kw)
