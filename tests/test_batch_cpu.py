"""Many images as one tile stream (`-batch B`, Model.run_u8_batch), the part that needs no GPU: the planning entry point (innfer_chop_multi_plan) against a
Python restatement -- the tile size, the tile counts and running counts, the packed offsets and the two tables the kernels read --, its refusals, the flag, the
refusals of `main`, which come before a model is loaded, and the public surface."""
import inspect

import numpy as np
import pytest

import innfer_amd.lib as L
from innfer_amd import run as R

SETS = ([(50, 77), (64, 50), (50, 50)], [(52, 52), (52, 90)], [(200, 231), (215, 200), (400, 300)])
CASES = [(s, 0) for s in SETS] + [(SETS[0], 16)]


def axis_origins(A, ps, step_int):
    """The chop lattice of one axis written out: multiples of the step while the tile fits, then one tile anchored at the end."""
    org = list(range(0, A - ps + 1, step_int))
    if org[-1] != A - ps:
        org.append(A - ps)
    return org


def restate(sizes, C, pad, scale, patch=200, step=0.5):
    """What innfer_chop_multi_plan is documented to return, in plain Python."""
    up = lambda v: -(-v // 16) * 16                                                      # noqa: E731
    pss = {min(h + 2 * pad, w + 2 * pad, patch) for h, w in sizes}
    assert len(pss) == 1
    ps = pss.pop()
    counts, first, in_off, out_off, tiles, images = [], [0], [0], [0], [], []
    for h, w in sizes:
        ys, xs = axis_origins(h + 2 * pad, ps, int(ps * step)), axis_origins(w + 2 * pad, ps, int(ps * step))
        images.append((out_off[-1], first[-1], scale * (h + 2 * pad), scale * (w + 2 * pad), len(ys), len(xs)))
        tiles += [(in_off[-1], h, w, y, x) for y in ys for x in xs]
        counts.append(len(ys) * len(xs))
        first.append(first[-1] + counts[-1])
        in_off.append(up(in_off[-1] + h * w * C))
        out_off.append(up(out_off[-1] + scale * h * scale * w * C))
    return ps, counts, first, in_off, out_off, tiles, images


@pytest.mark.parametrize("sizes, pad", CASES)
def test_plan_equals_its_restatement(sizes, pad):
    for C in (1, 3, 4):
        for scale in (1, 2, 3):
            ps, counts, first, in_off, out_off, tiles, images = restate(sizes, C, pad, scale)
            p = L.chop_multi_plan(sizes, C, pad=pad, scale=scale)
            assert p["ps"] == ps and p["sizes"].tolist() == [list(s) for s in sizes]
            assert p["counts"].tolist() == counts and p["first"].tolist() == first
            assert p["in_off"].tolist() == in_off and p["out_off"].tolist() == out_off
            assert p["tiles"].tolist() == tiles and p["images"].tolist() == images
            for (h, w), n in zip(sizes, counts):                                             # every image's own lattice, in its own order
                _, ys, xs = L.chop_plan(h + 2 * pad, w + 2 * pad, 200, 0.5)
                assert n == len(ys) * len(xs)
            k = 0
            for (h, w) in sizes:
                _, ys, xs = L.chop_plan(h + 2 * pad, w + 2 * pad, 200, 0.5)
                for y in ys:
                    for x in xs:
                        assert (p["tiles"]["oy"][k], p["tiles"]["ox"][k]) == (y, x)
                        k += 1


def test_plan_table_layouts_are_the_headers():
    assert np.dtype(L.MULTI_TILE).itemsize == 24 and np.dtype(L.MULTI_IMAGE).itemsize == 32          # int64 + 4 ints; 2 int64 + 4 ints: no padding


@pytest.mark.parametrize("sizes, kw, match", [
    ([(50, 77), (60, 60)], {}, "one tile stream needs one tile size"),                                # mixed ps
    ([(50, 77), (300, 300)], {}, "one tile stream needs one tile size"),
    ([(50, 77)], dict(channels=0), "channels"),
    ([(50, 77)], dict(channels=5), "channels"),
    ([(50, 0)], {}, "bad sizes"),
    ([(-3, 50)], {}, "bad sizes"),
    ([(50, 50)], dict(pad=-1), "bad sizes"),
    ([(50, 50)], dict(scale=0), "scale"),
    ([], {}, "0 images"),
])
def test_plan_refusals(sizes, kw, match):
    kw = dict(dict(channels=3), **kw)
    with pytest.raises(ValueError, match=match):
        L.chop_multi_plan(sizes, **kw)


def test_flag_parses_and_is_absent_by_default():
    p = R.build_parser()
    argv = ["-m", "4x_model.pth", "-i", "in", "-o", "out", "-cf"]
    plain = p.parse_args(argv)
    assert not hasattr(plain, "batch")
    assert vars(plain) == dict(models="4x_model.pth", arch="infer", input="in", output="out", scale="-1", cf=True, comp=False, no_gpu=True,
                               no_fp16=True, norm=False)                            # the namespace of the reference's flags, as before
    ns = p.parse_args(argv + ["-batch", "16"])
    assert ns.batch == 16
    d = vars(ns)
    del d["batch"]
    assert d == vars(plain)
    for bad in (["-batch"], ["-batch", "many"], ["-batch", "2.5"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv + bad)


@pytest.mark.parametrize("argv, match", [
    (["-batch", "0"], "-batch must be an int >= 1"),
    (["-batch", "-4"], "-batch must be an int >= 1"),
    (["-batch", "4", "-tile", "512"], "-batch 4 with -tile 512"),
    (["-batch", "4", "-tile", "0"], "-batch 4 with -tile 0"),
    (["-a", "p2p_256", "-batch", "4"], "-batch 4 with 'p2p_256'"),                    # the presets that run whole images
    (["-a", "unet_128", "-batch", "4"], "-batch 4 with 'unet_128'"),
    (["-a", "wbc", "-batch", "4"], "-batch 4 with 'wbcunet'"),
])
def test_main_refuses_before_it_loads_a_model(argv, match):
    with pytest.raises(ValueError, match=match):
        R.main(["-m", "no_such_model.pth"] + argv)


def test_public_surface():
    sig = inspect.signature(R.Model.run_u8_batch)
    assert list(sig.parameters) == ["self", "imgs", "normalize", "fp16", "seamless", "outscale", "outfilter", "fit_channels", "tta"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [False, True, None, None, "lanczos", False, False]
    assert list(inspect.signature(R.Model.run_u8).parameters) == ["self", "img", "normalize", "fp16", "out", "fit_channels", "seamless", "outscale", "outfilter",
                                                                  "tta"]                  # untouched
    assert L.ABI_VERSION == 124 and L.lib.innfer_version() == 124
    for f in ("innfer_chop_multi_plan", "innfer_extract_tiles_u8_multi", "innfer_recompose_u8_multi"):
        assert hasattr(L.lib, f) and f in L.SIGNATURES
