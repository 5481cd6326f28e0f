"""Many images as one tile stream on the GPU (`-batch B`; csrc/tiles_u8_multi.hip, Model.run_u8_batch).

1. the two kernels alone: the multi gather is the concatenation of the per-image innfer_extract_tiles_u8_seamless outputs and every image's slice of the
   packed multi blend is its innfer_recompose_u8_seamless, bit for bit, in guarded buffers; the refusals launch nothing;
2. the definition: run_u8_batch(imgs)[i] == run_u8(imgs[i]) for images of three tile sizes in interleaved order, with every option of the fast path, under
   a forced memory budget, and on the paths that loop;
3. the command line: `-batch 4` writes the files of a run without the flag, byte for byte.
Every comparison is exact.  Needs an MI355X: `pytest -m gpu`."""
import inspect

import numpy as np
import pytest
import torch

from test_gpu_tile import SENTINEL, _compact_model, _guarded, _rrdb_model, _tail_intact

pytestmark = pytest.mark.gpu

SETS = ([(50, 77), (64, 50), (50, 50)],                     # ps 50 (pad 16: 82): the scalar form
        [(52, 52), (52, 90)],                               # ps 52 (pad 16: 84): four pixels per thread
        [(200, 231), (215, 200), (400, 300)])               # ps 200: multi-tile images of different sizes in one stream
BORDERS = ((0, "replicate"), (16, "tile"), (16, "mirror"), (16, "replicate"), (16, "alpha_pad"))
MODEL_SIZES = ((40, 56), (56, 40), (40, 40), (64, 50), (64, 50), (210, 230), (200, 200))          # ps 40, 50 and 200, interleaved


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _code(dt):
    from innfer_amd import lib as L
    return L.F16 if dt == torch.float16 else L.F32


def _images(sizes, C, seed):
    from innfer_amd import synth
    return [synth.image_u8(h, w, C, seed + 7 * i) for i, (h, w) in enumerate(sizes)]


def _packed(imgs, plan, dev):
    """The images at the plan's offsets of one device buffer; the gaps hold a value no image byte has to share."""
    d = torch.full((int(plan["in_off"][-1]),), 0x5A, dtype=torch.uint8, device=dev)
    for im, off in zip(imgs, plan["in_off"]):
        d[off:off + im.size] = torch.from_numpy(im.reshape(-1)).to(dev)
    return d


def _table(records, dev):
    return torch.from_numpy(records.view(np.uint8).copy()).to(dev)


@pytest.fixture(scope="module")
def pools(dev):
    """Random HR values, made once: 2^22 synth.uniform floats per range, repeated to whatever length a case needs."""
    from innfer_amd import synth
    return {norm: torch.from_numpy(synth.uniform((1 << 22,), 91 + norm, -1.25 if norm else -0.25, 1.25)).to(dev) for norm in (0, 1)}


def _hr(pools, norm, shape, dt):
    n = int(np.prod(shape))
    pool = pools[norm]
    return pool.repeat(-(-n // pool.numel()))[:n].view(shape).to(dt).contiguous()


# ------------------------------------------------------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("sizes", SETS, ids=("ps50", "ps52", "ps200"))
def test_multi_gather_is_the_per_image_gathers(dev, sizes):
    from innfer_amd import lib as L
    for C in (1, 3, 4):
        imgs = _images(sizes, C, 11 * C)
        singles = [torch.from_numpy(im).to(dev) for im in imgs]
        for pad, mode in BORDERS:
            plan = L.chop_multi_plan(sizes, C, pad=pad)
            d, table = _packed(imgs, plan, dev), _table(plan["tiles"], dev)
            total, ps = int(plan["first"][-1]), plan["ps"]
            for dt in (torch.float16, torch.float32):
                for norm in (0, 1):
                    buf, got = _guarded((total, C, ps, ps), dt, dev)
                    L.check(L.lib.innfer_extract_tiles_u8_multi(d.data_ptr(), len(sizes), plan["sizes"].ctypes.data, C, norm, 200, 0.5, pad, L.BORDER_MODES[mode],
                                                                table.data_ptr(), buf.data_ptr(), _code(dt), _stream()))
                    assert _tail_intact(buf), (C, pad, mode, dt, norm)
                    for i, ((h, w), s) in enumerate(zip(sizes, singles)):
                        n = int(plan["counts"][i])
                        want = torch.empty((n, C, ps, ps), dtype=dt, device=dev)
                        L.check(L.lib.innfer_extract_tiles_u8_seamless(s.data_ptr(), C, h, w, norm, 200, 0.5, 0, n, pad, L.BORDER_MODES[mode], want.data_ptr(),
                                                                       _code(dt), _stream()))
                        f = int(plan["first"][i])
                        assert torch.equal(got[f:f + n], want), (C, pad, mode, dt, norm, i)


@pytest.mark.parametrize("sizes", SETS, ids=("ps50", "ps52", "ps200"))
def test_multi_blend_is_the_per_image_blends(dev, pools, sizes):
    from innfer_amd import lib as L
    for scale in (1, 2, 3):
        for pad in (0, 16):
            for C in (1, 3, 4):
                plan = L.chop_multi_plan(sizes, C, pad=pad, scale=scale)
                frames = _table(plan["images"], dev)
                total, P = int(plan["first"][-1]), scale * plan["ps"]
                for dt in (torch.float16, torch.float32):
                    for norm in (0, 1):
                        hr = _hr(pools, norm, (total, C, P, P), dt)
                        buf, got = _guarded((int(plan["out_off"][-1]),), torch.uint8, dev)
                        L.check(L.lib.innfer_recompose_u8_multi(hr.data_ptr(), _code(dt), len(sizes), plan["sizes"].ctypes.data, C, P, 200, 0.5, scale, _code(dt), norm,
                                                                pad, frames.data_ptr(), buf.data_ptr(), _stream()))
                        assert _tail_intact(buf), (scale, pad, C, dt, norm)
                        for i, (h, w) in enumerate(sizes):
                            f, n, o = int(plan["first"][i]), int(plan["counts"][i]), int(plan["out_off"][i])
                            want = torch.empty((scale * h, scale * w, C), dtype=torch.uint8, device=dev)
                            L.check(L.lib.innfer_recompose_u8_seamless(hr[f:f + n].data_ptr(), _code(dt), n, C, P, h + 2 * pad, w + 2 * pad, 0.5, scale, _code(dt),
                                                                       norm, pad, want.data_ptr(), _stream()))
                            assert torch.equal(got[o:o + want.numel()].view(want.shape), want), (scale, pad, C, dt, norm, i)
                            gap = got[o + want.numel():int(plan["out_off"][i + 1])]                  # the alignment gap behind the image stays untouched
                            assert bool((gap == SENTINEL[torch.uint8]).all())


def test_refusals_launch_nothing(dev):
    from innfer_amd import lib as L
    sizes = [(50, 77), (64, 50)]
    plan = L.chop_multi_plan(sizes, 3, pad=16, scale=2)
    imgs = _images(sizes, 3, 5)
    d, table, frames = _packed(imgs, plan, dev), _table(plan["tiles"], dev), _table(plan["images"], dev)
    total, ps = int(plan["first"][-1]), plan["ps"]
    tiles = torch.full((total, 3, ps, ps), SENTINEL[torch.float16], dtype=torch.float16, device=dev)
    out = torch.full((int(plan["out_off"][-1]),), SENTINEL[torch.uint8], dtype=torch.uint8, device=dev)
    hr = torch.zeros((total, 3, 2 * ps, 2 * ps), dtype=torch.float16, device=dev)

    def hw(s):
        return np.ascontiguousarray(np.asarray(s, dtype=np.int32))
    ok = dict(imgs=d.data_ptr(), sizes=hw(sizes), C=3, pad=16, mode=L.BORDER_MODES["mirror"], table=table.data_ptr(), tiles=tiles.data_ptr(), dtype=L.F16)
    for change, match in ((dict(sizes=hw([(50, 77), (60, 60)])), "one tile size"), (dict(C=5), "channels"), (dict(C=0), "channels"), (dict(mode=7), "border mode"),
                          (dict(sizes=hw([(1, 60), (1, 70)])), "mirror needs"), (dict(imgs=None), "null"), (dict(table=None), "null"), (dict(tiles=None), "null"),
                          (dict(dtype=L.U8), "dtype"), (dict(sizes=hw([(50, 77), (0, 50)])), "bad sizes"), (dict(pad=-1), "bad sizes")):
        a = dict(ok, **change)
        with pytest.raises(ValueError, match=match):
            L.check(L.lib.innfer_extract_tiles_u8_multi(a["imgs"], len(a["sizes"]), a["sizes"].ctypes.data, a["C"], 0, 200, 0.5, a["pad"], a["mode"], a["table"],
                                                        a["tiles"], a["dtype"], _stream()))
    ok = dict(hr=hr.data_ptr(), dtype=L.F16, sizes=hw(sizes), C=3, P=2 * ps, scale=2, via=L.F16, pad=16, frames=frames.data_ptr(), out=out.data_ptr())
    for change, match in ((dict(sizes=hw([(50, 77), (60, 60)])), "one tile size"), (dict(C=5), "channels"), (dict(hr=None), "null"), (dict(frames=None), "null"),
                          (dict(out=None), "null"), (dict(dtype=L.U8), "dtype"), (dict(via=7), "dtype"), (dict(sizes=hw([(50, 77), (-1, 50)])), "bad sizes"),
                          (dict(P=2 * ps + 1), "multiple of the scale"), (dict(P=2 * ps + 2), "tile size"), (dict(sizes=hw([(50, 77), (300, 300)])), "one tile size"), (dict(scale=0), "scale"), (dict(P=0), "scale")):
        a = dict(ok, **change)
        with pytest.raises(ValueError, match=match):
            L.check(L.lib.innfer_recompose_u8_multi(a["hr"], a["dtype"], len(a["sizes"]), a["sizes"].ctypes.data, a["C"], a["P"], 200, 0.5, a["scale"], a["via"], 0,
                                                    a["pad"], a["frames"], a["out"], _stream()))
    torch.cuda.synchronize()
    assert bool((tiles == SENTINEL[torch.float16]).all()) and bool((out == SENTINEL[torch.uint8]).all())


# ------------------------------------------------------------------------------------------------------------------ 2. the definition
@pytest.fixture(scope="module")
def rrdb(tmp_path_factory):
    return _rrdb_model(tmp_path_factory)


@pytest.fixture(scope="module")
def compact(tmp_path_factory):
    return _compact_model(tmp_path_factory)


@pytest.fixture(scope="module")
def imgs():
    return _images(MODEL_SIZES, 3, 40)


_REFS = {}


def _ref(m, imgs, **kw):
    """[run_u8(img, **kw)], computed once per model and option set."""
    key = (id(m), tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = [m.run_u8(im, **kw) for im in imgs]
    return _REFS[key]


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), i


def _no_loop(m, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the fast path must not call run_u8")
    monkeypatch.setattr(m, "run_u8", refuse)


@pytest.mark.parametrize("net", ("rrdb", "compact"))
def test_batch_equals_the_loop(dev, request, imgs, monkeypatch, net):
    m = request.getfixturevalue(net)
    options = [{}, dict(seamless="tile"), dict(outscale=1.5), dict(seamless="tile", outscale=1.5)] + ([dict(normalize=True, fp16=False)] if net == "rrdb" else [])
    wants = [_ref(m, imgs, **kw) for kw in options]
    cuda = [torch.from_numpy(im).to(dev) for im in imgs]
    calls = []
    inner = m._chop_u8_multi
    monkeypatch.setattr(m, "_chop_u8_multi", lambda *a, **k: (calls.append(len(a[1])), inner(*a, **k))[1])
    _no_loop(m, monkeypatch)
    for kw, want in zip(options, wants):
        _same(m.run_u8_batch(imgs, **kw), want)
    assert calls[:3] == [3, 2, 2] and len(calls) == 3 * len(options)                  # one gather, one stream, one blend per (C, ps) group
    for kw, want in zip(options[:4], wants):
        got = m.run_u8_batch(cuda, **kw)
        assert all(torch.is_tensor(g) and g.is_cuda and g.is_contiguous() for g in got)
        _same(got, want)


@pytest.mark.parametrize("net", ("rrdb", "compact"))
def test_batch_is_invariant_to_the_launch_sizes(request, imgs, monkeypatch, net):
    m = request.getfixturevalue(net)
    want = _ref(m, imgs)
    _no_loop(m, monkeypatch)
    for tb in (1, 3, None):
        monkeypatch.setattr(m, "tile_batch", tb)
        _same(m.run_u8_batch(imgs), want)


def test_a_small_memory_budget_gives_the_same_bits(rrdb, imgs, monkeypatch):
    want = _ref(rrdb, imgs)
    calls = []
    inner = rrdb._chop_u8_multi
    monkeypatch.setattr(rrdb, "_chop_u8_multi", lambda *a, **k: (calls.append(len(a[1])), inner(*a, **k))[1])
    monkeypatch.setattr(rrdb, "_batch_fits", lambda n, nbytes, device: n <= 2)
    alone = []
    run_u8 = rrdb.run_u8
    monkeypatch.setattr(rrdb, "run_u8", lambda im, **k: (alone.append(im.shape), run_u8(im, **k))[1])
    _same(rrdb.run_u8_batch(imgs), want)
    assert calls == [2, 2, 2] and alone == [(40, 40, 3)]                              # ps 40: three images as 2 + 1, and the one left alone runs as run_u8 does
    monkeypatch.setattr(rrdb, "_batch_fits", lambda n, nbytes, device: False)        # one image always runs
    _same(rrdb.run_u8_batch(imgs[:3]), want[:3])
    assert calls == [2, 2, 2] and len(alone) == 4


def test_other_channel_counts_and_mixed_groups(dev, tmp_path_factory):
    """BGRA and gray images through 4 -> 4 and 1 -> 1 networks, and a batch whose groups differ in the channel count only."""
    from innfer_amd import synth
    from innfer_amd.run import Model
    for C in (1, 4):
        sd = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.rrdbnet_shapes(nb=1, scale=2, in_nc=C, out_nc=C), 80 + C).items()}
        m = Model(None, "infer", 2, in_nc=C, out_nc=C, state_dict=sd)
        ims = _images(((40, 56), (56, 40), (44, 40)), C, 50 + C)
        _same(m.run_u8_batch(ims, seamless="mirror"), [m.run_u8(im, seamless="mirror") for im in ims])


def test_the_other_paths_loop(dev, tmp_path_factory, rrdb, imgs, monkeypatch):
    few = imgs[:3]

    def never(*a, **k):
        raise AssertionError("this path loops run_u8")
    monkeypatch.setattr(rrdb, "_chop_u8_multi", never)
    _same(rrdb.run_u8_batch(few, tta=True), [rrdb.run_u8(im, tta=True) for im in few])
    for kw in (dict(tile=32, tile_pad=8), dict(chop=False)):
        m = _rrdb_model(tmp_path_factory, **kw)
        monkeypatch.setattr(m, "_chop_u8_multi", never)
        _same(m.run_u8_batch(few), [m.run_u8(im) for im in few])
    assert rrdb.run_u8_batch([]) == []
    with pytest.raises(TypeError, match="all numpy arrays or all cuda tensors"):
        rrdb.run_u8_batch([few[0], torch.from_numpy(few[1]).to(dev)])
    with pytest.raises(ValueError, match="mirror"):
        rrdb.run_u8_batch([few[0], np.zeros((9, 1, 3), np.uint8)], seamless="mirror")
    assert "run_u8" in inspect.getdoc(type(rrdb).run_u8_batch)


# ------------------------------------------------------------------------------------------------------------------ 3. the command line
def test_command_line(dev, tmp_path, monkeypatch, capsys):
    """A folder of five small PNGs of two sizes and one unreadable file: `-batch 4` writes the files of the plain run, byte for byte, and says once that it
    skipped the unreadable one; the same with -cf."""
    from innfer_amd import run as R, synth
    from innfer_amd.utils import utils as U
    for sub in ("models", "in"):
        (tmp_path / sub).mkdir()
    torch.save({k: torch.from_numpy(v) for k, v in synth.fill_state_dict(synth.rrdbnet_shapes(nb=1, scale=2), 77).items()}, str(tmp_path / "models" / "2x_a.pth"))
    for i, (h, w) in enumerate(((40, 56), (48, 40), (40, 56), (48, 40), (40, 56))):
        U.save_img(synth.image_u8(h, w, 3, 60 + i), str(tmp_path / "in" / f"tex{i}.png"))
    (tmp_path / "in" / "tex2b.png").write_bytes(b"not a png at all")
    monkeypatch.chdir(tmp_path)
    seen = []
    inner = R.Model.run_u8_batch
    monkeypatch.setattr(R.Model, "run_u8_batch", lambda self, ims, **k: (seen.append(len(ims)), inner(self, ims, **k))[1])
    for tag, extra in (("plain", []), ("cf", ["-cf"])):
        del seen[:]
        assert R.main(["-m", "2x_a", "-i", "in", "-o", f"ref_{tag}"] + extra) == 0
        assert capsys.readouterr().out.count("Error reading image") == 1 and not seen
        assert R.main(["-m", "2x_a", "-i", "in", "-o", f"out_{tag}", "-batch", "4"] + extra) == 0
        said = capsys.readouterr().out
        assert said.count("Error reading image") == 1 and "tex2b.png, skipping." in said
        assert seen == [3, 2]                                                         # rounds of four files: three readable ones, then two
        names = sorted(p.name for p in (tmp_path / f"ref_{tag}").iterdir())
        assert names == [f"tex{i}.png" for i in range(5)] == sorted(p.name for p in (tmp_path / f"out_{tag}").iterdir())
        for name in names:
            assert (tmp_path / f"out_{tag}" / name).read_bytes() == (tmp_path / f"ref_{tag}" / name).read_bytes(), (tag, name)
    assert (tmp_path / "out_plain" / "tex0.png").read_bytes() != (tmp_path / "out_cf" / "tex0.png").read_bytes()
