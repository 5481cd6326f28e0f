"""DRCT: the host logic (no GPU) -- the reference against an independent module-style formulation, the key table, strict loading, checkpoint sniffing with and without
the buffers, the refusals, the new symbols, the engine's tensors taken apart again (and put together again: the engine's graph restated on the slab layout in float64 gives
the reference's result), and the test data's own figures: the storage model's error, the spread of the scores, and what each planted fault costs."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import _drct_ref as DR
import _hat_ref as HR
from innfer_amd import synth
from innfer_amd.run import infer_from_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (in_chans, C, R, num_heads of the published rule, mlp_ratio, s): DRCT, DRCT-L, and small ones
VARIANTS = [(3, 180, 6, 6, 2.0, 4), (3, 180, 12, 6, 2.0, 4), (3, 60, 2, 6, 2.0, 2), (1, 64, 1, 2, 3.0, 3), (4, 96, 2, 4, 1.5, 3)]
FAULTS = ("no_shift", "no_mask", "no_cat", "lrelu5", "no_res_scale")


def _zeros(v):
    return {k: torch.zeros(s) for k, s in DR.shapes(*v).items()}


def _ids(v):
    return f"in{v[0]}-C{v[1]}-R{v[2]}-nH{v[3]}-r{v[4]}-x{v[5]}"


# ------------------------------------------------------------------------------------------------ the reference against an independent formulation
class _Attn(nn.Module):
    def __init__(self, dim, nH):
        super().__init__()
        self.dim, self.nH = dim, nH
        self.relative_position_bias_table = nn.Parameter(torch.zeros(961, nH))
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        ch, cw = torch.meshgrid(torch.arange(16), torch.arange(16), indexing="ij")
        co = torch.stack([ch, cw]).flatten(1)
        rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0) + 15
        self.register_buffer("relative_position_index", rel[:, :, 0] * 31 + rel[:, :, 1], persistent=False)

    def forward(self, x, mask):          # x [B_, 256, dim]
        B_, T, Cc = x.shape
        qkv = self.qkv(x).reshape(B_, T, 3, self.nH, Cc // self.nH).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0] * (Cc // self.nH) ** -0.5, qkv[1], qkv[2]
        a = q @ k.transpose(-2, -1) + self.relative_position_bias_table[self.relative_position_index.view(-1)].view(T, T, -1).permute(2, 0, 1)[None]
        if mask is not None:
            nW = mask.shape[0]
            a = (a.view(B_ // nW, nW, self.nH, T, T) + mask[None, :, None]).view(B_, self.nH, T, T)
        return self.proj((a.softmax(-1) @ v).transpose(1, 2).reshape(B_, T, Cc))


class _Mlp(nn.Module):
    def __init__(self, dim, hid):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(dim, hid), nn.Linear(hid, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


def _label_mask(H, W):
    """The published way: an image of region labels, cut into windows."""
    img = torch.zeros(1, H, W, 1, dtype=torch.float64)
    cnt = 0
    for hs in (slice(0, -16), slice(-16, -8), slice(-8, None)):
        for ws in (slice(0, -16), slice(-16, -8), slice(-8, None)):
            img[:, hs, ws, :] = cnt
            cnt += 1
    mw = img.view(1, H // 16, 16, W // 16, 16, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, 256)
    m = mw[:, None, :] - mw[:, :, None]
    return m.masked_fill(m != 0, -100.0).masked_fill(m == 0, 0.0)


class _Swin(nn.Module):
    def __init__(self, dim, nH, hid, shift):
        super().__init__()
        self.shift = shift
        self.norm1, self.norm2 = nn.LayerNorm(dim), nn.LayerNorm(dim)
        self.attn, self.mlp = _Attn(dim, nH), _Mlp(dim, hid)

    def forward(self, x, H, W):          # x [N, H W, dim]
        N, L, Cc = x.shape
        short = x
        x = self.norm1(x).view(N, H, W, Cc)
        if self.shift:
            x = torch.roll(x, (-self.shift, -self.shift), (1, 2))
        xw = x.view(N, H // 16, 16, W // 16, 16, Cc).permute(0, 1, 3, 2, 4, 5).reshape(-1, 256, Cc)
        aw = self.attn(xw, _label_mask(H, W) if self.shift else None)
        x = aw.view(N, H // 16, W // 16, 16, 16, Cc).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, Cc)
        if self.shift:
            x = torch.roll(x, (self.shift, self.shift), (1, 2))
        x = short + x.view(N, L, Cc)
        return x + self.mlp(self.norm2(x))


class _RDG(nn.Module):
    def __init__(self, Cc, heads, hidden):
        super().__init__()
        for k in range(1, 6):
            dim = Cc + 32 * (k - 1)
            setattr(self, f"swin{k}", _Swin(dim, heads[k - 1], hidden[k - 1], 8 if k in (2, 4) else 0))
            setattr(self, f"adjust{k}", nn.Conv2d(dim, 32 if k < 5 else Cc, 1))

    def forward(self, x, H, W):          # tokens [N, H W, C]
        img = lambda t: t.transpose(1, 2).reshape(t.shape[0], t.shape[2], H, W)
        tok = lambda t: t.flatten(2).transpose(1, 2)
        cat = x
        for k in range(1, 5):
            xk = F.leaky_relu(self.__getattr__(f"adjust{k}")(img(self.__getattr__(f"swin{k}")(cat, H, W))), 0.2)
            cat = torch.cat([cat, tok(xk)], 2)
        return 0.2 * tok(self.adjust5(img(self.swin5(cat, H, W)))) + x


class _ModuleDRCT(nn.Module):
    """The network restated the module way (nn.Linear on tokens, F.layer_norm, torch.roll, the mask from a label image), with the published parameter names."""
    def __init__(self, cin, Cc, R, heads, hidden, s):
        super().__init__()
        self.s, self.cin = s, cin
        self.conv_first = nn.Conv2d(cin, Cc, 3, 1, 1)
        self.patch_embed = nn.Module()
        self.patch_embed.norm = nn.LayerNorm(Cc)
        self.layers = nn.ModuleList([_RDG(Cc, heads[5 * i:5 * i + 5], hidden[5 * i:5 * i + 5]) for i in range(R)])
        self.norm = nn.LayerNorm(Cc)
        self.conv_after_body = nn.Conv2d(Cc, Cc, 3, 1, 1)
        self.conv_before_upsample = nn.Sequential(nn.Conv2d(Cc, 64, 3, 1, 1), nn.LeakyReLU())
        ups = [nn.Conv2d(64, 576, 3, 1, 1), nn.PixelShuffle(3)] if s == 3 else [m for _ in range(s // 2) for m in (nn.Conv2d(64, 256, 3, 1, 1), nn.PixelShuffle(2))]
        self.upsample = nn.Sequential(*ups)
        self.conv_last = nn.Conv2d(64, cin, 3, 1, 1)

    def forward(self, x):
        N, _, H, W = x.shape
        mean = torch.tensor(DR.MEAN if self.cin == 3 else (0.0,) * self.cin, dtype=torch.float32).to(x.dtype).view(1, -1, 1, 1)          # (the mean is a float32 constant)
        x = F.pad(x, (0, -W % 16, 0, -H % 16), mode="reflect") - mean
        Hp, Wp = x.shape[2:]
        f0 = self.conv_first(x)
        t = self.patch_embed.norm(f0.flatten(2).transpose(1, 2))
        for layer in self.layers:
            t = layer(t, Hp, Wp)
        t = self.norm(t).transpose(1, 2).reshape(N, -1, Hp, Wp)
        f = self.conv_after_body(t) + f0
        y = self.conv_last(self.upsample(self.conv_before_upsample(f))) + mean
        return y[:, :, :H * self.s, :W * self.s]


def test_reference_against_a_module_style_formulation():
    """forward64 (functional, conv2d on images, the mask from coordinates) == the module-style restatement (Linear on tokens, the mask from a label image), in float64."""
    for name in ("C60 R2 x2 13x21 (padded)", "C96 R1 x3 batch of two 19x26"):
        Cc, nH, R, shape, s, stored, seed = DR.FIXTURES[name]
        sd, x, y64, ys, st = DR.case(name)
        heads = [int(sd[f"layers.{i}.swin{k}.attn.relative_position_bias_table"].shape[1]) for i in range(R) for k in range(1, 6)]
        hidden = [int(sd[f"layers.{i}.swin{k}.mlp.fc1.weight"].shape[0]) for i in range(R) for k in range(1, 6)]
        m = _ModuleDRCT(shape[1], Cc, R, heads, hidden, s).double()
        m.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        with torch.no_grad():
            ym = m(x.double())
        assert ym.shape == y64.shape and float((ym - y64).abs().max()) <= 1e-11, (name, float((ym - y64).abs().max()))
    assert torch.equal(_label_mask(32, 48), HR.shift_mask(32, 48))


# ------------------------------------------------------------------------------------------------ the shell
def test_key_table_and_strict_loading():
    """drct_shapes == the definition written out in _drct_ref; the shell's state dict has exactly those keys (no buffers), loads a filled one strictly and hands it back."""
    from innfer_amd.architectures.DRCT_arch import DRCT
    for v in VARIANTS:
        cin, Cc, R, nH, r, s = v
        want = DR.shapes(*v)
        assert synth.drct_shapes(cin, Cc, R, nH, r, s) == want
        if R > 2:
            continue
        net = DRCT(in_chans=cin, embed_dim=Cc, depths=[6] * R, num_heads=[nH] * R, window_size=16, mlp_ratio=r, upscale=s, upsampler="pixelshuffle")
        assert {k: tuple(t.shape) for k, t in net.state_dict().items()} == {k: tuple(sh) for k, sh in want.items()}
        sd = DR.fill(*v, seed=5)
        net.load_state_dict(sd, strict=True)
        back = net.state_dict()
        assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)          # the round trip
        assert net.heads_follow_rule and net.block_heads == [DR.head_rule(Cc + 32 * k, nH) for _ in range(R) for k in range(5)]
    assert [DR.head_rule(180 + 32 * k, 6) for k in range(5)] == [6, 4, 2, 6, 4]               # d = 30, 53, 122, 46, 77


@pytest.mark.parametrize("v", VARIANTS, ids=_ids)
def test_drct_checkpoints_are_inferred(v):
    """Everything from the shapes alone: bare and under params_ema / params, with and without the buffers (dropped from the state dict handed back); heads and hidden sizes
    are per-block arrays; the checkpoint handed back loads strictly."""
    from innfer_amd.architectures import get_network
    cin, Cc, R, nH, r, s = v
    sd = _zeros(v)
    full = dict(sd, **DR.buffers(sd))
    heads = [DR.head_rule(Cc + 32 * k, nH) for _ in range(R) for k in range(5)]
    hidden = [int((Cc + 32 * k) * r) for _ in range(R) for k in range(5)]
    for wrapped in (sd, {"params_ema": sd}, {"params": sd}, full, {"params_ema": full}):
        info = infer_from_state_dict(wrapped)
        assert (info["arch"], info["scale"], info["nf"], info["nb"], info["in_nc"], info["out_nc"]) == ("drct", s, Cc, 5 * R, cin, cin)
        p = info["net_params"]
        assert (p["type"], p["in_chans"], p["embed_dim"], len(p["depths"]), p["window_size"], p["upscale"], p["img_range"], p["upsampler"], p["gc"]) == \
            ("drct", cin, Cc, R, 16, s, 1.0, "pixelshuffle", 32)
        assert p["block_heads"] == heads and p["block_hidden"] == hidden and info["heads_follow_rule"]
        assert set(info["state_dict"]) == set(sd)
    if R <= 2:
        net = get_network(dict(info["net_params"]))
        net.load_state_dict(info["state_dict"], strict=True)
        assert (net.nf, net.n_groups, net.upscale, net.block_heads, net.block_hidden) == (Cc, R, s, heads, hidden)


def test_heads_and_hidden_come_from_the_checkpoint_not_the_rule():
    """A checkpoint whose blocks do not follow the published rule runs with what it states; the rule's failure is recorded."""
    from innfer_amd.architectures import get_network
    v = (3, 64, 1, 2, 2.0, 2)
    sd = _zeros(v)
    sd["layers.0.swin3.attn.relative_position_bias_table"] = torch.zeros(961, 4)          # 128 channels: 4 heads of 32 instead of the rule's 2 of 64
    sd["layers.0.swin2.mlp.fc1.weight"], sd["layers.0.swin2.mlp.fc1.bias"], sd["layers.0.swin2.mlp.fc2.weight"] = torch.zeros(100, 96), torch.zeros(100), torch.zeros(96, 100)
    info = infer_from_state_dict(sd)
    assert info["net_params"]["block_heads"][2] == 4 and info["net_params"]["block_hidden"][1] == 100 and not info["heads_follow_rule"]
    net = get_network(dict(info["net_params"]))
    net.load_state_dict(info["state_dict"], strict=True)
    assert not net.heads_follow_rule


def test_other_families_still_infer_as_before():
    """An incomplete DRCT key set falls through to the sniffing as it was -- conv_first.weight makes it a new-arch ESRGAN and mod2normal fails on it exactly as on the parent
    commit (a KeyError of the first key it looks for); SwinIR / HAT dictionaries with a stray DRCT key still meet their own refusals."""
    import _swinir_ref as SR
    from innfer_amd.architectures import keys
    from innfer_amd.utils.utils import mod2normal
    sd = _zeros(VARIANTS[2])
    for k in ("layers.0.adjust3.bias", "layers.0.swin5.mlp.fc2.weight", "patch_embed.norm.weight", "layers.0.swin2.attn.relative_position_bias_table"):
        less = {k2: t for k2, t in sd.items() if k2 != k}
        with pytest.raises(Exception) as theirs:
            mod2normal(dict(less))
        with pytest.raises(type(theirs.value)) as ours:
            infer_from_state_dict(less)
        assert str(ours.value) == str(theirs.value) and not isinstance(ours.value, NotImplementedError)
    sw = {k: torch.zeros(s) for k, s in SR.shapes(3, 60, (2,), 6, 2.0, 2, "pixelshuffle", "1conv").items()}
    assert infer_from_state_dict({"params_ema": sw})["arch"] == "swinir"
    assert infer_from_state_dict(dict(sw, **{"layers.0.adjust1.weight": torch.zeros(32, 60, 1, 1)}))["arch"] == "swinir"          # (a stray key no refusal names)
    hat = {k: torch.zeros(s) for k, s in HR.shapes(3, 60, (2,), 6, 2.0, 2, 3, 30).items()}
    with pytest.raises(NotImplementedError, match="DRCT"):
        infer_from_state_dict(dict(hat, **{"layers.0.swin_DRCT.x": torch.zeros(1)}))
    with pytest.raises(NotImplementedError, match="HAT / DRCT"):
        infer_from_state_dict(dict(sw, **{"layers.0.residual_group.overlap_attn.qkv.weight": torch.zeros(180, 60)}))
    new = infer_from_state_dict({k: torch.zeros(s) for k, s in keys.mrrdbnet_shapes(nb=23).items()})
    assert (new["arch"], new["scale"], new["nb"]) == ("esrgan", 4, 23)


def test_refusals():
    """Clear NotImplementedErrors, raised by the sniffing or the shell's constructor: nothing touches the GPU."""
    from innfer_amd.architectures import get_network
    from innfer_amd.architectures.DRCT_arch import DRCT
    v = (3, 60, 1, 6, 2.0, 2)
    sd = _zeros(v)

    def refused(changed, match):
        with pytest.raises(NotImplementedError, match=match):
            infer_from_state_dict({"params_ema": changed})
    bad = DR.buffers(sd)
    bad["layers.0.swin3.attn.relative_position_index"] = bad["layers.0.swin3.attn.relative_position_index"].clone()
    bad["layers.0.swin3.attn.relative_position_index"][3, 5] += 1
    refused(dict(sd, **bad), "swin3.attn.relative_position_index differs")
    refused(dict(sd, absolute_pos_embed=torch.zeros(1, 4096, 60)), "absolute_pos_embed")
    g16 = dict(sd)                                                                           # gc 16
    g16["layers.0.adjust1.weight"], g16["layers.0.adjust1.bias"] = torch.zeros(16, 60, 1, 1), torch.zeros(16)
    refused(g16, "gc 16")
    w8 = dict(sd)
    for k in sd:
        if k.endswith("attn.relative_position_bias_table"):
            w8[k] = torch.zeros(225, sd[k].shape[1])
    refused(w8, "window_size 8")
    refused(_zeros((3, 288, 1, 6, 2.0, 2)), "embed_dim 288")
    h5 = dict(sd)
    h5["layers.0.swin2.attn.relative_position_bias_table"] = torch.zeros(961, 5)            # 92 % 5 != 0
    refused(h5, "5 heads on 92 channels")
    h1 = dict(sd)
    h1["layers.0.swin4.attn.relative_position_bias_table"] = torch.zeros(961, 1)            # d = 156 > 128
    refused(h1, "1 heads on 156 channels")
    refused(_zeros((3, 72, 1, 9, 2.0, 2)), "9 heads on 72 channels")                        # more than 8 heads
    refused(_zeros((3, 180, 1, 6, 4.0, 2)), "hidden channels")                              # 308 x 4 > 1024 (the first block over the limit is named)
    refused({k: t for k, t in sd.items() if not k.startswith(("conv_before_upsample", "upsample", "conv_last"))}, "pixelshuffle tail")
    x8 = dict(sd)
    for st in (2, 4):
        x8[f"upsample.{st}.weight"], x8[f"upsample.{st}.bias"] = torch.zeros(256, 64, 3, 3), torch.zeros(256)
    refused(x8, "scale 8")
    refused(_zeros((5, 60, 1, 6, 2.0, 2)), "takes 5")
    o1 = dict(sd)
    o1["conv_last.weight"], o1["conv_last.bias"] = torch.zeros(1, 64, 3, 3), torch.zeros(1)
    refused(o1, "conv_last has 1 channels")
    info = infer_from_state_dict(sd)
    with pytest.raises(NotImplementedError, match="img_range"):                             # the -range net_param
        get_network(dict(info["net_params"], img_range=255.0))
    ok = dict(embed_dim=60, depths=[6], num_heads=[6], window_size=16, mlp_ratio=2.0, upscale=2, upsampler="pixelshuffle")
    for what, kw in (("window_size", dict(window_size=8)), ("gc", dict(gc=16)), ("upsampler", dict(upsampler="pixelshuffledirect")), ("upscale", dict(upscale=8)),
                     ("ape", dict(ape=True)), ("patch_norm", dict(patch_norm=False)), ("qkv_bias", dict(qkv_bias=False)), ("img_range", dict(img_range=255.0)),
                     ("in_chans", dict(in_chans=5)), ("num_heads", dict(depths=[6, 6], num_heads=[6, 3])), ("embed_dim", dict(embed_dim=288)),
                     ("hidden channels", dict(embed_dim=180, mlp_ratio=4.0)), ("patch_size", dict(patch_size=2)), ("resi_connection", dict(resi_connection="3conv")),
                     ("heads on", dict(block_heads=[6, 4, 2, 6, 5], block_hidden=[8] * 5))):
        with pytest.raises(NotImplementedError, match=what):
            DRCT(**dict(ok, **kw))
    net = DRCT(**ok)
    assert DRCT._has_fp32 is False                         # -no_fp16 is refused by run.py's check of this flag
    with pytest.raises(NotImplementedError, match="DRCT is built for the fp16 mode only"):
        net.forward(torch.zeros(1, 3, 16, 16))
    with pytest.raises(NotImplementedError, match="fp16 mode only"):
        net.tile_batch_bytes(1, 16, torch.float32)
    for H, W in ((8, 16), (16, 7), (1, 1), (2, 33)):
        with pytest.raises(NotImplementedError, match="reflection"):
            net.forward(torch.zeros(1, 3, H, W, dtype=torch.float16))


def test_new_symbols_are_declared_and_bound():
    """ABI 124; the revision note names the new entries; they are declared as additive, bound in lib.py, and their source is part of the build; win_attn16.hip is untouched
    by this file's feature (its kernel has no G)."""
    hdr = open(os.path.join(ROOT, "include", "innfer_amd.h")).read()
    lib_py = open(os.path.join(ROOT, "innfer_amd", "lib.py")).read()
    assert re.search(r"^#define INNFER_ABI_VERSION 124$", hdr, re.M) and "ABI_VERSION = 124" in lib_py
    note = hdr[hdr.index("/* ABI revision of this header"):hdr.index("#define INNFER_ABI_VERSION")]
    for sym in ("innfer_window_attention16_wide", "innfer_drct_create", "innfer_layer_norm_holed"):
        assert sym in note, sym
        assert re.search(r"/\* \(124, additive\)(?:(?!\*/).)*\*/\nint %s\(" % sym, hdr, re.S), sym
        assert '"%s"' % sym in lib_py, sym
    net = open(os.path.join(ROOT, "innfer_amd", "csrc", "net.hip")).read()
    assert "net->kind == 9" in net and "win_attn16_wide_launch" in net and "layer_norm_holed_launch" in net
    assert "csrc/win_attn16_wide.hip" in open(os.path.join(ROOT, "Makefile")).read()
    assert "template <int KW>" in open(os.path.join(ROOT, "innfer_amd", "csrc", "win_attn16.hip")).read()


_USAGE = {}


def _resource_usage(name):
    """hipcc's kernel resource-usage remarks for csrc/<name>.hip: {mangled kernel name: {field: value}} (compiled once per file)."""
    import shutil
    import subprocess
    if name in _USAGE:
        return _USAGE[name]
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    src = os.path.join(ROOT, "innfer_amd", "csrc", name + ".hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+))", line)
        if m and m.group(1):
            cur = kernels.setdefault(m.group(1), {})
        elif m:
            cur[m.group(2).strip()] = int(m.group(3))
    _USAGE[name] = kernels
    return kernels


def test_wide_attention_uses_no_scratch_and_fits_two_waves_a_simd():
    """The scratch condition, at compile time: hipcc's kernel resource-usage remarks for csrc/win_attn16_wide.hip state ScratchSize 0 for all three instantiations, and
    VGPRs + AGPRs <= 256, so that the two waves a SIMD that an 8-wave workgroup needs fit (DESIGN.md 3.4p records the figures)."""
    kernels = _resource_usage("win_attn16_wide")
    wide = {k: v for k, v in kernels.items() if "win_attn16_wide_kernel" in k}
    print({k: (v.get("VGPRs"), v.get("AGPRs"), v.get("ScratchSize")) for k, v in wide.items()})
    assert len(wide) == 3, list(kernels)
    for k, v in wide.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["VGPRs"] + v["AGPRs"] <= 256, (k, v)


# (file, the instantiation inside the mangled name): (static LDS bytes, waves a SIMD as the compiler reports them) of the build BEFORE the four kernels shared
# csrc/win_attn_core.h -- the copies the core replaced.  The wide kernel's LDS is dynamic (0 here).
WINDOW_KERNELS = {
    ("win_attn", "win_attn_kernelILb1E"): (19456, 4), ("win_attn", "win_attn_kernelILb0E"): (18432, 2),
    ("win_attn16", "win_attn16_kernelILi16E"): (16896, 2), ("win_attn16", "win_attn16_kernelILi24E"): (37376, 2),
    ("win_attn16_wide", "win_attn16_wide_kernelILi2E"): (0, 3), ("win_attn16_wide", "win_attn16_wide_kernelILi3E"): (0, 3),
    ("win_attn16_wide", "win_attn16_wide_kernelILi4E"): (0, 2),
    ("win_attn_rect", "win_attn_rect_kernelILi256E"): (16896, 2), ("win_attn_rect", "win_attn_rect_kernelILi128E"): (8704, 2),
}


@pytest.mark.parametrize("src", sorted({f for f, _ in WINDOW_KERNELS}))
def test_window_attention_kernels_keep_their_resources(src):
    """Every instantiation of the four window-attention kernels, built on the shared core: no scratch, the static LDS of the separate copies byte for byte, and no
    fewer waves a SIMD than they had (DESIGN.md 3.4p records the register counts of both)."""
    kernels = _resource_usage(src)
    for (f, inst), (lds, waves) in WINDOW_KERNELS.items():
        if f != src:
            continue
        hit = [v for k, v in kernels.items() if inst in k]
        assert len(hit) == 1, (inst, list(kernels))
        v = hit[0]
        print(inst, {q: v.get(q) for q in ("VGPRs", "AGPRs", "ScratchSize", "LDS Size", "Occupancy")})
        assert v["ScratchSize"] == 0, (inst, v)
        assert v["LDS Size"] == lds, (inst, v)
        assert v["Occupancy"] >= waves, (inst, v)


# ------------------------------------------------------------------------------------------------ the folds, taken apart and put together again
def _net(name):
    from innfer_amd.architectures import get_network
    info = infer_from_state_dict({"params_ema": DR.fixture_sd(name)})
    net = get_network(dict(info["net_params"]))
    net.load_state_dict(info["state_dict"], strict=True)
    return net


def _whole(net, key, sd):
    """The engine's whole weight / bias of a sliced conv."""
    return net._conv_tensors(key, sd)


def test_engine_tensors_taken_apart_again():
    """What the shell hands the engine for every Linear / adjust conv of a block, un-permuted, un-padded and un-folded, is the checkpoint: exactly where the re-layout is
    index work, within one float32 rounding where it folds (d^-0.5 into q, + mean into conv_last); everything the layout adds (the hole, the pads, the head padding, the
    32 zero rows of an adjust conv) is zero; the dense bias table's entries are the table's at the index formula."""
    from innfer_amd.architectures.DRCT_arch import pad64, slab_index
    for name in ("C60 R2 x2 13x21 (padded)", "C180 R1 x4 32x48"):
        Cc, nH0, R, shape, s, stored, seed = DR.FIXTURES[name]
        net = _net(name)
        sd = net.state_dict()
        gx, Cp = -(-Cc // 32), pad64(Cc)
        for i in range(R):
            for k in range(5):
                dim, nh, hid = Cc + 32 * k, net.block_heads[5 * i + k], net.block_hidden[5 * i + k]
                d = dim // nh
                Gh, cpk, lp = -(-d // 32), 32 * (gx + k), pad64(32 * (gx + k))
                pos = slab_index(Cc, dim)
                assert len(set(pos.tolist())) == dim and pos.max() < cpk and not ((pos >= Cc) & (pos < 32 * gx)).any()          # a permutation into the real channels
                hpos = np.array([(c // d) * 32 * Gh + c % d for c in range(dim)])
                b = f"layers.{i}.swin{k + 1}."
                w0 = lambda key: (sd[key + ".weight"].numpy().reshape(sd[key + ".weight"].shape[0], -1), sd[key + ".bias"].numpy())
                # qkv: rows head-padded per section, columns in slab order, q scaled
                w, bb = _whole(net, b + "attn.qkv", sd)
                wq, bq = w0(b + "attn.qkv")
                assert w.dtype == np.float32 and w.shape == ((3 * nh * Gh + 1) // 2 * 64, cpk, 1, 1)
                assert np.array_equal(net._conv_tensors(b + "attn.qkv#1", sd)[0], w[64:128])
                for which in range(3):
                    rows = which * nh * Gh * 32 + hpos
                    un, ub = w[rows][:, pos, 0, 0], bb[rows]
                    if which:
                        assert np.array_equal(un, wq[which * dim:(which + 1) * dim]) and np.array_equal(ub, bq[which * dim:(which + 1) * dim])
                    else:
                        assert np.allclose(un * np.float32(d ** 0.5), wq[:dim], rtol=2.0 ** -22, atol=0) and np.allclose(ub * np.float32(d ** 0.5), bq[:dim], rtol=2.0 ** -22, atol=0)
                        assert np.array_equal(un, (wq[:dim].astype(np.float64) * d ** -0.5).astype(np.float32))                    # the fold in float64, one rounding
                assert np.count_nonzero(w) == np.count_nonzero(wq) and np.count_nonzero(bb) == np.count_nonzero(bq)
                # proj: rows in slab order, columns head-padded
                w, bb = _whole(net, b + "attn.proj", sd)
                wp, bp = w0(b + "attn.proj")
                assert w.shape == (lp, 32 * nh * Gh, 1, 1) and np.array_equal(w[pos][:, hpos, 0, 0], wp) and np.array_equal(bb[pos], bp)
                assert np.count_nonzero(w) == np.count_nonzero(wp) and np.count_nonzero(bb) == np.count_nonzero(bp)
                w, bb = _whole(net, b + "mlp.fc1", sd)
                w1, b1 = w0(b + "mlp.fc1")
                assert w.shape == (pad64(hid), cpk, 1, 1) and np.array_equal(w[:hid][:, pos, 0, 0], w1) and np.array_equal(bb[:hid], b1) and np.count_nonzero(w) == np.count_nonzero(w1)
                w, bb = _whole(net, b + "mlp.fc2", sd)
                w2, b2 = w0(b + "mlp.fc2")
                assert w.shape == (lp, pad64(hid), 1, 1) and np.array_equal(w[pos][:, :hid, 0, 0], w2) and np.array_equal(bb[pos], b2) and np.count_nonzero(w) == np.count_nonzero(w2)
                w, bb = _whole(net, f"layers.{i}.adjust{k + 1}", sd)
                wa, ba = w0(f"layers.{i}.adjust{k + 1}")
                assert w.shape == ((64 if k < 4 else Cp), cpk, 1, 1) and np.array_equal(w[:wa.shape[0]][:, pos, 0, 0], wa) and np.array_equal(bb[:wa.shape[0]], ba)
                assert not w[wa.shape[0]:].any() and not bb[wa.shape[0]:].any() and np.count_nonzero(w) == np.count_nonzero(wa)   # (k < 4: the rows that clear the next group)
        w, bb = net._conv_tensors("conv_last", sd)
        assert np.array_equal(w, sd["conv_last.weight"].numpy()) and np.allclose(bb - np.float32(DR.MEAN), sd["conv_last.bias"].numpy(), rtol=0, atol=2.0 ** -24)
        for key, rows, cols in (("conv_first", Cp, 3), ("conv_after_body", Cp, Cp), ("conv_before_upsample.0", 64, Cp)):
            w, bb = net._conv_tensors(key, sd)
            wk = sd[key + ".weight"].numpy()
            assert w.shape == (rows, cols, 3, 3) and np.array_equal(w[:wk.shape[0], :wk.shape[1]], wk) and np.count_nonzero(w) == np.count_nonzero(wk)
        norms, tables = net.engine_tables()
        assert len(norms) == 2 + 10 * R and len(tables) == 5 * R
        idx = HR.index_sa()
        for blk, t in enumerate(tables):
            i, k = divmod(blk, 5)
            tab = sd[f"layers.{i}.swin{k + 1}.attn.relative_position_bias_table"]
            assert t.dtype == np.float32 and t.shape == (net.block_heads[blk], 256, 256) and np.array_equal(t, HR.dense_table(tab, idx).numpy())
            for q, kk in ((0, 0), (17, 200), (255, 3)):
                assert np.array_equal(t[:, q, kk], tab[(q // 16 - kk // 16 + 15) * 31 + (q % 16 - kk % 16 + 15)].numpy())
            for j, nk in ((1, "norm1"), (2, "norm2")):
                g, be = norms[2 * blk + j]
                dim = Cc + 32 * k
                pos = slab_index(Cc, dim)
                assert g.shape == (pad64(32 * (gx + k)),) and np.array_equal(g[pos], sd[f"layers.{i}.swin{k + 1}.{nk}.weight"].numpy())
                assert np.array_equal(be[pos], sd[f"layers.{i}.swin{k + 1}.{nk}.bias"].numpy()) and np.count_nonzero(g) == dim


def _engine_graph64(net, x):
    """The engine's graph (csrc/net.hip, kind 9) restated in float64 ON THE SLAB LAYOUT with the tensors the shell hands over: the dense slab with its hole, the holed
    LayerNorm, the head-padded qkv slab, adjust launches of 64 outputs that clear the next group, 0.2 x_5 + x in the adjust conv.  Unwritten groups hold NaN."""
    from innfer_amd.architectures.DRCT_arch import pad64
    dt = torch.float64
    sd = net.state_dict()
    Cc, s = net.nf, net.upscale
    gx, Cp = -(-Cc // 32), pad64(Cc)
    T = lambda key: tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dt) for a in net._conv_tensors(key, sd))
    conv = lambda key, t, cin=None: F.conv2d(t if cin is None else t[:, :cin], T(key)[0], T(key)[1], padding=T(key)[0].shape[-1] // 2)
    norms, tables = net.engine_tables()
    N, cin, H, W = x.shape
    x = F.pad(x.to(dt), (0, -W % 16, 0, -H % 16), mode="reflect") - torch.tensor(net.mean, dtype=dt).view(1, -1, 1, 1)
    Hp, Wp = x.shape[2:]
    f0 = conv("conv_first", x)

    def ln(idx, t, real):
        g, b = (torch.from_numpy(a).to(dt) for a in norms[idx])
        width = g.shape[0]
        tr = t[:, :width][:, real]
        y = (tr - tr.mean(1, keepdim=True)) / torch.sqrt(tr.var(1, unbiased=False, keepdim=True) + 1e-5)
        out = torch.zeros(N, width, Hp, Wp, dtype=dt)
        out[:, real] = y * g[real].view(1, -1, 1, 1) + b[real].view(1, -1, 1, 1)
        return out
    DG = (gx + 6) // 2 * 2
    D = torch.full((N, 32 * DG, Hp, Wp), float("nan"), dtype=dt)
    D[:, :Cp] = ln(0, f0, torch.arange(Cp) < Cc)
    M = HR.shift_mask(Hp, Wp)
    li = 1
    for i in range(net.n_groups):
        Dn = torch.full_like(D, float("nan"))
        for k in range(5):
            blk = 5 * i + k
            dim, nh = Cc + 32 * k, net.block_heads[blk]
            d = dim // nh
            Gh, cpk, lp = -(-d // 32), 32 * (gx + k), pad64(32 * (gx + k))
            real = torch.tensor([c < Cc or 32 * gx <= c < cpk for c in range(lp)])
            b = f"layers.{i}.swin{k + 1}."
            u = ln(li, D, real); li += 1
            qkv = conv(b + "attn.qkv", u, cpk)
            hg = nh * Gh
            shift = 8 if k & 1 else 0
            qs = torch.roll(qkv, (-shift, -shift), (2, 3)) if shift else qkv
            win = HR._windows(qs)                                                                    # [N, nW, 256, channels]
            sec = lambda w: win[..., w * hg * 32:(w + 1) * hg * 32].reshape(N, -1, 256, nh, 32 * Gh).permute(0, 1, 3, 2, 4)
            S = sec(0) @ sec(1).transpose(-1, -2) + torch.from_numpy(tables[blk]).to(dt)
            if shift:
                S = S + M[None, :, None]
            o = torch.softmax(S, -1) @ sec(2)
            o = o * (torch.arange(32 * Gh) < d).to(dt)                                               # channels >= d are written as zeros
            att = HR._unwindows(o.permute(0, 1, 3, 2, 4).reshape(N, -1, 256, hg * 32), Hp, Wp)
            if shift:
                att = torch.roll(att, (shift, shift), (2, 3))
            t = conv(b + "attn.proj", att) + D[:, :lp]
            u = ln(li, t, real); li += 1
            hid = F.gelu(conv(b + "mlp.fc1", u, cpk))
            t = conv(b + "mlp.fc2", hid) + t
            if k < 4:
                D[:, cpk:cpk + 64] = F.leaky_relu(conv(f"layers.{i}.adjust{k + 1}", t, cpk), 0.2)
            else:
                Dn[:, :Cp] = 0.2 * conv(f"layers.{i}.adjust5", t, cpk) + D[:, :Cp]
        D = Dn
    t = ln(li, D, torch.arange(Cp) < Cc)
    f = conv("conv_after_body", t) + f0
    y = F.leaky_relu(conv("conv_before_upsample.0", f), 0.01)
    for key in sorted(k[:-7] for k in sd if k.startswith("upsample.") and k.endswith(".weight")):
        y = F.pixel_shuffle(conv(key, y), 3 if s == 3 else 2)
    return conv("conv_last", y)[:, :, :H * s, :W * s]


@pytest.mark.parametrize("name", list(DR.FIXTURES))
def test_engine_graph_on_the_slab_layout_gives_the_reference(name):
    """Put together again: the engine's graph on the dense slab, in float64 with the shell's tensors, equals forward64 up to the float32 rounding of the folded weights --
    and stays finite although every group starts as NaN: no product reads a group before it is written (the order net.hip relies on)."""
    Cc, nH, R, shape, s, stored, seed = DR.FIXTURES[name]
    sd, x, y64, ys, st = DR.case(name)
    y = _engine_graph64(_net(name), x)
    assert torch.isfinite(y).all() and y.shape == y64.shape
    err, es = float((y - y64).abs().max()), float((ys - y64).abs().max())
    print(f"drct {name}: engine graph in float64 vs forward64 {err:.2e} (storage model {es:.2e})")
    assert err <= 1e-5 and err <= es / 50


def test_launch_formula():
    """2 S1 + 2 + sum over blocks (3 + SQ + 2 S + SH + A) + T + 2 [padded], written out for DRCT x4 (C 180, R 6)."""
    from innfer_amd.architectures.DRCT_arch import DRCT
    net = DRCT(embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, window_size=16, upscale=4, upsampler="pixelshuffle")
    per_group = 0
    for k, (nh, G, S, hid) in enumerate(((6, 1, 3, 360), (4, 2, 4, 424), (2, 4, 4, 488), (6, 2, 5, 552), (4, 3, 5, 616))):
        per_group += 3 + (3 * nh * G + 1) // 2 + 2 * S + -(-hid // 64) + (1 if k < 4 else 3)
    assert net.launches(False) == 2 * 3 + 2 + 6 * per_group + 4 and net.launches(True) == net.launches(False) + 2


# ------------------------------------------------------------------------------------------------ the fixtures' own conditions
@pytest.mark.parametrize("name", list(DR.FIXTURES))
def test_storage_model_is_what_the_gpu_tests_take_it_for(name):
    """Guards the test data of tests/test_gpu_drct.py: on every network fixture the fp16 storage model alone has 100 % of its uint8 codes within +-1 of float64 (its max
    error is printed: the GPU tests allow the engine twice that), something IS rounded, the result is an image that reaches both clips, and the scores of a wide-head block
    spread: max |q k^T| >= 4."""
    Cc, nH, R, shape, s, stored, seed = DR.FIXTURES[name]
    sd, x, y64, ys, st = DR.case(name)
    err = float((ys - y64).abs().max())
    share = DR.codes_within_one(ys, y64)
    wide = [v for d, v in st["smax"] if d > 32]
    print(f"drct {name} (seed {seed}): storage model max|err| {err:.2e}, codes within +-1 {share:.5f}, range [{float(y64.min()):.3f}, {float(y64.max()):.3f}]; "
          f"(d, max |S|) per block: {[(d, round(v, 1)) for d, v in st['smax']]}")
    assert tuple(y64.shape) == (shape[0], 3, shape[2] * s, shape[3] * s) and torch.isfinite(y64).all()
    assert share == 1.0, (name, share)
    assert err >= 2.0 ** -13, (name, err)                   # fp16 storage costs something: the model is not float64 by accident
    assert float(y64.min()) < 0.0 and float(y64.max()) > 0.8
    assert float(y64.min()) > -0.6 and float(y64.max()) < 1.6
    assert wide and max(wide) >= 4.0, (name, st["smax"])
    assert len(st["smax"]) == 5 * R and any(d <= 32 for d, v in st["smax"])          # both attention kernels run


def test_planted_faults_move_the_result():
    """Each mistake moves forward64 by at least 10 x the storage model's error on at least one fixture: the network tests would see it."""
    worst = {f: 0.0 for f in FAULTS}
    for name in DR.FIXTURES:
        Cc, nH, R, shape, s, stored, seed = DR.FIXTURES[name]
        sd, x, y64, ys, st = DR.case(name)
        es = float((ys - y64).abs().max())
        for f in FAULTS:
            if worst[f] >= 10.0:
                continue
            r = float((DR.forward64(sd, x, s, fault=f) - y64).abs().max()) / es
            print(f"drct fault {f} on {name}: {r:.1f} x the storage model's error")
            worst[f] = max(worst[f], r)
    assert all(r >= 10.0 for r in worst.values()), worst
