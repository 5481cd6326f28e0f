"""Single-launch cases of the fp32 mode's generic convolution (csrc/f32ops.hip f32conv_launch) and their float64 references -- TEST INFRASTRUCTURE.

A case is one layer in torch's terms (nn.Conv2d with a padding mode, a nearest-2x upsample in front, a dilation, WBC's `tf` stride-2 padding, or
nn.ConvTranspose2d(k, 2, 1)), plus the views and the epilogue of the launch.  `launches(case)` states it as the F32Conv launches the networks make
for that layer (the call site is named on each form); `reference(case, ...)` computes the same layer with stock torch.nn.functional in float64.
tests/test_f32_plan_cpu.py asks the planner about these launches, tests/test_gpu_f32ops.py runs them.
"""
import dataclasses

import numpy as np
import torch
import torch.nn.functional as F


@dataclasses.dataclass
class Case:
    name: str
    N: int
    C: int
    H: int                       # input grid
    W: int
    K: int
    kind: str = "conv"           # conv | convT4 (four phase launches) | convT1 (one launch, phase_k) | rows (1 x 1, 64-float output rows)
    k: int = 3                   # kernel size
    stride: int = 1
    pad: int = -1                # -1: k // 2 * dil
    dil: int = 1
    tf: bool = False             # stride-2 taps padded (0, 1): WBC tf_same_padding
    pad_mode: int = 0            # 0 zero, 1 reflect, 2 replicate
    up: bool = False             # nearest-2x upsample in front
    in_act: int = 0
    act: int = 0
    oscale: float = 0.0
    res: bool = False
    mul: bool = False
    ctot: int = 0                # channels of the tensor the input view lies in (0: C), view at channel coff
    coff: int = 0
    ktot: int = 0                # channels of the output tensor (0: K), view at channel koff
    koff: int = 0
    seed: int = 0

    def __post_init__(self):
        self.ctot = self.ctot or self.C + self.coff
        self.ktot = self.ktot or self.K + self.koff
        if self.pad < 0:
            self.pad = self.k // 2 * self.dil

    @property
    def out_hw(self):
        if self.kind in ("convT4", "convT1"):
            return 2 * self.H, 2 * self.W
        if self.up:
            return 2 * self.H, 2 * self.W
        return self.H // self.stride, self.W // self.stride


# ---- the taps of ConvTranspose2d(k, 2, 1, output_padding = k == 3) per output phase a (one axis): [(kernel index, input displacement)]
#      k = 4: unet.hip phase_taps (out 2 i + a takes in[i + d] * w[ky]); k = 3: resnet.hip phase_taps1d
def phase_taps1d(k, a):
    if k == 4:
        return [(1, 0), (3, -1)] if a == 0 else [(0, 1), (2, 0)]
    return [(1, 0)] if a == 0 else [(0, 1), (2, 0)]


def weights(case):
    """(weight in torch's layout, bias), fp32: conv [K][C][k][k], transposed [C][K][k][k]; scaled by 1 / sqrt(k k C)."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    shape = (case.C, case.K, case.k, case.k) if case.kind in ("convT4", "convT1") else (case.K, case.C, case.k, case.k)
    w = (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) / np.sqrt(case.k * case.k * case.C)
    b = torch.rand((case.K,), generator=g, dtype=torch.float64) - 0.5
    return w.float(), b.float()


def launches(case):
    """[(F32Conv fields without pointers, weight function w(k, c, tap) as a [K'][C][ntap] array, written pixels [Ho][Wo] bool)] of the layer."""
    w, _ = weights(case)
    w = w.numpy()
    Ho, Wo = case.out_hw
    base = dict(C=case.C, Hin=case.H, Win=case.W, N=case.N, pad_mode=case.pad_mode, in_act=case.in_act, act=case.act, oscale=case.oscale)
    out = []
    if case.kind == "conv":                                    # resnet.hip:618-625, wbcunet.hip:409-424, unet.hip:910-921 (4 x 4 s 2), ppon.hip:426-438 (dilated, up)
        k, p0 = case.k, (0 if case.tf else case.pad)
        taps = [(ky * case.dil - p0, kx * case.dil - p0) for ky in range(k) for kx in range(k)]
        d = dict(base, K=case.K, Wout=Wo, Ho=Ho, Wo=Wo, osy=1, osx=1, ooy=0, oox=0, isy=case.stride, isx=case.stride, up=int(case.up), taps=taps)
        out.append((d, w.reshape(case.K, case.C, k * k), np.ones((Ho, Wo), bool)))
    elif case.kind == "rows":                                  # pan.hip:1090-1098: [f | g | h] rows of 64 floats per pixel
        d = dict(base, K=case.K, Wout=Wo, Ho=Ho, Wo=Wo, osy=1, osx=1, ooy=0, oox=0, isy=1, isx=1, up=0, taps=[(0, 0)])
        out.append((d, w.reshape(case.K, case.C, 1), np.ones((Ho, Wo), bool)))
    elif case.kind == "convT4":                                # four phase launches: unet.hip:940-946 (k 4), resnet.hip:603-617 (k 3)
        for ph in range(4):
            a, b = ph >> 1, ph & 1
            ty, tx = phase_taps1d(case.k, a), phase_taps1d(case.k, b)
            taps = [(dy, dx) for (_, dy) in ty for (_, dx) in tx]
            wp = np.stack([w[:, :, ky, kx].T for (ky, _) in ty for (kx, _) in tx], axis=-1)     # [K][C][ntap]
            d = dict(base, K=case.K, Wout=2 * case.W, Ho=case.H, Wo=case.W, osy=2, osx=2, ooy=a, oox=b, isy=1, isx=1, up=0, taps=taps)
            m = np.zeros((2 * case.H, 2 * case.W), bool)
            m[a::2, b::2] = True
            out.append((d, np.ascontiguousarray(wp), m))
    elif case.kind == "convT1":                                # the four phases as ONE launch of K = 4 cout channels, 3 x 3 taps: unet.hip:925-930, 870-882
        taps = [(t // 3 - 1, t % 3 - 1) for t in range(9)]
        wp = np.zeros((4 * case.K, case.C, 9), np.float32)
        for ph in range(4):
            for (ky, dy) in phase_taps1d(case.k, ph >> 1):
                for (kx, dx) in phase_taps1d(case.k, ph & 1):
                    wp[ph * case.K:(ph + 1) * case.K, :, (dy + 1) * 3 + dx + 1] = w[:, :, ky, kx].T
        d = dict(base, K=4 * case.K, phase_k=case.K, Wout=2 * case.W, Ho=case.H, Wo=case.W, osy=1, osx=1, ooy=0, oox=0, isy=1, isx=1, up=0, taps=taps)
        out.append((d, wp, np.ones((2 * case.H, 2 * case.W), bool)))
    else:
        raise ValueError(case.kind)
    return out


def _act(v, act):
    if act == 1:
        return F.leaky_relu(v, 0.2)
    if act == 2:
        return F.relu(v)
    if act == 3:
        return torch.tanh(v)
    if act == 4:
        return torch.sigmoid(v)
    return v


def conv_only(case, x, w, pads=None):
    """The layer's convolution (no bias / epilogue) in float64: x [N][C][h][w] (the input view, or a crop of it whose borders `pads` (t, b, l, r)
    take the padding -- None: the layer's own)."""
    x = _act(x.double(), case.in_act)
    w = w.double()
    if case.kind in ("convT4", "convT1"):
        return F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1 if case.k == 3 else 0)
    if case.up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if pads is None:
        p = case.pad
        pads = (0, 1, 0, 1) if case.tf else (p, p, p, p)
    else:
        pads = (pads[2], pads[3], pads[0], pads[1])
    if any(pads):
        x = F.pad(x, pads, mode=("constant", "reflect", "replicate")[case.pad_mode])
    return F.conv2d(x, w, stride=case.stride, dilation=case.dil)


def epilogue(case, v, b, mul=None, res=None):
    """bias, gate, activation, scale, residual (the kernels' epilogue, f32ops.hip:9-14) in float64."""
    v = v + b.double().view(1, -1, 1, 1)
    if case.mul:
        v = mul.double() * torch.sigmoid(v)
    v = _act(v, case.act)
    if case.oscale != 0.0:
        v = v * case.oscale
    if case.res:
        v = v + res.double()
    return v


def reference(case, x, mul=None, res=None):
    """The whole output [N][K][Ho][Wo] in float64 from the fp32 input view x [N][C][H][W]."""
    w, b = weights(case)
    return epilogue(case, conv_only(case, x, w), b, mul, res)


# ---- the seeded sweep -----------------------------------------------------------------------------------------------------------------------------
# Named cases first: every form the networks launch, the views, the channel counts around the chunk size, the grids around the tile sizes, batches
# that leave a multi-image tile ragged.  Then random ones over the same axes.
def named_cases():
    c = []
    a = c.append
    # ResNet (CycleGAN): 7 x 7 reflect first / last conv, 3 x 3 reflect / replicate / zero residual-block convs, stride-2 down, k3 transposed phases
    a(Case("resnet_c7_reflect_first", 1, 3, 37, 70, 64, k=7, pad_mode=1, act=2))
    a(Case("resnet_c7_reflect_last_tanh", 2, 64, 21, 40, 3, k=7, pad_mode=1, act=3))
    a(Case("resnet_block_reflect", 2, 64, 19, 33, 64, pad_mode=1, act=2))
    a(Case("resnet_block_replicate_res", 1, 96, 17, 24, 96, pad_mode=2, res=True))
    a(Case("resnet_down_s2", 1, 64, 30, 62, 128, stride=2, act=2))
    a(Case("resnet_convT3_phases", 2, 128, 9, 14, 64, kind="convT4", k=3, act=2))
    a(Case("resnet_upconv_nearest_reflect", 1, 64, 13, 22, 48, up=True, pad_mode=1, act=1))
    # pix2pix UNet: 4 x 4 stride-2 down convs with LeakyReLU on the input, transposed convs (four phases / fused phase_k) with ReLU on the input
    a(Case("unet_down_k4s2", 1, 3, 64, 64, 64, k=4, stride=2, pad=1, in_act=1))
    a(Case("unet_down_k4s2_cat_view", 2, 128, 16, 16, 256, k=4, stride=2, pad=1, in_act=1, ctot=256, coff=128, ktot=512, koff=256))
    a(Case("unet_down_k4s2_1x1_grid", 65, 512, 2, 2, 512, k=4, stride=2, pad=1, in_act=1))
    a(Case("unet_convT4_phases", 3, 512, 4, 4, 256, kind="convT4", k=4, in_act=2, ktot=512, koff=0))
    a(Case("unet_convT4_phases_cat_out", 2, 128, 16, 16, 64, kind="convT4", k=4, in_act=2, ktot=128, koff=64))
    a(Case("unet_convT4_fused_outermost", 2, 128, 32, 32, 3, kind="convT1", k=4, in_act=2, act=3))
    a(Case("unet_convT3_fused", 1, 20, 11, 13, 4, kind="convT1", k=3, in_act=2))
    a(Case("unet_upconv", 1, 64, 8, 8, 32, up=True, in_act=2))
    # WBC UNet: tf stride-2 taps, 7 x 7 zero padding, residual
    a(Case("wbc_tf_s2", 2, 32, 24, 40, 32, stride=2, tf=True, act=1))
    a(Case("wbc_pt_s2", 1, 32, 24, 40, 64, stride=2, act=1))
    a(Case("wbc_c7", 1, 3, 32, 48, 32, k=7, act=1))
    a(Case("wbc_res", 1, 128, 6, 10, 128, res=True))
    # PPON: dilated taps up to 8 (zero padding = dilation), the 2x nearest up-stage, oscale + residual
    for dil in (2, 3, 5, 8):
        a(Case(f"ppon_dilated_{dil}", 1, 32, 20, 29, 32, dil=dil, act=1, ktot=256, koff=32 * (dil - 1), seed=dil))
    a(Case("ppon_dilated_8_tiny", 2, 24, 9, 9, 24, dil=8, act=1))
    a(Case("ppon_oscale_res", 1, 64, 15, 45, 64, oscale=0.2, res=True))
    a(Case("ppon_up_nearest", 1, 64, 10, 12, 64, up=True, act=1))
    # PAN: conv_first (3 -> 40), trunk conv (40 -> 40), FGH 1 x 1 rows of 64 floats, the pixel-attention gate, 20 / 24-channel tensors
    a(Case("pan_conv_first", 1, 3, 27, 48, 40))
    a(Case("pan_trunk_res", 2, 40, 27, 48, 40, res=True))
    a(Case("pan_fgh_rows", 2, 40, 7, 12, 50, kind="rows", k=1, pad=0))
    a(Case("pan_pa_gate", 1, 20, 16, 24, 20, k=1, pad=0, mul=True, act=1))
    a(Case("pan_pa_gate_3x3", 2, 24, 12, 20, 24, mul=True))
    a(Case("pan_upconv_24", 1, 40, 14, 18, 24, up=True, act=1))
    # channel counts around the chunks (C % 4 != 0, partial last chunk), K around the 16-channel tiles, every epilogue activation
    for i, (N, Cc, H, W, K, act) in enumerate([(1, 1, 9, 11, 16, 4), (2, 20, 13, 20, 12, 3), (3, 24, 17, 29, 20, 1), (1, 40, 21, 38, 48, 2),
                                               (2, 96, 25, 47, 24, 0), (2, 512, 9, 20, 64, 1)]):
        a(Case(f"chan_C{Cc}_K{K}", N, Cc, H, W, K, act=act, seed=100 + i))
    # every (NKT, NPT) instantiation of the tiled kernel: NKT follows the real batch (f32ops.hip, f32conv_plan), so large batches of small grids
    for i, (N, H, W, K) in enumerate([(200, 1, 1, 36), (260, 1, 1, 36), (260, 1, 1, 64), (200, 5, 12, 36), (260, 5, 12, 36), (260, 5, 12, 64)]):
        a(Case(f"inst_{N}x{H}x{W}_K{K}", N, 3, H, W, K, pad_mode=2 * (i % 2), act=i % 5, seed=150 + i))
    # grids: 1 x 1 .. 70 x 130, ragged tile rows / columns, batches that fill multi-image tiles raggedly
    for i, (N, H, W) in enumerate([(65, 1, 1), (33, 2, 3), (17, 4, 4), (9, 8, 8), (5, 3, 17), (3, 70, 130), (1, 1, 130), (1, 70, 1), (2, 33, 65)]):
        a(Case(f"grid_{N}x{H}x{W}", N, 20 if H * W > 1000 else 64, H, W, 16 if H * W > 1000 else 48, pad_mode=i % 3 if min(H, W) > 1 else 2, seed=200 + i))
    return c


def random_cases(n, seed=20261016):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        Cc = int(rng.choice([1, 3, 20, 24, 40, 64, 96, 512]))
        K = int(rng.choice([3, 12, 16, 20, 24, 48, 64, 256]))
        kind = str(rng.choice(["conv"] * 6 + ["convT4", "convT1", "rows"]))
        k = int(rng.choice([1, 3, 3, 4, 7])) if kind == "conv" else (int(rng.choice([3, 4])) if kind != "rows" else 1)
        stride = 2 if kind == "conv" and k in (3, 4) and rng.rand() < 0.3 else 1
        if k == 4:
            stride = 2
        if kind == "convT1":
            K = int(rng.choice([1, 3, 4]))
        if kind == "rows":
            K = min(K, 64)
        N = int(rng.choice([1, 1, 2, 3, 5, 9]))
        big = Cc * K >= 512 * 64
        H, W = int(rng.randint(1, 12 if big else 40)), int(rng.randint(1, 16 if big else 70))
        if stride == 2:
            H, W = 2 * max(H // 2, 1), 2 * max(W // 2, 1)
        pad_mode = int(rng.choice([0, 1, 2])) if kind == "conv" and stride == 1 else 0
        dil = int(rng.choice([1, 1, 2, 4])) if kind == "conv" and k == 3 and stride == 1 and pad_mode == 0 else 1
        up = kind == "conv" and stride == 1 and dil == 1 and rng.rand() < 0.2
        if pad_mode == 1:                                      # reflection needs pad < size
            H, W = max(H, k // 2 + 1), max(W, k // 2 + 1)
        tf = kind == "conv" and stride == 2 and k == 3 and rng.rand() < 0.5
        coff = int(rng.choice([0, 0, 4, 7]))
        koff = int(rng.choice([0, 0, 3, 16])) if kind in ("conv", "convT4") else 0
        c = Case(f"rand_{i}", N, Cc, H, W, K, kind=kind, k=k, stride=stride, dil=dil, tf=tf, pad_mode=pad_mode, up=bool(up),
                 in_act=int(rng.choice([0, 1, 2])), act=int(rng.choice([0, 1, 2, 3, 4])), oscale=float(rng.choice([0.0, 0.0, 0.2])),
                 res=bool(rng.rand() < 0.3), mul=bool(rng.rand() < 0.15), ctot=Cc + coff + int(rng.choice([0, 5])), coff=coff,
                  ktot=(K + koff + int(rng.choice([0, 4]))) if koff or kind in ("conv", "convT4") else 0, koff=koff, seed=300 + i)
        out.append(c)
    return out


def sweep():
    return named_cases() + random_cases(24)
