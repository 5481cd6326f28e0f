"""CPU side of the pass-kernel tests of the UNet / ResNet engines (tests/test_gpu_pass_kernels.py holds the kernels to these on the GPU): every reference of
tests/_pass_kernels_ref.py against the torch module it restates, in float64; the refusals of the entry points of ABI 123, called with pointers nothing may
dereference; planted faults that the comparators must catch; and the float32 emulation's e_emul of unet_deep_post, the figure the GPU bound is a multiple of.

e_emul (train mode; worst over HW, C, ks and N of an instantiation) -- printed by test_deep_post_emulation:
    <NPX, PL>    kind a      kind c
    <1, 1>       5.9e-08     5.9e-08
    <1, 4>       5.2e-07     2.1e-07
    <1, 16>      7.3e-07     2.8e-07
    <2, 32>      7.8e-07     3.8e-07
    <8, 32>      7.9e-07     4.8e-07
(<1, 1>: one pixel -- the mean is the value itself, the variance 0, and y = x alpha + (beta - x alpha) cancels exactly in the emulation; the working bound there is
4.7e-07, about 8 float32 roundings of |x alpha|.)

The split-K loop of unet_deep_post takes segment 0, then blocks of eight (z = 1 .. 8, 9 .. 16), then a tail loop: ks = 9 and 17 end on a whole block and have no
tail; ks = 2, 8 and 16 do (1, 7 and 7 segments).  "The tail dropped" is therefore planted at every ks of the list and must be caught where a tail exists.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _pass_kernels_ref as R
import innfer_amd.lib as L

FAKE = 0x1000


# ------------------------------------------------------------------------------------------------ the references restate the modules
def test_norm_reference_is_batchnorm_train_and_instancenorm():
    rng = np.random.default_rng(1)
    x = rng.normal(2.0, 3.0, (3, 5, 4, 7))
    g, b = rng.uniform(0.5, 1.5, 5), rng.uniform(-1, 1, 5)
    a, s = R.bn_alpha_shift(x.reshape(3, 5, -1), g, b)
    y = x * a[..., None, None] + s[..., None, None]
    bn = nn.BatchNorm2d(5).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(g)); bn.bias.copy_(torch.from_numpy(b))
        for n in range(3):              # a batch is N independent batch-1 forwards: the statistics of the CURRENT image
            assert np.abs(bn(torch.from_numpy(x[n:n + 1])).numpy() - y[n:n + 1]).max() < 1e-12
    a, s = R.bn_alpha_shift(x.reshape(3, 5, -1))
    with torch.no_grad():
        assert np.abs(nn.InstanceNorm2d(5).double()(torch.from_numpy(x)).numpy() - (x * a[..., None, None] + s[..., None, None])).max() < 1e-12
    v = rng.normal(0, 1, 100)
    assert np.array_equal(R.act(v, 1), F.leaky_relu(torch.from_numpy(v), 0.2).numpy()) and np.array_equal(R.act(v, 2), np.maximum(v, 0))


def test_ulp16():
    for v, u in ((0.0, 2.0 ** -24), (2.0 ** -15, 2.0 ** -24), (2.0 ** -14, 2.0 ** -24), (1.0, 2.0 ** -10), (1.999, 2.0 ** -10), (2.0, 2.0 ** -9), (-1000.0, 0.5)):
        assert R.ulp16(np.array(v)) == u, v
    h = torch.tensor([1.0, 0.3, 1000.0]).half()
    nxt = (h.view(torch.int16) + 1).view(torch.float16)
    assert np.array_equal(R.ulp16(h.double().numpy()), (nxt.double() - h.double()).numpy())


@pytest.mark.parametrize("Cc", (1, 3, 4))
def test_unet_patch_is_conv_4_2_1(Cc):
    g = torch.Generator().manual_seed(Cc)
    for N, H, W in ((1, 2, 2), (2, 6, 10), (1, 32, 34)):
        x = torch.randn(N, Cc, H, W, generator=g, dtype=torch.float64)
        conv = nn.Conv2d(Cc, 64, 4, 2, 1).double()
        with torch.no_grad():
            got = F.conv2d(R.unet_patch(x), R.unet_patch_weight(conv.weight)[:, :, None, None], conv.bias)
            assert (got - conv(x)).abs().max() < 1e-12


@pytest.mark.parametrize("Cc", (1, 3, 4))
def test_row_patch_is_reflectionpad3_conv7(Cc):
    g = torch.Generator().manual_seed(10 + Cc)
    for N, H, W in ((1, 4, 4), (2, 5, 7), (1, 9, 33)):
        x = torch.randn(N, Cc, H, W, generator=g, dtype=torch.float64)
        net = nn.Sequential(nn.ReflectionPad2d(3), nn.Conv2d(Cc, 8, 7)).double()
        wcol = torch.zeros(8, 32, 7, 1, dtype=torch.float64)                        # [co][kx * C + c][ky]
        with torch.no_grad():
            wcol[:, :7 * Cc, :, 0] = net[1].weight.permute(0, 3, 1, 2).reshape(8, 7 * Cc, 7)
            got = F.conv2d(F.pad(R.row_patch(x), (0, 0, 3, 3), mode="reflect"), wcol, net[1].bias)
            assert (got - net(x)).abs().max() < 1e-12


def test_pad_reference_is_reflectionpad3_plus_a_zero_ring():
    for H, W in ((4, 4), (4, 9), (5, 5), (7, 4), (8, 8), (16, 21)):
        v = torch.arange(2 * 3 * H * W, dtype=torch.float64).view(2, 3, H, W) + 1
        want = F.pad(nn.ReflectionPad2d(3)(v), (1, 1, 1, 1))
        assert np.array_equal(R.pad_ref(v.numpy()), want.numpy())
        assert np.array_equal(R.reflect_index(H), nn.ReflectionPad2d((0, 0, 3, 3))(torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)).view(-1).numpy())


@pytest.mark.parametrize("K", (1, 3))
def test_sum9_is_reflectionpad3_conv7(K):
    g = torch.Generator().manual_seed(20 + K)
    for N, H, W in ((1, 4, 4), (2, 5, 9), (1, 16, 21)):
        x = torch.randn(N, 6, H, W, generator=g, dtype=torch.float64)
        net = nn.Sequential(nn.ReflectionPad2d(3), nn.Conv2d(6, K, 7), nn.Tanh()).double()
        with torch.no_grad():
            P = torch.from_numpy(R.pad_ref(x.numpy()))
            Q = F.conv2d(P, R.sum9_weights(net[1].weight), None, padding=1)
            got = np.tanh(R.sum9_ref(Q.numpy(), net[1].bias.numpy(), K, H, W))
            assert np.abs(got - net(x).numpy()).max() < 1e-12


def test_first_conv_data():
    x32, x, w, b, ref, e32 = R.first_data(2, 6, 64, 3, True)
    assert torch.equal(x, x32.half().float()) and not torch.equal(x, x32) and torch.equal(w, w.half().float())
    assert ref.shape == (2, 64, 3, 32) and 0 < e32 < 1e-5
    conv = nn.Conv2d(3, 64, 4, 2, 1).double()
    with torch.no_grad():
        conv.weight.copy_(w); conv.bias.copy_(b)
        assert torch.equal(conv(x.double()), ref)


# ------------------------------------------------------------------------------------------------ refusals: nothing may launch (the pointers are never dereferenced)
def _dst(p=FAKE, gs=1 << 20, coff=0, a=1):
    return [p, gs, coff, a]


def _refused(rc, *codes):
    assert rc in (codes or (L.ERR_INVALID, L.ERR_UNSUPPORTED)), rc
    assert L.last_error()
    return True


def test_unet_entry_points_refuse():
    assert L.ABI_VERSION == 124 == L.lib.innfer_version()
    f, no = FAKE, [None, 0, 0, 0]
    lib = L.lib
    # innfer_unet_pre
    assert _refused(lib.innfer_unet_pre(None, 0, 3, 4, 4, 1, f, 1 << 20, 0, None), L.ERR_INVALID)
    assert _refused(lib.innfer_unet_pre(f, 0, 3, 4, 4, 1, None, 1 << 20, 0, None), L.ERR_INVALID)
    assert _refused(lib.innfer_unet_pre(f, 2, 3, 4, 4, 1, f, 1 << 20, 0, None), L.ERR_INVALID)                     # uint8 input
    assert _refused(lib.innfer_unet_pre(f, 0, 33, 4, 4, 1, f, 1 << 20, 0, None), L.ERR_UNSUPPORTED)                # more than one group
    assert _refused(lib.innfer_unet_pre(f, 0, 5, 4, 4, 1, f, 1 << 20, 1, None), L.ERR_UNSUPPORTED)                 # 16 C > 64
    assert _refused(lib.innfer_unet_pre(f, 0, 3, 5, 4, 1, f, 1 << 20, 1, None), L.ERR_INVALID)                     # odd H
    assert _refused(lib.innfer_unet_pre(f, 0, 3, 4, 4, 2, f, 2 * 2 * 2 * 32 - 1, 1, None), L.ERR_INVALID)          # group stride
    assert _refused(lib.innfer_unet_pre(f, 0, 3, 4, 4, 2, f, 2 * 16 * 32 - 1, 0, None), L.ERR_INVALID)
    # innfer_unet_post / _post_slab
    for fn, head in ((lib.innfer_unet_post, lambda C=32, cpad=64, HW=10, N=2, al=f, sh=f, ns=0, raw=f: [raw, cpad, C, HW, N, al, sh, ns]),
                     (lib.innfer_unet_post_slab, lambda C=32, cpad=64, HW=10, N=2, al=f, sh=f, ns=0, raw=f, gs=1 << 20: [raw, gs, C, HW, N, al, sh, ns])):
        assert _refused(fn(*head(raw=None), *_dst(), *no, None), L.ERR_INVALID)
        assert _refused(fn(*head(), *no, *no, None), L.ERR_INVALID)                                                   # no first destination
        assert _refused(fn(*head(C=36), *_dst(), *no, None), L.ERR_INVALID)                                           # C % 8
        assert _refused(fn(*head(), *_dst(coff=4), *no, None), L.ERR_INVALID)                                         # offset % 8
        assert _refused(fn(*head(), *_dst(), *_dst(coff=12), None), L.ERR_INVALID)
        assert _refused(fn(*head(), *_dst(gs=2 * 10 * 32 - 1), *no, None), L.ERR_INVALID)                             # group stride
        assert _refused(fn(*head(), *_dst(), *_dst(gs=2 * 10 * 32 - 1), None), L.ERR_INVALID)
        assert _refused(fn(*head(), *_dst(a=0), *no, None), L.ERR_INVALID) and _refused(fn(*head(), *_dst(), *_dst(a=3), None), L.ERR_INVALID)
        assert _refused(fn(*head(ns=16), *_dst(), *no, None), L.ERR_INVALID)                                          # nstride neither 0 nor C
        assert _refused(fn(*head(al=f, sh=None), *_dst(), *no, None), L.ERR_INVALID)
    assert _refused(lib.innfer_unet_post(f, 24, 32, 10, 2, f, f, 0, *_dst(), *no, None), L.ERR_INVALID)            # cpad < C
    assert _refused(lib.innfer_unet_post(f, 66, 32, 10, 2, f, f, 0, *_dst(), *no, None), L.ERR_INVALID)            # cpad % 4
    assert _refused(lib.innfer_unet_post_slab(f, 2 * 10 * 32 - 1, 32, 10, 2, f, f, 0, *_dst(), *no, None), L.ERR_INVALID)
    assert _refused(lib.innfer_unet_post_slab(f, 1 << 20, 32, 10, 2, None, None, 0, *_dst(), *no, None), L.ERR_INVALID)       # the slab form always normalises
    # innfer_unet_deep_post
    def deep(part=f, se=1 << 20, ks=2, cpad=64, C=40, HW=16, N=2, g=f, b=f, ea=None, es=None, d0=None, d1=None):
        return lib.innfer_unet_deep_post(part, se, ks, cpad, C, HW, N, g, b, ea, es, *(d0 or _dst()), *(d1 or no), None)
    assert _refused(deep(HW=257), L.ERR_UNSUPPORTED)
    assert _refused(deep(part=None), L.ERR_INVALID) and _refused(deep(d0=no), L.ERR_INVALID)
    assert _refused(deep(ks=0), L.ERR_INVALID) and _refused(deep(cpad=32), L.ERR_INVALID)
    assert _refused(deep(se=2 * 16 * 64 - 1), L.ERR_INVALID)                                                        # segment stride
    assert _refused(deep(b=None), L.ERR_INVALID) and _refused(deep(g=None, b=None, ea=f), L.ERR_INVALID) and _refused(deep(ea=f, es=f), L.ERR_INVALID)
    assert _refused(deep(d0=_dst(coff=4)), L.ERR_INVALID) and _refused(deep(d1=_dst(coff=20)), L.ERR_INVALID)
    assert _refused(deep(d0=_dst(gs=2 * 16 * 32 - 1)), L.ERR_INVALID) and _refused(deep(d1=_dst(gs=2 * 16 * 32 - 1)), L.ERR_INVALID)
    assert _refused(deep(d0=_dst(a=0)), L.ERR_INVALID)
    # innfer_unet_final
    assert _refused(lib.innfer_unet_final(None, 4, 3, 16, 1, f, f, 0, None), L.ERR_INVALID)
    assert _refused(lib.innfer_unet_final(f, 4, 3, 16, 1, None, f, 0, None), L.ERR_INVALID)
    assert _refused(lib.innfer_unet_final(f, 4, 3, 16, 1, f, None, 0, None), L.ERR_INVALID)
    assert _refused(lib.innfer_unet_final(f, 2, 3, 16, 1, f, f, 0, None), L.ERR_INVALID)                           # row shorter than C
    assert _refused(lib.innfer_unet_final(f, 4, 3, 16, 1, f, f, 2, None), L.ERR_INVALID)
    # the first conv and its packer
    assert lib.innfer_unet_first_packed_bytes() == 8192
    w = np.zeros((64, 5, 4, 4), np.float32)
    out = np.full(8192 + 64, 0xAB, np.uint8)
    assert _refused(lib.innfer_pack_unet_first(w.ctypes.data, 5, out.ctypes.data), L.ERR_UNSUPPORTED) and (out == 0xAB).all()
    assert _refused(lib.innfer_pack_unet_first(None, 3, out.ctypes.data), L.ERR_INVALID)
    assert _refused(lib.innfer_pack_unet_first(w.ctypes.data, 3, None), L.ERR_INVALID)
    def first(i=f, dt=0, C=3, H=32, W=32, N=1, pk=f, d0=f, gs=1 << 40):
        return lib.innfer_unet_first_conv(i, dt, C, H, W, N, pk, None, d0, None, gs, None)
    assert _refused(first(i=None), L.ERR_INVALID) and _refused(first(pk=None), L.ERR_INVALID) and _refused(first(d0=None), L.ERR_INVALID)
    assert _refused(first(dt=2), L.ERR_INVALID) and _refused(first(H=33), L.ERR_INVALID) and _refused(first(W=31), L.ERR_INVALID)
    assert _refused(first(C=5), L.ERR_UNSUPPORTED)                                                                  # 16 C > 64
    assert _refused(first(W=16), L.ERR_UNSUPPORTED) and "16" in L.last_error()                                      # wo % 16: the launcher says it
    assert _refused(first(W=48), L.ERR_UNSUPPORTED)
    assert _refused(first(gs=16 * 16 * 32 - 1), L.ERR_INVALID)
    assert _refused(first(C=4, H=32768, W=32768), L.ERR_UNSUPPORTED)                                                # 2^32 elements: offsets are 32-bit


def test_unet_first_packer_places_every_weight_once():
    """The panel the engine and the test share: every w[co][c][tap] lands in exactly one slot, the slots of the channels beyond C hold zero"""
    for Cc in (1, 3, 4):
        w = (np.arange(64 * Cc * 16, dtype=np.float32) % 2039 + 1).reshape(64, Cc, 4, 4)         # fp16-exact, non-zero
        out = np.zeros(4096, np.float16)
        L.check(L.lib.innfer_pack_unet_first(w.ctypes.data, Cc, out.ctypes.data))
        p = out.astype(np.float32).reshape(2, 4, 16, 32)                                            # [k-step][tile][row][k in step]
        for t in range(4):
            for rho in range(16):
                co = 32 * (t >> 1) + 8 * (rho >> 2) + 4 * (t & 1) + (rho & 3)
                k = np.concatenate([p[0, t, rho], p[1, t, rho]])                                    # k = c * 16 + ky * 4 + kx
                assert np.array_equal(k[:16 * Cc], w[co].reshape(-1)) and (k[16 * Cc:] == 0).all(), (Cc, t, rho)


def test_resnet_entry_points_refuse():
    f, lib = FAKE, L.lib
    assert _refused(lib.innfer_resnet_pre(None, 0, 3, 8, 8, 1, f, 1, None), L.ERR_INVALID)
    assert _refused(lib.innfer_resnet_pre(f, 0, 3, 8, 8, 1, None, 1, None), L.ERR_INVALID)
    assert _refused(lib.innfer_resnet_pre(f, 2, 3, 8, 8, 1, f, 1, None), L.ERR_INVALID)
    assert _refused(lib.innfer_resnet_pre(f, 0, 5, 8, 8, 1, f, 1, None), L.ERR_UNSUPPORTED)                        # 7 C > 32
    assert _refused(lib.innfer_resnet_pre(f, 0, 33, 8, 8, 1, f, 0, None), L.ERR_UNSUPPORTED)
    assert _refused(lib.innfer_resnet_pre(f, 0, 3, 3, 8, 1, f, 1, None), L.ERR_INVALID)                            # ReflectionPad2d(3) needs 4
    assert _refused(lib.innfer_resnet_pre(f, 0, 3, 8, 3, 1, f, 1, None), L.ERR_INVALID)
    for fn, head in ((lib.innfer_resnet_post, lambda src=f, C=32: [src, 64, C, 10, 2]), (lib.innfer_resnet_post_slab, lambda src=f, C=32: [src, C, 10, 2])):
        assert _refused(fn(*head(src=None), f, f, 1, None, f, 1 << 20, None), L.ERR_INVALID)
        assert _refused(fn(*head(), None, f, 1, None, f, 1 << 20, None), L.ERR_INVALID)
        assert _refused(fn(*head(), f, None, 1, None, f, 1 << 20, None), L.ERR_INVALID)
        assert _refused(fn(*head(), f, f, 1, None, None, 1 << 20, None), L.ERR_INVALID)
        assert _refused(fn(*head(C=36), f, f, 1, None, f, 1 << 20, None), L.ERR_INVALID)                            # C % 8
        assert _refused(fn(*head(), f, f, 1, None, f, 2 * 10 * 32 - 1, None), L.ERR_INVALID)                        # group stride
    assert _refused(lib.innfer_resnet_post(f, 24, 32, 10, 2, f, f, 1, None, f, 1 << 20, None), L.ERR_INVALID)      # cpad < C
    def pad(src=f, sg=1 << 20, C=64, H=8, W=8, N=2, al=f, sh=f, dst=f, dg=1 << 20):
        return lib.innfer_resnet_post_slab_pad(src, sg, C, H, W, N, al, sh, 1, dst, dg, None)
    assert _refused(pad(src=None), L.ERR_INVALID) and _refused(pad(al=None), L.ERR_INVALID) and _refused(pad(sh=None), L.ERR_INVALID) and _refused(pad(dst=None), L.ERR_INVALID)
    assert _refused(pad(C=40), L.ERR_INVALID)                                                                       # C % 32: the zero ring walks whole groups
    assert _refused(pad(H=3), L.ERR_INVALID) and _refused(pad(W=3), L.ERR_INVALID)
    assert _refused(pad(sg=2 * 64 * 32 - 1), L.ERR_INVALID) and _refused(pad(dg=2 * 256 * 32 - 1), L.ERR_INVALID)
    assert _refused(lib.innfer_resnet_sum9_tanh(None, f, f, 0, 3, 8, 8, 1, None), L.ERR_INVALID)
    assert _refused(lib.innfer_resnet_sum9_tanh(f, None, f, 0, 3, 8, 8, 1, None), L.ERR_INVALID)
    assert _refused(lib.innfer_resnet_sum9_tanh(f, f, None, 0, 3, 8, 8, 1, None), L.ERR_INVALID)
    assert _refused(lib.innfer_resnet_sum9_tanh(f, f, f, 2, 3, 8, 8, 1, None), L.ERR_INVALID)
    assert _refused(lib.innfer_resnet_sum9_tanh(f, f, f, 0, 0, 8, 8, 1, None), L.ERR_INVALID)
    assert _refused(lib.innfer_resnet_final(None, 4, 3, 16, 1, f, f, 0, None), L.ERR_INVALID)
    assert _refused(lib.innfer_resnet_final(f, 4, 3, 16, 1, None, f, 0, None), L.ERR_INVALID)
    assert _refused(lib.innfer_resnet_final(f, 4, 3, 16, 1, f, None, 0, None), L.ERR_INVALID)
    assert _refused(lib.innfer_resnet_final(f, 2, 3, 16, 1, f, f, 0, None), L.ERR_INVALID)


# ------------------------------------------------------------------------------------------------ the comparators have teeth
def _h(a):
    """what a faithful fp16 store of a float64 array holds, as float64"""
    return torch.from_numpy(np.asarray(a, np.float64)).half().double().numpy()


def _pad_case(H, W, Cc=32, N=2, seed=0):
    """A normalised, ReLU'd fp16 image v and the padded slab a faithful kernel writes"""
    rng = np.random.default_rng(seed + 100 * H + W)
    v = _h(np.maximum(rng.normal(0.3, 1.0, (N, Cc, H, W)), 0.0) + 2.0 ** -10)          # strictly positive: a zero ring is distinguishable from every pixel
    return v, R.pad_ref(v)


def test_planted_faults_fail_the_comparators():
    """Each fault is planted into the reference's output or is a deliberately wrong restatement; the comparator the GPU test uses must reject it at at least one
    of the GPU test's shapes (and accept the faithful output at all of them)."""
    caught = {}
    pad_shapes = ((4, 4), (4, 9), (5, 5), (7, 4), (8, 8), (16, 21))

    def placement_ok(got, v):
        return np.array_equal(got, R.pad_ref(v))
    for name, fault in (("a mirror target off by one row", lambda v: R.pad_ref(v, row_off=1)),
                        ("the two mirror ranges not both applied when H = 4", lambda v: R.pad_ref(v, both=False)),
                        ("the outer ring left non-zero", lambda v: R.pad_ref(v, ring=1234.0))):
        hit = []
        for H, W in pad_shapes:
            v, good = _pad_case(H, W)
            assert placement_ok(good, v)
            if not placement_ok(fault(v), v):
                hit.append((H, W))
        caught[name] = hit
    assert (4, 4) in caught["the two mirror ranges not both applied when H = 4"] and (8, 8) not in caught["the two mirror ranges not both applied when H = 4"]

    # the second view given the first view's activation; per-image alpha read with nstride = 0
    rng = np.random.default_rng(3)
    N, Cc, HW = 3, 32, 257
    x = _h(rng.normal(0, 1, (N, Cc, HW)))
    al, sh = rng.uniform(0.5, 2, (N, Cc, 1)).astype(np.float32).astype(np.float64), rng.uniform(-1, 1, (N, Cc, 1)).astype(np.float32).astype(np.float64)
    for acts in ((1, 2), (2, 1)):
        ref1, mag = R.pass_ref(x, al, sh, acts[1])
        assert R.passes(_h(ref1), ref1, R.pass_bound(ref1, _h(ref1), mag))
        wrong = _h(R.pass_ref(x, al, sh, acts[0])[0])
        if not R.passes(wrong, ref1, R.pass_bound(ref1, wrong, mag)):
            caught.setdefault("the second view given the first view's activation", []).append(acts)
    ref, mag = R.pass_ref(x, al, sh, 2)
    wrong = _h(R.pass_ref(x, al[:1], sh[:1], 2)[0])                  # every image normalised with image 0's vectors
    caught["per-image alpha read with nstride = 0"] = [] if R.passes(wrong, ref, R.pass_bound(ref, wrong, mag)) else [(N, Cc, HW)]
    assert R.passes(wrong[:1], ref[:1], R.pass_bound(ref[:1], wrong[:1], mag[:1]))          # (N = 1 cannot see it: the batch of 3 is what catches it)

    # split-K faults of unet_deep_post: train mode (the y metric under 8 x e_emul) and eval mode (the derived bound)
    for name, kw, kss in (("one split-K segment dropped", dict(drop_segment=1), (2, 8, 9, 16, 17)), ("the split-K tail dropped", dict(drop_tail=True), R.DEEP_KS),
                          ("the split-K blocks of eight dropped (ks = 9)", dict(drop_blocks=True), R.DEEP_KS)):
        hit = []
        for ks in kss:
            for kind in "ac":
                HW, Cc, N = 17, 40, 3
                p, x64 = R.deep_data(N, Cc, HW, ks, kind)
                g, b, _, _ = R.deep_params(Cc, "train")
                a64, s64 = R.bn_alpha_shift(x64, g, b)
                bound = R.deep_bound(R.deep_inst(HW), kind)

                def stored(**f):
                    x32, a32, s32 = R.emulate_deep_post(p, HW, g, b, **f)
                    y = (x32 * a32[..., None]).astype(np.float32) + s32[..., None]
                    return _h(np.maximum(y, np.float32(0.2) * y))
                assert R.y_excess(stored(), x64, a64, s64, 1) <= bound, (name, ks, kind)
                if R.y_excess(stored(**kw), x64, a64, s64, 1) > bound:
                    hit.append(("train", ks, kind))
                _, _, ea, es = R.deep_params(Cc, "eval")
                ref, mag = R.pass_ref(x64, ea[None, :, None].astype(np.float64), es[None, :, None].astype(np.float64), 2)
                extra = (ks - 1) * 2.0 ** -24 * np.abs(ea)[None, :, None] * np.abs(p.astype(np.float64)).sum(0).transpose(0, 2, 1)
                xw = R.emulate_deep_post(p, HW, g, b, **kw)[0].astype(np.float64)
                wrong = _h(R.pass_ref(xw, ea[None, :, None].astype(np.float64), es[None, :, None].astype(np.float64), 2)[0])
                x32 = R.emulate_deep_post(p, HW, g, b)[0].astype(np.float64)
                good = _h(R.pass_ref(x32, ea[None, :, None].astype(np.float64), es[None, :, None].astype(np.float64), 2)[0])
                assert R.passes(good, ref, R.pass_bound(ref, good, mag, extra)), (name, ks, kind)
                if not R.passes(wrong, ref, R.pass_bound(ref, wrong, mag, extra)):
                    hit.append(("eval", ks, kind))
        caught[name] = hit
        assert any(h[0] == "train" for h in hit) and any(h[0] == "eval" for h in hit), (name, hit)
        if "tail" in name:
            assert {h[1] for h in hit} == {2, 8, 16}, hit                     # ks = 9, 17 end on a whole block of eight: no tail to drop
        if "blocks" in name:
            assert {h[1] for h in hit} == {9, 16, 17}, hit                    # ks = 2, 8: the tail loop alone

    # wrong restatements of the gathers, compared bit for bit
    g = torch.Generator().manual_seed(5)
    hit = []
    for Cc in (1, 3, 4):
        for N, H, W in ((1, 2, 2), (2, 6, 10), (2, 32, 34)):
            x = torch.randn(N, Cc, H, W, generator=g).half()
            if not torch.equal(R.unet_patch(x.float(), "kx*4+ky").half(), R.unet_patch(x.float()).half()):
                hit.append((Cc, H, W))
    caught["patch-slab tap order transposed (kx*4+ky)"] = hit
    hit = []
    for Cc in (1, 3, 4):
        for N, H, W in ((1, 4, 4), (2, 5, 7), (2, 9, 33)):
            x = torch.randn(N, Cc, H, W, generator=g).half().float()
            wrong = torch.zeros(N, 32, H, W)
            for kx in range(7):              # X >= W -> 2 W - X instead of 2 W - 2 - X (clamped into the row here; the kernel would read beyond it)
                X = torch.arange(W) + kx - 3
                X = torch.where(X < 0, -X, torch.where(X >= W, 2 * W - X, X)).clamp(max=W - 1)
                wrong[:, kx * Cc:(kx + 1) * Cc] = x[:, :, :, X]
            if not torch.equal(wrong.half(), R.row_patch(x).half()):
                hit.append((Cc, H, W))
    caught["row-patch reflection without the -2"] = hit

    # a sub-block of the sum-9 gather displaced by 2 instead of 3
    hit = []
    rng = np.random.default_rng(9)
    for K in (1, 3):
        for N, H, W in ((1, 4, 4), (2, 5, 9), (2, 16, 21)):
            Q = rng.normal(0, 0.3, (N, 9 * K, H + 8, W + 8)).astype(np.float32)
            bias = rng.normal(0, 0.3, K).astype(np.float32)
            pre = R.sum9_ref(Q.astype(np.float64), bias, K, H, W)
            ref = np.tanh(pre)
            f32 = np.broadcast_to(bias[None, :, None, None], pre.shape).astype(np.float32).copy()
            for j in range(9):
                f32 = f32 + Q[:, j::9][:, :K, 3 * (j // 3) + 1:3 * (j // 3) + 1 + H, 3 * (j % 3) + 1:3 * (j % 3) + 1 + W]
            e32 = np.abs(np.tanh(f32).astype(np.float64) - ref).max()
            bound = 8 * e32 + R.TANH_HW
            assert R.passes(np.tanh(f32), ref, bound)
            if not R.passes(np.tanh(R.sum9_ref(Q.astype(np.float64), bias, K, H, W, disp=2)).astype(np.float32), ref, bound):
                hit.append((K, H, W))
    caught["a sub-block of the sum-9 gather displaced by 2 instead of 3"] = hit

    for name, hit in caught.items():
        print("CAUGHT %-62s at %s" % (name, hit))
    assert len(caught) == 11 and all(caught.values()), {k: v for k, v in caught.items() if not v}


def test_deep_post_emulation():
    """e_emul per (instantiation, kind) in train mode, printed (module docstring, docs/KERNELS.md); 8 x every one of them stays below the ceiling, and the
    emulation's statistics are the float64 ones to float32 accuracy."""
    insts = sorted({R.deep_inst(HW) for HW in R.DEEP_HW})
    assert insts == [(1, 1), (1, 4), (1, 16), (2, 32), (8, 32)]
    for inst in insts:
        ends = {(1, 1): (1, 1), (1, 4): (2, 4), (1, 16): (5, 16), (2, 32): (17, 64), (8, 32): (65, 256)}[inst]              # both ends of its range
        assert set(ends) <= {HW for HW in R.DEEP_HW if R.deep_inst(HW) == inst}
        for kind in "ac":
            e = R.deep_e_emul(inst, kind)
            print("E_EMUL unet_deep_post<%d, %d> train kind %s: %.2e (bound %.2e)" % (inst + (kind, e, R.deep_bound(inst, kind))))
            assert 0 < e and R.MARGIN * e <= R.CEILING
    # the modes without statistics (held to the derived bound on the GPU, not to these): the float32 segment sum and transform against float64, same metric
    for inst in insts:
        for mode in ("eval", "bias", "none"):
            worst = 0.0
            for HW in (h for h in R.DEEP_HW if R.deep_inst(h) == inst):
                for ks in R.DEEP_KS:
                    p, x64 = R.deep_data(3, 40, HW, ks, "c")
                    _, _, ea, es = R.deep_params(40, mode)
                    ea, es = (np.ones(40, np.float32), np.zeros(40, np.float32)) if ea is None else (ea, es)
                    x32 = R.emulate_deep_post(p, HW, ea, es)[0]
                    y32 = (x32 * ea[None, :, None]).astype(np.float32) + es[None, :, None]
                    xa = x64 * ea.astype(np.float64)[None, :, None]
                    y64 = xa + es.astype(np.float64)[None, :, None]
                    worst = max(worst, float((np.abs(y32 - y64) / np.maximum(1.0, np.maximum(np.abs(y64), np.abs(xa)))).max()))
            print("E_EMUL unet_deep_post<%d, %d> %s kind c: %.2e" % (inst + (mode, worst)))
            assert worst < 1e-5
    p, x64 = R.deep_data(3, 40, 65, 17, "c")
    g, b, _, _ = R.deep_params(40, "train")
    x32, al, sh = R.emulate_deep_post(p, 65, g, b)
    a64, s64 = R.bn_alpha_shift(x64, g, b)
    assert np.abs(x32 - x64).max() < 1e-5 and np.abs(al / a64 - 1).max() < 1e-5 and np.abs(sh - s64).max() < 1e-4
    ratio = np.abs(x64.mean(2)) / x64.std(2)
    assert 6.0 <= ratio.min() and ratio.max() <= 10.0
