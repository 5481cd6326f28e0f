"""CPU side of tests/test_gpu_conv_forms.py: the bound and the references hold for a kernel that is right, and fail for one that is subtly wrong.

A stand-in takes the place of the launch: fp16(the same operation in float32 on the CPU), in the kernel's output formats (slab with foreign groups, planar, uint8
image), with the roundings the kernel makes on purpose (the self gate's v = fp16(conv + bias)).  With it the GPU test functions run unchanged (the many-tile sizes
shrunk: the reference does not know about tiles):

  * fp16(float32 conv) against float64 reaches 0.96 .. 0.99 of the bound in every family, with and without tanh: the reference alone stays inside;
  * the uint8 image differs from the float64 codes on fewer than 1 % of the values for the seeds the GPU test uses (its cap);
  * planted faults -- two channels swapped, one product of the 7x7 dropped, v rounded twice in the self gate, a phase in the wrong quadrant -- fail.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
import test_gpu_conv_forms as T
from _conv_ref import Case


def _standin(fault=None):
    def run(dev, c, out="slab", act=0, res1=None, s1=1.0, res2=None, s2=1.0, out_groups=None, out_off=0, rows=None, plane_rows=0, gate=False, expect=0, **fields):
        if expect:
            return None
        w = R.up2x_phase_weights(R.data(c)[1]).half() if c.form == "upph" else None
        if fault == "centre tap" and c.form == "7x7":
            w = R.data(c)[1].half().clone()
            w[:, :, 3, 3] = 0
        y = R.conv(c, torch.float32, w)
        if gate:
            v = y.half().float()                                # the kernel's v
            if fault == "v twice":
                v = ((y * 3.0).half().float() * np.float32(1.0 / 3.0)).half().float()
            o, _ = R.self_gate(c, v, 0.0, act)
        else:
            o, _ = R.epilogue(y, act, fields.get("outm", 0), res1, s1, res2, s2)
        if c.form == "shuffle":
            o = F.pixel_shuffle(o, 2)
        if fault == "swap" and o.shape[1] > 4:
            o = o.clone()
            o[:, [3, 4]] = o[:, [4, 3]]
        if fault == "quadrant" and c.form == "phases":
            o = torch.roll(o, 1, 3)
        N, K, Ho, Wo = o.shape
        if out == "u8":
            return R.image_codes(o, fields.get("out_denorm", 0), fields.get("out_round16", 0))[0]
        o = o.half() if out != "f32" else o
        if rows:
            full = torch.full_like(o, T.FILL)
            full[:, :, rows[0]:rows[1]] = o[:, :, rows[0]:rows[1]]
            o = full
        if out == "slab":
            full = torch.full((N, (out_groups or max(K, 32) // 32) * 32, Ho, Wo), T.FILL, dtype=torch.float16)
            full[:, out_off:out_off + K] = o
            o = full
        return o
    return run


@pytest.fixture
def small(monkeypatch):
    monkeypatch.setattr(T, "MANY24", (1, 49, 65))
    monkeypatch.setattr(T, "MANY16", (1, 33, 65))
    R.MEASURED.clear()


def test_reference_alone_stays_inside_the_bound(small, monkeypatch):
    """Every family of the GPU test with fp16(float32 conv) standing in for the kernel: passes, and comes close to the bound (so the bound is not slack)."""
    monkeypatch.setattr(T, "_run", _standin())
    T.test_planar_3x3_k_le_16(None, 3)
    T.test_planar_3x3_k_le_16(None, 5)
    T.test_planar_3x3_reflection_padding(None, 16)
    T.test_planar_phase_scatter(None, 3)
    T.test_planar_7x7(None, 32, 3)
    T.test_conv1x1(None, 96, 32)
    T.test_conv1x1_running_sum_operand(None, 256)
    T.test_self_gate(None, 32, 0)
    T.test_self_gate(None, 64, 1)
    T.test_upconv_phases(None, 1, 17, 33)
    for i in range(len(T.SWEEP)):
        T.test_reachable_forms_within_fp16_rounding(None, i)
    worst = {f: m[1] for f, m in R.MEASURED.items()}
    assert all(v <= 1.0 for v in worst.values()), worst
    assert max(worst.values()) > 0.9, worst
    assert all(3e-8 < m[0] < 3e-6 for m in R.MEASURED.values()), R.MEASURED


@pytest.mark.parametrize("K", [1, 3, 4])
def test_uint8_stand_in_stays_under_the_cap(small, monkeypatch, K):
    """The seeds of test_planar_uint8_image: fp16(float32 conv) through tensor2np differs from the float64 codes on < 1 % of the values, each next to a boundary."""
    monkeypatch.setattr(T, "_run", _standin())
    T.test_planar_uint8_image(None, K)
    assert R.MEASURED["planar uint8 image"][1] <= 1.0


@pytest.mark.parametrize("fault,test,args", [
    ("swap", "test_planar_3x3_k_le_16", (5,)),
    ("swap", "test_planar_3x3_k_le_16", (16,)),
    ("centre tap", "test_planar_7x7", (64, 16)),
    ("v twice", "test_self_gate", (32, 0)),
    ("quadrant", "test_planar_phase_scatter", (3,)),
])
def test_planted_faults_fail(small, monkeypatch, fault, test, args):
    monkeypatch.setattr(T, "_run", _standin(fault))
    with pytest.raises(AssertionError, match="worst err / bound"):
        getattr(T, test)(None, *args)


def test_bound_helper_and_code_window():
    """ulp16 at the binade edges and below the normal range; one dropped product of 1728 fails."""
    v = torch.tensor([1.0, 1.999, 2.0, 0.05, 2.0 ** -14, 1e-7, 0.0, -0.75])
    assert torch.equal(R.ulp16(v), torch.tensor([2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -15, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -11], dtype=torch.float64))
    c = Case("3x3", 1, 192, 64, 9, 11, seed=7)
    y64, e32 = R.pre(c)
    x, w, b = R.data(c)
    R.assert_within_fp16_rounding(y64.half(), y64, e32)
    w2 = w.half().clone()
    w2[5, 100, 1, 1] = 0                                        # one product of 1728 gone in channel 5
    bad = R.conv(c, torch.float32, w2).half()
    with pytest.raises(AssertionError, match="worst err / bound"):
        R.assert_within_fp16_rounding(bad, y64, e32)
    with pytest.raises(AssertionError, match="away from a rounding boundary"):      # a swapped channel in the image
        c3 = Case("3x3", 1, 64, 3, 9, 11, seed=8, blo=0.0)
        y3, e3 = R.pre(c3)
        R.assert_image_codes(R.image_codes(y3.float(), 0, 1)[0][..., [1, 0, 2]].contiguous(), y3, e3, 0, 1)
