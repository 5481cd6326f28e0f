"""The references of one SCPA block (tests/_pan_scpa_ref.py) on the CPU: that the clean float32 model stays inside the bound the device is held to, and that the sweep
of tests/test_gpu_pan_scpa.py DISCRIMINATES -- each of twelve planted faults, switched on in the model, exceeds the fp16 forms' bound and the split form's bound by
more than 10x on some element, in every weight family and on some case of every kind the fault can act on.  No GPU and no library call.

Why this matters: through a whole PAN forward with synth.fill_state_dict weights none of these faults is visible (the block's branch is a small correction to x, the
gate is flat).  Max / mean change of the network output with the fault in EVERY block, oracle.pan_forward on the CPU:

    planted fault                                         nb 4, seed 41, 50 x 70     nb 16, seed 0, 50 x 70
    gate replaced by 0.5                                  1.7e-5 / 2.8e-6            4.3e-5 / 6.9e-6
    k2's bias dropped                                     1.8e-5 / 2.8e-6            3.6e-5 / 5.8e-6
    k1's taps transposed                                  5.7e-4 / 8.6e-5            1.3e-3 / 2.1e-4
    LeakyReLU after k1 -> ReLU                            1.6e-4 / 2.6e-5            3.3e-4 / 5.6e-5
    Y not zero outside the image                          4.4e-5 / 1.2e-6            7.3e-5 / 2.5e-6
    Y's halo column missing at every 32-pixel seam        1.4e-4 / 4.0e-6            2.4e-4 / 6.5e-6
    Y's halo row missing at every 8th row                 1.5e-4 / 1.5e-5            2.8e-4 / 3.0e-5
    channel 19 of b' dropped before conv3                 3.3e-5 / 5.2e-6            1.4e-4 / 2.9e-5
    a' and b' swapped in front of conv3                   1.4e-3 / 2.5e-4            2.5e-3 / 6.2e-4
    output channels 32..39 never updated                  3.6e-4 / 5.5e-5            1.3e-3 / 3.4e-4

against network bounds of 1e-2 / 1.5e-3 (fp16) and 1e-4 (fp32 mode).  test_report prints the margins docs/KERNELS.md 3.5c quotes.
"""
import numpy as np
import pytest
import torch

import _pan_scpa_ref as R

CASES = R.cases(R.CPU_SHAPES)
MARGINS = {}           # (fault, bound) -> {family: worst err / bound}


def test_sweep_is_what_the_issue_lists():
    cs = R.cases()
    assert len(cs) == 18 and len(set(cs)) == 18
    assert R.SHAPES == ((1, 4, 4), (1, 8, 32), (1, 9, 33), (2, 6, 40), (1, 16, 32), (1, 17, 33), (1, 50, 70), (3, 37, 45), (1, 273, 513))
    assert len(R.FAULTS) == 12
    for c in CASES:
        x = R.data(c)
        assert x.shape == (c.N, 40, c.H, c.W) and x.abs().max() <= 1.0 and torch.equal(x, x.half().float())
    for fam, kb, gate_span in (("flat", 0.2, (0.3, 0.7)), ("live", 2.0, (0.05, 0.95))):
        w, w16 = R.weights(fam), R.weights16(fam)
        assert 0.9 * kb < w["k2b"].abs().max() <= kb and torch.equal(w16["k2b"], w["k2b"])
        assert all(torch.equal(w16[k], w16[k].half().float()) for k in R.KEYS if k != "k2b")
        # the gate of the family on a real case: flat stays near 1/2, live spans its range
        c = R.Case(fam, 1, 17, 33)
        B = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(R.data(c).double(), w16["c1b"].double()), 0.2)
        s = torch.sigmoid(torch.nn.functional.conv2d(B, w16["k2"].double()) + w["k2b"].double().reshape(1, -1, 1, 1))
        if fam == "flat":
            assert gate_span[0] < s.min() and s.max() < gate_span[1]
        else:
            assert s.min() < gate_span[0] and s.max() > gate_span[1]


def test_layouts_round_trip():
    """The numpy slab / compact-plane / split-plane builders of the GPU test invert each other and place what include/innfer_amd.h says where it says."""
    c = R.Case("flat", 2, 3, 5)
    x = R.data(c)
    npx = 30
    for c8 in (False, True):
        s = R.to_slab(x, c8, fill=0.0, rest=7.0)
        assert s.shape == (npx * 64,)
        y, rest = R.from_slab(s, 2, 3, 5, c8)
        assert torch.equal(y.float(), x) and (rest == (7.0 if c8 else 0.0)).all() and rest.size == npx * 24
    p, q = 1 * 15 + 2 * 5 + 4, 37                          # pixel (n 1, y 2, x 4), channel 37
    assert R.to_slab(x)[npx * 32 + p * 32 + (q - 32)] == x[1, q, 2, 4] and R.to_slab(x, True)[npx * 32 + p * 8 + (q - 32)] == x[1, q, 2, 4]
    assert R.to_slab(x)[p * 32 + 5] == x[1, 5, 2, 4]
    x32 = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (2, 40, 3, 5)).astype(np.float32))
    pl = R.to_split_planes(x32)
    assert pl.shape == (npx * 80,) and (pl[npx * 40:] != 0).any()
    back = R.from_split_planes(pl, 2, 3, 5)
    assert ((back - x32.double()).abs() <= 2.0 ** -22 * x32.double().abs() + 2.0 ** -36).all()
    assert pl[npx * 32 + p * 8 + (q - 32)] == np.float16(x32[1, q, 2, 4].item())


@pytest.mark.parametrize("c", CASES, ids=str)
def test_clean_model_is_inside_the_bounds(c):
    """The float32 model with its output rounded to fp16 against the float64 model: inside the fp16 forms' bound (the final rounding + e_model).  The split model is
    e_split from the exact block by definition; what is checked is that e_split is of the size 22-bit pairs allow: 2^-22 relative per tensor over the block's six
    tensors (x, A | B, a' | Y, b', the weights, the output pair), max |value| <= 4."""
    f = R.figures(c)
    got = R.r16(f["model32"])
    ratio = ((got - f["model64"]).abs() / R.bound16(c, got)).max().item()
    print(f"{c}: e_model {f['e_model']:.2e} e_split {f['e_split']:.2e} trans {f['trans']:.2e}; clean float32 model at {ratio:.2f} of the fp16 bound")
    assert ratio <= 1.0
    assert torch.isfinite(f["model64"]).all() and f["model64"].abs().max() <= 4.0
    assert 0 < f["e_split"] <= 6 * 4.0 * 2.0 ** -22
    assert f["e_model"] <= 2.0 ** -10          # a handful of one-ulp16 flips of values below 2, carried through gains of ~1: nowhere near a wrong term


def faulty_ratios(fault, c):
    x, f = R.data(c), R.figures(c)
    with torch.no_grad():
        g16 = R.r16(R.block(x, R.weights16(c.family), torch.float32, "fp16", fault)).double()
        gs = R.block(x, R.weights(c.family), torch.float64, "split", fault)
    return ((g16 - f["model64"]).abs() / R.bound16(c, g16)).max().item(), ((gs - f["exact"]).abs().max() / R.bound_split(c)).item()


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_exceeds_both_bounds(fault):
    """In both weight families, on at least one case the fault can act on (seams only where W > 32 / H > 8, the neighbouring image only where N > 1, the others on every
    case), model(fault) misses the fp16 forms' bound and the split form's bound by >= 10x on some element."""
    seen16, seens = {}, {}
    for c in CASES:
        if not R.fault_acts(fault, c):
            continue
        r16, rs = faulty_ratios(fault, c)
        print(f"{fault} {c}: err / bound fp16 {r16:.1f} split {rs:.0f}")
        seen16[c.family] = max(seen16.get(c.family, 0.0), r16)
        seens[c.family] = max(seens.get(c.family, 0.0), rs)
    MARGINS[(fault, "fp16")], MARGINS[(fault, "split")] = seen16, seens
    assert tuple(seen16) == R.FAMILIES
    for fam in R.FAMILIES:
        assert seen16[fam] >= 10.0, f"{fault} is invisible to the fp16 bound in family {fam}: worst err / bound {seen16[fam]:.2f}"
        assert seens[fam] >= 10.0, f"{fault} is invisible to the split bound in family {fam}: worst err / bound {seens[fam]:.2f}"


def test_faults_act_where_they_should():
    assert [R.fault_acts("seam_col", R.Case("flat", *s)) for s in R.CPU_SHAPES] == [True, True, True]
    assert [R.fault_acts("seam_row", R.Case("flat", 1, h, 40)) for h in (8, 9)] == [False, True]
    assert [R.fault_acts("prev_image", R.Case("flat", *s)) for s in R.CPU_SHAPES] == [False, False, True]
    c = R.Case("live", 1, 8, 32)                  # one 8 x 32 tile, one image: the seam and image faults change nothing
    x, w = R.data(c), R.weights16("live")
    clean = R.block(x, w, torch.float64, "fp16")
    for fault in ("seam_col", "seam_row", "prev_image"):
        assert torch.equal(R.block(x, w, torch.float64, "fp16", fault), clean)
    with pytest.raises(AssertionError):
        R.block(x, w, torch.float64, "fp16", "nonsense")


def test_wiring_network_discriminates():
    """The network of test_gpu_pan_scpa.py's wiring test (SCPA convs x 2.75): the restatement of PAN.forward used to plant faults is the oracle, every fault of the
    table moves the oracle by >= 3x the networks' fp16 bound, and the fp16 restatement stays within a third of it."""
    for line in R.assert_wiring_discriminates(R.wiring()):
        print("[pan-scpa] wiring:", line)


def test_report():
    print("\n[pan-scpa] fault | bound | worst err / bound per family")
    for (fault, b), seen in MARGINS.items():
        print(f"[pan-scpa] {fault} | {b} | " + ", ".join(f"{k} {v:.0f}" for k, v in seen.items()))
