"""The references of PAN's self-attention block (tests/_pan_attention_ref.py) on the CPU: that the model of pan_attention_mfma stays where its declared roundings
put it, and that the sweep of tests/test_gpu_pan_fsa.py DISCRIMINATES -- each of five planted faults, switched on in the model, exceeds the bound the device is
held to by more than 10x on some case of every operand family it can act on.  No GPU and no library call.

Why this matters: through a whole PAN forward none of these faults is visible (gamma -0.003, scores flat to three digits, 100x damping in the up-convs):

    planted fault (max change of the network output, G8 weights, 50 x 70)      seed 0 (gamma -0.003)    seed 41, gamma forced to 1
    attention output dropped altogether                                     7.4e-6                   2.6e-3
    p replaced by 1 / Np (scores ignored)                                   6.0e-8                   9.5e-7
    keys of p permuted against keys of h (j ^ 4)                            6.0e-8                   9.8e-7
    ragged last 32-key block dropped                                        6.0e-8                   1.4e-5
    padding keys admitted with score 0                                      6.6e-7                   --

against network bounds of 1e-2 (fp16) and 1e-4 (fp32 mode).
"""
import numpy as np
import pytest

import _pan_attention_ref as R

CASES = R.cases()


def test_sweep_is_what_the_issue_lists():
    assert len(CASES) == len(R.FAMILIES) * len(R.NP_SWEEP) == 52 and len(set(CASES)) == 52
    assert R.NP_SWEEP == (1, 2, 31, 32, 33, 64, 65, 96, 127, 129, 257, 513, 1057)
    for c in CASES:
        rows, bf, bg, bh, f, g, h = R.operands(c)
        assert rows.shape == (c.Np, 64) and np.isnan(rows[:, 50:]).all() and np.isfinite(rows[:, :50]).all()
        assert np.abs(f).max() <= 6.0 + 1e-5 and np.abs(g).max() <= 6.0 + 1e-5 and np.abs(h).max() <= 1.0 + 1e-6
        s = f.astype(np.float64) @ g.astype(np.float64).T
        if c.family == "negative":
            assert -36.0 <= s.min() and s.max() <= -9.0, (str(c), s.min(), s.max())
        if c.family == "flat":
            assert np.abs(s).max() <= 0.46
        if c.family == "peaked" and c.Np >= 31:
            assert (s.max(axis=1) - s.min(axis=1)).max() > 20.0
        if c.family == "ramp" and c.Np >= 31:          # rising and falling rows in the first wave's sixteen queries, the level row among them
            d = s[:16, -1] - s[:16, 0]
            assert (d > 1.0).any() and (d < -1.0).any() and (d == 0.0).any(), str(c)


def test_rtz16():
    x = np.array([0.0, 1.0, 1.0 - 2.0 ** -12, 2.0 ** -14 * (1 + 2.0 ** -10) * (1 + 2.0 ** -13), 2.0 ** -24 * 1.9, 2.0 ** -24 * 0.9, 3 * 2.0 ** -24 + 2.0 ** -30])
    want = np.array([0.0, 1.0, 1.0 - 2.0 ** -11, 2.0 ** -14 * (1 + 2.0 ** -10), 2.0 ** -24, 0.0, 3 * 2.0 ** -24])
    assert (R.rtz16(x) == want).all()
    r = np.random.default_rng(5).uniform(0, 1, 4096) ** 4
    t = R.rtz16(r)
    assert (t <= r).all() and (t.astype(np.float16).astype(np.float64) == t).all()          # below, and on the fp16 grid
    assert (r - t < np.maximum(np.abs(r) * 2.0 ** -10, 2.0 ** -24)).all()


@pytest.mark.parametrize("c", CASES, ids=str)
def test_model_holds_to_exact(c):
    """Non-split: fp16 h (2^-12 max|h| per value) and p truncated to fp16 (<= 2^-11 relative, numerator and denominator alike) stay within 3 * 2^-11 * max|h|.
    Split: within what its (hi, lo) pairs can cost (R.split_budget, from the number formats), and no worse than the non-split form."""
    _, _, _, _, f, g, h = R.operands(c)
    ref, e32, em, ems = R.figures(c)
    hm = float(np.abs(h).max())
    print(f"{c}: e32 {e32:.2e}  e_model {em:.2e} (limit {3 * 2.0 ** -11 * hm:.2e})  e_model split {ems:.2e} (budget {R.split_budget(f, g, h):.2e})")
    assert np.isfinite(ref).all() and np.abs(ref).max() <= hm
    assert em <= 3 * 2.0 ** -11 * hm, (str(c), em)
    assert ems <= R.split_budget(f, g, h), (str(c), ems)
    assert ems <= em


@pytest.mark.parametrize("form", (1, 2))
@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_exceeds_the_gpu_bound(fault, form):
    """On at least one case of every family the fault can act on, model(fault) misses the device's bound of tests/test_gpu_pan_fsa.py (8 e_model for form 1,
    8 (e_model split + e32) for form 2) by >= 10x."""
    seen = {}
    for c in CASES:
        if not R.fault_acts(fault, c):
            continue
        _, _, _, _, f, g, h = R.operands(c)
        ref = R.figures(c)[0]
        e = R.err(R.model(f, g, h, form == 2, fault), ref)
        ratio = e / R.bound(c, form)
        seen[c.family] = max(seen.get(c.family, 0.0), ratio)
    print(f"{fault}, form {form}: worst err / bound per family {({k: f'{v:.0f}' for k, v in seen.items()})}")
    want = ("negative",) if fault == "first_pair_m0" else R.FAMILIES
    assert tuple(k for k in R.FAMILIES if k in seen) == want
    for fam, ratio in seen.items():
        assert ratio >= 10.0, f"{fault} is invisible in family {fam}: worst err / bound {ratio:.2f} -- change the family, not the margin"


def test_faults_off_is_the_model():
    c = R.Case("ramp", 129, 3129)
    _, _, _, _, f, g, h = R.operands(c)
    assert (R.model(f, g, h, False) == R.model(f, g, h, False, None)).all()
    with pytest.raises(AssertionError):
        R.model(f, g, h, False, "nonsense")
