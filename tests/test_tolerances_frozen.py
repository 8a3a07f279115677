"""
The tolerances of the parity tests are frozen at <= 10x the worst deviation measured on MI355X (round-4 review: they were 25x - 260x looser than anything
measured).  This CPU test keeps them honest: every named tolerance of tests/tol.py and oracle/parity.py carries its measured worst value, and
tolerance / measured must lie in [1, 10] -- looser is a test without teeth, tighter would fail on the evidence.  The evidence itself is committed:
profiles/r5_tolerances_measured.json (`TMVB_TOL_RECORD=1 pytest -m gpu` on the box, merged with bench.py's full-size parity blocks).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import tol  # noqa: E402
from oracle import parity  # noqa: E402


def _ratio_ok(name, t, m):
    assert m is not None, f"{name}: no measured value"
    if m == 0.0:
        return                                   # nothing ever deviated (CTM sweep mismatches): any small bound
    assert 1.0 <= t / m <= 10.0, f"{name}: tolerance {t:g} is {t / m:.1f}x the measured worst {m:g}"


def test_every_test_tolerance_is_within_10x_of_its_measurement():
    assert len(tol.TOL) >= 25
    for k, t in tol.TOL.items():
        _ratio_ok(k, t, tol.MEASURED[k])


def test_every_full_size_tolerance_is_within_10x_of_its_measurement():
    for model, d in (("lda", parity.LDA_TOL), ("ctm", parity.CTM_TOL), ("ctpf", parity.CTPF_TOL)):
        assert set(d) == set(parity.MEASURED[model]), model
        for k, t in d.items():
            _ratio_ok(f"{model}.{k}", t, parity.MEASURED[model][k])
    assert (parity.LAMBDA_ABS, parity.LAMBDA_REL) == (tol.LAMBDA_ABS, tol.LAMBDA_REL)


def test_the_measured_values_are_the_committed_evidence():
    ev = json.load(open(os.path.join(ROOT, "profiles", "r5_tolerances_measured.json")))
    ev6 = json.load(open(os.path.join(ROOT, "profiles", "r6_tolerances_measured.json")))       # the round-6 keys (section 8(f) rows, full-size free-running CTM)
    evt = json.load(open(os.path.join(ROOT, "profiles", "trained_tolerances_measured.json")))   # the trained-state keys (tests/test_trained_state_parity_gpu.py)
    assert not (set(ev6) & set(ev)), "a key is measured in one round's evidence file only"
    # the trained fLDA keys (tests/test_trained_state_parity_gpu.py::test_flda_trained_state): their own evidence file, measured later
    evf = json.load(open(os.path.join(ROOT, "profiles", "flda_trained_tolerances_measured.json")))
    assert not (set(evt) & (set(ev) | set(ev6))) and all(k.startswith("trained.") for k in evt)
    assert not (set(evf) & (set(ev) | set(ev6) | set(evt))) and all(k.startswith("trained.flda.") for k in evf)
    ev.update(ev6); ev.update(evt); ev.update(evf)
    assert {k for k in tol.MEASURED if k.startswith("trained.")} == set(evt) | set(evf), "every trained.* key has its measurement and no more"
    scale = 10.0                                  # the evidence file holds lambda_err in units of the round-4 bound (1.5e-4): x 10 in today's units
    for k, m in tol.MEASURED.items():
        e = ev[k] * (scale if k == "ctm.lambda_err" else 1.0)
        assert abs(m - e) <= 0.02 * e, (k, m, e)
    for model in ("lda", "ctm", "ctpf"):
        for k, m in parity.MEASURED[model].items():
            e = ev[f"parity.{model}.{k}"] * (scale if k.startswith("lambda_err") else 1.0)
            assert abs(m - e) <= 0.02 * max(e, 1e-300), (model, k, m, e)
