"""
The fp64 oracle -> fp32 device tolerances of the GPU parity tests, in ONE place, FROZEN at <= 10x the worst deviation ever measured on MI355X.

Round-4 review: the tolerances were 25x - 260x looser than anything measured -- a kernel that dropped epsilon, or used the wrong rate in a
logarithm, could still have passed.  SURVEY.md section 8(c) had said "to be confirmed by measurement, then frozen".  Procedure (round 5):
  1. every comparison of a parity test goes through within(key, value): one named tolerance per kind of quantity and kind of test;
  2. `TMVB_TOL_RECORD=1 pytest -m gpu` never fails a within() -- it records the worst value seen per key and writes them, at the end of
     the session, to gpurun_out/tolerances_measured.json (tests/conftest.py); profiles/r5_tolerances_measured.json is that file from the
     MI355X box, the evidence behind the numbers below;
  3. TOL[key] = the measured worst, rounded UP to 1 / 1.5 / 2 / 3 / 5 x 10^n within a factor 3 - 10 (MEASURED[key] is kept beside it and
     tests/test_tolerances_frozen.py -- CPU -- asserts TOL <= 10 x MEASURED for every key);
  4. tests/test_mutants_gpu.py builds three deliberately wrong libraries and asserts that named parity tests FAIL on them.
oracle/parity.py (the full-size checker, also used by bench.py) holds its own three dicts under the same rule.
"""
import json
import os

import numpy as np

RECORD = os.environ.get("TMVB_TOL_RECORD", "") not in ("", "0")
SEEN = {}

# key: (tolerance, worst value measured on MI355X -- profiles/r5_tolerances_measured.json; the round-6 keys: profiles/r6_tolerances_measured.json;
#      the trained.* keys: profiles/trained_tolerances_measured.json, the trained.flda.* keys: profiles/flda_trained_tolerances_measured.json)
_T = {
    # ---- LDA (tests/test_lda_gpu.py, tests/test_full_size_parity_gpu.py): max over every entry
    "lda.gamma_rel":            (1e-05, 1.94e-06),
    "lda.Elogtheta_rel":        (2e-05, 3.37e-06),
    "lda.beta_rel":             (2e-05, 2.37e-06),
    "lda.beta_abs":             (3e-07, 6.76e-08),
    "lda.alpha_rel":            (2e-05, 2.65e-06),
    "lda.elbo_rel_step":        (1e-06, 2.4e-07),
    "lda.elbo_rel_free":        (2e-06, 2.39e-07),
    "lda.elbo_forms_rel":      (5e-07, 6.8e-08),     # decomposed update_elbo! against the token walk on the same device state (tests/test_lda_elbo_parts_gpu.py)
    "lda.alpha_rel_free":       (5e-05, 5.65e-06),
    "lda.beta_abs_free":        (2e-05, 2.25e-06),
    # 10 free-running iterations of the FULL SYN-NSF corpus, K = 50
    "lda.elbo_rel_free_full":   (1.5e-06, 1.92e-07),
    "lda.alpha_rel_free_full":  (0.0002, 2.66e-05),
    "lda.beta_abs_free_full":   (3e-05, 3.55e-06),
    # ---- CTM (tests/test_ctm_gpu.py); lambda_err = max |dlambda| / (LAMBDA_ABS + LAMBDA_REL |lambda|)
    "ctm.lambda_err":           (5, 0.881),
    "ctm.vsq_rel":              (0.0001, 1.74e-05),
    "ctm.logzeta_abs":          (1e-05, 2.03e-06),
    "ctm.beta_rel":             (0.0001, 1.98e-05),
    "ctm.mu_abs":               (5e-06, 1.09e-06),
    "ctm.sigma_rel":            (1e-05, 1.45e-06),
    "ctm.invsigma_rel":         (1e-05, 1.57e-06),
    "ctm.elbo_rel_step":        (2e-07, 3.7e-08),
    "ctm.elbo_rel_free":        (1e-06, 1.06e-07),
    "ctm.elbo_forms_rel":      (1.5e-07, 2.29e-08),     # decomposed update_elbo! against the token walk on the same device state (tests/test_ctm_elbo_parts_gpu.py)
    # ---- CTPF (tests/test_ctpf_gpu.py): shapes = gimel, zayin, alef, he (K <= 256; _bigk: K > 256); rates = bet, vav, dalet, het
    "ctpf.shape_rel":           (0.002, 0.000493),
    "ctpf.shape_rel_bigk":      (0.005, 0.000965),
    "ctpf.rates_rel":           (0.0003, 5.61e-05),
    "ctpf.elbo_rel_step":       (5e-07, 8.43e-08),
    "ctpf.elbo_forms_rel":     (5e-07, 8.88e-08),     # decomposed update_elbo! against the table form on the same device state (tests/test_ctpf_elbo_parts_gpu.py)
    "ctpf.long.shape_rel":      (0.0001, 1.11e-05),
    "ctpf.long.rates_rel":      (3e-06, 4.75e-07),
    "ctpf.elbo_rel_free":       (0.0001, 2.72e-05),
    # ---- random shapes (tests/test_random_shapes_gpu.py: K, M, V, U drawn at random, one-document and one-term corpora, long documents)
    "rand.lda.gamma_rel":       (5e-06, 7.08e-07),
    "rand.lda.beta_rel":        (5e-06, 9.56e-07),
    "rand.lda.alpha_rel":       (0.0001, 1.43e-05),
    "rand.lda.elbo_rel":        (5e-06, 1.13e-06),
    "rand.ctm.lambda_err":      (5e-05, 6.17e-06),      # max |dlambda| / (1 + max |lambda|), default exit rules
    "rand.ctm.vsq_rel":         (5e-05, 9.53e-06),
    "rand.ctm.mu_abs":          (1e-05, 1.35e-06),
    "rand.ctm.sigma_err":       (2e-05, 3.1e-06),
    "rand.ctpf.shape_rel":      (3e-05, 4.63e-06),
    "rand.ctpf.rates_rel":      (5e-06, 7.61e-07),
    # ---- round 6: the SURVEY.md section 8(f) rows (tests/test_flda_gpu.py, test_fctm_gpu.py, test_predict_gpu.py, test_f*_elbo_parts_gpu.py) and the full-size
    # free-running CTM run (tests/test_full_size_parity_gpu.py); measured on MI355X: profiles/r6_tolerances_measured.json.  fctm.lambda_err in units of
    # LAMBDA_ABS + LAMBDA_REL |lambda| like ctm.lambda_err; .bigk = K > 128; predict.*: q90 over the documents and the maximum
    "ctm.beta_abs_free_full":            (1.5e-06, 3.61e-07),
    "ctm.elbo_rel_free_full":            (1.5e-07, 4.22e-08),
    "ctm.mu_abs_free_full":              (2e-05, 6.4e-06),
    "ctm.sigma_rel_free_full":           (1e-05, 2.47e-06),
    "fctm.beta_abs_free":                (3e-07, 6.75e-08),
    "fctm.beta_rel":                     (5e-05, 1.2e-05),
    "fctm.beta_rel.bigk":                (2e-05, 6.52e-06),
    "fctm.elbo_forms_rel":               (3e-07, 6.91e-08),
    "fctm.elbo_rel_free":                (1.5e-07, 4.21e-08),
    "fctm.elbo_rel_step":                (3e-07, 7.05e-08),
    "fctm.elbo_rel_step.bigk":           (3e-07, 7.38e-08),
    "fctm.kappa_abs_free":               (5e-08, 1.62e-08),
    "fctm.kappa_rel":                    (0.0001, 3.03e-05),
    "fctm.kappa_rel.bigk":               (0.00015, 4.72e-05),
    "fctm.lambda_err":                   (3, 0.707),
    "fctm.lambda_err.bigk":              (0.5, 0.129),
    "fctm.logzeta_abs":                  (1e-05, 1.71e-06),
    "fctm.logzeta_abs.bigk":             (3e-06, 7.9e-07),
    "fctm.mu_abs":                       (1e-05, 1.86e-06),
    "fctm.mu_abs.bigk":                  (2e-06, 6.07e-07),
    "fctm.mu_abs_free":                  (3e-06, 8.11e-07),
    "fctm.sigma_rel":                    (1e-05, 1.9e-06),
    "fctm.sigma_rel.bigk":               (5e-06, 1.43e-06),
    "fctm.tau_abs":                      (5e-06, 1.29e-06),
    "fctm.tau_abs.bigk":                 (1e-05, 1.75e-06),
    "fctm.tau_abs_free":                 (2e-06, 5.3e-07),
    "fctm.vsq_rel":                      (5e-05, 1.28e-05),
    "fctm.vsq_rel.bigk":                 (1.5e-05, 3.81e-06),
    "flda.Elogtheta_rel":                (3e-06, 9.61e-07),
    "flda.alpha_rel":                    (1.5e-05, 3.68e-06),
    "flda.alpha_rel_free":               (3e-06, 9.71e-07),
    "flda.beta_abs":                     (1e-06, 1.97e-07),
    "flda.beta_abs_free":                (5e-07, 1.44e-07),
    "flda.beta_rel":                     (5e-05, 1.03e-05),
    "flda.elbo_forms_rel":               (3e-07, 8.41e-08),
    "flda.elbo_rel_free":                (2e-07, 5.27e-08),
    "flda.elbo_rel_step":                (1e-06, 2.5e-07),
    "flda.eta_abs":                      (2e-07, 6.59e-08),
    "flda.eta_abs_free":                 (3e-07, 9.33e-08),
    "flda.gamma_rel":                    (1e-05, 1.73e-06),
    "flda.kappa_abs_free":               (1e-07, 3.26e-08),
    "flda.kappa_rel":                    (0.001, 0.000217),
    "flda.tau_abs":                      (1e-05, 2.58e-06),
    "predict.ctm.lambda_abs_max":        (1.5e-05, 3.81e-06),
    "predict.ctm.lambda_abs_q90":        (1e-05, 2.42e-06),
    "predict.fctm.lambda_abs_max":       (1.5e-05, 4.5e-06),
    "predict.fctm.lambda_abs_q90":       (1e-05, 2.44e-06),
    "predict.fctm.tau_abs_q99":          (1e-06, 2.8e-07),
    "predict.flda.gamma_rel_max":        (1e-05, 2.07e-06),
    "predict.flda.gamma_rel_q90":        (5e-06, 1.43e-06),
    "predict.flda.tau_abs_q99":          (1.5e-06, 4.01e-07),
    "predict.lda.gamma_rel_max":         (3e-06, 7.22e-07),
    "predict.lda.gamma_rel_q90":         (2e-06, 5.76e-07),
    # ---- trained states (tests/test_trained_state_parity_gpu.py): teacher-forced steps from states the device trained for 300 - 600 iterations
    # (ctm_host: a state the fp64 oracle trained, entering the device through gpuCTM(_from=host)); measured on MI355X: profiles/trained_tolerances_measured.json.
    # beta_rel_tail: every entry where the oracle holds >= 1e-30, no 1e-6 mask; beta_rel_floor: the fp32 normal band [2^-126, 1e-30).
    # trained.fctm.beta_rel_floor is 70x fctm.beta_rel: gradual underflow of the per-token contributions, DESIGN.md section 6
    "trained.ctm.beta_rel_floor":        (5e-06, 1.32e-06),
    "trained.ctm.beta_rel_tail":         (1e-05, 2.1e-06),
    "trained.ctm.elbo_rel":              (1.5e-07, 3.36e-08),
    "trained.ctm.invsigma_rel":          (1.5e-07, 3.92e-08),
    "trained.ctm.lambda_err":            (15, 3.74),
    "trained.ctm.logzeta_abs":           (5e-06, 1.34e-06),
    "trained.ctm.mu_abs":                (3e-05, 9.1e-06),
    "trained.ctm.sigma_rel":             (1e-05, 1.91e-06),
    "trained.ctm.vsq_rel":               (0.0001, 1.75e-05),
    "trained.ctm_host.beta_rel_floor":   (5e-06, 1.44e-06),
    "trained.ctm_host.beta_rel_tail":    (1e-05, 2.97e-06),
    "trained.ctm_host.elbo_rel":         (1.5e-07, 3.45e-08),
    "trained.ctm_host.lambda_err":       (10, 2.13),
    "trained.ctm_host.logzeta_abs":      (1e-05, 1.69e-06),
    "trained.ctm_host.vsq_rel":          (5e-05, 1.65e-05),
    "trained.ctpf.elbo_rel":             (5e-07, 1.14e-07),
    "trained.ctpf.rates_rel":            (1e-06, 2.66e-07),
    "trained.ctpf.shape_rel":            (1e-05, 1.72e-06),
    "trained.fctm.beta_rel_floor":       (0.003, 0.000846),
    "trained.fctm.beta_rel_tail":        (0.0001, 1.67e-05),
    "trained.fctm.elbo_rel":             (1e-07, 2.95e-08),
    "trained.fctm.invsigma_rel":         (1.5e-07, 4.48e-08),
    "trained.fctm.kappa_rel":            (0.0001, 2.04e-05),
    "trained.fctm.lambda_err":           (5, 1.42),
    "trained.fctm.logzeta_abs":          (5e-06, 1.36e-06),
    "trained.fctm.mu_abs":               (5e-06, 1.6e-06),
    "trained.fctm.sigma_rel":            (1.5e-06, 4.92e-07),
    "trained.fctm.tau_abs":              (3e-06, 8.79e-07),
    "trained.fctm.vsq_rel":              (0.0001, 1.93e-05),
    # fLDA (K = 50, 100 after 300 device iterations): alpha grows to hundreds, where alpha is ill-conditioned in the mean Elogtheta it is solved from
    # (an fp32 rounding of Elogtheta moves alpha by alpha x that much): alpha_rel and elbo_rel 10x the cold-start keys, DESIGN.md section 6;
    # measured on MI355X: profiles/flda_trained_tolerances_measured.json
    "trained.flda.Elogtheta_rel":       (3e-06, 5.38e-07),
    "trained.flda.alpha_rel":           (0.001, 0.000143),
    "trained.flda.beta_rel_tail":       (5e-05, 7.76e-06),
    "trained.flda.elbo_rel":            (5e-05, 9.15e-06),
    "trained.flda.eta_abs":             (2e-07, 4.09e-08),
    "trained.flda.gamma_rel":           (1e-06, 1.13e-07),
    "trained.flda.kappa_rel":           (3e-05, 4.88e-06),
    "trained.flda.tau_abs":             (1e-05, 1.88e-06),
    "trained.lda.Elogtheta_rel":         (3e-05, 8.97e-06),
    "trained.lda.alpha_rel":             (1e-06, 2.12e-07),
    "trained.lda.beta_rel_floor":        (1e-05, 2.55e-06),
    "trained.lda.beta_rel_tail":         (1e-05, 3.23e-06),
    "trained.lda.elbo_rel":              (5e-07, 1.61e-07),
    "trained.lda.gamma_rel":             (5e-05, 1.2e-05),
}
LAMBDA_ABS, LAMBDA_REL = 1.5e-5, 1.5e-5           # the bound ctm.lambda_err is measured against (round 4: 1.5e-4 + 1.5e-4 |lambda|, 11x looser than the worst case)

TOL = {k: v[0] for k, v in _T.items()}
MEASURED = {k: v[1] for k, v in _T.items()}


def within(key, value, detail=None):
    """assert value <= TOL[key] (and record it).  value may be an array: its max is taken."""
    v = float(np.max(value)) if np.size(value) else 0.0
    if not (v <= SEEN.get(key, -1.0)):
        SEEN[key] = v
    if RECORD:
        return True
    assert np.isfinite(v) and v <= TOL[key], f"{key}: {v:.3g} > {TOL[key]:.3g}" + (f"  [{detail}]" if detail is not None else "")
    return True


def rel(a, b, floor=0.0):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), floor if floor else 1e-300)


def dump(path):
    seen = dict(SEEN)
    try:
        from oracle import parity
        seen.update({"parity." + k: v for k, v in parity.SEEN.items()})
    except Exception:
        pass
    if seen:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        old = {}
        if os.path.exists(path):
            try:
                old = json.load(open(path))
            except Exception:
                old = {}
        for k, v in seen.items():
            old[k] = max(v, old.get(k, 0.0))
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)
