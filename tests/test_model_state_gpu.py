"""
update_buffer() then update_host() returns every state field of every device model as itself.

The five models send and fetch their state through one shared implementation driven by a per-model field list (topicmodelsvb.jl_amd/_model.py),
so a swapped or shifted argument there would put one field's values into another.  Every field gets values from a range of its own (no two
fields of a model overlap, equal shapes or not), chosen not to be fp32 numbers, and must come back:

  * exactly, where the library keeps fp64 (tmvb_<m>_set_state copies the doubles: alpha, mu, sigma, invsigma, eta, CTPF's rate vectors, elbo);
  * as the float32 rounding of what was sent, where it keeps fp32 (upload_f32 / *_upload_beta cast once, download_f32 widens).

Which is which is read off tmvb_lda_set_state / _get_state (csrc/tmvb_lda.hip), tmvb_flda_* (csrc/tmvb_flda.hip), tmvb_ctm_* and tmvb_fctm_*
(csrc/tmvb_ctm.hip), tmvb_ctpf_set_state / _set_state_old / _get_state (csrc/tmvb_ctpf.hip) and listed per model below.  No returned field is
derived: what the library derives from the state (CTPF's log rates, the filtered models' L tables) stays on the device.  CTPF's hyper-parameters
a..h go to the handle and are not part of tmvb_ctpf_get_state, so they are not compared.

The corpus is the smallest with every field non-empty: M = 5, V = 7, K = 3, one count above 1; U = 4 readers for CTPF; tau has nnz entries.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 3
DOC_PTR = [0, 2, 4, 7, 9, 11]
TERMS = [0, 3, 1, 4, 2, 5, 6, 0, 6, 3, 5]
COUNTS = [1, 2, 1, 1, 3, 1, 1, 1, 1, 2, 1]
RDR_PTR = [0, 1, 3, 4, 6, 7]
READERS = [0, 1, 2, 3, 0, 2, 1]
RATINGS = [1, 2, 1, 1, 3, 1, 1]

# model -> (constructor, fields the library keeps in fp64, fields it keeps in fp32), each list in the order of the model's set_state
MODELS = {
    "lda": ("gpuLDA", ("alpha",), ("beta", "beta_old", "gamma", "Elogtheta", "Elogtheta_old")),
    "flda": ("gpufLDA", ("eta", "alpha"), ("kappa", "kappa_old", "beta", "beta_old", "gamma", "Elogtheta", "Elogtheta_old", "tau", "tau_old")),
    "ctm": ("gpuCTM", ("mu", "sigma", "invsigma"), ("beta", "beta_old", "lam", "lam_old", "vsq", "logzeta")),
    "fctm": ("gpufCTM", ("eta", "mu", "sigma", "invsigma"), ("kappa", "kappa_old", "beta", "beta_old", "lam", "lam_old", "vsq", "logzeta", "tau", "tau_old")),
    "ctpf": ("gpuCTPF", ("bet", "vav", "dalet", "het", "bet_old", "vav_old", "dalet_old", "het_old"),
             ("alef", "alef_old", "he", "he_old", "gimel", "gimel_old", "zayin", "zayin_old")),
}


def corpus(tmvb, readers):
    if readers:
        return tmvb.PackedCorpus(DOC_PTR, TERMS, COUNTS, 7, RDR_PTR, READERS, RATINGS, 4)
    return tmvb.PackedCorpus(DOC_PTR, TERMS, COUNTS, 7)


def pattern(q, nfields, shape):
    """Values of field number q of nfields: inside ((q + 1) / (nfields + 2), (q + 2) / (nfields + 2)), all different, in memory (column-major) order."""
    n = int(np.prod(shape)) if shape else 1
    v = (q + 1 + 0.987654321 * np.arange(1, n + 1) / (n + 1.0)) / (nfields + 2.0)        # (the odd factor: no entry is an fp32 number)
    return v.reshape(shape, order="F") if shape else float(v[0])


@pytest.mark.parametrize("fam", sorted(MODELS))
def test_every_state_field_comes_back_as_itself(tmvb, fam):
    ctor, f64, f32 = MODELS[fam]
    g = getattr(tmvb, ctor)(corpus(tmvb, fam == "ctpf"), K)
    names = f64 + f32
    sent = {}
    for q, name in enumerate(names):
        shape = np.shape(getattr(g, name))
        v = pattern(q, len(names), shape)
        if name in ("sigma", "invsigma"):                   # symmetric and positive-definite (tmvb_ctm_set_state checks invsigma): diagonally dominant
            v = np.asfortranarray(0.5 * (v + v.T) + K * np.eye(K))
        if name.startswith("Elogtheta"):                    # E[log theta] <= 0
            v = -v
        sent[name] = v
        setattr(g, name, v.copy(order="F") if shape else v)
    g.elbo = -1234.000000000001
    assert all(np.size(sent[n]) > 0 for n in names), "a field of this corpus is empty"
    distinct = lambda n: sent[n][np.tril_indices(K)] if n in ("sigma", "invsigma") else np.ravel(sent[n])      # (a symmetric matrix repeats its off-diagonal)
    flat = np.abs(np.concatenate([distinct(n) for n in names]))
    assert len(np.unique(flat)) == len(flat), "two entries of the state share a value"
    assert not np.any(flat == flat.astype(np.float32)), "a value that fp32 holds exactly would not show the rounding"

    g.update_buffer()
    for name in names:                                      # what update_host must overwrite
        setattr(g, name, None)
    g.elbo = 0.0
    g.update_host()

    for name in f64:
        got = getattr(g, name)
        assert np.shape(got) == np.shape(sent[name]), name
        assert np.array_equal(np.asarray(got), np.asarray(sent[name])), (fam, name, "fp64 field must return exactly")
    for name in f32:
        got = getattr(g, name)
        assert got.dtype == np.float64 and got.shape == sent[name].shape, name
        assert np.array_equal(got, sent[name].astype(np.float32).astype(np.float64)), (fam, name, "fp32 field must return the float32 rounding")
    assert g.elbo == -1234.000000000001
    g.close()
