"""
The device against the oracle on one corpus in seven presentations (tests/presentations.py): entries shuffled / descending inside the documents,
documents permuted, vocabulary and users relabelled, ids REPEATED inside documents (un-condensed; quirk Q1 of SURVEY.md: the engine accumulates
repeats, so the result is that of the condensed document), and all of it at once.  Every other GPU test feeds sorted, condensed corpora in
generation order, so a kernel or a host builder that leans on that presentation would go unseen: tmvb_build_inv_index (a document twice in a
posting list, its two postings in different partial-sum slots of termstats_multi_kernel: presentations.straddle), the length buckets (a document's
length is its number of ENTRIES: P5 moves the two long documents to other kernels), the longest-first order and its map back to corpus order for
every per-document output, the tile gathers that read terms[] in entry order, and the decomposed ELBO forms (sum_n c_n log s_n per postings chunk).

The fp64 C oracle runs ONCE per case, on the canonical corpus; its states are carried into each presentation's labelling and order to force the
device and to compare with (the maps are bijections except for tau, which holds one value per entry: every repeat of an id is compared with the id's
value), doc_sweeps() is carried back.  tests/test_corpus_presentations.py (CPU) proves the premise: in fp64 every presentation reproduces the
canonical run to 1e-10.  The tolerances are the frozen keys of each model's own teacher-forced test in tests/tol.py: same quantity, same kind of test.

One exception, named: CTPF's ELBO holds -lgamma(c + 1) per entry (the Binomial sums of _binom_lgamma_sum and _multinomial_entropy cancel, what is
left of the multinomial entropy is not additive in the count), so under P5 / P6 it differs from the canonical value by
sum over the split entries of lgamma(c + 1) - sum_parts lgamma(c_part + 1), a constant of the presentation, whatever the state.
The CPU file proves that identity with the accumulating NumPy oracle run on the presentation itself, at 1e-10 on a corpus small enough for its
Python loops (its update_elbo! needs minutes at this size); here the canonical C oracle's ELBO plus that constant is the reference, at ctpf.elbo_rel_step.
"""
import numpy as np
import pytest

import presentations as P
import test_ctm_gpu as T_ctm
import test_ctpf_gpu as T_ctpf
import test_fctm_gpu as T_fctm
import test_flda_gpu as T_flda
import test_lda_gpu as T_lda
from tol import LAMBDA_ABS, LAMBDA_REL, rel, within

pytestmark = pytest.mark.gpu

VITER = 3


# ------------------------------------------------------------------------------------------------ the five models
def _lda_step(m, **kw):
    sw = m.estep(**kw)
    if hasattr(m, "reduce_docs"):
        m.reduce_docs()
    m.update_beta(); m.update_alpha()
    return sw


def _ctm_step(m, **kw):
    sw = m.estep(**kw)
    if hasattr(m, "reduce_docs"):
        m.reduce_docs(); m.update_beta(); m.update_sigma(); m.update_mu()
    else:
        m.update_beta(); m.update_sigma_mu()
    return sw


def _mstep_step(m, **kw):
    sw = m.estep(**kw)
    if hasattr(m, "reduce_docs"):
        m.reduce_docs()
    m.mstep()
    return sw


def _lda_compare(gm, o, e_g, tag):
    within("lda.gamma_rel", rel(gm.gamma, o.gamma), tag)
    within("lda.Elogtheta_rel", rel(gm.Elogtheta, o.Elogtheta), tag)
    within("lda.Elogtheta_rel", rel(gm.Elogtheta_old, o.Elogtheta_old), (tag, "old"))
    big = o.beta > 1e-6
    within("lda.beta_rel", rel(gm.beta[big], o.beta[big]), tag)
    within("lda.beta_abs", np.abs(gm.beta - o.beta), tag)
    within("lda.alpha_rel", rel(gm.alpha, o.alpha), tag)
    within("lda.elbo_rel_step", abs(e_g - o.elbo) / abs(o.elbo), (tag, e_g, o.elbo))
    np.testing.assert_allclose(gm.beta.sum(axis=1), 1.0, rtol=1e-5)
    assert np.all(gm.gamma > 0) and np.all(gm.Elogtheta <= 0)


def _ctm_compare(gm, o, e_g, tag):
    within("ctm.lambda_err", np.abs(gm.lam - o.lam) / (LAMBDA_ABS + LAMBDA_REL * np.abs(o.lam)), (tag, np.abs(gm.lam - o.lam).max()))
    within("ctm.vsq_rel", np.abs(gm.vsq - o.vsq) / o.vsq, tag)
    within("ctm.logzeta_abs", np.abs(gm.logzeta - o.logzeta), tag)
    big = o.beta > 1e-6
    within("ctm.beta_rel", np.abs(gm.beta[big] - o.beta[big]) / o.beta[big], tag)
    within("ctm.mu_abs", np.abs(gm.mu - o.mu), tag)
    within("ctm.sigma_rel", np.abs(gm.sigma - o.sigma).max() / np.abs(o.sigma).max(), tag)
    within("ctm.invsigma_rel", np.abs(gm.invsigma - o.invsigma).max() / np.abs(o.invsigma).max(), tag)
    within("ctm.elbo_rel_step", abs(e_g - o.elbo) / abs(o.elbo), (tag, e_g, o.elbo))
    np.testing.assert_allclose(gm.beta.sum(axis=1), 1.0, rtol=1e-5)
    assert np.all(gm.vsq > 0)
    np.linalg.cholesky(gm.sigma)


def _ctpf_compare(gm, o, e_g, tag):
    for n in ("gimel", "zayin", "alef", "he"):
        within("ctpf.shape_rel", T_ctpf.rel(getattr(gm, n), getattr(o, n)), (tag, n))
    for n in ("bet", "vav", "dalet", "het"):
        within("ctpf.rates_rel", T_ctpf.rel(getattr(gm, n), getattr(o, n)), (tag, n))
    assert np.isfinite(e_g)
    within("ctpf.elbo_rel_step", abs(e_g - o.elbo) / abs(o.elbo), (tag, e_g, o.elbo))
    assert np.all(gm.alef > 0) and np.all(gm.he > 0) and np.all(gm.gimel > 0) and np.all(gm.zayin > 0)


def _flda_compare(gm, o, e_g, tag):
    r = T_flda.rel
    within("flda.gamma_rel", r(gm.gamma, o.gamma), tag)
    within("flda.Elogtheta_rel", r(gm.Elogtheta, o.Elogtheta), tag)
    within("flda.tau_abs", np.abs(gm.tau - o.tau).max(initial=0.0), tag)
    within("flda.tau_abs", np.abs(gm.tau_old - o.tau_old).max(initial=0.0), (tag, "tau_old"))
    big = o.beta > 1e-6
    within("flda.beta_rel", r(gm.beta[big], o.beta[big]), tag)
    within("flda.beta_abs", np.abs(gm.beta - o.beta).max(), tag)
    bk = o.kappa > 1e-8
    within("flda.kappa_rel", r(gm.kappa[bk], o.kappa[bk]), tag)
    within("flda.alpha_rel", r(gm.alpha, o.alpha), tag)
    within("flda.eta_abs", abs(gm.eta - o.eta), (tag, gm.eta, o.eta))
    within("flda.elbo_rel_step", abs(e_g - o.elbo) / abs(o.elbo), (tag, e_g, o.elbo))
    np.testing.assert_allclose(gm.beta.sum(axis=1), 1.0, rtol=1e-5)
    np.testing.assert_allclose(gm.kappa.sum(), 1.0, rtol=1e-5)
    assert np.all((gm.tau >= 0) & (gm.tau <= 1)) and np.all(gm.gamma > 0) and np.all(gm.Elogtheta <= 0)


def _fctm_compare(gm, o, e_g, tag):
    T_fctm.compare(gm, o, tag)
    within("fctm.elbo_rel_step", abs(e_g - o.elbo) / abs(o.elbo), (tag, e_g, o.elbo))


def _init(tmvb, model, K, V):
    if model == "ctpf":
        return dict(alef0=np.exp(tmvb.dirichlet_rows(K, V, seed=6) - 0.5))
    g = dict(beta0=tmvb.dirichlet_rows(K, V, seed=5))
    if model in ("flda", "fctm"):
        g["kappa0"] = tmvb.dirichlet_rows(1, V, seed=9)[0]
    return g


MODELS = {
    # module with make_pair / force, step, comparison, state fields, (the field of the exit test, its _old)
    "lda": (T_lda, _lda_step, _lda_compare, P.FIELDS["lda"], ("Elogtheta", "Elogtheta_old")),
    "ctm": (T_ctm, _ctm_step, _ctm_compare, P.FIELDS["ctm"], ("lam", "lam_old")),
    "ctpf": (T_ctpf, _mstep_step, _ctpf_compare, P.FIELDS["ctpf"], ("gimel", "gimel_old")),
    "flda": (T_flda, _mstep_step, _flda_compare, P.FIELDS["flda"], ("Elogtheta", "Elogtheta_old")),
    "fctm": (T_fctm, _mstep_step, _fctm_compare, P.FIELDS["fctm"], ("lam", "lam_old")),
}
U_CTPF = 120

_CANON, _PRES, _ORACLE = {}, {}, {}


def canon(model):
    key = "ctpf" if model == "ctpf" else "cover" if model in ("ctm", "fctm") else "plain"
    if key not in _CANON:
        _CANON[key] = P.canonical(U=U_CTPF if key == "ctpf" else 0, cover=(key == "cover"))
    return _CANON[key]


def pres(model, name):
    c = canon(model)
    if (id(c), name) not in _PRES:
        _PRES[(id(c), name)] = P.present(c, name)
    return _PRES[(id(c), name)]


def new_oracle(tmvb, oracle, model, K):
    c = canon(model)
    _, om = MODELS[model][0].make_pair(tmvb, oracle, c.case(K=K, **_init(tmvb, model, K, c.V)))
    return om


def oracle_states(tmvb, oracle, model, K, fixed):
    """states before / after each teacher-forced iteration of the canonical corpus (after: with the sweeps and the ELBO), computed once"""
    key = (model, K, fixed)
    if key not in _ORACLE:
        _, step, _, names, _ = MODELS[model]
        om = new_oracle(tmvb, oracle, model, K)
        states = [P.snapshot(om, names)]
        for it in range(2 if fixed else 3):
            sw = step(om, **(dict(viter=VITER, vtol=0.0) if fixed else {}))
            states.append(P.snapshot(om, names, sw=np.array(sw), elbo=om.update_elbo() if fixed else None))
        _ORACLE[key] = states
    return _ORACLE[key]


def device_model(tmvb, oracle, model, K, p):
    c = canon(model)
    init = {n: p.cols(v) for n, v in _init(tmvb, model, K, c.V).items()}
    gm, _ = MODELS[model][0].make_pair(tmvb, oracle, p.case(K=K, **init))
    return gm


def check_info(gm, p):
    """tmvb_corpus_info against NumPy counts of the presented CSR"""
    got, want = gm.dcorp.info(), p.numpy_info()
    for n in ("n_docs_with_duplicate_terms", "n_docs_with_duplicate_readers", "max_doc_len", "sum_counts", "sum_ratings", "nnz", "nR", "n_empty_docs", "max_readers"):
        assert got[n] == want[n], (p.name, n, got[n], want[n])
    c0 = p.canon.numpy_info()
    assert want["sum_counts"] == c0["sum_counts"] and want["sum_ratings"] == c0["sum_ratings"]        # no presentation changes them
    if p.name in ("P5", "P6"):
        assert want["n_docs_with_duplicate_terms"] > p.M // 2 and want["max_doc_len"] > c0["max_doc_len"]


# ------------------------------------------------------------------------------------------------ the tests
CASES = [("lda", 7, 0), ("lda", 50, 0), ("lda", 100, 0), ("lda", 130, 0), ("lda", 50, 3), ("ctm", 12, 0), ("ctm", 50, 0), ("ctm", 100, 0),
         ("ctpf", 8, 0), ("ctpf", 50, 0), ("ctpf", 150, 0), ("flda", 9, 0), ("flda", 50, 0), ("fctm", 4, 0), ("fctm", 50, 0)]


@pytest.mark.parametrize("name", P.NAMES)
@pytest.mark.parametrize("model,K,pieces", CASES, ids=[f"{m}_k{k}" + (f"_pieces{q}" if q else "") for m, k, q in CASES])
def test_teacher_forced_fixed_sweeps(tmvb, oracle, model, K, pieces, name, monkeypatch):
    """Two teacher-forced iterations with pinned sweeps (vtol = 0) per case and presentation: every per-document field, every global and update_elbo!
    against the canonical oracle run at the model's frozen teacher-forced tolerances; doc_sweeps() in corpus order; tmvb_corpus_info."""
    if pieces:
        monkeypatch.setenv("TMVB_LDA_PIECES", str(pieces))             # read at create: the piece cuts follow the longest-first order
    mod, step, compare, names, _ = MODELS[model]
    p = pres(model, name)
    if name == "P5":
        assert P.straddle(p) is not None
    states = oracle_states(tmvb, oracle, model, K, True)
    gm = device_model(tmvb, oracle, model, K, p)
    check_info(gm, p)
    nonempty = np.diff(canon(model).doc_ptr) > 0
    for it in range(2):
        mod.force(gm, P.view({n: states[it][n] for n in names}, p))
        step(gm, viter=VITER, vtol=0.0)
        e_g = gm.update_elbo()
        gm.update_host()
        want = dict(states[it + 1])
        if model == "ctpf" and name in ("P5", "P6"):
            want["elbo"] = want["elbo"] + P.ctpf_elbo_shift(p)
        compare(gm, P.view(want, p), e_g, (model, K, name, it))
        sw = p.docs_back(gm.doc_sweeps())
        assert np.all(want["sw"][nonempty] == VITER)
        assert np.array_equal(sw, want["sw"]), (name, it, np.flatnonzero(sw != want["sw"]))


EXIT_CASES = {"lda": (7, "lda.gamma_rel", "gamma"), "ctm": (12, "ctm.lambda_err", "lam"), "ctpf": (8, "ctpf.shape_rel", "gimel"),
              "flda": (9, "flda.gamma_rel", "gamma"), "fctm": (4, "fctm.lambda_err", "lam")}


def near_threshold(tmvb, oracle, model, K, pre, sw):
    """documents whose exit test ||x - x_old|| < vtol comes within 1e-4 relative of vtol = 1 / K^2 at some sweep up to the oracle's exit: the
    oracle re-run from the same state with s = 1 .. 10 pinned sweeps gives every document's norm at sweep s"""
    _, _, _, names, (x, x_old) = MODELS[model]
    vtol = 1.0 / K ** 2
    near = np.zeros(len(sw), dtype=bool)
    for s in range(1, int(np.max(sw)) + 1):
        om = new_oracle(tmvb, oracle, model, K)
        P.restore(om, pre)
        om.estep(viter=s, vtol=0.0)
        norm = np.linalg.norm(getattr(om, x) - getattr(om, x_old), axis=0)
        near |= (sw >= s) & (np.abs(norm - vtol) <= 1e-4 * vtol)
    return near


@pytest.mark.parametrize("model", sorted(EXIT_CASES))
def test_default_exit_rule(tmvb, oracle, model):
    """The default per-document exit (vtol = 1 / K^2), three teacher-forced iterations: a document whose sweep count agrees with the oracle's is
    compared at the model's per-document key; the others are counted.  The canonical presentation stays within the 5 % cap of the models' own
    default-exit tests, and no presentation may have more mismatches than it plus the documents at the threshold (near_threshold)."""
    K, key, field = EXIT_CASES[model]
    mod, step, _, names, _ = MODELS[model]
    states = oracle_states(tmvb, oracle, model, K, False)
    nears = [near_threshold(tmvb, oracle, model, K, states[it], states[it + 1]["sw"]) for it in range(3)]
    mism = {}
    for name in P.NAMES:
        p = pres(model, name)
        gm = device_model(tmvb, oracle, model, K, p)
        mism[name] = 0
        for it in range(3):
            mod.force(gm, P.view({n: states[it][n] for n in names}, p))
            gm.estep()
            gm.update_host()
            o = P.view(states[it + 1], p)
            same = gm.doc_sweeps() == o.sw
            mism[name] += int((~same).sum())
            assert same.any()
            a, b = getattr(gm, field)[:, same], getattr(o, field)[:, same]
            within(key, np.abs(a - b) / (LAMBDA_ABS + LAMBDA_REL * np.abs(b)) if field == "lam" else rel(a, b), (model, name, it))
        print(f"default exit {model} {name}: {mism[name]} mismatching documents, near the threshold {[int(n.sum()) for n in nears]}")
    tot = 3 * canon(model).M
    assert mism["P0"] <= 0.05 * tot, f"{mism['P0']}/{tot} documents changed sweep count on the canonical presentation"
    for name in P.NAMES:
        assert mism[name] <= mism["P0"] + sum(int(n.sum()) for n in nears), (name, mism)


FREE = {"lda": (7, "lda.elbo_rel_free", (("alpha", "lda.alpha_rel_free", "rel"), ("beta", "lda.beta_abs_free", "abs"))),
        "ctm": (12, "ctm.elbo_rel_free", ()),
        "ctpf": (8, "ctpf.elbo_rel_free", ()),
        "flda": (9, "flda.elbo_rel_free", (("alpha", "flda.alpha_rel_free", "rel"), ("beta", "flda.beta_abs_free", "abs"), ("kappa", "flda.kappa_abs_free", "abs"),
                                          ("eta", "flda.eta_abs_free", "abs"))),
        "fctm": (4, "fctm.elbo_rel_free", (("mu", "fctm.mu_abs_free", "abs"), ("beta", "fctm.beta_abs_free", "abs"), ("kappa", "fctm.kappa_abs_free", "abs"),
                                          ("tau", "fctm.tau_abs_free", "abs")))}


@pytest.mark.parametrize("model", sorted(FREE))
def test_train_free_running(tmvb, oracle, model):
    """train!(iter = 5, checkelbo = 1) on P0 and P6 against the oracle's train! on the canonical corpus: the ELBO trajectory at the model's
    *.elbo_rel_free and the globals at its *_free keys (CTM and CTPF have none besides the ELBO's)."""
    K, ekey, fields = FREE[model]
    om = new_oracle(tmvb, oracle, model, K)
    t_o = np.asarray(om.train(iter=5, tol=0.0, checkelbo=1))
    assert len(t_o) == 5
    final = P.snapshot(om, MODELS[model][3])
    for name in ("P0", "P6"):
        p = pres(model, name)
        gm = device_model(tmvb, oracle, model, K, p)
        kw = dict(recs=False) if model == "ctpf" else {}
        t_g = np.asarray(gm.train(iter=5, tol=0.0, checkelbo=1, printelbo=False, **kw))
        want = t_o + (P.ctpf_elbo_shift(p) if model == "ctpf" and name == "P6" else 0.0)
        assert len(t_g) == 5
        within(ekey, np.abs(t_g - want) / np.abs(want), (model, name, t_g, want))
        o = P.view(final, p)
        for f, key, how in fields:
            a, b = np.asarray(getattr(gm, f), dtype=np.float64), np.asarray(getattr(o, f), dtype=np.float64)
            within(key, np.abs(a - b) / (np.abs(b) if how == "rel" else 1.0), (model, name, f))
