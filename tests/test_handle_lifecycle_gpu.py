"""
One whole life of a handle of every model family, twice: create, train three checked iterations, read the ELBO form, the sweep counts and their
histogram, hand the statistics to a buffer of the host's (tmvb_*_bind_stats), for LDA and CTM build, run and destroy a two-batch stochastic driver
next to it (shared globals, borrowed streams), destroy.  Everything a handle keeps on the device goes through its tmvb_owned (csrc/tmvb_handle.h);
a buffer released early, twice, or under a side stream that still works on it shows here as a fault or as a second life that differs from the
first.  The two lives must agree byte for byte: the downloaded state, the ELBO trajectory, the statistics.

The golden corpus of M = 40 documents over V = 60 terms (U = 15 readers for CTPF), K = 5.  LDA runs with TMVB_LDA_PIECES=3, so that the document
pieces, their events and the high-priority side stream exist.  No free-memory assertion: the card is shared.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ctpf_m40_v60_u15_k4.npz")
K = 5
FAMILIES = {"lda": "gpuLDA", "flda": "gpufLDA", "ctm": "gpuCTM", "fctm": "gpufCTM", "ctpf": "gpuCTPF"}
STOCHASTIC = {"lda": "gpuLDAStochastic", "ctm": "gpuCTMStochastic"}


def corpus(tmvb, readers):
    g = np.load(GOLD)
    assert (int(g["M"]), int(g["V"]), int(g["U"])) == (40, 60, 15)
    if readers:
        return tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], 60, g["rdr_ptr"], g["readers"], g["ratings"], 15)
    return tmvb.PackedCorpus(g["doc_ptr"], g["terms"], g["counts"], 60)


def life(tmvb, fam):
    """-> {what: bytes} of one handle's life"""
    import torch
    out = {}
    corp = corpus(tmvb, fam == "ctpf")
    g = getattr(tmvb, FAMILIES[fam])(corp, K)
    if fam == "lda":
        assert g.estep_pieces() == 3
    traj = g.train(iter=3, tol=0.0, checkelbo=1, printelbo=False)
    assert len(traj) >= 1 and np.all(np.isfinite(traj))
    out["traj"] = np.asarray(traj, dtype=np.float64).tobytes()
    out["form"] = bytes([g.elbo_form()])
    sweeps = g.doc_sweeps()
    assert sweeps.shape == (40,) and sweeps.max() >= 1
    out["sweeps"] = sweeps.tobytes()
    if hasattr(g, "sweep_hist"):
        hist = g.sweep_hist()
        if isinstance(hist, tuple):                      # CTM, fCTM: the Newton steps of the last E-step next to it
            hist, newton = hist
            assert newton > 0
            out["newton"] = np.int64(newton).tobytes()
        assert int(np.sum(hist)) == 40
        out["hist"] = np.asarray(hist).tobytes()
    bound = None
    if hasattr(g, "bind_stats"):
        ptr, n = g.stats()
        assert ptr and n > 0
        bound = torch.zeros(n, dtype=torch.float32, device="cuda")
        g.bind_stats(bound.data_ptr(), n)
        ptr2, n2 = g.stats()
        assert (ptr2, n2) == (bound.data_ptr(), n)
        g.synchronize()
        out["stats"] = bound.cpu().numpy().tobytes()
    if fam in STOCHASTIC:
        drv = getattr(tmvb, STOCHASTIC[fam])(corp, K, cuts=[0, 20, 40], ctx=g.ctx)
        drv.run([0, 1, 0])
        drv.update_host()
        out["svi_beta"] = np.asfortranarray(drv.beta).tobytes()
        drv.close()
    g.update_host()
    for name, _ in g._STATE:
        out[name] = np.asfortranarray(getattr(g, name)).tobytes()
    out["elbo"] = np.float64(g.elbo).tobytes()
    g.close()
    g.dcorp.close()
    g.ctx.close()
    del bound                                            # the bound buffer outlives the handle that used it
    return out


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_two_lives_of_a_handle_agree_byte_for_byte(tmvb, fam, monkeypatch):
    if fam == "lda":
        monkeypatch.setenv("TMVB_LDA_PIECES", "3")      # read at create
    first = life(tmvb, fam)
    second = life(tmvb, fam)
    assert sorted(first) == sorted(second)
    for what in first:
        assert first[what] == second[what], f"{fam}: {what} differs between two lives of a handle"
