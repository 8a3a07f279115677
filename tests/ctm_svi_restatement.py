"""
The fp64 restatement of stochastic (minibatch) CTM training (include/tmvb.h, "stochastic (minibatch) training for CTM"), written
from the existing fp64 oracle: oracle.CTM.estep(d0, d1) on the batch's documents, NumPy fp64 for rho_t = (tau0 + t)^(-kappa), c0 = fp32(1 - rho_t),
c1 = fp32(rho_t M / M_b), the recentring of the running scatter matrix and the blends, the oracle's update_beta() on the blended statistic, and NumPy fp64
for sigma = (diag(vbar) + Cbar) / M, np.linalg.inv and mu = lbar / M.  Shared by tests/test_ctm_svi_host.py and tests/test_ctm_svi_gpu.py.
"""
import numpy as np


def recentre(cbar, lbar, mref, mu, M):
    """C' = Cbar + a d^T + d a^T + M d d^T with a = lbar - M m_ref, d = m_ref - mu: the scatter about mu of the weighted population (total weight M, weighted
    sum lbar) whose scatter about m_ref is Cbar"""
    a, d = lbar - M * mref, mref - mu
    return cbar + np.outer(a, d) + np.outer(d, a) + M * np.outer(d, d)


def coefficients(t, tau0, kappa, M, Mb):
    rho = (tau0 + t) ** -kappa
    return rho, float(np.float32(1.0 - rho)), float(np.float32(rho * M / Mb))


class Restatement:
    def __init__(self, oracle, doc_ptr, terms, counts, V, K, cuts, beta0, tau0, kappa):
        self.om = oracle.CTM(oracle.CSR(doc_ptr, terms, counts, V), K, beta0)
        om = self.om
        self.K, self.M, self.V, self.cuts, self.tau0, self.kappa = K, om.M, V, [int(c) for c in cuts], tau0, kappa
        self.sbar = (float(np.sum(counts, dtype=np.int64)) / K) * om.beta              # normalising it gives beta_0 back
        self.reset_tail()
        self.t = 0

    def reset_tail(self):
        """the initial tail from the per-document state about the current mu"""
        om = self.om
        L = om.lam - om.mu[:, None]
        self.lbar, self.vbar, self.cbar, self.mref = om.lam.sum(axis=1), om.vsq.sum(axis=1), L @ L.T, om.mu.copy()

    def step(self, b, viter, vtol, niter=1000, ntol=None):
        om, (d0, d1) = self.om, self.cuts[b:b + 2]
        om.beta_temp[:] = 0.0
        sw = om.estep(niter=niter, ntol=ntol, viter=viter, vtol=vtol, d0=d0, d1=d1)
        lam, vsq = om.lam[:, d0:d1], om.vsq[:, d0:d1]
        L = lam - om.mu[:, None]
        s_b, l_b, v_b, c_b = om.beta_temp.copy(order="F"), lam.sum(axis=1), vsq.sum(axis=1), L @ L.T
        self.t += 1
        rho, c0, c1 = coefficients(self.t, self.tau0, self.kappa, self.M, d1 - d0)
        cp = recentre(self.cbar, self.lbar, self.mref, om.mu, self.M)                  # before lbar moves
        self.cbar = c0 * cp + c1 * c_b
        self.sbar = c0 * self.sbar + c1 * s_b
        self.lbar = c0 * self.lbar + c1 * l_b
        self.vbar = c0 * self.vbar + c1 * v_b
        self.mref = om.mu.copy()
        om.beta_temp[:] = self.sbar
        om.update_beta()
        om.beta_temp[:] = 0.0
        om.sigma = np.asfortranarray((np.diag(self.vbar) + self.cbar) / self.M)        # about the pre-step mu: update_sigma! before update_mu!
        om.invsigma = np.asfortranarray(np.linalg.inv(om.sigma))
        om.mu = self.lbar / self.M
        return np.asarray(sw), rho, c0, c1

    def final_pass(self, viter, vtol, niter=1000, ntol=None):
        sw = np.concatenate([self.om.estep(niter=niter, ntol=ntol, viter=viter, vtol=vtol, d0=self.cuts[b], d1=self.cuts[b + 1])
                             for b in range(len(self.cuts) - 1)])
        self.om.beta_temp[:] = 0.0
        return sw
