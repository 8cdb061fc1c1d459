"""Dense restatements of one spectral-mixture component (FastFoodGM, basis_functions.py:1386-1562) on the dense equivalent
V = _makeVX(I_d) of its chain -- NumPy only -- and the mixed case the fused small-minibatch kernel's spectral-mixture children
are held to (tests/test_fused_gm_host.py, tests/test_gpu_fused_svi_gm.py).

    Phi = [cos(VX + mX) | sin(VX + mX) | cos(VX - mX) | sin(VX - mX)] / sqrt(2 n),   VX = (X / l) V,   mX = X . mean

the reference's column order (:1471-1473); `gm_grad` returns (dPhi / dmean, dPhi / dlenscale) in the reference's shapes:
(N, 4n, d) each, (N, 4n) when d == 1 (:1477-1537)."""
import numpy as np


def gm_transform(X, V, mean, ls):
    X = np.asarray(X, dtype=float)
    d, n = V.shape
    ls, mean = np.broadcast_to(np.asarray(ls, dtype=float), (d,)), np.broadcast_to(np.asarray(mean, dtype=float), (d,))
    VX = (X / ls) @ V
    mX = (X @ mean)[:, None]
    return np.concatenate((np.cos(VX + mX), np.sin(VX + mX), np.cos(VX - mX), np.sin(VX - mX)), axis=1) / np.sqrt(2 * n)


def gm_grad(X, V, mean, ls):
    X = np.asarray(X, dtype=float)
    d, n = V.shape
    ls, mean = np.broadcast_to(np.asarray(ls, dtype=float), (d,)), np.broadcast_to(np.asarray(mean, dtype=float), (d,))
    VX = (X / ls) @ V
    mX = (X @ mean)[:, None]
    msp, msm, cp, cm = -np.sin(VX + mX), -np.sin(VX - mX), np.cos(VX + mX), np.cos(VX - mX)
    rt = np.sqrt(2 * n)
    dmean, dlen = [], []
    for i in range(d):
        xi = X[:, i:i + 1]
        dmean.append(np.concatenate((xi * msp, xi * cp, -xi * msm, -xi * cm), axis=1) / rt)
        dV = -(xi / ls[i] ** 2) * V[i][None, :]   # d VX / d l_i
        dlen.append(np.concatenate((dV * msp, dV * cp, dV * msm, dV * cm), axis=1) / rt)
    if d == 1:
        return dmean[0], dlen[0]
    return np.stack(dmean, axis=2), np.stack(dlen, axis=2)


def rff_transform(X, W, ls):
    Z = np.asarray(X, dtype=float) @ (W / np.asarray(ls, dtype=float)[:, None])
    return np.concatenate((np.cos(Z), np.sin(Z)), axis=1) / np.sqrt(W.shape[1])


def rff_grad(X, W, ls):
    """(N, 2n, d): ARD length scales (basis_functions.py:866-901)"""
    X, ls = np.asarray(X, dtype=float), np.asarray(ls, dtype=float)
    Z = X @ (W / ls[:, None])
    out = []
    for i in range(W.shape[0]):
        dZ = -(X[:, i:i + 1] / ls[i] ** 2) * W[i][None, :]
        out.append(np.concatenate((-np.sin(Z) * dZ, np.cos(Z) * dZ), axis=1) / np.sqrt(W.shape[1]))
    return np.stack(out, axis=2)


class Mixed(object):
    """Linear(onescol) on 5 columns | GM on columns [0, 2, 4] (d = 3, n = 8, mean [0.7, 0.0, -1.1]) | RFF, ARD, d = 5, n = 6 |
    GM on column [1] (d = 1, n = 5); Gaussian; N = 80, K = 3, L = 20, minibatches of 20 rows (B = 4): L and M one full 16-block
    plus a partial one.  Widths [6, 32, 12, 20]: F = 70; dsum = 5 + 3 + 5 + 1 = 14, M dsum = 280; n_ls = 6 + 5 + 2 = 13 -- the
    one-wave-per-slot loop takes a second turn, a random Fourier child's slots between two GM children's.
    z = [m | C | 4 regularisers | variance | GM1 mean (3), ls (3) | RFF ls (5) | GM2 mean, ls].  V and W are plain RandomState
    normals; the draws are rounded to float32 ONCE, for both sides."""

    N, d, K, L, M, F, n_ls = 80, 5, 3, 20, 20, 70, 13

    def __init__(self):
        rs = np.random.RandomState(17)
        self.X = rs.randn(self.N, self.d)
        self.y = np.sin(self.X[:, 0]) + 0.3 * self.X[:, 1] + 0.1 * rs.randn(self.N)
        self.ind1, self.ind2 = [0, 2, 4], [1]
        self.V1, self.W, self.V2 = rs.randn(3, 8), rs.randn(5, 6), rs.randn(1, 5)
        self.B = self.N / float(self.M)
        F, K = self.F, self.K
        self.slices = [slice(0, 6), slice(6, 38), slice(38, 50), slice(50, 70)]
        self.m = 0.3 * rs.randn(F, K)
        self.C = rs.gamma(2., 0.5, size=(F, K))
        self.regs = np.array([1.3, 0.8, 2.1, 0.6])
        self.var = 0.45
        self.mean1, self.ls1 = np.array([0.7, 0.0, -1.1]), np.array([0.9, 1.2, 1.5])
        self.ls_r = np.linspace(0.8, 1.4, 5)
        self.mean2, self.ls2 = np.array([-0.4]), np.array([1.1])
        self.x0 = np.concatenate([self.m.ravel(), self.C.ravel(), self.regs, [self.var], self.mean1, self.ls1, self.ls_r, self.mean2,
                                  self.ls2])
        fk, o = F * K, 2 * F * K + 5
        self.mean_slots = np.array([o, o + 1, o + 2, o + 11])           # plain space always: zero and negative values among them
        self.len_slots = np.array([o + 3, o + 4, o + 5, o + 6, o + 7, o + 8, o + 9, o + 10, o + 12])
        self.positive = np.concatenate([np.zeros(fk, dtype=bool), np.ones(self.x0.size - fk, dtype=bool)])
        self.positive[self.mean_slots] = False
        self.idx = np.stack([rs.permutation(self.N)[:self.M] for _ in range(4)]).astype(np.int32)
        self.e = rs.randn(4, K, self.L, F).astype(np.float32)

    def children(self, h1, hr, h2):
        """the child tuples of _hip.FusedSvi, each with its columns of X as a float64 host matrix (h1, hr, h2: RffHandles of V1,
        W, V2)"""
        X = self.X
        return [("linear", self.d, True, X), ("gm", h1, 6, np.ascontiguousarray(X[:, self.ind1])), ("rff", hr, 5, X),
                ("gm", h2, 2, np.ascontiguousarray(X[:, self.ind2]))]

    def elbo(self, x, idx, e):
        """oracle.glm_elbo at the flat x on rows idx with draws e (K, L, F): (-ELBO, gradient in x's layout)"""
        import revrand_oracle as orc
        F, K = self.F, self.K
        o = 2 * F * K
        m, C = x[:F * K].reshape(F, K), x[F * K:o].reshape(F, K)
        regs, var = x[o:o + 4], x[o + 4]
        mean1, ls1, ls_r, mean2, ls2 = x[o + 5:o + 8], x[o + 8:o + 11], x[o + 11:o + 16], x[o + 16:o + 17], x[o + 17:o + 18]
        Xb, yb = self.X[idx], self.y[idx]
        X1, X2 = Xb[:, self.ind1], Xb[:, self.ind2]
        Phi = np.hstack([orc.linear_transform(Xb, True), gm_transform(X1, self.V1, mean1, ls1), rff_transform(Xb, self.W, ls_r),
                         gm_transform(X2, self.V2, mean2, ls2)])
        assert Phi.shape == (len(idx), F)

        def slab(block, sl):
            out = np.zeros_like(Phi)
            out[:, sl] = block
            return out
        dm1, dl1 = gm_grad(X1, self.V1, mean1, ls1)
        dr = rff_grad(Xb, self.W, ls_r)
        dm2, dl2 = gm_grad(X2, self.V2, mean2, ls2)
        dPhis = [slab(dm1[:, :, i], self.slices[1]) for i in range(3)] + [slab(dl1[:, :, i], self.slices[1]) for i in range(3)]
        dPhis += [slab(dr[:, :, i], self.slices[2]) for i in range(5)]
        dPhis += [slab(dm2, self.slices[3]), slab(dl2, self.slices[3])]
        rd = np.concatenate([np.full(s.stop - s.start, r) for s, r in zip(self.slices, regs)])
        obj, (ndm, ndC, dL, dlp, dbp) = orc.glm_elbo(m, C, rd, self.slices, "gaussian", [var], (), Phi, dPhis, yb,
                                                     np.asarray(e, dtype=np.float64), self.B)
        return obj, np.concatenate([ndm.ravel(), ndC.ravel(), np.ravel(dL), np.ravel(dlp), np.ravel(dbp)])

    def blocks(self, v):
        """m, C, regularisers, variance, the four means, the nine length scales"""
        fk = self.F * self.K
        return v[:fk], v[fk:2 * fk], v[2 * fk:2 * fk + 4], v[2 * fk + 4:2 * fk + 5], v[self.mean_slots], v[self.len_slots]
