"""Numpy restatement of the ResNet and PolyNet model families (include/almpc.h ALMPC_NET_*), test infrastructure.

Both use the Fnn weight layout (mpc_oracle.FnnModel: y_1 = W_in z, x+ = W_out y_{L+1}, z = [x; u]) and differ in the hidden layer:
    ResNet   y_{j+1} = y_j + act(W_j y_j + b_j)
    PolyNet  p_j = act(W_j y_j + b_j),  y_{j+1} = y_j + p_j + act(W_j p_j + b_j)     (the same W_j, b_j twice)
The models override forward / jacobian only, so mpc_oracle.fnn_rollout, sqp_fnn, nlp_kkt_residual, sqp_solve_ref and
sqp_exact_ref work on them unchanged; sqp_exact_ref.exact_qp looks stage_hessian up at call time (substitute it with
stage_hessian below).
Stage Hessian of lam' f: the sum over activation sites s of M_s' diag(abar_s act''(a_s)) M_s, M_s = d a_s / d z, abar_s the adjoint
of the site's output."""
import numpy as np

import mpc_oracle as mo
import sqp_exact_ref as ex


class ResNetModel(mo.FnnModel):
    def forward(self, x, u):
        y = self.W_in @ np.concatenate([x, u])
        for W, b in zip(self.W_h, self.b_h):
            y = y + self._act(W @ y + b)[0]
        return self.W_out @ y

    def jacobian(self, x, u):
        y = self.W_in @ np.concatenate([x, u])
        J = self.W_in.copy()
        for W, b in zip(self.W_h, self.b_h):
            v, d = self._act(W @ y + b)
            J = J + (W @ J) * d[:, None]
            y = y + v
        J = self.W_out @ J
        n = self.W_out.shape[0]
        return J[:, :n].copy(), J[:, n:].copy()


class PolyNetModel(mo.FnnModel):
    def forward(self, x, u):
        y = self.W_in @ np.concatenate([x, u])
        for W, b in zip(self.W_h, self.b_h):
            p = self._act(W @ y + b)[0]
            y = y + p + self._act(W @ p + b)[0]
        return self.W_out @ y

    def jacobian(self, x, u):
        y = self.W_in @ np.concatenate([x, u])
        J = self.W_in.copy()
        for W, b in zip(self.W_h, self.b_h):
            p, d1 = self._act(W @ y + b)
            P = (W @ J) * d1[:, None]
            v2, d2 = self._act(W @ p + b)
            J = J + P + (W @ P) * d2[:, None]
            y = y + p + v2
        J = self.W_out @ J
        n = self.W_out.shape[0]
        return J[:, :n].copy(), J[:, n:].copy()


MODELS = {"fnn": mo.FnnModel, "resnet": ResNetModel, "polynet": PolyNetModel}


def _resnet_hessian(model, z, lam):
    y, J = model.W_in @ z, model.W_in.copy()
    sites = []
    for W, b in zip(model.W_h, model.b_h):
        a = W @ y + b
        M = W @ J
        v, d1, _ = ex.act2(model.act, a)
        sites.append((W, a, M))
        J = J + M * d1[:, None]
        y = y + v
    yb = model.W_out.T @ lam
    Wz = np.zeros((z.size, z.size))
    for W, a, M in reversed(sites):
        _, d1, d2 = ex.act2(model.act, a)
        Wz += M.T @ ((yb * d2)[:, None] * M)
        yb = yb + W.T @ (yb * d1)
    return Wz


def _polynet_hessian(model, z, lam):
    y, J = model.W_in @ z, model.W_in.copy()
    layers = []
    for W, b in zip(model.W_h, model.b_h):
        a1 = W @ y + b
        M1 = W @ J
        p, d1, _ = ex.act2(model.act, a1)
        P = M1 * d1[:, None]
        a2 = W @ p + b
        M2 = W @ P
        v2, e1, _ = ex.act2(model.act, a2)
        layers.append((W, a1, M1, a2, M2))
        J = J + P + M2 * e1[:, None]
        y = y + p + v2
    yb = model.W_out.T @ lam
    Wz = np.zeros((z.size, z.size))
    for W, a1, M1, a2, M2 in reversed(layers):
        _, e1, e2 = ex.act2(model.act, a2)
        Wz += M2.T @ ((yb * e2)[:, None] * M2)
        pb = yb + W.T @ (yb * e1)
        _, d1, d2 = ex.act2(model.act, a1)
        Wz += M1.T @ ((pb * d2)[:, None] * M1)
        yb = yb + W.T @ (pb * d1)
    return Wz


def stage_hessian(model, x, u, lam):
    """(n+m) x (n+m) Hessian of lam' f(x, u) for any of the three kinds (sqp_exact_ref.stage_hessian's signature)."""
    if type(model) is ResNetModel:
        Wz = _resnet_hessian(model, np.concatenate([x, u]), lam)
    elif type(model) is PolyNetModel:
        Wz = _polynet_hessian(model, np.concatenate([x, u]), lam)
    else:
        return ex.stage_hessian(model, x, u, lam)
    return 0.5 * (Wz + Wz.T)


def act_any(act, a):
    """value and derivative of the activation in the array's own precision (FnnModel._act for any float type)"""
    one = a.dtype.type(1)
    if act == "relu":
        return np.maximum(a, 0), (a > 0).astype(a.dtype)
    if act == "tanh":
        t = np.tanh(a)
        return t, one - t * t
    if act in ("sigmoid", "swish"):
        s = one / (one + np.exp(-a))
        return (s, s * (one - s)) if act == "sigmoid" else (a * s, s * (one + a * (one - s)))
    if act == "identity":
        return a, np.ones_like(a)
    raise ValueError(act)


def evaluate_points(model, X, U, dtype=np.longdouble):
    """(A (p, n, n), B (p, n, m), f (p, n)) of an Fnn, ResNet or PolyNet at the points X (p, n), U (p, m), every operation in `dtype`:
    numpy long double (the yardstick of the float64 restatement) or float64 (the restatement itself, over all points at once)."""
    c = lambda w: np.asarray(w, dtype=dtype)
    Z = np.concatenate([c(X), c(U)], axis=1)
    W_in, W_out = c(model.W_in), c(model.W_out)
    y = Z @ W_in.T
    J = np.broadcast_to(W_in, (Z.shape[0],) + W_in.shape).copy()
    for W, b in zip(model.W_h, model.b_h):
        W, b = c(W), c(b)
        v, d = act_any(model.act, y @ W.T + b)
        WJ = np.einsum("ij,pjc->pic", W, J) * d[:, :, None]
        if type(model) is ResNetModel:
            J, y = J + WJ, y + v
        elif type(model) is PolyNetModel:
            v2, d2 = act_any(model.act, v @ W.T + b)
            J, y = J + WJ + np.einsum("ij,pjc->pic", W, WJ) * d2[:, :, None], y + v + v2
        elif type(model) is mo.FnnModel:
            J, y = WJ, v
        else:
            raise TypeError(type(model))
    Jo = np.einsum("ij,pjc->pic", W_out, J)
    n = W_out.shape[0]
    return Jo[:, :, :n], Jo[:, :, n:], y @ W_out.T


def as_kind(f, kind):
    """The same weights as a model of another kind (no rescaling)."""
    return MODELS[kind](f.W_in.copy(), [w.copy() for w in f.W_h], [b.copy() for b in f.b_h], f.W_out.copy(), f.act)


def synthetic_net(kind, n=4, m=2, H=16, L=2, seed=0x5EED0004, act="relu"):
    """The weights of mo.synthetic_fnn, with W_out rescaled so that the Jacobian at the origin has spectral radius 0.95 for this kind."""
    f = as_kind(mo.synthetic_fnn(n=n, m=m, H=H, L=L, seed=seed, act=act), kind)
    A0, _ = f.jacobian(np.zeros(n), np.zeros(m))
    f.W_out = f.W_out * (0.95 / max(1e-12, float(np.max(np.abs(np.linalg.eigvals(A0))))))
    return f
