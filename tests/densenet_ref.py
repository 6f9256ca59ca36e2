"""Numpy restatement of the DenseNet model family (include/almpc.h, the almpc_*densenet* calls), test infrastructure.

The reference's network (.../densenet/mpc_modeler_implementation_densenet.jl:85-161), z = [x; u]:
    y_1 = W_in z,   y_{j+1} = [act(W_h[j-1] y_j + b_h[j-1]); y_j]  (new features first),   x+ = W_out y_{L+1}
W_h[l] is H x (l+1) H and W_out n x (L+1) H.  DenseNetModel overrides forward / jacobian only, so mpc_oracle.fnn_rollout, sqp_fnn,
nlp_kkt_residual, sqp_solve_ref and sqp_exact_ref work on it unchanged (substitute sqp_exact_ref.stage_hessian with stage_hessian
below).  Stage Hessian of lam' f: one activation site per hidden layer, M_j = W_h[j] J_j; the adjoint of y_{j+1} splits into the
new rows (the site's output) and the old ones, which collect W_h[j]' (act'(a_j) .* ybar_new)."""
import numpy as np

import mpc_oracle as mo
import sqp_exact_ref as ex


class DenseNetModel(mo.FnnModel):
    def forward(self, x, u):
        y = self.W_in @ np.concatenate([x, u])
        for W, b in zip(self.W_h, self.b_h):
            y = np.concatenate([self._act(W @ y + b)[0], y])
        return self.W_out @ y

    def jacobian(self, x, u):
        y = self.W_in @ np.concatenate([x, u])
        J = self.W_in.copy()
        for W, b in zip(self.W_h, self.b_h):
            v, d = self._act(W @ y + b)
            J = np.vstack([(W @ J) * d[:, None], J])
            y = np.concatenate([v, y])
        J = self.W_out @ J
        n = self.W_out.shape[0]
        return J[:, :n].copy(), J[:, n:].copy()


def stage_hessian(model, x, u, lam):
    """(n+m) x (n+m) Hessian of lam' f(x, u) (sqp_exact_ref.stage_hessian's signature); other kinds go to sqp_exact_ref."""
    if type(model) is not DenseNetModel:
        return ex.stage_hessian(model, x, u, lam)
    y = model.W_in @ np.concatenate([x, u])
    J = model.W_in.copy()
    sites = []
    for W, b in zip(model.W_h, model.b_h):
        a = W @ y + b
        M = W @ J
        v, d1, _ = ex.act2(model.act, a)
        sites.append((W, a, M))
        J = np.vstack([M * d1[:, None], J])
        y = np.concatenate([v, y])
    H = model.W_in.shape[0]
    yb = model.W_out.T @ lam
    Wz = np.zeros((J.shape[1], J.shape[1]))
    for W, a, M in reversed(sites):
        _, d1, d2 = ex.act2(model.act, a)
        new, old = yb[:H], yb[H:]
        Wz += M.T @ ((new * d2)[:, None] * M)
        yb = old + W.T @ (new * d1)
    return 0.5 * (Wz + Wz.T)


def evaluate_points(model, X, U, dtype=np.longdouble):
    """net_ref.evaluate_points for a DenseNet: (A (p, n, n), B (p, n, m), f (p, n)) at X (p, n), U (p, m), every operation in `dtype`."""
    import net_ref
    if type(model) is not DenseNetModel:
        return net_ref.evaluate_points(model, X, U, dtype)
    c = lambda w: np.asarray(w, dtype=dtype)
    Z = np.concatenate([c(X), c(U)], axis=1)
    W_in, W_out = c(model.W_in), c(model.W_out)
    y = Z @ W_in.T
    J = np.broadcast_to(W_in, (Z.shape[0],) + W_in.shape).copy()
    for W, b in zip(model.W_h, model.b_h):
        W, b = c(W), c(b)
        v, d = net_ref.act_any(model.act, y @ W.T + b)
        J = np.concatenate([np.einsum("ij,pjc->pic", W, J) * d[:, :, None], J], axis=1)
        y = np.concatenate([v, y], axis=1)
    Jo = np.einsum("ij,pjc->pic", W_out, J)
    n = W_out.shape[0]
    return Jo[:, :, :n], Jo[:, :, n:], y @ W_out.T


def synthetic_densenet(n=4, m=2, H=16, L=2, seed=0x5EED0004, act="relu"):
    """Weights ~ U(-1, 1) / sqrt(fan_in) (biases 0.1 U(-1, 1)), W_out rescaled so that A at the origin has spectral radius 0.95, as
    net_ref.synthetic_net does."""
    r = np.random.default_rng(seed)
    uni = lambda shape, fan_in: (2.0 * r.random(shape) - 1.0) / np.sqrt(fan_in)
    W_in = uni((H, n + m), n + m)
    W_h = [uni((H, (l + 1) * H), (l + 1) * H) for l in range(L)]
    b_h = [0.1 * (2.0 * r.random(H) - 1.0) for _ in range(L)]
    W_out = uni((n, (L + 1) * H), (L + 1) * H)
    f = DenseNetModel(W_in, W_h, b_h, W_out, act)
    A0, _ = f.jacobian(np.zeros(n), np.zeros(m))
    f.W_out = W_out * (0.95 / max(1e-12, float(np.max(np.abs(np.linalg.eigvals(A0))))))
    return f


def pack(model):
    """The ABI buffers of include/almpc.h, flat in memory order: W_in, W_h (block l H x (l+1) H at H^2 l (l+1) / 2), b_h [L][H],
    W_out, all column-major."""
    W_h = np.concatenate([w.ravel(order="F") for w in model.W_h]) if model.W_h else np.zeros(0)
    b_h = np.concatenate(model.b_h) if model.b_h else np.zeros(0)
    return model.W_in.ravel(order="F"), W_h, b_h, model.W_out.ravel(order="F")
