"""CPU checks of the DenseNet restatement (tests/densenet_ref.py), of its packed ABI layout and of the bindings that expose the
almpc_*densenet* calls (header, _capi, controller, Julia shim)."""
import os
import re

import numpy as np
import pytest

import densenet_ref as dn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = ("identity", "relu", "tanh", "sigmoid", "swish")
SMOOTH = ("identity", "tanh", "sigmoid", "swish")
ENTRY_POINTS = ("almpc_densenet_linearize", "almpc_relin_densenet_setup", "almpc_sqp_densenet_setup",
                "almpc_group_relin_densenet_setup", "almpc_group_sqp_densenet_setup")


def _pre_activations(f, x, u):
    y = f.W_in @ np.concatenate([x, u])
    out = []
    for W, b in zip(f.W_h, f.b_h):
        a = W @ y + b
        out.append(a)
        y = np.concatenate([f._act(a)[0], y])
    return np.concatenate(out) if out else np.zeros(0)


def _points(f, n, m, k, seed, margin):
    """k points whose pre-activations all lie `margin` away from 0 (the relu kink)"""
    r = np.random.default_rng(seed)
    pts = []
    while len(pts) < k:
        x, u = r.normal(size=n), r.normal(size=m)
        if np.all(np.abs(_pre_activations(f, x, u)) > margin):
            pts.append((x, u))
    return pts


def _fd_jacobian(f, x, u, h):
    n, m = x.size, u.size
    z = np.concatenate([x, u])
    Jd = np.empty((n, n + m))
    for c in range(n + m):
        e = np.zeros(n + m); e[c] = h
        Jd[:, c] = (f.forward(*np.split(z + e, [n])) - f.forward(*np.split(z - e, [n]))) / (2 * h)
    return Jd


@pytest.mark.parametrize("L", [0, 1, 3])
@pytest.mark.parametrize("act", ACTS)
def test_jacobian_matches_central_differences(act, L):
    n, m = 4, 2
    f = dn.synthetic_densenet(n, m, H=8, L=L, act=act)
    for x, u in _points(f, n, m, 4, 1, 1e-3):
        A, B = f.jacobian(x, u)
        J = np.hstack([A, B])
        assert np.abs(J - _fd_jacobian(f, x, u, 1e-6)).max() <= 1e-7 * np.abs(J).max(), (act, L)


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("act", SMOOTH)
def test_stage_hessian_matches_central_differences(act, L):
    """d/dz of the gradient J' lam (from the restated Jacobian) against densenet_ref.stage_hessian."""
    n, m = 4, 2
    f = dn.synthetic_densenet(n, m, H=8, L=L, act=act)
    r = np.random.default_rng(3)
    h = 1e-5
    for _ in range(3):
        x, u, lam = r.normal(size=n), r.normal(size=m), r.normal(size=n)
        z = np.concatenate([x, u])
        g = lambda zz: np.hstack(f.jacobian(zz[:n], zz[n:])).T @ lam
        Wd = np.empty((n + m, n + m))
        for c in range(n + m):
            e = np.zeros(n + m); e[c] = h
            Wd[:, c] = (g(z + e) - g(z - e)) / (2 * h)
        W = dn.stage_hessian(f, x, u, lam)
        assert np.array_equal(W, W.T)
        assert np.abs(W - Wd).max() <= 1e-6 * max(1.0, np.abs(W).max()), (act, L)


def _jump_transcription(W_layer, B_layer, act, x, u):
    """The reference's JuMP constraints (.../densenet/mpc_modeler_implementation_densenet.jl:127-161) line by line, scalar by scalar:
    y_1[i] = W_layer[1][i, :]' [x; u];  y_j[i] = f(W_layer[j][i, :]' y_{j-1} + B_layer[j-1][i]), y_j[H+1:end] = y_{j-1};
    x+ = W_layer[end] y_{L+1}  (0-based lists here)."""
    fa = lambda a: dn.DenseNetModel(None, [], [], None, act)._act(np.array([a]))[0][0]
    H = W_layer[0].shape[0]
    nbr_hidden = len(B_layer)
    xu = np.concatenate([x, u])
    y = {1: np.array([W_layer[0][i, :] @ xu for i in range(H)])}
    for j in range(2, nbr_hidden + 2):
        yj = np.empty(j * H)
        for i in range(H):
            yj[i] = fa(W_layer[j - 1][i, :] @ y[j - 1] + B_layer[j - 2][i])
        yj[H:] = y[j - 1]
        y[j] = yj
    return W_layer[-1] @ y[nbr_hidden + 1]


@pytest.mark.parametrize("act", ACTS)
def test_concatenation_order_is_the_references(act):
    """The restatement is the reference's network, new features first; the same weights with the old block first are another
    network (the column blocks of every W_h[l] and of W_out differ, so the order is pinned)."""
    n, m, H, L = 3, 2, 5, 3
    f = dn.synthetic_densenet(n, m, H=H, L=L, act=act, seed=11)
    for l, W in enumerate(f.W_h):   # make the blocks distinct beyond doubt
        for k in range(l + 1):
            W[:, k * H:(k + 1) * H] *= 1.0 + 0.5 * k
    f.W_out[:, :H] *= 3.0
    W_layer = [f.W_in] + list(f.W_h) + [f.W_out]
    r = np.random.default_rng(5)
    for _ in range(4):
        x, u = r.normal(size=n), r.normal(size=m)
        ref = _jump_transcription(W_layer, f.b_h, act, x, u)
        assert np.abs(f.forward(x, u) - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())

        def old_first(x, u):   # y_{j+1} = [y_j; act(a)]: the order the kernels must NOT read
            y = f.W_in @ np.concatenate([x, u])
            for W, b in zip(f.W_h, f.b_h):
                y = np.concatenate([y, f._act(W @ y + b)[0]])
            return f.W_out @ y

        assert np.abs(old_first(x, u) - ref).max() > 1e-3 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("act", ACTS)
def test_no_hidden_layer_is_the_fnn(mo, act):
    f = dn.synthetic_densenet(4, 2, H=8, L=0, act=act)
    g = mo.FnnModel(f.W_in, [], [], f.W_out, act)
    x, u = np.array([0.3, -0.2, 0.5, 0.1]), np.array([0.4, -0.7])
    assert np.array_equal(f.forward(x, u), g.forward(x, u))
    for a, b in zip(f.jacobian(x, u), g.jacobian(x, u)):
        assert np.array_equal(a, b)


def test_packed_offsets_and_sizes():
    n, m, H, L = 4, 2, 3, 3
    f = dn.synthetic_densenet(n, m, H=H, L=L, act="tanh")
    W_in, W_h, b_h, W_out = dn.pack(f)
    assert W_in.size == H * (n + m) and b_h.size == L * H and W_out.size == n * (L + 1) * H
    assert W_h.size == H * H * L * (L + 1) // 2
    total = H * (n + m) + H * H * L * (L + 1) // 2 + L * H + n * (L + 1) * H   # the DESIGN.md / fnn_weights_doubles count
    assert W_in.size + W_h.size + b_h.size + W_out.size == total
    for l in range(L):
        off = H * H * l * (l + 1) // 2
        blk = W_h[off:off + H * (l + 1) * H].reshape((H, (l + 1) * H), order="F")
        assert np.array_equal(blk, f.W_h[l])
    assert np.array_equal(W_out.reshape((n, (L + 1) * H), order="F"), f.W_out)


def test_capi_packer_validates_every_shape(pkg):
    capi = pkg._capi
    f = dn.synthetic_densenet(4, 2, H=4, L=2, act="tanh")
    H, L, W_in, W_h, b_h, W_out = capi._pack_densenet(f.W_in, f.W_h, f.b_h, f.W_out, 4, 2)
    assert (H, L) == (4, 2) and W_in.flags.f_contiguous and W_out.flags.f_contiguous
    assert np.array_equal(W_h, np.concatenate(dn.pack(f)[1:2])) and np.array_equal(b_h.ravel(), dn.pack(f)[2])
    bad = [
        (f.W_in, [f.W_h[0], f.W_h[0]], f.b_h, f.W_out),               # second block H x H, not H x 2H
        (f.W_in, [f.W_h[1], f.W_h[0]], f.b_h, f.W_out),               # blocks swapped
        (f.W_in, f.W_h, f.b_h[:1], f.W_out),                          # one bias short
        (f.W_in, f.W_h, [f.b_h[0], np.zeros(5)], f.W_out),            # bias of the wrong length
        (f.W_in, f.W_h, f.b_h, f.W_out[:, :8]),                       # W_out n x 2H: an Fnn-sized output layer
        (f.W_in[:, :5], f.W_h, f.b_h, f.W_out),                       # W_in does not take n + m inputs
        (f.W_in, f.W_h, f.b_h, f.W_out[:3]),                          # W_out does not give n outputs
    ]
    for args in bad:
        with pytest.raises(ValueError):
            capi._pack_densenet(*args, 4, 2)
    with pytest.raises(ValueError):   # the same checks guard densenet_linearize before any device call
        capi.densenet_linearize(f.W_in, [f.W_h[0], f.W_h[0]], f.b_h, f.W_out, np.zeros((1, 4)), np.zeros((1, 2)))
    with pytest.raises(ValueError):
        capi.densenet_linearize(f.W_in, f.W_h, f.b_h, f.W_out, np.zeros((1, 4)), np.zeros((1, 2)), act="gelu")


def test_controller_dispatches_densenet_and_keeps_the_fnn_codes(pkg):
    kind = pkg.controller._net_kind
    W = np.zeros((2, 2))
    assert "DenseNet" in pkg.controller.__all__ and pkg.DenseNet is pkg.controller.DenseNet
    assert kind(pkg.DenseNet(W, [], [], W)) == "densenet"
    assert pkg._capi.NET_KINDS == {"fnn", "resnet", "polynet"}
    assert [pkg._capi.net_code(k, "tanh") for k in ("fnn", "resnet", "polynet")] == [2, 258, 514]
    with pytest.raises(ValueError):
        pkg._capi.net_code("densenet", "tanh")

    class DenseNet(pkg.Fnn):   # a user's Fnn subclass of that name is still refused, with the reason
        pass

    with pytest.raises(NotImplementedError, match="controller.DenseNet"):
        kind(DenseNet(W, [], [], W))


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "almpc.h")).read()
    for e in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % e, hdr), e
    assert "H^2 l (l+1) / 2" in hdr


def test_julia_shim_binds_the_entry_points():
    shim = open(os.path.join(ROOT, "julia", "AlmpcHIP.jl")).read()
    for e in ENTRY_POINTS:
        assert ":%s" % e in shim, e
    assert "net === :densenet" in shim and "densenet_pack" in shim
    patch = open(os.path.join(ROOT, "julia", "reference_hip.patch")).read()
    assert "almpc_group_sqp_densenet_setup" in patch   # the patch embeds the shim verbatim
