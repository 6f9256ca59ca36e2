"""CPU checks of the ResNet / PolyNet restatement (tests/net_ref.py) and of the bindings that name the new network kinds."""
import os

import numpy as np
import pytest

import net_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("fnn", "resnet", "polynet")
SMOOTH = ("identity", "tanh", "sigmoid", "swish")


def _points(n, m, k, seed):
    r = np.random.default_rng(seed)
    return r.normal(size=(k, n)), r.normal(size=(k, m))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("act", SMOOTH)
def test_jacobian_matches_central_differences(kind, act):
    f = net_ref.synthetic_net(kind, act=act)
    n, m = 4, 2
    h = 1e-6
    for x, u in zip(*_points(n, m, 4, 1)):
        A, B = f.jacobian(x, u)
        J = np.hstack([A, B])
        z = np.concatenate([x, u])
        Jd = np.empty_like(J)
        for c in range(n + m):
            e = np.zeros(n + m); e[c] = h
            Jd[:, c] = (f.forward(*np.split(z + e, [n])) - f.forward(*np.split(z - e, [n]))) / (2 * h)
        assert np.abs(J - Jd).max() <= 1e-7 * np.abs(J).max(), (kind, act)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("act", SMOOTH)
def test_stage_hessian_matches_central_differences(kind, act):
    """d/dz of the gradient J' lam (from the restated Jacobian) against net_ref.stage_hessian."""
    f = net_ref.synthetic_net(kind, act=act)
    n, m = 4, 2
    h = 1e-5
    lam = np.array([1.0, -0.5, 0.25, 2.0])
    for x, u in zip(*_points(n, m, 3, 2)):
        W = net_ref.stage_hessian(f, x, u, lam)
        z = np.concatenate([x, u])
        g = lambda zz: np.hstack(f.jacobian(*np.split(zz, [n]))).T @ lam
        Wd = np.empty_like(W)
        for c in range(n + m):
            e = np.zeros(n + m); e[c] = h
            Wd[:, c] = (g(z + e) - g(z - e)) / (2 * h)
        assert np.array_equal(W, W.T)
        assert np.abs(W - Wd).max() <= 1e-7 * max(np.abs(W).max(), 1e-300), (kind, act)


def test_the_kinds_differ_and_agree_at_no_hidden_layer():
    x, u = _points(4, 2, 1, 3)
    x, u = x[0], u[0]
    f = {k: net_ref.synthetic_net(k, act="tanh") for k in KINDS}
    g = {k: net_ref.as_kind(f["fnn"], k) for k in KINDS}
    assert not np.allclose(g["fnn"].forward(x, u), g["resnet"].forward(x, u))
    assert not np.allclose(g["resnet"].forward(x, u), g["polynet"].forward(x, u))
    z = {k: net_ref.as_kind(net_ref.synthetic_net("fnn", L=0, act="tanh"), k) for k in KINDS}
    for k in KINDS[1:]:
        assert np.array_equal(z[k].forward(x, u), z["fnn"].forward(x, u))
        for a, b in zip(z[k].jacobian(x, u), z["fnn"].jacobian(x, u)):
            assert np.array_equal(a, b)


def test_synthetic_net_has_the_spectral_radius_of_its_kind():
    for k in KINDS:
        A0, _ = net_ref.synthetic_net(k).jacobian(np.zeros(4), np.zeros(2))
        assert abs(np.max(np.abs(np.linalg.eigvals(A0))) - 0.95) <= 1e-12


def test_header_defines_the_network_codes():
    h = open(os.path.join(ROOT, "include", "almpc.h")).read()
    for name in ("ALMPC_NET_FNN 0", "ALMPC_NET_RESNET 1", "ALMPC_NET_POLYNET 2", "ALMPC_NET_CODE(kind, act) (((kind) << 8) | (act))"):
        assert "#define " + name in h, name


def test_bindings_name_the_kinds(pkg):
    assert pkg._capi.NET_KINDS == {"fnn", "resnet", "polynet"}
    assert pkg._capi.net_code("fnn", "tanh") == 2 and pkg._capi.net_code("polynet", "swish") == (2 << 8) | 4
    with pytest.raises(ValueError):
        pkg._capi.net_code("densenet", "tanh")
    for name in ("ResNet", "PolyNet", "Icnn"):
        assert name in pkg.controller.__all__ and issubclass(getattr(pkg, name), pkg.Fnn)


def test_mirror_dispatches_on_the_exact_model_type(pkg):
    """A subclass of Fnn is not an Fnn: the kind comes from the exact type, unknown families are refused with the reason."""
    kind = pkg.controller._net_kind
    W = np.zeros((2, 3))
    assert kind(pkg.Fnn(W, [], [], W)) == "fnn" and kind(pkg.Icnn(W, [], [], W)) == "fnn"
    assert kind(pkg.ResNet(W, [], [], W)) == "resnet" and kind(pkg.PolyNet(W, [], [], W)) == "polynet"

    class DenseNet(pkg.Fnn):
        pass

    class MyNet(pkg.Fnn):
        pass

    with pytest.raises(NotImplementedError, match="layer widths grow"):
        kind(DenseNet(W, [], [], W))
    with pytest.raises(NotImplementedError, match="MyNet"):
        kind(MyNet(W, [], [], W))


def test_julia_shim_and_reference_patch_name_the_kinds():
    shim = open(os.path.join(ROOT, "julia", "AlmpcHIP.jl")).read()
    assert ":resnet => 1" in shim and ":polynet => 2" in shim and "net_code(net, activation)" in shim
    patch = open(os.path.join(ROOT, "julia", "reference_hip.patch")).read()
    for t in ("AutomationLabsSystems.ResNet", "AutomationLabsSystems.PolyNet", "AutomationLabsSystems.Icnn", "_hip_net_kind"):
        assert t in patch, t
