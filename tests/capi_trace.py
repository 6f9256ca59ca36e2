"""A recording stand-in for libalmpc.so and a script of calls that drives the whole Python binding through it.

`trace(capi)` installs the stand-in as `capi._lib`, runs the script and returns the lines of tests/golden/capi_calls.txt: one line
per C call the binding makes (symbol, every scalar, and for every pointer NULL or dtype and byte count, plus a hash of the bytes if
include/almpc.h declares the parameter const) and one per wrapper call (what it returned: dtype, shape, strides and content hash of
every array; or the exception type).  No GPU and no library are needed.

    python tests/capi_trace.py            # print the trace of the binding in the tree
    python tests/capi_trace.py --write    # ... and store it as the golden file (only ever from a binding known to be right)
"""
import ctypes
import hashlib
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_calls.txt")

# non-const parameters whose content the library reads before it writes (slots of failed instances keep what the caller put there)
IN_OUT = {("almpc_dare_batched", "P_batch"), ("almpc_c2d_batched", "Ad_batch"), ("almpc_c2d_batched", "Bd_batch"),
          ("almpc_dare_vjp_batched", "gA_batch"), ("almpc_dare_vjp_batched", "gB_batch"), ("almpc_dare_vjp_batched", "gQ_batch"),
          ("almpc_dare_vjp_batched", "gR_batch")}


def header_text():
    src = open(os.path.join(ROOT, "include", "almpc.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


def declarations():
    """{symbol: (return type, [(type, name), ...])} of every function include/almpc.h declares; a type is its tokens joined by one
    blank with every '*' a token of its own ("const double *")."""
    out = {}
    for ret, name, params in re.findall(r"\b(void|int|const\s+char\s*\*|almpc_handle\s*\*)\s*(almpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_text()):
        plist = []
        for p in params.split(","):
            toks = p.replace("*", " * ").split()
            if toks == ["void"] or not toks:
                continue
            plist.append((" ".join(toks[:-1]), toks[-1]))
        out[name] = (" ".join(ret.replace("*", " * ").split()), plist)
    return out


def _h(data):
    return hashlib.sha1(bytes(data)).hexdigest()[:12]


def _addr(p):
    return ctypes.cast(p, ctypes.c_void_p).value


_DT = {"float64": "f8", "int32": "i4", "float32": "f4"}


class _Fn:
    def __init__(self, lib, name):
        self.lib, self.name = lib, name
        self.argtypes, self.restype = None, ctypes.c_int   # the binding may declare prototypes on the stand-in as on a CDLL

    def __call__(self, *args):
        return self.lib.call(self.name, args)


class RecordingLib:
    """Stands in for the ctypes.CDLL of libalmpc.so."""

    def __init__(self, log):
        self.log = log
        self.decl = declarations()
        self.dims = {}        # handle value -> (kind "H" / "G", label, n, m, N, batch)
        self.shards = {}      # group value -> [(first, count, handle value)]
        self.tickets = {}     # ticket -> want mask
        self.next_ticket = 0
        self.next_handle = 0x1000
        self.fail_next = 0    # the next call that returns a status returns this one
        self.keep = []        # scratch buffers handed out by pointer
        self._fns = {}

    def __getattr__(self, name):
        if not name.startswith("almpc_"):
            raise AttributeError(name)
        if name not in self.decl:
            raise AttributeError(f"{name}: include/almpc.h declares no such function")
        return self._fns.setdefault(name, _Fn(self, name))

    # ---- the record
    def _new_handle(self, kind, n, m, N, batch):
        v = self.next_handle
        self.next_handle += 0x100
        self.dims[v] = (kind, f"{kind}{sum(1 for d in self.dims.values() if d[0] == kind)}", n, m, N, batch)
        return v

    def _scratch(self, count, ctype, base):
        buf = np.arange(base, base + count).astype(np.float64 if ctype is ctypes.c_double else np.int32)
        self.keep.append(buf)
        return buf.ctypes.data

    def _fill(self, a, pos):
        """the element index (in memory order) plus 1000 times the argument's position, into the bytes `a` addresses"""
        flat = np.ctypeslib.as_array(ctypes.cast(a.ctypes.data, ctypes.POINTER(np.ctypeslib.as_ctypes_type(a.dtype))), shape=(a.size,))
        flat[:] = np.arange(a.size) + 1000 * pos

    def _pointer(self, name, pos, ptype, pname, a):
        const = ptype.startswith("const")
        if a is None:
            return "NULL"
        if isinstance(a, bytes):
            return f"bytes[{len(a)}]:{_h(a)}"
        if hasattr(a, "_arr"):                      # array.ctypes.data_as(...): the array rides along
            arr = a._arr
            want = {"double": "float64", "int32_t": "int32", "float": "float32", "int": "int32"}.get(ptype.replace("const", "").replace("*", "").strip())
            text = f"{_DT.get(arr.dtype.name, arr.dtype.name)}[{arr.nbytes}]"
            if arr.dtype.name != want or _addr(a) != arr.ctypes.data:
                text += "!dtype"
            if not (arr.flags.c_contiguous or arr.flags.f_contiguous):
                text += "!strided"
            if const or (name, pname) in IN_OUT:
                text += ":" + _h(ctypes.string_at(arr.ctypes.data, arr.nbytes))
            if not const:
                self._fill(arr, pos)
            return text
        if hasattr(a, "_obj"):                      # ctypes.byref(x)
            a = a._obj
        if isinstance(a, ctypes.Structure):
            text = f"{type(a).__name__}[{ctypes.sizeof(a)}]"
            if const and type(a).__name__ == "almpc_opts":      # (almpc_param_grads holds addresses: _param_grads below records it)
                text += ":" + _h(ctypes.string_at(ctypes.addressof(a), ctypes.sizeof(a)))
            return text
        if isinstance(a, ctypes.Array):
            text = f"{a._type_.__name__}[{len(a)}]"
            return text + ":" + _h(ctypes.string_at(ctypes.addressof(a), ctypes.sizeof(a))) if const else text
        if isinstance(a, ctypes.c_void_p) and const and ptype.count("*") == 1:
            return f"address:{a.value:#x}"          # a device pointer of the caller's
        return type(a).__name__

    def call(self, name, args):
        ret, params = self.decl[name]
        if len(args) != len(params):
            self.log.append(f"C {name}: {len(args)} arguments for {len(params)} parameters")
            raise TypeError(f"{name}: {len(args)} arguments for {len(params)} parameters")
        parts = []
        for pos, ((ptype, pname), a) in enumerate(zip(params, args)):
            base = ptype.replace("const", "").strip()
            if base in ("almpc_handle *", "almpc_group *"):
                v = a.value if hasattr(a, "value") else a
                parts.append(f"{pname}=" + ("NULL" if not v else self.dims[v][1]))
            elif "*" in ptype:
                parts.append(f"{pname}={self._pointer(name, pos, ptype, pname, a)}")
            elif base == "double":
                if not isinstance(a, float):
                    raise TypeError(f"{name}: {pname} is not a float")
                parts.append(f"{pname}={a!r}")
            else:
                if not isinstance(a, int) or isinstance(a, bool):
                    raise TypeError(f"{name}: {pname} is not an int")
                parts.append(f"{pname}={a}")
        self.log.append(f"C {name}({', '.join(parts)})")
        if ret == "int" and self.fail_next:
            rc, self.fail_next = self.fail_next, 0
            return rc
        do = getattr(self, "_do_" + name[6:], None)
        if do is None and ret != "int":
            raise NotImplementedError(f"the stand-in has no {name}")
        return do(*args) if do else 0

    # ---- what the wrappers read back
    def _do_default_opts(self, o):
        o = o._obj
        o.rho, o.sigma, o.alpha, o.eps_abs, o.eps_rel = 0.1, 1e-6, 1.6, 1e-3, 1e-3
        o.max_iter, o.check_every, o.polish, o.polish_max_iter, o.warm_start = 25, 25, 1, 0, 0

    def _do_destroy(self, h):
        pass

    _do_group_destroy = _do_destroy

    def _do_last_error(self, h):
        return b"the stand-in's error text"

    _do_group_last_error = _do_last_error

    def _do_create(self, out, n, m, N, batch, device, flags):
        out._obj.value = self._new_handle("H", n, m, N, batch)
        return 0

    def _do_group_create(self, out, n, m, N, batch, k, devs, flags):
        g = self._new_handle("G", n, m, N, batch)
        sh, first = [], 0
        for i in range(k):
            cnt = batch // k + (1 if i < batch % k else 0)
            sh.append((first, cnt, self._new_handle("H", n, m, N, cnt)))
            first += cnt
        self.shards[g] = sh
        out._obj.value = g
        return 0

    def _do_group_size(self, g):
        return len(self.shards[g.value])

    def _do_group_handle(self, g, i):
        return self.shards[g.value][i][2]

    def _do_group_shard(self, g, i, first, count):
        first._obj.value, count._obj.value = self.shards[g.value][i][:2]
        return 0

    def _do_x0_staging(self, h, slot):
        _, _, n, m, N, b = self.dims[h.value]
        slot._obj.contents = ctypes.c_double.from_address(self._scratch(b * n, ctypes.c_double, 500))
        return 0

    def _do_group_x0_staging(self, g, slots):
        n = self.dims[g.value][2]
        for i, (_, cnt, _) in enumerate(self.shards[g.value]):
            slots[i] = ctypes.cast(self._scratch(cnt * n, ctypes.c_double, 600 + 100 * i), ctypes.POINTER(ctypes.c_double))
        return 0

    def _do_get_results_async(self, h, want):
        t = self.next_ticket
        self.next_ticket += 1
        self.tickets[t] = want
        return t

    _do_group_get_results_async = _do_get_results_async

    def _do_host_results(self, h, ticket, *outs):
        _, _, n, m, N, b = self.dims[h.value]
        sizes = (b * (N + 1) * n, b * (N + 1) * n, b * N * m, b * N * m, b * m, b, b, b)
        bits = (0x01, 0x02, 0x04, 0x08, 0x80, 0x10, 0x20, 0x40)   # ALMPC_WANT_* of the arguments: u0 comes fifth but is the last bit
        for i, (o, sz) in enumerate(zip(outs, sizes)):
            if self.tickets[ticket] & bits[i]:
                o._obj.value = self._scratch(sz, ctypes.c_double if i < 5 else ctypes.c_int32, 1000 * (i + 2))
        return 0

    def _views(self, outs):
        for i, o in enumerate(outs):
            o._obj.value = 0xD000 + 0x100 * i
        return 0

    def _do_device_results(self, h, *outs):
        return self._views(outs)

    _do_device_sensitivity = _do_device_certificate = _do_device_certificate_ltv = _do_device_results

    def _scalars(self, outs, base):
        for i, o in enumerate(outs):
            o._obj.value = base + i
        return 0

    def _do_get_timing(self, h, *outs):
        return self._scalars(outs, 0.5)

    def _do_relin_fnn_timing(self, h, *outs):
        return self._scalars(outs, 0.25)

    def _do_timing_summary(self, h, steps, *outs):
        steps._obj.value = 17
        return self._scalars(outs, 1.5)

    def _do_timing_samples(self, h, cap, count, *outs):
        count._obj.value = 3
        return 0

    def _do_comm_summary(self, h, out4):
        out4[:] = [2, 1, 30, 4]
        return 0

    def _do_comm_unique_id(self, buf):
        buf.raw = bytes(range(128))
        return 0

    def _param_grads(self, h, out):
        """almpc_param_grads holds bare pointers: the sizes are the header's"""
        _, _, n, m, N, b = self.dims[h.value]
        sizes = dict(x0=b * n, f=b * N * m, u_ref=b * N * m, u_min=b * m, u_max=b * m, Q=b * n * n, P=b * n * n, A=b * n * n,
                     R=b * m * m, S=b * m * m, B=b * n * m)
        out = out._obj
        first = min(_addr(getattr(out, k)) for k in sizes if getattr(out, k))
        for i, (k, sz) in enumerate(sizes.items()):
            p = getattr(out, k)
            if p:
                np.ctypeslib.as_array(p, shape=(sz,))[:] = np.arange(sz) + 1000 * i
        np.ctypeslib.as_array(out.rows, shape=(b,))[:] = np.arange(b) + 7
        self.log[-1] += " grads{" + ", ".join(f"{k}@{_addr(getattr(out, k)) - first}" for k in sizes if getattr(out, k)) + "}"
        return 0

    def _do_sensitivity_params_vjp(self, h, gu, gx, tol, out, *rest):
        return self._param_grads(h, out)

    _do_group_sensitivity_params_vjp = _do_sensitivity_params_vjp_dare = _do_group_sensitivity_params_vjp_dare = _do_sensitivity_params_vjp


def describe(v):
    """one token for what a wrapper returned"""
    if v is None or isinstance(v, (bool, int, str)):
        return repr(v)
    if isinstance(v, float):
        return repr(v)
    if isinstance(v, bytes):
        return f"bytes[{len(v)}]:{_h(v)}"
    if isinstance(v, np.ndarray):
        return f"{v.dtype.name}{list(v.shape)}/{list(v.strides)}:{_h(np.ascontiguousarray(v).tobytes())}"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {describe(v[k])}" for k in sorted(v)) + "}"     # (some are built from a set: no order to pin)
    if isinstance(v, (tuple, list)):
        return ("(%s)" if isinstance(v, tuple) else "[%s]") % ", ".join(describe(x) for x in v)
    if isinstance(v, ctypes.Structure):
        return f"{type(v).__name__}:{_h(ctypes.string_at(ctypes.addressof(v), ctypes.sizeof(v)))}"
    return type(v).__name__


def script(capi, lib, log):
    """Every public function and every method of Solver and Group, with every optional-argument branch.  No two extents are equal."""
    n, m, N, b, H = 3, 2, 4, 7, 6
    rng = np.random.default_rng(20240229)
    r = lambda *shape: rng.standard_normal(shape)

    def do(label, fn, *a, **kw):
        log.append(f"> {label}")
        try:
            out = fn(*a, **kw)
        except Exception as e:      # the trace pins which exception
            log.append(f"! {type(e).__name__}")
            return None
        log.append(f"< {describe(out)}")
        return out

    # ---- module functions
    do("default_opts", capi.default_opts)
    opts = do("default_opts fields", capi.default_opts, max_iter=40, warm_start=1, keep_warm_state=False)
    do("default_opts keep", capi.default_opts, keep_warm_state=True)
    do("default_opts unknown", capi.default_opts, no_such=1)
    do("comm_unique_id", capi.comm_unique_id)
    lib.fail_next = -3
    do("comm_unique_id fails", capi.comm_unique_id)
    A, B, Q, R, S, P = r(n, n), r(n, m), r(n, n), r(m, m), r(m, m), r(n, n)
    Ab, Bb, Qb, Rb, Sb, Pb = r(b, n, n), r(b, n, m), r(b, n, n), r(b, m, m), r(b, m, m), r(b, n, n)
    umin, umax, xmin, xmax = r(m), r(m), r(n), r(n)
    do("dare", capi.dare, A, B, Q, R)
    do("dare bad Q", capi.dare, A, B, r(m, m), R)
    lib.fail_next = -6
    do("dare fails", capi.dare, A, B, Q, R)
    do("dare_vjp", capi.dare_vjp, A, B, Q, R, P, r(n, n))
    do("dare_vjp subset", capi.dare_vjp, A, B, Q, R, P, r(n, n), want=("B", "Q"))
    lib.fail_next = -6
    do("dare_vjp fails", capi.dare_vjp, A, B, Q, R, P, r(n, n))
    do("dare_batched", capi.dare_batched, Ab, Bb, Q, R)
    do("dare_batched init", capi.dare_batched, Ab, Bb, Q, R, device=1, P_init=Pb)
    do("dare_batched bad", capi.dare_batched, Ab, Bb[:-1], Q, R)
    init = {"A": r(b, n, n), "B": r(b, n, m), "R": r(b, m, m)}
    do("dare_vjp_batched", capi.dare_vjp_batched, Ab, Bb, Q, R, Pb, r(b, n, n))
    do("dare_vjp_batched init", capi.dare_vjp_batched, Ab, Bb, Q, R, Pb, r(b, n, n), device=1, want=("A", "B", "R"), init=init)
    do("dare_vjp_batched bad", capi.dare_vjp_batched, Ab, Bb, Q, R, Pb[:-1], r(b, n, n))
    do("c2d", capi.c2d, A, B, 0.05)
    do("c2d vector B", capi.c2d, A, r(n), 0.05)
    do("c2d_batched", capi.c2d_batched, Ab, Bb, 0.05)
    do("c2d_batched init", capi.c2d_batched, Ab, Bb, 0.05, device=1, out_init=(r(b, n, n), r(b, n, m)))
    do("c2d_batched bad", capi.c2d_batched, Ab, Bb.transpose(0, 2, 1), 0.05)
    for net, act in (("fnn", "relu"), ("resnet", "tanh"), ("polynet", "swish"), ("gru", "relu")):
        do(f"net_code {net}", capi.net_code, net, act)
    nets = {0: (r(H, n + m), [], [], r(n, H)), 2: (r(H, n + m), [r(H, H), r(H, H)], [r(H), r(H)], r(n, H))}
    dense = (r(H, n + m), [r(H, H), r(H, 2 * H)], [r(H), r(H)], r(n, 3 * H))
    dense_bad = (dense[0], [r(H, H), r(H, H)], dense[2], dense[3])
    x, u = r(b, n), r(b, m)
    for L_, w in nets.items():
        do(f"fnn_linearize L={L_}", capi.fnn_linearize, *w, x, u)
        do(f"fnn_linearize L={L_} f", capi.fnn_linearize, *w, x, u, act="tanh", device=1, want_f=True, net="resnet")
    do("fnn_linearize bad net", capi.fnn_linearize, *nets[2], x, u, net="gru")
    do("fnn_linearize one point", capi.fnn_linearize, *nets[2], x[0], u[0])
    do("densenet_linearize", capi.densenet_linearize, *dense, x, u)
    do("densenet_linearize f", capi.densenet_linearize, *dense, x, u, act="sigmoid", device=1, want_f=True)
    do("densenet_linearize bad block", capi.densenet_linearize, *dense_bad, x, u)
    do("densenet_linearize bad act", capi.densenet_linearize, *dense, x, u, act="gelu")
    do("densenet_linearize L=0", capi.densenet_linearize, dense[0], [], [], r(n, H), x, u)
    do("multipliers", capi.multipliers, r(b, m, N), np.clip(r(b, m, N), -1, 1), -np.ones(m), np.ones(m))

    # ---- what Solver and Group both have (the group's devices all 0)
    def make(kind, **kw):
        if kind == "solver":
            return do(f"Solver {kw}", capi.Solver, n, m, N, b, **kw)
        return do(f"Group {kw}", capi.Group, n, m, N, b, [0, 0, 0], **kw)

    xr, ur = r(n, N + 1), r(m, N)
    gu, gx = r(b, m, N), r(b, n, N + 1)
    for kind in ("solver", "group"):
        make(kind, timing=True, structured=True, structured_fallback=True)
        make(kind, structured_fallback=False)
        lib.fail_next = -2
        make(kind)
        s = make(kind, device=1) if kind == "solver" else make(kind)
        t = lambda label, name, *a, **kw: do(f"{kind}.{name} {label}", getattr(s, name), *a, **kw)
        lib.fail_next = -5
        t("fails", "synchronize")
        t("", "design_shared", A, B, Q, R, umin=umin, umax=umax)
        t("all", "design_shared", A, B, Q, R, S=S, P=P, umin=umin, umax=umax, xmin=xmin, xmax=xmax, rho=0.3, sigma=1e-5,
          terminal="equality", rho_profile="stiffness")
        t("xmin only", "design_shared", A, B, Q, R, umin=umin, umax=umax, xmin=xmin)
        t("bad terminal", "design_shared", A, B, Q, R, umin=umin, umax=umax, terminal="soft")
        t("bad profile", "design_shared", A, B, Q, R, umin=umin, umax=umax, rho_profile="vector")
        t("bad A", "design_shared", B, B, Q, R, umin=umin, umax=umax)
        for name, w in (("design_batched", (Ab, Bb, Q, R)), ("design_batched_weighted", (Ab, Bb, Qb, Rb))):
            Sarg = {"S": S} if name == "design_batched" else {"S_batch": Sb}
            t("", name, *w, umin=umin, umax=umax)
            t("shared P", name, *w, **Sarg, P=P, umin=umin, umax=umax, rho=0.3, sigma=1e-5, rho_profile="stiffness", xmin=xmin, xmax=xmax,
              terminal="equality")
            t("P per instance", name, *w, P=Pb, umin=umin, umax=umax)
            t("xmax only", name, *w, umin=umin, umax=umax, xmax=xmax)
            t("bad terminal", name, *w, umin=umin, umax=umax, terminal="soft")
            t("bad profile", name, *w, umin=umin, umax=umax, rho_profile="vector")
            t("bad P", name, *w, P=r(m, m), umin=umin, umax=umax)
        for setup in ("sqp_fnn_setup", "relin_fnn_setup"):
            sqp = setup.startswith("sqp")
            for L_, w in nets.items():
                t(f"L={L_}", setup, *w, xr, ur, Q, R, P=P, umin=umin, umax=umax)
                t(f"L={L_} no refs", setup, *w, None, None, Q, R, P=P, umin=umin, umax=umax)
            w = nets[2]
            kw = dict(S=S, P=P, umin=umin, umax=umax, act="tanh", rho=0.3, sigma=1e-5, rho_profile="stiffness", xmin=xmin, xmax=xmax,
                      terminal="equality")
            t("all", setup, *w, xr, ur, Q, R, net="resnet", **(dict(kw, qp_solver="structured") if sqp else kw))
            t("polynet", setup, *w, xr, ur, Q, R, P=P, umin=umin, umax=umax, net="polynet")
            t("bad net", setup, *w, xr, ur, Q, R, P=P, umin=umin, umax=umax, net="gru")
            t("xmin only", setup, *w, xr, ur, Q, R, P=P, umin=umin, umax=umax, xmin=xmin)
            t("bad profile", setup, *w, xr, ur, Q, R, P=P, umin=umin, umax=umax, rho_profile="vector")
            t("P per instance", setup, *w, xr, ur, Q, R, P=Pb, umin=umin, umax=umax)
            dsetup = setup.replace("fnn", "densenet")
            t("", dsetup, *dense, xr, ur, Q, R, P=P, umin=umin, umax=umax)
            t("no refs", dsetup, *dense, None, None, Q, R, P=P, umin=umin, umax=umax)
            t("all", dsetup, *dense, xr, ur, Q, R, **dict(dict(kw, qp_solver="structured") if sqp else kw, act="sigmoid"))
            t("bad block", dsetup, *dense_bad, xr, ur, Q, R, P=P, umin=umin, umax=umax)
            t("bad act", dsetup, *dense, xr, ur, Q, R, P=P, umin=umin, umax=umax, act="gelu")
            t("P per instance", dsetup, *dense, xr, ur, Q, R, P=Pb, umin=umin, umax=umax)
        for sync in (True, False):
            t(f"sync={sync}", "relin_fnn_step", sync=sync)
            t(f"opts sync={sync}", "relin_fnn_step", opts, sync=sync)
            t(f"sync={sync}", "calculate", sync=sync)
            t(f"opts sync={sync}", "calculate", opts, sync=sync)
        t("", "synchronize")
        t("", "relin_fnn_advance")
        t("", "advance_plant")
        t("", "relin_terminal_status")
        t("", "sqp_fnn_start", r(b, n))
        t("guess", "sqp_fnn_start", r(b, n), r(b, m, N))
        t("", "sqp_fnn_iterate", 5)
        t("all", "sqp_fnn_iterate", 5, step_scale=0.5, opts=opts, step_rule="merit")
        t("bad rule", "sqp_fnn_iterate", 5, step_rule="armijo")
        t("", "sqp_fnn_solve", 9, 1e-6)
        t("all", "sqp_fnn_solve", 9, 1e-6, opts=opts, step_rule="fixed")
        t("gn", "sqp_fnn_set_hessian", "gauss_newton")
        t("exact", "sqp_fnn_set_hessian", "exact")
        t("bad", "sqp_fnn_set_hessian", "bfgs")
        t("on", "sqp_fnn_set_row_multipliers", True)
        t("off", "sqp_fnn_set_row_multipliers", False)
        t("", "sqp_fnn_state_multipliers")
        t("", "sqp_fnn_skipped")
        for mode in ("given", "dare_device", 1, "riccati"):
            t(repr(mode), "set_terminal_weight", mode)
        for mode in ("discrete", "continuous", 1, "tustin"):
            t(repr(mode), "set_model_time", mode, 0.05)
        t("default Ts", "set_model_time", "discrete")
        for i in (0, 4, 6):
            t(str(i), "model_instance", i)
            t(str(i), "terminal_weight_instance", i)
        t("", "set_reference", xr, ur)
        t("per instance", "set_reference", r(b, n, N + 1), r(b, m, N), per_instance=True)
        t("bad", "set_reference", ur, ur)
        t("", "update_initialization", r(b, n))
        t("bad", "update_initialization", r(b, m))
        t("", "get_results")
        t("subset", "get_results", want=("u", "status"))
        t("list", "get_results", want=["e_x", "iters", "polish_iters"])
        t("string", "get_results", want="e_u")
        t("empty", "get_results", want=())
        t("unknown", "get_results", want=("u", "slack"))
        for want in (("u0", "status"), tuple(capi.WANT), ("x",), (), "u", ("u", "slack")):
            ticket = t(repr(want), "get_results_async", want=want)
            if ticket is not None:
                t(repr(want), "get_results_wait", ticket, want=want)
        t("", "get_results_async")
        t("", "get_results_wait", 9)
        t("unknown", "get_results_wait", 9, want=("u", "slack"))
        t("string", "get_results_wait", 9, want="status")
        lib.fail_next = -1
        t("fails", "get_results_async")
        t("", "sensitivity")
        t("subset", "sensitivity", want=("dX", "K0"), act_tol=1e-8)
        for name in ("sensitivity", "sensitivity_stagewise", "sensitivity_stagewise_rate", "sensitivity_rows"):
            t("string", name, want="dU")
            t("empty", name, want=())
            t("unknown", name, want=("K0", "dP"))
            t("", name + "_vjp", gu)
            t("g_x", name + "_vjp", gu, gx)
        t("tol", "sensitivity_stagewise", ("K0",), 1e-8)
        t("tol", "sensitivity_stagewise_rate", ("K0", "dU"), act_tol=1e-8)
        t("tols", "sensitivity_rows", ("K0",), 1e-8, 1e-6)
        t("tol", "sensitivity_vjp", gu, gx, 1e-8)
        t("tol", "sensitivity_stagewise_vjp", gu, gx, act_tol=1e-8)
        t("tol", "sensitivity_stagewise_rate_vjp", gu, None, 1e-8)
        t("tols", "sensitivity_rows_vjp", gu, gx, 1e-8, 1e-6)
        t("", "sensitivity_params_vjp", gu)
        t("g_x", "sensitivity_params_vjp", gu, gx, want=("B", "x0", "f", "R"), act_tol=1e-8)
        t("string", "sensitivity_params_vjp", gu, want="Q")
        t("unknown", "sensitivity_params_vjp", gu, want=("Q", "W"))
        t("data", "sensitivity_params_vjp", gu, gx, terminal="data")
        t("dare", "sensitivity_params_vjp", gu, gx, want=("A", "P", "u_min"), terminal="dare")
        t("bad terminal", "sensitivity_params_vjp", gu, terminal="riccati")
        for name in ("certificate", "relin_fnn_certificate"):
            t("", name)
            t("subset", name, want=("costate", "cost"))
            t("string", name, want="grad")
            t("empty", name, want=())
            t("unknown", name, want=("cost", "gap"))
        lib.fail_next = -5
        t("fails", "certificate")
        if kind == "group":
            do("group.g, n, m, N, batch, nz", lambda: (type(s.g).__name__, s.n, s.m, s.N, s.batch, s.nz))
            do("group.shards", lambda: s.shards)
            do("group.handles", lambda: [(type(hv).__name__, isinstance(hv, capi.Solver), hv.batch, hv.nz) for hv in s.handles])
            slots = t("", "x0_staging")
            t("", "update_initialization_staged")
            t("resident", "update_initialization", r(b, n), resident=True)
            t("not resident", "update_initialization", r(b, n), resident=False)
            t("", "get_results", want=("u0", "x"))
            do("group.handles[1].get_first_input", s.handles[1].get_first_input)
            do("group.handles[2].design_shared", s.handles[2].design_shared, A, B, Q, R, umin=umin, umax=umax)
            do("group.handles[0].close", s.handles[0].close)
            t("", "close")
            t("again", "close")
            continue
        # ---- what only a handle has
        do("solver.h, n, m, N, batch, nz", lambda: (type(s.h).__name__, s.n, s.m, s.N, s.batch, s.nz))
        ltv = (r(b, N, n, n), r(b, N, n, m), r(b, N, n), r(b, n, N + 1), r(b, m, N))
        t("", "design_ltv", *ltv, xr, ur, Q, R, P=P, umin=umin, umax=umax)
        t("all", "design_ltv", *ltv, xr, ur, Q, R, S=S, P=Pb, umin=umin, umax=umax, rho=0.3, sigma=1e-5, rho_profile="stiffness", xmin=xmin,
          xmax=xmax, terminal="equality", keep_stage_models=True)
        t("no c, no refs", "design_ltv", ltv[0], ltv[1], None, ltv[3], ltv[4], None, None, Q, R, P=P, umin=umin, umax=umax,
          keep_stage_models=False)
        t("xmin only", "design_ltv", *ltv, xr, ur, Q, R, P=P, umin=umin, umax=umax, xmin=xmin)
        t("bad profile", "design_ltv", *ltv, xr, ur, Q, R, P=P, umin=umin, umax=umax, rho_profile="vector")
        t("", "set_keep_stage_models")
        t("off", "set_keep_stage_models", False)
        for name in ("get_weights_instance", "get_gradient_instance", "get_design_instance"):
            t("5", name, 5)
        t("", "get_design")
        t("", "get_first_input")
        t("", "relin_fnn_timing")
        t("bad id", "comm_init", b"short", 0, 2)
        t("", "comm_init", bytes(range(128)), 1, 2)
        t("", "comm_summary")
        t("", "comm_allgather_first_input")
        other = do("Solver other", capi.Solver, n, m, N + 3, b)
        t("", "start_from", other)
        t("on", "set_step_fusion", True)
        t("off", "set_step_fusion", False)
        t("", "update_initialization_device", 0xABC000)
        t("", "update_initialization_async", r(b, n))
        slot = t("", "x0_staging")
        t("staged", "update_initialization_async", slot)
        ticket = t("", "get_results_async", want=("u0", "status", "x"))
        t("views", "get_results_wait", ticket, want=("x", "status"), copy=False)
        t("views all", "get_results_wait", ticket, want=("u0", "status", "x"), copy=False)
        t("views not asked for", "get_results_wait", ticket, want=("u", "status"), copy=False)
        t("views unknown", "get_results_wait", ticket, want=("slack",), copy=False)
        t("copy", "get_results_wait", ticket, want=("x", "status"), copy=True)
        for name in ("device_results", "device_sensitivity", "device_certificate", "device_certificate_ltv"):
            t("", name)
        t("", "certificate_ltv")
        t("subset", "certificate_ltv", want=("x", "cost"))
        t("string", "certificate_ltv", want="e_x")
        t("empty", "certificate_ltv", want=())
        t("unknown", "certificate_ltv", want=("cost", "gap"))
        for name in ("get_timing", "debug_poison_lds", "timing_summary", "timing_samples"):
            t("", name)
        t("cap", "timing_samples", cap=2)
        t("", "timing_set_stride", 8)
        t("", "timing_reset")
        t("reserve", "timing_reset", 64)
        do("other.close", other.close)
        t("", "close")
        t("again", "close")


def trace(capi):
    log = []
    lib = RecordingLib(log)
    before, capi._lib = capi._lib, lib
    try:
        script(capi, lib, log)
    finally:
        capi._lib = before
    return log


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    import almpc_loader
    lines = trace(almpc_loader.load_package()._capi)
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        print("\n".join(lines))
