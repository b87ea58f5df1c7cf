"""The compiled reference's recorded answers, for checkouts where the reference itself is absent.

The pinning tests (test_oracle_pin.py, test_epic.py) call the reference's own compiled C (oracle/_ref, built by oracle/Makefile where
the reference sources lie).  Where that library is absent they get a Replay instead.  Every call is looked up by a digest of the
method's name and all of its inputs in a committed fixture under tests/golden/; a call whose inputs were not recorded raises, so a
changed input can never pass silently.  For each recorded call the fixture holds the SHA-256 of every output the reference produced:
what it returned, and the valid region (the first w columns) of every array argument after the call, written in place or not.

  * Where an oracle call computes the same thing (COUNTERPART: the same operator of oracle/slowflow_oracle.c on the same inputs), only
    those digests are stored.  The replay runs that oracle call on the caller's arguments -- in place where the reference works in
    place -- and accepts its outputs only if every digest equals the reference's: what the test then receives is, byte for byte in
    the valid region, what the reference computed.  A differing digest fails the call with the output it concerns.
  * Where no oracle call reproduces the reference bit for bit (the two-frame smoothness and data-term operators, near-pinned only, and
    the EpicFlow library), the outputs themselves are stored and returned.

tests/golden/make_golden_pin.py records the fixtures (SFA_REF_RECORD=1) against the live library; where a counterpart exists the recorder
checks it against the reference and stores values instead of digests for any call where it does not reproduce the reference.
"""
import atexit
import ctypes
import hashlib
import inspect
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORD = os.environ.get("SFA_REF_RECORD") == "1"


# ---- the oracle's computation of each reference entry point that it restates bit for bit (oracle/__init__.py: RefLib vs Oracle) ----
def _truncated(x):
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    return x[:(x.size // 4) * 4].copy()


def _penalty_derivative(o, pid, eps, trunc, x):
    import oracle as orc
    xs = _truncated(x)
    s, v = o.psi_deriv(orc.Penalty(pid, eps, trunc), xs)
    return xs, s, v


def _penalty_apply(o, pid, eps, trunc, x):
    import oracle as orc
    xs = _truncated(x)
    return xs, o.psi_apply(orc.Penalty(pid, eps, trunc), xs)


COUNTERPART = {
    "convolve": lambda o, src, w, order, horiz: o.convolve(src, w, order, horiz),
    "gaussian_presmooth": lambda o, src, w, sigma: o.gaussian_presmooth(src, w, sigma),
    "variational_2frame": lambda o, wx, wy, im1, im2, w, p: o.variational_2frame(wx, wy, im1, im2, w, p),
    "sor": lambda o, du, dv, a11, a12, a22, b1, b2, sh, sv, w, iterations, omega, readable=False:
        o.sor(du, dv, a11, a12, a22, b1, b2, sh, sv, w, iterations, omega, readable=readable),
    "image_warp_prescaled": lambda o, src3, fwx, fwy, w: o.image_warp(src3, fwx, fwy, w, 1),      # the flow is already scaled: factor 1
    "sub_laplacian": lambda o, dst, src, wh, wv, w: o.sub_laplacian(dst, src, wh, wv, w),
    "dpsis_weight": lambda o, im3, w, coef=5.0: o.dpsis_weight(im3, w, coef=coef),
    "get_derivatives": lambda o, im1, im2, w: list(o.derivative_stack(im2, im1, w)),           # dt = im2 - im1 is the stack's I1 - I2
    "penalty_derivative": _penalty_derivative,
    "penalty_apply": _penalty_apply,
}


# ---- digests ----------------------------------------------------------------------------------------------------------------------
def _feed(h, v):
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        h.update(("nd%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    elif isinstance(v, ctypes.Structure):
        h.update(("st" + type(v).__name__).encode())
        h.update(bytes(v))
    elif isinstance(v, (list, tuple)):
        h.update(("sq%d" % len(v)).encode())
        for x in v:
            _feed(h, x)
    elif isinstance(v, np.generic):
        h.update(("np%s%r" % (v.dtype.str, v.item())).encode())
    elif v is None or isinstance(v, (bool, int, float, str)):
        h.update(("py%s%r" % (type(v).__name__, v)).encode())
    else:
        raise TypeError("cannot digest an argument of type %s" % type(v).__name__)


def digest(name, args, kwargs):
    """the key of a call: its method and every input, padding included"""
    h = hashlib.sha256(name.encode())
    _feed(h, list(args))
    for k in sorted(kwargs):
        _feed(h, k)
        _feed(h, kwargs[k])
    return h.hexdigest()[:32]


def _valid(a, w):
    return a[..., :w] if (w is not None and a.ndim >= 2) else a


def out_digest(a, w):
    """SHA-256 (first 128 bits) of an output's valid region (the pins compare the first w columns; the padding is not part of a result)"""
    h = hashlib.sha256()
    _feed(h, np.ascontiguousarray(_valid(np.asarray(a), w)))
    return h.hexdigest()[:32]


def _arrays(args, kwargs):
    """the array arguments in a fixed order (lists of arrays flattened): the places a call may write to"""
    out = []

    def walk(v):
        if isinstance(v, np.ndarray):
            out.append(v)
        elif isinstance(v, (list, tuple)):
            for x in v:
                walk(x)
    walk(list(args))
    for k in sorted(kwargs):
        walk(kwargs[k])
    return out


def _width(fn, args, kwargs):
    try:
        return inspect.signature(fn).bind(*args, **kwargs).arguments.get("w")
    except TypeError:
        return None


def _returned(ret):
    if ret is None:
        return "none", []
    if isinstance(ret, np.ndarray):
        return "array", [ret]
    return ("tuple" if isinstance(ret, tuple) else "list"), list(ret)


def _outputs(ret, args, kwargs, w):
    """digests of everything a caller sees after the call: the returned arrays, then every array argument"""
    kind, rets = _returned(ret)
    return kind, [out_digest(r, w) for r in rets], [out_digest(a, w) for a in _arrays(args, kwargs)]


def _copy(v):
    if isinstance(v, np.ndarray):
        import oracle as orc
        c = orc.aligned_zeros(v.shape) if v.dtype == np.float32 else np.empty_like(v)
        c[...] = v
        return c
    if isinstance(v, (list, tuple)):
        return type(v)(_copy(x) for x in v)
    return v


def _fixture(name):
    return os.path.join(GOLDEN, name + ".npz")


class Recorder:
    """passes every call through to the live library and keeps the digests of what it returned and left in its arguments -- and the
    values themselves where no oracle call reproduces them bit for bit; the fixture is written at exit"""
    _open = {}

    def __init__(self, name, live):
        self._live, self._name = live, name
        self._oracle = None
        if not Recorder._open:
            atexit.register(Recorder._save_all)
        self._meta, self._data = Recorder._open.setdefault(name, ({}, {}))

    def __getattr__(self, method):
        fn = getattr(self._live, method)

        def call(*args, **kwargs):
            d = digest(method, args, kwargs)
            w = _width(fn, args, kwargs)
            cargs, ckw = _copy(list(args)), {k: _copy(v) for k, v in kwargs.items()}
            before = [out_digest(a, w) for a in _arrays(args, kwargs)]
            ret = fn(*args, **kwargs)
            kind, rd, ad = _outputs(ret, args, kwargs, w)
            values = True
            if method in COUNTERPART:                   # does the oracle give the reference's bytes on this call?
                import oracle as orc
                self._oracle = self._oracle or orc.Oracle()
                cret = COUNTERPART[method](self._oracle, *cargs, **ckw)
                ckind, crd, cad = _outputs(cret if kind != "none" else None, cargs, ckw, w)
                values = (ckind, crd, cad) != (kind, rd, ad)
            if values:
                for i, r in enumerate(_returned(ret)[1]):
                    self._data["%s.r%d" % (d, i)] = np.asarray(r).copy()
                for j, a in enumerate(_arrays(args, kwargs)):
                    if ad[j] != before[j]:                  # written by the call
                        self._data["%s.a%d" % (d, j)] = np.ascontiguousarray(_valid(a, w)).copy()
            self._meta[d] = {"call": method, "w": w, "ret": kind, "n_ret": len(rd), "values": values}
            if not values:
                self._meta[d].update(ret_digests=rd, arg_digests=ad)
            return ret
        return call

    @staticmethod
    def _save_all():
        for name, (meta, data) in Recorder._open.items():
            if meta:
                np.savez_compressed(_fixture(name), __meta__=np.array(json.dumps(meta, sort_keys=True)), **data)


class Replay:
    """the library's interface answered from the fixture tests/golden/<name>.npz"""

    def __init__(self, name):
        self._name = name
        self._z = np.load(_fixture(name))
        self._meta = json.loads(str(self._z["__meta__"]))
        self._oracle = None

    def _get(self, key):
        a = self._z[key]
        if a.dtype == np.float32:                      # the reference's planes are 64-byte aligned (oracle.aligned_zeros); keep that
            import oracle as orc
            b = orc.aligned_zeros(a.shape)
            b[...] = a
            return b
        return a.copy()

    def __getattr__(self, method):
        if method.startswith("_"):
            raise AttributeError(method)

        def call(*args, **kwargs):
            d = digest(method, args, kwargs)
            m = self._meta.get(d)
            if m is None or m["call"] != method:
                raise LookupError("%s: no recorded reference output for this call of %s (its inputs changed?); "
                                  "re-record with tests/golden/make_golden_pin.py where the reference is built" % (self._name, method))
            w, arrs = m["w"], _arrays(args, kwargs)
            if m["values"]:
                for j, a in enumerate(arrs):
                    if "%s.a%d" % (d, j) in self._z.files:
                        _valid(a, w)[...] = self._z["%s.a%d" % (d, j)]
                rets = [self._get("%s.r%d" % (d, i)) for i in range(m["n_ret"])]
            else:
                import oracle as orc
                self._oracle = self._oracle or orc.Oracle()
                _, rets = _returned(COUNTERPART[method](self._oracle, *args, **kwargs))
                if m["ret"] == "none":
                    rets = []
                if len(rets) != len(m["ret_digests"]):
                    raise AssertionError("%s.%s: %d outputs returned, the reference returned %d" % (self._name, method, len(rets), len(m["ret_digests"])))
                for i, (r, want) in enumerate(zip(rets, m["ret_digests"])):
                    if out_digest(r, w) != want:
                        raise AssertionError("%s.%s: returned output %d is not the reference's (SHA-256 of its valid region differs)" % (self._name, method, i))
                for j, (a, want) in enumerate(zip(arrs, m["arg_digests"])):
                    if out_digest(a, w) != want:
                        raise AssertionError("%s.%s: array argument %d after the call is not the reference's (SHA-256 of its valid region differs)"
                                             % (self._name, method, j))
            if m["ret"] == "none":
                return None
            if m["ret"] == "array":
                return rets[0]
            return tuple(rets) if m["ret"] == "tuple" else list(rets)
        return call


def library(name, live_factory, available):
    """the live library (recording it under SFA_REF_RECORD=1) where it is available, its recorded answers elsewhere"""
    if available:
        live = live_factory()
        return Recorder(name, live) if RECORD else live
    if RECORD:
        raise RuntimeError("SFA_REF_RECORD=1 needs the compiled reference (oracle/_ref)")
    return Replay(name)
