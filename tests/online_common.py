"""FP64 / long-double reference of the online (batch-1, iterate one sample until it converges)
rule, with fixtures, tolerances and mutants for the unit tests of csrc/gpu/online.hip (CPU only).

run() restates the rule in numpy, not the C: forward; Ep; deltas with the pre-update weights; BP
(W += lr d (x) h) or BPM (v += lr d (x) h; W += v; v *= alpha); re-forward; dEp = Ep - Ep'; first
maximum from a probe of -1.0; target = last t == 1 (0 when none); the stop rule of
hpnn_cpu_train_sample.  Every dot product and sum runs in a selectable order ("natural",
"reversed", "strided": 64 strided partial sums, then those in order) in float64, or in natural
order in np.longdouble ("longdouble").  The spread of those variants is what the tests'
tolerance is built from (tolerances()); `mutant` runs a deliberately wrong rule."""
import functools
from types import SimpleNamespace

import numpy as np

TINY = 1e-14
TYPES = {"ANN": 0, "LNN": 1, "SNN": 2}
ORDERS = ("natural", "reversed", "strided", "longdouble")
EPS = float(np.finfo(np.float64).eps)
MARGIN = 16.0      # the kernels sum in an order no variant uses; device exp / log are 1-ulp functions
FLOOR_ULP = 4.0    # where the variants happen to coincide
# the project's default limits (include/libhpnn.h: MIN_*/MAX_*_ITER, DELTA_*), by momentum
DEFAULTS = {False: dict(min_iter=31, max_iter=102399, delta=1e-6), True: dict(min_iter=15, max_iter=102399, delta=1e-6)}

MUTANTS = ("deltas_after_update", "momentum_scaled_first", "first_target", "last_max", "min_ge", "max_ge",
           "snn_no_guard", "skip_col_1024", "drop_partial")


# ----------------------------------------------------------------------------- ordered sums
def _seq(P):
    """strictly sequential sum along the last axis (np.sum is pairwise)"""
    if P.shape[-1] == 0:
        return np.zeros(P.shape[:-1], P.dtype)
    return np.cumsum(P, axis=-1)[..., -1]


def _osum(P, order):
    if order == "reversed":
        return _seq(P[..., ::-1])
    if order == "strided":
        n = P.shape[-1]
        pad = (-n) % 64
        if pad:
            P = np.concatenate([P, np.zeros(P.shape[:-1] + (pad,), P.dtype)], axis=-1)
        lanes = _seq(np.swapaxes(P.reshape(P.shape[:-1] + (-1, 64)), -1, -2))
        return _seq(lanes)
    return _seq(P)


def _quantum(a):
    """the largest power of two that divides every entry (inf for all zeros)"""
    a = np.asarray(a, np.float64).ravel()
    a = a[a != 0]
    if a.size == 0:
        return np.inf
    m, e = np.frexp(np.abs(a))
    mi = (m * 2.0 ** 53).astype(np.int64)
    return float(np.min((mi & -mi).astype(np.float64) * 2.0 ** (e - 53)))


def _dot(W, v, order, exact=None):
    """W [N, M] . v [M]; exact: the name under which the exactness condition is asserted"""
    if exact is not None and W.size:
        q = _quantum(W) * _quantum(v)
        top = float((np.abs(W) @ np.abs(v)).max())
        assert not np.isfinite(q) or top < 2.0 ** 52 * q, f"{exact}: sum of |terms| {top} over quantum {q}"
    return _osum(W * v[None, :], order)


def act(z):
    with np.errstate(over="ignore"):  # the integer fixtures reach z of -1000s: e^-z = inf and f = -1
        return 2.0 / (1.0 + np.exp(-z)) - 1.0


def dact(y):
    return -0.5 * (y * y - 1.0)


# ----------------------------------------------------------------------------- the rule
def run(W, dW, x, t, net, momentum, lr, alpha=0.0, delta=1e-6, min_iter=0, max_iter=0, order="natural",
        mutant=None, grid=0, forward_only=False, exact=False):
    """One sample.  W / dW: lists of [N, M] arrays (not modified).  Returns a namespace: W, dW
    (float64 / long double), out, dEp, init_err, iters, ok, first_ok, hist (dEp per iteration),
    z0 (the pre-activations of the first forward), d0 (the deltas of the first iteration)."""
    assert order in ORDERS and (mutant is None or mutant in MUTANTS)
    dt = np.longdouble if order == "longdouble" else np.float64
    W = [np.array(w, dt) for w in W]
    V = [np.array(v, dt) for v in dW]
    x, t = np.asarray(x, dt), np.asarray(t, dt)
    L, typ = len(W), TYPES[net]
    lr, alpha, tiny = dt(lr), dt(alpha), dt(TINY)
    ex = (lambda name: name) if exact else (lambda name: None)

    def forward(first=False):
        hs, zs, h = [], [], x
        for l in range(L):
            z = _dot(W[l], h, order, ex(f"forward {l}") if first else None)
            zs.append(z)
            if l < L - 1 or typ == 0:
                h = act(z)
            elif typ == 2:
                e = np.exp(z - dt(1.0))
                h = e / (tiny + _osum(e, order))
            else:
                h = z
            hs.append(h)
        return hs, zs

    def error(o):
        if typ == 2:
            terms = t * np.log(o + tiny)
            if mutant != "snn_no_guard":
                terms = np.where(o > 0, terms, dt(0))  # an output of exactly 0 leaves the sum
            return -_osum(terms, order) / dt(o.size)
        return dt(0.5) * _osum((t - o) * (t - o), order)

    def hidden_delta(l, d_next, h):
        """delta of layer l from the deltas of layer l + 1 through the CURRENT W[l + 1]"""
        dn = d_next
        if mutant == "drop_partial" and grid > 0 and l == L - 2:
            dn = d_next.copy()
            dn[0::grid] = 0  # the partial of workgroup 0 (rows 0, G, 2G, ..)
        return _dot(W[l + 1].T, dn, order, ex(f"delta {l}")) * dact(h)

    def update(l, d, hin):
        G = (lr * d)[:, None] * hin[None, :]
        skip = mutant == "skip_col_1024" and W[l].shape[1] > 1024
        if exact:
            q = min(_quantum(W[l]), _quantum(V[l]), _quantum(G), _quantum(np.asarray(alpha, np.float64)) * min(
                _quantum(V[l]), _quantum(G)))
            top = float((np.abs(W[l]) + np.abs(V[l]) + np.abs(G)).max())
            assert top < 2.0 ** 52 * q, f"update {l}: {top} over quantum {q}"
            assert np.array_equal((lr * d).astype(np.longdouble)[:, None] * hin.astype(np.longdouble)[None, :], G)
        keepW, keepV = (W[l][:, 1024].copy(), V[l][:, 1024].copy()) if skip else (None, None)
        if momentum:
            if mutant == "momentum_scaled_first":
                V[l] = (V[l] + G) * alpha
                W[l] = W[l] + V[l]
            else:
                V[l] = V[l] + G
                W[l] = W[l] + V[l]
                V[l] = V[l] * alpha
        else:
            W[l] = W[l] + G
        if skip:
            W[l][:, 1024], V[l][:, 1024] = keepW, keepV

    hs, z0 = forward(first=True)
    Ep = error(hs[-1])
    res = SimpleNamespace(init_err=Ep, z0=z0, d0=None, hist=[], dEp=dt(0), iters=0, ok=0, first_ok=0)
    if forward_only:
        res.W, res.dW, res.out = W, V, hs[-1]
        return res
    it, ok, first_ok, dEp = 0, False, False, dt(0)
    while True:
        it += 1
        o = hs[-1]
        d = [None] * L
        d[L - 1] = (t - o) * dact(o) if typ == 0 else (t - o)
        if mutant == "deltas_after_update":
            for l in range(L - 1, -1, -1):
                update(l, d[l], hs[l - 1] if l else x)
                if l:
                    d[l - 1] = hidden_delta(l - 1, d[l], hs[l - 1])
        else:
            for l in range(L - 2, -1, -1):
                d[l] = hidden_delta(l, d[l + 1], hs[l])
            for l in range(L):
                update(l, d[l], hs[l - 1] if l else x)
        if it == 1:
            res.d0 = d
        hs, _ = forward()
        Epr = error(hs[-1])
        dEp, Ep = Ep - Epr, Epr
        res.hist.append(dEp)
        o = hs[-1]
        max_p, probe = 0, dt(-1.0)
        for j in range(o.size):  # the first maximum wins; nothing above the probe: index 0
            if o[j] >= probe if mutant == "last_max" else o[j] > probe:
                probe, max_p = o[j], j
        ones = np.nonzero(t == 1)[0]
        p_trg = 0 if ones.size == 0 else int(ones[0] if mutant == "first_target" else ones[-1])
        ok = max_p == p_trg
        if it == 1:
            first_ok = ok
        if (it >= max_iter) if mutant == "max_ge" else (it > max_iter):
            break
        ok = ok and ((it >= min_iter) if mutant == "min_ge" else (it > min_iter))
        if not (dEp > delta or not ok):
            break
    res.W, res.dW, res.out = W, V, hs[-1]
    res.dEp, res.iters, res.ok, res.first_ok = dEp, it, int(ok), int(first_ok)
    return res


# ----------------------------------------------------------------------------- fixtures
def make_case(name, sizes, net, momentum, seed, lr=0.01, alpha=0.2, delta=1e-6, min_iter=2, max_iter=2, target=None,
              scale=1.0):
    """weights scale x uniform(-1, 1) / sqrt(M), x in [0, 1), t one-hot (-1/1, SNN 0/1); BPM: a
    non-zero initial dW (the host always zeroes it, so the kernels' read of it is otherwise
    unobserved)"""
    rng = np.random.default_rng(seed)
    W = [scale * rng.uniform(-1, 1, (n, m)) / np.sqrt(m) for m, n in zip(sizes[:-1], sizes[1:])]
    dW = [rng.uniform(-1, 1, w.shape) * 1e-3 if momentum else np.zeros_like(w) for w in W]
    x = rng.uniform(0, 1, sizes[0])
    t = np.full(sizes[-1], 0.0 if net == "SNN" else -1.0)
    t[int(rng.integers(sizes[-1])) if target is None else target] = 1.0
    return SimpleNamespace(name=name, sizes=list(sizes), net=net, momentum=bool(momentum), lr=lr, alpha=alpha,
                           delta=delta, min_iter=min_iter, max_iter=max_iter, W=W, dW=dW, x=x, t=t)


def run_case(c, order="natural", **kw):
    a = dict(momentum=c.momentum, lr=c.lr, alpha=c.alpha, delta=c.delta, min_iter=c.min_iter, max_iter=c.max_iter)
    a.update(kw)
    return run(c.W, c.dW, c.x, c.t, c.net, order=order, **a)


L16 = [20] + [18] * 15 + [6]
SINGLE_SHAPES = {  # the single-workgroup table of the tests (name -> layer sizes)
    "a63": [63, 17, 3], "a64": [64, 17, 3], "a65": [65, 17, 3],
    "b1023": [1023, 20, 5], "b1024": [1024, 20, 5], "b1025": [1025, 20, 5],
    "c": [2100, 9, 28, 7], "d": [30, 1500, 6], "e": [130, 10], "f": L16, "g": [16, 12, 1030],
    "h": [6200, 8, 4], "i": [19000, 8, 4], "j": [19300, 8, 4],
}
COOP_SHAPES = {
    "A": [70, 48, 200, 33, 7], "B65": [65, 29, 3], "B1025": [1025, 29, 3], "C": [40, 64, 300], "D": [130, 40],
    "E": [6000, 40, 4], "F": L16,
}
COOP_GRIDS = {"A": (None, 1, 3, 64, 65, 128), "B65": (8,), "B1025": (8,), "C": (None,), "D": (None,), "E": (None,),
              "F": (5,)}
LDS_ONLY = ("h", "i")
# the nets of the run to convergence, at the project's default limits and lr = 0.01 (the GPU
# engines' rate): 3633, 1642 and 310 iterations
CONVERGE = {"conv70": ([70, 33, 17, 7], "ANN", True, 0.01), "conv1100": ([1100, 20, 9, 5], "SNN", False, 0.01),
            "conv130": ([130, 90, 300, 40], "SNN", True, 0.01)}
CONVERGE_SEED = {"conv70": 1, "conv1100": 1, "conv130": 1}


def nets_of(shape):
    """every shape runs ANN + BPM and SNN + BP; the wide-output shapes run LNN and SNN"""
    if shape in ("g", "C"):
        return (("LNN", True), ("SNN", False))
    return (("ANN", True), ("SNN", False))


def case_names():
    out = []
    for s in list(SINGLE_SHAPES) + list(COOP_SHAPES):
        for net, mom in nets_of(s):
            out.append(f"{s}-{net}-{'BPM' if mom else 'BP'}")
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    if name in CONVERGE:
        sizes, net, mom, lr = CONVERGE[name]
        return make_case(name, sizes, net, mom, CONVERGE_SEED[name], lr=lr, **DEFAULTS[mom])
    shape, net, train = name.split("-")
    sizes = SINGLE_SHAPES.get(shape) or COOP_SHAPES[shape]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    # 16 layers: at 1 / sqrt(M) the signal dies on the way (a gain of 0.3 per layer, updates of
    # 1e-10 in the SNN + BP case); at 3 / sqrt(M) the deltas reach the first layer
    return make_case(name, sizes, net, train == "BPM", seed, scale=3.0 if len(sizes) == 17 else 1.0)


# ----------------------------------------------------------------------------- tolerance
def _f64(a):
    return np.asarray(a, np.float64)


def compared(r, forward_only=False):
    """the toleranced quantities of a result, by name"""
    d = {"out": _f64(r.out), "init_err": _f64(r.init_err)}
    if not forward_only:
        d["dEp"] = _f64(r.dEp)
        for l, (w, v) in enumerate(zip(r.W, r.dW)):
            d[f"W{l}"], d[f"dW{l}"] = _f64(w), _f64(v)
    return d


@functools.lru_cache(maxsize=None)
def reference(name, forward_only=False):
    """(natural-order result, {quantity: tolerance}, {quantity: spread}, largest weight update).
    Tolerance = MARGIN x the largest deviation of the reversed, strided and long-double runs from
    the natural-order run + FLOOR_ULP ulp of the quantity's largest magnitude."""
    c = case(name)
    runs = {o: run_case(c, o, forward_only=forward_only) for o in ORDERS}
    nat = compared(runs["natural"], forward_only)
    spread = {k: 0.0 for k in nat}
    for o in ORDERS[1:]:
        for k, v in compared(runs[o], forward_only).items():
            spread[k] = max(spread[k], float(np.abs(v - nat[k]).max()))
    tol = {k: MARGIN * spread[k] + FLOOR_ULP * EPS * float(np.abs(nat[k]).max()) for k in nat}
    upd = 0.0 if forward_only else max(float(np.abs(nat[f"W{l}"] - c.W[l]).max()) for l in range(len(c.W)))
    iters = {o: runs[o].iters for o in ORDERS}
    return runs["natural"], tol, spread, upd, iters


def check_precondition(name):
    """the tolerance of every weight tensor is below 1e-6 of the largest weight update of the case:
    what keeps the tolerance from hiding a dropped element"""
    _, tol, _, upd, _ = reference(name)
    worst = max(v for k, v in tol.items() if k.startswith(("W", "dW")))
    assert upd > 0 and worst < 1e-6 * upd, (name, worst, upd)
    return worst / upd


def check_converge_precondition(name):
    """the dEp history stays at least 1000 tolerances from delta at the deciding iteration and at
    the one before, and every order gives the same iteration count"""
    nat, tol, _, _, iters = reference(name)
    c = case(name)
    assert len(set(iters.values())) == 1, iters
    assert nat.iters <= c.max_iter, (name, nat.iters)
    for h in nat.hist[-2:]:
        assert abs(float(h) - c.delta) >= 1000 * tol["dEp"], (name, float(h), tol["dEp"])


# ----------------------------------------------------------------------------- exact fixtures
def exact_case(name, sizes, net, momentum, seed):
    """Integer data on which the first iteration is exact in FP64 in any order: x in 1..3, every
    hidden row either "saturated" (weights multiples of 64 with a non-zero sum: |z| >= 64, f = +-1,
    f' = 0) or "open" (integer weights with z exactly 0: f = 0, f' = 1/2); unit 0 of every hidden
    layer is saturated so an open row of the next layer can cancel on it.  Output rows: ANN open
    (z = 0, o = 0), LNN small integers.  lr = 2^-4, alpha = 1/4, dW0 multiples of 2^-3, one
    iteration (max_iter = 0)."""
    assert net in ("ANN", "LNN")
    rng = np.random.default_rng(seed)
    L = len(sizes) - 1
    x = rng.integers(1, 4, sizes[0]).astype(np.float64)
    x[0] = 1.0
    W, h = [], x
    for l in range(L):
        N, M = sizes[l + 1], sizes[l]
        last = l == L - 1
        w = np.zeros((N, M))
        z = np.zeros(N)
        for j in range(N):
            open_row = (last and net == "ANN") or (not last and j > 0 and rng.random() < 0.6)
            if last and net == "LNN":
                w[j] = rng.integers(-2, 3, M)
            elif open_row:
                w[j] = rng.integers(-3, 4, M)
                w[j, 0] = 0
                w[j, 0] = -float(w[j] @ h) / h[0]  # h[0] = +-1: cancels exactly
            else:
                w[j] = 64.0 * rng.integers(-2, 3, M)
                if float(w[j] @ h) == 0.0:
                    w[j, 0] += 64.0 * h[0]
            z[j] = float(w[j] @ h)
        W.append(w)
        h = z if last else np.sign(z)
    dW = [rng.integers(-8, 9, w.shape) / 8.0 if momentum else np.zeros_like(w) for w in W]
    t = np.full(sizes[-1], -1.0)
    t[int(rng.integers(sizes[-1]))] = 1.0
    return SimpleNamespace(name=name, sizes=list(sizes), net=net, momentum=bool(momentum), lr=2.0 ** -4, alpha=0.25,
                           delta=1e-6, min_iter=0, max_iter=0, W=W, dW=dW, x=x, t=t)


EXACT_SHAPES = {"b1025": SINGLE_SHAPES["b1025"], "c": SINGLE_SHAPES["c"], "d": SINGLE_SHAPES["d"],
                "A": COOP_SHAPES["A"]}


def exact_names():
    return [f"{s}-{n}-{tr}" for s in EXACT_SHAPES for n, tr in (("ANN", "BPM"), ("LNN", "BP"))]


@functools.lru_cache(maxsize=None)
def exact_reference(name):
    """(case, result): asserts the conditions that make W and dW after one iteration exact"""
    shape, net, train = name.split("-")
    seed = 1000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    c = exact_case(name, EXACT_SHAPES[shape], net, train == "BPM", seed)
    r = run_case(c, "natural", exact=True)
    L = len(c.W)
    for l in range(L - 1):
        z = np.abs(r.z0[l])
        assert bool(((z == 0) | (z >= 64)).all()), (name, l)
        assert 0.2 < float((z == 0).mean()) < 0.9, (name, l, float((z == 0).mean()))
    if net == "ANN":
        assert bool((r.z0[-1] == 0).all())
    for l in range(L):  # the deltas reach a fair share of the rows of every layer
        assert float((r.d0[l] != 0).mean()) >= 0.2, (name, l, float((r.d0[l] != 0).mean()))
    for o in ORDERS[1:]:
        v = run_case(c, o)
        for l in range(L):
            assert np.array_equal(_f64(v.W[l]), r.W[l]) and np.array_equal(_f64(v.dW[l]), r.dW[l]), (name, o, l)
            assert np.array_equal(v.W[l], r.W[l]) and np.array_equal(v.dW[l], r.dW[l]), (name, o, l)
    changed = sum(int((r.W[l] != c.W[l]).sum()) for l in range(L))
    assert changed > 0.1 * sum(w.size for w in c.W), (name, changed)
    return c, r


# ----------------------------------------------------------------------------- stop-rule fixtures
def _lnn_case(name, outs, t, min_iter, max_iter, net="LNN", n_in=5):
    """one layer, lr = 0: out = W x with W[:, 0] = outs and x = (1, 2, 0, 1, 3): exact, and the
    weights never move, so dEp is exactly 0"""
    outs = np.asarray(outs, np.float64)
    W = np.zeros((outs.size, n_in))
    W[:, 0] = outs
    W[:, 2] = 7.0  # meets x[2] = 0
    x = np.array([1.0, 2.0, 0.0, 1.0, 3.0])
    W[:, 1], W[:, 3] = 1.0, -2.0  # 2 - 2 = 0
    return SimpleNamespace(name=name, sizes=[n_in, outs.size], net=net, momentum=False, lr=0.0, alpha=0.0, delta=1e-6,
                           min_iter=min_iter, max_iter=max_iter, W=[W], dW=[np.zeros_like(W)], x=x,
                           t=np.asarray(t, np.float64))


def _onehot(n, i, lo=-1.0):
    t = np.full(n, lo)
    t[i] = 1.0
    return t


def stop_cases():
    """name -> (case, expected words or None).  expected: dict of iters / ok / first_ok"""
    o5 = [0.0, 3.0, -1.0, 2.0, 1.0]
    wide = np.zeros(1030)
    wide[1027] = 5.0
    mid = np.zeros(300)
    mid[290] = 5.0
    # 37 logits so that the summation orders differ and the tolerance is not its floor alone
    neg = np.random.default_rng(9).integers(-3, 4, 37).astype(np.float64)
    neg[1], neg[2], neg[3] = -800.0, 5.0, -900.0
    t9 = np.zeros(37)
    t9[1] = t9[2] = 1.0  # one target on an output that underflowed to 0, the last on a positive one
    return {
        "1-correct": (_lnn_case("s1", o5, _onehot(5, 1), 3, 10), dict(iters=4, ok=1, first_ok=1)),
        "2-wrong": (_lnn_case("s2", o5, _onehot(5, 3), 3, 5), dict(iters=6, ok=0, first_ok=0)),
        "3-min-ge-max": (_lnn_case("s3", o5, _onehot(5, 1), 7, 4), dict(iters=5, ok=1, first_ok=1)),
        "3-min-eq-max": (_lnn_case("s3e", o5, _onehot(5, 1), 4, 4), dict(iters=5, ok=1, first_ok=1)),
        "4-tie-second": (_lnn_case("s4a", [0.0, 3.0, -1.0, 3.0, 1.0], _onehot(5, 3), 1, 3),
                         dict(iters=4, ok=0, first_ok=0)),
        "4-tie-first": (_lnn_case("s4b", [0.0, 3.0, -1.0, 3.0, 1.0], _onehot(5, 1), 1, 3),
                        dict(iters=2, ok=1, first_ok=1)),
        "5-two-ones-last": (_lnn_case("s5a", o5, [-1.0, 1.0, -1.0, 1.0, -1.0], 1, 3), dict(iters=4, ok=0, first_ok=0)),
        "5-two-ones-hit": (_lnn_case("s5b", [0.0, 2.0, -1.0, 3.0, 1.0], [-1.0, 1.0, -1.0, 1.0, -1.0], 1, 3),
                           dict(iters=2, ok=1, first_ok=1)),
        "6-no-one-hit": (_lnn_case("s6a", [4.0, 3.0, -1.0, 2.0, 1.0], [-1.0] * 5, 1, 3),
                         dict(iters=2, ok=1, first_ok=1)),
        "6-no-one-miss": (_lnn_case("s6b", o5, [-1.0] * 5, 1, 3), dict(iters=4, ok=0, first_ok=0)),
        "7-all-minus-one-hit": (_lnn_case("s7a", [-64.0] * 5, _onehot(5, 0), 1, 3, net="ANN"),
                                dict(iters=2, ok=1, first_ok=1)),
        "7-all-minus-one-miss": (_lnn_case("s7b", [-64.0] * 5, _onehot(5, 2), 1, 3, net="ANN"),
                                 dict(iters=4, ok=0, first_ok=0)),
        "8-beyond-1024": (_lnn_case("s8", wide, _onehot(1030, 1027), 1, 3), dict(iters=2, ok=1, first_ok=1)),
        "8-beyond-1024-miss": (_lnn_case("s8m", wide, _onehot(1030, 1028), 1, 3), dict(iters=4, ok=0, first_ok=0)),
        "8b-beyond-256": (_lnn_case("s8b", mid, _onehot(300, 290), 1, 3), dict(iters=2, ok=1, first_ok=1)),
        "8b-beyond-256-miss": (_lnn_case("s8bm", mid, _onehot(300, 291), 1, 3), dict(iters=4, ok=0, first_ok=0)),
        "9-snn-underflow": (_lnn_case("s9", neg, t9, 1, 3, net="SNN"), dict(iters=2, ok=1, first_ok=1)),
    }
