"""Plain-PyTorch reference of the libhpnn math (any dtype; FP64 = the oracle).

Mirrors csrc/cpu/cpu_engine.cpp (online step) and csrc/cpu/cpu_batched.cpp (minibatch
step) -- i.e. reference ann.c / snn.c semantics, SURVEY 2.4.
"""
import torch

TINY = 1e-14


def act(x):
    return 2.0 / (1.0 + torch.exp(-x)) - 1.0


def dact(y):
    return -0.5 * (y * y - 1.0)


def forward(weights, X, net_type):
    """X [B, n_in] -> list of activations per layer (last = network output)."""
    hs = []
    h = X
    L = len(weights)
    for l, W in enumerate(weights):
        z = h @ W.t()
        if l < L - 1 or net_type == "ANN":
            h = act(z)
        elif net_type == "SNN":
            e = torch.exp(z - 1.0)
            h = e / (TINY + e.sum(1, keepdim=True))
        else:
            h = z
        hs.append(h)
    return hs


def loss_per_sample(o, T, net_type):
    if net_type == "SNN":
        return -(T * torch.log(o + TINY) * (o > 0)).sum(1) / o.shape[1]
    return 0.5 * ((T - o) ** 2).sum(1)


def deltas(weights, hs, T, net_type):
    L = len(weights)
    o = hs[-1]
    d = [None] * L
    d[L - 1] = (T - o) * dact(o) if net_type == "ANN" else (T - o)
    for l in range(L - 2, -1, -1):
        d[l] = (d[l + 1] @ weights[l + 1]) * dact(hs[l])
    return d


def adam_new_state(lr=0.001, beta1=0.9, beta2=0.999, eps=1e-8, decay=0.0):
    """the state of adam_step: the coefficients, t = 0 and the running products p1 = p2 = 1"""
    return {"lr": float(lr), "beta1": float(beta1), "beta2": float(beta2), "eps": float(eps), "decay": float(decay),
            "t": 0, "p1": 1.0, "p2": 1.0}


def adam_step(W, M, V, G, state, advance=True):
    """One Adam / AdamW step of include/libhpnn/adam.h in place on the tensors (or lists of
    tensors) W, M (first moment), V (second moment) of one dtype (float64 / float32), G the
    ascent direction the project's BP adds to W: torch.optim.Adam / AdamW with maximize=True.
    Written independently of the C form: the state advances first (t += 1, p1 *= beta1,
    p2 *= beta2, unless advance=False: the caller did), then with c1 = lr / (1 - p1),
    s2 = sqrt(1 - p2) rounded to the tensors' dtype
        m = beta1 m + (1 - beta1) g,  v = beta2 v + ((1 - beta2) g) g,
        w = w - lr decay w  (decay != 0),  w = w + c1 (m / (sqrt(v) / s2 + eps))."""
    import math
    if advance:
        state["t"] += 1
        state["p1"] *= state["beta1"]
        state["p2"] *= state["beta2"]
    c1 = state["lr"] / (1.0 - state["p1"])
    s2 = math.sqrt(1.0 - state["p2"])
    wd = state["lr"] * state["decay"]
    many = isinstance(W, (list, tuple))
    for w, m, v, g in zip(*((W, M, V, G) if many else ([W], [M], [V], [G]))):
        dt = w.dtype
        c = lambda x: torch.tensor(x, dtype=torch.float64).to(dt)  # noqa: E731  (one rounding to T)
        g = g.to(dt)
        m.copy_(c(state["beta1"]) * m + c(1.0 - state["beta1"]) * g)
        v.copy_(c(state["beta2"]) * v + (c(1.0 - state["beta2"]) * g) * g)
        if state["decay"] != 0.0:
            w.copy_(w - c(wd) * w)
        # a full tensor as the divisor: PyTorch turns a division by a scalar into a product with its
        # reciprocal, which is another rounding than the rule's
        # and the square root through FP64 (correctly rounded to T; PyTorch's vectorised FP32 sqrt
        # is not on every CPU)
        root = torch.sqrt(v.double()).to(dt)
        w.copy_(w + c(c1) * (m / (root / torch.full_like(v, s2) + c(state["eps"]))))


def clip_coefficient(G, max_norm):
    """gradient clipping by global norm, the independent form: the L2 norm over every layer's
    gradient (torch.linalg.vector_norm) and the coefficient min(1, max_norm / norm).  Returns
    (coefficient, norm) as floats; a NaN norm gives 1."""
    norm = float(torch.linalg.vector_norm(torch.cat([g.reshape(-1).double() for g in G])))
    return (max_norm / norm if norm > max_norm else 1.0), norm


def batched_step(weights, X, T, net_type, lr, momentum=None, alpha=0.2, adam=None, clip=None, norms=None):
    """In-place minibatch step; returns the mean loss before the update.
    momentum: list of dW tensors (BPM) or None (BP).  adam: (M, V, state) -- lists of moment
    tensors and an adam_new_state dict -- selects adam_step (lr, alpha are then unused).
    clip: None | max_norm -- the whole gradient is multiplied by clip_coefficient first; norms: a
    list the step's gradient norm is appended to."""
    hs = forward(weights, X, net_type)
    loss = loss_per_sample(hs[-1], T, net_type).mean()
    d = deltas(weights, hs, T, net_type)
    B = X.shape[0]
    G = [d[l].t() @ (X if l == 0 else hs[l - 1]) / B for l in range(len(weights))]
    if clip is not None or norms is not None:
        coef, norm = clip_coefficient(G, float("inf") if clip is None else clip)
        if norms is not None:
            norms.append(norm)
        if clip is not None:
            G = [g * coef for g in G]
    if adam is not None:
        adam_step(weights, adam[0], adam[1], G, adam[2])
        return loss
    for l, W in enumerate(weights):
        if momentum is not None:
            momentum[l] += lr * G[l]
            W += momentum[l]
            momentum[l] *= alpha
        else:
            W += lr * G[l]
    return loss


def online_step(weights, x, t, net_type, lr, momentum=None, alpha=0.2):
    """One reference training iteration for one sample: returns Ep - Epr."""
    X, T = x[None, :], t[None, :]
    hs = forward(weights, X, net_type)
    Ep = loss_per_sample(hs[-1], T, net_type)[0]
    d = deltas(weights, hs, T, net_type)
    for l, W in enumerate(weights):
        hin = X if l == 0 else hs[l - 1]
        G = d[l].t() @ hin
        if momentum is not None:
            momentum[l] += lr * G
            W += momentum[l]
            momentum[l] *= alpha
        else:
            W += lr * G
    hs = forward(weights, X, net_type)
    return Ep - loss_per_sample(hs[-1], T, net_type)[0], hs[-1][0]


# ----------------------------------------------------------------------------- [train] CG
CG_TRIALS = 6
CG_FAILED, CG_RESTART, CG_VERTEX, CG_TOOK7 = 1, 2, 4, 8


def cg_loss(weights, X, T, net_type):
    """mean loss (a Python float, summed in FP64) and argmax hits of the set"""
    o = forward(weights, X, net_type)[-1]
    hits = int((o.argmax(1) == T.argmax(1)).sum())
    return float(loss_per_sample(o, T, net_type).double().sum()) / X.shape[0], hits


def cg_gradient(weights, X, T, net_type, batch=None):
    """the descent direction g = (1/n) sum delta (x) h, accumulated in chunks of `batch` rows"""
    n = X.shape[0]
    batch = batch or n
    g = [torch.zeros_like(W) for W in weights]
    for s in range(0, n, batch):
        Xb, Tb = X[s:s + batch], T[s:s + batch]
        hs = forward(weights, Xb, net_type)
        d = deltas(weights, hs, Tb, net_type)
        for l in range(len(weights)):
            g[l] += d[l].t() @ (Xb if l == 0 else hs[l - 1])
    return [x / n for x in g]


def cg_state(weights, lr):
    """the state of one CG call: the first a_init is lr, the first direction is g"""
    return {"a_init": float(lr), "first": True, "gg_prev": 0.0, "d": [torch.zeros_like(W) for W in weights],
            "g_prev": [torch.zeros_like(W) for W in weights]}


def cg_iteration(weights, X, T, net_type, state, batch=None):
    """One nonlinear conjugate-gradient iteration over the whole set, in place on `weights`
    (include/libhpnn/cg.h, docs/DESIGN.md 3.2h; FP64 tensors = the oracle): Polak-Ribiere+
    direction, six fixed trials a_init 2^(j-2), the parabola point as the seventh, all
    forward-only.  Returns the record: f0, f1, beta, alpha, trial (None: every trial a NaN), flags,
    hits, and phi (the seven trial losses) for the tests' preconditions."""
    def dot(a, b):
        return float(sum((x.double() * y.double()).sum() for x, y in zip(a, b)))

    g = cg_gradient(weights, X, T, net_type, batch)
    f0, hits = cg_loss(weights, X, T, net_type)
    gg, gp, gd = dot(g, g), dot(g, state["g_prev"]), dot(g, state["d"])
    beta, flags = 0.0, 0
    if state["first"] or not state["gg_prev"] > 0.0:
        flags = CG_RESTART
    else:
        beta = (gg - gp) / state["gg_prev"]
        if not beta > 0.0:
            beta = 0.0
        if not gg + beta * gd > 0.0:
            beta, flags = 0.0, CG_RESTART
    d = [gi + beta * di if beta else gi.clone() for gi, di in zip(g, state["d"])]
    state["d"], state["g_prev"], state["gg_prev"] = d, g, gg
    W0 = [W.clone() for W in weights]

    def phi(a):
        for W, w0, di in zip(weights, W0, d):
            W.copy_(w0 + a * di if a else w0)
        return cg_loss(weights, X, T, net_type)[0]

    a_init = state["a_init"]
    steps = [a_init * 2.0 ** (j - 2) for j in range(CG_TRIALS)]
    phis = [phi(a) for a in steps]
    js = None
    for j, p in enumerate(phis):
        if p == p and (js is None or p < phis[js]):
            js = j
    a7 = 0.0
    if js is None or not phis[js] < f0:
        flags |= CG_FAILED
    else:
        b, fb = steps[js], phis[js]
        a7 = b
        if js + 1 < CG_TRIALS:
            a, fa = (steps[js - 1], phis[js - 1]) if js else (0.0, f0)
            c, fc = steps[js + 1], phis[js + 1]
            p, q = (b - a) * (fb - fc), (b - c) * (fb - fa)
            den = p - q
            if den != 0.0 and den == den:
                x = b - 0.5 * ((b - a) * p - (b - c) * q) / den
                if a < x < c:
                    a7, flags = x, flags | CG_VERTEX
    f7 = phi(a7)
    if flags & CG_FAILED:
        astar, f1 = 0.0, f0
        state["a_init"], state["first"] = a_init / 16.0, True
    else:
        astar, f1 = steps[js], phis[js]
        if f7 < f1:
            astar, f1, flags = a7, f7, flags | CG_TOOK7
        state["a_init"], state["first"] = astar, False
    phi(astar)
    return {"f0": f0, "f1": f1, "beta": beta, "alpha": astar, "trial": js, "flags": flags, "hits": hits,
            "phi": phis + [f7]}
