"""fp64 restatement of FlatAdam's orthogonalised-momentum step (include/avmoe.h, avmoe_opt_muon_step) from fp32 operands, in numpy.

The rule is torch.optim.Muon's with the Newton-Schulz iteration in full precision:

    g'  = grad * gscale (+ wd * w under coupled decay)
    m   = mu m + (1 - mu) g'
    u   = (1 - mu) g' + mu m   (nesterov)   |   m
    X0  = u / (||u||_F + 1e-7)
    X  <- a X + (b A + c A A) X,  A = X X^T          ns_steps times, on the orientation whose Gram side is min(rows, cols)
    s   = 0.2 sqrt(max(rows, cols))  ("match_rms_adamw")   |   sqrt(max(1, rows / cols))  ("original")
    w   = w (1 - lr wd)   (decoupled decay only) ;   w = w - lr s X

`ns(..., dtype=np.float32)` runs the same iteration in numpy fp32: the yardstick for what fp32 arithmetic in another summation order
may differ by (the device test's bound is a multiple of ITS distance from the fp64 result)."""
import numpy as np

NS_COEFFS = (3.4445, -4.7750, 2.0315)
NS_EPS = 1e-7


def as_matrix(x):
    """a parameter's array as the rows x cols matrix it is orthogonalised as: rows = shape[0], the rest flattened"""
    x = np.asarray(x)
    return x.reshape(x.shape[0], -1)


def ns(G, steps=5, dtype=np.float64, coeffs=NS_COEFFS):
    """The orthogonalised form of a 2-D array (fp32 values): normalised by its Frobenius norm (summed in double), then `steps`
    Newton-Schulz iterations in `dtype`.  All zeros give all zeros."""
    a, b, c = (dtype(v) for v in coeffs)
    G = np.asarray(G)
    assert G.ndim == 2
    nrm = np.sqrt(np.sum(G.astype(np.float64) ** 2))
    X = (G.astype(np.float64) / (nrm + NS_EPS)).astype(dtype)
    tall = G.shape[0] > G.shape[1]
    if tall:
        X = X.T
    for _ in range(steps):
        A = X @ X.T
        B = b * A + c * (A @ A)
        X = a * X + B @ X
    return np.ascontiguousarray(X.T if tall else X)


def scale_of(rows, cols, mode="match_rms_adamw"):
    if mode == "original":
        return float(np.sqrt(max(1.0, rows / cols)))
    if mode == "match_rms_adamw":
        return 0.2 * float(np.sqrt(max(rows, cols)))
    raise ValueError(mode)


def step(w, m, g, *, lr, wd=0.0, mu=0.95, nesterov=True, ns_steps=5, scale="match_rms_adamw", decoupled=False, gscale=1.0, ns_dtype=np.float64):
    """One step of one parameter in fp64 from its fp32 operands (arrays shaped like the parameter) -> dict with the new momentum "m",
    the direction "u", its norm "norm", the orthogonalised direction "O" (shaped like the parameter) and the new weights "w"."""
    shape = np.asarray(w).shape
    w64, m64, g64 = (np.asarray(x).astype(np.float64) for x in (w, m, g))
    gr = g64 * float(gscale)
    if not decoupled:
        gr = gr + float(wd) * w64
    m1 = mu * m64 + (1.0 - mu) * gr
    u = (1.0 - mu) * gr + mu * m1 if nesterov else m1
    U = as_matrix(u)
    O = ns(U.astype(np.float32), ns_steps, ns_dtype).astype(np.float64).reshape(shape)
    s = scale_of(U.shape[0], U.shape[1], scale)
    w1 = w64 * (1.0 - lr * wd) if decoupled else w64
    w1 = w1 - (lr * s) * O
    return {"m": m1, "u": u, "norm": float(np.sqrt(np.sum(u ** 2))), "O": O, "w": w1, "s": s}


def rms(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.sqrt(np.mean(x ** 2))) if x.size else 0.0


def ns_tolerance(G, steps=5, factor=8.0):
    """-> (O64, tol): the fp64 result for the fp32 input G and the largest element deviation allowed to an fp32 implementation:
    factor * max(max|O32 - O64|, 1e-5 rms(O64)) with O32 the same iteration in numpy fp32"""
    G = np.asarray(G, dtype=np.float32)
    o64 = ns(G, steps, np.float64)
    o32 = ns(G, steps, np.float32).astype(np.float64)
    return o64, factor * max(float(np.max(np.abs(o32 - o64))) if o64.size else 0.0, 1e-5 * rms(o64))


def inputs(kind, rows, cols, rng):
    """the input kinds of the device test, as fp32: "gauss"; "lowrank": rank d/4 (at least 1) plus 1e-3 noise; "rowscale": Gaussian rows
    scaled by exp(2 N(0, 1)) 1e-4; "zeros" """
    d = min(rows, cols)
    if kind == "gauss":
        x = rng.standard_normal((rows, cols))
    elif kind == "lowrank":
        k = max(1, d // 4)
        x = rng.standard_normal((rows, k)) @ rng.standard_normal((k, cols)) + 1e-3 * rng.standard_normal((rows, cols))
    elif kind == "rowscale":
        x = rng.standard_normal((rows, cols)) * (np.exp(2.0 * rng.standard_normal((rows, 1))) * 1e-4)
    elif kind == "zeros":
        x = np.zeros((rows, cols))
    else:
        raise ValueError(kind)
    return x.astype(np.float32)
