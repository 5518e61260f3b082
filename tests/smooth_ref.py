"""A plain NumPy restatement of the smoothness enumeration's contract (include/iq.h: iq_smoothness_enum), written as closed forms:
no autograd, no torch.  Own code, from include/iq.h and oracle/ref_cpu.py (smoothness_enumerate); tests/test_smooth_edges_cpu.py
holds it to the float64 run of that oracle, which proves the closed-form gradient against autograd once, and
tests/test_smooth_edges_gpu.py uses its float64 run as the anchor of the kernel.

Per region of S >= 2 points, X the region's points (S,3), X0 the same points of ``origin``:
  orientations   o1, o2, o3 = eigenvectors of cov(X0) = (X0 - mean)^T (X0 - mean) / (S - 1), largest eigenvalue first (np.linalg.eigh)
  variances      p_k = X o_k, m_k = mean(p_k), var_k = sum (p_k - m_k)^2 / (S - 1)
  bounds         var_k is DETACHED (a constant for the gradient) when var_k > var0_k + var_threshold or var_k < var0_k - var_threshold
  order          stable argsort of (var_1, var_2, var_3), NaN last -> s_min, s_mid, s_max
  smoothness     linearity (s_max - s_mid) / s_max, planarity (s_mid - s_min) / s_max, scattering s_min / s_max
  gradient       d smoothness / d X = sum_k c_k (2 / (S - 1)) (p_k - m_k) o_k^T, c_k = d smoothness / d var_k, 0 for a detached var_k;
                 there is NO gradient when every variance the ratio reads (linearity: max, mid; planarity: all; scattering: max, min)
                 is detached - the region then stops
  step           X <- X +- step g / |g|_F, or X <- X +- 1e-8 (every coordinate) when |g|_F == 0
  distance       count = #{i : |X_i - X0_i| > dist_threshold}; such a point is projected back to X0_i + dist_threshold (X_i - X0_i) /
                 |X_i - X0_i| only with ``project_to_bound``
  stop           count / S > stop_ratio, or no gradient, or iterations of this epoch > max_iteration
An epoch runs steps while smoothness < target (inc; > for dec), target = the smoothness recorded by the previous epoch +- enum_step;
a region that stopped keeps its points and its recorded smoothness.  NaN smoothness enters no step.

``dtype``: every array and threshold in that precision (float64: the anchor; float32: a second float32 yardstick where the oracle
has no such path, i.e. ``project_to_bound``).  ``variant``: one deliberately WRONG reading of the contract (VARIANTS), for the power
test.  Not collected by pytest (no test_ prefix)."""
import numpy as np

MODES = ("linearity", "planarity", "scattering")
DEFAULTS = dict(step=1e-3, enum_step=0.05, var_threshold=0.003, dist_threshold=0.03, stop_ratio=0.5, epochs=50, max_iteration=100)
# wrong on purpose: the detach flags ignored; the coefficients of the middle and the smallest variance swapped; the mean not
# subtracted in the gradient; S for S - 1 in the variance (and in the covariance)
VARIANTS = ("ignore_detach", "swap_mid_min", "no_mean", "biased_var")


def orientations(x0, ddof=1):
    """(S,3) -> (3,3), ROW k the orientation o_{k+1}; eigenvalues of the covariance descending (3,)."""
    d = x0 - x0.mean(axis=0)
    cov = d.T @ d / x0.dtype.type(x0.shape[0] - ddof)
    w, v = np.linalg.eigh(cov)
    return np.ascontiguousarray(v[:, ::-1].T), w[::-1].copy()


def variances(x, o, ddof=1):
    p = x @ o.T                                        # (S,3): column k the projection on o_k
    m = p.mean(axis=0)
    return ((p - m) ** 2).sum(axis=0) / x.dtype.type(x.shape[0] - ddof), p, m


def ratio(mode, s_min, s_mid, s_max):
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == "linearity":
            return (s_max - s_mid) / s_max
        if mode == "planarity":
            return (s_mid - s_min) / s_max
        return s_min / s_max


def coefficients(mode, s_min, s_mid, s_max):
    """d ratio / d (s_min, s_mid, s_max) and which of the three the ratio reads."""
    one = s_max.dtype.type(1)
    if mode == "linearity":
        return (0 * one, -one / s_max, one / s_max - (s_max - s_mid) / (s_max * s_max)), (False, True, True)
    if mode == "planarity":
        return (-one / s_max, one / s_max, -(s_mid - s_min) / (s_max * s_max)), (True, True, True)
    return (one / s_max, 0 * one, -s_min / (s_max * s_max)), (True, False, True)


def enumerate_regions(pts, rid, num_regions, mode, objective, origin=None, project_to_bound=False, dtype=np.float64, variant=None,
                      **overrides):
    """pts (N,3), rid (N,) -> dict: data (E,N,3), smoothness (E,R), var (E,R,3), orig (R,4), stop_epoch (R,) - the outputs of
    iq_smoothness_enum, in ``dtype`` - and trace {region: dict(iters [steps taken per epoch], stop (epoch, or None), steps
    [(order (3,), live (3,), count)])} for every region of at least two points."""
    assert mode in MODES and objective in ("inc", "dec") and variant in (None,) + VARIANTS
    prm = dict(DEFAULTS, **overrides)
    f = np.dtype(dtype).type
    step, vth, dth = f(prm["step"]), f(prm["var_threshold"]), f(prm["dist_threshold"])
    E, R, N = int(prm["epochs"]), int(num_regions), pts.shape[0]
    sign = 1.0 if objective == "inc" else -1.0
    ddof = 0 if variant == "biased_var" else 1
    pts = np.asarray(pts).astype(dtype)
    org_all = pts if origin is None else np.asarray(origin).astype(dtype)
    rid = np.asarray(rid)
    data = np.repeat(pts[None], E, axis=0)
    smooth_out, var_out = np.full((E, R), np.nan, dtype), np.full((E, R, 3), np.nan, dtype)
    orig, stop_epoch, trace = np.full((R, 4), np.nan, dtype), np.full((R,), -1, np.int32), {}
    for r in range(R):
        sel = np.flatnonzero(rid == r)
        S = len(sel)
        if S < 2:
            continue
        x0, x = org_all[sel], pts[sel].copy()
        o, _ = orientations(x0, ddof)
        var0 = variances(x0, o, ddof)[0]
        ub, lb = var0 + vth, var0 - vth
        order = np.argsort(var0, kind="stable")
        smooth = ratio(mode, *var0[order])
        orig[r, :3], orig[r, 3] = var0, smooth
        tr = trace[r] = dict(iters=[], stop=None, steps=[])
        active, stop, last = True, E, var0
        for e in range(E):
            it = 0
            if active:
                target = float(smooth) + sign * prm["enum_step"]
                sm = smooth
                while (float(sm) < target) if sign > 0 else (float(sm) > target):
                    var, p, m = variances(x, o, ddof)
                    last = var
                    live = ~((var > ub) | (var < lb))
                    if variant == "ignore_detach":
                        live = np.ones(3, bool)
                    order = np.argsort(var, kind="stable")
                    s_min, s_mid, s_max = var[order]
                    sm = ratio(mode, s_min, s_mid, s_max)
                    c_sorted, reads = coefficients(mode, s_min, s_mid, s_max)
                    if variant == "swap_mid_min":
                        c_sorted = (c_sorted[1], c_sorted[0], c_sorted[2])
                    has_grad = any(rd and live[k] for rd, k in zip(reads, order))
                    if has_grad:
                        c = np.zeros(3, dtype)
                        for ck, k in zip(c_sorted, order):
                            c[k] = ck if live[k] else 0
                        dev = p if variant == "no_mean" else p - m
                        g = (dev * (c * f(2) / f(S - ddof))) @ o                   # (S,3)
                        norm = np.sqrt((g * g).sum())
                        delta = step * g / norm if norm != 0 else f(1e-8)
                        x = x + delta if sign > 0 else x - delta
                    diff = x - x0
                    dist = np.sqrt((diff * diff).sum(axis=1))
                    far = dist > dth
                    count = int(far.sum())
                    if project_to_bound and count:
                        x[far] = x0[far] + dth * diff[far] / dist[far, None]
                    tr["steps"].append((tuple(int(k) for k in order), tuple(bool(b) for b in live), count))
                    it += 1
                    if count / S > prm["stop_ratio"] or not has_grad or it > prm["max_iteration"]:
                        active, stop = False, e
                        tr["stop"] = e
                        break
                smooth = sm
            tr["iters"].append(it)
            data[e, sel] = x
            smooth_out[e, r], var_out[e, r] = smooth, last
        stop_epoch[r] = stop
    return dict(data=data, smoothness=smooth_out, var=var_out, orig=orig, stop_epoch=stop_epoch, trace=trace)
