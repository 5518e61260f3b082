"""NumPy restatement of iq_reward_classes and iq_shapley_accum_games (include/iq.h): the per-class reward in float32 in the
kernel's order, the accumulation as the reference's host loop (final_shapley_value.py:145-150, once per game)."""
import numpy as np

F32 = np.float32


def reward_row(z, label, modified):
    """One row of logits ``z`` (C,) float32 -> the float32 reward of ``label``: maximum and sum over c ascending, the label
    skipped when ``modified``; a maximum of +-inf is not subtracted; zy - (log(s) + m) modified, (zy - m) - log(s) normal."""
    z = np.asarray(z, dtype=F32)
    with np.errstate(all="ignore"):
        m = F32(-np.inf)
        for c in range(z.size):
            if not modified or c != label:
                m = max(m, z[c])
        ms = F32(0) if np.isinf(m) else m
        s = F32(0)
        for c in range(z.size):
            if not modified or c != label:
                s = F32(s + np.exp(F32(z[c] - ms)))
        if modified:
            return F32(z[label] - F32(np.log(s) + ms))
        return F32(F32(z[label] - ms) - np.log(s))


def reward_classes(logits, labels=None, modified=True):
    """logits (B,C) -> (G,B) float32; ``labels`` None = 0 .. C-1."""
    logits = np.asarray(logits, dtype=F32)
    labels = list(range(logits.shape[1])) if labels is None else [int(x) for x in labels]
    return np.array([[reward_row(row, lab, modified) for row in logits] for lab in labels], dtype=F32).reshape(len(labels), logits.shape[0])


def shapley_accum_games(v, orders, snap_counts=()):
    """v (G,M >= S*(R+1)) float32, orders (S,R) -> (total (G,R) float64, snaps (G,len(snap_counts),R) float64): float32
    differences, widened, added per region in permutation order; a region a row does not name gets nothing from it."""
    v = np.asarray(v, dtype=F32)
    orders = np.asarray(orders)
    s, r = orders.shape
    total = np.zeros((v.shape[0], r))
    snaps = np.zeros((v.shape[0], len(snap_counts), r))
    for g in range(v.shape[0]):
        for o in range(s):
            row = v[g, o * (r + 1):(o + 1) * (r + 1)]
            dv = row[1:] - row[:-1]                       # float32
            for j in range(r):
                if 0 <= orders[o, j] < r:
                    total[g, orders[o, j]] += np.float64(dv[j])
            for k, count in enumerate(snap_counts):
                if count == o + 1:
                    snaps[g, k] = total[g]
    return total, snaps
