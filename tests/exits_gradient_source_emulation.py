"""The exit list of the gradient on a scene with a source term in numpy (a helper of the tests, not a test): how
wost_exits_apply_gradient joins the in-ball term a list carries (include/wost.h "Exit lists of the gradient", item 4) to the walk
part that exits_gradient_emulation.py computes, in float64 and in the order the header states, rounded to float32 once.

The term is three float64 arrays per list, as exits_gradient_terms() returns them: T and seT (n, dim, 3), U (n, 3).  They do not
depend on the colours, so every one of the K sets gets the same ones:
    grad = walk part + T,   stderr = sqrt(walk part^2 + seT^2),   field = mean + U;
a degenerate point: NaN, NaN and its mean without U."""
import numpy as np

import exits_gradient_emulation as xg

F32 = np.float32


def join(grad, stderr, mean, T, seT, U, degenerate):
    """the walk part of one set -- grad, stderr (n, dim, 3) and mean (n, 3), float64, NaN where exits_gradient_emulation.reduce
    puts it -- and the term -> (grad, stderr, field) float32.  Each line is one float64 operation per entry."""
    deg = np.asarray(degenerate, bool)
    with np.errstate(invalid="ignore"):
        g = np.asarray(grad, np.float64) + np.asarray(T, np.float64)
        se = np.asarray(stderr, np.float64)
        se_t = np.asarray(seT, np.float64)
        se = np.sqrt(se * se + se_t * se_t)
    m = np.asarray(mean, np.float64)
    field = np.where(deg[:, None], m, m + np.asarray(U, np.float64))
    g[deg] = se[deg] = np.nan
    return g.astype(F32), se.astype(F32), field.astype(F32)


def apply(rec, grec, color_sets, prims, intensity, eps, dim, T, seT, U):
    """exits_gradient_emulation.apply with the term joined to every set -> {"grad", "stderr": (K, n, dim, 3), "field": (K, n, 3)},
    float32"""
    walk = xg.apply(rec, grec, color_sets, prims, intensity, eps, dim)
    deg = xg.degenerate(grec["radius"], eps)
    parts = [join(walk["grad"][k], walk["stderr"][k], walk["field"][k], T, seT, U, deg) for k in range(len(walk["grad"]))]
    return {"grad": np.stack([p[0] for p in parts]), "stderr": np.stack([p[1] for p in parts]), "field": np.stack([p[2] for p in parts])}
