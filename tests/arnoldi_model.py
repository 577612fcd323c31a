"""Extended-precision model of ONE step of the lockstep GMRES' Arnoldi / Givens layer (ricadi_arnoldi.hip: the three
passes dots, update + dots, update [+ Hessenberg]; the one-reduction form K3L; cycle start; back substitution and
correction) with the componentwise bound a correct FP64 implementation of each quantity satisfies.

Plain NumPy on top of dense_model (``ld``, ``gamma``, ``ratio``) and precond_model (``to_fp16``, ``to_fp32``): no GPU.

How a step is judged.  The inputs of every stage are values the DEVICE holds and the kernels themselves read from
memory -- the stored Krylov vectors and w, and, stage by stage, the coefficients h1, h2, the rotations, g, the reduced
sums and the pending column read back after the step -- so no error compounds from step to step or from stage to
stage.  A stage's model runs in ``np.longdouble``; what it may differ by from a correct FP64 evaluation:

* a dot product of n terms: ``gamma(n, u) sum |a_i b_i|`` -- whatever the order of summation, FMA or not, per-chunk
  partials or not (dense_model);  a sum of k products with l more roundings applied to it: ``gamma(k + l, u)``;
* a quantity that is NOT stored between two stages (w' where w is kept, h_{j+1,j}, 1 / r_j) carries its bound into the
  next stage to first order: through the square root ``b / (2 sqrt x)``, the quotient, the rotations
  (``|c| b_cur + |s| b_nxt``) and ``1 / hnext`` (``b / hnext^2``);
* sqrt, division and hypot of the device library: ``ULP_LIBM`` units in the last place each (the OpenCL bound for
  hypot; the first two are correctly rounded -- one allowance keeps the formulas short);
* u = 2^-53 + u_longdouble throughout (``UT``): the model's own arithmetic gets the same analysis.

Stored vectors (``check_stored``): the model value x with bound b; the device must hold the stored type's rounding
of SOME FP64 number in [x - b, x + b].  Rounding is monotone, so that is lo <= dev <= hi with lo, hi the roundings of
the interval ends; where both coincide it is exact equality.  For the FP16 basis the rounding through FP32,
RN16(RN32(.)), is accepted beside the direct RN16 (a compiler may convert either way); ``StoreStats`` counts which of
the two the device matches where they differ, the entries accepted only because the interval straddles a rounding
boundary (fewer than one per 10^6 entries of a case, ``StoreStats.ok``) and that those are within one unit in the last
place.

Frozen columns (``!(sub > 1e-300) || |g_j| <= 0.01 tol ||b||``): the models apply the rule as the kernels do, to the
device's own values; every bound of an inert quantity is then zero, i.e. the comparison is exact equality
(``ratio``: a non-zero error against a zero bound is inf).

``Float64Device`` is a float64 NumPy implementation of the same steps with the workspace layout of the library (what
``check_case`` reads through the ``read`` interface), storage emulated with ``to_fp16`` / ``to_fp32``; it takes one
``mutation`` -- the faults the bounds exist to catch.  ``check_case`` drives a device (that one, or the GPU probe)
through a whole cycle and returns the largest error / bound per quantity.
"""
import numpy as np

from dense_model import LD, U, U_REF, gamma, ld, ratio
from precond_model import to_fp16, to_fp32

TINY = 1e-300
UT = U + U_REF
ULP_LIBM = 4
FORM_BITS = ("b16", "b32", "h16", "keepw", "fuseh", "x32", "w32", "lowsync")
MUTATIONS = ("drop_last_vector", "swap_cs_sn", "h1_only", "skip_second_pass", "rotation_wrong_pair", "stale_parity",
             "backsolve_extra_column", "ignore_g_frozen")


def f64(a):
    return np.asarray(a, dtype=np.float64)


def fa(a):
    return np.abs(f64(a))


def store_fn(form):
    return to_fp16 if form["b16"] else to_fp32 if form["b32"] else f64


def frozen_rule(sub, gabs, thr):
    """column_frozen of ricadi_arnoldi.hip, elementwise."""
    return ~(f64(sub) > TINY) | (f64(gabs) <= f64(thr))


def threshold(tol, bnorm):
    return 0.01 * tol * f64(bnorm)          # evaluated as the kernels do: (0.01 * tol) * ||b||


# ------------------------------------------------------------------------------------------------ vector stages
def dots(V, w):
    """``V_i^T w`` per column: V [k, n, m], w [n, m] -> value [k, m], bound [k, m] (n-term dot products)."""
    V, w = ld(V), ld(w)
    n = w.shape[0]
    val = np.einsum("knm,nm->km", V, w) if V.shape[0] else np.zeros((0, w.shape[1]), dtype=LD)
    bnd = gamma(n, UT) * np.einsum("knm,nm->km", fa(V), fa(w)) if V.shape[0] else np.zeros((0, w.shape[1]))
    return val, bnd


def combine(w, V, coef, extra=2):
    """``w - sum_i coef_i V_i`` per column: value [n, m] and bound (k FMAs, ``extra`` more roundings: the sum of two
    accumulators and the subtraction)."""
    k = V.shape[0]
    val = ld(w) - np.einsum("knm,km->nm", ld(V), ld(coef))
    bnd = gamma(k + extra, UT) * (fa(w) + np.einsum("knm,km->nm", fa(V), fa(coef)))
    return val, bnd


def dots_perturbed(V, x, bx):
    """``V_i^T x`` and ``x^T x`` (last row) for a vector x known to within bx: first-order propagation on top of the
    dot-product bounds."""
    val, bnd = dots(V, x)
    bnd = bnd + np.einsum("knm,nm->km", fa(V), f64(bx))
    n = x.shape[0]
    xx = np.einsum("nm,nm->m", ld(x), ld(x))
    bxx = gamma(n, UT) * f64(xx) + 2.0 * np.einsum("nm,nm->m", fa(x), f64(bx)) + np.einsum("nm,nm->m", f64(bx), f64(bx))
    return np.concatenate([val, xx[None]]), np.concatenate([bnd, bxx[None]])


# ------------------------------------------------------------------------------------------------ scalar stages
def sqrt_pos(x, bx):
    """``x > 0 ? sqrt(x) : 0`` with its bound (x as the device computed it, to within bx)."""
    x = ld(x)
    pos = x > 0
    s = np.sqrt(np.where(pos, x, LD(0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.where(pos, f64(bx) / (2.0 * f64(s)) + ULP_LIBM * UT * f64(s), 0.0)
    return s, np.where(np.isfinite(b), b, np.inf)


def apply_rotations(col, cs, sn, upto):
    """The stored rotations 0 .. upto-1 on a column [rows, m] (exact FP64 inputs): rotated entries 0 .. upto-1 with
    bounds, and the running entry ``cur`` with its bound.  Three roundings per output."""
    col = ld(col)
    m = col.shape[1]
    out, bout = np.zeros((upto, m), dtype=LD), np.zeros((upto, m))
    cur, bcur = col[0].copy(), np.zeros(m)
    for i in range(upto):
        c, s, nxt = ld(cs[:, i]), ld(sn[:, i]), col[i + 1]
        t, un = c * cur + s * nxt, -s * cur + c * nxt
        mag = fa(c * cur) + fa(s * nxt)
        out[i], bout[i] = t, gamma(3, UT) * mag + fa(c) * bcur
        bcur = gamma(3, UT) * (fa(s * cur) + fa(c * nxt)) + fa(s) * bcur
        cur = un
    return out, bout, cur, bcur


def givens_tail(cur, bcur, sub, bsub, gj):
    """givens_tail of ricadi_arnoldi.hip: d, cs_j, sn_j, g_j, g_{j+1}, estimate -- (value, bound) each."""
    cur, sub, gj = ld(cur), ld(sub), ld(gj)
    d = np.hypot(cur, sub)
    ok = f64(d) > TINY
    dd = np.where(ok, d, LD(1))
    bd = np.where(ok, (fa(cur) * bcur + fa(sub) * bsub) / f64(dd) + ULP_LIBM * UT * f64(d), 0.0)
    cj, sj = np.where(ok, cur / dd, LD(1)), np.where(ok, sub / dd, LD(0))
    bc = np.where(ok, (bcur + fa(cj) * bd) / f64(dd) + ULP_LIBM * UT * fa(cj), 0.0)
    bs = np.where(ok, (bsub + fa(sj) * bd) / f64(dd) + ULP_LIBM * UT * fa(sj), 0.0)
    g1, g0 = np.where(ok, -sj * gj, LD(0)), np.where(ok, cj * gj, LD(0))
    bg1, bg0 = bs * fa(gj) + UT * fa(g1), bc * fa(gj) + UT * fa(g0)
    return dict(diag=(np.where(ok, d, LD(1)), bd), cs=(cj, bc), sn=(sj, bs), g0=(g0, bg0), g1=(g1, bg1),
                est=(np.abs(g1), bg1))


# ------------------------------------------------------------------------------------------------ stored vectors
class StoreStats:
    """Entries compared, entries accepted only through a straddled rounding boundary, and -- FP16 -- the entries at
    which RN16(x) and RN16(RN32(x)) differ, by which of the two the device held."""

    def __init__(self):
        self.total = self.straddle = self.bad = self.far = self.direct = self.via32 = 0

    def ok(self):
        return self.bad == 0 and self.far == 0 and self.straddle * 10 ** 6 < max(self.total, 1)

    def __repr__(self):
        return "entries %d, straddling %d, outside %d, beyond one ulp %d, RN16 direct %d / through FP32 %d" % (
            self.total, self.straddle, self.bad, self.far, self.direct, self.via32)


def check_stored(dev, x, bx, form, stats):
    """The device's stored vector ``dev`` (as FP64) against the model value x +- bx (see the module docstring).
    FP64 storage: returns error / bound; FP16 / FP32: updates ``stats`` and returns 0 or inf."""
    x64 = f64(x)
    b = f64(bx) + U * np.abs(x64)               # (+ the rounding of the model value to FP64)
    dev = f64(dev)
    if not (form["b16"] or form["b32"]):
        return ratio(dev, x, b)
    if form["b16"]:
        rnd = (to_fp16, lambda v: to_fp16(to_fp32(v)))
    else:
        rnd = (to_fp32,)
    with np.errstate(over="ignore"):
        lo = np.minimum.reduce([r(x64 - b) for r in rnd])
        hi = np.maximum.reduce([r(x64 + b) for r in rnd])
        exact = [r(x64) for r in rnd]
    inside = (dev >= lo) & (dev <= hi)
    hit = np.logical_or.reduce([dev == e for e in exact])
    st = store_fn(form)
    spacing = np.abs(st(exact[0] * (1 + 2.0 ** -10 if form["b16"] else 1 + 2.0 ** -23)) - exact[0])
    spacing = np.maximum(spacing, 2.0 ** -24 if form["b16"] else 2.0 ** -149)
    stats.total += dev.size
    stats.bad += int(np.count_nonzero(~inside))
    stats.straddle += int(np.count_nonzero(inside & ~hit))
    stats.far += int(np.count_nonzero(inside & ~hit & (np.abs(dev - exact[0]) > spacing)))
    if form["b16"]:
        differ = exact[0] != exact[1]
        stats.direct += int(np.count_nonzero(differ & (dev == exact[0])))
        stats.via32 += int(np.count_nonzero(differ & (dev == exact[1])))
    return 0.0 if inside.all() else float("inf")


# ------------------------------------------------------------------------------------------------ three-pass form
def cgs2_expect(V, w, j, pre, post, form, tol):
    """Expected values of step j of the three-pass form for ONE group.  V [j+1, n, m]: the stored vectors; w [n, m]
    as stored; pre: cs, sn, g, est (the estimate buffer the step reads), bnorm before the step; post: h1, h2 and --
    where the form stores them -- wp (w'), scale after it.  Returns name -> (value, bound)."""
    nv = j + 1
    exp = {}
    exp["h1"] = dots(V, w)
    h1 = post["h1"][:nv]
    if form["keepw"]:
        wp, bwp = combine(w, V, h1)
        exp["h2"] = dots_perturbed(V, wp, bwp)
    else:
        exp["wp"] = combine(w, V, h1)
        exp["h2"] = dots_perturbed(V, post["wp"], np.zeros_like(post["wp"]))
    h2, ww = post["h2"][:nv], post["h2"][nv]
    hcol = h1 + h2                                   # FP64 sum of two stored FP64 values: exact to the bit
    exp["hsum"] = (hcol, np.zeros_like(hcol))
    h2sq = np.einsum("km,km->m", ld(h2), ld(h2))
    hn2 = ld(ww) - h2sq
    hnext, bh = sqrt_pos(hn2, gamma(nv, UT) * f64(h2sq) + UT * fa(hn2))
    gabs = pre["est"] if form["fuseh"] else np.abs(pre["g"][:, j])
    frozen = frozen_rule(hnext, gabs, threshold(tol, pre["bnorm"]))
    hnext, bh = np.where(frozen, LD(0), hnext), np.where(frozen, 0.0, bh)
    col = np.concatenate([hcol, np.zeros((1, hcol.shape[1]))])
    rot, brot, cur, bcur = apply_rotations(col, pre["cs"], pre["sn"], j)
    tail = givens_tail(cur, bcur, hnext, bh, pre["g"][:, j])
    exp["Hcol"] = (np.concatenate([rot, tail["diag"][0][None], np.zeros((1, rot.shape[1]), dtype=LD)]),
                   np.concatenate([brot, tail["diag"][1][None], np.zeros((1, rot.shape[1]))]))
    for k in ("cs", "sn", "g0", "g1", "est"):
        exp[k] = tail[k]
    live = f64(hnext) > TINY
    hs = np.where(live, hnext, LD(1))
    scale = np.where(live, 1 / hs, LD(0))
    bscale = np.where(live, bh / f64(hs) ** 2 + ULP_LIBM * UT * f64(scale), 0.0)
    exp["scale"] = (scale, bscale)
    if form["fuseh"]:
        sc, bsc = scale, bscale                      # derived inside the launch, never stored
    else:
        sc, bsc = ld(post["scale"]), np.zeros_like(bscale)
    if form["keepw"]:
        t, bt = combine(w, V, hcol, extra=3)         # (one more: the sum h1 + h2 is formed per workgroup)
    else:
        t, bt = combine(post["wp"], V, h2)
    exp["vnext"] = (t * sc, fa(sc) * bt + fa(t) * bsc + UT * fa(t * sc))
    exp["frozen"] = frozen
    return exp


# ------------------------------------------------------------------------------------------------ one-reduction form
def ls_layout(coef, restart):
    """ls_coef of one group [4 restart + 10, 16] -> sums [restart + 2, 2, 16], pending [2] of (p, rho, gj)."""
    ns = 2 * (restart + 2)
    sums = coef[:ns].reshape(restart + 2, 2, 16)
    pend = []
    for par in range(2):
        blk = coef[ns + par * (restart + 3): ns + (par + 1) * (restart + 3)]
        pend.append((blk[:restart + 1], blk[restart + 1], blk[restart + 2]))
    return sums, pend


def lowsync_sums(V, u, w):
    """The reduced sums of step j: S rows 0 .. j+1 = V^T u, u^T u, w^T w;  T rows = V^T w, u^T w, 0.  w None: the
    end-of-cycle pass (T = 0, S_{j+1} = 0)."""
    m = u.shape[1]
    s, bs = dots(np.concatenate([V, u[None]]), u)
    if w is None:
        z = np.zeros((1, m))
        return (np.concatenate([s, ld(z)]), np.concatenate([bs, z])), (np.zeros((s.shape[0] + 1, m), dtype=LD),
                                                                      np.zeros((s.shape[0] + 1, m)))
    t, bt = dots(np.concatenate([V, u[None]]), w)
    ww, bww = dots(w[None], w)
    z = np.zeros((1, m))
    return (np.concatenate([s, ww]), np.concatenate([bs, bww])), (np.concatenate([t, ld(z)]), np.concatenate([bt, z]))


def lowsync_complete(S, j, pend_prev, pre, tol, restart):
    """Completion of column j-1 (ls_column, ``complete``) from the device's reduced sums S [j+1, m], the pending column
    of parity (j-1) & 1 and the rotations / g before the step.  Returns the expectations and (r, b_r, dead)."""
    p, rho, gj = pend_prev
    ssq = np.einsum("km,km->m", ld(S[:j]), ld(S[:j]))
    r2 = ld(S[j]) - ssq
    r, br = sqrt_pos(r2, gamma(j, UT) * f64(ssq) + UT * fa(r2))
    sub = ld(rho) * r
    bsub = fa(rho) * br + UT * fa(sub)
    dead = frozen_rule(sub, np.abs(gj), threshold(tol, pre["bnorm"]))
    sub, bsub = np.where(dead, LD(0), sub), np.where(dead, 0.0, bsub)
    col = ld(p[:j]) + ld(rho) * ld(S[:j])            # fma(rho, S_i, p_i): one rounding each
    bcol = UT * fa(col)
    col = np.concatenate([col, np.zeros((1, col.shape[1]), dtype=LD)])
    # (the rounding of the column's entries enters the rotations as an input perturbation)
    rot, brot, cur, bcur = apply_rotations(col, pre["cs"], pre["sn"], j - 1)
    infl = np.cumsum(bcol, axis=0)                   # each rotated entry depends on the entries up to its pair
    brot = brot + (infl[1:j] if j > 1 else infl[:0])
    bcur = bcur + infl[j - 1]
    tail = givens_tail(cur, bcur, sub, bsub, gj)
    m = col.shape[1]
    exp = {"Hcol": (np.concatenate([rot, tail["diag"][0][None], np.zeros((1, m), dtype=LD)]),
                    np.concatenate([brot, tail["diag"][1][None], np.zeros((1, m))]))}
    for k in ("cs", "sn", "g0", "g1"):
        exp[k] = tail[k]
    return exp, (r, br, dead)


def lowsync_expect(V, u, w, j, pre, post, tol, restart):
    """Expected values of step j of the one-reduction form for ONE group.  V [j, n, 16]: v_0 .. v_{j-1}; u: slot j as
    stored before the step; w [n, 16] as stored (FP32).  pre: cs, sn, g, bnorm, pend (both parities) before the step;
    post: sums (S, T), cs, sn, g, pend, vj (slot j) after it."""
    m = u.shape[1]
    exp = {}
    exp["S"], exp["T"] = lowsync_sums(V, u, w)
    S, T = post["S"], post["T"]
    r, br, dead = ld(np.ones(m)), np.zeros(m), np.zeros(m, dtype=bool)
    if j > 0:
        exp["complete"], (r, br, dead) = lowsync_complete(S, j, pre["pend"][(j - 1) & 1], pre, tol, restart)
    live = ~dead & (f64(r) > TINY)
    rs = np.where(live, r, LD(1))
    invr = np.where(live, 1 / rs, LD(0))
    binvr = np.where(live, br / f64(rs) ** 2 + ULP_LIBM * UT * f64(invr), 0.0)
    st = np.einsum("km,km->m", ld(S[:j]), ld(T[:j]))
    tsq = np.einsum("km,km->m", ld(T[:j]), ld(T[:j]))
    num = ld(T[j]) - st
    bnum = gamma(j + 1, UT) * (fa(T[j]) + np.einsum("km,km->m", fa(S[:j]), fa(T[:j])))
    hjj = num * invr
    bhjj = fa(invr) * bnum + fa(num) * binvr + UT * fa(hjj)
    ww = ld(S[j + 1])
    wn, bwn = sqrt_pos(np.maximum(ww, 0), np.zeros(m))
    rho2 = ww - tsq - hjj * hjj
    brho2 = gamma(j + 3, UT) * (fa(ww) + f64(tsq) + f64(hjj * hjj)) + 2 * fa(hjj) * bhjj
    rs2, brs2 = sqrt_pos(rho2, brho2)
    floor, bfloor = LD(1e-3) * wn, 1e-3 * bwn + UT * f64(wn) * 1e-3
    rho = np.maximum(rs2, floor)
    brho = np.maximum(brs2, bfloor)                  # max of two bounded quantities
    off = dead | ~(f64(rho) > TINY)
    rho, brho = np.where(off, LD(0), rho), np.where(off, 0.0, brho)
    hjj, bhjj = np.where(dead, LD(0), hjj), np.where(dead, 0.0, bhjj)
    pcol = np.concatenate([np.where(dead[None], 0.0, T[:j]), f64(hjj)[None]])
    exp["p"] = (ld(pcol), np.concatenate([np.zeros((j, m)), bhjj[None]]))
    exp["rho"] = (rho, brho)
    exp["pend_g"] = (ld(post["g"][:, j]), np.zeros(m))            # a copy of g_j as the completion left it
    # provisional estimate: the pending column as the device stored it through the rotations after the step
    pdev, rhodev, gjdev = post["pend"][j & 1]
    thr = threshold(tol, pre["bnorm"])
    sub = np.where(dead | (np.abs(gjdev) <= thr), 0.0, rhodev)
    col = np.concatenate([pdev[:j + 1], np.zeros((1, m))])
    _, _, cur, bcur = apply_rotations(col, post["cs"], post["sn"], j)
    d = np.hypot(ld(cur), ld(sub))
    ok = f64(d) > TINY
    dd = np.where(ok, d, LD(1))
    est = np.where(ok, np.abs(ld(sub) / dd * ld(gjdev)), LD(0))
    bd = np.where(ok, fa(cur) * bcur / f64(dd) + ULP_LIBM * UT * f64(d), 0.0)
    exp["est"] = (est, np.where(ok, f64(est) * bd / f64(dd) + 3 * ULP_LIBM * UT * f64(est), 0.0))
    # v_j = (u - V s) / r_j;  u_{j+1} = (w - V t - v_j h_jj) / rho_j with the STORED v_j, h_jj and rho_j
    t, bt = combine(u, V, S[:j]) if j else (ld(u), np.zeros_like(u))
    exp["vj"] = (t * invr, fa(invr) * bt + fa(t) * binvr + UT * fa(t * invr))
    hdev = np.where(dead, 0.0, pdev[j])
    sig = np.where(f64(rhodev) > 0, 1.0 / np.where(f64(rhodev) > 0, ld(rhodev), LD(1)), LD(0))
    coef = np.concatenate([T[:j], hdev[None]])
    t2, bt2 = combine(w, np.concatenate([V, post["vj"][None]]), coef, extra=3)
    exp["unext"] = (t2 * sig, fa(sig) * bt2 + (ULP_LIBM + 1) * UT * fa(t2 * sig))
    exp["dead"] = dead
    return exp


# ------------------------------------------------------------------------------------------------ cycle start / end
def start_expect(r):
    """Cycle start of one group from the residual panel r [n, m]: nrm2, beta = g_0 = estimate, scale, v_0 unrounded."""
    n = r.shape[0]
    nrm2 = np.einsum("nm,nm->m", ld(r), ld(r))
    bn = gamma(n, UT) * f64(nrm2)
    return {"nrm2": (nrm2, bn)}


def start_from_nrm2(nrm2):
    """... the scalars and v_0 from the device's own nrm2."""
    beta, bb = sqrt_pos(np.maximum(ld(nrm2), 0), np.zeros(np.shape(nrm2)))
    live = f64(beta) > TINY
    bs = np.where(live, beta, LD(1))
    scale = np.where(live, 1 / bs, LD(0))
    bscale = np.where(live, bb / f64(bs) ** 2 + ULP_LIBM * UT * f64(scale), 0.0)
    return {"beta": (beta, bb), "scale": (scale, bscale)}


def backsolve_residual(Hdev, gdev, y, k):
    """Largest ``|R y - g| / (gamma_k |R| |y|)`` over the columns of one group: Hdev [m, restart, restart + 1]
    (column-major per panel column: Hdev[c, col, row]), gdev [m, restart + 1], y [restart, m]."""
    worst = 0.0
    for c in range(Hdev.shape[0]):
        R = np.triu(Hdev[c, :k, :k].T)
        yy = y[:k, c]
        res = ld(R) @ ld(yy) - ld(gdev[c, :k])
        worst = max(worst, ratio(res, np.zeros(k), gamma(k + 1, UT) * (fa(R) @ fa(yy))))
    return worst


def correction_expect(x0, Z, y, k):
    """``x0 + sum_{i < k} y_i Z_i`` with its bound: x0 [n, m], Z [k.., n, m] (FP32 values), y [restart, m]."""
    val = ld(x0) + np.einsum("knm,km->nm", ld(Z[:k]), ld(y[:k]))
    bnd = gamma(k + 3, UT) * (fa(x0) + np.einsum("knm,km->nm", fa(Z[:k]), fa(y[:k])))
    return val, bnd


# ------------------------------------------------------------------------------------------------ float64 device
class Float64Device:
    """The steps in float64 NumPy with the library's workspace layout.  ``form``: the IterationForm bits;
    ``mutation``: one of MUTATIONS or None."""

    def __init__(self, n, restart, tol, form, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.n, self.restart, self.tol, self.form, self.mut = n, restart, tol, dict(form), mutation
        self.store = store_fn(form)

    def begin(self, R, bnorm):
        ng, n, m = R.shape
        rs = self.restart
        nan = lambda *s: np.full(s, np.nan)
        self.ng, self.m = ng, m
        self.bnorm = f64(bnorm).copy()
        self.V = nan(rs + 1, ng, n, m)
        self.w, self.w32, self.vcur = R.copy(), nan(ng, n, m), nan(ng, n, m)
        self.h1, self.h2, self.hsum = nan(ng, rs + 2, m), nan(ng, rs + 2, m), nan(ng, rs + 2, m)
        self.H, self.cs, self.sn = nan(ng, m, rs, rs + 1), nan(ng, m, rs), nan(ng, m, rs)
        self.g = np.zeros((ng, m, rs + 1))
        self.y = nan(ng, rs, m)
        self.resid = nan(2, ng, m)
        self.ls = nan(ng, 4 * rs + 10, 16)
        self.nrm2 = np.einsum("gnm,gnm->gm", R, R)
        b = np.sqrt(np.maximum(self.nrm2, 0.0))
        self.g[:, :, 0] = b
        with np.errstate(divide="ignore"):
            self.scale = np.where(b > TINY, 1.0 / np.where(b > TINY, b, 1.0), 0.0)
        self.resid[0] = b
        v0 = self.store(R * self.scale[:, None, :])
        self.V[0] = v0
        if self.form["b16"] or self.form["b32"]:
            self.vcur = v0.copy()

    def _frozen(self, sub, gabs, thr):
        if self.mut == "ignore_g_frozen":
            return ~(sub > TINY)
        return frozen_rule(sub, gabs, thr)

    def _rotate(self, col, cs, sn, upto):
        """stored rotations on col [rows, m] in place; returns cur"""
        cur = col[0].copy()
        for i in range(upto):
            k = max(i - 1, 0) if self.mut == "rotation_wrong_pair" else i
            c, s = (sn[:, k], cs[:, k]) if self.mut == "swap_cs_sn" else (cs[:, k], sn[:, k])
            nxt = col[i + 1]
            col[i], cur = c * cur + s * nxt, -s * cur + c * nxt
        return cur

    def _tail(self, g, j, cur, sub, gj, Hc, cs, sn):
        d = np.hypot(cur, sub)
        ok = d > TINY
        dd = np.where(ok, d, 1.0)
        cj, sj = np.where(ok, cur / dd, 1.0), np.where(ok, sub / dd, 0.0)
        cs[:, j], sn[:, j] = cj, sj
        Hc[:, j], Hc[:, j + 1] = np.where(ok, d, 1.0), 0.0
        g[:, j + 1] = np.where(ok, -sj * gj, 0.0)
        g[:, j] = np.where(ok, cj * gj, 0.0)
        return np.where(ok, np.abs(sj * gj), 0.0)

    def step(self, j, W, groups):
        for g in groups:
            w = to_fp32(W[g]) if self.form["w32"] else f64(W[g]).copy()
            if self.form["w32"]:
                self.w32[g] = w
            else:
                self.w[g] = w
            (self._lowsync if self.form["lowsync"] else self._cgs2)(g, j, w)

    def _cgs2(self, g, j, w):
        f, nv, m = self.form, j + 1, self.m
        V = self.V[:nv, g]
        thr = threshold(self.tol, self.bnorm[g])
        h1 = np.einsum("knm,nm->km", V, w)
        if self.mut == "drop_last_vector":
            h1[nv - 1] = 0.0
        wp = w - np.einsum("knm,km->nm", V, h1)
        h2 = np.einsum("knm,nm->km", V, wp)
        ww = np.einsum("nm,nm->m", wp, wp)
        self.h1[g, :nv], self.h2[g, :nv], self.h2[g, nv] = h1, h2, ww
        if not f["keepw"]:
            self.w[g] = wp
        hn2 = ww - (0.0 if self.mut == "skip_second_pass" else np.einsum("km,km->m", h2, h2))
        hnext = np.where(hn2 > 0, np.sqrt(np.maximum(hn2, 0.0)), 0.0)
        est_in = self.resid[j & 1, g] if f["fuseh"] else np.abs(self.g[g, :, j])
        hnext = np.where(self._frozen(hnext, est_in, thr), 0.0, hnext)
        hsum = h1 + h2
        if f["keepw"] and not f["fuseh"]:
            self.hsum[g, :nv] = hsum
        col = np.concatenate([h1 if self.mut == "h1_only" else hsum, np.zeros((1, m))])
        cur = self._rotate(col, self.cs[g], self.sn[g], j)
        Hc = self.H[g, :, j, :]
        Hc[:, :j] = col[:j].T
        rnew = self._tail(self.g[g], j, cur, hnext, self.g[g, :, j].copy(), Hc, self.cs[g], self.sn[g])
        scale = np.where(hnext > TINY, 1.0 / np.where(hnext > TINY, hnext, 1.0), 0.0)
        if f["fuseh"]:
            self.resid[(j + 1) & 1, g] = rnew
        else:
            self.resid[0, g] = rnew
            self.scale[g] = scale
        t = (w - np.einsum("knm,km->nm", V, hsum)) if f["keepw"] else (wp - np.einsum("knm,km->nm", V, h2))
        v = self.store(t * scale)
        self.V[nv, g] = v
        if (f["b16"] or f["b32"]) and not f["h16"]:
            self.vcur[g] = v

    def _ls_column(self, g, j, S, T, with_w):
        rs, m = self.restart, self.m
        thr = threshold(self.tol, self.bnorm[g])
        sums, pend = ls_layout(self.ls[g], rs)
        r, dead = np.ones(m), np.zeros(m, dtype=bool)
        if j > 0:
            p, rho, gj = pend[(j & 1) if self.mut == "stale_parity" else ((j - 1) & 1)]
            p, rho, gj = p.copy(), rho.copy(), gj.copy()
            r2 = S[j] - np.einsum("km,km->m", S[:j], S[:j])
            r = np.where(r2 > 0, np.sqrt(np.maximum(r2, 0.0)), 0.0)
            sub = rho * r
            dead = self._frozen(sub, np.abs(gj), thr)
            sub = np.where(dead, 0.0, sub)
            col = np.concatenate([p[:j] + rho * S[:j], np.zeros((1, m))])
            cur = self._rotate(col, self.cs[g], self.sn[g], j - 1)
            Hc = self.H[g, :, j - 1, :]
            Hc[:, :j - 1] = col[:j - 1].T
            self._tail(self.g[g], j - 1, cur, sub, gj, Hc, self.cs[g], self.sn[g])
        if not with_w:
            return None
        live = ~dead & (r > TINY)
        invr = np.where(live, 1.0 / np.where(live, r, 1.0), 0.0)
        hjj = (T[j] - np.einsum("km,km->m", S[:j], T[:j])) * invr
        ww = S[j + 1]
        rho2 = ww - np.einsum("km,km->m", T[:j], T[:j]) - hjj * hjj
        rho = np.maximum(np.where(rho2 > 0, np.sqrt(np.maximum(rho2, 0.0)), 0.0), 1e-3 * np.sqrt(np.maximum(ww, 0.0)))
        rho = np.where(dead | ~(rho > TINY), 0.0, rho)
        hjj = np.where(dead, 0.0, hjj)
        pn, rhon, gn = pend[j & 1]
        pn[:j] = np.where(dead[None], 0.0, T[:j])
        pn[j] = hjj
        rhon[:] = rho
        gj = self.g[g, :, j].copy()
        gn[:] = gj
        sub = np.where(dead | (np.abs(gj) <= thr), 0.0, rho)
        col = np.concatenate([pn[:j + 1], np.zeros((1, m))])
        cur = self._rotate(col, self.cs[g], self.sn[g], j)
        d = np.hypot(cur, sub)
        self.resid[j & 1, g] = np.where(d > TINY, np.abs(sub / np.where(d > TINY, d, 1.0) * gj), 0.0)
        return invr, hjj, np.where(rho > 0, 1.0 / np.where(rho > 0, rho, 1.0), 0.0)

    def _ls_sums(self, g, j, w):
        rs = self.restart
        sums, _ = ls_layout(self.ls[g], rs)
        V, u = self.V[:j, g], self.V[j, g]
        sums[:j + 2] = 0.0
        sums[:j, 0] = np.einsum("knm,nm->km", V, u)
        sums[j, 0] = np.einsum("nm,nm->m", u, u)
        if w is not None:
            sums[:j, 1] = np.einsum("knm,nm->km", V, w)
            sums[j, 1] = np.einsum("nm,nm->m", u, w)
            sums[j + 1, 0] = np.einsum("nm,nm->m", w, w)
        return sums[:, 0], sums[:, 1]

    def _lowsync(self, g, j, w):
        S, T = self._ls_sums(g, j, w)
        invr, hjj, sig = self._ls_column(g, j, S, T, True)
        V, u = self.V[:j, g], self.V[j, g]
        v = to_fp16((u - np.einsum("knm,km->nm", V, S[:j])) * invr)
        self.V[j, g] = v
        self.V[j + 1, g] = to_fp16((w - np.einsum("knm,km->nm", V, T[:j]) - v * hjj) * sig)

    def close(self, ks, Z, X):
        X = f64(X).copy()
        for g in range(self.ng):
            k = int(ks[g])
            if k <= 0:
                continue
            if self.form["lowsync"]:
                S, T = self._ls_sums(g, k, None)
                self._ls_column(g, k, S, T, False)
            kk = k + 1 if self.mut == "backsolve_extra_column" else k
            for c in range(self.m):
                R = np.triu(self.H[g, c, :kk, :kk].T)
                yy = np.zeros(kk)
                for i in range(kk - 1, -1, -1):
                    yy[i] = (self.g[g, c, i] - R[i, i + 1:] @ yy[i + 1:]) / R[i, i]
                self.y[g, :k, c] = yy[:k]
            X[g] += np.einsum("knm,km->nm", f64(Z[:k, g]), self.y[g, :k])
        return X

    def read(self, what, slot=0):
        if what == "basis":
            return self.V[slot].copy()
        if what == "resid0" or what == "resid1":
            return self.resid[int(what[-1])].copy()
        if what == "ls_coef":
            return self.ls.copy()
        return getattr(self, what).copy()


# ------------------------------------------------------------------------------------------------ cases and driver
def case_inputs(n, m, ng, restart, seed=0, zero_rhs=None, zero_w=None, converged=None):
    """Seeded inputs of a case: residual panels R [ng, n, m] (column ``zero_rhs`` zero), ||b|| = the column norms of
    R, the noise panels of the steps, the Z slots (FP32) and the iterate x0.  ``zero_w = (step, column)``: that column
    of W is exactly zero at that step;  ``converged``: a column with W_0 = v_0 + 1e-6 (unit-norm noise)."""
    rng = np.random.default_rng([seed, n, m, ng])
    R = rng.standard_normal((ng, n, m))
    if zero_rhs is not None:
        R[:, :, zero_rhs] = 0.0
    noise = rng.standard_normal((restart, ng, n, m)) / np.sqrt(n)
    Z = rng.standard_normal((restart, ng, n, m)).astype(np.float32)
    x0 = rng.standard_normal((ng, n, m))
    for a in (R, noise, Z, x0):
        a.setflags(write=False)
    return dict(R=R, bnorm=np.sqrt(np.einsum("gnm,gnm->gm", R, R)), noise=noise, Z=Z, x0=x0, zero_w=zero_w,
                converged=converged)


def step_panel(inp, j, vj):
    """W_j = noise_j + 3 v_j (vj: slot j of the device, [ng, n, m]) with the case's special columns."""
    W = inp["noise"][j] + 3.0 * vj
    if inp["converged"] is not None and j == 0:
        c = inp["converged"]
        nz = inp["noise"][0][:, :, c]
        W[:, :, c] = vj[:, :, c] + 1e-6 * nz / np.linalg.norm(nz, axis=1, keepdims=True)
    if inp["zero_w"] is not None and j == inp["zero_w"][0]:
        W[:, :, inp["zero_w"][1]] = 0.0
    return W


class Report(dict):
    """quantity -> largest error / bound seen;  ``stats``: StoreStats of the stored vectors."""

    def __init__(self):
        super().__init__()
        self.stats = StoreStats()
        self.inert = 0

    def put(self, name, r):
        self[name] = max(self.get(name, 0.0), float(r))

    def cmp(self, name, got, exp):
        self.put(name, ratio(got, exp[0], exp[1]))

    def worst(self):
        return max(self.values()) if self else 0.0

    def ok(self):
        return self.worst() <= 1.0 and self.stats.ok()


def _snapshot(dev, g, restart, form):
    names = ["h1", "h2", "H", "cs", "sn", "g", "scale", "resid0", "resid1", "w"]
    names += ["ls_coef", "w32"] if form["lowsync"] else (["w32"] if form["w32"] else [])
    snap = {k: dev.read(k)[g].copy() for k in names}
    for s in range(restart + 1):
        snap["basis%d" % s] = dev.read("basis", s)[g].copy()
    return snap


def check_case(dev, inp, restart, tol, form, ks, leave=None, steps=None):
    """One restart cycle on ``dev`` (begin, steps 0 .. steps-1, close with ``ks``), every quantity against the model.
    ``leave = {group: step}``: the group is not in the table after that step and its whole state must stay bitwise
    what it was then, up to the cycle end.  Returns a Report."""
    R, bnorm = inp["R"], inp["bnorm"]
    ng, n, m = R.shape
    steps = restart if steps is None else steps
    rep = Report()
    st = store_fn(form)
    dev.begin(R, bnorm)
    # ---- cycle start
    nrm2 = dev.read("nrm2")
    g = dev.read("g")
    v0 = dev.read("basis", 0)
    for q in range(ng):
        rep.cmp("start nrm2", nrm2[q], start_expect(R[q])["nrm2"])
        se = start_from_nrm2(nrm2[q])
        rep.cmp("start g0", g[q][:, 0], se["beta"])
        rep.cmp("start estimate", dev.read("resid0")[q], se["beta"])
        rep.put("start g rest", 0.0 if not g[q][:, 1:].any() else np.inf)
        rep.cmp("start scale", dev.read("scale")[q], se["scale"])
        sc = dev.read("scale")[q]
        rep.put("v0", check_stored(v0[q], ld(R[q]) * ld(sc), UT * fa(R[q] * sc), form, rep.stats))
        if form["b16"] or form["b32"]:
            rep.put("v0 FP64 copy", 0.0 if np.array_equal(dev.read("vcur")[q], v0[q]) else np.inf)
    V = [v0]
    live = list(range(ng))
    leave = dict(leave or {})
    snap = {}
    for j in range(steps):
        pre = dict(cs=dev.read("cs"), sn=dev.read("sn"), g=dev.read("g"), est=dev.read("resid%d" % (j & 1)))
        if form["lowsync"]:
            pre["ls"] = dev.read("ls_coef")
        W = step_panel(inp, j, V[j])
        dev.step(j, W, live)
        post = {k: dev.read(k) for k in ("h1", "h2", "H", "cs", "sn", "g", "scale")}
        vnew = dev.read("basis", j + 1)
        if form["lowsync"]:
            post["ls"], post["vj"] = dev.read("ls_coef"), dev.read("basis", j)
            wst = dev.read("w32")
        elif form["w32"]:
            wst = dev.read("w32")
        else:
            wst = dev.read("w")
        for q in live:
            if form["w32"]:
                rep.put("w as FP32", 0.0 if np.array_equal(wst[q], to_fp32(W[q])) else np.inf)
            w = to_fp32(W[q]) if form["w32"] else W[q]
            pq = dict(cs=pre["cs"][q], sn=pre["sn"][q], g=pre["g"][q], est=pre["est"][q], bnorm=bnorm[q])
            if form["lowsync"]:
                _check_lowsync(rep, dev, q, j, V, w, pq, pre, post, vnew, form, tol, restart)
            else:
                _check_cgs2(rep, dev, q, j, V, w, wst, pq, post, vnew, form, tol)
        if form["lowsync"]:
            V[j] = post["vj"]                        # slot j now holds v_j
        V.append(vnew)
        for q in [q for q in live if leave.get(q) == j]:
            live.remove(q)
            snap[q] = _snapshot(dev, q, restart, form)
        if not live:
            break
    for q in snap:
        now = _snapshot(dev, q, restart, form)
        same = all(np.array_equal(snap[q][k], now[k], equal_nan=True) for k in now)
        rep.put("state of a group that left", 0.0 if same else np.inf)
    # ---- cycle end
    Hb, gb = dev.read("H"), dev.read("g")
    pre = dict(cs=dev.read("cs"), sn=dev.read("sn"), g=gb)
    if form["lowsync"]:
        pre["ls"] = dev.read("ls_coef")
    nz = max(max(ks), 1)
    X = dev.close(ks, inp["Z"][:nz], inp["x0"])
    Ha, ga, y = dev.read("H"), dev.read("g"), dev.read("y")
    for q in range(ng):
        k = int(ks[q])
        if form["lowsync"] and k > 0:
            sums, pend = ls_layout(pre["ls"][q], restart)
            Vq = np.stack([V[i][q] for i in range(k)])
            es, _ = lowsync_sums(Vq, V[k][q], None)
            sdev, _ = ls_layout(dev.read("ls_coef")[q], restart)
            rep.cmp("close S", sdev[:k + 1, 0], (es[0][:k + 1], es[1][:k + 1]))
            pq = dict(cs=pre["cs"][q], sn=pre["sn"][q], g=pre["g"][q], bnorm=bnorm[q])
            ce, _ = lowsync_complete(sdev[:, 0], k, pend[(k - 1) & 1], pq, tol, restart)
            _check_completed(rep, "close ", ce, k, Ha[q], dev.read("cs")[q], dev.read("sn")[q], ga[q])
        elif not form["lowsync"]:
            rep.put("close leaves H, g", 0.0 if np.array_equal(Hb[q], Ha[q], equal_nan=True) and
                    np.array_equal(gb[q], ga[q]) else np.inf)
        if k > 0:
            rep.put("back substitution", backsolve_residual(Ha[q], ga[q], y[q], k))
        rep.cmp("correction", X[q], correction_expect(inp["x0"][q], inp["Z"][:, q], y[q], k))
    return rep


def _check_completed(rep, tag, ce, j, H, cs, sn, g):
    """column j-1 as completed: H [m, restart, restart+1], cs, sn [m, restart], g [m, restart+1] of one group."""
    rep.cmp(tag + "H column", H[:, j - 1, :j + 1].T, ce["Hcol"])
    rep.cmp(tag + "cs", cs[:, j - 1], ce["cs"])
    rep.cmp(tag + "sn", sn[:, j - 1], ce["sn"])
    rep.cmp(tag + "g_j", g[:, j - 1], ce["g0"])
    rep.cmp(tag + "g_j+1", g[:, j], ce["g1"])


def _check_cgs2(rep, dev, q, j, V, w, wst, pq, post, vnew, form, tol):
    nv = j + 1
    Vq = np.stack([V[i][q] for i in range(nv)])
    pp = dict(h1=post["h1"][q], h2=post["h2"][q], scale=post["scale"][q])
    if not form["keepw"]:
        pp["wp"] = wst[q]
    e = cgs2_expect(Vq, w, j, pq, pp, form, tol)
    rep.cmp("h1", pp["h1"][:nv], e["h1"])
    rep.cmp("h2, ||w'||^2", pp["h2"][:nv + 1], e["h2"])
    if "wp" in e:
        rep.cmp("w'", pp["wp"], e["wp"])
    elif not form["w32"]:
        rep.put("w kept", 0.0 if np.array_equal(wst[q], w) else np.inf)
    if form["keepw"] and not form["fuseh"]:
        rep.cmp("h1 + h2", dev.read("hsum")[q][:nv], e["hsum"])
    rep.cmp("H column", post["H"][q][:, j, :j + 2].T, e["Hcol"])
    rep.cmp("cs", post["cs"][q][:, j], e["cs"])
    rep.cmp("sn", post["sn"][q][:, j], e["sn"])
    rep.cmp("g_j", post["g"][q][:, j], e["g0"])
    rep.cmp("g_j+1", post["g"][q][:, j + 1], e["g1"])
    est = dev.read("resid%d" % ((j + 1) & 1 if form["fuseh"] else 0))[q]
    rep.cmp("estimate", est, e["est"])
    rep.put("estimate = |g_j+1|", 0.0 if np.array_equal(est, np.abs(post["g"][q][:, j + 1])) else np.inf)
    if not form["fuseh"]:
        rep.cmp("scale", pp["scale"], e["scale"])
    rep.put("v_j+1", check_stored(vnew[q], e["vnext"][0], e["vnext"][1], form, rep.stats))
    if (form["b16"] or form["b32"]) and not form["h16"]:
        rep.put("v_j+1 FP64 copy", 0.0 if np.array_equal(dev.read("vcur")[q], vnew[q]) else np.inf)
    fz = e["frozen"]
    if fz.any():
        # inert values, exactly: no sub-diagonal, a non-singular diagonal, g_j+1 = 0, no new vector
        rep.inert += int(fz.sum())
        Hq = post["H"][q][fz, j, :]
        inert = (not Hq[:, j + 1].any() and np.all(np.isfinite(Hq[:, j]) & (Hq[:, j] != 0)) and
                 not post["g"][q][fz, j + 1].any() and not est[fz].any() and not vnew[q][:, fz].any() and
                 (form["fuseh"] or not pp["scale"][fz].any()))
        rep.put("frozen column inert", 0.0 if inert else np.inf)


def _check_lowsync(rep, dev, q, j, V, w, pq, pre, post, vnew, form, tol, restart):
    Vq = np.stack([V[i][q] for i in range(j)]) if j else np.zeros((0,) + w.shape)
    _, pend0 = ls_layout(pre["ls"][q], restart)
    sums, pend1 = ls_layout(post["ls"][q], restart)
    pq = dict(pq, pend=pend0)
    pp = dict(S=sums[:, 0], T=sums[:, 1], cs=post["cs"][q], sn=post["sn"][q], g=post["g"][q], pend=pend1,
              vj=post["vj"][q])
    e = lowsync_expect(Vq, V[j][q], w, j, pq, pp, tol, restart)
    rep.cmp("sums s, alpha, ||w||^2", pp["S"][:j + 2], e["S"])
    rep.cmp("sums t, beta", pp["T"][:j + 2], e["T"])
    if j > 0:
        _check_completed(rep, "completed ", e["complete"], j, post["H"][q], pp["cs"], pp["sn"], pp["g"])
    pdev, rhodev, gjdev = pend1[j & 1]
    rep.cmp("pending column (t, h_jj)", pdev[:j + 1], e["p"])
    rep.cmp("rho_j", rhodev, e["rho"])
    rep.cmp("pending g", gjdev, e["pend_g"])
    rep.cmp("provisional estimate", dev.read("resid%d" % (j & 1))[q], e["est"])
    rep.put("v_j", check_stored(pp["vj"], e["vj"][0], e["vj"][1], form, rep.stats))
    rep.put("u_j+1", check_stored(vnew[q], e["unext"][0], e["unext"][1], form, rep.stats))
    dead = e["dead"]
    if dead.any():
        rep.inert += int(dead.sum())
        inert = (not pp["vj"][:, dead].any() and not vnew[q][:, dead].any() and not pdev[:j + 1, dead].any() and
                 not rhodev[dead].any() and not post["H"][q][dead, j - 1, j].any() and not pp["g"][dead, j].any())
        rep.put("frozen column inert", 0.0 if inert else np.inf)


# ------------------------------------------------------------------------------------------------ the cases
RESTART, TOL = 10, 1e-3
N_ROWS = {"th3": 65, "th4": 122, "th11": 1025, "cfg1": 1937}      # n % 64 = 1, 58, 1, 17
WIDTHS = (5, 8, 16, 24, 32)
# (switch, width): RICADI_ARNOLDI=cgs2, RICADI_W32=0 and RICADI_FUSEH=0 act at 16 columns only
COMBOS = ([("default", m) for m in WIDTHS] + [("cgs2", 16), ("w32off", 16), ("fuseh0", 16)] +
          [("basis32", m) for m in WIDTHS] + [("basis64", m) for m in WIDTHS])
LEAVE_A, KS_A = {1: 3}, (10, 4, 10)
LEAVE_B, KS_B = {0: 6, 1: 3, 2: 1}, (7, 4, 2)
FROZEN = dict(zero_rhs=2, zero_w=(5, 3), converged=4)     # three columns of one panel


def _case(op, switch, m, ng=1, restart=RESTART, leave=None, ks=None, frozen=False):
    ks = tuple(ks) if ks else (RESTART,) * ng
    name = "%s-%s-m%d-g%d%s%s%s" % (op, switch, m, ng, "-r%d" % restart if restart != RESTART else "",
                                     "-k" + "".join(map(str, ks)) if leave else "", "-frozen" if frozen else "")
    return dict(name=name, op=op, switch=switch, m=m, ng=ng, restart=restart, leave=leave, ks=ks, frozen=frozen)


CASES = ([_case("th3", s, m) for s, m in COMBOS] +
         [_case("th4", s, m, ng=3, leave=LEAVE_A, ks=KS_A) for s, m in COMBOS] +
         [_case("th4", s, m, frozen=True) for s, m in (("default", 16), ("cgs2", 16), ("fuseh0", 16), ("default", 8), ("basis64", 5))] +
         [_case("th11", s, m) for s, m in (("default", 16), ("cgs2", 16), ("w32off", 16), ("basis32", 16),
                                            ("basis64", 16), ("default", 5), ("default", 24))] +
         [_case("cfg1", "default", 16, ng=3, leave=LEAVE_A, ks=KS_A),
          _case("cfg1", "default", 16, ng=3, leave=LEAVE_B, ks=KS_B),
          _case("cfg1", "cgs2", 16, ng=3, leave=LEAVE_B, ks=KS_B),
          _case("cfg1", "fuseh0", 16, ng=3, leave=LEAVE_A, ks=KS_A),
          _case("cfg1", "w32off", 16), _case("cfg1", "basis32", 8), _case("cfg1", "basis64", 32),
          _case("cfg1", "default", 5), _case("cfg1", "default", 16, restart=30)])


def nominal_form(switch, m):
    """The IterationForm the library takes for a switch and width where the operator admits the hot form (the GPU
    test takes the bits the probe reports instead)."""
    f = dict.fromkeys(FORM_BITS, False)
    f["b16"] = switch not in ("basis32", "basis64")
    f["b32"] = switch == "basis32"
    hot = f["b16"] and m == 16
    f["keepw"] = f["h16"] = f["x32"] = hot
    f["fuseh"] = hot and switch != "fuseh0"
    f["w32"] = f["fuseh"] and switch != "w32off"
    f["lowsync"] = f["w32"] and switch != "cgs2"
    return f


def run_case(dev, case, n, form, seed=0):
    fz = FROZEN if case["frozen"] else {}
    inp = case_inputs(n, case["m"], case["ng"], case["restart"], seed=seed, **fz)
    return check_case(dev, inp, case["restart"], TOL, form, case["ks"], leave=case["leave"], steps=RESTART)
