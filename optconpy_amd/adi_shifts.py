"""Problem-adapted ADI shifts: ``ms='auto'`` of the drop-in (``proj_ric_utils``).

Recipe (Penzl's heuristic on a Krylov-like subspace of the ADI itself):

1. **Basis.**  ``W0 = P^T W`` (the projection the ADI applies to its right-hand side) and ``warm_steps`` ADI steps
   at ``p0 = -sqrt(min * max |diag cal A / diag cal E|)``; thin QR of ``[W0, Z_warm]`` on the device, truncated by
   an SVD of ``R`` to at most 128 directions (down to 1e-10 relative).
2. **Projection.**  ``H_A = Q^T cal A Q``, ``H_E = Q^T cal E Q`` on the device (``Context.project_pencil``, with the
   low-rank term of the context if one is set); the candidates are ``-|lambda|`` for the finite Ritz values
   ``lambda`` of ``(H_A, H_E)``.
3. **Selection.**  :func:`penzl_select`: Penzl's greedy min-max choice among the candidates.
4. **Admissibility.**  :func:`admissible_order`: every window of consecutive shifts the sweep driver can take must
   have a well-conditioned Cauchy matrix (``ricadi_host_cauchy``); the list is put in the order of
   ``problems.logshifts(interleave=True)`` and thinned until that holds.

Everything after the projection is host arithmetic on at most 128 numbers.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla

from . import _lib

__all__ = ["auto_shifts", "penzl_select", "admissible_order", "initial_shift", "ShiftList",
           "MAX_BASIS", "BASIS_RTOL", "MERGE_RTOL", "CAUCHY_WIDTH"]

MAX_BASIS = 128       # directions kept of [W0, Z_warm] (the projection kernel's limit)
BASIS_RTOL = 1e-10    # singular values of R below this fraction of the largest are dropped
MERGE_RTOL = 0.01     # candidates closer than 1 % are one candidate
CAUCHY_WIDTH = 16     # widest sweep of the ADI drivers


class ShiftList(list):
    """A shift list with how it came about in ``.info``: ``candidates`` (distinct Ritz candidates),
    ``warm_solves`` (shift-solves spent on the basis), ``fallback`` (True: no candidate, the default list)."""

    info: dict


def initial_shift(diag_ratio):
    """``-sqrt(min * max)`` of ``|diag cal A / diag cal E|`` (-1 where there is nothing to go by)."""
    r = np.asarray(diag_ratio if diag_ratio is not None else [], dtype=float)
    r = r[np.isfinite(r) & (r > 0)]
    if r.size == 0:
        return -1.0
    return -float(np.sqrt(r.min() * r.max()))


def _merge(cands, rtol=MERGE_RTOL):
    """Sorted by magnitude; a candidate within ``rtol`` of the last one kept is dropped."""
    c = np.sort(np.abs(np.asarray(cands, dtype=float)))
    out = []
    for x in c:
        if not out or x - out[-1] > rtol * out[-1]:
            out.append(x)
    return -np.asarray(out)


def _ratio(c, p):
    return np.abs((c - p) / (c + p))


def _merge_complex(cands, rtol=MERGE_RTOL):
    """Candidates with a complex entry: every one in the closed upper half plane (a pair is held by its member with
    ``Im > 0``), sorted by magnitude, then phase; one within ``rtol`` (relative distance) of a kept one is dropped."""
    c = np.asarray(cands, dtype=complex)
    c = np.where(c.imag < 0, c.conj(), c)
    c = c[np.lexsort((np.angle(c), np.abs(c)))]
    out = []
    for x in c:
        if all(abs(x - y) > rtol * abs(y) for y in out):
            out.append(x)
    return np.asarray(out, dtype=complex)


def _pair_ratio(t, p):
    """``|(t - p)/(t + p)|`` for a real ``p``, ``|(t - p)(t - conj p) / ((t + p)(t + conj p))|`` for a pair."""
    r = np.abs((t - p) / (t + p))
    return r if p.imag == 0.0 else r * np.abs((t - p.conjugate()) / (t + p.conjugate()))


def _penzl_select_pairs(cands, num):
    """:func:`penzl_select` for candidates off the real axis: a complex candidate stands for its conjugate pair, the
    min-max and the running products are taken over the conjugate-symmetric set of test points with the pair factor,
    and a pair counts as two of ``num`` (with one left, the best real candidate is taken, if there is one).  Returns
    floats and -- for the pairs -- complex numbers with a positive imaginary part, in the order of the picks."""
    c = _merge_complex(cands)
    if c.size == 0 or num < 1:
        return []
    t = np.concatenate([c, c[c.imag != 0.0].conj()])
    cost = np.where(c.imag != 0.0, 2, 1)
    picks, count = [], 0
    prod = np.ones(t.size)
    taken = np.zeros(c.size, dtype=bool)
    while count < num:
        ok = ~taken & (cost <= num - count)
        if not ok.any():
            break
        if not picks:
            score = np.array([-_pair_ratio(t, p).max() for p in c])     # the first minimises the worst ratio
        else:
            score = prod[:c.size]
            if score[ok].max() == 0.0:
                break
        i = int(np.flatnonzero(ok)[np.argmax(score[ok])])
        taken[i] = True
        picks.append(complex(c[i]) if c[i].imag != 0.0 else float(c[i].real))
        count += int(cost[i])
        prod = prod * _pair_ratio(t, c[i])
    return picks


def penzl_select(cands, num):
    """Penzl's greedy selection of ``num`` shifts among negative real candidates (merged within 1 % first):
    the first minimises ``max_c |(c - p)/(c + p)|``, each further one is the candidate where the running product
    ``prod_i |(c - p_i)/(c + p_i)|`` is largest.  Returns the picks in the order they were made.  Candidates with a
    complex entry (``candidates(..., keep_complex=True)``) are selected as conjugate pairs:
    :func:`_penzl_select_pairs`."""
    if np.iscomplexobj(cands) and np.any(np.asarray(cands).imag != 0.0):
        return _penzl_select_pairs(cands, num)
    cands = np.real(cands)
    c = _merge(cands)
    if c.size == 0 or num < 1:
        return []
    worst = np.array([_ratio(c, p).max() for p in c])
    first = int(np.argmin(worst))
    picks = [float(c[first])]
    prod = _ratio(c, c[first])
    while len(picks) < min(num, c.size):
        i = int(np.argmax(prod))
        if prod[i] == 0.0:
            break
        picks.append(float(c[i]))
        prod = prod * _ratio(c, c[i])
    return picks


def _log_order(ms):
    """The order ``problems.logshifts(interleave=True)`` gives the same values: by magnitude, interleaved in
    groups of ``ceil(len / 16)`` when longer than 16."""
    ms = sorted(ms, key=abs)
    if len(ms) > 16:
        k = -(-len(ms) // 16)
        ms = [ms[i] for r in range(k) for i in range(r, len(ms), k)]
    return ms


def _windows_ok(ms, width=CAUCHY_WIDTH):
    n = len(ms)
    for g in range(2, min(width, n) + 1):
        for s in range(n):
            try:
                _lib.host_cauchy([ms[(s + i) % n] for i in range(g)])
            except (RuntimeError, ValueError):
                return False
    return True


def admissible_order(picks, width=CAUCHY_WIDTH):
    """``picks`` (in order of preference) in logshifts order, thinned until every cyclic window of width
    ``<= width`` passes ``ricadi_host_cauchy``: while one fails, of the two closest shifts (by ratio) the
    later pick goes."""
    keep = list(picks)
    while True:
        ms = _log_order(keep)
        if len(ms) <= 1 or _windows_ok(ms, width):
            return ms
        best, drop = np.inf, None
        for i in range(len(keep)):
            for j in range(i + 1, len(keep)):
                d = abs(np.log(abs(keep[i]) / abs(keep[j])))
                if d < best:
                    best, drop = d, j
        del keep[drop]


def _project_w(ctx, W):
    """``P^T W`` as the ADI drivers form it (one saddle solve with ``cal E``, then ``cal E x``), without the
    context's low-rank term."""
    if ctx.np_ == 0:
        return W.copy()
    lr = ctx._lowrank
    if lr is not None:
        ctx.set_lowrank(None, None)
    try:
        X, _, _ = ctx.shift_solve(1.0, 0.0, W)
        X[ctx.nv:] = 0.0
        return ctx.spmm(1.0, 0.0, X)[:ctx.nv]
    finally:
        if lr is not None:
            ctx.set_lowrank(*lr)


def basis(Qraw, R, max_dim=MAX_BASIS, rtol=BASIS_RTOL):
    """Orthonormal basis of the range of ``Qraw R`` (``Qraw`` orthonormal, ``R`` upper triangular): the left
    singular vectors of ``R`` above ``rtol`` of the largest singular value, at most ``max_dim``."""
    U, s, _ = np.linalg.svd(R)
    if s.size == 0 or s[0] == 0.0:
        return Qraw[:, :0]
    keep = min(int(np.count_nonzero(s > rtol * s[0])), max_dim)
    return Qraw @ U[:, :keep]


COMPLEX_RTOL = 1e-3   # keep_complex: a Ritz value with |Im| above this fraction of its modulus stays complex


def candidates(HA, HE, keep_complex=False):
    """``-|lambda|`` for the finite, nonzero generalised eigenvalues of ``(HA, HE)``.  ``keep_complex``: a stable
    one with ``|Im lambda| > 1e-3 |lambda|`` is kept as ``Re lambda + i |Im lambda|`` (it stands for its conjugate
    pair), the others as ``-|lambda|``; the array is complex then."""
    lam = sla.eigvals(HA, HE)
    lam = lam[np.isfinite(lam)]
    c = -np.abs(lam)
    if keep_complex:
        off = (np.abs(lam.imag) > COMPLEX_RTOL * np.abs(lam)) & (lam.real < 0)
        c = np.where(off, lam.real + 1j * np.abs(lam.imag), c.astype(complex))
        return c[c.real < 0]
    return c[c < 0]


def auto_shifts(ctx, W, num=8, warm_steps=2, default=None, keep_complex=False):
    """Shifts for the ADI on the operator of ``ctx`` (its low-rank term included) with right-hand side
    factor ``W`` (NV x m): a :class:`ShiftList` of distinct negative reals, at most ``num`` of them.
    ``keep_complex``: Ritz values off the real axis are candidates as they are and the list may hold complex entries,
    one per conjugate pair, each counted as two of ``num``; such a list is returned in the order of the picks
    (:func:`admissible_order` serves the Cauchy windows of the sweep form, which takes no pairs)."""
    W = _lib.as_panel(W, ctx.nv)
    p0 = initial_shift(ctx.diag_ratio)
    W0 = _project_w(ctx, W)
    solves = 0
    blocks = [W0]
    if warm_steps > 0:
        prm = _lib.adi_params(dict(adi_max_steps=int(warm_steps), adi_newZ_reltol=0.0, sweep_width=1))
        Zw, info = ctx.lyap_adi([p0], W, prm)
        solves += info["shift_solves"]
        blocks.append(Zw)
    B = np.hstack(blocks)
    if B.shape[1] > ctx.nv:
        # an operator with fewer velocity unknowns than [W0, Z_warm] has columns: ricadi_qr takes c <= NV only, and
        # such a block (NV < c rows, a handful of columns) is factorised on the host
        Qraw, R = np.linalg.qr(B)
    else:
        Qraw, R = ctx.qr(B)
    Q = np.ascontiguousarray(basis(Qraw, R))
    cands = np.zeros(0)
    if Q.shape[1] > 0:
        HA, HE = ctx.project_pencil(Q)
        cands = candidates(HA, HE, keep_complex=keep_complex)
    if cands.size == 0:
        from .proj_ric_utils import DEFAULT_MS
        out = ShiftList(DEFAULT_MS if default is None else default)
        fallback = True
    else:
        picks = penzl_select(cands, num)
        out = ShiftList(picks if any(isinstance(p, complex) for p in picks) else admissible_order(picks))
        fallback = False
    ncand = _merge_complex(cands).size if np.iscomplexobj(cands) else _merge(cands).size
    out.info = dict(candidates=int(ncand), warm_solves=int(solves), fallback=fallback,
                    basis_dim=int(Q.shape[1]), p0=p0)
    return out
