"""LQG-balanced truncation (and plain balanced truncation) from two low-rank factors, on the device.

The system is ``M v' = A v + J^T p + B u``, ``J v = 0``, ``y = C v``.  With the regulator factor ``Zc``
(``X = Zc Zc^T`` solves ``A^T X M + M^T X A - M^T X B B^T X M + C^T C = 0`` on ker J: the Riccati functions of
:mod:`optconpy_amd.proj_ric_utils` with ``transposed=False``, ``bmat=B``, ``wmat=C^T``) and the filter factor ``Zf``
(``Y = Zf Zf^T`` solves ``A Y M^T + M Y A^T - M Y C^T C Y M^T + B B^T = 0``: ``transposed=True``, ``bmat=C^T``,
``wmat=B``) the square-root method forms

    S = Zc^T M Zf = U Sigma V^T,   T_l = Zc U_r Sigma_r^-1/2,   T_r = Zf V_r Sigma_r^-1/2,   T_l^T M T_r = I_r,
    A_r = T_l^T A T_r,   E_r = T_l^T M T_r,   B_r = T_l^T B,   C_r = C T_r,

keeping the ``r`` values ``sigma_i > tol sigma_1`` (at most ``order``).  The ``sigma_i`` are the LQG characteristic
values; ``Sigma_r`` solves both reduced Riccati equations (``X M T_r = T_l Sigma_r``, ``Y M^T T_l = T_r Sigma_r``),
which gives the controller ``A_K = A_r - B_r B_r^T Sigma_r - Sigma_r C_r^T C_r``, ``B_K = Sigma_r C_r^T``,
``C_K = -B_r^T Sigma_r``.  With the factors of the two Lyapunov equations the same step is balanced truncation and the
``sigma_i`` are the Hankel singular values.

Everything of size NV runs in ``libricadi_hip.so`` (``ricadi_lqg_balance_dev``): the ``M``
product, the cross-Gram matrices on the FP64 matrix cores, the two-sided projected pencil, ``Z (U_r Sigma_r^-1/2)``;
the SVD of the small ``S`` is the library's host Jacobi SVD.  Extension of the mirror: the reference has no counterpart.
"""
from __future__ import annotations

import numpy as np

from . import _lib, backend
from . import proj_ric_utils as pru

__all__ = ["balance_factors", "lqgbt_reduce", "freq_response", "reduced_freq_response", "reduction_error",
           "MAX_COLS", "MAX_ORDER"]

MAX_COLS = 1024          # widest factor ricadi_lqg_balance_dev takes
MAX_ORDER = _lib.MAX_M   # largest reduced order


def _narrow(ctx, z, tol):
    """A factor of more than ``MAX_COLS`` columns compressed (``Context.compress``: ``Zn Zn^T ~ Z Z^T``) to the singular
    values above ``0.1 tol ||Z||_2`` and at most ``MAX_COLS``; others as they are."""
    if z.shape[1] <= MAX_COLS:
        return z
    zh = np.ascontiguousarray(pru._dense(pru._host(z)))
    zn, sv = ctx.compress(zh, thresh=None, k=None)       # all singular values first: the threshold is relative
    keep = int(min(MAX_COLS, max(1, np.count_nonzero(sv > 0.1 * tol * sv[0]))))
    return np.ascontiguousarray(zn[:, :keep])


def balance_factors(mmat=None, amat=None, jmat=None, zc=None, zf=None, bmat=None, cmat=None, tol=1e-10, order=None):
    """Square-root balancing of the factors ``zc`` (``X = Zc Zc^T``) and ``zf`` (``Y = Zf Zf^T``) for the system
    ``(M, A, J, B, C)`` -- ``cmat`` is ``C`` (NY x NV) --, on the device.

    ``zc`` / ``zf``: ndarrays or :class:`~optconpy_amd.proj_ric_utils.DeviceFactor` (then nothing of size NV crosses
    PCIe except ``B`` and ``C^T``).  ``tol``: singular values ``sigma_i > tol sigma_1`` are kept; ``order``: at most
    that many (``None``: ``MAX_ORDER`` = 128, the largest order the library reduces to).

    A factor wider than ``MAX_COLS`` = 1024 columns is first compressed with the library's compression
    (``compress_Zsvd``'s) to its singular values above ``0.1 tol ||Z||_2`` -- on the host side of the library, so such
    a factor is downloaded once.

    Returns a dict: ``hsv`` (ALL singular values of ``Zc^T M Zf``, descending), ``order`` (r), ``tl`` / ``tr`` (NV x r;
    ``DeviceFactor`` if a factor came as one, else ndarrays), ``ar`` / ``er`` (r x r), ``br`` (r x NU), ``cr``
    (NY x r).  The same inputs give bitwise the same outputs.

    Side effects on the process-wide context, as with every function of :mod:`proj_ric_utils`: ``(A, M, J)`` becomes the
    resident operator, and a low-rank term set on the context (``Context.set_lowrank``) is CLEARED and stays cleared --
    the reduced model is that of ``A`` itself.  The RADI settings are not touched."""
    import torch
    calA, calE = pru._orient(amat, mmat, True)                       # cal A = A, cal E = M: the filter call's
    ctx = backend.context_for(calA, calE, jmat)
    ctx.set_lowrank(None, None)
    on_dev = pru._on_device(zc) or pru._on_device(zf)
    order = MAX_ORDER if order is None else int(order)
    if not 1 <= order <= MAX_ORDER:
        raise ValueError("order must be in [1, {0}]".format(MAX_ORDER))
    zc, zf = _narrow(ctx, zc, tol), _narrow(ctx, zf, tol)
    B = pru._dense(bmat)
    Ct = np.ascontiguousarray(pru._dense(cmat).T)
    if B.shape[0] != ctx.nv or Ct.shape[0] != ctx.nv:
        raise ValueError("bmat must be NV x NU and cmat NY x NV")
    r, sig, tl, tr, ar, er, br, cr = ctx.lqg_balance_dev(pru.to_device(zc).t, pru.to_device(zf).t, pru.to_device(B).t,
                                                         pru.to_device(Ct).t, tol, order)
    if on_dev:
        tl, tr = pru.DeviceFactor(tl.contiguous()), pru.DeviceFactor(tr.contiguous())
    else:
        torch.cuda.synchronize()
        tl, tr = tl.cpu().numpy(), tr.cpu().numpy()
    return dict(hsv=sig, order=r, tl=tl, tr=tr, ar=ar, er=er, br=br, cr=cr)


def _context_settings(ctx):
    """The RADI settings of a context, as the setters report them."""
    w = ctx.set_radi_sweep_width(1)
    ctx.set_radi_sweep_width(w)
    m = ctx.set_radi_shifts("cycle")
    ctx.set_radi_shifts(m)
    s = ctx.set_radi_sweep_shifts(False)
    ctx.set_radi_sweep_shifts(s)
    return dict(sweep_width=w, shifts=m, sweep_shifts=s)


def _restore(ctx, st):
    ctx.set_radi_sweep_shifts(st["sweep_shifts"])
    ctx.set_radi_shifts(st["shifts"])
    ctx.set_radi_sweep_width(st["sweep_width"])


def lqgbt_reduce(mmat=None, amat=None, jmat=None, bmat=None, cmat=None, radi_dict=None, ric_solver="radi",
                 gramians="riccati", tol=1e-10, order=None, return_factors=False):
    """LQG-balanced truncation of ``M v' = A v + J^T p + B u``, ``J v = 0``, ``y = C v``: the two Riccati solves with
    :func:`~optconpy_amd.proj_ric_utils.proj_alg_ric_radi` (``ric_solver='radi'``) or ``proj_alg_ric_newtonadi``
    (``'newtonadi'``), then :func:`balance_factors`.  ``bmat`` (NV x NU) and ``cmat`` = ``C`` (NY x NV) are expected
    Leray-projected (``P^T B``, ``(P^T C^T)^T``, ``lau.app_prj_via_sadpnt(..., transposedprj=True)``), as the callers
    of the Riccati functions prepare them.  ``radi_dict`` is the options dict of the chosen solver (``radi_dict`` /
    ``nwtn_adi_dict`` / ``adi_dict``); the factors stay on the device.

    ``gramians='lyapunov'``: the two Lyapunov equations ``A^T Q M + M^T Q A + C^T C = 0`` and
    ``A P M^T + M P A^T + B B^T = 0`` with ``solve_proj_lyap_stein`` instead -- plain balanced truncation (a stable
    ``A`` is needed), ``hsv`` the Hankel singular values, no controller.

    Returns :func:`balance_factors`' dict (``tl`` / ``tr`` as ndarrays) plus ``ak`` (r x r), ``bk`` (r x NY), ``ck``
    (NU x r) -- the LQG controller ``x_K' = A_K x_K + B_K y``, ``u = C_K x_K`` in the balanced coordinates
    (``E_r = I``) -- and ``info_c`` / ``info_f``, the two solves' own dicts without their factors (``return_factors``:
    also ``zc`` / ``zf``, the two factors as ``DeviceFactor``).  The RADI settings of the context are after the call
    what they were before it, also when it fails."""
    if ric_solver not in ("radi", "newtonadi"):
        raise ValueError("ric_solver must be 'radi' or 'newtonadi'")
    if gramians not in ("riccati", "lyapunov"):
        raise ValueError("gramians must be 'riccati' or 'lyapunov'")
    d = dict({} if radi_dict is None else radi_dict, device_resident=True)
    B = pru._dense(bmat)
    Ct = np.ascontiguousarray(pru._dense(cmat).T)
    ctx = backend.context()
    before = _context_settings(ctx)
    try:
        if gramians == "lyapunov":
            rc = pru.solve_proj_lyap_stein(amat=amat, mmat=mmat, jmat=jmat, wmat=Ct, transposed=False, adi_dict=d)
            rf = pru.solve_proj_lyap_stein(amat=amat, mmat=mmat, jmat=jmat, wmat=B, transposed=True, adi_dict=d)
        elif ric_solver == "radi":
            rc = pru.proj_alg_ric_radi(mmat=mmat, amat=amat, jmat=jmat, bmat=B, wmat=Ct, transposed=False, radi_dict=d)
            rf = pru.proj_alg_ric_radi(mmat=mmat, amat=amat, jmat=jmat, bmat=Ct, wmat=B, transposed=True, radi_dict=d)
        else:
            rc = pru.proj_alg_ric_newtonadi(mmat=mmat, amat=amat, jmat=jmat, bmat=B, wmat=Ct, transposed=False,
                                            nwtn_adi_dict=d)
            rf = pru.proj_alg_ric_newtonadi(mmat=mmat, amat=amat, jmat=jmat, bmat=Ct, wmat=B, transposed=True,
                                            nwtn_adi_dict=d)
        out = balance_factors(mmat=mmat, amat=amat, jmat=jmat, zc=rc["zfac"], zf=rf["zfac"], bmat=B, cmat=Ct.T,
                              tol=tol, order=order)
    finally:
        _restore(ctx, before)
    out["tl"], out["tr"] = out["tl"].numpy(), out["tr"].numpy()
    out["info_c"] = {k: v for k, v in rc.items() if k != "zfac"}
    out["info_f"] = {k: v for k, v in rf.items() if k != "zfac"}
    if return_factors:
        out["zc"], out["zf"] = rc["zfac"], rf["zfac"]
    if gramians == "riccati":
        sg = out["hsv"][:out["order"]]
        br, cr = out["br"], out["cr"]
        out["ak"] = out["ar"] - br @ (br.T * sg) - (sg[:, None] * cr.T) @ cr
        out["bk"] = sg[:, None] * cr.T
        out["ck"] = -(br.T * sg)
    return out


# ---- frequency response ----------------------------------------------------------------------
FREQ_BATCH = 16          # frequencies per lockstep batch (the library's group limit)
FREQ_COLS = _lib.MAX_MC  # columns of B per solve (the widest complex panel)


def _omegas(omegas):
    om = np.atleast_1d(np.asarray(omegas, dtype=np.float64)).ravel()
    if om.size == 0 or not np.all(np.isfinite(om)) or not np.all(om > 0.0):
        raise ValueError("omegas must be positive and finite")
    return om


def freq_response(mmat=None, amat=None, jmat=None, bmat=None, cmat=None, omegas=None, info=False):
    """The transfer function ``G(i w) = C (i w M - A)^-1 B`` on ker J of ``M v' = A v + J^T p + B u``, ``J v = 0``,
    ``y = C v`` at the frequencies ``omegas`` (positive, finite; else ``ValueError``), on the device.

    ``G[k] = C V_k`` with ``[[A - i w_k M, J^T], [J, 0]] [V_k; L] = [-B; 0]``: saddle solves at the complex shifts
    ``-i w_k`` on the operator ``(cal A, cal E) = (A, M)`` -- the orientation :func:`balance_factors` uses --, sixteen
    frequencies per lockstep batch, the columns of ``B`` in chunks of eight.  ``bmat`` (NV x NU) and ``cmat`` = ``C``
    (NY x NV) are expected Leray-projected, as for :func:`lqgbt_reduce`.  Only ``B``, ``C^T`` and ``G`` cross PCIe.

    Returns ``G`` (``len(omegas)`` x NY x NU, complex128); with ``info=True`` a pair ``(G, d)``, ``d['iters']`` the
    GMRES iterations per frequency (summed over the column chunks) and ``d['relres']`` the worst true relative residual
    per frequency.  A low-rank term set on the context is cleared, as by :func:`balance_factors`."""
    import torch
    om = _omegas(omegas)
    calA, calE = pru._orient(amat, mmat, True)
    ctx = backend.context_for(calA, calE, jmat)
    ctx.set_lowrank(None, None)
    B = pru._dense(bmat)
    Cm = pru._dense(cmat)
    if B.shape[0] != ctx.nv or Cm.shape[1] != ctx.nv:
        raise ValueError("bmat must be NV x NU and cmat NY x NV")
    nu, ny, nv = B.shape[1], Cm.shape[0], ctx.nv
    Bd = pru.to_device(-B).t.to(torch.complex128)
    Cd = pru.to_device(np.ascontiguousarray(Cm.T)).t.to(torch.complex128).T      # C as a view of the uploaded C^T
    G = torch.empty((om.size, ny, nu), dtype=torch.complex128, device=Bd.device)
    iters = np.zeros(om.size, dtype=np.int64)
    relres = np.zeros(om.size)
    for k0 in range(0, om.size, FREQ_BATCH):
        w = om[k0:k0 + FREQ_BATCH]
        for c0 in range(0, nu, FREQ_COLS):
            R = Bd[:, c0:c0 + FREQ_COLS].contiguous()
            X, its, rr = ctx.shift_solve_cplx_batch_dev(-1j * w, R)
            G[k0:k0 + w.size, :, c0:c0 + R.shape[1]] = torch.matmul(Cd, X[:, :nv, :])
            iters[k0:k0 + w.size] += np.asarray(its)
            relres[k0:k0 + w.size] = np.maximum(relres[k0:k0 + w.size], rr.max(axis=1))
    torch.cuda.synchronize()
    Gh = G.cpu().numpy()
    return (Gh, dict(iters=iters, relres=relres)) if info else Gh


def reduced_freq_response(red, omegas):
    """``G_r(i w) = C_r (i w E_r - A_r)^-1 B_r`` of a reduced model (the dict of :func:`balance_factors` /
    :func:`lqgbt_reduce`) at the frequencies ``omegas``; NumPy, ``len(omegas)`` x NY x NU complex128."""
    om = _omegas(omegas)
    ar, er, br, cr = (np.asarray(red[k], dtype=np.float64) for k in ("ar", "er", "br", "cr"))
    return np.stack([cr @ np.linalg.solve(1j * w * er - ar, br.astype(np.complex128)) for w in om])


def reduction_error(mmat=None, amat=None, jmat=None, bmat=None, cmat=None, red=None, omegas=None):
    """How far the reduced model ``red`` is from the full one on the imaginary axis: a dict with ``omegas``, ``err``
    (``sigma_max(G(i w) - G_r(i w))`` per frequency), ``full`` (``sigma_max(G(i w))``) and ``hinf_lower`` (``max err``:
    a lower bound of the H-infinity error, to be held against ``2 sum_{i > r} hsv_i`` for balanced truncation).  The full
    response comes from :func:`freq_response`, the reduced one from :func:`reduced_freq_response`."""
    om = _omegas(omegas)
    G = freq_response(mmat=mmat, amat=amat, jmat=jmat, bmat=bmat, cmat=cmat, omegas=om)
    Gr = reduced_freq_response(red, om)
    err = np.array([np.linalg.norm(G[k] - Gr[k], 2) for k in range(om.size)])
    full = np.array([np.linalg.norm(G[k], 2) for k in range(om.size)])
    return dict(omegas=om, err=err, full=full, hinf_lower=float(err.max()))
