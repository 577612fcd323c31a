"""Host-side mirror of ``sadptprj_riclyap_adi.proj_ric_utils`` on the HIP path.

Same names, keyword arguments and return conventions as the functions optconpy
calls (``/root/reference/optcont_main.py:488-492,498-499,505-506``;
``/root/reference/solve_dae_ric.py:101,152-159,162-163,183,189``;
``/root/reference/tests/test_units_compfacres_compress.py:62-64,82,92,104``).
The arithmetic runs in ``libricadi_hip.so`` on the GPU; this module only
normalises the inputs (csr / csc / scaled / transposed sparse matrices, C-order
float64 panels) and resolves the ``transposed`` flag into the orientation the
C-ABI expects.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sps

from . import _lib, adi_shifts, backend

__all__ = [
    "solve_proj_lyap_stein", "proj_alg_ric_newtonadi", "proj_alg_ric_radi", "compress_Zsvd",
    "get_mTzzTtb", "comp_proj_lyap_res_norm", "DEFAULT_MS", "DeviceFactor", "to_device",
]


class DeviceFactor:
    """A dense ``NV x c`` panel that lives in HBM (a contiguous float64 torch CUDA tensor ``.t``).

    Extension of the mirror, not part of the reference's interface: ``proj_alg_ric_newtonadi`` returns its
    ``'zfac'`` as one when it was GIVEN device panels (``bmat`` / ``wmat`` / ``z0`` as ``DeviceFactor`` or CUDA
    tensors) or when ``nwtn_adi_dict['device_resident']`` is set, and accepts one as ``z0``;
    ``get_mTzzTtb`` takes one as ``Z`` / ``tb``.  The factor then never crosses PCIe between the calls of a
    time loop (``solve_dae_ric.py:147-189``: ``z0 = Zc`` of the previous step, gain from the new factor).
    ``np.asarray(f)`` (or ``f.numpy()``) downloads it; everything that expects an ndarray still works that way."""

    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t

    @property
    def shape(self):
        return tuple(self.t.shape)

    ndim = 2
    dtype = np.dtype(np.float64)

    def numpy(self):
        return self.t.cpu().numpy()

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype, copy=False)


def to_device(a):
    """Upload a dense / sparse ``NV x q`` matrix once; the result can be passed wherever the mirror takes a
    dense panel (``bmat``, ``wmat``, ``z0``, ``tb``)."""
    import torch
    if isinstance(a, DeviceFactor):
        return a
    if torch.is_tensor(a):
        return DeviceFactor(a.to(device="cuda", dtype=torch.float64).contiguous())
    h = np.array(_dense(a), dtype=np.float64, order="C")           # private, writable copy for from_numpy
    t = torch.from_numpy(h).to("cuda:%d" % backend.device_id())
    torch.cuda.synchronize()
    return DeviceFactor(t)


def _host(a):
    """ndarray / sparse matrix as is; a device panel downloaded."""
    if isinstance(a, DeviceFactor):
        return a.numpy()
    if _on_device(a):
        return a.cpu().numpy()
    return a


def _on_device(a):
    if isinstance(a, DeviceFactor):
        return True
    try:
        import torch
    except ImportError:
        return False
    return torch.is_tensor(a) and a.is_cuda

# Built-in shift list for an ``adi_dict`` without ``'ms'``
# (tests/test_units_compfacres_compress.py:54-64 relies on such a default; the
# upstream values are not in the container) [INFERRED].
DEFAULT_MS = [-30.0, -20.0, -10.0, -5.0, -3.0, -1.0]


def _dense(a):
    if sps.issparse(a):
        return np.asarray(a.todense())
    a = np.asarray(a, dtype=float)
    return a.reshape(-1, 1) if a.ndim == 1 else a


_orient_memo = {}


def _content_sig(m):
    """Exact content key of a scipy sparse matrix as handed over (no format conversion): see backend.content_hash."""
    return backend.content_hash(m)


def _orient(amat, mmat, transposed):
    """(cal A, cal E) in CSR.  The reference re-passes the same matrices with every call
    (``optcont_main.py:488-492``): the conversion (two CSR transposes, ~5 ms at n = 3e4) is remembered for the last
    operands -- keyed by object identity AND the exact content key (128-bit hash of the index and value bytes), so an
    operand changed in place is converted anew, whatever its sums."""
    key = (id(amat), id(mmat), bool(transposed))
    if sps.issparse(amat) and sps.issparse(mmat):
        sig = (_content_sig(amat), _content_sig(mmat))
        hit = _orient_memo.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1], hit[2]
    else:
        sig = None
    a = sps.csr_matrix(amat)
    e = sps.csr_matrix(mmat)
    if not transposed:
        a, e = a.T.tocsr(), e.T.tocsr()
    if sig is not None:
        if a is amat or e is mmat:            # never tag or keep the caller's own objects
            a, e = a.copy(), e.copy()
        a._ricadi_fp = backend._fingerprint(a)
        e._ricadi_fp = backend._fingerprint(e)
        _orient_memo.clear()
        _orient_memo[key] = (sig, a, e)
    return a, e


def _is_auto(ms):
    return isinstance(ms, str) and ms in ("auto", "auto-complex")


def _has_pairs(ms):
    return any(isinstance(p, complex) for p in ms)


def _shifts(d):
    """The shift list of an ``adi_dict``: ``DEFAULT_MS`` without ``'ms'``, the strings ``'auto'`` and
    ``'auto-complex'`` as they are (the caller generates the list, :func:`_auto_shifts`), else a list of negative
    reals -- or, with a complex entry in it, of negative reals (``float``) and complex numbers with a negative real
    part (``complex``), each of which stands for the pair ``(p, conj p)``; an entry immediately followed by its exact
    conjugate is that one pair."""
    ms = d.get("ms", DEFAULT_MS)
    if _is_auto(ms):
        return ms
    ms = list(ms)
    if all(np.isreal(p) for p in ms):
        if any(p >= 0 for p in ms):
            raise ValueError("ADI shifts must be negative real numbers")
        return [float(np.real(p)) for p in ms]
    out, i = [], 0
    while i < len(ms):
        p = complex(ms[i])
        if not (np.isfinite(p.real) and np.isfinite(p.imag) and p.real < 0):
            raise ValueError("ADI shifts must be negative real numbers")
        if p.imag == 0.0:
            out.append(p.real)
        else:
            out.append(p)
            if i + 1 < len(ms) and complex(ms[i + 1]) == p.conjugate():
                i += 1
        i += 1
    return out


def _real_shifts(d):
    """:func:`_shifts` for the iterations that take real shifts only (Newton-ADI, RADI)."""
    ms = _shifts(d)
    if ms == "auto-complex" or (not _is_auto(ms) and _has_pairs(ms)):
        raise ValueError("ADI shifts must be negative real numbers")
    return ms


def _broadcast_shifts(ms):
    """Rank 0's list on every rank of the default ``torch.distributed`` group (all ranks must solve with the
    same shifts; their Ritz values may differ in the last bits).  No-op in a single process."""
    try:
        import torch
        import torch.distributed as dist
    except ImportError:
        return ms
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() <= 1:
        return ms
    dev = "cuda:%d" % backend.device_id() if dist.get_backend() == "nccl" else "cpu"
    buf = torch.zeros(_lib.MAX_M + 1, dtype=torch.float64, device=dev)
    if dist.get_rank() == 0:
        buf[0] = len(ms)
        buf[1:1 + len(ms)] = torch.tensor(list(ms), dtype=torch.float64)
    dist.broadcast(buf, src=0)
    h = buf.cpu().numpy()
    out = adi_shifts.ShiftList(float(x) for x in h[1:1 + int(h[0])])
    out.info = dict(getattr(ms, "info", {}), broadcast=True)
    return out


def _auto_shifts(ctx, d, W, keep_complex=False):
    """``ms='auto'``: shifts from the operator of ``ctx`` as it stands (low-rank term included) and the
    right-hand side factor ``W``; ``adi_dict['num_shifts']`` / ``['shift_warm_steps']``.  ``keep_complex``
    (``ms='auto-complex'``): Ritz values off the real axis stay complex and are selected as pairs."""
    ms = adi_shifts.auto_shifts(ctx, W, num=int(d.get("num_shifts", 8)),
                                warm_steps=int(d.get("shift_warm_steps", 2)), default=DEFAULT_MS,
                                keep_complex=keep_complex)
    return ms if _has_pairs(ms) else _broadcast_shifts(ms)


def solve_proj_lyap_stein(amat=None, mmat=None, jmat=None, wmat=None,
                          umat=None, vmat=None, transposed=False,
                          adi_dict=None, nwtn_adi_dict=None, **kw):
    """Low-rank ADI for ``F^T X M + M^T X F + W W^T = 0`` on ker(J M^-1 ...).

    ``F = amat - umat*vmat``; ``transposed=True`` swaps the roles
    (``F X M^T + M X F^T``).  Signature and ``['zfac']`` return as at
    ``tests/test_units_compfacres_compress.py:62-64``.

    ``adi_dict['ms']`` may hold complex entries with a negative real part: each stands for the conjugate pair
    ``(p, conj p)`` and is one complex solve and two steps (step form, ``umat`` / ``vmat`` included);
    ``ms='auto-complex'`` generates such a list.  The call then also returns ``['ms']`` (the list as parsed, one
    entry per pair) and ``['pair_info']`` (``Context.adi_pair_info``).
    """
    d = nwtn_adi_dict if adi_dict is None else adi_dict
    d = {} if d is None else d
    calA, calE = _orient(amat, mmat, transposed)
    ctx = backend.context_for(calA, calE, jmat)
    # low-rank term in cal A's orientation:  cal A - U V^T
    if umat is not None and vmat is not None:
        if transposed:
            ctx.set_lowrank(_dense(umat), _dense(vmat).T)
        else:                      # (amat - U V)^T = amat^T - V^T U^T
            ctx.set_lowrank(_dense(vmat).T, _dense(umat))
    else:
        ctx.set_lowrank(None, None)
    prm = _lib.adi_params(d)
    W = _dense(wmat)
    out = {}
    want_hist = _wants_res_hist(d, prm)
    ctx.set_adi_res_history(bool(d.get("adi_res_hist", False)))
    try:
        if W.shape[1] > _lib.MAX_M:
            raise ValueError("right-hand side factor wider than {0} columns".format(_lib.MAX_M))
        ms = _shifts(d)
        if _is_auto(ms):
            ms = _auto_shifts(ctx, d, W, keep_complex=ms == "auto-complex")
            out["ms"], out["shift_info"] = list(ms), dict(ms.info)
        elif _has_pairs(ms):
            out["ms"] = list(ms)          # as parsed: one complex entry per pair
        backend.ensure_exchange(ctx, W.shape[1], len(ms))
        if d.get("device_resident", False):
            # the factor stays in HBM (DeviceFactor): NV x (steps m) doubles need not cross PCIe to form a gain
            import torch
            _, info = ctx.lyap_adi(ms, W, prm, fetch=False)
            Zt = torch.empty((ctx.nv, info["cols"]), dtype=torch.float64, device="cuda")
            if info["cols"] > 0:
                ctx.factor_get_dev(Zt.data_ptr(), info["cols"])
            Z = DeviceFactor(Zt)
        else:
            Z, info = ctx.lyap_adi(ms, W, prm)
        if d.get("check_lyap_res", False):
            # optcont_main.py:130 -- the residual of the equation just solved, evaluated
            # independently of the ADI recurrence from the factors (a5, same context)
            out["lyap_res"] = float(np.sqrt(abs(ctx.lyap_res_norm(_dense(_host(Z)), W))))
            if d.get("verbose", False):
                print("projected Lyapunov residual (factored): {0:.3e}; ADI recurrence: {1:.3e}"
                      .format(out["lyap_res"], info["res_fro"]))
        if want_hist:
            out["adi_res_hist"] = ctx.adi_res_history()
    finally:
        ctx.set_lowrank(None, None)
        ctx.set_adi_res_history(False)
    out["zfac"] = Z
    out.update(info)
    return out


def _wants_res_hist(d, prm):
    """``out['adi_res_hist']`` is returned when the residual rule is on (``adi_res_reltol`` > 0) or
    ``adi_dict['adi_res_hist']`` asks for it."""
    return prm.adi_res_reltol > 0.0 or bool(d.get("adi_res_hist", False))


def proj_alg_ric_newtonadi(mmat=None, amat=None, jmat=None, bmat=None,
                           wmat=None, z0=None, mtxoldb=None,
                           transposed=False, nwtn_adi_dict=None, **kw):
    """Newton-Kleinman ADI for the projected algebraic Riccati equation.

    ``cal A X cal E^T + cal E X cal A^T - cal E X B B^T X cal E^T + W W^T = 0``
    with ``cal A = amat^T``, ``cal E = mmat^T`` (as given if ``transposed``).
    Call sites: ``optcont_main.py:488-492`` (steady state),
    ``solve_dae_ric.py:152-159`` (one call per backward time step).  Returns a
    dict whose ``'zfac'`` is the low-rank factor.
    """
    d = {} if nwtn_adi_dict is None else nwtn_adi_dict
    calA, calE = _orient(amat, mmat, transposed)
    ctx = backend.context_for(calA, calE, jmat)
    ctx.set_lowrank(None, None)
    prm = _lib.adi_params(d)
    if "sweep_width" not in d:
        # Sweep form of the inner ADI (up to 16 steps = one batched solve): the same
        # Z Z^T per step count, inner stopping rule applied once per sweep; 2.5-3x the
        # throughput of one shift-solve at a time on one GPU.  ``sweep_width=1`` in the
        # dict restores the step-by-step recurrence of the reference.
        prm.sweep_width = 16
    ms = _real_shifts(d)
    sinfo = None
    if _is_auto(ms):
        ms = _newton_auto_shifts(ctx, d, calE, bmat, wmat, z0, mtxoldb)
        sinfo = dict(ms.info)
    want_hist = _wants_res_hist(d, prm)
    ctx.set_adi_res_history(bool(d.get("adi_res_hist", False)))
    try:
        out, info = _newtonadi_call(ctx, d, ms, prm, bmat, wmat, z0, mtxoldb)
        if want_hist:
            # of the last Newton step's Lyapunov solve
            out["adi_res_hist"] = ctx.adi_res_history()
    finally:
        ctx.set_adi_res_history(False)
    out.update(info)
    if sinfo is not None:
        out["ms"], out["shift_info"] = list(ms), sinfo
    if d.get("check_lyap_res", False):
        # optcont_main.py:130: residual of the last Newton step's Lyapunov equation --
        # in residual-form ADI it is W_end W_end^T, whose norm the driver returns
        out["lyap_res"] = info["lyap_res_fro"]
        if d.get("verbose", False):
            print("last Newton step: projected Lyapunov residual {0:.3e} (rhs {1:.3e})"
                  .format(info["lyap_res_fro"], info["lyap_rhs_fro"]))
    return out


def _newtonadi_call(ctx, d, ms, prm, bmat, wmat, z0, mtxoldb):
    """The library call of :func:`proj_alg_ric_newtonadi`; returns ``(out, info)``."""
    if d.get("device_resident", False) or any(_on_device(x) for x in (bmat, wmat, z0, mtxoldb)):
        # every panel in HBM (uploaded here once if it came as an ndarray), the new factor returned as a
        # DeviceFactor: no PCIe traffic in the call when the caller keeps its panels on the device
        Bt, Wt = to_device(bmat).t, to_device(wmat).t
        backend.ensure_exchange(ctx, Bt.shape[1] + Wt.shape[1], len(ms))
        Zt, info = ctx.ric_newtonadi_dev(ms, Bt, Wt, prm,
                                         Z0_t=None if z0 is None else to_device(z0).t,
                                         old_t=None if mtxoldb is None else to_device(mtxoldb).t)
        out = dict(zfac=DeviceFactor(Zt))
    else:
        B, W = _dense(bmat), _dense(wmat)
        backend.ensure_exchange(ctx, B.shape[1] + W.shape[1], len(ms))
        Z, info = ctx.ric_newtonadi(ms, B, W, prm,
                                    Z0=None if z0 is None else _dense(z0),
                                    oldB=None if mtxoldb is None else _dense(mtxoldb))
        out = dict(zfac=Z)
    return out, info


def proj_alg_ric_radi(mmat=None, amat=None, jmat=None, bmat=None, wmat=None, z0=None, mtxoldb=None,
                      transposed=False, radi_dict=None):
    """Low-rank RADI (Benner, Bujanovic, Kuerschner, Saak 2018) for the projected algebraic Riccati equation of
    :func:`proj_alg_ric_newtonadi` -- same operands, same orientation rules --, solved directly: one saddle-point
    shift solve with the current closed loop per step, no Newton loop, no initial iterate.  The projected Riccati
    residual of the iterate is ``R_j R_j^T`` with the residual factor the iteration carries, so the call stops on
    ``||R_j^T R_j||_F / ||R_0^T R_0||_F <= radi_res_reltol``.

    ``z0`` is accepted for call compatibility with :func:`proj_alg_ric_newtonadi` and IGNORED: the iteration
    starts from zero.

    ``radi_dict`` keys: ``ms`` (negative real shifts, cycled; ``'auto'`` generates them as the Newton call does for
    its first step; ``'hamiltonian'`` starts with ``adi_shifts.initial_shift`` of the operator and generates every
    later shift from the iteration itself -- ``ricadi_set_radi_shifts``; needs at most 32 columns in
    ``wmat``; ``'hamiltonian-dominant'`` is the same rule on the at most 32 dominant directions of the new block,
    for a ``wmat`` of any width RADI takes -- DESIGN.md 3d-2; ``'hamiltonian-sweep'`` is that rule in SWEEPS: the
    iteration generates up to ``sweep_width`` shifts at a time from all blocks the last sweep kept and solves them in
    ONE lockstep batch, ``ricadi_set_radi_sweep_shifts``, DESIGN.md 3d-4 -- ``sweep_width`` defaults to 8 for this
    ``ms`` only, 1 .. 16 are accepted, and at 1 it is ``'hamiltonian-dominant'``), ``ms_fallback`` (with a generated ``ms`` only: a list of negative reals that replaces that one-element
    list -- its first entry starts, the list is cycled where a shift cannot be generated), ``radi_max_steps`` (200),
    ``radi_res_reltol`` (1e-10), ``compress_cols`` (the factor is recompressed whenever it has grown by that many
    columns; default 512), ``sweep_width`` (1; with a list of shifts, up to that many consecutive steps are solved
    in ONE lockstep batch against the same panel and recombined -- the sweep form; at most 16, what
    runs is what the list allows; a ``ValueError`` with a generated ``ms`` other than ``'hamiltonian-sweep'``),
    ``verbose``, ``device_resident``.

    Returns a dict: ``zfac`` (ndarray; a :class:`DeviceFactor` when given device panels or with
    ``device_resident``), ``gain`` = ``cal E X B`` (ndarray), ``radi_steps``, ``res_hist`` (the relative residual
    after every step), ``stop_rule`` (``_lib.RICADI_STOP_RES`` or ``_lib.RICADI_STOP_MAX_STEPS``),
    ``gmres_nonconverged``, ``shift_solves`` (every solve issued: with sweeps up to ``sweep_width - 1`` more than
    ``radi_steps``), ``gmres_iters``, ``sweep_width`` (the width that ran), ``sweeps`` (and ``ms`` / ``shift_info`` with ``ms='auto'``; with
    a generated ``ms``: ``ms`` -- the shift of every step -- and ``shift_fallbacks``; with ``'hamiltonian-sweep'`` also
    ``sweep_widths``, the solves of every sweep, and ``sweep_width`` is the cap of the call)."""
    d = {} if radi_dict is None else radi_dict
    calA, calE = _orient(amat, mmat, transposed)
    ctx = backend.context_for(calA, calE, jmat)
    ctx.set_lowrank(None, None)
    gensweep = isinstance(d.get("ms"), str) and d["ms"] == "hamiltonian-sweep"
    generated = gensweep or (isinstance(d.get("ms"), str) and d["ms"] in ("hamiltonian", "hamiltonian-dominant"))
    sinfo = None
    if generated:
        fb = d.get("ms_fallback")
        ms = [adi_shifts.initial_shift(ctx.diag_ratio)] if fb is None else _real_shifts(dict(ms=list(fb)))
    else:
        ms = _real_shifts(d)
        if _is_auto(ms):
            ms = _newton_auto_shifts(ctx, d, calE, bmat, wmat, None, mtxoldb)
            sinfo = dict(ms.info)
    kw = dict(max_steps=int(d.get("radi_max_steps", 200)), res_reltol=float(d.get("radi_res_reltol", 1e-10)),
              compress_cols=int(d.get("compress_cols", 0)), verbose=bool(d.get("verbose", False)))
    # the shift mode is a context setting: set for this call, and as before after it, also when the call fails
    # ... and so is the sweep width
    # ... and the generated sweep shifts ('hamiltonian-sweep': the dominant mode, the setting, a default width of 8)
    width_before = ctx.set_radi_sweep_width(int(d.get("sweep_width", 8 if gensweep else 1)))   # (else the default MEANS 1)
    mode_before = sweep_shifts_before = None
    try:
        if generated:
            mode_before = ctx.set_radi_shifts("hamiltonian-dominant" if gensweep else d["ms"])
        if gensweep:
            sweep_shifts_before = ctx.set_radi_sweep_shifts(True)
        if d.get("device_resident", False) or any(_on_device(x) for x in (bmat, wmat, mtxoldb)):
            Zt, Kt, info = ctx.ric_radi_dev(ms, to_device(bmat).t, to_device(wmat).t,
                                            old_t=None if mtxoldb is None else to_device(mtxoldb).t, **kw)
            Z, K = DeviceFactor(Zt), Kt.cpu().numpy()
        else:
            Z, K, info = ctx.ric_radi(ms, _dense(bmat), _dense(wmat),
                                      oldB=None if mtxoldb is None else _dense(mtxoldb), **kw)
    finally:
        if sweep_shifts_before is not None:
            ctx.set_radi_sweep_shifts(sweep_shifts_before)
        if mode_before is not None:
            ctx.set_radi_shifts(mode_before)
        ctx.set_radi_sweep_width(width_before)
    swi = ctx.radi_sweep_info()
    out = dict(zfac=Z, gain=K, radi_steps=info["radi_steps"], res_hist=ctx.adi_res_history(),
               stop_rule=ctx.STOP_RULES.index(info["stop_rule"]), gmres_nonconverged=info["gmres_nonconverged"],
               shift_solves=info["shift_solves"], gmres_iters=info["gmres_iters"], sweep_width=swi["width"],
               sweeps=swi["sweeps"])
    if sinfo is not None:
        out["ms"], out["shift_info"] = list(ms), sinfo
    if generated:
        out["ms"], out["shift_fallbacks"] = list(ctx.radi_shift_history()), ctx.radi_shift_fallbacks()
    if gensweep:
        out["sweep_widths"] = [int(v) for v in ctx.radi_sweep_widths()]
    return out


def _newton_auto_shifts(ctx, d, calE, bmat, wmat, z0, mtxoldb):
    """``ms='auto'`` of the Newton iteration: one list for every Newton step of the call, generated on the first
    step's Lyapunov operator ``cal A - (K_0 - old) B^T`` with right-hand side ``[W, K_0]``, ``K_0 = cal E Z_0 Z_0^T B``
    (just ``W`` and ``cal A + old B^T`` without ``z0``)."""
    B, W = _dense(_host(bmat)), _dense(_host(wmat))
    K0 = None if z0 is None else np.asarray(calE @ (_dense(_host(z0)) @ (_dense(_host(z0)).T @ B)))
    U = None
    if K0 is not None:
        U = K0.copy()
    if mtxoldb is not None:
        old = _dense(_host(mtxoldb))
        U = -old if U is None else U - old
    rhs = W if K0 is None else np.hstack([W, K0])
    if U is not None:
        ctx.set_lowrank(U, B)
    try:
        return _auto_shifts(ctx, d, rhs)
    finally:
        ctx.set_lowrank(None, None)


def compress_Zsvd(Z, thresh=None, k=None, shplot=False):
    """Column compression ``Zc Zc^T ~ Z Z^T`` (``solve_dae_ric.py:162-163``).

    Keeps the singular values above ``thresh`` (absolute) and at most ``k``.
    On the GPU, as the reference's comment has it ("QR ... SVD", ``optcont_main.py:133-134``):
    thin block QR of ``Z`` on the FP64 matrix cores, SVD of the small ``R``, ``Zc = Z V_k``
    (factors wider than 1024 columns, or ``backend.configure(compress_qr=0)``: Gram matrix +
    symmetric eigendecomposition).  ``shplot`` is accepted and ignored.
    """
    Z = _dense(_host(Z))
    ctx = backend.context_dims(Z.shape[0])
    Zc, _ = ctx.compress(Z, thresh=thresh, k=k)
    return Zc


def get_mTzzTtb(MT, Z, tb, output=None):
    """``MT * (Z * (Z^T * tb))``; the feedback gain is its negative
    (``optcont_main.py:505-506``; ``solve_dae_ric.py:101,183,189``)."""
    if _on_device(Z) and backend.operator_has_cale(MT):
        # factor (and, if it was staged, tb) in HBM and MT = cal E of the resident operator: K on the device,
        # only the NV x q result comes back
        import torch
        ctx = backend.context()
        Zt, Bt = to_device(Z).t, to_device(tb).t
        Kt = torch.empty_like(Bt)
        torch.cuda.current_stream().synchronize()
        ctx.gain_dev(1.0, Zt.data_ptr(), Zt.shape[1], Zt.shape[1], Bt.data_ptr(), Bt.shape[1], Kt.data_ptr())
        return Kt.cpu().numpy()
    Z = _dense(_host(Z))
    ctx = backend.context_dims(Z.shape[0])
    return ctx.gain(_dense(_host(tb)), Z=Z, MT=sps.csr_matrix(MT))


def comp_proj_lyap_res_norm(Z, amat=None, mmat=None, wmat=None, jmat=None,
                            umat=None, vmat=None):
    """Squared Frobenius norm of the projected Lyapunov residual from factors.

    Positional use ``comp_proj_lyap_res_norm(Z, F, M, W, J)`` as at
    ``tests/test_units_compfacres_compress.py:82,104``.
    """
    calA, calE = _orient(amat, mmat, False)
    ctx = backend.context_for(calA, calE, jmat)
    if umat is not None and vmat is not None:
        ctx.set_lowrank(_dense(vmat).T, _dense(umat))
    else:
        ctx.set_lowrank(None, None)
    try:
        return ctx.lyap_res_norm(_dense(Z), _dense(wmat))
    finally:
        ctx.set_lowrank(None, None)
