"""ctypes binding of the C-ABI declared in include/gpe.h.

``libgpengine.so`` (prefix ``gpe_``) is the product: hand-written HIP for gfx950.
:func:`load_engine` raises if it is missing — there is no CPU fallback, and this module
knows of no other implementation.  (``Lib`` takes the symbol prefix as an argument so that
the test infrastructure under ``oracle/`` can bind its checker, which exports the same
signatures, with the same ``Handle`` class; that loader lives in ``oracle/binding.py``.)
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
ROOT = _PKG.parent
ENGINE_SO = _PKG / "libgpengine.so"

KERNEL_SE_ARD, KERNEL_MATERN52, KERNEL_MATERN32, KERNEL_EXP, KERNEL_HOST_K = range(5)
KERNEL_NAMES = {"se_ard": 0, "matern52": 1, "matern32": 2, "exp": 3, "host_k": 4}
SELECT_UCB, SELECT_EI, SELECT_VAR = range(3)  # include/gpe_batch_select.h: the rules of select_batch
REMOVE_AUTO, REMOVE_UPDATE, REMOVE_RECOMPUTE = range(3)  # include/gpe_remove.h: the `how` of remove_samples
REMOVE_HOW = {"auto": 0, "update": 1, "recompute": 2}
KG_MAX_ALTERNATIVES = 2048  # include/gpe_kg.h: GPE_KG_MAX_ALTERNATIVES
EHVI_MAX_FRONT = 2048  # include/gpe_ehvi.h: GPE_EHVI_MAX_FRONT
EHVI3_MAX_FRONT = 1024  # include/gpe_ehvi3.h: GPE_EHVI3_MAX_FRONT
CEI_MAX_CONSTRAINTS = 16  # include/gpe_cei.h: GPE_CEI_MAX_CONSTRAINTS
MES_MAX_OUTPUTS, MES_MAX_SAMPLES = 8, 1024  # include/gpe_mes.h: GPE_MES_MAX_OUTPUTS, GPE_MES_MAX_SAMPLES
NEI_MAX_BASELINE, NEI_MAX_SAMPLES = 1024, 1024  # include/gpe_nei.h: GPE_NEI_MAX_BASELINE, GPE_NEI_MAX_SAMPLES

PH_KERNEL_BUILD, PH_POTRF_PANEL, PH_POTRF_UPDATE, PH_SOLVE, PH_LOGLIK, PH_INV, PH_GRAD, PH_QUERY, PH_POTRF_TALL, PH_POTRF_TAIL = range(10)
PH_COUNT = 10
PHASE_NAMES = ["kernel_build", "potrf_panel", "potrf_update", "solve", "loglik", "inv", "grad", "query", "potrf_tall", "potrf_tail"]

_dp = C.POINTER(C.c_double)
_i64 = C.c_int64
_vp = C.c_void_p


class EngineError(RuntimeError):
    pass


def _sig(lib, prefix):
    """Declare argtypes/restype for every symbol of include/gpe.h (required symbols
    must exist; a missing one raises AttributeError -> surfaced by tests)."""
    S = {
        "create": [C.c_int, C.POINTER(_vp)],
        "clone": [_vp, C.POINTER(_vp)],
        "clone_to": [_vp, C.c_int, C.POINTER(_vp)],
        "device_count": [C.POINTER(C.c_int)],
        "get_device": [_vp, C.POINTER(C.c_int)],
        "destroy": [_vp],
        "set_data": [_vp, _dp, _i64, C.c_int, _dp, C.c_int],
        "set_data_device": [_vp, _vp, _i64, C.c_int, _vp, C.c_int],
        "set_kernel": [_vp, C.c_int, _dp, C.c_int, C.c_double],
        "set_K_host": [_vp, _dp, _i64],
        "compute": [_vp],
        "update_alpha": [_vp, _dp],
        "add_sample": [_vp, _dp, C.c_int, _dp, C.c_int],
        "log_lik": [_vp, _dp],
        "compute_inv_kernel": [_vp],
        "log_lik_grad": [_vp, _dp, C.c_int, C.c_int],
        "sparsify": [C.c_int, _dp, _i64, C.c_int, _i64, C.POINTER(_i64), C.POINTER(_i64)],
        "log_loo_cv": [_vp, _dp],
        "log_loo_cv_grad": [_vp, _dp, C.c_int, C.c_int],
        "get_loo_weights": [_vp, _dp, _i64],
        "hp_objective": [_vp, C.c_int, _dp, C.c_int, C.c_double, C.c_int, C.c_int, _dp, _dp],
        "query_batch": [_vp, _dp, _i64, _dp, _dp],
        "query_batch_cross": [_vp, _dp, _i64, _dp, _dp],
        "set_obs_mean": [_vp, _dp],
        "nb_samples": [_vp, C.POINTER(_i64)],
        "get_L": [_vp, _dp, _i64],
        "set_L": [_vp, _dp, _i64],
        "get_alpha": [_vp, _dp],
        "set_alpha": [_vp, _dp],
        "get_Kinv": [_vp, _dp, _i64],
        "get_K": [_vp, _dp, _i64],
        "batch_compute": [C.POINTER(_vp), C.c_int, C.POINTER(C.c_int)],
        "batch_log_lik": [C.POINTER(_vp), C.c_int, _dp],
        "batch_hp_objective": [C.POINTER(_vp), C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, C.POINTER(C.c_int)],
        "synchronize": [_vp],
    }
    for name, args in S.items():
        f = getattr(lib, prefix + name)
        f.argtypes = args
        f.restype = C.c_int
    for name in ("last_error",):
        f = getattr(lib, prefix + name)
        f.argtypes = [_vp]
        f.restype = C.c_char_p
    f = getattr(lib, prefix + "version")
    f.argtypes = []
    f.restype = C.c_char_p
    if prefix == "gpe_":
        G = {
            "get_stream": [_vp, C.POINTER(_vp)],
            "set_profiling": [_vp, C.c_int],
            "get_phase_ms": [_vp, _dp, C.POINTER(_i64), _dp, C.c_int],
            "reset_phase_ms": [_vp],
            "flow_retries": [_vp, C.POINTER(_i64)],
            "handover_reruns": [_vp, C.POINTER(_i64)],
            "small_calls": [_vp, C.POINTER(_i64)],
            "mfma_f64_peak": [C.c_int, _dp],
            "trace": [C.c_int],
            "trace_dump": [C.c_char_p],
            "hbm_stream_peak": [C.c_int, _dp],
            "epoch": [_vp, C.POINTER(C.c_uint64)],
            "xproc_waits": [C.POINTER(_i64)],
            "debug_live_buffers": [C.POINTER(_i64), C.POINTER(_i64)],
            # include/gpe_joint.h: the joint posterior over a point batch
            "joint_query": [_vp, _dp, _i64, C.c_double, _dp, _dp, _i64],
            "joint_draws": [_vp, _dp, _i64, C.c_double, _dp, _dp, C.c_int, _dp, C.POINTER(_i64), _dp],
            "joint_max_points": [_vp, C.POINTER(_i64)],
            "joint_phase_ms": [_vp, _dp],
            "debug_cov_plan": [_i64, _i64, C.c_int, C.POINTER(_i64), _i64],
            # include/gpe_append.h: a batch of samples appended in one blocked update
            "add_samples": [_vp, _dp, _i64, C.c_int, _dp, C.c_int],
            "append_max_chunk": [],
            "debug_append_slices": [_i64, C.POINTER(_i64), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_i64)],
            # include/gpe_remove.h: samples removed by a blocked update of the factor
            "remove_samples": [_vp, C.POINTER(_i64), _i64, _dp, C.c_int, C.c_int],
            "remove_max_vectors": [],
            "debug_remove_plan": [_i64, _i64, _i64, C.c_int, C.POINTER(_i64)],
            # include/gpe_sparse.h: the sparse pseudo-input GP
            "sp_create": [C.c_int, C.POINTER(_vp)],
            "sp_destroy": [_vp],
            "sp_set_data": [_vp, _dp, _i64, C.c_int, _dp, C.c_int],
            "sp_set_pseudo": [_vp, _dp, _i64],
            "sp_set_hparams": [_vp, _dp, C.c_double, C.c_double, C.c_double],
            "sp_compute": [_vp],
            "sp_nlml": [_vp, _dp],
            "sp_objective": [_vp, _dp, C.c_double, C.c_double, C.c_double, _dp],
            "sp_predict": [_vp, _dp, _i64, _dp, _dp],
            "sp_get_L": [_vp, _dp, _i64],
            "sp_get_Lm": [_vp, _dp, _i64],
            "sp_get_bet": [_vp, _dp],
            "sp_get_ep": [_vp, _dp],
            "sp_set_profiling": [_vp, C.c_int],
            "sp_phase_ms": [_vp, _dp],
            "debug_gram_plan": [_i64, _i64, _i64, C.c_int, C.POINTER(_i64), _i64],
            # include/gpe_sparse_grad.h: its analytic gradient
            "sp_grad": [_vp, _dp, _dp],
            "sp_objective_grad": [_vp, _dp, _dp, C.c_double, C.c_double, C.c_double, _dp, _dp, _dp],
            "sp_grad_phase_ms": [_vp, _dp],
            # include/gpe_query_grad.h: the batched posterior with its gradient in the query point
            "query_batch_grad": [_vp, _dp, _i64, _dp, _dp, _dp, _dp],
            "query_grad_phase_ms": [_vp, _dp],
            # include/gpe_pathwise.h: posterior draws as functions of the query point
            "paths_create": [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(_vp)],
            "paths_eval": [_vp, _dp, _i64, _dp, _dp, _dp],
            "paths_argmax": [_vp, _dp, _i64, _dp, C.POINTER(_i64), _dp],
            "paths_info": [_vp, C.POINTER(_i64), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
            "paths_phase_ms": [_vp, _dp],
            "paths_destroy": [_vp],
            # include/gpe_batch_select.h: greedy batch selection with hallucinated observations
            "select_batch": [_vp, _dp, _i64, C.c_int, C.c_int, C.c_double, _dp, C.c_double, C.c_double, C.c_int, C.POINTER(_i64), _dp, _dp,
                             _dp, _i64],
            "select_phase_ms": [_vp, _dp],
            "debug_select_plan": [_i64, _i64, C.c_int, C.POINTER(_i64), _i64],
            # include/gpe_kg.h: the knowledge gradient over a finite alternative set
            "kg_batch": [_vp, _dp, _i64, _dp, _dp, _i64, _dp, C.c_double, C.c_int, _dp, _dp, _dp, _i64],
            "kg_envelope": [_vp, _dp, _i64, _dp, _i64, _i64, _dp, C.POINTER(C.c_int32)],
            "kg_phase_ms": [_vp, _dp],
            # include/gpe_ehvi.h: the two-objective expected hypervolume improvement over a Pareto front
            "ehvi2_front": [_dp, _i64, _dp, _dp, C.POINTER(_i64)],
            "ehvi2_values": [_vp, _dp, _i64, _dp, _dp, _dp, _dp, _dp, _i64, _dp, _dp],
            "ehvi2_batch": [_vp, C.c_int, C.c_int, _dp, _i64, _dp, C.c_double, _dp, _i64, _dp, _dp, _dp, _dp, _dp],
            "ehvi_phase_ms": [_vp, _dp],
            # include/gpe_ehvi3.h: the three-objective expected hypervolume improvement over a Pareto front
            "ehvi3_front": [_dp, _i64, _dp, _dp, C.POINTER(_i64)],
            "ehvi3_boxes": [_dp, _i64, _dp, C.c_int, _dp, _i64, C.POINTER(_i64)],
            "ehvi3_values": [_vp, _dp, _i64, _dp, _dp, _dp, _i64, _dp, _dp],
            "ehvi3_batch": [_vp, C.POINTER(C.c_int), _dp, _i64, _dp, C.c_double, _dp, _i64, _dp, _dp, _dp, _dp, _dp],
            "ehvi3_phase_ms": [_vp, _dp],
            # include/gpe_cei.h: constrained expected improvement in the log domain
            "logcei_values": [_vp, C.c_int, C.c_double, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _dp, _i64, _dp, _dp, _dp],
            "logcei_batch": [_vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), _dp, _dp, _i64, _dp, C.c_double,
                             _dp, _dp, _dp, _dp, _dp],
            "cei_phase_ms": [_vp, _dp],
            # include/gpe_mes.h: max-value entropy search in the log domain
            "mes_values": [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _i64, _dp, _dp, _dp],
            "mes_batch": [_vp, C.c_int, C.POINTER(C.c_int), C.c_int, _dp, _dp, _i64, _dp, C.c_double, _dp, _dp, _dp, _dp, _dp],
            "mes_phase_ms": [_vp, _dp],
            # include/gpe_nei.h: noisy expected improvement in the log domain
            "lognei_values": [_vp, C.c_int, _dp, C.c_double, _dp, _i64, _dp, _i64, _dp, _dp],
            "lognei_batch": [_vp, C.c_int, _dp, _i64, _dp, C.c_double, _dp, C.c_int, C.c_double, _dp, _i64, _dp, _dp, _dp, _dp, _dp, _dp,
                             _dp, _i64],
            "nei_phase_ms": [_vp, _dp],
        }
        for name, args in G.items():
            f = getattr(lib, prefix + name)
            f.argtypes = args
            f.restype = C.c_int
        f = getattr(lib, prefix + "sp_last_error")
        f.argtypes = [_vp]
        f.restype = C.c_char_p


class Lib:
    def __init__(self, path, prefix):
        self.path = str(path)
        self.prefix = prefix
        self.cdll = C.CDLL(self.path, mode=getattr(os, "RTLD_NOW", 2) | getattr(os, "RTLD_LOCAL", 0))
        _sig(self.cdll, prefix)

    def fn(self, name):
        return getattr(self.cdll, self.prefix + name)


_libs = {}


def load_engine() -> Lib:
    """The HIP library.  Fails loudly when it has not been built (no CPU fallback)."""
    if "gpe" not in _libs:
        if not ENGINE_SO.exists():
            raise EngineError(
                f"{ENGINE_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        _libs["gpe"] = Lib(ENGINE_SO, "gpe_")
    return _libs["gpe"]


def _d(a):
    return a.ctypes.data_as(_dp)


def _c(a, order="C"):
    return np.require(np.asarray(a, dtype=np.float64), requirements=["C" if order == "C" else "F", "A"])


def _front_args(front, ref):
    F = _c(np.asarray(front, dtype=np.float64).reshape(-1, 2))
    r = _c(np.asarray(ref, dtype=np.float64).reshape(2))
    return F, r


def ehvi2_front(points, ref, check=True):
    """gpe_ehvi2_front (include/gpe_ehvi.h; host only, no handle): the Pareto front of `points` (n x 2, both objectives maximised)
    above ref — dominated points, duplicates and points not above ref dropped, ascending in f1.  Returns (status, front (k, 2))."""
    F, r = _front_args(points, ref)
    out = np.zeros((max(F.shape[0], 1), 2))
    k = _i64(0)
    rc = load_engine().fn("ehvi2_front")(_d(F), F.shape[0], _d(r), _d(out), C.byref(k))
    if check and rc < 0:
        raise EngineError(f"gpe_ehvi2_front failed: status {rc}")
    return rc, out[: k.value].copy()


def _front3_args(front, ref):
    F = _c(np.asarray(front, dtype=np.float64).reshape(-1, 3))
    r = _c(np.asarray(ref, dtype=np.float64).reshape(3))
    return F, r


def ehvi3_front(points, ref, check=True):
    """gpe_ehvi3_front (include/gpe_ehvi3.h; host only, no handle): the Pareto front of `points` (n x 3, all objectives maximised)
    above ref — dominated points, duplicates and points not above ref dropped, descending in f3, ties ascending in f1, then f2.
    Returns (status, front (k, 3))."""
    F, r = _front3_args(points, ref)
    out = np.zeros((max(F.shape[0], 1), 3))
    k = _i64(0)
    rc = load_engine().fn("ehvi3_front")(_d(F), F.shape[0], _d(r), _d(out), C.byref(k))
    if check and rc < 0:
        raise EngineError(f"gpe_ehvi3_front failed: status {rc}")
    return rc, out[: k.value].copy()


def ehvi3_boxes(front, ref, axis, cap=None, check=True):
    """gpe_ehvi3_boxes (host only, no handle): the box table of a prepared front (n x 3) for the height axis `axis`, rows
    {l_a, u_a, l_b, u_b, h} with a < b the other two axes; also the prepared-front check.  cap: the rows there is room for (default
    2n + 1, which always suffices).  Returns (status, boxes (k, 5))."""
    F, r = _front3_args(front, ref)
    cap = 2 * F.shape[0] + 1 if cap is None else int(cap)
    out = np.zeros((max(cap, 1), 5))
    k = _i64(0)
    rc = load_engine().fn("ehvi3_boxes")(_d(F), F.shape[0], _d(r), int(axis), _d(out), cap, C.byref(k))
    if check and rc < 0:
        raise EngineError(f"gpe_ehvi3_boxes failed: status {rc}")
    return rc, out[: k.value].copy()


class Handle:
    """One GP behind the C-ABI.  Method names follow include/gpe.h."""

    def __init__(self, lib: Lib, device: int = 0, _h=None):
        self.lib = lib
        self.N = 0
        self.D = 0
        self.P = 0
        self.n_theta = 0
        if _h is None:
            h = _vp()
            self._chk(lib.fn("create")(device, C.byref(h)), None)
            self._h = h
        else:
            self._h = _h

    # -- plumbing
    def _chk(self, rc, what="call"):
        if rc < 0:
            msg = ""
            if what is not None and getattr(self, "_h", None):
                m = self.lib.fn("last_error")(self._h)
                msg = m.decode() if m else ""
            raise EngineError(f"{self.lib.prefix}{what} failed: status {rc} {msg}")
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self.lib.fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clone(self, device=None) -> "Handle":
        h = _vp()
        if device is None:
            self._chk(self.lib.fn("clone")(self._h, C.byref(h)), "clone")
        else:
            self._chk(self.lib.fn("clone_to")(self._h, int(device), C.byref(h)), "clone_to")
        o = Handle(self.lib, _h=h)
        o.N, o.D, o.P, o.n_theta = self.N, self.D, self.P, self.n_theta
        return o

    def device(self) -> int:
        d = C.c_int()
        self._chk(self.lib.fn("get_device")(self._h, C.byref(d)), "get_device")
        return d.value

    def epoch(self) -> int:
        """Moves with every call that can change what a query answers (include/gpe.h: gpe_epoch)."""
        e = C.c_uint64()
        self._chk(self.lib.fn("epoch")(self._h, C.byref(e)), "epoch")
        return e.value

    def flow_retries(self) -> int:
        n = _i64()
        self._chk(self.lib.fn("flow_retries")(self._h, C.byref(n)), "flow_retries")
        return n.value

    def handover_reruns(self) -> int:
        n = _i64()
        self._chk(self.lib.fn("handover_reruns")(self._h, C.byref(n)), "handover_reruns")
        return n.value

    def small_calls(self) -> int:
        n = _i64()
        self._chk(self.lib.fn("small_calls")(self._h, C.byref(n)), "small_calls")
        return n.value

    # -- data
    def set_data(self, X, obs_mean):
        X = _c(X)
        om = np.asarray(obs_mean, dtype=np.float64)
        if om.ndim == 1:
            om = om[:, None]
        om = _c(om, "F")
        self.N, self.D = X.shape
        self.P = om.shape[1]
        assert om.shape[0] == self.N
        self._chk(self.lib.fn("set_data")(self._h, _d(X), self.N, self.D, _d(om), self.P), "set_data")

    def set_data_device(self, dX_ptr: int, N: int, D: int, dom_ptr: int, P: int):
        self.N, self.D, self.P = N, D, P
        self._chk(self.lib.fn("set_data_device")(self._h, _vp(dX_ptr), N, D, _vp(dom_ptr), P), "set_data_device")

    def set_kernel(self, kind, log_theta, noise):
        kind = KERNEL_NAMES.get(kind, kind)
        th = _c(log_theta)
        self.n_theta = th.size
        self.kind = kind
        self._chk(self.lib.fn("set_kernel")(self._h, kind, _d(th), th.size, float(noise)), "set_kernel")

    def set_K_host(self, K):
        K = _c(K, "F")
        self._chk(self.lib.fn("set_K_host")(self._h, _d(K), K.shape[0]), "set_K_host")

    # -- hot path
    def compute(self) -> int:
        return self._chk(self.lib.fn("compute")(self._h), "compute")

    def update_alpha(self, obs_mean=None):
        if obs_mean is None:
            return self._chk(self.lib.fn("update_alpha")(self._h, None), "update_alpha")
        om = np.asarray(obs_mean, dtype=np.float64)
        if om.ndim == 1:
            om = om[:, None]
        om = _c(om, "F")
        return self._chk(self.lib.fn("update_alpha")(self._h, _d(om)), "update_alpha")

    def add_sample(self, x, obs_mean):
        x = _c(x)
        om = np.asarray(obs_mean, dtype=np.float64)
        if om.ndim == 1:
            om = om[:, None]
        om = _c(om, "F")
        if self.N == 0:
            self.D = x.size
            self.P = om.shape[1]
        assert om.shape[0] == self.N + 1
        rc = self._chk(self.lib.fn("add_sample")(self._h, _d(x), x.size, _d(om), om.shape[1]), "add_sample")
        self.N += 1
        return rc

    def add_samples(self, Xnew, obs_mean) -> int:
        """gpe_add_samples (include/gpe_append.h; HIP library only): q rows of Xnew appended in one blocked update; obs_mean has
        ALL N + q rows.  Returns the status: 0, or the 1-based first non-positive pivot."""
        om = np.asarray(obs_mean, dtype=np.float64)
        if om.ndim == 1:
            om = om[:, None]
        om = _c(om, "F")
        X = _c(Xnew)
        X = X.reshape(-1, self.D if self.N else (X.shape[-1] if X.ndim > 1 else X.size))
        q, D = X.shape
        if self.N == 0:
            self.D = D
            self.P = om.shape[1]
        assert om.shape[0] == self.N + q
        rc = self._chk(self.lib.fn("add_samples")(self._h, _d(X), q, D, _d(om), om.shape[1]), "add_samples")
        self.N += q
        return rc

    def remove_samples(self, idx, obs_mean, how="auto") -> int:
        """gpe_remove_samples (include/gpe_remove.h; HIP library only): the samples at the indices idx (any order) leave the model;
        obs_mean has ALL N - q remaining rows.  how: "auto", "update" (the factor update) or "recompute".  Returns the status, 0."""
        om = np.asarray(obs_mean, dtype=np.float64)
        if om.ndim == 1:
            om = om[:, None]
        om = _c(om, "F")
        ix = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).ravel())
        q = int(ix.size)
        assert om.shape[0] == self.N - q
        how = REMOVE_HOW.get(how, how)
        rc = self._chk(self.lib.fn("remove_samples")(self._h, ix.ctypes.data_as(C.POINTER(_i64)), q, _d(om), om.shape[1], int(how)),
                       "remove_samples")
        self.N -= q
        return rc

    def log_lik(self) -> float:
        out = C.c_double()
        self._chk(self.lib.fn("log_lik")(self._h, C.byref(out)), "log_lik")
        return out.value

    def compute_inv_kernel(self):
        return self._chk(self.lib.fn("compute_inv_kernel")(self._h), "compute_inv_kernel")

    def log_lik_grad(self, optimize_noise=False):
        n = self.n_theta + (1 if optimize_noise else 0)
        g = np.zeros(n)
        self._chk(self.lib.fn("log_lik_grad")(self._h, _d(g), n, int(optimize_noise)), "log_lik_grad")
        return g

    def log_loo_cv(self) -> float:
        out = C.c_double()
        self._chk(self.lib.fn("log_loo_cv")(self._h, C.byref(out)), "log_loo_cv")
        return out.value

    def log_loo_cv_grad(self, optimize_noise=False):
        n = self.n_theta + (1 if optimize_noise else 0)
        g = np.zeros(n)
        self._chk(self.lib.fn("log_loo_cv_grad")(self._h, _d(g), n, int(optimize_noise)), "log_loo_cv_grad")
        return g

    def get_loo_weights(self):
        W = np.zeros((self.N, self.N), order="F")
        self._chk(self.lib.fn("get_loo_weights")(self._h, _d(W), self.N), "get_loo_weights")
        return W

    def hp_objective(self, kind, log_theta, noise, optimize_noise=False, want_grad=True):
        kind = KERNEL_NAMES.get(kind, kind)
        th = _c(log_theta)
        self.n_theta = th.size
        lik = C.c_double()
        g = np.zeros(th.size + (1 if optimize_noise else 0))
        rc = self._chk(self.lib.fn("hp_objective")(self._h, kind, _d(th), th.size, float(noise),
                                                   int(optimize_noise), int(want_grad), C.byref(lik),
                                                   _d(g) if want_grad else None), "hp_objective")
        return (lik.value, g if want_grad else None, rc)

    def query_batch(self, Xq, want_mu=True, want_var=True):
        Xq = _c(Xq)
        M = Xq.shape[0]
        assert Xq.shape[1] == self.D
        kta = np.zeros((M, self.P), order="F") if want_mu else None
        var = np.zeros(M) if want_var else None
        self._chk(self.lib.fn("query_batch")(self._h, _d(Xq), M, _d(kta) if want_mu else None,
                                             _d(var) if want_var else None), "query_batch")
        return kta, var

    # -- the joint posterior over a point batch (include/gpe_joint.h; HIP library only)
    def joint_query(self, Xq, jitter=0.0, want_mu=True, want_cov=True):
        """(kta (M x P), cov (M x M, full symmetric, jitter on the diagonal)); either may be None."""
        Xq = _c(Xq).reshape(-1, self.D)
        M = Xq.shape[0]
        kta = np.zeros((M, self.P), order="F") if want_mu else None
        cov = np.zeros((M, M), order="F") if want_cov else None
        self._chk(self.lib.fn("joint_query")(self._h, _d(Xq), M, float(jitter), _d(kta) if want_mu else None,
                                             _d(cov) if want_cov else None, max(M, 1)), "joint_query")
        return kta, cov

    def joint_draws(self, Xq, Z, jitter, mean_q=None, want_F=True, want_argmax=True):
        """Z: (M, S, P) standard normals.  Returns (status, F (M, S, P) or None, argmax (S, P) or None, fmax (S, P) or None);
        status > 0 is the first non-positive pivot of cov + jitter I (the other results are then undefined)."""
        Xq = _c(Xq).reshape(-1, self.D)
        M = Xq.shape[0]
        Z = np.asarray(Z, dtype=np.float64)
        if Z.ndim == 2:
            Z = Z[:, :, None]
        assert Z.shape[0] == M and Z.shape[2] == self.P
        S = Z.shape[1]
        Zf = _c(Z.reshape(M, S * self.P, order="F"), "F")
        mq = None
        if mean_q is not None:
            mq = _c(np.asarray(mean_q, dtype=np.float64).reshape(M, self.P), "F")
        F = np.zeros((M, S * self.P), order="F") if want_F else None
        am = np.zeros(S * self.P, dtype=np.int64) if want_argmax else None
        fm = np.zeros(S * self.P) if want_argmax else None
        rc = self._chk(self.lib.fn("joint_draws")(self._h, _d(Xq), M, float(jitter), _d(mq) if mq is not None else None, _d(Zf), S,
                                                  _d(F) if want_F else None,
                                                  am.ctypes.data_as(C.POINTER(_i64)) if want_argmax else None,
                                                  _d(fm) if want_argmax else None), "joint_draws")
        return (rc, F.reshape(M, S, self.P, order="F") if want_F else None,
                am.reshape(S, self.P, order="F") if want_argmax else None,
                fm.reshape(S, self.P, order="F") if want_argmax else None)

    def joint_phase_ms(self):
        """{Z, cov, chol, draws} of the last joint call in ms (set_profiling(True) first)."""
        ms = np.zeros(4)
        self._chk(self.lib.fn("joint_phase_ms")(self._h, _d(ms)), "joint_phase_ms")
        return dict(zip(("Z", "cov", "chol", "draws"), ms.tolist()))

    def joint_max_points(self) -> int:
        n = _i64()
        self._chk(self.lib.fn("joint_max_points")(self._h, C.byref(n)), "joint_max_points")
        return n.value

    # -- greedy batch selection with hallucinated observations (include/gpe_batch_select.h; HIP library only)
    def select_batch(self, Xq, q, rule, param, mu_q=None, var_add=0.0, obs_noise=0.0, distinct=True, want=("idx", "score", "var", "W"),
                     check=True):
        """q greedy picks among the rows of Xq.  rule: SELECT_UCB (param = beta), SELECT_EI (param = f+ + jitter) or SELECT_VAR.
        Returns (status, idx (q), score (q), var (M), W (M, q)), None for what `want` leaves out; status > 0 is the 1-based round
        whose pivot was not positive (rounds before it are valid).  check=False hands a negative GPE_ERR_* back instead of raising."""
        Xq = _c(Xq).reshape(-1, self.D)
        M, q = Xq.shape[0], int(q)
        mq = _c(np.asarray(mu_q, dtype=np.float64).reshape(M)) if mu_q is not None else None
        idx = np.zeros(max(q, 0), dtype=np.int64) if "idx" in want else None
        score = np.zeros(max(q, 0)) if "score" in want else None
        var = np.zeros(M) if "var" in want else None
        W = np.zeros((M, max(q, 0)), order="F") if "W" in want else None
        rc = self.lib.fn("select_batch")(self._h, _d(Xq), M, q, int(rule), float(param), _d(mq) if mq is not None else None, float(var_add),
                                         float(obs_noise), int(bool(distinct)),
                                         idx.ctypes.data_as(C.POINTER(_i64)) if idx is not None else None,
                                         _d(score) if score is not None else None, _d(var) if var is not None else None,
                                         _d(W) if W is not None else None, max(M, 1))
        if check:
            self._chk(rc, "select_batch")
        return rc, idx, score, var, W

    def select_phase_ms(self):
        """{setup, rounds, readback} of the last select_batch call in ms (set_profiling(True) first)."""
        ms = np.zeros(3)
        self._chk(self.lib.fn("select_phase_ms")(self._h, _d(ms)), "select_phase_ms")
        return dict(zip(("setup", "rounds", "readback"), ms.tolist()))

    # -- the knowledge gradient over a finite alternative set (include/gpe_kg.h; HIP library only)
    def kg_batch(self, Xa, Xc, obs_noise, with_self=False, mu_a=None, mu_c=None, want=("kg", "var", "cov"), check=True):
        """The knowledge gradient of every row of Xc over the alternatives Xa.  mu_a / mu_c: complete means, or None for
        k(X, .)^T alpha_0.  Returns (status, kg (M), var_c (M), cov (A, M)), None for what `want` leaves out.  check=False hands a
        negative GPE_ERR_* back instead of raising."""
        Xa = _c(Xa).reshape(-1, self.D)
        Xc = _c(Xc).reshape(-1, self.D)
        A, M = Xa.shape[0], Xc.shape[0]
        ma = _c(np.asarray(mu_a, dtype=np.float64).reshape(A)) if mu_a is not None else None
        mc = _c(np.asarray(mu_c, dtype=np.float64).reshape(M)) if mu_c is not None else None
        kg = np.zeros(M) if "kg" in want else None
        var = np.zeros(M) if "var" in want else None
        cov = np.zeros((A, M), order="F") if "cov" in want else None
        rc = self.lib.fn("kg_batch")(self._h, _d(Xa), A, _d(ma) if ma is not None else None, _d(Xc), M, _d(mc) if mc is not None else None,
                                     float(obs_noise), int(bool(with_self)), _d(kg) if kg is not None else None,
                                     _d(var) if var is not None else None, _d(cov) if cov is not None else None, max(A, 1))
        if check:
            self._chk(rc, "kg_batch")
        return rc, kg, var, cov

    def kg_envelope(self, a, B, ldb=None, want_nseg=True, check=True):
        """h(a, B[:, m]) for every column of B (A x M, slopes already scaled) on host-supplied beliefs; any handle serves.  ldb:
        hand B over with that leading dimension (>= A; a copy is made).  Returns (status, kg (M), nseg (M) or None)."""
        a = _c(np.asarray(a, dtype=np.float64).reshape(-1))
        B = np.asarray(B, dtype=np.float64)
        B = B.reshape(B.shape[0], -1)
        A, M = B.shape
        assert a.shape[0] == A
        ld = A if ldb is None else int(ldb)
        Bf = np.zeros((max(ld, A), M), order="F")
        Bf[:A] = B
        kg = np.zeros(M)
        nseg = np.zeros(M, dtype=np.int32) if want_nseg else None
        rc = self.lib.fn("kg_envelope")(self._h, _d(a), A, _d(Bf), ld, M, _d(kg),
                                        nseg.ctypes.data_as(C.POINTER(C.c_int32)) if want_nseg else None)
        if check:
            self._chk(rc, "kg_envelope")
        return rc, kg, nseg

    def kg_phase_ms(self):
        """{alternatives, candidates, envelope, readback} of the last kg_batch call in ms (set_profiling(True) first)."""
        ms = np.zeros(4)
        self._chk(self.lib.fn("kg_phase_ms")(self._h, _d(ms)), "kg_phase_ms")
        return dict(zip(("alternatives", "candidates", "envelope", "readback"), ms.tolist()))

    # -- the two-objective expected hypervolume improvement (include/gpe_ehvi.h; HIP library only)
    def ehvi2_values(self, front, ref, mu1, s1, mu2, s2, want_partials=True, check=True):
        """The strip sums alone on host-supplied beliefs (s: standard deviations) over a prepared front (n x 2; ehvi2_front makes
        one); any handle serves.  Returns (status, ehvi (M), partials (M, 4: d/d mu1, s1, mu2, s2) or None).  check=False hands a
        negative GPE_ERR_* back instead of raising."""
        F, r = _front_args(front, ref)
        b = [_c(np.asarray(v, dtype=np.float64).reshape(-1)) for v in (mu1, s1, mu2, s2)]
        M = b[0].shape[0]
        assert all(v.shape[0] == M for v in b)
        ehvi = np.zeros(M)
        part = np.zeros((M, 4), order="F") if want_partials else None
        rc = self.lib.fn("ehvi2_values")(self._h, _d(F), F.shape[0], _d(r), _d(b[0]), _d(b[1]), _d(b[2]), _d(b[3]), M, _d(ehvi),
                                         _d(part) if want_partials else None)
        if check:
            self._chk(rc, "ehvi2_values")
        return rc, ehvi, part

    def ehvi2_batch(self, Xc, front, ref, out1=0, out2=1, mean_add=None, var_add=0.0, want=("ehvi", "partials", "mu", "var"), check=True):
        """The expected hypervolume improvement of every row of Xc under the handle's outputs (out1, out2), which share sigma.
        mean_add: (M, 2) added to k^T alpha, or None; var_add: added to the clamped variance (0: the latent function).  Returns
        (status, ehvi (M), partials (M, 4), mu (M, 2), var (M)), None for what `want` leaves out."""
        Xc = _c(Xc).reshape(-1, self.D)
        M = Xc.shape[0]
        F, r = _front_args(front, ref)
        ma = _c(np.asarray(mean_add, dtype=np.float64).reshape(M, 2), "F") if mean_add is not None else None
        out = {"ehvi": np.zeros(M), "partials": np.zeros((M, 4), order="F"), "mu": np.zeros((M, 2), order="F"), "var": np.zeros(M)}
        ptr = [_d(out[k]) if k in want else None for k in ("ehvi", "partials", "mu", "var")]
        rc = self.lib.fn("ehvi2_batch")(self._h, int(out1), int(out2), _d(Xc), M, _d(ma) if ma is not None else None, float(var_add), _d(F),
                                        F.shape[0], _d(r), *ptr)
        if check:
            self._chk(rc, "ehvi2_batch")
        return (rc,) + tuple(out[k] if k in want else None for k in ("ehvi", "partials", "mu", "var"))

    def ehvi_phase_ms(self):
        """{solves, kernel, readback} of the last ehvi2_batch call in ms (set_profiling(True) first)."""
        ms = np.zeros(3)
        self._chk(self.lib.fn("ehvi_phase_ms")(self._h, _d(ms)), "ehvi_phase_ms")
        return dict(zip(("solves", "kernel", "readback"), ms.tolist()))

    # -- the three-objective expected hypervolume improvement (include/gpe_ehvi3.h; HIP library only)
    def ehvi3_values(self, front, ref, mu, s, want_partials=True, check=True):
        """The box sums alone on host-supplied beliefs mu, s (M, 3; s: standard deviations) over a prepared front (n x 3;
        ehvi3_front makes one); any handle serves.  Returns (status, ehvi (M), partials (M, 6: d/d mu1, s1, mu2, s2, mu3, s3) or
        None).  check=False hands a negative GPE_ERR_* back instead of raising."""
        F, r = _front3_args(front, ref)
        mu, s = (_c(np.asarray(v, dtype=np.float64).reshape(-1, 3), "F") for v in (mu, s))
        M = mu.shape[0]
        assert s.shape[0] == M
        ehvi = np.zeros(M)
        part = np.zeros((M, 6), order="F") if want_partials else None
        rc = self.lib.fn("ehvi3_values")(self._h, _d(F), F.shape[0], _d(r), _d(mu), _d(s), M, _d(ehvi), _d(part) if want_partials else None)
        if check:
            self._chk(rc, "ehvi3_values")
        return rc, ehvi, part

    def ehvi3_batch(self, Xc, front, ref, outs=(0, 1, 2), mean_add=None, var_add=0.0, want=("ehvi", "partials", "mu", "var"), check=True):
        """The expected hypervolume improvement of every row of Xc under the handle's three outputs `outs`, which share sigma.
        mean_add: (M, 3) added to k^T alpha, or None; var_add: added to the clamped variance (0: the latent function).  Returns
        (status, ehvi (M), partials (M, 6), mu (M, 3), var (M)), None for what `want` leaves out."""
        Xc = _c(Xc).reshape(-1, self.D)
        M = Xc.shape[0]
        F, r = _front3_args(front, ref)
        o = (C.c_int * 3)(*[int(v) for v in outs])
        ma = _c(np.asarray(mean_add, dtype=np.float64).reshape(M, 3), "F") if mean_add is not None else None
        out = {"ehvi": np.zeros(M), "partials": np.zeros((M, 6), order="F"), "mu": np.zeros((M, 3), order="F"), "var": np.zeros(M)}
        ptr = [_d(out[k]) if k in want else None for k in ("ehvi", "partials", "mu", "var")]
        rc = self.lib.fn("ehvi3_batch")(self._h, o, _d(Xc), M, _d(ma) if ma is not None else None, float(var_add), _d(F), F.shape[0], _d(r),
                                        *ptr)
        if check:
            self._chk(rc, "ehvi3_batch")
        return (rc,) + tuple(out[k] if k in want else None for k in ("ehvi", "partials", "mu", "var"))

    def ehvi3_phase_ms(self):
        """{solves, kernel, readback} of the last ehvi3_batch call in ms (set_profiling(True) first)."""
        ms = np.zeros(3)
        self._chk(self.lib.fn("ehvi3_phase_ms")(self._h, _d(ms)), "ehvi3_phase_ms")
        return dict(zip(("solves", "kernel", "readback"), ms.tolist()))

    # -- constrained expected improvement in the log domain (include/gpe_cei.h; HIP library only)
    def logcei_values(self, thr, mu_c, s_c, mu0=None, s0=None, f_best=0.0, xi=0.0, with_ei=True, want=("terms", "partials"), check=True):
        """The kernel alone on host-supplied beliefs (s: standard deviations): constraints k feasible when c_k >= thr[k], beliefs
        mu_c, s_c (M, C); the objective's belief mu0, s0 (M) against the incumbent f_best (not read when with_ei is false).  Any
        handle serves.  Returns (status, logcei (M), terms (M, 1 + C) or None, partials (M, 2 + 2 C) or None).  check=False hands a
        negative GPE_ERR_* back instead of raising."""
        t = _c(np.asarray(thr, dtype=np.float64).reshape(-1))
        Cn = t.shape[0]
        if mu0 is not None:
            m0, sd0 = (_c(np.asarray(v, dtype=np.float64).reshape(-1)) for v in (mu0, s0))
            M = m0.shape[0]
            assert sd0.shape[0] == M
        else:
            m0 = sd0 = None
            M = np.asarray(mu_c).reshape(-1, max(Cn, 1)).shape[0] if Cn else 0
        mc, sc = (_c(np.asarray(v, dtype=np.float64).reshape(M, Cn), "F") for v in (mu_c, s_c))
        val = np.zeros(M)
        terms = np.zeros((M, 1 + Cn), order="F") if "terms" in want else None
        part = np.zeros((M, 2 + 2 * Cn), order="F") if "partials" in want else None
        opt = lambda a: _d(a) if a is not None and a.size else None
        rc = self.lib.fn("logcei_values")(self._h, int(bool(with_ei)), float(f_best), float(xi), Cn, opt(t), opt(m0), opt(sd0), opt(mc), opt(sc),
                                          M, _d(val), opt(terms), opt(part))
        if check:
            self._chk(rc, "logcei_values")
        return rc, val, terms, part

    def logcei_batch(self, Xc, thr, con_outs, out0=0, f_best=0.0, xi=0.0, with_ei=True, mean_add=None, var_add=0.0,
                     want=("logcei", "terms", "partials", "mu", "var"), check=True):
        """The log constrained expected improvement of every row of Xc under the handle's output out0 (the objective) and outputs
        con_outs (the constraints, thresholds thr), which share sigma.  mean_add: (M, 1 + C) added to k^T alpha, or None; var_add:
        added to the clamped variance (0: the latent function).  Returns (status, logcei (M), terms (M, 1 + C), partials
        (M, 2 + 2 C), mu (M, 1 + C), var (M)), None for what `want` leaves out."""
        Xc = _c(Xc).reshape(-1, self.D)
        M = Xc.shape[0]
        t = _c(np.asarray(thr, dtype=np.float64).reshape(-1))
        Cn = t.shape[0]
        outs = np.ascontiguousarray(np.asarray(con_outs, dtype=np.int32).reshape(-1))
        assert outs.shape[0] == Cn
        ma = _c(np.asarray(mean_add, dtype=np.float64).reshape(M, 1 + Cn), "F") if mean_add is not None else None
        names = ("logcei", "terms", "partials", "mu", "var")
        out = {"logcei": np.zeros(M), "terms": np.zeros((M, 1 + Cn), order="F"), "partials": np.zeros((M, 2 + 2 * Cn), order="F"),
               "mu": np.zeros((M, 1 + Cn), order="F"), "var": np.zeros(M)}
        ptr = [_d(out[k]) if k in want else None for k in names]
        rc = self.lib.fn("logcei_batch")(self._h, int(bool(with_ei)), int(out0), float(f_best), float(xi), Cn,
                                         outs.ctypes.data_as(C.POINTER(C.c_int)) if Cn else None, _d(t) if Cn else None, _d(Xc), M,
                                         _d(ma) if ma is not None else None, float(var_add), *ptr)
        if check:
            self._chk(rc, "logcei_batch")
        return (rc,) + tuple(out[k] if k in want else None for k in names)

    def cei_phase_ms(self):
        """{solves, kernel, readback} of the last logcei_batch call in ms (set_profiling(True) first)."""
        ms = np.zeros(3)
        self._chk(self.lib.fn("cei_phase_ms")(self._h, _d(ms)), "cei_phase_ms")
        return dict(zip(("solves", "kernel", "readback"), ms.tolist()))

    # -- max-value entropy search in the log domain (include/gpe_mes.h; HIP library only)
    def mes_values(self, ystar, mu, s, want=("terms", "partials"), check=True):
        """The kernel alone on host-supplied beliefs (s: standard deviations): ystar (K, J) sampled maxima, mu and s (M, J).  Any
        handle serves.  Returns (status, logmes (M), terms (M, J) or None, partials (M, 2 J) or None: d/d mu_j, then d/d s_j).
        check=False hands a negative GPE_ERR_* back instead of raising."""
        ys = np.asarray(ystar, dtype=np.float64)
        ys = _c(ys.reshape(ys.shape[0], -1), "F")
        K, J = ys.shape
        m_, s_ = (_c(np.asarray(v, dtype=np.float64).reshape(-1, J), "F") for v in (mu, s))
        M = m_.shape[0]
        assert s_.shape[0] == M
        val = np.zeros(M)
        terms = np.zeros((M, J), order="F") if "terms" in want else None
        part = np.zeros((M, 2 * J), order="F") if "partials" in want else None
        opt = lambda a: _d(a) if a is not None and a.size else None
        rc = self.lib.fn("mes_values")(self._h, J, K, _d(ys), opt(m_), opt(s_), M, opt(val), opt(terms), opt(part))
        if check:
            self._chk(rc, "mes_values")
        return rc, val, terms, part

    def mes_batch(self, Xc, ystar, outs=None, mean_add=None, var_add=0.0, want=("logmes", "terms", "partials", "mu", "var"), check=True):
        """The log max-value entropy search of every row of Xc under the handle's outputs `outs` (default: all), which share sigma,
        against the sampled maxima ystar (K, J).  mean_add: (M, J) added to k^T alpha, or None; var_add: added to the clamped
        variance (0: the latent function).  Returns (status, logmes (M), terms (M, J), partials (M, 2 J), mu (M, J), var (M)), None
        for what `want` leaves out."""
        Xc = _c(Xc).reshape(-1, self.D)
        M = Xc.shape[0]
        ys = np.asarray(ystar, dtype=np.float64)
        ys = _c(ys.reshape(ys.shape[0], -1), "F")
        K, J = ys.shape
        o = np.ascontiguousarray(np.asarray(range(J) if outs is None else outs, dtype=np.int32).reshape(-1))
        assert o.shape[0] == J
        ma = _c(np.asarray(mean_add, dtype=np.float64).reshape(M, J), "F") if mean_add is not None else None
        names = ("logmes", "terms", "partials", "mu", "var")
        out = {"logmes": np.zeros(M), "terms": np.zeros((M, J), order="F"), "partials": np.zeros((M, 2 * J), order="F"),
               "mu": np.zeros((M, J), order="F"), "var": np.zeros(M)}
        ptr = [_d(out[k]) if k in want else None for k in names]
        rc = self.lib.fn("mes_batch")(self._h, J, o.ctypes.data_as(C.POINTER(C.c_int)), K, _d(ys), _d(Xc), M,
                                      _d(ma) if ma is not None else None, float(var_add), *ptr)
        if check:
            self._chk(rc, "mes_batch")
        return (rc,) + tuple(out[k] if k in want else None for k in names)

    def mes_phase_ms(self):
        """{solves, kernel, readback} of the last mes_batch call in ms (set_profiling(True) first)."""
        ms = np.zeros(3)
        self._chk(self.lib.fn("mes_phase_ms")(self._h, _d(ms)), "mes_phase_ms")
        return dict(zip(("solves", "kernel", "readback"), ms.tolist()))

    # -- noisy expected improvement in the log domain (include/gpe_nei.h; HIP library only)
    def lognei_values(self, fplus, cmean, csd, xi=0.0, want=("terms",), check=True):
        """The kernel alone on host-supplied conditional beliefs: fplus (S) the draws' incumbents, cmean (S, M) the mean at
        candidate m given draw s — any array whose columns are contiguous, what lies behind row S of a wider one is not read — and csd
        (M) standard deviations.  Any handle serves.  Returns (status, lognei (M), terms (S, M) or None).  check=False hands a negative
        GPE_ERR_* back instead of raising."""
        fp = _c(np.asarray(fplus, dtype=np.float64).reshape(-1))
        S = fp.shape[0]
        cm = np.asarray(cmean, dtype=np.float64)
        if cm.ndim != 2 or cm.strides[0] != 8 or (cm.shape[1] > 1 and cm.strides[1] % 8):
            cm = _c(cm.reshape(S, -1), "F")
        M = cm.shape[1]
        ldm = cm.strides[1] // 8 if M > 1 else max(cm.shape[0], 1)
        cm_ptr = C.cast(cm.ctypes.data, _dp) if cm.size else None
        sd = _c(np.asarray(csd, dtype=np.float64).reshape(-1))
        assert sd.shape[0] == M
        val = np.zeros(M)
        terms = np.zeros((S, M), order="F") if "terms" in want else None
        opt = lambda a: _d(a) if a is not None and a.size else None
        rc = self.lib.fn("lognei_values")(self._h, S, opt(fp), float(xi), cm_ptr, ldm, opt(sd), M, opt(val), opt(terms))
        if check:
            self._chk(rc, "lognei_values")
        return rc, val, terms

    def lognei_batch(self, Xc, Xb, Z, out=0, jitter=0.0, xi=0.0, mean_b=None, mean_add=None,
                     want=("lognei", "fplus", "mu", "var", "cvar", "cmean"), check=True):
        """The log noisy expected improvement of every row of Xc under the handle's output `out`: baseline points Xb (B, D), standard
        normals Z (B, S) of the caller's, jitter added to the baseline's covariance (no hidden default).  mean_b (B), mean_add (M):
        the mean functor's values, or None.  Returns (status, lognei (M), fplus (S), mu (M), var (M), cvar (M), cmean (S, M)), None
        for what `want` leaves out; status > 0: the 1-based first non-positive pivot of the baseline's covariance, nothing written."""
        Xc = _c(Xc).reshape(-1, self.D)
        Xb = _c(Xb).reshape(-1, self.D)
        M, B = Xc.shape[0], Xb.shape[0]
        Zn = np.asarray(Z, dtype=np.float64)
        Zn = _c(Zn.reshape(B, -1), "F")
        S = Zn.shape[1]
        mb = _c(np.asarray(mean_b, dtype=np.float64).reshape(B)) if mean_b is not None else None
        ma = _c(np.asarray(mean_add, dtype=np.float64).reshape(M)) if mean_add is not None else None
        names = ("lognei", "fplus", "mu", "var", "cvar", "cmean")
        res = {"lognei": np.zeros(M), "fplus": np.zeros(S), "mu": np.zeros(M), "var": np.zeros(M), "cvar": np.zeros(M),
               "cmean": np.zeros((S, M), order="F")}
        ptr = [_d(res[k]) if k in want else None for k in names]
        rc = self.lib.fn("lognei_batch")(self._h, int(out), _d(Xb), B, _d(mb) if mb is not None else None, float(jitter), _d(Zn), S,
                                         float(xi), _d(Xc), M, _d(ma) if ma is not None else None, *ptr, max(S, 1))
        if check:
            self._chk(rc, "lognei_batch")
        return (rc,) + tuple(res[k] if k in want else None for k in names)

    def nei_phase_ms(self):
        """{baseline, factor_draws, solves, conditioning, kernel} of the last lognei_batch call in ms (set_profiling(True) first)."""
        ms = np.zeros(5)
        self._chk(self.lib.fn("nei_phase_ms")(self._h, _d(ms)), "nei_phase_ms")
        return dict(zip(("baseline", "factor_draws", "solves", "conditioning", "kernel"), ms.tolist()))

    # -- the posterior with its gradient in the query point (include/gpe_query_grad.h; HIP library only)
    def query_batch_grad(self, Xq, want=("kta", "var", "dkta", "dvar")):
        """(kta (M, P), var (M), dkta (M, D, P), dvar (M, D)), None for what `want` leaves out: dkta[m, d, p] = d(k^T alpha_p)/dv_d,
        dvar[m, d] = d var / dv_d at point m.  No mean functor, no clamp, no + noise."""
        Xq = _c(Xq).reshape(-1, self.D)
        M, D, P = Xq.shape[0], self.D, self.P
        out = {"kta": np.zeros((M, P), order="F"), "var": np.zeros(M), "dkta": np.zeros((M, D * P), order="F"),
               "dvar": np.zeros((M, D), order="F")}
        for k in list(out):
            if k not in want:
                out[k] = None
        ptr = [_d(out[k]) if out[k] is not None else None for k in ("kta", "var", "dkta", "dvar")]
        self._chk(self.lib.fn("query_batch_grad")(self._h, _d(Xq), M, *ptr), "query_batch_grad")
        if out["dkta"] is not None:
            out["dkta"] = out["dkta"].reshape(M, D, P, order="F")
        return out["kta"], out["var"], out["dkta"], out["dvar"]

    def query_grad_phase_ms(self):
        """{forward, backward, grad} of the last query_batch_grad call in ms (set_profiling(True) first)."""
        ms = np.zeros(3)
        self._chk(self.lib.fn("query_grad_phase_ms")(self._h, _d(ms)), "query_grad_phase_ms")
        return dict(zip(("forward", "backward", "grad"), ms.tolist()))

    # -- posterior draws as functions of the query point (include/gpe_pathwise.h; HIP library only)
    def paths(self, R, S, Omega0, phase, W, E=None) -> "Paths":
        """A set of S pathwise draws per output on R Fourier features.  Omega0: (R, Dw) unit-scale frequencies, phase: (R),
        W: (R, S, P) and E: (N, S, P) standard normals (E = None: zeros)."""
        return Paths(self, R, S, Omega0, phase, W, E)

    # -- accessors
    def nb_samples(self) -> int:
        n = _i64()
        self._chk(self.lib.fn("nb_samples")(self._h, C.byref(n)), "nb_samples")
        return n.value

    def _get_mat(self, name):
        n = self.N
        A = np.zeros((n, n), order="F")
        self._chk(self.lib.fn(name)(self._h, _d(A), n), name)
        return A

    def get_L(self):
        return self._get_mat("get_L")

    def get_K(self):
        return self._get_mat("get_K")

    def get_Kinv(self):
        return self._get_mat("get_Kinv")

    def set_L(self, L):
        L = _c(L, "F")
        self._chk(self.lib.fn("set_L")(self._h, _d(L), L.shape[0]), "set_L")

    def get_alpha(self):
        a = np.zeros((self.N, self.P), order="F")
        self._chk(self.lib.fn("get_alpha")(self._h, _d(a)), "get_alpha")
        return a

    def set_alpha(self, a):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 1:
            a = a[:, None]
        a = _c(a, "F")
        self._chk(self.lib.fn("set_alpha")(self._h, _d(a)), "set_alpha")

    def synchronize(self):
        self._chk(self.lib.fn("synchronize")(self._h), "synchronize")

    # -- instrumentation (HIP library only)
    def get_stream(self) -> int:
        s = _vp()
        self._chk(self.lib.fn("get_stream")(self._h, C.byref(s)), "get_stream")
        return s.value or 0

    def set_profiling(self, on: bool):
        self._chk(self.lib.fn("set_profiling")(self._h, int(on)), "set_profiling")

    def reset_phase_ms(self):
        self._chk(self.lib.fn("reset_phase_ms")(self._h), "reset_phase_ms")

    def get_phase_ms(self):
        ms = np.zeros(PH_COUNT)
        fl = np.zeros(PH_COUNT)
        ln = (C.c_int64 * PH_COUNT)()
        self._chk(self.lib.fn("get_phase_ms")(self._h, _d(ms), ln, _d(fl), PH_COUNT), "get_phase_ms")
        return {PHASE_NAMES[i]: {"ms": float(ms[i]), "launches": int(ln[i]), "flops": float(fl[i])}
                for i in range(PH_COUNT)}


class Paths:
    """A path set behind include/gpe_pathwise.h: a snapshot of the model it was made from, independent of the handle afterwards."""

    def __init__(self, handle: Handle, R, S, Omega0, phase, W, E=None):
        self.lib = handle.lib
        P = handle.P
        Om = _c(Omega0).reshape(R, -1)
        ph = _c(phase).reshape(R)
        Wf = _c(np.asarray(W, dtype=np.float64).reshape(R, S * P, order="F"), "F")
        Ef = None if E is None else _c(np.asarray(E, dtype=np.float64).reshape(-1, S * P, order="F"), "F")
        ps = _vp()
        rc = self.lib.fn("paths_create")(handle._h, int(R), int(S), _d(Om), _d(ph), _d(Wf), _d(Ef) if Ef is not None else None, C.byref(ps))
        self._ps = None
        handle._chk(rc, "paths_create")
        self._ps = ps
        n, d, p, r, s = _i64(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.fn("paths_info")(ps, C.byref(n), C.byref(d), C.byref(p), C.byref(r), C.byref(s)), "paths_info")
        self.N, self.D, self.P, self.R, self.S = n.value, d.value, p.value, r.value, s.value

    def _chk(self, rc, what):
        if rc < 0:
            raise EngineError(f"gpe_{what} failed: status {rc}")
        return rc

    def close(self):
        if getattr(self, "_ps", None):
            self.lib.fn("paths_destroy")(self._ps)
            self._ps = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _points(self, V, mean_q):
        V = _c(V).reshape(-1, self.D)
        mq = None if mean_q is None else _c(np.asarray(mean_q, dtype=np.float64).reshape(V.shape[0], self.P), "F")
        return V, mq

    def eval(self, V, want=("F", "dF"), mean_q=None):
        """(F (T, S, P), dF (T, D, S, P)), None for what `want` leaves out: dF[t, d, s, p] = d f_sp / d x_d at point t (without the
        mean functor's derivative); mean_q (T, P): m(v), added to F."""
        V, mq = self._points(V, mean_q)
        T, D, S, P = V.shape[0], self.D, self.S, self.P
        F = np.zeros((T, S * P), order="F") if "F" in want else None
        dF = np.zeros((T, D * S * P), order="F") if "dF" in want else None
        self._chk(self.lib.fn("paths_eval")(self._ps, _d(V), T, _d(mq) if mq is not None else None, _d(F) if F is not None else None,
                                            _d(dF) if dF is not None else None), "paths_eval")
        return (F.reshape(T, S, P, order="F") if F is not None else None, dF.reshape(T, D, S, P, order="F") if dF is not None else None)

    def argmax(self, V, mean_q=None):
        """(argmax (S, P), fmax (S, P)) of every draw over the points; the lowest index on exact ties"""
        V, mq = self._points(V, mean_q)
        am, fm = np.zeros(self.S * self.P, dtype=np.int64), np.zeros(self.S * self.P)
        self._chk(self.lib.fn("paths_argmax")(self._ps, _d(V), V.shape[0], _d(mq) if mq is not None else None,
                                              am.ctypes.data_as(C.POINTER(_i64)), _d(fm)), "paths_argmax")
        return am.reshape(self.S, self.P, order="F"), fm.reshape(self.S, self.P, order="F")

    def phase_ms(self):
        """{create_features, create_solve, eval_features, eval_data} in ms"""
        ms = np.zeros(4)
        self._chk(self.lib.fn("paths_phase_ms")(self._ps, _d(ms)), "paths_phase_ms")
        return dict(zip(("create_features", "create_solve", "eval_features", "eval_data"), ms.tolist()))


def sparsify(lib, X, max_points, device_id=0):
    """SparsifiedGP::_sparsify (sparsified_gp.hpp:157-183): indices of the samples that survive."""
    X = _c(X)
    N, D = X.shape
    keep = np.zeros(N, dtype=np.int64)
    n = _i64(0)
    rc = lib.fn("sparsify")(int(device_id), _d(X), N, D, int(max_points), keep.ctypes.data_as(C.POINTER(_i64)),
                            C.byref(n))
    if rc != 0:
        raise EngineError(f"sparsify failed with status {rc}")
    return keep[: n.value].copy()


def batch_compute(handles):
    lib = handles[0].lib
    arr = (_vp * len(handles))(*[h._h for h in handles])
    st = (C.c_int * len(handles))()
    rc = lib.fn("batch_compute")(arr, len(handles), st)
    if rc < 0:
        raise EngineError(f"batch_compute failed: {rc}")
    return list(st)


def batch_log_lik(handles):
    lib = handles[0].lib
    arr = (_vp * len(handles))(*[h._h for h in handles])
    out = np.zeros(len(handles))
    rc = lib.fn("batch_log_lik")(arr, len(handles), _d(out))
    if rc < 0:
        raise EngineError(f"batch_log_lik failed: {rc}")
    return out


def batch_hp_objective(handles, kind, thetas, noises, optimize_noise=False, want_grad=True):
    """gpe_batch_hp_objective: thetas (G x n_theta), noises (G,) -> (lik (G,), grad (G x n_grad) or None, status list)."""
    lib = handles[0].lib
    G = len(handles)
    kind = KERNEL_NAMES.get(kind, kind)
    th = _c(np.asarray(thetas, dtype=np.float64).reshape(G, -1))
    nz = _c(np.broadcast_to(np.asarray(noises, dtype=np.float64), (G,)).copy())
    n_theta = th.shape[1]
    n_grad = n_theta + (1 if optimize_noise else 0)
    arr = (_vp * G)(*[h._h for h in handles])
    lik = np.zeros(G)
    grad = np.zeros((G, n_grad))
    st = (C.c_int * G)()
    rc = lib.fn("batch_hp_objective")(arr, G, int(kind), _d(th), n_theta, _d(nz), int(optimize_noise), int(want_grad), _d(lik),
                                      _d(grad) if want_grad else None, st)
    if rc < 0:
        raise EngineError(f"batch_hp_objective failed: {rc}")
    for h in handles:
        h.n_theta = n_theta
        h.kind = kind
    return lik, (grad if want_grad else None), list(st)


def device_count(lib) -> int:
    n = C.c_int()
    rc = lib.fn("device_count")(C.byref(n))
    if rc < 0:
        raise EngineError(f"device_count failed: {rc}")
    return n.value


def append_max_chunk(lib) -> int:
    """gpe_append_max_chunk: rows the device tail of gpe_add_samples factorises at once."""
    return int(lib.fn("append_max_chunk")())


def remove_max_vectors(lib) -> int:
    """gpe_remove_max_vectors: update vectors one pass of gpe_remove_samples carries."""
    return int(lib.fn("remove_max_vectors")())


def debug_remove_plan(lib, n, i0, q, tail_only=False):
    """gpe_debug_remove_plan: (path AUTO takes: 1 update / 2 recompute, passes, launches on the factor, scratch doubles) of a
    call that removes q indices, the smallest i0, from a model of n samples.  Raises EngineError on a bad argument."""
    out = (_i64 * 4)()
    rc = lib.fn("debug_remove_plan")(int(n), int(i0), int(q), int(bool(tail_only)), out)
    if rc != 0:
        raise EngineError(f"debug_remove_plan: bad argument ({n}, {i0}, {q}, {tail_only}): status {rc}")
    return tuple(int(v) for v in out)


def debug_live_buffers(lib):
    """gpe_debug_live_buffers: (count, bytes) of the device buffers this process's handles own right now."""
    n, b = _i64(0), _i64(0)
    if lib.fn("debug_live_buffers")(C.byref(n), C.byref(b)) != 0:
        raise EngineError("debug_live_buffers failed")
    return n.value, b.value


def debug_append_slices(lib, n):
    """gpe_debug_append_slices: (kslice, nslices, slices_cap, scratch_doubles) of the append tail for a factor of order n."""
    ks, sd, ns, cap = _i64(), _i64(), C.c_int(), C.c_int()
    if lib.fn("debug_append_slices")(int(n), C.byref(ks), C.byref(ns), C.byref(cap), C.byref(sd)) != 0:
        raise EngineError(f"debug_append_slices: bad argument {n}")
    return ks.value, ns.value, cap.value, sd.value


def debug_cov_plan(lib, M, N, cus):
    """gpe_debug_cov_plan: the (tile i, tile j, k0, k1, partial slot) rows of the joint covariance's launch, as an int64 array."""
    n = lib.fn("debug_cov_plan")(int(M), int(N), int(cus), None, 0)
    if n < 0:
        raise EngineError(f"debug_cov_plan: bad arguments ({M}, {N}, {cus})")
    out = np.zeros((n, 5), dtype=np.int64)
    lib.fn("debug_cov_plan")(int(M), int(N), int(cus), out.ctypes.data_as(C.POINTER(_i64)), n)
    return out


def debug_select_plan(lib, M, N, cus):
    """gpe_debug_select_plan: the (m0, m1, k0, k1, partial slot) rows of one round's column product, as an int64 array."""
    n = lib.fn("debug_select_plan")(int(M), int(N), int(cus), None, 0)
    if n < 0:
        raise EngineError(f"debug_select_plan: bad arguments ({M}, {N}, {cus})")
    out = np.zeros((n, 5), dtype=np.int64)
    lib.fn("debug_select_plan")(int(M), int(N), int(cus), out.ctypes.data_as(C.POINTER(_i64)), n)
    return out


def debug_gram_plan(lib, M, N, chunk=0, cus=256):
    """gpe_debug_gram_plan: the (tile i, tile j, k0, k1, slot) rows of the sparse GP's weighted Gram, as an int64 array
    (chunk <= 0: the default chunk for M)."""
    n = lib.fn("debug_gram_plan")(int(M), int(N), int(chunk), int(cus), None, 0)
    if n < 0:
        raise EngineError(f"debug_gram_plan: bad arguments ({M}, {N}, {chunk}, {cus})")
    out = np.zeros((n, 5), dtype=np.int64)
    lib.fn("debug_gram_plan")(int(M), int(N), int(chunk), int(cus), out.ctypes.data_as(C.POINTER(_i64)), n)
    return out


class SparseHandle:
    """One sparse pseudo-input GP (SPGP / FITC) behind include/gpe_sparse.h (HIP library only).  Statuses come back as they are:
    0, the 1-based first non-positive pivot, or a negative GPE_ERR_* — ``check=True`` raises on the negative ones."""

    def __init__(self, lib: Lib, device: int = 0):
        self.lib = lib
        self.N = self.M = self.D = self.P = 0
        h = _vp()
        rc = lib.fn("sp_create")(device, C.byref(h))
        if rc < 0:
            raise EngineError(f"gpe_sp_create failed: status {rc}")
        self._h = h

    def _chk(self, rc, what, check=True):
        if rc < 0 and check:
            m = self.lib.fn("sp_last_error")(self._h)
            raise EngineError(f"gpe_sp_{what} failed: status {rc} {m.decode() if m else ''}")
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self.lib.fn("sp_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, X, obs_zm, check=True):
        X = _c(X)
        y = np.asarray(obs_zm, dtype=np.float64)
        if y.ndim == 1:
            y = y[:, None]
        y = _c(y, "F")
        rc = self._chk(self.lib.fn("sp_set_data")(self._h, _d(X), X.shape[0], X.shape[1], _d(y), y.shape[1]), "set_data", check)
        if rc == 0:
            self.N, self.D = X.shape
            self.P = y.shape[1]
        return rc

    def set_pseudo(self, Xb, check=True):
        Xb = _c(Xb)
        rc = self._chk(self.lib.fn("sp_set_pseudo")(self._h, _d(Xb), Xb.shape[0]), "set_pseudo", check)
        if rc == 0:
            self.M = Xb.shape[0]
        return rc

    def set_hparams(self, log_b, log_c, log_sig, jitter, check=True):
        b = _c(log_b)
        return self._chk(self.lib.fn("sp_set_hparams")(self._h, _d(b), float(log_c), float(log_sig), float(jitter)), "set_hparams", check)

    def compute(self, check=True) -> int:
        return self._chk(self.lib.fn("sp_compute")(self._h), "compute", check)

    def nlml(self):
        out = np.zeros(max(self.P, 1))
        self._chk(self.lib.fn("sp_nlml")(self._h, _d(out)), "nlml")
        return out

    def objective(self, log_b, log_c, log_sig, jitter):
        """(status, nlml per output): set_hparams + compute + nlml in one call."""
        b = _c(log_b)
        out = np.zeros(max(self.P, 1))
        rc = self._chk(self.lib.fn("sp_objective")(self._h, _d(b), float(log_c), float(log_sig), float(jitter), _d(out)), "objective")
        return rc, out

    def predict(self, Xt, want_mu=True, want_s2=True):
        """(mu (T x P) without the mean functor, s2 (T) without the '+ sig' and without a clamp); either may be None."""
        Xt = _c(Xt).reshape(-1, self.D)
        T = Xt.shape[0]
        mu = np.zeros((T, self.P), order="F") if want_mu else None
        s2 = np.zeros(T) if want_s2 else None
        self._chk(self.lib.fn("sp_predict")(self._h, _d(Xt), T, _d(mu) if want_mu else None, _d(s2) if want_s2 else None), "predict")
        return mu, s2

    def get_L(self):
        L = np.zeros((self.M, self.M), order="F")
        self._chk(self.lib.fn("sp_get_L")(self._h, _d(L), self.M), "get_L")
        return L

    def get_Lm(self):
        L = np.zeros((self.M, self.M), order="F")
        self._chk(self.lib.fn("sp_get_Lm")(self._h, _d(L), self.M), "get_Lm")
        return L

    def get_bet(self):
        b = np.zeros((self.M, self.P), order="F")
        self._chk(self.lib.fn("sp_get_bet")(self._h, _d(b)), "get_bet")
        return b

    def get_ep(self):
        e = np.zeros(self.N)
        self._chk(self.lib.fn("sp_get_ep")(self._h, _d(e)), "get_ep")
        return e

    def set_profiling(self, on: bool):
        self._chk(self.lib.fn("sp_set_profiling")(self._h, int(on)), "set_profiling")

    def phase_ms(self):
        """{kmn_v, ep, gram, factor, predict} in ms (set_profiling(True) first)."""
        ms = np.zeros(5)
        self._chk(self.lib.fn("sp_phase_ms")(self._h, _d(ms)), "phase_ms")
        return dict(zip(("kmn_v", "ep", "gram", "factor", "predict"), ms.tolist()))

    def grad(self, want_xb=True, check=True):
        """(status, d_xb (M x D, as the pseudo-inputs were given) or None, d_hp (D + 2: log b .., log c, log sig)): the gradient of
        sum_p nlml_p of the model as computed (include/gpe_sparse_grad.h)."""
        gx = np.zeros((self.M, self.D)) if want_xb else None
        gh = np.zeros(self.D + 2)
        rc = self._chk(self.lib.fn("sp_grad")(self._h, _d(gx) if want_xb else None, _d(gh)), "grad", check)
        return rc, gx, gh

    def objective_grad(self, Xb, log_b, log_c, log_sig, jitter, want_xb=True, check=True):
        """(status, nlml per output, d_xb or None, d_hp): set_pseudo (Xb, M x D with the handle's M, or None: keep) + set_hparams +
        compute + nlml + grad in one call.  A status other than 0 leaves the outputs as they were created: NaN."""
        b = _c(log_b)
        xb = None if Xb is None else _c(Xb).reshape(self.M, self.D)
        f = np.full(max(self.P, 1), np.nan)
        gx = np.full((self.M, self.D), np.nan) if want_xb else None
        gh = np.full(self.D + 2, np.nan)
        rc = self._chk(self.lib.fn("sp_objective_grad")(self._h, None if xb is None else _d(xb), _d(b), float(log_c), float(log_sig), float(jitter),
                                                        _d(f), _d(gx) if want_xb else None, _d(gh)), "objective_grad", check)
        return rc, f, gx, gh

    def grad_phase_ms(self):
        """{setup, products, rows, tt, finish} of the last gradient in ms (set_profiling(True) first)."""
        ms = np.zeros(5)
        self._chk(self.lib.fn("sp_grad_phase_ms")(self._h, _d(ms)), "grad_phase_ms")
        return dict(zip(("setup", "products", "rows", "tt", "finish"), ms.tolist()))
