"""PnPsolver (src/PnPsolver.cc) on the GPU: include/orbx_match.h, orbx_pnp_*.

``PnPsolver`` takes host arrays and follows the reference's names (SetRansacParameters, iterate,
find); ``ORBmatcher.pnp_iterate_batch_device`` runs many solvers from device arrays on the
matcher's stream, ``ORBmatcher.pnp_correspondences_batch_device`` builds their correspondences
from the batched SearchByBoW(KF, Frame) matches and ``ORBmatcher.pnp_apply_batch_device`` turns
their results into the poses and the MapPoint tables PoseOptimization starts from.  The caller
keeps the rand() stream (pass the raw values to ``pnp_sample_quads``) and every decision between
the calls.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import RAND_MAX, _sample_minimal_sets, _solver_limits, check, load, ptr

PNP_CORR_DTYPE = np.dtype([("i", "<i4"), ("X", "<f4", 3), ("u", "<f4"), ("v", "<f4"),
                           ("octave", "<i4")])
PNP_JOB_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                          ("sigma2", "<f4", 16), ("nlevels", "<i4"), ("th2", "<f4"),
                          ("n_matches", "<i4"), ("N", "<i4"), ("corr_off", "<i4"),
                          ("inlier_off", "<i4"), ("quad_off", "<i4"), ("best_off", "<i4"),
                          ("min_inliers", "<i4"), ("max_its", "<i4"), ("n_iterations", "<i4")])
PNP_STATE_DTYPE = np.dtype([("iterations", "<i4"), ("best_inliers", "<i4"),
                            ("best_Tcw", "<f4", 16)])
PNP_RESULT_DTYPE = np.dtype([("found", "<i4"), ("source", "<i4"), ("iteration", "<i4"),
                             ("n_run", "<i4"), ("n_inliers", "<i4"), ("no_more", "<i4"),
                             ("info", "<u4"), ("best_inliers", "<i4"), ("Tcw", "<f4", 16)])

PNP_REFINES_MASK = 0xffff
PNP_REFUSED_OCTAVE = 1 << 24
PNP_REFUSED_QUAD = 1 << 25
PNP_REFUSED_I = 1 << 26
PNP_REFUSED_LIMIT = 1 << 27
PNP_REFUSED_RANGE = 1 << 28
PNP_REFUSED_ANY = 0x1f << 24
PNP_QR_SINGULAR = 1 << 29
PNP_SVD_COMPLETED = 1 << 30


def pnp_ransac_parameters(prob: float, min_inliers: int, max_its: int, min_set: int,
                          epsilon: float, N: int) -> tuple[int, int]:
    """(mRansacMinInliers, mRansacMaxIts) after SetRansacParameters (PnPsolver.cc:121-152); host
    only."""
    a, b = ctypes.c_int32(), ctypes.c_int32()
    check("orbx_pnp_ransac_parameters",
          load().orbx_pnp_ransac_parameters(float(prob), int(min_inliers), int(max_its),
                                            int(min_set), float(epsilon), int(N),
                                            ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def pnp_sample_quads(N: int, rand_values) -> np.ndarray:
    """The minimal sets (:188-201) of len(rand_values) / 4 iterations from raw rand() values, as
    an (n_its, 4) int32 array; host only."""
    return _sample_minimal_sets("orbx_pnp_sample_quads", 4, "four", N, rand_values)


def pnp_limits() -> dict:
    """The largest N, max_its / iterations per call and jobs per call, and the scratch bound."""
    return _solver_limits("orbx_pnp_limits")


def pnp_window(max_its: int, iterations: int, n_iterations: int) -> int:
    """The iterations one iterate(n_iterations) call runs unless it returns early (`||` at :182)."""
    return max(int(max_its) - int(iterations), int(n_iterations), 0)


def pnp_job(K4, sigma2, th2: float, n_matches: int, N: int, min_inliers: int, max_its: int,
            n_iterations: int, corr_off: int = 0, inlier_off: int = 0, quad_off: int = 0,
            best_off: int = 0) -> np.ndarray:
    """One orbx_pnp_job record; K4 = (fx, fy, cx, cy)."""
    j = np.zeros((), PNP_JOB_DTYPE)
    s = np.asarray(sigma2, np.float32)
    j["fx"], j["fy"], j["cx"], j["cy"] = K4
    j["nlevels"] = len(s)
    j["sigma2"][:min(len(s), 16)] = s[:16]
    j["th2"], j["n_matches"], j["N"] = th2, n_matches, N
    j["corr_off"], j["inlier_off"], j["quad_off"], j["best_off"] = (corr_off, inlier_off,
                                                                    quad_off, best_off)
    j["min_inliers"], j["max_its"], j["n_iterations"] = min_inliers, max_its, n_iterations
    return j


def pnp_iterate(job, corr, quads, state, best, result=None, inliers=None, device: int = 0):
    """orbx_pnp_iterate: one iterate() call of one solver from host arrays.  `state`
    (PNP_STATE_DTYPE) and `best` (N bytes) are updated in place; `quads` holds the minimal sets
    from iteration 0 on, at least state.iterations + window of them; `result` / `inliers` may be
    passed in to see what the call leaves untouched.  Returns (result, inliers)."""
    jb = np.ascontiguousarray(job, PNP_JOB_DTYPE).reshape(())
    c = np.ascontiguousarray(corr, PNP_CORR_DTYPE)
    q = np.ascontiguousarray(quads, np.int32)
    if state.dtype != PNP_STATE_DTYPE or not state.flags.c_contiguous or state.size != 1:
        raise ValueError("state: one contiguous PNP_STATE_DTYPE record")
    if best.dtype != np.uint8 or best.size != int(jb["N"]) or not best.flags.c_contiguous:
        raise ValueError("best: N contiguous bytes")
    need = int(state["iterations"].reshape(-1)[0]) + pnp_window(
        jb["max_its"], state["iterations"].reshape(-1)[0], jb["n_iterations"])
    if c.size != int(jb["N"]) or q.size < 4 * need:
        raise ValueError("corr holds N records and quads 4 * (iterations + window) indices")
    res = np.zeros((), PNP_RESULT_DTYPE) if result is None else result
    inl = np.zeros(int(jb["n_matches"]), np.uint8) if inliers is None else inliers
    if inl.dtype != np.uint8 or inl.size != int(jb["n_matches"]) or not inl.flags.c_contiguous:
        raise ValueError("inliers: n_matches contiguous bytes")
    check("orbx_pnp_iterate", load().orbx_pnp_iterate(ptr(jb), ptr(c), ptr(q), ptr(state),
                                                      ptr(best), ptr(res), ptr(inl), device))
    return res, inl


class PnPsolver:
    """The reference's PnPsolver over host arrays.

    K4: the frame's (fx, fy, cx, cy); keys_un: its mvKeysUn (orbx keypoint records: x, y and
    octave are read); sigma2: its mvLevelSigma2; points / valid: vpMapPointMatches as an
    (n_matches, 3) float32 array of world positions and the mask of the slots that hold a MapPoint
    that is not bad; rand_values: the raw rand() values the iterations will consume, four each."""

    def __init__(self, K4, keys_un, sigma2, points, valid, rand_values, device: int = 0):
        pts = np.asarray(points, np.float32).reshape(-1, 3)
        ok = np.asarray(valid, bool).reshape(-1)
        idx = np.flatnonzero(ok)
        self.corr = np.zeros(len(idx), PNP_CORR_DTYPE)
        self.corr["i"] = idx
        self.corr["X"] = pts[idx]
        self.corr["u"], self.corr["v"] = keys_un["x"][idx], keys_un["y"][idx]
        self.corr["octave"] = keys_un["octave"][idx]
        self.K4, self.sigma2 = tuple(float(v) for v in K4), np.asarray(sigma2, np.float32)
        self.n_matches, self.N = len(ok), len(idx)
        self.rand_values = np.ascontiguousarray(rand_values, np.int32).reshape(-1)
        self.cursor = 0                       # rand() values consumed so far
        self.device = device
        self.state = np.zeros(1, PNP_STATE_DTYPE)
        self.best = np.zeros(self.N, np.uint8)
        self.SetRansacParameters()

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 8,
                            maxIterations: int = 300, minSet: int = 4, epsilon: float = 0.4,
                            th2: float = 5.991):
        self.min_inliers, self.max_its = pnp_ransac_parameters(probability, minInliers,
                                                               maxIterations, minSet, epsilon,
                                                               self.N)
        self.th2 = float(th2)

    def iterate(self, nIterations: int):
        """-> (Tcw as a 4x4 array or None, bNoMore, vbInliers as n_matches bools, nInliers)"""
        it = int(self.state["iterations"][0])
        w = pnp_window(self.max_its, it, nIterations)
        # N < mRansacMinInliers returns at once (:173-177): no rand() value is read, and the
        # window's minimal sets, which the entry still takes, stay zero
        runs = self.N >= self.min_inliers
        if runs and self.rand_values.size < self.cursor + 4 * w:
            raise ValueError(f"{self.cursor + 4 * w} rand() values are needed")
        # the call's minimal sets sit where the job expects iteration `it`'s
        quads = np.zeros((it + w, 4), np.int32)
        if runs and w:
            quads[it:] = pnp_sample_quads(self.N, self.rand_values[self.cursor:self.cursor + 4 * w])
        job = pnp_job(self.K4, self.sigma2, self.th2, self.n_matches, self.N, self.min_inliers,
                      self.max_its, int(nIterations))
        res, inl = pnp_iterate(job, self.corr, quads, self.state, self.best, device=self.device)
        if int(res["info"]) & PNP_REFUSED_ANY:
            raise ValueError(f"PnPsolver: the job was refused, info = {int(res['info']):#x}")
        self.cursor += 4 * int(res["n_run"])
        self.info = int(res["info"])
        T = res["Tcw"].reshape(4, 4).copy() if res["found"] else None
        return T, bool(res["no_more"]), inl.astype(bool), int(res["n_inliers"])

    def find(self):
        """-> (Tcw or None, vbInliers, nInliers)"""
        T, _, inl, n = self.iterate(self.max_its)
        return T, inl, n
