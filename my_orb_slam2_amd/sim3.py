"""Sim3Solver (src/Sim3Solver.cc) on the GPU: include/orbx_match.h, orbx_sim3_*.

``Sim3Solver`` takes host arrays and follows the reference's names (SetRansacParameters, iterate,
find, GetEstimatedRotation / Translation / Scale); ``ORBmatcher.sim3_iterate_batch_device`` runs
many solvers from device arrays on the matcher's stream.  The caller keeps the object tests of the
reference's constructor (isBad, GetIndexInKeyFrame) and the rand() stream (pass the raw values to
``sim3_sample_triples``).  ``OptimizeSim3`` / ``sim3_optimize`` (Optimizer::OptimizeSim3) refine
the solver's model over the matches; ``ORBmatcher.sim3_optimize_batch_device`` does so for many
candidates from device arrays, reading the solver's result records in place.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import RAND_MAX, _sample_minimal_sets, _solver_limits, check, load, ptr
from .features import FRAME_POSE_DTYPE

SIM3_CORR_DTYPE = np.dtype([("i1", "<i4"), ("X1w", "<f4", 3), ("X2w", "<f4", 3),
                            ("octave1", "<i4"), ("octave2", "<i4")])
SIM3_JOB_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("sigma2_1", "<f4", 16),
                           ("sigma2_2", "<f4", 16), ("nlevels1", "<i4"), ("nlevels2", "<i4"),
                           ("mN1", "<i4"), ("N", "<i4"), ("corr_off", "<i4"),
                           ("inlier_off", "<i4"), ("triple_off", "<i4"), ("fix_scale", "<i4"),
                           ("min_inliers", "<i4"), ("max_its", "<i4"), ("n_iterations", "<i4")])
SIM3_STATE_DTYPE = np.dtype([("iterations", "<i4"), ("best_inliers", "<i4")])
SIM3_RESULT_DTYPE = np.dtype([("found", "<i4"), ("iteration", "<i4"), ("n_inliers", "<i4"),
                              ("no_more", "<i4"), ("info", "<u4"), ("best_updated", "<i4"),
                              ("best_inliers", "<i4"), ("R12", "<f4", 9), ("t12", "<f4", 3),
                              ("s12", "<f4"), ("T12", "<f4", 16)])

SIM3_REFUSED_OCTAVE = 1 << 24
SIM3_REFUSED_TRIPLE = 1 << 25
SIM3_REFUSED_I1 = 1 << 26
SIM3_REFUSED_LIMIT = 1 << 27
SIM3_REFUSED_RANGE = 1 << 28
SIM3_REFUSED_ANY = 0x1f << 24


def sim3_ransac_iterations(prob: float, min_inliers: int, max_its: int, N: int) -> int:
    """mRansacMaxIts after SetRansacParameters (Sim3Solver.cc:114-138); host only."""
    return int(load().orbx_sim3_ransac_iterations(float(prob), int(min_inliers), int(max_its),
                                                  int(N)))


def sim3_sample_triples(N: int, rand_values) -> np.ndarray:
    """The minimal sets (:163-177) of len(rand_values) / 3 iterations from raw rand() values, as
    an (n_its, 3) int32 array; host only."""
    return _sample_minimal_sets("orbx_sim3_sample_triples", 3, "three", N, rand_values)


def sim3_limits() -> dict:
    """The largest N, max_its / iterations per call and jobs per call, and the scratch bound."""
    return _solver_limits("orbx_sim3_limits")


def sim3_job(sigma2_1, sigma2_2, mN1: int, N: int, fix_scale: bool, min_inliers: int,
             max_its: int, n_iterations: int, kf1: int = 0, kf2: int = 1, corr_off: int = 0,
             inlier_off: int = 0, triple_off: int = 0) -> np.ndarray:
    """One orbx_sim3_job record."""
    j = np.zeros((), SIM3_JOB_DTYPE)
    s1, s2 = np.asarray(sigma2_1, np.float32), np.asarray(sigma2_2, np.float32)
    j["nlevels1"], j["nlevels2"] = len(s1), len(s2)
    j["sigma2_1"][:min(len(s1), 16)] = s1[:16]
    j["sigma2_2"][:min(len(s2), 16)] = s2[:16]
    j["kf1"], j["kf2"], j["mN1"], j["N"] = kf1, kf2, mN1, N
    j["corr_off"], j["inlier_off"], j["triple_off"] = corr_off, inlier_off, triple_off
    j["fix_scale"], j["min_inliers"] = int(bool(fix_scale)), min_inliers
    j["max_its"], j["n_iterations"] = max_its, n_iterations
    return j


def sim3_iterate(pose1, pose2, job, corr, triples, state, result=None, inliers=None,
                 device: int = 0):
    """orbx_sim3_iterate: one iterate() call of one solver from host arrays.  `state`
    (SIM3_STATE_DTYPE) is updated in place; `result` / `inliers` may be passed in to see what the
    call leaves untouched.  Returns (result, inliers)."""
    p1 = np.ascontiguousarray(pose1, FRAME_POSE_DTYPE).reshape(())
    p2 = np.ascontiguousarray(pose2, FRAME_POSE_DTYPE).reshape(())
    jb = np.ascontiguousarray(job, SIM3_JOB_DTYPE).reshape(())
    c = np.ascontiguousarray(corr, SIM3_CORR_DTYPE)
    t = np.ascontiguousarray(triples, np.int32)
    if state.dtype != SIM3_STATE_DTYPE or not state.flags.c_contiguous:
        raise ValueError("state: a contiguous SIM3_STATE_DTYPE record")
    if c.size != int(jb["N"]) or t.size != 3 * int(jb["max_its"]):
        raise ValueError("corr holds N records and triples 3 * max_its indices")
    res = np.zeros((), SIM3_RESULT_DTYPE) if result is None else result
    inl = np.zeros(int(jb["mN1"]), np.uint8) if inliers is None else inliers
    if inl.dtype != np.uint8 or inl.size != int(jb["mN1"]) or not inl.flags.c_contiguous:
        raise ValueError("inliers: mN1 contiguous bytes")
    check("orbx_sim3_iterate", load().orbx_sim3_iterate(ptr(p1), ptr(p2), ptr(jb), ptr(c), ptr(t),
                                                        ptr(state), ptr(res), ptr(inl), device))
    return res, inl


class Sim3Solver:
    """The reference's Sim3Solver over host arrays.

    pose1 / pose2: frame_pose records of the two keyframes (Rcw, tcw and the intrinsics are read);
    corr: SIM3_CORR_DTYPE, the correspondences the reference's constructor keeps, in its order;
    sigma2_1 / sigma2_2: the keyframes' mvLevelSigma2; mN1 = len(vpMatched12); rand_values: the
    raw rand() values the iterations will consume, three each (at least 3 * max_iterations)."""

    def __init__(self, pose1, pose2, corr, sigma2_1, sigma2_2, mN1: int, fix_scale: bool,
                 rand_values, device: int = 0):
        self.pose1, self.pose2 = pose1, pose2
        self.corr = np.ascontiguousarray(corr, SIM3_CORR_DTYPE)
        self.sigma2 = (sigma2_1, sigma2_2)
        self.mN1, self.N, self.fix_scale = int(mN1), int(self.corr.size), bool(fix_scale)
        self.rand_values = np.ascontiguousarray(rand_values, np.int32).reshape(-1)
        self.device = device
        self.state = np.zeros((), SIM3_STATE_DTYPE)
        self._best = None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 6,
                            maxIterations: int = 300):
        self.min_inliers = int(minInliers)
        self.max_its = sim3_ransac_iterations(probability, minInliers, maxIterations, self.N)
        if self.rand_values.size < 3 * self.max_its:
            raise ValueError(f"{3 * self.max_its} rand() values are needed")
        if self.N >= 3:
            self.triples = sim3_sample_triples(self.N, self.rand_values[:3 * self.max_its])
        else:
            self.triples = np.zeros((self.max_its, 3), np.int32)
        self.state["iterations"] = 0          # :137; mnBestInliers stays

    def iterate(self, nIterations: int):
        """-> (T12 as a 4x4 array or None, bNoMore, vbInliers as mN1 bools, nInliers)"""
        job = sim3_job(self.sigma2[0], self.sigma2[1], self.mN1, self.N, self.fix_scale,
                       self.min_inliers, self.max_its, int(nIterations))
        res, inl = sim3_iterate(self.pose1, self.pose2, job, self.corr, self.triples, self.state,
                                device=self.device)
        if int(res["info"]) & SIM3_REFUSED_ANY:
            raise ValueError(f"Sim3Solver: the job was refused, info = {int(res['info']):#x}")
        if res["best_updated"]:
            self._best = res.copy()
        T = res["T12"].reshape(4, 4).copy() if res["found"] else None
        return T, bool(res["no_more"]), inl.astype(bool), int(res["n_inliers"])

    def find(self):
        """-> (T12 or None, vbInliers12, nInliers)"""
        T, _, inl, n = self.iterate(self.max_its)
        return T, inl, n

    def _need_best(self):
        if self._best is None:
            raise RuntimeError("no iteration has recorded a model yet")
        return self._best

    def GetEstimatedRotation(self):
        return self._need_best()["R12"].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return self._need_best()["t12"].copy()

    def GetEstimatedScale(self) -> float:
        return float(self._need_best()["s12"])


# ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:1070-1265): include/orbx_match.h, orbx_sim3_optimize* ----

SIM3OPT_CORR_DTYPE = np.dtype([("i1", "<i4"), ("X1w", "<f4", 3), ("X2w", "<f4", 3),
                               ("kp1", "<f4", 2), ("kp2", "<f4", 2), ("octave1", "<i4"),
                               ("octave2", "<i4")])
SIM3OPT_JOB_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("sigma2_1", "<f4", 16),
                              ("sigma2_2", "<f4", 16), ("nlevels1", "<i4"), ("nlevels2", "<i4"),
                              ("mN1", "<i4"), ("N", "<i4"), ("corr_off", "<i4"),
                              ("flag_off", "<i4"), ("th2", "<f4"), ("fix_scale", "<i4")])
SIM3OPT_IN_DTYPE = np.dtype([("R12", "<f4", 9), ("t12", "<f4", 3), ("s12", "<f4")])
SIM3OPT_RESULT_DTYPE = np.dtype([("n_inliers", "<i4"), ("n_correspondences", "<i4"),
                                 ("n_bad", "<i4"), ("info", "<u4"), ("q", "<f8", 4),
                                 ("t", "<f8", 3), ("s", "<f8"), ("T12", "<f4", 16)])
# where an orbx_sim3_result holds an orbx_sim3opt_in (R12, t12, s12)
SIM3_RESULT_IN_OFFSET = SIM3_RESULT_DTYPE.fields["R12"][1]

SIM3OPT_REFUSED_OCTAVE = 1 << 23
SIM3OPT_REFUSED_I1 = 1 << 24
SIM3OPT_REFUSED_LIMIT = 1 << 25
SIM3OPT_REFUSED_RANGE = 1 << 26
SIM3OPT_REFUSED_ANY = 0xf << 23
SIM3OPT_THETA_LIMIT = 1 << 27
SIM3OPT_EXP_LIMIT = 1 << 28
SIM3OPT_NONPOSITIVE_SOLVE = 1 << 29
SIM3OPT_FEW_INLIERS = 1 << 30
SIM3OPT_DROPPED = 1 << 31


def sim3opt_limits() -> dict:
    """The largest N and the most jobs a call of sim3_optimize* takes."""
    a, b = ctypes.c_int32(), ctypes.c_int32()
    check("orbx_sim3opt_limits", load().orbx_sim3opt_limits(ctypes.byref(a), ctypes.byref(b)))
    return dict(max_n=a.value, max_jobs=b.value)


def sim3opt_job(sigma2_1, sigma2_2, mN1: int, N: int, th2: float = 10.0, fix_scale: bool = False,
                kf1: int = 0, kf2: int = 1, corr_off: int = 0, flag_off: int = 0) -> np.ndarray:
    """One orbx_sim3opt_job record."""
    j = np.zeros((), SIM3OPT_JOB_DTYPE)
    s1, s2 = np.asarray(sigma2_1, np.float32), np.asarray(sigma2_2, np.float32)
    j["nlevels1"], j["nlevels2"] = len(s1), len(s2)
    j["sigma2_1"][:min(len(s1), 16)] = s1[:16]
    j["sigma2_2"][:min(len(s2), 16)] = s2[:16]
    j["kf1"], j["kf2"], j["mN1"], j["N"] = kf1, kf2, mN1, N
    j["corr_off"], j["flag_off"] = corr_off, flag_off
    j["th2"], j["fix_scale"] = th2, int(bool(fix_scale))
    return j


def sim3_optimize(pose1, pose2, job, corr, sim3_in, keep=None, device: int = 0):
    """orbx_sim3_optimize: one OptimizeSim3 call from host arrays.  `sim3_in`: a SIM3OPT_IN_DTYPE
    record (the solver's R12, t12, s12); `keep`: mN1 bytes (vpMatches1 != NULL going in; ones when
    omitted), returned with the dropped pairs' entries zeroed.  Returns (result, keep)."""
    p1 = np.ascontiguousarray(pose1, FRAME_POSE_DTYPE).reshape(())
    p2 = np.ascontiguousarray(pose2, FRAME_POSE_DTYPE).reshape(())
    jb = np.ascontiguousarray(job, SIM3OPT_JOB_DTYPE).reshape(())
    c = np.ascontiguousarray(corr, SIM3OPT_CORR_DTYPE)
    s = np.ascontiguousarray(sim3_in, SIM3OPT_IN_DTYPE).reshape(())
    if c.size != int(jb["N"]):
        raise ValueError("corr holds N records")
    mN1 = int(jb["mN1"])
    k = np.ones(max(mN1, 0), np.uint8) if keep is None else np.array(keep, np.uint8)
    if k.size != max(mN1, 0):
        raise ValueError("keep: mN1 bytes")
    res = np.zeros((), SIM3OPT_RESULT_DTYPE)
    check("orbx_sim3_optimize", load().orbx_sim3_optimize(ptr(p1), ptr(p2), ptr(jb), ptr(c), ptr(s),
                                                          ptr(res), ptr(k), device))
    return res, k


def OptimizeSim3(pose1, pose2, corr, sigma2_1, sigma2_2, mN1: int, R12, t12, s12: float,
                 th2: float = 10.0, bFixScale: bool = False, keep=None, device: int = 0):
    """Optimizer::OptimizeSim3 by the reference's name over host arrays.  corr: SIM3OPT_CORR_DTYPE,
    the correspondences the reference's loop keeps, in increasing i1; R12, t12, s12: the solver's
    model (g2oS12 going in).  Returns (nInliers, S12, keep): S12 = dict(q (x, y, z, w), t, s, T12
    (4x4 float32, Converter::toCvMat(g2oS12))) and keep = vpMatches1 != NULL after the call."""
    c = np.ascontiguousarray(corr, SIM3OPT_CORR_DTYPE)
    s_in = np.zeros((), SIM3OPT_IN_DTYPE)
    s_in["R12"] = np.asarray(R12, np.float32).reshape(9)
    s_in["t12"] = np.asarray(t12, np.float32).reshape(3)
    s_in["s12"] = s12
    job = sim3opt_job(sigma2_1, sigma2_2, int(mN1), int(c.size), th2, bFixScale)
    res, k = sim3_optimize(pose1, pose2, job, c, s_in, keep, device)
    if int(res["info"]) & SIM3OPT_REFUSED_ANY:
        raise ValueError(f"OptimizeSim3: the job was refused, info = {int(res['info']):#x}")
    S12 = dict(q=res["q"].copy(), t=res["t"].copy(), s=float(res["s"]),
               T12=res["T12"].reshape(4, 4).copy(), info=int(res["info"]))
    return int(res["n_inliers"]), S12, k
