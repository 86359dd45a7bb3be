#!/usr/bin/env python3
"""Cost of PnPsolver::iterate on the device (k_pnp_hypotheses, k_pnp_select) for the candidates of
one relocalisation round, beside the batched SearchByBoW(KF, Frame) call in front of it.

    python tools/pnp_step.py [--out profiles/pnp_step.json]

8 candidate keyframes against one frame of 1000 features; each candidate shares 60 to 95 features
with the frame (a third of the MapPoints displaced), Tracking's parameters (0.99, 10, 300, 4, 0.5,
5.991), so mRansacMaxIts is 35 and a first iterate(5) call runs 35 iterations (`||` at
PnPsolver.cc:182).  One process alternates

  bow        orbx_search_by_bow_kf_frame_batch_device for the 8 candidates
  corr       orbx_pnp_correspondences_batch_device
  iterate5   orbx_pnp_iterate_batch_device, iterate(5) of every candidate from a zeroed state;
             the two fills that zero the state and the best bytes are inside the timed window
  reset      those two fills alone
  apply      orbx_pnp_apply_batch_device

each timed with device events over a window of `steps` calls (sized from a calibration step so that
a window lasts about --window seconds), `--repeats` windows each, alternating.  tests/native/pnp_ref
(one thread) runs the same eight jobs on the host; it stops at the first returned pose, the device
scores every iteration of the window, so the two do different amounts of work
(`iterations_until_return`).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SHARED = (60, 65, 70, 75, 80, 85, 90, 95)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pnp_step.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("pnp_step: no GPU visible; nothing measured", file=sys.stderr)
        return 2
    import pnp_cases as pc
    from my_orb_slam2_amd import ORBmatcher, synth
    from my_orb_slam2_amd import build as b
    from my_orb_slam2_amd.features import FRAME_POSE_DTYPE, frame_pose
    from my_orb_slam2_amd.matcher import DeviceFeatureSet, DeviceKfDb
    from my_orb_slam2_amd.pnp import (PNP_CORR_DTYPE, PNP_JOB_DTYPE, PNP_RESULT_DTYPE,
                                      PNP_STATE_DTYPE, pnp_job, pnp_ransac_parameters,
                                      pnp_sample_quads, pnp_window)
    dev = torch.device("cuda", 0)
    T = lambda x: torch.from_numpy(np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8).copy()).to(dev)
    frame, R, t, kfs, valids, mps = pc.small_map(700, n_frame=1000, shared=SHARED, n_kf=900)
    rng = np.random.default_rng(1)
    for mp, m in zip(mps, SHARED):                       # a third of the shared MapPoints displaced
        bad = rng.choice(m, m // 3, replace=False)
        mp["pos"][bad] += rng.normal(size=(len(bad), 3)).astype(np.float32)
    K, nf = len(kfs), frame.n
    scale, sigma2, _ = synth.scale_tables()
    matcher = ORBmatcher(0.75, True)
    sync = matcher.sync
    db, df = DeviceKfDb(kfs, valids, dev), DeviceFeatureSet(frame, dev)
    mp_off = np.cumsum([0] + [len(m) for m in mps]).astype(np.int32)
    d_mps, d_mp_off = T(np.concatenate(mps)), T(mp_off)
    d_match = torch.full((K, nf), -1, dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(K, dtype=torch.int32, device=dev)
    d_corr, d_N = T(np.zeros(K * nf, PNP_CORR_DTYPE)), torch.zeros(K, dtype=torch.int32, device=dev)

    def bow():
        matcher.search_by_bow_kf_frame_batch_device(db.c, df.c, d_match, d_cnt)

    def corr():
        matcher.pnp_correspondences_batch_device(K, d_match, nf, df.keys, nf, d_mps, d_mp_off,
                                                 d_corr, nf, d_N)
    bow(), corr(), sync()
    N = d_N.cpu().numpy()
    params = [pnp_ransac_parameters(0.99, 10, 300, 4, 0.5, int(n)) for n in N]
    n_q = 64
    rand = rng.integers(0, pc.RAND_MAX, size=(K, 4 * n_q), endpoint=True).astype(np.int32)
    quads = np.stack([pnp_sample_quads(int(N[j]), rand[j]) for j in range(K)])
    jobs = np.zeros(K, PNP_JOB_DTYPE)
    for j in range(K):
        jobs[j] = pnp_job(pc.K4, sigma2, 5.991, nf, int(N[j]), params[j][0], params[j][1], 5,
                          corr_off=j * nf, inlier_off=j * nf, quad_off=j * n_q, best_off=j * nf)
    window_its = max(pnp_window(p[1], 0, 5) for p in params)
    d_jobs, d_quads = T(jobs), T(quads)
    d_state, d_best = T(np.zeros(K, PNP_STATE_DTYPE)), T(np.zeros(K * nf, np.uint8))
    d_res, d_inl = T(np.zeros(K, PNP_RESULT_DTYPE)), T(np.zeros(K * nf, np.uint8))
    d_tmpl = T(np.asarray(frame_pose(np.eye(3), np.zeros(3), pc.K4, (0, 640, 0, 480), scale)))
    d_poses = T(np.zeros(K, FRAME_POSE_DTYPE))
    d_mpf = torch.full((K, nf), -1, dtype=torch.int32, device=dev)

    def reset():
        d_state.zero_()
        d_best.zero_()

    def iterate5():
        reset()
        matcher.pnp_iterate_batch_device(d_jobs, K, nf, window_its, d_corr, d_quads, d_state, d_best,
                                         d_res, d_inl)

    def apply():
        matcher.pnp_apply_batch_device(K, d_jobs, d_res, d_inl, d_match, nf, nf, d_tmpl, d_poses,
                                       d_mpf, nf)

    def window(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    work = {"bow": bow, "corr": corr, "iterate5": iterate5, "reset": reset, "apply": apply}
    steps = {}
    for name, fn in work.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        steps[name] = max(3, math.ceil(a.window * 1e3 / max(window(fn, 5), 1e-3)))
    times = {name: [] for name in work}
    for _ in range(a.repeats):
        for name, fn in work.items():                  # alternate within every repeat
            times[name].append(window(fn, steps[name]))
    sync()

    # the restatement on the same jobs, one thread, and its results against the device's
    corr_h = np.frombuffer(d_corr.cpu().numpy().tobytes(), PNP_CORR_DTYPE)
    res = np.frombuffer(d_res.cpu().numpy().tobytes(), PNP_RESULT_DTYPE)
    ref_bin = b.build_pnp_ref()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        with open(tmp / "cases.bin", "wb") as f:
            f.write(np.int32(K).tobytes())
            for j in range(K):
                n = int(N[j])
                f.write(np.array([n, nf, 1, n_q], np.int32).tobytes())
                f.write(jobs[j].tobytes() + np.int32(5).tobytes())
                f.write(np.zeros(1, PNP_STATE_DTYPE).tobytes() + bytes(n))
                f.write(corr_h[j * nf:j * nf + n].tobytes() + quads[j].tobytes())
        subprocess.run([str(ref_bin), str(tmp / "cases.bin"), str(tmp / "out.bin")], check=True)
        data = (tmp / "out.bin").read_bytes()
        o, agree, until = 0, True, []
        for j in range(K):
            rec = data[o:o + PNP_RESULT_DTYPE.itemsize]
            o += PNP_RESULT_DTYPE.itemsize + nf + PNP_STATE_DTYPE.itemsize + int(N[j])
            agree = agree and pc.canon(rec) == pc.canon(res[j:j + 1].tobytes())
            until.append(int(np.frombuffer(rec, PNP_RESULT_DTYPE)["n_run"][0]))
        runs = []
        for _ in range(3):
            lines = subprocess.run([str(ref_bin), "--time", str(tmp / "cases.bin")], check=True,
                                   capture_output=True, text=True).stdout.split("\n")
            runs.append(sum(float(l.split()[2]) for l in lines if l.strip()) / 1e3)
    med = {n: float(np.median(v)) for n, v in times.items()}
    out = {"tool": "tools/pnp_step.py", "device": torch.cuda.get_device_name(0),
           "timing": "device events around `steps` calls",
           "settings": {"candidates": K, "frame_features": nf, "N": [int(n) for n in N],
                        "min_inliers": [p[0] for p in params], "max_its": [p[1] for p in params],
                        "window_iterations": window_its, "steps": steps, "repeats": a.repeats},
           "ms_per_call": {n: {"median": med[n], "min": float(min(v)), "max": float(max(v)),
                               "repeats": [float(x) for x in v]} for n, v in times.items()},
           "restatement": {"program": "tests/native/pnp_ref --time (one thread)",
                           "ms_per_8_jobs": float(np.median(runs)), "runs": runs,
                           "equals_the_device": bool(agree), "iterations_until_return": until},
           "found": [int(r) for r in res["found"]]}
    p = pathlib.Path(a.out)
    os.makedirs(p.parent, exist_ok=True)
    p.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"ms_per_call": med, "restatement_ms_per_8_jobs": out["restatement"]["ms_per_8_jobs"],
                      "equal": bool(agree), "N": out["settings"]["N"], "found": out["found"],
                      "iterations_until_return": until}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
