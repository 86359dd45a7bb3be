#!/usr/bin/env python3
"""Cost of Optimizer::PoseOptimization on the device (k_pose_opt) behind the TrackWithMotionModel
search it follows.

    python tools/poseopt_step.py [--batch 256] [--out profiles/poseopt_step.json]

EuRoC settings (752x480, 1000 features), B frames resident after one MonoTrackBatch.frames call
and B after one RGBDTrackBatch.frames call (a synthetic depth map; the features whose sampled
depth is positive give stereo edges, 0.94 of the edges in the recorded run, the others mono
ones), 1000 last-frame MapPoints per frame taken from the frame's own features.
Per front-end one process alternates

  track       track_with_motion_model                   projection + search (the parent's step)
  track_opt   track_with_motion_model_and_optimize      + k_match_scatter + k_pose_opt, no host step
  track_d2h   track, then d_match copied to pinned host memory and a synchronise: what a caller
              pays before g2o can start

each timed over a window of `steps` calls (sized from a calibration step so that a window lasts
about --window seconds), `--repeats` windows each, alternating: device events for the first two,
the wall clock for the third.  Beside them tests/native/poseopt_ref (one thread) runs the distinct
frames with the MapPoints the device matched: the restatement's speed, not g2o's.  The JSON also
holds the edges per frame and, from the info words, the Levenberg iterations and trials per frame
(an iteration evaluates errors and builds H and b: 28 ordered sums; a trial evaluates errors: one).
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
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

W, H, NFEATURES, NPOINTS, MBF = 752, 480, 1000, 1000, 47.9


def measure(rgbd: bool, a, dev):
    import torch
    import my_orb_slam2_amd as m
    import poseopt_cases as pc
    from my_orb_slam2_amd import build as b
    from my_orb_slam2_amd import synth
    from my_orb_slam2_amd.features import (FRAME_POSE_DTYPE, PROJ_JOB_DTYPE, PROJ_QUERY_DTYPE,
                                           frame_pose, proj_job)
    from project_step import points_onto

    def points_at_depth(pose, kp, z):
        """MapPoints that project through `pose` within a pixel of the keypoints, at their depth."""
        from my_orb_slam2_amd.features import MAP_POINT_DTYPE
        fx, fy, cx, cy = (float(pose[q]) for q in ("fx", "fy", "cx", "cy"))
        u = kp["x"] + rng.normal(0, 0.7, len(kp))
        v = kp["y"] + rng.normal(0, 0.7, len(kp))
        R, t = pose["Rcw"].reshape(3, 3).astype(np.float64), pose["tcw"].astype(np.float64)
        z = z.astype(np.float64) * (1 + rng.normal(0, 0.002, len(kp)))
        Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
        mp = np.zeros(len(kp), MAP_POINT_DTYPE)
        mp["pos"] = ((Pc - t[None, :]) @ R).astype(np.float32)
        mp["min_dist"], mp["max_dist"] = 0.1, 1000.0
        return mp

    B = a.batch
    k = min(a.distinct, B)
    K4, dist = synth.EUROC_CAM
    imgs = np.stack([synth.frame(900 + i, W, H) for i in range(k)])
    idx = np.arange(B) % k
    if rgbd:
        yy, xx = np.mgrid[0:H, 0:W]
        depth = np.stack([(5000.0 * (3.0 + np.sin(xx / 60.0 + i) + 0.8 * np.cos(yy / 45.0)))
                          .astype(np.uint16) for i in range(k)])
        mt = m.RGBDTrackBatch(B, W, H, K4, dist, MBF, depth_factor=float(np.float32(1) / np.float32(5000)),
                              nfeatures=NFEATURES)
        mt.frames(torch.from_numpy(imgs[idx]).to(dev),
                  torch.from_numpy(depth[idx].view(np.int16)).to(dev))
        u_right, fdepth = mt.fetch_stereo()
    else:
        mt = m.MonoTrackBatch(B, W, H, K4, dist, nfeatures=NFEATURES)
        mt.frames(torch.from_numpy(imgs[idx]).to(dev))
        u_right = None
    nkp, ku, desc = mt.fetch_undistorted()
    kc = mt.kp_cap
    scale = synth.scale_tables()[0]
    rng = np.random.default_rng(0)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)

    jobs, poses, mps, keys, qdesc = [], [], [], [], []
    for j in range(k):
        n = int(nkp[j])
        pose = frame_pose(synth._rot(rng, 20.0), rng.normal(0, 1.0, 3), K4, mt.bounds, scale,
                          mbf=MBF if rgbd else 0.0)
        tgt = rng.integers(0, n, NPOINTS)
        jobs.append(proj_job(pose, 15.0, synth._rot(rng, 3.0), rng.normal(0, 0.1, 3), 0.11, not rgbd))
        poses.append(pose)
        mps.append(points_at_depth(pose, ku[j, :n][tgt], fdepth[j, :n][tgt]) if rgbd else
                   points_onto(rng, pose, ku[j, :n], tgt))
        keys.append(ku[j, :n][tgt])
        qdesc.append(desc[j, :n][tgt])
    tile = lambda parts: np.concatenate([parts[i] for i in idx])
    d_jobs = T(np.stack([jobs[i] for i in idx]).astype(PROJ_JOB_DTYPE))
    d_poses = T(np.stack([poses[i] for i in idx]).astype(FRAME_POSE_DTYPE))
    d_mps, d_keys, d_qdesc = T(tile(mps)), T(tile(keys)), T(tile(qdesc))
    nq = B * NPOINTS
    i32 = dict(dtype=torch.int32, device=dev)
    d_off = torch.arange(B + 1, **i32) * NPOINTS
    d_skip = torch.zeros(nq, dtype=torch.uint8, device=dev)
    d_q = torch.zeros(nq * PROJ_QUERY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_match, d_cnt, d_na = torch.zeros(nq, **i32), torch.zeros(B, **i32), torch.zeros(B, **i32)
    d_mpf, d_flagged = torch.zeros(B * kc, **i32), torch.zeros(1, **i32)
    d_out = torch.zeros_like(d_poses)
    d_outl = torch.zeros(B * kc, dtype=torch.uint8, device=dev)
    d_ng, d_info = torch.zeros(B, **i32), torch.zeros(B, **i32)
    h_match = torch.empty(nq, dtype=torch.int32).pin_memory()

    def track():
        mt.track_with_motion_model(d_jobs, d_mps, d_off, NPOINTS, d_keys, d_skip, d_q, d_qdesc,
                                   d_match, d_cnt, None, d_na)

    def track_opt():
        mt.track_with_motion_model_and_optimize(d_jobs, d_poses, d_mps, d_off, NPOINTS, d_keys,
                                                d_skip, d_q, d_qdesc, d_match, d_cnt, d_mpf,
                                                d_flagged, d_out, d_outl, d_ng, d_info, None, d_na)

    def track_d2h():
        track()
        h_match.copy_(d_match, non_blocking=True)
        torch.cuda.synchronize()

    def window_events(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    def window_wall(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    work = {"track": (track, window_events), "track_opt": (track_opt, window_events),
            "track_d2h": (track_d2h, window_wall)}
    steps = {}
    for name, (fn, win) in work.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        steps[name] = max(3, math.ceil(a.window * 1e3 / max(win(fn, 5), 1e-3)))
    times = {name: [] for name in work}
    for _ in range(a.repeats):
        for name, (fn, win) in work.items():       # alternate within every repeat
            times[name].append(win(fn, steps[name]))
    mt.matcher.sync()
    med = {n: float(np.median(t)) for n, t in times.items()}

    track_opt()
    torch.cuda.synchronize()
    mpf = d_mpf.cpu().numpy().reshape(B, kc)
    info = d_info.cpu().numpy().view(np.uint32)
    ng = d_ng.cpu().numpy()
    edges = (mpf >= 0).sum(1)
    iters = (info >> pc.ITERS_SHIFT) & pc.ITERS_MASK
    trials = (info >> pc.TRIALS_SHIFT) & pc.TRIALS_MASK
    # the restatement on the distinct frames, one thread
    cases = [dict(name=f"f{j}", pose=poses[j], keys=ku[j], mp_of_feat=mpf[j], mps=mps[j],
                  ur=None if u_right is None else u_right[j],
                  outlier_in=np.zeros(kc, np.uint8), max_feat=kc) for j in range(k)]
    ref_bin = b.build_poseopt_ref()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        pc.write_cases(tmp / "cases.bin", cases)
        subprocess.run([str(ref_bin), str(tmp / "cases.bin"), str(tmp / "out.bin")], check=True)
        ref = pc.read_results(tmp / "out.bin", cases)
        us = [float(subprocess.run([str(ref_bin), "--time", str(tmp / "cases.bin")], check=True,
                                   capture_output=True, text=True).stdout) for _ in range(3)]
    out = d_out.cpu().numpy().view(FRAME_POSE_DTYPE)
    agree = all(out[j].tobytes() == ref[j][0].tobytes() and int(ng[j]) == ref[j][1] and
                int(info[j]) == ref[j][2] for j in range(k))
    diff = [t - s for t, s in zip(times["track_opt"], times["track"])]
    return {
        "settings": {"batch": B, "distinct_frames": k, "points_per_frame": NPOINTS, "steps": steps,
                     "repeats": a.repeats},
        "ms_per_step": {n: {"median": med[n], "min": float(min(t)), "max": float(max(t)),
                            "repeats": [float(v) for v in t]} for n, t in times.items()},
        "pose_opt_ms": float(np.median(diff)), "pose_opt_ms_spread": [float(min(diff)), float(max(diff))],
        "pose_opt_over_track": float(np.median(diff)) / med["track"],
        "track_opt_beats_track_d2h": bool(med["track_opt"] < med["track_d2h"]),
        "mean_keypoints": float(nkp.mean()), "matches_per_frame": float(d_cnt.float().mean().item()),
        "edges_per_frame": {"mean": float(edges.mean()), "min": int(edges.min()), "max": int(edges.max())},
        "stereo_edge_share": 0.0 if u_right is None else
        float(((u_right >= 0) & (mpf >= 0)).sum() / max(int((mpf >= 0).sum()), 1)),
        "ngood_per_frame": float(ng.mean()),
        "levenberg_iterations_per_frame": float(iters.mean()),
        "levenberg_trials_per_frame": float(trials.mean()),
        "evaluations_per_frame": float((iters + trials).mean()),
        "flags_seen": sorted({n for v in info for n in pc.info_fields(v)["flags"]}),
        "restatement": {"program": "tests/native/poseopt_ref --time (one thread)",
                        "us_per_frame": float(np.median(us)), "runs": us,
                        "equals_the_device": bool(agree)},
    }


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16, help="distinct synthetic frames, tiled")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "poseopt_step.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("poseopt_step: no GPU visible; nothing measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    res = {"tool": "tools/poseopt_step.py", "device": torch.cuda.get_device_name(0),
           "timing": "device events around `steps` calls (track, track_opt); wall clock around "
                     "track + D2H copy + synchronise (track_d2h)",
           "width": W, "height": H, "nfeatures": NFEATURES,
           "mono": measure(False, a, dev), "rgbd": measure(True, a, dev)}
    out = pathlib.Path(a.out)
    os.makedirs(out.parent, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    for kind in ("mono", "rgbd"):
        r = res[kind]
        print(kind, json.dumps({n: r["ms_per_step"][n]["median"] for n in r["ms_per_step"]}),
              json.dumps({n: r[n] for n in ("pose_opt_ms", "pose_opt_over_track", "edges_per_frame",
                                            "evaluations_per_frame", "track_opt_beats_track_d2h")}),
              json.dumps(r["restatement"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
