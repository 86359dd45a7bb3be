#!/usr/bin/env python3
"""Cost of projecting MapPoints on the device (k_project) next to the projection search it feeds.

    python tools/project_step.py [--batch 256] [--out profiles/project_step.json]

EuRoC settings (752x480, 1000 features), B frames resident after one MonoTrackBatch.frames call,
1000 last-frame MapPoints per frame taken from the frame's own features.  One process alternates

  project   MonoTrackBatch.project_last_frame       k_project<LAST_FRAME> alone
  search    search_by_projection_batch_device       the LAST_FRAME batched search on ready-made
                                                    resident queries (the path before k_project)
  track     MonoTrackBatch.track_with_motion_model  project + search
  fuse      project_map_points_batch_device         k_project<FUSE>, 32 jobs x 4000 points

each timed with device events over a window of `steps` calls (sized from a calibration step so
that a window lasts about --window seconds), `--repeats` windows each, alternating.  The JSON
holds the per-step times (median over the repeats and their spread), track / search with its
spread, and for the two projections the algorithmic bytes (32 B read + 32 B written per point,
28 B of keypoint where read, 1 B of skip flag) over their time against the HBM peak.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

W, H, NFEATURES, NPOINTS = 752, 480, 1000, 1000
FUSE_JOBS, FUSE_POINTS = 32, 4000
HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes per second (spec)


def points_onto(rng, pose, keys, target):
    """MapPoints that project through `pose` within a pixel of keys[target], at the depth that
    puts PredictScale at the feature's octave, the viewing ray as normal."""
    from my_orb_slam2_amd.features import MAP_POINT_DTYPE
    n = len(target)
    fx, fy, cx, cy = (float(pose[k]) for k in ("fx", "fy", "cx", "cy"))
    u = keys["x"][target] + rng.normal(0, 0.7, n)
    v = keys["y"][target] + rng.normal(0, 0.7, n)
    Z = rng.uniform(2.0, 30.0, n)
    R, t = pose["Rcw"].reshape(3, 3).astype(np.float64), pose["tcw"].astype(np.float64)
    Pc = np.stack([(u - cx) / fx * Z, (v - cy) / fy * Z, Z], 1)
    P = (Pc - t[None, :]) @ R
    PO = P + (R.T @ t)[None, :]
    dist = np.linalg.norm(PO, axis=1)
    mp = np.zeros(n, MAP_POINT_DTYPE)
    mp["pos"], mp["normal"] = P.astype(np.float32), (PO / dist[:, None]).astype(np.float32)
    mp["max_dist"] = (dist * 1.2 ** (keys["octave"][target] - 0.5)).astype(np.float32)
    mp["min_dist"] = mp["max_dist"] / np.float32(1.2 ** 7)
    return mp


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16, help="distinct synthetic frames, tiled")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "project_step.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("project_step: no GPU visible; nothing measured", file=sys.stderr)
        return 2
    import my_orb_slam2_amd as m
    from my_orb_slam2_amd import synth
    from my_orb_slam2_amd.features import (PROJ_FUSE, PROJ_JOB_DTYPE, PROJ_LAST_FRAME,
                                           PROJ_QUERY_DTYPE, frame_pose, proj_job,
                                           project_map_points_batch_device)

    dev = torch.device("cuda", 0)
    B = a.batch
    k = min(a.distinct, B)
    K4, dist = synth.EUROC_CAM
    imgs = np.stack([synth.frame(900 + i, W, H) for i in range(k)])
    idx = np.arange(B) % k
    mt = m.MonoTrackBatch(B, W, H, K4, dist, nfeatures=NFEATURES)
    mt.frames(torch.from_numpy(imgs[idx]).to(dev))
    nkp, ku, desc = mt.fetch_undistorted()
    scale = synth.scale_tables()[0]
    rng = np.random.default_rng(0)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)

    # TrackWithMotionModel: 1000 last-frame MapPoints per frame, observed as the frame's features
    jobs, mps, keys, qdesc = [], [], [], []
    for j in range(k):
        n = int(nkp[j])
        pose = frame_pose(synth._rot(rng, 20.0), rng.normal(0, 1.0, 3), K4, mt.bounds, scale)
        tgt = rng.integers(0, n, NPOINTS)
        jobs.append(proj_job(pose, 15.0, synth._rot(rng, 3.0), rng.normal(0, 0.1, 3), 0.11, True))
        mps.append(points_onto(rng, pose, ku[j, :n], tgt))
        keys.append(ku[j, :n][tgt])
        qdesc.append(desc[j, :n][tgt])
    tile = lambda parts: np.concatenate([parts[i] for i in idx])
    d_jobs = T(np.stack([jobs[i] for i in idx]).astype(PROJ_JOB_DTYPE))
    d_mps, d_keys, d_qdesc = T(tile(mps)), T(tile(keys)), T(tile(qdesc))
    nq = B * NPOINTS
    d_off = torch.arange(B + 1, dtype=torch.int32, device=dev) * NPOINTS
    d_skip = torch.zeros(nq, dtype=torch.uint8, device=dev)
    d_q = torch.zeros(nq * PROJ_QUERY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_match = torch.zeros(nq, dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    d_na = torch.zeros(B, dtype=torch.int32, device=dev)

    # Fuse: 32 neighbour keyframes x 4000 MapPoints
    fpose = frame_pose(synth._rot(rng, 20.0), rng.normal(0, 1.0, 3), K4, mt.bounds, scale, mbf=40.0)
    fmp = points_onto(rng, fpose, ku[0, :int(nkp[0])], rng.integers(0, int(nkp[0]), FUSE_POINTS))
    fjobs = np.repeat(proj_job(fpose, 3.0).reshape(1), FUSE_JOBS).astype(PROJ_JOB_DTYPE)
    d_fjobs, d_fmps = T(fjobs), T(np.tile(fmp, FUSE_JOBS))
    nf = FUSE_JOBS * FUSE_POINTS
    d_foff = torch.arange(FUSE_JOBS + 1, dtype=torch.int32, device=dev) * FUSE_POINTS
    d_fskip = torch.zeros(nf, dtype=torch.uint8, device=dev)
    d_fq = torch.zeros(nf * PROJ_QUERY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_fna = torch.zeros(FUSE_JOBS, dtype=torch.int32, device=dev)

    def project():
        mt.project_last_frame(d_jobs, d_mps, d_off, NPOINTS, d_keys, d_skip, d_q, d_na)

    def search():
        mt.matcher.search_by_projection_batch_device(PROJ_LAST_FRAME, mt, d_qdesc, d_q, d_off,
                                                     d_match, d_cnt)

    def track():
        mt.track_with_motion_model(d_jobs, d_mps, d_off, NPOINTS, d_keys, d_skip, d_q, d_qdesc,
                                   d_match, d_cnt, None, d_na)

    def fuse():
        project_map_points_batch_device(PROJ_FUSE, d_fjobs, FUSE_JOBS, d_fmps, d_foff, FUSE_POINTS,
                                        None, d_fskip, d_fq, d_fna)

    project()          # the resident queries `search` reads
    work = {"project": project, "search": search, "track": track, "fuse": fuse}

    def window(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    steps = {}
    for name, fn in work.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        steps[name] = max(5, math.ceil(a.window * 1e3 / max(window(fn, 20), 1e-3)))
    times = {name: [] for name in work}
    for _ in range(a.repeats):
        for name, fn in work.items():        # alternate within every repeat
            times[name].append(window(fn, steps[name]))
    mt.matcher.sync()
    med = {n: float(np.median(t)) for n, t in times.items()}
    byts = {"project": nq * (32 + 32 + 28 + 1), "fuse": nf * (32 + 32 + 1)}
    ratio = [c / b for c, b in zip(times["track"], times["search"])]
    res = {
        "tool": "tools/project_step.py", "device": torch.cuda.get_device_name(0),
        "settings": {"width": W, "height": H, "nfeatures": NFEATURES, "batch": B,
                     "points_per_frame": NPOINTS, "fuse_jobs": FUSE_JOBS,
                     "fuse_points_per_job": FUSE_POINTS, "distinct_frames": k, "steps": steps,
                     "repeats": a.repeats, "timing": "device events around `steps` calls"},
        "ms_per_step": {n: {"median": med[n], "min": float(min(t)), "max": float(max(t)),
                            "repeats": [float(v) for v in t]} for n, t in times.items()},
        "ratio_track_over_search": float(np.median(ratio)),
        "ratio_spread": [float(min(ratio)), float(max(ratio))],
        "mean_keypoints": float(nkp.mean()),
        "active_queries_per_frame": float(d_na.float().mean().item()),
        "matches_per_frame": float(d_cnt.float().mean().item()),
        "fuse_active_per_job": float(d_fna.float().mean().item()),
        "algorithmic_bytes": byts,
        "fraction_of_hbm_peak": {n: byts[n] / (med[n] * 1e-3) / HBM_PEAK for n in byts},
        "hbm_peak_bytes_per_s": HBM_PEAK,
    }
    out = pathlib.Path(a.out)
    os.makedirs(out.parent, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k2: res[k2] for k2 in ("ratio_track_over_search", "ratio_spread",
                                            "fraction_of_hbm_peak")}))
    print(json.dumps({n: med[n] for n in med}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
