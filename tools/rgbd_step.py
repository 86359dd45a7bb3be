#!/usr/bin/env python3
"""Cost of the RGB-D front-end next to the monocular one it extends, on the GPU.

    python tools/rgbd_step.py [--batch 256] [--out profiles/rgbd_step.json]

TUM settings (640x480, 1000 features, fr1 camera), B frames per step.  One process alternates

  mono    MonoTrackBatch.frames           extraction, undistortion, grid
  rgbd    RGBDTrackBatch.frames           extraction, undistortion fused with the depth sampling
                                          (k_rgbd_depth), grid
  close   RGBDTrackBatch.close_points     the depth sort and unprojection (k_close_points)

each timed with device events over a window of `steps` calls (sized from a calibration step so
that a window lasts about --window seconds), `--repeats` windows each, alternating.  The JSON
holds the per-step times (median over the repeats and their spread), the ratios, and the bytes
the depth stage reads per frame computed from the shapes: the reference's whole-image convertTo
against one 64-byte sector per sampled keypoint.
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

W, H, NFEATURES = 640, 480, 1000
TUM1_K4 = (517.306408, 516.469215, 318.643040, 255.313989)
TUM1_DIST = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
MBF, DEPTH_FACTOR, TH_DEPTH = 40.0, 1.0 / 5000.0, 40.0 * 40.0 / 517.306408   # TUM1.yaml


def depth_map(seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    z = 2.5 + 1.8 * np.sin(xx / 97.0 + seed) + 1.5 * np.cos(yy / 61.0) + rng.uniform(0, 0.02, (H, W))
    d = np.clip(z * 5000.0, 2000, 40000).astype(np.uint16)
    for _ in range(12):
        x0, y0 = int(rng.integers(0, W - 80)), int(rng.integers(0, H - 60))
        d[y0:y0 + int(rng.integers(10, 60)), x0:x0 + int(rng.integers(10, 80))] = 0
    return d


def bytes_per_frame(nkp: float) -> dict:
    """What the depth stage reads per frame, from the shapes."""
    return {"convert_whole_image": W * H * (2 + 4),     # u16 read + f32 written, then sampled
            "sampled_sectors": int(round(nkp)) * 64,      # one 64-byte sector per keypoint
            "keypoints": float(nkp)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16, help="distinct synthetic frames, tiled")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rgbd_step.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("rgbd_step: no GPU visible; nothing measured", file=sys.stderr)
        return 2
    import my_orb_slam2_amd as m
    from my_orb_slam2_amd import synth
    from my_orb_slam2_amd.features import FRAME_POSE_DTYPE, frame_pose

    dev = torch.device("cuda", 0)
    B = a.batch
    k = min(a.distinct, B)
    imgs = np.stack([synth.frame(900 + i, W, H) for i in range(k)])
    deps = np.stack([depth_map(i) for i in range(k)])
    idx = np.arange(B) % k
    d_imgs = torch.from_numpy(imgs[idx]).to(dev)
    d_depth = torch.from_numpy(deps[idx].view(np.int16)).to(dev)
    kw = dict(nfeatures=NFEATURES)
    mono = m.MonoTrackBatch(B, W, H, TUM1_K4, TUM1_DIST, **kw)
    rgbd = m.RGBDTrackBatch(B, W, H, TUM1_K4, TUM1_DIST, MBF, depth_factor=DEPTH_FACTOR,
                            th_depth=TH_DEPTH, **kw)
    pose = frame_pose(np.eye(3), np.zeros(3), TUM1_K4, rgbd.bounds, 1.2 ** np.arange(8), mbf=MBF)
    poses = np.repeat(pose.reshape(1), B).astype(FRAME_POSE_DTYPE)
    d_poses = torch.from_numpy(poses.view(np.uint8).reshape(-1).copy()).to(dev)

    work = {"mono": lambda: mono.frames(d_imgs),
            "rgbd": lambda: rgbd.frames(d_imgs, d_depth),
            "close": lambda: rgbd.close_points(d_poses)}

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
        steps[name] = max(5, math.ceil(a.window * 1e3 / max(window(fn, 3), 1e-3)))
    times = {name: [] for name in work}
    for _ in range(a.repeats):
        for name, fn in work.items():        # alternate within every repeat
            times[name].append(window(fn, steps[name]))
    nkp, _, _ = rgbd.fetch_undistorted()
    counts = rgbd.counts.cpu().numpy()
    med = {n: float(np.median(t)) for n, t in times.items()}
    res = {
        "tool": "tools/rgbd_step.py", "device": torch.cuda.get_device_name(0),
        "settings": {"width": W, "height": H, "nfeatures": NFEATURES, "batch": B,
                     "depth": "u16, factor 1/5000", "distinct_frames": k, "steps": steps,
                     "repeats": a.repeats, "timing": "device events around `steps` calls"},
        "ms_per_step": {n: {"median": med[n], "min": float(min(t)), "max": float(max(t)),
                            "repeats": [float(v) for v in t]} for n, t in times.items()},
        "ratio_rgbd_over_mono": med["rgbd"] / med["mono"],
        "ratio_rgbd_plus_close_over_mono": (med["rgbd"] + med["close"]) / med["mono"],
        "ratio_spread": [min(r / q for r, q in zip(times["rgbd"], times["mono"])),
                         max(r / q for r, q in zip(times["rgbd"], times["mono"]))],
        "mean_keypoints": float(nkp.mean()),
        "mean_close_counts_M_V": [float(counts[:, 0].mean()), float(counts[:, 1].mean())],
        "depth_stage_bytes_per_frame": bytes_per_frame(float(nkp.mean())),
    }
    out = pathlib.Path(a.out)
    os.makedirs(out.parent, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k2: res[k2] for k2 in ("ratio_rgbd_over_mono",
                                            "ratio_rgbd_plus_close_over_mono", "ratio_spread")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
