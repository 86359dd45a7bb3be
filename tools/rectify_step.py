#!/usr/bin/env python3
"""Cost of rectifying raw stereo pairs on the device, next to the stereo step it precedes.

    python tools/rectify_step.py [--batch 512] [--out profiles/rectify_step.json]

EuRoC settings (752x480, the maps of tests/golden/euroc_stereo.yaml, 1200 features), B pairs per
step.  One process alternates

  remap      orbx_remap_stereo_batch_device   both views of B raw pairs into the level-0 slots
  stereo     StereoBatch.run_resident         the stereo front-end on already rectified inputs
  rectified  RectifiedStereoBatch.__call__    the remap + the stereo front-end

each timed with device events over a window of `steps` calls (sized from a calibration step so
that a window lasts about --window seconds), `--repeats` windows each, alternating.  The JSON holds
the per-step times (median over the repeats and their spread), the remap's GB/s against its
algorithmic bytes (1 B read + 1 B written per pixel + the 8-byte map entry once per chunk of
images) and the ratio rectified / stereo.  The stereo line is the code of the parent commit: the
remap adds a stage in front of it and changes nothing in it.
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

NFEATURES = 1200
MAP_ENTRY_BYTES = 8


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic pairs, tiled")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--settings", default=str(ROOT / "tests" / "golden" / "euroc_stereo.yaml"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rectify_step.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("rectify_step: no GPU visible; nothing measured", file=sys.stderr)
        return 2
    import my_orb_slam2_amd as m
    from my_orb_slam2_amd import rectify, synth

    dev = torch.device("cuda", 0)
    s = m.load_stereo_settings(a.settings)
    W, H = s["left"]["width"], s["left"]["height"]
    maps = [m.init_undistort_rectify_map(c["K"], c["D"], c["R"], c["P"], W, H)
            for c in (s["left"], s["right"])]
    rl, rr = m.Rectifier(*maps[0]), m.Rectifier(*maps[1])
    B = a.batch
    k = min(a.distinct, B)
    pairs = [synth.stereo_pair(900 + i, W, H) for i in range(k)]
    idx = np.arange(B) % k
    rawL = torch.from_numpy(np.stack([p[0] for p in pairs])[idx]).to(dev)
    rawR = torch.from_numpy(np.stack([p[1] for p in pairs])[idx]).to(dev)
    mbf = float(s["bf"])
    mb = float(np.float32(s["bf"]) / np.float32(s["fx"]))

    rect = m.RectifiedStereoBatch(B, rl, rr, nfeatures=NFEATURES)
    plain = m.StereoBatch(B, nfeatures=NFEATURES)
    dl, dr = rect.input_views(W, H)
    pl, pr = plain.input_views(W, H)
    m.remap_stereo_batch_device(rl, rr, rawL, rawR, pl, pr)      # same-size rectified inputs
    torch.cuda.synchronize()

    work = {"remap": lambda: m.remap_stereo_batch_device(rl, rr, rawL, rawR, dl, dr),
            "stereo": lambda: plain.run_resident(mbf, mb),
            "rectified": lambda: rect(rawL, rawR, mbf, mb)}

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
    med = {n: float(np.median(t)) for n, t in times.items()}
    chunk = rectify.images_per_chunk()
    nimg = 2 * B
    nchunks = 2 * math.ceil(B / chunk)
    algo_bytes = nimg * W * H * 2 + nchunks * W * H * MAP_ENTRY_BYTES
    res = {
        "tool": "tools/rectify_step.py", "device": torch.cuda.get_device_name(0),
        "settings": {"width": W, "height": H, "nfeatures": NFEATURES, "pairs": B,
                     "distinct_pairs": k, "images_per_chunk": chunk, "steps": steps,
                     "repeats": a.repeats, "timing": "device events around `steps` calls"},
        "ms_per_step": {n: {"median": med[n], "min": float(min(t)), "max": float(max(t)),
                            "repeats": [float(v) for v in t]} for n, t in times.items()},
        "remap_algorithmic_bytes": algo_bytes,
        "remap_gb_per_s": algo_bytes / (med["remap"] * 1e-3) / 1e9,
        "remap_pairs_per_s": B / (med["remap"] * 1e-3),
        "stereo_pairs_per_s": B / (med["stereo"] * 1e-3),
        "rectified_pairs_per_s": B / (med["rectified"] * 1e-3),
        "ratio_rectified_over_stereo": med["rectified"] / med["stereo"],
        "ratio_spread": [min(r / q for r, q in zip(times["rectified"], times["stereo"])),
                         max(r / q for r, q in zip(times["rectified"], times["stereo"]))],
        "ratio_remap_over_stereo": med["remap"] / med["stereo"],
    }
    out = pathlib.Path(a.out)
    os.makedirs(out.parent, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k2: res[k2] for k2 in ("remap_gb_per_s", "ratio_rectified_over_stereo",
                                            "ratio_remap_over_stereo", "ratio_spread")}
                     | {"ms": med}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
