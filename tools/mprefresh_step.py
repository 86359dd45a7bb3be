#!/usr/bin/env python3
"""Cost of the MapPoint refresh on the device (k_refresh_map_points) against what it replaces.

    python tools/mprefresh_step.py [--points 2000] [--out profiles/mprefresh_step.json]

--points MapPoints with 2 to 20 observations each over --keyframes keyframes (local mapping's
usual rows), a tenth of the keyframes bad, every point refreshed with both parts (max_obs 32).
One process alternates

  device   orbx_refresh_map_points_batch_device, device events around a window of calls
  parent   the parent commit's route, wall clock: the descriptor rows of the keyframes that are not
           bad gathered on the host in kf_order (numpy fancy indexing), uploaded,
           orbx_compute_distinctive_descriptors_device, the indices back, the chosen rows copied
           on the host and the descriptors and records uploaded; the normal and the depth range by
           the per-point numpy restatement of tests/mprefresh_cases.py (reported on its own: it is
           Python, not what a C++ caller pays)
  one_core tests/native/mprefresh_ref --time: both reference functions on the objects, one core

The device's records and descriptors are checked against mprefresh_ref's before anything is timed.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import pathlib
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

MAX_OBS = 32


def scene(n_mp: int, n_kf: int, seed: int = 0):
    import mprefresh_cases as mc
    rng = np.random.RandomState(seed)
    rows = [list(rng.permutation(n_kf)[:rng.randint(2, 21)]) for _ in range(n_mp)]
    bad = list(rng.permutation(n_kf)[:n_kf // 10])
    return mc.snapshot(n_kf, rows, seed=seed, bad_kf=bad)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--keyframes", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds per timed window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mprefresh_step.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("mprefresh_step: no GPU visible; nothing measured", file=sys.stderr)
        return 2
    import mprefresh_cases as mc
    from my_orb_slam2_amd import ORBmatcher, build as b
    from my_orb_slam2_amd._lib import check, ptr
    from my_orb_slam2_amd.localmap import LocalMapView, refresh_map_points
    dev = torch.device("cuda", 0)
    S = scene(a.points, a.keyframes)
    n_mp = S["n_mp"]
    ids = np.arange(n_mp, dtype=np.int32)
    view = LocalMapView({k: S[k] for k in mc.ARRAYS}).set_refresh_inputs({k: S[k] for k in mc.EXTRA})
    d_ids = torch.from_numpy(ids).to(dev)
    d_rec = torch.from_numpy(S["mp_rec"].view(np.uint8).reshape(-1).copy()).to(dev)
    d_desc = torch.from_numpy(S["mp_desc"].copy()).to(dev)
    d_info = torch.zeros(n_mp, dtype=torch.int32, device=dev)

    def device():
        refresh_map_points(view, d_ids, mc.BOTH, MAX_OBS, d_desc, d_info, d_mp_rec=d_rec)

    device()
    torch.cuda.synchronize()
    info = d_info.cpu().numpy()
    assert set(info.tolist()) <= {0, mc.DESC_KEPT}, sorted(set(info.tolist()))

    # one core, and its results against the device's
    c = mc.case("step", S, ids=ids)
    exe = b.build_mprefresh_ref()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        mc.write_cases(tmp / "cases.bin", [c])
        us = []
        for _ in range(3):
            out = subprocess.run([str(exe), str(tmp / "cases.bin"), str(tmp / "out.bin"), "--time", "10"],
                                 check=True, capture_output=True, text=True).stdout
            us.append(float(re.search(r"([0-9.]+) us per call", out).group(1)))
        ref = mc.read_results(tmp / "out.bin", [c])[0]
    got_rec = d_rec.cpu().numpy().view(mc.MAP_POINT_DTYPE)
    agree = mc.same_records(got_rec, ref["rec"]) and \
        d_desc.cpu().numpy().tobytes() == ref["desc"].tobytes()
    assert agree, "the device differs from tests/native/mprefresh_ref"

    # the parent's route for the descriptors
    m = ORBmatcher(0.6, False)
    rank = S["kf_order"][S["mp_obs"]]
    owner = np.repeat(np.arange(n_mp), np.diff(S["mp_obs_off"]))
    src = S["kf_mp_off"][S["mp_obs"]] + S["mp_obs_feat"]
    cap = int(np.diff(S["mp_obs_off"]).sum())
    h_rows = torch.empty((cap, 32), dtype=torch.uint8).pin_memory()
    h_off = torch.empty(n_mp + 1, dtype=torch.int32).pin_memory()
    h_best = torch.empty(n_mp, dtype=torch.int32).pin_memory()
    h_desc = torch.from_numpy(S["mp_desc"].copy()).pin_memory()
    h_rec = torch.from_numpy(S["mp_rec"].view(np.uint8).reshape(-1).copy()).pin_memory()
    d_rows = torch.empty((cap, 32), dtype=torch.uint8, device=dev)
    d_off = torch.empty(n_mp + 1, dtype=torch.int32, device=dev)
    d_best = torch.empty(n_mp, dtype=torch.int32, device=dev)
    d_desc2, d_rec2 = torch.empty_like(d_desc), torch.empty_like(d_rec)
    parts = {"gather": [], "copies_and_kernel": [], "pick": [], "upload": []}

    def parent():
        t0 = time.perf_counter()
        keep = np.flatnonzero(S["kf_bad"][S["mp_obs"]] == 0)
        order = keep[np.lexsort((rank[keep], owner[keep]))]        # per point, by kf_order
        n = len(order)
        np.take(S["kf_desc"], src[order], axis=0, out=h_rows.numpy()[:n])
        off = h_off.numpy()
        off[0] = 0
        np.cumsum(np.bincount(owner[order], minlength=n_mp), out=off[1:])
        t1 = time.perf_counter()
        d_rows[:n].copy_(h_rows[:n], non_blocking=True)
        d_off.copy_(h_off, non_blocking=True)
        check("orbx_compute_distinctive_descriptors_device",
              m._lib.orbx_compute_distinctive_descriptors_device(
                  m._h, ptr(d_rows), ptr(d_off), n_mp, ptr(d_best),
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        h_best.copy_(d_best, non_blocking=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        best = h_best.numpy()
        has = best >= 0
        h_desc.numpy()[has] = h_rows.numpy()[off[:-1][has] + best[has]]
        t3 = time.perf_counter()
        d_desc2.copy_(h_desc, non_blocking=True)
        d_rec2.copy_(h_rec, non_blocking=True)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            parts[k].append(v * 1e3)

    parent()
    assert h_desc.numpy().tobytes() == ref["desc"].tobytes(), "the parent's route differs"

    t0 = time.perf_counter()
    nd = mc.refresh_np(S, ids, mc.NORMAL_DEPTH, MAX_OBS)
    numpy_nd_ms = (time.perf_counter() - t0) * 1e3
    assert mc.same_records(nd["rec"], ref["rec"])

    def window_events(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            device()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    for _ in range(a.warmup):
        device()
        parent()
    torch.cuda.synchronize()
    steps = max(3, math.ceil(a.window * 1e3 / max(window_events(5), 1e-3)))
    for v in parts.values():
        v.clear()
    dev_ms = []
    for _ in range(a.repeats):                               # alternate within every repeat
        dev_ms.append(window_events(steps))
        for _ in range(5):
            parent()
    med = lambda v: float(np.median(v))
    pp = {n: {"median": med(v), "min": float(min(v)), "max": float(max(v))} for n, v in parts.items()}
    parent_desc = sum(v["median"] for v in pp.values())
    nobs = np.diff(S["mp_obs_off"])
    out = {
        "tool": "tools/mprefresh_step.py", "device": torch.cuda.get_device_name(0),
        "timing": "device events around `steps` calls (device); wall clock per part (parent); "
                  "tests/native/mprefresh_ref --time 10 on one core, median of 3 runs (one_core); "
                  "one wall-clock run (numpy normal / depth)",
        "settings": {"points": n_mp, "keyframes": a.keyframes, "observations": int(nobs.sum()),
                     "obs_per_point": {"min": int(nobs.min()), "max": int(nobs.max()),
                                       "mean": float(nobs.mean())},
                     "max_obs": MAX_OBS, "steps": steps, "repeats": a.repeats},
        "device_ms_per_call": {"median": med(dev_ms), "min": float(min(dev_ms)),
                               "max": float(max(dev_ms)), "repeats": [float(v) for v in dev_ms]},
        "one_core_ms_per_call": {"median": med(us) * 1e-3, "runs": [u * 1e-3 for u in us]},
        "parent_descriptor_route_ms_per_call": {"total": parent_desc, **pp},
        "parent_numpy_normal_depth_ms": numpy_nd_ms,
        "equals_mprefresh_ref": bool(agree),
    }
    p = pathlib.Path(a.out)
    os.makedirs(p.parent, exist_ok=True)
    p.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: out[k] for k in ("device_ms_per_call", "one_core_ms_per_call",
                                          "parent_descriptor_route_ms_per_call",
                                          "parent_numpy_normal_depth_ms")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
