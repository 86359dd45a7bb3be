"""The RGB-D glue compiled: orbx_glue::ComputeStereoFromRGBD (integration/orbx_slam2_glue.h,
replacing Frame::ComputeStereoFromRGBD, Frame.cc:689-710, and Tracking.cc:244-245's convertTo)
built by g++ into tests/native/rgbd_test.cpp with the cv stand-in headers and the Frame stand-in
of tests/native/rgbd_standin.h.

* CPU: the program compiles with -Wall -Wextra and, on a host without a GPU, the glue throws
  std::runtime_error naming the failing call.
* GPU: directed depth cases (tests/rgbd_cases.py) through the glue, a CV_32F cv::Mat header over
  padded rows and a raw 16-bit image: mvuRight / mvDepth equal the numpy restatement bit for bit,
  and the program's own run of the reference's statements agrees."""
import subprocess

import numpy as np
import pytest

import rgbd_cases as rc
from my_orb_slam2_amd.features import DEPTH_F32, DEPTH_U16


@pytest.fixture(scope="module")
def rgbd_bin(orbx_lib):
    from my_orb_slam2_amd import build as b
    return b.build_rgbd_test()


def test_rgbd_glue_fails_loudly_without_gpu(rgbd_bin):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([str(rgbd_bin), "nogpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orbx_compute_stereo_from_rgbd" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("depth_type,factor", [(DEPTH_U16, "tum"), (DEPTH_F32, "one+5e-6"),
                                               (DEPTH_F32, "one+2e-5")])
def test_rgbd_glue(rgbd_bin, gpu, tmp_path, depth_type, factor):
    c = rc.depth_case(17, depth_type, factor, 257)
    n = len(c["kps"])
    c["alloc"].tofile(tmp_path / "depth.raw")
    c["kps"].tofile(tmp_path / "kps.bin")
    c["kps_un"].tofile(tmp_path / "kps_un.bin")
    (tmp_path / "params.txt").write_text(
        f"{rc.W} {rc.H} {depth_type} {c['row_stride']} {c['alloc'].shape[0]} "
        f"{float(c['factor']).hex()} {float(c['mbf']).hex()} {n}\n")
    r = subprocess.run([str(rgbd_bin), "run", str(tmp_path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ur = np.fromfile(tmp_path / "uRight.bin", np.float32)
    de = np.fromfile(tmp_path / "depth.bin", np.float32)
    ur_o, de_o = rc.compute_stereo_from_rgbd(c["img"], depth_type, c["factor"], c["mbf"],
                                             c["kps"], c["kps_un"])
    assert np.array_equal(ur.view(np.uint32), ur_o.view(np.uint32))
    assert np.array_equal(de.view(np.uint32), de_o.view(np.uint32))
    assert f"n {n} valid {int((de_o > 0).sum())} " in r.stdout and " bad 0" in r.stdout
