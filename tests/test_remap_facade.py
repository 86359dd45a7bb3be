"""The rectifier glue compiled: orbx_glue::Rectifier (integration/orbx_slam2_glue.h, replacing the
per-frame cv::remap of Examples/Stereo/stereo_euroc.cc:136-137) built by g++ with -Wall -Wextra
into tests/native/remap_test.cpp with the cv stand-in headers.

* CPU: the program compiles and, on a host without a GPU, the glue throws std::runtime_error
  naming the failing call.
* GPU: one case with padded source and destination rows through cv::Mat headers equals the numpy
  restatement ``remap_closed`` bit for bit, the padding bytes intact."""
import subprocess

import numpy as np
import pytest

import remap_cases as rc


@pytest.fixture(scope="module")
def remap_bin(orbx_lib):
    from my_orb_slam2_amd import build as b
    return b.build_remap_test()


def test_remap_glue_fails_loudly_without_gpu(remap_bin):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([str(remap_bin), "nogpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orbx_rectifier_create" in r.stdout


@pytest.mark.gpu
def test_remap_glue(remap_bin, gpu, tmp_path):
    rng = np.random.default_rng(5)
    sw, sh, dw, dh, sstep, dstep = 37, 11, 65, 9, 41, 71
    src = rng.integers(1, 256, (sh, sstep), dtype=np.uint8)
    m1 = rng.uniform(-1.5, sw + 0.5, (dh, dw)).astype(np.float32)
    m2 = rng.uniform(-1.5, sh + 0.5, (dh, dw)).astype(np.float32)
    dst = np.full((dh, dstep), rc.SENTINEL, np.uint8)
    src.tofile(tmp_path / "src.raw")
    m1.tofile(tmp_path / "map1.bin")
    m2.tofile(tmp_path / "map2.bin")
    dst.tofile(tmp_path / "dst.raw")
    (tmp_path / "params.txt").write_text(f"{sw} {sh} {sstep} {dw} {dh} {dstep}\n")
    r = subprocess.run([str(remap_bin), "run", str(tmp_path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " bad 0" in r.stdout
    got = np.fromfile(tmp_path / "dst.raw", np.uint8).reshape(dh, dstep)
    want = dst.copy()
    want[:, :dw] = rc.remap_closed(src[None, :, :sw], m1, m2)[0]
    assert np.array_equal(got, want)
