"""The output-block layouts of the extractor (csrc/orbx_layout.h) on their own: every offset equal
to the expression the host code spelled out at each use before, no overlap, every part 256-aligned,
and k_octree's LDS carve (OctreeCarve) equal to the size the host computed and the offsets the kernel
took before the two shared it, in a stand-alone program built with -fsanitize=address,undefined
(tests/native/layout_test.cpp).  No GPU and no liborbx."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def layout_test():
    from my_orb_slam2_amd import build as b
    return b.build_layout_test()


def test_output_block_layouts(layout_test):
    r = subprocess.run([str(layout_test)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    for name in ("keypoint_size", "workspace", "stereo_one_pair", "stereo_batch", "server",
                 "octree_carve"):
        assert "ok " + name in lines, r.stdout
    assert lines[-2] == "all ok" and not r.stderr
