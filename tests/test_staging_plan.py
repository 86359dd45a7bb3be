"""The staging plan of the host-array entry points (csrc/orbx_stage.h) on its own: alignment,
absent parts, the two spans, copy-out and block reuse, in a stand-alone program built with
-fsanitize=address,undefined (tests/native/staging_test.cpp).  No GPU and no liborbx."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def staging_test():
    from my_orb_slam2_amd import build as b
    return b.build_staging_test()


def test_staging_plan(staging_test):
    r = subprocess.run([str(staging_test)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    for name in ("alignment", "absent", "spans canonical", "spans shuffled", "spans", "copy_out",
                 "block_reuse"):
        assert "ok " + name in lines, r.stdout
    assert lines[-2] == "all ok" and not r.stderr
