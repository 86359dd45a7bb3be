"""k_fast's 4-pixel compass pre-test (csrc/orbx_fast_pretest.h) on its own: for every threshold
and every byte pair the flag equals the 7-bit closed form and covers the exact compass test, and
no byte's flag depends on its neighbours in the dword, in a stand-alone program built with
-fsanitize=address,undefined (tests/native/fast_pretest_test.cpp).  No GPU and no liborbx."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def fast_pretest_test():
    from my_orb_slam2_amd import build as b
    return b.build_fast_pretest_test()


def test_fast_pretest(fast_pretest_test):
    r = subprocess.run([str(fast_pretest_test)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    for name in ("gather", "all_byte_pairs", "no_byte_crossing", "unit4", "unit2", "unit1"):
        assert "ok " + name in lines, r.stdout
    assert lines[-2] == "all ok" and not r.stderr
