"""Guards on k_refresh_map_points' gfx950 code (CPU only, with the helpers of
tests/test_isa_guards.py: tools/isa_dump.py on the built library): no scratch (private segment),
denormals kept in both precisions, since the restatement it is compared with runs on x86-64, and no
flat (generic address space) load, store or atomic."""
import pathlib
import re
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import isa_dump  # noqa: E402

LIB = ROOT / "my_orb_slam2_amd" / "liborbx.so"
KERNEL = "k_refresh_map_points"


def _need_tools():
    if not LIB.exists() or not isa_dump.available():
        pytest.skip("liborbx.so or the LLVM tools are missing")


def test_k_refresh_map_points_uses_no_scratch_and_keeps_denormals(orbx_lib, tmp_path):
    _need_tools()
    kd = {n: d for n, d in isa_dump.descriptors(LIB, tmp_path).items() if KERNEL in n}
    assert kd, f"{KERNEL}'s kernel descriptor not found"
    for n, d in kd.items():
        assert d.get(".amdhsa_private_segment_fixed_size") == "0", (n, d)
        assert d.get(".amdhsa_float_denorm_mode_32") == "3", (n, d)
        assert d.get(".amdhsa_float_denorm_mode_16_64") == "3", (n, d)


def test_k_refresh_map_points_has_no_flat_memory_ops(orbx_lib, tmp_path):
    _need_tools()
    funcs = {n: b for n, b in isa_dump.kernels(LIB, tmp_path).items() if KERNEL in n}
    assert funcs, f"{KERNEL} not found in any code object"
    for n, body in funcs.items():
        bad = [l for l in body if re.search(r"\bflat_(load|store|atomic)", l)]
        assert not bad, (n, bad[:4])
