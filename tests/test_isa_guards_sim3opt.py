"""Guards on the gfx950 code of k_sim3_opt (CPU only, with the helpers of tests/test_isa_guards.py:
tools/isa_dump.py on the built library): no flat (generic address space) load, store or atomic; no
scratch (private segment): the estimate, the Levenberg state and both edges' Jacobians stay in
registers; and denormals kept in every precision, since the restatements it is compared with run
on x86-64."""
import pathlib
import re
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import isa_dump  # noqa: E402

LIB = ROOT / "my_orb_slam2_amd" / "liborbx.so"
KERNELS = ("k_sim3_opt",)


def _need_tools():
    if not LIB.exists() or not isa_dump.available():
        pytest.skip("liborbx.so or the LLVM tools are missing")


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_has_no_flat_memory_ops(orbx_lib, tmp_path, kernel):
    _need_tools()
    funcs = {n: b for n, b in isa_dump.kernels(LIB, tmp_path).items() if kernel in n}
    assert funcs, f"{kernel} not found in any code object"
    for n, body in funcs.items():
        bad = [l for l in body if re.search(r"\bflat_(load|store|atomic)", l)]
        assert not bad, (n, bad[:4])
        assert not [l for l in body if l.startswith("scratch_")], n
        assert any(l.startswith("global_") for l in body), n


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_uses_no_scratch_and_keeps_denormals(orbx_lib, tmp_path, kernel):
    _need_tools()
    kd = {n: d for n, d in isa_dump.descriptors(LIB, tmp_path).items() if kernel in n}
    assert kd, f"{kernel}'s kernel descriptor not found"
    for n, d in kd.items():
        assert d.get(".amdhsa_private_segment_fixed_size") == "0", (n, d)
        assert d.get(".amdhsa_enable_private_segment", "0") == "0", (n, d)
        assert d.get(".amdhsa_float_denorm_mode_32") == "3", (n, d)
        assert d.get(".amdhsa_float_denorm_mode_16_64") == "3", (n, d)
