"""Guards on k_remap's gfx950 code (CPU only, with the helpers of tests/test_isa_guards.py:
tools/isa_dump.py on the built library): no flat (generic address space) load, store or atomic,
and no scratch (private segment): the lane's map entries and offsets stay in registers."""
import pathlib
import re
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import isa_dump  # noqa: E402

LIB = ROOT / "my_orb_slam2_amd" / "liborbx.so"


def _need_tools():
    if not LIB.exists() or not isa_dump.available():
        pytest.skip("liborbx.so or the LLVM tools are missing")


def test_k_remap_has_no_flat_memory_ops(orbx_lib, tmp_path):
    _need_tools()
    funcs = {n: b for n, b in isa_dump.kernels(LIB, tmp_path).items() if "k_remap" in n}
    assert funcs, "k_remap not found in any code object"
    for n, body in funcs.items():
        bad = [l for l in body if re.search(r"\bflat_(load|store|atomic)", l)]
        assert not bad, (n, bad[:4])
        assert not [l for l in body if l.startswith("scratch_")], n
        assert any(l.startswith("global_load_ubyte") for l in body), n


def test_k_remap_uses_no_scratch(orbx_lib, tmp_path):
    _need_tools()
    kd = {n: d for n, d in isa_dump.descriptors(LIB, tmp_path).items() if "k_remap" in n}
    assert kd, "k_remap's kernel descriptor not found"
    for n, d in kd.items():
        assert d.get(".amdhsa_private_segment_fixed_size") == "0", (n, d)
        assert d.get(".amdhsa_enable_private_segment", "0") == "0", (n, d)
