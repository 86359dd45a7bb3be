"""Build liborbx.so (the HIP kernels + C ABI) in-tree for gfx950.

    python -m my_orb_slam2_amd.build        # or __graft_entry__.build()

hipcc cross-compiles for gfx950 without a GPU.  The .so lands next to this file so it
travels with the repo snapshot to the GPU box (it is git-ignored, not gpurun-ignored).

Staleness is decided by content, not by file times: the build embeds a hash of every source
and header (``orbx-src:<hash>`` in the binary, also reported by ``orbx_version()``), and a
library whose embedded hash differs from the tree's is rebuilt.  A snapshot copied to another
machine keeps a fresh library fresh whatever the copy does to modification times.
"""
from __future__ import annotations

import hashlib
import os
import pathlib
import subprocess
import sys

PKG = pathlib.Path(__file__).resolve().parent
CSRC = PKG / "csrc"
LIB = PKG / "liborbx.so"
SOURCES = ["orbx_pyramid.hip", "orbx_extract.hip", "orbx_stereo.hip", "orbx_match.hip",
           "orbx_capi.hip", "orbx_match_capi.hip", "orbx_vocab.hip", "orbx_frame.hip",
           "orbx_kfdb.hip", "orbx_bf.hip", "orbx_rectify.hip", "orbx_triangulate.hip",
           "orbx_poseopt.hip", "orbx_sim3.hip", "orbx_sim3opt.hip", "orbx_pnp.hip"]
HEADERS = ["orbx_internal.h", "orbx_device.h", "orbx_math.h", "orbx_hypot.h", "orbx_kernels.h",
           "orbx_host.h", "orbx_match_kernels.h", "orbx_pattern.inc", "../../include/orbx.h",
           "../../include/orbx_match.h", "../../include/orbx_vocab.h", "../../include/orbx_frame.h",
           "../../include/orbx_kfdb.h"]
HASH_TAG = b"orbx-src:"

# -ffp-contract=off: every float a*b+c in the path is two roundings, as in the x86 reference
# (hipcc defaults to fast contraction).  No -ffast-math: IEEE division/rounding throughout.
# -amdgpu-mfma-vgpr-form: MFMA accumulators in VGPRs (k_bf_mfma's 16-bit keys are read by
# VALU min / max straight from them; in AGPRs each read costs a v_accvgpr_read).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
         "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
         "-mllvm", "-amdgpu-mfma-vgpr-form",
         "-I" + str(PKG.parent / "include")]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if cand and pathlib.Path(cand).exists():
            return cand
    return "hipcc"


def source_hash(extra_flags=()) -> str:
    """16 hex digits over the sources, headers and compile flags of the library."""
    h = hashlib.sha256()
    for name in SOURCES + HEADERS:
        p = CSRC / name
        h.update(name.encode() + b"\0")
        h.update(p.read_bytes() if p.exists() else b"<missing>")
    h.update(" ".join(FLAGS[:-1] + list(extra_flags)).encode())
    return h.hexdigest()[:16]


def embedded_hash(path: pathlib.Path = LIB) -> str | None:
    """The source hash a built library carries, or None."""
    try:
        data = path.read_bytes()
    except OSError:
        return None
    i = data.find(HASH_TAG)
    if i < 0:
        return None
    return data[i + len(HASH_TAG):i + len(HASH_TAG) + 16].decode("ascii", "replace")


def stale() -> bool:
    return embedded_hash() != source_hash()


def build(force: bool = False, verbose: bool = False, extra_flags=(),
          out: pathlib.Path | None = None) -> pathlib.Path:
    """Compile the library (if stale, or always with force).  `extra_flags` / `out` build a
    tuning variant (tools/variants.py) next to the product library."""
    target = pathlib.Path(out) if out else LIB
    if extra_flags and target.resolve() == LIB.resolve():
        # the product library is the sources as they are: no variant or diagnostic switches
        raise ValueError(f"refusing to build {LIB.name} with extra flags {list(extra_flags)}")
    digest = source_hash(extra_flags)
    if not force and embedded_hash(target) == digest:
        return target
    srcs = [str(CSRC / s) for s in SOURCES if (CSRC / s).exists()]
    cmd = ([hipcc()] + FLAGS + list(extra_flags) + [f'-DORBX_SRC_HASH="{digest}"'] + srcs +
           ["-o", str(target) + ".tmp"])
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(target) + ".tmp", target)
    return target


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
    print(LIB, source_hash())


# ---- the C++ boundary consumer (tests/native/boundary_test.cpp) -------------------------------
BOUNDARY_SRC = PKG.parent / "tests" / "native" / "boundary_test.cpp"
BOUNDARY_BIN = PKG.parent / "tests" / "native" / "boundary_test"


def build_boundary_test(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ against include/orbx*.h only, linked to the in-tree liborbx.so (found at run time
    through the binary's RUNPATH, $ORIGIN-relative, so the tree can move)."""
    hdrs = sorted((PKG.parent / "include").glob("*.h"))
    newest = max([BOUNDARY_SRC.stat().st_mtime] + [h.stat().st_mtime for h in hdrs])
    if not force and BOUNDARY_BIN.exists() and BOUNDARY_BIN.stat().st_mtime >= newest:
        return BOUNDARY_BIN
    build(verbose=verbose)
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I" + str(PKG.parent / "include"),
           str(BOUNDARY_SRC), "-L" + str(PKG), "-lorbx", "-L/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,$ORIGIN/../../my_orb_slam2_amd",
           "-pthread", "-o", str(BOUNDARY_BIN) + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(BOUNDARY_BIN) + ".tmp", BOUNDARY_BIN)
    return BOUNDARY_BIN


# ---- the drop-in facade compiled as ORB-SLAM2 would include it (tests/native/facade_test.cpp) --
FACADE_SRC = PKG.parent / "tests" / "native" / "facade_test.cpp"
FACADE_BIN = PKG.parent / "tests" / "native" / "facade_test"


def build_facade_test(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on integration/ORBextractor.h + integration/orbx_slam2_glue.h with the cv stand-in
    headers of tests/native/cv_standin, linked to the in-tree liborbx.so."""
    root = PKG.parent
    deps = ([FACADE_SRC] + sorted((root / "include").glob("*.h")) +
            sorted((root / "integration").glob("*.h")) +
            sorted((root / "tests" / "native" / "cv_standin").rglob("*.hpp")))
    newest = max(p.stat().st_mtime for p in deps)
    if not force and FACADE_BIN.exists() and FACADE_BIN.stat().st_mtime >= newest:
        return FACADE_BIN
    build(verbose=verbose)
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + str(root / "include"),
           "-I" + str(root / "integration"), "-I" + str(root / "tests" / "native" / "cv_standin"),
           str(FACADE_SRC), "-L" + str(PKG), "-lorbx", "-L/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,$ORIGIN/../../my_orb_slam2_amd",
           "-pthread", "-o", str(FACADE_BIN) + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(FACADE_BIN) + ".tmp", FACADE_BIN)
    return FACADE_BIN


# ---- the ORBmatcher drop-in compiled as ORB-SLAM2 would include it (tests/native/matcher_test.cpp)
MATCHER_SRC = PKG.parent / "tests" / "native" / "matcher_test.cpp"
MATCHER_BIN = PKG.parent / "tests" / "native" / "matcher_test"
MATCHER_CPU_BIN = PKG.parent / "tests" / "native" / "matcher_test_cpu"


def build_matcher_test(force: bool = False, verbose: bool = False, cpu: bool = False) -> pathlib.Path:
    """g++ on integration/ORBmatcher.h with the ORB-SLAM2 stand-in classes
    (tests/native/slam2_standin) and the cv stand-in, plus the CPU restatement it is checked
    against (oracle/orb_matcher_objects.h).  cpu=False: linked to the in-tree liborbx.so (the
    searches run on the GPU).  cpu=True: matcher_test_cpu, linked instead to the C-ABI test
    double tests/native/oracle_abi.cpp over oracle/orb_matcher_oracle.cpp (no GPU, no liborbx),
    for the CPU test suite."""
    root = PKG.parent
    native = root / "tests" / "native"
    out = MATCHER_CPU_BIN if cpu else MATCHER_BIN
    deps = ([MATCHER_SRC, native / "oracle_abi.cpp", root / "oracle" / "orb_matcher_oracle.cpp",
             root / "oracle" / "orb_matcher_objects.h"] + sorted((root / "include").glob("*.h")) +
            sorted((root / "integration").glob("*.h")) +
            sorted((native / "cv_standin").rglob("*.hpp")) + sorted((native / "slam2_standin").glob("*.h")))
    newest = max(p.stat().st_mtime for p in deps)
    if not force and out.exists() and out.stat().st_mtime >= newest:
        return out
    # -ffp-contract=off: the facade's and the restatement's float expressions as written
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off",
           "-I" + str(root / "include"), "-I" + str(root / "integration"),
           "-I" + str(root / "oracle"), "-I" + str(native / "cv_standin"),
           "-I" + str(native / "slam2_standin"), str(MATCHER_SRC)]
    if cpu:
        cmd += [str(native / "oracle_abi.cpp"), str(root / "oracle" / "orb_matcher_oracle.cpp")]
    else:
        build(verbose=verbose)
        cmd += ["-L" + str(PKG), "-lorbx", "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib",
                "-Wl,-rpath,$ORIGIN/../../my_orb_slam2_amd"]
    cmd += ["-pthread", "-o", str(out) + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(out) + ".tmp", out)
    return out


# ---- the RGB-D glue compiled as ORB-SLAM2 would include it (tests/native/rgbd_test.cpp) ---------
RGBD_SRC = PKG.parent / "tests" / "native" / "rgbd_test.cpp"
RGBD_BIN = PKG.parent / "tests" / "native" / "rgbd_test"


def build_rgbd_test(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on integration/orbx_slam2_glue.h (ComputeStereoFromRGBD) with the cv stand-in and
    tests/native/rgbd_standin.h, linked to the in-tree liborbx.so."""
    root = PKG.parent
    native = root / "tests" / "native"
    deps = ([RGBD_SRC, native / "rgbd_standin.h"] + sorted((root / "include").glob("*.h")) +
            sorted((root / "integration").glob("*.h")) +
            sorted((native / "cv_standin").rglob("*.hpp")))
    newest = max(p.stat().st_mtime for p in deps)
    if not force and RGBD_BIN.exists() and RGBD_BIN.stat().st_mtime >= newest:
        return RGBD_BIN
    build(verbose=verbose)
    # -ffp-contract=off: the reference's float statements restated in the program, as written
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off",
           "-I" + str(root / "include"), "-I" + str(root / "integration"),
           "-I" + str(native / "cv_standin"), "-I" + str(native), str(RGBD_SRC), "-L" + str(PKG),
           "-lorbx", "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib",
           "-Wl,-rpath,$ORIGIN/../../my_orb_slam2_amd", "-pthread", "-o", str(RGBD_BIN) + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(RGBD_BIN) + ".tmp", RGBD_BIN)
    return RGBD_BIN


# ---- the rectifier glue compiled as ORB-SLAM2 would include it (tests/native/remap_test.cpp) ----
REMAP_SRC = PKG.parent / "tests" / "native" / "remap_test.cpp"
REMAP_BIN = PKG.parent / "tests" / "native" / "remap_test"


def build_remap_test(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on integration/orbx_slam2_glue.h (orbx_glue::Rectifier) with the cv stand-in, linked to
    the in-tree liborbx.so."""
    root = PKG.parent
    native = root / "tests" / "native"
    deps = ([REMAP_SRC] + sorted((root / "include").glob("*.h")) +
            sorted((root / "integration").glob("*.h")) +
            sorted((native / "cv_standin").rglob("*.hpp")))
    newest = max(p.stat().st_mtime for p in deps)
    if not force and REMAP_BIN.exists() and REMAP_BIN.stat().st_mtime >= newest:
        return REMAP_BIN
    build(verbose=verbose)
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off",
           "-I" + str(root / "include"), "-I" + str(root / "integration"),
           "-I" + str(native / "cv_standin"), str(REMAP_SRC), "-L" + str(PKG),
           "-lorbx", "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib",
           "-Wl,-rpath,$ORIGIN/../../my_orb_slam2_amd", "-pthread", "-o", str(REMAP_BIN) + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(REMAP_BIN) + ".tmp", REMAP_BIN)
    return REMAP_BIN


# ---- the projection loops restated over the cv stand-in (tests/native/project_ref.cpp) ----------
PROJECT_REF_SRC = PKG.parent / "tests" / "native" / "project_ref.cpp"
PROJECT_REF_BIN = PKG.parent / "tests" / "native" / "project_ref"


def build_project_ref(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on the cv stand-in and the record layouts of include/orbx_frame.h only: no liborbx and
    no GPU (the CPU reference of orbx_project_map_points*)."""
    root = PKG.parent
    native = root / "tests" / "native"
    deps = ([PROJECT_REF_SRC] + sorted((root / "include").glob("*.h")) +
            sorted((native / "cv_standin").rglob("*.hpp")))
    newest = max(p.stat().st_mtime for p in deps)
    if not force and PROJECT_REF_BIN.exists() and PROJECT_REF_BIN.stat().st_mtime >= newest:
        return PROJECT_REF_BIN
    # -ffp-contract=off: the reference's float statements as written
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off",
           "-I" + str(root / "include"), "-I" + str(native / "cv_standin"),
           str(PROJECT_REF_SRC), "-o", str(PROJECT_REF_BIN) + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(PROJECT_REF_BIN) + ".tmp", PROJECT_REF_BIN)
    return PROJECT_REF_BIN


# ---- CreateNewMapPoints' loop restated over the cv stand-in (tests/native/triangulate_ref.cpp) ----
TRIANGULATE_REF_SRC = PKG.parent / "tests" / "native" / "triangulate_ref.cpp"
TRIANGULATE_REF_BIN = PKG.parent / "tests" / "native" / "triangulate_ref"


def build_triangulate_ref(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on the cv stand-in and the record layouts of include/ only: no liborbx and no GPU (the
    CPU reference of orbx_triangulate_matches*)."""
    root = PKG.parent
    native = root / "tests" / "native"
    deps = ([TRIANGULATE_REF_SRC] + sorted((root / "include").glob("*.h")) +
            sorted((native / "cv_standin").rglob("*.hpp")))
    newest = max(p.stat().st_mtime for p in deps)
    if (not force and TRIANGULATE_REF_BIN.exists() and
            TRIANGULATE_REF_BIN.stat().st_mtime >= newest):
        return TRIANGULATE_REF_BIN
    # -ffp-contract=off: the reference's float statements as written
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off",
           "-I" + str(root / "include"), "-I" + str(native / "cv_standin"),
           str(TRIANGULATE_REF_SRC), "-o", str(TRIANGULATE_REF_BIN) + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(TRIANGULATE_REF_BIN) + ".tmp", TRIANGULATE_REF_BIN)
    return TRIANGULATE_REF_BIN


# ---- PoseOptimization restated in plain C++ doubles (tests/native/poseopt_ref.cpp) ---------------
POSEOPT_REF_SRC = PKG.parent / "tests" / "native" / "poseopt_ref.cpp"
POSEOPT_REF_BIN = PKG.parent / "tests" / "native" / "poseopt_ref"


def build_poseopt_ref(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on the record layouts of include/ and csrc/orbx_math.h (orbx_sincos_f64) only: no
    liborbx and no GPU (the CPU reference of orbx_pose_optimization*)."""
    root = PKG.parent
    deps = [POSEOPT_REF_SRC, CSRC / "orbx_math.h"] + sorted((root / "include").glob("*.h"))
    newest = max(p.stat().st_mtime for p in deps)
    if (not force and POSEOPT_REF_BIN.exists() and
            POSEOPT_REF_BIN.stat().st_mtime >= newest):
        return POSEOPT_REF_BIN
    # -ffp-contract=off: every operation rounded on its own, as in the kernel
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off",
           "-I" + str(root / "include"), "-I" + str(CSRC), str(POSEOPT_REF_SRC),
           "-o", str(POSEOPT_REF_BIN) + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(POSEOPT_REF_BIN) + ".tmp", POSEOPT_REF_BIN)
    return POSEOPT_REF_BIN


# ---- Sim3Solver restated over the cv stand-in (tests/native/sim3_ref.cpp) -------------------------
SIM3_REF_SRC = PKG.parent / "tests" / "native" / "sim3_ref.cpp"
SIM3_REF_BIN = PKG.parent / "tests" / "native" / "sim3_ref"


def build_sim3_ref(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on the cv stand-in, tests/native/cv_sim3_standin.hpp, the record layouts of include/ and
    csrc/orbx_math.h (orbx_atan2_f64, orbx_sincos_f64) only: no liborbx and no GPU (the CPU
    reference of orbx_sim3_iterate*)."""
    root = PKG.parent
    native = root / "tests" / "native"
    deps = ([SIM3_REF_SRC, native / "cv_sim3_standin.hpp", CSRC / "orbx_math.h"] +
            sorted((root / "include").glob("*.h")) + sorted((native / "cv_standin").rglob("*.hpp")))
    newest = max(p.stat().st_mtime for p in deps)
    if not force and SIM3_REF_BIN.exists() and SIM3_REF_BIN.stat().st_mtime >= newest:
        return SIM3_REF_BIN
    # -ffp-contract=off: every operation rounded on its own, as in the kernels
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off",
           "-I" + str(root / "include"), "-I" + str(CSRC), "-I" + str(native / "cv_standin"),
           "-I" + str(native), str(SIM3_REF_SRC), "-o", str(SIM3_REF_BIN) + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(SIM3_REF_BIN) + ".tmp", SIM3_REF_BIN)
    return SIM3_REF_BIN


# ---- OptimizeSim3 restated in plain C++ doubles (tests/native/sim3opt_ref.cpp) --------------------
SIM3OPT_REF_SRC = PKG.parent / "tests" / "native" / "sim3opt_ref.cpp"
SIM3OPT_REF_BIN = PKG.parent / "tests" / "native" / "sim3opt_ref"


def build_sim3opt_ref(force: bool = False, verbose: bool = False, sanitize: bool = False,
                      out: pathlib.Path | None = None) -> pathlib.Path:
    """g++ on the record layouts of include/ and csrc/orbx_math.h (orbx_sincos_f64, orbx_exp_f64)
    only: no liborbx and no GPU (the CPU reference of orbx_sim3_optimize*).  sanitize: the
    stand-alone program with -fsanitize=address,undefined, to `out`."""
    root = PKG.parent
    target = pathlib.Path(out) if out else SIM3OPT_REF_BIN
    if sanitize and target.resolve() == SIM3OPT_REF_BIN.resolve():
        raise ValueError("the sanitized program goes to a path of its own")
    deps = [SIM3OPT_REF_SRC, CSRC / "orbx_math.h"] + sorted((root / "include").glob("*.h"))
    newest = max(p.stat().st_mtime for p in deps)
    if not force and target.exists() and target.stat().st_mtime >= newest:
        return target
    # -ffp-contract=off: every operation rounded on its own, as in the kernel
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off",
           "-I" + str(root / "include"), "-I" + str(CSRC), str(SIM3OPT_REF_SRC)]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd += ["-o", str(target) + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(target) + ".tmp", target)
    return target


# ---- PnPsolver restated in plain C++ (tests/native/pnp_ref.cpp) -------------------------------------
PNP_REF_SRC = PKG.parent / "tests" / "native" / "pnp_ref.cpp"
PNP_REF_BIN = PKG.parent / "tests" / "native" / "pnp_ref"


def build_pnp_ref(force: bool = False, verbose: bool = False, sanitize: bool = False,
                  out: pathlib.Path | None = None) -> pathlib.Path:
    """g++ on the record layouts of include/ only: no liborbx and no GPU (the CPU reference of
    orbx_pnp_iterate*).  sanitize: the stand-alone program with -fsanitize=address,undefined, to
    `out`."""
    root = PKG.parent
    target = pathlib.Path(out) if out else PNP_REF_BIN
    if sanitize and target.resolve() == PNP_REF_BIN.resolve():
        raise ValueError("the sanitized program goes to a path of its own")
    deps = [PNP_REF_SRC] + sorted((root / "include").glob("*.h"))
    newest = max(p.stat().st_mtime for p in deps)
    if not force and target.exists() and target.stat().st_mtime >= newest:
        return target
    # -ffp-contract=off: every operation rounded on its own, as in the kernels
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off",
           "-I" + str(root / "include"), str(PNP_REF_SRC)]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd += ["-o", str(target) + ".tmp"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(target) + ".tmp", target)
    return target
