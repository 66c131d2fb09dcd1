"""The rule that routes a chained solve's next noise beside its rollout (csrc/gen_overlap.h), on the host:
tests/native/gen_overlap_host.cpp (its own main) built host-only with ASan + UBSan, as tests/test_iterations.py builds
its program, and the new entries' place in the ABI."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import PKG, REPO

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

WANTED = ("248 + 248 + 16 fits", "252 + 252 + 16 does not", "248 + 248 + 20 does not", "size threshold: both sides",
          "philox4x32_10_row == philox4x32_10")


@pytest.fixture(scope="module")
def host_out(tmp_path_factory):
    assert os.path.exists(HIPCC), "hipcc is needed to build the host form of the rule"
    exe = str(tmp_path_factory.mktemp("gen_overlap") / "gen_overlap_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{PKG}/csrc", os.path.join(REPO, "tests", "native", "gen_overlap_host.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    return r.returncode, r.stdout, r.stderr


def test_the_rules_arithmetic_holds_on_the_host(host_out):
    rc, out, err = host_out
    lines = out.splitlines()
    assert rc == 0 and lines and all(ln.startswith("ok ") for ln in lines), out + err[-2000:]
    for name in WANTED:  # the checks the rule stands on ran
        assert f"ok {name}" in lines, name


def test_the_rules_constants():
    """The header's figures as the kernels use them: 16 registers for the generator, the reduce's own 128 MiB."""
    with open(os.path.join(PKG, "csrc", "gen_overlap.h")) as f:
        src = f.read()
    for decl in ("constexpr int kGenVgprs = 16;", "constexpr int kGenRegGranule = 8;", "constexpr int kGenSimdRegs = 512;",
                 "constexpr uint64_t kGenMinNoiseBytes = 128ull * 1024 * 1024;"):
        assert decl in src, decl


def test_entries_are_bound_and_refuse_null():
    from mppi_hip import _lib as L
    for name in ("mppi_gen_route", "mppi_noise_beside_eval"):
        assert name in L.EXPORTED
    lib = L.load()
    assert (lib.mppi_gen_route(None) or b"") == b""
    buf = (ctypes.c_float * 4)()
    assert lib.mppi_noise_beside_eval(None, 1, ctypes.c_uint64(1), buf) == L.MPPI_E_ARG
    assert b"mppi_noise_beside_eval" in lib.mppi_last_error()
