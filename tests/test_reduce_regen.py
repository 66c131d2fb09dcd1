"""The rule by which the read-only reduce regenerates part of the noise it sums (csrc/reduce_regen.h), on the host:
tests/native/reduce_regen_host.cpp (its own main) built host-only with ASan + UBSan, as tests/test_gen_overlap.py
builds its program, and the read-out's place in the ABI."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, REPO

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

WANTED = ("size threshold is strict", "whole rows: eighths of any 8 consecutive rows",
          "a row regenerates its tile's last slots", "Kp 96: every quad once", "Kp 1024: every quad once",
          "Kp 1536: every quad once", "Kp 1024: the share is eighths / 8", "rule: content is never overridden",
          "rule: a forced share ignores the size")


@pytest.fixture(scope="module")
def host_out(tmp_path_factory):
    assert os.path.exists(HIPCC), "hipcc is needed to build the host form of the rule"
    exe = str(tmp_path_factory.mktemp("reduce_regen") / "reduce_regen_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address",
           "-Xarch_host", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           f"-I{REPO}/include", f"-I{PKG}/csrc", os.path.join(REPO, "tests", "native", "reduce_regen_host.cpp"),
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
    """The header's figures as the kernel uses them: the reduce's tile of four quads per lane, its own 128 MiB."""
    with open(os.path.join(PKG, "csrc", "reduce_regen.h")) as f:
        src = f.read()
    for decl in ("constexpr int kRegenTileQuads = 4;", "constexpr int kRegenMaxEighths = 7;",
                 "constexpr uint64_t kRegenMinNoiseBytes = 128ull * 1024 * 1024;"):
        assert decl in src, decl
    with open(os.path.join(PKG, "csrc", "kernels_common.hip")) as f:
        kern = f.read()
    assert "static_assert(!(GEN && REGEN)" in kern
    assert "kRU == kRegenTileQuads" in kern


def test_entry_is_bound_and_takes_null():
    from mppi_hip import _lib as L
    assert "mppi_reduce_regen" in L.EXPORTED
    lib = L.load()
    assert lib.mppi_reduce_regen(None) == 0
    with open(os.path.join(REPO, "include", "mppi.h")) as f:
        assert "int mppi_reduce_regen(mppi_handle* h);" in f.read()
