"""tests/san_start_main.cpp with csrc/rcw_rules.hip in one translation unit, host side only, under -fsanitize=address,undefined:
rcw_start_rule on the hand-made maps of tests/start_distance_ref.py, on maps without a wall ring and on every refused argument, each map in
a heap block of exactly its size.  A stand-alone program on the CPU: no sanitizer's runtime is loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_under_asan_and_ubsan_as_a_program_of_its_own(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "san_start")
    build = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                            "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", exe,
                            os.path.join(ROOT, "tests", "san_start_main.cpp")], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert run.returncode == 0 and "san_start_main: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
