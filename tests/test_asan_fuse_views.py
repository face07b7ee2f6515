"""Sanitizer tier for the host side of the in-memory fusion
(acmmp_fuse_views_jacobi's argument checks, acmmp_write_ply_points,
acmmp_resize_bilinear_u8): tests/asan/fuse_views_driver.cpp, a stand-alone
program built with AddressSanitizer + UndefinedBehaviorSanitizer
(tests/asan/Makefile.fuse_views). Any sanitizer report fails the test. CPU
only; the kernels are covered by tests/test_gpu_fuse_views.py."""
import fcntl
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN_DIR = os.path.join(ROOT, "tests", "asan")
DRIVER = os.path.join(ASAN_DIR, "build", "fuse_views_driver")
ENV = dict(os.environ,
           ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=1:halt_on_error=1:abort_on_error=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ with libasan needed")


def test_fuse_views_host_side_under_sanitizers(tmp_path):
    os.makedirs(os.path.join(ASAN_DIR, "build"), exist_ok=True)
    with open(os.path.join(ASAN_DIR, "build", ".make_fuse_views.lock"), "w") as lk:  # one make at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", ASAN_DIR, "-f", "Makefile.fuse_views"], capture_output=True,
                           text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([DRIVER, str(tmp_path)], env=ENV, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0 and "fuse_views host ok" in out, out[-4000:]
