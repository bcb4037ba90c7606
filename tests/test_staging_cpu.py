"""CPU: the staging vocabulary of the host forms (csrc/staging.hpp: DevBuf upload / download / wipe, HIPCHK) against a
stand-in for HIP with a live-allocation counter and a switch that fails the k-th call -- tests/host/staging_host_test.cpp.
Built by g++, so it also runs under the sanitizers with BPP_HOST_SANITIZE=1 (a leak or a read of freed memory on an error
path ends the program)."""

import subprocess

from test_host_arith_cpu import _build


def test_staging_vocabulary_on_every_error_path(tmp_path):
    out = subprocess.run([_build("staging_host_test", tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "ok staging" in out.stdout, out.stdout + out.stderr
