"""Host check of the wire encoder that host and device code share
(etcd_amd/csrc/ewal_wire.h): the closed-form varint size against the shift
loop, entry_head / frame_head against entry_marshal / frame_write and against
bytes spelled out with a loop varint (tests/host/wire_forms.cpp), plain and
under ASan + UBSan.  CPU only: the GPU parity suites check the kernels that
call the same functions."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1"] + SAN], ids=["plain", "asan_ubsan"])
def test_wire_forms(tmp_path, flags):
    exe = str(tmp_path / "wire_forms")
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "etcd_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "host", "wire_forms.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
