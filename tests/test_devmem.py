"""The capacity rule of the growing device buffers (csrc/sph_devmem.hpp, grown_capacity).

A C++ program (tests/cpp/devmem_host.cpp) checks the rule against a literal table; it is built
from the header's host part alone, once plainly and once with the address and undefined
behaviour sanitizers.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_grown_capacity_table(flags, tmp_path):
    exe = str(tmp_path / "devmem_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "devmem_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 of 6 rows differ" in r.stdout
