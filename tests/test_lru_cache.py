"""CPU: the workspace cache template and its key structs (attack-vc_amd/csrc/avc_lru.h), through a
stand-alone C++ program (tests/lru_cache_test.cpp) built with the host side of hipcc only: LRU order, the
cap and its quiesce hook, keys that differ only in engine / lengths / raggedness, erase, a cap of 1."""
import os
import subprocess

import __graft_entry__ as entry
from conftest import ROOT


def test_lru_cache_program(tmp_path):
    src = os.path.join(ROOT, "tests", "lru_cache_test.cpp")
    exe = str(tmp_path / "lru_cache_test")
    # a .cpp file: plain host C++, no offload architecture, no HIP runtime
    subprocess.run([entry._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lru_cache_test: ok" in r.stdout
