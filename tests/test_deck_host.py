"""Host C++ of the public-deck proof under ASan + UBSan, as a stand-alone CPU
program (tests/c/deck_witness_check.cpp): the deck circuit's rows, the host
witness (the k > 1536 path) and the deck product of the host replay."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "bulletproof-perm_amd" / "csrc"


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_deck_witness_host_asan_ubsan(tmp_path):
    exe = tmp_path / "deck_witness"
    srcs = [ROOT / "tests" / "c" / "deck_witness_check.cpp",
            *(CSRC / "host" / f for f in ("perm_circuit.cpp", "keccak.cpp", "keccak_x8.cpp"))]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-march=x86-64-v3",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC), *map(str, srcs),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, BPP_HOST_THREADS="4", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout, (r.stdout + r.stderr)[-3000:]
