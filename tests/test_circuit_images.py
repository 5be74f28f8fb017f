"""What circuit::compile builds and what it refuses first, pinned without a GPU.

Images: tests/c/circuit_image_check.cpp compiles a fixed list of descriptions
with csrc/host/circuit.cpp (ASan + UBSan) and prints digests of the device
images, the level schedule, the matrices, c and the program digest; they equal
tests/golden/circuit_images.json, recorded with the same program before
circuit.cpp stated its term checks, its image tail, its levels and its gate walk
once.  The witness kernels read nothing else of a circuit.

Refusals: a description with two faults of different codes returns the code of
the fault the checks reach first -- one test per shared check (the
description's term table, the hint program's)."""
import json
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import circuit_wire_hints_ref as wr  # noqa: E402

ROOT = HERE.parent
CSRC = ROOT / "bulletproof-perm_amd" / "csrc"
L = wr.L
ARG, NONCANONICAL = 1, 4
NAMES = ["no_aux", "public_inputs", "early_hint_of_every_op", "early_hint_of_every_op_wire_entry", "late_chain_7",
         "late_chain_7_unhinted", "late_chain_7_early_old_entry", "late_chain_40", "late_chain_40_unhinted",
         "late_chain_40_early_old_entry", "large_tiled", "three_gates"]
KEYS = ["program_dev", "program_dev_offsets", "hints_dev", "levels", "WL", "WR", "WO", "WV", "WU", "c", "shape", "digest"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_compiled_images_equal_the_recorded_ones(tmp_path):
    exe = tmp_path / "circuit_image_check"
    srcs = [ROOT / "tests" / "c" / "circuit_image_check.cpp",
            *(CSRC / "host" / f for f in ("circuit.cpp", "perm_circuit.cpp", "keccak.cpp", "keccak_x8.cpp"))]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-march=x86-64-v3",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC), *map(str, srcs),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "failures: 0" in r.stdout, (r.stdout + r.stderr)[-3000:]
    got = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("failures:"):
            continue
        name, key, val = ln.split()
        assert key not in got.setdefault(name, {}), (name, key)
        got[name][key] = val
    want = json.loads((HERE / "golden" / "circuit_images.json").read_text())
    assert sorted(want) == sorted(NAMES) and all(sorted(v) == sorted(KEYS) for v in want.values())
    assert sorted(got) == sorted(NAMES)
    for name in NAMES:
        for key in KEYS:
            assert got[name].get(key) == want[name][key], (name, key)
    # the hints are no part of the statement; the wire entry point builds the old one's images of an early program
    same = lambda a, b, keys: all(want[a][k] == want[b][k] for k in keys)
    statement = ["WL", "WR", "WO", "WV", "WU", "c", "shape", "digest"]
    for n in ("7", "40"):
        assert same("late_chain_" + n, "late_chain_" + n + "_unhinted", statement)
        assert same("late_chain_" + n, "late_chain_" + n + "_early_old_entry", statement)
        assert not same("late_chain_" + n, "late_chain_" + n + "_unhinted", ["program_dev", "levels"])
    assert same("early_hint_of_every_op", "early_hint_of_every_op_wire_entry", KEYS)


def _code(desc, **kw):
    import bpperm
    with pytest.raises(bpperm.BppError) as e:
        bpperm.Circuit(desc, **kw)
    return e.value.code


def _two_gates():
    """v_0 * v_1 and (o_0 + 2) * v_0: five terms, gate 1's left side holds two."""
    d = wr.Desc(2, 0)
    d.gate([(d.v(0), 1)], [(d.v(1), 1)])
    d.gate([(0, 2), (d.w(0, 2), 1)], [(d.v(0), 1)])
    return d


def test_description_with_two_faults_returns_the_first_one_s_code():
    """The description's term table: an id out of range (ARG), then a coefficient
    not below l (NONCANONICAL) in a later term -- ARG, as before the checks were
    shared (ids and coefficients are checked term by term, the id first); the
    same two faults in one term -- ARG; the coefficient's term first --
    NONCANONICAL."""
    import bpperm
    bad, nvar = L.to_bytes(32, "little"), 2 + 2 + 3 * 2
    assert not bpperm.Circuit(_two_gates(), hints=False).has_hints  # the description itself is fine
    d = _two_gates()
    d.lc_var[1], d.lc_coef[3] = nvar, bad  # gate 0 right: id out of range; gate 1 left, second term: coefficient = l
    assert _code(d, hints=False) == ARG
    d = _two_gates()
    d.lc_var[3], d.lc_coef[3] = nvar + 5, bad  # one term with both
    assert _code(d, hints=False) == ARG
    d = _two_gates()
    d.lc_coef[1], d.lc_var[3] = bad, nvar
    assert _code(d, hints=False) == NONCANONICAL
    d = _two_gates()
    d.lc_var[3], d.lc_coef[4] = d.w(1, 0), bad  # a wire of its own gate, then the coefficient
    assert _code(d, hints=False) == ARG
    d = _two_gates()
    d.lc_coef[2], d.lc_var[3] = bad, d.w(1, 0)  # the other way round, within one side
    assert _code(d, hints=False) == NONCANONICAL


def _two_hints():
    """aux_0 = v_0 + 3 and aux_1 = 5 v_1 feed the right sides of two gates."""
    d = wr.Desc(2, 0)
    t0 = d.hint(wr.VALUE, 0, [(0, 3), (d.v(0), 1)])
    t1 = d.hint(wr.VALUE, 0, [(d.v(1), 5)])
    d.gate([(d.v(0), 1)], t0)
    d.gate([(d.v(1), 1)], t1)
    return d


@pytest.mark.parametrize("wire", [False, True], ids=["hinted", "wire_hinted"])
def test_hint_program_with_two_faults_returns_the_first_one_s_code(wire):
    """The hint program's term table: an unknown op (ARG) on a hint in front of
    one with a coefficient not below l (NONCANONICAL) -- ARG, as before the
    checks were shared (a hint's op is checked before its terms, hints in
    order); both on one hint -- ARG; the coefficient's hint first --
    NONCANONICAL.  A fault of the description comes before either."""
    import bpperm
    bad = L.to_bytes(32, "little")
    assert bpperm.Circuit(_two_hints(), wire_hints=wire).has_hints
    d = _two_hints()
    d.hints.op[0], d.hints.lc_coef[2] = 5, bad
    assert _code(d, wire_hints=wire) == ARG
    d = _two_hints()
    d.hints.op[1], d.hints.lc_coef[2] = 0xFF, bad
    assert _code(d, wire_hints=wire) == ARG
    d = _two_hints()
    d.hints.lc_coef[0], d.hints.op[1] = bad, 5
    assert _code(d, wire_hints=wire) == NONCANONICAL
    d = _two_hints()
    d.lc_coef[0], d.hints.op[0] = bad, 5  # the description's coefficient, then the hint's op
    assert _code(d, wire_hints=wire) == NONCANONICAL
    d = _two_hints()
    d.lc_var[0], d.hints.lc_coef[0] = 2 + 2 + 3 * 2, bad  # the description's id, then the hint's coefficient
    assert _code(d, wire_hints=wire) == ARG
