"""Host check of the identity the fused stepper's grid path rests on (rotate_bounded, constraint_solver_amd/csrc/xpbd_step.hpp):
`fma(c, 2.0, v)` and `c * 2.0 + v` are the same bits for every c when |v| <= 2^970 -- tests/fma_double_add_host.cpp, a
stand-alone program built with -ffp-contract=off, over random c of every exponent, |c| in [2^1022, max], subnormals, zeros,
infinities and NaN.  It also has to show the counter-example at |v| = 2^971: the bound is not decoration."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma " in line + " " for line in f)
    except OSError:
        return False


def test_fma_of_doubled_value_equals_multiply_then_add_under_the_bound(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the host check of rotate_bounded's identity cannot be built")
    exe = str(tmp_path / "fma_double_add_host")
    # -mfma only makes __builtin_fma one instruction instead of a libm call; -ffp-contract=off keeps `c * 2.0 + v` two roundings
    flags = ["-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wextra"] + (["-mfma"] if _cpu_has_fma() else [])
    subprocess.run([cxx] + flags + [os.path.join(ROOT, "tests", "fma_double_add_host.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    print(p.stdout)
    m = re.search(r"fma_double_add: (\d+) pairs \((\d+) with 2c overflowing\), (\d+) differences; "
                  r"counter-example at 2\^971: (\w+); tie at 2\^970: (.+)", p.stdout)
    assert m, p.stdout
    n, n_overflow, bad = map(int, m.group(1, 2, 3))
    assert bad == 0
    assert m.group(4) == "yes" and m.group(5).strip() == "inf"
    assert p.returncode == 0
    assert n >= 10 ** 7 and n_overflow >= 10 ** 6      # the overflow branch of the argument was really walked
