"""Host check of constraint_solver_amd/csrc/xpbd_exact.hpp: the two sequences the stepper uses in place of `sqrt` followed
by `1.0 / s`, and of `x / h`, compiled for the CPU with an injected reciprocal-square-root seed of relative error up to
2^-20 (tests/exact_math_host.cpp; no bound for v_rsq_f64 is documented here, so the fall-back figure is used) and
compared bit for bit with `/` and `sqrt` on more than 10^8 operands.  Zero differences allowed."""
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


def test_exact_math_sequences_agree_with_divide_and_sqrt_on_the_host(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the host check of xpbd_exact.hpp cannot be built")
    exe = str(tmp_path / "exact_math_host")
    # -mfma only makes __builtin_fma one instruction instead of a libm call; -ffp-contract=off keeps every other a*b+c unfused
    flags = ["-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wextra"] + (["-mfma"] if _cpu_has_fma() else [])
    subprocess.run([cxx] + flags + ["-I" + os.path.join(ROOT, "constraint_solver_amd", "csrc"),
                                    os.path.join(ROOT, "tests", "exact_math_host.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    print(p.stdout)
    pair = re.search(r"pair: (\d+) operands \((\d+) fast\), (\d+) root differences, (\d+) reciprocal differences", p.stdout)
    div = re.search(r"div_by: (\d+) operands \((\d+) fast\), (\d+) differences", p.stdout)
    assert pair and div, p.stdout
    n_pair, fast_pair, bad_root, bad_recip = map(int, pair.groups())
    n_div, fast_div, bad_div = map(int, div.groups())
    assert (bad_root, bad_recip, bad_div) == (0, 0, 0)
    assert p.returncode == 0
    assert n_pair + n_div >= 10 ** 8
    # both paths of both guards ran: most operands fast, the edges slow
    assert 0 < n_pair - fast_pair < fast_pair and 0 < n_div - fast_div < fast_div
