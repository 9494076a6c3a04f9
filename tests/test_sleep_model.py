"""Island sleeping without a GPU: hand-written answers for the independent model (sleep_model.py) that the GPU tests hold the
library to, the layout of xpbd_sleep_config against the header, and SleepTarget -- the argument checks of the sleeping calls
(csrc/xpbd_checks.cpp) -- built with plain g++ (no hipcc, no ROCm include path) into a stand-alone program,
tests/sleep_checks_standalone_main.cpp, which makes the calls the checks accept and one call for every way they refuse.

The same program is also built and run under ASan + UBSan and must leave stderr empty.  A sanitizer-linked executable refuses
to start where something else is preloaded into every process, so that variant is skipped there, and only there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sleep_model as sm
from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
NONE = sm.GROUP_NONE
CFG = (0.1, 0.5, 3)


def bodies_of(n, speed=0.0, spin=0.0, fixed=()):
    """n movable bodies (identity inertia) with the given speeds (scalars or per body), the listed ones fixed."""
    b = np.zeros((n, 38))
    b[:, 0] = 1.0
    b[:, [1, 5, 9]] = 1.0
    b[:, 22] = speed
    b[:, 27] = spin
    for i in fixed:
        b[i, 0:10] = 0.0
    return b


def pairs_of(*ends):
    return np.array(ends, dtype=np.uint32).reshape(-1, 2)


def state_of(asleep, rest, group):
    s = sm.State(len(asleep))
    s.asleep[:], s.rest_frames[:], s.group[:] = asleep, rest, group
    return s


def rows(s):
    return s.asleep.tolist(), s.rest_frames.tolist(), s.group.tolist()


# ---- the model, by hand ---------------------------------------------------------------------------------------------------------------
def test_an_island_sleeps_when_its_slowest_counter_reaches_the_bound():
    # 0-1 touch, 2 alone, 3 too fast
    b = bodies_of(4, speed=[0.0, 0.05, 0.1, 0.2])
    s = sm.State(4)
    for frame in (1, 2):
        s, woken, slept = sm.frame(s, b, pairs_of((0, 1)), None, CFG)
        assert (woken, slept) == (0, 0) and rows(s) == ([0, 0, 0, 0], [frame, frame, frame, 0], [NONE] * 4)
    s, woken, slept = sm.frame(s, b, pairs_of((0, 1)), None, CFG)
    assert (woken, slept) == (0, 3)
    assert rows(s) == ([1, 1, 1, 0], [3, 3, 3, 0], [0, 0, 2, NONE]) and s.counts() == (3, 2)


def test_one_restless_member_keeps_its_island_awake_and_the_threshold_is_inclusive():
    b = bodies_of(3, speed=[0.1, 0.1, 0.1], spin=[0.5, 0.5, 0.5000001])
    s = sm.State(3)
    for _ in range(5):
        s, _, slept = sm.frame(s, b, pairs_of((0, 1), (1, 2)), None, CFG)
        assert slept == 0
    assert rows(s) == ([0, 0, 0], [5, 5, 0], [NONE] * 3)
    s, _, slept = sm.frame(s, b, pairs_of((0, 1)), None, CFG)            # 2 lets go: 0-1 have rested long enough
    assert slept == 2 and rows(s) == ([1, 1, 0], [6, 6, 0], [0, 0, NONE])


def test_a_nan_is_not_at_rest():
    b = bodies_of(2)
    b[1, 23] = np.nan
    s = sm.State(2)
    for _ in range(3):
        s, _, _ = sm.frame(s, b, None, None, CFG)
    assert rows(s) == ([1, 0], [3, 0], [0, NONE])


def test_a_touch_by_an_awake_body_wakes_the_whole_group_and_a_fixed_or_asleep_one_does_not():
    # 0-1-2 asleep as group 0; 3 asleep alone; 4 fixed; 5 awake
    asleep, rest, group = [1, 1, 1, 1, 0, 0], [3, 3, 3, 7, 0, 1], [0, 0, 0, 3, NONE, NONE]
    b = bodies_of(6, fixed=(4,))
    s, woken, slept = sm.sleep_pass(state_of(asleep, rest, group), b, pairs_of((2, 4), (3, 4)), None, *CFG)
    assert (woken, slept) == (0, 0) and rows(s) == ([1, 1, 1, 1, 0, 0], [3, 3, 3, 7, 0, 2], [0, 0, 0, 3, NONE, NONE])
    s, woken, slept = sm.sleep_pass(state_of(asleep, rest, group), b, pairs_of((2, 5)), None, *CFG)
    # the group wakes with zero counters and counts this frame; 5 (now 2) is in an island with bodies that have not rested
    assert (woken, slept) == (3, 0) and rows(s) == ([0, 0, 0, 1, 0, 0], [1, 1, 1, 7, 0, 2], [NONE, NONE, NONE, 3, NONE, NONE])


def test_a_joint_to_a_sleeper_holds_an_island_awake():
    b = bodies_of(2)
    joints = np.zeros(1, dtype=capi.JOINT_DTYPE)
    joints["body_a"], joints["body_b"] = 0, 1
    s, woken, slept = sm.sleep_pass(state_of([1, 0], [3, 9], [0, NONE]), b, None, joints, *CFG)
    assert (woken, slept) == (0, 0) and rows(s) == ([1, 0], [3, 10], [0, NONE])


def test_requests_wake_groups_before_the_frame():
    asleep, rest, group = [1, 1, 1, 1, 0, 0], [3, 3, 3, 7, 0, 2], [0, 0, 0, 3, NONE, NONE]
    fixed = np.array([0, 0, 0, 0, 1, 0], dtype=bool)
    s = sm.frame_begin(state_of(asleep, rest, group), fixed, sm.Requests([1, 5]))
    assert rows(s) == ([0, 0, 0, 1, 0, 0], [0, 0, 0, 7, 0, 2], [NONE, NONE, NONE, 3, NONE, NONE])
    s = sm.frame_begin(state_of(asleep, rest, group), fixed, sm.Requests([4]))                 # a fixed body: everybody
    assert rows(s) == ([0] * 6, [0, 0, 0, 0, 0, 2], [NONE] * 6)
    s = sm.frame_begin(state_of(asleep, rest, group), fixed, sm.Requests(wake_all=True, zero_counters=True))
    assert rows(s) == ([0] * 6, [0] * 6, [NONE] * 6)
    s = sm.frame_begin(state_of(asleep, rest, group), fixed, None)
    assert rows(s) == (asleep, rest, group)


def test_the_counter_saturates():
    s, _, slept = sm.sleep_pass(state_of([0], [0xFFFFFFFF], [NONE]), bodies_of(1), None, None, 0.1, 0.5, 0xFFFFFFFF)
    assert slept == 1 and rows(s) == ([1], [0xFFFFFFFF], [0])


# ---- the struct against the header ----------------------------------------------------------------------------------------------------
def test_sleep_config_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "xpbd.h"\n'
                   "int main() { std::printf(\"%zu %zu %zu %zu %zu %x\\n\", sizeof(xpbd_sleep_config), offsetof(xpbd_sleep_config, linear_speed),\n"
                   "  offsetof(xpbd_sleep_config, angular_speed), offsetof(xpbd_sleep_config, frames_to_sleep), offsetof(xpbd_sleep_config, flags),\n"
                   "  XPBD_SLEEP_GROUP_NONE); return 0; }\n")
    exe = str(tmp_path / "layout")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    got = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=60).stdout.split()
    S = capi.SLEEP_CONFIG
    assert [int(v) for v in got[:5]] == [C.sizeof(S), S.linear_speed.offset, S.angular_speed.offset, S.frames_to_sleep.offset, S.flags.offset]
    assert C.sizeof(S) == 24 and int(got[5], 16) == capi.SLEEP_GROUP_NONE == sm.GROUP_NONE


# ---- the checks, stand-alone ----------------------------------------------------------------------------------------------------------
SOURCES = [os.path.join(CSRC, "xpbd_checks.cpp"), os.path.join(CSRC, "xpbd_error.cpp"), os.path.join(ROOT, "tests", "sleep_checks_standalone_main.cpp")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
VARIANTS = {
    "plain": ["-O1"],
    "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


def something_is_preloaded():
    preload_file = "/etc/ld.so.preload"
    return bool(os.environ.get("LD_PRELOAD", "").strip()) or (os.path.exists(preload_file) and os.path.getsize(preload_file) > 0)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_sleep_checks_build_and_run_without_a_device(variant, tmp_path):
    sanitized = variant != "plain"
    if sanitized and something_is_preloaded():
        pytest.skip("a library is preloaded into every process here: a sanitizer-linked program would not start")
    exe = str(tmp_path / ("sleep_checks_standalone_" + variant))
    build = subprocess.run(["g++"] + FLAGS + VARIANTS[variant] + SOURCES + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "24 calls ok" in run.stdout
    if sanitized:
        assert run.stderr == ""
