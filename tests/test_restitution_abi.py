"""xpbd_world_set_restitution in the ABI: declared in the header, exported by the library, listed in both bindings; a NULL world
is an error without a device; on a device every rejected call leaves the previous values in place."""
import os
import re
import subprocess

import numpy as np
import pytest

from constraint_solver_amd import capi
from golden_util import bits_equal
from halo_common import pile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "xpbd_world_set_restitution"


def test_symbol_is_in_header_library_and_both_bindings():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xpbd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(xpbd_world \*w, const double \*restitution, uint32_t n, double ground_restitution,\s*"
                     r"double bounce_threshold\);" % NAME, header)
    assert NAME in capi.ABI_SYMBOLS
    assert hasattr(capi.hip_lib(), NAME)
    rust = open(os.path.join(ROOT, "constraint_solver_amd", "ffi", "xpbd_ffi.rs")).read()
    assert re.search(r"pub fn %s\(w: \*mut XpbdWorld, restitution: \*const f64, n: u32, ground_restitution: f64, bounce_threshold: f64\)\s*"
                     r"-> c_int;" % NAME, rust)
    assert "xpbd_multi_world_set_restitution" not in header      # out of scope, and said so in the header


def test_null_world_is_an_error_not_a_crash():
    L = capi.hip_lib()
    values = np.zeros(4)
    assert L.xpbd_world_set_restitution(None, None, 0, 0.0, 0.0) == capi.E_INVALID
    assert L.xpbd_world_set_restitution(None, values.ctypes.data, 4, 0.5, 0.0) == capi.E_INVALID
    assert b"xpbd_world_set_restitution" in L.xpbd_last_error()


@pytest.mark.parametrize("flag,value", [("--friction", "-1"), ("--friction", "nan"), ("--friction", "0.5x"), ("--restitution", "-0.1"),
                                        ("--restitution", "1.5"), ("--restitution", "bouncy")])
def test_headless_rejects_bad_material_flags_before_it_touches_a_device(flag, value):
    p = subprocess.run([os.path.join(capi.LIB_DIR, "xpbd_headless"), "--mode", "contacts", "--bodies", "8", flag, value],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 2 and flag in p.stderr


def test_headless_material_flags_need_the_contact_mode():
    p = subprocess.run([os.path.join(capi.LIB_DIR, "xpbd_headless"), "--bodies", "8", "--restitution", "0.5"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 2 and "--mode contacts" in p.stderr


@pytest.mark.gpu
def test_headless_runs_with_friction_and_restitution_and_they_change_the_result(tmp_path):
    """BatchWorld::set_materials / set_restitution through the driver: the dump differs from a run without the flags."""
    def dump(name, *flags):
        out = str(tmp_path / name)
        p = subprocess.run([os.path.join(capi.LIB_DIR, "xpbd_headless"), "--mode", "contacts", "--scene", "boxes-drop", "--bodies", "512",
                            "--substeps", "6", "--frames", "20", "--warmup", "0", "--dump", out] + list(flags), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        state = np.fromfile(out, dtype=np.float64)
        assert np.isfinite(state).all()
        return state.tobytes()

    plain = dump("plain.bin")
    assert dump("again.bin") == plain
    assert dump("zero.bin", "--restitution", "0") == plain
    assert dump("bouncy.bin", "--restitution", "0.8") != plain
    assert dump("icy.bin", "--friction", "0.1") != plain


@pytest.mark.gpu
def test_rejected_calls_leave_the_previous_values():
    kind, n, substeps = capi.SCENE_BOXES_DROP, 96, 6
    bodies, sid = pile(capi, kind, n, 7, 4.0, 3.0)
    e = np.array([0.0, 0.3, 0.8, 1.0])[np.random.default_rng(1).integers(0, 4, n)]

    def run(disturb):
        with capi.World(mode=capi.MODE_CONTACTS) as w:
            w.set_polytopes(capi.scene_polytopes(kind))
            w.upload(bodies, sid)
            w.set_restitution(e, 0.5, 0.01)
            for _ in range(4):
                w.step(1.0 / 60.0, substeps)
            if disturb:
                disturb(w)
            for _ in range(4):
                w.step(1.0 / 60.0, substeps)
            return w.download()

    def bad_calls(w):
        L = capi.hip_lib()
        above, below, nan = e.copy(), e.copy(), e.copy()
        above[3], below[n - 1], nan[0] = 1.0 + 1e-12, -1e-300, np.nan
        for values, ground, threshold in ((e[:-1], 0.5, 0.0), (np.concatenate([e, e[:1]]), 0.5, 0.0), (above, 0.5, 0.0), (below, 0.5, 0.0),
                                          (nan, 0.5, 0.0), (e, 1.5, 0.0), (e, -0.1, 0.0), (e, np.nan, 0.0), (e, 0.5, -1.0), (e, 0.5, np.inf),
                                          (e, 0.5, np.nan), (None, 2.0, 0.0)):
            with pytest.raises(capi.XpbdError) as err:
                w.set_restitution(values, ground, threshold)
            assert err.value.code == capi.E_INVALID
        assert L.xpbd_world_set_restitution(w._h, None, n, 0.5, 0.0) == capi.E_INVALID

    want = run(None)
    assert not np.isnan(want).any()
    assert bits_equal(run(bad_calls), want)
    assert not bits_equal(run(lambda w: w.set_restitution(None, 0.0, 0.0)), want)     # (an accepted call does change them)
