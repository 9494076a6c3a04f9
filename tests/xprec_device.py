"""What the test_gpu_xprec_*.py files share on the device side: the far field, the world every family creates, the one ordered
list of setters a scene dict can carry, the single-substep runner, the three runs of a seam test and the verdict.  Used only
by tests marked gpu."""
import numpy as np

import xprec_check as xk
import xprec_pairs_cases as pc
from constraint_solver_amd import capi

SMALL_WORLD = 16384          # must equal XPBD_SMALL_WORLD in xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body
SAT_SCHEDULES = (capi.SAT_SCHEDULE_AUTO, capi.SAT_SCHEDULE_ONE_PASS, capi.SAT_SCHEDULE_TWO_PASS)
SCHEDULE_IDS = ["auto", "one-pass", "two-pass"]


def far_field(far):
    """That many boxes on a 4 m grid 200 m away, to stand behind a scene's bodies: (bodies, shape ids)."""
    if not far:
        return np.zeros((0, 38)), np.zeros(0, dtype=np.uint32)
    extra, extra_sid = capi.scene_generate(capi.SCENE_BOXES, 9, far)
    k = np.arange(far)
    extra[:, 31], extra[:, 32] = 200.0 + 4.0 * (k % 128), 4.0 * (k // 128)
    extra[:, 22:25] *= 0.3
    return extra, extra_sid


def new_world(schedule=capi.SAT_SCHEDULE_AUTO, narrowphase=capi.NARROWPHASE_SAT):
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes(pc.capi_polytopes(capi))
    w.set_narrowphase(narrowphase)
    w.set_sat_schedule(schedule)
    return w


def apply_settings(w, scene, n_extra=0, without=(), kinematics=None):
    """Every setter the scene dict carries, after the upload and in the order the header requires (set_joints clears the
    dampers, an upload everything), each padded for n_extra far bodies.  without: the controls, settings left out ("slide
    limits", "drives", "restitution", "terrain", "damping", "joint_damping", "kinematics") or "flat": the field all zero."""
    if len(scene.get("joints", ())):
        w.set_joints(scene["joints"])
    limits = scene.get("limits", ())
    if "slide limits" in without and len(limits):
        limits = limits[limits["kind"] != capi.LIMIT_SLIDE]
    if len(limits):
        w.set_joint_limits(limits)
    if len(scene.get("drives", ())) and "drives" not in without:
        w.set_joint_drives(scene["drives"])
    if scene.get("speed"):
        w.set_max_depenetration_speed(scene["speed"])
    if scene.get("mu") is not None:
        w.set_materials(np.concatenate([scene["mu"], np.full(n_extra, np.inf)]), scene["ground_mu"])
    if scene.get("e") is not None and "restitution" not in without:
        w.set_restitution(np.concatenate([scene["e"], np.zeros(n_extra)]), scene["ground_e"], scene["threshold"])
    if "terrain" in scene:
        field = None if "terrain" in without else scene["terrain"]
        if field is None:
            w.set_terrain(None)
        else:
            w.set_terrain(field["heights"] * 0.0 if "flat" in without else field["heights"], field["origin"], field["cell"])
    if scene.get("rows") is not None and "damping" not in without:
        w.set_damping(np.concatenate([scene["rows"], capi.body_damping(n_extra)]))
    if scene.get("dampers") is not None and "joint_damping" not in without:
        w.set_joint_damping(scene["dampers"])
    if scene.get("kinematics") is not None and "kinematics" not in without:
        w.set_kinematics(scene["kinematics"] if kinematics is None else kinematics)


def prepare(w, scene, start, extra=None, without=(), kinematics=None):
    """The scene's bodies in state `start` with the far field `extra` (far_field's pair) behind them, then the scene's settings."""
    extra = far_field(0) if extra is None else extra
    w.upload(np.concatenate([start, extra[0]]), np.concatenate([scene["sid"], extra[1]]).astype(np.uint32))
    apply_settings(w, scene, len(extra[0]), without, kinematics)


def run_frames(starts_and_scenes, schedule=capi.SAT_SCHEDULE_AUTO, far=0, without=(), frames=None):
    """Every single-substep frame on the device in one world, each from its start state: the downloaded states, the far field cut off."""
    extra = far_field(far)
    out = []
    with new_world(schedule) as w:
        for start, scene in starts_and_scenes[:frames]:
            prepare(w, scene, start, extra, without)
            w.step(scene["h"], 1)
            out.append(w.download()[:len(start)])
    return out


def seam_runs(w, prepare, h, split=True):
    """From what prepare() uploads and sets: step(4 h, 4), four step(h, 1), and contacts_begin(4 h) + four contacts_substep(h) if
    asked.  Returns (fused, single, split or None)."""
    prepare()
    w.step(4 * h, 4)
    fused = w.download()
    prepare()
    for _ in range(4):
        w.step(h, 1)
    single = w.download()
    if not split:
        return fused, single, None
    prepare()
    w.contacts_begin(4 * h)
    for _ in range(4):
        w.contacts_substep(h)
    return fused, single, w.download()


def verdict(cases, name, got):
    """The family's bound (cases.check_states) and the exclusion caps on this run, and the printed figure."""
    errs, excl, entry = cases.check_states(name, got)
    xk.assert_caps(name, excl, entry)
    print("%s: device against the model %.1f" % (name, xk.worst(errs, excl)))
