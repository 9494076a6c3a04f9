"""Sliders, SLIDE limits and joint drives in contact, shared by test_xprec_drives_oracle.py (f64 evaluation vs the longdouble
model, CPU) and test_gpu_xprec_drives.py (HIP vs the model): the scenes, each as a sequence of SINGLE-SUBSTEP frames (dt = h,
substeps = 1), the model (xprec_pairs_model.substep with joints=, limits= and drives=) re-seeded before every one, the bound
and the exclusions.  Helpers, normalisation and constants are those of xprec_joints_cases.py and xprec_pairs_cases.py.

Seeding.  A frame starts from the previous frame's result of the f64 evaluation of the model (xprec_model.f64()): the oracle
knows no sliders and no drives, and nothing else in f64 is independent of the code under test.

Scenes, 24 bodies or fewer each, 12 frames, at h = 1/1200 and 1/240:
  (a) lifts   boxes on sliders standing on static slabs, on each other and on the ground: the axis vertical, tilted 0.5 rad
              and horizontal; VELOCITY drives with max_force below and above the load, POSITION drives stiff and soft; SLIDE
              limits that bind from the first frame, that start to bind within the frames and that never bind; a prismatic
              joint (slider + LIMIT_HINGE 0/0) with a SLIDE limit, an ANGLE and a VELOCITY drive
  (b) wheels  boxes hinged to the slab they lie on, some against a neighbour: ANGULAR_VELOCITY drives (one started at
              phi = pi - 1e-3 and carried across pi within the frames, one force-limited), ANGLE drives with targets +pi, -pi
              (exactly) and 0, a soft one, and a hinge whose drive pushes into its HINGE limit
  (c) exact   binary-exact poses re-made every frame, boxes on a static slab EXACT_DEPTH deep and on each other: a slider
              whose anchor is exactly on the axis (no perpendicular entry) with s exactly on its SLIDE bound, a POSITION drive
              with s == target, an ANGLE drive with phi == target == 0
  (d) ends    the categories of edge_rigids as slider and driven-hinge ends in touching pairs; one joint with
              body_a > body_b; one pair joined by a driven slider and a rod; a hub box on a slab with 12 driven joints; ball
              joints without extras interleaved; the drive list shuffled against the joint order
  (e) mixed   scene (a) with mixed friction (MUS, GROUND_MU) and the depenetration limit at 3 m/s

Measured (test_xprec_drives_oracle.py prints them), largest normalised error of a checked body-substep per scene, f64
evaluation against the longdouble model:
  lifts-h1200 2.0   wheels-h1200 3.8   exact-h1200 0.5   ends-h1200  7.1   mixed-h1200 0.7
  lifts-h240  2.7   wheels-h240  1.9   exact-h240  0.6   ends-h240  25.2   mixed-h240  1.8
  (body 0 of scene (d), the asym_inertia edge body at the end of a driven slider, a SLIDE limit and a rod, holds the maximum)
The bound is 8x the largest of all of them (the margin K_PAIRS, K_MANIFOLD and K_JOINTS took: the device differs from the f64
reading in operation order and in its atan2 only).  8 x 25.2 = 201 fits under K_PAIRS = 656, so K_DRIVES is K_PAIRS
(test_the_bound_is_eight_times_the_measured_maximum keeps that true).  tests/joint_drive_model.py's contact-free scenes lie
within 1.0 of the model (its known-answer scenes within 0.7); the 40-digit mpmath model moves the substep that holds a scene's
maximum by 0.0077 at most (1.2e-5 of the bound).  Excluded: 0 of 1 320 body-substeps, 0 of 1 095 of those with an extra entry
and a pair or ground point.  Scene (d)'s seed was not chosen by its figure: seeds 82 to 87 of it give maxima from 11 to 492,
the large ones all on the `spin` edge body (h |w| / 2 near 1) at a one-ulp sensitivity of 4 to 5, below SENSITIVITY_MAX."""
import functools

import numpy as np

import xprec_check as xk
import xprec_joints_cases as jc
import xprec_pairs_cases as pc
import xprec_pairs_model as pm
from constraint_solver_amd import capi
from xprec_cases import TAU
from xprec_joints_cases import EXACT_DEPTH, X, Y, Z, axis_to_object, ball, joints_of, limits_of, rod, tilt, to_world, yaw
from xprec_pairs_cases import CUBE, GROUND_MU, HS, K_PAIRS, MUS, SLAB

K_DRIVES = K_PAIRS
INF = float("inf")
SUBSTEPS = 12
NO_DRIVES = np.zeros(0, dtype=capi.JOINT_DRIVE_DTYPE)
ANGULAR = (capi.DRIVE_ANGLE, capi.DRIVE_ANGULAR_VELOCITY)


def drives_of(rows):
    """rows of dicts with the fields of xpbd_joint_drive (max_force defaults to +inf, the references to y)."""
    out = np.zeros(len(rows), dtype=capi.JOINT_DRIVE_DTYPE)
    for k, r in enumerate(rows):
        out[k]["max_force"], out[k]["ref_a"], out[k]["ref_b"] = INF, Y, Y
        for key, value in r.items():
            out[k][key] = value
    return out


def perpendicular(direction, turn=0.0):
    """A unit vector perpendicular to `direction`, turned by `turn` about it."""
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    u = np.cross(d, X if abs(d[0]) < 0.9 else Y)
    u /= np.linalg.norm(u)
    return u * np.cos(turn) + np.cross(d, u) * np.sin(turn)


def slider(bodies, a, b, world, direction, error=(0.0, 0.0, 0.0), lean=(0.0, 0.0, 0.0)):
    """A slider of bodies a, b through the world point `world` along `direction`; b's anchor `error` away, its axis `lean` off."""
    d = np.asarray(direction, dtype=np.float64)
    return ball(bodies, a, b, world, error, kind=capi.JOINT_SLIDER, axis_a=axis_to_object(bodies[a], d),
                axis_b=axis_to_object(bodies[b], d + lean))


def hinge(bodies, a, b, world, direction, error=(0.0, 0.0, 0.0), lean=(0.0, 0.0, 0.0)):
    d = np.asarray(direction, dtype=np.float64)
    return ball(bodies, a, b, world, error, kind=capi.JOINT_HINGE, axis_a=axis_to_object(bodies[a], d),
                axis_b=axis_to_object(bodies[b], d + lean))


def refs(bodies, joint_row, phi=0.0):
    """ref_a, ref_b of an angular drive or HINGE limit of the joint: perpendicular to its axes, b's turned by `phi` about
    its axis ahead of a's (the angle the joint starts at, to the misalignment of the axes)."""
    a, b = joint_row["body_a"], joint_row["body_b"]
    ref_a = perpendicular(joint_row["axis_a"])
    world_a = jc._rot(bodies[a][34:38], ref_a)
    axis_b_world = jc._rot(bodies[b][34:38], joint_row["axis_b"])
    flat = world_a - axis_b_world * (world_a @ axis_b_world)
    flat /= np.linalg.norm(flat)
    world_b = flat * np.cos(phi) + np.cross(axis_b_world, flat) * np.sin(phi)
    return dict(ref_a=ref_a, ref_b=axis_to_object(bodies[b], world_b))


def travel(bodies, row):
    """s of a slider row on the bodies as placed."""
    a, b = row["body_a"], row["body_b"]
    d = to_world(bodies[b], row["anchor_b"]) - to_world(bodies[a], row["anchor_a"])
    return float(d @ jc._rot(bodies[a][34:38], row["axis_a"]))


def centre(body):
    return to_world(body, (0.5, 0.5, 0.5))


# ---- (a) lifts --------------------------------------------------------------------------------------------------------
def scene_lifts(h, seed=61):
    """Two static slabs (tops at z = 0.5).  On slab 0: `stall` (vertical slider, VELOCITY up, max_force 5 N below the 9.81 N
    load), `lift` under `rider` (vertical slider, VELOCITY up with 50 N; the rider on a slider to the lift tilted 0.5 rad,
    soft POSITION drive), `ramp` (slider tilted 0.5 rad, stiff POSITION drive, SLIDE limit 5 mm violated from the start).  On
    slab 1: `drag` (horizontal slider, VELOCITY 0.5 m/s, SLIDE limit reached after five to six frames), `prism` (vertical
    slider + LIMIT_HINGE 0/0, SLIDE limit that never binds, soft ANGLE drive and VELOCITY drive pressing it down at 0.3 m/s).  Beside
    slab 1 on the ground: `floor` (horizontal slider to slab 1, POSITION drive with compliance, SLIDE limit never binding)."""
    rng = np.random.default_rng(seed)
    top = 0.5
    bodies, labels, rows, lims, drvs = [], [], [], [], []

    def box(label, x, y, z, depth, size=0.03):
        bodies.append(pc.new_body(CUBE, (x, y, z - rng.uniform(*depth)), tilt(rng, size), velocity=rng.uniform(-0.1, 0.1, 3),
                                  spin=rng.uniform(-1.0, 1.0, 3)))
        labels.append(label)
        return len(bodies) - 1

    def small():
        return rng.uniform(-0.004, 0.004, 3)

    for k in range(2):
        bodies.append(pc.new_body(SLAB, (8.0 * k, 0.0, -3.5), static=True))
        labels.append("slab")
    tilted = np.array([np.sin(0.5), 0.0, np.cos(0.5)])
    stall = box("stall", 0.3, 0.3, top, (0.002, 0.008))
    rows.append(slider(bodies, 0, stall, centre(bodies[stall]), Z, small(), rng.normal(size=3) * 0.01))
    drvs.append(dict(joint=len(rows) - 1, kind=capi.DRIVE_VELOCITY, target=0.5, max_force=5.0))
    lift = box("lift", 2.4, 0.3, top, (0.002, 0.008))
    rows.append(slider(bodies, 0, lift, centre(bodies[lift]), Z, small(), rng.normal(size=3) * 0.01))
    drvs.append(dict(joint=len(rows) - 1, kind=capi.DRIVE_VELOCITY, target=0.2, max_force=50.0))
    rider = box("rider", 2.5, 0.4, top + 1.0, (0.012, 0.02))
    rows.append(slider(bodies, lift, rider, centre(bodies[rider]), tilted, small(), rng.normal(size=3) * 0.01))
    drvs.append(dict(joint=len(rows) - 1, kind=capi.DRIVE_POSITION, target=travel(bodies, rows[-1]) + 0.01, compliance=0.01))
    ramp = box("ramp", 0.3, 2.4, top, (0.002, 0.008))
    rows.append(slider(bodies, ramp, 0, centre(bodies[ramp]), tilted, small(), rng.normal(size=3) * 0.01))   # the slab is b
    s0 = travel(bodies, rows[-1])
    drvs.append(dict(joint=len(rows) - 1, kind=capi.DRIVE_POSITION, target=s0 - 0.01))
    lims.append((len(rows) - 1, capi.LIMIT_SLIDE, s0 + 0.005, s0 + 0.3))                                     # binds at once
    drag = box("drag", 8.3, 0.3, top, (0.002, 0.008))
    rows.append(slider(bodies, 1, drag, centre(bodies[drag]), X, small(), rng.normal(size=3) * 0.01))
    bodies[drag][22:25] = [0.5, 0.0, 0.0]
    s0 = travel(bodies, rows[-1])
    drvs.append(dict(joint=len(rows) - 1, kind=capi.DRIVE_VELOCITY, target=0.5))
    lims.append((len(rows) - 1, capi.LIMIT_SLIDE, s0 - 1.0, s0 + 0.5 * h * 5.5))                             # starts to bind
    prism = box("prism", 8.3, 2.4, top, (0.002, 0.008))
    rows.append(slider(bodies, 1, prism, centre(bodies[prism]), Z, small(), rng.normal(size=3) * 0.01))
    k = len(rows) - 1
    lims.append((k, capi.LIMIT_HINGE, 0.0, 0.0, *refs(bodies, rows[k]).values()))
    lims.append((k, capi.LIMIT_SLIDE, travel(bodies, rows[k]) - 1.0, travel(bodies, rows[k]) + 1.0))         # never binds
    drvs.append(dict(joint=k, kind=capi.DRIVE_ANGLE, target=0.05, compliance=0.005, **refs(bodies, rows[k])))
    drvs.append(dict(joint=k, kind=capi.DRIVE_VELOCITY, target=-0.3))
    floor = box("floor", 12.6, 1.0, 0.0, (0.002, 0.008))
    rows.append(slider(bodies, 1, floor, centre(bodies[floor]), X, small(), rng.normal(size=3) * 0.01))
    drvs.append(dict(joint=len(rows) - 1, kind=capi.DRIVE_POSITION, target=travel(bodies, rows[-1]) + 0.02, compliance=0.002))
    lims.append((len(rows) - 1, capi.LIMIT_SLIDE, travel(bodies, rows[-1]) - 0.5, travel(bodies, rows[-1]) + 0.5))
    n = len(bodies)
    order = rng.permutation(len(drvs))
    return {"bodies": np.array(bodies), "sid": np.array([SLAB] * 2 + [CUBE] * (n - 2), dtype=np.uint32), "labels": np.array(labels),
            "joints": joints_of(rows), "limits": limits_of([lims[i] for i in rng.permutation(len(lims))]),
            "drives": drives_of([drvs[i] for i in order]), "mu": MUS[rng.integers(0, len(MUS), n)], "exact": ()}


# ---- (b) wheels -------------------------------------------------------------------------------------------------------
CROSSING_START = np.pi - 1e-3
CROSSING_RATE = 1e-3 / 2.5             # radians per frame


def scene_wheels(h, seed=71):
    """Two static slabs, eight boxes lying on them, seven hinged to its slab about a (nearly) vertical axis through its
    centre, two of them against a free neighbour box, the eighth on a slider: `spin` (ANGULAR_VELOCITY 2 rad/s), `cross` (ANGULAR_VELOCITY from
    phi = pi - 1e-3 at 1e-3 rad per 2.5 frames, the box already turning at 0.8 of that rate), `plus` and `minus` (ANGLE targets
    +pi and -pi exactly, from 0.01 and 0.02 rad short of them), `zero` (ANGLE target 0 from 0.03 rad, soft), `weak`
    (ANGULAR_VELOCITY 5 rad/s with 0.5 N m), `stop` (HINGE limit +-0.01 rad, phi 0.012 rad, ANGLE drive to 0.2 rad); and `latch`,
    the one box that is not a wheel: a horizontal slider whose SLIDE limit is violated by 4 mm (the control without the SLIDE
    limits needs one in this scene too)."""
    rng = np.random.default_rng(seed)
    top = 0.5
    bodies, labels, rows, lims, drvs = [], [], [], [], []
    for k in range(2):
        bodies.append(pc.new_body(SLAB, (8.0 * k, 20.0, -3.5), static=True))
        labels.append("slab")
    rate = CROSSING_RATE / h
    spots = [("spin", 0, 0.3, 0.3), ("cross", 0, 2.7, 0.3), ("plus", 0, 0.3, 2.7), ("minus", 0, 2.7, 2.7),
             ("zero", 1, 0.3, 0.3), ("weak", 1, 2.5, 0.3), ("stop", 1, 1.6, 2.7), ("latch", 1, 0.15, 2.75)]
    for label, slab, x, y in spots:
        spin = np.array([0.0, 0.0, 0.8 * rate]) if label == "cross" else rng.uniform(-0.5, 0.5, 3)
        bodies.append(pc.new_body(CUBE, (8.0 * slab + x, 20.0 + y, top - rng.uniform(0.002, 0.008)), yaw(rng.uniform(-0.2, 0.2)),
                                  velocity=rng.uniform(-0.05, 0.05, 3), spin=spin))
        labels.append(label)
        b = len(bodies) - 1
        lean = rng.normal(size=3) * 0.01
        a, c = (b, slab) if label == "minus" else (slab, b)                      # one wheel is the joint's body a
        if label == "latch":
            rows.append(slider(bodies, slab, b, centre(bodies[b]), X, rng.uniform(-0.003, 0.003, 3), lean))
            lims.append((len(rows) - 1, capi.LIMIT_SLIDE, travel(bodies, rows[-1]) + 0.004, travel(bodies, rows[-1]) + 0.5))
            continue
        rows.append(hinge(bodies, a, c, centre(bodies[b]), Z, rng.uniform(-0.003, 0.003, 3), lean))
        k = len(rows) - 1
        if label == "spin":
            drvs.append(dict(joint=k, kind=capi.DRIVE_ANGULAR_VELOCITY, target=2.0, **refs(bodies, rows[k], 0.4)))
        elif label == "cross":
            drvs.append(dict(joint=k, kind=capi.DRIVE_ANGULAR_VELOCITY, target=rate, **refs(bodies, rows[k], CROSSING_START)))
        elif label == "plus":
            drvs.append(dict(joint=k, kind=capi.DRIVE_ANGLE, target=np.pi, **refs(bodies, rows[k], np.pi - 0.01)))
        elif label == "minus":
            drvs.append(dict(joint=k, kind=capi.DRIVE_ANGLE, target=-np.pi, **refs(bodies, rows[k], -np.pi + 0.02)))
        elif label == "zero":
            drvs.append(dict(joint=k, kind=capi.DRIVE_ANGLE, target=0.0, compliance=0.01, **refs(bodies, rows[k], 0.03)))
        elif label == "weak":
            drvs.append(dict(joint=k, kind=capi.DRIVE_ANGULAR_VELOCITY, target=5.0, max_force=0.5, **refs(bodies, rows[k], -1.0)))
        else:
            lims.append((k, capi.LIMIT_HINGE, -0.01, 0.01, *refs(bodies, rows[k], 0.012).values()))
            drvs.append(dict(joint=k, kind=capi.DRIVE_ANGLE, target=0.2, **refs(bodies, rows[k], 0.012)))
    for label in ("spin", "weak"):                                                # free neighbours 5 mm into the wheel's side
        wheel = bodies[labels.index(label)]
        bodies.append(pc.new_body(CUBE, wheel[31:34] + jc._rot(wheel[34:38], (0.1, 0.995, 0.0)), wheel[34:38], velocity=(0.0, -0.1, 0.0)))
        labels.append("neighbour")
    n = len(bodies)
    return {"bodies": np.array(bodies), "sid": np.array([SLAB] * 2 + [CUBE] * (n - 2), dtype=np.uint32), "labels": np.array(labels),
            "joints": joints_of(rows), "limits": limits_of(lims), "drives": drives_of([drvs[i] for i in rng.permutation(len(drvs))]),
            "mu": MUS[rng.integers(0, len(MUS), n)], "exact": ()}


# ---- (c) exact --------------------------------------------------------------------------------------------------------
def scene_exact(h):
    """Binary-exact poses, identity rotations, at rest, no forces, re-made every frame: a static slab (top at z = 0.5), three
    boxes EXACT_DEPTH deep in it and a box EXACT_DEPTH deep on each.  The poses stay exact up to the joint pass (the pair
    points are entries of the same Jacobi pass), so every `== 0` of the header is met exactly and decided by the stated rule:
      unit 1  slab -> lower box, slider along x, d = (1/4, 0, 0): no perpendicular entry; SLIDE upper bound 1/4 == s: no entry;
              a VELOCITY drive is its one extra entry.  Lower -> upper box: hinge along z, aligned (no hinge entry), anchors
              2^-7 m apart, ANGLE drive with phi == target == 0: no entry
      unit 2  lower -> upper box, slider along z, d = (2^-6, 0, 1/8): a perpendicular entry; POSITION target 1/8 == s: no entry
      unit 3  upper -> lower box (body_a > body_b), slider along y with d = 0 exactly and a SLIDE limit [0, 1]: s == lower;
              VELOCITY and ANGULAR_VELOCITY drives with target 0 on bodies at rest: e == 0, so the unit has no extra entry"""
    kw = {"gravity": False}
    top, d = 0.5, EXACT_DEPTH
    bodies = [pc.new_body(SLAB, (100.0, 0.0, -3.5), static=True)]
    for k in range(3):
        bodies.append(pc.new_body(CUBE, (100.25 + 1.25 * k, 0.5, top - d), **kw))
        bodies.append(pc.new_body(CUBE, (100.5 + 1.25 * k, 0.75, top + 1.0 - 2 * d), **kw))
    rows = [dict(body_a=0, body_b=1, anchor_a=(0.5, 1.0, 4.0), anchor_b=(0.5, 0.5, d), kind=capi.JOINT_SLIDER, axis_a=X, axis_b=X),
            dict(body_a=1, body_b=2, anchor_a=(0.5, 0.5, 1.0), anchor_b=(0.25, 0.25, 2 * d), kind=capi.JOINT_HINGE, axis_a=Z, axis_b=Z),
            dict(body_a=3, body_b=4, anchor_a=(0.5, 0.5, 1.0), anchor_b=(0.25 + 2 * d, 0.25, 0.125 + d), kind=capi.JOINT_SLIDER,
                 axis_a=Z, axis_b=Z),
            dict(body_a=6, body_b=5, anchor_a=(0.25, 0.25, d), anchor_b=(0.5, 0.5, 1.0), kind=capi.JOINT_SLIDER, axis_a=Y, axis_b=Y)]
    lims = [(0, capi.LIMIT_SLIDE, -1.0, 0.25), (3, capi.LIMIT_SLIDE, 0.0, 1.0)]
    drvs = [dict(joint=0, kind=capi.DRIVE_VELOCITY, target=0.25), dict(joint=1, kind=capi.DRIVE_ANGLE, target=0.0, ref_a=X, ref_b=X),
            dict(joint=2, kind=capi.DRIVE_POSITION, target=0.125), dict(joint=3, kind=capi.DRIVE_VELOCITY, target=0.0),
            dict(joint=3, kind=capi.DRIVE_ANGULAR_VELOCITY, target=0.0, ref_a=X, ref_b=X)]
    labels = ["slab"] + ["lower", "upper"] * 3
    return {"bodies": np.array(bodies), "sid": np.array([SLAB] + [CUBE] * 6, dtype=np.uint32), "labels": np.array(labels),
            "joints": joints_of(rows), "limits": limits_of(lims), "drives": drives_of(drvs), "mu": None,
            "exact": tuple(range(7)), "refresh_every_frame": True}


# ---- (d) edge bodies at the ends of sliders and driven hinges -----------------------------------------------------------
def scene_ends(h, seed=81):
    """From xprec_pairs_cases.scene_edge: one touching pair (an edge body and a box) per category, two of mass_extreme
    (inverse mass 1e-6 and 1e6), and the two boxes on static slabs: 18 bodies.  Pairs are joined in turn by a driven slider
    and a driven hinge (POSITION, ANGLE, VELOCITY, ANGULAR_VELOCITY in turn; every third soft, every fourth force-limited);
    pair 1 with body_a > body_b; pair 0 also by a rod; ball joints (no extras) between the boxes of neighbouring pairs
    interleaved; the box on slab 0 is a hub with 12 driven joints to its slab, six sliders and six hinges, its being body a
    of every other one.  The drives are listed in a shuffled order."""
    rng = np.random.default_rng(seed)
    all_bodies, all_sid, all_labels = pc.scene_edge(h)
    keep, seen = [], {}
    for k in range(18):
        cat = all_labels[2 * k]
        seen[cat] = seen.get(cat, 0) + 1
        if seen[cat] == 1 or (cat == "mass_extreme" and seen[cat] == 2):
            keep += [2 * k, 2 * k + 1]
    keep += [36, 37, 38, 39]
    bodies, sid, labels = all_bodies[keep].copy(), all_sid[keep], all_labels[keep]
    n_pairs = (len(keep) - 4) // 2
    rows, lims, drvs = [], [], []

    def drive(k, kind, target):
        d = dict(joint=k, kind=kind, target=target)
        if len(drvs) % 3 == 1:
            d["compliance"] = rng.uniform(0.001, 0.01)
        if len(drvs) % 4 == 2:
            d["max_force"] = rng.uniform(0.5, 5.0)
        if kind in ANGULAR:
            d.update(refs(bodies, rows[k], rng.uniform(-0.5, 0.5)))
        drvs.append(d)

    for k in range(n_pairs):
        a, b = 2 * k, 2 * k + 1
        world = 0.5 * (to_world(bodies[a], pc.table()[1][int(sid[a])]["centroid"]) + centre(bodies[b]))
        i, j = (b, a) if k == 1 else (a, b)
        make = slider if k % 2 == 0 else hinge
        # the axis is the line of the two centres: a slider's drive presses the box against the edge body, a hinge holds the
        # box's centre 3 mm deeper than it is, 1 to 20 mm deep, and its drive spins the box about that line
        d = centre(bodies[b]) - to_world(bodies[a], pc.table()[1][int(sid[a])]["centroid"])
        rows.append(make(bodies, i, j, world if k % 2 == 0 else centre(bodies[b]), d,
                         rng.uniform(-0.005, 0.005, 3) * (1.0 if k % 2 == 0 else 0.4) - (0.0 if k % 2 == 0 else 0.003) * d / np.linalg.norm(d),
                         rng.normal(size=3) * 0.05))
        kind = (capi.DRIVE_POSITION, capi.DRIVE_ANGLE, capi.DRIVE_VELOCITY, capi.DRIVE_ANGULAR_VELOCITY)[k % 4]
        target = {capi.DRIVE_POSITION: travel(bodies, rows[-1]) - 0.01, capi.DRIVE_ANGLE: 0.1, capi.DRIVE_VELOCITY: -0.4,
                  capi.DRIVE_ANGULAR_VELOCITY: 1.5}[kind]
        drive(len(rows) - 1, kind, target)
        if k % 2 == 0:
            s0 = travel(bodies, rows[-1])
            lims.append((len(rows) - 1, capi.LIMIT_SLIDE, s0 - (0.5 if k % 4 else -0.002), s0 + 0.5))
        if k == 0:
            rows.append(rod(bodies, a, b, (0.2, 0.3, 0.1), (0.3, 0.1, 0.2), 0.02))                 # the pair joined twice
        if k + 1 < n_pairs and np.linalg.norm(bodies[b][31:34] - bodies[2 * k + 3][31:34]) < 100.0:
            rows.append(rod(bodies, b, 2 * k + 3, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), 0.01))         # no extras
    base = 2 * n_pairs
    slab, hub = base, base + 1
    for k in range(12):
        corner = to_world(bodies[hub], (k % 2, k // 2 % 2, 0.5 * (k // 4)))
        d = rng.normal(size=3)
        a, b = (hub, slab) if k % 2 else (slab, hub)
        make = slider if k < 6 else hinge
        rows.append(make(bodies, a, b, corner, d, rng.uniform(-0.004, 0.004, 3), rng.normal(size=3) * 0.02))
        kind = (capi.DRIVE_POSITION, capi.DRIVE_VELOCITY)[k % 2] if k < 6 else (capi.DRIVE_ANGLE, capi.DRIVE_ANGULAR_VELOCITY)[k % 2]
        target = {capi.DRIVE_POSITION: travel(bodies, rows[-1]) + 0.005, capi.DRIVE_ANGLE: 0.05, capi.DRIVE_VELOCITY: 0.2,
                  capi.DRIVE_ANGULAR_VELOCITY: -1.0}[kind]
        drive(len(rows) - 1, kind, target)
    joints = joints_of(rows)
    assert ((joints["body_a"] == hub) | (joints["body_b"] == hub)).sum() == 12 and (joints["body_a"] > joints["body_b"]).any()
    drives = drives_of([drvs[i] for i in rng.permutation(len(drvs))])
    assert not np.array_equal(drives["joint"], np.sort(drives["joint"]))
    return {"bodies": bodies, "sid": sid.astype(np.uint32), "labels": labels, "joints": joints, "limits": limits_of(lims),
            "drives": drives, "mu": None, "exact": ()}


# name -> (builder, h, friction?, depenetration speed)
def _scenes():
    out = {}
    for h in HS:
        tag = "h%d" % round(1.0 / h)
        out["lifts-" + tag] = (scene_lifts, h, False, 0.0)
        out["wheels-" + tag] = (scene_wheels, h, False, 0.0)
        out["exact-" + tag] = (scene_exact, h, False, 0.0)
        out["ends-" + tag] = (scene_ends, h, False, 0.0)
        out["mixed-" + tag] = (scene_lifts, h, True, 3.0)
    return out


SCENES = _scenes()
MAX_BODIES = 24


@functools.lru_cache(maxsize=None)
def build(name):
    builder, h, friction, speed = SCENES[name]
    s = dict(builder(h))
    assert len(s["sid"]) <= MAX_BODIES
    s.update(h=h, speed=speed, mu=s["mu"] if friction else None, ground_mu=GROUND_MU if friction else np.inf)
    s["ext"] = np.maximum(pc.extents(s["sid"], s["bodies"]), jc.arms(s))
    return s


def model(name, state, num=None, mutation=None, tau=0.0, manifolds=None, without=()):
    """The model's substep of the scene from `state`.  without: "drives" and / or "slide limits" left out (the controls)."""
    s = build(name)
    limits = s["limits"][s["limits"]["kind"] != capi.LIMIT_SLIDE] if "slide limits" in without else s["limits"]
    return pm.substep(state, pc.table()[1], s["sid"], s["h"], manifolds, s["mu"], s["ground_mu"], s["speed"], num=num,
                      mutation=mutation, tau=tau, joints=s["joints"], limits=limits,
                      drives=NO_DRIVES if "drives" in without else s["drives"])


def errors(name, got, res, start):
    return xk.scene_errors(build(name), got, res, start)


def excluded(res):
    """xprec_joints_cases.excluded, and the extras' own: a SLIDE limit whose s is within (0, TAU] of a bound, a drive whose
    |e| is in (0, TAU] (exactly 0 is the stated skip: entry or no entry changes the count), the argument of wrap within TAU of
    +-pi.  |r| of the perpendicular term is in joint_cond.  The clamp is continuous and excludes nothing."""
    x = jc.excluded(res)
    for key in ("slide_margin", "drive_margin"):
        x = x | xk.in_band(res[key])
    return x | (res["drive_wrap_margin"] <= TAU)


@functools.lru_cache(maxsize=None)
def trajectory(name):
    """Returns dict of the scene (build) and frames: [(start, want, res, want)]: `want` the f64 evaluation's state after the
    substep, res the longdouble model's result from `start` with its one-ulp sensitivity (the tuple has the layout of
    xprec_joints_cases.trajectory)."""
    s = build(name)
    exact = list(s["exact"])
    state, out = s["bodies"], []
    for f in range(SUBSTEPS):
        exact_now = bool(exact) and (f == 0 or s.get("refresh_every_frame", False))
        if exact and f and exact_now:
            state = state.copy()
            state[exact] = s["bodies"][exact]
        res, want = xk.model_frame(s, functools.partial(model, name), state, f, exact if exact_now else ())
        out.append((state, want, res, want))
        state = want
    return dict(s, frames=out)


def both(res):
    """The body-substeps that carry an extra entry and a pair or ground point."""
    return (res["n_extra"] > 0) & ((res["n_points"] > 0) | (res["mask"] != 0))


def check_states(name, got_states):
    """got_states[f]: the state after substep f of an implementation under test.  Asserts the bound on every body-substep
    that is not excluded; returns (normalised errors, excluded, carries extra entry and contact point), lists over frames."""
    t = trajectory(name)
    return xk.check_frames(name, [(start, res, t) for start, _, res, _ in t["frames"]], got_states, errors=xk.scene_errors,
                           excluded=lambda res, scene: excluded(res), bound=lambda res: K_DRIVES,
                           carries=lambda res, scene: both(res))


def crossing(name):
    """The frames f of a wheels scene where the `cross` wheel's phi is just below +pi in frame f and just above -pi in frame
    f + 1, neither frame excluded for the wheel."""
    t = trajectory(name)
    wheel = int(np.nonzero(t["labels"] == "cross")[0][0])
    index = int(np.nonzero(t["drives"]["target"] == CROSSING_RATE / t["h"])[0][0])
    phi = [[d[4] for d in fr[2]["drives"] if d[0] == index][0] for fr in t["frames"]]
    ok = [not excluded(fr[2])[wheel] for fr in t["frames"]]
    return [f for f in range(len(phi) - 1) if np.pi - 0.01 < phi[f] <= np.pi and -np.pi <= phi[f + 1] < -np.pi + 0.01 and ok[f] and ok[f + 1]]


def seen(names):
    """Over the scenes, what was seen both ways: {("perp" | "slide" | drive kind, binding?)} and {clamped?} of drive entries."""
    kinds, clamps = set(), set()
    for name in names:
        for _, _, res, _ in trajectory(name)["frames"]:
            kinds |= {("perp", length != 0) for _, length in res["perps"]}
            kinds |= {("slide", e != 0) for _, _, e in res["slides"]}
            kinds |= {(kind, e != 0) for _, kind, e, _, _ in res["drives"]}
            clamps |= {clamped for _, _, e, clamped, _ in res["drives"] if e != 0}
    return kinds, clamps
