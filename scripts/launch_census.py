#!/usr/bin/env python3
"""Which form of every contact-pipeline kernel a launcher picks, and with what launch shape: for a change to the launchers
that must leave every launch as it was.  A launch that picks the wrong lane width is bit-identical and only slower, so the
tests cannot see it; the kernel trace can.

  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python scripts/launch_census.py
        steps a few tiny worlds, each a few frames, one after the other in one process (the library: XPBD_HIP_LIB, or the
        tree's own).  Once with the parent's library, once with this tree's, into two directories.
  python scripts/launch_census.py --compare <parent dir> <this dir> [--out file.json]
        the two traces' ordered sequences of (kernel, grid, workgroup, LDS bytes) must be equal row for row, and together
        must hold every form in REQUIRED; prints the comparison as JSON and exits non-zero otherwise.

The worlds: plain; filters; jointed-pair exclusion; filters + jointed; each of those four with sleeping on; materials; terrain;
contact trace on; restitution without and with terrain; and one world of SMALL_WORLD + 1 bodies, plain and with materials,
on the fused (step) and the unfused (contacts_begin + contacts_substep) schedule."""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = 1.0 / 60.0
SMALL_WORLD = 16384          # xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body
FRAMES, SUBSTEPS, BODIES = 3, 4, 48

B = ("false", "true")
REQUIRED = sorted(
    [("k_neighbour_%s" % k, "%s, %s%s" % (f, j, i)) for k in ("count", "fill") for f in B for j in B for i in ("", ", xpbd::InertBodies")]
    + [("k_pair_solve_derive", "%s, %s" % (g, m)) for g in ("8", "1") for m in B]
    + [("k_integrate_ground", "false, false, %s" % t) for t in B]
    + [("k_restitution", t) for t in B]
    + [("k_pair_solve_integrate_ground", "false, %s, false" % g) for g in ("8", "1")])


def step_worlds():
    import numpy as np
    from constraint_solver_amd import capi

    kind = capi.SCENE_BOX_STACKS
    rng = np.random.default_rng(7)

    def world(n, **kw):
        bodies, sid = capi.scene_generate(kind, 1, n)
        w = capi.World(mode=capi.MODE_CONTACTS, **kw)
        w.set_polytopes(capi.scene_polytopes(kind))
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        w.upload(bodies, sid)
        return w

    def joints(n):
        j = np.zeros(n // 2, dtype=capi.JOINT_DTYPE)
        j["body_a"], j["body_b"] = np.arange(0, n - 1, 2), np.arange(1, n, 2)
        j["anchor_a"], j["anchor_b"] = [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]
        j["distance"] = 1.0
        return j

    def filters(n):
        f = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
        f["group"], f["mask"] = 1 << rng.integers(0, 2, n), rng.integers(1, 4, n)
        return f

    def frames(w, count=FRAMES, substeps=SUBSTEPS):
        for _ in range(count):
            w.step(DT, substeps)
        w.synchronize()

    heights = 0.05 * np.add.outer(np.arange(12.0), np.arange(12.0)) - 2.0
    terrain = (heights, (-40.0, -40.0), (8.0, 8.0))
    for sleeping in (False, True):
        for with_filters, jointed in ((False, False), (True, False), (False, True), (True, True)):
            with world(BODIES) as w:
                if jointed:
                    w.set_joints(joints(BODIES))
                if with_filters or jointed:
                    w.set_collision_filters(filters(BODIES) if with_filters else None, capi.FILTER_JOINTED if jointed else 0)
                if sleeping:
                    w.set_contact_report(True)
                    w.set_sleeping(0.5, 2.0, 30)
                frames(w)
    with world(BODIES) as w:
        w.set_materials(np.full(BODIES, 0.5), 0.7)
        frames(w)
    with world(BODIES) as w:
        w.set_terrain(*terrain)
        frames(w)
    with world(BODIES, trace_contacts=True) as w:
        frames(w)
    for with_terrain in (False, True):
        with world(BODIES) as w:
            w.set_restitution(np.full(BODIES, 0.5), 0.5, 0.0)
            if with_terrain:
                w.set_terrain(*terrain)
            frames(w)
    n = SMALL_WORLD + 1
    for materials in (False, True):
        with world(n) as w:
            if materials:
                w.set_materials(np.full(n, 0.5), 0.7)
            frames(w, 1, 3)                      # fused: integrate, two fused kernels, the last derive
            w.contacts_begin(DT)                 # unfused: integrate and derive per substep
            for _ in range(2):
                w.contacts_substep(DT / 2)
            w.synchronize()
    print("launch_census: stepped every world", flush=True)


def form_of(name):
    """('k_pair_solve_derive', '8, false') of a demangled kernel name; (name, '') without template arguments."""
    head = name.split("(anonymous namespace)::")[-1]
    m = re.match(r"(\w+)(?:<(.*)>)?\(", head) or re.match(r"(\w+)(?:<(.*)>)?$", head)
    if not m:
        return head, ""
    args = (m.group(2) or "").replace("(bool)0", "false").replace("(bool)1", "true").replace("(unsigned int)", "")
    return m.group(1), re.sub(r"(\d+)[uU]\b", r"\1", args)


def launches(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        raise SystemExit("%s: expected one kernel trace, found %d" % (directory, len(files)))
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Dispatch_Id"]))
    dims = lambda r, what: [int(r["%s_Size_%s" % (what, a)]) for a in "XYZ"]
    return [(r["Kernel_Name"], dims(r, "Grid"), dims(r, "Workgroup"), int(r.get("LDS_Block_Size", 0) or 0)) for r in rows]


def compare(parent_dir, this_dir, out):
    a, b = launches(parent_dir), launches(this_dir)
    first = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), None)
    if first is None and len(a) != len(b):
        first = min(len(a), len(b))
    forms = {}
    for name, grid, wg, lds in a + b:
        f = form_of(name)
        e = forms.setdefault("%s<%s>" % f if f[1] else f[0], {"launches": 0, "workgroup": wg[0], "lds_bytes": set()})
        e["launches"] += 1
        e["lds_bytes"].add(lds)
    reached = {form_of(name) for name, _, _, _ in a} & {form_of(name) for name, _, _, _ in b}
    missing = ["%s<%s>" % f for f in REQUIRED if f not in reached]
    res = {"what": "scripts/launch_census.py under rocprofv3 --kernel-trace, once with the parent's library (XPBD_HIP_LIB) and once "
                   "with this tree's: the ordered sequences of (kernel name, grid, workgroup, LDS bytes), compared row for row",
           "launches_parent": len(a), "launches_this_tree": len(b), "equal_row_for_row": first is None,
           "first_difference": None if first is None else {"row": first, "parent": a[first] if first < len(a) else None,
                                                           "this_tree": b[first] if first < len(b) else None},
           "required_forms": ["%s<%s>" % f for f in REQUIRED], "forms_not_reached": missing,
           "kernels": {k: {"launches_both_runs": v["launches"], "workgroup": v["workgroup"], "lds_bytes": sorted(v["lds_bytes"])}
                       for k, v in sorted(forms.items())}}
    text = json.dumps(res, indent=1)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    print(text)
    print("forms not reached:", missing)
    return 0 if first is None and not missing else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("PARENT_DIR", "THIS_DIR"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.out))
    step_worlds()


if __name__ == "__main__":
    main()
