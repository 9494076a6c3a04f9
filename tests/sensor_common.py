"""Shared by the sensor-body GPU tests (test_gpu_sensors.py) and their torch child process (sensor_device_child.py): the scenes,
the three kinds of world every pass-through test compares -- A flags its sensors, B gives the same bodies the collision filter
{group 0, mask 0} and flags nobody, C does neither -- and what one frame leaves behind."""
import numpy as np

from constraint_solver_amd import capi

DT = 1.0 / 60.0
GAP = 0.002
IDENT = (1.0, 0.0, 0.0, 0.0)
BIG, SMALL = 3.0, 0.5
# the mixed scene's three shapes, then a cube of edge BIG (shape 3) and one of edge SMALL (shape 4)
MIXED_NAMES = [("cube", 1.0), ("tetrahedron", 0.5), ("icosahedron", 0.5), ("cube", BIG), ("cube", SMALL)]
SHAPE_BIG, SHAPE_SMALL = 3, 4
BOX_NAMES = [("cube", 1.0), ("cube", BIG), ("cube", SMALL)]
CLUMP, CLUMP_SEED = 300, 5


def mixed_polytopes():
    return capi.scene_polytopes(capi.SCENE_MIXED) + [capi.polytope(capi.SHAPE_CUBE, BIG), capi.polytope(capi.SHAPE_CUBE, SMALL)]


def box_polytopes():
    return [capi.polytope(capi.SHAPE_CUBE), capi.polytope(capi.SHAPE_CUBE, BIG), capi.polytope(capi.SHAPE_CUBE, SMALL)]


def cube_rows(positions, fixed):
    """Unit-box rows (the seeded box scene's mass properties) at rest, upright, at `positions`; fixed: zero inverse mass and inertia."""
    positions = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    rows, _ = capi.scene_generate(capi.SCENE_BOXES, 3, len(positions))
    rows[:, 22:28] = 0.0
    rows[:, 34:38] = IDENT
    rows[:, 31:34] = positions
    if fixed:
        rows[:, 0:10] = 0.0
    return rows


def clump_scene(extra_sensor="kinematic"):
    """test_gpu_contact_report.py's clump -- cluster(SCENE_MIXED, 300, seed, 0.5) -- with four fixed bodies behind it: three big boxes
    that overlap the clump (300-302) and a unit box inside it (303), which `extra_sensor` == "kinematic" moves through the clump
    on a VELOCITY entry.  Sensors: every 10th body of the clump (dynamic), and the four.  Returns (bodies, sid, is_sensor, table)."""
    rng = np.random.default_rng(CLUMP_SEED)
    bodies, sid = capi.scene_generate(capi.SCENE_MIXED, CLUMP_SEED, CLUMP)
    bodies[:, 31:34] = rng.uniform(-0.5, 0.5, (CLUMP, 3))
    fixed = cube_rows([[-2.6, -1.0, 0.0], [0.1, -1.6, 0.0], [-1.2, 0.4, 0.2], [-1.2, 0.0, 0.3]], fixed=True)
    bodies = np.concatenate([bodies, fixed])
    sid = np.concatenate([sid, [SHAPE_BIG, SHAPE_BIG, SHAPE_BIG, 0]]).astype(np.uint32)
    is_sensor = np.zeros(len(bodies), dtype=np.uint8)
    is_sensor[0:CLUMP:10] = 1
    is_sensor[CLUMP:] = 1
    table = capi.kinematics([CLUMP + 3], capi.KINEMATIC_VELOCITY, [[6.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]]) if extra_sensor == "kinematic" else None
    return bodies, sid, is_sensor, table


def cells_scene(cells):
    """`cells` dynamic unit boxes (bodies 0 .. cells-1), each resting on its own fixed floor box (cells .. 2 cells-1) and
    overlapping its own small fixed sensor box (2 cells .. 3 cells-1), the cells 4 m apart: every dynamic body has exactly two
    neighbours, one of them a sensor."""
    w = int(np.ceil(np.sqrt(cells)))
    k = np.arange(cells)
    at = np.stack([4.0 * (k % w), 4.0 * (k // w), np.full(cells, 2.0)], axis=1)
    floors = cube_rows(at, fixed=True)
    boxes = cube_rows(at + [0.0, 0.0, 1.0 + GAP], fixed=False)
    probes = cube_rows(at + [0.8, 0.3, 1.8], fixed=True)           # (over the box's upper corner: out of reach of the floor's sphere)
    bodies = np.concatenate([boxes, floors, probes])
    sid = np.concatenate([np.zeros(2 * cells), np.full(cells, 2)]).astype(np.uint32)       # BOX_NAMES: 2 = the small cube
    is_sensor = np.zeros(3 * cells, dtype=np.uint8)
    is_sensor[2 * cells:] = 1
    return bodies, sid, is_sensor


def filters_for(is_sensor):
    """World B's filters: {0, 0} for the sensor bodies, every bit for the others (the default)."""
    f = np.zeros(len(is_sensor), dtype=capi.COLLISION_FILTER_DTYPE)
    f["group"] = f["mask"] = np.where(is_sensor != 0, 0, 0xFFFFFFFF)
    return f


def make_world(kind, polytopes, bodies, sid, is_sensor, narrowphase=capi.NARROWPHASE_SAT, restitution=False, materials=False, table=None,
               trace=True, report=True):
    """kind "A": sensors flagged; "B": the same bodies filtered out; "C": neither."""
    n = len(bodies)
    w = capi.World(mode=capi.MODE_CONTACTS, trace_contacts=trace)
    w.set_polytopes(polytopes)
    w.set_narrowphase(narrowphase)
    w.upload(bodies, sid)
    if report:
        w.set_contact_report(True)
    rng = np.random.default_rng(77)
    if materials:
        w.set_materials(rng.uniform(0.1, 1.0, n), ground_friction=0.6)
    if restitution:
        w.set_restitution(rng.uniform(0.2, 0.6, n), 0.3, 0.0)
    if table is not None:
        w.set_kinematics(table)
    if kind == "A":
        w.set_sensors(is_sensor)
    elif kind == "B":
        w.set_collision_filters(filters_for(is_sensor))
    return w


class Frame:
    """What a host can see after one step of a traced world."""

    def __init__(self, w, substeps):
        self.bodies = w.download()
        self.contacts = np.asarray(w.contacts()).copy()
        self.masks = w.contact_masks(substeps).copy()

    def same(self, other):
        return (self.bodies.tobytes() == other.bodies.tobytes() and self.contacts.tobytes() == other.contacts.tobytes()
                and self.masks.tobytes() == other.masks.tobytes())


def sensor_pairs(pairs, is_sensor):
    """Which of the report's records have a sensor end."""
    return (is_sensor[pairs["body_a"]] | is_sensor[pairs["body_b"]]) != 0


def rebased(pairs):
    """The records with first_point counted over these records alone."""
    out = pairs.copy()
    out["first_point"] = np.concatenate([[0], np.cumsum(out["n_points"])[:-1]]).astype(np.uint32) if len(out) else out["first_point"]
    return out


def occupancy_scene():
    """The clump scene without the kinematic entry, and three bodies more: a sensor nobody is near (304), a sensor whose only
    neighbour misses it (305: bounding spheres overlap, boxes 0.3 m apart) and that neighbour (306, dynamic)."""
    bodies, sid, is_sensor, _ = clump_scene(extra_sensor="fixed")
    more = np.concatenate([cube_rows([[100.0, 100.0, 5.0], [200.0, 0.0, 5.0]], fixed=True), cube_rows([[201.3, 0.0, 5.0]], fixed=False)])
    bodies = np.concatenate([bodies, more])
    sid = np.concatenate([sid, [0, 0, 0]]).astype(np.uint32)
    is_sensor = np.concatenate([is_sensor, [1, 1, 0]]).astype(np.uint8)
    return bodies, sid, is_sensor


LONELY, MISSED = CLUMP + 4, CLUMP + 5
OCC_FRAMES, OCC_SUBSTEPS = 3, 4


def occupancy_world():
    bodies, sid, is_sensor = occupancy_scene()
    w = make_world("A", mixed_polytopes(), bodies, sid, is_sensor, trace=False)
    for _ in range(OCC_FRAMES):
        w.step(DT, OCC_SUBSTEPS)
    return w, is_sensor
