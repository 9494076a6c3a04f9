"""Crafted terrain distance queries with known answers, shared by tests/test_terrain_distance_model.py (which asserts the answers on
the CPU model) and tests/test_gpu_terrain_distance.py (walk == brute force == model on the device).  Fields at binary spacing --
cells of 0.5 x 0.25, heights multiples of 1/8 -- so that the arithmetic of the expected answers is exact.

A case is (name, field, query record); a field is (heights (ny, nx), origin, cell).  The one polytope is the unit cube
raycast_model.box(), spanning [0, 1]^3 in its own space: vertex 0 at its origin, face 0 its bottom (-z), edge 0 along x from
vertex 0."""
import math

import numpy as np

import distance_model as dm
import raycast_model as rm

ORIGIN, CELL = (-1.0, 2.0), (0.5, 0.25)
CUBE = 0
IDENT = (1.0, 0.0, 0.0, 0.0)


def polytopes():
    return [rm.box()]


def field(heights):
    return (np.asarray(heights, dtype=np.float64), ORIGIN, CELL)


ONE_CELL = field([[0.25, 0.25], [0.25, 0.25]])                                # x in [-1, -0.5], y in [2, 2.25]
FLAT = field(np.full((3, 4), 0.25))                                           # 4 x 3, x in [-1, 0.5], y in [2, 2.5]
ROOF = field([[0.0, 0.5, 0.0, 0.0]] * 3)                                      # 4 x 3, a ridge along y at x = -0.5
PEAK = field([[0.0] * 5, [0.0, 0.0, 0.5, 0.0, 0.0], [0.0] * 5])               # 5 x 3, one peak at (0, 2.25)
RIMS = field([[0.0, 0.5, 0.0, 0.5, 0.0]] * 3)                                 # 5 x 3, a valley between the rims x = -0.5 and x = 0.5
DOWNHILL = field([[0.5, 0.375, 0.25, 0.125, 0.0]] * 3)                        # 5 x 3, falling by 0.25 per metre of x
RIDGE = field([[0.0, 0.0, 0.5, 0.0, 0.0]] * 3)                                # 5 x 3, a ridge along y at x = 0
LIFT = 0.25
C8, S8 = math.cos(math.pi / 8.0), math.sin(math.pi / 8.0)                     # a quarter of pi about x: the cube stands on edge 0


def point(position, max_distance=np.inf):
    return dm.one(position, max_distance=max_distance)


def cube(position, rotation=IDENT, max_distance=np.inf):
    return dm.one(position, rotation=rotation, shape=CUBE, max_distance=max_distance)


def cases():
    return [
        ("point_over_triangle", FLAT, point((-0.625, 2.0625, 1.25))),
        ("point_over_grid_line", FLAT, point((-0.5, 2.0625, 1.25))),
        ("point_on_surface", FLAT, point((-0.625, 2.0625, 0.25))),
        ("point_beside_field", FLAT, point((-2.0, 2.0625, 0.25))),
        ("point_over_ridge", ROOF, point((-0.5, 2.125, 1.5))),
        ("point_under_ground_inside", FLAT, point((-0.625, 2.0625, -1.0))),
        ("point_under_ground_outside", FLAT, point((-2.0, 2.0625, -0.75))),
        ("cube_over_peak", PEAK, cube((-0.5, 1.75, 1.0))),
        ("cube_edge_across_rim", RIMS, cube((-1.0, 2.125, 1.0), (C8, S8, 0.0, 0.0))),
        ("cube_vertex_under_slope", DOWNHILL, cube((-0.75, 2.0625, 0.4375 - 2.0 ** -20))),
        ("cube_on_ridge", RIDGE, cube((-0.5, 1.75, 0.45))),
        ("cube_over_ridge", RIDGE, cube((-0.5, 1.75, 0.5 + LIFT))),
        ("cube_over_peak_at_reach", PEAK, cube((-0.5, 1.75, 1.0), max_distance=0.5)),
        ("cube_over_peak_below_reach", PEAK, cube((-0.5, 1.75, 1.0), max_distance=float(np.nextafter(0.5, 0.0)))),
        # the one-cell field: over its lower triangle, over its diagonal, beside its corner, under it
        ("one_cell_over_triangle", ONE_CELL, point((-0.625, 2.0625, 0.75))),
        ("one_cell_over_diagonal", ONE_CELL, point((-0.75, 2.125, 0.75))),
        ("one_cell_beside_corner", ONE_CELL, point((-1.5, 1.5, 0.25))),
        ("one_cell_under", ONE_CELL, point((-0.75, 2.125, 0.0))),
        ("one_cell_cube_around", ONE_CELL, cube((-1.25, 1.75, 0.125))),
    ]


def by_field():
    """[(field, [names], query records)] with the cases grouped by their field, in order of first appearance."""
    groups = []
    for name, f, q in cases():
        for g in groups:
            if g[0] is f:
                g[1].append(name)
                g[2].append(q)
                break
        else:
            groups.append((f, [name], [q]))
    return [(f, names, np.concatenate(qs)) for f, names, qs in groups]
