"""Plain references for the planner and the rasteriser -- test infrastructure only, no product code imported.

``shortest_cost`` is a textbook Dijkstra on the 8-connected grid, ``check_route`` states what a reference trajectory of
the planner has to be (a shortest lattice route from the start's neighbour to the goal, with the yaw of every step), and
``rasterise`` marks obstacle boxes cell by cell with an explicit bounds test: clipping to the map is the contract."""
import heapq
import math

import numpy as np

SQRT2 = math.sqrt(2.0)
STEPS = tuple((dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if dr or dc)


def shortest_cost(grid, start, goal):
    """cost of a shortest 8-connected route start -> goal over free cells (grid != 1); a step costs 1 or sqrt(2), and a
    diagonal step may pass between two occupied cells, as in the reference.  The start cell itself may be occupied (the
    search leaves it).  None when the goal cannot be reached."""
    grid = np.asarray(grid)
    rows, cols = grid.shape
    start, goal = (int(start[0]), int(start[1])), (int(goal[0]), int(goal[1]))
    occ = (grid == 1).tolist()
    if occ[goal[0]][goal[1]] and goal != start:
        return None
    dist = {start: 0.0}
    done = set()
    heap = [(0.0, start)]
    while heap:
        d, cur = heapq.heappop(heap)
        if cur in done:
            continue
        if cur == goal:
            return d
        done.add(cur)
        for dr, dc in STEPS:
            r, c = cur[0] + dr, cur[1] + dc
            if not (0 <= r < rows and 0 <= c < cols) or occ[r][c]:
                continue
            nd = d + (SQRT2 if dr and dc else 1.0)
            if nd < dist.get((r, c), math.inf):
                dist[(r, c)] = nd
                heapq.heappush(heap, (nd, (r, c)))
    return None


def check_route(grid, start, goal, path, plen, cost=None):
    """asserts that path [3, path_max] / plen (> 0) is a valid reference trajectory for start -> goal (both (row, col)):
    integer free cells inside the grid, first point a neighbour of the start (the route excludes the start cell),
    consecutive points 8-neighbours, last point the goal, yaw = arctan2 of each step with the last one repeated, padding =
    the last point, and a cost equal to ``shortest_cost`` within plen * 2^-52 * cost: both are sums of at most plen terms
    1 and sqrt(2), each within plen * 2^-53 (relative) of the exact sum.  ``cost`` may carry a shortest_cost computed
    before.  Returns the route's cost."""
    grid = np.asarray(grid)
    rows, cols = grid.shape
    path = np.asarray(path, float)
    plen = int(plen)
    assert plen >= 1 and path.shape[0] == 3 and path.shape[1] >= plen, (plen, path.shape)
    xs, ys, yaw = path[0, :plen], path[1, :plen], path[2, :plen]
    assert np.array_equal(xs, np.rint(xs)) and np.array_equal(ys, np.rint(ys)), "points are not integer cells"
    c, r = xs.astype(np.int64), ys.astype(np.int64)
    assert (r >= 0).all() and (r < rows).all() and (c >= 0).all() and (c < cols).all(), "point outside the grid"
    assert not (grid[r, c] == 1).any(), "route crosses an occupied cell"
    dr = np.diff(np.concatenate([[int(start[0])], r]))
    dc = np.diff(np.concatenate([[int(start[1])], c]))
    assert (np.abs(dr) <= 1).all() and (np.abs(dc) <= 1).all() and ((dr != 0) | (dc != 0)).all(), \
        "points are not 8-neighbours (the first one of the start)"
    assert (int(r[-1]), int(c[-1])) == (int(goal[0]), int(goal[1])), "route does not end at the goal"
    if plen >= 2:
        want = np.arctan2(dr[1:].astype(float), dc[1:].astype(float))
        assert np.array_equal(yaw[:-1], want), "yaw is not arctan2 of the step"
        assert yaw[-1] == yaw[-2], "last yaw does not repeat the one before"
    else:
        assert yaw[0] == 0.0, "one-point route carries yaw 0"
    assert np.array_equal(path[:, plen:], np.repeat(path[:, plen - 1:plen], path.shape[1] - plen, axis=1)), \
        "padding does not repeat the last point"
    total = 0.0
    for diag in ((dr != 0) & (dc != 0)).tolist():
        total += SQRT2 if diag else 1.0
    best = shortest_cost(grid, start, goal) if cost is None else cost
    assert best is not None, "a route was returned but the goal is unreachable"
    assert abs(total - best) <= plen * 2.0 ** -52 * best, (total, best, plen)
    return total


def rasterise(boxes, res, rows, cols):
    """occupancy grid [rows, cols] uint8 of boxes [K, 4] = (xmin, ymin, xmax, ymax) in world units, with the float64
    divisions and truncations include/obca_mpc.h documents: x = int(xmin/res), y = int(ymin/res), cells x .. x +
    int(xmax/res - xmin/res) and y .. y + int(ymax/res - ymin/res) -- int() truncates towards zero.  A box with a NaN or
    with min > max is skipped; cells outside the map are dropped."""
    grid = np.zeros((rows, cols), np.uint8)
    for q in np.asarray(boxes, float).reshape(-1, 4):
        xmin, ymin, xmax, ymax = (float(v) / float(res) for v in q)
        if not (xmin <= xmax) or not (ymin <= ymax):
            continue
        x, y = int(xmin), int(ymin)
        xl, yl = int(xmax - xmin) + 1, int(ymax - ymin) + 1
        for r in range(y, y + yl):
            for c in range(x, x + xl):
                if 0 <= r < rows and 0 <= c < cols:
                    grid[r, c] = 1
    return grid


def edge_boxes(rows, cols, res):
    """the box list of the edge tests for a rows x cols map of cell size res, in world units: one box across each of the
    four edges and each corner, boxes wholly outside on every side, zero-width boxes (inside, on the far edge, outside),
    a box inside and one covering the whole map.  Name -> (xmin, ymin, xmax, ymax)."""
    W, H = cols * res, rows * res
    mx, my = 0.5 * W, 0.5 * H
    a, o = 1.6 * res, 2.5 * res                                  # reach inside / outside the map
    return {
        "inside": (0.3 * W, 0.3 * H, 0.3 * W + a, 0.3 * H + a),
        "left": (-o, my - a, a, my + a), "right": (W - a, my - a, W + o, my + a),
        "bottom": (mx - a, -o, mx + a, a), "top": (mx - a, H - a, mx + a, H + o),
        "corner00": (-o, -1.5 * res, a, a), "corner01": (W - a, -o, W + o, a),
        "corner10": (-o, H - a, a, H + o), "corner11": (W - a, H - a, W + o, H + o),
        "out_left": (-o - a, my, -o, my + a), "out_right": (W + o, my, W + o + a, my + a),
        "out_below": (mx, -o - a, mx + a, -o), "out_above": (mx, H + o, mx + a, H + o + a),
        "out_corner": (-o - a, -o - a, -o, -o),
        "zero_width": (0.4 * W, 0.2 * H, 0.4 * W, 0.2 * H + a), "zero_height": (0.2 * W, 0.6 * H, 0.2 * W + a, 0.6 * H),
        "point": (0.7 * W, 0.7 * H, 0.7 * W, 0.7 * H), "zero_on_edge": (W, my, W, my + a),
        "zero_outside": (-o, my, -o, my + a),
        "whole_map": (-o, -o, W + o, H + o), "exact_map": (0.0, 0.0, W - res, H - res),
    }


def box_polygon(q):
    """a box as the closed vertex list the host mirror (mapModel.shape2grid) takes"""
    x0, y0, x1, y1 = q
    return [[x0, y0], [x0, y1], [x1, y1], [x1, y0], [x0, y0]]


def serpentine(rows, cols):
    """maze with every odd row a wall and one gap at alternating ends (row 1 opens at the last column, row 3 at the first,
    ...), rows odd; returns (grid, start, goal): start = (0, 0), the goal in the last row at the far end from its gap."""
    assert rows % 2 == 1
    g = np.zeros((rows, cols), np.uint8)
    right = True
    for r in range(1, rows, 2):
        g[r, :] = 1
        g[r, cols - 1 if right else 0] = 0
        right = not right
    goal = (rows - 1, cols - 1 if right else 0)                  # `right` is now the side opposite the last gap
    return g, (0, 0), goal
