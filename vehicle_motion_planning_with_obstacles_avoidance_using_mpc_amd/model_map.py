"""Occupancy grid -- host-side mirror of the reference's ``model_map.mapModel`` (src/model_map.py:14-101).
What the A* global planner needs: ``shape2grid`` and ``dilate_map`` (the disk dilation the route-seeded open-loop planner
searches on, restated in plain numpy: skimage is not a dependency); ``erode_map`` of the reference is unused and not
provided."""
import numpy as np


class mapModel:
    def __init__(self, map_size, resolution):
        rows = int((map_size[1] - 1) / resolution) + 1
        cols = int((map_size[0] - 1) / resolution) + 1
        self.grid_map = np.zeros((rows, cols))
        self.resolution = resolution

    def shape2grid(self, org_gridMap, obstacle_location):
        """Mark the axis-aligned bounding box of every obstacle polygon, clipped to the map: the part of a box outside
        the grid is dropped (the reference indexes cell by cell and raises there; ``obca_rasterise_batch`` clips too)."""
        grid = self.grid_map if (isinstance(org_gridMap, list) and len(org_gridMap) == 0) else org_gridMap
        for poly in obstacle_location:
            xs = [p[0] / self.resolution for p in poly]
            ys = [p[1] / self.resolution for p in poly]
            x0, y0 = int(min(xs)), int(min(ys))
            nx = int(max(xs) - min(xs)) + 1
            ny = int(max(ys) - min(ys)) + 1
            grid[max(y0, 0):max(y0 + ny, 0), max(x0, 0):max(x0 + nx, 0)] = 1   # a negative slice bound would wrap
        return grid

    def dilate_map(self, grid_map, dilation_level):
        return dilate_map(grid_map, dilation_level)


def dilate_map(grid_map, dilation_level):
    """Disk dilation (src/model_map.py:103-107) by the rule of ``obca_grid_dilate_batch``: out[r, c] = 1 iff some cell
    (r + dy, c + dx) inside the grid with dy^2 + dx^2 <= dilation_level^2 is non-zero, else 0; cells outside the grid
    count as free, level 0 copies (non-zero becomes 1).  Returns a uint8 array."""
    level = int(dilation_level)
    if level < 0:
        raise ValueError("dilation_level >= 0, got %d" % level)
    occ = np.asarray(grid_map) != 0
    rows, cols = occ.shape
    out = np.zeros((rows, cols), bool)
    for dy in range(-level, level + 1):
        for dx in range(-level, level + 1):
            if dy * dy + dx * dx > level * level:
                continue
            # out[r, c] |= occ[r + dy, c + dx] over the part of the shifted grid that stays inside
            r0, r1, c0, c1 = max(0, -dy), min(rows, rows - dy), max(0, -dx), min(cols, cols - dx)
            if r0 < r1 and c0 < c1:
                out[r0:r1, c0:c1] |= occ[r0 + dy:r1 + dy, c0 + dx:c1 + dx]
    return out.astype(np.uint8)
