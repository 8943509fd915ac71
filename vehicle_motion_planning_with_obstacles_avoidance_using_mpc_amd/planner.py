"""Batched global planner on the GPU -- B grid A* searches at once (reference src/a_star.py:16-102 followed by
rebuild_path / create_reference_path, :137-200), producing the (3,P) reference trajectories the closed loop tracks
(reference src/closed_loop.py:340: ``update_path(..., type="A_star")``) directly in device memory.

``a_star.a_star`` stays the readable per-rollout mirror of the reference class; tests compare the two."""
import ctypes

import numpy as np

from . import _lib


def yaw_table():
    """arctan2(dy, dx) for the nine lattice steps, evaluated by numpy like the reference's create_reference_path"""
    t = np.zeros(9)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            t[(dy + 1) * 3 + (dx + 1)] = np.arctan2(float(dy), float(dx))
    return t


def plan_batch(grids, starts, goals, path_max=None, device=None):
    """grids [B,rows,cols] (1 = occupied; ``setting.org_gridMap``), starts / goals [B,2] as (row, col) =
    (pose_y, pose_x).  Returns device tensors path [B,3,path_max] (x, y, yaw; padded with the last point) and
    path_len [B] (negative: -1 no route, -2 open list overflow, -3 path_max too small, -4 start or goal outside the
    grid; the path of an instance with a negative code is left unwritten)."""
    import torch
    _lib.require_gpu("plan_batch")
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if isinstance(grids, torch.Tensor):                      # e.g. the output of rasterise_batch: stays on the device
        g = grids.to(device=dev, dtype=torch.uint8).contiguous()
    else:
        g = torch.as_tensor(np.ascontiguousarray(grids), device=dev).to(torch.uint8).contiguous()
    B, rows, cols = g.shape
    st = torch.as_tensor(np.ascontiguousarray(starts), device=dev).to(torch.int32).contiguous()
    go = torch.as_tensor(np.ascontiguousarray(goals), device=dev).to(torch.int32).contiguous()
    P = int(path_max) if path_max is not None else rows * cols
    path = torch.empty(B, 3, P, dtype=torch.float64, device=dev)
    plen = torch.empty(B, dtype=torch.int32, device=dev)
    need = int(lib.obca_astar_workspace_bytes(B, rows, cols))
    if need < 0:
        raise ValueError("grid too large for the planner (rows*cols <= 65535)")
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    yaw = (ctypes.c_double * 9)(*yaw_table().tolist())
    ptr = _lib.ptr
    _lib.check(lib.obca_astar_batch(ptr(g), B, rows, cols, ptr(st), ptr(go), yaw, P, ptr(path), ptr(plen), ptr(work),
                                    need, _lib.stream_ptr(dev)))
    # the launch is asynchronous: the tensors it reads, the workspace among them, are tied to the RESULT (see _lib.keep_alive)
    _lib.keep_alive(path, (g, st, go, work), dev)
    return path, plen


def rasterise_batch(obstacle_lists, map_size, resolution=1.0, device=None):
    """Occupancy grids of B worlds in one launch (reference ``mapModel.shape2grid``, src/model_map.py:21-56).
    obstacle_lists: per world a list of polygons (vertex lists, e.g. ``setting.static_gridlObs``); map_size = (x, y) as in
    ``problemSetting`` (src/demo_setting.py:67-68).  Returns a device tensor [B, rows, cols] uint8 = ``org_gridMap``."""
    import torch
    _lib.require_gpu("rasterise_batch")
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    B = len(obstacle_lists)
    K = max(1, max(len(o) for o in obstacle_lists))
    boxes = np.full((B, K, 4), np.nan)
    for b, polys in enumerate(obstacle_lists):
        for k, poly in enumerate(polys):                       # reOrderVertex: the polygon's bounding box
            xs, ys = [float(p[0]) for p in poly], [float(p[1]) for p in poly]
            boxes[b, k] = (min(xs), min(ys), max(xs), max(ys))
    rows = int((map_size[1] - 1) / resolution) + 1
    cols = int((map_size[0] - 1) / resolution) + 1
    bx = torch.as_tensor(boxes, device=dev)
    grid = torch.empty(B, rows, cols, dtype=torch.uint8, device=dev)
    _lib.check(lib.obca_rasterise_batch(_lib.ptr(bx), B, K, float(resolution), rows, cols, _lib.ptr(grid), _lib.stream_ptr(dev)))
    _lib.keep_alive(grid, (bx,), dev)                        # the launch is asynchronous: see plan_batch
    return grid


def dilate_batch(grids, level, device=None):
    """Disk dilation of B occupancy grids in one launch (obca_grid_dilate_batch; reference ``mapModel.dilate_map``,
    src/model_map.py:103-107; host mirror ``model_map.mapModel.dilate_map``).  grids [B,rows,cols] (non-zero = occupied; a
    device tensor, e.g. ``rasterise_batch``'s, stays on the device), 0 <= level <= 16.  Returns a device tensor
    [B,rows,cols] uint8 of 0 / 1, which ``plan_batch`` takes."""
    import torch
    _lib.require_gpu("dilate_batch")
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if isinstance(grids, torch.Tensor):
        g = grids.to(device=dev, dtype=torch.uint8).contiguous()
    else:
        g = torch.as_tensor(np.ascontiguousarray(grids), device=dev).to(torch.uint8).contiguous()
    if g.dim() != 3:
        raise ValueError("expected grids [B,rows,cols], got %s" % (tuple(g.shape),))
    B, rows, cols = g.shape
    out = torch.empty(B, rows, cols, dtype=torch.uint8, device=dev)
    _lib.launch(lib.obca_grid_dilate_batch, _lib.ptr(g), B, rows, cols, int(level), _lib.ptr(out), dev=dev)
    _lib.keep_alive(out, (g,), dev)                          # the launch is asynchronous: see plan_batch
    return out
