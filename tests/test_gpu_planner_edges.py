"""The two kernels of csrc/obca_astar.hip at their edges.  astar_kernel: every launch geometry obca_astar_batch picks (one
lane per block, ragged last blocks at 2, 4 and 64 lanes per block), mixed outcomes inside one wavefront, and grid shapes
from 1 x 1 to the 65535-cell limit -- bit for bit against the host build of the same core (tests/native), which
tests/test_planner_edges_core.py holds to Dijkstra and to the reference's own routes; every route also goes through
planner_ref.check_route here.  rasterise_kernel: boxes across every edge and corner of the map, outside it, of zero width,
with NaN and inverted padding, against planner_ref.rasterise and the host mirror.  The C ABI is called directly so that
every output buffer can sit between guard regions, which have to come back untouched.

Measured on an MI355X (launch + synchronise, first launch of the process included in B = 1): 5 x 7 grids, B = 1: 0.49 ms,
63: 0.17 ms, 1023: 0.22 ms, 2049: 0.23 ms, 4097: 0.24 ms, 65537: 0.53 ms; the mixed wavefront of 13 x 13: 0.85 ms; the batch
of three at 255 x 257 (empty both ways + the 32768-point serpentine): 121 ms, so the serpentine stays at full size.  Whole
file: 3.8 s, of which 1.9 s is the host-side check of the 65537 seeded grids, done once; no test above 0.4 s."""
import ctypes
import time

import numpy as np
import pytest

from tests import native_build, planner_ref
from tests.test_planner_edges_core import MAP_SHAPES, RESOLUTIONS, mirror_grid

pytestmark = pytest.mark.gpu

FILL = -7.25                              # what an unwritten path word holds, on the device and in the host run
GEOMETRY = (1, 63, 1023, 2049, 4097, 65537)
BIG = (255, 257)                          # 65535 cells: the limit of the uint16 queue counters


def device_plan(grids, starts, goals, path_max):
    """obca_astar_batch through the C ABI with path, path_len and the workspace each between two guard regions; asserts the
    guards untouched and returns path [B,3,path_max] (FILL where nothing was written), path_len [B] and the seconds the
    launch took"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.planner import yaw_table
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    if isinstance(grids, torch.Tensor):
        g = grids.to(device=dev, dtype=torch.uint8).contiguous()
    else:
        g = torch.as_tensor(np.ascontiguousarray(grids, np.uint8), device=dev)
    B, rows, cols = g.shape
    st = torch.as_tensor(np.ascontiguousarray(starts, np.int32).reshape(B, 2), device=dev)
    go = torch.as_tensor(np.ascontiguousarray(goals, np.int32).reshape(B, 2), device=dev)
    need = int(lib.obca_astar_workspace_bytes(B, rows, cols))
    assert need == B * native_build.astar_work_bytes(rows, cols)
    gp, gl, gw = 3 * path_max + 64, 256, max(need // B, 4096)         # guard sizes: one instance's worth at least
    path = torch.full((gp + B * 3 * path_max + gp,), FILL, dtype=torch.float64, device=dev)
    plen = torch.full((gl + B + gl,), -77, dtype=torch.int32, device=dev)
    work = torch.full((gw + need + gw,), 0xA5, dtype=torch.uint8, device=dev)
    assert gw % 8 == 0 and work.data_ptr() % 8 == 0
    yaw = (ctypes.c_double * 9)(*yaw_table().tolist())
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off * t.element_size())
    torch.cuda.synchronize()
    t0 = time.time()
    _lib.check(lib.obca_astar_batch(ptr(g), B, rows, cols, ptr(st), ptr(go), yaw, path_max, ptr(path, gp), ptr(plen, gl),
                                    ptr(work, gw), need, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert bool((path[:gp] == FILL).all()) and bool((path[gp + B * 3 * path_max:] == FILL).all()), "path guard written"
    assert bool((plen[:gl] == -77).all()) and bool((plen[gl + B:] == -77).all()), "path_len guard written"
    assert bool((work[:gw] == 0xA5).all()) and bool((work[gw + need:] == 0xA5).all()), "workspace guard written"
    return path[gp:gp + B * 3 * path_max].reshape(B, 3, path_max).cpu().numpy(), plen[gl:gl + B].cpu().numpy(), dt


def assert_equals_host(grids, starts, goals, path_max, path, plen, host=None):
    """device == host core, every word: the lengths, the whole path of every instance with plen >= 0, and FILL where an
    instance returned a negative code (neither side writes then)"""
    hp, hl = native_build.astar_batch(grids, starts, goals, path_max, fill=FILL) if host is None else host
    bad = np.flatnonzero(plen != hl)
    assert bad.size == 0, (bad[:8], plen[bad[:8]], hl[bad[:8]])
    bad = np.flatnonzero((path != hp).any(axis=(1, 2)))
    assert bad.size == 0, (bad[:8], plen[bad[:8]])
    assert (path[plen < 0] == FILL).all()


def check_all(grids, starts, goals, path, plen, lanes=None, costs=None):
    """planner_ref on every lane: a route is valid and shortest, -1 means unreachable, 0 means start == goal"""
    for i in (range(len(plen)) if lanes is None else lanes):
        s, t = tuple(int(v) for v in starts[i]), tuple(int(v) for v in goals[i])
        cost = costs[i] if costs is not None else planner_ref.shortest_cost(grids[i], s, t)
        if s == t:
            assert plen[i] == 0, (i, plen[i])
        elif cost is None:
            assert plen[i] == -1, (i, plen[i])
        else:
            assert plen[i] >= 1, (i, plen[i])
            planner_ref.check_route(grids[i], s, t, path[i], plen[i], cost=cost)


# ---- launch geometry ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def geometry_cases():
    """65537 distinct seeded 5 x 7 grids with a free start and goal each; the smaller batches are prefixes.  The host core's
    answers are computed and checked once: check_route on every lane below 4097 (all lanes of the five smaller batches),
    and beyond on every 61st lane and the last 128, the ragged block of the largest batch."""
    rng = np.random.default_rng(20261017)
    n = max(GEOMETRY)
    g = (rng.uniform(size=(n + n // 8, 35)) < 0.25).astype(np.uint8)
    g = g[(g == 0).sum(axis=1) >= 2]
    _, first = np.unique(g, axis=0, return_index=True)
    g = g[np.sort(first)][:n]
    assert g.shape[0] == n                                       # all distinct
    free = g == 0
    s = np.argmax(rng.uniform(size=g.shape) * free, axis=1)
    t = np.argmax(rng.uniform(size=g.shape) * free, axis=1)
    starts, goals = np.stack([s // 7, s % 7], 1).astype(np.int32), np.stack([t // 7, t % 7], 1).astype(np.int32)
    grids = g.reshape(n, 5, 7)
    host = native_build.astar_batch(grids, starts, goals, 35, fill=FILL)
    lanes = sorted(set(range(4097)) | set(range(4097, n, 61)) | set(range(n - 128, n)))
    check_all(grids, starts, goals, host[0], host[1], lanes=lanes)
    codes = set(np.unique(host[1]).tolist())
    assert {-1, 0, 1, 2, 3} <= codes and min(codes) == -1, codes
    return grids, starts, goals, host


@pytest.mark.parametrize("B", GEOMETRY)
def test_every_launch_geometry(geometry_cases, B):
    """tpb halves until there are 1024 blocks: B = 1, 63 and 1023 run one lane per block, 2049 two (last block ragged), 4097
    four (ragged), 65537 sixty-four (ragged: one live lane, 63 past B).  Lanes past B must write nothing: guards."""
    grids, starts, goals, host = geometry_cases
    path, plen, dt = device_plan(grids[:B], starts[:B], goals[:B], 35)
    print("B = %d: %.2f ms" % (B, dt * 1e3))
    assert_equals_host(grids[:B], starts[:B], goals[:B], 35, path, plen, host=(host[0][:B], host[1][:B]))


# ---- mixed outcomes in one wavefront ---------------------------------------------------------------------------------------

def test_mixed_outcomes_in_one_wavefront():
    """64 lanes of 13 x 13 cycle through -1, 0, 1, -3, -4, a serpentine that fits path_max exactly and an open field: lanes
    that leave at once, lanes that exhaust their component and lanes that walk a maze share a wavefront, and every lane
    carries its own answer"""
    maze, s0, t0 = planner_ref.serpentine(13, 13)
    wall = np.zeros((13, 13), np.uint8)
    wall[:, 6] = 1
    empty = np.zeros((13, 13), np.uint8)
    outside = [((-1, 4), (3, 3)), ((13, 4), (3, 3)), ((4, -1), (3, 3)), ((4, 13), (3, 3)),
               ((3, 3), (-1, 4)), ((3, 3), (13, 4)), ((3, 3), (4, -1)), ((3, 3), (4, 13)), ((-5, -5), (20, 20))]
    grids, starts, goals, want = [], [], [], []
    for lane in range(64):
        kind, k = lane % 7, lane // 7
        if kind == 0:
            grids.append(wall); starts.append((k, 0)); goals.append((12 - k, 12)); want.append(-1)
        elif kind == 1:
            grids.append(empty); starts.append((k, 12 - k)); goals.append((k, 12 - k)); want.append(0)
        elif kind == 2:
            grids.append(empty); starts.append((k + 1, 5)); goals.append((k + (-1, 0, 1)[k % 3] + 1, 6)); want.append(1)
        elif kind == 3:
            grids.append(maze); starts.append(s0); goals.append(t0); want.append(-3)            # 84 points: too long
        elif kind == 4:
            grids.append(empty); starts.append(outside[k][0]); goals.append(outside[k][1]); want.append(-4)
        elif kind == 5:
            grids.append(maze); starts.append((0, 12)); goals.append(t0); want.append(73)       # 84 less row 0's 11 points
        else:
            grids.append(empty); starts.append((0, 0)); goals.append((12, 12)); want.append(12)
    grids = np.stack(grids)
    path, plen, dt = device_plan(grids, starts, goals, 73)                                        # path_max == the longest fit
    print("mixed wavefront: %.2f ms" % (dt * 1e3))
    assert plen.tolist() == want
    assert_equals_host(grids, starts, goals, 73, path, plen)
    check_all(grids, starts, goals, path, plen, lanes=[i for i in range(64) if want[i] > 0])


# ---- extreme shapes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,start,goal", [((1, 300), (0, 0), (0, 299)), ((1, 300), (0, 299), (0, 0)),
                                              ((300, 1), (0, 0), (299, 0)), ((300, 1), (299, 0), (0, 0))])
def test_strips_on_device(shape, start, goal):
    g = np.zeros((1,) + shape, np.uint8)
    for path_max, want in ((300, 299), (299, 299), (298, -3)):
        path, plen, _ = device_plan(g, [start], [goal], path_max)
        assert plen[0] == want
        assert_equals_host(g, [start], [goal], path_max, path, plen)
        if want > 0:
            planner_ref.check_route(g[0], start, goal, path[0], plen[0], cost=299.0)


def test_single_cell_grid_on_device():
    for occupied in (0, 1):
        g = np.full((2, 1, 1), occupied, np.uint8)
        path, plen, _ = device_plan(g, [(0, 0), (0, 0)], [(0, 0), (0, 0)], 2)
        assert plen.tolist() == [0, 0] and not path.any()
        assert_equals_host(g, [(0, 0)] * 2, [(0, 0)] * 2, 2, path, plen)


def test_the_cell_limit():
    """255 x 257 = 65535 cells, the most the uint16 queue counters allow: an empty field corner to corner both ways and the
    serpentine (32768 points, every free cell expanded) in one batch of three; one cell more is refused"""
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib
    lib = _lib.load()
    assert lib.obca_astar_workspace_bytes(1, 256, 256) == -1 and lib.obca_astar_workspace_bytes(3, *BIG) > 0
    rows, cols = BIG
    maze, s, t = planner_ref.serpentine(rows, cols)
    grids = np.stack([np.zeros(BIG, np.uint8), np.zeros(BIG, np.uint8), maze])
    starts, goals = [(0, 0), (rows - 1, cols - 1), s], [(rows - 1, cols - 1), (0, 0), t]
    P = (rows + 1) // 2 * (cols - 1)                              # the serpentine's length: path_max == len
    path, plen, dt = device_plan(grids, starts, goals, P)
    print("%d x %d, empty both ways + serpentine: %.1f ms" % (rows, cols, dt * 1e3))
    assert plen.tolist() == [cols - 1, cols - 1, P]
    assert_equals_host(grids, starts, goals, P, path, plen)
    diag = (rows - 1) * planner_ref.SQRT2 + (cols - rows)         # rows - 1 diagonal steps, the rest straight
    check_all(grids, starts, goals, path, plen, costs=[diag, diag, planner_ref.shortest_cost(maze, s, t)])


# ---- rasteriser ----------------------------------------------------------------------------------------------------------

def device_rasterise(boxes, res, rows, cols):
    """obca_rasterise_batch through the C ABI, the grid between two guard regions; returns the DEVICE tensor [B,rows,cols]"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    B, K = boxes.shape[:2]
    bx = torch.as_tensor(np.ascontiguousarray(boxes, float), device=dev)
    n, guard = B * rows * cols, 1024
    buf = torch.full((guard + n + guard,), 0x5A, dtype=torch.uint8, device=dev)
    _lib.check(lib.obca_rasterise_batch(ctypes.c_void_p(bx.data_ptr()), B, K, float(res), rows, cols,
                                        ctypes.c_void_p(buf.data_ptr() + guard),
                                        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize()
    assert bool((buf[:guard] == 0x5A).all()) and bool((buf[guard + n:] == 0x5A).all()), "grid guard written"
    return buf[guard:guard + n].reshape(B, rows, cols)


def padded_worlds(rows, cols, res, n_worlds=19):
    """n_worlds obstacle lists of ragged length drawn from planner_ref.edge_boxes, as rows of a [n_worlds, K, 4] array:
    the entries a world does not use are padding -- NaN rows and inverted boxes, some of them BETWEEN real boxes.  Returns
    the array and, per world, the list of its real boxes."""
    named = planner_ref.edge_boxes(rows, cols, res)
    names = [n for n in named if n not in ("whole_map", "exact_map")]
    nan = float("nan")
    pads = [(nan, nan, nan, nan), (3.0 * res, 0.0, 1.0 * res, 2.0 * res), (0.0, nan, res, res), (0.0, 3.0 * res, res, res),
            (res, res, nan, 2 * res), (2 * res, 2 * res, res, res)]
    real = []
    for w in range(n_worlds):
        if w == 0:
            real.append([])                                       # a world of padding alone
        elif w == 1:
            real.append([named["whole_map"]])
        elif w == 2:
            real.append([named[n] for n in names])                # every edge box at once: K
        else:
            real.append([named[names[(w * 5 + j * 3) % len(names)]] for j in range(1 + w % 6)])
    K = max(len(r) for r in real) + 1
    boxes = np.zeros((n_worlds, K, 4))
    for w, r in enumerate(real):
        slots = [None] * K
        at = [(w + 2 * j) % K for j in range(len(r))] if 2 * len(r) <= K else list(range(len(r)))
        for j, q in zip(at, r):
            slots[j] = q
        boxes[w] = [q if q is not None else pads[(w + j) % len(pads)] for j, q in enumerate(slots)]
    return boxes, real


@pytest.mark.parametrize("rows,cols", MAP_SHAPES)
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_rasteriser_clips_and_skips_padding(res, rows, cols):
    """B = 1, 3 and 257 worlds (B * cells is a multiple of 256 only at 16 x 16): bit-equal to planner_ref.rasterise on the
    padded rows and to the host mirror on the real boxes; the device grid then goes to the planner as it is"""
    import torch
    from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.planner import plan_batch
    boxes, real = padded_worlds(rows, cols, res)
    want = np.stack([planner_ref.rasterise(b, res, rows, cols) for b in boxes])
    for w, r in enumerate(real):
        assert np.array_equal(mirror_grid(r, res, rows, cols), want[w]), w
    assert not want[0].any() and want[1].all()
    for B in (1, 3, 257):
        world = (np.arange(B) + (2 if B == 1 else 0)) % len(boxes)
        grid = device_rasterise(boxes[world], res, rows, cols)
        got = grid.cpu().numpy()
        bad = np.flatnonzero((got != want[world]).any(axis=(1, 2)))
        assert bad.size == 0, (B, bad[:8])
    starts, goals = [(0, 0)] * B, [(rows - 1, cols - 1)] * B
    path, plen = plan_batch(grid, starts, goals)                  # device grid -> device planner, no host copy
    torch.cuda.synchronize()
    path, plen = path.cpu().numpy(), plen.cpu().numpy()
    hp, hl = native_build.astar_batch(want[world], starts, goals, rows * cols)
    assert np.array_equal(plen, hl)
    assert np.array_equal(path[plen >= 0], hp[plen >= 0])
    first = [int(np.flatnonzero(world == w)[0]) for w in range(len(boxes))]
    check_all(want[world], starts, goals, path, plen, lanes=first)
