"""CPU tier of the grid-to-pool cover (csrc/obca_gridpool_core.h: obca_grid_pool's serial definition, the rows of a rectangle,
the spare slots, the argument check), built for the host from tests/native/grid_pool_host.cpp.

Yardsticks: the cover against ``numpy_cover``, a restatement of the serial definition on a boolean array written here,
exactly; the invariants (disjoint, union = occupied set, ascending seeds) directly on the rectangles; the rows against
``obstacleModel.obstacle_H_Represent`` on the clockwise polygon of the padded box and against numpy with the same operations
in the same order, word for word; the reference's demo maps against a numpy restatement of ``shape2grid``.  Then the spare
slots, the overflow flag and every refused call with guard-banded outputs.  The helpers are shared with
tests/test_gpu_grid_pool.py."""
import ctypes
import os

import numpy as np
import pytest

from tests import native_build
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import demo_setting
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.model_obstacle import obstacleModel

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "grid_pool_host.cpp")
E_INVAL = -22
GUARD = 8
FILL_X, FILL_I = -777.25, -777
# (rows, cols): the GPU list -- one cell; one word short by a column, exactly one word, one column into the second word; two
# words exactly and one column more; one chunk of 64 rows exactly and one row more; three chunks and two words; the demo size
GPU_SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 128), (3, 129), (64, 5), (65, 5), (130, 70), (11, 40)]
SHAPES = [(1, 7), (9, 1)] + GPU_SHAPES


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def load_host():
    lib = native_build.build_shim("grid_pool_host", [SRC])
    lib.grid_pool_host.restype = ctypes.c_int
    lib.grid_pool_host.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_double] * 3 + [ctypes.c_void_p] * 5
    return lib


@pytest.fixture(scope="module")
def host():
    return load_host()


def words(a):
    return np.ascontiguousarray(a, float).view(np.uint64)


def banded(shape, dtype, fill):
    """(whole, view): GUARD + prod(shape) + GUARD elements of ``fill`` and the middle as ``shape`` (float64 views are 16-byte
    aligned: GUARD is even and numpy aligns to 16)"""
    n = int(np.prod(shape))
    whole = np.full(n + 2 * GUARD, fill, dtype)
    return whole, whole[GUARD:GUARD + n].reshape(shape)


def out_shapes(B, K):
    K = max(int(K), 1)
    return {"pool_A": ((B, K, 4, 2), np.float64, FILL_X), "pool_b": ((B, K, 4), np.float64, FILL_X),
            "rect": ((B, K, 4), np.int32, FILL_I), "count": ((B,), np.int32, FILL_I), "ok": ((B,), np.int32, FILL_I)}


def host_pool(host, grids, K, res=1.0, pad=0.5, far=100.0, rc=0, null=(), over=None):
    """grid_pool_host on numpy arrays: a dict of the outputs (views into guard-banded buffers pre-filled with FILL_X / FILL_I;
    ``_whole`` holds the buffers).  ``null``: names of pointers handed over as NULL; ``over``: scalar arguments the call is told
    instead of the arrays' own (B, rows, cols, K)"""
    g = np.ascontiguousarray(grids, np.uint8)
    B, rows, cols = g.shape
    o, whole = {}, {}
    for k, (shape, dt, fill) in out_shapes(B, K).items():
        whole[k], o[k] = banded(shape, dt, fill)
    a = dict(o, grid=g)
    for k in null:
        a[k] = None
    s = dict(B=B, rows=rows, cols=cols, K=K)
    s.update(over or {})
    got = host.grid_pool_host(_p(a["grid"]), s["B"], s["rows"], s["cols"], s["K"], res, pad, far, _p(a["pool_A"]), _p(a["pool_b"]),
                              _p(a["rect"]), _p(a["count"]), _p(a["ok"]))
    assert got == rc
    o["_whole"] = whole
    return o


def bands_clean(o, B, K):
    return all(np.all(o["_whole"][k][:GUARD] == fill) and np.all(o["_whole"][k][-GUARD:] == fill)
               for k, (_, _, fill) in out_shapes(B, K).items())


# ------------------------------------------------------------------------------------------------ the yardstick
def numpy_cover(grid):
    """the serial definition on a boolean array: every rectangle (r0, c0, r1, c1), however many"""
    work = np.asarray(grid) != 0
    rows, cols = work.shape
    rects = []
    for r, c in zip(*np.nonzero(work)):                          # row-major; a cell removed meanwhile is skipped
        if not work[r, c]:
            continue
        c1, r1 = c, r
        while c1 + 1 < cols and work[r, c1 + 1]:
            c1 += 1
        while r1 + 1 < rows and work[r1 + 1, c:c1 + 1].all():
            r1 += 1
        work[r:r1 + 1, c:c1 + 1] = False
        rects.append((int(r), int(c), int(r1), int(c1)))
    return rects


def box_rows(xlo, xhi, ylo, yhi):
    return np.array([[0.0, 1.0], [1.0, 0.0], [0.0, -1.0], [-1.0, 0.0]]), np.array([yhi, xhi, -ylo, -xlo])


def expected(grids, K, res=1.0, pad=0.5, far=100.0):
    """what obca_grid_pool must write, from ``numpy_cover``: numpy rounds every product and difference on its own"""
    B = len(grids)
    res, pad, far = np.float64(res), np.float64(pad), np.float64(far)
    o = {"pool_A": np.zeros((B, K, 4, 2)), "pool_b": np.zeros((B, K, 4)), "rect": np.full((B, K, 4), -1, np.int32),
         "count": np.zeros(B, np.int32), "ok": np.zeros(B, np.int32)}
    for i, g in enumerate(grids):
        rects = numpy_cover(g)
        o["count"][i], o["ok"][i] = len(rects), int(len(rects) <= K)
        for k in range(K):
            if k < len(rects):
                r0, c0, r1, c1 = rects[k]
                o["rect"][i, k] = rects[k]
                box = (np.float64(c0) * res - pad, np.float64(c1) * res + pad, np.float64(r0) * res - pad, np.float64(r1) * res + pad)
            else:
                box = (-far - 1.0, -far, -far - 1.0, -far)
            o["pool_A"][i, k], o["pool_b"][i, k] = box_rows(*box)
    return o


def assert_equal(got, ref):
    for k in ("rect", "count", "ok"):
        assert np.array_equal(got[k], ref[k]), k
    for k in ("pool_A", "pool_b"):
        assert np.array_equal(words(got[k] + 0.0), words(ref[k] + 0.0)), k      # + 0.0: -0.0 (b = -xlo at column 0, pad 0) is 0.0


# ------------------------------------------------------------------------------------------------ maps
def patterns(rows, cols, seed=0):
    """name -> grid [rows,cols] uint8; every pattern is clipped to the grid, so small shapes see what fits of it"""
    z = lambda: np.zeros((rows, cols), np.uint8)
    rr, cc = np.mgrid[0:rows, 0:cols]
    p = {"empty": z(), "full": z() + 1, "checkerboard": ((rr + cc) % 2).astype(np.uint8)}
    p["staircase"] = (cc < np.maximum(1, (rr + 1) * cols // rows)).astype(np.uint8)      # rows grow to the right going down
    p["staircase_up"] = p["staircase"][::-1].copy()                                      # long run first, extension stops
    g = z(); g[:, 0] = 1; g[-1, :] = 1; p["L"] = g
    g = z(); g[0, :] = 1; g[:, cols // 2] = 7; p["T"] = g                                 # bytes other than 0 / 1 as well
    # the column is seeded first and takes the bar's middle cell with it: the bar's run is split in two
    g = z(); g[:rows // 2 + 1, cols // 2] = 1; g[rows // 2, :] = 255; p["T_split"] = g
    g = z(); g[rows // 2, 60:71] = 1; p["run_60_70"] = g                                  # across the 63|64 boundary
    g = z(); r0 = max(0, min(5, rows - 101)); g[r0:r0 + 100, cols // 3:cols // 3 + 3] = 1; p["tall_100"] = g
    g = z(); g[0, max(0, cols - 20):] = 1; g[-1, -1] = 1; p["to_last_column"] = g         # ends with the word at 64 / 128 columns
    rng = np.random.default_rng(1000 * rows + cols + seed)
    for d in (0.1, 0.5, 0.9):
        p["random_%.1f" % d] = (rng.random((rows, cols)) < d).astype(np.uint8)
    return p


# ------------------------------------------------------------------------------------------------ cover
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_cover_matches_the_serial_definition(host, shape):
    """every pattern of a shape as one batch, K = 64 and K = 3 (overflow on most), against ``numpy_cover``; then the invariants
    on the host's own rectangles where the map is covered"""
    rows, cols = shape
    pats = patterns(rows, cols)
    grids = np.stack(list(pats.values()))
    for K in (64, 3):
        o = host_pool(host, grids, K)
        assert_equal(o, expected(grids, K))
        assert bands_clean(o, len(grids), K)
    o = host_pool(host, grids, 64)
    for i, name in enumerate(pats):
        n = int(o["count"][i])
        rect = o["rect"][i, :min(n, 64)]
        paint = np.zeros((rows, cols), int)
        for r0, c0, r1, c1 in rect:
            assert 0 <= r0 <= r1 < rows and 0 <= c0 <= c1 < cols, name
            paint[r0:r1 + 1, c0:c1 + 1] += 1
        assert paint.max(initial=0) <= 1, name                   # disjoint
        assert np.all((grids[i] != 0)[paint == 1]), name         # inside the occupied set
        if o["ok"][i]:
            assert np.array_equal(paint == 1, grids[i] != 0), name                           # union = occupied set
        seeds = [(int(q[0]), int(q[1])) for q in rect]
        assert seeds == sorted(set(seeds)), name                 # strictly ascending (r0, c0)
        assert np.all(o["rect"][i, n:] == -1)


def test_named_covers(host):
    """the T splits a later run, the staircase ends a downward extension early, a full map is one rectangle"""
    g = np.zeros((3, 5, 5), np.uint8)
    g[0, :3, 2] = 1; g[0, 2, :] = 1                              # column seeded first, then the bar in two pieces
    g[1] = patterns(5, 5)["staircase"]
    g[2] = 1
    o = host_pool(host, g, 8)
    assert o["count"].tolist() == [3, 5, 1] and o["ok"].tolist() == [1, 1, 1]
    assert o["rect"][0, :3].tolist() == [[0, 2, 2, 2], [2, 0, 2, 1], [2, 3, 2, 4]]
    assert o["rect"][1, :5].tolist() == [[0, 0, 4, 0], [1, 1, 4, 1], [2, 2, 4, 2], [3, 3, 4, 3], [4, 4, 4, 4]]
    assert o["rect"][2, 0].tolist() == [0, 0, 4, 4]


def test_the_largest_grids_are_taken(host):
    """rows * ceil(cols / 64) = 4096 exactly (1024 x 256) and 255 x 255: a few boxes, against the serial definition"""
    for rows, cols in ((1024, 256), (255, 255)):
        g = np.zeros((1, rows, cols), np.uint8)
        g[0, 0, :] = 1; g[0, -1, :] = 1; g[0, 100:230, 60:200] = 1; g[0, 150:160, 0:70] = 1; g[0, -3:, -1] = 1
        o = host_pool(host, g, 16, res=0.25, pad=0.125)
        assert_equal(o, expected(g, 16, res=0.25, pad=0.125))
        assert o["ok"][0] == 1 and bands_clean(o, 1, 16)


# ------------------------------------------------------------------------------------------------ rows
def h_rows(xlo, xhi, ylo, yhi):
    poly = [[xlo, yhi], [xhi, yhi], [xhi, ylo], [xlo, ylo], [xlo, yhi]]
    A, b = obstacleModel().obstacle_H_Represent(1, [5], [poly])
    return A, b[:, 0]


@pytest.mark.parametrize("pad", [0.0, 0.5])
def test_rows_are_obstacle_h_represent(host, pad):
    """every rectangle of the 11 x 40 patterns with area: pad = 0.5 all of them, pad = 0 those of more than one row and column"""
    pats = patterns(11, 40)
    grids = np.stack(list(pats.values()))
    o = host_pool(host, grids, 64, pad=pad)
    seen = 0
    for i in range(len(grids)):
        for k in range(min(int(o["count"][i]), 64)):
            r0, c0, r1, c1 = (int(v) for v in o["rect"][i, k])
            if pad == 0.0 and (r0 == r1 or c0 == c1):
                continue
            A, b = h_rows(c0 - pad, c1 + pad, r0 - pad, r1 + pad)
            assert np.array_equal(o["pool_A"][i, k], A) and np.array_equal(o["pool_b"][i, k], b)
            seen += 1
    assert seen > 20                                             # the patterns do hold rectangles with area


def test_rows_round_every_operation_on_its_own(host):
    """resolution 0.3 and pad 0.1: c res - pad fused is another word than the product rounded first for most c"""
    grids = np.stack(list(patterns(11, 40).values()))
    o = host_pool(host, grids, 64, res=0.3, pad=0.1, far=1000.0)
    assert_equal(o, expected(grids, 64, res=0.3, pad=0.1, far=1000.0))


# ------------------------------------------------------------------------------------------------ the reference's worlds
def numpy_shape2grid(rows, cols, boxes):
    """mapModel.shape2grid at resolution 1 restated: boxes (xlo, xhi, ylo, yhi)"""
    g = np.zeros((rows, cols), np.uint8)
    for xlo, xhi, ylo, yhi in boxes:
        x0, y0 = int(xlo), int(ylo)
        g[y0:y0 + int(yhi - ylo) + 1, x0:x0 + int(xhi - xlo) + 1] = 1
    return g


def _axis_parallel(polys):
    return all(p[j][0] == p[(j + 1) % len(p)][0] or p[j][1] == p[(j + 1) % len(p)][1] for p in polys for j in range(len(p)))


def test_reference_worlds_round_trip(host):
    """every demo whose grid polygons are axis-parallel: the pad = 0 boxes of the cover of org_gridMap rasterise back to it"""
    done = 0
    for name in sorted(demo_setting._DEMOS):
        s = demo_setting.problemSetting(name)
        if not _axis_parallel(s.static_gridlObs):
            continue
        grid = np.asarray(s.org_gridMap).astype(np.uint8)
        o = host_pool(host, grid[None], 64, pad=0.0)
        n = int(o["count"][0])
        assert o["ok"][0] == 1 and n >= 2, name
        b = o["pool_b"][0, :n]
        back = numpy_shape2grid(grid.shape[0], grid.shape[1], [(-q[3], q[1], -q[2], q[0]) for q in b])
        assert np.array_equal(back, grid), name
        if name == "demo1":
            assert grid.shape == (11, 40)
            assert o["rect"][0, :n].tolist() == [[0, 0, 1, 39], [2, 10, 5, 15], [9, 0, 10, 39]]
        done += 1
    assert done >= 11


# ------------------------------------------------------------------------------------------------ spare slots, overflow
def test_spare_slots_and_overflow(host):
    """K isolated cells fill a pool of K (ok 1); one more overflows it: ok 0, the true count, the first K rectangles valid"""
    K, far = 5, 250.0
    g = np.zeros((3, 4, 9), np.uint8)
    g[0, 1, [1, 3]] = 1                                          # 2 of 5: three spare slots
    g[1, 1, [0, 2, 4, 6, 8]] = 1                                 # 5 of 5
    g[2, 1, [0, 2, 4, 6, 8]] = 1; g[2, 3, 4] = 1                 # 6 of 5
    o = host_pool(host, g, K, far=far)
    assert_equal(o, expected(g, K, far=far))
    assert o["count"].tolist() == [2, 5, 6] and o["ok"].tolist() == [1, 1, 0]
    A, b = h_rows(-far - 1.0, -far, -far - 1.0, -far)
    for k in (2, 3, 4):
        assert o["rect"][0, k].tolist() == [-1] * 4
        assert np.array_equal(o["pool_A"][0, k], A) and np.array_equal(o["pool_b"][0, k], b)
    assert np.all(o["rect"][1:] >= 0) and o["rect"][2, 4].tolist() == [1, 8, 1, 8]
    assert not np.isnan(o["pool_A"]).any() and not np.isnan(o["pool_b"]).any()
    # rect may be NULL: everything else as before
    o2 = host_pool(host, g, K, far=far, null=("rect",))
    for k in ("pool_A", "pool_b", "count", "ok"):
        assert np.array_equal(o2[k], o[k])
    assert np.all(o2["_whole"]["rect"] == FILL_I)


# ------------------------------------------------------------------------------------------------ refusals
REFUSED = [dict(over=dict(B=0)), dict(over=dict(K=0)), dict(over=dict(K=65)), dict(over=dict(rows=0)), dict(over=dict(cols=0)),
           dict(over=dict(rows=-1)), dict(over=dict(rows=4097, cols=1)), dict(over=dict(rows=2049, cols=65)),
           dict(over=dict(rows=1, cols=4096 * 64 + 1)), dict(over=dict(rows=2 ** 31 - 1, cols=2 ** 31 - 1)),
           dict(res=0.0), dict(res=-1.0), dict(res=np.nan), dict(res=np.inf), dict(pad=-0.5), dict(pad=np.nan), dict(pad=np.inf),
           dict(far=0.0), dict(far=-100.0), dict(far=np.nan), dict(far=np.inf)] + \
          [dict(null=(k,)) for k in ("grid", "pool_A", "pool_b", "count", "ok")]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: repr(c).replace(" ", ""))
def test_refused_calls_touch_nothing(host, case):
    g = patterns(4, 9)["checkerboard"][None].repeat(2, 0)
    o = host_pool(host, g, 6, rc=E_INVAL, **case)
    for k, (_, _, fill) in out_shapes(2, 6).items():
        assert np.all(o["_whole"][k] == fill), k


def test_misaligned_rows_are_refused(host):
    """pool_A takes one 16-byte store per row"""
    g = patterns(4, 9)["checkerboard"][None]
    shapes = out_shapes(1, 6)
    bufs = {k: np.full(int(np.prod(s)) + 3, fill, dt) for k, (s, dt, fill) in shapes.items()}
    A_odd = bufs["pool_A"][(1 if bufs["pool_A"].ctypes.data % 16 == 0 else 0):]
    assert A_odd.ctypes.data % 16 == 8
    rc = host.grid_pool_host(_p(g), 1, 4, 9, 6, 1.0, 0.5, 100.0, _p(A_odd), _p(bufs["pool_b"]), _p(bufs["rect"]), _p(bufs["count"]),
                             _p(bufs["ok"]))
    assert rc == E_INVAL
    for k, (_, _, fill) in shapes.items():
        assert np.all(bufs[k] == fill)
