"""GPU tier of the opt-in swept, inflated rows of moving boxes: obca_moving_rows_batch equals the host shim word for word at
the edges of its lane layout; the closed loop with swept rows (obca_rollouts_set_swept_rows through DeviceRollouts) gives
the same words in lock step and in the persistent kernel (every queue mode), agrees with the host core, and keeps the
clearance between knots that csrc/obca_rollout_core.h derives; off -- never set, or set to (0, 0) -- it is today's
exact-sensing run; refused calls change nothing."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.test_rollout_stop_core import q8_case
from tests.test_rollout_swept_core import check_guarantee, host, host_rows, random_boxes, run as host_run  # noqa: F401 (host: fixture)
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd import _lib
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.rollouts import DeviceRollouts, pack_worlds
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.scenarios import make_world_c5
from vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd.solver import moving_rows

pytestmark = pytest.mark.gpu
E_INVAL = -22
H, R, N_SUB = 0.5, 0.5, 16
SWEPT = dict(collision_stop=N_SUB, exact_sensing=True, swept_rows={"half_window": H, "margin": R})


def _np(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _run(w, mode="fused", **kw):
    dr = DeviceRollouts(w, N=5, **kw)
    if mode == "lockstep":
        dr.set_mode("lockstep")
        for _ in range(dr.max_steps):
            dr.step()
    else:
        dr.run()
    return dr, _np(dr.read())


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# -------------------------------------------------------------------------------------------------------------- builder
# (B, N, n_box, Ms): B (N + 1) n_box = 1 x 6 x 2, then 63, 64, 65 and 4097 lanes; no box; no static row; static lanes > box lanes
SHAPES = [(1, 5, 2, 6), (3, 6, 3, 6), (4, 7, 2, 5), (13, 4, 1, 6), (241, 16, 1, 3), (5, 5, 0, 6), (7, 5, 2, 0), (9, 5, 1, 31)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("hr", [(0.0, 0.0), (H, R), (1.0, 0.0), (0.0, 2.0)])
def test_builder_equals_the_host_shim(host, shape, hr):
    B, n, nb, Ms = shape
    rng = np.random.default_rng(B * 1000 + n * 10 + nb)
    boxes = np.stack([random_boxes("axis" if i % 2 else "oblique", nb, rng) for i in range(B)]).reshape(B, nb, 13)
    sA, sb, Ts = rng.normal(size=(B, Ms, 2)), rng.normal(size=(B, Ms)), rng.uniform(0.05, 1.0, B)
    A, b = moving_rows(sA, sb, boxes, Ts, n, *hr)
    eA, eb = host_rows(host, sA, sb, boxes, Ts, n, *hr)
    torch.cuda.synchronize()
    assert A.shape == eA.shape and b.shape == eb.shape
    assert np.array_equal(A.cpu().numpy(), eA) and np.array_equal(b.cpu().numpy(), eb)


def test_builder_writes_nothing_beyond_its_outputs_and_refuses_bad_arguments():
    lib = _lib.load()
    B, n, nb, Ms = 13, 4, 1, 3
    M = Ms + 4 * nb
    rng = np.random.default_rng(5)
    dev = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda").contiguous()
    boxes, sA, sb, Ts = dev(random_boxes("oblique", B * nb, rng).reshape(B, nb, 13)), dev(rng.normal(size=(B, Ms, 2))), \
        dev(rng.normal(size=(B, Ms))), dev(rng.uniform(0.1, 1.0, B))
    nA, nb_ = B * (n + 1) * M * 2, B * (n + 1) * M
    A, b = torch.full((nA + 64,), -7.0, dtype=torch.float64, device="cuda"), torch.full((nb_ + 64,), -7.0, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda *a: lib.obca_moving_rows_batch(*a, 0, stream)
    bad = [(0, n, Ms, nb, p(sA), p(sb), p(boxes), p(Ts), H, R, p(A), p(b)), (B, 0, Ms, nb, p(sA), p(sb), p(boxes), p(Ts), H, R, p(A), p(b)),
           (B, n, -1, nb, p(sA), p(sb), p(boxes), p(Ts), H, R, p(A), p(b)), (B, n, 33, nb, p(sA), p(sb), p(boxes), p(Ts), H, R, p(A), p(b)),
           (B, n, Ms, 9, p(sA), p(sb), p(boxes), p(Ts), H, R, p(A), p(b)), (B, n, 0, 0, None, None, None, None, H, R, p(A), p(b)),
           (B, n, Ms, nb, None, p(sb), p(boxes), p(Ts), H, R, p(A), p(b)), (B, n, Ms, nb, p(sA), p(sb), None, p(Ts), H, R, p(A), p(b)),
           (B, n, Ms, nb, p(sA), p(sb), p(boxes), None, H, R, p(A), p(b)), (B, n, Ms, nb, p(sA), p(sb), p(boxes), p(Ts), H, R, None, p(b)),
           (B, n, Ms, nb, p(sA), p(sb), p(boxes), p(Ts), math.nan, R, p(A), p(b)), (B, n, Ms, nb, p(sA), p(sb), p(boxes), p(Ts), -0.1, R, p(A), p(b)),
           (B, n, Ms, nb, p(sA), p(sb), p(boxes), p(Ts), 1.5, R, p(A), p(b)), (B, n, Ms, nb, p(sA), p(sb), p(boxes), p(Ts), H, 2.5, p(A), p(b)),
           (B, n, Ms, nb, p(sA), p(sb), p(boxes), p(Ts), H, math.inf, p(A), p(b)),
           (B, n, Ms, nb, p(sA), p(sb), p(boxes), p(Ts), H, R, ctypes.c_void_p(A.data_ptr() + 8), p(b))]
    for a in bad:
        assert call(*a) == E_INVAL, a[:4] + a[8:10]
    torch.cuda.synchronize()
    assert (A == -7.0).all() and (b == -7.0).all()                              # refused: no side effect
    assert call(B, n, Ms, nb, p(sA), p(sb), p(boxes), p(Ts), H, R, p(A), p(b)) == 0
    torch.cuda.synchronize()
    eA, eb = moving_rows(sA, sb, boxes, Ts, n, H, R)
    assert torch.equal(A[:nA], eA.reshape(-1)) and torch.equal(b[:nb_], eb.reshape(-1))
    assert (A[nA:] == -7.0).all() and (b[nb_:] == -7.0).all()


@pytest.mark.parametrize("hr", [(H, R), (1.0, 0.25), (0.0, 0.0)])
def test_debug_harness_shows_the_builder_rows(hr):
    """a fixed-time step with one sensed box: the rows the harness hands the solver are the builder's for that box"""
    w, x0, Ts, info, V = q8_case()
    kw = dict(swept_rows={"half_window": hr[0], "margin": hr[1]}) if hr != (0.0, 0.0) else {}
    dr = DeviceRollouts(w, N=5, exact_sensing=True, **kw)
    var, A, b = dr.debug_harness(1, Ts, x0, g=1)
    assert var[0] == 6
    eA, eb = moving_rows(w.static_A[:1], w.static_b[:1], np.asarray(info[1])[None, None, :], [Ts], 5, *hr)
    torch.cuda.synchronize()
    assert np.array_equal(A, eA.cpu().numpy()) and np.array_equal(b, eb.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------- closed loop
@pytest.fixture(scope="module")
def c5():
    return pack_worlds([make_world_c5(i, n_dyn=2) for i in range(256)])


@pytest.fixture(scope="module")
def swept_lockstep(c5):
    return _run(c5, "lockstep", **SWEPT)[1]


def test_lockstep_and_every_queue_mode_give_the_same_words(c5, swept_lockstep, monkeypatch):
    assert "clearance" in swept_lockstep and (swept_lockstep["variant"] >= 6).any()
    for env in ("2", "1", "0"):
        monkeypatch.setenv("OBCA_ROLLOUT_QUEUE", env)
        dr, got = _run(c5, "fused", **SWEPT)
        assert dr.queue_mode() == int(env)
        _same(swept_lockstep, got)


def test_swept_run_differs_from_the_plain_one(c5, swept_lockstep):
    _, plain = _run(c5, "fused", collision_stop=N_SUB, exact_sensing=True)
    assert not np.array_equal(plain["x_closed"], swept_lockstep["x_closed"])


def test_gpu_agrees_with_the_host_core(host, c5, swept_lockstep):
    """first 8 worlds against the host core.  The harness words (what is present, what is sensed, which variant, how a
    rollout ends) are equal; the solves run through different kernels on the two sides (wavefront reductions on the device,
    serial sums on the host), so their outputs agree to the 1e-6 every device-against-host-core test of this suite uses
    (tests/test_gpu_rollouts.py), not word for word: measured 4.8e-10 on x_openloop, 2.2e-10 on x_closed, 4.3e-10 on the
    clearance, iteration counts up to 3 apart."""
    w = c5.slice(0, 8)
    rc, ref = host_run(host, w, H, R, stop_nsub=N_SUB)
    assert rc == 0
    got = {k: v[:8] for k, v in swept_lockstep.items()}
    print("max |GPU - host|:", {k: float(np.nanmax(np.abs(np.where(np.isfinite(ref[k]), got[k] - ref[k], 0.0)))) for k in ref})
    for k in ("steps", "flags", "variant", "status"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["dyn"][..., 2:], ref["dyn"][..., 2:])            # present / sensed
    for k in ("x_closed", "u_closed", "T_closed", "x_openloop", "dyn"):
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-6, err_msg=k)
    fin = np.isfinite(ref["clearance"])
    assert np.array_equal(fin, np.isfinite(got["clearance"]))
    np.testing.assert_allclose(got["clearance"][fin], ref["clearance"][fin], rtol=0, atol=1e-6)


def test_clearance_between_knots_on_the_device(c5, swept_lockstep):
    pairs, worst = check_guarantee(swept_lockstep, c5, H, R, n_sub=N_SUB)
    print("rollouts with a pair", int((pairs > 0).sum()), "pairs", int(pairs.sum()), "smallest distance - bound", worst)
    assert (pairs > 0).sum() * 2 >= c5.batch


@pytest.mark.parametrize("mode", ["fused", "lockstep"])
def test_never_set_and_set_to_zero_are_todays_exact_sensing_run(c5, mode):
    w = c5.slice(0, 128)
    _, ref = _run(w, mode, collision_stop=N_SUB, exact_sensing=True)
    _, none = _run(w, mode, collision_stop=N_SUB, exact_sensing=True, swept_rows=None)
    _, zero = _run(w, mode, collision_stop=N_SUB, exact_sensing=True, swept_rows={"half_window": 0.0, "margin": 0.0})
    dr = DeviceRollouts(w, N=5, collision_stop=N_SUB, exact_sensing=True)
    assert dr.lib.obca_rollouts_set_swept_rows(dr._h, 0.0, 0.0) == 0               # the ABI call itself, with (0, 0)
    dr.reset()
    if mode == "lockstep":
        dr.set_mode("lockstep")
        for _ in range(dr.max_steps):
            dr.step()
    else:
        dr.run()
    for got in (none, zero, _np(dr.read())):
        _same(ref, got)


def test_refused_calls_leave_a_following_run_unchanged(c5):
    w = c5.slice(0, 128)
    dr, ref = _run(w, **SWEPT)
    lib, h = dr.lib, dr._h
    for hw, mg in ((math.nan, R), (H, math.nan), (-0.1, R), (H, -0.1), (1.5, R), (H, 2.5), (math.inf, R), (H, math.inf)):
        assert lib.obca_rollouts_set_swept_rows(h, hw, mg) == E_INVAL, (hw, mg)
    assert lib.obca_rollouts_set_swept_rows(None, H, R) == E_INVAL
    dr.reset()
    dr.run()
    _same(ref, _np(dr.read()))
    # swept rows on, exact sensing off: the reset refuses before it touches anything ...
    assert lib.obca_rollouts_set_exact_sensing(h, 0) == 0
    ptrs = [ctypes.c_void_p(x.data_ptr()) for x in dr._inputs]
    assert lib.obca_rollouts_reset(h, *ptrs, dr.Ts0, w.sense_dis, ctypes.byref(dr._cparams), dr._stream()) == E_INVAL
    # ... and with exact sensing back on the same handle runs the same words
    assert lib.obca_rollouts_set_exact_sensing(h, 1) == 0
    dr.reset()
    dr.run()
    _same(ref, _np(dr.read()))
